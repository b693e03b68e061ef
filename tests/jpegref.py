"""numpy restatement of the baseline JPEG the library writes (quality 100, 4:4:4, Annex K tables, restart intervals): libjpeg's
jccolor, edge replication, jfdctint, divisor 8, jchuff's entropy coding.  The Huffman tables are read from the library's own header
(sarpro_amd.host_jpeg_header), so the restatement codes with what the file declares.  test_jpeg_host.py holds it against Pillow
(libjpeg-turbo) byte for byte; the stage functions (ycc, coefficients, split_segments) localise a failing GPU comparison."""
import functools

import numpy as np

import sarpro_amd

C = [2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172]
(F0_298, F0_390, F0_541, F0_765, F0_899, F1_175, F1_501, F1_847, F1_961, F2_053, F2_562, F3_072) = C


def fix(x):
    return int(x * 65536 + 0.5)


def zigzag_order():
    """natural index (row * 8 + col) of the k-th coefficient in zigzag order"""
    out = []
    for s in range(15):
        for i in range(s + 1):
            r = i if s & 1 else s - i
            c = s - r
            if r < 8 and c < 8:
                out.append(r * 8 + c)
    return np.array(out)


ZIGZAG = zigzag_order()


def ycc(img):
    """(rows, cols, 3) uint8 RGB -> (3, rows, cols) int64 Y, Cb, Cr; a gray plane -> (1, rows, cols)"""
    if img.ndim == 2:
        return img.astype(np.int64)[None]
    r, g, b = (img[..., i].astype(np.int64) for i in range(3))
    y = (fix(.299) * r + fix(.587) * g + fix(.114) * b + 32768) >> 16
    cb = (-fix(.16874) * r - fix(.33126) * g + fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (fix(.5) * r - fix(.41869) * g - fix(.08131) * b + (128 << 16) + 32767) >> 16
    return np.stack([y, cb, cr])


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def fdct_pass(d, first):
    """d: (..., 8) int64 along the last axis -> the same shape"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else descale(t10 - t11, 2)
    z1 = (t12 + t13) * F0_541
    o[2] = descale(z1 + t13 * F0_765, n)
    o[6] = descale(z1 - t12 * F1_847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F1_175
    t4, t5, t6, t7 = t4 * F0_298, t5 * F2_053, t6 * F3_072, t7 * F1_501
    z1, z2, z3, z4 = -z1 * F0_899, -z2 * F2_562, -z3 * F1_961 + z5, -z4 * F0_390 + z5
    o[7] = descale(t4 + z1 + z3, n)
    o[5] = descale(t5 + z2 + z4, n)
    o[3] = descale(t6 + z2 + z3, n)
    o[1] = descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def coefficients(img):
    """-> (n_mcus, components, 64) quantised coefficients in zigzag order, MCUs in raster order"""
    p = ycc(np.asarray(img))
    nc, rows, cols = p.shape
    pr, pc = -rows % 8, -cols % 8
    p = np.pad(p, ((0, 0), (0, pr), (0, pc)), mode="edge") - 128   # last column, then last row, of the converted samples
    by, bx = p.shape[1] // 8, p.shape[2] // 8
    blocks = p.reshape(nc, by, 8, bx, 8).transpose(1, 3, 0, 2, 4).reshape(by * bx, nc, 8, 8)
    t = fdct_pass(blocks, True)                                    # rows
    t = fdct_pass(t.swapaxes(-1, -2), False).swapaxes(-1, -2)      # columns
    q = np.sign(t) * ((np.abs(t) + 4) // 8)
    return q.reshape(by * bx, nc, 64)[..., ZIGZAG]


def parse_header(data):
    """-> dict: 'segments' [(marker, payload)], 'sof', 'dqt' {id: 64 values}, 'dht' {(class, id): (bits[16], vals)}, 'dri',
    'sos' (component selectors), 'scan_start' (offset behind the SOS header)"""
    assert data[:2] == b"\xff\xd8"
    out = {"segments": [], "dqt": {}, "dht": {}, "dri": None}
    pos = 2
    while True:
        assert data[pos] == 0xFF, pos
        marker = data[pos + 1]
        n = int.from_bytes(data[pos + 2:pos + 4], "big")
        body = data[pos + 4:pos + 2 + n]
        out["segments"].append((marker, body))
        pos += 2 + n
        if marker == 0xDB:
            while body:
                assert body[0] >> 4 == 0
                out["dqt"][body[0] & 15] = list(body[1:65])
                body = body[65:]
        elif marker == 0xC0:
            out["sof"] = {"precision": body[0], "rows": int.from_bytes(body[1:3], "big"), "cols": int.from_bytes(body[3:5], "big"),
                          "components": [(body[6 + 3 * i], body[7 + 3 * i], body[8 + 3 * i]) for i in range(body[5])]}
        elif marker == 0xC4:
            while body:
                bits = list(body[1:17])
                out["dht"][(body[0] >> 4, body[0] & 15)] = (bits, list(body[17:17 + sum(bits)]))
                body = body[17 + sum(bits):]
        elif marker == 0xDD:
            out["dri"] = int.from_bytes(body[:2], "big")
        elif marker == 0xDA:
            out["sos"] = [(body[1 + 2 * i], body[2 + 2 * i]) for i in range(body[0])]
            out["scan_start"] = pos
            return out


def scan_bytes(data):
    """the entropy-coded scan of a file: everything between the SOS header and EOI"""
    h = parse_header(data)
    assert data[-2:] == b"\xff\xd9"
    return data[h["scan_start"]:-2]


def split_segments(scan):
    """restart segments of a scan (an FF Dn pair inside a scan is always a marker: data FFs are stuffed)"""
    out, start, i = [], 0, 0
    while i + 1 < len(scan):
        if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7:
            out.append((scan[start:i], scan[i + 1] - 0xD0))
            start = i = i + 2
        else:
            i += 2 if scan[i] == 0xFF else 1
    out.append((scan[start:], None))
    return out


def huff_codes(bits, vals):
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


def library_tables(components):
    h = parse_header(sarpro_amd.host_jpeg_header(8, 8, components, 1))
    return {k: huff_codes(*v) for k, v in h["dht"].items()}


def encode_scan(img, restart):
    """the scan (restart markers included, EOI not) of `img` with a restart interval of `restart` MCUs (None / 0: no restarts)"""
    q = coefficients(img)
    n_mcus, nc, _ = q.shape
    tabs = library_tables(nc)
    out = bytearray()
    acc = nbits = 0
    pred = [0] * nc
    rst = 0

    def flush():
        nonlocal acc, nbits
        pad = -nbits % 8
        v = (acc << pad) | ((1 << pad) - 1)
        out.extend(v.to_bytes((nbits + pad) // 8, "big").replace(b"\xff", b"\xff\x00"))
        acc = nbits = 0

    def put(code, length):
        nonlocal acc, nbits
        acc = (acc << length) | code
        nbits += length

    def put_value(v, size):
        put((v - 1 if v < 0 else v) & ((1 << size) - 1), size)

    for m in range(n_mcus):
        if restart and m and m % restart == 0:
            flush()
            out.extend(bytes([0xFF, 0xD0 + rst]))
            rst = (rst + 1) & 7
            pred = [0] * nc
        for c in range(nc):
            dc_tab, ac_tab = tabs[(0, 1 if c else 0)], tabs[(1, 1 if c else 0)]
            blk = [int(x) for x in q[m, c]]
            diff = blk[0] - pred[c]
            pred[c] = blk[0]
            size = abs(diff).bit_length()
            put(*dc_tab[size])
            put_value(diff, size)
            run = 0
            for v in blk[1:]:
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    put(*ac_tab[0xF0])
                    run -= 16
                size = abs(v).bit_length()
                put(*ac_tab[(run << 4) | size])
                put_value(v, size)
                run = 0
            if run:
                put(*ac_tab[0])
    flush()
    return bytes(out)


def encode_file(img, restart):
    """the library's header + the restatement's scan + EOI"""
    img = np.asarray(img)
    rows, cols = img.shape[:2]
    return sarpro_amd.host_jpeg_header(cols, rows, 1 if img.ndim == 2 else 3, restart) + encode_scan(img, restart) + b"\xff\xd9"


# ---- which entropy symbols a raster makes the coder emit, and a raster built to make it emit all of them

def ac_events(q):
    """q: (n_blocks, 64) zigzag coefficients -> (block, run, size) of every coded AC coefficient, run = the zeros in front of it (0..62)"""
    b, p = np.nonzero(q[:, 1:])
    p = p + 1
    first = np.r_[True, b[1:] != b[:-1]] if b.size else np.zeros(0, bool)
    prev = np.where(first, 0, np.r_[0, p[:-1]])
    return b, p - prev - 1, np.frexp(np.abs(q[b, p]).astype(np.float64))[1]


def symbol_coverage(img, restart):
    """What the entropy coder meets in `img`, from coefficients(img) alone.  -> {table: dict}, table 0 (luminance / gray) and, for RGB,
    1 (both chrominance components): 'ac' the set of (run & 15, size) symbols, 'runs' the number of coded runs >= 16, >= 32, >= 48 (one,
    two, three ZRLs), 'no_eob' / 'eob' the number of blocks whose coefficient 63 is non-zero / zero, 'dc' the set of (size, sign) of the
    DC differences (sign -1, 0, 1) with the predictors reset every `restart` MCUs (None / 0: never)."""
    q = coefficients(img)
    n_mcus, nc, _ = q.shape
    out = {}
    for t in range(2 if nc == 3 else 1):
        qt = q[:, 1:] if t else q[:, :1]                      # (n_mcus, components of the table, 64)
        _, run, size = ac_events(qt.reshape(-1, 64))
        dc = qt[..., 0]
        diff = dc - np.concatenate([np.zeros_like(dc[:1]), dc[:-1]])
        if restart:
            diff[::restart] = dc[::restart]
        diff = diff.ravel()
        no_eob = int(np.count_nonzero(qt[..., 63]))
        out[t] = {"ac": set(zip((run & 15).tolist(), size.tolist())), "runs": tuple(int((run >= k).sum()) for k in (16, 32, 48)),
                  "no_eob": no_eob, "eob": qt.shape[0] * qt.shape[1] - no_eob,
                  "dc": set(zip(np.frexp(np.abs(diff).astype(np.float64))[1].tolist(), np.sign(diff).tolist()))}
    return out


ALL_AC = {(r, s) for r in range(16) for s in range(1, 11)}
ALL_DC = {(0, 0)} | {(s, g) for s in range(1, 12) for g in (-1, 1)}


def assert_full_coverage(cov, restart):
    """The conditions a crafted raster is built for, per table it uses: all 160 (run, size) AC symbols; a coded run in each of 16-31,
    32-47 and 48-62; blocks that end in EOB and blocks that do not; all 23 DC classes.  With an interval of 1 every DC difference is a
    block's own DC, (sum of 64 samples - 64 * 128) / 8, which lies in [-1024, 1016]: (11, +) needs >= 1024 and cannot occur, the other 22
    must."""
    for t, c in cov.items():
        assert c["ac"] == ALL_AC, (t, sorted(ALL_AC - c["ac"]))
        n16, n32, n48 = c["runs"]
        assert n16 - n32 >= 1 and n32 - n48 >= 1 and n48 >= 1, (t, c["runs"])
        assert c["no_eob"] >= 1 and c["eob"] >= 1, (t, c["no_eob"], c["eob"])
        want = ALL_DC - {(11, 1)} if restart == 1 else ALL_DC
        assert c["dc"] == want, (t, sorted(want ^ c["dc"]))


def segments_ending_stuffed(scan):
    """how many restart segments of a scan end in FF 00: a last, 1-padded byte of 0xFF, stuffed like a data byte"""
    return sum(1 for s, _ in split_segments(scan) if s[-2:] == b"\xff\x00")


def dct_basis():
    """(64, 8, 8): the orthonormal 8 x 8 DCT basis functions in zigzag order -- with every quantiser 1 the k-th coefficient of a block is
    its inner product with the k-th of these"""
    u = np.arange(8)
    c = np.cos((2 * u[None, :] + 1) * u[:, None] * np.pi / 16) * np.where(u[:, None] == 0, np.sqrt(0.125), 0.5)
    return (c[:, None, :, None] * c[None, :, None, :]).reshape(64, 8, 8)[ZIGZAG]


BASIS = dct_basis()
CHROMA_SWING = 70    # |Cb - 128|, |Cr - 128| of the random chroma blocks: with Y = 128 the RGB stays within 0..255


def random_planes(rng, n, lo, hi):
    """n level-shifted 8 x 8 float planes within [lo, hi]: 1, 2, 3 or 6 coefficients at random zigzag positions 1..63 with signed
    amplitudes log-uniform in 1..590, the AC part scaled down where the samples would leave the range, on a DC that is dense near 0 and
    reaches both ends of the range"""
    out = np.empty((n, 8, 8))
    for i in range(n):
        k = rng.choice(np.arange(1, 64), size=rng.choice([1, 2, 3, 6]), replace=False)
        amp = rng.choice([-1.0, 1.0], k.size) * np.exp(rng.uniform(0, np.log(590.0), k.size))
        ac = np.tensordot(amp, BASIS[k], 1)
        u = rng.uniform(-1, 1)
        dc = u ** 3 * (hi if u > 0 else -lo)
        out[i] = dc + ac * min(1.0, (hi - dc) / max(ac.max(), 1e-9), (dc - lo) / max(-ac.min(), 1e-9))
    return out


def to_u8(x):
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def gray_blocks(planes):
    return to_u8(planes + 128)


def chroma_blocks(cb, cr):
    """(n, 8, 8) level-shifted Cb and Cr planes on Y = 128 -> (n, 8, 8, 3) RGB"""
    return to_u8(np.stack([128 + 1.402 * cr, 128 - 0.344136 * cb - 0.714136 * cr, 128 + 1.772 * cb], -1))


def sign_blocks(colours):
    """2 x 63 blocks per pair of colours: the first colour where basis function k is positive and the second elsewhere, then the
    inverse, k = 1..63 -- the largest coefficient a block can have at position k (size 10), position 63 included (no EOB)"""
    out = []
    for a, b in colours:
        a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
        for k in range(1, 64):
            pos = BASIS[k] > 0
            out += [np.where(pos[..., None], a, b), np.where(pos[..., None], b, a)]
    return np.stack(out)


def block_classes(q):
    """q: (n, 64) -> per block the set of what it contributes to the AC conditions"""
    out = [{("end", bool(v))} for v in q[:, 63]]
    for b, run, size in zip(*(x.tolist() for x in ac_events(q))):
        out[b].add((run & 15, size))
        if run >= 16:
            out[b].add(("run", run >> 4))
    return out


def pick(classes, have, n):
    """indices of n items of `classes` (a list of sets): in order, those that bring a class `have` lacks (`have` is updated), then the
    first of the others"""
    first = []
    for i, c in enumerate(classes):
        if not c <= have:
            first.append(i)
            have |= c
    assert len(first) <= n, (len(first), n)
    taken = set(first)
    return first + [i for i in range(len(classes)) if i not in taken][: n - len(first)]


def mosaic(blocks, by, bx):
    """(by * bx, 8, 8[, 3]) blocks in MCU (raster) order -> the raster"""
    assert len(blocks) == by * bx, (len(blocks), by, bx)
    b = blocks.reshape((by, bx) + blocks.shape[1:])
    return np.ascontiguousarray(b.swapaxes(1, 2).reshape((by * 8, bx * 8) + blocks.shape[3:]))


def read_only(a):
    a.flags.writeable = False
    return a


def strip_coefficients(blocks):
    """coefficients of blocks taken one by one -> (n, components, 64)"""
    return coefficients(mosaic(blocks, 1, len(blocks)))


# the last block of a crafted raster: a checkerboard of two levels whose coefficient 63 (the last value coded, in the last component) is
# -256 -- value bits 0 1111 1111 (-257 in 9 bits), so whatever bit position they start at, the scan's last byte, and with it the last
# restart segment's at every interval, is eight 1-bits of data and padding: an 0xFF that has to be stuffed
END_GRAY = (167, 89)                           # the level where basis function 63 is negative, then where it is positive
END_RGB = ((206, 128, 128), (50, 128, 128))    # the same in Cr, the last component coded

# blocks: 296 x 352 gray (0.104 M samples), 296 x 392 RGB (0.348 M samples); neither count is a multiple of 5
CRAFTED_SHAPE = {1: (37, 44), 3: (37, 49)}


@functools.lru_cache(maxsize=None)
def crafted_raster(nc, seed=0):
    """A deterministic mosaic of 8 x 8 blocks that makes the entropy coder emit every symbol class (assert_full_coverage), gray
    (nc = 1) or RGB (nc = 3), under 0.35 M samples.  In MCU order:
      - five flat blocks, black, black, white, white, black (RGB: blue, blue, yellow, yellow, black, the ends of Y and of Cb): DC
        differences of size 11 with both signs and of size 0 within one segment of 5, and a DC of -1024 by itself
      - random blocks (random_planes), chosen from a pool three times as large: first the ones that bring a missing class
        (block_classes), then the pool in order.  RGB: gray ones for the luminance table, then ones with Y = 128 and random Cb and Cr
        planes within +-CHROMA_SWING for the chrominance table
      - the sign blocks: black / white; RGB: blue / yellow and red / cyan as well, the full swing of Cb and of Cr
      - the last block (END_GRAY / END_RGB)"""
    rng = np.random.default_rng(seed)
    by, bx = CRAFTED_SHAPE[nc]
    n = by * bx
    if nc == 1:
        flat = np.repeat(np.array([0, 0, 255, 255, 0], np.uint8), 64).reshape(5, 8, 8)
        signs = sign_blocks([(255, 0)])[..., 0]
        checker = np.where(BASIS[63] > 0, np.uint8(END_GRAY[1]), np.uint8(END_GRAY[0]))[None]
        n_rand = n - len(flat) - len(signs) - 1
        pool = gray_blocks(random_planes(rng, 3 * n_rand, -128, 127))
        have = set().union(*block_classes(strip_coefficients(signs)[:, 0]))
        rand = pool[pick(block_classes(strip_coefficients(pool)[:, 0]), have, n_rand)]
        return read_only(mosaic(np.concatenate([flat, rand, signs, checker]), by, bx))
    blue, yellow, red, cyan = (0, 0, 255), (255, 255, 0), (255, 0, 0), (0, 255, 255)
    flat = np.broadcast_to(np.array([blue, blue, yellow, yellow, (0, 0, 0)], np.uint8)[:, None, None], (5, 8, 8, 3))
    signs = sign_blocks([((255,) * 3, (0,) * 3), (blue, yellow), (red, cyan)])
    checker = np.where((BASIS[63] > 0)[..., None], np.array(END_RGB[1], np.uint8), np.array(END_RGB[0], np.uint8))[None]
    n_rand = n - len(flat) - len(signs) - 1
    n_luma = n_rand // 2
    q = strip_coefficients(signs)
    have_y, have_c = set().union(*block_classes(q[:, 0])), set().union(*block_classes(q[:, 1]), *block_classes(q[:, 2]))
    pool = np.repeat(gray_blocks(random_planes(rng, 3 * n_luma, -128, 127))[..., None], 3, -1)
    luma = pool[pick(block_classes(strip_coefficients(pool)[:, 0]), have_y, n_luma)]
    m = 3 * (n_rand - n_luma)
    pool = chroma_blocks(random_planes(rng, m, -CHROMA_SWING, CHROMA_SWING), random_planes(rng, m, -CHROMA_SWING, CHROMA_SWING))
    q = strip_coefficients(pool)
    chroma = pool[pick([a | b for a, b in zip(block_classes(q[:, 1]), block_classes(q[:, 2]))], have_c, n_rand - n_luma)]
    return read_only(mosaic(np.concatenate([flat, luma, chroma, signs, checker]), by, bx))
