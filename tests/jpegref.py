"""numpy restatement of the baseline JPEG the library writes (quality 100, 4:4:4, Annex K tables, restart intervals): libjpeg's
jccolor, edge replication, jfdctint, divisor 8, jchuff's entropy coding.  The Huffman tables are read from the library's own header
(sarpro_amd.host_jpeg_header), so the restatement codes with what the file declares.  test_jpeg_host.py holds it against Pillow
(libjpeg-turbo) byte for byte; the stage functions (ycc, coefficients, split_segments) localise a failing GPU comparison."""
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
