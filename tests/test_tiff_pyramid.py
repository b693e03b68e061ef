"""The tiled TIFF writer with overviews (sarpro_hip_tiff_create_pyramid), no GPU: the file's structure through a
struct-based parser of this test's own (classic TIFF and BigTIFF), the pixels through Pillow, the geo tags, the BigTIFF size rule."""
import struct

import numpy as np
import pytest

import sarpro_amd as S
from sarpro_amd import _lib

TYPE_FMT = {1: "B", 2: "c", 3: "H", 4: "I", 12: "d", 16: "Q"}


def parse(path):
    """-> (big, [ {tag: (type, values)} per directory ], [offset of each directory], raw bytes)"""
    raw = open(path, "rb").read()
    assert raw[:2] == b"II"
    magic = struct.unpack_from("<H", raw, 2)[0]
    big = magic == 43
    assert magic in (42, 43)
    if big:
        assert struct.unpack_from("<HH", raw, 4) == (8, 0)
        off = struct.unpack_from("<Q", raw, 8)[0]
    else:
        off = struct.unpack_from("<I", raw, 4)[0]
    dirs, offs, extents = [], [], []
    while off:
        offs.append(off)
        n = struct.unpack_from("<Q" if big else "<H", raw, off)[0]
        p = off + (8 if big else 2)
        d, end = {}, p + n * (20 if big else 12) + (8 if big else 4)
        for _ in range(n):
            tag, typ = struct.unpack_from("<HH", raw, p)
            cnt = struct.unpack_from("<Q" if big else "<I", raw, p + 4)[0]
            size = struct.calcsize(TYPE_FMT[typ]) * cnt
            cap = 8 if big else 4
            vp = p + (12 if big else 8)
            if size > cap:
                vp = struct.unpack_from("<Q" if big else "<I", raw, vp)[0]
                end = max(end, vp + size)
            vals = struct.unpack_from("<%d%s" % (cnt, TYPE_FMT[typ]), raw, vp)
            assert tag not in d and (not d or tag > max(d))                        # ascending tags
            d[tag] = (typ, list(vals))
            p += 20 if big else 12
        dirs.append(d)
        extents.append(end)
        off = struct.unpack_from("<Q" if big else "<I", raw, p)[0]
    return big, dirs, offs, extents, raw


def level_shapes(w, h, levels):
    out = [(w, h)]
    for _ in range(levels):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def make_levels(w, h, samples, dtype, levels, seed):
    rng = np.random.default_rng(seed)
    hi = 256 if dtype == np.uint8 else 65536
    return [rng.integers(1, hi, (lh, lw, samples)).astype(dtype) for lw, lh in level_shapes(w, h, levels)]   # (never 0: padding must be)


def write(path, data, tile, seed=0, **kw):
    """every level in shuffled row chunks of uneven sizes"""
    h, w, samples = data[0].shape
    wr = S.TiffPyramidWriter(str(path), w, h, samples, data[0].dtype.itemsize * 8, len(data) - 1, tile=tile, **kw)
    rng = np.random.default_rng(seed)
    jobs = []
    for k, a in enumerate(data):
        r = 0
        while r < a.shape[0]:
            n = int(min(a.shape[0] - r, rng.integers(1, 2 * (tile or 512) + 3)))
            jobs.append((k, r, n))
            r += n
    for i in rng.permutation(len(jobs)):
        k, r, n = jobs[i]
        wr.write_level_rows(k, r, data[k][r:r + n])
    wr.finish()


def tiles_of(raw, d, samples, itemsize, dtype):
    """the level's raster reassembled from its tiles, and the padding bytes"""
    w, h, tw, th = d[256][1][0], d[257][1][0], d[322][1][0], d[323][1][0]
    tx, ty = (w + tw - 1) // tw, (h + th - 1) // th
    offs, lens = d[324][1], d[325][1]
    assert len(offs) == len(lens) == tx * ty and all(n == tw * th * samples * itemsize for n in lens)
    full = np.zeros((ty * th, tx * tw, samples), dtype)
    for i, o in enumerate(offs):
        t = np.frombuffer(raw, dtype, tw * th * samples, o).reshape(th, tw, samples)
        full[(i // tx) * th:(i // tx + 1) * th, (i % tx) * tw:(i % tx + 1) * tw] = t
    return full[:h, :w], full[h:], full[:, w:]


CASES = [(np.uint8, 1, 16, 37, 53, 2), (np.uint8, 3, 16, 50, 33, 2), (np.uint16, 1, 64, 130, 67, 2), (np.uint16, 2, 64, 65, 129, 1),
         (np.uint8, 3, 64, 200, 130, 3), (np.uint16, 1, 16, 16, 16, 0)]


@pytest.mark.parametrize("dtype,samples,tile,w,h,levels", CASES)
def test_structure(tmp_path, dtype, samples, tile, w, h, levels):
    data = make_levels(w, h, samples, dtype, levels, 1)
    path = tmp_path / "p.tif"
    write(path, data, tile)
    big, dirs, offs, extents, raw = parse(path)
    isz = np.dtype(dtype).itemsize
    assert not big and len(dirs) == levels + 1                                      # the directory count
    first_tile = min(o for d in dirs for o in d[324][1])
    assert offs == sorted(offs) and max(extents) <= first_tile                       # every directory and array lies before the first tile byte
    prev_last = None
    for k in range(levels, -1, -1):                                                  # smaller levels come first in the file
        o = dirs[k][324][1]
        assert all(b > a for a, b in zip(o, o[1:]))                                  # strictly increasing within a level
        assert all(b - a == tile * tile * samples * isz for a, b in zip(o, o[1:]))  # row-major, back to back
        assert prev_last is None or o[0] > prev_last
        prev_last = o[-1]
    assert prev_last + tile * tile * samples * isz == len(raw)                       # the file ends with the full resolution's last tile
    for k, (d, (lw, lh)) in enumerate(zip(dirs, level_shapes(w, h, levels))):
        assert (254 in d) == (k > 0) and (k == 0 or d[254][1] == [1])                # NewSubfileType = 1 on the overviews
        assert (d[256][1], d[257][1]) == ([lw], [lh])
        assert d[258][1] == [8 * isz] * samples and d[259][1] == [1] and d[277][1] == [samples] and d[284][1] == [1]
        assert d[262][1] == [2 if samples >= 3 else 1] and d[339][1] == [1] * samples
        assert (338 in d) == (samples == 2) and (samples != 2 or d[338][1] == [0])   # as the strip writer's directory
        assert d[322][1] == [tile] and d[323][1] == [tile] and 273 not in d and 278 not in d
        assert not any(t in d for t in (33550, 33922, 34735))
        img, pad_rows, pad_cols = tiles_of(raw, d, samples, isz, dtype)
        assert np.array_equal(img, data[k]), k
        assert not pad_rows.any() and not pad_cols.any()                             # edge-tile padding is zero


def test_the_strip_writers_tags_for_the_same_samples(tmp_path):
    """Photometric / ExtraSamples / SampleFormat / BitsPerSample equal what sarpro_hip_tiff_create writes"""
    for samples, dtype in ((1, np.uint8), (2, np.uint16), (3, np.uint8)):
        a = make_levels(20, 10, samples, dtype, 0, 3)
        write(tmp_path / "t.tif", a, 16)
        s = S.TiffWriter(str(tmp_path / "s.tif"), 20, 10, samples, a[0].dtype.itemsize * 8)
        s.write_rows(0, a[0])
        s.finish()
        dt, ds = parse(tmp_path / "t.tif")[1][0], parse(tmp_path / "s.tif")[1][0]
        for tag in (256, 257, 258, 259, 262, 277, 284, 338, 339):
            assert dt.get(tag) == ds.get(tag), tag


def test_tile_defaults_and_argument_checks(tmp_path):
    write(tmp_path / "d.tif", make_levels(600, 20, 1, np.uint8, 1, 2), 0)
    d = parse(tmp_path / "d.tif")[1]
    assert d[0][322][1] == [512] and d[1][323][1] == [512] and len(d[0][324][1]) == 2
    for bad in (dict(tile=24), dict(levels=17), dict(levels=-1), dict(bits=12), dict(width=0)):
        kw = dict(width=10, height=10, samples=1, bits=8, levels=1, tile=16)
        kw.update(bad)
        with pytest.raises(S.SarproHipError):
            S.TiffPyramidWriter(str(tmp_path / "x.tif"), kw["width"], kw["height"], kw["samples"], kw["bits"], kw["levels"], tile=kw["tile"])
    wr = S.TiffPyramidWriter(str(tmp_path / "y.tif"), 10, 10, 1, 8, 1, tile=16)
    with pytest.raises(S.SarproHipError):
        wr.write_level_rows(2, 0, np.zeros((1, 10), np.uint8))                      # no such level
    with pytest.raises(S.SarproHipError):
        wr.write_level_rows(1, 4, np.zeros((2, 5), np.uint8))                       # level 1 has 5 rows
    with pytest.raises(S.SarproHipError):
        wr.write_level_rows(0, 0, np.zeros((1, 9), np.uint8))                       # a row shorter than the level's
    wr.finish()
    sw = S.TiffWriter(str(tmp_path / "z.tif"), 10, 10, 1, 8)
    assert _lib.lib.sarpro_hip_tiff_write_level_rows(sw._h, 0, 0, 1, np.zeros(10, np.uint8).ctypes.data, 10) == _lib.ERR_INVALID_ARG  # a strip writer
    sw.finish()


def test_unwritten_tiles_read_as_zeros_and_the_reader_stays_strip_only(tmp_path):
    wr = S.TiffPyramidWriter(str(tmp_path / "u.tif"), 40, 40, 1, 8, 1, tile=16)
    wr.write_level_rows(0, 16, np.full((3, 40), 9, np.uint8))
    wr.finish()
    _, dirs, _, _, raw = parse(tmp_path / "u.tif")
    img = tiles_of(raw, dirs[0], 1, 1, np.uint8)[0][..., 0]
    assert img[16:19].min() == 9 and img[:16].max() == 0 and img[19:].max() == 0 and not tiles_of(raw, dirs[1], 1, 1, np.uint8)[0].any()
    with pytest.raises(S.SarproHipError):
        S.TiffReader(str(tmp_path / "u.tif"))


@pytest.mark.parametrize("dtype,samples,mode", [(np.uint8, 1, "L"), (np.uint8, 3, "RGB"), (np.uint16, 1, "I;16")])
def test_read_back_with_pillow(tmp_path, dtype, samples, mode):
    from PIL import Image                                                            # (an independent reader: its absence is a failure, not a skip)
    data = make_levels(150, 97, samples, dtype, 3, 5)
    path = tmp_path / "pil.tif"
    write(path, data, 32, seed=7)
    with Image.open(str(path)) as im:
        assert im.n_frames == 4
        for k, a in enumerate(data):
            im.seek(k)
            assert im.size == (a.shape[1], a.shape[0]) and im.mode == mode
            got = np.asarray(im)
            assert np.array_equal(got.reshape(a.shape), a), k


def test_geo_tags_on_directory_0_round_trip(tmp_path):
    src = tmp_path / "src.tif"                                                       # a strip file with a GeoKey directory to carry over ...
    keys = [1, 1, 0, 3, 1024, 0, 1, 2, 1025, 0, 1, 1, 2048, 0, 1, 4326]
    img = np.arange(6, dtype=np.uint16).reshape(2, 3)
    ents = [(256, 3, [3]), (257, 3, [2]), (258, 3, [16]), (259, 3, [1]), (262, 3, [1]), (273, 4, [8]), (277, 3, [1]), (278, 3, [2]),
            (279, 4, [12]), (34735, 3, keys), (34736, 12, [6378137.0, 298.25]), (34737, 2, [bytes([c]) for c in b"WGS 84|\0"])]
    ifd_at = 8 + 12
    body, extra = struct.pack("<H", len(ents)), b""
    extra_at = ifd_at + 2 + 12 * len(ents) + 4
    for tag, typ, vals in ents:
        payload = struct.pack("<%d%s" % (len(vals), TYPE_FMT[typ]), *vals)
        if len(payload) <= 4:
            field = payload.ljust(4, b"\0")
        else:
            field = struct.pack("<I", extra_at + len(extra))
            extra += payload + b"\0" * (-len(payload) % 2)
        body += struct.pack("<HHI", tag, typ, len(vals)) + field
    src.write_bytes(b"II" + struct.pack("<HI", 42, ifd_at) + img.tobytes() + body + struct.pack("<I", 0) + extra)
    rd = S.TiffReader(str(src))
    gt = [500000.0, 10.0, 0.0, 4100000.0, 0.0, -10.0]
    data = make_levels(40, 30, 3, np.uint8, 2, 8)
    write(tmp_path / "g.tif", data, 16, geotransform=gt, geo_keys_from=rd)
    _, dirs, _, _, _ = parse(tmp_path / "g.tif")
    d0 = dirs[0]
    assert d0[33550] == (12, [10.0, 10.0, 0.0]) and d0[33922] == (12, [0.0, 0.0, 0.0, 500000.0, 4100000.0, 0.0])
    assert d0[34735] == (3, keys) and d0[34736] == (12, [6378137.0, 298.25]) and b"".join(d0[34737][1]) == b"WGS 84|\0"
    for d in dirs[1:]:
        assert not any(t in d for t in (33550, 33922, 34735, 34736, 34737))         # the geo tags go on directory 0 only


@pytest.mark.parametrize("dtype,samples,tile", [(np.uint8, 3, 32), (np.uint16, 1, 16)])
def test_bigtiff_form_on_a_small_file(tmp_path, monkeypatch, dtype, samples, tile):
    """SARPRO_HIP_TIFF_BIGTIFF=YES at creation writes the BigTIFF form whatever the size: 16-byte header, 20-byte entries, LONG8 offset
    and byte-count arrays, 8-byte next-directory pointers -- the same structure, pixels and geo tags, read by this file's parser and
    by Pillow"""
    from PIL import Image
    data = make_levels(150, 97, samples, dtype, 3, 11)
    gt = [1.0, 2.0, 0.0, 3.0, 0.0, -2.0]
    write(tmp_path / "classic.tif", data, tile, seed=3, geotransform=gt)
    monkeypatch.setenv("SARPRO_HIP_TIFF_BIGTIFF", "YES")
    write(tmp_path / "big.tif", data, tile, seed=3, geotransform=gt)
    monkeypatch.delenv("SARPRO_HIP_TIFF_BIGTIFF")
    big, dirs, offs, extents, raw = parse(tmp_path / "big.tif")
    cbig, cdirs, _, _, _ = parse(tmp_path / "classic.tif")
    isz = np.dtype(dtype).itemsize
    assert big and not cbig and len(dirs) == len(cdirs) == 4
    assert offs[0] == 16 and offs == sorted(offs) and max(extents) <= min(o for d in dirs for o in d[324][1])
    prev_last = None
    for k in range(3, -1, -1):
        o = dirs[k][324][1]
        assert dirs[k][324][0] == dirs[k][325][0] == 16                               # LONG8 arrays
        assert all(b - a == tile * tile * samples * isz for a, b in zip(o, o[1:])) and (prev_last is None or o[0] > prev_last)
        prev_last = o[-1]
    assert prev_last + tile * tile * samples * isz == len(raw)
    for k, (d, c) in enumerate(zip(dirs, cdirs)):
        assert set(d) == set(c) and all(d[t][1] == c[t][1] for t in d if t not in (324, 325)), k   # the classic file's tags and values
        img, pad_rows, pad_cols = tiles_of(raw, d, samples, isz, dtype)
        assert np.array_equal(img, data[k]) and not pad_rows.any() and not pad_cols.any()
    assert dirs[0][33550][1] == [2.0, 2.0, 0.0] and 33550 not in dirs[1]
    with Image.open(str(tmp_path / "big.tif")) as im:
        assert im.n_frames == 4
        for k, a in enumerate(data):
            im.seek(k)
            assert np.array_equal(np.asarray(im).reshape(a.shape), a), k
    assert S.tiff_pyramid_is_bigtiff(150, 97, samples, isz * 8, tile, 3)[0] is False  # (the rule itself does not read the request)


def test_bigtiff_size_rule():
    """The strip writer's rule on the whole file: BigTIFF once the file and a 1 MiB reserve reach 2^32 - 1 bytes.  (No multi-GiB
    file is written: the rule is a pure function.)"""
    big, n = S.tiff_pyramid_is_bigtiff(20000, 20000, 3, 8, 512, 6)
    # 40 x 40 tiles of 768 KiB at level 0, then 20^2, 10^2, 5^2, 3^2, 2^2, 1: the data alone
    tiles = 1600 + 400 + 100 + 25 + 9 + 4 + 1
    assert not big and tiles * 512 * 512 * 3 < n < tiles * 512 * 512 * 3 + (1 << 20)
    assert S.tiff_pyramid_is_bigtiff(40000, 40000, 3, 8, 512, 7)[0]                  # 4.8 GB of RGB
    assert S.tiff_pyramid_is_bigtiff(16, 16, 1, 8, 16, 0) == (False, 8 + 152 + 256)    # header, 12 entries (2 + 144 + 4, padded to 8), one tile
    # the edge, on one row of 512 x 512 u8 tiles (256 KiB each): n tiles of data + the classic directory
    for ntiles in range(16370, 16384):
        big, n = S.tiff_pyramid_is_bigtiff(512 * ntiles, 512, 1, 8, 512, 0)
        classic = 8 + 152 + 2 * ((4 * ntiles + 7) // 8 * 8)                         # ... and the two LONG arrays, each padded to 8
        classic = (classic + 15) // 16 * 16 + ntiles * 512 * 512
        assert big == (classic + (1 << 20) >= 0xFFFFFFFF), ntiles
        assert big or n == classic
    with pytest.raises(S.SarproHipError):
        S.tiff_pyramid_is_bigtiff(10, 10, 1, 8, 20, 0)
