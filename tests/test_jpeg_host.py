"""The JPEG encoder's host half (no GPU): the numpy restatement of its arithmetic (tests/jpegref.py) against Pillow's libjpeg-turbo byte
for byte, the header the library builds, the size bound and the argument rules."""
import io

import numpy as np
import pytest
from PIL import Image

import jpegref
import sarpro_amd
from sarpro_amd import _lib

SHAPES = [(1, 1), (8, 8), (16, 16), (37, 53), (64, 64), (24, 200), (129, 250)]  # (rows, cols)
RESTARTS = [None, 1, 3, 5, 8]


def pillow_file(img, restart):
    buf = io.BytesIO()
    kw = {"restart_marker_blocks": restart} if restart else {}
    Image.fromarray(img).save(buf, "JPEG", quality=100, subsampling=0, **kw)
    return buf.getvalue()


def raster(rows, cols, nc, seed, kind="noise"):
    rng = np.random.default_rng(seed)
    shape = (rows, cols) if nc == 1 else (rows, cols, 3)
    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "smooth":  # low-amplitude texture on a gradient: long zero runs, ZRL and EOB symbols
        y, x = np.mgrid[0:rows, 0:cols]
        base = (x * 2 + y * 3) % 256
        img = np.stack([base, base[::-1], (base + 40) % 256], -1) if nc == 3 else base
        return (img + rng.integers(0, 2, shape)).astype(np.uint8)
    if kind == "extremes":  # alternating 0 / 255: the largest coefficients the transform produces
        y, x = np.mgrid[0:rows, 0:cols]
        v = (((x + y) & 1) * 255).astype(np.uint8)
        return v if nc == 1 else np.stack([v, 255 - v, v], -1)
    raise ValueError(kind)


@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_scan_equals_pillow(shape, nc):
    rows, cols = shape
    for kind in ("noise", "smooth"):
        img = raster(rows, cols, nc, rows * 1000 + cols, kind)
        for r in RESTARTS:
            assert jpegref.encode_scan(img, r) == jpegref.scan_bytes(pillow_file(img, r)), (shape, nc, kind, r)


def test_restart_cycle_wraps_and_scans_hold_stuffed_bytes():
    img = raster(64, 64, 3, 5)
    scan = jpegref.encode_scan(img, 1)
    segs = jpegref.split_segments(scan)
    assert len(segs) == 64 and [n for _, n in segs[:10]] == [0, 1, 2, 3, 4, 5, 6, 7, 0, 1] and segs[-1][1] is None
    assert b"\xff\x00" in scan
    assert scan == jpegref.scan_bytes(pillow_file(img, 1))


@pytest.mark.parametrize("nc", [1, 3])
def test_crafted_raster_is_small_and_deterministic(nc):
    img = jpegref.crafted_raster(nc)
    assert img.dtype == np.uint8 and img.ndim == (2 if nc == 1 else 3) and img.size < 350_000   # samples: under 0.35 MP either way
    n_mcus = img.shape[0] * img.shape[1] // 64
    assert img.shape[0] % 8 == 0 and img.shape[1] % 8 == 0 and n_mcus > 1600 and n_mcus % 5   # an interval of 5 leaves a ragged segment
    assert np.array_equal(img, jpegref.crafted_raster.__wrapped__(nc))


@pytest.mark.parametrize("r", [None, 1, 5, 65535])
@pytest.mark.parametrize("nc", [1, 3])
def test_restatement_scan_of_the_crafted_raster_equals_pillow(nc, r):
    """every (run, size) symbol of each table, single, double and triple ZRLs, blocks with and without EOB, every DC class and a
    segment that ends in a stuffed FF: asserted on the raster first, then the restatement's scan against libjpeg-turbo's"""
    img = jpegref.crafted_raster(nc)
    jpegref.assert_full_coverage(jpegref.symbol_coverage(img, r), r)
    ref = jpegref.scan_bytes(pillow_file(img, r))
    assert jpegref.segments_ending_stuffed(ref) >= 1
    assert len(jpegref.split_segments(ref)) == (-(-(img.shape[0] * img.shape[1] // 64) // r) if r else 1)
    assert jpegref.encode_scan(img, r) == ref


def test_symbol_coverage_counts_what_it_says():
    """two hand-made coefficient blocks through the report's own counting (ac_events) and a raster whose report is known"""
    q = np.zeros((2, 64), np.int64)
    q[0, [1, 18, 63]] = [5, -1, 700]           # runs 0, 16, 44
    q[1, [50]] = [-512]                        # run 49
    b, run, size = jpegref.ac_events(q)
    assert b.tolist() == [0, 0, 0, 1] and run.tolist() == [0, 16, 44, 49] and size.tolist() == [3, 1, 10, 10]
    flat = np.repeat(np.repeat(np.array([[0, 255, 255, 130]], np.uint8), 8, 0), 8, 1)   # DCs -1024, 1016, 1016, 16
    c = jpegref.symbol_coverage(flat, None)[0]
    assert c == {"ac": set(), "runs": (0, 0, 0), "no_eob": 0, "eob": 4, "dc": {(11, -1), (11, 1), (0, 0), (10, -1)}}
    assert jpegref.symbol_coverage(flat, 1)[0]["dc"] == {(11, -1), (10, 1), (5, 1)}
    assert jpegref.symbol_coverage(flat, 2)[0]["dc"] == {(11, -1), (11, 1), (10, 1), (10, -1)}
    assert set(jpegref.symbol_coverage(np.repeat(flat[..., None], 3, -1), 1)) == {0, 1}


ANNEX_K_COUNTS = {(0, 0): [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], (0, 1): [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0],
                  (1, 0): [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], (1, 1): [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]}


@pytest.mark.parametrize("nc", [1, 3])
def test_header(nc):
    rows, cols, r = 129, 250, 5
    data = sarpro_amd.host_jpeg_header(cols, rows, nc, r)
    h = jpegref.parse_header(data)
    assert h["scan_start"] == len(data)
    markers = [m for m, _ in h["segments"]]
    assert markers == [0xE0] + [0xDB] * (2 if nc == 3 else 1) + [0xC0] + [0xC4] * (4 if nc == 3 else 2) + [0xDD, 0xDA]
    assert h["segments"][0][1] == b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    assert h["sof"]["precision"] == 8 and h["sof"]["rows"] == rows and h["sof"]["cols"] == cols
    assert h["sof"]["components"] == [(1, 0x11, 0), (2, 0x11, 1), (3, 0x11, 1)][:nc]
    assert h["dqt"] == {t: [1] * 64 for t in range(2 if nc == 3 else 1)}
    assert h["dri"] == r
    assert h["sos"] == [(1, 0x00), (2, 0x11), (3, 0x11)][:nc]
    # Annex K.3-K.6: the counts as printed in the standard, the symbols as libjpeg-turbo (Pillow, tables not optimised) writes them
    ref = jpegref.parse_header(pillow_file(raster(8, 8, nc, 0), None))["dht"]
    assert sorted(h["dht"]) == sorted(ref) == ([(0, 0), (0, 1), (1, 0), (1, 1)] if nc == 3 else [(0, 0), (1, 0)])
    for k in h["dht"]:
        assert h["dht"][k][0] == ANNEX_K_COUNTS[k] and h["dht"][k] == ref[k], k
    # the default interval is declared too
    assert jpegref.parse_header(sarpro_amd.host_jpeg_header(cols, rows, nc))["dri"] >= 1


@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("shape,r", [((37, 53), 3), ((64, 64), 1), ((24, 200), 8)])
def test_round_trip_through_pillow(shape, r, nc):
    img = raster(shape[0], shape[1], nc, 11)
    ours = jpegref.encode_file(img, r)
    dec = np.asarray(Image.open(io.BytesIO(ours)))
    ref = np.asarray(Image.open(io.BytesIO(pillow_file(img, r))))
    assert dec.shape == img.shape and np.array_equal(dec, ref)


@pytest.mark.parametrize("nc", [1, 3])
def test_bound_holds(nc):
    for (rows, cols), r in [((37, 53), 1), ((64, 64), 3), ((24, 200), 8), ((16, 16), 0)]:
        bound = sarpro_amd.jpeg_bound(cols, rows, nc, r)
        for kind in ("noise", "extremes"):
            img = raster(rows, cols, nc, 3, kind)
            rr = r or jpegref.parse_header(sarpro_amd.host_jpeg_header(cols, rows, nc))["dri"]
            assert len(jpegref.encode_file(img, rr)) <= bound, (rows, cols, nc, r, kind)


def test_invalid_arguments_are_refused():
    for cols, rows, nc, r in [(0, 8, 3, 1), (8, 0, 3, 1), (65536, 8, 3, 1), (8, 65536, 1, 1), (8, 8, 2, 1), (8, 8, 4, 1), (8, 8, 0, 1),
                              (8, 8, 3, 65536)]:
        for f in (sarpro_amd.host_jpeg_header, sarpro_amd.jpeg_bound):
            with pytest.raises(sarpro_amd.SarproHipError) as ei:
                f(cols, rows, nc, r)
            assert ei.value.code == _lib.ERR_INVALID_ARG, (cols, rows, nc, r)
    assert sarpro_amd.jpeg_bound(65535, 65535, 3, 65535) > 65535 * 65535 * 3
    import ctypes as C
    n = C.c_size_t(0)
    small = np.empty(16, np.uint8)
    rc = _lib.lib.sarpro_hip_host_jpeg_header(8, 8, 3, 1, small.ctypes.data_as(C.c_void_p), small.size, C.byref(n))
    assert rc == _lib.ERR_BUFFER_TOO_SMALL and n.value == len(sarpro_amd.host_jpeg_header(8, 8, 3, 1))
