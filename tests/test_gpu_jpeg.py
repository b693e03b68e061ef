"""The device JPEG encoder against Pillow's libjpeg-turbo (quality=100, subsampling=0, restart_marker_blocks=R): the entropy-coded scan
is equal byte for byte, and the library's whole file opens in Pillow and decodes to Pillow's pixels.  tests/jpegref.py (held against
Pillow without a GPU by test_jpeg_host.py) localises a difference to a stage in the assertion message."""
import io

import numpy as np
import pytest
from PIL import Image

import f32data
import jpegref
import sarpro_amd
from sarpro_amd import AutoscaleStrategy as St, _lib, synth

pytestmark = pytest.mark.gpu


def pillow_file(img, restart):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=100, subsampling=0, restart_marker_blocks=restart)
    return buf.getvalue()


def check_against_pillow(data, img, restart=None):
    """`data`: the library's file of `img`; restart None: whatever the file declares (the library's default)"""
    h = jpegref.parse_header(data)
    r = h["dri"]
    assert r >= 1 and (restart is None or r == restart)
    assert (h["sof"]["rows"], h["sof"]["cols"], len(h["sof"]["components"])) == (img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3)
    ref = pillow_file(img, r)
    ours, theirs = jpegref.scan_bytes(data), jpegref.scan_bytes(ref)
    if ours != theirs:  # where?
        a, b = jpegref.split_segments(ours), jpegref.split_segments(theirs)
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        pytest.fail(f"scan differs from Pillow's: {len(ours)} vs {len(theirs)} bytes, {len(a)} vs {len(b)} segments, first differing segment {first}")
    dec = np.asarray(Image.open(io.BytesIO(data)))
    assert dec.shape == img.shape and np.array_equal(dec, np.asarray(Image.open(io.BytesIO(ref))))
    return ours


def noise(rows, cols, nc, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols) if nc == 1 else (rows, cols, 3), dtype=np.uint8)


def half_white(rows, cols, nc):
    a = np.zeros((rows, cols) if nc == 1 else (rows, cols, 3), np.uint8)
    a[:, : cols // 2 + 3] = 255  # the edge falls inside a block
    return a


# (rows, cols, restart interval; 0 = the library's default)
SHAPES = [(1, 1, 1), (8, 8, 1), (37, 53, 5), (64, 64, 1), (24, 200, 3), (24, 200, 8), (129, 250, 0)]


@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("rows,cols,r", SHAPES)
def test_scan_equals_pillow(ctx, rows, cols, r, nc):
    img = noise(rows, cols, nc, rows + cols)
    data = ctx.jpeg_encode(img, r)
    check_against_pillow(data, img, r or None)
    if (rows, cols, r) == (64, 64, 1):  # 64 segments: the RST0..7 cycle wraps
        segs = jpegref.split_segments(jpegref.scan_bytes(data))
        assert len(segs) == 64 and [n for _, n in segs[:9]] == [0, 1, 2, 3, 4, 5, 6, 7, 0]


@pytest.mark.parametrize("nc", [1, 3])
def test_all_zero_raster_is_eob_only_blocks(ctx, nc):
    img = np.zeros((40, 72) if nc == 1 else (40, 72, 3), np.uint8)
    check_against_pillow(ctx.jpeg_encode(img, 3), img, 3)


@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("kind", ["half_white", "noise"])
def test_stuffed_bytes(ctx, kind, nc):
    img = half_white(64, 96, nc) if kind == "half_white" else noise(64, 96, nc, 7)
    scan = check_against_pillow(ctx.jpeg_encode(img, 4), img, 4)
    assert b"\xff\x00" in scan


@pytest.mark.parametrize("nc", [1, 3])
def test_pitched_input_host_and_device_entries_agree(ctx, nc):
    import torch
    rows, cols, r = 37, 53, 5
    wide = noise(rows, cols + 11, nc, 3)
    img = wide[:, :cols]                      # a view: pitch_bytes > cols * components
    assert img.strides[0] > cols * nc
    data = ctx.jpeg_encode(img, r)
    check_against_pillow(data, np.ascontiguousarray(img), r)
    d_in = torch.from_numpy(wide).cuda()
    cap = sarpro_amd.jpeg_bound(cols, rows, nc, r)
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    n = ctx.dev_jpeg_encode(d_in.data_ptr(), cols, rows, wide.strides[0], nc, d_out.data_ptr(), cap, r)
    assert n == len(data) and d_out[:n].cpu().numpy().tobytes() == data


@pytest.mark.parametrize("nc", [1, 3])
def test_buffer_too_small_reports_the_size_and_writes_nothing_past_the_capacity(ctx, nc):
    import torch
    rows, cols, r = 64, 96, 4
    img = noise(rows, cols, nc, 9)
    full = ctx.jpeg_encode(img, r)
    d_in = torch.from_numpy(img).cuda()
    cap = len(full) // 2
    d_out = torch.full((len(full) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(sarpro_amd.SarproHipError) as ei:
        ctx.dev_jpeg_encode(d_in.data_ptr(), cols, rows, cols * nc, nc, d_out.data_ptr(), cap, r)
    assert ei.value.code == _lib.ERR_BUFFER_TOO_SMALL and ei.value.needed == len(full)
    got = d_out.cpu().numpy()
    assert (got[cap:] == 0xA5).all()
    assert got[:cap].tobytes() == full[:cap]
    n = ctx.dev_jpeg_encode(d_in.data_ptr(), cols, rows, cols * nc, nc, d_out.data_ptr(), ei.value.needed, r)  # the retry
    got = d_out.cpu().numpy()
    assert n == len(full) and got[:n].tobytes() == full and (got[n:] == 0xA5).all()
    # the host entry: the same status and size, the caller's buffer untouched past its capacity
    import ctypes as C
    buf = np.full(len(full), 0xA5, np.uint8)
    need = C.c_size_t(0)
    rc = _lib.lib.sarpro_hip_jpeg_encode(ctx._h, img.ctypes.data_as(C.c_void_p), cols, rows, cols * nc, nc, r, buf.ctypes.data_as(C.c_void_p), cap, C.byref(need))
    assert rc == _lib.ERR_BUFFER_TOO_SMALL and need.value == len(full) and (buf[cap:] == 0xA5).all()


def test_invalid_arguments_are_refused(ctx):
    import ctypes as C
    img = noise(8, 8, 3)
    buf = np.empty(4096, np.uint8)
    n = C.c_size_t(0)
    p, o = img.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)
    for cols, rows, pitch, nc, r in [(0, 8, 24, 3, 1), (8, 0, 24, 3, 1), (65536, 8, 65536 * 3, 3, 1), (8, 8, 24, 2, 1), (8, 8, 23, 3, 1), (8, 8, 24, 3, 65536)]:
        assert _lib.lib.sarpro_hip_jpeg_encode(ctx._h, p, cols, rows, pitch, nc, r, o, buf.size, C.byref(n)) == _lib.ERR_INVALID_ARG


@pytest.fixture(scope="module")
def scene_u16():
    rows, cols = 384, 520
    return synth.scene_u16(rows, cols, 0), synth.scene_u16(rows, cols, 1)


def test_pipeline_raster_1024(ctx):
    """a 1024 x 1024 RGB raster the resized dual-pol flow produces from synthetic scenes"""
    b1, b2 = synth.scene_u16(1100, 1300, 0), synth.scene_u16(1100, 1300, 1)
    rgb, _ = ctx.dualpol_synrgb_resized(b1, b2, St.Robust, 1024, True)
    assert rgb.shape == (1024, 1024, 3)
    check_against_pillow(ctx.jpeg_encode(rgb), rgb)
    gray = np.ascontiguousarray(rgb[..., 1])
    check_against_pillow(ctx.jpeg_encode(gray, 16), gray, 16)


def meta_tuple(m):
    return (m.final_cols, m.final_rows, m.scale_x, m.scale_y, m.pad_left, m.pad_top)


@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("strategy", [St.Robust, St.Clahe])
def test_u16_jpeg_flow_is_the_existing_flow_then_the_encoder(ctx, scene_u16, strategy, pad):
    b1, b2 = scene_u16
    rgb, m = ctx.dualpol_synrgb_resized(b1, b2, strategy, 128, pad)
    data, mj = ctx.dualpol_synrgb_resized_jpeg(b1, b2, strategy, 128, pad)
    assert meta_tuple(mj) == meta_tuple(m)
    check_against_pillow(data, rgb)
    data3, _ = ctx.dualpol_synrgb_resized_jpeg(b1, b2, strategy, 128, pad, restart_mcus=3)
    check_against_pillow(data3, rgb, 3)


@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("strategy", [St.Robust, St.Tamed])
def test_f32_jpeg_flow_is_the_existing_flow_then_the_encoder(ctx, strategy, pad):
    b1, b2 = f32data.resampled_scene(300, 410, 0), f32data.resampled_scene(300, 410, 1)
    rgb, m = ctx.dualpol_synrgb_resized_f32(b1, b2, strategy, 128, pad)
    data, mj = ctx.dualpol_synrgb_resized_f32_jpeg(b1, b2, strategy, 128, pad)
    assert meta_tuple(mj) == meta_tuple(m)
    check_against_pillow(data, rgb)


def test_kernel_times_carry_the_encoder(scene_u16):
    with sarpro_amd.Context(0, timing=True) as c:
        c.jpeg_encode(noise(64, 96, 3), 4)
        names = [n for n, _ in c.last_kernel_times() if not n.startswith("host:")]
        assert names == ["jpeg_transform", "jpeg_entropy_size", "jpeg_scan", "jpeg_entropy_write"]
        c.dualpol_synrgb_resized_jpeg(scene_u16[0], scene_u16[1], St.Robust, 128, True)
        names = [n for n, _ in c.last_kernel_times() if not n.startswith("host:")]
        assert "resize_h" in names and names[-4:] == ["jpeg_transform", "jpeg_entropy_size", "jpeg_scan", "jpeg_entropy_write"]
