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


@pytest.mark.parametrize("r", [1, 5, 65535])
@pytest.mark.parametrize("nc", [1, 3])
def test_crafted_raster_reaches_every_symbol_class(ctx, nc, r):
    """jpegref.crafted_raster: all 160 (run, size) symbols of each table, one, two and three ZRLs in front of a coefficient, blocks with
    and without EOB, every DC class, a segment whose padded last byte is a stuffed FF -- asserted on the raster, then encoded with every
    block its own segment (1), with a ragged last segment (5) and as ONE segment (65535: the bit and byte carry of the block loop runs
    through more than 1600 blocks)"""
    img = jpegref.crafted_raster(nc)
    assert img.shape[0] * img.shape[1] // 64 > 1600 and (img.shape[0] * img.shape[1] // 64) % 5
    jpegref.assert_full_coverage(jpegref.symbol_coverage(img, r), r)
    scan = check_against_pillow(ctx.jpeg_encode(img, r), img, r)
    assert jpegref.segments_ending_stuffed(scan) >= 1


@pytest.mark.parametrize("nc", [1, 3])
def test_crafted_raster_cropped_off_the_block_grid(ctx, nc):
    """3 rows and 5 columns less: the last block row and column are completed by replication next to the long-run blocks"""
    img = np.ascontiguousarray(jpegref.crafted_raster(nc)[:-3, :-5])
    assert img.shape[0] % 8 == 5 and img.shape[1] % 8 == 3
    for c in jpegref.symbol_coverage(img, 5).values():
        n16, n32, n48 = c["runs"]
        assert n16 - n32 >= 1 and n32 - n48 >= 1 and n48 >= 1 and c["no_eob"] >= 1 and c["eob"] >= 1
    check_against_pillow(ctx.jpeg_encode(img, 5), img, 5)


def sparse(rows, cols, seed=0):
    """gray 128 with 0.2 % of the samples random: segments of different lengths, quick in Pillow at tens of megapixels"""
    rng = np.random.default_rng(seed)
    a = np.full((rows, cols), 128, np.uint8)
    k = rng.integers(0, a.size, a.size // 500)
    a.flat[k] = rng.integers(0, 256, k.size, dtype=np.uint8)
    return a


SCAN_CHUNK = 2048   # kJpegScanChunk: segments per workgroup of the offset scan; its partial sums are scanned 256 at a time


def check_sparse(ctx, rows, cols, segments):
    """gray, interval 1: one segment per block.  The scan, the decoded pixels and the file's length (what the offset scan returns as
    its total) against Pillow"""
    img = sparse(rows, cols, rows + cols)
    assert ((rows + 7) // 8) * ((cols + 7) // 8) == segments
    data = ctx.jpeg_encode(img, 1)
    scan = check_against_pillow(data, img, 1)
    assert len(data) == len(sarpro_amd.host_jpeg_header(cols, rows, 1, 1)) + len(jpegref.scan_bytes(pillow_file(img, 1))) + 2
    assert len({len(s) for s, _ in jpegref.split_segments(scan[: 1 << 16])}) > 1   # the lengths do differ
    return data


# (rows, cols, segments, chunks): one more than a chunk, exactly two, one more than two, exactly 256, 257 (a second round of the loop
# over the partial sums)
SCAN_SHAPES = [(8, 16392, 2049, 2), (64, 4096, 4096, 2), (136, 1928, 4097, 3), (4096, 8192, 524288, 256), (4104, 8192, 525312, 257)]


@pytest.mark.parametrize("rows,cols,segments,chunks", SCAN_SHAPES)
def test_offset_scan_over_several_chunks(ctx, rows, cols, segments, chunks):
    assert -(-segments // SCAN_CHUNK) == chunks
    check_sparse(ctx, rows, cols, segments)


def test_offset_scan_over_several_chunks_rgb_default_interval(ctx):
    img = noise(1032, 1024, 3, 5)
    data = ctx.jpeg_encode(img)
    r = jpegref.parse_header(data)["dri"]
    assert (129 * 128 + r - 1) // r > SCAN_CHUNK   # 2064 segments at the interval of 8
    check_against_pillow(data, img)


def test_one_context_sizes_out_of_order():
    """257 chunks, one segment, 2 chunks, one segment on a context of its own: the workspace grows once and is then larger than the
    image needs, with the lengths, partial sums and offsets of the image before still in it"""
    small = noise(8, 8, 1, 3)
    with sarpro_amd.Context(0) as c:
        for rows, cols, segments in [(4104, 8192, 525312), (8, 8, 1), (8, 16392, 2049), (8, 8, 1)]:
            if segments == 1:
                check_against_pillow(c.jpeg_encode(small, 1), small, 1)
            else:
                check_sparse(c, rows, cols, segments)


def test_capacity_edges_on_the_device_entry(ctx):
    """the crafted gray raster at interval 5 through the device entry with capacities that cut the EOI, a stuffed FF 00 pair, an RST
    marker and the header, and the size query (capacity 0, no buffer): ERR_BUFFER_TOO_SMALL with the exact size, the file's prefix
    below the capacity, nothing written at or past it; then the retry at the reported size"""
    import re

    import torch
    img, r = jpegref.crafted_raster(1), 5
    rows, cols = img.shape
    full = ctx.jpeg_encode(img, r)
    check_against_pillow(full, img, r)
    start = jpegref.parse_header(full)["scan_start"]
    stuffed = full.index(b"\xff\x00", start) + 1          # in a scan FF 00 is a data FF and its stuffed 00
    rst = re.search(rb"\xff[\xd0-\xd7]", full[start:]).start() + start + 1
    assert full[stuffed - 1:stuffed + 1] == b"\xff\x00" and full[rst - 1] == 0xFF and 0xD0 <= full[rst] <= 0xD7
    d_in = torch.from_numpy(np.array(img)).cuda()
    for cap in [len(full) - 1, stuffed, rst, start // 2, 0]:
        d_out = torch.full((len(full) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        with pytest.raises(sarpro_amd.SarproHipError) as ei:
            ctx.dev_jpeg_encode(d_in.data_ptr(), cols, rows, cols, 1, d_out.data_ptr() if cap else 0, cap, r)
        assert ei.value.code == _lib.ERR_BUFFER_TOO_SMALL and ei.value.needed == len(full), cap
        got = d_out.cpu().numpy()
        assert got[:cap].tobytes() == full[:cap] and (got[cap:] == 0xA5).all(), cap
        n = ctx.dev_jpeg_encode(d_in.data_ptr(), cols, rows, cols, 1, d_out.data_ptr(), ei.value.needed, r)
        got = d_out.cpu().numpy()
        assert n == len(full) and got[:n].tobytes() == full and (got[n:] == 0xA5).all(), cap


def test_width_past_libjpegs_limit(ctx):
    """8 x 65535 gray, the widest raster the library takes.  libjpeg refuses dimensions over 65500 ("Maximum supported image dimension
    is 65500 pixels"), so Pillow can neither write nor read this one: the whole file is compared with the restatement
    (jpegref.encode_file, itself held against Pillow in test_jpeg_host.py), not with Pillow."""
    img = noise(8, 65535, 1, 6)
    data = ctx.jpeg_encode(img)
    h = jpegref.parse_header(data)
    assert (h["sof"]["rows"], h["sof"]["cols"]) == (8, 65535) and data[:h["scan_start"]] == sarpro_amd.host_jpeg_header(65535, 8, 1)
    assert data == jpegref.encode_file(img, h["dri"])


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
