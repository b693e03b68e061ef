"""Lanczos downsample on read on the device: k_read_lanczos_u16 against the restatement (tests/readlanczosref.py) by f32
BIT PATTERN, the signed lobes of isolated targets, the vector and element load paths, the argument rules, and -- on a context of this
module's own with the READ_LANCZOS attribute on -- the four read flows against each other, against dualpol_synrgb_resized_f32 on the
restatement's bands and against the oracle chain.  A default context keeps refusing."""
import ctypes as C
import functools
import io

import numpy as np
import pytest

import oracle
import readlanczosref as L
import sarpro_amd as S
from sarpro_amd import AutoscaleStrategy as St, SarproHipError, _lib, synth

pytestmark = pytest.mark.gpu

# (cols, rows, target_size): fractional ratio, 19 taps | integer ratio 2 | two strips, several row bands | wide and tall, 23 taps |
# ratio 1.5 | identity | ratio 5, both edges clipped | one destination row | an explicit request beyond the rule, 28 taps
SHAPES = [(37, 23, 12), (64, 48, 32), (1013, 509, 300), (4099, 41, 1100), (41, 4099, 1100), (30, 20, 20), (30, 20, 64), (5, 7, 2), (500, 3, 126),
          (64, 48, 14)]
BIG = (1013, 509, 300)
SMALL_FLOWS = [s for s in SHAPES if s != BIG]
TARGETS = "targets"  # the band argument that selects the isolated-targets pair


@functools.lru_cache(maxsize=None)
def scene(cols, rows, band=0, kind="scene"):
    if kind == TARGETS:  # isolated 65535 targets on zeros (a different lattice per band)
        a = np.zeros((rows, cols), np.uint16)
        a[3 + band::7, 2 + band::5] = 65535
    else:
        a = synth.scene_u16(rows, cols, band)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(cols, rows, ts, band=0, kind="scene"):
    """the restatement's f32 band, computed once per shape and shared (read-only)"""
    oc, orows, _ = S.read_output_dims(cols, rows, ts)
    out = L.lanczos_u16(scene(cols, rows, band, kind), orows, oc)
    out.setflags(write=False)
    return out


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def lctx():
    """a context with the READ_LANCZOS attribute on: the flows take the rule's (or the caller's) Lanczos there"""
    c = S.Context(0)
    c.set_attr("READ_LANCZOS", 1)
    yield c
    c.close()


@pytest.mark.parametrize("cols,rows,ts", SHAPES)
def test_kernel_equals_the_restatement_bit_for_bit(ctx, cols, rows, ts):
    oc, orows, _ = S.read_output_dims(cols, rows, ts)
    ref = reference(cols, rows, ts)
    assert ref.shape == (orows, oc)
    got = ctx.read_lanczos(scene(cols, rows), orows, oc)
    assert bits_equal(got, ref), (int((got.view(np.uint32) != ref.view(np.uint32)).sum()), float(np.abs(got - ref).max()))
    if ts >= max(cols, rows):
        assert bits_equal(got, scene(cols, rows).astype(np.float32))  # ratio 1: the cast


@pytest.mark.parametrize("cols,rows,ts", [(64, 48, 32), (37, 23, 12), BIG])
def test_isolated_targets_give_negative_lobes(ctx, cols, rows, ts):
    oc, orows, _ = S.read_output_dims(cols, rows, ts)
    ref = reference(cols, rows, ts, 0, TARGETS)
    assert float(ref.min()) < 0.0 and float(ref.max()) > 0.0  # no clamp in the definition
    got = ctx.read_lanczos(scene(cols, rows, 0, TARGETS), orows, oc)
    assert bits_equal(got, ref), int((got.view(np.uint32) != ref.view(np.uint32)).sum())


def _dev_lanczos(c, v, in_pitch, byte_offset, orows, oc):
    """the band in device memory with the given pitch (the padding holds 0xFFFF) at a base `byte_offset` past an aligned allocation;
    the f32 raster with a pitch of its own whose padding must come back untouched"""
    import torch
    rows, cols = v.shape
    host = np.full((rows, in_pitch), 0xFFFF, np.uint16)
    host[:, :cols] = v
    raw = np.concatenate([np.zeros(byte_offset, np.uint8), host.reshape(-1).view(np.uint8), np.zeros(16, np.uint8)])
    d_in = torch.from_numpy(raw).cuda()
    assert d_in.data_ptr() % 16 == 0
    out_pitch = oc + 3
    d_out = torch.full((orows, out_pitch), -7.0, dtype=torch.float32, device="cuda")
    c.dev_read_lanczos(d_in.data_ptr() + byte_offset, rows, cols, in_pitch, orows, oc, d_out.data_ptr(), out_pitch)
    out = d_out.cpu().numpy()
    assert np.all(out[:, oc:] == -7.0)
    return np.ascontiguousarray(out[:, :oc])


@pytest.mark.parametrize("cols,rows,ts,odd_pitch", [(37, 23, 12, 333), (64, 48, 14, 333)])
def test_element_load_path_and_dev_form(ctx, cols, rows, ts, odd_pitch):
    """A pitch that is no multiple of 8 elements (333) and a base 2 bytes past alignment take the element loads, each alone and
    together; an aligned pitch and base take the 16-byte loads: all four equal the restatement and the host-pointer form."""
    oc, orows, _ = S.read_output_dims(cols, rows, ts)
    ref = reference(cols, rows, ts)
    v = scene(cols, rows)
    assert odd_pitch % 8 and odd_pitch >= cols
    even_pitch = (cols + 7) // 8 * 8 + 8
    for pitch, off in ((odd_pitch, 2), (odd_pitch, 0), (even_pitch, 2), (even_pitch, 0)):
        assert bits_equal(_dev_lanczos(ctx, v, pitch, off, orows, oc), ref), (pitch, off)
    assert bits_equal(ctx.read_lanczos(v, orows, oc), ref)


def test_kernel_time_is_reported_and_arguments_are_checked():
    import torch
    v = scene(64, 48)
    with S.Context(0, timing=True) as c:
        assert bits_equal(c.read_lanczos(v, 24, 32), reference(64, 48, 32))
        assert "read_lanczos" in [n for n, _ in c.last_kernel_times()]
        d = torch.zeros(64 * 48, dtype=torch.int16, device="cuda")
        o = torch.full((64 * 48,), -7.0, dtype=torch.float32, device="cuda")
        for bad in ((49, 32), (24, 65), (0, 32)):  # out_rows > rows, out_cols > cols, an empty raster
            with pytest.raises(SarproHipError) as ei:
                c.dev_read_lanczos(d.data_ptr(), 48, 64, 64, bad[0], bad[1], o.data_ptr(), 64)
            assert ei.value.code == _lib.ERR_INVALID_ARG
        with pytest.raises(SarproHipError) as ei:
            c.dev_read_lanczos(d.data_ptr(), 48, 64, 63, 24, 32, o.data_ptr(), 64)  # pitch < cols
        assert ei.value.code == _lib.ERR_INVALID_ARG
        # a ratio of 8 on both axes: refused with the ratio in the message, nothing written, by the device and the host form
        with pytest.raises(SarproHipError) as ei:
            c.dev_read_lanczos(d.data_ptr(), 48, 64, 64, 6, 8, o.data_ptr(), 8)
        assert ei.value.code == _lib.ERR_UNSUPPORTED and "8.0000" in str(ei.value)
        torch.cuda.synchronize()
        assert bool(torch.all(o == -7.0))
        out = np.full((6, 8), -7.0, np.float32)
        rc = _lib.lib.sarpro_hip_read_lanczos_u16(c._h, v.ctypes.data_as(C.c_void_p), 48, 64, 6, 8, out.ctypes.data_as(C.c_void_p))
        assert rc == _lib.ERR_UNSUPPORTED and np.all(out == -7.0)
        with pytest.raises(SarproHipError) as ei:
            c.read_lanczos(v, 24, 12)  # one axis beyond (64 / 12 = 5.33)
        assert ei.value.code == _lib.ERR_UNSUPPORTED and "5.3333" in str(ei.value)
        assert bits_equal(c.read_lanczos(v, 24, 32), reference(64, 48, 32))  # the context stays usable


# ---------------------------------------------------------------------------- the flows
def _flow_oracle(b1, b2, strategy, target, pad, plain=False):
    """save.rs:317-351 (Tamed re-autoscale) or api/mod.rs:404-437 (plain), then resize -> pad per band and the composition on the final
    rasters, step by step through the oracle (the chain tests/test_gpu_read.py checks the Average flows with)."""
    us = []
    for k, b in enumerate((b1, b2)):
        if not plain and strategy == St.Tamed:
            u = oracle.tamed_synrgb_u8(b, k == 0)
        else:
            rc, u = oracle.pipeline(b, 0, int(strategy))
            assert rc == 0
        u, _ = oracle.resize_image_data_with_meta(u, target, pad)
        us.append(u)
    return oracle.synrgb(0, int(strategy), us[0], us[1])


def _alg_for(cols, rows, ts):
    """the rule's own choice where it is Lanczos, the explicit request where the rule would average"""
    return _lib.READ_DEFAULT if S.read_output_dims(cols, rows, ts)[2] == _lib.READ_LANCZOS else _lib.READ_LANCZOS


def _check_flow(lctx, cols, rows, ts, strategy, pad, kind="scene"):
    f1, f2 = reference(cols, rows, ts, 0, kind), reference(cols, rows, ts, 1, kind)
    ref = _flow_oracle(f1, f2, strategy, ts, pad)
    rgb, m = lctx.dualpol_synrgb_read(scene(cols, rows, 0, kind), scene(cols, rows, 1, kind), strategy, ts, pad, alg=_alg_for(cols, rows, ts))
    assert rgb.shape == ref.shape and np.array_equal(rgb, ref), (strategy, pad, int((rgb != ref).sum()))
    via_f32, m2 = lctx.dualpol_synrgb_resized_f32(f1, f2, strategy, ts, pad)
    assert np.array_equal(rgb, via_f32)
    assert (m.final_cols, m.final_rows, m.pad_left, m.pad_top) == (m2.final_cols, m2.final_rows, m2.pad_left, m2.pad_top)
    return rgb


@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("strategy", [St.Standard, St.Robust])
@pytest.mark.parametrize("cols,rows,ts", SMALL_FLOWS)
def test_flow_equals_the_oracle_chain_at_small_shapes(lctx, cols, rows, ts, strategy, pad):
    _check_flow(lctx, cols, rows, ts, strategy, pad)


@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("strategy", [St.Standard, St.Robust, St.Clahe, St.Tamed])
def test_flow_equals_the_oracle_chain_with_several_tiles(lctx, strategy, pad):
    _check_flow(lctx, *BIG, strategy, pad)


@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("cols,rows,ts,strategy", [(64, 48, 32, St.Standard), (64, 48, 32, St.Robust), BIG + (St.Clahe,), BIG + (St.Tamed,)])
def test_flow_on_the_isolated_targets_pair(lctx, cols, rows, ts, strategy, pad):
    assert float(reference(cols, rows, ts, 1, TARGETS).min()) < 0.0
    _check_flow(lctx, cols, rows, ts, strategy, pad, TARGETS)


def _tiff_pair(tmp_path, cols, rows, kind):
    readers = []
    for k in (0, 1):
        p = str(tmp_path / f"band{k}.tif")
        w = S.TiffWriter(p, cols, rows, 1, 16)
        w.write_rows(0, scene(cols, rows, k, kind))
        w.finish()
        readers.append(S.TiffReader(p))
    return S.TiffPair(*readers)


@pytest.mark.parametrize("cols,rows,ts,strategy,kind", [(37, 23, 12, St.Standard, "scene"), (64, 48, 14, St.Robust, "scene"), BIG + (St.Robust, "scene"),
                                                        BIG + (St.Clahe, TARGETS)])
def test_host_dev_stream_and_jpeg_flows_agree(lctx, tmp_path, cols, rows, ts, strategy, kind):
    import torch
    from PIL import Image
    alg = _alg_for(cols, rows, ts)
    want = _check_flow(lctx, cols, rows, ts, strategy, True, kind)
    # device-resident bands
    pitch = (cols + 63) // 64 * 64
    d = []
    for k in (0, 1):
        t = torch.zeros((rows, pitch), dtype=torch.int16, device="cuda")
        t[:, :cols] = torch.from_numpy(scene(cols, rows, k, kind).view(np.int16).copy()).cuda()
        d.append(t)
    out = torch.zeros(want.size, dtype=torch.uint8, device="cuda")
    m = lctx.dev_dualpol_synrgb_read(d[0].data_ptr(), d[1].data_ptr(), rows, cols, pitch, strategy, ts, True, out.data_ptr(), alg=alg)
    assert (m.final_rows, m.final_cols) == want.shape[:2]
    assert np.array_equal(out.cpu().numpy().reshape(want.shape), want)
    # the row reader, up to the raster and up to the file
    pair = _tiff_pair(tmp_path, cols, rows, kind)
    rgb, m = lctx.dualpol_synrgb_read_stream(pair.reader(), rows, cols, strategy, ts, True, alg=alg)
    assert np.array_equal(rgb, want)
    data, _ = lctx.dualpol_synrgb_read_stream_jpeg(pair.reader(), rows, cols, strategy, ts, True, alg=alg)
    existing = lctx.jpeg_encode(want)
    assert data == existing
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), np.asarray(Image.open(io.BytesIO(existing)).convert("RGB")))


def test_timing_names_the_filter_of_the_flow():
    cols, rows, ts = 64, 48, 32
    with S.Context(0, timing=True) as c:
        c.set_attr("READ_LANCZOS", 1)
        c.dualpol_synrgb_read(scene(cols, rows, 0), scene(cols, rows, 1), St.Standard, ts, True)
        names = [n for n, _ in c.last_kernel_times()]
        assert "read_lanczos" in names and "read_average" not in names
        c.dualpol_synrgb_read(scene(cols, rows, 0), scene(cols, rows, 1), St.Standard, 8, True)  # reduction 8: the rule averages
        names = [n for n, _ in c.last_kernel_times()]
        assert "read_average" in names and "read_lanczos" not in names


def test_switch_off_keeps_the_refusal_and_ratios_beyond_five_are_refused_when_on(ctx, lctx):
    cols, rows, ts = 64, 48, 32
    b1, b2 = scene(cols, rows, 0), scene(cols, rows, 1)
    assert ctx.get_attr("READ_LANCZOS") is None
    for alg in (_lib.READ_DEFAULT, _lib.READ_LANCZOS):
        with pytest.raises(SarproHipError) as ei:
            ctx.dualpol_synrgb_read(b1, b2, St.Standard, ts, True, alg=alg)
        assert ei.value.code == _lib.ERR_UNSUPPORTED and "not built" in str(ei.value)
    with S.Context(0) as c:  # the attribute set to 0 is the same as unset
        c.set_attr("READ_LANCZOS", 0)
        with pytest.raises(SarproHipError) as ei:
            c.dualpol_synrgb_read(b1, b2, St.Standard, ts, True)
        assert ei.value.code == _lib.ERR_UNSUPPORTED and "not built" in str(ei.value)
    # on: an explicit request at 64 -> 8 names the ratio and writes nothing; AVERAGE is unchanged
    rgb = np.full((8, 8, 3), 0x5A, np.uint8)
    m = _lib.ResizeMeta()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib.lib.sarpro_hip_dualpol_synrgb_read_u16(lctx._h, vp(b1), vp(b2), rows, cols, _lib.READ_LANCZOS, int(St.Standard), 0, 0, 8, 1, vp(rgb), C.byref(m))
    assert rc == _lib.ERR_UNSUPPORTED and "8.0000" in _lib.lib.sarpro_hip_last_error(lctx._h).decode() and np.all(rgb == 0x5A)
    a_on, _ = lctx.dualpol_synrgb_read(b1, b2, St.Standard, ts, True, alg=_lib.READ_AVERAGE)
    a_off, _ = ctx.dualpol_synrgb_read(b1, b2, St.Standard, ts, True, alg=_lib.READ_AVERAGE)
    assert np.array_equal(a_on, a_off)
