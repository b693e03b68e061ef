"""Speckle filters on the device (the definition is this project's own): k_speckle_u16 / k_speckle_f32 against the
restatement (tests/speckleref.py) by f32 BIT PATTERN at the smallest shapes that reach every structural case, the vector and element
load paths, the flows "two u16 bands in, filtered, RGB out" against the oracle chain on the restatement's bands, and the argument rules."""
import ctypes as C
import functools

import numpy as np
import pytest

import f32data
import oracle
import sarpro_amd as S
import speckleref as R
from sarpro_amd import AutoscaleStrategy as St, SarproHipError, SpeckleFilter as F, _lib, synth

pytestmark = pytest.mark.gpu

PAIRS = [(f, k) for f in (F.Lee, F.Kuan) for k in (3, 5, 7)]
# (rows, cols): smaller than every window | smaller than some | odd, one tile | four strips, the last ragged (245 columns) | 94 row
# bands of 16 rows, the last ragged | three strips x 19 row bands
SHAPES = [(1, 1), (2, 5), (5, 2), (23, 37), (41, 1013), (1500, 41), (300, 600)]
# bands taller than a 28 / 30-row LDS stage (the host picks 32 and 68 rows here): 2 and 3 stages per tile, the next one in flight
TALL = [(33000, 41), (70001, 41)]


@functools.lru_cache(maxsize=None)
def scene(rows, cols, band=0):
    """a synthetic band with a black-fill border on two sides, ~5 % scattered zeros, one fully zero 9 x 9 block (invalid centres) and a
    second one around a single valid sample (a valid pixel whose only valid neighbour is itself)"""
    a = synth.scene_u16(rows, cols, band).copy()
    rng = np.random.default_rng(1000 * band + rows + cols)
    a[rng.random(a.shape) < 0.05] = 0
    a[: min(3, rows - 1), :] = 0
    a[:, : min(4, cols - 1)] = 0
    r0, c0 = rows // 3, cols // 3
    a[r0:r0 + 9, c0:c0 + 9] = 0
    r1, c1 = rows // 2 + 3, cols // 2 + 1
    a[r1:r1 + 9, c1:c1 + 9] = 0
    if r1 + 4 < rows and c1 + 4 < cols:
        a[r1 + 4, c1 + 4] = 4321
    a[rows - 1, cols - 1] = 65535
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(rows, cols, filt, k, looks, band=0):
    """the restatement's raster, computed once per case and shared (read-only)"""
    out = R.speckle_u16(scene(rows, cols, band), int(filt), k, looks)
    out.setflags(write=False)
    return out


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ndiff(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).sum()), float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64))))


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("filt,k", PAIRS)
def test_kernel_equals_the_restatement_bit_for_bit(ctx, filt, k, rows, cols):
    got = ctx.speckle(scene(rows, cols), filt, k, 4.4)
    ref = reference(rows, cols, filt, k, 4.4)
    assert bits_equal(got, ref), ndiff(got, ref)


@pytest.mark.parametrize("looks", [1.0, 1e-2, 1e6])
@pytest.mark.parametrize("filt,k", PAIRS)
def test_looks_one_and_the_two_extremes(ctx, filt, k, looks):
    """1e-2: w = 0 everywhere (the boxcar mean); 1e6: w next to 1"""
    for rows, cols in ((23, 37), (300, 600)):
        got = ctx.speckle(scene(rows, cols), filt, k, looks)
        ref = reference(rows, cols, filt, k, looks)
        assert bits_equal(got, ref), (rows, cols, ndiff(got, ref))


@pytest.mark.parametrize("rows,cols", TALL)
@pytest.mark.parametrize("filt,k", [(F.Lee, 3), (F.Kuan, 5), (F.Lee, 7)])
def test_row_bands_taller_than_an_lds_stage(ctx, filt, k, rows, cols):
    got = ctx.speckle(scene(rows, cols), filt, k, 4.4)
    ref = reference(rows, cols, filt, k, 4.4)
    assert bits_equal(got, ref), ndiff(got, ref)


@pytest.mark.parametrize("filt", [F.Lee, F.Kuan])
def test_constant_rasters(ctx, filt):
    """every sample 65535: a 7 x 7 window's S2 is 49 * 65535^2, past 32 bits; all-zero input: all 0.0"""
    out = ctx.speckle(np.full((48, 64), 65535, np.uint16), filt, 7, 4.4)
    assert out.dtype == np.float32 and np.all(out == np.float32(65535.0))
    out = ctx.speckle(np.zeros((48, 64), np.uint16), filt, 7, 4.4)
    assert np.all(out.view(np.uint32) == 0)


def _dev_speckle(c, v, in_pitch, byte_offset, filt, k, looks):
    """the band in device memory with the given pitch (the padding holds 0xFFFF) at a base `byte_offset` past an aligned allocation;
    the f32 raster with a pitch of its own whose padding must come back untouched"""
    import torch
    rows, cols = v.shape
    host = np.full((rows, in_pitch), 0xFFFF, np.uint16)
    host[:, :cols] = v
    raw = np.concatenate([np.zeros(byte_offset, np.uint8), host.reshape(-1).view(np.uint8), np.zeros(16, np.uint8)])
    d_in = torch.from_numpy(raw).cuda()
    assert d_in.data_ptr() % 16 == 0
    out_pitch = cols + 3
    d_out = torch.full((rows, out_pitch), -7.0, dtype=torch.float32, device="cuda")
    c.dev_speckle_u16(d_in.data_ptr() + byte_offset, rows, cols, in_pitch, filt, k, looks, d_out.data_ptr(), out_pitch)
    out = d_out.cpu().numpy()
    assert np.all(out[:, cols:] == -7.0)
    return np.ascontiguousarray(out[:, :cols])


@pytest.mark.parametrize("rows,cols,odd_pitch", [(23, 37, 333), (41, 1013, 1333)])
def test_element_load_path_and_dev_form(ctx, rows, cols, odd_pitch):
    """A pitch that is no multiple of 8 elements and a base 2 bytes past alignment take the element loads, each alone and together; an
    aligned pitch and base take the 16-byte loads (the samples of the row's padding, 0xFFFF here, must not count): all four equal the
    host-pointer form and the restatement."""
    v = scene(rows, cols)
    ref = reference(rows, cols, F.Kuan, 7, 4.4)
    assert odd_pitch % 8 and odd_pitch >= cols
    even_pitch = (cols + 7) // 8 * 8 + 8
    for pitch, off in ((odd_pitch, 2), (odd_pitch, 0), (even_pitch, 2), (even_pitch, 0)):
        got = _dev_speckle(ctx, v, pitch, off, F.Kuan, 7, 4.4)
        assert bits_equal(got, ref), (pitch, off, ndiff(got, ref))
    assert bits_equal(ctx.speckle(v, F.Kuan, 7, 4.4), ref)


# ---------------------------------------------------------------------------- the f32 flavour
@functools.lru_cache(maxsize=None)
def scene_f32(rows, cols, kind):
    x = (f32data.resampled_scene(rows, cols) * np.float32(1e-3) if kind == "scaled" else f32data.nasty_scene(rows, cols)).copy()
    flat = x.ravel()
    flat[1::19] = np.nan
    flat[2::23] = np.inf
    flat[3::29] = 0.0
    flat[4::31] *= -1.0
    flat[6::37] = np.float32(1e-5)  # just below the threshold: invalid
    flat[8::41] = R.THR             # equal to it: valid
    flat[10::43] = -np.inf
    r0, c0 = rows // 3, cols // 3
    x[r0:r0 + 9, c0:c0 + 9] = np.nan
    x[r0 + 4, c0 + 4] = 0.5
    x.view(np.uint32)[0, 0] = 0x7FC12345  # a NaN with a payload: an invalid centre keeps its bit pattern
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("rows,cols", [(23, 37), (300, 600)])
@pytest.mark.parametrize("kind", ["scaled", "nasty"])
@pytest.mark.parametrize("filt,k", PAIRS)
def test_f32_kernel_equals_the_restatement_bit_for_bit(ctx, filt, k, kind, rows, cols):
    v = scene_f32(rows, cols, kind)
    assert np.float32(S.host_f32_valid_threshold()).view(np.uint32) == R.THR.view(np.uint32)
    ref = R.speckle_f32(v, int(filt), k, 4.4)
    got = ctx.speckle(v, filt, k, 4.4)
    assert bits_equal(got, ref), ndiff(got, ref)
    with np.errstate(invalid="ignore"):
        invalid = ~((v >= R.THR) & (v < np.inf))
    assert invalid.sum() > 20 and np.array_equal(got.view(np.uint32)[invalid], v.view(np.uint32)[invalid])


def test_f32_device_form_with_pitches(ctx):
    import torch
    v = scene_f32(23, 37, "scaled")
    ref = R.speckle_f32(v, R.LEE, 5, 1.0)
    d_in = torch.full((23, 41), float("nan"), dtype=torch.float32, device="cuda")
    d_in[:, :37] = torch.from_numpy(v.copy()).cuda()
    d_out = torch.full((23, 40), -7.0, dtype=torch.float32, device="cuda")
    ctx.dev_speckle_f32(d_in.data_ptr(), 23, 37, 41, F.Lee, 5, 1.0, d_out.data_ptr(), 40)
    out = d_out.cpu().numpy()
    assert np.all(out[:, 37:] == -7.0) and bits_equal(np.ascontiguousarray(out[:, :37]), ref)


# ---------------------------------------------------------------------------- the flows
def _flow_oracle(b1, b2, strategy, target, pad, plain):
    """save.rs:317-351 (Tamed re-autoscale) or api/mod.rs:404-437 (plain), then resize -> pad per band and the composition on the final
    rasters, step by step through the oracle (as tests/test_gpu_read.py checks its flows)."""
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


FLOW = (900, 1200, 128)   # rows, cols, target_size
NATIVE = (120, 160)
FLOW_FILTER = (F.Lee, 5, 4.4)
STRATEGIES = [(St.Clahe, False), (St.Robust, False), (St.Tamed, False), (St.Tamed, True)]


@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("strategy,plain", STRATEGIES)
def test_flow_equals_the_oracle_chain_on_the_restatements_bands(ctx, strategy, plain, pad):
    rows, cols, ts = FLOW
    f1, f2 = (reference(rows, cols, *FLOW_FILTER, band=b) for b in (0, 1))
    ref = _flow_oracle(f1, f2, strategy, ts, pad, plain)
    rgb, m = ctx.dualpol_synrgb_speckle(scene(rows, cols, 0), scene(rows, cols, 1), *FLOW_FILTER, strategy, ts, pad, plain_pipeline=plain)
    assert rgb.shape == ref.shape and np.array_equal(rgb, ref), (strategy, plain, pad, int((rgb != ref).sum()))
    via_f32, m2 = ctx.dualpol_synrgb_resized_f32(f1, f2, strategy, ts, pad, plain_pipeline=plain)
    assert np.array_equal(rgb, via_f32)
    assert (m.final_cols, m.final_rows, m.pad_left, m.pad_top) == (m2.final_cols, m2.final_rows, m2.pad_left, m2.pad_top)


@pytest.mark.parametrize("strategy,plain", STRATEGIES)
def test_flow_at_native_size(ctx, strategy, plain):
    rows, cols = NATIVE
    assert S.host_clahe_shape_ok(rows, cols)
    f1, f2 = (reference(rows, cols, F.Kuan, 7, 1.0, band=b) for b in (0, 1))
    ref = _flow_oracle(f1, f2, strategy, None, False, plain)
    rgb, m = ctx.dualpol_synrgb_speckle(scene(rows, cols, 0), scene(rows, cols, 1), F.Kuan, 7, 1.0, strategy, None, False, plain_pipeline=plain)
    assert rgb.shape == (rows, cols, 3) and (m.final_rows, m.final_cols) == (rows, cols)
    assert np.array_equal(rgb, ref), (strategy, plain, int((rgb != ref).sum()))
    via_f32, _ = ctx.dualpol_synrgb_resized_f32(f1, f2, strategy, None, False, plain_pipeline=plain)
    assert np.array_equal(rgb, via_f32)


@pytest.mark.parametrize("ts,pad", [(128, True), (None, False)])
def test_flow_with_device_bands_equals_the_host_flow(ctx, ts, pad):
    import torch
    rows, cols = FLOW[:2] if ts else NATIVE
    pitch = (cols + 63) // 64 * 64 + 64
    d = []
    for k in (0, 1):
        t = torch.zeros((rows, pitch), dtype=torch.int16, device="cuda")
        t[:, :cols] = torch.from_numpy(scene(rows, cols, k).view(np.int16).copy()).cuda()
        d.append(t)
    want, _ = ctx.dualpol_synrgb_speckle(scene(rows, cols, 0), scene(rows, cols, 1), *FLOW_FILTER, St.Clahe, ts, pad)
    out = torch.zeros(want.size, dtype=torch.uint8, device="cuda")
    m = ctx.dev_dualpol_synrgb_speckle(d[0].data_ptr(), d[1].data_ptr(), rows, cols, pitch, *FLOW_FILTER, St.Clahe, ts, pad, out.data_ptr())
    assert (m.final_rows, m.final_cols) == want.shape[:2]
    assert np.array_equal(out.cpu().numpy().reshape(want.shape), want)


# ---------------------------------------------------------------------------- arguments and timing
def test_invalid_arguments_write_nothing_and_leave_the_context_usable(ctx):
    import torch
    rows, cols = 23, 37
    v = scene(rows, cols)
    vf = v.astype(np.float32)
    lib, h = _lib.lib, ctx._h
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    bad = [(2, 5, 4.4), (-1, 5, 4.4), (0, 4, 4.4), (0, 9, 4.4), (0, 1, 4.4), (0, 5, 0.0), (0, 5, -1.0), (0, 5, float("nan")), (0, 5, float("inf"))]
    for filt, k, looks in bad:
        for fn, src in ((lib.sarpro_hip_speckle_u16, v), (lib.sarpro_hip_speckle_f32, vf)):
            out = np.full((rows, cols), -7.0, np.float32)
            assert fn(h, vp(src), rows, cols, filt, k, looks, vp(out)) == _lib.ERR_INVALID_ARG, (filt, k, looks)
            assert _lib.lib.sarpro_hip_last_error(h) and np.all(out == -7.0)
    out = np.full((rows, cols), -7.0, np.float32)
    assert lib.sarpro_hip_speckle_u16(h, vp(v), 0, cols, 0, 5, 4.4, vp(out)) == _lib.ERR_INVALID_ARG  # an empty raster
    assert lib.sarpro_hip_speckle_u16(h, vp(v), rows, 0, 0, 5, 4.4, vp(out)) == _lib.ERR_INVALID_ARG
    assert lib.sarpro_hip_speckle_u16(h, None, rows, cols, 0, 5, 4.4, vp(out)) == _lib.ERR_INVALID_ARG  # null pointers
    assert lib.sarpro_hip_speckle_f32(h, vp(vf), rows, cols, 0, 5, 4.4, None) == _lib.ERR_INVALID_ARG
    assert np.all(out == -7.0)
    d16 = torch.from_numpy(v.view(np.int16).copy()).cuda()
    d32 = torch.from_numpy(vf.copy()).cuda()
    o = torch.full((rows, cols + 3), -7.0, dtype=torch.float32, device="cuda")
    for call in (lambda: ctx.dev_speckle_u16(d16.data_ptr(), rows, cols, cols - 1, F.Lee, 5, 4.4, o.data_ptr(), cols + 3),   # pitch < cols
                 lambda: ctx.dev_speckle_u16(d16.data_ptr(), rows, cols, cols, F.Lee, 5, 4.4, o.data_ptr(), cols - 1),
                 lambda: ctx.dev_speckle_f32(d32.data_ptr(), rows, cols, cols - 1, F.Lee, 5, 4.4, o.data_ptr(), cols + 3),
                 lambda: ctx.dev_speckle_u16(0, rows, cols, cols, F.Lee, 5, 4.4, o.data_ptr(), cols + 3),                       # null pointers
                 lambda: ctx.dev_speckle_f32(d32.data_ptr(), rows, cols, cols, F.Lee, 5, 4.4, 0, cols + 3),
                 lambda: ctx.dev_speckle_u16(d16.data_ptr(), rows, cols, cols, F.Lee, 6, 4.4, o.data_ptr(), cols + 3),          # a bad window
                 lambda: ctx.dev_speckle_f32(d32.data_ptr(), rows, cols, cols, F.Lee, 5, 4.4, d32.data_ptr(), cols),            # aliasing: in place
                 lambda: ctx.dev_speckle_f32(d32.data_ptr(), rows, cols, cols, F.Lee, 5, 4.4, d32.data_ptr() + 4 * cols * 3, cols)):  # ... overlapping
        with pytest.raises(SarproHipError) as ei:
            call()
        assert ei.value.code == _lib.ERR_INVALID_ARG
    assert np.all(o.cpu().numpy() == -7.0) and np.array_equal(d32.cpu().numpy(), vf)
    rgb = np.full((128, 128, 3), 0x5A, np.uint8)
    m = _lib.ResizeMeta()
    for filt, k, looks, strategy in ((2, 5, 4.4, int(St.Clahe)), (0, 8, 4.4, int(St.Clahe)), (0, 5, 0.0, int(St.Clahe)), (0, 5, 4.4, 99)):
        rc = lib.sarpro_hip_dualpol_synrgb_speckle_u16(h, vp(v), vp(v), rows, cols, filt, k, looks, strategy, 0, 0, 128, 1, vp(rgb), C.byref(m))
        assert rc == _lib.ERR_INVALID_ARG and np.all(rgb == 0x5A)
    assert bits_equal(ctx.speckle(v, F.Lee, 5, 4.4), reference(rows, cols, F.Lee, 5, 4.4))


def test_kernel_times_are_reported():
    v = scene(23, 37)
    with S.Context(0, timing=True) as c:
        assert bits_equal(c.speckle(v, F.Lee, 3, 4.4), reference(23, 37, F.Lee, 3, 4.4))
        assert "speckle_u16" in [n for n, _ in c.last_kernel_times()]
        c.speckle(v.astype(np.float32), F.Lee, 3, 4.4)
        assert "speckle_f32" in [n for n, _ in c.last_kernel_times()]
        c.dualpol_synrgb_speckle(v, v, F.Lee, 3, 4.4, St.Robust, 16, True)
        assert "speckle_u16" in [n for n, _ in c.last_kernel_times()]
