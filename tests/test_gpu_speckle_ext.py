"""Frost and Refined Lee on the device (the definitions are this project's own): k_speckle_frost_u16 / k_speckle_rlee_u16
against the restatement (tests/speckleextref.py) by f32 BIT PATTERN at the smallest shapes that reach every structural case, the vector
and element load paths, the _ext flows "two u16 bands in, filtered, RGB out" against the oracle chain on the restatement's bands, Lee and
Kuan through the _ext calls against the calls they had already, and the argument rules.  tests/test_speckle_ext_host.py asserts that the
scene used here reaches every case of Refined Lee (each half-window, ties, fallbacks)."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import sarpro_amd as S
import speckleextref as X
from sarpro_amd import AutoscaleStrategy as St, SarproHipError, SpeckleFilter as F, _lib

pytestmark = pytest.mark.gpu

LOOKS, DAMPING = 4.4, 2.0
# (filter, window): what the restatement is asked for beside looks and damping
FILTERS = [(F.Frost, 3), (F.Frost, 5), (F.Frost, 7), (F.RefinedLee, 7)]
# (rows, cols): smaller than every window | smaller than some | odd, one tile | four strips, the last ragged (245 columns) | 94 row
# bands of 16 rows, the last ragged | three strips x 19 row bands
SHAPES = [(1, 1), (2, 5), (5, 2), (23, 37), (41, 1013), (1500, 41), (300, 600)]
TALL = (33000, 41)  # row bands of 32 rows: longer than a 28-row LDS stage, so a tile takes two stages with the second in flight


@functools.lru_cache(maxsize=None)
def scene(rows, cols, band=0):
    return X.scene(rows, cols, band)


@functools.lru_cache(maxsize=None)
def reference(rows, cols, filt, k, looks, damping, band=0):
    """the restatement's raster, computed once per case and shared (read-only)"""
    out = X.speckle_ext_u16(scene(rows, cols, band), int(filt), k, looks, damping)
    out.setflags(write=False)
    return out


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ndiff(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).sum()), float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64))))


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("filt,k", FILTERS)
def test_kernel_equals_the_restatement_bit_for_bit(ctx, filt, k, rows, cols):
    got = ctx.speckle_ext(scene(rows, cols), filt, k, LOOKS, DAMPING)
    ref = reference(rows, cols, filt, k, LOOKS, DAMPING)
    assert bits_equal(got, ref), ndiff(got, ref)


@pytest.mark.parametrize("damping", [1e-3, 50.0, 1e300])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_frost_at_small_large_and_overflowing_damping(ctx, k, damping):
    """1e-3: next to the boxcar mean; 50: most weights tiny; 1e300: a overflows to +inf, every weight but the centre's is 0"""
    for rows, cols in ((23, 37), (300, 600)):
        got = ctx.speckle_ext(scene(rows, cols), F.Frost, k, LOOKS, damping)
        ref = reference(rows, cols, F.Frost, k, LOOKS, damping)
        assert bits_equal(got, ref), (rows, cols, ndiff(got, ref))
        assert np.all(np.isfinite(got))


@pytest.mark.parametrize("looks", [1e-2, 1e6])
def test_refined_lee_at_the_two_extremes_of_looks(ctx, looks):
    """1e-2: w = 0 everywhere (the mean of the half-window or of the window); 1e6: w next to 1"""
    for rows, cols in ((23, 37), (300, 600)):
        got = ctx.speckle_ext(scene(rows, cols), F.RefinedLee, 7, looks, DAMPING)
        ref = reference(rows, cols, F.RefinedLee, 7, looks, DAMPING)
        assert bits_equal(got, ref), (rows, cols, ndiff(got, ref))


@pytest.mark.parametrize("filt,k", [(F.Frost, 7), (F.RefinedLee, 7)])
def test_row_bands_longer_than_an_lds_stage(ctx, filt, k):
    rows, cols = TALL
    got = ctx.speckle_ext(scene(rows, cols), filt, k, LOOKS, DAMPING)
    ref = reference(rows, cols, filt, k, LOOKS, DAMPING)
    assert bits_equal(got, ref), ndiff(got, ref)


@pytest.mark.parametrize("filt,k", FILTERS)
def test_constant_rasters(ctx, filt, k):
    """every sample 65535: a 7 x 7 window's S2 is 49 * 65535^2, past 32 bits, and a class sum reaches 8 * 65535; all-zero input: all 0.0"""
    out = ctx.speckle_ext(np.full((48, 64), 65535, np.uint16), filt, k, LOOKS, DAMPING)
    assert out.dtype == np.float32 and np.all(out == np.float32(65535.0))
    out = ctx.speckle_ext(np.zeros((48, 64), np.uint16), filt, k, LOOKS, DAMPING)
    assert np.all(out.view(np.uint32) == 0)


def _dev_speckle_ext(c, v, in_pitch, byte_offset, filt, k):
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
    c.dev_speckle_ext_u16(d_in.data_ptr() + byte_offset, rows, cols, in_pitch, filt, k, LOOKS, DAMPING, d_out.data_ptr(), out_pitch)
    out = d_out.cpu().numpy()
    assert np.all(out[:, cols:] == -7.0)
    return np.ascontiguousarray(out[:, :cols])


@pytest.mark.parametrize("rows,cols,odd_pitch", [(23, 37, 333), (41, 1013, 1333)])
@pytest.mark.parametrize("filt,k", [(F.Frost, 7), (F.Frost, 3), (F.RefinedLee, 7)])
def test_element_load_path_and_dev_form(ctx, filt, k, rows, cols, odd_pitch):
    """A pitch that is no multiple of 8 elements and a base 2 bytes past alignment take the element loads, each alone and together; an
    aligned pitch and base take the 16-byte loads (the samples of the row's padding, 0xFFFF here, must not count): all four equal the
    host-pointer form and the restatement."""
    v = scene(rows, cols)
    ref = reference(rows, cols, filt, k, LOOKS, DAMPING)
    assert odd_pitch % 8 and odd_pitch >= cols
    even_pitch = (cols + 7) // 8 * 8 + 8
    for pitch, off in ((odd_pitch, 2), (odd_pitch, 0), (even_pitch, 2), (even_pitch, 0)):
        got = _dev_speckle_ext(ctx, v, pitch, off, filt, k)
        assert bits_equal(got, ref), (pitch, off, ndiff(got, ref))
    assert bits_equal(ctx.speckle_ext(v, filt, k, LOOKS, DAMPING), ref)


@pytest.mark.parametrize("filt", [F.Lee, F.Kuan])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_ext_with_lee_and_kuan_equals_the_calls_that_were_there(ctx, filt, k):
    for rows, cols in ((23, 37), (300, 600)):
        v = scene(rows, cols)
        want = ctx.speckle(v, filt, k, LOOKS)
        assert bits_equal(ctx.speckle_ext(v, filt, k, LOOKS, DAMPING), want)
        assert bits_equal(ctx.speckle_ext(v, filt, k, LOOKS, float("nan")), want)  # damping is ignored
        assert bits_equal(want, X.speckle_ext_u16(v, int(filt), k, LOOKS, DAMPING))


# ---------------------------------------------------------------------------- the flows
def _flow_oracle(b1, b2, strategy, target, pad, plain):
    """save.rs:317-351 (Tamed re-autoscale) or api/mod.rs:404-437 (plain), then resize -> pad per band and the composition on the final
    rasters, step by step through the oracle (as tests/test_gpu_speckle.py checks its flows)."""
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
# strategy, plain pipeline, and the filter of the case: one filter each
FLOW_CASES = [(St.Clahe, False, (F.Frost, 7)), (St.Robust, False, (F.RefinedLee, 7)), (St.Tamed, False, (F.Frost, 5)), (St.Tamed, True, (F.RefinedLee, 7))]


@pytest.mark.parametrize("strategy,plain,fk", FLOW_CASES)
def test_flow_equals_the_oracle_chain_on_the_restatements_bands(ctx, strategy, plain, fk):
    rows, cols, ts = FLOW
    f1, f2 = (reference(rows, cols, *fk, LOOKS, DAMPING, band=b) for b in (0, 1))
    ref = _flow_oracle(f1, f2, strategy, ts, True, plain)
    rgb, m = ctx.dualpol_synrgb_speckle_ext(scene(rows, cols, 0), scene(rows, cols, 1), *fk, LOOKS, DAMPING, strategy, ts, True, plain_pipeline=plain)
    assert rgb.shape == ref.shape and np.array_equal(rgb, ref), (strategy, plain, int((rgb != ref).sum()))
    via_f32, m2 = ctx.dualpol_synrgb_resized_f32(f1, f2, strategy, ts, True, plain_pipeline=plain)
    assert np.array_equal(rgb, via_f32)
    assert (m.final_cols, m.final_rows, m.pad_left, m.pad_top) == (m2.final_cols, m2.final_rows, m2.pad_left, m2.pad_top)


@pytest.mark.parametrize("strategy,plain,fk", FLOW_CASES)
def test_flow_at_native_size(ctx, strategy, plain, fk):
    rows, cols = NATIVE
    assert S.host_clahe_shape_ok(rows, cols)
    f1, f2 = (reference(rows, cols, *fk, LOOKS, DAMPING, band=b) for b in (0, 1))
    ref = _flow_oracle(f1, f2, strategy, None, False, plain)
    rgb, m = ctx.dualpol_synrgb_speckle_ext(scene(rows, cols, 0), scene(rows, cols, 1), *fk, LOOKS, DAMPING, strategy, None, False, plain_pipeline=plain)
    assert rgb.shape == (rows, cols, 3) and (m.final_rows, m.final_cols) == (rows, cols)
    assert np.array_equal(rgb, ref), (strategy, plain, int((rgb != ref).sum()))
    via_f32, _ = ctx.dualpol_synrgb_resized_f32(f1, f2, strategy, None, False, plain_pipeline=plain)
    assert np.array_equal(rgb, via_f32)


@pytest.mark.parametrize("ts,pad", [(128, True), (None, False)])
@pytest.mark.parametrize("fk", [(F.Frost, 7), (F.RefinedLee, 7)])
def test_flow_with_device_bands_equals_the_host_flow(ctx, fk, ts, pad):
    import torch
    rows, cols = FLOW[:2] if ts else NATIVE
    pitch = (cols + 63) // 64 * 64 + 64
    d = []
    for k in (0, 1):
        t = torch.zeros((rows, pitch), dtype=torch.int16, device="cuda")
        t[:, :cols] = torch.from_numpy(scene(rows, cols, k).view(np.int16).copy()).cuda()
        d.append(t)
    want, _ = ctx.dualpol_synrgb_speckle_ext(scene(rows, cols, 0), scene(rows, cols, 1), *fk, LOOKS, DAMPING, St.Clahe, ts, pad)
    out = torch.zeros(want.size, dtype=torch.uint8, device="cuda")
    m = ctx.dev_dualpol_synrgb_speckle_ext(d[0].data_ptr(), d[1].data_ptr(), rows, cols, pitch, *fk, LOOKS, DAMPING, St.Clahe, ts, pad, out.data_ptr())
    assert (m.final_rows, m.final_cols) == want.shape[:2]
    assert np.array_equal(out.cpu().numpy().reshape(want.shape), want)


def test_ext_flow_with_lee_equals_the_flow_that_was_there(ctx):
    rows, cols = NATIVE
    b1, b2 = scene(rows, cols, 0), scene(rows, cols, 1)
    want, _ = ctx.dualpol_synrgb_speckle(b1, b2, F.Lee, 5, LOOKS, St.Clahe, None, False)
    got, _ = ctx.dualpol_synrgb_speckle_ext(b1, b2, F.Lee, 5, LOOKS, DAMPING, St.Clahe, None, False)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------- arguments and timing
NAN, INF = float("nan"), float("inf")
# (filter, window, looks, damping) the _ext calls refuse
BAD = [(4, 7, 4.4, 2.0), (-1, 7, 4.4, 2.0), (99, 3, 4.4, 2.0),                                                     # a filter outside 0..3
       (0, 4, 4.4, 2.0), (1, 9, 4.4, 2.0), (0, 5, 0.0, 2.0), (1, 5, NAN, 2.0),                                     # what the old calls reject
       (2, 4, 4.4, 2.0), (2, 9, 4.4, 2.0), (2, 1, 4.4, 2.0), (2, 0, 4.4, 2.0),                                     # Frost: the window
       (2, 7, 4.4, 0.0), (2, 7, 4.4, -1.0), (2, 7, 4.4, NAN), (2, 7, 4.4, INF), (2, 7, 4.4, -INF),                 # Frost: the damping
       (3, 3, 4.4, 2.0), (3, 5, 4.4, 2.0), (3, 9, 4.4, 2.0),                                                       # Refined Lee: the window
       (3, 7, 0.0, 2.0), (3, 7, -1.0, 2.0), (3, 7, NAN, 2.0), (3, 7, INF, 2.0)]                                    # Refined Lee: the looks
# ... and what they accept although one parameter is nonsense: the one the filter ignores
IGNORED = [(2, 7, NAN, 2.0), (2, 5, -1.0, 2.0), (3, 7, 4.4, NAN), (3, 7, 4.4, -1.0)]


def test_invalid_arguments_write_nothing_and_leave_the_context_usable(ctx):
    import torch
    rows, cols = 23, 37
    v = scene(rows, cols)
    lib, h = _lib.lib, ctx._h
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    d16 = torch.from_numpy(v.view(np.int16).copy()).cuda()
    o = torch.full((rows, cols + 3), -7.0, dtype=torch.float32, device="cuda")
    rgb = np.full((128, 128, 3), 0x5A, np.uint8)
    d_rgb = torch.full((128 * 128 * 3,), 0x5A, dtype=torch.uint8, device="cuda")
    m = _lib.ResizeMeta()
    torch.cuda.synchronize()
    for filt, k, looks, damping in BAD:
        out = np.full((rows, cols), -7.0, np.float32)
        assert lib.sarpro_hip_speckle_ext_u16(h, vp(v), rows, cols, filt, k, looks, damping, vp(out)) == _lib.ERR_INVALID_ARG, (filt, k, looks, damping)
        assert lib.sarpro_hip_last_error(h) and np.all(out == -7.0)
        rc = lib.sarpro_hip_speckle_ext_u16_dev(h, d16.data_ptr(), rows, cols, cols, filt, k, looks, damping, o.data_ptr(), cols + 3)
        assert rc == _lib.ERR_INVALID_ARG, (filt, k, looks, damping)
        rc = lib.sarpro_hip_dualpol_synrgb_speckle_ext_u16(h, vp(v), vp(v), rows, cols, filt, k, looks, damping, int(St.Clahe), 0, 0, 128, 1, vp(rgb), C.byref(m))
        assert rc == _lib.ERR_INVALID_ARG and np.all(rgb == 0x5A), (filt, k, looks, damping)
        rc = lib.sarpro_hip_dualpol_synrgb_speckle_ext_u16_dev(h, d16.data_ptr(), d16.data_ptr(), rows, cols, cols, filt, k, looks, damping, int(St.Clahe),
                                                               0, 0, 128, 1, d_rgb.data_ptr(), C.byref(m))
        assert rc == _lib.ERR_INVALID_ARG, (filt, k, looks, damping)
    out = np.full((rows, cols), -7.0, np.float32)
    for filt, k in FILTERS:
        assert lib.sarpro_hip_speckle_ext_u16(h, vp(v), 0, cols, int(filt), k, LOOKS, DAMPING, vp(out)) == _lib.ERR_INVALID_ARG  # an empty raster
        assert lib.sarpro_hip_speckle_ext_u16(h, vp(v), rows, 0, int(filt), k, LOOKS, DAMPING, vp(out)) == _lib.ERR_INVALID_ARG
        assert lib.sarpro_hip_speckle_ext_u16(h, None, rows, cols, int(filt), k, LOOKS, DAMPING, vp(out)) == _lib.ERR_INVALID_ARG  # null pointers
        assert lib.sarpro_hip_speckle_ext_u16(h, vp(v), rows, cols, int(filt), k, LOOKS, DAMPING, None) == _lib.ERR_INVALID_ARG
        for call in (lambda: ctx.dev_speckle_ext_u16(d16.data_ptr(), rows, cols, cols - 1, filt, k, LOOKS, DAMPING, o.data_ptr(), cols + 3),  # pitch < cols
                     lambda: ctx.dev_speckle_ext_u16(d16.data_ptr(), rows, cols, cols, filt, k, LOOKS, DAMPING, o.data_ptr(), cols - 1),
                     lambda: ctx.dev_speckle_ext_u16(0, rows, cols, cols, filt, k, LOOKS, DAMPING, o.data_ptr(), cols + 3),                   # null pointers
                     lambda: ctx.dev_speckle_ext_u16(d16.data_ptr(), rows, cols, cols, filt, k, LOOKS, DAMPING, 0, cols + 3)):
            with pytest.raises(SarproHipError) as ei:
                call()
            assert ei.value.code == _lib.ERR_INVALID_ARG
        rc = lib.sarpro_hip_dualpol_synrgb_speckle_ext_u16(h, vp(v), vp(v), rows, cols, int(filt), k, LOOKS, DAMPING, 99, 0, 0, 128, 1, vp(rgb), C.byref(m))
        assert rc == _lib.ERR_INVALID_ARG and np.all(rgb == 0x5A)  # a bad strategy
    assert np.all(out == -7.0) and np.all(o.cpu().numpy() == -7.0) and np.all(d_rgb.cpu().numpy() == 0x5A)
    for filt, k, looks, damping in IGNORED:
        assert bits_equal(ctx.speckle_ext(v, filt, k, looks, damping), reference(rows, cols, filt, k, LOOKS, DAMPING)), (filt, k, looks, damping)


def test_the_old_entry_points_still_refuse_frost_and_refined_lee(ctx):
    rows, cols = 23, 37
    v = scene(rows, cols)
    vf = v.astype(np.float32)
    lib, h = _lib.lib, ctx._h
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rgb = np.full((128, 128, 3), 0x5A, np.uint8)
    m = _lib.ResizeMeta()
    for filt in (2, 3):
        for fn, src in ((lib.sarpro_hip_speckle_u16, v), (lib.sarpro_hip_speckle_f32, vf)):
            out = np.full((rows, cols), -7.0, np.float32)
            assert fn(h, vp(src), rows, cols, filt, 7, LOOKS, vp(out)) == _lib.ERR_INVALID_ARG and np.all(out == -7.0)
        rc = lib.sarpro_hip_dualpol_synrgb_speckle_u16(h, vp(v), vp(v), rows, cols, filt, 7, LOOKS, int(St.Clahe), 0, 0, 128, 1, vp(rgb), C.byref(m))
        assert rc == _lib.ERR_INVALID_ARG and np.all(rgb == 0x5A)
        with pytest.raises(SarproHipError):
            ctx.speckle(v, filt, 7, LOOKS)
    assert bits_equal(ctx.speckle_ext(v, F.Frost, 7, LOOKS, DAMPING), reference(rows, cols, F.Frost, 7, LOOKS, DAMPING))


def test_kernel_times_are_reported():
    v = scene(23, 37)
    with S.Context(0, timing=True) as c:
        assert bits_equal(c.speckle_ext(v, F.Frost, 3, LOOKS, DAMPING), reference(23, 37, F.Frost, 3, LOOKS, DAMPING))
        names = [n for n, _ in c.last_kernel_times()]
        assert "speckle_frost_u16" in names and "speckle_u16" not in names
        c.speckle_ext(v, F.RefinedLee, 7, LOOKS, DAMPING)
        names = [n for n, _ in c.last_kernel_times()]
        assert "speckle_rlee_u16" in names and "speckle_u16" not in names
        c.speckle_ext(v, F.Kuan, 7, LOOKS, DAMPING)
        assert "speckle_u16" in [n for n, _ in c.last_kernel_times()]
        c.dualpol_synrgb_speckle_ext(v, v, F.Frost, 5, LOOKS, DAMPING, St.Robust, 16, True)
        assert "speckle_frost_u16" in [n for n, _ in c.last_kernel_times()]
        c.dualpol_synrgb_speckle_ext(v, v, F.RefinedLee, 7, LOOKS, DAMPING, St.Robust, 16, True)
        assert "speckle_rlee_u16" in [n for n, _ in c.last_kernel_times()]
