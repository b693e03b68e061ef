"""Downsample on read on the device (io/sentinel1.rs:1074-1108 -> io/gdal.rs:145-177, ResampleAlg::Average): k_read_average_u16
against the restatement (tests/readref.py) by f32 BIT PATTERN, the vector and element load paths, the flows "two u16 bands in,
quicklook RGB / JPEG out" against the oracle chain on the restatement's bands, and the Lanczos refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import readref
import sarpro_amd as S
from sarpro_amd import AutoscaleStrategy as St, SarproHipError, _lib, synth

pytestmark = pytest.mark.gpu

# (cols, rows, target_size): fractional on both axes | integer ratio | primes, slivers of weight | several strips, rows wider than one
# wave load | many destination rows | 125-wide windows | one destination row | ratio 1.5, two-sample windows | ratio 1, the plain cast
SHAPES = [(37, 23, 8), (64, 48, 16), (1013, 509, 200), (4099, 41, 512), (41, 4099, 512), (2000, 1500, 16), (500, 3, 64), (30, 20, 20), (30, 20, 64)]
EXPLICIT_AVERAGE = [(30, 20, 20), (30, 20, 64)]  # the rule picks Lanczos there: the flows take them with SARPRO_READ_AVERAGE


@functools.lru_cache(maxsize=None)
def scene(cols, rows, band=0):
    a = synth.scene_u16(rows, cols, band)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(cols, rows, ts, band=0):
    """the restatement's f32 band, computed once per shape and shared (read-only)"""
    oc, orows, _ = readref.output_dims(cols, rows, ts)
    out = readref.average_u16(scene(cols, rows, band), orows, oc)
    out.setflags(write=False)
    return out


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("cols,rows,ts", SHAPES)
def test_kernel_equals_the_restatement_bit_for_bit(ctx, cols, rows, ts):
    oc, orows, _ = S.read_output_dims(cols, rows, ts)
    ref = reference(cols, rows, ts)
    assert ref.shape == (orows, oc)
    got = ctx.read_average(scene(cols, rows), orows, oc)
    assert bits_equal(got, ref), (int((got.view(np.uint32) != ref.view(np.uint32)).sum()), float(np.abs(got - ref).max()))


def test_interior_sum_past_32_bits_and_one_destination_sample(ctx):
    """70000 x 8 -> 1 x 1, all samples 65535: the interior sum of one row is 69998 * 65535 > 2^32, the window is 23 LDS slabs wide."""
    v = np.full((8, 70000), 65535, np.uint16)
    assert S.read_output_dims(70000, 8, 1)[:2] == (1, 1)
    ref = readref.average_u16(v, 1, 1)
    got = ctx.read_average(v, 1, 1)
    assert bits_equal(got, ref) and float(got[0, 0]) == 65535.0


def _dev_average(c, v, in_pitch, byte_offset, orows, oc):
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
    c.dev_read_average(d_in.data_ptr() + byte_offset, rows, cols, in_pitch, orows, oc, d_out.data_ptr(), out_pitch)
    out = d_out.cpu().numpy()
    assert np.all(out[:, oc:] == -7.0)
    return np.ascontiguousarray(out[:, :oc])


@pytest.mark.parametrize("cols,rows,ts,odd_pitch", [(37, 23, 8, 333), (4099, 41, 512, 4333)])
def test_element_load_path_and_dev_form(ctx, cols, rows, ts, odd_pitch):
    """A pitch that is no multiple of 8 elements (333; 4333 for the raster wider than 333) and a base 2 bytes past alignment take the
    element loads, each alone and together; an aligned pitch and base take the 16-byte loads: all four equal the host-pointer form."""
    oc, orows, _ = S.read_output_dims(cols, rows, ts)
    ref = reference(cols, rows, ts)
    v = scene(cols, rows)
    assert odd_pitch % 8 and odd_pitch >= cols
    even_pitch = (cols + 7) // 8 * 8 + 8
    for pitch, off in ((odd_pitch, 2), (odd_pitch, 0), (even_pitch, 2), (even_pitch, 0)):
        assert bits_equal(_dev_average(ctx, v, pitch, off, orows, oc), ref), (pitch, off)
    assert bits_equal(ctx.read_average(v, orows, oc), ref)


def test_kernel_time_is_reported_and_arguments_are_checked():
    import torch
    v = scene(64, 48)
    with S.Context(0, timing=True) as c:
        assert bits_equal(c.read_average(v, 12, 16), reference(64, 48, 16))
        assert "read_average" in [n for n, _ in c.last_kernel_times()]
        d = torch.zeros(64 * 48, dtype=torch.int16, device="cuda")
        o = torch.zeros(64 * 48, dtype=torch.float32, device="cuda")
        for bad in ((49, 16), (12, 65), (0, 16)):  # out_rows > rows, out_cols > cols, an empty raster
            with pytest.raises(SarproHipError) as ei:
                c.dev_read_average(d.data_ptr(), 48, 64, 64, bad[0], bad[1], o.data_ptr(), 64)
            assert ei.value.code == _lib.ERR_INVALID_ARG
        with pytest.raises(SarproHipError):
            c.dev_read_average(d.data_ptr(), 48, 64, 63, 12, 16, o.data_ptr(), 64)  # pitch < cols


# ---------------------------------------------------------------------------- the flows
def _flow_oracle(b1, b2, strategy, target, pad, plain):
    """save.rs:317-351 (Tamed re-autoscale) or api/mod.rs:404-437 (plain), then resize -> pad per band and the composition on the final
    rasters, step by step through the oracle (the chain tests/test_gpu_f32.py checks the resized f32 flow with)."""
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


FLOW = (1200, 900, 128)  # -> 128 x 96, clear of the CLAHE underflow shapes


@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("strategy,plain", [(s, False) for s in St] + [(St.Tamed, True)])
def test_flow_equals_the_oracle_chain_on_the_restatements_bands(ctx, strategy, plain, pad):
    cols, rows, ts = FLOW
    assert len(list(St)) == 7
    f1, f2 = reference(cols, rows, ts, 0), reference(cols, rows, ts, 1)
    assert f1.shape == (96, 128)
    ref = _flow_oracle(f1, f2, strategy, ts, pad, plain)
    rgb, m = ctx.dualpol_synrgb_read(scene(cols, rows, 0), scene(cols, rows, 1), strategy, ts, pad, plain_pipeline=plain)
    assert rgb.shape == ref.shape and np.array_equal(rgb, ref), (strategy, plain, pad, int((rgb != ref).sum()))
    via_f32, m2 = ctx.dualpol_synrgb_resized_f32(f1, f2, strategy, ts, pad, plain_pipeline=plain)
    assert np.array_equal(rgb, via_f32)
    assert (m.final_cols, m.final_rows, m.pad_left, m.pad_top) == (m2.final_cols, m2.final_rows, m2.pad_left, m2.pad_top)


def test_flow_with_device_bands(ctx):
    import torch
    cols, rows, ts = FLOW
    pitch = 1216
    d = []
    for k in (0, 1):
        t = torch.zeros((rows, pitch), dtype=torch.int16, device="cuda")
        t[:, :cols] = torch.from_numpy(scene(cols, rows, k).view(np.int16).copy()).cuda()
        d.append(t)
    want, _ = ctx.dualpol_synrgb_read(scene(cols, rows, 0), scene(cols, rows, 1), St.Clahe, ts, True)
    out = torch.zeros(want.size, dtype=torch.uint8, device="cuda")
    m = ctx.dev_dualpol_synrgb_read(d[0].data_ptr(), d[1].data_ptr(), rows, cols, pitch, St.Clahe, ts, True, out.data_ptr())
    assert (m.final_rows, m.final_cols) == want.shape[:2]
    assert np.array_equal(out.cpu().numpy().reshape(want.shape), want)


@pytest.mark.parametrize("cols,rows,ts", EXPLICIT_AVERAGE)
def test_explicit_average_is_honoured_below_a_reduction_of_four(ctx, cols, rows, ts):
    f1, f2 = reference(cols, rows, ts, 0), reference(cols, rows, ts, 1)
    b1, b2 = scene(cols, rows, 0), scene(cols, rows, 1)
    if ts >= max(cols, rows):
        assert bits_equal(f1, b1.astype(np.float32))  # ratio 1: the cast
    with pytest.raises(SarproHipError) as ei:
        ctx.dualpol_synrgb_read(b1, b2, St.Standard, ts, True)
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    rgb, _ = ctx.dualpol_synrgb_read(b1, b2, St.Standard, ts, True, alg=_lib.READ_AVERAGE)
    want, _ = ctx.dualpol_synrgb_resized_f32(f1, f2, St.Standard, ts, True)
    assert np.array_equal(rgb, want)
    assert np.array_equal(rgb, _flow_oracle(f1, f2, St.Standard, ts, True, False))


def _tiff_pair(tmp_path, cols, rows):
    readers = []
    for k in (0, 1):
        p = str(tmp_path / f"band{k}.tif")
        w = S.TiffWriter(p, cols, rows, 1, 16)
        w.write_rows(0, scene(cols, rows, k))
        w.finish()
        readers.append(S.TiffReader(p))
    return S.TiffPair(*readers)


@pytest.mark.parametrize("cols,rows,ts", [FLOW, (1013, 509, 200)])
def test_stream_forms_from_strip_tiffs(ctx, tmp_path, cols, rows, ts):
    pair = _tiff_pair(tmp_path, cols, rows)
    want, mw = ctx.dualpol_synrgb_read(scene(cols, rows, 0), scene(cols, rows, 1), St.Robust, ts, True)
    rgb, m = ctx.dualpol_synrgb_read_stream(pair.reader(), rows, cols, St.Robust, ts, True)
    assert np.array_equal(rgb, want) and (m.final_cols, m.final_rows) == (mw.final_cols, mw.final_rows)
    data, _ = ctx.dualpol_synrgb_read_stream_jpeg(pair.reader(), rows, cols, St.Robust, ts, True)
    assert data == ctx.jpeg_encode(want)
    with pytest.raises(SarproHipError) as ei:
        ctx.dualpol_synrgb_read_stream_jpeg(pair.reader(), rows, cols, St.Robust, ts, True, capacity=1000)
    assert ei.value.code == _lib.ERR_BUFFER_TOO_SMALL and ei.value.needed == len(data)


def test_lanczos_range_is_refused_and_the_context_stays_usable(ctx):
    cols, rows, ts = 2000, 1500, 1000
    assert S.read_output_dims(cols, rows, ts) == (1000, 750, _lib.READ_LANCZOS)
    b = scene(cols, rows)
    rgb = np.full((1000, 1000, 3), 0x5A, np.uint8)
    m = _lib.ResizeMeta()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib.lib.sarpro_hip_dualpol_synrgb_read_u16(ctx._h, vp(b), vp(b), rows, cols, _lib.READ_DEFAULT, int(St.Standard), 0, 0, ts, 1, vp(rgb), C.byref(m))
    assert rc == _lib.ERR_UNSUPPORTED
    msg = _lib.lib.sarpro_hip_last_error(ctx._h).decode()
    assert "Lanczos" in msg and "2.0000" in msg
    assert np.all(rgb == 0x5A)
    rc = _lib.lib.sarpro_hip_dualpol_synrgb_read_u16(ctx._h, vp(b), vp(b), rows, cols, _lib.READ_LANCZOS, int(St.Standard), 0, 0, 100, 1, vp(rgb), C.byref(m))
    assert rc == _lib.ERR_UNSUPPORTED and np.all(rgb == 0x5A)  # requested, at a reduction the rule would average
    assert bits_equal(ctx.read_average(scene(64, 48), 12, 16), reference(64, 48, 16))
