"""Overview pyramids on the device: k_overviews against the numpy restatement (tests/overviewref.py) byte for byte at
every type, component count, flag and levels-per-launch setting; the vector and element load paths and unaligned destinations; the
host-pointer form against the device form and the library's host twin; the flow "two u16 bands in, RGB and its pyramid out" against
the oracle chain; and the file flow that ends in a tiled GeoTIFF with overviews."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import overviewref as R
import sarpro_amd as S
from sarpro_amd import AutoscaleStrategy as St, SarproHipError, _lib, synth

pytestmark = pytest.mark.gpu

# (cols, rows, min_size): one pixel out | odd sizes below a tile | exactly one tile | a tile and a sliver on both axes | several tiles,
# odd | several rows and columns of tiles | a wide strip past 2^12 columns, one row of tiles | 8 levels: a tail launch at depth 6
SHAPES = [(2, 2, 1), (3, 5, 1), (64, 64, 1), (65, 63, 1), (130, 67, 1), (1000, 300, 16), (4099, 41, 8), (200, 130, 1)]
DEPTHS = (1, 3, 6)


@functools.lru_cache(maxsize=None)
def raster(cols, rows, comps, dtype):
    a = R.wedge_raster(rows, cols, comps, dtype, cols * 7 + rows)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(cols, rows, ms, comps, dtype, skip):
    """the restatement's packed buffer (0xA5 wherever no level writes), computed once per case and shared (read-only)"""
    a = raster(cols, rows, comps, dtype)
    out = R.pack(R.overviews(a, ms, skip), cols, rows, a.dtype.itemsize * 8, ms)
    out.setflags(write=False)
    return out


class depth:
    """OVR_DEPTH on a context for the length of a block"""

    def __init__(self, c, d):
        self.c, self.d = c, d

    def __enter__(self):
        self.old = self.c.get_attr("OVR_DEPTH")
        self.c.set_attr("OVR_DEPTH", self.d)

    def __exit__(self, *exc):
        self.c.set_attr("OVR_DEPTH", self.old)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("comps", [1, 2, 3])
@pytest.mark.parametrize("skip", [False, True])
def test_kernel_equals_the_restatement_byte_for_byte(ctx, dtype, comps, skip):
    for cols, rows, ms in SHAPES:
        ref = reference(cols, rows, ms, comps, dtype, skip)
        for d in DEPTHS:
            with depth(ctx, d):
                plan, got = ctx.overviews(raster(cols, rows, comps, dtype), ms, skip)
            assert plan.total_bytes == ref.size
            assert np.array_equal(got, ref), (cols, rows, d, int((got != ref).sum()))   # the levels and the untouched 0xA5 padding


def test_launches_per_pyramid():
    """(200, 130) down to 1 x 1 is 8 levels: two launches at depth 6 (the tail launch reads level 6), three at 3, eight at 1, four at
    the default of 2; every launch is listed as `overviews`"""
    a = raster(200, 130, 3, np.uint8)
    with S.Context(0, timing=True) as c:
        assert c.get_attr("OVR_DEPTH") is None                                          # unset: 2 levels per launch
        for d, n in ((None, 4), (6, 2), (3, 3), (1, 8), (2, 4), (99, 2), (0, 8)):               # (values outside 1..6 are clamped)
            c.set_attr("OVR_DEPTH", d)
            plan, got = c.overviews(a, 1, False)
            assert plan.levels == 8 and np.array_equal(got, reference(200, 130, 1, 3, np.uint8, False))
            times = c.last_kernel_times()
            assert [n_ for n_, _ in times].count("overviews") == n and all(t >= 0 for _, t in times), (d, times)


def _dev_overviews(c, a, pitch_bytes, src_off, dst_off, ms, skip):
    """the raster in device memory with the given pitch (the padding holds 0xEE) at a base `src_off` bytes past an aligned allocation;
    the packed buffer `dst_off` bytes past one, 0xA5 everywhere before the call"""
    import torch
    rows, cols, comps = a.shape
    rb = cols * comps * a.dtype.itemsize
    host = np.full((rows, pitch_bytes), 0xEE, np.uint8)
    host[:, :rb] = a.reshape(rows, -1).view(np.uint8)
    d_in = torch.from_numpy(np.concatenate([np.zeros(src_off, np.uint8), host.reshape(-1), np.zeros(16, np.uint8)])).cuda()
    plan = S.overview_plan(cols, rows, comps, a.dtype.itemsize * 8, ms)
    d_out = torch.full((dst_off + plan.total_bytes + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    c.dev_overviews(d_in.data_ptr() + src_off, cols, rows, pitch_bytes, comps, a.dtype.itemsize * 8, plan, d_out.data_ptr() + dst_off, skip_zero=skip)
    out = d_out.cpu().numpy()
    assert np.all(out[:dst_off] == 0xA5) and np.all(out[dst_off + plan.total_bytes:] == 0xA5)
    return out[dst_off:dst_off + plan.total_bytes]


@pytest.mark.parametrize("dtype,comps", [(np.uint8, 3), (np.uint16, 1), (np.uint16, 3), (np.uint8, 1)])
@pytest.mark.parametrize("cols,rows,ms", [(130, 67, 1), (4099, 41, 8)])
def test_load_paths_and_dev_form(ctx, dtype, comps, cols, rows, ms):
    """A pitch that is no multiple of 16 bytes and a base 2 bytes past alignment take the element loads, each alone and together; an
    aligned pitch and base take the 16-byte loads; a packed buffer 2 bytes past alignment takes the narrower stores: all equal the
    restatement, and nothing outside the levels' rows is written."""
    a = raster(cols, rows, comps, dtype)
    skip = comps == 3
    ref = reference(cols, rows, ms, comps, dtype, skip)
    rb = cols * comps * a.dtype.itemsize
    odd, even = rb + 6, (rb + 15) // 16 * 16 + 16
    assert odd % 16 and even % 16 == 0
    for pitch, src_off, dst_off in ((odd, 2, 0), (odd, 0, 0), (even, 2, 0), (even, 0, 0), (even, 0, 2), (odd, 2, 2)):
        got = _dev_overviews(ctx, a, pitch, src_off, dst_off, ms, skip)
        assert np.array_equal(got, ref), (pitch, src_off, dst_off, int((got != ref).sum()))


def test_host_pointer_form_equals_the_dev_form_and_the_host_twin(ctx):
    for dtype, comps, skip in ((np.uint8, 3, True), (np.uint16, 2, False)):
        a = raster(1000, 300, comps, dtype)
        plan, got = ctx.overviews(a, 16, skip)
        rb = 1000 * comps * a.dtype.itemsize
        dev = _dev_overviews(ctx, a, (rb + 15) // 16 * 16, 0, 0, 16, skip)
        _, host = S.host_overviews(a, 16, skip)
        assert np.array_equal(got, dev) and np.array_equal(got, host) and np.array_equal(got, reference(1000, 300, 16, comps, dtype, skip))
        levels = S.overview_levels(plan, got)
        want = R.overviews(a, 16, skip)
        assert len(levels) == len(want) and all(np.array_equal(x, y) for x, y in zip(levels, want))


def test_kernel_time_is_reported_and_arguments_are_checked():
    import torch
    a = raster(64, 64, 1, np.uint8)
    with S.Context(0, timing=True) as c:
        _, got = c.overviews(a, 1, False)
        assert np.array_equal(got, reference(64, 64, 1, 1, np.uint8, False))
        assert "overviews" in [n for n, _ in c.last_kernel_times()]
        d = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
        plan = S.overview_plan(64, 64, 1, 8, 1)
        o = torch.zeros(plan.total_bytes, dtype=torch.uint8, device="cuda")
        f = _lib.lib.sarpro_hip_overviews_dev
        vp = C.c_void_p
        assert f(c._h, vp(d.data_ptr()), 64, 64, 64, 1, 8, 0, C.byref(plan), vp(o.data_ptr())) == _lib.OK
        for cols, rows, pitch, comps, bits, flags in ((0, 64, 64, 1, 8, 0), (64, 0, 64, 1, 8, 0), (64, 64, 63, 1, 8, 0), (64, 64, 64, 4, 8, 0),
                                                      (64, 64, 64, 1, 12, 0), (64, 64, 64, 1, 8, 2), (32, 64, 64, 1, 8, 0), (64, 64, 128, 1, 16, 0)):
            assert f(c._h, vp(d.data_ptr()), cols, rows, pitch, comps, bits, flags, C.byref(plan), vp(o.data_ptr())) == _lib.ERR_INVALID_ARG
        assert f(c._h, None, 64, 64, 64, 1, 8, 0, C.byref(plan), vp(o.data_ptr())) == _lib.ERR_INVALID_ARG
        assert f(c._h, vp(d.data_ptr()), 64, 64, 64, 1, 8, 0, C.byref(plan), None) == _lib.ERR_INVALID_ARG
        assert f(c._h, vp(d.data_ptr()), 64, 64, 64, 1, 8, 0, None, vp(o.data_ptr())) == _lib.ERR_INVALID_ARG
        p16 = S.overview_plan(32, 32, 1, 16, 1)
        assert f(c._h, vp(d.data_ptr() + 1), 32, 32, 64, 1, 16, 0, C.byref(p16), vp(o.data_ptr())) == _lib.ERR_INVALID_ARG   # a u16 raster at an odd address
        empty = S.overview_plan(1, 1, 1, 8, 1)
        assert f(c._h, vp(d.data_ptr()), 1, 1, 1, 1, 8, 0, C.byref(empty), None) == _lib.OK    # 0 levels: a successful no-op
        with pytest.raises(SarproHipError):
            c.overviews(a.astype(np.uint16), plan=plan)                                         # the plan of another sample type


@pytest.mark.parametrize("strategy", [St.Clahe, St.Robust])
@pytest.mark.parametrize("skip", [False, True])
def test_flow_rgb_equals_the_oracle_and_the_levels_equal_the_restatement(ctx, strategy, skip):
    rows, cols = 384, 520
    b1, b2 = synth.scene_u16(rows, cols, 0), synth.scene_u16(rows, cols, 1)
    rc, ref, _, _ = oracle.dualpol_synrgb(b1.astype(np.float32), b2.astype(np.float32), int(strategy))
    assert rc == 0
    rgb, plan, packed = ctx.dualpol_synrgb_pyramid(b1, b2, strategy, min_size=8, skip_zero=skip)
    assert np.array_equal(rgb, ref)                                                             # as smoke() checks the plain flow
    assert plan.levels == 7 and np.array_equal(packed, R.pack(R.overviews(ref, 8, skip), cols, rows, 8, 8))
    assert np.array_equal(rgb, ctx.dualpol_synrgb(b1, b2, strategy))                            # bit for bit the plain flow's RGB


@pytest.mark.parametrize("strategy", [St.Clahe, St.Robust])
def test_flow_hands_out_the_chains_statistics_behind_its_one_synchronisation(strategy):
    """The chain's read-back is completed behind the sweep: the statistics are sarpro_hip_dualpol_synrgb_u16_dev's, the kernel times list
    the chain's kernels and then `overviews`, and the next plain call on the context is unaffected."""
    import torch
    rows, cols = 384, 520
    b = [synth.scene_u16(rows, cols, k) for k in (0, 1)]
    d = [torch.from_numpy(x.view(np.int16)).cuda() for x in b]
    plan = S.overview_plan(cols, rows, 3, 8, 8)
    with S.Context(0, timing=True) as c:
        d_rgb = [torch.zeros((rows, cols, 3), dtype=torch.uint8, device="cuda") for _ in range(3)]
        d_ovr = torch.full((plan.total_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
        ref_st = c.dev_dualpol_synrgb_u16(d[0].data_ptr(), d[1].data_ptr(), rows, cols, cols, strategy, 0, d_rgb[0].data_ptr(), cols)
        st = c.dev_dualpol_synrgb_pyramid(d[0].data_ptr(), d[1].data_ptr(), rows, cols, cols, strategy, 0, d_rgb[1].data_ptr(), cols, plan, d_ovr.data_ptr())
        names = [n for n, _ in c.last_kernel_times()]
        again = c.dev_dualpol_synrgb_u16(d[0].data_ptr(), d[1].data_ptr(), rows, cols, cols, strategy, 0, d_rgb[2].data_ptr(), cols)
    assert [bytes(s_) for s_ in st] == [bytes(s_) for s_ in ref_st] == [bytes(s_) for s_ in again] and st[0].valid_count > 0   # bit for bit
    assert "overviews" in names and names.index("overviews") > 0 and not any(n.startswith("overviews") for n in names[:names.index("overviews")])
    rgb = d_rgb[1].cpu().numpy()
    assert np.array_equal(rgb, d_rgb[0].cpu().numpy()) and np.array_equal(rgb, d_rgb[2].cpu().numpy())
    assert np.array_equal(d_ovr.cpu().numpy(), R.pack(R.overviews(rgb, 8), cols, rows, 8, 8))


def test_flow_is_stream_ordered_on_an_async_context():
    """SARPRO_HIP_CTX_ASYNC_DEV: the chain and the sweep are enqueued behind each other, the rasters are complete after synchronize()"""
    rows, cols = 384, 520
    b1, b2 = synth.scene_u16(rows, cols, 0), synth.scene_u16(rows, cols, 1)
    rc, ref, _, _ = oracle.dualpol_synrgb(b1.astype(np.float32), b2.astype(np.float32), int(St.Clahe))
    with S.Context(0, async_dev=True) as c:
        rgb, plan, packed = c.dualpol_synrgb_pyramid(b1, b2, St.Clahe, min_size=8)
    assert rc == 0 and np.array_equal(rgb, ref) and np.array_equal(packed, R.pack(R.overviews(ref, 8), cols, rows, 8, 8))


def test_file_flow_writes_the_product_as_a_tiled_tiff_with_overviews(ctx, tmp_path):
    import test_tiff_pyramid as T
    rows, cols = 700, 900
    b = [synth.scene_u16(rows, cols, k) for k in (0, 1)]
    paths = [str(tmp_path / f"b{k}.tif") for k in (0, 1)]
    for p, a in zip(paths, b):
        w = S.TiffWriter(p, cols, rows, 1, 16)
        w.write_rows(0, a)
        w.finish()
    rd = [S.TiffReader(p) for p in paths]
    out = str(tmp_path / "cog.tif")
    gt = [500000.0, 10.0, 0.0, 4100000.0, 0.0, -10.0]
    st = ctx.dualpol_synrgb_stream_cog(S.TiffPair(*rd).reader(), rows, cols, St.Clahe, out, skip_zero=True, tile=64, min_size=64, geotransform=gt,
                                       want_stats=True)
    rc, ref, _, _ = oracle.dualpol_synrgb(b[0].astype(np.float32), b[1].astype(np.float32), int(St.Clahe))
    assert rc == 0 and st[0].valid_count > 0
    big, dirs, offs, extents, raw = T.parse(out)                                                # the file parses
    want = [ref] + R.overviews(ref, 64, True)
    assert not big and len(dirs) == len(want) == 5 and dirs[0][33550][1] == [10.0, 10.0, 0.0]
    assert max(extents) <= min(o for d in dirs for o in d[324][1])
    for k, (d, a) in enumerate(zip(dirs, want)):
        img, pad_rows, pad_cols = T.tiles_of(raw, d, 3, 1, np.uint8)
        assert np.array_equal(img, a), k                                                        # directory 0: the oracle's RGB; every overview: the restatement
        assert not pad_rows.any() and not pad_cols.any() and d[322][1] == [64] and ((254 in d) == (k > 0))
