"""Overview pyramids without a GPU: the numpy restatement (tests/overviewref.py) against hand-derived cases, the
plan of the packed buffer, and the library's host twin of the device pass (sarpro_hip_host_overviews) against the restatement, byte
for byte."""
import ctypes as C

import numpy as np
import pytest

import overviewref as R
import sarpro_amd as S
from sarpro_amd import _lib

SHAPES = [(2, 2, 1), (3, 5, 1), (64, 64, 1), (65, 63, 1), (130, 67, 1), (200, 130, 1)]  # (cols, rows, min_size): every one down to 1 x 1


def _px(a, **k):
    return R.next_level(np.asarray(a)[..., None] if np.asarray(a).ndim == 2 else np.asarray(a), **k)


def test_hand_derived_cases():
    assert _px(np.array([[1, 2], [3, 4]], np.uint8)).tolist() == [[[3]]]            # (10 + 2) // 4
    assert _px(np.array([[255, 254]], np.uint8)).tolist() == [[[255]]]              # (509 + 1) // 2: half rounds up
    z = np.array([[0, 7], [0, 0]], np.uint8)
    assert _px(z, skip_zero=True).tolist() == [[[7]]]                               # one pixel takes part
    assert _px(z).tolist() == [[[2]]]                                               # (7 + 2) // 4
    rgb = np.zeros((2, 2, 3), np.uint8)
    rgb[0, 0], rgb[0, 1], rgb[1, 0] = (1, 0, 0), (0, 1, 0), (0, 0, 1)               # three valid pixels, the fourth no-data
    assert _px(rgb, skip_zero=True).tolist() == [[[0, 0, 0]]]                       # (1 + 1) // 3 = 0: no-data one level up
    assert _px(np.array([[65535, 65535], [65535, 65534]], np.uint16)).tolist() == [[[65535]]]
    assert _px(np.zeros((2, 2), np.uint16), skip_zero=True).tolist() == [[[0]]]     # n = 0
    col = np.array([[9], [4], [5]], np.uint8)                                        # an odd height: the last row stands alone
    assert _px(col).tolist() == [[[7]], [[5]]]


def test_the_cascade_reads_the_rounded_level():
    a = np.array([[1, 2, 0, 0], [2, 2, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]], np.uint8)
    l1, l2 = R.overviews(a, min_size=1)
    assert l1[..., 0].tolist() == [[2, 0], [0, 0]] and l2.tolist() == [[[1]]]       # (7 + 2) // 4 = 2, 1 // 4 -> 0; then (2 + 2) // 4 = 1
    assert (sum(map(int, a.ravel())) + 8) // 16 == 1                                  # (here the direct 4 x 4 mean agrees)
    b = np.array([[1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 2, 2], [1, 1, 2, 2]], np.uint8)
    assert R.overviews(b, min_size=1)[1].tolist() == [[[1]]]                          # (1 + 1 + 1 + 2 + 2) // 4 = 1


def _plan_tuple(p):
    return [(p.cols[k], p.rows[k], p.pitch_bytes[k], p.offset_bytes[k]) for k in range(p.levels)]


def test_plan():
    p = S.overview_plan(20000, 20000, 3, 8, 512)
    assert p.levels == 6 and (p.cols[5], p.rows[5]) == (313, 313)
    assert S.overview_plan(20000, 20000, 3, 8, 0).levels == 6                        # min_size 0 means 512
    p = S.overview_plan(200, 130, 1, 8, 1)
    assert p.levels == 8 and (p.cols[7], p.rows[7]) == (1, 1)
    p = S.overview_plan(65, 63, 2, 16, 1)
    assert [(p.cols[k], p.rows[k]) for k in range(p.levels)] == [(33, 32), (17, 16), (9, 8), (5, 4), (3, 2), (2, 1), (1, 1)]
    p = S.overview_plan(1, 1, 1, 8, 1)
    assert p.levels == 0 and p.total_bytes == 0
    assert S.overview_plan(1 << 30, 1, 1, 8, 1).levels == 16                          # capped
    for cols, rows, ms in SHAPES + [(20000, 20000, 0), (4099, 41, 0)]:
        for comps in (1, 2, 3):
            for bits in (8, 16):
                p = S.overview_plan(cols, rows, comps, bits, ms)
                lay, total = R.plan(cols, rows, comps, bits, ms)
                assert p.levels > 0
                assert _plan_tuple(p) == lay and p.total_bytes == total and (p.components, p.bits) == (comps, bits)
                end = 0
                for w, h, pitch, off in lay:
                    assert pitch % 16 == 0 and off % 256 == 0 and pitch >= w * comps * bits // 8 and off >= end   # no overlap
                    end = off + h * pitch


def test_plan_argument_checks():
    p = _lib.OvrPlan()
    f = _lib.lib.sarpro_hip_overview_plan
    for args in ((0, 5, 1, 8), (5, 0, 1, 8), (5, 5, 0, 8), (5, 5, 4, 8), (5, 5, 1, 12), (5, 5, 1, 32)):
        assert f(*args, 1, C.byref(p)) == _lib.ERR_INVALID_ARG, args
    assert f(5, 5, 1, 8, 1, None) == _lib.ERR_INVALID_ARG
    with pytest.raises(S.SarproHipError):
        S.overview_plan(5, 5, 7, 8)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("comps", [1, 2, 3])
@pytest.mark.parametrize("skip", [False, True])
def test_host_overviews_match_the_restatement(dtype, comps, skip):
    for n, (cols, rows, ms) in enumerate(SHAPES):
        a = R.wedge_raster(rows, cols, comps, dtype, 100 + n)
        want = R.pack(R.overviews(a, ms, skip), cols, rows, a.dtype.itemsize * 8, ms)
        plan, got = S.host_overviews(a, ms, skip)
        assert plan.levels == len(R.level_shapes(cols, rows, ms)) > 0 and got.size > 0           # (no case compares empty buffers)
        assert np.array_equal(got, want), (cols, rows)                               # the levels AND the 0xA5 padding, untouched
        # a source pitch larger than the row
        pitch = (cols * comps + 5) * a.dtype.itemsize
        buf = np.full((rows, pitch // a.dtype.itemsize), 0xEE, dtype)
        buf[:, :cols * comps] = a.reshape(rows, cols * comps)
        _, got2 = S.host_overviews(buf, ms, skip, pitch_bytes=pitch, shape=(rows, cols, comps))
        assert np.array_equal(got2, want), (cols, rows)


def test_host_overviews_argument_checks():
    a = np.zeros((4, 4), np.uint8)
    plan = S.overview_plan(4, 4, 1, 8, 1)
    out = np.zeros(plan.total_bytes, np.uint8)
    f = _lib.lib.sarpro_hip_host_overviews
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    assert f(vp(a), 4, 4, 4, 1, 8, 0, C.byref(plan), vp(out)) == _lib.OK
    assert f(vp(a), 4, 4, 3, 1, 8, 0, C.byref(plan), vp(out)) == _lib.ERR_INVALID_ARG    # pitch < row
    assert f(vp(a), 4, 4, 4, 1, 8, 2, C.byref(plan), vp(out)) == _lib.ERR_INVALID_ARG    # unknown flag
    assert f(vp(a), 5, 4, 8, 1, 8, 0, C.byref(plan), vp(out)) == _lib.ERR_INVALID_ARG    # another raster's plan
    assert f(vp(a), 4, 4, 4, 2, 8, 0, C.byref(plan), vp(out)) == _lib.ERR_INVALID_ARG
    assert f(None, 4, 4, 4, 1, 8, 0, C.byref(plan), vp(out)) == _lib.ERR_INVALID_ARG
    assert f(vp(a), 4, 4, 4, 1, 8, 0, None, vp(out)) == _lib.ERR_INVALID_ARG
    empty = S.overview_plan(1, 1, 1, 8, 1)
    assert f(vp(a), 1, 1, 1, 1, 8, 0, C.byref(empty), None) == _lib.OK                   # 0 levels: a no-op
    assert (_lib.OVR_MAX_LEVELS, _lib.OVR_SKIP_ZERO, R.MAX_LEVELS, R.SKIP_ZERO) == (16, 1, 16, 1)
