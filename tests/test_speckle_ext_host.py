"""Frost and Refined Lee without a GPU: the library's host EXP against the restatement's (tests/speckleextref.py) by f64
bit pattern and against math.exp in ulps; the two restatements against an independent brute-force evaluation of the definition -- a
per-pixel Python loop over Python ints and floats -- by f32 bit pattern; the properties the definition states; and the conditions the
GPU tests' scene has to meet for those tests to reach every case."""
import functools
import math

import numpy as np
import pytest

import sarpro_amd as S
import speckleextref as X
import speckleref as R

ROWS, COLS = 23, 37
DAMPINGS = [1e-3, 1.0, 2.0, 50.0, 1e6, 1e300]


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def band():
    rng = np.random.default_rng(21)
    v = (rng.gamma(2.0, 300.0, (ROWS, COLS)).clip(1, 65535)).astype(np.uint16)
    v[:, 20:] = (v[:, 20:].astype(np.uint32) * 5).clip(1, 65535).astype(np.uint16)  # an edge: directed pixels of every kind
    v[rng.random((ROWS, COLS)) < 0.01] = 0    # a few scattered zeros: fallback pixels inside the raster
    v[:, :1] = 0                              # a fill border
    v[2:5, 30:36] = 65535                     # saturated samples
    v[8:20, 3:19] = 500                       # a flat patch: D = 0 and gradient ties
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def exp_arguments():
    rng = np.random.default_rng(5)
    special = [0.0, -0.0, -708.0, np.nextafter(-708.0, 0.0), np.nextafter(-708.0, -np.inf), -709.0, -745.2, -1e4, -1e308, -np.inf,
               -5e-324, -2.2250738585072014e-308, -1e-300, -1e-20, -2.0 ** -53, -2.0 ** -52, -math.log(2.0) / 2, -math.log(2.0), -1.0, -0.5]
    x = np.concatenate([np.array(special), -rng.random(60000) * 708.0, -np.exp(rng.uniform(-80.0, 1.0, 40000)), -rng.random(20000),
                        -(np.arange(1, 1023) * math.log(2.0) * 0.5),                      # next to the ties of rint(x * LOG2E)
                        -rng.random(2000) * 40.0 - 708.0])                                # below -708
    x = x[x <= 0]
    assert x.size >= 100000
    return x


def py_exp(x):
    """EXP of the definition in Python floats (IEEE f64, one rounding per operation); round() of a float rounds ties to even"""
    if x < -708.0:
        return 0.0
    kf = float(round(x * X.LOG2E))
    r = (x - kf * X.LN2_HI) - kf * X.LN2_LO
    p = 1.0 / math.factorial(13)
    for i in range(12, -1, -1):
        p = p * r + 1.0 / math.factorial(i)
    return math.ldexp(p, int(kf))


def test_host_exp_equals_the_restatement_bit_for_bit():
    x = exp_arguments()
    got = np.array([S.host_speckle_exp(float(t)) for t in x])
    ref = X.exp(x)
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), int((got.view(np.uint64) != ref.view(np.uint64)).sum())
    assert S.host_speckle_exp(0.0) == 1.0 and S.host_speckle_exp(-0.0) == 1.0
    assert S.host_speckle_exp(-np.inf) == 0.0 and S.host_speckle_exp(float(np.nextafter(-708.0, -np.inf))) == 0.0
    assert S.host_speckle_exp(-708.0) > 0.0
    assert np.all((got >= 0.0) & (got <= 1.0)) and np.all(got[x >= -708.0] > 0.0)
    some = x[:: max(1, x.size // 3000)]
    assert [py_exp(float(t)) for t in some] == [S.host_speckle_exp(float(t)) for t in some]
    assert math.isnan(S.host_speckle_exp(float("nan"))) and math.isnan(S.host_speckle_exp(1.0))  # defined for x <= 0 only


def test_host_exp_stays_within_two_ulp_of_libm_and_is_monotone():
    """1 ulp was measured against glibc's correctly rounded-in-practice exp; 2 leaves room for another libm"""
    x = exp_arguments()
    x = np.sort(x[x >= -708.0])
    got = np.array([S.host_speckle_exp(float(t)) for t in x])
    ref = np.array([math.exp(float(t)) for t in x])
    ulps = np.abs(got.view(np.int64) - ref.view(np.int64))
    print("largest distance from math.exp:", int(ulps.max()), "ulp")
    assert int(ulps.max()) <= 2
    assert np.all(np.diff(got) >= 0.0)


# ---------------------------------------------------------------------------- brute force
def brute_frost(v, k, damping):
    rows, cols = v.shape
    h = k // 2
    lst = v.tolist()
    out = np.zeros((rows, cols), np.float32)
    lo = np.full((rows, cols), np.nan, np.float32)
    hi = np.full((rows, cols), np.nan, np.float32)
    for y in range(rows):
        for x in range(cols):
            if lst[y][x] < 1:
                continue
            T, N = {}, {}
            n = S1 = S2 = 0
            vals = []
            for dy in range(-h, h + 1):
                for dx in range(-h, h + 1):
                    yy, xx = y + dy, x + dx
                    c = dy * dy + dx * dx
                    T.setdefault(c, 0); N.setdefault(c, 0)
                    if 0 <= yy < rows and 0 <= xx < cols and lst[yy][xx] >= 1:
                        s = lst[yy][xx]
                        T[c] += s; N[c] += 1
                        n += 1; S1 += s; S2 += s * s
                        vals.append(s)
            A = S1 * S1
            D = n * S2 - A
            a = damping * (float(D) / float(A))
            num = den = 0.0
            for c in sorted(T):
                w = 1.0 if c == 0 else py_exp(-(a * math.sqrt(float(c))))
                num = num + w * float(T[c])
                den = den + w * float(N[c])
            out[y, x] = np.float32(num / den)
            lo[y, x], hi[y, x] = np.float32(min(vals)), np.float32(max(vals))
    return out, lo, hi


def brute_refined_lee(v, looks):
    rows, cols = v.shape
    lst = v.tolist()
    cu2 = 1.0 / looks
    out = R.speckle_u16(v, R.LEE, 7, looks).copy()
    for y in range(3, rows - 3):
        for x in range(3, cols - 3):
            w = [[lst[y + dy][x + dx] for dx in range(-3, 4)] for dy in range(-3, 4)]
            if min(min(r) for r in w) < 1:
                continue
            B = [[sum(w[2 * i + a][2 * j + b] for a in range(3) for b in range(3)) for j in range(3)] for i in range(3)]
            g = [abs((B[0][2] + B[1][2] + B[2][2]) - (B[0][0] + B[1][0] + B[2][0])), abs((B[0][1] + B[0][2] + B[1][2]) - (B[1][0] + B[2][0] + B[2][1])),
                 abs((B[0][0] + B[0][1] + B[0][2]) - (B[2][0] + B[2][1] + B[2][2])), abs((B[0][0] + B[0][1] + B[1][0]) - (B[1][2] + B[2][1] + B[2][2]))]
            d = g.index(max(g))
            P, fp, Q, fq = [(B[1][2], lambda dy, dx: dx >= 0, B[1][0], lambda dy, dx: dx <= 0),
                            (B[0][2], lambda dy, dx: dx >= dy, B[2][0], lambda dy, dx: dx <= dy),
                            (B[0][1], lambda dy, dx: dy <= 0, B[2][1], lambda dy, dx: dy >= 0),
                            (B[0][0], lambda dy, dx: dx + dy <= 0, B[2][2], lambda dy, dx: dx + dy >= 0)][d]
            f = fp if abs(P - B[1][1]) <= abs(Q - B[1][1]) else fq
            half = [w[dy + 3][dx + 3] for dy in range(-3, 4) for dx in range(-3, 4) if f(dy, dx)]
            assert len(half) == 28
            S1, S2 = sum(half), sum(s * s for s in half)
            A = S1 * S1
            D = 28 * S2 - A
            m = S1 / 28.0
            if not D > 0:
                o = m
            else:
                q = (cu2 * float(A)) / float(D)
                wt = 1.0 - q
                if not wt > 0:
                    wt = 0.0
                o = m + wt * (float(lst[y][x]) - m)
            out[y, x] = np.float32(o)
    return out


@pytest.mark.parametrize("damping", [1e-3, 2.0, 1e300])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_frost_restatement_equals_the_brute_force(k, damping):
    ref, _, _ = brute_frost(band(), k, damping)
    got = X.frost_u16(band(), k, damping)
    assert bits_equal(got, ref), int((got.view(np.uint32) != ref.view(np.uint32)).sum())


@pytest.mark.parametrize("looks", [1.0, 4.4, 1e6])
def test_refined_lee_restatement_equals_the_brute_force(looks):
    ref = brute_refined_lee(band(), looks)
    got, info = X.refined_lee_u16(band(), looks, info=True)
    assert bits_equal(got, ref), int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    assert info["directed"].sum() > 200 and len(set(info["half"][info["directed"]].tolist())) == 8 and info["ties"] >= 1


@pytest.mark.parametrize("k", [3, 5, 7])
def test_frost_properties(k):
    v = band()
    valid = v >= 1
    _, lo, hi = brute_frost(v, k, 1.0)
    for damping in DAMPINGS:
        out = X.frost_u16(v, k, damping)
        assert np.all(np.isfinite(out)) and np.all(out[~valid] == 0.0)
        assert np.all(out[valid] >= lo[valid]) and np.all(out[valid] <= hi[valid]), damping
        if damping >= 1e6:  # every weight but the centre's is 0 wherever the window is not flat, and a flat window's mean is v
            assert np.array_equal(out, v.astype(np.float32))
    # a pixel whose window is flat (D = 0) gets the boxcar mean, which is v
    h = k // 2
    flat = np.zeros(v.shape, bool)
    flat[8 + h:20 - h, 3 + h:19 - h] = True
    out = X.frost_u16(v, k, 2.0)
    assert flat.sum() >= 60 and np.all(out[flat] == np.float32(500.0))


def test_constant_rasters_come_back_unchanged():
    for dn in (65535, 1, 1234):
        c = np.full((12, 15), dn, np.uint16)
        for k in (3, 5, 7):
            for damping in (1e-3, 2.0, 1e300):
                out = X.frost_u16(c, k, damping)
                assert out.dtype == np.float32 and np.all(out == np.float32(dn)), (dn, k, damping)
        assert np.all(X.refined_lee_u16(c, 4.4) == np.float32(dn))
    z = np.zeros((12, 15), np.uint16)
    assert np.all(X.frost_u16(z, 7, 2.0).view(np.uint32) == 0) and np.all(X.refined_lee_u16(z, 4.4).view(np.uint32) == 0)


def test_refined_lee_is_lee_7_on_every_fallback_pixel_and_lies_between_m_and_v_elsewhere():
    for v in (band(), X.scene(60, 90)):
        out, info = X.refined_lee_u16(v, 4.4, info=True)
        lee = R.speckle_u16(v, R.LEE, 7, 4.4)
        fb = ~info["directed"]
        assert fb.sum() > 100 and np.array_equal(out.view(np.uint32)[fb], lee.view(np.uint32)[fb])
        d = info["directed"]
        m32, c = info["m"][d].astype(np.float32), v[d].astype(np.float32)
        assert np.all(out[d] >= np.minimum(m32, c)) and np.all(out[d] <= np.maximum(m32, c))
        assert (out.view(np.uint32)[d] != lee.view(np.uint32)[d]).mean() > 0.5  # the directed case is another filter


def test_ext_dispatch_gives_lee_and_kuan_unchanged():
    v = band()
    for filt in (X.LEE, X.KUAN):
        assert bits_equal(X.speckle_ext_u16(v, filt, 5, 4.4, 123.0), R.speckle_u16(v, filt, 5, 4.4))


def test_the_gpu_tests_scene_reaches_every_case():
    """what tests/test_gpu_speckle_ext.py relies on at 300 x 600: most pixels directed, every half-window chosen often, gradient ties,
    and many valid-centre pixels that fall back"""
    v = X.scene(300, 600)
    assert np.all(v[:3] == 0) and np.all(v[:, :4] == 0) and v[-1, -1] == 65535
    base = S.synth.scene_u16(300, 600, 0)
    assert 0.001 < ((v == 0) & (base != 0))[3:, 4:].mean() < 0.004  # the scattered zeros, beside the synthetic scene's own no-data wedges
    r1, c1 = 300 // 2 + 3, 600 // 2 + 1
    blk = v[r1:r1 + 9, c1:c1 + 9]
    assert (blk != 0).sum() == 1 and blk[4, 4] == 4321
    _, info = X.refined_lee_u16(v, 4.4, info=True)
    directed = info["directed"]
    counts = np.bincount(info["half"][directed], minlength=8)
    fallbacks = int(((v >= 1) & ~directed).sum())
    print("directed", float(directed.mean()), "halves", dict(zip([n for n, _ in X.HALVES], counts.tolist())), "ties", info["ties"], "fallbacks", fallbacks)
    assert directed.mean() >= 0.5
    assert counts.min() >= 1000
    assert info["ties"] >= 1
    assert fallbacks >= 1000
