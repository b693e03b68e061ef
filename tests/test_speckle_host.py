"""The speckle filters' restatement (tests/speckleref.py, what the kernels are compared with) against an independent brute-force
evaluation of DESIGN.md 9c -- a per-pixel Python loop, exact `int` sums, the same f64 formula in Python floats -- by f32 bit pattern,
and the properties the definition states.  No GPU."""
import functools
import math

import numpy as np
import pytest

import sarpro_amd as S
import speckleref as R

PAIRS = [(f, k) for f in (R.LEE, R.KUAN) for k in (3, 5, 7)]
ROWS, COLS = 30, 40


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def band_u16():
    rng = np.random.default_rng(11)
    v = (rng.gamma(2.0, 300.0, (ROWS, COLS)).clip(1, 65535)).astype(np.uint16)
    v[rng.random((ROWS, COLS)) < 0.08] = 0    # scattered black fill
    v[:, :2] = 0                              # a fill border
    v[10:19, 20:29] = 0                       # a 9 x 9 hole ...
    v[14, 24] = 777                           # ... around one valid sample: its only valid neighbour is itself
    v[3:6, 30:36] = 65535                     # saturated samples
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def band_f32():
    rng = np.random.default_rng(12)
    x = np.exp(rng.standard_normal((ROWS, COLS)) * 2.0).astype(np.float32) * np.float32(50.0)
    flat = x.ravel()
    flat[::17] *= -1.0
    flat[5::29] = 0.0
    flat[7::31] = np.nan
    flat[11::37] = np.float32(1e-5)           # just below the threshold: invalid
    flat[13::41] = R.THR                      # equal to it: valid
    flat[3::43] = np.inf
    flat[9::53] = np.float32(3e38)
    flat[19::59] = -np.inf
    x[10:19, 20:29] = np.nan
    x[14, 24] = 2.5
    x.setflags(write=False)
    return x


def brute(v, filt, k, looks):
    """-> (out f32 array, m as f64 array with NaN where the centre is invalid)"""
    is_u16 = v.dtype == np.uint16
    rows, cols = v.shape
    h = k // 2
    cu2 = 1.0 / looks
    g = 1.0 / (1.0 + cu2)
    thr = float(R.THR)
    ok = (lambda s: s >= 1) if is_u16 else (lambda s: thr <= s < math.inf)  # (NaN compares false)
    out = np.empty((rows, cols), np.float32)
    mean = np.full((rows, cols), np.nan)
    lst = v.tolist()
    for y in range(rows):
        for x in range(cols):
            c = lst[y][x]
            if not ok(c):
                out[y, x] = v[y, x] if not is_u16 else np.float32(c)
                continue
            n = 0
            S1 = S2 = 0 if is_u16 else 0.0
            for yy in range(max(y - h, 0), min(y + h + 1, rows)):
                r1 = r2 = 0 if is_u16 else 0.0
                for xx in range(max(x - h, 0), min(x + h + 1, cols)):
                    s = lst[yy][xx]
                    if ok(s):
                        n += 1
                        r1 = r1 + s
                        r2 = r2 + s * s
                S1 = S1 + r1
                S2 = S2 + r2
            A = S1 * S1
            D = n * S2 - A if is_u16 else float(n) * S2 - A
            m = float(S1) / float(n)
            mean[y, x] = m
            if not D > 0:
                o = m
            else:
                q = (cu2 * float(A)) / float(D)
                w = 1.0 - q
                if filt == R.KUAN:
                    w = w * g
                if not w > 0:
                    w = 0.0
                o = m + w * (float(c) - m)
            with np.errstate(over="ignore"):
                out[y, x] = np.float32(o)
    if not is_u16:  # an invalid centre keeps its bits (the assignment above may quiet a NaN's payload on some hosts)
        inv = ~np.isfinite(mean)
        out.view(np.uint32)[inv] = v.view(np.uint32)[inv]
    return out, mean


def test_threshold_is_the_librarys():
    assert np.float32(S.host_f32_valid_threshold()).view(np.uint32) == R.THR.view(np.uint32)


@pytest.mark.parametrize("looks", [1.0, 4.4])
@pytest.mark.parametrize("filt,k", PAIRS)
def test_restatement_equals_the_brute_force_u16(filt, k, looks):
    v = band_u16()
    ref, _ = brute(v, filt, k, looks)
    got = R.speckle_u16(v, filt, k, looks)
    assert bits_equal(got, ref), int((got.view(np.uint32) != ref.view(np.uint32)).sum())


@pytest.mark.parametrize("looks", [1.0, 4.4])
@pytest.mark.parametrize("filt,k", PAIRS)
def test_restatement_equals_the_brute_force_f32(filt, k, looks):
    v = band_f32()
    ref, _ = brute(v, filt, k, looks)
    got = R.speckle_f32(v, filt, k, looks)
    assert bits_equal(got, ref), int((got.view(np.uint32) != ref.view(np.uint32)).sum())


@pytest.mark.parametrize("filt,k", PAIRS)
def test_constant_rasters_come_back_unchanged(filt, k):
    for dn in (65535, 1, 1234):
        out = R.speckle_u16(np.full((12, 9), dn, np.uint16), filt, k, 4.4)
        assert np.all(out == np.float32(dn)) and out.dtype == np.float32
    assert np.all(R.speckle_u16(np.zeros((12, 9), np.uint16), filt, k, 4.4) == 0.0)
    c = np.full((12, 9), np.float32(0.1), np.float32)
    assert bits_equal(R.speckle_f32(c, filt, k, 4.4), c)


@pytest.mark.parametrize("filt,k", PAIRS)
def test_output_lies_between_mean_and_centre_and_valid_stays_valid(filt, k):
    for v, fn in ((band_u16(), R.speckle_u16), (band_f32(), R.speckle_f32)):
        out = fn(v, filt, k, 4.4)
        _, m = brute(v, filt, k, 4.4)
        valid = np.isfinite(m)
        with np.errstate(over="ignore"):
            m32 = m[valid].astype(np.float32)
        c = v[valid].astype(np.float32)
        assert np.all(out[valid] >= np.minimum(m32, c)) and np.all(out[valid] <= np.maximum(m32, c))
        if v.dtype == np.uint16:
            assert np.array_equal(valid, v >= 1) and np.all(out[valid] >= 1.0) and np.all(out[~valid] == 0.0)
        else:
            assert np.all(out[valid] >= R.THR) and np.all(np.isfinite(out[valid]))
            assert np.array_equal(out.view(np.uint32)[~valid], v.view(np.uint32)[~valid])  # invalid centres keep their bits


@pytest.mark.parametrize("filt,k", PAIRS)
def test_very_few_looks_give_the_boxcar_mean_of_the_valid_samples(filt, k):
    """cu2 = 100 >= n: q = cu2 * S1^2 / D >= cu2 * S1^2 / (n * S2) >= cu2 / n >= 1, so w = 0 everywhere"""
    for v, fn in ((band_u16(), R.speckle_u16), (band_f32(), R.speckle_f32)):
        out = fn(v, filt, k, 1e-2)
        _, m = brute(v, filt, k, 1e-2)
        valid = np.isfinite(m)
        with np.errstate(over="ignore"):
            assert np.array_equal(out[valid], m[valid].astype(np.float32))


@pytest.mark.parametrize("filt", [R.LEE, R.KUAN])
def test_very_many_looks_approach_the_input(filt):
    v = band_u16()
    err = [float(np.abs(R.speckle_u16(v, filt, 7, looks) - v.astype(np.float32)).mean()) for looks in (1.0, 1e2, 1e4, 1e30)]
    assert err[0] > err[1] > err[2] > err[3] == 0.0, err
    x = np.abs(band_f32()).clip(1.0, 1e4)
    x = np.where(np.isfinite(x), x, np.float32(3.0)).astype(np.float32)
    out = R.speckle_f32(x, filt, 7, 1e30)
    assert float(np.abs(out - x).max()) <= 1e-3
