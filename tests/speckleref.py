"""The speckle filters' definition (include/sarpro_hip.h), restated in numpy from the text, not from the C++.  The
definition is this project's own -- the reference's roadmap names Lee and Kuan and ships neither -- so this file IS what the kernels
are compared with, by f32 bit pattern.

    cu2 = 1 / looks;  g = 1 / (1 + cu2)                                      (f64, once per call)
    valid: u16 v >= 1;  f32 THR <= v < +inf
    window k x k clipped to the raster, valid samples only; n of them
    centre invalid -> (float)v (u16) / the input's bits (f32)
    S1 = sum v, S2 = sum v^2, A = S1 * S1, D = n * S2 - A, m = S1 / n
    !(D > 0) -> (float)m;  else q = (cu2 * A) / D, w = 1 - q (Lee) | (1 - q) * g (Kuan), !(w > 0) -> w = 0, (float)(m + w * (v - m))
u16: the sums, A and D are exact integers (int64 here, from 2-D prefix sums).  f32: f64 sums in the fixed order -- per window row left
to right from 0.0, the rows' partials top to bottom from 0.0.  (An invalid sample enters these sums as +0.0: the sums are non-negative,
so adding +0.0 leaves every bit as it is, which is "only valid samples count".)  numpy's f64 + - * / are IEEE operations, one rounding
each, nothing fused."""
import numpy as np

LEE, KUAN = 0, 1
# sarpro_hip_host_f32_valid_threshold(): the smallest f32 with 10 * log10(v) > -50; f32(1e-5) lies below 1e-5, its successor above
THR = np.nextafter(np.float32(1e-5), np.float32(1.0))


def _params(filt, window, looks):
    assert filt in (LEE, KUAN) and window in (3, 5, 7) and np.isfinite(looks) and looks > 0
    cu2 = np.float64(1.0) / np.float64(looks)
    g = np.float64(1.0) / (np.float64(1.0) + cu2)
    return cu2, g


def _box(a, h):
    """int64 sums of `a` over the (2h + 1)^2 window around every pixel, clipped to the raster"""
    rows, cols = a.shape
    p = np.zeros((rows + 1, cols + 1), np.int64)
    p[1:, 1:] = a.cumsum(0).cumsum(1)
    y0 = np.clip(np.arange(rows) - h, 0, rows)[:, None]
    y1 = np.clip(np.arange(rows) + h + 1, 0, rows)[:, None]
    x0 = np.clip(np.arange(cols) - h, 0, cols)[None, :]
    x1 = np.clip(np.arange(cols) + h + 1, 0, cols)[None, :]
    return p[y1, x1] - p[y0, x1] - p[y1, x0] + p[y0, x0]


def _tail(filt, cu2, g, n, S1, A, D, v):
    """f64 arrays in, f64 `o` (the value before its one rounding to f32) out; entries with n == 0 are meaningless"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = S1 / n
        q = (cu2 * A) / D
        w = np.float64(1.0) - q
        if filt == KUAN:
            w = w * g
        w = np.where(w > 0, w, np.float64(0.0))
        o = m + w * (v - m)
        return np.where(D > 0, o, m), m


def speckle_u16(v, filt, window, looks):
    assert v.dtype == np.uint16 and v.ndim == 2
    cu2, g = _params(filt, window, looks)
    h = window // 2
    vi = v.astype(np.int64)
    n = _box((vi > 0).astype(np.int64), h)
    S1 = _box(vi, h)
    S2 = _box(vi * vi, h)
    A = S1 * S1
    D = n * S2 - A
    assert int(A.max(initial=0)) < 1 << 45 and int(D.max(initial=0)) < 1 << 45 and int(D.min(initial=0)) >= 0
    o, _ = _tail(filt, cu2, g, n.astype(np.float64), S1.astype(np.float64), A.astype(np.float64), D.astype(np.float64), vi.astype(np.float64))
    with np.errstate(invalid="ignore"):
        out = o.astype(np.float32)
    out[v == 0] = np.float32(0.0)
    return out


def speckle_f32(v, filt, window, looks):
    assert v.dtype == np.float32 and v.ndim == 2
    cu2, g = _params(filt, window, looks)
    h = window // 2
    rows, cols = v.shape
    with np.errstate(invalid="ignore"):
        valid = (v >= THR) & (v < np.float32(np.inf))
    d = np.where(valid, v, np.float32(0)).astype(np.float64)
    dp = np.pad(d, h)
    vp = np.pad(valid, h)
    S1 = np.zeros((rows, cols), np.float64)
    S2 = np.zeros((rows, cols), np.float64)
    n = np.zeros((rows, cols), np.int64)
    with np.errstate(over="ignore"):
        for dy in range(window):          # window rows, top to bottom
            r1 = np.zeros((rows, cols), np.float64)
            r2 = np.zeros((rows, cols), np.float64)
            for dx in range(window):      # left to right
                s = dp[dy:dy + rows, dx:dx + cols]
                r1 = r1 + s
                r2 = r2 + s * s
                n += vp[dy:dy + rows, dx:dx + cols]
            S1 = S1 + r1
            S2 = S2 + r2
        A = S1 * S1
        B = n.astype(np.float64) * S2
        D = B - A
    o, _ = _tail(filt, cu2, g, n.astype(np.float64), S1, A, D, d)
    with np.errstate(invalid="ignore", over="ignore"):
        out = o.astype(np.float32)
    return np.where(valid, out.view(np.uint32), v.view(np.uint32)).view(np.float32)
