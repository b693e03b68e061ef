"""Lanczos downsample on read, restated: the filter `SafeReader::open_with_options(.., target_size)` asks of GDAL below a reduction of 4
(io/sentinel1.rs:1093-1102, io/gdal.rs:145-177 with ResampleAlg::Lanczos) for a u16 measurement band, as DESIGN.md 9d fixes it: the
a = 3 kernel with its support scaled by the reduction, separable, in f64 with one rounding to f32, no clamp.  Written from the
definition, not from the library's C++; parity with GDAL's own `Lanczos` is unpinned (GDAL is absent and the reference does not lock
its version).

Only numpy and math: the CPU tests and the GPU tests share it.  The sines are math.sin (the C library's), never np.sin."""
import math

import numpy as np

TAPS = 32       # weight slots per destination sample
MAX_RATIO = 5.0


def lanczos_axis(n: int, m: int):
    """The windows and weights of one axis: n source samples -> m destination samples, 1 <= m <= n, n / m <= 5.
    -> (first, count, weights): int64 [m], int64 [m], f64 [m, 32] (slots past a window's count are 0.0)."""
    assert 1 <= m <= n and float(n) / float(m) <= MAX_RATIO
    first = np.zeros(m, np.int64)
    count = np.zeros(m, np.int64)
    w = np.zeros((m, TAPS), np.float64)
    if m == n:
        first[:] = np.arange(m)
        count[:] = 1
        w[:, 0] = 1.0
        return first, count, w
    r = float(n) / float(m)
    s = 3.0 * r
    for j in range(m):
        x = (float(j) + 0.5) * r
        lo = max(0, int(math.floor(x - s + 0.5)))
        hi = min(n, int(math.floor(x + s + 0.5)))
        assert 1 <= hi - lo <= TAPS
        raw = []
        tot = 0.0
        for c in range(lo, hi):
            t = ((float(c) + 0.5) - x) / r
            if t == 0.0:
                v = 1.0
            elif abs(t) >= 3.0:
                v = 0.0
            else:
                pt = math.pi * t
                v = (3.0 * math.sin(pt) * math.sin(pt / 3.0)) / (pt * pt)
            raw.append(v)
            tot = tot + v
        first[j], count[j] = lo, hi - lo
        for k, v in enumerate(raw):
            w[j, k] = v / tot
    return first, count, w


def _apply_axis(src: np.ndarray, first, count, w) -> np.ndarray:
    """src: f64 [n, lanes] -> f64 [m, lanes]: out[i] = sum_k w[i][k] * src[first[i] + k] in ascending k from 0.0, every product and
    every sum rounded on its own (numpy fuses nothing)."""
    n = src.shape[0]
    out = np.zeros((len(first), src.shape[1]), np.float64)
    for k in range(int(count.max())):
        on = k < count
        idx = np.minimum(first + k, n - 1)
        out = np.where(on[:, None], out + w[:, k][:, None] * src[idx], out)
    return out


def lanczos_u16(v: np.ndarray, out_rows: int, out_cols: int) -> np.ndarray:
    """(rows, cols) uint16 -> (out_rows, out_cols) float32: H[y][j] over the columns, then the rows of H, one rounding to f32."""
    assert v.dtype == np.uint16 and v.ndim == 2
    rows, cols = v.shape
    cf, cc, cw = lanczos_axis(cols, out_cols)
    rf, rc, rw = lanczos_axis(rows, out_rows)
    h = _apply_axis(np.ascontiguousarray(v.T).astype(np.float64), cf, cc, cw)  # [out_cols, rows]: H[y][j] at [j][y]
    out = _apply_axis(np.ascontiguousarray(h.T), rf, rc, rw)                    # [out_rows, out_cols]
    return out.astype(np.float32)


def dense_weights(n: int, m: int) -> np.ndarray:
    """the axis as an [m, n] matrix (for the independent dense evaluation)"""
    first, count, w = lanczos_axis(n, m)
    d = np.zeros((m, n), np.float64)
    for j in range(m):
        d[j, first[j]:first[j] + count[j]] = w[j, :count[j]]
    return d
