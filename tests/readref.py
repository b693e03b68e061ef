"""Downsample on read, restated: what `SafeReader::open_with_options(.., target_size)` asks of GDAL (io/sentinel1.rs:1084-1105,
io/gdal.rs:145-177) for a u16 measurement band -- the output shape, the filter choice and the `Average` filter itself as a separable
weighted box in f64 with one rounding to f32.  Written from the definition, not from the library's C++; parity with
GDAL's own `Average` is unpinned (GDAL is absent and the reference does not lock its version).

Only numpy: the CPU tests and the GPU tests share it."""
import math

import numpy as np

READ_DEFAULT, READ_AVERAGE, READ_LANCZOS = -1, 0, 1


def rust_round(x: float) -> float:
    """f64::round for the non-negative values met here: half away from zero (Python's round is half to even)."""
    return float(math.floor(x + 0.5))


def output_dims(cols: int, rows: int, target_size: int):
    """sentinel1.rs:1084-1102 -> (out_cols, out_rows, filter)"""
    long_side = max(cols, rows)
    scale = min(float(target_size) / float(long_side), 1.0)
    out_cols = int(max(rust_round(float(cols) * scale), 1.0))
    out_rows = int(max(rust_round(float(rows) * scale), 1.0))
    reduction = max(float(long_side) / float(target_size), 1.0)
    return out_cols, out_rows, (READ_AVERAGE if reduction >= 4.0 else READ_LANCZOS)


def average_axis(n: int, m: int):
    """The windows and weights of one axis: n source samples -> m destination samples, 1 <= m <= n.
    -> (first, count, w_first, w_last, w_sum): int64, int64, f64, f64, f64 arrays of length m."""
    assert 1 <= m <= n
    r = float(n) / float(m)
    j = np.arange(m, dtype=np.float64)
    x0 = j * r
    x1 = np.minimum((j + 1.0) * r, float(n))
    c0 = np.minimum(np.floor(x0), float(n - 1)).astype(np.int64)
    c1 = np.maximum(np.minimum(np.ceil(x1), float(n)).astype(np.int64), c0 + 1)
    count = c1 - c0
    one = count == 1
    w_first = np.where(one, x1 - x0, (c0 + 1).astype(np.float64) - x0)
    w_last = np.where(one, 0.0, x1 - (c1 - 1).astype(np.float64))
    interior = np.maximum(count - 2, 0).astype(np.float64)
    w_sum = (w_first + interior) + w_last
    return c0, count, w_first, w_last, w_sum


def average_u16(v: np.ndarray, out_rows: int, out_cols: int) -> np.ndarray:
    """(rows, cols) uint16 -> (out_rows, out_cols) float32.  Per source row: the exact integer sum of a window's interior columns (from
    the row's integer prefix sums) plus the two weighted edge samples, in f64; the rows of a window accumulated top to bottom; one
    division and one rounding to f32."""
    assert v.dtype == np.uint16 and v.ndim == 2
    rows, cols = v.shape
    cf, cc, cwf, cwl, cws = average_axis(cols, out_cols)
    rf, rc, rwf, rwl, rws = average_axis(rows, out_rows)
    last = cf + cc - 1
    wide = cc > 1
    interior = cc > 2

    def row_sums(y):  # L of the definition for every destination column
        p = np.zeros(cols + 1, np.int64)
        np.cumsum(v[y], dtype=np.int64, out=p[1:])
        s = np.where(interior, p[last] - p[np.minimum(cf + 1, cols)], 0)  # columns first + 1 .. last - 1
        line = s.astype(np.float64) + cwf * v[y, cf].astype(np.float64)
        return np.where(wide, line + cwl * v[y, last].astype(np.float64), line)

    out = np.empty((out_rows, out_cols), np.float32)
    cached_y, cached = -1, None
    for i in range(out_rows):
        t = np.zeros(out_cols, np.float64)
        r0, n = int(rf[i]), int(rc[i])
        for y in range(r0, r0 + n):
            if y != cached_y:  # (a fractional boundary's row belongs to two windows)
                cached_y, cached = y, row_sums(y)
            wy = rwf[i] if y == r0 else (rwl[i] if y == r0 + n - 1 else 1.0)
            t = t + wy * cached
        out[i] = (t / (cws * rws[i])).astype(np.float32)
    return out
