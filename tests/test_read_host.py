"""Downsample on read without a GPU: the output shape and filter rule (sentinel1.rs:1084-1102), the per-axis window tables of the
Average filter against the restatement (tests/readref.py) in every f64 bit, known answers of the restatement itself, an independent
dense-matrix check of it, and the argument rules."""
import ctypes as C

import numpy as np
import pytest

import readref
import sarpro_amd as S
from sarpro_amd import _lib

AXIS_PAIRS = [(37, 8), (64, 16), (1013, 200), (4099, 512), (3, 2), (3, 1), (20000, 2048), (25000, 2048), (7, 7)]


def test_output_dims_and_filter_follow_the_rule():
    assert S.read_output_dims(5, 10, 5) == (3, 5, readref.READ_LANCZOS)          # 2.5 rounds away from zero
    assert S.read_output_dims(500, 3, 64) == (64, 1, readref.READ_AVERAGE)       # 0.384 -> max(.., 1)
    assert S.read_output_dims(20000, 20000, 2048) == (2048, 2048, readref.READ_AVERAGE)
    assert S.read_output_dims(25000, 16700, 2048)[2] == readref.READ_AVERAGE
    # ts >= long side: identity, Lanczos by the rule
    assert S.read_output_dims(300, 200, 300) == (300, 200, readref.READ_LANCZOS)
    assert S.read_output_dims(300, 200, 5000) == (300, 200, readref.READ_LANCZOS)
    # reductions just below and at 4.0
    assert S.read_output_dims(4000, 1000, 1000)[2] == readref.READ_AVERAGE
    assert S.read_output_dims(3999, 1000, 1000)[2] == readref.READ_LANCZOS
    assert S.read_output_dims(1000, 4001, 1000)[2] == readref.READ_AVERAGE
    n = 0
    for cols in (1, 2, 3, 5, 7, 10, 37, 64, 500, 1013, 4099, 20000, 25000):
        for rows in (1, 2, 3, 10, 23, 41, 509, 16700, 20000):
            for ts in (1, 2, 3, 5, 8, 16, 64, 128, 200, 512, 1000, 2048, 5000, 6250, 30000):
                assert S.read_output_dims(cols, rows, ts) == readref.output_dims(cols, rows, ts), (cols, rows, ts)
                n += 1
    assert n > 1000


@pytest.mark.parametrize("n,m", AXIS_PAIRS)
def test_axis_tables_equal_the_restatement_bit_for_bit(n, m):
    first, count, wf, wl, ws = S.host_read_average_axis(n, m)
    rf, rc, rwf, rwl, rws = readref.average_axis(n, m)
    assert np.array_equal(first.astype(np.int64), rf) and np.array_equal(count.astype(np.int64), rc)
    for got, ref in ((wf, rwf), (wl, rwl), (ws, rws)):
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))
    # what the definition promises: the windows tile the axis (a fractional boundary's sample belongs to both neighbours)
    assert first[0] == 0 and first[-1] + count[-1] == n
    nxt = first[1:].astype(np.int64) - (first[:-1].astype(np.int64) + count[:-1])
    assert set(nxt.tolist()) <= {-1, 0}


def test_known_answers_of_the_restatement():
    v = np.full((3, 3), 7, np.uint16)
    v[1, 1] = 100
    out = readref.average_u16(v, 2, 2)
    # rows 0 and 1 with weights 1 and 0.5, columns likewise: (7 + 3.5 + 0.5 * (7 + 50)) / 2.25 = 39 / 2.25
    assert np.array_equal(out, np.full((2, 2), np.float32(39.0 / 2.25))) and abs(float(out[0, 0]) - 17.333334) < 1e-6
    rng = np.random.default_rng(5)
    v = rng.integers(0, 65536, (8, 12), dtype=np.uint16)
    blocks = v.reshape(2, 4, 3, 4).astype(np.int64).sum(axis=(1, 3))
    assert np.array_equal(readref.average_u16(v, 2, 3), (blocks.astype(np.float64) / 16.0).astype(np.float32))  # exact block mean
    v = np.full((23, 37), 65535, np.uint16)
    assert np.array_equal(readref.average_u16(v, 5, 8), np.full((5, 8), 65535.0, np.float32))
    assert np.array_equal(readref.average_u16(v, 23, 37), v.astype(np.float32))  # ratio 1: the cast


def _dense_weights(n, m):
    first, count, wf, wl, ws = readref.average_axis(n, m)
    w = np.zeros((m, n), np.float64)
    for j in range(m):
        w[j, first[j]:first[j] + count[j]] = 1.0
        w[j, first[j]] = wf[j]
        if count[j] > 1:
            w[j, first[j] + count[j] - 1] = wl[j]
    return w, ws


@pytest.mark.parametrize("rows,cols,out_rows,out_cols", [(23, 37, 5, 8), (48, 64, 12, 16), (61, 101, 12, 20), (20, 30, 13, 20), (8, 300, 1, 1)])
def test_restatement_agrees_with_dense_weight_matrices(rows, cols, out_rows, out_cols):
    """An independent route to the same numbers: out = Wy v Wx^T / (sy sx^T) in f64.  The sums associate differently, so the f64
    values differ by a few units of 1e-16 relative ahead of the one rounding to f32: at most 1 ulp of f32 apart."""
    rng = np.random.default_rng(rows * 1000 + cols)
    v = rng.integers(0, 65536, (rows, cols), dtype=np.uint16)
    wy, sy = _dense_weights(rows, out_rows)
    wx, sx = _dense_weights(cols, out_cols)
    dense = (np.einsum("ir,rc,jc->ij", wy, v.astype(np.float64), wx) / np.outer(sy, sx)).astype(np.float32)
    ref = readref.average_u16(v, out_rows, out_cols)
    ulps = np.abs(dense.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    assert int(ulps.max()) <= 1


def test_argument_rules():
    oc, orows, alg = C.c_size_t(0), C.c_size_t(0), C.c_int(0)
    f = _lib.lib.sarpro_hip_read_output_dims
    assert f(100, 50, 0, C.byref(oc), C.byref(orows), C.byref(alg)) == _lib.ERR_INVALID_ARG
    assert f(0, 50, 10, C.byref(oc), C.byref(orows), C.byref(alg)) == _lib.ERR_INVALID_ARG
    assert f(100, 50, 10, None, C.byref(orows), C.byref(alg)) == _lib.ERR_INVALID_ARG
    assert f(100, 50, 10, C.byref(oc), None, C.byref(alg)) == _lib.ERR_INVALID_ARG
    assert f(100, 50, 10, C.byref(oc), C.byref(orows), None) == _lib.ERR_INVALID_ARG
    assert f(100, 50, 10, C.byref(oc), C.byref(orows), C.byref(alg)) == _lib.OK and (oc.value, orows.value, alg.value) == (10, 5, 0)
    with pytest.raises(S.SarproHipError) as ei:
        S.read_output_dims(100, 50, 0)
    assert ei.value.code == _lib.ERR_INVALID_ARG
    g = _lib.lib.sarpro_hip_host_read_average_axis
    a = [np.zeros(8, np.uint32), np.zeros(8, np.uint32), np.zeros(8), np.zeros(8), np.zeros(8)]
    p = [x.ctypes.data_as(C.c_void_p) for x in a]
    assert g(7, 8, *p) == _lib.ERR_INVALID_ARG   # n_dst > n_src
    assert g(7, 0, *p) == _lib.ERR_INVALID_ARG
    for k in range(5):
        q = list(p)
        q[k] = None
        assert g(8, 8, *q) == _lib.ERR_INVALID_ARG
    assert g(8, 8, *p) == _lib.OK and a[0].tolist() == list(range(8)) and a[2].tolist() == [1.0] * 8
    with pytest.raises(S.SarproHipError):
        S.host_read_average_axis(3, 4)
    assert (_lib.ERR_UNSUPPORTED, _lib.READ_DEFAULT, _lib.READ_AVERAGE, _lib.READ_LANCZOS) == (-10, -1, 0, 1)
