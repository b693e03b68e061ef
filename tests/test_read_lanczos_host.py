"""Lanczos downsample on read without a GPU: the exported per-axis tables against the restatement
(tests/readlanczosref.py) in every f64 bit, what the definition promises of them, the argument rules, and the restatement itself:
an independent dense-matrix evaluation, constants, the identity shape."""
import ctypes as C

import numpy as np
import pytest

import readlanczosref as L
import sarpro_amd as S
from sarpro_amd import _lib

AXIS_PAIRS = [(37, 12), (23, 7), (64, 32), (1013, 300), (4099, 1100), (5, 1), (7, 2), (64, 14), (3, 1), (7, 7), (20000, 8192)]


@pytest.mark.parametrize("n,m", AXIS_PAIRS)
def test_axis_tables_equal_the_restatement_bit_for_bit(n, m):
    first, count, w = S.host_read_lanczos_axis(n, m)
    rf, rc, rw = L.lanczos_axis(n, m)
    assert first.dtype == count.dtype == np.uint32 and w.shape == (m, 32) and w.dtype == np.float64
    assert np.array_equal(first.astype(np.int64), rf) and np.array_equal(count.astype(np.int64), rc)
    assert np.array_equal(w.view(np.uint64), rw.view(np.uint64))
    # what the definition promises
    assert int(count.min()) >= 1 and int(count.max()) <= 30
    assert np.all(first.astype(np.int64) + count <= n)
    slot = np.arange(32)[None, :]
    assert np.all(w[slot >= count[:, None]] == 0.0)                     # unused slots
    sums = np.array([float(np.sum(w[j, :count[j]])) for j in range(m)])  # (a window's weights sum to 1 within 4 ulp)
    assert np.all(np.abs(sums - 1.0) <= 4 * np.finfo(np.float64).eps)
    if n == m:
        assert np.array_equal(first, np.arange(m)) and np.all(count == 1) and np.all(w[:, 0] == 1.0)


def test_windows_of_known_shapes():
    first, count, w = S.host_read_lanczos_axis(5, 1)      # ratio 5: [-12.5, 17.5) clipped at both edges
    assert (int(first[0]), int(count[0])) == (0, 5)
    assert w[0, 2] > w[0, 1] > w[0, 0] > 0 and np.array_equal(w[0, :2], w[0, 4:2:-1])  # symmetric around the centre sample
    first, count, w = S.host_read_lanczos_axis(64, 32)    # ratio 2: 12 taps in the interior, the outer lobes negative
    assert int(count[16]) == 12 and int(first[16]) == 27
    assert w[16, 5] == w[16, 6] and w[16, 3] < 0 and w[16, 1] > 0 and w[16, 5] > 0.25
    assert int(S.host_read_lanczos_axis(23, 7)[1].max()) == 19 and int(S.host_read_lanczos_axis(64, 14)[1].max()) == 28
    assert int(S.host_read_lanczos_axis(4099, 1100)[1].max()) == 23


def test_argument_rules():
    g = _lib.lib.sarpro_hip_host_read_lanczos_axis
    a = [np.zeros(8, np.uint32), np.zeros(8, np.uint32), np.zeros(8 * 32)]
    p = [x.ctypes.data_as(C.c_void_p) for x in a]
    assert g(7, 8, *p) == _lib.ERR_INVALID_ARG             # n_dst > n_src
    assert g(7, 0, *p) == _lib.ERR_INVALID_ARG
    assert g(41, 8, *p) == _lib.ERR_INVALID_ARG            # 5.125 > 5
    assert g(6, 1, *p) == _lib.ERR_INVALID_ARG
    assert g((1 << 30) + 1, 1 << 30, *p) == _lib.ERR_INVALID_ARG
    for k in range(3):
        q = list(p)
        q[k] = None
        assert g(8, 8, *q) == _lib.ERR_INVALID_ARG
    assert g(40, 8, *p) == _lib.OK and a[1].max() == 30    # exactly 5
    assert g(8, 8, *p) == _lib.OK and a[0].tolist() == list(range(8)) and a[2].reshape(8, 32)[:, 0].tolist() == [1.0] * 8
    for n, m in ((3, 4), (11, 2), (64, 8)):
        with pytest.raises(S.SarproHipError) as ei:
            S.host_read_lanczos_axis(n, m)
        assert ei.value.code == _lib.ERR_INVALID_ARG


@pytest.mark.parametrize("rows,cols,out_rows,out_cols", [(23, 37, 7, 12), (48, 64, 24, 32), (61, 101, 20, 33), (20, 30, 13, 20), (7, 5, 2, 1)])
def test_restatement_agrees_with_dense_weight_matrices(rows, cols, out_rows, out_cols):
    """An independent route to the same numbers: out = Wy v Wx^T in f64.  The sums associate differently, so the f64 values differ by
    a few units of 1e-16 relative to the window's mass (~1e5) ahead of the one rounding to f32: at most 1 ulp of f32 apart (the
    results of random DNs sit near 32768, nowhere near the zero where the signed lobes' cancellation would matter)."""
    rng = np.random.default_rng(rows * 1000 + cols)
    v = rng.integers(0, 65536, (rows, cols), dtype=np.uint16)
    wy, wx = L.dense_weights(rows, out_rows), L.dense_weights(cols, out_cols)
    dense = np.einsum("ir,rc,jc->ij", wy, v.astype(np.float64), wx).astype(np.float32)
    ref = L.lanczos_u16(v, out_rows, out_cols)
    assert ref.shape == (out_rows, out_cols) and ref.dtype == np.float32
    ulps = np.abs(dense.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    assert int(ulps.max()) <= 1


def test_restatement_returns_constants_and_the_identity():
    for value in (1, 12345, 65535):
        v = np.full((23, 37), value, np.uint16)
        assert np.array_equal(L.lanczos_u16(v, 7, 12), np.full((7, 12), float(value), np.float32)), value
    rng = np.random.default_rng(9)
    v = rng.integers(0, 65536, (20, 30), dtype=np.uint16)
    assert np.array_equal(L.lanczos_u16(v, 20, 30), v.astype(np.float32))   # ratio 1: the cast
    t = np.zeros((48, 64), np.uint16)
    t[24, 31] = 65535
    out = L.lanczos_u16(t, 24, 32)
    assert float(out.min()) < -1000.0 and float(out.max()) > 10000.0        # no clamp: the signed lobes of a lone target
