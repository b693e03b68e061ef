"""Frost and Refined Lee over u16 bands (include/sarpro_hip.h), restated in numpy from the text, not from the C++.  The
definitions are this project's own, so this file IS what the kernels are compared with, by f32 bit pattern.

Common: a sample is valid iff v >= 1; the window is clipped to the raster (no reflection); only valid samples count; an invalid centre
gives 0.0f; integer sums in int64 (exact); f64 arithmetic, numpy's IEEE + - * / with one rounding each, nothing fused; one conversion to f32.

    EXP(x), x <= 0:  x < -708 -> +0.0;  kf = rint(x * LOG2E);  r = (x - kf * LN2_HI) - kf * LN2_LO;
                     p = c_13, p = p * r + c_i for i = 12..0 (c_i = 1.0 / i!);  ldexp(p, kf)
    Frost(k, damping):  a = damping * (D / A) with the window's exact S1, S2, A = S1^2, D = n * S2 - A;  per class r2 = dy^2 + dx^2 in
                     ascending order: w = 1.0 (r2 = 0) or EXP(-(a * sqrt(r2))), num += w * T_c, den += w * N_c;  out = num / den
    Refined Lee(looks):  window 7; a window that leaves the raster or holds an invalid sample: Lee 7 (speckleref).  Otherwise the nine
                     3 x 3 block sums -> four gradients -> direction (lowest index on a tie) -> the side whose block is closer to the
                     central block -> Lee's formula with n = 28 over that half-window.
The test scene both test files use is here too."""
import math

import numpy as np

import speckleref
from sarpro_amd import synth

LEE, KUAN, FROST, REFINED_LEE = 0, 1, 2, 3
LOG2E = float.fromhex("0x1.71547652b82fep+0")
LN2_HI = float.fromhex("0x1.62e42fee00000p-1")
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
C = [np.float64(1.0) / np.float64(math.factorial(i)) for i in range(14)]
# the eight half-windows in the order d0 P, d0 Q, d1 P, d1 Q, ...: name and membership of the offset (dy, dx)
HALVES = [("E", lambda dy, dx: dx >= 0), ("W", lambda dy, dx: dx <= 0), ("NE", lambda dy, dx: dx >= dy), ("SW", lambda dy, dx: dx <= dy),
          ("N", lambda dy, dx: dy <= 0), ("S", lambda dy, dx: dy >= 0), ("NW", lambda dy, dx: dx + dy <= 0), ("SE", lambda dy, dx: dx + dy >= 0)]


def exp(x):
    """EXP of the definition over an f64 array (or scalar) of arguments <= 0"""
    x = np.asarray(x, np.float64)
    zero = x < -708.0
    xs = np.where(zero, np.float64(0.0), x)
    kf = np.rint(xs * np.float64(LOG2E))
    r = (xs - kf * np.float64(LN2_HI)) - kf * np.float64(LN2_LO)
    p = np.full(x.shape, C[13], np.float64)
    for i in range(12, -1, -1):
        p = p * r + C[i]
    return np.where(zero, np.float64(0.0), np.ldexp(p, kf.astype(np.int64)))


def _window(v, h):
    """-> win(dy, dx): the int64 raster of the samples at that offset, 0 outside the raster"""
    rows, cols = v.shape
    pad = np.pad(v.astype(np.int64), h)
    return lambda dy, dx: pad[h + dy:h + dy + rows, h + dx:h + dx + cols]


def frost_u16(v, window, damping):
    assert v.dtype == np.uint16 and v.ndim == 2 and window in (3, 5, 7) and np.isfinite(damping) and damping > 0
    h = window // 2
    win = _window(v, h)
    T, N = {}, {}
    S2 = np.zeros(v.shape, np.int64)
    for dy in range(-h, h + 1):
        for dx in range(-h, h + 1):
            s = win(dy, dx)
            c = dy * dy + dx * dx
            T[c] = T.get(c, 0) + s
            N[c] = N.get(c, 0) + (s >= 1)
            S2 += s * s
    classes = sorted(T)
    assert classes == {3: [0, 1, 2], 5: [0, 1, 2, 4, 5, 8], 7: [0, 1, 2, 4, 5, 8, 9, 10, 13, 18]}[window]
    S1 = sum(T[c] for c in classes)
    n = sum(N[c].astype(np.int64) for c in classes)
    A = S1 * S1
    D = n * S2 - A
    assert int(D.min(initial=0)) >= 0 and int(A.max(initial=0)) < 1 << 45 and int(D.max(initial=0)) < 1 << 45
    valid = v >= 1
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = np.float64(damping) * (D.astype(np.float64) / A.astype(np.float64))
        a = np.where(valid, a, np.float64(0.0))  # (an invalid centre's output is 0.0 whatever a is; A may be 0 there)
        num = np.zeros(v.shape, np.float64)
        den = np.zeros(v.shape, np.float64)
        for c in classes:
            w = np.float64(1.0) if c == 0 else exp(-(a * np.sqrt(np.float64(c))))
            num = num + w * T[c].astype(np.float64)
            den = den + w * N[c].astype(np.float64)
        out = (num / den).astype(np.float32)
    out[~valid] = np.float32(0.0)
    return out


def refined_lee_u16(v, looks, info=False):
    """-> the f32 raster; info=True: (raster, dict(directed=bool raster, half=index into HALVES (-1: fallback), ties=number of directed
    pixels whose largest gradient is not unique, m=the chosen half's mean as f64 (NaN: fallback)))"""
    assert v.dtype == np.uint16 and v.ndim == 2 and np.isfinite(looks) and looks > 0
    rows, cols = v.shape
    out = speckleref.speckle_u16(v, speckleref.LEE, 7, looks).copy()
    win = _window(v, 3)
    nvalid = sum((win(dy, dx) >= 1).astype(np.int64) for dy in range(-3, 4) for dx in range(-3, 4))
    directed = nvalid == 49  # (samples outside the raster read as 0 here, so a window that leaves the raster never has 49)
    B = [[sum(win(-3 + 2 * i + a, -3 + 2 * j + b) for a in range(3) for b in range(3)) for j in range(3)] for i in range(3)]
    g = np.stack([np.abs((B[0][2] + B[1][2] + B[2][2]) - (B[0][0] + B[1][0] + B[2][0])),
                  np.abs((B[0][1] + B[0][2] + B[1][2]) - (B[1][0] + B[2][0] + B[2][1])),
                  np.abs((B[0][0] + B[0][1] + B[0][2]) - (B[2][0] + B[2][1] + B[2][2])),
                  np.abs((B[0][0] + B[0][1] + B[1][0]) - (B[1][2] + B[2][1] + B[2][2]))])
    d = np.argmax(g, axis=0)  # the first of equal maxima: the lowest index
    P = np.choose(d, [B[1][2], B[0][2], B[0][1], B[0][0]])
    Q = np.choose(d, [B[1][0], B[2][0], B[2][1], B[2][2]])
    half = 2 * d + (np.abs(P - B[1][1]) > np.abs(Q - B[1][1]))
    S1 = np.zeros(v.shape, np.int64)
    S2 = np.zeros(v.shape, np.int64)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            member = np.array([bool(f(dy, dx)) for _, f in HALVES])
            s = np.where(member[half], win(dy, dx), 0)
            S1 += s
            S2 += s * s
    assert all(sum(bool(f(dy, dx)) for dy in range(-3, 4) for dx in range(-3, 4)) == 28 for _, f in HALVES)
    A = S1 * S1
    D = 28 * S2 - A
    assert int(D[directed].min(initial=0)) >= 0 and int(A.max(initial=0)) < 1 << 42
    cu2 = np.float64(1.0) / np.float64(looks)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = S1.astype(np.float64) / np.float64(28.0)
        q = (cu2 * A.astype(np.float64)) / D.astype(np.float64)
        w = np.float64(1.0) - q
        w = np.where(w > 0, w, np.float64(0.0))
        o = m + w * (v.astype(np.float64) - m)
        o = np.where(D > 0, o, m).astype(np.float32)
    out[directed] = o[directed]
    if not info:
        return out
    gs = np.sort(g, axis=0)
    return out, {"directed": directed, "half": np.where(directed, half, -1), "ties": int(((gs[3] == gs[2]) & directed).sum()),
                 "m": np.where(directed, m, np.nan)}


def speckle_ext_u16(v, filt, window, looks, damping):
    if filt == FROST:
        return frost_u16(v, window, damping)
    if filt == REFINED_LEE:
        assert window == 7
        return refined_lee_u16(v, looks)
    return speckleref.speckle_u16(v, filt, window, looks)


# ---------------------------------------------------------------------------- the test scene
SCENE_SEED = 7


def scene(rows, cols, band=0):
    """synth.scene_u16 with 0.2 % scattered zeros (few enough that most 7 x 7 windows stay fully valid), rows 0-2 and columns 0-3
    zeroed (a black-fill border), one zero 9 x 9 block around a single valid sample, and 65535 in the last corner"""
    a = synth.scene_u16(rows, cols, band).copy()
    rng = np.random.default_rng(SCENE_SEED + 1000 * band + rows + cols)
    a[rng.random(a.shape) < 0.002] = 0
    a[: min(3, rows - 1), :] = 0
    a[:, : min(4, cols - 1)] = 0
    r1, c1 = rows // 2 + 3, cols // 2 + 1
    a[r1:r1 + 9, c1:c1 + 9] = 0
    if r1 + 4 < rows and c1 + 4 < cols:
        a[r1 + 4, c1 + 4] = 4321
    a[rows - 1, cols - 1] = 65535
    a.setflags(write=False)
    return a
