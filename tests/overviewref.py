"""The overview pyramid of DESIGN.md 9g, restated in plain numpy (no library calls): the definition the device pass
(sarpro_amd/csrc/overview_kernels.hip) and its host twin (sarpro_hip_host_overviews) are checked against, byte for byte.

    rasters   (rows, cols, components) uint8 / uint16, components 1..3
    shapes    level 0 is the raster; level k has w_k = ceil(w_{k-1} / 2), h_k = ceil(h_{k-1} / 2)
    levels    the smallest L >= 0 with max(w_L, h_L) <= min_size (0 means 512), at most 16
    a pixel   of level k, per component: (sum + n // 2) // n over the n in {1, 2, 4} samples of the ROUNDED level k - 1 at rows
              2i, 2i + 1 and columns 2j, 2j + 1 that exist
    SKIP_ZERO a source pixel takes part only if one of its components is non-zero; n = 0 gives 0 in every component

Parity with GDAL's AVERAGE overviews is unpinned (GDAL is absent; it takes fractional source windows at odd sizes)."""
import numpy as np

MAX_LEVELS = 16
SKIP_ZERO = 1


def level_shapes(cols, rows, min_size=0):
    """[(cols_k, rows_k) for k = 1..L]"""
    m = min_size or 512
    out, w, h = [], cols, rows
    while max(w, h) > m and len(out) < MAX_LEVELS:
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def plan(cols, rows, components, bits, min_size=0):
    """The packed buffer of levels 1..L: [(cols, rows, pitch_bytes, offset_bytes)], total_bytes.  Pitches are row bytes rounded up to
    16, offsets are rounded up to 256."""
    px = components * bits // 8
    out, off, end = [], 0, 0
    for w, h in level_shapes(cols, rows, min_size):
        pitch = (w * px + 15) // 16 * 16
        out.append((w, h, pitch, off))
        end = off + h * pitch
        off = (end + 255) // 256 * 256
    return out, end


def next_level(a, skip_zero=False):
    """(rows, cols, C) -> (ceil(rows / 2), ceil(cols / 2), C) of the same dtype"""
    h, w, c = a.shape
    nh, nw = (h + 1) // 2, (w + 1) // 2
    v = np.zeros((2 * nh, 2 * nw, c), np.int64)
    v[:h, :w] = a
    exists = np.zeros((2 * nh, 2 * nw), bool)
    exists[:h, :w] = True
    take = exists & (v.any(axis=2) if skip_zero else True)
    s = np.zeros((nh, nw, c), np.int64)
    n = np.zeros((nh, nw), np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            t = take[dy::2, dx::2]
            s += v[dy::2, dx::2] * t[..., None]
            n += t
    nn = np.maximum(n, 1)[..., None]
    return np.where(n[..., None] > 0, (s + nn // 2) // nn, 0).astype(a.dtype)


def overviews(raster, min_size=0, skip_zero=False):
    """[level 1, ..., level L] as (rows_k, cols_k, C) arrays"""
    a = raster if raster.ndim == 3 else raster[..., None]
    out = []
    for _ in level_shapes(a.shape[1], a.shape[0], min_size):
        a = next_level(a, skip_zero)
        out.append(a)
    return out


def pack(levels, cols, rows, bits, min_size=0, fill=0xA5):
    """The levels in the packed layout, every byte no level owns = fill -> uint8 buffer"""
    c = levels[0].shape[2] if levels else 1
    lay, total = plan(cols, rows, c, bits, min_size)
    buf = np.full(total, fill, np.uint8)
    for lv, (w, h, pitch, off) in zip(levels, lay):
        rb = np.ascontiguousarray(lv).view(np.uint8).reshape(h, -1)
        for r in range(h):
            buf[off + r * pitch: off + r * pitch + rb.shape[1]] = rb[r]
    return buf


def wedge_raster(rows, cols, components, dtype, seed):
    """Random samples with a zero wedge over about 30 % of the raster (this project's no-data shape), a few isolated zero pixels and
    some zero components inside valid pixels"""
    rng = np.random.default_rng(seed)
    hi = 256 if dtype == np.uint8 else 65536
    a = rng.integers(0, hi, (rows, cols, components)).astype(dtype)
    yy, xx = np.mgrid[0:rows, 0:cols]
    a[(xx * rows + yy * cols * 0.6) < 0.6 * rows * cols] = 0  # the triangle x / cols + 0.6 y / rows < 0.6: 30 % of the area
    a[rng.random((rows, cols)) < 0.02] = 0
    a[rng.random((rows, cols, components)) < 0.02] = 0
    return a
