"""Scenes whose lowest CLAHE level occurs only OFF the rows the speculative chain samples (test support, numpy + the CPU oracle).

The fused CLAHE -> RGB pass predicts a band's lowest level from the sampled rows (row r of the scene is sampled iff r % stride ==
stride // 2: kernels.h ClaheApplyArgs::sample_stride, api_u16_chain.cpp) and counts every level byte below the prediction.  A band
built here undercuts that prediction NATURALLY -- no SPEC_FORCE -- so the pass's record of the true lowest level (true_min,
below_hist), the second k_chain_predict launch and the retry kernel run on a minimum that differs from the sampled one.

"Levels" are the oracle's u8 levels BEFORE the u8 rescale (oracle.clahe_levels_u8), which is what the device's sample counts.
tests/test_undercut_scenes.py pins, on the CPU, that every scene the GPU tests use is on the case it is used for.
"""
import numpy as np

import oracle

STRAT_CLAHE = 4  # types.rs:115-123
FEW = (np.array([90, 200, 420, 800, 1300, 1900, 2600, 3100], np.uint16),  # as tests/test_gpu_spec_chain.py::_no_level0_scene: every
       np.array([40, 130, 260, 500, 700, 1000], np.uint16))               # occupied bin is clipped, the CDF's foot lies above 1/255


def few_band(shape, band, seed=23):
    """The plain few-valued band (no level 0, nothing undercut: its lowest level is on every row)."""
    return np.random.default_rng(seed + band).choice(FEW[band], size=shape)


def undercut_band(shape, band, ndark, stride, seed=23):
    """A few-valued band with a block of 2 x 2 CLAHE tiles (tile = rows // 8 x cols // 8, the block starts at tile (2, 2)) of a wide
    distribution, uniform in [max(few) // 8, max(few)): inside it the CDF starts low.  `ndark` pixels in [min(few) // 4, min(few) // 2)
    are planted at random places of the block's inner half, on rows the device does not sample: they alone take the lowest level."""
    rows, cols = shape
    few = FEW[band]
    rng = np.random.default_rng(seed + band)
    x = rng.choice(few, size=shape)
    th, tw = rows // 8, cols // 8
    r0, c0 = 2 * th, 2 * tw
    x[r0:r0 + 2 * th, c0:c0 + 2 * tw] = rng.integers(int(few.max()) // 8, int(few.max()), (2 * th, 2 * tw)).astype(np.uint16)
    cand = np.array([(r, c) for r in range(r0 + th // 2, r0 + 2 * th - th // 2) if r % stride != stride // 2
                     for c in range(c0 + tw // 2, c0 + 2 * tw - tw // 2)])
    pick = cand[rng.choice(len(cand), size=ndark, replace=False)]
    x[pick[:, 0], pick[:, 1]] = rng.integers(int(few.min()) // 4, int(few.min()) // 2, ndark).astype(np.uint16)
    return x


def untracked_band(shape, stride, seed=3, plant=True):
    """Two values, the sampled rows all at the upper one: the sample holds the two highest levels only, the prediction lies above 127
    (the pass tracks undercuts of predictions <= 127 only: its byte test has seven bits), every other row undercuts it."""
    rows, _ = shape
    x = np.random.default_rng(seed).choice(np.array([120, 2000], np.uint16), size=shape)
    if plant:
        x[np.arange(rows) % stride == stride // 2] = 2000
    return x


STRIDE = 5
# planted pixels of the "to nonzero" scene per shape: enough of them that their level's CDF value rounds to 1, not to 0, and few
# enough that the planted bin stays below the block's own (measured with facts(); pinned by tests/test_undercut_scenes.py)
NDARK_NONZERO = {(264, 520): 40, (403, 520): 80, (1000, 777): 300}
CASES = ("to_zero_proven", "to_zero_rescaled", "to_nonzero", "both", "swapped", "untracked", "tracked+untracked")


def scene(case, shape, planted=True, stride=STRIDE):
    """(band 1, band 2) of a named case; planted = False: the same scene without what undercuts the prediction."""
    from sarpro_amd import synth
    n3 = 3 if planted else 0
    natural = lambda: synth.scene_u16(shape[0], shape[1], 1)  # its no-data wedge proves level 0
    if case == "to_zero_proven":      # Rescaled -> Identity on the retry
        return undercut_band(shape, 0, n3, stride), natural()
    if case == "to_zero_rescaled":    # Rescaled -> Rescaled, min_pred[0] 1 -> 0
        return undercut_band(shape, 0, n3, stride), few_band(shape, 1)
    if case == "to_nonzero":          # Rescaled -> Rescaled, min_pred[0] 2 -> 1
        return undercut_band(shape, 0, NDARK_NONZERO[shape] if planted else 0, stride), few_band(shape, 1)
    if case == "both":                # an undercut in each band; both to 0: Rescaled -> Identity
        return undercut_band(shape, 0, n3, stride), undercut_band(shape, 1, n3, stride)
    if case == "swapped":             # "to_zero_proven" with the bands exchanged
        return natural(), undercut_band(shape, 0, n3, stride)
    if case == "untracked":           # a prediction above 127: no record, the exact kernels
        return untracked_band(shape, stride, plant=planted), few_band(shape, 1)
    if case == "tracked+untracked":   # a good record in band 1 must not stand in for the missing one of band 2
        return undercut_band(shape, 0, n3, stride), untracked_band(shape, stride, plant=planted)
    raise ValueError(case)


# per case and band: "zero" / "nonzero" = an undercut down to level 0 / to a level above 0, "untracked", "plain" (no level 0, nothing
# undercut), "proven" (level 0 is on the sampled rows or the band has invalid pixels)
KINDS = {"to_zero_proven": ("zero", "proven"), "to_zero_rescaled": ("zero", "plain"), "to_nonzero": ("nonzero", "plain"),
         "both": ("zero", "zero"), "swapped": ("proven", "zero"), "untracked": ("untracked", "plain"),
         "tracked+untracked": ("zero", "untracked")}


def facts(x, stride):
    """What the speculative chain meets in band `x` at this sample stride (levels before the u8 rescale)."""
    lv = oracle.clahe_levels_u8(x.astype(np.float32), STRAT_CLAHE)
    sampled = lv[np.arange(x.shape[0]) % stride == stride // 2]
    smin = int(sampled.min())
    below = lv < smin
    return {"true_min": int(lv.min()),                      # the band's lowest level
            "sampled_min": smin,                            # the lowest level on the sampled rows: the device's prediction
            "n_below": int(below.sum()),                    # pixels below the prediction
            "n_at_min": int((lv == lv.min()).sum()),
            "has255_sampled": bool((sampled == 255).any()),  # the proof of the rescale's upper end
            "below_rows": np.flatnonzero(below.any(axis=1)),  # the rows that hold those pixels
            "n_invalid": int((x == 0).sum())}
