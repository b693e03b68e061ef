"""The scenes of tests/undercutscenes.py are on the cases the GPU tests use them for (CPU oracle only, no GPU).

tests/test_gpu_spec_chain.py, test_gpu_multirank_local.py and test_gpu_resident_batch.py run these scenes without any SPEC_FORCE and
assert the path the device takes.  Which path that is follows from the oracle's levels on and off the sampled rows; a change to the
oracle or to the generators that moves a scene off its case fails here, on a machine without a GPU, instead of letting a GPU test
pass on another path."""
import numpy as np
import pytest

import undercutscenes as U

ONE_DEVICE = [(264, 520), (1000, 777)]  # tests/test_gpu_spec_chain.py (the resident batch uses the first)
STRIPES = (403, 520)                    # tests/test_gpu_multirank_local.py
STRIPE_CASES = ("to_zero_proven", "to_nonzero")
USED = [(case, shape) for shape in ONE_DEVICE for case in U.CASES] + [(case, STRIPES) for case in STRIPE_CASES]


def check_band(kind, f):
    assert f["has255_sampled"], f  # the rescale's upper end is proven from the sample in every case
    if kind == "proven":
        assert f["true_min"] == 0 and (f["n_invalid"] > 0 or f["sampled_min"] == 0), f
        return
    assert f["n_invalid"] == 0, f  # an invalid pixel is level 0 and proves it: nothing would be predicted
    if kind == "plain":
        assert 0 < f["true_min"] == f["sampled_min"] <= 127 and f["n_below"] == 0, f
    elif kind == "zero":
        assert f["true_min"] == 0 < f["sampled_min"] <= 127 and f["n_below"] > 0, f
    elif kind == "nonzero":
        assert 0 < f["true_min"] < f["sampled_min"] <= 127 and f["n_below"] > 0, f
    elif kind == "untracked":
        assert f["true_min"] < f["sampled_min"] and f["sampled_min"] > 127 and f["n_below"] > 0, f
    else:
        raise ValueError(kind)


@pytest.mark.parametrize("case,shape", USED)
def test_scene_is_on_its_case(case, shape):
    bands = U.scene(case, shape)
    for kind, x in zip(U.KINDS[case], bands):
        assert x.shape == shape and x.dtype == np.uint16
        f = U.facts(x, U.STRIDE)
        check_band(kind, f)
        if kind in ("zero", "nonzero"):  # the planted pixels lie off the sampled rows, and nothing else undercuts
            assert all(r % U.STRIDE != U.STRIDE // 2 for r in f["below_rows"]), f
    # the un-planted twin (the GPU tests run it between two runs of the planted scene): the same bands but for the planted pixels
    twins = U.scene(case, shape, planted=False)
    for kind, x, y in zip(U.KINDS[case], bands, twins):
        differ = int((x != y).sum())
        assert (differ == 0) == (kind in ("proven", "plain")), (kind, differ)
        assert y.min() > 0 or kind == "proven"


@pytest.mark.parametrize("case", STRIPE_CASES)
def test_stripes_scene_keeps_its_dark_pixels_in_few_stripes(case):
    """Row stripes: the levels below the prediction are met by some ranks only, the others learn of them through the all-reduced
    presence counts (below_hist).  The rows that hold them lie in the upper half of the scene and below the first five rows: with 2
    or 8 equal stripes the last rank holds none, nor do the 5-row and the 97-row stripe of the ragged split."""
    rows = STRIPES[0]
    f = U.facts(U.scene(case, STRIPES)[0], U.STRIDE)
    br = f["below_rows"]
    assert len(br) > 0 and br.min() >= 5 and br.max() < rows // 2, br
