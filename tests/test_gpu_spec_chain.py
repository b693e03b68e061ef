"""GPU parity of the speculative CLAHE chain (whole dual-pol u8 scene on one device).

The apply pass counts its level histogram on sampled rows only; k_chain_predict proves from the sample that the u8 rescale
(autoscale.rs:348-364) is the identity and predicts the suppressed-synRGB floor (synthetic_rgb.rs:99-113); the compose pass
composes with the prediction and verifies it exactly; refuted (or unproven), the gated recount -> finish -> compose run.
Whatever the route, the raster must be the oracle's, bit for bit.  SARPRO_HIP_SAMPLED_HIST_MIN_PX=0 takes the route on the
small rasters the oracle can check (the product only takes it from 32 MP on); SARPRO_HIP_SPEC_FORCE forces the rare branches.
"""
import numpy as np
import pytest
import torch

import oracle
import undercutscenes as U
from sarpro_amd import AutoscaleStrategy as St, SyntheticRgbMode as Mode
from sarpro_amd import synth
import sarpro_amd as S

pytestmark = pytest.mark.gpu


def run(c, b1, b2):
    rgb, u1, u2 = c.dualpol_synrgb(b1, b2, St.Clahe, want_u8=True)
    names = [n for n, _ in c.last_kernel_times()]
    return rgb, u1, u2, names


def run_rgb_only(c, b1, b2):
    """No per-band outputs requested: the chain takes the fused CLAHE -> RGB pass (no level rasters)."""
    rgb = c.dualpol_synrgb(b1, b2, St.Clahe)
    return rgb, [n for n, _ in c.last_kernel_times()]


def ref(b1, b2):
    rc, rrgb, r1, r2 = oracle.dualpol_synrgb(b1.astype(np.float32), b2.astype(np.float32), int(St.Clahe))
    assert rc == 0
    return rrgb, r1, r2


@pytest.mark.parametrize("shape", [(264, 512), (512, 640), (1000, 777), (300, 4100), (2000, 1500)])
@pytest.mark.parametrize("seed", [0, 5])
def test_speculative_chain_matches_oracle(shape, seed, monkeypatch):
    rows, cols = shape
    monkeypatch.setenv("SARPRO_HIP_SAMPLED_HIST_MIN_PX", "0")
    b1, b2 = synth.scene_u16(rows, cols, 0, seed=synth.SEED_SCENE_A + seed), synth.scene_u16(rows, cols, 1, seed=synth.SEED_SCENE_A + seed)
    rrgb, r1, r2 = ref(b1, b2)
    with S.Context(0, timing=True) as c:
        rgb, u1, u2, names = run(c, b1, b2)
        rep = c.spec_report()
    assert "chain_predict" in names and "level_hist_guard" not in names
    assert np.array_equal(u1, r1) and np.array_equal(u2, r2) and np.array_equal(rgb, rrgb), rep
    if rep["spec_ok"] and rep["verdict"] == 0:  # an accepted floor is the reference's floor: the counts bracket the target
        f = rep["floor_pred"]
        assert f == 37 or rep["n_lt"][0] < rep["target"] <= rep["n_lt"][1]
        lv = np.concatenate([r1.ravel(), r2.ravel()])
        assert rep["n_lt"][0] == int((lv < f).sum()) and (f == 37 or rep["n_lt"][1] == int((lv <= f).sum()))


@pytest.mark.parametrize("force", ["mispredict", "nospec", "mispredict,nospec"])
def test_speculative_chain_forced_fallbacks(force, monkeypatch):
    """A floor that is wrong by one must be refuted by the compose pass's counts; without the identity proof no speculative
    composition may run at all.  Both end in the exact kernels and the oracle's raster."""
    rows, cols = 700, 1100
    monkeypatch.setenv("SARPRO_HIP_SAMPLED_HIST_MIN_PX", "0")
    monkeypatch.setenv("SARPRO_HIP_SAMPLE_STRIDE", "5")
    b1, b2 = synth.scene_u16(rows, cols, 0), synth.scene_u16(rows, cols, 1)
    rrgb, r1, r2 = ref(b1, b2)
    with S.Context(0, timing=True) as c:
        rgb, u1, u2, _ = run(c, b1, b2)  # unforced first: the state of an accepted scene must not leak into the next
        assert np.array_equal(rgb, rrgb)
        monkeypatch.setenv("SARPRO_HIP_SPEC_FORCE", force)
        rgb, u1, u2, names = run(c, b1, b2)
        rep = c.spec_report()
        assert rep["verdict"] == 1 and rep["spec_ok"] == (0 if "nospec" in force else 1), rep
        assert np.array_equal(u1, r1) and np.array_equal(u2, r2) and np.array_equal(rgb, rrgb), rep
        monkeypatch.delenv("SARPRO_HIP_SPEC_FORCE")
        rgb, u1, u2, _ = run(c, b1, b2)  # and back
        assert np.array_equal(u1, r1) and np.array_equal(u2, r2) and np.array_equal(rgb, rrgb)


@pytest.mark.parametrize("kind", ["two_values", "high_plateau", "constant", "no_invalid", "all_invalid_band", "bright_only"])
def test_rasters_whose_sample_lacks_level_0_or_255(kind, monkeypatch):
    """No identity proof (a band without level 0 or without level 255) => spec_ok = 0 and the exact kernels decide the rescale.  A band
    without a single valid sample is level 0 everywhere (autoscale.rs:466-468) and its u8 rescale is the identity by autoscale.rs:356
    (max == min): nothing needs a sample to be proven there, the speculation stands on the other band's proof (round 5)."""
    monkeypatch.setenv("SARPRO_HIP_SAMPLED_HIST_MIN_PX", "0")
    rng = np.random.default_rng(11)
    rows, cols = 264, 512
    lacks = True
    if kind == "two_values":      # two populated bins: levels ~127 and 255 only
        b1 = rng.choice(np.array([120, 4000], np.uint16), size=(rows, cols))
        b2 = rng.choice(np.array([300, 900], np.uint16), size=(rows, cols))
    elif kind == "high_plateau":  # 80 % of the pixels in the lowest bin: its CDF foot is already at ~0.8
        b1 = np.where(rng.random((rows, cols)) < 0.8, 50, rng.integers(51, 6000, (rows, cols))).astype(np.uint16)
        b2 = np.where(rng.random((rows, cols)) < 0.5, 70, rng.integers(71, 3000, (rows, cols))).astype(np.uint16)
    elif kind == "constant":
        b1 = np.full((rows, cols), 777, np.uint16)
        b2 = np.full((rows, cols), 12, np.uint16)
    elif kind == "all_invalid_band":
        b1 = np.zeros((rows, cols), np.uint16)
        b2 = synth.scene_u16(rows, cols, 1)
        lacks = False
    elif kind == "bright_only":   # wide DN range, no invalid pixel: level 0 only where a tile's first bin is nearly empty
        b1 = rng.integers(1, 60000, (rows, cols)).astype(np.uint16)
        b2 = rng.integers(200, 9000, (rows, cols)).astype(np.uint16)
        lacks = None
    else:                         # natural scene without its no-data wedge
        b1, b2 = np.maximum(synth.scene_u16(rows, cols, 0), 1), np.maximum(synth.scene_u16(rows, cols, 1), 1)
        lacks = None
    rrgb, r1, r2 = ref(b1, b2)
    with S.Context(0, timing=True) as c:
        rgb, u1, u2, _ = run(c, b1, b2)
        rep = c.spec_report()
    assert np.array_equal(u1, r1) and np.array_equal(u2, r2) and np.array_equal(rgb, rrgb), (kind, rep)
    if lacks:
        assert rep["spec_ok"] == 0 and rep["verdict"] == 1, rep
    if kind == "all_invalid_band":
        assert rep["spec_ok"] == 1 and rep["verdict"] == 0 and rep["floor_pred"] == 0, rep  # half of the band-pixels sit at level 0: floor 0


@pytest.mark.parametrize("stride", [5, 7, 9, 13, 64])
def test_every_sample_stride_gives_the_same_raster(stride, monkeypatch):
    rows, cols = 900, 1300
    monkeypatch.setenv("SARPRO_HIP_SAMPLED_HIST_MIN_PX", "0")
    monkeypatch.setenv("SARPRO_HIP_SAMPLE_STRIDE", str(stride))
    b1, b2 = synth.scene_u16(rows, cols, 0), synth.scene_u16(rows, cols, 1)
    rrgb, r1, r2 = ref(b1, b2)
    with S.Context(0, timing=True) as c:
        rgb, u1, u2, _ = run(c, b1, b2)
        rep = c.spec_report()
    assert np.array_equal(u1, r1) and np.array_equal(u2, r2) and np.array_equal(rgb, rrgb), rep
    for k, b in enumerate((b1, b2)):  # the stratum the estimate is scaled by: the sampled rows' valid pixels, each work item's
        # count weighted by rows / sampled rows (fixed point, 4096 = 1.0), estimate the band's valid pixels
        valid = int((b != 0).sum())
        if stride > 16:  # work items of this small raster are 16 rows tall: most hold no sampled row and go unrepresented
            continue
        assert abs(rep["sample_valid"][k] / 4096.0 - valid) <= 0.06 * valid + stride * cols, (k, rep["sample_valid"][k] / 4096.0, valid)


def test_sampled_route_equals_partial_and_full_histogram_routes(monkeypatch):
    """Three routes to the same raster: sampled histogram + speculative composition (default from 32 MP on),
    SARPRO_HIP_NO_SAMPLED_HIST=1 (partial histogram of every row), SARPRO_HIP_FULL_LEVEL_HIST=1."""
    rows, cols = 6000, 6016  # 36 MP: the product's own threshold
    pitch = cols
    q = synth.q_tables()
    with S.Context(0, timing=True) as c:
        band = [torch.empty((rows, pitch), dtype=torch.int16, device="cuda") for _ in range(2)]
        for b in range(2):
            c.dev_synth_scene_u16(synth.SEED_SCENE_A + 3, b, q, rows, cols, 0, rows, band[b].data_ptr(), pitch)
        out = []
        for env in ({}, {"SARPRO_HIP_NO_SAMPLED_HIST": "1"}, {"SARPRO_HIP_FULL_LEVEL_HIST": "1"}, {"SARPRO_HIP_SPEC_FORCE": "mispredict"}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            rgb = torch.zeros((rows, pitch * 3), dtype=torch.uint8, device="cuda")
            c.dev_dualpol_synrgb_u16(band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, St.Clahe, Mode.Default, rgb.data_ptr(), pitch)
            names = [n for n, _ in c.last_kernel_times()]
            assert ("chain_predict" in names) == (not env or "SARPRO_HIP_SPEC_FORCE" in env), (env, names)
            for k in env:
                monkeypatch.delenv(k)
            out.append(rgb)
        assert int(out[0].max().item()) > 0
        for o in out[1:]:
            assert torch.equal(out[0], o)


# ---------------------------------------------------------------------------- the fused CLAHE -> RGB pass (RGB only requested)
@pytest.mark.parametrize("shape", [(264, 512), (512, 640), (1000, 777), (300, 4100), (2000, 1500), (700, 1100)])
@pytest.mark.parametrize("seed", [0, 5])
def test_fused_rgb_pass_matches_oracle(shape, seed, monkeypatch):
    rows, cols = shape
    monkeypatch.setenv("SARPRO_HIP_SAMPLED_HIST_MIN_PX", "0")
    monkeypatch.setenv("SARPRO_HIP_SAMPLE_STRIDE", "5")
    b1, b2 = synth.scene_u16(rows, cols, 0, seed=synth.SEED_SCENE_A + seed), synth.scene_u16(rows, cols, 1, seed=synth.SEED_SCENE_A + seed)
    rrgb, r1, r2 = ref(b1, b2)
    with S.Context(0, timing=True) as c:
        rgb, names = run_rgb_only(c, b1, b2)
        rep = c.spec_report()
    assert "clahe_rgb_fused" in names and "clahe_sample" in names
    assert np.array_equal(rgb, rrgb), (rep, int((rgb != rrgb).sum()))
    if rep["spec_ok"] and rep["verdict"] == 0:
        f = rep["floor_pred"]
        lv = np.concatenate([r1.ravel(), r2.ravel()])
        assert rep["n_lt"][0] == int((lv < f).sum()) and (f == 37 or rep["n_lt"][1] == int((lv <= f).sum()))


@pytest.mark.parametrize("force", ["", "mispredict", "mispredict,noretry", "mispredict2", "nospec"])
def test_fused_rgb_pass_fallbacks(force, monkeypatch):
    """Refuted floor / no identity proof: the gated apply -> finish -> compose kernels produce the raster; accepted: they do nothing.
    A floor that is off by one gets ONE second fused pass with the floor the first pass's counts point to (round 6: `retried`); off by
    two, or with SPEC_FORCE = noretry, the exact kernels.  Three scenes in a row on one context: the state of one must not leak into the next."""
    rows, cols = 900, 1300
    monkeypatch.setenv("SARPRO_HIP_SAMPLED_HIST_MIN_PX", "0")
    monkeypatch.setenv("SARPRO_HIP_SAMPLE_STRIDE", "5")
    b1, b2 = synth.scene_u16(rows, cols, 0), synth.scene_u16(rows, cols, 1)
    rrgb, _, _ = ref(b1, b2)
    with S.Context(0, timing=True) as c:
        rgb, _ = run_rgb_only(c, b1, b2)
        assert np.array_equal(rgb, rrgb)
        if force:
            monkeypatch.setenv("SARPRO_HIP_SPEC_FORCE", force)
        rgb, names = run_rgb_only(c, b1, b2)
        rep = c.spec_report()
        assert np.array_equal(rgb, rrgb), rep
        assert "chain_repredict" in names and "clahe_rgb_fused_retry" in names, names  # (enqueued on every scene; they return at once unless armed)
        if force == "mispredict":  # the prediction of this scene is right: + 1 is refuted, the counts point back to it
            assert rep["verdict"] == 0 and rep["retried"] == 1 and rep["outcome"] == "retried" and rep["floor_pred"] == rep["floor_first"] - 1, rep
        elif force == "mispredict2":  # two off: the second pass tries + 1 and is refuted too
            assert rep["verdict"] == 1 and rep["retried"] == 1 and rep["outcome"] == "refuted", rep
        elif force:
            assert rep["verdict"] == 1 and rep["retried"] == 0, rep
        else:
            assert rep["verdict"] == 0 and rep["retried"] == 0 and rep["outcome"] == "accepted", rep
        if force:
            monkeypatch.delenv("SARPRO_HIP_SPEC_FORCE")
        rgb, _ = run_rgb_only(c, b1, b2)
        assert np.array_equal(rgb, rrgb) and c.spec_report()["outcome"] == "accepted"


def test_fused_rgb_pass_steps_aside_for_windows_beyond_its_lds_pool(monkeypatch):
    """DN windows wider than the pass's pool of DN-indexed LDS entries: the pass returns at once, the gated kernels run."""
    monkeypatch.setenv("SARPRO_HIP_SAMPLED_HIST_MIN_PX", "0")
    rng = np.random.default_rng(3)
    rows, cols = 520, 768
    b1 = rng.integers(1, 40000, (rows, cols)).astype(np.uint16)  # p99 far beyond 3072 DNs
    b2 = rng.integers(1, 30000, (rows, cols)).astype(np.uint16)
    b1[:40] = 0
    rrgb, _, _ = ref(b1, b2)
    with S.Context(0, timing=True) as c:
        rgb, names = run_rgb_only(c, b1, b2)
        rep = c.spec_report()
    assert "clahe_rgb_fused" in names and rep["verdict"] == 1
    assert np.array_equal(rgb, rrgb)


@pytest.mark.parametrize("kind", ["two_values", "constant", "all_invalid_band", "edge_heavy"])
def test_fused_rgb_pass_degenerate_rasters(kind, monkeypatch):
    monkeypatch.setenv("SARPRO_HIP_SAMPLED_HIST_MIN_PX", "0")
    rng = np.random.default_rng(11)
    rows, cols = 264, 520
    if kind == "two_values":
        b1 = rng.choice(np.array([120, 2000], np.uint16), size=(rows, cols)); b2 = rng.choice(np.array([300, 900], np.uint16), size=(rows, cols))
    elif kind == "constant":
        b1 = np.full((rows, cols), 777, np.uint16); b2 = np.full((rows, cols), 12, np.uint16)
    elif kind == "all_invalid_band":
        b1 = np.zeros((rows, cols), np.uint16); b2 = synth.scene_u16(rows, cols, 1)
    else:  # bright saturated stretches in the extrapolating border cells
        b1 = synth.scene_u16(rows, cols, 0); b2 = synth.scene_u16(rows, cols, 1)
        b1[:40, :] = 2500; b2[:, :70] = 900; b1[-30:, -90:] = 2400
    rrgb, _, _ = ref(b1, b2)
    with S.Context(0, timing=True) as c:
        rgb, _ = run_rgb_only(c, b1, b2)
    assert np.array_equal(rgb, rrgb), kind


def _no_level0_scene(kind, rows, cols, rng):
    """Rasters without an invalid pixel whose CLAHE levels start above 0 in at least one band (few distinct DNs: every occupied bin
    of every tile is clipped and the redistributed excess lifts the CDF's foot above 1/255)."""
    few1 = np.array([90, 200, 420, 800, 1300, 1900, 2600, 3100], np.uint16)
    few2 = np.array([40, 130, 260, 500, 700, 1000], np.uint16)
    if kind == "few_values":
        return rng.choice(few1, size=(rows, cols)), rng.choice(few2, size=(rows, cols))
    if kind == "one_band":       # band 1: the natural scene with its no-data wedge (level 0 proven); band 2: no level 0
        return synth.scene_u16(rows, cols, 0), rng.choice(few2, size=(rows, cols))
    if kind == "two_values":     # levels ~127 and 255 only
        return rng.choice(np.array([120, 2000], np.uint16), size=(rows, cols)), rng.choice(np.array([300, 900], np.uint16), size=(rows, cols))
    if kind == "high_plateau":   # 80 % of the pixels in the lowest bin
        return (np.where(rng.random((rows, cols)) < 0.8, 50, rng.integers(51, 3000, (rows, cols))).astype(np.uint16),
                np.where(rng.random((rows, cols)) < 0.5, 70, rng.integers(71, 2500, (rows, cols))).astype(np.uint16))
    if kind == "constant":       # one level per band: max == min, the rescale's scale is 1.0 (autoscale.rs:356)
        return np.full((rows, cols), 777, np.uint16), np.full((rows, cols), 12, np.uint16)
    if kind == "gradient":       # few values whose mix changes across the scene: the tiles' lowest levels differ
        w = np.linspace(0.0, 1.0, cols)[None, :]
        pick = (rng.random((rows, cols)) < w)
        return (np.where(pick, rng.choice(few1[:3], size=(rows, cols)), rng.choice(few1[4:], size=(rows, cols))).astype(np.uint16),
                np.where(pick, rng.choice(few2[3:], size=(rows, cols)), rng.choice(few2[:3], size=(rows, cols))).astype(np.uint16))
    raise ValueError(kind)


@pytest.mark.parametrize("shape", [(264, 520), (1000, 777), (700, 2100)])
@pytest.mark.parametrize("kind", ["few_values", "one_band", "two_values", "high_plateau", "constant", "gradient"])
def test_fused_rgb_pass_predicts_the_rescale_of_a_band_without_level_0(kind, shape, monkeypatch):
    """A band without level 0 (a crop with no invalid pixel) has no identity proof.  Its lowest sampled level becomes a prediction:
    the rescale (min_pred, 255) of autoscale.rs:348-364 is folded into the tables, the floor is predicted on the rescaled levels and
    the fused pass counts the level bytes below min_pred beside the floor counts (spec_ok = 2).  Accepted or refuted, the raster is
    the oracle's; accepted, the counts are the oracle's final levels'."""
    rows, cols = shape
    monkeypatch.setenv("SARPRO_HIP_SAMPLED_HIST_MIN_PX", "0")
    monkeypatch.setenv("SARPRO_HIP_SAMPLE_STRIDE", "5")
    b1, b2 = _no_level0_scene(kind, rows, cols, np.random.default_rng(23))
    rrgb, r1, r2 = ref(b1, b2)
    with S.Context(0, timing=True) as c:
        rgb, names = run_rgb_only(c, b1, b2)
        rep = c.spec_report()
        assert "clahe_rgb_fused" in names
        assert np.array_equal(rgb, rrgb), (kind, rep, int((rgb != rrgb).sum()))
        if kind == "constant":  # one level per band, and it is not 255 (the clipped bin's share of the redistributed excess): level 255 is
            assert rep["spec_ok"] == 0 and rep["verdict"] == 1, rep  # what the proof of the rescale's upper end needs -- the exact kernels run
            return
        assert rep["spec_ok"] == 2 and max(rep["min_pred"]) > 0, rep
        if kind == "one_band":
            assert rep["min_pred"][0] == 0, rep
        if rep["verdict"] == 0:
            assert rep["n_below_min"] == 0
            f = rep["floor_pred"]
            lv = np.concatenate([r1.ravel(), r2.ravel()])  # the oracle's FINAL levels
            assert rep["n_lt"][0] == int((lv < f).sum()) and (f == 37 or rep["n_lt"][1] == int((lv <= f).sum())), rep
            assert f == 37 or rep["n_lt"][0] < rep["target"] <= rep["n_lt"][1]
        accepted = rep["verdict"] == 0
        # a lowest level that the raster undercuts, and a floor that is off by one: both must be refuted, and the exact kernels' raster stands
        for force in ("lowmin,noretry", "lowmin", "mispredict,noretry", "mispredict", "mispredict2"):
            c.set_attr("SPEC_FORCE", force)
            rgb, _ = run_rgb_only(c, b1, b2)
            rep2 = c.spec_report()
            assert np.array_equal(rgb, rrgb), (kind, force, rep2)
            if force == "lowmin,noretry":  # an undercut lowest level, the exact kernels (round 5's behaviour)
                assert rep2["spec_ok"] == 2 and rep2["verdict"] == 1 and rep2["n_below_min"] > 0 and rep2["retried"] == 0, rep2
            if force == "lowmin" and accepted:  # round 6: the pass records the lowest byte it met below the prediction, the second pass runs on it
                assert rep2["verdict"] == 0 and rep2["retried"] == 1 and rep2["n_below_min"] == 0 and rep2["min_pred"] == rep["min_pred"], (rep2, rep)
            if force == "mispredict,noretry" and accepted:
                assert rep2["verdict"] == 1 and rep2["retried"] == 0, rep2
            if force == "mispredict" and accepted and rep["floor_pred"] < 36:  # the rescaled form's second pass: its thresholds are rebuilt for the new floor
                assert rep2["verdict"] == 0 and rep2["retried"] == 1 and rep2["floor_pred"] == rep["floor_pred"], rep2
            if force == "mispredict2" and accepted and rep["floor_pred"] < 35:
                assert rep2["verdict"] == 1 and rep2["retried"] == 1, rep2
        c.set_attr("SPEC_FORCE", None)
        c.set_attr("NO_SPEC_RESCALE", 1)  # the round-4 behaviour: no proof, no speculation
        rgb, _ = run_rgb_only(c, b1, b2)
        rep3 = c.spec_report()
        assert np.array_equal(rgb, rrgb) and rep3["spec_ok"] == 0 and rep3["verdict"] == 1, rep3
        c.set_attr("NO_SPEC_RESCALE", None)
        rgb, _ = run_rgb_only(c, b1, b2)  # and back: nothing of the refuted scenes leaks
        assert np.array_equal(rgb, rrgb) and c.spec_report()["verdict"] == rep["verdict"]
    assert accepted or kind in ("gradient",), rep  # the simple cases are all accepted: the route is worth something


@pytest.mark.parametrize("item_rows,tail_rows,tail_item_rows", [(16, 0, 16), (48, 100, 16), (512, 2500, 128), (4096, 64, 24), (96, 100000, 32)])
def test_fused_rgb_pass_item_geometry_does_not_change_the_raster(item_rows, tail_rows, tail_item_rows, monkeypatch):
    """The pass's work list: items of RGB_ITEM_ROWS rows, the last RGB_TAIL_ROWS rows of the scene in items of RGB_TAIL_ITEM_ROWS rows, handed
    out by a device counter; inside an item the rows are handed out by an LDS counter.  Whatever the cut -- one row per wave, a tail
    longer than the scene, one item per cell -- the raster is the oracle's and the verification counts are the whole scene's."""
    rows, cols = 1000, 1300
    monkeypatch.setenv("SARPRO_HIP_SAMPLED_HIST_MIN_PX", "0")
    monkeypatch.setenv("SARPRO_HIP_SAMPLE_STRIDE", "5")
    b1, b2 = synth.scene_u16(rows, cols, 0, seed=synth.SEED_SCENE_A + 2), synth.scene_u16(rows, cols, 1, seed=synth.SEED_SCENE_A + 2)
    rrgb, r1, r2 = ref(b1, b2)
    with S.Context(0, timing=True) as c:
        c.set_attr("RGB_ITEM_ROWS", item_rows); c.set_attr("RGB_TAIL_ROWS", tail_rows); c.set_attr("RGB_TAIL_ITEM_ROWS", tail_item_rows)
        for _ in range(2):  # (twice: the counter is cleared per scene)
            rgb, names = run_rgb_only(c, b1, b2)
            rep = c.spec_report()
            assert "clahe_rgb_fused" in names and np.array_equal(rgb, rrgb), rep
            if rep["verdict"] == 0:
                f = rep["floor_pred"]
                lv = np.concatenate([r1.ravel(), r2.ravel()])
                assert rep["n_lt"][0] == int((lv < f).sum()) and (f == 37 or rep["n_lt"][1] == int((lv <= f).sum())), rep


def test_fused_rgb_route_equals_the_other_routes_at_36mp(monkeypatch):
    rows, cols = 6000, 6016
    pitch = cols
    q = synth.q_tables()
    with S.Context(0, timing=True) as c:
        band = [torch.empty((rows, pitch), dtype=torch.int16, device="cuda") for _ in range(2)]
        for b in range(2):
            c.dev_synth_scene_u16(synth.SEED_SCENE_A + 9, b, q, rows, cols, 0, rows, band[b].data_ptr(), pitch)
        out = []
        for env in ({}, {"SARPRO_HIP_NO_FUSED_RGB": "1"}, {"SARPRO_HIP_NO_SAMPLED_HIST": "1"}, {"SARPRO_HIP_SPEC_FORCE": "mispredict"}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            rgb = torch.zeros((rows, pitch * 3), dtype=torch.uint8, device="cuda")
            c.dev_dualpol_synrgb_u16(band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, St.Clahe, Mode.Default, rgb.data_ptr(), pitch)
            names = [n for n, _ in c.last_kernel_times()]
            assert ("clahe_rgb_fused" in names) == (not env or "SARPRO_HIP_SPEC_FORCE" in env), (env, names)
            if not env:
                assert c.spec_report()["verdict"] == 0  # the product's default at this size: accepted
            for k in env:
                monkeypatch.delenv(k)
            out.append(rgb)
        assert int(out[0].max().item()) > 0
        for o in out[1:]:
            assert torch.equal(out[0], o)


def test_predicted_rescale_equals_the_exact_routes_at_36mp():
    """The scene of the test above with its DNs coarsened to a dozen values and no invalid pixel left: no band holds level 0, the fused
    pass runs its rescaled form (spec_ok = 2).  Its raster against the exact kernels' (the same context with the prediction switched
    off, and without the fused pass at all), at a size where every work item shape of the pass occurs."""
    rows, cols = 6000, 6016
    pitch = cols
    q = synth.q_tables()
    with S.Context(0, timing=True) as c:
        band = [torch.empty((rows, pitch), dtype=torch.int16, device="cuda") for _ in range(2)]
        for b in range(2):
            c.dev_synth_scene_u16(synth.SEED_SCENE_A + 9, b, q, rows, cols, 0, rows, band[b].data_ptr(), pitch)
            t = band[b].to(torch.int32) & 0xFFFF
            band[b].copy_((((t >> 8) << 8) + 77 + 40 * b).clamp_(max=32767).to(torch.int16))
        torch.cuda.synchronize()
        out = []
        for attr in (None, "NO_SPEC_RESCALE", "NO_FUSED_RGB"):
            if attr:
                c.set_attr(attr, 1)
            rgb = torch.zeros((rows, pitch * 3), dtype=torch.uint8, device="cuda")
            c.dev_dualpol_synrgb_u16(band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, St.Clahe, Mode.Default, rgb.data_ptr(), pitch)
            rep = c.spec_report()
            if attr is None:
                assert rep["spec_ok"] == 2 and rep["verdict"] == 0 and rep["n_below_min"] == 0 and max(rep["min_pred"]) > 0, rep
            else:
                assert rep["spec_ok"] == 0 and rep["verdict"] == 1, (attr, rep)
                # the exact kernels' level histogram holds EVERY band-pixel (no level 0 here: bin 0 = pixels - others must come out 0,
                # or the rescale is taken for the identity -- round 5: the pass's last LDS adds were not waited for before the flush)
                cr = c.chain_report()
                assert [int(cr["level_hist"][b][1:].sum()) for b in range(2)] == [rows * cols] * 2, cr["level_hist"][:, :4]
                assert cr["identity"] == [0, 0] and cr["floor_with_cushion"] == 3 and list(cr["rescale"][0][:4]) == [0, 0, 0, 1], cr
                c.set_attr(attr, None)
            out.append(rgb)
        assert int(out[0].max().item()) > 0
        for o in out[1:]:
            assert torch.equal(out[0], o)


@pytest.mark.parametrize("kind", ["uniform", "scene", "edge_bright"])
def test_fused_rgb_pass_wide_windows_take_the_byte_table_form(kind, monkeypatch):
    """DN windows beyond the pass's pool of DN-indexed entries but within its DN -> bin byte table (3072 < windows <= 44000 DNs in
    total): the pass runs in its WIDE form -- a byte read per sample for the bin, bin-indexed entries -- instead of stepping aside."""
    monkeypatch.setenv("SARPRO_HIP_SAMPLED_HIST_MIN_PX", "0")
    monkeypatch.setenv("SARPRO_HIP_SAMPLE_STRIDE", "5")
    rng = np.random.default_rng(5)
    rows, cols = 520, 1100
    if kind == "uniform":
        b1 = rng.integers(1, 9000, (rows, cols)).astype(np.uint16); b2 = rng.integers(1, 6000, (rows, cols)).astype(np.uint16)
        b1[:30] = 0; b2[:30] = 0
    elif kind == "scene":
        q = synth.q_tables(sigma=(420.0, 260.0))
        b1, b2 = synth.scene_u16(rows, cols, 0, q=q), synth.scene_u16(rows, cols, 1, q=q)
    else:  # saturated stretches in the extrapolating border cells, invalid pixels inside them
        q = synth.q_tables(sigma=(600.0, 300.0))
        b1, b2 = synth.scene_u16(rows, cols, 0, q=q), synth.scene_u16(rows, cols, 1, q=q)
        b1[:25, :] = 14000; b2[:, :60] = 9000; b1[5:9, 100:400] = 0; b2[200:260, 10:30] = 0
    rrgb, r1, r2 = ref(b1, b2)
    with S.Context(0, timing=True) as c:
        for _ in range(2):  # (twice: the second scene finds the context's state of the first)
            rgb, names = run_rgb_only(c, b1, b2)
            rep = c.spec_report()
            assert "clahe_rgb_fused" in names and rep["pool_overflow"] == 0, rep
            assert np.array_equal(rgb, rrgb), (kind, rep, int((rgb != rrgb).sum()))
            if rep["spec_ok"] and rep["verdict"] == 0:
                f = rep["floor_pred"]
                lv = np.concatenate([r1.ravel(), r2.ravel()])
                assert rep["n_lt"][0] == int((lv < f).sum()) and (f == 37 or rep["n_lt"][1] == int((lv <= f).sum()))


# ---------------------------------------------------------------------------- a lowest level that occurs only OFF the sampled rows
# (tests/undercutscenes.py; tests/test_undercut_scenes.py pins on the CPU that every scene is on its case).  No SPEC_FORCE: the level
# the pass records below the prediction differs from the sampled one, min_pred changes between the passes and spec_ok may too.
def _check_undercut_report(case, rep, facts, finals):
    """The report the device must give for a scene of `case`; facts = undercutscenes.facts per band, finals = the oracle's FINAL levels."""
    kinds = U.KINDS[case]
    if "untracked" in kinds:  # a prediction above 127 has no record: min_known is false whatever the other band recorded, the exact kernels run
        k = kinds.index("untracked")
        assert rep["spec_ok"] == 2 and rep["min_pred"][k] > 127, rep  # (the scene IS on the rescaled form with an untracked band)
        assert rep["verdict"] == 1 and rep["retried"] == 0 and rep["n_below_min"] > 0, rep
        return
    want = [0 if kind == "proven" else f["true_min"] for kind, f in zip(kinds, facts)]  # the second pass runs on the TRUE lowest levels
    assert rep["retried"] == 1 and rep["min_pred"] == want and rep["n_below_min"] == 0, (rep, want)
    assert rep["spec_ok"] == (1 if want == [0, 0] else 2), (rep, want)
    for kind, m in zip(kinds, want):
        assert (m > 0) == (kind in ("nonzero", "plain")), (kinds, want)
    assert rep["verdict"] == 0 and rep["outcome"] == "retried", rep
    f = rep["floor_pred"]
    lv = np.concatenate([x.ravel() for x in finals])
    assert rep["n_lt"][0] == int((lv < f).sum()) and (f == 37 or rep["n_lt"][1] == int((lv <= f).sum())), rep
    assert f == 37 or rep["n_lt"][0] < rep["target"] <= rep["n_lt"][1], rep


@pytest.mark.parametrize("shape", [(264, 520), (1000, 777)])
@pytest.mark.parametrize("case", U.CASES)
def test_fused_rgb_pass_second_chance_on_a_natural_undercut(case, shape, monkeypatch):
    """The fused pass finds level bytes below the predicted lowest level of a band, records the lowest of them, k_chain_predict runs again
    on that level and the retry kernel recomposes: Rescaled -> Identity when the true minimum is 0 and the other band holds level 0
    (the retry kernel's identity body behind a first pass in the rescaled body; tables, thresholds, identity_out and resc_out rebuilt
    for another rescale), Rescaled -> Rescaled with another min_pred otherwise.  A band whose prediction lies above 127 is not tracked:
    the exact kernels.  Then the un-planted twin and the planted scene again on the same context: nothing of the retry leaks."""
    monkeypatch.setenv("SARPRO_HIP_SAMPLED_HIST_MIN_PX", "0")
    monkeypatch.setenv("SARPRO_HIP_SAMPLE_STRIDE", str(U.STRIDE))
    b1, b2 = U.scene(case, shape)
    t1, t2 = U.scene(case, shape, planted=False)
    facts = [U.facts(b, U.STRIDE) for b in (b1, b2)]
    rrgb, r1, r2 = ref(b1, b2)
    trgb, _, _ = ref(t1, t2)
    with S.Context(0, timing=True) as c:
        rgb, names = run_rgb_only(c, b1, b2)
        rep = c.spec_report()
        print("\nundercut", case, shape, {k: rep[k] for k in ("spec_ok", "verdict", "retried", "min_pred", "floor_pred", "floor_first", "n_below_min", "n_lt", "target")})
        assert "clahe_rgb_fused" in names and "clahe_rgb_fused_retry" in names, names
        assert np.array_equal(rgb, rrgb), (case, rep, int((rgb != rrgb).sum()))
        _check_undercut_report(case, rep, facts, (r1, r2))
        rgb, _ = run_rgb_only(c, t1, t2)
        rept = c.spec_report()
        assert np.array_equal(rgb, trgb), (case, rept, int((rgb != trgb).sum()))
        rgb, _ = run_rgb_only(c, b1, b2)
        rep2 = c.spec_report()
        assert np.array_equal(rgb, rrgb), (case, rep2, int((rgb != rrgb).sum()))
        _check_undercut_report(case, rep2, facts, (r1, r2))
        assert all(rep2[k] == rep[k] for k in ("spec_ok", "verdict", "retried", "min_pred", "floor_pred", "floor_first", "n_lt", "n_below_min")), (rep, rep2)


def test_fused_rgb_pass_natural_undercut_without_the_second_chance(monkeypatch):
    """SPEC_FORCE = noretry on the Rescaled -> Identity scene: the undercut refutes, no second prediction, the exact kernels."""
    monkeypatch.setenv("SARPRO_HIP_SAMPLED_HIST_MIN_PX", "0")
    monkeypatch.setenv("SARPRO_HIP_SAMPLE_STRIDE", str(U.STRIDE))
    monkeypatch.setenv("SARPRO_HIP_SPEC_FORCE", "noretry")
    b1, b2 = U.scene("to_zero_proven", (264, 520))
    rrgb, _, _ = ref(b1, b2)
    with S.Context(0, timing=True) as c:
        rgb, names = run_rgb_only(c, b1, b2)
        rep = c.spec_report()
        print("\nundercut noretry", rep)
        assert "clahe_rgb_fused" in names and np.array_equal(rgb, rrgb), rep
        assert rep["verdict"] == 1 and rep["retried"] == 0 and rep["spec_ok"] == 2 and rep["n_below_min"] > 0 and rep["min_pred"][0] > 0, rep


def test_fused_rgb_pass_natural_undercut_with_a_wrong_floor(monkeypatch):
    """SPEC_FORCE = mispredict on the Rescaled -> Identity scene: an undercut and a floor that is one too high coincide.  The undercut
    decides the first verdict (retry_floor stays -1: k_chain_repredict returns), the second k_chain_predict launch shifts its floor by
    one as well and the one second pass runs on it.  Two endings are legal: the shifted floor is refuted (verdict 1, retried 1: the
    exact kernels produced the raster), or the sample's estimate was one too low and the shift made it right (verdict 0, retried 1,
    the oracle's counts).  Either way the second pass ran on the true lowest levels, and the raster is the oracle's.
    Observed on an MI355X: the first ending -- floor_first 2, the second pass on floor 3 refuted (n_lt = [22283, 22296] above the target
    13728), verdict 1, retried 1, spec_ok 1, min_pred [0, 0]."""
    monkeypatch.setenv("SARPRO_HIP_SAMPLED_HIST_MIN_PX", "0")
    monkeypatch.setenv("SARPRO_HIP_SAMPLE_STRIDE", str(U.STRIDE))
    monkeypatch.setenv("SARPRO_HIP_SPEC_FORCE", "mispredict")
    b1, b2 = U.scene("to_zero_proven", (264, 520))
    rrgb, r1, r2 = ref(b1, b2)
    with S.Context(0, timing=True) as c:
        rgb, names = run_rgb_only(c, b1, b2)
        rep = c.spec_report()
        print("\nundercut mispredict", rep)
        assert "clahe_rgb_fused" in names and np.array_equal(rgb, rrgb), rep
        assert rep["retried"] == 1 and rep["spec_ok"] == 1 and rep["min_pred"] == [0, 0] and rep["n_below_min"] == 0, rep
        assert rep["verdict"] in (0, 1), rep
        if rep["verdict"] == 0:
            f = rep["floor_pred"]
            lv = np.concatenate([r1.ravel(), r2.ravel()])
            assert rep["n_lt"][0] == int((lv < f).sum()) and (f == 37 or rep["n_lt"][1] == int((lv <= f).sum())), rep
