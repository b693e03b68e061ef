#!/usr/bin/env python3
"""Frost and Refined Lee on the device (k_speckle_frost_u16, k_speckle_rlee_u16) on one MI355X: kernel times from the
context's event pairs, one warm-up and the median of 7 runs, one process, the 20000^2 synthetic scene.

  1. Frost (damping 2.0) at windows 3 / 5 / 7 and Refined Lee (looks 4.4), for one band (sarpro_hip_speckle_ext_u16_dev) and for both
     bands in one launch (inside sarpro_hip_dualpol_synrgb_speckle_ext_u16_dev): ms, and the ratio to Lee 7 of the same run;
  2. in the same process the yardsticks: Lee 7 (speckle_u16, through the _ext call) and k_dn_hist_pieces (kernel time dn_hist_u16 of the
     CLAHE dual-pol chain, 2 B/px) on the same rasters;
  3. the resident _ext flow -> 2048^2 padded RGB (Robust; Frost 7 and Refined Lee), wall time per call on a context without timing;
  4. whether the kernels' rasters equal the numpy restatement (tests/speckleextref.py) bit for bit AT A REDUCED SIZE (2000^2).

    python tools/time_speckle_ext.py [--out DIR] [--small]     (DIR defaults to profiles/speckle; --small: a 4096^2 scene)
Prints as it goes and writes DIR/time_speckle_ext.json."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import speckleextref
import sarpro_amd as S
from sarpro_amd import AutoscaleStrategy as St, SpeckleFilter as F, SyntheticRgbMode, synth, resize_output_dims

REPS = 7
LOOKS, DAMPING = 4.4, 2.0
TS = 2048
small = "--small" in sys.argv
out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "speckle")
rows = cols = 4096 if small else 20000
ref_side = 1000 if small else 2000
CASES = [("lee7", F.Lee, 7, "speckle_u16"), ("frost3", F.Frost, 3, "speckle_frost_u16"), ("frost5", F.Frost, 5, "speckle_frost_u16"),
         ("frost7", F.Frost, 7, "speckle_frost_u16"), ("refined_lee7", F.RefinedLee, 7, "speckle_rlee_u16")]


def median(xs):
    return sorted(xs)[len(xs) // 2]


def kernel_ms(c, name):
    return sum(v for k, v in c.last_kernel_times() if k == name)


def timed(fn, reps=REPS):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return median(out)


q = synth.q_tables()
pitch = (cols + 63) // 64 * 64
px = rows * cols
fc, fr = resize_output_dims(cols, rows, TS, True)
band = [torch.empty((rows, pitch), dtype=torch.int16, device="cuda") for _ in range(2)]
f32 = torch.empty((rows, pitch), dtype=torch.float32, device="cuda")
rgb = torch.empty(fr * fc * 3, dtype=torch.uint8, device="cuda")
result = {"cols": cols, "rows": rows, "looks": LOOKS, "damping": DAMPING, "reps": REPS, "passes": []}
with S.Context(0, timing=True) as c:
    for b in range(2):
        c.dev_synth_scene_u16(synth.SEED_SCENE_A, b, q, rows, cols, 0, rows, band[b].data_ptr(), pitch)
    c.synchronize()
    for name, filt, k, kernel in CASES:
        one, two = [], []
        for it in range(REPS + 1):
            c.dev_speckle_ext_u16(band[0].data_ptr(), rows, cols, pitch, filt, k, LOOKS, DAMPING, f32.data_ptr(), pitch)
            a = kernel_ms(c, kernel)
            c.dev_dualpol_synrgb_speckle_ext(band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, filt, k, LOOKS, DAMPING, St.Robust, TS, True,
                                             rgb.data_ptr())
            b2 = kernel_ms(c, kernel)
            if it:
                one.append(a); two.append(b2)
        w = {"pass": name, "kernel_time": kernel, "window": k, "one_band_ms": round(median(one), 4), "both_bands_ms": round(median(two), 4),
             "one_band_Gpx_per_s": round(px / median(one) / 1e6, 2)}
        print(w, flush=True)
        result["passes"].append(w)
    lee = result["passes"][0]
    for w in result["passes"]:
        w["one_band_over_lee7"] = round(w["one_band_ms"] / lee["one_band_ms"], 2)
        w["both_bands_over_lee7"] = round(w["both_bands_ms"] / lee["both_bands_ms"], 2)
    hist = []
    native = torch.empty((rows, cols * 3), dtype=torch.uint8, device="cuda")
    for it in range(REPS + 1):
        c.dev_dualpol_synrgb_u16(band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, St.Clahe, SyntheticRgbMode.Default, native.data_ptr(), cols,
                                 want_stats=False)
        c.synchronize()
        if it:
            hist.append(kernel_ms(c, "dn_hist_u16"))
    del native
    result["dn_hist_pieces_both_bands_ms"] = round(median(hist), 4)
with S.Context(0) as c:
    for name, filt, k in (("frost7", F.Frost, 7), ("refined_lee7", F.RefinedLee, 7), ("lee7", F.Lee, 7)):
        result[f"resident_flow_{name}_robust_ms"] = round(timed(lambda: c.dev_dualpol_synrgb_speckle_ext(
            band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, filt, k, LOOKS, DAMPING, St.Robust, TS, True, rgb.data_ptr()), 3), 3)
    hb = np.ascontiguousarray(band[0][:ref_side, :ref_side].cpu().numpy().view(np.uint16))
    equal = {}
    for name, filt, k, _ in CASES[1:]:
        ref = speckleextref.speckle_ext_u16(hb, int(filt), k, LOOKS, DAMPING)
        got = c.speckle_ext(hb, filt, k, LOOKS, DAMPING)
        equal[name] = bool(np.array_equal(got.view(np.uint32), ref.view(np.uint32)))
    result["kernel_equals_restatement_bit_for_bit"] = equal
    result["restatement_note"] = f"tests/speckleextref.py at the REDUCED size {ref_side} x {ref_side}"
print(result, flush=True)
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "time_speckle_ext.json"), "w") as f:
    json.dump(result, f, indent=1)
print("wrote", os.path.join(out_dir, "time_speckle_ext.json"))
