#!/usr/bin/env python3
"""Speckle filtering on the device (k_speckle_u16) on one MI355X: kernel times from the context's event pairs, one warm-up
and the median of 7 runs, one process.

  1. speckle_u16 (Lee, looks 4.4, windows 3 / 5 / 7) for one band (sarpro_hip_speckle_u16_dev) and for both bands in one launch (inside
     sarpro_hip_dualpol_synrgb_speckle_u16_dev) of the 20000^2 synthetic scene: ms and TB/s of algorithmic traffic (6 B/px: 2 B of DNs
     in, 4 B of f32 out);
  2. in the same process the yardsticks: k_dn_hist_pieces (kernel time dn_hist_u16 of the CLAHE dual-pol chain, 2 B/px) on the same
     rasters, and the time of 6 B/px at the 6.29 TB/s copy ceiling (profiles/r2/stream_bench.txt);
  3. the resident flow sarpro_hip_dualpol_synrgb_speckle_u16_dev -> 2048^2 padded RGB (CLAHE and Robust, window 7), wall time per call on
     a context without timing;
  4. the numpy restatement (tests/speckleref.py, one host thread) for one band AT A REDUCED SIZE (4000^2), and whether the kernel's
     raster equals it bit for bit there.

    python tools/time_speckle.py [--out DIR] [--small]     (DIR defaults to profiles/speckle; --small: a 4096^2 scene)
    SARPRO_HIP_LIB=$PWD/sarpro_amd/lib_<name>.so python tools/time_speckle.py --variant     (one JSON line: step 1 at window 7 only)
Prints as it goes and writes DIR/time_speckle.json.  The ablation variants (profiles/speckle/variants.json) are built with
    tools/build_variant.sh speckle_notail "-DSARPRO_SPECKLE_ABLATE_TAIL" speckle_kernels.hip   (no f64 tail: wrong results)
    tools/build_variant.sh speckle_nosum  "-DSARPRO_SPECKLE_ABLATE_SUM"  speckle_kernels.hip   (no LDS window reads / row sums: wrong results)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import speckleref
import sarpro_amd as S
from sarpro_amd import AutoscaleStrategy as St, SpeckleFilter, SyntheticRgbMode, synth, resize_output_dims

COPY_CEILING = 6.29e12
REPS = 7
LOOKS = 4.4
TS = 2048
small = "--small" in sys.argv
variant = "--variant" in sys.argv
out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "speckle")
rows = cols = 4096 if small else 20000
ref_side = 1000 if small else 4000


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
result = {"cols": cols, "rows": rows, "filter": "Lee", "looks": LOOKS, "reps": REPS, "bytes_per_px": 6, "copy_ceiling_TBps": COPY_CEILING / 1e12,
          "copy_ceiling_source": "profiles/r2/stream_bench.txt", "one_band_at_copy_ceiling_ms": round(px * 6 / COPY_CEILING * 1e3, 4),
          "both_bands_at_copy_ceiling_ms": round(2 * px * 6 / COPY_CEILING * 1e3, 4), "windows": []}
with S.Context(0, timing=True) as c:
    for b in range(2):
        c.dev_synth_scene_u16(synth.SEED_SCENE_A, b, q, rows, cols, 0, rows, band[b].data_ptr(), pitch)
    c.synchronize()
    for k in ((7,) if variant else (3, 5, 7)):
        one, two = [], []
        for it in range(REPS + 1):
            c.dev_speckle_u16(band[0].data_ptr(), rows, cols, pitch, SpeckleFilter.Lee, k, LOOKS, f32.data_ptr(), pitch)
            a = kernel_ms(c, "speckle_u16")
            try:
                c.dev_dualpol_synrgb_speckle(band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, SpeckleFilter.Lee, k, LOOKS, St.Robust, TS, True,
                                             rgb.data_ptr())
            except S.SarproHipError as e:  # (an ablation variant may feed the chain bands it cannot scale)
                print("flow:", e)
            b2 = kernel_ms(c, "speckle_u16")
            if it:
                one.append(a); two.append(b2)
        w = {"window": k, "one_band_ms": round(median(one), 4), "one_band_TBps": round(px * 6 / median(one) / 1e9, 3),
             "both_bands_ms": round(median(two), 4), "both_bands_TBps": round(2 * px * 6 / median(two) / 1e9, 3)}
        print(w, flush=True)
        result["windows"].append(w)
    if variant:
        print(json.dumps({"lib": os.environ.get("SARPRO_HIP_LIB", "default"), **result["windows"][0]}))
        sys.exit(0)
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
    result["dn_hist_pieces_both_bands_TBps_of_2_B_per_px"] = round(2 * px * 2 / median(hist) / 1e9, 3) if median(hist) > 0 else None
with S.Context(0) as c:
    for name, st in (("clahe", St.Clahe), ("robust", St.Robust)):
        result[f"resident_flow_window7_{name}_ms"] = round(timed(lambda: c.dev_dualpol_synrgb_speckle(
            band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, SpeckleFilter.Lee, 7, LOOKS, st, TS, True, rgb.data_ptr()), 3), 3)
    hb = np.ascontiguousarray(band[0][:ref_side, :ref_side].cpu().numpy().view(np.uint16))
    t = time.perf_counter()
    ref = speckleref.speckle_u16(hb, speckleref.LEE, 7, LOOKS)
    result["numpy_restatement_one_band_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    result["numpy_restatement_note"] = f"tests/speckleref.py at the REDUCED size {ref_side} x {ref_side} (window 7), vectorised numpy on one host thread"
    got = c.speckle(hb, SpeckleFilter.Lee, 7, LOOKS)
    result["kernel_equals_restatement_bit_for_bit"] = bool(np.array_equal(got.view(np.uint32), ref.view(np.uint32)))
print(result, flush=True)
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "time_speckle.json"), "w") as f:
    json.dump(result, f, indent=1)
print("wrote", os.path.join(out_dir, "time_speckle.json"))
