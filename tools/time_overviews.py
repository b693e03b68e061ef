#!/usr/bin/env python3
"""Overview pyramids on the device (k_overviews) on one MI355X: kernel times from the context's event pairs, one warm-up and
the median of 9 runs, the configurations interleaved in one process.

  1. the RGB raster (u8 x 3) of the 20000^2 synthetic scene, device-resident, 6 levels down to 313^2 (sarpro_hip_overviews_dev): at
     OVR_DEPTH 6 (one sweep), 3, 2 and 1 (one launch per level), alternating; ms (the sum of the call's `overviews` entries) and
     TB/s of the ALGORITHMIC traffic -- the source read once, each level written once -- beside the time of that byte count at the
     6.29 TB/s copy ceiling (profiles/r2/stream_bench.txt);
  2. the same for a single u16 band of that scene;
  3. the flow sarpro_hip_dualpol_synrgb_pyramid_u16_dev against sarpro_hip_dualpol_synrgb_u16_dev alone (CLAHE), wall time per
     synchronous call on a context without timing, alternating;
  4. whether the device levels equal the library's host twin (sarpro_hip_host_overviews) on a 2048^2 corner of the RGB.

    python tools/time_overviews.py [--out DIR] [--small]     (DIR defaults to profiles/overviews; --small: a 4096^2 scene)
    SARPRO_HIP_LIB=$PWD/sarpro_amd/lib_<name>.so python tools/time_overviews.py --variant     (one JSON line: step 1 only)
Prints as it goes and writes DIR/time_overviews.json.  The ablation variants (wrong results, timing only; their --variant lines are
kept in profiles/overviews/variants.jsonl) are built with
    tools/build_variant.sh ovr_noload   "-DSARPRO_OVR_ABLATE_LOAD"   overview_kernels.hip   (no source loads: reduction and stores)
    tools/build_variant.sh ovr_noreduce "-DSARPRO_OVR_ABLATE_REDUCE" overview_kernels.hip   (a level = one sample per block: no sums)
    tools/build_variant.sh ovr_nostore  "-DSARPRO_OVR_ABLATE_STORE"  overview_kernels.hip   (one 16-byte slot per piece leaves)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import sarpro_amd as S
from sarpro_amd import AutoscaleStrategy as St, SyntheticRgbMode, synth

COPY_CEILING = 6.29e12
REPS = 9
DEPTHS = (6, 3, 2, 1)  # OVR_DEPTH settings, measured interleaved
small = "--small" in sys.argv
variant = "--variant" in sys.argv
out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "overviews")
rows = cols = 4096 if small else 20000


def median(xs):
    return sorted(xs)[len(xs) // 2]


def kernel_ms(c, name):
    return sum(v for k, v in c.last_kernel_times() if k == name)


def traffic(plan, cols, rows):
    """bytes the algorithm needs: the source read once, each level written once"""
    px = plan.components * plan.bits // 8
    return cols * rows * px + sum(plan.cols[k] * plan.rows[k] * px for k in range(plan.levels))


def sweep(c, name, d_src, pitch_bytes, comps, bits):
    plan = S.overview_plan(cols, rows, comps, bits, 512)
    d_out = torch.empty(plan.total_bytes, dtype=torch.uint8, device="cuda")
    nbytes = traffic(plan, cols, rows)
    ms = {d: [] for d in DEPTHS}
    for it in range(REPS + 1):
        for d in DEPTHS:  # interleaved
            c.set_attr("OVR_DEPTH", d)
            c.dev_overviews(d_src, cols, rows, pitch_bytes, comps, bits, plan, d_out.data_ptr())
            if it:
                ms[d].append(kernel_ms(c, "overviews"))
    c.set_attr("OVR_DEPTH", None)
    r = {"raster": name, "levels": plan.levels, "last_level": [plan.cols[plan.levels - 1], plan.rows[plan.levels - 1]], "algorithmic_bytes": nbytes,
         "at_copy_ceiling_ms": round(nbytes / COPY_CEILING * 1e3, 4)}
    for d in DEPTHS:
        m = median(ms[d])
        r[f"depth{d}_ms"] = round(m, 4)
        r[f"depth{d}_min_max_ms"] = [round(min(ms[d]), 4), round(max(ms[d]), 4)]
        r[f"depth{d}_TBps"] = round(nbytes / m / 1e9, 3)
        r[f"depth{d}_launches"] = -(-plan.levels // d)
    print(r, flush=True)
    return r, plan, d_out


q = synth.q_tables()
pitch = (cols + 63) // 64 * 64
band = [torch.empty((rows, pitch), dtype=torch.int16, device="cuda") for _ in range(2)]
rgb = torch.empty((rows, pitch * 3), dtype=torch.uint8, device="cuda")
result = {"cols": cols, "rows": rows, "reps": REPS, "copy_ceiling_TBps": COPY_CEILING / 1e12, "copy_ceiling_source": "profiles/r2/stream_bench.txt",
          "lib": os.environ.get("SARPRO_HIP_LIB", "default"), "sweeps": []}
with S.Context(0, timing=True) as c:
    for b in range(2):
        c.dev_synth_scene_u16(synth.SEED_SCENE_A, b, q, rows, cols, 0, rows, band[b].data_ptr(), pitch)
    c.dev_dualpol_synrgb_u16(band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, St.Clahe, SyntheticRgbMode.Default, rgb.data_ptr(), pitch, want_stats=False)
    c.synchronize()
    r, plan, d_out = sweep(c, "rgb_u8x3", rgb.data_ptr(), pitch * 3, 3, 8)
    result["sweeps"].append(r)
    if variant:
        print(json.dumps({"lib": result["lib"], **r}))
        sys.exit(0)
    side = min(2048, rows)
    corner = np.ascontiguousarray(rgb.cpu().numpy().reshape(rows, pitch, 3)[:side, :side])
    _, dev = c.overviews(corner, 64)
    _, host = S.host_overviews(corner, 64)
    result["device_equals_host_twin_on_a_corner"] = bool(np.array_equal(dev, host))
    del d_out
    r, _, d_out = sweep(c, "band_u16x1", band[0].data_ptr(), pitch * 2, 1, 16)
    result["sweeps"].append(r)
    del d_out
with S.Context(0) as c:
    plan = S.overview_plan(cols, rows, 3, 8, 512)
    d_ovr = torch.empty(plan.total_bytes, dtype=torch.uint8, device="cuda")
    args = (band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, St.Clahe, SyntheticRgbMode.Default, rgb.data_ptr(), pitch)
    flows = {"dualpol_synrgb_u16_dev": lambda: c.dev_dualpol_synrgb_u16(*args, want_stats=False),
             "dualpol_synrgb_pyramid_u16_dev": lambda: c.dev_dualpol_synrgb_pyramid(*args, plan, d_ovr.data_ptr(), want_stats=False)}
    wall = {k: [] for k in flows}
    for it in range(REPS + 1):
        for k, fn in flows.items():  # interleaved
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            if it:
                wall[k].append((time.perf_counter() - t) * 1e3)
    for k in flows:
        result[f"flow_{k}_ms"] = round(median(wall[k]), 4)
        result[f"flow_{k}_min_max_ms"] = [round(min(wall[k]), 4), round(max(wall[k]), 4)]
print(result, flush=True)
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "time_overviews.json"), "w") as f:
    json.dump(result, f, indent=1)
print("wrote", os.path.join(out_dir, "time_overviews.json"))
