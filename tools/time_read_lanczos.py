#!/usr/bin/env python3
"""Lanczos downsample on read on the device (k_read_lanczos_u16) on one MI355X: kernel times from the context's event
pairs, one warm-up and the median of 7 runs.

  1. read_lanczos for one band (sarpro_hip_read_lanczos_u16_dev) and for both bands in one launch (inside
     sarpro_hip_dualpol_synrgb_read_u16_dev on a context with READ_LANCZOS on) of the 20000^2 synthetic scene -> 8192^2 (reduction
     2.44) and -> 5001^2 (3.999), and of 25000 x 16700 -> 8192 x 5472: ms, and the time the bytes moved (2 B per source sample + 4 B per
     destination sample) take at the 6.29 TB/s copy ceiling (profiles/r2/stream_bench.txt);
  2. in the same process the yardsticks on the same rasters: read_average (-> 2048, the Average filter's own range) and
     k_dn_hist_pieces (kernel time dn_hist_u16 of the CLAHE dual-pol chain);
  3. the resident flow sarpro_hip_dualpol_synrgb_read_u16_dev (Robust), wall time per call on a context without timing, and host to
     host sarpro_hip_dualpol_synrgb_read_u16 on the first scene;
  4. the numpy restatement (tests/readlanczosref.py) on one host thread on the scene's top-left 4883 x 4883 sub-scene -> 2000^2 (the
     first shape's ratio) -- NOT GDAL, which is absent -- and the kernel against it by bit pattern.

    python tools/time_read_lanczos.py [--out DIR] [--small]   (DIR defaults to profiles/read; --small: 4096^2 and 5000 x 3340 -> 1678 / 1025)
With SARPRO_HIP_LIB naming a timing variant (tools/build_variant.sh lanczos_notaps "-DSARPRO_LANCZOS_ABLATE_TAPS" read_kernels.hip: the
pass without the lanes' tap reads and f64 products, wrong results) only step 1 runs and the file is DIR/time_read_lanczos_<variant>.json.
Prints as it goes and writes DIR/time_read_lanczos.json."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import readlanczosref
import sarpro_amd as S
from sarpro_amd import AutoscaleStrategy as St, SyntheticRgbMode, synth, read_output_dims, resize_output_dims

COPY_CEILING = 6.29e12
REPS = 7
small = "--small" in sys.argv
out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "read")
variant = os.path.basename(os.environ.get("SARPRO_HIP_LIB", ""))[4:-3] if os.environ.get("SARPRO_HIP_LIB") else ""
# (cols, rows, target_size)
cases = [(4096, 4096, 1678), (4096, 4096, 1025), (5000, 3340, 1678)] if small else [(20000, 20000, 8192), (20000, 20000, 5001), (25000, 16700, 8192)]
TS_AVERAGE = 512 if small else 2048
result = {"reps": REPS, "copy_ceiling_TBps": COPY_CEILING / 1e12, "copy_ceiling_source": "profiles/r2/stream_bench.txt", "variant": variant or None, "cases": []}


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
band, shape = None, None
for cols, rows, ts in cases:
    pitch = (cols + 63) // 64 * 64
    oc, orows, alg = read_output_dims(cols, rows, ts)
    assert alg == S._lib.READ_LANCZOS
    fc, fr = resize_output_dims(oc, orows, ts, True)
    row = {"cols": cols, "rows": rows, "target_size": ts, "out_cols": oc, "out_rows": orows, "reduction": round(max(cols, rows) / ts, 3),
           "col_taps": int(S.host_read_lanczos_axis(cols, oc)[1].max()), "row_taps": int(S.host_read_lanczos_axis(rows, orows)[1].max())}
    if shape != (cols, rows):
        del band
        torch.cuda.empty_cache()
        band = [torch.empty((rows, pitch), dtype=torch.int16, device="cuda") for _ in range(2)]
        shape = None
    opitch = (oc + 63) // 64 * 64
    f32 = torch.empty((orows, opitch), dtype=torch.float32, device="cuda")
    rgb = torch.empty(fr * fc * 3, dtype=torch.uint8, device="cuda")
    px, opx = rows * cols, orows * oc
    with S.Context(0, timing=True) as c:
        c.set_attr("READ_LANCZOS", 1)
        if shape is None:
            for b in range(2):
                c.dev_synth_scene_u16(synth.SEED_SCENE_A, b, q, rows, cols, 0, rows, band[b].data_ptr(), pitch)
            c.synchronize()
            shape = (cols, rows)
        one, two, avg, hist = [], [], [], []
        for it in range(REPS + 1):
            c.dev_read_lanczos(band[0].data_ptr(), rows, cols, pitch, orows, oc, f32.data_ptr(), opitch)
            a = kernel_ms(c, "read_lanczos")
            try:
                c.dev_dualpol_synrgb_read(band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, St.Robust, ts, True, rgb.data_ptr())
            except S.SarproHipError as e:  # (a variant without its taps feeds the chain empty bands)
                print("flow:", e)
            b2 = kernel_ms(c, "read_lanczos")
            if it:
                one.append(a); two.append(b2)
        row["read_lanczos_one_band_ms"] = round(median(one), 4)
        row["read_lanczos_both_bands_ms"] = round(median(two), 4)
        row["one_band_bytes_moved"] = px * 2 + opx * 4
        row["one_band_at_copy_ceiling_ms"] = round((px * 2 + opx * 4) / COPY_CEILING * 1e3, 4)
        row["both_bands_at_copy_ceiling_ms"] = round(2 * (px * 2 + opx * 4) / COPY_CEILING * 1e3, 4)
        row["one_band_source_Gsamples_per_s"] = round(px / median(one) / 1e6, 1)
        if not variant:
            aoc, aorows, _ = read_output_dims(cols, rows, TS_AVERAGE)
            af32 = torch.empty((aorows, aoc), dtype=torch.float32, device="cuda")
            native = torch.empty((rows, cols * 3), dtype=torch.uint8, device="cuda")
            for it in range(REPS + 1):
                c.dev_read_average(band[0].data_ptr(), rows, cols, pitch, aorows, aoc, af32.data_ptr(), aoc)
                a = kernel_ms(c, "read_average")
                c.dev_dualpol_synrgb_u16(band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, St.Clahe, SyntheticRgbMode.Default, native.data_ptr(), cols, want_stats=False)
                c.synchronize()
                h = kernel_ms(c, "dn_hist_u16")
                if it:
                    avg.append(a); hist.append(h)
            del native, af32
            row["read_average_one_band_to_%d_ms" % TS_AVERAGE] = round(median(avg), 4)
            row["dn_hist_pieces_both_bands_ms"] = round(median(hist), 4)
    if not variant:
        with S.Context(0) as c:
            c.set_attr("READ_LANCZOS", 1)
            row["resident_flow_robust_ms"] = round(timed(lambda: c.dev_dualpol_synrgb_read(band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, St.Robust, ts, True,
                                                                                           rgb.data_ptr())), 4)
            if (cols, rows, ts) == cases[0]:
                hb = [np.ascontiguousarray(band[b][:, :cols].cpu().numpy().view(np.uint16)) for b in range(2)]
                row["host_flow_read_ms"] = round(timed(lambda: c.dualpol_synrgb_read(hb[0], hb[1], St.Robust, ts, True), 3), 2)
                row["host_flow_upload_bytes"] = int(hb[0].nbytes + hb[1].nbytes)
                sub_n, sub_m = (1000, 410) if small else (4883, 2000)
                sub = np.ascontiguousarray(hb[0][:sub_n, :sub_n])
                t = time.perf_counter()
                ref = readlanczosref.lanczos_u16(sub, sub_m, sub_m)
                row["numpy_restatement_sub_scene"] = f"{sub_n} x {sub_n} -> {sub_m} x {sub_m}"
                row["numpy_restatement_sub_scene_one_thread_ms"] = round((time.perf_counter() - t) * 1e3, 1)
                row["numpy_restatement_note"] = "tests/readlanczosref.py, vectorised numpy on one host thread; not GDAL (absent here)"
                got = c.read_lanczos(sub, sub_m, sub_m)
                row["kernel_equals_restatement_bit_for_bit"] = bool(np.array_equal(got.view(np.uint32), ref.view(np.uint32)))
                del hb
    print(row, flush=True)
    result["cases"].append(row)
    del f32, rgb
os.makedirs(out_dir, exist_ok=True)
name = os.path.join(out_dir, f"time_read_lanczos_{variant}.json" if variant else "time_read_lanczos.json")
with open(name, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", name)
