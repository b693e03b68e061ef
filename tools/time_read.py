#!/usr/bin/env python3
"""Downsample on read on the device (k_read_average_u16) on one MI355X: kernel times from the context's event pairs,
one warm-up and the median of 7 runs.

  1. read_average for one band (sarpro_hip_read_average_u16_dev) and for both bands in one launch (inside
     sarpro_hip_dualpol_synrgb_read_u16_dev) of the 20000^2 synthetic scene -> 2048^2 and of 25000 x 16700 -> 2048 x 1368: ms and
     TB/s of raster read (2 B per source sample);
  2. in the same process the yardstick: k_dn_hist_pieces (kernel time dn_hist_u16 of the CLAHE dual-pol chain) on the same two
     rasters, and the 6.29 TB/s copy ceiling (profiles/r2/stream_bench.txt);
  3. the resident flow sarpro_hip_dualpol_synrgb_read_u16_dev (CLAHE and Robust), wall time per call on a context without timing;
  4. host to host: sarpro_hip_dualpol_synrgb_read_u16 against sarpro_hip_dualpol_synrgb_resized_u16 on the same scene (both upload the
     same two rasters);
  5. the vectorised numpy restatement of the average (tests/readref.py) on one host thread -- NOT GDAL, which is absent.

    python tools/time_read.py [--out DIR] [--small]      (DIR defaults to profiles/read; --small: 4096^2 and 5000 x 3340)
Prints as it goes and writes DIR/time_read.json."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import readref
import sarpro_amd as S
from sarpro_amd import AutoscaleStrategy as St, SyntheticRgbMode, synth, read_output_dims, resize_output_dims

COPY_CEILING = 6.29e12
REPS = 7
small = "--small" in sys.argv
out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "read")
scenes = [(4096, 4096), (5000, 3340)] if small else [(20000, 20000), (25000, 16700)]  # (cols, rows)
TS = 2048
result = {"target_size": TS, "reps": REPS, "copy_ceiling_TBps": COPY_CEILING / 1e12, "copy_ceiling_source": "profiles/r2/stream_bench.txt", "scenes": []}


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
for cols, rows in scenes:
    pitch = (cols + 63) // 64 * 64
    oc, orows, alg = read_output_dims(cols, rows, TS)
    fc, fr = resize_output_dims(oc, orows, TS, True)
    row = {"cols": cols, "rows": rows, "out_cols": oc, "out_rows": orows, "reduction": round(max(cols, rows) / TS, 3)}
    band = [torch.empty((rows, pitch), dtype=torch.int16, device="cuda") for _ in range(2)]
    opitch = (oc + 63) // 64 * 64
    f32 = torch.empty((orows, opitch), dtype=torch.float32, device="cuda")
    rgb = torch.empty(fr * fc * 3, dtype=torch.uint8, device="cuda")
    with S.Context(0, timing=True) as c:
        for b in range(2):
            c.dev_synth_scene_u16(synth.SEED_SCENE_A, b, q, rows, cols, 0, rows, band[b].data_ptr(), pitch)
        c.synchronize()
        one, two, hist = [], [], []
        for it in range(REPS + 1):
            c.dev_read_average(band[0].data_ptr(), rows, cols, pitch, orows, oc, f32.data_ptr(), opitch)
            a = kernel_ms(c, "read_average")
            c.dev_dualpol_synrgb_read(band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, St.Robust, TS, True, rgb.data_ptr())
            b2 = kernel_ms(c, "read_average")
            native = torch.empty((rows, cols * 3), dtype=torch.uint8, device="cuda") if it == 0 else native
            c.dev_dualpol_synrgb_u16(band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, St.Clahe, SyntheticRgbMode.Default, native.data_ptr(), cols, want_stats=False)
            c.synchronize()
            h = kernel_ms(c, "dn_hist_u16")
            if it:
                one.append(a); two.append(b2); hist.append(h)
        del native
        px = rows * cols
        row["read_average_one_band_ms"] = round(median(one), 4)
        row["read_average_one_band_TBps"] = round(px * 2 / median(one) / 1e9, 3)
        row["read_average_both_bands_ms"] = round(median(two), 4)
        row["read_average_both_bands_TBps"] = round(2 * px * 2 / median(two) / 1e9, 3)
        row["dn_hist_pieces_both_bands_ms"] = round(median(hist), 4)
        row["dn_hist_pieces_both_bands_TBps"] = round(2 * px * 2 / median(hist) / 1e9, 3) if median(hist) > 0 else None
        row["both_bands_at_copy_ceiling_ms"] = round(2 * px * 2 / COPY_CEILING * 1e3, 4)
    with S.Context(0) as c:
        for name, st in (("clahe", St.Clahe), ("robust", St.Robust)):
            row[f"resident_flow_{name}_ms"] = round(timed(lambda: c.dev_dualpol_synrgb_read(band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, st, TS, True,
                                                                                                 rgb.data_ptr())), 4)
        if (cols, rows) == scenes[0]:
            hb = [np.ascontiguousarray(band[b][:, :cols].cpu().numpy().view(np.uint16)) for b in range(2)]
            row["host_flow_read_ms"] = round(timed(lambda: c.dualpol_synrgb_read(hb[0], hb[1], St.Robust, TS, True), 3), 2)
            row["host_flow_resized_u16_ms"] = round(timed(lambda: c.dualpol_synrgb_resized(hb[0], hb[1], St.Robust, TS, True), 3), 2)
            row["host_flow_upload_bytes"] = int(hb[0].nbytes + hb[1].nbytes)
            t = time.perf_counter()
            ref = readref.average_u16(hb[0], orows, oc)
            row["numpy_restatement_one_band_one_thread_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            row["numpy_restatement_note"] = "tests/readref.py, vectorised numpy on one host thread; not GDAL (absent here)"
            got = c.read_average(hb[0], orows, oc)
            row["kernel_equals_restatement_bit_for_bit"] = bool(np.array_equal(got.view(np.uint32), ref.view(np.uint32)))
            del hb
    print(row, flush=True)
    result["scenes"].append(row)
    del band, f32, rgb
    torch.cuda.empty_cache()
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "time_read.json"), "w") as f:
    json.dump(result, f, indent=1)
print("wrote", os.path.join(out_dir, "time_read.json"))
