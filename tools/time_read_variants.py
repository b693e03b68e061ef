#!/usr/bin/env python3
"""read_average (k_read_average_u16) of the library named by SARPRO_HIP_LIB (default: the built one) on the 20000^2
synthetic scene -> 2048^2: one band and both bands in one launch, kernel times from the context's event pairs, a warm-up and the median
of 7.  One process per library; the timing variants are built with

    tools/build_variant.sh read_generic "-DSARPRO_READ_ABLATE_GENERIC" read_kernels.hip   (the several-slabs form at every shape)
    tools/build_variant.sh read_nosum   "-DSARPRO_READ_ABLATE_SUM"     read_kernels.hip   (no LDS reads / sums by the lanes: wrong results)
    SARPRO_HIP_LIB=$PWD/sarpro_amd/lib_read_nosum.so python tools/time_read_variants.py

Prints one JSON line; profiles/read/variants.json keeps the three lines of one MI355X."""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import sarpro_amd as S
from sarpro_amd import AutoscaleStrategy as St, synth, read_output_dims, resize_output_dims
rows = cols = 20000
pitch = (cols + 63) // 64 * 64
oc, orows, _ = read_output_dims(cols, rows, 2048)
fc, fr = resize_output_dims(oc, orows, 2048, True)
q = synth.q_tables()
band = [torch.empty((rows, pitch), dtype=torch.int16, device="cuda") for _ in range(2)]
f32 = torch.empty((orows, 2048), dtype=torch.float32, device="cuda")
rgb = torch.empty(fr * fc * 3, dtype=torch.uint8, device="cuda")
med = lambda xs: sorted(xs)[len(xs) // 2]
with S.Context(0, timing=True) as c:
    for b in range(2):
        c.dev_synth_scene_u16(synth.SEED_SCENE_A, b, q, rows, cols, 0, rows, band[b].data_ptr(), pitch)
    c.synchronize()
    one, two = [], []
    for it in range(8):
        c.dev_read_average(band[0].data_ptr(), rows, cols, pitch, orows, oc, f32.data_ptr(), 2048)
        a = sum(v for k, v in c.last_kernel_times() if k == "read_average")
        try:
            c.dev_dualpol_synrgb_read(band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, St.Robust, 2048, True, rgb.data_ptr())
        except S.SarproHipError as e:  # (a variant without its sums feeds the chain empty bands)
            print("flow:", e)
        b2 = sum(v for k, v in c.last_kernel_times() if k == "read_average")
        if it:
            one.append(a); two.append(b2)
print(json.dumps({"lib": os.environ.get("SARPRO_HIP_LIB", "default"), "one_band_ms": round(med(one), 4), "one_band_TBps": round(rows * cols * 2 / med(one) / 1e9, 3),
                  "both_bands_ms": round(med(two), 4), "both_bands_TBps": round(2 * rows * cols * 2 / med(two) / 1e9, 3)}))
