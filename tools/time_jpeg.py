#!/usr/bin/env python3
"""The device JPEG encoder (sarpro_hip_jpeg_encode_dev) on pipeline-produced RGB rasters, alone and inside the _jpeg flow.

  1. the encoder alone at 2048^2 (the resized dual-pol product of a 20000^2 synthetic scene) and at 20000^2 (the native-resolution
     product), for restart intervals R in {1, 4, 8, 16, one MCU row} and the library's default: ms per image, the kernels' shares,
     GB/s of the raster read, file bytes per pixel, the file-size overhead over the largest interval measured;
  2. Pillow (libjpeg-turbo, quality 100, 4:4:4) on the same rasters on one host thread and on 16 (16 images at once at 2048^2,
     16 row stripes of the one image at 20000^2), and the time to read the raster once at the 6.29 TB/s copy ceiling;
  3. sarpro_hip_dualpol_synrgb_resized_u16_jpeg against sarpro_hip_dualpol_synrgb_resized_u16 + Pillow on the host.

    python tools/time_jpeg.py [--out DIR] [--small]      (DIR defaults to profiles/jpeg; --small: 4096^2 instead of 20000^2)
Prints as it goes and writes DIR/time_jpeg.json."""
import io, json, os, sys, time
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image
import sarpro_amd as S
from sarpro_amd import AutoscaleStrategy as St, SyntheticRgbMode, synth, resize_output_dims, jpeg_bound

Image.MAX_IMAGE_PIXELS = None
COPY_CEILING = 6.29e12
out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "jpeg")
big = 4096 if "--small" in sys.argv else 20000
result = {"big": big, "encoder": [], "pillow": [], "flow": {}}


def median(xs):
    return sorted(xs)[len(xs) // 2]


def pillow_bytes(a):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=100, subsampling=0)
    return buf.tell()


def time_encoder(c, d_rgb, n, label):
    """d_rgb: n x n x 3 on the device"""
    cap = min(jpeg_bound(n, n, 3, 1), 4 * n * n * 3)
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    mcus_x = (n + 7) // 8
    rows = []
    for r in (1, 4, 8, 16, mcus_x, 0):
        reps = 7 if n <= 4096 else 3
        dts, nbytes = [], 0
        for it in range(reps + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            nbytes = c.dev_jpeg_encode(d_rgb.data_ptr(), n, n, n * 3, 3, d_out.data_ptr(), cap, r)
            if it:
                dts.append((time.perf_counter() - t) * 1e3)
        kt = {k: round(v, 4) for k, v in c.last_kernel_times()}
        ms = median(dts)
        rows.append({"size": n, "raster": label, "R": r if r else "default", "ms": round(ms, 4), "kernels_ms": kt, "raster_GBps": round(n * n * 3 / ms / 1e6, 1),
                     "file_bytes": nbytes, "bytes_per_px": round(nbytes / (n * n), 4)})
        print(rows[-1], flush=True)
    base = min(x["file_bytes"] for x in rows)
    for x in rows:
        x["size_overhead_pct"] = round(100.0 * (x["file_bytes"] - base) / base, 3)
    print({"size": n, "overhead_pct": {str(x["R"]): x["size_overhead_pct"] for x in rows}, "read_once_at_copy_ceiling_ms": round(n * n * 3 / COPY_CEILING * 1e3, 4)}, flush=True)
    result["encoder"] += rows
    result.setdefault("read_once_at_copy_ceiling_ms", {})[str(n)] = round(n * n * 3 / COPY_CEILING * 1e3, 4)


def time_pillow(a, label):
    n = a.shape[0]
    t = time.perf_counter(); nb = pillow_bytes(a); one = (time.perf_counter() - t) * 1e3
    with ThreadPoolExecutor(16) as ex:
        if n <= 4096:   # 16 images at once: ms per image at that throughput
            t = time.perf_counter(); list(ex.map(pillow_bytes, [a] * 16)); many = (time.perf_counter() - t) * 1e3 / 16
            how = "16 images at once, per image"
        else:           # the one image as 16 row stripes (16 files, not one: the time a 16-thread host encoder could at best reach)
            parts = np.array_split(a, 16, axis=0)
            t = time.perf_counter(); list(ex.map(pillow_bytes, parts)); many = (time.perf_counter() - t) * 1e3
            how = "16 row stripes of the image"
    row = {"size": n, "raster": label, "pillow_1_thread_ms": round(one, 2), "pillow_16_threads_ms": round(many, 2), "16_threads_mean": how, "pillow_bytes_per_px": round(nb / (n * n), 4)}
    print(row, flush=True)
    result["pillow"].append(row)


rows = cols = big
pitch = (cols + 63) // 64 * 64
q = synth.q_tables()
with S.Context(0, timing=True) as c:
    torch.cuda.synchronize()
    band = [torch.empty((rows, pitch), dtype=torch.int16, device="cuda") for _ in range(2)]
    for b in range(2):
        c.dev_synth_scene_u16(synth.SEED_SCENE_A, b, q, rows, cols, 0, rows, band[b].data_ptr(), pitch)
    fc, fr = resize_output_dims(cols, rows, 2048, True)
    small = torch.empty((fr, fc, 3), dtype=torch.uint8, device="cuda")
    c.dev_dualpol_synrgb_resized(band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, St.Robust, 2048, True, small.data_ptr())
    time_encoder(c, small, 2048, f"resized product of the {big}^2 scene (Robust)")
    time_pillow(small.cpu().numpy(), "resized product")
    native = torch.empty((rows, cols, 3), dtype=torch.uint8, device="cuda")
    c.dev_dualpol_synrgb_u16(band[0].data_ptr(), band[1].data_ptr(), rows, cols, pitch, St.Robust, SyntheticRgbMode.Default, native.data_ptr(), cols, want_stats=False)
    c.synchronize()
    time_encoder(c, native, big, "native-resolution product (Robust)")
    time_pillow(native.cpu().numpy(), "native-resolution product")
    del native
    # the flow: host bands in, the file out, against the existing flow + Pillow on one host thread
    hb = [np.ascontiguousarray(band[b][:, :cols].cpu().numpy().view(np.uint16)) for b in range(2)]
    del band
    torch.cuda.empty_cache()
    for it in range(3):
        t = time.perf_counter(); data, _ = c.dualpol_synrgb_resized_jpeg(hb[0], hb[1], St.Robust, 2048, True); t_jpeg = (time.perf_counter() - t) * 1e3
        t = time.perf_counter(); rgb, _ = c.dualpol_synrgb_resized(hb[0], hb[1], St.Robust, 2048, True); t_flow = (time.perf_counter() - t) * 1e3
        t = time.perf_counter(); nb = pillow_bytes(rgb); t_pil = (time.perf_counter() - t) * 1e3
    result["flow"] = {"scene": big, "target": 2048, "jpeg_flow_ms": round(t_jpeg, 2), "existing_flow_ms": round(t_flow, 2), "pillow_1_thread_ms": round(t_pil, 2),
                      "file_bytes": len(data), "pillow_file_bytes": nb}
    print(result["flow"], flush=True)
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "time_jpeg.json"), "w") as f:
    json.dump(result, f, indent=1)
print("wrote", os.path.join(out_dir, "time_jpeg.json"))
