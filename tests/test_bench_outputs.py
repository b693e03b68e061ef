"""bench.py --dump-outputs: the raster of the last timed step reaches the files as the caller of the timed entry point receives it
(checked against the CPU oracle on a small scene), a raster too large to keep is sampled by whole rows with a fixed seed, and a
plain run (no --full) carries none of the records that are measured beside the headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_of_a_large_raster_is_a_seeded_row_sample_with_a_whole_raster_histogram(tmp_path):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    rows, cols, pitch = 2100, 2048, 2112          # 2100 x 2048 x 3 x 4 B = 51.6 MB as float32: above the limit, so rows are drawn
    rng = np.random.default_rng(7)
    host = rng.integers(0, 256, size=(rows, pitch, 3), dtype=np.uint8)
    rgb = torch.from_numpy(host.reshape(rows, pitch * 3).copy())
    for d in ("a", "b"):
        bench.dump_outputs(torch, str(tmp_path / d), rgb, rows, cols, pitch, 0)
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("rgb", "rgb_rows", "rgb_hist")}
    b = {n: np.load(tmp_path / "b" / f"{n}.npy") for n in ("rgb", "rgb_rows", "rgb_hist")}
    assert all(np.array_equal(a[n], b[n]) for n in a)                      # the same rows every time
    assert a["rgb"].dtype == np.float32 and a["rgb_rows"].dtype == np.float64 and a["rgb_hist"].dtype == np.float64
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    pick = a["rgb_rows"].astype(np.int64)
    assert 0 < len(pick) < rows and np.all(np.diff(pick) > 0) and pick[0] >= 0 and pick[-1] < rows
    assert a["rgb"].shape == (len(pick), cols, 3)
    assert np.array_equal(a["rgb"], host[pick, :cols].astype(np.float32))  # the pad columns of the pitch are cut off
    want = np.stack([np.bincount(host[:, :cols, ch].reshape(-1), minlength=256) for ch in range(3)])
    assert np.array_equal(a["rgb_hist"], want.astype(np.float64))          # every pixel, not the sample


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_s_raster_and_it_equals_the_oracle(tmp_path):
    import oracle
    from sarpro_amd import AutoscaleStrategy, synth
    rows, cols, steps = 600, 700, 2
    out_dir = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--rows", str(rows),
                        "--cols", str(cols), "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["steps"] == steps and rec["ms_per_step"] > 0 and rec["unit"] == "Mpix/s" and rec["higher_is_better"] is True
    # value (Mpix/s, one decimal) and ms_per_step (three decimals) are rounded from the same elapsed time
    assert abs(rec["value"] * rec["ms_per_step"] * 1e3 / (rows * cols) - 1.0) <= 1.01 * (0.0005 / rec["ms_per_step"] + 0.05 / rec["value"])
    assert rec["full"] is False
    for beside in ("cpu_baseline", "secondary", "ms_per_step_one_stream", "ms_per_step_scene_a"):
        assert beside not in rec, beside
    # the last timed step is scene (steps - 1) of the cycle
    name, off, flags, qkw, _ = synth.BENCH_SCENES[(steps - 1) % len(synth.BENCH_SCENES)]
    q = synth.q_tables(**qkw) if qkw else synth.q_tables()
    b1, b2 = (synth.scene_u16(rows, cols, b, seed=synth.SEED_SCENE_A + off, q=q, flags=flags) for b in (0, 1))
    rc, ref, _, _ = oracle.dualpol_synrgb(b1.astype(np.float32), b2.astype(np.float32), int(AutoscaleStrategy.Clahe))
    assert rc == 0
    got = np.load(out_dir / "rgb.npy")
    assert got.dtype == np.float32 and got.shape == (rows, cols, 3)
    assert np.array_equal(np.load(out_dir / "rgb_rows.npy"), np.arange(rows, dtype=np.float64))   # small enough to be kept whole
    assert np.array_equal(got, ref.reshape(rows, cols, 3).astype(np.float32)), name
    want = np.stack([np.bincount(ref.reshape(rows, cols, 3)[:, :, ch].reshape(-1), minlength=256) for ch in range(3)])
    assert np.array_equal(np.load(out_dir / "rgb_hist.npy"), want.astype(np.float64))
