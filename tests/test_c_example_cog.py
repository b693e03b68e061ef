"""examples/grd_to_cog.c (TIFF files in, one tiled GeoTIFF with overviews out, nothing but the shared library): it must build as
strict C99 against include/sarpro_hip.h, and its file must hold the oracle's RGB and the restatement's overviews."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "sarpro_amd")


def _build(tmp_path):
    exe = str(tmp_path / "grd_to_cog")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-O2", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "grd_to_cog.c"), "-L" + LIBDIR, "-lsarpro_hip", "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_the_example_is_strict_c99_and_links(tmp_path):
    exe = _build(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr


@pytest.mark.gpu
def test_c_example_writes_the_oracles_rgb_and_the_restatements_overviews(tmp_path):
    import oracle
    import overviewref as R
    import sarpro_amd as S
    import test_tiff_pyramid as T
    from sarpro_amd import synth

    exe = _build(tmp_path)
    rows, cols = 333, 520
    b = [synth.scene_u16(rows, cols, k) for k in (0, 1)]
    paths = [str(tmp_path / f"b{k}.tif") for k in (0, 1)]
    for p, a in zip(paths, b):
        w = S.TiffWriter(p, cols, rows, 1, 16)
        w.write_rows(0, a)
        w.finish()
    out = str(tmp_path / "cog.tif")
    r = subprocess.run([exe, paths[0], paths[1], out, "4", "128", "100"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "3 overviews down to 65 x 42" in r.stdout, r.stdout + r.stderr
    rc, ref, _, _ = oracle.dualpol_synrgb(b[0].astype(np.float32), b[1].astype(np.float32), 4)
    assert rc == 0
    want = [ref] + R.overviews(ref, 100, True)                                     # (the example sets SKIP_ZERO)
    big, dirs, _, _, raw = T.parse(out)
    assert not big and len(dirs) == len(want) == 4
    for k, (d, a) in enumerate(zip(dirs, want)):
        assert d[322][1] == [128] and np.array_equal(T.tiles_of(raw, d, 3, 1, np.uint8)[0], a), k
