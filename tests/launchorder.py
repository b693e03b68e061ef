"""The launch order of the u16 routes: a table of routes and one function that runs each of them on a fresh Context(0, timing=True) and
returns the names `last_kernel_times()` reports, in order (`host:` entries included; the times themselves are dropped).

tests/golden/launch_order_u16.json holds what this module gave BEFORE the host code of the u16 flavour was restructured into route
functions; tests/test_gpu_launch_order.py compares route by route.  The fixture is a record of that library, not of the current one:
it is not regenerated when the test fails -- a difference is a defect of the change that caused it.

    PYTHONPATH=.:tests python tests/launchorder.py OUT.json      # (how the fixture was written)
"""
import json
import sys

import numpy as np

import sarpro_amd as S
from sarpro_amd import AutoscaleStrategy as St, BitDepth as Bd, SyntheticRgbMode as Mode, synth

ROWS, COLS = 264, 512                      # the smallest shape of the CLAHE tests
S_ROWS, S_COLS, S_PITCH = 403, 520, 576    # the stripe tests' shape

_bands = {}


def bands(rows, cols, seed_off=0):
    key = (rows, cols, seed_off)
    if key not in _bands:
        _bands[key] = [synth.scene_u16(rows, cols, b, seed=synth.SEED_SCENE_A + seed_off) for b in (0, 1)]
    return _bands[key]


def _names(c):
    return [n for n, _ in c.last_kernel_times()]


def dualpol(strategy, want_u8=False, want_stats=False):
    def run(attrs):
        b = bands(ROWS, COLS)
        with S.Context(0, timing=True) as c:
            for k, v in attrs.items():
                c.set_attr(k, v)
            c.dualpol_synrgb(b[0], b[1], strategy, want_u8=want_u8, want_stats=want_stats)
            return _names(c)
    return run


def single(strategy, bd):
    def run(attrs):
        b = bands(ROWS, COLS)
        with S.Context(0, timing=True) as c:
            for k, v in attrs.items():
                c.set_attr(k, v)
            c.process_scalar_data_pipeline(b[0], bd, strategy)
            return _names(c)
    return run


def stripes(strategy, ranks=2):
    def run(attrs):
        import torch
        from test_gpu_multirank_local import run_ranks, to_dev
        b = bands(S_ROWS, S_COLS)
        splits = list(zip(*S.host_stripe_plan(S_ROWS, ranks)))
        d = [[to_dev(x[r0:r0 + nr], S_PITCH, torch.int16) for x in b] for r0, nr in splits]
        rgb = [torch.zeros((max(nr, 1), S_PITCH * 3), dtype=torch.uint8, device="cuda") for _, nr in splits]

        def body(c, k, r0, nr):
            return c.stripe_run_u16(d[k][0].data_ptr(), d[k][1].data_ptr(), S_ROWS, S_COLS, r0, nr, S_PITCH, strategy, Mode.Default, rgb[k].data_ptr(), S_PITCH)
        _, names = run_ranks(splits, body, attrs)
        return names  # every rank's list
    return run


def batch(scenes=3, lanes=2):
    def run(attrs):
        import torch
        pitch = (COLS + 63) // 64 * 64
        dev = []
        for k in range(scenes):
            db = []
            for x in bands(ROWS, COLS, k):
                t = torch.zeros((ROWS, pitch), dtype=torch.int16, device="cuda")
                t[:, :COLS] = torch.from_numpy(x.view(np.int16)).cuda()
                db.append(t)
            dev.append(db)
        outs = [torch.zeros((ROWS, pitch * 3), dtype=torch.uint8, device="cuda") for _ in range(scenes)]
        torch.cuda.synchronize()
        with S.Context(0, timing=True) as c:
            for k, v in attrs.items():
                c.set_attr(k, v)
            sc = [(d[0].data_ptr(), d[1].data_ptr(), o.data_ptr()) for d, o in zip(dev, outs)]
            c.dev_batch_dualpol_synrgb_u16(sc, ROWS, COLS, pitch, St.Clahe, Mode.Default, pitch, lanes=lanes)
            return _names(c)
    return run


def pyramid(strategy):
    def run(attrs):
        b = bands(ROWS, COLS)
        with S.Context(0, timing=True) as c:
            for k, v in attrs.items():
                c.set_attr(k, v)
            c.dualpol_synrgb_pyramid(b[0], b[1], strategy)
            return _names(c)
    return run


SAMPLED = {"SAMPLED_HIST_MIN_PX": 0}

# route -> (runner, attributes)
ROUTES = {
    "clahe_dualpol_fused": (dualpol(St.Clahe), SAMPLED),
    "clahe_dualpol_fused_stats": (dualpol(St.Clahe, want_stats=True), SAMPLED),
    "clahe_dualpol_sampled_u8": (dualpol(St.Clahe, want_u8=True), SAMPLED),
    "clahe_dualpol_guarded": (dualpol(St.Clahe), {}),
    "clahe_dualpol_guarded_u8": (dualpol(St.Clahe, want_u8=True), {}),
    "clahe_dualpol_exact": (dualpol(St.Clahe), {"NO_SPEC": 1}),
    "clahe_dualpol_exact_u8": (dualpol(St.Clahe, want_u8=True), {"NO_SPEC": 1}),
    "clahe_dualpol_no_fused_rgb": (dualpol(St.Clahe), {"NO_FUSED_RGB": 1, **SAMPLED}),
    "clahe_dualpol_separate_cdfs": (dualpol(St.Clahe), {"SEPARATE_CDFS": 1}),
    "clahe_dualpol_fused_separate_cdfs": (dualpol(St.Clahe), {"SEPARATE_CDFS": 1, **SAMPLED}),
    "clahe_dualpol_fused_retried": (dualpol(St.Clahe), {"SPEC_FORCE": "mispredict", "SAMPLE_STRIDE": 5, **SAMPLED}),
    "clahe_dualpol_fused_refuted": (dualpol(St.Clahe), {"SPEC_FORCE": "mispredict,noretry", "SAMPLE_STRIDE": 5, **SAMPLED}),
    "clahe_dualpol_fused_nospec": (dualpol(St.Clahe), {"SPEC_FORCE": "nospec", **SAMPLED}),
    "clahe_dualpol_no_sampled_hist": (dualpol(St.Clahe), {"NO_SAMPLED_HIST": 1}),
    "clahe_dualpol_full_level_hist": (dualpol(St.Clahe), {"FULL_LEVEL_HIST": 1}),
    "clahe_dualpol_no_spec_rescale": (dualpol(St.Clahe), {"NO_SPEC_RESCALE": 1, **SAMPLED}),
    "clahe_single_u8": (single(St.Clahe, Bd.U8), {}),
    "clahe_single_u8_sampled": (single(St.Clahe, Bd.U8), SAMPLED),
    "clahe_single_u8_exact": (single(St.Clahe, Bd.U8), {"NO_SPEC": 1}),
    "clahe_single_u16": (single(St.Clahe, Bd.U16), {}),
    "clahe_single_u16_no_cf": (single(St.Clahe, Bd.U16), {"NO_U16_CF": 1}),
    "robust_dualpol": (dualpol(St.Robust), {}),
    "robust_dualpol_u8": (dualpol(St.Robust, want_u8=True), {}),
    "tamed_dualpol": (dualpol(St.Tamed), {}),
    "robust_single_u8": (single(St.Robust, Bd.U8), {}),
    "robust_single_u16": (single(St.Robust, Bd.U16), {}),
    "host_route_clahe_dualpol": (dualpol(St.Clahe), {"NO_CHAIN": 1}),
    "host_route_robust_dualpol": (dualpol(St.Robust), {"NO_CHAIN": 1}),
    "stripes2_clahe": (stripes(St.Clahe), {}),
    "stripes2_clahe_fused": (stripes(St.Clahe), {"SAMPLE_STRIDE": 5, **SAMPLED}),
    "stripes2_robust": (stripes(St.Robust), {}),
    "batch3x2_order0": (batch(), {"PIPE_ORDER": 0}),
    "batch3x2_order3": (batch(), {"PIPE_ORDER": 3}),
    "batch3x2_order0_fused": (batch(), {"PIPE_ORDER": 0, **SAMPLED}),
    "batch3x2_order3_fused": (batch(), {"PIPE_ORDER": 3, **SAMPLED}),
    "pyramid_clahe_deferred_tail": (pyramid(St.Clahe), {}),
    "pyramid_clahe_fused_deferred_tail": (pyramid(St.Clahe), SAMPLED),
    "pyramid_robust_deferred_tail": (pyramid(St.Robust), {}),
}


def run_route(route):
    runner, attrs = ROUTES[route]
    return runner(dict(attrs))


def run_all():
    return {route: run_route(route) for route in ROUTES}


if __name__ == "__main__":
    out = run_all()
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("routes:", len(out), "entries:", sum(len(v) for v in out.values()))
