#!/usr/bin/env python
"""Times the Lyman-alpha forest on the device: a whole asora_lyman_alpha_forest call (host clock around the
synchronising call) with the automatic and with the same explicit window, and each of its stages (HIP events, ASORA_OPT_TIMING), at
256^3 on a field with ionisation fronts -- ionised bubbles in a neutral box, a log-normal density, a Gaussian velocity -- for a cold
box and for a photo-heated one (the ionised gas hot), along each line of sight.  The erf evaluations of a call are counted on the
host from the specification (two per term inside the cut with g != 0 of a cell that is not degenerate) and set against the stage
time and the FP64 vector peak given with --fp64-tflops (an erf is many operations: the share is that of the evaluations alone, at
--flops-per-erf each).  The numpy/scipy statement (tests/lyman_alpha_reference.py) is timed on the first --reference-planes planes
of lines along axis 2 and scaled to the mesh.  One JSON line per case.  Not a test.

    python tools/time_lyman_alpha.py [--mesh 256] [--reps 11] [--warmup 2] [--reference-planes 16] [--fp64-tflops 78.6]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from time_power_spectrum import timed      # noqa: E402

STAGES = ("reach", "optical_depth_and_gaps", "statistics", "fold")


def bubbles(N, rng, count=40):
    """x: 1 - 1e-4 inside `count` spheres of 6 ... 24 cells radius (periodic), 1e-3 outside, with fronts one cell sharp"""
    x = np.full((N, N, N), 1.0e-3)
    ax = np.arange(N)
    for _ in range(count):
        c, r = rng.integers(0, N, 3), rng.uniform(6.0, 24.0)
        d = [np.minimum(np.abs(ax - c[q]), N - np.abs(ax - c[q])) ** 2 for q in range(3)]
        x[d[0][:, None, None] + d[1][None, :, None] + d[2][None, None, :] <= r * r] = 1.0 - 1.0e-4
    return x


def erf_evaluations(R, x, n, T, v, axis, vscale, b_scale, tau_scale, W):
    lo, hi, bt, g = R.line_quantities(*(np.moveaxis(a, axis, -1) for a in (x, n, T, v)), vscale, b_scale, tau_scale)
    live = (g != 0.0) & (hi - lo >= R.FLOOR)
    total = 0
    for o in range(-W, W + 1):
        s = o + 0.5
        total += 2 * int(np.count_nonzero(live & ~(((s - hi) > 6.0 * bt) | ((lo - s) > 6.0 * bt))))
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, default=256)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reference-planes", type=int, default=16)
    ap.add_argument("--fp64-tflops", type=float, default=78.6, help="the FP64 vector peak the erf rate is set against (spec)")
    ap.add_argument("--flops-per-erf", type=float, default=50.0, help="operations counted per erf for the share of the peak (an estimate)")
    a = ap.parse_args()
    import lyman_alpha_reference as R
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    N = a.mesh
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)
    rng = np.random.default_rng(N)
    x = bubbles(N, rng)
    n = np.exp(0.7 * rng.normal(size=(N, N, N)))
    v = np.clip(0.5 * rng.normal(size=(N, N, N)), -1.5, 1.5)       # cells
    tau_scale, vscale = 3.0e3, 1.0                                 # tau about 3 in the neutral gas, 0.3 in the bubbles
    b_scale = 1.3 / math.sqrt(2.0e4)                               # bt = 1.3 cells at 2e4 K
    cases = {"cold": np.full((N, N, N), 50.0), "heated": np.where(x > 0.5, 2.0e4, 50.0)}
    lib.grid_to_device(_capi.GRID_XH, x)
    lib.grid_to_device(_capi.GRID_NDENS, n)
    lib.los_velocity_to_device(v)
    edges = np.linspace(0.0, 1.0, 21)
    edges[-1] = np.nextafter(1.0, 2.0)
    for name, T in cases.items():
        lib.grid_to_device(_capi.GRID_TEMP, T)
        for axis in (2, 1, 0):
            call = lambda window=0: lib.lyman_alpha_forest(axis, vscale, b_scale, tau_scale, window=window, edges=edges)
            lib.set_option(_capi.OPT_TIMING, 0)
            got = call()
            W = int(got["counts"][_capi.LYA_WINDOW])
            out = dict(case=name, N=N, axis=axis, W=W, clipped=int(got["counts"][_capi.LYA_CLIPPED]), reps=a.reps, warmup=a.warmup,
                       mean_flux=float(got["stats"][_capi.LYA_SUM_F]) / N ** 3, n_gaps=int(got["counts"][_capi.LYA_N_GAPS]),
                       longest=int(got["counts"][_capi.LYA_LONGEST]))
            out["call_ms_automatic"] = timed(call, a.reps, a.warmup)
            out["call_ms_explicit"] = timed(lambda: call(W), a.reps, a.warmup)
            lib.set_option(_capi.OPT_TIMING, 1)
            rows = []
            for _ in range(a.reps):
                call()
                rows.append(lib.lyman_alpha_forest_ms())
            lib.set_option(_capi.OPT_TIMING, 0)
            rows = np.array(rows)
            out["stage_ms"] = dict(zip(STAGES, (float(t) for t in np.median(rows, axis=0))))
            out["stage_ms_min_max_optical_depth"] = [float(rows[:, 1].min()), float(rows[:, 1].max())]
            if axis == 2:
                evals = erf_evaluations(R, x, n, T, v, axis, vscale, b_scale, tau_scale, W)
                out["erf_evaluations"] = evals
                out["terms_in_window"] = (2 * W + 1) * N ** 3
                rate = evals / (out["stage_ms"]["optical_depth_and_gaps"] * 1e-3)
                out["erf_per_s"] = rate
                out["share_of_fp64_peak"] = rate * a.flops_per_erf / (a.fp64_tflops * 1e12)
                planes = min(a.reference_planes, N)
                t0 = time.perf_counter()
                R.forest(x, n, T, v, axis, vscale, b_scale, tau_scale, window=W, lines=np.arange(planes * N))
                out["reference_s_scaled"] = (time.perf_counter() - t0) * N / planes
                out["reference_planes"] = planes
            print(json.dumps(out), flush=True)
    if p.cuda_is_init():
        p.device_close()


if __name__ == "__main__":
    main()
