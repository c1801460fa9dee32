#!/usr/bin/env python
"""Times the bispectrum on the device: a whole asora_bispectrum call (host clock around the synchronising
call) and each of its stages (HIP events, ASORA_OPT_TIMING) on a field with ionisation fronts, for (a) 8 shells and every triangle,
(b) 16 shells and every triangle, (c) 8 shells and the equilateral triangles -- each with the counts computed and with the counts
kept from the call before.  Next to them: the time of an asora_smooth_field call with a 0/1 radial table, 2 n_shells of which are
what the composed route costs before any product; the bytes the product stage reads from the cubes, and the rate that makes of its
time; and how far the counts are from integers.  A fourth case, (d), is one shell that holds every mode: the cost of a shell's three passes
back when no column can be skipped.  One JSON line per case.  Not a test.

    python tools/time_bispectrum.py [--mesh 256] [--reps 7] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ("mean_density", "along_k", "along_j", "along_i", "binning", "shell_fields", "products", "count_shell_fields", "count_products")


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)))


def field_with_fronts(N, seed):
    """ionised spheres with fronts a cell wide in a neutral box, a log-normal density, a warm gas"""
    rng = np.random.default_rng(seed)
    c = np.arange(N)
    x = np.zeros((N, N, N))
    for _ in range(24):
        o, r = rng.integers(0, N, 3), rng.uniform(0.03, 0.12) * N
        d = [np.minimum(np.abs(c - o[q]), N - np.abs(c - o[q])) for q in range(3)]
        dist = np.sqrt(d[0][:, None, None] ** 2 + d[1][None, :, None] ** 2 + d[2][None, None, :] ** 2)
        x = np.maximum(x, np.clip(r - dist + 0.5, 0.0, 1.0))
    n = 1e-4 * np.exp(0.5 * rng.normal(size=(N, N, N)))
    return x, n, 1e4 * np.ones((N, N, N))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    from pyc2ray_amd.bispectrum import bispectrum_spec
    lib = load_asora()
    N = a.mesh
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)
    for which, grid in zip((_capi.GRID_XH, _capi.GRID_NDENS, _capi.GRID_TEMP), field_with_fronts(N, N)):
        lib.grid_to_device(which, grid)
    w_r = np.zeros(3 * (N // 2) ** 2 + 1)
    w_r[7:13] = 1.0
    smooth = timed(lambda: lib.smooth_field(_capi.PS_HI, 27.0, 30.0, w_r=w_r), a.reps, a.warmup)
    lib.set_option(_capi.OPT_TIMING, 1)
    stages = []
    for _ in range(a.reps):
        lib.smooth_field(_capi.PS_HI, 27.0, 30.0, w_r=w_r)
        stages.append(lib.smooth_field_ms())
    lib.set_option(_capi.OPT_TIMING, 0)
    smooth["inverse_passes_ms"] = float(np.median(np.array(stages), axis=0)[4:7].sum())
    # (d): one shell that holds every mode, so that no column is pruned: what a shell's three passes back cost in full
    for name, shells, triangles in (("a", 8, "all"), ("b", 16, "all"), ("c", 8, "equilateral"), ("d", [0.5, N // 2 + 0.5], "equilateral")):
        spec = bispectrum_spec("time_bispectrum", N, shells=shells, triangles=triangles)
        shells = len(spec["edges"]) - 1
        thr, tri = spec["thresholds"], spec["triangles"]
        other = thr.copy()
        other[-1] += 1
        plan = lib.bispectrum_plan(N, shells, len(tri))
        used = [len(set(tri[q:q + plan["chunk"]].ravel().tolist())) for q in range(0, len(tri), plan["chunk"])]
        cube_bytes = float(sum(used)) * N ** 3 * 8
        out = dict(case=name, N=N, n_shells=shells, n_triangles=int(len(tri)), plan=plan, reps=a.reps, warmup=a.warmup,
                   smooth_field_call_ms=smooth, composed_route_ms=2 * shells * smooth["median"], product_cube_bytes=cube_bytes)
        kept = lambda: lib.bispectrum(_capi.PS_HI, 27.0, 30.0, thr, tri)

        def computed():
            lib.bispectrum(_capi.PS_HI, 27.0, 30.0, other, tri[:1])      # (one triangle of other shells: the kept counts are not these)
            return lib.bispectrum(_capi.PS_HI, 27.0, 30.0, thr, tri)
        lib.set_option(_capi.OPT_TIMING, 0)
        got = computed()
        out["kept_call_ms"] = timed(kept, a.reps, a.warmup)
        lib.set_option(_capi.OPT_TIMING, 1)
        for label, call in (("computed", computed), ("kept", kept)):
            stages = []
            for _ in range(a.reps):
                call()
                stages.append(lib.bispectrum_ms())
            med = np.median(np.array(stages), axis=0)
            out[label + "_stage_ms"] = dict(zip(STAGES, (float(v) for v in med)))
            out[label + "_total_ms"] = float(med.sum())
        lib.set_option(_capi.OPT_TIMING, 0)
        out["product_GB_per_s"] = cube_bytes / (out["computed_stage_ms"]["products"] * 1e-3) / 1e9
        resid = np.abs(got["sum_iii"] - np.rint(got["sum_iii"]))
        out["count_residual"] = float(resid.max())
        out["largest_count"] = float(got["sum_iii"].max())
        out["shell_width"] = float(spec["edges"][1] - spec["edges"][0])
        print(json.dumps(out), flush=True)
    if p.cuda_is_init():
        p.device_close()


if __name__ == "__main__":
    main()
