#!/usr/bin/env python3
"""Mean raytrace launch time with periodic and with open boundaries (ASORA_OPT_OPEN_BOUNDARIES) at BASELINE configs[2] (256^3
uniform medium, 1000 sources, r_RT = 32) and configs[3] (the log-normal medium, sources on the densest cells): whole-list
asora_raytrace_device calls timed with HIP events (ASORA_OPT_TIMING) on bench.py's workloads.  The modes alternate call by
call, `--rounds` times `--reps` calls each, so that a drift of the box shows in every mode alike:
  periodic         the library's defaults
  periodic_noskip  periodic with ASORA_OPT_SKIP_ZERO_RATES = 2: the open forms add exact zeros as well, so this is the like-for-like
  open             ASORA_OPT_OPEN_BOUNDARIES = 1
On a library without the option (an older build selected with PYC2RAY_AMD_LIBASORA) only the periodic modes run.
    python tools/time_open_boundaries.py [--N 256] [--nsrc 1000] [--R 32] [--rounds 3] [--reps 10] [--out file.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (workloads and tables of the benchmark)

OPT_OPEN_BOUNDARIES = 18


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--nsrc", type=int, default=1000)
    ap.add_argument("--R", type=float, default=32.0)
    ap.add_argument("--numtau", type=int, default=bench.NUMTAU)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi as capi
    from pyc2ray_amd.load_extensions import load_asora
    from pyc2ray_amd.utils.sourceutils import format_sources
    lib = load_asora()
    N, nsrc, R = a.N, a.nsrc, a.R
    thin, thick, dlog = bench.make_tables(a.numtau)
    p.device_init(N, 8)
    p.photo_table_to_device(thin, thick)
    numtau = thin.shape[0]
    lib.set_option(capi.OPT_TIMING, 1)
    modes = {"periodic": {}, "periodic_noskip": {capi.OPT_SKIP_ZERO_RATES: 2}}
    if lib.get_option(OPT_OPEN_BOUNDARIES) == 0:             # (-1: the library does not know the option)
        modes["open"] = {OPT_OPEN_BOUNDARIES: 1}
    result = {"build": lib.build_id(), "rounds": a.rounds, "reps": a.reps}
    for kind, label in (("uniform", "configs[2]"), ("cosmo", "configs[3]")):
        ndens, xh, temp, dr, pos, flux = bench.make_workload(kind, N, nsrc)
        p0, f0 = format_sources(pos, flux)
        lib.source_data_to_device(p0, f0, nsrc)
        lib.grid_to_device(capi.GRID_NDENS, ndens)
        lib.grid_to_device(capi.GRID_XH_AV, xh)
        ms = {m: [] for m in modes}
        info = {}

        def trace(m, timed=True):
            for o, v in modes[m].items():
                lib.set_option(o, v)
            try:
                lib.kernel_time_reset()
                lib.raytrace_device(R, bench.SIG, dr, 0, nsrc, bench.MINLOGTAU, dlog, numtau)
                t, n = lib.kernel_time_ms(capi.KERNEL_RAYTRACE)
            finally:
                for o in modes[m]:
                    lib.set_option(o, 0)
            if timed:
                ms[m].append(t / max(n, 1))
            info[m] = dict(lib.last_raytrace_variant(), rated_pairs=lib.last_raytrace_counts()[0], launches=n)

        for m in modes:                                      # warm-up: geometry tables, the zero-rate probe
            for _ in range(3):
                trace(m, timed=False)
        for _ in range(a.rounds):
            for _ in range(a.reps):
                for m in modes:
                    trace(m)
        block = {"workload": f"BASELINE {label}: {N}^3 {kind} medium, {nsrc} sources, r_RT = {R:g}, numtau = {a.numtau}"}
        for m, v in ms.items():
            block[m] = {"launch_ms_mean": float(np.mean(v)), "launch_ms_median": float(np.median(v)), "launch_ms_min": float(np.min(v)),
                        "launch_ms_max": float(np.max(v)), "calls": len(v), "variant": info[m], "launch_ms": [round(x, 4) for x in v]}
            print(label, m, json.dumps({k: x for k, x in block[m].items() if k != "launch_ms"}), flush=True)
        # the library caches the geometry tables of ONE launch shape: modes that differ in it would rebuild them at every switch
        shapes = {m: (info[m]["units"], info[m]["threads"], info[m]["aligned"]) for m in modes}
        block["same_launch_shape_in_every_mode"] = len(set(shapes.values())) == 1
        if not block["same_launch_shape_in_every_mode"]:
            print(label, "WARNING: the modes take different launch shapes", shapes, "-- alternating them rebuilds the geometry tables "
                  "between calls (host time, not in the launch times)", flush=True)
        result[label] = block
    p.device_close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
