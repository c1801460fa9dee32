#!/usr/bin/env python3
"""Per-iteration cost of the thermal mode against the isothermal loop at BASELINE configs[2] (256^3, 1000 sources, r_RT = 32):
raytrace and fused pass timed separately (HIP events, ASORA_OPT_TIMING), on the headline's quiet medium (bench.py's uniform
workload, the first time step) and on a field with ionisation fronts (the log-normal medium with fluxes x 1e3: the second
1 Myr time step, as bench.py --evolving-state), with the thermal substep statistics (asora_thermal_stats) next to the times.
    python tools/time_thermal.py [--N 256] [--nsrc 1000] [--R 32] [--out file.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (workloads and tables of the benchmark)


def heat_tables(numtau):
    from pyc2ray_amd.radiation import BlackBodySource, make_tau_table
    ev2fr = 0.241838e15
    tau, _ = make_tau_table(bench.MINLOGTAU, bench.MAXLOGTAU, numtau)
    src = BlackBodySource(1e5, False, ev2fr * 13.598, 2.8)
    return src.make_heat_table(tau, ev2fr * 13.598, 10 * ev2fr * 54.416, 1e48)


def run_step(lib, capi, chem, R, dr, dlog, numtau, nsrc, N, thermal):
    conv_fraction = 1e-4
    crit = min(int(conv_fraction * N ** 3), (nsrc - 1) / 3)
    if thermal:
        lib.thermal_params(True)
    try:
        lib.evolve_begin(*chem, R, bench.SIG, dr, bench.MINLOGTAU, dlog, numtau, 0, nsrc, crit, conv_fraction)
        rows, done = [], False
        while not done and len(rows) < 200:
            lib.kernel_time_reset()
            lib.evolve_enqueue(1)
            _, done, _ = lib.evolve_poll(4)
            rt, _ = lib.kernel_time_ms(capi.KERNEL_RAYTRACE)
            ch, _ = lib.kernel_time_ms(capi.KERNEL_CHEMISTRY)
            rows.append((rt, ch))
        stats = lib.thermal_stats() if thermal else None
    finally:
        lib.thermal_params(False)
    return rows, stats


def summary(rows, stats):
    rt = [r[0] for r in rows]
    ch = [r[1] for r in rows]
    out = {"iterations": len(rows), "raytrace_ms_mean": float(np.mean(rt)), "pass_ms_mean": float(np.mean(ch)),
           "raytrace_ms": [round(v, 4) for v in rt], "pass_ms": [round(v, 4) for v in ch]}
    if stats is not None:
        out.update({"cells_max_substeps": stats[0], "cells_floored": stats[1], "max_substeps_used": stats[2]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--nsrc", type=int, default=1000)
    ap.add_argument("--R", type=float, default=32.0)
    ap.add_argument("--numtau", type=int, default=bench.NUMTAU)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi as capi
    from pyc2ray_amd.load_extensions import load_asora
    from pyc2ray_amd.utils.sourceutils import format_sources
    lib = load_asora()
    N, nsrc, R = a.N, a.nsrc, a.R
    thin, thick, dlog = bench.make_tables(a.numtau)
    hthin, hthick = heat_tables(a.numtau)
    p.device_init(N, 8)
    p.photo_table_to_device(thin, thick)
    lib.heat_table_to_device(hthin, hthick, thin.shape[0])
    numtau = thin.shape[0]
    lib.set_option(capi.OPT_TIMING, 1)
    chem = (bench.MYR, bench.BH00, bench.ALBPOW, bench.COLH0, bench.TEMPH0, bench.ABU_C)
    result = {"workload": f"{N}^3, {nsrc} sources, r_RT = {R:g}, numtau = {a.numtau}", "build": lib.build_id()}
    for medium in ("quiet", "fronts"):
        kind, scale = ("uniform", 1.0) if medium == "quiet" else ("cosmo", 1e3)
        ndens, xh, temp, dr, pos, flux = bench.make_workload(kind, N, nsrc)
        p0, f0 = format_sources(pos, flux * scale)
        lib.source_data_to_device(p0, f0, nsrc)
        lib.grid_to_device(capi.GRID_NDENS, ndens)
        for mode in ("isothermal", "thermal"):
            lib.grid_to_device(capi.GRID_TEMP, temp)
            lib.grid_to_device(capi.GRID_XH, xh)
            thermal = mode == "thermal"
            if medium == "fronts":       # the second time step: it starts with the fronts of the first
                run_step(lib, capi, chem, R, dr, dlog, numtau, nsrc, N, thermal)
                lib.grid_copy(capi.GRID_XH, capi.GRID_XH_INTERMED)
                if thermal:
                    lib.grid_copy(capi.GRID_TEMP, capi.GRID_TEMP_END)
            rows, stats = run_step(lib, capi, chem, R, dr, dlog, numtau, nsrc, N, thermal)
            result[f"{medium}_{mode}"] = summary(rows, stats)
            print(medium, mode, json.dumps({k: v for k, v in result[f"{medium}_{mode}"].items() if not isinstance(v, list)}),
                  flush=True)
    p.device_close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
