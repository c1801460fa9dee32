#!/usr/bin/env python3
"""Per-iteration cost of the LLS opacity (asora_lls_opacity) against the loop without it at BASELINE configs[2] (256^3, 1000
sources, r_RT = 32): raytrace and fused pass timed separately (HIP events, ASORA_OPT_TIMING) on bench.py's uniform workload, with
the opacity off, with (0, 0) set explicitly, and with a uniform absorber density worth `--tau-cell` per cell.  The modes are run in
turn, `--rounds` times, so that a drift of the box shows in every mode alike.  With absorbers the medium is more opaque: its
trace is another trace, not a slower form of the same one.
    python tools/time_lls.py [--N 256] [--nsrc 1000] [--R 32] [--rounds 3] [--tau-cell 0.05] [--out file.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (workloads and tables of the benchmark)


def run_step(lib, capi, chem, R, dr, dlog, numtau, nsrc, N, lls):
    conv_fraction = 1e-4
    crit = min(int(conv_fraction * N ** 3), (nsrc - 1) / 3)
    if lls is not None:
        lib.lls_opacity(*lls)
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
    finally:
        lib.lls_opacity(0.0, 0.0)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--nsrc", type=int, default=1000)
    ap.add_argument("--R", type=float, default=32.0)
    ap.add_argument("--numtau", type=int, default=bench.NUMTAU)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tau-cell", type=float, default=0.05, help="sig * n_const * dr of the mode with absorbers")
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
    chem = (bench.MYR, bench.BH00, bench.ALBPOW, bench.COLH0, bench.TEMPH0, bench.ABU_C)
    ndens, xh, temp, dr, pos, flux = bench.make_workload("uniform", N, nsrc)
    p0, f0 = format_sources(pos, flux)
    lib.source_data_to_device(p0, f0, nsrc)
    lib.grid_to_device(capi.GRID_NDENS, ndens)
    lib.grid_to_device(capi.GRID_TEMP, temp)
    modes = {"off": None, "zeros": (0.0, 0.0), "absorbers": (a.tau_cell / (bench.SIG * dr), 0.0)}
    rows = {m: [] for m in modes}
    for _ in range(a.rounds):
        for m, lls in modes.items():
            lib.grid_to_device(capi.GRID_XH, xh)
            rows[m] += run_step(lib, capi, chem, R, dr, dlog, numtau, nsrc, N, lls)
    result = {"workload": f"{N}^3 uniform medium, {nsrc} sources, r_RT = {R:g}, numtau = {a.numtau}, {a.rounds} rounds",
              "build": lib.build_id(), "absorbers": {"n_const": modes["absorbers"][0], "tau_cell": a.tau_cell}}
    for m, r in rows.items():
        rt, ch = [v[0] for v in r], [v[1] for v in r]
        result[m] = {"iterations": len(r), "raytrace_ms_mean": float(np.mean(rt)), "raytrace_ms_median": float(np.median(rt)),
                     "pass_ms_mean": float(np.mean(ch)), "pass_ms_median": float(np.median(ch)),
                     "raytrace_ms": [round(v, 4) for v in rt], "pass_ms": [round(v, 4) for v in ch]}
        print(m, json.dumps({k: v for k, v in result[m].items() if not isinstance(v, list)}), flush=True)
    p.device_close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
