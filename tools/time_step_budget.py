#!/usr/bin/env python3
"""Cost of one asora_step_budget call (the photon budget of a time step) next to the fused pass of the
same process, at 256^3 on bench.py's uniform workload, in its three configurations: clumping off (6 grids, 48 B per cell), a
clumping grid (56 B), a thermal step (use_temp_end, 56 B).  Each configuration runs one time step of the device loop to convergence
(the pass's time per iteration: HIP events, ASORA_OPT_TIMING, ASORA_KERNEL_CHEMISTRY), then calls the budget `--reps` times on the
grids the step left: the device time per call (both of its kernels, counted under ASORA_KERNEL_FINISH) and the host's wall time
per call, which adds the launch, the 96-byte copy and the synchronisation.
    python tools/time_step_budget.py [--N 256] [--nsrc 1000] [--R 32] [--reps 50] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (workloads and tables of the benchmark)

CONFIGS = {"clumping off": 48, "clumping grid": 56, "thermal": 56}       # bytes per cell the budget's pass loads


def run_step(lib, capi, chem, R, dr, dlog, numtau, nsrc, N):
    """one time step of the device loop; the fused pass's ms of each iteration"""
    conv_fraction = 1e-4
    crit = min(int(conv_fraction * N ** 3), (nsrc - 1) / 3)
    lib.evolve_begin(*chem, R, bench.SIG, dr, bench.MINLOGTAU, dlog, numtau, 0, nsrc, crit, conv_fraction)
    passes, done = [], False
    while not done and len(passes) < 200:
        lib.kernel_time_reset()
        lib.evolve_enqueue(1)
        _, done, _ = lib.evolve_poll(4)
        passes.append(lib.kernel_time_ms(capi.KERNEL_CHEMISTRY)[0])
    return passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--nsrc", type=int, default=1000)
    ap.add_argument("--R", type=float, default=32.0)
    ap.add_argument("--numtau", type=int, default=bench.NUMTAU)
    ap.add_argument("--reps", type=int, default=50)
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
    lib.heat_table_to_device(1e-11 * thin, 0.7e-11 * thick, thin.shape[0])
    numtau = thin.shape[0]
    lib.set_option(capi.OPT_TIMING, 1)
    chem = (bench.MYR, bench.BH00, bench.ALBPOW, bench.COLH0, bench.TEMPH0, bench.ABU_C)
    ndens, xh, temp, dr, pos, flux = bench.make_workload("uniform", N, nsrc)
    p0, f0 = format_sources(pos, flux)
    lib.source_data_to_device(p0, f0, nsrc)
    lib.grid_to_device(capi.GRID_NDENS, ndens)
    clump = np.exp(np.random.default_rng(1).normal(1.0, 0.8, (N, N, N))).clip(1.0, 50.0)
    result = {"workload": f"{N}^3 uniform medium, {nsrc} sources, r_RT = {R:g}, numtau = {a.numtau}, {a.reps} calls per configuration",
              "build": lib.build_id()}
    for name, bytes_per_cell in CONFIGS.items():
        lib.grid_to_device(capi.GRID_TEMP, temp)
        lib.grid_to_device(capi.GRID_XH, xh)
        thermal = name == "thermal"
        if name == "clumping grid":
            lib.grid_to_device(capi.GRID_CLUMP, clump)
            lib.clumping(2)
        if thermal:
            lib.thermal_params(True)
        try:
            passes = run_step(lib, capi, chem, R, dr, dlog, numtau, nsrc, N)
        finally:
            lib.thermal_params(False)
        try:
            first = lib.step_budget(chem, use_temp_end=thermal)             # (allocates the buffers; not timed)
            lib.synchronize()
            lib.kernel_time_reset()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                sums = lib.step_budget(chem, use_temp_end=thermal)
            wall_ms = (time.perf_counter() - t0) * 1e3 / a.reps
            dev_total, launches = lib.kernel_time_ms(capi.KERNEL_FINISH)
        finally:
            lib.clumping(0)
        assert sums.tobytes() == first.tobytes() and launches == a.reps
        dev_ms = dev_total / launches
        result[name] = {"budget_device_ms": dev_ms, "budget_wall_ms": wall_ms, "bytes_per_cell": bytes_per_cell,
                        "TB_per_s": bytes_per_cell * N ** 3 / (dev_ms * 1e-3) / 1e12, "fused_pass_ms_median": float(np.median(passes)),
                        "fused_pass_ms": [round(v, 4) for v in passes], "iterations": len(passes),
                        "budget_over_pass": dev_ms / float(np.median(passes)),
                        "mean_xh_mass": sums[capi.BUDGET_NX] / sums[capi.BUDGET_N]}
        print(name, json.dumps({k: v for k, v in result[name].items() if not isinstance(v, list)}), flush=True)
    p.device_close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
