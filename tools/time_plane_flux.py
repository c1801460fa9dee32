#!/usr/bin/env python3
"""Time of one face's sweep of the plane-parallel flux (asora_plane_flux) at 256^3, for each of the six
faces, without and with heating: asora_raytrace_device calls with no point source and one face, timed with HIP events around the
launch (ASORA_OPT_TIMING) on bench.py's log-normal medium.  The twelve modes alternate call by call, `--reps` calls each, so that
a drift of the box shows in every mode alike.  Each time is also stated as a share of the streaming rate the fused pass reaches on
the same box (6.0 TB/s), from the sweep's algorithmic bytes: n_abs read, the accumulator read and written -- 24 B per
cell, 40 B with heating.
Writes profiles/time_plane_flux.json (--out) and prints the rows of the table in DESIGN.md section 4.1d, which are pasted from here.
    python tools/time_plane_flux.py [--N 256] [--reps 20] [--out file.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (workloads and tables of the benchmark)

STREAM_TBS = 6.0
FACES = ("-x", "+x", "-y", "+y", "-z", "+z")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--numtau", type=int, default=bench.NUMTAU)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_plane_flux.json"), help="'' = write no file")
    a = ap.parse_args()
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi as capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    N = a.N
    thin, thick, dlog = bench.make_tables(a.numtau)
    p.device_init(N, 8)
    p.photo_table_to_device(thin, thick)
    numtau = thin.shape[0]
    lib.heat_table_to_device(1e-11 * thin, 0.7e-11 * thick, numtau)
    ndens, xh, _temp, dr, _pos, _flux = bench.make_workload("cosmo", N, 8)
    lib.source_data_to_device(np.zeros(0, dtype=np.int32), np.zeros(0), 0)
    lib.grid_to_device(capi.GRID_NDENS, ndens)
    lib.grid_to_device(capi.GRID_XH_AV, xh)
    lib.set_option(capi.OPT_TIMING, 1)
    modes = [(f, heat) for heat in (False, True) for f in range(6)]
    ms = {m: [] for m in modes}

    def sweep(m, timed=True):
        face, heat = m
        lib.set_option(capi.OPT_HEATING, 1 if heat else 0)
        lib.plane_flux([face], [1.0e-6])
        try:
            lib.kernel_time_reset()
            lib.raytrace_device(32.0, bench.SIG, dr, 0, 0, bench.MINLOGTAU, dlog, numtau)
            t, n = lib.kernel_time_ms(capi.KERNEL_RAYTRACE)
        finally:
            lib.plane_flux((), ())
            lib.set_option(capi.OPT_HEATING, 0)
        assert n == 1, n
        if timed:
            ms[m].append(t)

    for m in modes:
        for _ in range(2):
            sweep(m, timed=False)
    for _ in range(a.reps):
        for m in modes:
            sweep(m)
    result = {"build": lib.build_id(), "N": N, "reps": a.reps, "stream_TBs": STREAM_TBS,
              "workload": f"bench.py's log-normal medium at {N}^3, numtau = {a.numtau}, no point source, one face per call"}
    for (face, heat), v in ms.items():
        bytes_ = (40 if heat else 24) * N ** 3
        mean = float(np.mean(v))
        row = {"ms_mean": mean, "ms_median": float(np.median(v)), "ms_min": float(np.min(v)), "ms_max": float(np.max(v)),
               "TBs": bytes_ / (mean * 1e-3) / 1e12, "share_of_stream": bytes_ / (mean * 1e-3) / 1e12 / STREAM_TBS, "calls": len(v),
               "ms": [round(x, 4) for x in v]}
        result[f"{FACES[face]}{' heat' if heat else ''}"] = row
        print(FACES[face], "heat" if heat else "    ", json.dumps({k: x for k, x in row.items() if k != "ms"}), flush=True)
    p.device_close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(markdown_rows(result))


def markdown_rows(result):
    """The rows of DESIGN.md's table: face | ms mean (min ... max) | TB/s | share | the same with heating."""
    cell = lambda r: f"{r['ms_mean']:.3f} ({r['ms_min']:.3f} ... {r['ms_max']:.3f}) | {r['TBs']:.2f} | {100 * r['share_of_stream']:.0f} %"
    return "\n".join(f"| {f} | {cell(result[f])} | {cell(result[f + ' heat'])} |" for f in FACES)


if __name__ == "__main__":
    main()
