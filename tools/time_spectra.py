#!/usr/bin/env python3
"""Cost of per-source spectra (asora_spectra_to_device) on the raytrace at BASELINE configs[2] (256^3, 1000 sources, r_RT = 32):
the trace of bench.py's uniform workload timed with HIP events (ASORA_OPT_TIMING) with one table set, and with two sets and 10 %
and 50 % of the sources on the second, at NumTau = 2000 and 20000 -- what the larger table footprint costs the caches.  The
configurations are run in turn, `--rounds` times, so that a drift of the box shows in every one alike.
    python tools/time_spectra.py [--N 256] [--nsrc 1000] [--R 32] [--rounds 3] [--reps 10] [--out file.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (workloads and tables of the benchmark)


def time_trace(lib, capi, R, dr, dlog, numtau, nsrc, reps):
    lib.raytrace_device(R, bench.SIG, dr, 0, nsrc, bench.MINLOGTAU, dlog, numtau)      # warm-up: geometry tables, zero probe
    out = []
    for _ in range(reps):
        lib.kernel_time_reset()
        lib.raytrace_device(R, bench.SIG, dr, 0, nsrc, bench.MINLOGTAU, dlog, numtau)
        lib.synchronize()
        out.append(lib.kernel_time_ms(capi.KERNEL_RAYTRACE)[0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--nsrc", type=int, default=1000)
    ap.add_argument("--R", type=float, default=32.0)
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
    p.device_init(N, 8)
    lib.set_option(capi.OPT_TIMING, 1)
    ndens, xh, temp, dr, pos, flux = bench.make_workload("uniform", N, nsrc)
    p0, f0 = format_sources(pos, flux)
    lib.grid_to_device(capi.GRID_NDENS, ndens)
    lib.grid_to_device(capi.GRID_XH_AV, xh)
    rng = np.random.default_rng(11)
    result = {"workload": f"{N}^3 uniform medium, {nsrc} sources, r_RT = {R:g}, {a.rounds} rounds x {a.reps} traces",
              "build": lib.build_id()}
    for num_tau in (2000, 20000):
        thin, thick, dlog = bench.make_tables(num_tau)
        numtau = thin.shape[0]
        # the second set: a hotter black body on the same tau grid, built like bench.make_tables builds the first
        from pyc2ray_amd.radiation import BlackBodySource, make_tau_table
        ev2fr = 0.241838e15
        tau, _ = make_tau_table(bench.MINLOGTAU, bench.MAXLOGTAU, num_tau)
        hard_thin, hard_thick = BlackBodySource(2e5, False, ev2fr * 13.598, 2.8).make_photo_table(
            tau, ev2fr * 13.598, 10 * ev2fr * 54.416, 1e48)
        two = (np.stack([thin, hard_thin]), np.stack([thick, hard_thick]))
        configs = {"one set": None, "two sets, all sources on the first": 0.0, "two sets, 10 % on the second": 0.1,
                   "two sets, 50 % on the second": 0.5}
        rows = {k: [] for k in configs}
        for _ in range(a.rounds):
            for name, share in configs.items():
                if share is None:
                    p.photo_table_to_device(thin, thick)
                else:
                    lib.spectra_to_device(*two)
                lib.source_data_to_device(p0, f0, nsrc)
                if share:
                    spec = np.zeros(nsrc, dtype=np.int32)
                    spec[rng.permutation(nsrc)[:int(round(share * nsrc))]] = 1
                    lib.source_spectra_to_device(spec)
                rows[name] += time_trace(lib, capi, R, dr, dlog, numtau, nsrc, a.reps)
        result[f"NumTau {num_tau}"] = {k: {"raytrace_ms_median": float(np.median(v)), "raytrace_ms_min": float(np.min(v)),
                                           "raytrace_ms_max": float(np.max(v)), "raytrace_ms": [round(x, 4) for x in v]}
                                       for k, v in rows.items()}
        for k, v in rows.items():
            print(f"NumTau {num_tau}: {k}: median {np.median(v):.4f} ms (min {np.min(v):.4f}, max {np.max(v):.4f})", flush=True)
    p.device_close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
