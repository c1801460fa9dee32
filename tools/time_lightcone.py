#!/usr/bin/env python
"""Times the light cone on the device: the four stages of asora_lightcone_advance (HIP events,
ASORA_OPT_TIMING) and the whole call (host clock around the synchronising call, the slices' download included) at 256^3 for 25
slices -- a step of dz = 0.1 near z = 8 with cells of 1 Mpc -- along each axis, for the ionised fraction (the refresh moves 16 bytes
per cell) and for the brightness temperature with and without a spin temperature (32 and 24).  On every axis the same 25 planes are
also handed over in an order without two consecutive ones, which along axis 2 takes the per-slice form of the emit instead of the
tiled one.  Two yardsticks from the same run: asora_grid_copy of one grid (16 bytes per cell), and the route the call replaces --
three grid_to_host downloads and the numpy statement (tests/lightcone_reference.py).  One JSON line per case.  Not a test.

    python tools/time_lightcone.py [--mesh 256] [--slices 25] [--reps 21] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from time_power_spectrum import timed      # noqa: E402

STAGES = ("mean_density", "emit", "moments", "refresh")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, default=256)
    ap.add_argument("--slices", type=int, default=25)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import lightcone_reference as R
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    N, M = a.mesh, a.slices
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)
    rng = np.random.default_rng(N)
    shape = (N, N, N)
    x, n, T = rng.random(shape), np.exp(0.7 * rng.normal(size=shape)), 10.0 ** rng.uniform(1.0, 4.0, shape)
    for which, grid in ((_capi.GRID_XH, x), (_capi.GRID_NDENS, n), (_capi.GRID_TEMP, T)):
        lib.grid_to_device(which, grid)
    ncell = float(N) ** 3
    # the yardsticks
    def copy():                                                     # ten in a row per synchronisation: the launch is not what is timed
        for _ in range(10):
            lib.grid_copy(_capi.GRID_XH_AV, _capi.GRID_XH)
        lib.synchronize()
    t_copy = {key: t / 10.0 for key, t in timed(copy, a.reps, a.warmup).items()}
    print(json.dumps(dict(case="grid_copy", N=N, ms=t_copy, bytes_per_cell=16, gb_per_s=16 * ncell / (t_copy["median"] * 1e-3) / 1e9)), flush=True)
    run = (40 - np.arange(M)) % N                                   # consecutive planes, descending: what the Python layer hands over
    apart = np.r_[run[0::2], run[1::2]]                             # the same planes, no two consecutive ones next to each other
    f = np.linspace(0.0, 1.0, M)
    holders = [np.empty(shape) for _ in range(3)]

    def host_route():
        got = [lib.grid_to_host(which, h) for which, h in zip((_capi.GRID_XH, _capi.GRID_NDENS, _capi.GRID_TEMP), holders)]
        g = R.form(R.HI, got[0], got[1], got[2], float(np.mean(got[1])), 27.0)
        return R.blend(g, g, run, 1.0 - f, f, 2)
    t_host = timed(host_route, max(3, a.reps // 4), 1)
    print(json.dumps(dict(case="three_downloads_and_numpy", N=N, slices=M, ms=t_host)), flush=True)
    kinds = (("xh", _capi.PS_XH, 0.0, 16), ("dtb", _capi.PS_HI, 0.0, 24), ("dtb_spin", _capi.PS_HI, 27.0, 32))
    for name, kind, tg, refresh_bytes in kinds:
        lib.lightcone_reset(0)
        lib.lightcone_advance(0, kind, None, tg, 2, (), (), (), True)
        for axis in (0, 1, 2):
            for order, planes in (("run", run), ("apart", apart)):
                call = lambda slices=True: lib.lightcone_advance(0, kind, None, tg, axis, planes, 1.0 - f, f, True, slices=slices)
                lib.set_option(_capi.OPT_TIMING, 0)
                out = dict(case=name, N=N, axis=axis, slices=M, order=order, reps=a.reps, warmup=a.warmup, refresh_bytes_per_cell=refresh_bytes)
                out["call_ms"] = timed(call, a.reps, a.warmup)
                out["call_ms_moments_only"] = timed(lambda: call(False), a.reps, a.warmup)
                lib.set_option(_capi.OPT_TIMING, 1)
                rows = []
                for _ in range(a.reps):
                    call()
                    rows.append(lib.lightcone_ms())
                lib.set_option(_capi.OPT_TIMING, 0)
                rows = np.array(rows)
                out["stage_ms"] = dict(zip(STAGES, (float(t) for t in np.median(rows, axis=0))))
                out["stage_ms_min_max_emit"] = [float(rows[:, 1].min()), float(rows[:, 1].max())]
                out["refresh_gb_per_s"] = refresh_bytes * ncell / (out["stage_ms"]["refresh"] * 1e-3) / 1e9
                out["refresh_time_per_byte_over_grid_copy"] = (out["stage_ms"]["refresh"] / refresh_bytes) / (t_copy["median"] / 16)
                print(json.dumps(out), flush=True)
    if p.cuda_is_init():
        p.device_close()


if __name__ == "__main__":
    main()
