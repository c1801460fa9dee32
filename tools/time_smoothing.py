#!/usr/bin/env python
"""Times the smoothing on the device: a whole asora_smooth_field call (host clock around the synchronising
call) and each of its stages (HIP events, ASORA_OPT_TIMING) at 256^3 and 250^3, for the brightness temperature through
``telescope(3, 3)`` with the mean removed and a histogram of 64 bins; and, in the same run, a whole auto-spectrum call of the same
field, and the ratio of the three inverse passes to the three forward passes.  One JSON line per mesh.  Not a test.

    python tools/time_smoothing.py [--meshes 256 250] [--reps 11] [--warmup 2] [--fwhm 3] [--width 3]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_power_spectrum import timed      # noqa: E402

STAGES = ("mean_density", "forward_k", "forward_j", "forward_i", "back_i_filter", "back_j", "back_k_stats", "moments_hist")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, nargs="+", default=[256, 250])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fwhm", type=float, default=3.0)
    ap.add_argument("--width", type=float, default=3.0)
    a = ap.parse_args()
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    from pyc2ray_amd.powerspec import powerspec_spec
    from pyc2ray_amd.smoothing import telescope
    lib = load_asora()
    for N in a.meshes:
        if p.cuda_is_init():
            p.device_close()
        p.device_init(N, 8)
        rng = np.random.default_rng(N)
        x = rng.random((N, N, N))
        n = 1e-4 * np.exp(0.5 * rng.normal(size=(N, N, N)))
        T = 1e4 * np.ones((N, N, N))
        for which, grid in ((_capi.GRID_XH, x), (_capi.GRID_NDENS, n), (_capi.GRID_TEMP, T)):
            lib.grid_to_device(which, grid)
        tables = telescope(a.fwhm, a.width).tables(N)
        edges = np.linspace(-30.0, 30.0, 65)
        thr = powerspec_spec("time_smoothing", N)["thresholds"]
        out = dict(N=N, filter=f"telescope({a.fwhm:g}, {a.width:g})", n_hist=int(edges.size - 1), reps=a.reps, warmup=a.warmup)
        call = lambda: lib.smooth_field(_capi.PS_HI, 27.0, 30.0, *tables, subtract_mean=True, edges=edges)
        spectrum = lambda: lib.power_spectrum(_capi.PS_HI, None, 27.0, 30.0, thr)
        lib.set_option(_capi.OPT_TIMING, 0)
        out["call_ms"] = timed(call, a.reps, a.warmup)
        out["power_spectrum_call_ms"] = timed(spectrum, a.reps, a.warmup)
        out["call_over_power_spectrum_call"] = out["call_ms"]["median"] / out["power_spectrum_call_ms"]["median"]
        lib.set_option(_capi.OPT_TIMING, 1)
        stages = []
        for _ in range(a.reps):
            call()
            stages.append(lib.smooth_field_ms())
        lib.set_option(_capi.OPT_TIMING, 0)
        med = np.median(np.array(stages), axis=0)
        s = out["stage_ms"] = dict(zip(STAGES, (float(v) for v in med)))
        out["stages_total_ms"] = float(med.sum())
        out["inverse_over_forward"] = (s["back_i_filter"] + s["back_j"] + s["back_k_stats"]) / (s["forward_k"] + s["forward_j"] + s["forward_i"])
        print(json.dumps(out), flush=True)
    if p.cuda_is_init():
        p.device_close()


if __name__ == "__main__":
    main()
