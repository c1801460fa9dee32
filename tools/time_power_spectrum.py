#!/usr/bin/env python
"""Times the power spectrum on the device: a whole asora_power_spectrum call (host clock around the
synchronising call) and each of its stages (HIP events, ASORA_OPT_TIMING) at 128^3, 250^3 and 256^3, for the auto-spectrum of the
brightness temperature and for its cross-spectrum with the density.  Where torch sees the device, ``torch.fft.rfftn`` of the same
array (rocFFT) is timed as a yardstick for the three transform passes.  One JSON line per mesh.  Not a test.

    python tools/time_power_spectrum.py [--meshes 128 250 256] [--reps 11] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, nargs="+", default=[128, 250, 256])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    from pyc2ray_amd.powerspec import powerspec_spec
    lib = load_asora()
    try:
        import torch
        have_torch = torch.cuda.is_available()
    except ImportError:
        have_torch = False
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
        thr = powerspec_spec("time_power_spectrum", N)["thresholds"]
        out = dict(N=N, n_bins=int(thr.size - 1), reps=a.reps, warmup=a.warmup)
        for name, kind_b in (("auto", None), ("cross", _capi.PS_DENSITY)):
            call = lambda: lib.power_spectrum(_capi.PS_HI, kind_b, 27.0, 30.0, thr)
            lib.set_option(_capi.OPT_TIMING, 0)
            out[name + "_call_ms"] = timed(call, a.reps, a.warmup)
            lib.set_option(_capi.OPT_TIMING, 1)
            stages = []
            for _ in range(a.reps):
                call()
                stages.append(lib.power_spectrum_ms())
            lib.set_option(_capi.OPT_TIMING, 0)
            med = np.median(np.array(stages), axis=0)
            out[name + "_stage_ms"] = dict(zip(("mean_density", "along_k", "along_j", "along_i", "binning"), (float(v) for v in med)))
        if have_torch:
            g = torch.from_numpy((27.0 * (1.0 - x)) * (n / n.mean())).cuda()

            def fft():
                torch.fft.rfftn(g)
                torch.cuda.synchronize()
            out["torch_rfftn_ms"] = timed(fft, a.reps, a.warmup)
            s = out["auto_stage_ms"]
            out["transform_over_torch_rfftn"] = (s["along_k"] + s["along_j"] + s["along_i"]) / out["torch_rfftn_ms"]["median"]
            del g
        print(json.dumps(out), flush=True)
    if p.cuda_is_init():
        p.device_close()


if __name__ == "__main__":
    main()
