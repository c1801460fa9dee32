#!/usr/bin/env python
"""Times the redshift-space analysis on the device: a whole asora_power_spectrum_los call (host clock
around the synchronising call) with and without a velocity, and each of its stages (HIP events, ASORA_OPT_TIMING) at 256^3 and
250^3, for the brightness temperature with the spin factor (four reads and one write per cell in the mapping) along each line of
sight, in the multipoles' bins and in 32 x 32 cylindrical bins; and, in the same run, a whole auto-spectrum call of the same field
with its stages.  The mapping's share of the HBM bandwidth is its 40 algorithmic bytes per cell over its stage time and the peak
rate given with --hbm-tbs.  One JSON line per mesh.  Not a test.

    python tools/time_redshift_space.py [--meshes 256 250] [--reps 11] [--warmup 2] [--displacement 2.5] [--hbm-tbs 8.0]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_power_spectrum import timed      # noqa: E402

STAGES = ("mean_density", "mapping", "forward_k", "forward_j", "forward_i", "binning")
PS_STAGES = ("mean_density", "forward_k", "forward_j", "forward_i", "binning")
MAP_BYTES_PER_CELL = 40                    # x, n, T and v read, h written


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, nargs="+", default=[256, 250])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--displacement", type=float, default=2.5, help="the largest displacement in cells (W = floor of it + 1)")
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="the peak HBM rate the mapping's share is taken of, TB/s")
    a = ap.parse_args()
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    from pyc2ray_amd.powerspec import powerspec_spec
    from pyc2ray_amd.redshift_space import redshift_space_spec
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
        v = rng.uniform(-a.displacement, a.displacement, size=(N, N, N))
        lib.los_velocity_to_device(v)
        thr = powerspec_spec("time_redshift_space", N)["thresholds"]
        multi = redshift_space_spec("time_redshift_space", N, binning="multipoles")
        cyl = redshift_space_spec("time_redshift_space", N)
        out = dict(N=N, displacement=a.displacement, reps=a.reps, warmup=a.warmup, hbm_peak_tbs=a.hbm_tbs,
                   bins=dict(multipoles=[int(multi["thr_a"].size - 1), 1], cylindrical=[int(cyl["thr_a"].size - 1), int(cyl["thr_b"].size - 1)]))

        def los(spec, axis, vscale):
            return lambda: lib.power_spectrum_los(_capi.PS_HI, 27.0, 30.0, axis, vscale, spec["mode"], spec["thr_a"], spec["thr_b"])

        def stage_times(call, read):
            lib.set_option(_capi.OPT_TIMING, 1)
            rows = []
            for _ in range(a.reps):
                call()
                rows.append(read())
            lib.set_option(_capi.OPT_TIMING, 0)
            return np.median(np.array(rows), axis=0)

        spectrum = lambda: lib.power_spectrum(_capi.PS_HI, None, 27.0, 30.0, thr)
        lib.set_option(_capi.OPT_TIMING, 0)
        out["power_spectrum_call_ms"] = timed(spectrum, a.reps, a.warmup)
        out["power_spectrum_stage_ms"] = dict(zip(PS_STAGES, (float(t) for t in stage_times(spectrum, lib.power_spectrum_ms))))
        out["real_space_call_ms"] = timed(los(multi, 2, None), a.reps, a.warmup)
        out["real_space_stage_ms"] = dict(zip(STAGES, (float(t) for t in stage_times(los(multi, 2, None), lib.power_spectrum_los_ms))))
        for axis in (2, 1, 0):
            for name, spec in (("multipoles", multi), ("cylindrical", cyl)):
                if name == "cylindrical" and axis != 2:
                    continue
                key = f"axis{axis}_{name}"
                call = los(spec, axis, 1.0)
                out[key + "_call_ms"] = timed(call, a.reps, a.warmup)
                s = dict(zip(STAGES, (float(t) for t in stage_times(call, lib.power_spectrum_los_ms))))
                out[key + "_stage_ms"] = s
                rate = MAP_BYTES_PER_CELL * float(N) ** 3 / (s["mapping"] * 1e-3) / 1e12
                out[key + "_mapping"] = dict(tb_per_s=rate, share_of_hbm_peak=rate / a.hbm_tbs, over_forward_k=s["mapping"] / s["forward_k"])
                out[key + "_binning_over_spherical"] = s["binning"] / out["power_spectrum_stage_ms"]["binning"]
        out["call_over_power_spectrum_call"] = out["axis2_multipoles_call_ms"]["median"] / out["power_spectrum_call_ms"]["median"]
        print(json.dumps(out), flush=True)
    if p.cuda_is_init():
        p.device_close()


if __name__ == "__main__":
    main()
