#!/usr/bin/env python
"""Times the halo-catalogue sources on the device at 256^3 with 10^7 haloes: the catalogue call (upload,
bin, row counts and scan, the download of n_cells with the allocations it sizes, table; HIP events under ASORA_OPT_TIMING, and the
host clock around the whole call, of which what lies outside the stages is reported as `host_ms_outside_stages`) for a clustered
catalogue -- tests/halo_sources_reference.clustered: positions in proportion to a log-normal density, masses from dn/dM ~ M^-2
between 1e8 and 1e13 -- and for a uniform one, with the bin kernel's 64-bit atomic adds per second on each; the per-step build
(flux, scan, emit, and the whole call with the list's download) for subsets of the uniform catalogue with some 10^5 and 10^6
occupied cells and for the full catalogues.  Yardsticks from the same run: the numpy statement of the table, and what a host-side
suppression costs per step -- one grid_to_host of the ionised fraction plus the statement's per-step part.  One JSON line per case.
Not a test.

    python tools/time_halo_sources.py [--mesh 256] [--haloes 10000000] [--seed 2561] [--sigma 1.5] [--reps 11] [--warmup 2]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from time_power_spectrum import timed      # noqa: E402

CATALOGUE_STAGES = ("upload", "bin", "count_scan", "room", "table")
BUILD_STAGES = ("flux", "scan", "emit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, default=256)
    ap.add_argument("--haloes", type=int, default=10_000_000)
    ap.add_argument("--seed", type=int, default=2561)
    ap.add_argument("--sigma", type=float, default=1.5)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import halo_sources_reference as R
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    N, n = a.mesh, a.haloes
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)
    rng = np.random.default_rng(a.seed)
    x = rng.random((N, N, N)) ** 3                     # 46 % of the cells above x_suppress = 0.1
    lib.grid_to_device(_capi.GRID_XH, x)
    pos_c, mass = R.clustered(N, n, a.seed, a.sigma)
    pos_u = rng.uniform(0.0, N, size=(n, 3))
    e = R.unit_exponent(mass)
    holder = np.empty((N, N, N))
    build_args = (_capi.GRID_XH, 30.0, 130.0, 1.0e-9, _capi.HALO_MODEL_FULL, 0.1, 0.0)

    def stages(call, read, names, reps):
        lib.set_option(_capi.OPT_TIMING, 1)
        rows = []
        for _ in range(reps):
            call()
            rows.append(read())
        lib.set_option(_capi.OPT_TIMING, 0)
        rows = np.array(rows)
        return {name: dict(median=float(np.median(rows[:, q])), min=float(rows[:, q].min()), max=float(rows[:, q].max()))
                for q, name in enumerate(names)}

    def build_case(case, pos, m, extra):
        counts = lib.halo_catalogue_to_device(pos, m, m, 1e8, 1e9, True, e)
        call = lambda: lib.halo_sources_build(*build_args)
        out = dict(case=case, N=N, haloes=int(m.size), n_cells=counts["n_cells"], n_active=int(call()["summary"][0]), reps=a.reps, warmup=a.warmup)
        out["call_ms"] = timed(call, a.reps, a.warmup)
        out["stage_ms"] = stages(call, lambda: lib.halo_sources_ms()[5:], BUILD_STAGES, a.reps)
        out["list_bytes"] = 20 * out["n_active"]
        if extra:
            table = lib.halo_table_to_host()
            def host_route():
                got = lib.grid_to_host(_capi.GRID_XH, holder)
                return R.build(*table, got, *build_args[1:])
            out["grid_to_host_ms"] = timed(lambda: lib.grid_to_host(_capi.GRID_XH, holder), max(3, a.reps // 3), 1)
            out["download_and_numpy_ms"] = timed(host_route, max(3, a.reps // 3), 1)
        print(json.dumps(out), flush=True)

    for name, pos in (("clustered", pos_c), ("uniform", pos_u)):
        call = lambda: lib.halo_catalogue_to_device(pos, mass, mass, 1e8, 1e9, True, e)
        counts = call()
        per_cell = np.bincount(((np.floor(pos[:, 0]).astype(np.int64) % N) * N + np.floor(pos[:, 1]).astype(np.int64) % N) * N
                               + np.floor(pos[:, 2]).astype(np.int64) % N, minlength=N ** 3)
        out = dict(case="catalogue_" + name, N=N, haloes=n, seed=a.seed, sigma=a.sigma if name == "clustered" else None, counts=counts,
                   most_haloes_in_a_cell=int(per_cell.max()), unit_exponent=e, reps=a.reps, warmup=a.warmup)
        out["call_ms"] = timed(call, a.reps, a.warmup)
        out["stage_ms"] = stages(call, lambda: lib.halo_sources_ms()[:5], CATALOGUE_STAGES, a.reps)
        out["host_ms_outside_stages"] = out["call_ms"]["median"] - sum(v["median"] for v in out["stage_ms"].values())
        adds = n - counts["below"] - counts["outside"] - counts["nonfinite"]
        out["atomic_adds"] = adds
        out["atomic_adds_per_s"] = adds / (out["stage_ms"]["bin"]["median"] * 1e-3)
        out["upload_gb_per_s"] = 40.0 * n / (out["stage_ms"]["upload"]["median"] * 1e-3) / 1e9
        out["numpy_table_ms"] = timed(lambda: R.table(pos, mass, mass, N, 1e8, 1e9, True, e), 3, 0)
        print(json.dumps(out), flush=True)
    for target in (120_000, 1_300_000):
        build_case("build_uniform", pos_u[:target], mass[:target], True)
    build_case("build_uniform", pos_u, mass, False)
    build_case("build_clustered", pos_c, mass, True)
    if p.cuda_is_init():
        p.device_close()


if __name__ == "__main__":
    main()
