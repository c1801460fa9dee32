#!/usr/bin/env python3
"""What the thermal mode costs on the two device loops across ranks, on ONE GPU under a world-1 RCCL group (the build box has one
GPU: nothing can be measured between two): ms per iteration of the sharded ("slab") and the all-reduce loop against the one-GPU
loop in the same process, thermal and isothermal, at BASELINE configs[3] (256^3 log-normal density, 1000 sources, r_RT = 32),
iterations that never converge, in batches of eight per poll.  PYC2RAY_AMD_FORCE_COLLECTIVE=1 is set, so the all-reduces of the
out-boxes really run.  Also the kernel time of the combined fold-out of a thermal step (rates and heating in one launch) against
two launches of the isothermal one, on half the planes.
    python tools/time_thermal_ranks.py [--N 256] [--nsrc 1000] [--R 32] [--out file.json]"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench  # noqa: E402
from time_thermal import heat_tables  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--nsrc", type=int, default=1000)
    ap.add_argument("--R", type=float, default=32.0)
    ap.add_argument("--numtau", type=int, default=bench.NUMTAU)
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["PYC2RAY_AMD_FORCE_COLLECTIVE"] = "1"
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi as capi
    from pyc2ray_amd import dist as pd
    from pyc2ray_amd.load_extensions import load_asora
    from pyc2ray_amd.utils.sourceutils import format_sources
    lib = load_asora()
    N, nsrc, R = a.N, a.nsrc, a.R
    thin, thick, dlog = bench.make_tables(a.numtau)
    hthin, hthick = heat_tables(a.numtau)
    numtau = thin.shape[0]
    p.device_init(N, 8)
    p.photo_table_to_device(thin, thick)
    lib.heat_table_to_device(hthin, hthick, numtau)
    pd.init_process_group_from_env("nccl")
    comm = pd.TorchComm()
    ndens, xh, temp, dr, pos, flux = bench.make_workload("cosmo", N, nsrc)
    spos, sflux, _ = comm.shard_sources_by_slab(pos, flux, 1)
    plan = pd.SlabPlan(N, 1, R, [spos[0] - 1])
    p0, f0 = format_sources(spos, sflux)
    lib.source_data_to_device(p0, f0, nsrc)
    chem = (bench.MYR, bench.BH00, bench.ALBPOW, bench.COLH0, bench.TEMPH0, bench.ABU_C)
    never = (-1.0, 0.0)                                       # a convergence test that never passes
    rt = (R, bench.SIG, dr, bench.MINLOGTAU, dlog, numtau)

    def upload():
        for which, g in ((capi.GRID_NDENS, ndens), (capi.GRID_TEMP, temp), (capi.GRID_XH, xh)):
            lib.grid_to_device(which, g)

    def timed(begin, enqueue, poll):
        """Median over `repeats` regions of `iterations` iterations, eight per poll, after one untimed batch."""
        upload()
        begin()
        enqueue(8); poll()
        lib.synchronize()
        out = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            done = 0
            while done < a.iterations:
                n = min(8, a.iterations - done)
                enqueue(n); poll()
                done += n
            lib.synchronize()
            out.append((time.perf_counter() - t0) * 1e3 / a.iterations)
        return {"ms_per_iteration": float(np.median(out)), "min": float(min(out)), "max": float(max(out))}

    result = {"workload": f"{N}^3 log-normal, {nsrc} sources, r_RT = {R:g}, numtau = {a.numtau}; world-1 RCCL group, collectives forced",
              "build": lib.build_id(), "iterations_per_region": a.iterations, "repeats": a.repeats}
    for thermal in (False, True):
        tag = "thermal" if thermal else "isothermal"
        if thermal:
            lib.thermal_params(True)
        try:
            one = timed(lambda: lib.evolve_begin(*chem, *rt, 0, nsrc, *never), lib.evolve_enqueue, lambda: lib.evolve_poll(0))
            comm.exchange = "slab"
            slab = timed(lambda: comm.slab_begin(lib, plan, N, *rt[:3], nsrc, *rt[3:], chem, *never, thermal=thermal),
                         lambda n: comm.slab_enqueue(lib, n), lambda: comm.slab_poll(lib, 0))
            comm.exchange = "allreduce"
            red = timed(lambda: comm.reduce_begin(lib, N, *rt[:3], nsrc, *rt[3:], chem, *never, thermal=thermal),
                        lambda n: comm.slab_enqueue(lib, n), lambda: comm.slab_poll(lib, 0))
        finally:
            lib.thermal_params(False)
        result[tag] = {"one_gpu_loop": one, "world1_slab": slab, "world1_allreduce": red,
                       "slab_over_one_gpu": slab["ms_per_iteration"] / one["ms_per_iteration"],
                       "allreduce_over_one_gpu": red["ms_per_iteration"] / one["ms_per_iteration"]}
        print(tag, json.dumps(result[tag]), flush=True)

    # the combined fold-out: this process owns the lower half of the planes and folds the upper half out
    lib.set_option(capi.OPT_TIMING, 1)
    half = N // 2
    fold = {}
    for thermal in (False, True):
        if thermal:
            lib.thermal_params(True)
        try:
            upload()
            (lib.evolve_begin_slab_thermal if thermal else lib.evolve_begin_slab)(*chem, *rt, 0, nsrc, *never, 0, half)
            lib.evolve_slab_trace(0, nsrc)
            lib.evolve_slab_fold_out(half, N - half)
            lib.synchronize()
            lib.kernel_time_reset()
            for _ in range(20):
                lib.evolve_slab_fold_out(half, N - half)
            lib.synchronize()
            ms, n = lib.kernel_time_ms(capi.KERNEL_FINISH)
            fold["pair_one_launch" if thermal else "single"] = {"ms_per_launch": ms / max(n, 1), "launches": n, "planes": N - half}
        finally:
            lib.thermal_params(False)
    fold["two_single_launches_ms"] = 2.0 * fold["single"]["ms_per_launch"]
    result["fold_out"] = fold
    print("fold_out", json.dumps(fold), flush=True)
    p.device_close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    import torch.distributed as dist
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
