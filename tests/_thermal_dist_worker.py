"""Worker of tests/test_gpu_thermal_ranks.py: one rank of a torch.distributed job on GPU 0 with the HIP library, running two
consecutive thermal steps -- the second from the first's x and T, with another source set -- through the slab or the all-reduce
device loop.
    python _thermal_dist_worker.py rank world port out.npz slab|allreduce oracle|identity|clumped|iso_after|iso_fresh [gloo|nccl]
iso_after: the thermal steps of "oracle", then an isothermal evolve3D_MPI step (keys iso_*); iso_fresh: that isothermal step alone.
world >= 2 (gloo, every rank on GPU 0): evolve3D_MPI(thermal=tp).  world == 1 (nccl = RCCL; evolve3D_MPI takes the distributed
branch only with nprocs > 1): the same loop driven through the functions evolve3D_MPI drives it with, batches of eight
iterations per poll, after the one-GPU evolve3D(thermal=tp) of the same steps, which is saved beside it (keys one_*)."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N = 24
P2 = 2.0 ** -35
CLUMP = 3.0
#: cooling: all five channels, Compton at z = 8
ZRED, MAX_SUBSTEPS = 8.0, 10000
#: the seed of the medium and of the sources' second and third coordinates (chosen so that the oracle loop converges, with at
#: least 3 outer iterations in both steps: tests/test_gpu_thermal_ranks.py asserts it before any rank starts)
SEED = 4243


def _lattice(ns, rng):
    """ns sources on the lattice of spacing N // 2 (one on a box corner): with 2 floor(R) < N // 2 no two spheres share a cell.
    The spheres at first coordinate 1 + N // 2 straddle plane N // 2, those at 1 wrap through plane 0."""
    h = N // 2
    pts = np.array([(1 + a * h, 1 + b * h, 1 + c * h) for a in (0, 1) for b in (0, 1) for c in (0, 1)]).T
    pick = np.concatenate([[0], 1 + rng.permutation(7)[:ns - 1]])
    return pts[:, pick]


def case(kind):
    """The two steps every rank and the comparison run.  kind = "oracle" / "clumped": black-body photo and heating tables, eight
    and nine overlapping sources of radius 4 and 5 whose first coordinates put both ranks' reach across plane N / 2 and two
    spheres through plane 0; "identity": heating tables = 2^-35 x the photo tables, non-overlapping sources on the N / 2 lattice."""
    import cases
    rng = np.random.default_rng(SEED)
    thin, thick, hthin, hthick, dlog = cases.blackbody_photo_and_heat_tables(num_tau=600)
    if kind == "identity":
        hthin, hthick = P2 * thin, P2 * thick
    nd, xh, dr = cases.grid(N, "lognormal", SEED, 0.3, xlo=1e-4, xhi=2e-3)
    temp = 10 ** rng.uniform(2.0, 4.0, size=(N, N, N))
    steps = []
    # 1-based first coordinates: sorted and cut in two, rank 0 traces the first half.  Step 0: rank 0 reaches planes 20..23 (the
    # sphere at plane 0 wraps) and 12..14, rank 1 reaches 8..11 and 0..1 (the sphere at plane 21 wraps)
    for first, R in (([1, 6, 10, 11, 14, 15, 19, 22], 4.0), ([3, 8, 9, 12, 13, 13, 17, 20, 24], 5.0)):
        ns = len(first)
        if kind == "identity":
            ns, R = (8, 4.0) if not steps else (6, 2.5)
            pos = _lattice(ns, rng)
        else:
            pos = np.stack([np.array(first), 1 + rng.integers(0, N, ns), 1 + rng.integers(0, N, ns)])
            pos = pos[:, rng.permutation(ns)]
        flux = rng.uniform(0.5, 2.0, size=ns) * 3e-4 * (N / 16.0) ** 3 / ns
        steps.append(dict(pos=pos, flux=flux, R=R))
    return dict(N=N, thin=thin, thick=thick, hthin=hthin, hthick=hthick, dlog=dlog, ndens=nd, xh=xh, temp=temp, dr=dr,
                dt=3.15576e13 * 2.0, steps=steps, clumping=CLUMP if kind == "clumped" else None)


def thermal_params(c):
    from pyc2ray_amd.thermal import ThermalParams
    return ThermalParams(c["hthin"], c["hthick"], relative_denergy=0.1, t_floor=1.0, max_substeps=MAX_SUBSTEPS, cooling=31, zred=ZRED)


def reference_params():
    import thermal_reference as TR
    return TR.Params(relative_denergy=0.1, t_floor=1.0, max_substeps=MAX_SUBSTEPS, cooling_mask=31, compton=True,
                     t_cmb=2.7255 * (1.0 + ZRED))


def _chem():
    import cases
    return (cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)


def _one_gpu(p, lib, capi, c, tp):
    """The two steps through evolve3D(thermal=tp) on this process's GPU."""
    import cases
    out, x, T = {}, c["xh"], c["temp"]
    for k, s in enumerate(c["steps"]):
        x, phi, T = p.evolve3D(c["dt"], c["dr"], s["flux"], s["pos"], True, 1000, N, 1e-2, T, c["ndens"], x, c["thin"], c["thick"],
                               cases.MINLOGTAU, c["dlog"], s["R"], 1e-4, cases.SIG, *_chem(), logfile=None, quiet=True, thermal=tp,
                               clumping=c["clumping"])
        x, T = np.array(x), np.array(T)
        out.update({f"one_xh{k}": x, f"one_temp{k}": T, f"one_phi{k}": np.array(phi), f"one_niter{k}": p.evolve._evolve.last_niter,
                    f"one_heat{k}": lib.grid_to_host(capi.GRID_PHI_HEAT, np.empty((N, N, N))),
                    f"one_stats{k}": np.array(p.evolve._evolve.last_thermal_stats)})
    return out


def _world1_step(ev, pd, lib, capi, comm, c, tp, s, x, T):
    """One thermal step on the loop evolve3D_MPI runs across ranks, with one rank: its prologue, the plan, the ranks' device loop
    (on RCCL: eight iterations per poll), the gathers."""
    import cases
    ranks = (pd.MPI, comm, 0, 1)
    scalars = ev._scalars(c["dt"], c["dr"], s["R"], 1e-4, cases.SIG, cases.MINLOGTAU, c["dlog"], _chem(), None, True)
    uploads = {capi.GRID_NDENS: c["ndens"], capi.GRID_TEMP: T, capi.GRID_XH: x}
    if comm.exchange == "slab":
        pos, flux, _ = comm.shard_sources_by_slab(s["pos"], s["flux"], 1)
        plan = pd.SlabPlan(N, 1, s["R"], [pos[0] - 1])
        begin = functools.partial(comm.slab_begin, lib, plan)
    else:
        pos, flux, plan = s["pos"], s["flux"], None
        begin = functools.partial(comm.reduce_begin, lib)
    step = ev._prologue(lib, scalars, N, c["thin"].shape[0], s["flux"], pos, flux, uploads, None, ranks=ranks, xh_copies=True)
    niter = ev._ranks_device_loop(lib, step, comm, begin, "thermal step", tp)
    if plan is not None:
        for which in (capi.GRID_XH_INTERMED, capi.GRID_PHI_ION, capi.GRID_TEMP_END, capi.GRID_PHI_HEAT):
            comm.slab_gather(lib, plan, which, N)
    g = lambda which: lib.grid_to_host(which, np.empty((N, N, N)))
    return g(capi.GRID_XH_INTERMED), g(capi.GRID_PHI_ION), g(capi.GRID_TEMP_END), niter


def main():
    rank, world, port, out, exchange, kind = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5], sys.argv[6]
    backend = sys.argv[7] if len(sys.argv) > 7 else "gloo"
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    import cases
    import pyc2ray_amd as p
    import pyc2ray_amd.evolve as ev
    from pyc2ray_amd import _capi as capi
    from pyc2ray_amd import dist as pd
    from pyc2ray_amd.load_extensions import load_asora

    pd.init_process_group_from_env(backend)
    comm = pd.TorchComm()
    comm.exchange = exchange
    comm.device_loop = True
    c = case(kind)
    tp = thermal_params(c)
    lib = load_asora()
    p.device_init(N, 8, device_id=0)
    p.photo_table_to_device(c["thin"], c["thick"])
    res = _one_gpu(p, lib, capi, c, tp) if world == 1 else {}
    x, T = c["xh"], c["temp"]
    for k, s in enumerate(c["steps"] if kind != "iso_fresh" else []):
        if world == 1:
            x, phi, T, niter = _world1_step(ev, pd, lib, capi, comm, c, tp, s, x, T)
        else:
            x, phi, T = ev.evolve3D_MPI(c["dt"], c["dr"], s["flux"], s["pos"], True, 1000, N, 1e-2, pd.MPI, comm, rank, world, T,
                                        c["ndens"], x, c["thin"], c["thick"], cases.MINLOGTAU, c["dlog"], s["R"], 1e-4, cases.SIG,
                                        *_chem(), logfile=None, quiet=True, thermal=tp, clumping=c["clumping"])
            niter = ev._evolve.last_niter
        x, T = np.array(x), np.array(T)
        heat = lib.grid_to_host(capi.GRID_PHI_HEAT, np.empty((N, N, N)))
        # hygiene: the step leaves the library isothermal and unclumped
        lib.evolve_begin_slab(c["dt"], *_chem(), s["R"], cases.SIG, c["dr"], cases.MINLOGTAU, c["dlog"], c["thin"].shape[0], 0, 0,
                              -1.0, 0.0, 0, N)                  # (fails while thermal mode is on)
        res.update({f"xh{k}": x, f"temp{k}": T, f"phi{k}": np.array(phi), f"heat{k}": heat, f"niter{k}": niter,
                    f"stats{k}": np.array(ev._evolve.last_thermal_stats)})
    if kind.startswith("iso_"):
        s = c["steps"][0]
        xi, phi = ev.evolve3D_MPI(c["dt"], c["dr"], s["flux"], s["pos"], True, 1000, N, 1e-2, pd.MPI, comm, rank, world, c["temp"],
                                  c["ndens"], c["xh"], c["thin"], c["thick"], cases.MINLOGTAU, c["dlog"], s["R"], 1e-4, cases.SIG,
                                  *_chem(), logfile=None, quiet=True)
        res.update(iso_xh=np.array(xi), iso_phi=np.array(phi), iso_niter=ev._evolve.last_niter)
    np.savez(out, **res)
    p.device_close()
    comm.Barrier()
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
