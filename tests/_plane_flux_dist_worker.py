"""Worker of tests/test_gpu_plane_flux.py: one rank of a world_size-N gloo job, every rank on GPU 0 with the HIP library, running
evolve3D_MPI(plane_flux=) with a communicator set up for the slab exchange (which then runs the all-reduce device loop), for the
all-reduce device loop, and for the three-call loop, in turn.  With world = 1 (backend nccl = RCCL, PYC2RAY_AMD_FORCE_COLLECTIVE=1):
the one-GPU evolve3D(plane_flux=) step, then the same step on the loop evolve3D_MPI runs across ranks, with one rank -- the only
configuration that enqueues batches of several iterations, beyond convergence too.
    python _plane_flux_dist_worker.py rank world port out.npz [backend]"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOOPS = ("slab", "allreduce", "threecalls")


def case():
    """The step both the ranks and the single-GPU comparison run: 24^3, R = 6, four sources sharded two and two, and two faces."""
    import cases
    N = 24
    nd, xh, dr = cases.grid(N, "lognormal", 34, 0.15, xlo=1e-4, xhi=2e-3)
    thin, thick, dlog = cases.soft_tables()
    pos = np.array([(3, 7, 7), (22, 16, 16), (12, 12, 12), (7, 20, 4)]).T.copy()           # (3, ns), 1-based
    return dict(N=N, ndens=nd, xh=xh, dr=dr, temp=np.full((N, N, N), 1e4), pos=pos, flux=np.full(4, 1.5e-4), thin=thin, thick=thick,
                dlogtau=dlog, R=6.0, dt=2 * cases.MYR, conv=1e-4, faces=(("+x", 3.0e-45), ("-z", 1.5e-45)))


def _world1_step(ev, pd, lib, capi, comm, c, faces):
    """The step on the loop evolve3D_MPI takes across ranks with faces, with one rank: strategy, prologue, the faces set for the
    duration, the ranks' device loop on reduce_begin (on RCCL: eight iterations per poll)."""
    import cases
    from pyc2ray_amd.load_extensions import load_asora
    from pyc2ray_amd.planeflux import plane_flux_reset
    N = c["N"]
    assert ev._loop_strategy(lib, comm, True, faces) == "all-reduce"
    scalars = ev._scalars(c["dt"], c["dr"], c["R"], c["conv"], cases.SIG, cases.MINLOGTAU, c["dlogtau"],
                          (cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C), None, True)
    uploads = {capi.GRID_NDENS: c["ndens"], capi.GRID_TEMP: c["temp"], capi.GRID_XH: c["xh"]}
    with plane_flux_reset(faces, load_asora):
        step = ev._prologue(lib, scalars, N, c["thin"].shape[0], c["flux"], c["pos"], c["flux"], uploads, None,
                            ranks=(pd.MPI, comm, 0, 1), xh_copies=True, faces=faces)
        niter = ev._ranks_device_loop(lib, step, comm, functools.partial(comm.reduce_begin, lib), "step with faces")
    assert lib.get_plane_flux() == []
    g = lambda which: lib.grid_to_host(which, np.empty((N, N, N)))
    return g(capi.GRID_XH_INTERMED), g(capi.GRID_PHI_ION), niter


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    backend = sys.argv[5] if len(sys.argv) > 5 else "gloo"
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    import cases
    import pyc2ray_amd as p
    import pyc2ray_amd.evolve as ev
    from pyc2ray_amd import dist as pd
    from pyc2ray_amd.load_extensions import load_asora
    from pyc2ray_amd.planeflux import PlaneFlux

    from pyc2ray_amd import _capi as capi
    pd.init_process_group_from_env(backend)
    c = case()
    N = c["N"]
    faces = [PlaneFlux(f, x) for f, x in c["faces"]]
    p.device_init(N, 8, device_id=0)
    p.photo_table_to_device(c["thin"], c["thick"])
    results = {}
    if world == 1:
        xh, phi = p.evolve3D(c["dt"], c["dr"], c["flux"], c["pos"], True, 1000, N, 1e-2, c["temp"], c["ndens"], c["xh"], c["thin"],
                             c["thick"], cases.MINLOGTAU, c["dlogtau"], c["R"], c["conv"], cases.SIG, cases.BH00, cases.ALBPOW,
                             cases.COLH0, cases.TEMPH0, cases.ABU_C, logfile=None, quiet=True, plane_flux=faces)
        results.update(one_xh=np.array(xh), one_phi=np.array(phi), one_niter=ev._evolve.last_niter)
        for loop in LOOPS[:2]:
            comm = pd.TorchComm()
            comm.exchange = "slab" if loop == "slab" else "allreduce"
            comm.device_loop = True
            xh, phi, niter = _world1_step(ev, pd, load_asora(), capi, comm, c, faces)
            results.update({f"{loop}_xh": xh, f"{loop}_phi": phi, f"{loop}_niter": niter})
    for loop in (LOOPS if world > 1 else ()):
        comm = pd.TorchComm()
        comm.exchange = "slab" if loop == "slab" else "allreduce"
        comm.device_loop = loop != "threecalls"
        assert ev._loop_strategy(load_asora(), comm, True, faces) == ("three calls" if loop == "threecalls" else "all-reduce")
        xh, phi = ev.evolve3D_MPI(c["dt"], c["dr"], c["flux"], c["pos"], True, 1000, N, 1e-2, pd.MPI, comm, rank, world, c["temp"],
                                  c["ndens"], c["xh"], c["thin"], c["thick"], cases.MINLOGTAU, c["dlogtau"], c["R"], c["conv"],
                                  cases.SIG, cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C, logfile=None, quiet=True,
                                  plane_flux=faces)
        assert load_asora().get_plane_flux() == []                               # (left switched off on every rank)
        results.update({f"{loop}_xh": np.array(xh), f"{loop}_phi": np.array(phi), f"{loop}_niter": ev._evolve.last_niter})
    np.savez(out, **results)
    p.device_close()
    pd.TorchComm().Barrier()
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
