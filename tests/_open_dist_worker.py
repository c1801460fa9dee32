"""Worker of tests/test_gpu_open_boundaries.py: one rank of a world_size-N gloo job, every rank on GPU 0 with the HIP library,
running evolve3D_MPI(periodic=False) through the two device loops across ranks in turn (slab exchange, all-reduce).
    python _open_dist_worker.py rank world port out.npz"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOOPS = ("slab", "allreduce")


def case():
    """The step both the ranks and the single-GPU comparison run: 24^3, R = 8, four sources of which one sits on the first and one
    on the last plane -- with two ranks the planes their periodic traces would wrap into are the other rank's."""
    import cases
    N = 24
    nd, xh, dr = cases.grid(N, "lognormal", 34, 0.15, xlo=1e-4, xhi=2e-3)
    thin, thick, dlog = cases.soft_tables()
    pos = np.array([(1, 7, 7), (24, 16, 16), (12, 12, 12), (7, 20, 4)]).T.copy()           # (3, ns), 1-based
    return dict(N=N, ndens=nd, xh=xh, dr=dr, temp=np.full((N, N, N), 1e4), pos=pos, flux=np.full(4, 1.5e-4), thin=thin, thick=thick,
                dlogtau=dlog, R=8.0, dt=3 * cases.MYR, conv=1e-4)


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    import cases
    import pyc2ray_amd as p
    import pyc2ray_amd.evolve as ev
    from pyc2ray_amd import _capi
    from pyc2ray_amd import dist as pd
    from pyc2ray_amd.load_extensions import load_asora

    pd.init_process_group_from_env("gloo")
    c = case()
    N = c["N"]
    p.device_init(N, 8, device_id=0)
    p.photo_table_to_device(c["thin"], c["thick"])
    results = {}
    for loop in LOOPS:
        comm = pd.TorchComm()
        comm.exchange = "slab" if loop == "slab" else "allreduce"
        comm.device_loop = True
        assert ev._loop_strategy(load_asora(), comm, True) == {"allreduce": "all-reduce"}.get(loop, loop)
        xh, phi = ev.evolve3D_MPI(c["dt"], c["dr"], c["flux"], c["pos"], True, 1000, N, 1e-2, pd.MPI, comm, rank, world, c["temp"],
                                  c["ndens"], c["xh"], c["thin"], c["thick"], cases.MINLOGTAU, c["dlogtau"], c["R"], c["conv"],
                                  cases.SIG, cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C, logfile=None, quiet=True,
                                  periodic=False)
        assert load_asora().last_raytrace_variant()["open"]
        assert load_asora().get_option(_capi.OPT_OPEN_BOUNDARIES) == 0          # (left periodic on every rank)
        results.update({f"{loop}_xh": np.array(xh), f"{loop}_phi": np.array(phi), f"{loop}_niter": ev._evolve.last_niter})
    np.savez(out, **results)
    p.device_close()
    pd.TorchComm().Barrier()
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
