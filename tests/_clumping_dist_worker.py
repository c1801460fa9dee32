"""Worker of tests/test_gpu_clumping.py: one rank of a world_size-N gloo job, every rank on GPU 0 with the HIP library, running
evolve3D_MPI with a clumping grid through the slab or the all-reduce device loop.
    python _clumping_dist_worker.py rank world port out.npz slab|allreduce"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def case():
    """The step both the ranks and the single-GPU comparison run (tests/cases.py, 'l24_gpu_F_37src', with a clumping grid)."""
    import cases
    c = cases.evolve_case("l24_gpu_F_37src")
    N = c["N"]
    c["clump"] = np.exp(np.random.default_rng(123).normal(1.0, 0.8, (N, N, N))).clip(1.0, 50.0)
    return c


def main():
    rank, world, port, out, exchange = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    import cases
    import pyc2ray_amd as p
    import pyc2ray_amd.evolve as ev
    from pyc2ray_amd import dist as pd

    pd.init_process_group_from_env("gloo")
    comm = pd.TorchComm()
    comm.exchange = exchange
    comm.device_loop = True
    c = case()
    N = c["N"]
    p.device_init(N, 8, device_id=0)
    p.photo_table_to_device(c["thin"], c["thick"])
    xh, phi = ev.evolve3D_MPI(c["dt"], c["dr"], c["flux"], c["pos"], True, 1000, N, 1e-2, pd.MPI, comm, rank, world, c["temp"],
                              c["ndens"], c["xh"], c["thin"], c["thick"], cases.MINLOGTAU, c["dlogtau"], c["R"],
                              c["convergence_fraction"], cases.SIG, cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0,
                              cases.ABU_C, logfile=None, quiet=True, clumping=c["clump"])
    np.savez(out, xh=np.array(xh), phi=np.array(phi), niter=ev._evolve.last_niter)
    p.device_close()
    comm.Barrier()
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
