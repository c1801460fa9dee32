"""Worker of tests/test_gpu_lls.py: one rank of a world_size-N gloo job, every rank on GPU 0 with the HIP library, running
evolve3D_MPI with LLS opacity through each of the four loops across ranks in turn (slab, all-reduce, pipelined, three calls).
    python _lls_dist_worker.py rank world port out.npz"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOOPS = ("slab", "allreduce", "pipelined", "threecalls")


def case():
    """The step both the ranks and the single-GPU comparison run (tests/cases.py, 'l24_gpu_F_37src', with LLS opacity: a uniform
    absorber density worth tau = 0.05 per cell, and one absorber per five atoms)."""
    import cases
    from pyc2ray_amd.lls import LLSOpacity
    c = cases.evolve_case("l24_gpu_F_37src")
    c["lls"] = LLSOpacity(0.05 / (cases.SIG * c["dr"]), 0.2)
    return c


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    import cases
    import pyc2ray_amd as p
    import pyc2ray_amd.evolve as ev
    from pyc2ray_amd import dist as pd
    from pyc2ray_amd.load_extensions import load_asora

    pd.init_process_group_from_env("gloo")
    c = case()
    N = c["N"]
    p.device_init(N, 8, device_id=0)
    p.photo_table_to_device(c["thin"], c["thick"])
    results = {}
    for loop in LOOPS:
        comm = pd.TorchComm(overlap=True, chunks=4, pipeline_chemistry=True) if loop == "pipelined" else pd.TorchComm()
        comm.exchange = "slab" if loop == "slab" else "allreduce"
        comm.device_loop = loop != "threecalls"
        assert ev._loop_strategy(load_asora(), comm, True) == {"allreduce": "all-reduce", "threecalls": "three calls"}.get(loop, loop)
        xh, phi = ev.evolve3D_MPI(c["dt"], c["dr"], c["flux"], c["pos"], True, 1000, N, 1e-2, pd.MPI, comm, rank, world, c["temp"],
                                  c["ndens"], c["xh"], c["thin"], c["thick"], cases.MINLOGTAU, c["dlogtau"], c["R"],
                                  c["convergence_fraction"], cases.SIG, cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0,
                                  cases.ABU_C, logfile=None, quiet=True, lls=c["lls"])
        assert load_asora().get_lls_opacity() == (0.0, 0.0)          # (left switched off on every rank)
        results.update({f"{loop}_xh": np.array(xh), f"{loop}_phi": np.array(phi), f"{loop}_niter": ev._evolve.last_niter})
    np.savez(out, **results)
    p.device_close()
    pd.TorchComm().Barrier()
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
