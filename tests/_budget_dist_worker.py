"""Worker of tests/test_gpu_budget.py: one rank of a world_size-N gloo job, every rank on GPU 0 with the HIP library, running
evolve3D_MPI with budget=StepBudget() through the slab and the all-reduce device loops.  Every GPU step runs under a time limit
of its own (SIGALRM ends the process), and the first failure ends the worker.
    python _budget_dist_worker.py rank world port out.npz"""
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEP_LIMIT_S = 120
EXCHANGES = ("slab", "allreduce")
FIELDS = ("emitted", "new_ions", "photoionisations", "lls_absorbed", "recombinations", "collisional", "mean_xh_volume",
          "mean_xh_mass", "mean_xh_mass_before", "mean_temp", "mean_temp_mass")


def case():
    """The step both the ranks and the single-GPU comparison run (tests/cases.py, 'l24_gpu_F_37src': 24^3, 37 sources)."""
    import cases
    return cases.evolve_case("l24_gpu_F_37src")


def evolve(ev, c, ranks=None, budget=None):
    """(xh, phi, niter) of one step; ranks = (MPI, comm, rank, world) or None for the single-GPU evolve3D."""
    import cases
    N = c["N"]
    head = (c["dt"], c["dr"], c["flux"], c["pos"], True, 1000, N, 1e-2)
    tail = (c["temp"], c["ndens"], c["xh"], c["thin"], c["thick"], cases.MINLOGTAU, c["dlogtau"], c["R"], c["convergence_fraction"],
            cases.SIG, cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)
    kw = dict(logfile=None, quiet=True)
    if budget is not None:
        kw["budget"] = budget
    xh, phi = ev.evolve3D(*head, *tail, **kw) if ranks is None else ev.evolve3D_MPI(*head, *ranks, *tail, **kw)
    return np.array(xh), np.array(phi), ev._evolve.last_niter


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    import pyc2ray_amd as p
    import pyc2ray_amd.evolve as ev
    from pyc2ray_amd import dist as pd
    from pyc2ray_amd.budget import StepBudget

    pd.init_process_group_from_env("gloo")
    comm = pd.TorchComm()
    comm.device_loop = True
    c = case()
    signal.alarm(STEP_LIMIT_S)
    p.device_init(c["N"], 8, device_id=0)
    p.photo_table_to_device(c["thin"], c["thick"])
    res = {}
    for exchange in EXCHANGES:
        comm.exchange = exchange
        b = StepBudget()
        signal.alarm(STEP_LIMIT_S)
        xh, phi, niter = evolve(ev, c, (pd.MPI, comm, rank, world), b)
        signal.alarm(0)
        res.update({f"{exchange}_xh": xh, f"{exchange}_phi": phi, f"{exchange}_niter": niter, f"{exchange}_sums": b.sums,
                    f"{exchange}_fields": np.array([getattr(b, k) for k in FIELDS])})
    np.savez(out, **res)
    p.device_close()
    comm.Barrier()
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
