"""Worker of tests/test_gpu_spectra_ranks.py: one rank of a world_size-N gloo job, every rank on GPU 0 with the HIP library, running
evolve3D_MPI with two spectra through the slab or the all-reduce device loop.  Every GPU step runs under a time limit of its own
(SIGALRM ends the process), and the first failure ends the worker.
    python _spectra_dist_worker.py rank world port out.npz slab|allreduce"""
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEP_LIMIT_S = 120


def hard_tables(num_tau=2000):
    """(thin, thick) of a second, harder spectrum on the tau grid of cases.soft_tables: half the photons, a tail that falls more
    slowly with the optical depth, so not proportional to the soft pair.  Like that pair, thick falls monotonically and
    thin = -d thick / d tau: a thick table that rises anywhere gives negative rates T(tau_in) - T(tau_out), and the outer
    iteration of a step then alternates between two states instead of converging."""
    import cases
    tau, _ = cases.tau_table(num_tau)
    thick = 0.5e48 * (0.3 * np.exp(-tau) + 0.7 / (1.0 + tau) ** 2)
    thin = 0.5e48 * (0.3 * np.exp(-tau) + 1.4 / (1.0 + tau) ** 3)
    return thin, thick


def case():
    """The step both the ranks and the single-GPU comparison run (tests/cases.py, 'l24_gpu_F_37src'), with a second, harder
    table set and a spectrum per source."""
    import cases
    c = cases.evolve_case("l24_gpu_F_37src")
    hard_thin, hard_thick = hard_tables(c["thin"].shape[0] - 1)
    c["spectra"] = (np.stack([c["thin"], hard_thin]), np.stack([c["thick"], hard_thick]))
    c["spec"] = np.random.RandomState(77).randint(0, 2, c["flux"].shape[0])
    return c


def evolve(p, ev, c, ranks=None, spectrum=True):
    """(xh, phi, niter) of one step; ranks = (MPI, comm, rank, world) or None for the single-GPU evolve3D."""
    import cases
    N = c["N"]
    head = (c["dt"], c["dr"], c["flux"], c["pos"], True, 1000, N, 1e-2)
    tail = (c["temp"], c["ndens"], c["xh"], c["thin"], c["thick"], cases.MINLOGTAU, c["dlogtau"], c["R"], c["convergence_fraction"],
            cases.SIG, cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)
    kw = dict(logfile=None, quiet=True, src_spectrum=c["spec"] if spectrum else None)
    xh, phi = ev.evolve3D(*head, *tail, **kw) if ranks is None else ev.evolve3D_MPI(*head, *ranks, *tail, **kw)
    return np.array(xh), np.array(phi), ev._evolve.last_niter


def main():
    rank, world, port, out, exchange = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    import pyc2ray_amd as p
    import pyc2ray_amd.evolve as ev
    from pyc2ray_amd import dist as pd

    pd.init_process_group_from_env("gloo")
    comm = pd.TorchComm()
    comm.exchange = exchange
    comm.device_loop = True
    c = case()
    signal.alarm(STEP_LIMIT_S)
    p.device_init(c["N"], 8, device_id=0)
    p.spectra_to_device(*c["spectra"])
    signal.alarm(STEP_LIMIT_S)
    xh, phi, niter = evolve(p, ev, c, (pd.MPI, comm, rank, world))
    signal.alarm(0)
    np.savez(out, xh=xh, phi=phi, niter=niter)
    p.device_close()
    comm.Barrier()
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
