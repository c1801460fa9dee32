"""Worker of tests/test_gpu_feature_matrix.py: one rank of a world_size-N gloo job, every rank on GPU 0 with the HIP library,
running rows of the feature-combination matrix (tests/step_reference.py) through evolve3D_MPI on the two device loops across
ranks in turn: a communicator set up for the slab exchange (with faces it runs the all-reduce loop) and the all-reduce loop.
Also home of what the test and the worker share: how a row becomes the library's keywords and which tables go up for it.
    python _matrix_dist_worker.py rank world port out.npz"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOOPS = ("slab", "allreduce")
N = 24


def load_tables(p, lib, row, c):
    """The tables a row runs on: with the spectra column both table sets and their heating tables (spectra_to_device), without
    it the first set alone (photo_table_to_device; the heating tables of a thermal row then go up with its ThermalParams)."""
    import step_reference as SR
    if SR.features_of(row)["spectra"]:
        lib.spectra_to_device(*(np.stack([s[k] for s in c["sets"]]) for k in range(4)))
        assert lib.num_spectra() == 2
    else:
        p.photo_table_to_device(c["thin"], c["thick"])
        assert lib.num_spectra() == 1


def library_options(row, c):
    """The keywords of evolve3D / evolve3D_MPI / evolve3D_resident for a row on the case `c` -- what step_reference.reference_options
    is to the reference.  A row with the budget column gets a fresh StepBudget under "budget"."""
    import step_reference as SR
    from pyc2ray_amd.budget import StepBudget
    from pyc2ray_amd.lls import LLSOpacity
    from pyc2ray_amd.planeflux import PlaneFlux
    from pyc2ray_amd.thermal import ThermalParams
    f = SR.features_of(row)
    kw = {}
    if f["thermal"]:
        t = SR.THERMAL
        kw["thermal"] = ThermalParams(c["heat_thin"], c["heat_thick"], relative_denergy=t["relative_denergy"], t_floor=t["t_floor"],
                                      max_substeps=t["max_substeps"], cooling=t["cooling_mask"], zred=None)
    if f["clumping"]:
        kw["clumping"] = c["clump"]
    if f["spectra"]:
        kw["src_spectrum"] = c["spectrum"]
    if f["lls"]:
        kw["lls"] = LLSOpacity(*c["lls"])
    if f["open"]:
        kw["periodic"] = False
    if f["faces"]:
        kw["plane_flux"] = [PlaneFlux(face, x, s if f["spectra"] else 0) for face, x, s in c["faces"]]
    if f["budget"]:
        kw["budget"] = StepBudget()
    return kw


def emitted(c, kw):
    """StepBudget.emitted of the row's step, in the operations of StepBudget.fill."""
    area = (c["N"] * float(c["dr"])) ** 2
    return (float(np.sum(c["flux"])) + sum(f.flux * area for f in kw.get("plane_flux", ()))) * 1e48 * float(c["dt"])


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    import cases
    import pyc2ray_amd as p
    import pyc2ray_amd.evolve as ev
    import step_reference as SR
    from pyc2ray_amd import _capi
    from pyc2ray_amd import dist as pd
    from pyc2ray_amd.load_extensions import load_asora

    pd.init_process_group_from_env("gloo")
    lib = load_asora()
    p.device_init(N, 8, device_id=0)
    results = {}
    for row in SR.RANK_ROWS:
        c = SR.case_of(row, N)
        f = SR.features_of(row)
        load_tables(p, lib, row, c)
        for loop in LOOPS:
            comm = pd.TorchComm()
            comm.exchange = "slab" if loop == "slab" else "allreduce"
            comm.device_loop = True
            kw = library_options(row, c)
            strategy = ev._loop_strategy(lib, comm, True, kw.get("plane_flux", ()))
            assert strategy == ("slab" if loop == "slab" and not f["faces"] else "all-reduce"), (row, loop, strategy)
            got = ev.evolve3D_MPI(c["dt"], c["dr"], c["flux"], c["pos"], True, 1000, N, 1e-2, pd.MPI, comm, rank, world, c["temp"],
                                  c["ndens"], c["xh"], c["thin"], c["thick"], cases.MINLOGTAU, c["dlogtau"], c["R"], c["conv"],
                                  cases.SIG, *SR.CHEM, logfile=None, quiet=True, **kw)
            assert len(got) == (3 if f["thermal"] else 2)
            assert bool(lib.last_raytrace_variant()["open"]) == f["open"], (row, loop)
            # every rank's library is back to its defaults
            assert lib.get_option(_capi.OPT_OPEN_BOUNDARIES) == 0 and lib.get_lls_opacity() == (0.0, 0.0) and lib.get_plane_flux() == []
            tag = f"{row}_{loop}"
            results.update({f"{tag}_xh": np.array(got[0]), f"{tag}_phi": np.array(got[1]), f"{tag}_niter": ev._evolve.last_niter})
            if f["thermal"]:
                results.update({f"{tag}_T": np.array(got[2]), f"{tag}_heat": lib.grid_to_host(_capi.GRID_PHI_HEAT, np.empty((N, N, N)))})
            if f["budget"]:
                results.update({f"{tag}_sums": kw["budget"].sums.copy(), f"{tag}_emitted": kw["budget"].emitted})
    np.savez(out, **results)
    p.device_close()
    pd.TorchComm().Barrier()
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
