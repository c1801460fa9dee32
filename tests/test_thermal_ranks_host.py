"""CPU: what the thermal mode across ranks decides on the host -- which communicators evolve3D_MPI(thermal=...) accepts, the
bytes a thermal step's exchanges move, and the binding of the new exports."""
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


class _Mpi4pyShaped:
    """What a real mpi4py run hands to evolve3D_MPI: Reduce / Bcast on numpy buffers, nothing else."""
    def Get_rank(self): return 0
    def Get_size(self): return 2
    def Reduce(self, *a, **k): raise AssertionError("no exchange may start")
    def Bcast(self, *a, **k): raise AssertionError("no exchange may start")


class _TorchCommLike:
    """The attributes evolve.py reads from a pyc2ray_amd.dist.TorchComm; every method fails the test when it is reached."""
    exchange, device_loop, backend = "slab", True, "gloo"

    def __init__(self, overlap):
        self.overlap = overlap

    def _never(self, *a, **k):
        raise AssertionError("no GPU work and no exchange may start")
    slab_enqueue = slab_begin = reduce_begin = slab_poll = thermal_stats = raytrace_and_allreduce = shard_sources_by_slab = _never


def test_thermal_step_refuses_other_communicators_before_any_gpu_work(monkeypatch):
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.evolve as ev
    from pyc2ray_amd.thermal import ThermalParams

    def no_gpu(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ev, "load_asora", no_gpu)
    monkeypatch.setattr(ev, "cuda_is_init", no_gpu)
    th = ThermalParams(np.zeros(5), np.zeros(5))
    g = np.ones((4, 4, 4))

    def step(comm, use_mpi=object(), use_gpu=True):
        return pc2r.evolve3D_MPI(1.0, 1.0, np.ones(2), np.ones((3, 2)), use_gpu, 10, 4, 0.01, use_mpi, comm, 0, 2, g, g, g, np.ones(5),
                                 np.ones(5), -20.0, 0.1, 4.0, 1e-4, 1e-18, 1.0, 1.0, 1.0, 1.0, 1.0, quiet=True, logfile=None, thermal=th)
    for comm in (None, _Mpi4pyShaped(), _TorchCommLike(overlap=True)):
        with pytest.raises(ValueError, match="single-GPU"):
            step(comm)
    legacy = _TorchCommLike(overlap=False)
    legacy.exchange, legacy.device_loop = "allreduce", False           # the three-call loop
    with pytest.raises(ValueError, match="single-GPU"):
        step(legacy)
    with pytest.raises(ValueError, match="use_gpu=True"):
        step(_TorchCommLike(overlap=False), use_gpu=False)
    # a TorchComm on a device loop passes the check: the next thing the step does is ask for the GPU
    with pytest.raises(AssertionError, match="the library was reached"):
        step(_TorchCommLike(overlap=False))


def test_slab_plan_bytes_of_a_thermal_step():
    from pyc2ray_amd.dist import SlabPlan, TorchComm
    rng = np.random.default_rng(3)
    for N, P, R in ((24, 2, 4.0), (33, 3, 2.5), (64, 8, 6.0), (16, 4, 1000.0)):
        pos = 1 + rng.integers(0, N, size=(3, 5 * P))
        spos, _, b = TorchComm.shard_sources_by_slab(pos, np.ones(5 * P), P)
        plan = SlabPlan(N, P, R, [spos[0, b[r]:b[r + 1]] - 1 for r in range(P)])
        assert plan.largest_transfer() > 0
        for r in range(P):
            sent, recv = plan.bytes_per_rank(r)
            assert plan.bytes_per_rank(r, thermal=False, exchange="xh_av") == (sent, recv)
            assert plan.bytes_per_rank(r, thermal=True) == plan.bytes_per_rank(r, thermal=True, exchange="rates") == (2 * sent, 2 * recv)
            assert plan.bytes_per_rank(r, thermal=True, exchange="xh_av") == (sent, recv)
        assert plan.largest_transfer(thermal=True) == 2 * plan.largest_transfer()
        assert plan.largest_transfer(thermal=True, exchange="xh_av") == plan.largest_transfer()
        with pytest.raises(ValueError):
            plan.bytes_per_rank(0, thermal=True, exchange="heat")


NEW_EXPORTS = ("asora_evolve_begin_slab_thermal", "asora_evolve_slab_heat_outbox", "asora_evolve_slab_heat_outbox_to_host",
               "asora_evolve_slab_heat_outbox_from_host", "asora_evolve_slab_add_heat", "asora_evolve_slab_add_heat_host")


def test_new_exports_are_declared_bound_and_exported():
    import ctypes
    import __graft_entry__ as g
    g.build()
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import _LibAsora
    header = open(os.path.join(os.path.dirname(HERE), "include", "asora_hip.h")).read()
    declared = set(re.findall(r"\b((?:asora|c2ray)_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_capi.SIGNATURES), declared ^ set(_capi.SIGNATURES)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW_EXPORTS:
        assert name in declared and name in _capi.SIGNATURES and hasattr(lib, name), name
    # the thermal begin takes what the isothermal one takes
    assert _capi.SIGNATURES["asora_evolve_begin_slab_thermal"] == _capi.SIGNATURES["asora_evolve_begin_slab"]
    for method in ("evolve_begin_slab_thermal", "evolve_slab_heat_outbox_ptr", "evolve_slab_heat_outbox_to_host",
                   "evolve_slab_heat_outbox_from_host", "evolve_slab_add_heat", "evolve_slab_add_heat_host"):
        assert callable(getattr(_LibAsora, method)), method


def test_yaml_non_isothermal_accepts_the_torch_communicator_module(tmp_path, monkeypatch):
    """`isothermal: false` with use_mpi: accepted for pyc2ray_amd.dist.MPI, refused ("single-GPU") for any other module."""
    import pyc2ray_amd as pc2r
    from pyc2ray_amd import dist
    from pyc2ray_amd.c2ray_base import C2Ray

    class Sim:
        _ld = {"Material": {"isothermal": False}, "Photo": {"compute_heating_rates": 1}}
    sim = Sim()
    C2Ray._thermal_mode_init(sim, True, dist.MPI)
    assert sim.isothermal is False
    with pytest.raises(ValueError, match="single-GPU"):
        C2Ray._thermal_mode_init(Sim(), True, object())
    C2Ray._thermal_mode_init(sim, True, None)
