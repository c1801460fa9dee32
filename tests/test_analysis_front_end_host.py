"""CPU: what the analyses of a thresholded field share, stated once (pyc2ray_amd/_fieldspec.py): the
refusals of the common arguments -- one message each, the entry's own name in front --, the order of the front end, the two forms
of the call on the stand-ins for the library; and the one mechanism behind the statistics of a time step (C2Ray._statistic_init,
C2Ray._close_step): seven switches, seven lines in one order, and nothing at all when they are off."""
import importlib
import os

import numpy as np
import pytest

import bubble_standin_backend as BB
import budget_standin_backend as BS
import granulometry_standin_backend as GB
import lls_standin_backend as SB
import powerspec_standin_backend as PB
import regions_standin_backend as RB
import smoothing_standin_backend as MB
import topology_standin_backend as TB

HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_test.yml")

#: the public function (its module and name; the name is the `who` of its messages), its stand-in, the library entry it calls
ANALYSES = [pytest.param("pyc2ray_amd.bubbles", "mfp_distribution", BB.Bubbling, "bubble_mfp", id="mfp_distribution"),
            pytest.param("pyc2ray_amd.regions", "region_sizes", RB.Labelling, "region_sizes", id="region_sizes"),
            pytest.param("pyc2ray_amd.topology", "topology", TB.Counting, "topology", id="topology"),
            pytest.param("pyc2ray_amd.granulometry", "granulometry", GB.Counting, "granulometry", id="granulometry")]
analyses = pytest.mark.parametrize("module, who, backend, entry", ANALYSES)


MODULES = ("pyc2ray_amd.bubbles", "pyc2ray_amd.regions", "pyc2ray_amd.topology", "pyc2ray_amd.granulometry", "pyc2ray_amd.powerspec",
           "pyc2ray_amd.smoothing", "pyc2ray_amd.c2ray_base")


def _install(monkeypatch, backend, ready=True):
    """The stand-in where the entries look the library up: each module's own ``load_asora`` and ``cuda_is_init``, which the four
    thresholded analyses hand to the shared front end."""
    for mod in map(importlib.import_module, MODULES):
        monkeypatch.setattr(mod, "load_asora", lambda: backend)
        monkeypatch.setattr(mod, "cuda_is_init", lambda: ready)
    return backend


class _Resident:
    """What pyc2ray_amd._residency asks to take its data home: it writes the request among the calls of the library."""

    def __init__(self, lib):
        self.lib = lib

    def _leave_device(self):
        self.lib.calls.append(("reclaim", (), {}))


@pytest.fixture
def resident():
    from pyc2ray_amd import _residency
    held = []

    def make(lib):
        held.append(_Resident(lib))
        _residency.register(held[-1])
        return held[-1]
    yield make
    for r in held:
        _residency._resident.discard(r)


@analyses
def test_common_arguments_are_refused_with_one_message(monkeypatch, module, who, backend, entry):
    fn = getattr(importlib.import_module(module), who)
    _install(monkeypatch, SB.Untouchable())
    f = np.zeros((8, 8, 8))
    cases = [(dict(threshold=v), f"threshold must be a finite number, not {v!r}") for v in (np.nan, np.inf, "0.5", True, None)]
    cases += [(dict(phase=v), f"phase must be 'ionised' or 'neutral', not {v!r}") for v in ("ionized", 0, None)]
    cases += [(dict(periodic=v), f"periodic must be a bool, not {type(v).__name__}") for v in (1, 0, None, "yes")]
    cases += [(dict(dr=v), f"dr must be None or a finite number > 0, not {v!r}") for v in (0.0, -1.0, np.nan, np.inf, "1", True)]
    # of two bad arguments the one checked first is the one named: threshold, phase, periodic, dr
    cases += [(dict(threshold="x", phase="x"), "threshold must be a finite number, not 'x'"),
              (dict(phase="x", periodic=1), "phase must be 'ionised' or 'neutral', not 'x'"),
              (dict(periodic=1, dr=0), "periodic must be a bool, not int")]
    for kw, what in cases:
        for field in (f, None):
            with pytest.raises(ValueError) as e:
                fn(field, **kw)
            assert str(e.value) == f"{who}: {what}"
    with pytest.raises(ValueError) as e:
        fn(f, grid=4)
    assert str(e.value) == f"{who}: grid selects a device grid and goes with field=None"
    with pytest.raises(ValueError) as e:            # (before the field itself is looked at)
        fn(np.zeros((8, 8)), grid=4)
    assert str(e.value) == f"{who}: grid selects a device grid and goes with field=None"
    for bad in (np.zeros((8, 8)), np.zeros((8, 8, 4)), np.zeros((4, 4, 4), dtype=complex), [["a"]]):
        with pytest.raises(ValueError) as e:
            fn(bad)
        assert str(e.value) == f"{who}: field must be a real (N, N, N) array"
    for bad in (-1, 9, 1.0, "xh", True):
        with pytest.raises(ValueError) as e:
            fn(None, grid=bad)
        assert str(e.value) == f"{who}: grid must be one of the _capi.GRID_* selectors, not {bad!r}"


@analyses
def test_the_device_is_asked_for_after_the_arguments(monkeypatch, module, who, backend, entry):
    fn = getattr(importlib.import_module(module), who)
    f = np.zeros((8, 8, 8))
    _install(monkeypatch, SB.Untouchable(), ready=False)
    for field in (f, None):
        with pytest.raises(RuntimeError, match="^GPU not initialized. Please initialize it by calling device_init"):
            fn(field)
        with pytest.raises(ValueError, match=f"^{who}: threshold must be"):        # (the arguments come first)
            fn(field, threshold="x")
    lib = _install(monkeypatch, backend(None))       # a library that no device_init of the package has told its mesh
    with pytest.raises(RuntimeError) as e:
        fn(None)
    assert str(e.value) == f"{who}: field=None needs a device initialised through device_init (the mesh size)" and lib.calls == []


@analyses
def test_the_two_forms_of_a_call(monkeypatch, resident, module, who, backend, entry):
    from pyc2ray_amd import _capi
    fn = getattr(importlib.import_module(module), who)
    N = 9
    lib = _install(monkeypatch, backend(N))
    resident(lib)
    f = np.random.default_rng(1).random((N, N, N)).astype(np.float32)
    # a host field: whoever keeps grids on the device is told, the field goes up to the ionised fraction's grid, then the entry
    fn(f, threshold=0.25, phase="neutral", periodic=False)
    assert lib.names() == ["reclaim", "grid_to_device", entry]
    up, call = lib.calls[1:]
    assert up[1][0] == _capi.GRID_XH and up[1][1].dtype == np.float64 and np.array_equal(up[1][1], f)
    assert call[1][:4] == (_capi.GRID_XH, 0.25, 1, False)
    # no field: the device grid where it lies, nobody is disturbed, and the mesh is the library's
    lib.calls.clear()
    got = fn(None, grid=_capi.GRID_XH_AV)
    assert lib.names() == [entry] and lib.calls[0][1][:4] == (_capi.GRID_XH_AV, 0.5, 0, True)
    assert getattr(got, "N", N) == N
    lib.calls.clear()
    fn(None)
    assert lib.names() == [entry] and lib.calls[0][1][0] == _capi.GRID_XH


class _Everything(BB.Bubbling, RB.Labelling, TB.Counting, GB.Counting, PB.Counting, MB.Counting):
    """The stand-ins of the six analyses in one: each answers its own entry and hands every other name on to the next."""

    def __init__(self, N):
        BS.Converging.__init__(self)
        self._N = N


SWITCHES = ("photon_budget", "bubble_stats", "region_stats", "topology_stats", "granulometry_stats", "power_spectrum_stats",
            "observed_stats")
LAST = ("last_budget", "last_bubble_sizes", "last_regions", "last_topology", "last_granulometry", "last_power_spectrum", "last_observed")
LINES = ("Photon budget: ", "Bubble sizes (", "Regions (", "Topology (", "Granulometry (", "Power spectrum (", "Smoothed field (")
ENTRIES = ["bubble_mfp", "region_sizes", "topology", "granulometry", "power_spectrum", "smooth_field"]
KEYS = "".join(f"  {key}: 1\n" for key in ("photon_budget", "bubble_sizes", "region_sizes", "topology", "granulometry", "power_spectrum",
                                            "observed_map"))


def test_seven_switches_one_step_seven_lines(tmp_path, monkeypatch):
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.c2ray_base as B
    assert B.C2Ray._STEP_STATISTICS == SWITCHES
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 8
        body = open(PLAIN_PARAMS).read()
        with open("p.yml", "w") as f:
            f.write(body.replace("  logfile: pyC2Ray.log\n", f"  logfile: pyC2Ray.log\n{KEYS}"))
        assert KEYS in open("p.yml").read()
        # the keys are refused without use_gpu, and the first statistic of the order is the one that says so
        with pytest.raises(ValueError, match="^Output: photon_budget: 1: photon_budget needs use_gpu=True"):
            pc2r.C2Ray_Test("p.yml", N, False)
        # an object with use_gpu (as one constructed with use_gpu=True has it) reading its keys
        sim = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        assert not any(getattr(sim, s) for s in SWITCHES)
        sim.gpu = True
        sim._read_paramfile("p.yml")
        for name in SWITCHES:
            sim._statistic_init(name)
        assert all(getattr(sim, s) is True for s in SWITCHES) and all(getattr(sim, a) is None for a in LAST)
        lib = _install(monkeypatch, _Everything(N))

        def step(*args, **kw):
            if "budget" in kw:
                kw["budget"].fill(BS.SUMS.copy(), args[0], args[1], N, args[2])
        monkeypatch.setattr(B, "evolve3D_resident", step)
        flux, pos = np.ones(1), np.ones((3, 1), dtype=int)
        sim.device_resident = True
        before = open(sim.logfile).read()
        sim.evolve3D(2.0, flux, pos)
        lines = open(sim.logfile).read()[len(before):].splitlines()
        assert len(lines) == 7 and all(line.startswith(head) for line, head in zip(lines, LINES))
        assert all(getattr(sim, a) is not None for a in LAST) and sim.total_budget.steps == 1
        assert lines == [getattr(sim, a).log_line() for a in LAST]
        # (the resident path: every analysis on the device grids where they lie, one library call each, nothing uploaded)
        assert lib.names() == ENTRIES
        # all off: the library sees no call, the log gets no line, and the last results are left alone
        kept = [getattr(sim, a) for a in LAST]
        for s in SWITCHES:
            setattr(sim, s, False)
        lib.calls.clear()
        before = open(sim.logfile).read()
        sim.evolve3D(1.0, flux, pos)
        assert lib.calls == [] and open(sim.logfile).read() == before
        assert all(getattr(sim, a) is k for a, k in zip(LAST, kept)) and sim.total_budget.steps == 1
    finally:
        os.chdir(cwd)
        if "sim" in locals():      # (nothing of this object lives on a device: a later step elsewhere must not ask it to fetch)
            sim._device_newer.clear()
            sim.device_resident = False
