"""CPU: the host side of the topology: the C-ABI symbol, Topology's arithmetic, the argument checks of
topology (before the library is touched), the YAML keys and attributes of the class, and which form of the call the class takes
(on a stand-in for the library)."""
import importlib
import os

import numpy as np
import pytest

import lls_standin_backend as SB
import topology_standin_backend as TB

HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_test.yml")
TOPOLOGY_PARAMS = os.path.join(HERE, "data", "parameters_topology.yml")


@pytest.fixture(scope="module", autouse=True)
def no_leftover_device():
    """As in tests/test_regions_host.py: the code-2 check below needs a library without a device, so one that an earlier test left
    initialised behind the package's back is closed first; a device the package itself holds is left alone."""
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    lib = _capi.load()
    if lib.asora_device_ptr(_capi.GRID_NDENS) and not p.cuda_is_init():
        assert lib.asora_device_close() == 0
    yield


def _module():
    """pyc2ray_amd.topology the MODULE (the package's attribute of that name is the function)"""
    return importlib.import_module("pyc2ray_amd.topology")


def _install(monkeypatch, backend, ready=True):
    import pyc2ray_amd.c2ray_base as B
    for mod in (_module(), B):
        monkeypatch.setattr(mod, "load_asora", lambda: backend)
        monkeypatch.setattr(mod, "cuda_is_init", lambda: ready)
    return backend


def test_capi_symbol_and_header():
    from pyc2ray_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "asora_hip.h")).read()
    assert ("int asora_topology(int which_grid, double threshold, int phase, int periodic, int connectivity,\n"
            "                   unsigned long long *tallies /* [ASORA_TOPO_TALLIES] */);") in header
    order = ("CELLS", "CLOSED_FACES", "CLOSED_EDGES", "CLOSED_VERTICES", "OPEN_FACES", "OPEN_EDGES", "OPEN_VERTICES", "COMPONENTS",
             "COMPLEMENT_COMPONENTS", "CAVITIES")
    for n, name in enumerate(order):
        assert f"ASORA_TOPO_{name} = {n}," in header and getattr(_capi, f"TOPO_{name}") == n
    assert "ASORA_TOPO_TALLIES = 10" in header and _capi.TOPO_TALLIES == 10
    assert len(_capi.SIGNATURES["asora_topology"][1]) == 6
    lib = _capi.load()                    # (opening the library resolves every declared symbol)
    if not lib.asora_device_ptr(_capi.GRID_NDENS):      # no device initialised in this process: refused as every entry is
        out = np.full(10, 9, dtype=np.uint64)
        rc = lib.asora_topology(_capi.GRID_XH, 0.5, 0, 1, 6, out.ctypes.data_as(_capi._u64p))
        assert rc == 2 and b"topology" in lib.asora_last_error() and b"not initialised" in lib.asora_last_error()
        assert np.all(out == 9)                             # (a refused call writes nothing)


def test_topology_arithmetic():
    Topology = _module().Topology
    # the 5^3 cube with its centre removed, open box of 9: V, E, F, C = 216, 540, 450, 124 closed and 56, 228, 294, 124 open
    t = Topology([124, 450, 540, 216, 294, 228, 56, 1, 2, 1], 9, threshold=0.3, phase="neutral", connectivity=26, periodic=False, dr=2.0)
    assert (t.cells, t.closed_faces, t.closed_edges, t.closed_vertices, t.open_faces, t.open_edges, t.open_vertices) == (124, 450, 540, 216, 294, 228, 56)
    assert (t.components, t.complement_components, t.cavities) == (1, 2, 1)
    assert t.tallies.dtype == np.uint64 and t.tallies.tolist() == [124, 450, 540, 216, 294, 228, 56, 1, 2, 1]
    assert t.euler_26 == 216 - 540 + 450 - 124 == 2 and t.euler_6 == 124 - 294 + 228 - 56 == 2 and t.euler == 2
    assert t.betti == (1, 0, 1) and t.tunnels_minus_cavities == -1 and t.full is False
    # Minkowski functionals of the closed complex: the outer surface 6 * 25 and the cavity's 6
    assert (t.volume, t.surface, t.mean_breadth) == (124, 2 * 450 - 6 * 124, (3 * 124 - 2 * 450 + 540) / 2) == (124, 156, 6.0)
    assert t.minkowski == (124, 156, 6.0, 2)
    assert (t.volume_phys, t.surface_phys, t.mean_breadth_phys) == (8.0 * 124, 4.0 * 156, 12.0)
    line = t.log_line()
    assert line.startswith("Topology (neutral, x < 0.3, 26 neighbours, open): Euler characteristic 2, 1 components, Betti numbers 1, 0, 1; "
                           "volume 124, surface 156, mean breadth 6.0") and "\n" not in line and "in units of dr^3, dr^2, dr" in line
    assert repr(t) == f"<Topology: {line}>"
    # the two Euler characteristics differ where cells touch at a corner only: chi follows the connectivity
    pair = [2, 12, 24, 15, 0, 0, 0]
    six, many = Topology(pair + [2, 1, 0], 9, connectivity=6, periodic=False), Topology(pair + [1, 1, 0], 9, connectivity=26, periodic=False)
    assert (six.euler_6, six.euler_26, six.euler, many.euler) == (2, 1, 2, 1) and six.betti == (2, 0, 0) and many.betti == (1, 0, 0)
    assert six.volume_phys is None and six.surface_phys is None and six.mean_breadth_phys is None and "in units of" not in six.log_line()
    # periodic: no Betti triple; the full box is the 3-torus, b = (1, 3, 3, 1): tunnels - cavities = 0
    full = Topology([125, 375, 375, 125, 375, 375, 125, 1, 0, 0], 5)
    assert full.betti is None and full.euler == full.euler_26 == 0 and full.full and full.tunnels_minus_cavities == 0
    assert "tunnels - cavities 0, 0 components of the complement" in full.log_line() and "periodic" in full.log_line()
    # all but one island (the complement of one cell in a periodic box of 5): b = (1, 3, 3, 0), chi = 1, tunnels - cavities = 0
    island = Topology([124, 375, 375, 125, 369, 363, 117, 1, 1, 0], 5)
    assert island.euler_26 == 1 and island.euler_6 == 124 - 369 + 363 - 117 == 1 and island.tunnels_minus_cavities == 0
    empty = Topology([0] * 10, 5, dr=3.0)
    assert (empty.euler, empty.euler_26, empty.volume, empty.surface, empty.mean_breadth, empty.tunnels_minus_cavities) == (0, 0, 0, 0, 0.0, 0)
    assert empty.betti is None and "\n" not in empty.log_line() and empty.volume_phys == 0.0
    assert Topology([0] * 10, 5, periodic=False).betti == (0, 0, 0)
    with pytest.raises(ValueError, match="10 tallies"):
        Topology([0] * 14, 5)


def test_bad_arguments_are_refused_before_the_library_is_touched(monkeypatch):
    M = _module()
    topology, topology_spec = M.topology, M.topology_spec
    _install(monkeypatch, SB.Untouchable())
    f = np.zeros((8, 8, 8))
    for kw, what in ((dict(threshold=np.nan), "threshold must be a finite number"), (dict(threshold=np.inf), "threshold must be"),
                     (dict(threshold="0.5"), "threshold must be"), (dict(threshold=True), "threshold must be"),
                     (dict(phase="ionized"), "phase must be 'ionised' or 'neutral'"), (dict(phase=0), "phase must be"),
                     (dict(connectivity=18), "connectivity must be 6"), (dict(connectivity=6.0), "connectivity must be"),
                     (dict(connectivity="6"), "connectivity must be"), (dict(connectivity=True), "connectivity must be"),
                     (dict(periodic=1), "periodic must be a bool"), (dict(dr=0.0), "dr must be None or a finite number > 0"),
                     (dict(dr=np.nan), "dr must be"), (dict(grid=4), "grid selects a device grid and goes with field=None")):
        with pytest.raises(ValueError, match=f"topology: .*{what}"):
            topology(f, **kw)
        if "grid" not in kw:
            with pytest.raises(ValueError, match=f"topology: .*{what}"):
                topology(None, **kw)
    for bad in (np.zeros((8, 8)), np.zeros((8, 8, 4)), np.zeros((4, 4, 4), dtype=complex), [["a"]]):
        with pytest.raises(ValueError, match="field must be a real"):
            topology(bad)
    for bad in (-1, 9, 1.0, "xh", True):
        with pytest.raises(ValueError, match="grid must be one of"):
            topology(None, grid=bad)
    with pytest.raises(ValueError, match="1 ... 645 cells a side"):
        topology_spec("x", 646)
    with pytest.raises(ValueError, match="1 ... 645 cells a side"):
        topology_spec("x", 0)
    assert topology_spec("x", None) is None
    assert topology_spec("x", 645, dr=2) == dict(N=645, threshold=0.5, phase="ionised", connectivity=6, periodic=True, dr=2.0)
    _install(monkeypatch, SB.Untouchable(), ready=False)
    with pytest.raises(RuntimeError, match="GPU not initialized"):
        topology(f)


def test_the_two_forms_of_the_module_entry(monkeypatch):
    from pyc2ray_amd import _capi
    topology = _module().topology
    lib = _install(monkeypatch, TB.Counting(9))
    f = np.random.default_rng(0).random((9, 9, 9))
    t = topology(f, threshold=0.25, phase="neutral", connectivity=26, periodic=False, dr=3.0)
    assert lib.names() == ["grid_to_device", "topology"]
    up, call = lib.calls
    assert up[1][0] == _capi.GRID_XH and np.array_equal(up[1][1], f)
    assert call[1] == (_capi.GRID_XH, 0.25, 1, False, 26) and call[2] == {}
    assert t.tallies.tolist() == TB.TALLIES.tolist() and (t.N, t.dr, t.phase, t.threshold, t.connectivity, t.periodic) == (9, 3.0, "neutral", 0.25, 26, False)
    assert t.betti == (1, 0, 1)
    lib.calls.clear()
    t = topology(None, grid=_capi.GRID_XH_AV)                       # the device grid where it lies
    assert lib.names() == ["topology"] and lib.calls[0][1] == (_capi.GRID_XH_AV, 0.5, 0, True, 6) and t.N == 9 and t.betti is None
    lib.calls.clear()
    assert topology(None).dr is None and lib.calls[0][1][0] == _capi.GRID_XH


def test_yaml_keys_the_attribute_and_the_forms_the_class_takes(tmp_path, monkeypatch):
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.c2ray_base as B
    from pyc2ray_amd import _capi
    M = _module()
    assert pc2r.topology is M.topology and pc2r.Topology is M.Topology
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 8
        plain = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        assert plain.topology_stats is False and plain.last_topology is None
        with pytest.raises(ValueError, match="C2Ray.topology_stats: topology_stats needs use_gpu=True"):
            plain.topology_stats = True
        plain.topology_stats = False
        for bad in (1, 0, None, "on", 1.0):
            with pytest.raises(ValueError, match="topology_stats must be a bool"):
                plain.topology_stats = bad
        body = open(PLAIN_PARAMS).read()
        key = lambda text: body.replace("  logfile: pyC2Ray.log\n", f"  logfile: pyC2Ray.log\n{text}")
        assert key("x") != body
        for text, what in (("  topology: 2\n", "Output: topology must be 0 or 1"), ("  topology: 'yes'\n", "must be 0 or 1"),
                           ("  topology: 1.0\n", "must be 0 or 1"),
                           ("  topology: 1\n", "Output: topology: 1: topology_stats needs use_gpu=True"),
                           ("  topology_threshold: .nan\n", "threshold must be a finite number"), ("  topology_threshold: half\n", "threshold must be"),
                           ("  topology_connectivity: 18\n", "connectivity must be 6"), ("  topology_connectivity: 6.0\n", "connectivity must be")):
            with open("p.yml", "w") as f:
                f.write(key(text))
            with pytest.raises(ValueError, match=what):
                pc2r.C2Ray_Test("p.yml", N, False)
        with open("p.yml", "w") as f:
            f.write(key("  topology: 0\n  topology_connectivity: 26\n"))
        assert pc2r.C2Ray_Test("p.yml", N, False).topology_stats is False
        # the committed parameter file is refused without use_gpu, as the key says
        with pytest.raises(ValueError, match="Output: topology: 1: topology_stats needs use_gpu=True"):
            pc2r.C2Ray_Test(TOPOLOGY_PARAMS, N, False)
        # an object with use_gpu (as one constructed with use_gpu=True has it) reading its keys
        sim = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        sim.gpu = True
        sim._read_paramfile(TOPOLOGY_PARAMS)
        sim._statistic_init("topology_stats")
        assert sim.topology_stats is True and sim.last_topology is None
        lib = _install(monkeypatch, TB.Counting(N))
        steps = []
        monkeypatch.setattr(B, "evolve3D", lambda *a, **kw: steps.append("evolve3D") or (np.full((N, N, N), 0.75), np.zeros((N, N, N))))
        monkeypatch.setattr(B, "evolve3D_resident", lambda *a, **kw: steps.append("evolve3D_resident"))
        flux, pos = np.ones(1), np.ones((3, 1), dtype=int)
        # the resident path: the device grid where it lies -- no upload, no download, the bookkeeping untouched
        sim.device_resident = True
        sim.evolve3D(2.0, flux, pos)
        assert steps == ["evolve3D_resident"] and lib.names() == ["topology"]
        assert lib.calls[0][1] == (_capi.GRID_XH, 0.4, 0, True, 26) and lib.calls[0][2] == {}
        first = sim.last_topology
        assert (first.components, first.dr, first.periodic, first.connectivity, first.threshold, first.N) == (1, sim.dr, True, 26, 0.4, N)
        assert sim._device_newer >= {"xh", "phi_ion"} and "xh" not in sim._host_newer
        lib.calls.clear()
        t = sim.topology(connectivity=6, phase="neutral", dr=None, periodic=False)       # keywords override keys and defaults
        assert lib.names() == ["topology"] and lib.calls[0][1] == (_capi.GRID_XH, 0.4, 1, False, 6)
        assert t.dr is None and t.periodic is False and t is not sim.last_topology and sim.last_topology is first
        assert sim._device_newer >= {"xh", "phi_ion"} and "xh" not in sim._host_newer
        # periodic and dr are the object's
        lib.calls.clear()
        sim.periodic = False
        t = sim.topology()
        assert lib.calls[0][1] == (_capi.GRID_XH, 0.4, 0, False, 26) and t.periodic is False and t.dr == sim.dr and t.betti == (1, 0, 1)
        sim.periodic = True
        for name in ("field", "grid"):
            with pytest.raises(ValueError, match=f"C2Ray.topology: {name} is not for the class"):
                sim.topology(**{name: None})
        with pytest.raises(ValueError, match="C2Ray.topology: connectivity must be"):
            sim.topology(connectivity=8)
        # otherwise: the host array goes up first
        lib.calls.clear()
        sim._device_newer.clear()
        sim.device_resident = False
        sim.evolve3D(3.0, flux, pos)
        assert steps[-1] == "evolve3D" and lib.names() == ["grid_to_device", "topology"]
        assert lib.calls[0][1][0] == _capi.GRID_XH and np.all(lib.calls[0][1][1] == 0.75) and lib.calls[1][1][4] == 26
        assert sim.last_topology is not first
        assert open(sim.logfile).read().count("Topology (ionised, x >= 0.4, 26 neighbours, periodic): Euler characteristic 2, 1 components") == 2
        # off: a step makes no library call of the feature's, and leaves the last result alone
        kept = sim.last_topology
        sim.topology_stats = False
        for resident in (True, False):
            lib.calls.clear()
            sim._device_newer.clear()
            sim.device_resident = resident
            sim.evolve3D(1.0, flux, pos)
            assert lib.calls == [] and sim.last_topology is kept
        assert open(sim.logfile).read().count("Topology (") == 2
    finally:
        os.chdir(cwd)
        if "sim" in locals():      # (nothing of this object lives on a device: a later step elsewhere must not ask it to fetch)
            sim._device_newer.clear()
            sim.device_resident = False


def test_feature_off_adds_no_library_call_to_a_step(monkeypatch, tmp_path):
    """evolve3D of the module on a recording stand-in: the sequence of library calls of a step holds nothing of the feature."""
    import budget_standin_backend as BS
    import pyc2ray_amd as pc2r
    lib = SB.install(monkeypatch, BS.Converging())
    g = np.ones((4, 4, 4))
    pc2r.evolve3D(1.0, 1.0, np.ones(1), np.ones((3, 1)), True, 10, 4, 0.01, g, g, g, np.ones(5), np.ones(5), -20.0, 0.1, 4.0, 1e-4, 1e-18,
                  1.0, 1.0, 1.0, 1.0, 1.0, quiet=True, logfile=str(tmp_path / "log"))
    assert lib.names() and not [n for n in lib.names() if "topology" in n]
