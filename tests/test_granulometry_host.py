"""CPU: the host side of the granulometry: the C-ABI symbol, Granulometry's arithmetic, the argument checks
of granulometry (before the library is touched), the YAML keys and attributes of the class, and which form of the call the class
takes (on a stand-in for the library)."""
import importlib
import os

import numpy as np
import pytest

import granulometry_standin_backend as GB
import lls_standin_backend as SB

HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_test.yml")
GRANULOMETRY_PARAMS = os.path.join(HERE, "data", "parameters_granulometry.yml")


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
    """pyc2ray_amd.granulometry the MODULE (the package's attribute of that name is the function)"""
    return importlib.import_module("pyc2ray_amd.granulometry")


def _install(monkeypatch, backend, ready=True):
    import pyc2ray_amd.c2ray_base as B
    for mod in (_module(), B):
        monkeypatch.setattr(mod, "load_asora", lambda: backend)
        monkeypatch.setattr(mod, "cuda_is_init", lambda: ready)
    return backend


def test_capi_symbol_and_header():
    from pyc2ray_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "asora_hip.h")).read()
    assert ("int asora_granulometry(int which_grid, double threshold, int phase, int periodic, int n_radii, const double *radii,\n"
            "                       unsigned long long *eroded, unsigned long long *opened, unsigned long long *tallies,\n"
            "                       unsigned *dist2 /* NULL, or host [N^3] */);") in header
    for n, name in enumerate(("N_PHASE", "D2_MAX", "N_UNBOUNDED", "SUM_D2")):
        assert f"ASORA_GRAN_{name} = {n}," in header and getattr(_capi, f"GRAN_{name}") == n
    assert "ASORA_GRAN_TALLIES = 4" in header and _capi.GRAN_TALLIES == 4
    assert "#define ASORA_GRAN_UNBOUNDED 0xFFFFFFFFu" in header and _capi.GRAN_UNBOUNDED == 0xFFFFFFFF
    assert "ASORA_KERNEL_SLOTS = 7" in header and "ASORA_OPT_COUNT = 19" in header           # (no timing slot, no option)
    assert len(_capi.SIGNATURES["asora_granulometry"][1]) == 10
    lib = _capi.load()                    # (opening the library resolves every declared symbol)
    if not lib.asora_device_ptr(_capi.GRID_NDENS):      # no device initialised in this process: refused as every entry is
        radii = np.array([1.0, 2.0])
        e, o, t = np.full(2, 9, dtype=np.uint64), np.full(2, 9, dtype=np.uint64), np.full(4, 9, dtype=np.uint64)
        rc = lib.asora_granulometry(_capi.GRID_XH, 0.5, 0, 1, 2, _capi.dptr(radii), e.ctypes.data_as(_capi._u64p),
                                    o.ctypes.data_as(_capi._u64p), t.ctypes.data_as(_capi._u64p), None)
        assert rc == 2 and b"granulometry" in lib.asora_last_error() and b"not initialised" in lib.asora_last_error()
        assert np.all(e == 9) and np.all(o == 9) and np.all(t == 9)      # (a refused call writes nothing)


def test_granulometry_arithmetic():
    Granulometry = _module().Granulometry
    # 400 cells in phase; openings of radius 1, 2, 4 keep 360, 300, 100 of them
    g = Granulometry([1, 2, 4], [200, 90, 10], [360, 300, 100], [400, 26, 0, 3000], 20, threshold=0.3, phase="neutral", periodic=False, dr=2.0)
    assert g.radii.tolist() == [1.0, 2.0, 4.0] and g.r2.tolist() == [1, 4, 16]
    assert g.eroded.dtype == g.opened.dtype == np.uint64 and g.eroded.tolist() == [200, 90, 10] and g.opened.tolist() == [360, 300, 100]
    assert (g.n_phase, g.d2_max, g.n_unbounded, g.sum_d2) == (400, 26, 0, 3000) and g.tallies.tolist() == [400, 26, 0, 3000]
    assert g.tallies.dtype == np.uint64 and g.unbounded is False and g.dist2 is None
    assert np.allclose(g.opened_fraction, [0.9, 0.75, 0.25]) and np.allclose(g.cumulative, [0.1, 0.25, 0.75])
    assert np.allclose(g.dF, [0.1, 0.15, 0.5]) and g.mid_radii.tolist() == [0.5, 1.5, 3.0]
    assert np.allclose(g.dFdR, [0.1, 0.15, 0.25]) and np.allclose(g.RdFdR, [0.05, 0.225, 0.75])
    assert g.unresolved == 0.25 and abs(g.dF.sum() + g.unresolved - 1.0) < 1e-12
    assert abs(g.mean_radius - (0.5 * 0.1 + 1.5 * 0.15 + 3.0 * 0.5) / 0.75) < 1e-12 and g.peak_radius == 3.0
    assert g.max_inscribed_r2 == 25 and g.max_inscribed_radius == 5.0 and g.max_inscribed_radius_phys == 10.0
    assert g.radii_phys.tolist() == [2.0, 4.0, 8.0] and g.mid_radii_phys.tolist() == [1.0, 3.0, 6.0]
    assert np.allclose(g.dFdR_phys, [0.05, 0.075, 0.125]) and g.mean_radius_phys == 2.0 * g.mean_radius and g.peak_radius_phys == 6.0
    line = g.log_line()
    assert line.startswith("Granulometry (neutral, x < 0.3, open, 3 radii to 4): 400 cells, largest inscribed ball r2 25; "
                           "mean radius 2.367, peak 3.000") and "\n" not in line and "in units of dr" in line
    assert line.endswith("25.00 % above the last radius") and repr(g) == f"<Granulometry: {line}>"
    # floor(R^2) in double, and a first radius of 0 (an interval of no width: nothing lies in it)
    z = Granulometry([0, 1.5, 2.9], [400, 100, 0], [400, 320, 0], [400, 8, 0, 900], 20)
    assert z.r2.tolist() == [0, 2, 8] and z.dF.tolist()[0] == 0.0 and z.dFdR[0] == 0.0 and np.isfinite(z.dFdR).all()
    assert z.unresolved == 0.0 and abs(z.dF.sum() - 1.0) < 1e-12 and abs(z.peak_radius - 2.2) < 1e-12
    assert z.radii_phys is None and z.mean_radius_phys is None and z.max_inscribed_radius_phys is None and "in units of" not in z.log_line()
    # digital balls are no granulometry in the strict sense: a later opening may hold more cells, and dF says so
    odd = Granulometry(np.sqrt([8.5, 9.5]), [40, 30], [479, 482], [2716, 20, 0, 4158], 17, periodic=False)
    assert odd.r2.tolist() == [8, 9] and odd.opened.tolist() == [479, 482] and abs(odd.dF[1] - (479 - 482) / 2716) < 1e-12 and odd.dF[1] < 0
    assert odd.cumulative[1] < odd.cumulative[0] and abs(odd.dF.sum() + odd.unresolved - 1.0) < 1e-12
    # unbounded: a periodic box entirely in phase
    full = Granulometry([1, 2], [125, 125], [125, 125], [125, 0, 125, 0], 5)
    assert full.unbounded and full.max_inscribed_r2 is None and full.max_inscribed_radius is None and full.unresolved == 1.0
    assert full.dF.tolist() == [0.0, 0.0] and full.mean_radius == 0.0 and "the whole periodic box in phase" in full.log_line()
    # the empty phase: zeros, no NaN
    empty = Granulometry([1, 2], [0, 0], [0, 0], [0, 0, 0, 0], 5, dr=3.0)
    for v in (empty.opened_fraction, empty.cumulative, empty.dF, empty.dFdR, empty.RdFdR):
        assert v.tolist() == [0.0, 0.0]
    assert (empty.unresolved, empty.mean_radius, empty.peak_radius, empty.max_inscribed_r2) == (0.0, 0.0, 0.0, None)
    assert "no cell in phase" in empty.log_line() and "\n" not in empty.log_line() and empty.mean_radius_phys == 0.0
    with pytest.raises(ValueError, match="4 tallies"):
        Granulometry([1], [0], [0], [0] * 10, 5)
    with pytest.raises(ValueError, match="one common length"):
        Granulometry([1, 2], [0], [0, 0], [0] * 4, 5)


def test_bad_arguments_are_refused_before_the_library_is_touched(monkeypatch):
    M = _module()
    granulometry, granulometry_spec = M.granulometry, M.granulometry_spec
    _install(monkeypatch, SB.Untouchable())
    f = np.zeros((8, 8, 8))
    for kw, what in ((dict(threshold=np.nan), "threshold must be a finite number"), (dict(threshold=np.inf), "threshold must be"),
                     (dict(threshold="0.5"), "threshold must be"), (dict(threshold=True), "threshold must be"),
                     (dict(phase="ionized"), "phase must be 'ionised' or 'neutral'"), (dict(phase=0), "phase must be"),
                     (dict(periodic=1), "periodic must be a bool"), (dict(dr=0.0), "dr must be None or a finite number > 0"),
                     (dict(dr=np.nan), "dr must be"), (dict(distances=1), "distances must be a bool"),
                     (dict(radii=0), "radii as an int must be in \\[1, 256\\]"), (dict(radii=257), "radii as an int must be in"),
                     (dict(radii=True), "not a bool"), (dict(radii=[]), "one-dimensional array of 1 ... 256 radii"),
                     (dict(radii=np.arange(257.0)), "1 ... 256 radii"), (dict(radii=[[1.0, 2.0]]), "one-dimensional"),
                     (dict(radii=2.5), "one-dimensional"), (dict(radii="three"), "radii must be None, an int or an array"),
                     (dict(radii=[1.0, np.nan]), "radii must be finite"), (dict(radii=[1.0, np.inf]), "radii must be finite"),
                     (dict(radii=[-1.0, 2.0]), "radii must be >= 0"), (dict(radii=[1.0, 1.0]), "strictly ascending"),
                     (dict(radii=[3.0, 2.0]), "strictly ascending"), (dict(radii=[1.0, 46341.0]), "R\\^2 < 2\\^31"),
                     (dict(grid=4), "grid selects a device grid and goes with field=None")):
        with pytest.raises(ValueError, match=f"granulometry: .*{what}"):
            granulometry(f, **kw)
        if "grid" not in kw:
            with pytest.raises(ValueError, match=f"granulometry: .*{what}"):
                granulometry(None, **kw)
    for bad in (np.zeros((8, 8)), np.zeros((8, 8, 4)), np.zeros((4, 4, 4), dtype=complex), [["a"]]):
        with pytest.raises(ValueError, match="field must be a real"):
            granulometry(bad)
    for bad in (-1, 9, 1.0, "xh", True):
        with pytest.raises(ValueError, match="grid must be one of"):
            granulometry(None, grid=bad)
    with pytest.raises(ValueError, match="1 ... 645 cells a side"):
        granulometry_spec("x", 646)
    with pytest.raises(ValueError, match="1 ... 645 cells a side"):
        granulometry_spec("x", 0)
    assert granulometry_spec("x", None) is None and granulometry_spec("x", None, radii=[0.0, 46340.9]) is None
    spec = granulometry_spec("x", 645, dr=2)
    assert spec.pop("radii").tolist() == list(range(1, 33))
    assert spec == dict(N=645, threshold=0.5, phase="ionised", periodic=True, dr=2.0, distances=False)
    # the default radii: 1 ... max(1, min(N // 4, 32)); an int n: 1 ... n
    for N, n in ((2, 1), (3, 1), (8, 2), (70, 17), (128, 32), (256, 32)):
        assert granulometry_spec("x", N)["radii"].tolist() == list(range(1, n + 1))
    assert granulometry_spec("x", 8, radii=5)["radii"].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
    assert granulometry_spec("x", 8, radii=(0, 1.5, 7))["radii"].tolist() == [0.0, 1.5, 7.0]
    _install(monkeypatch, SB.Untouchable(), ready=False)
    with pytest.raises(RuntimeError, match="GPU not initialized"):
        granulometry(f)


def test_the_two_forms_of_the_module_entry(monkeypatch):
    from pyc2ray_amd import _capi
    granulometry = _module().granulometry
    lib = _install(monkeypatch, GB.Counting(9))
    f = np.random.default_rng(0).random((9, 9, 9))
    g = granulometry(f, threshold=0.25, phase="neutral", periodic=False, radii=(1, 2.5), dr=3.0, distances=True)
    assert lib.names() == ["grid_to_device", "granulometry"]
    up, call = lib.calls
    assert up[1][0] == _capi.GRID_XH and np.array_equal(up[1][1], f)
    assert call[1][:4] == (_capi.GRID_XH, 0.25, 1, False) and call[1][4].tolist() == [1.0, 2.5] and call[2] == {"distances": True}
    assert g.opened.tolist() == [360, 300] and g.eroded.tolist() == [180, 150] and g.tallies.tolist() == GB.TALLIES.tolist()
    assert (g.N, g.dr, g.phase, g.threshold, g.periodic) == (9, 3.0, "neutral", 0.25, False) and g.dist2.shape == (9, 9, 9)
    lib.calls.clear()
    g = granulometry(None, grid=_capi.GRID_XH_AV)                   # the device grid where it lies, the default radii of its mesh
    assert lib.names() == ["granulometry"] and lib.calls[0][1][:4] == (_capi.GRID_XH_AV, 0.5, 0, True)
    assert lib.calls[0][1][4].tolist() == [1.0, 2.0] and lib.calls[0][2] == {"distances": False} and g.N == 9 and g.dist2 is None
    lib.calls.clear()
    assert granulometry(None, radii=3).dr is None and lib.calls[0][1][0] == _capi.GRID_XH and lib.calls[0][1][4].tolist() == [1.0, 2.0, 3.0]


def test_yaml_keys_the_attribute_and_the_forms_the_class_takes(tmp_path, monkeypatch):
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.c2ray_base as B
    from pyc2ray_amd import _capi
    M = _module()
    assert pc2r.granulometry is M.granulometry and pc2r.Granulometry is M.Granulometry
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 8
        plain = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        assert plain.granulometry_stats is False and plain.last_granulometry is None
        with pytest.raises(ValueError, match="C2Ray.granulometry_stats: granulometry_stats needs use_gpu=True"):
            plain.granulometry_stats = True
        plain.granulometry_stats = False
        for bad in (1, 0, None, "on", 1.0):
            with pytest.raises(ValueError, match="granulometry_stats must be a bool"):
                plain.granulometry_stats = bad
        body = open(PLAIN_PARAMS).read()
        key = lambda text: body.replace("  logfile: pyC2Ray.log\n", f"  logfile: pyC2Ray.log\n{text}")
        assert key("x") != body
        for text, what in (("  granulometry: 2\n", "Output: granulometry must be 0 or 1"), ("  granulometry: 'yes'\n", "must be 0 or 1"),
                           ("  granulometry: 1.0\n", "must be 0 or 1"),
                           ("  granulometry: 1\n", "Output: granulometry: 1: granulometry_stats needs use_gpu=True"),
                           ("  granulometry_threshold: .nan\n", "threshold must be a finite number"),
                           ("  granulometry_threshold: half\n", "threshold must be"),
                           ("  granulometry_radii: 0\n", "radii as an int must be in"), ("  granulometry_radii: [2, 1]\n", "strictly ascending"),
                           ("  granulometry_radii: [1, .inf]\n", "radii must be finite"), ("  granulometry_radii: many\n", "radii must be None, an int")):
            with open("p.yml", "w") as f:
                f.write(key(text))
            with pytest.raises(ValueError, match=what):
                pc2r.C2Ray_Test("p.yml", N, False)
        with open("p.yml", "w") as f:
            f.write(key("  granulometry: 0\n  granulometry_radii: [1, 2.5, 4]\n"))
        assert pc2r.C2Ray_Test("p.yml", N, False).granulometry_stats is False
        # the committed parameter file is refused without use_gpu, as the key says
        with pytest.raises(ValueError, match="Output: granulometry: 1: granulometry_stats needs use_gpu=True"):
            pc2r.C2Ray_Test(GRANULOMETRY_PARAMS, N, False)
        # an object with use_gpu (as one constructed with use_gpu=True has it) reading its keys
        sim = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        sim.gpu = True
        sim._read_paramfile(GRANULOMETRY_PARAMS)
        sim._statistic_init("granulometry_stats")
        assert sim.granulometry_stats is True and sim.last_granulometry is None
        lib = _install(monkeypatch, GB.Counting(N))
        steps = []
        monkeypatch.setattr(B, "evolve3D", lambda *a, **kw: steps.append("evolve3D") or (np.full((N, N, N), 0.75), np.zeros((N, N, N))))
        monkeypatch.setattr(B, "evolve3D_resident", lambda *a, **kw: steps.append("evolve3D_resident"))
        flux, pos = np.ones(1), np.ones((3, 1), dtype=int)
        # the resident path: the device grid where it lies -- no upload, no download, the bookkeeping untouched
        sim.device_resident = True
        sim.evolve3D(2.0, flux, pos)
        assert steps == ["evolve3D_resident"] and lib.names() == ["granulometry"]
        assert lib.calls[0][1][:4] == (_capi.GRID_XH, 0.4, 0, True) and lib.calls[0][1][4].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
        assert lib.calls[0][2] == {"distances": False}
        first = sim.last_granulometry
        assert (first.n_phase, first.dr, first.periodic, first.threshold, first.N) == (400, sim.dr, True, 0.4, N)
        assert first.opened.tolist() == [360, 320, 280, 240, 200] and first.unresolved == 0.5
        assert sim._device_newer >= {"xh", "phi_ion"} and "xh" not in sim._host_newer
        lib.calls.clear()
        g = sim.granulometry(radii=[2.0, 6.0], phase="neutral", dr=None, periodic=False, distances=True)     # keywords override keys and defaults
        assert lib.names() == ["granulometry"] and lib.calls[0][1][:4] == (_capi.GRID_XH, 0.4, 1, False)
        assert lib.calls[0][1][4].tolist() == [2.0, 6.0] and lib.calls[0][2] == {"distances": True}
        assert g.dr is None and g.periodic is False and g is not sim.last_granulometry and sim.last_granulometry is first
        assert g.dist2 is not None and sim._device_newer >= {"xh", "phi_ion"} and "xh" not in sim._host_newer
        # periodic and dr are the object's
        lib.calls.clear()
        sim.periodic = False
        g = sim.granulometry()
        assert lib.calls[0][1][:4] == (_capi.GRID_XH, 0.4, 0, False) and g.periodic is False and g.dr == sim.dr
        sim.periodic = True
        for name in ("field", "grid"):
            with pytest.raises(ValueError, match=f"C2Ray.granulometry: {name} is not for the class"):
                sim.granulometry(**{name: None})
        with pytest.raises(ValueError, match="C2Ray.granulometry: radii must be strictly ascending"):
            sim.granulometry(radii=[2, 2])
        # otherwise: the host array goes up first
        lib.calls.clear()
        sim._device_newer.clear()
        sim.device_resident = False
        sim.evolve3D(3.0, flux, pos)
        assert steps[-1] == "evolve3D" and lib.names() == ["grid_to_device", "granulometry"]
        assert lib.calls[0][1][0] == _capi.GRID_XH and np.all(lib.calls[0][1][1] == 0.75) and lib.calls[1][1][4].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
        assert sim.last_granulometry is not first
        assert open(sim.logfile).read().count("Granulometry (ionised, x >= 0.4, periodic, 5 radii to 5): 400 cells, largest inscribed ball r2 49") == 2
        # off: a step makes no library call of the feature's, and leaves the last result alone
        kept = sim.last_granulometry
        sim.granulometry_stats = False
        for resident in (True, False):
            lib.calls.clear()
            sim._device_newer.clear()
            sim.device_resident = resident
            sim.evolve3D(1.0, flux, pos)
            assert lib.calls == [] and sim.last_granulometry is kept
        assert open(sim.logfile).read().count("Granulometry (") == 2
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
    assert lib.names() and not [n for n in lib.names() if "granulometry" in n]
