"""CPU: the host side of the redshift-space analysis: the C-ABI symbols and the enums the header pins, what
redshift_space_spec refuses before the library is touched and what it makes of the three binnings, AnisotropicSpectrum's
normalisations, the forms of the module's calls and the wiring of the class (on a stand-in for the library)."""
import ctypes as C
import importlib
import math
import os

import numpy as np
import pytest

import lls_standin_backend as SB
import redshift_space_reference as RR
import redshift_space_standin_backend as ZB

HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_test.yml")
RS_PARAMS = os.path.join(HERE, "data", "parameters_redshift_space.yml")


@pytest.fixture(scope="module", autouse=True)
def no_leftover_device():
    """As in tests/test_powerspec_host.py: the code-2 check below needs a library without a device."""
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    lib = _capi.load()
    if lib.asora_device_ptr(_capi.GRID_NDENS) and not p.cuda_is_init():
        assert lib.asora_device_close() == 0
    yield


def _module():
    return importlib.import_module("pyc2ray_amd.redshift_space")


def _install(monkeypatch, backend, ready=True):
    import pyc2ray_amd.c2ray_base as B
    for mod in (_module(), B):
        monkeypatch.setattr(mod, "load_asora", lambda: backend)
        monkeypatch.setattr(mod, "cuda_is_init", lambda: ready)
    return backend


def test_capi_symbols_and_header():
    from pyc2ray_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "asora_hip.h")).read()
    assert ("int asora_power_spectrum_los(int kind, double scale, double t_gamma, int los_axis, int use_velocity, double velocity_scale, "
            "int mode,\n") in header
    assert "int asora_los_velocity_to_device(const double *v, int N, char order, double *max_abs);" in header
    assert "int asora_los_velocity_clear(void);" in header
    assert "int asora_debug_power_spectrum_los_ms(double *ms /* [ASORA_PSLOS_STAGES] */);" in header
    assert "int asora_redshift_space_field(int kind, double scale, double t_gamma, int los_axis, int use_velocity, double velocity_scale,\n" in header
    assert "ASORA_ANISO_CYLINDRICAL = 0, ASORA_ANISO_MU = 1, ASORA_ANISO_MODES = 2, ASORA_ANISO_MAX_BINS = 1024" in header
    assert (_capi.ANISO_CYLINDRICAL, _capi.ANISO_MU, _capi.ANISO_MODES, _capi.ANISO_MAX_BINS) == (0, 1, 2, 1024)
    assert "ASORA_PSLOS_STAGES = 6" in header and _capi.PSLOS_STAGES == 6
    assert (RR.CYLINDRICAL, RR.MU, RR.MAX_BINS) == (_capi.ANISO_CYLINDRICAL, _capi.ANISO_MU, _capi.ANISO_MAX_BINS)
    # the enums the header pins keep their values: the velocity is no grid, the mapped field no kind, no stage, slot or option is new
    for pinned in ("ASORA_GRID_COUNT = 9", "ASORA_PS_KINDS = 4", "ASORA_PS_STAGES = 5", "ASORA_KERNEL_COUNT = 4", "ASORA_KERNEL_SLOTS = 7",
                   "ASORA_OPT_COUNT = 19", "ASORA_SMOOTH_STAGES = 8", "ASORA_BUBBLE_MAX_BINS = 256"):
        assert pinned in header, pinned
    assert (_capi.GRID_COUNT, _capi.PS_KINDS, _capi.PS_STAGES, _capi.SMOOTH_STAGES, _capi.BUBBLE_MAX_BINS) == (9, 4, 5, 8, 256)
    n_args = {"asora_power_spectrum_los": 21, "asora_redshift_space_field": 9, "asora_los_velocity_to_device": 4, "asora_los_velocity_clear": 0,
              "asora_debug_power_spectrum_los_ms": 1, "asora_power_spectrum": 15, "asora_smooth_field": 15}
    for name, n in n_args.items():
        assert len(_capi.SIGNATURES[name][1]) == n, name
    lib = _capi.load()                    # (opening the library resolves every declared symbol)
    if not lib.asora_device_ptr(_capi.GRID_NDENS):      # no device initialised in this process: refused as every entry is
        ta, tb = np.array([1, 4, 9], dtype=np.uint32), np.array([0.0, 2.0])
        n = np.full(2, 9, dtype=np.uint64)
        out = [np.full(2, 9.0) for _ in range(7)]
        rc = lib.asora_power_spectrum_los(_capi.PS_XH, 1.0, 0.0, 2, 0, 1.0, _capi.ANISO_MU, 2, ta.ctypes.data_as(C.POINTER(C.c_uint32)), 1,
                                          _capi.dptr(tb), n.ctypes.data_as(_capi._u64p), *[_capi.dptr(a) for a in out], None, None)
        assert rc == 2 and b"power_spectrum_los" in lib.asora_last_error() and np.all(n == 9) and all(np.all(a == 9.0) for a in out)
        assert lib.asora_redshift_space_field(_capi.PS_XH, 1.0, 0.0, 2, 0, 1.0, -1, None, None) == 2
        v, vmax = np.zeros(8), C.c_double(-1.0)
        assert lib.asora_los_velocity_to_device(_capi.dptr(v), 2, b"C", C.byref(vmax)) == 2 and vmax.value == -1.0
        assert lib.asora_los_velocity_clear() == 0
    ms = np.full(6, -1.0)
    assert lib.asora_debug_power_spectrum_los_ms(_capi.dptr(ms)) == 0 and np.all(ms >= 0.0)
    assert lib.asora_debug_power_spectrum_los_ms(None) == 3


def test_spec_refusals_come_before_the_library():
    M = _module()
    S = M.redshift_space_spec
    N = 16
    ones = np.ones((N, N, N))
    bad = [(dict(kind="tb"), "kind must be one of"), (dict(los_axis=3), "los_axis must be 0, 1 or 2"), (dict(los_axis=True), "los_axis must be"),
           (dict(los_axis=1.0), "los_axis must be"), (dict(binning="spherical"), "binning must be one of"),
           (dict(velocity_scale=math.nan), "velocity_scale must be a finite number"), (dict(velocity_scale="1"), "velocity_scale must be"),
           (dict(velocity=np.ones((N, N))), "velocity must be a real"), (dict(velocity=np.ones((4, 4, 4))), "velocity must have the shape"),
           (dict(velocity=np.where(np.arange(N ** 3).reshape(N, N, N) == 77, np.nan, 1.0)), "velocity has a non-finite entry"),
           (dict(velocity=np.where(np.arange(N ** 3).reshape(N, N, N) == 77, np.inf, 1.0)), "velocity has a non-finite entry"),
           (dict(velocity=ones, max_velocity=1.0), "max_velocity goes with a velocity that is on the device"),
           (dict(max_velocity=-1.0), "max_velocity must be a finite number >= 0"),
           (dict(velocity=ones, velocity_scale=7.0), "wider than the N = 16 cells of a line"),
           (dict(max_velocity=3.5, velocity_scale=-2.0), "2 W \\+ 1 = 17 cells"),
           (dict(bins=4), "binning 'cylindrical' takes bins_perp and bins_par"), (dict(mu_bins=4), "takes bins_perp and bins_par"),
           (dict(binning="mu", bins_perp=3), "takes bins and mu_bins, not bins_perp or bins_par"),
           (dict(binning="multipoles", mu_bins=3), "has one bin of mu"), (dict(binning="multipoles", bins_par=3), "takes bins, not"),
           (dict(bins_perp=0), "bins_perp as an int must be in"), (dict(bins_par=1025), "bins_par as an int must be in"),
           (dict(bins_perp=[1, 1]), "the edges of bins_perp must be finite, >= 0 and strictly ascending"),
           (dict(bins_par=[-1, 1]), "finite, >= 0 and strictly ascending"), (dict(bins_perp=True), "not a bool"),
           (dict(bins_perp=33, bins_par=32), "33 x 32 bins are more than the 1024"),
           (dict(binning="mu", mu_bins=0), "mu_bins as an int must be in"), (dict(binning="mu", mu_bins=[0.5, 0.2]), "mu_bins must be finite"),
           (dict(binning="mu", bins=[0, 1]), "must be > 0"), (dict(binning="mu", bins=300), "bins as an int must be in"),
           (dict(binning="mu", bins=205, mu_bins=5), "205 x 5 bins are more than"),
           (dict(box_len=0), "box_len must be None or a finite number > 0"), (dict(scale=math.inf), "scale must be a finite number"),
           (dict(t_gamma=-1), "t_gamma must be a finite number >= 0"), (dict(into=9), "into must be None or a grid selector"),
           (dict(return_field=1), "return_field must be a bool"), (dict(return_modes="no"), "return_modes must be a bool")]
    for kw, what in bad:
        with pytest.raises(ValueError, match="^who: .*" + what.replace("(", "\\(").replace(")", "\\)")):
            S("who", N, **kw)
    with pytest.raises(ValueError, match="the mesh must have 1 ... 645 cells a side"):
        S("who", 646)
    # the entries: the same refusals with no library in reach, and before a device is asked for
    import pyc2ray_amd.redshift_space as Z
    for entry in (Z.power_spectrum_los, Z.redshift_space_field):
        with pytest.raises(ValueError, match="los_axis must be 0, 1 or 2"):
            entry(np.zeros((4, 4, 4)), los_axis=5)
        with pytest.raises(ValueError, match="a host field is analysed as kind 'xh' or 'xhi'"):
            entry(np.zeros((4, 4, 4)), kind="density")
        with pytest.raises(ValueError, match="wider than the N = 4 cells"):
            entry(np.zeros((4, 4, 4)), velocity=np.ones((4, 4, 4)), velocity_scale=1.5)


def test_spec_thresholds_of_the_three_binnings():
    S = _module().redshift_space_spec
    from pyc2ray_amd import _capi
    N = 16
    s = S("who", N)
    assert s["mode"] == _capi.ANISO_CYLINDRICAL and s["velocity_scale"] is None and s["max_velocity"] is None
    assert s["edges_a"].tolist() == [0.0] + [b + 0.5 for b in range(9)] and s["thr_a"].tolist() == [0, 1, 3, 7, 13, 21, 31, 43, 57, 73]
    assert s["thr_a"].dtype == np.uint32 and s["thr_b"].dtype == np.float64 and s["thr_b"].tolist() == s["thr_a"].tolist()
    s = S("who", 100)
    assert (s["thr_a"].size - 1) * (s["thr_b"].size - 1) == 32 * 32 == _capi.ANISO_MAX_BINS
    s = S("who", N, bins_perp=[0, 1, 2.5], bins_par=2)
    assert s["thr_a"].tolist() == [0, 1, 7] and s["edges_b"].tolist() == [0.0, 4.25, 8.5] and s["thr_b"].tolist() == [0.0, 19.0, 73.0]
    s = S("who", N, binning="mu")
    assert s["mode"] == _capi.ANISO_MU and s["thr_a"].tolist() == [1, 3, 7, 13, 21, 31, 43, 57, 73]
    assert s["edges_b"].tolist() == np.linspace(0, 1, 6).tolist() and s["thr_b"].tolist() == (np.linspace(0, 1, 6) ** 2).tolist()[:-1] + [2.0]
    s = S("who", N, binning="mu", bins=[1, 2, 3], mu_bins=[0, 0.5, math.sqrt(0.5), 1.0])
    assert s["thr_a"].tolist() == [1, 4, 9] and s["thr_b"].tolist() == [0.0, 0.25, math.sqrt(0.5) ** 2, 1.0]      # (mu = 1 left out)
    s = S("who", N, binning="multipoles", bins=3, velocity=np.full((N, N, N), -2.0), velocity_scale=1.7, los_axis=0, box_len=3.0)
    assert s["mode"] == _capi.ANISO_MU and s["thr_b"].tolist() == [0.0, 2.0] and s["edges_b"].tolist() == [0.0, 1.0] and s["thr_a"].size == 4
    assert (s["velocity_scale"], s["max_velocity"], s["los_axis"], s["box_len"]) == (1.7, 2.0, 0, 3.0) and s["velocity"].shape == (N, N, N)
    assert M_window(2.0, 1.7) == 4 == RR.library_window(2.0, 1.7)
    assert S("who", N, max_velocity=6.9 / 1.7, velocity_scale=1.7)["velocity"] is None                  # W = 7: 15 <= 16
    assert S("who", None, binning="mu", bins=3) is None


def M_window(vmax, scale):
    return _module().window_of(vmax, scale)


def test_anisotropic_spectrum_normalisations():
    from pyc2ray_amd import AnisotropicSpectrum
    N, L = 8, 16.0
    a = ZB.answer(N, [1, 4, 9], [0.0, 0.25, 2.0])
    args = [a[k] for k in ("count", "sum_1", "sum_2", "sum_aa", "sum_l2", "sum_l4", "moments_real", "moments_rs")]
    sp = AnisotropicSpectrum("mu", [1, 2, 3], [0.0, 0.5, 1.0], *args, N, los_axis=1, velocity=True, box_len=L)
    unit = 2 * math.pi / L
    assert sp.n_modes.shape == (2, 2) and np.allclose(sp.P, 4 * L ** 3) and np.allclose(sp.k, unit * np.array([[1, 1], [2, 2]]))
    assert np.allclose(sp.mu, 0.5) and np.allclose(sp.k_par, sp.k * 0.5) and np.allclose(sp.k_perp, sp.k * math.sqrt(0.75))
    assert np.allclose(sp.P0, 4 * L ** 3) and np.allclose(sp.P2, 5 * 2 * L ** 3) and np.allclose(sp.P4, 9 * 0.5 * L ** 3)
    assert np.allclose(sp.k_multipoles, unit * np.array([1.0, 2.0]))
    assert (sp.mean_real, sp.mean_rs) == (1.0, 1.0) and (sp.variance_real, sp.variance_rs) == (3.0, 5.0)
    line = sp.log_line()
    assert line.startswith("Redshift-space spectrum (dtb, mu, 2 x 2 bins, line of sight 1, redshift space, L = 16 units of box_len): 60 modes, ")
    assert "P2 / P0 there 2.5000" in line
    cyl = AnisotropicSpectrum("cylindrical", [0, 1, 2], [0.0, 1.0, 2.0], *args, N)
    assert cyl.P0 is None and cyl.P2 is None and cyl.k_multipoles is None and cyl.L == 8.0
    assert np.allclose(cyl.k_perp, 2 * math.pi / 8 * np.array([[1, 1], [2, 2]])) and np.allclose(cyl.k_par, 2 * math.pi / 8 * 0.5)
    assert np.allclose(cyl.k, np.hypot(cyl.k_perp, cyl.k_par)) and "real space: no velocity, L = 8 cells" in cyl.log_line()
    empty = AnisotropicSpectrum("multipoles", [1, 2], [0, 1], np.zeros((1, 1), dtype=np.uint64), *[np.zeros((1, 1))] * 5, [0, 0], [0, 0], N)
    assert np.isnan(empty.P0[0]) and empty.log_line().endswith("; no mode in any bin")
    with pytest.raises(ValueError, match="go with arrays of shape"):
        AnisotropicSpectrum("mu", [1, 2, 3, 4], [0.0, 0.5, 1.0], *args, N)
    with pytest.raises(ValueError, match="binning must be one of"):
        AnisotropicSpectrum("polar", [1, 2, 3], [0.0, 0.5, 1.0], *args, N)


def test_the_forms_of_the_modules_calls(monkeypatch):
    import pyc2ray_amd as pc2r
    from pyc2ray_amd import _capi
    M = _module()
    assert pc2r.power_spectrum_los is M.power_spectrum_los and pc2r.redshift_space_field is M.redshift_space_field
    assert pc2r.AnisotropicSpectrum is M.AnisotropicSpectrum and pc2r.redshift_space is M
    N = 8
    f, v = np.random.default_rng(3).random((N, N, N)), np.full((N, N, N), 0.25)
    monkeypatch.setattr(M, "cuda_is_init", lambda: False)
    monkeypatch.setattr(M, "load_asora", lambda: SB.Untouchable())
    with pytest.raises(RuntimeError, match="GPU not initialized"):
        M.power_spectrum_los(f)
    lib = _install(monkeypatch, ZB.Counting(N))
    sp = M.power_spectrum_los(f, velocity=v, velocity_scale=2.0, los_axis=0, binning="mu", bins=[1, 2, 3], mu_bins=2, box_len=16.0,
                              return_field=True)
    assert lib.names() == ["grid_to_device", "los_velocity_to_device", "power_spectrum_los"]
    up, vel, call = lib.calls
    assert up[1][0] == _capi.GRID_XH and np.array_equal(up[1][1], f) and np.array_equal(vel[1][0], v)
    assert call[1][:6] == (_capi.PS_XH, 1.0, 0.0, 0, 2.0, _capi.ANISO_MU) and call[1][6].tolist() == [1, 4, 9] and call[1][7].tolist() == [0.0, 0.25, 2.0]
    assert call[2] == {"field": True, "modes": False}
    assert (sp.binning, sp.kind, sp.N, sp.los_axis, sp.velocity, sp.box_len) == ("mu", "xh", N, 0, True, 16.0) and sp.field.shape == (N, N, N)
    assert sp.n_modes.tolist() == [[10, 10], [20, 20]] and np.array_equal(sp.moments_rs, ZB.MOMENTS_RS)
    lib.calls.clear()
    sp = M.power_spectrum_los(None, kind="dtb", scale=25.0, t_gamma=30.0, binning="multipoles", return_modes=True)     # the device grids
    assert lib.names() == ["power_spectrum_los"] and lib.calls[0][1][:6] == (_capi.PS_HI, 25.0, 30.0, 2, None, _capi.ANISO_MU)
    assert lib.calls[0][1][7].tolist() == [0.0, 2.0] and not sp.velocity and sp.modes.shape == (N, N, N // 2 + 1) and sp.P2.shape == (4,)
    lib.calls.clear()
    sp = M.power_spectrum_los(f, kind="xhi")
    assert lib.names() == ["grid_to_device", "power_spectrum_los"] and lib.calls[1][1][0] == _capi.PS_XHI and lib.calls[1][1][5] == _capi.ANISO_CYLINDRICAL
    assert sp.n_modes.shape == (5, 5)
    lib.calls.clear()
    cube = M.redshift_space_field(f, velocity=v, velocity_scale=-1.0, los_axis=1)
    assert lib.names() == ["grid_to_device", "los_velocity_to_device", "redshift_space_field"] and cube.shape == (N, N, N)
    assert lib.calls[2][1] == (_capi.PS_XH, 1.0, 0.0, 1, -1.0) and lib.calls[2][2] == {"dst_grid": None, "field": True}
    lib.calls.clear()
    assert M.redshift_space_field(None, kind="density", into=_capi.GRID_XH) is None
    assert lib.names() == ["redshift_space_field"] and lib.calls[0][1] == (_capi.PS_DENSITY, 1.0, 0.0, 2, None)
    assert lib.calls[0][2] == {"dst_grid": _capi.GRID_XH, "field": False}


def test_yaml_keys_the_attributes_and_the_forms_the_class_takes(tmp_path, monkeypatch):
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.c2ray_base as B
    from pyc2ray_amd import _capi
    assert B.C2Ray._STEP_STATISTICS_APPENDED == ("redshift_space_stats",) and len(B.C2Ray._STEP_STATISTICS) == 7
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 8
        plain = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        assert plain.redshift_space_stats is False and plain.last_redshift_space is None and plain.los_velocity is None and plain.los_axis == 2
        with pytest.raises(ValueError, match="C2Ray.redshift_space_stats: redshift_space_stats needs use_gpu=True"):
            plain.redshift_space_stats = True
        with pytest.raises(ValueError, match="redshift_space_stats must be a bool"):
            plain.redshift_space_stats = 1
        body = open(PLAIN_PARAMS).read()
        key = lambda text: body.replace("  logfile: pyC2Ray.log\n", f"  logfile: pyC2Ray.log\n{text}")
        for text, what in (("  redshift_space: 2\n", "Output: redshift_space must be 0 or 1"),
                           ("  redshift_space: 1\n", "Output: redshift_space: 1: redshift_space_stats needs use_gpu=True"),
                           ("  redshift_space_binning: polar\n", "binning must be one of"), ("  redshift_space_bins: 0\n", "bins as an int must be in"),
                           ("  redshift_space_binning: cylindrical\n  redshift_space_bins: [2, 1]\n", "the edges of bins_perp must be finite, >= 0 and strictly"),
                           ("  redshift_space_los_axis: 3\n", "los_axis must be 0, 1 or 2")):
            with open("p.yml", "w") as f:
                f.write(key(text))
            with pytest.raises(ValueError, match=what):
                pc2r.C2Ray_Test("p.yml", N, False)
        with pytest.raises(ValueError, match="Output: redshift_space: 1: redshift_space_stats needs use_gpu=True"):
            pc2r.C2Ray_Test(RS_PARAMS, N, False)
        # an object with use_gpu (as one constructed with use_gpu=True has it) reading its keys
        sim = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        sim.gpu = True
        sim._read_paramfile(RS_PARAMS)
        sim._statistic_init("redshift_space_stats")
        assert sim.redshift_space_stats is True and sim.last_redshift_space is None and sim.los_axis == 1
        cs = sim._ld["Cosmology"]
        z = sim.zred
        hubble = 100 * cs["h"] * math.sqrt(cs["Omega0"] * (1 + z) ** 3 + 1 - cs["Omega0"])          # (radiation: below 1e-2 at this z)
        want = (1 + z) / (hubble * sim.boxsize_c / B.Mpc / N)
        assert abs(sim.velocity_scale() - want) <= 1e-2 * want and sim.velocity_scale() > 0
        box = sim.boxsize_c / B.Mpc
        for bad, what in ((np.ones((N, N)), "must be None or a real"), (np.full((N, N, N), np.nan), "non-finite entry"), ("v", "must be None")):
            with pytest.raises(ValueError, match="C2Ray.los_velocity: .*" + what):
                sim.los_velocity = bad
        with pytest.raises(ValueError, match="C2Ray.los_axis: los_axis must be 0, 1 or 2"):
            sim.los_axis = 4
        lib = _install(monkeypatch, ZB.Counting(N))
        steps = []
        monkeypatch.setattr(B, "evolve3D_resident", lambda *a, **kw: steps.append("evolve3D_resident"))
        flux, pos = np.ones(1), np.ones((3, 1), dtype=int)
        sim.device_resident = True
        # no velocity: the real-space spectrum, resolved in direction, and the line says so
        sim.evolve3D(2.0, flux, pos)
        assert steps == ["evolve3D_resident"] and lib.names() == ["power_spectrum_los"]
        assert lib.calls[0][1][:6] == (_capi.PS_HI, sim.brightness_temperature_scale(), 0.0, 1, None, _capi.ANISO_MU)
        assert lib.calls[0][1][6].tolist() == [1, 3, 7, 13, 21] and lib.calls[0][1][7].tolist() == [0.0, 2.0]
        first = sim.last_redshift_space
        assert (first.binning, first.kind, first.los_axis, first.velocity, first.box_len) == ("multipoles", "dtb", 1, False, box)
        assert sim._device_newer >= {"xh", "phi_ion"} and "xh" not in sim._host_newer
        # a velocity: uploaded once per assignment, not per step
        v = np.full((N, N, N), 1.0)
        v[0, 0, 0] = -2.0
        sim.los_velocity = v
        lib.calls.clear()
        sim.evolve3D(2.0, flux, pos)
        sim.evolve3D(2.0, flux, pos)
        assert lib.names() == ["los_velocity_to_device", "power_spectrum_los", "power_spectrum_los"]
        assert np.array_equal(lib.calls[0][1][0], v) and lib.calls[1][1][4] == sim.velocity_scale() and sim.last_redshift_space.velocity
        assert sim._device_newer >= {"xh", "phi_ion"}
        log = open(sim.logfile).read()
        head = f"Redshift-space spectrum (dtb, multipoles, 4 x 1 bins, line of sight 1, "
        assert log.count(head + f"real space: no velocity, L = {box:g} units of box_len): 100 modes, ") == 1
        assert log.count(head + f"redshift space, L = {box:g} units of box_len): 100 modes, ") == 2
        sim.los_velocity = v                                       # assigned again: up again
        lib.calls.clear()
        sim.los_axis = 0
        sp = sim.power_spectrum_los(binning="cylindrical", bins=2, spin="kinetic", kind="xhi", box_len=None)
        assert lib.names() == ["los_velocity_to_device", "power_spectrum_los"] and lib.calls[1][1][3] == 0 and lib.calls[1][1][5] == _capi.ANISO_CYLINDRICAL
        assert lib.calls[1][1][2] == cs["cmbtemp"] * (1 + sim.zred) and sp.n_modes.shape == (2, 2) and sp.box_len is None
        assert sim.last_redshift_space is not sp
        lib.calls.clear()
        cube = sim.redshift_space_field()
        assert lib.names() == ["redshift_space_field"] and cube.shape == (N, N, N) and lib.calls[0][1][3:] == (0, sim.velocity_scale())
        for name in ("field", "velocity", "max_velocity"):
            with pytest.raises(ValueError, match=f"C2Ray.power_spectrum_los: {name} is not for the class"):
                sim.power_spectrum_los(**{name: None})
        with pytest.raises(ValueError, match="C2Ray.power_spectrum_los: into is for redshift_space_field"):
            sim.power_spectrum_los(into=1)
        # a velocity too large for the mesh is refused before the library hears of it
        sim.los_velocity = np.full((N, N, N), 4.0 / sim.velocity_scale())
        lib.calls.clear()
        with pytest.raises(ValueError, match="C2Ray.power_spectrum_los: .*wider than the N = 8 cells of a line"):
            sim.power_spectrum_los()
        assert lib.calls == []
        sim.los_velocity = None
        # off: a step makes no library call of the feature's, and leaves the last result alone
        kept = sim.last_redshift_space
        sim.redshift_space_stats = False
        before = open(sim.logfile).read()
        sim.evolve3D(1.0, flux, pos)
        assert lib.calls == [] and sim.last_redshift_space is kept and open(sim.logfile).read() == before
    finally:
        os.chdir(cwd)
        if "sim" in locals():      # (nothing of this object lives on a device: a later step elsewhere must not ask it to fetch)
            sim._device_newer.clear()
            sim.device_resident = False
