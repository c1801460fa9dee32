"""CPU: the host side of the power spectrum: the C-ABI symbols, PowerSpectrum's normalisations, the three forms
of ``bins``, the argument checks of power_spectrum (before the library is touched), the YAML keys and attributes of the class, and
which form of the call the class takes (on a stand-in for the library)."""
import importlib
import math
import os

import numpy as np
import pytest

import lls_standin_backend as SB
import powerspec_reference as PR
import powerspec_standin_backend as PB

HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_test.yml")
POWER_PARAMS = os.path.join(HERE, "data", "parameters_power_spectrum.yml")


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
    return importlib.import_module("pyc2ray_amd.powerspec")


def _install(monkeypatch, backend, ready=True):
    import pyc2ray_amd.c2ray_base as B
    for mod in (_module(), B):
        monkeypatch.setattr(mod, "load_asora", lambda: backend)
        monkeypatch.setattr(mod, "cuda_is_init", lambda: ready)
    return backend


def test_capi_symbol_and_header():
    import ctypes as C
    from pyc2ray_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "asora_hip.h")).read()
    assert ("int asora_power_spectrum(int kind_a, int kind_b, double scale, double t_gamma, int n_bins, const unsigned *thresholds,\n"
            "                         unsigned long long *count, double *sum_k, double *sum_aa, double *sum_bb, double *sum_ab,\n") in header
    assert "int asora_debug_power_spectrum_ms(double *ms /* [ASORA_PS_STAGES] */);" in header
    for n, name in enumerate(("XH", "XHI", "DENSITY", "HI")):
        assert f"ASORA_PS_{name} = {n}," in header and getattr(_capi, f"PS_{name}") == n
    assert "ASORA_PS_KINDS = 4" in header and _capi.PS_KINDS == 4 and "ASORA_PS_STAGES = 5" in header and _capi.PS_STAGES == 5
    assert "ASORA_KERNEL_SLOTS = 7" in header and "ASORA_OPT_COUNT = 19" in header           # (no timing slot, no option)
    assert len(_capi.SIGNATURES["asora_power_spectrum"][1]) == 15
    lib = _capi.load()                    # (opening the library resolves every declared symbol)
    if not lib.asora_device_ptr(_capi.GRID_NDENS):      # no device initialised in this process: refused as every entry is
        thr = np.array([1, 4, 9], dtype=np.uint32)
        n, k, aa, m = np.full(2, 9, dtype=np.uint64), np.full(2, 9.0), np.full(2, 9.0), np.full(2, 9.0)
        rc = lib.asora_power_spectrum(_capi.PS_XH, -1, 1.0, 0.0, 2, thr.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      n.ctypes.data_as(_capi._u64p), _capi.dptr(k), _capi.dptr(aa), None, None, _capi.dptr(m), None, None, None)
        assert rc == 2 and b"power_spectrum" in lib.asora_last_error() and b"not initialised" in lib.asora_last_error()
        assert np.all(n == 9) and np.all(k == 9) and np.all(aa == 9) and np.all(m == 9)      # (a refused call writes nothing)
        ms = np.full(5, 9.0)
        assert lib.asora_debug_power_spectrum_ms(_capi.dptr(ms)) == 0 and np.all(ms == 0) and lib.asora_debug_power_spectrum_ms(None) == 3


def test_power_spectrum_normalisations():
    PowerSpectrum = _module().PowerSpectrum
    N, L = 4, 8.0
    n6 = float(N) ** 6
    # two bins: 6 modes of |n| = 1 and 12 of |n| = sqrt 2
    ps = PowerSpectrum([0.5, 1.2, 1.6], [6, 12], [6.0, 12 * math.sqrt(2)], [6 * 2 * n6, 12 * 5 * n6], [32.0, 80.0], N, box_len=L, kind="xh")
    assert ps.n_modes.dtype == np.uint64 and ps.n_modes.tolist() == [6, 12] and ps.thresholds.tolist() == [1, 2, 3] and ps.L == L
    assert np.allclose(ps.k, 2 * math.pi / L * np.array([1.0, math.sqrt(2)]), rtol=1e-15)
    assert np.allclose(ps.P, L ** 3 * np.array([2.0, 5.0]), rtol=1e-15)
    assert np.allclose(ps.Delta2, ps.k ** 3 * ps.P / (2 * math.pi ** 2), rtol=1e-15)
    assert ps.mean == 0.5 and ps.variance == 80.0 / 64 - 0.25
    assert ps.cross is False and ps.P_b is None and ps.P_cross is None and ps.r is None and ps.mean_b is None and ps.variance_b is None
    assert abs(ps.parseval_residual - ((12 + 60) * n6 / 64 / (80.0 - 32.0 ** 2 / 64) - 1.0)) < 1e-12
    line = ps.log_line()
    assert line.startswith("Power spectrum (xh, 2 bins to |n| = 1.6, L = 8 units of box_len): 18 modes, mean 5.000000e-01, variance 1.000000e+00; "
                           "largest Delta2 ") and "\n" not in line and repr(ps) == f"<PowerSpectrum: {line}>"
    # units of cells without box_len; an empty bin gives NaN and nothing else does
    cells = PowerSpectrum([0.5, 1.5, 1.6, 2.5], [6, 0, 20], [6.0, 0.0, 30.0], [6 * n6, 0.0, 40 * n6], [0.0, 64.0], N)
    assert cells.L == 4.0 and cells.box_len is None and "L = 4 cells" in cells.log_line()
    assert np.isnan(cells.k[1]) and np.isnan(cells.P[1]) and np.isnan(cells.Delta2[1]) and np.isfinite(cells.P[[0, 2]]).all()
    assert np.allclose(cells.P[[0, 2]], [64.0, 128.0]) and np.allclose(cells.k[[0, 2]], 2 * math.pi / 4 * np.array([1.0, 1.5]))
    # the cross-spectrum and the correlation coefficient
    x = PowerSpectrum([0.5, 1.5], [6], [6.0], [6 * 4 * n6], [0.0, 64.0], N, sum_bb=[6 * 9 * n6], sum_ab=[-6 * 3 * n6], moments_b=[64.0, 128.0],
                      kind="xh", kind_b="density")
    assert x.cross and np.allclose(x.P_b, [9 * 64.0]) and np.allclose(x.P_cross, [-3 * 64.0]) and np.allclose(x.r, [-0.5])
    assert x.mean_b == 1.0 and x.variance_b == 1.0 and "xh x density" in x.log_line() and "r there -0.5000" in x.log_line()
    empty = PowerSpectrum([5.5, 6.5], [0], [0.0], [0.0], [0.0, 0.0], N, sum_bb=[0.0], sum_ab=[0.0], moments_b=[0.0, 0.0])
    assert np.isnan(empty.r[0]) and math.isnan(empty.parseval_residual) and "no mode in any bin" in empty.log_line()
    with pytest.raises(ValueError, match="3 edges go with 2 bins"):
        PowerSpectrum([1, 2, 3], [1], [1.0], [1.0], [0, 0], N)
    with pytest.raises(ValueError, match="come together"):
        PowerSpectrum([1, 2], [1], [1.0], [1.0], [0, 0], N, sum_bb=[1.0])
    with pytest.raises(ValueError, match="2 moments"):
        PowerSpectrum([1, 2], [1], [1.0], [1.0], [0, 0, 0], N)


def test_the_three_forms_of_bins():
    spec = _module().powerspec_spec
    for N, nb in ((1, 1), (2, 1), (3, 1), (8, 4), (9, 4), (250, 125), (256, 128), (600, 256), (645, 256)):
        s = spec("x", N)
        assert s["edges"].tolist() == [b + 0.5 for b in range(nb + 1)], N
        assert s["thresholds"].tolist() == [1] + [b * b + b + 1 for b in range(1, nb + 1)]       # ceil((b + 1/2)^2) = b^2 + b + 1
        assert np.array_equal(s["thresholds"], PR.thresholds_of(s["edges"])) and s["thresholds"].dtype == np.uint32
    s = spec("x", 16, bins=4)
    assert s["edges"].tolist() == [0.5, 2.5, 4.5, 6.5, 8.5] and s["thresholds"].tolist() == [1, 7, 21, 43, 73]
    assert spec("x", 1, bins=2)["edges"].tolist() == [0.5, 1.0, 1.5]
    s = spec("x", 16, bins=(1, 2, 3.5))
    assert s["edges"].tolist() == [1.0, 2.0, 3.5] and s["thresholds"].tolist() == [1, 4, 13]          # modes on an edge: the upper bin
    assert spec("x", 16, bins=[1e-200, 1e30])["thresholds"].tolist() == [1, 2 ** 32 - 1]
    assert spec("x", None, bins=[1, 2]) is None and spec("x", None) is None and spec("x", None, bins=7) is None
    full = spec("x", 645, kind="hi", kind_b="density", box_len=3, scale=2, t_gamma=30, return_field=True)
    assert {k: v for k, v in full.items() if k not in ("edges", "thresholds")} == dict(
        N=645, kind="hi", kind_b="density", box_len=3.0, scale=2.0, t_gamma=30.0, return_field=True, return_modes=False)


def test_bad_arguments_are_refused_before_the_library_is_touched(monkeypatch):
    M = _module()
    power_spectrum, spec = M.power_spectrum, M.powerspec_spec
    _install(monkeypatch, SB.Untouchable())
    f = np.zeros((8, 8, 8))
    for kw, what in ((dict(kind="HI"), "kind must be one of"), (dict(kind=3), "kind must be one of"), (dict(kind=None), "kind must be one of"),
                     (dict(kind_b="ndens"), "kind_b must be None or one of"), (dict(kind_b=2), "kind_b must be None or"),
                     (dict(bins=0), "bins as an int must be in \\[1, 256\\]"), (dict(bins=257), "bins as an int must be in"),
                     (dict(bins=True), "not a bool"), (dict(bins=[1.0]), "one-dimensional array of 2 ... 257 edges"),
                     (dict(bins=np.arange(1.0, 259.0)), "2 ... 257 edges"), (dict(bins=[[1.0, 2.0]]), "one-dimensional"),
                     (dict(bins=2.5), "one-dimensional"), (dict(bins="many"), "bins must be None, an int or an array"),
                     (dict(bins=[1.0, np.nan]), "edges of bins must be finite"), (dict(bins=[1.0, np.inf]), "must be finite"),
                     (dict(bins=[0.0, 1.0]), "edges of bins must be > 0"), (dict(bins=[-1.0, 1.0]), "must be > 0"),
                     (dict(bins=[1.0, 1.0]), "strictly ascending"), (dict(bins=[2.0, 1.0]), "strictly ascending"),
                     (dict(box_len=0.0), "box_len must be None or a finite number > 0"), (dict(box_len=np.inf), "box_len must be"),
                     (dict(box_len="1"), "box_len must be"), (dict(scale=np.nan), "scale must be a finite number"),
                     (dict(scale=None), "scale must be"), (dict(scale=True), "scale must be"),
                     (dict(t_gamma=-1.0), "t_gamma must be a finite number >= 0"), (dict(t_gamma=np.inf), "t_gamma must be"),
                     (dict(t_gamma="3"), "t_gamma must be"), (dict(return_field=1), "return_field must be a bool"),
                     (dict(return_modes=0), "return_modes must be a bool")):
        with pytest.raises(ValueError, match=f"power_spectrum: .*{what}"):
            power_spectrum(None, **kw)
        if "kind" not in kw and "kind_b" not in kw:
            with pytest.raises(ValueError, match=f"power_spectrum: .*{what}"):
                power_spectrum(f, **kw)
    for bad in (np.zeros((8, 8)), np.zeros((8, 8, 4)), np.zeros((4, 4, 4), dtype=complex), [["a"]]):
        with pytest.raises(ValueError, match="field must be a real"):
            power_spectrum(bad)
        with pytest.raises(ValueError, match="field_b must be a real"):
            power_spectrum(f, bad)
    with pytest.raises(ValueError, match="field_b must have the shape of field"):
        power_spectrum(f, np.zeros((4, 4, 4)))
    with pytest.raises(ValueError, match="field_b goes with field"):
        power_spectrum(None, f)
    with pytest.raises(ValueError, match="a host field is analysed as kind 'xh' or 'xhi', not 'density'"):
        power_spectrum(f, kind="density")
    with pytest.raises(ValueError, match="a host field_b is analysed as kind_b 'density', not 'xh'"):
        power_spectrum(f, f, kind_b="xh")
    with pytest.raises(ValueError, match="kind_b goes with field_b"):
        power_spectrum(f, kind_b="density")
    with pytest.raises(ValueError, match="1 ... 645 cells a side"):
        spec("x", 646)
    with pytest.raises(ValueError, match="1 ... 645 cells a side"):
        spec("x", 0)
    _install(monkeypatch, SB.Untouchable(), ready=False)
    with pytest.raises(RuntimeError, match="GPU not initialized"):
        power_spectrum(f)


def test_the_two_forms_of_the_module_entry(monkeypatch):
    from pyc2ray_amd import _capi
    power_spectrum = _module().power_spectrum
    N = 8
    lib = _install(monkeypatch, PB.Counting(N))
    rng = np.random.default_rng(0)
    f, d = rng.random((N, N, N)), rng.random((N, N, N))
    ps = power_spectrum(f, d, bins=(1, 2, 3), box_len=16.0, return_field=True)
    assert lib.names() == ["grid_to_device", "grid_to_device", "power_spectrum"]
    up, up_b, call = lib.calls
    assert up[1][0] == _capi.GRID_XH and np.array_equal(up[1][1], f) and up_b[1][0] == _capi.GRID_NDENS and np.array_equal(up_b[1][1], d)
    assert call[1][:4] == (_capi.PS_XH, _capi.PS_DENSITY, 1.0, 0.0) and call[1][4].tolist() == [1, 4, 9]
    assert call[2] == {"field": True, "modes": False}
    assert (ps.kind, ps.kind_b, ps.N, ps.box_len) == ("xh", "density", N, 16.0) and ps.field.shape == (N, N, N) and ps.modes is None
    assert ps.n_modes.tolist() == [10, 20] and np.allclose(ps.P, 4 * 16.0 ** 3) and np.allclose(ps.P_b, 9 * 16.0 ** 3)
    assert np.allclose(ps.r, -0.5) and np.allclose(ps.k, 2 * math.pi / 16 * np.array([1.0, 2.0]))
    assert np.array_equal(ps.moments, PB.MOMENTS_A) and np.array_equal(ps.moments_b, PB.MOMENTS_B)
    lib.calls.clear()
    ps = power_spectrum(f, kind="xhi")                             # one host field, as its complement
    assert lib.names() == ["grid_to_device", "power_spectrum"] and lib.calls[1][1][:2] == (_capi.PS_XHI, None) and not ps.cross
    lib.calls.clear()
    ps = power_spectrum(None, scale=25.0, t_gamma=30.0, kind_b="density", return_modes=True)      # the device grids where they lie
    assert lib.names() == ["power_spectrum"] and lib.calls[0][1][:4] == (_capi.PS_HI, _capi.PS_DENSITY, 25.0, 30.0)
    assert lib.calls[0][1][4].tolist() == [1, 3, 7, 13, 21] and lib.calls[0][2] == {"field": False, "modes": True}
    assert (ps.kind, ps.kind_b, ps.N, ps.box_len, ps.L) == ("dtb", "density", N, None, 8.0) and ps.modes.shape == (N, N, N // 2 + 1)
    lib.calls.clear()
    assert power_spectrum(None, kind="density", bins=2).edges.tolist() == [0.5, 2.5, 4.5] and lib.calls[0][1][:2] == (_capi.PS_DENSITY, None)


def test_yaml_keys_the_attribute_and_the_forms_the_class_takes(tmp_path, monkeypatch):
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.c2ray_base as B
    from pyc2ray_amd import _capi
    M = _module()
    assert pc2r.power_spectrum is M.power_spectrum and pc2r.PowerSpectrum is M.PowerSpectrum and pc2r.powerspec is M
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 8
        plain = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        assert plain.power_spectrum_stats is False and plain.last_power_spectrum is None
        with pytest.raises(ValueError, match="C2Ray.power_spectrum_stats: power_spectrum_stats needs use_gpu=True"):
            plain.power_spectrum_stats = True
        plain.power_spectrum_stats = False
        for bad in (1, 0, None, "on", 1.0):
            with pytest.raises(ValueError, match="power_spectrum_stats must be a bool"):
                plain.power_spectrum_stats = bad
        body = open(PLAIN_PARAMS).read()
        key = lambda text: body.replace("  logfile: pyC2Ray.log\n", f"  logfile: pyC2Ray.log\n{text}")
        assert key("x") != body
        for text, what in (("  power_spectrum: 2\n", "Output: power_spectrum must be 0 or 1"), ("  power_spectrum: 'yes'\n", "must be 0 or 1"),
                           ("  power_spectrum: 1.0\n", "must be 0 or 1"),
                           ("  power_spectrum: 1\n", "Output: power_spectrum: 1: power_spectrum_stats needs use_gpu=True"),
                           ("  power_spectrum_kind: tb\n", "kind must be one of"), ("  power_spectrum_kind: 3\n", "kind must be one of"),
                           ("  power_spectrum_bins: 0\n", "bins as an int must be in"), ("  power_spectrum_bins: [2, 1]\n", "strictly ascending"),
                           ("  power_spectrum_bins: [1, .inf]\n", "must be finite"), ("  power_spectrum_bins: many\n", "bins must be None, an int")):
            with open("p.yml", "w") as f:
                f.write(key(text))
            with pytest.raises(ValueError, match=what):
                pc2r.C2Ray_Test("p.yml", N, False)
        with open("p.yml", "w") as f:
            f.write(key("  power_spectrum: 0\n  power_spectrum_bins: [1, 2.5, 4]\n"))
        assert pc2r.C2Ray_Test("p.yml", N, False).power_spectrum_stats is False
        with pytest.raises(ValueError, match="Output: power_spectrum: 1: power_spectrum_stats needs use_gpu=True"):
            pc2r.C2Ray_Test(POWER_PARAMS, N, False)
        # an object with use_gpu (as one constructed with use_gpu=True has it) reading its keys
        sim = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        sim.gpu = True
        sim._read_paramfile(POWER_PARAMS)
        sim._statistic_init("power_spectrum_stats")
        assert sim.power_spectrum_stats is True and sim.last_power_spectrum is None
        cs = sim._ld["Cosmology"]
        scale = 27.0 * math.sqrt((1 + sim.zred) / 10 * 0.15 / (cs["Omega0"] * cs["h"] ** 2)) * (cs["Omega_B"] * cs["h"] ** 2 / 0.023)
        assert abs(sim.brightness_temperature_scale() - scale) <= 1e-15 * scale and 5.0 < scale < 100.0
        box = sim.boxsize_c / B.Mpc
        lib = _install(monkeypatch, PB.Counting(N))
        steps = []
        monkeypatch.setattr(B, "evolve3D", lambda *a, **kw: steps.append("evolve3D") or (np.full((N, N, N), 0.75), np.zeros((N, N, N))))
        monkeypatch.setattr(B, "evolve3D_resident", lambda *a, **kw: steps.append("evolve3D_resident"))
        flux, pos = np.ones(1), np.ones((3, 1), dtype=int)
        # the resident path: the device grids where they lie -- no upload, no download, the bookkeeping untouched
        sim.device_resident = True
        sim.evolve3D(2.0, flux, pos)
        assert steps == ["evolve3D_resident"] and lib.names() == ["power_spectrum"]
        assert lib.calls[0][1][:4] == (_capi.PS_HI, None, sim.brightness_temperature_scale(), 0.0)
        assert lib.calls[0][1][4].tolist() == PR.thresholds_of(np.linspace(0.5, 4.5, 7)).tolist() and lib.calls[0][2] == {"field": False, "modes": False}
        first = sim.last_power_spectrum
        assert (first.kind, first.kind_b, first.N, first.box_len) == ("dtb", None, N, box) and first.n_modes.tolist() == [10, 20, 30, 40, 50, 60]
        assert sim._device_newer >= {"xh", "phi_ion"} and "xh" not in sim._host_newer
        lib.calls.clear()
        ps = sim.power_spectrum(kind="xhi", kind_b="density", bins=[1, 2], box_len=None, scale=2.0, spin="kinetic", return_field=True)
        assert lib.names() == ["power_spectrum"] and lib.calls[0][1][:3] == (_capi.PS_XHI, _capi.PS_DENSITY, 2.0)
        assert lib.calls[0][1][3] == cs["cmbtemp"] * (1 + sim.zred) and lib.calls[0][1][4].tolist() == [1, 4]
        assert lib.calls[0][2] == {"field": True, "modes": False} and ps.box_len is None and ps.cross and sim.last_power_spectrum is first
        for name in ("field", "field_b"):
            with pytest.raises(ValueError, match=f"C2Ray.power_spectrum: {name} is not for the class"):
                sim.power_spectrum(**{name: None})
        with pytest.raises(ValueError, match="C2Ray.power_spectrum: spin must be None or 'kinetic'"):
            sim.power_spectrum(spin="saturated")
        with pytest.raises(ValueError, match="spin='kinetic' sets t_gamma itself"):
            sim.power_spectrum(spin="kinetic", t_gamma=1.0)
        with pytest.raises(ValueError, match="C2Ray.power_spectrum: the edges of bins must be strictly ascending"):
            sim.power_spectrum(bins=[2, 2])
        assert lib.calls[1:] == []
        # otherwise: the host arrays go up first
        lib.calls.clear()
        sim._device_newer.clear()
        sim.device_resident = False
        sim.evolve3D(3.0, flux, pos)
        assert steps[-1] == "evolve3D" and lib.names() == ["grid_to_device"] * 3 + ["power_spectrum"]
        assert [c[1][0] for c in lib.calls[:3]] == [_capi.GRID_XH, _capi.GRID_NDENS, _capi.GRID_TEMP] and np.all(lib.calls[0][1][1] == 0.75)
        assert sim.last_power_spectrum is not first
        assert open(sim.logfile).read().count(f"Power spectrum (dtb, 6 bins to |n| = 4.5, L = {box:g} units of box_len): 210 modes, ") == 2
        # off: a step makes no library call of the feature's, and leaves the last result alone
        kept = sim.last_power_spectrum
        sim.power_spectrum_stats = False
        for resident in (True, False):
            lib.calls.clear()
            sim._device_newer.clear()
            sim.device_resident = resident
            sim.evolve3D(1.0, flux, pos)
            assert lib.calls == [] and sim.last_power_spectrum is kept
        assert open(sim.logfile).read().count("Power spectrum (") == 2
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
    assert lib.names() and not [n for n in lib.names() if "power_spectrum" in n]
