"""CPU: the host side of the smoothing: the C-ABI symbols, SmoothedField's arithmetic, the forms of ``bins``
and the two calls an integer takes, the argument checks of smoothed_field (before the library is touched), the comoving distance and
the beam of the class, its YAML keys and attributes, and which form of the call it takes (on a stand-in for the library)."""
import importlib
import math
import os

import numpy as np
import pytest

import lls_standin_backend as SB
import smoothing_standin_backend as MB

HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_test.yml")
OBSERVED_PARAMS = os.path.join(HERE, "data", "parameters_observed_map.yml")


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
    return importlib.import_module("pyc2ray_amd.smoothing")


def _install(monkeypatch, backend, ready=True):
    import pyc2ray_amd.c2ray_base as B
    for mod in (_module(), B):
        monkeypatch.setattr(mod, "load_asora", lambda: backend)
        monkeypatch.setattr(mod, "cuda_is_init", lambda: ready)
    return backend


def test_capi_symbol_and_header():
    from pyc2ray_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "asora_hip.h")).read()
    assert ("int asora_smooth_field(int kind, double scale, double t_gamma,\n"
            "                       const double *w_i, const double *w_j, const double *w_k,") in header
    assert "double *stats, uint64_t *hist, double *field_out);" in header
    assert "int asora_debug_smooth_field_ms(double *ms /* [ASORA_SMOOTH_STAGES] */);" in header
    assert header.index("int asora_debug_power_spectrum_ms(") < header.index("int asora_smooth_field(") < header.index("C. Options, measurement")
    assert "ASORA_SMOOTH_STATS = 10" in header and _capi.SMOOTH_STATS == 10 and "ASORA_SMOOTH_MAX_BINS = 4096" in header
    assert _capi.SMOOTH_MAX_BINS == 4096 and f"ASORA_SMOOTH_STAGES = {_capi.SMOOTH_STAGES}" in header
    assert (_capi.SMOOTH_N_FINITE, _capi.SMOOTH_N_NONFINITE, _capi.SMOOTH_MIN, _capi.SMOOTH_MAX, _capi.SMOOTH_INPUT_SUM,
            _capi.SMOOTH_INPUT_SUM2, _capi.SMOOTH_SUM, _capi.SMOOTH_S2, _capi.SMOOTH_S3, _capi.SMOOTH_S4) == tuple(range(10))
    assert "ASORA_GRID_COUNT = 9" in header and "ASORA_KERNEL_COUNT = 4" in header and "ASORA_KERNEL_SLOTS = 7" in header
    assert "ASORA_OPT_COUNT = 19" in header                                    # (no grid, no timing slot, no option)
    assert len(_capi.SIGNATURES["asora_smooth_field"][1]) == 15
    lib = _capi.load()                    # (opening the library resolves every declared symbol)
    if not lib.asora_device_ptr(_capi.GRID_NDENS):      # no device initialised in this process: refused as every entry is
        stats, field = np.full(10, 9.0), np.full(8, 9.0)
        rc = lib.asora_smooth_field(_capi.PS_XH, 1.0, 0.0, None, None, None, None, 0, 0, 0, None, -1, _capi.dptr(stats), None, _capi.dptr(field))
        assert rc == 2 and b"smooth_field" in lib.asora_last_error() and b"not initialised" in lib.asora_last_error()
        assert np.all(stats == 9) and np.all(field == 9)                       # (a refused call writes nothing)
        ms = np.full(_capi.SMOOTH_STAGES, 9.0)
        assert lib.asora_debug_smooth_field_ms(_capi.dptr(ms)) == 0 and np.all(ms == 0) and lib.asora_debug_smooth_field_ms(None) == 3


def test_smoothed_field_arithmetic():
    SmoothedField = _module().SmoothedField
    N = 4
    n = 64.0
    #          finite nonfinite min max  sum g  sum g^2  sum h   S2       S3        S4
    stats = [n - 1, 1.0, -1.5, 2.5, 16.0, 80.0, 32.0, 4.0 * n, -16.0 * n, 64.0 * n]
    sf = SmoothedField(stats, N, edges=[-2.0, 0.0, 1.0, 3.0], hist=[10, 21, 32, 0, 0], kind="xh", subtract_mean=True)
    assert sf.mean == 0.5 and sf.variance == 4.0 and sf.skewness == -2.0 and sf.kurtosis == 1.0 and (sf.min, sf.max) == (-1.5, 2.5)
    assert sf.input_mean == 0.25 and sf.input_variance == 80.0 / 64 - 0.0625 and sf.n_finite == 63 and sf.n_nonfinite == 1
    assert sf.hist.dtype == np.uint64 and sf.hist.tolist() == [10, 21, 32] and (sf.below, sf.above) == (0, 0)
    assert sf.bin_centres.tolist() == [-1.0, 0.5, 2.0] and np.allclose(sf.pdf, np.array([10 / 2.0, 21 / 1.0, 32 / 2.0]) / 63, rtol=1e-15)
    assert abs(float(np.sum(sf.pdf * np.diff(sf.edges))) - 1.0) < 1e-15
    line = sf.log_line()
    assert line.startswith("Smoothed field (xh, identity, mean removed): mean 5.000000e-01, variance 4.000000e+00, skewness -2.0000, "
                           "kurtosis 1.0000, min -1.500000e+00, max 2.500000e+00; input variance 1.187500e+00; 1 non-finite cells; "
                           "3 bins hold 63 cells") and "\n" not in line and repr(sf) == f"<SmoothedField: {line}>"
    plain = SmoothedField(stats, N)
    assert plain.hist is None and plain.pdf is None and plain.bin_centres is None and plain.below is None and "bins" not in plain.log_line()
    flat = SmoothedField([n, 0, 1.0, 1.0, n, n, n, 0.0, 0.0, 0.0], N)
    assert flat.variance == 0.0 and math.isnan(flat.skewness) and math.isnan(flat.kurtosis) and flat.mean == 1.0
    with pytest.raises(ValueError, match="10 stats, not 9"):
        SmoothedField(stats[:9], N)
    with pytest.raises(ValueError, match="come together"):
        SmoothedField(stats, N, edges=[0, 1])
    with pytest.raises(ValueError, match="2 edges go with 1 bins and two more counts, not 2"):
        SmoothedField(stats, N, edges=[0, 1], hist=[1, 2])


def test_the_forms_of_bins_and_the_two_calls_of_an_integer(monkeypatch):
    from pyc2ray_amd import _capi
    M = _module()
    N = 8
    lib = _install(monkeypatch, MB.Counting(N))
    f = np.random.default_rng(0).random((N, N, N))
    filt = M.gaussian(2.0) * M.sharp_k(3)
    # no bins: one call, no histogram
    sf = M.smoothed_field(f, filter=filt, subtract_mean=True)
    assert lib.names() == ["grid_to_device", "smooth_field"] and lib.calls[0][1][0] == _capi.GRID_XH and np.array_equal(lib.calls[0][1][1], f)
    name, args, kw = lib.calls[1]
    assert args == (_capi.PS_XH, 1.0, 0.0) and kw["subtract_mean"] is True and kw["edges"] is None and kw["dst_grid"] is None and kw["field"] is False
    want = filt.tables(N)
    assert all(np.array_equal(kw[k], w) for k, w in zip(("w_i", "w_j", "w_k", "w_r"), want)) and kw["w_r"].size == 3 * 16 + 1
    assert sf.hist is None and sf.kind == "xh" and sf.filter is filt and sf.subtract_mean and sf.mean == 0.5 and sf.kurtosis == -1.0
    # an array of edges: one call
    lib.calls.clear()
    sf = M.smoothed_field(f, kind="xhi", bins=[-1.0, 0.0, 2.5], into=_capi.GRID_XH_AV, return_field=True)
    assert lib.names() == ["grid_to_device", "smooth_field"]
    kw = lib.calls[1][2]
    assert lib.calls[1][1][0] == _capi.PS_XHI and kw["edges"].tolist() == [-1.0, 0.0, 2.5] and kw["dst_grid"] == _capi.GRID_XH_AV and kw["field"] is True
    assert all(kw[k] is None for k in ("w_i", "w_j", "w_k", "w_r"))
    assert sf.hist.tolist() == [10, 20] and (sf.below, sf.above) == (3, 4) and sf.field.shape == (N, N, N)
    # an int: the range is the first call's, the histogram (and into, and the download) the second's
    lib.calls.clear()
    sf = M.smoothed_field(None, kind="dtb", scale=25.0, t_gamma=30.0, bins=4, into=_capi.GRID_XH, return_field=True)
    assert lib.names() == ["smooth_field", "smooth_field"]
    (_, a1, k1), (_, a2, k2) = lib.calls
    assert a1 == a2 == (_capi.PS_HI, 25.0, 30.0)
    assert k1["edges"] is None and k1["dst_grid"] is None and k1["field"] is False
    assert k2["edges"].tolist() == [-1.0, 0.0, 1.0, 2.0, float(np.nextafter(3.0, np.inf))] and k2["dst_grid"] == _capi.GRID_XH and k2["field"] is True
    assert sf.edges.tolist() == k2["edges"].tolist() and sf.hist.tolist() == [10, 20, 30, 40]
    assert M.edges_for_range("x", 2, 1.5, 1.5).tolist() == [1.0, 1.5, float(np.nextafter(2.0, np.inf))]
    with pytest.raises(ValueError, match="needs a finite cell"):
        M.edges_for_range("x", 2, math.inf, -math.inf)
    with pytest.raises(ValueError, match="too narrow for 4096 bins"):
        M.edges_for_range("x", 4096, 1.0, float(np.nextafter(1.0, 2.0)))


def test_bad_arguments_are_refused_before_the_library_is_touched(monkeypatch):
    M = _module()
    smoothed_field = M.smoothed_field
    _install(monkeypatch, SB.Untouchable())
    f = np.zeros((8, 8, 8))
    for kw, what in ((dict(kind="HI"), "kind must be one of"), (dict(kind=3), "kind must be one of"),
                     (dict(filter="gaussian"), "filter must be None or a Filter"), (dict(filter=2.0), "filter must be None or a Filter"),
                     (dict(subtract_mean=1), "subtract_mean must be a bool"), (dict(return_field=0), "return_field must be a bool"),
                     (dict(bins=0), "bins as an int must be in \\[1, 4096\\]"), (dict(bins=4097), "bins as an int must be in"),
                     (dict(bins=True), "not a bool"), (dict(bins=[1.0]), "one-dimensional array of 2 ... 4097 edges"),
                     (dict(bins=np.arange(4099.0)), "2 ... 4097 edges"), (dict(bins=[[1.0, 2.0]]), "one-dimensional"),
                     (dict(bins="many"), "bins must be None, an int or an array"), (dict(bins=[1.0, np.nan]), "must be finite"),
                     (dict(bins=[1.0, 1.0]), "strictly ascending"), (dict(bins=[2.0, 1.0]), "strictly ascending"),
                     (dict(scale=np.nan), "scale must be a finite number"), (dict(scale=True), "scale must be"),
                     (dict(t_gamma=-1.0), "t_gamma must be a finite number >= 0"), (dict(t_gamma=np.inf), "t_gamma must be"),
                     (dict(into=9), "into must be None or a grid selector 0 ... 8"), (dict(into=-1), "into must be"),
                     (dict(into="xh"), "into must be"), (dict(into=True), "into must be")):
        with pytest.raises(ValueError, match=f"smoothed_field: .*{what}"):
            smoothed_field(None, **kw)
        if "kind" not in kw:
            with pytest.raises(ValueError, match=f"smoothed_field: .*{what}"):
                smoothed_field(f, **kw)
    for bad in (np.zeros((8, 8)), np.zeros((8, 8, 4)), np.zeros((4, 4, 4), dtype=complex)):
        with pytest.raises(ValueError, match="field must be a real"):
            smoothed_field(bad)
    with pytest.raises(ValueError, match="a host field is analysed as kind 'xh' or 'xhi', not 'density'"):
        smoothed_field(f, kind="density")
    with pytest.raises(ValueError, match="1 ... 645 cells a side"):
        M.smoothing_spec("x", 646)
    bad = M.Filter([(0, lambda m, N: np.where(m == 1, np.inf, 1.0))], "bad")
    with pytest.raises(ValueError, match="has a non-finite entry at N = 8"):
        smoothed_field(f, filter=bad)
    _install(monkeypatch, SB.Untouchable(), ready=False)
    with pytest.raises(RuntimeError, match="GPU not initialized"):
        smoothed_field(f)


def test_comoving_distance_and_the_beam(tmp_path):
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.c2ray_base as B
    # Einstein-de Sitter: D_c = 2 c / H0 (1 - 1 / sqrt(1 + z)), a closed form
    eds = B.FlatLambdaCDMLite(70.0, 1.0, Tcmb0=0.0)
    for z in (0.0, 0.5, 3.0, 9.0, 30.0):
        want = 2.0 * 299792.458 / 70.0 * (1.0 - 1.0 / math.sqrt(1.0 + z))
        assert abs(eds.comoving_distance(z) - want) <= 1e-10 * max(want, 1.0), z
    # the beam in cells for a stated z, B and box: lambda_21 (1 + z) / B x D_c / (boxsize / N)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 24
        sim = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
    finally:
        os.chdir(cwd)
    cs = sim._ld["Cosmology"]
    lite = B.FlatLambdaCDMLite(100 * cs["h"], cs["Omega0"], cs["cmbtemp"])
    z = 9.0
    d_c = lite.comoving_distance(z)
    assert abs(sim.comoving_distance(z) - d_c) <= 1e-6 * d_c and 5000.0 < d_c < 12000.0          # (Mpc; astropy or the lite class)
    cell = sim._ld["Grid"]["boxsize"] / N
    want = 0.211 * (1 + z) / (8000.0 * 1e3) * d_c / cell
    assert abs(sim.beam_fwhm_cells(8000.0, z=z) - want) <= 1e-6 * want
    assert abs(sim.beam_fwhm_cells(2.0, z=z) / sim.beam_fwhm_cells(8000.0, z=z) - 4000.0) <= 1e-9 * 4000.0
    assert sim.beam_fwhm_cells(8000.0) == sim.beam_fwhm_cells(8000.0, z=sim.zred)


def test_yaml_keys_the_attribute_and_the_forms_the_class_takes(tmp_path, monkeypatch):
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.c2ray_base as B
    from pyc2ray_amd import _capi
    M = _module()
    assert pc2r.smoothed_field is M.smoothed_field and pc2r.SmoothedField is M.SmoothedField and pc2r.smoothing is M
    assert pc2r.telescope is M.telescope and pc2r.gaussian is M.gaussian and pc2r.Filter is M.Filter
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 8
        plain = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        assert plain.observed_stats is False and plain.last_observed is None
        with pytest.raises(ValueError, match="C2Ray.observed_stats: observed_stats needs use_gpu=True"):
            plain.observed_stats = True
        plain.observed_stats = False
        for bad in (1, 0, None, "on"):
            with pytest.raises(ValueError, match="observed_stats must be a bool"):
                plain.observed_stats = bad
        body = open(PLAIN_PARAMS).read()
        key = lambda text: body.replace("  logfile: pyC2Ray.log\n", f"  logfile: pyC2Ray.log\n{text}")
        assert key("x") != body
        for text, what in (("  observed_map: 2\n", "Output: observed_map must be 0 or 1"), ("  observed_map: 'yes'\n", "must be 0 or 1"),
                           ("  observed_map: 1\n", "Output: observed_map: 1: observed_stats needs use_gpu=True"),
                           ("  observed_baseline_km: 0\n", "baseline_km must be a finite number > 0"),
                           ("  observed_baseline_km: far\n", "baseline_km must be"), ("  observed_los_axis: 3\n", "los_axis must be 0, 1 or 2"),
                           ("  observed_los_axis: 1.0\n", "los_axis must be"), ("  observed_bins: 0\n", "bins as an int must be in"),
                           ("  observed_bins: [2, 1]\n", "strictly ascending")):
            with open("p.yml", "w") as f:
                f.write(key(text))
            with pytest.raises(ValueError, match=what):
                pc2r.C2Ray_Test("p.yml", N, False)
        with open("p.yml", "w") as f:
            f.write(key("  observed_map: 0\n  observed_bins: [-1, 0, 1]\n"))
        assert pc2r.C2Ray_Test("p.yml", N, False).observed_stats is False
        with pytest.raises(ValueError, match="Output: observed_map: 1: observed_stats needs use_gpu=True"):
            pc2r.C2Ray_Test(OBSERVED_PARAMS, N, False)
        # an object with use_gpu (as one constructed with use_gpu=True has it) reading its keys
        sim = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        sim.gpu = True
        sim._read_paramfile(OBSERVED_PARAMS)
        sim._statistic_init("observed_stats")
        assert sim.observed_stats is True and sim.last_observed is None
        lib = _install(monkeypatch, MB.Counting(N))
        steps = []
        monkeypatch.setattr(B, "evolve3D", lambda *a, **kw: steps.append("evolve3D") or (np.full((N, N, N), 0.75), np.zeros((N, N, N))))
        monkeypatch.setattr(B, "evolve3D_resident", lambda *a, **kw: steps.append("evolve3D_resident"))
        flux, pos = np.ones(1), np.ones((3, 1), dtype=int)
        # the resident path: the device grids where they lie -- no upload, no download; observed_bins: 5 takes two calls
        sim.device_resident = True
        sim.evolve3D(2.0, flux, pos)
        assert steps == ["evolve3D_resident"] and lib.names() == ["smooth_field", "smooth_field"]
        width = sim.beam_fwhm_cells(8000.0)
        want = M.telescope(width, width, los_axis=1).tables(N)
        for (_, args, kw), binned in zip(lib.calls, (False, True)):
            assert args == (_capi.PS_HI, sim.brightness_temperature_scale(), 0.0) and kw["subtract_mean"] is True and kw["dst_grid"] is None
            assert kw["field"] is False and (kw["edges"] is not None) == binned and kw["w_r"] is None
            assert all(np.array_equal(kw[k], w) for k, w in zip(("w_i", "w_j", "w_k"), want))
        assert np.array_equal(want[1], M.boxcar(width, 1).tables(N)[1]) and np.array_equal(want[0], want[2])
        first = sim.last_observed
        assert first.kind == "dtb" and first.N == N and first.subtract_mean and first.hist.tolist() == [10, 20, 30, 40, 50]
        assert first.edges.size == 6 and first.edges[0] == -1.0 and first.edges[-1] == np.nextafter(3.0, np.inf)
        assert sim._device_newer >= {"xh", "phi_ion"} and "xh" not in sim._host_newer
        # the keywords of a call: the class's filter or any other, spin, into (which gives up the residency)
        lib.calls.clear()
        sf = sim.observed_map(baseline_km=4000.0, los_axis=0, subtract_mean=False, bins=None, spin="kinetic", return_field=True)
        assert lib.names() == ["smooth_field"] and lib.calls[0][1][2] == sim._ld["Cosmology"]["cmbtemp"] * (1 + sim.zred)
        assert lib.calls[0][2]["subtract_mean"] is False and lib.calls[0][2]["field"] is True and sf.hist is None and sim.last_observed is first
        assert np.array_equal(lib.calls[0][2]["w_i"], M.boxcar(2 * width, 0).tables(N)[0])
        lib.calls.clear()
        sf = sim.smoothed_field(kind="xh", filter=M.sharp_k(2), scale=3.0)
        assert lib.names() == ["smooth_field"] and lib.calls[0][1] == (_capi.PS_XH, 3.0, 0.0) and lib.calls[0][2]["w_r"] is not None
        for call, what in ((lambda: sim.smoothed_field(field=None), "field is not for the class"),
                           (lambda: sim.observed_map(filter=M.sharp_k(2)), "the filter is the telescope's"),
                           (lambda: sim.smoothed_field(spin="saturated"), "spin must be None or 'kinetic'"),
                           (lambda: sim.smoothed_field(spin="kinetic", t_gamma=1.0), "spin='kinetic' sets t_gamma itself"),
                           (lambda: sim.observed_map(baseline_km=-1.0), "C2Ray.observed_map: baseline_km must be"),
                           (lambda: sim.observed_map(los_axis=5), "C2Ray.observed_map: los_axis must be"),
                           (lambda: sim.smoothed_field(bins=[2, 2]), "C2Ray.smoothed_field: the edges of bins must be strictly ascending")):
            with pytest.raises(ValueError, match=what):
                call()
        assert lib.calls[1:] == []
        # otherwise: the host arrays go up first
        lib.calls.clear()
        sim._device_newer.clear()
        sim.device_resident = False
        sim.evolve3D(3.0, flux, pos)
        assert steps[-1] == "evolve3D" and lib.names() == ["grid_to_device"] * 3 + ["smooth_field"] * 2
        assert [c[1][0] for c in lib.calls[:3]] == [_capi.GRID_XH, _capi.GRID_NDENS, _capi.GRID_TEMP] and np.all(lib.calls[0][1][1] == 0.75)
        assert sim.last_observed is not first
        assert open(sim.logfile).read().count("Smoothed field (dtb, gaussian(") == 2 and "mean removed): mean 5.000000e-01" in open(sim.logfile).read()
        # off: a step makes no library call of the feature's, and leaves the last result alone
        kept = sim.last_observed
        sim.observed_stats = False
        for resident in (True, False):
            lib.calls.clear()
            sim._device_newer.clear()
            sim.device_resident = resident
            sim.evolve3D(1.0, flux, pos)
            assert lib.calls == [] and sim.last_observed is kept
        assert open(sim.logfile).read().count("Smoothed field (") == 2
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
    assert lib.names() and not [n for n in lib.names() if "smooth" in n]
