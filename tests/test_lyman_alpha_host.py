"""CPU: the host side of the Lyman-alpha forest: the C-ABI symbols and the enums the header pins, what
lyman_alpha_spec refuses before the library is touched, LymanAlphaForest's derived numbers, the forms of the module's calls and the
wiring of the class with its two scale factors (on a stand-in for the library)."""
import ctypes as C
import importlib
import math
import os

import numpy as np
import pytest

import lls_standin_backend as SB
import lyman_alpha_reference as R
import lyman_alpha_standin_backend as LB

HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_test.yml")
LYA_PARAMS = os.path.join(HERE, "data", "parameters_lyman_alpha.yml")


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
    return importlib.import_module("pyc2ray_amd.lyman_alpha")


def _install(monkeypatch, backend, ready=True):
    import pyc2ray_amd.c2ray_base as B
    for mod in (_module(), B):
        monkeypatch.setattr(mod, "load_asora", lambda: backend)
        monkeypatch.setattr(mod, "cuda_is_init", lambda: ready)
    return backend


def test_capi_symbols_and_header():
    from pyc2ray_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "asora_hip.h")).read()
    assert "int asora_lyman_alpha_forest(int los_axis, int use_velocity, double velocity_scale, double b_scale, double tau_scale,\n" in header
    assert "int asora_debug_lya_forest_ms(double *ms /* [ASORA_LYA_STAGES] */);" in header
    assert "ASORA_LYA_FLUX = 0, ASORA_LYA_TAU = 1, ASORA_LYA_MAX_BINS = 1024" in header
    assert "ASORA_LYA_SUM_F = 0, ASORA_LYA_SUM_F2 = 1, ASORA_LYA_TAU_MIN = 2, ASORA_LYA_TAU_MAX = 3, ASORA_LYA_STATS = 4" in header
    assert "ASORA_LYA_NONFINITE = 0, ASORA_LYA_WINDOW = 1, ASORA_LYA_CLIPPED = 2, ASORA_LYA_DEGENERATE = 3, ASORA_LYA_N_DARK = 4," in header
    assert "ASORA_LYA_N_GAPS = 5, ASORA_LYA_LONGEST = 6, ASORA_LYA_FULL_LINES = 7, ASORA_LYA_COUNTS = 8" in header
    assert "ASORA_LYA_STAGES = 4" in header and _capi.LYA_STAGES == 4
    assert (_capi.LYA_FLUX, _capi.LYA_TAU, _capi.LYA_MAX_BINS, _capi.LYA_STATS, _capi.LYA_COUNTS) == (0, 1, 1024, 4, 8)
    assert (_capi.LYA_SUM_F, _capi.LYA_SUM_F2, _capi.LYA_TAU_MIN, _capi.LYA_TAU_MAX) == (0, 1, 2, 3)
    assert (_capi.LYA_NONFINITE, _capi.LYA_WINDOW, _capi.LYA_CLIPPED, _capi.LYA_DEGENERATE, _capi.LYA_N_DARK, _capi.LYA_N_GAPS, _capi.LYA_LONGEST,
            _capi.LYA_FULL_LINES) == tuple(range(8))
    assert (R.FLUX, R.TAU, R.MAX_BINS) == (_capi.LYA_FLUX, _capi.LYA_TAU, _capi.LYA_MAX_BINS)
    # the enums the header pins keep their values: F and tau are no grids, no kernel slot or option is new
    for pinned in ("ASORA_GRID_COUNT = 9", "ASORA_PS_KINDS = 4", "ASORA_KERNEL_COUNT = 4", "ASORA_KERNEL_SLOTS = 7", "ASORA_OPT_COUNT = 19",
                   "ASORA_SMOOTH_STAGES = 8", "ASORA_PSLOS_STAGES = 6", "ASORA_ANISO_MAX_BINS = 1024"):
        assert pinned in header, pinned
    assert len(_capi.SIGNATURES["asora_lyman_alpha_forest"][1]) == 17 and len(_capi.SIGNATURES["asora_debug_lya_forest_ms"][1]) == 1
    lib = _capi.load()                    # (opening the library resolves every declared symbol)
    if not lib.asora_device_ptr(_capi.GRID_NDENS):      # no device initialised in this process: refused as every entry is
        stats, counts, gaps = np.full(4, 9.0), np.full(8, 9, dtype=np.uint64), np.full(9, 9, dtype=np.uint64)
        rc = lib.asora_lyman_alpha_forest(2, 0, 1.0, 1.0, 1.0, 0, 0.05, 0, None, -1, 0, _capi.dptr(stats), counts.ctypes.data_as(_capi._u64p), None,
                                          gaps.ctypes.data_as(_capi._u64p), None, None)
        assert rc == 2 and b"lyman_alpha_forest" in lib.asora_last_error()
        assert np.all(stats == 9.0) and np.all(counts == 9) and np.all(gaps == 9)
    ms = np.full(4, -1.0)
    assert lib.asora_debug_lya_forest_ms(_capi.dptr(ms)) == 0 and np.all(ms >= 0.0)
    assert "int asora_debug_lya_forest_tiles(int N, int los_axis, int *tiles /* [4] */);" in header
    assert len(_capi.SIGNATURES["asora_debug_lya_forest_tiles"][1]) == 3
    assert lib.asora_debug_lya_forest_ms(None) == 3


def test_tiles_by_mesh():
    """The tiles the documents name (csrc/lya_forest.hip): 16 columns up to N = 307, 8 up to 611, then 4, with 1024
    work items and no more than 156 KiB of LDS; rows to 48 KiB with 256 work items.  A host computation: no device."""
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    for axis in (0, 1):
        got = {N: lib.lyman_alpha_forest_tiles(N, axis) for N in (1, 24, 70, 256, 307, 308, 320, 611, 612, 645)}
        assert {N: t["lines"] for N, t in got.items()} == {1: 16, 24: 16, 70: 16, 256: 16, 307: 16, 308: 8, 320: 8, 611: 8, 612: 4, 645: 4}
        assert all(t["work_items"] == 1024 and t["lds_bytes"] <= 156 * 1024 for t in got.values())
        assert got[307]["lds_bytes"] > 150 * 1024 and got[611]["lds_bytes"] > 150 * 1024
        for N, t in got.items():
            per_plane = -(-N // t["lines"]) if axis == 1 else None
            assert t["workgroups"] == (N * per_plane if axis == 1 else -(-N * N // t["lines"])), (N, axis)
    got = {N: lib.lyman_alpha_forest_tiles(N, 2) for N in (1, 24, 33, 70, 256, 320, 645)}
    assert {N: t["lines"] for N, t in got.items()} == {1: 128, 24: 60, 33: 45, 70: 21, 256: 5, 320: 4, 645: 2}
    assert all(t["work_items"] == 256 and t["lds_bytes"] <= 48 * 1024 and t["workgroups"] == -(-N * N // t["lines"]) for N, t in got.items())
    for bad in ((0, 2), (646, 2), (24, 3), (24, -1)):
        with pytest.raises(RuntimeError, match="debug_lya_forest_tiles failed \\(code 3\\)"):
            lib.lyman_alpha_forest_tiles(*bad)
    assert _capi_load().asora_debug_lya_forest_tiles(24, 2, None) == 3


def _capi_load():
    from pyc2ray_amd import _capi
    return _capi.load()


def test_spec_refusals_come_before_the_library():
    S = _module().lyman_alpha_spec
    N = 16
    ones = np.ones((N, N, N))
    ok = dict(b_scale=0.01, tau_scale=2.0)
    bad = [(dict(xh=np.ones((N, N))), "xh must be a real"), (dict(ndens=np.ones((4, 4, 4))), "ndens must have the shape \\(16, 16, 16\\)"),
           (dict(temp="T"), "temp must be a real"), (dict(velocity=np.ones((N, N))), "velocity must be a real"),
           (dict(velocity=np.ones((4, 4, 4))), "velocity must have the shape"),
           (dict(velocity=np.where(np.arange(N ** 3).reshape(N, N, N) == 77, np.nan, 1.0)), "velocity has a non-finite entry"),
           (dict(velocity=ones, device_velocity=True), "device_velocity goes with a velocity that is on the device"),
           (dict(device_velocity=1), "device_velocity must be a bool"),
           (dict(velocity_scale=math.nan), "velocity_scale must be a finite number"), (dict(velocity_scale="1"), "velocity_scale must be"),
           (dict(b_scale=None), "b_scale must be a finite number > 0, not None"), (dict(b_scale=0.0), "b_scale must be a finite number > 0"),
           (dict(b_scale=math.inf), "b_scale must be"), (dict(b_scale=True), "b_scale must be"),
           (dict(tau_scale=None), "tau_scale must be a finite number > 0, not None"), (dict(tau_scale=-1.0), "tau_scale must be a finite number > 0"),
           (dict(tau_scale=math.nan), "tau_scale must be"),
           (dict(los_axis=3), "los_axis must be 0, 1 or 2"), (dict(los_axis=True), "los_axis must be"), (dict(los_axis=1.0), "los_axis must be"),
           (dict(window=0), "window must be None \\(automatic\\) or an int >= 1"), (dict(window=1.5), "window must be None"),
           (dict(window=True), "window must be None"), (dict(window=8), "2 W \\+ 1 = 17 cells is wider than the N = 16 cells of a line"),
           (dict(gap_threshold=math.nan), "gap_threshold must be a finite number"), (dict(gap_threshold="dark"), "gap_threshold must be"),
           (dict(bins=0), "bins as an int must be in \\[1, 1024\\]"), (dict(bins=1025), "bins as an int must be in"), (dict(bins=True), "not a bool"),
           (dict(bins=[0.5]), "bins must be a one-dimensional array of 2 ... 1025 edges"), (dict(bins=[[0, 1], [1, 2]]), "one-dimensional array"),
           (dict(bins=[0.5, 0.2]), "the edges of bins must be finite and non-decreasing"), (dict(bins=[0.0, math.inf]), "finite and non-decreasing"),
           (dict(bins="ten"), "bins must be None, an int or an array of edges"),
           (dict(into=9), "into must be None or a grid selector"), (dict(into=1.0), "into must be None or"),
           (dict(into_what="F"), "into_what must be 'flux' or 'tau'"), (dict(into_what=1), "into_what must be"),
           (dict(return_tau=1), "return_tau must be a bool"), (dict(return_flux="no"), "return_flux must be a bool")]
    for kw, what in bad:
        with pytest.raises(ValueError, match="^who: .*" + what):
            S("who", N, **{**ok, **kw})
    with pytest.raises(ValueError, match="xh, ndens and temp must have one shape"):
        S("who", None, xh=ones, temp=np.ones((4, 4, 4)), **ok)
    with pytest.raises(ValueError, match="velocity must have the shape \\(16, 16, 16\\)"):
        S("who", None, xh=ones, velocity=np.ones((4, 4, 4)), **ok)
    with pytest.raises(ValueError, match="the mesh must have 1 ... 645 cells a side"):
        S("who", 646, **ok)
    # what it makes of good keywords
    assert S("who", None, **ok) is None
    s = S("who", N, **ok)
    assert (s["N"], s["window"], s["velocity_scale"], s["into"], s["into_what"], s["gap_threshold"]) == (N, 0, None, None, "flux", 0.05)
    assert s["edges"].size == 21 and s["edges"][0] == 0.0 and s["edges"][-1] == np.nextafter(1.0, 2.0) and s["fields"] == {}
    s = S("who", N, xh=ones, velocity=2 * ones, velocity_scale=7.0, window=7, bins=[0.0, 0.5, 0.5, 1.0], into=3, into_what="tau", return_tau=True, **ok)
    assert (s["window"], s["velocity_scale"], s["into"], s["into_what"], s["return_tau"], s["return_flux"]) == (7, 7.0, 3, "tau", True, False)
    assert s["edges"].tolist() == [0.0, 0.5, 0.5, 1.0] and list(s["fields"]) == ["xh"]          # (no window of the mapping's: 14 cells are taken)
    assert S("who", N, device_velocity=True, velocity_scale=-2.0, **ok)["velocity_scale"] == -2.0
    # the entry: the same refusals with no library in reach, and before a device is asked for
    entry = _module().lyman_alpha_forest
    with pytest.raises(ValueError, match="lyman_alpha_forest: los_axis must be 0, 1 or 2"):
        entry(np.zeros((4, 4, 4)), los_axis=5, **ok)
    with pytest.raises(ValueError, match="lyman_alpha_forest: b_scale must be"):
        entry(b_scale=-1.0, tau_scale=1.0)
    with pytest.raises(TypeError):
        entry()                                                     # (the two scale factors have no default)


def test_result_class():
    from pyc2ray_amd import LymanAlphaForest, _capi
    N = 8
    a = LB.answer(N, edges=np.linspace(0, 1, 5))
    f = LymanAlphaForest(N, 1, a["stats"], a["counts"], a["gaps"], pdf=a["pdf"], bin_edges=np.linspace(0, 1, 5), gap_threshold=0.1, velocity=True)
    assert f.mean_flux == 0.5 and f.tau_eff == math.log(2.0) and f.flux_variance == pytest.approx(1.0 / 3.0 - 0.25)
    assert (f.tau_min, f.tau_max, f.window, f.clipped, f.degenerate, f.nonfinite) == (0.25, 8.0, 3, 5, 2, 0)
    assert (f.n_gaps, f.longest_gap, f.full_lines, f.dark_fraction) == (2, 6, 0, 8 / 512)
    assert f.gap_counts.dtype == np.uint64 and f.gap_lengths_cells.tolist() == [2, 6] and f.pdf.tolist() == [128] * 4
    lengths, counts = f.gap_lengths(12.5)
    assert lengths.tolist() == [25.0, 75.0] and counts.tolist() == [1, 1]
    with pytest.raises(ValueError, match="dv must be a finite number > 0"):
        f.gap_lengths(0.0)
    line = f.log_line()
    assert line.startswith("Lyman-alpha forest (line of sight 1, with peculiar velocities, W = 3): mean flux 5.000000e-01, tau_eff 6.931472e-01, ")
    assert "2 dark gaps (F < 0.1), longest 6 cells, dark fraction 0.015625, 0 lines wholly dark; clipped 5; degenerate 2" in line
    assert "nonfinite" not in line and repr(f) == f"<LymanAlphaForest: {line}>"
    dark = LymanAlphaForest(N, 2, [0.0, 0.0, 30.0, 40.0], np.zeros(_capi.LYA_COUNTS), np.zeros(N + 1))
    assert dark.tau_eff == math.inf and dark.pdf is None and dark.bin_edges is None and "no velocity" in dark.log_line()
    with pytest.raises(ValueError, match="N \\+ 1 = 9 gap counts"):
        LymanAlphaForest(N, 2, a["stats"], a["counts"], np.zeros(N))
    with pytest.raises(ValueError, match="pdf and bin_edges go together"):
        LymanAlphaForest(N, 2, a["stats"], a["counts"], a["gaps"], pdf=a["pdf"])
    with pytest.raises(ValueError, match="4 bins go with 5 edges, not 4"):
        LymanAlphaForest(N, 2, a["stats"], a["counts"], a["gaps"], pdf=a["pdf"], bin_edges=[0, 1, 2, 3])


class _Holder:
    left = 0

    def _leave_device(self):
        self.left += 1


def test_the_forms_of_the_modules_calls(monkeypatch):
    import pyc2ray_amd as pc2r
    from pyc2ray_amd import _capi, _residency
    M = _module()
    assert pc2r.lyman_alpha_forest is M.lyman_alpha_forest and pc2r.LymanAlphaForest is M.LymanAlphaForest and pc2r.lyman_alpha is M
    N = 8
    rng = np.random.default_rng(3)
    x, n, T, v = rng.random((N, N, N)), rng.random((N, N, N)), 1e4 * rng.random((N, N, N)), np.full((N, N, N), 0.25)
    monkeypatch.setattr(M, "cuda_is_init", lambda: False)
    monkeypatch.setattr(M, "load_asora", lambda: SB.Untouchable())
    with pytest.raises(RuntimeError, match="GPU not initialized"):
        M.lyman_alpha_forest(x, b_scale=0.01, tau_scale=1.0)
    lib = _install(monkeypatch, LB.Counting(N))
    holder = _Holder()
    _residency.register(holder)
    f = M.lyman_alpha_forest(x, n, T, velocity=v, velocity_scale=2.0, b_scale=0.01, tau_scale=3.0, los_axis=0, window=2, gap_threshold=0.2, bins=4,
                             return_flux=True)
    assert lib.names() == ["grid_to_device"] * 3 + ["los_velocity_to_device", "lyman_alpha_forest"] and holder.left == 2
    for call, which, grid in zip(lib.calls, (_capi.GRID_XH, _capi.GRID_NDENS, _capi.GRID_TEMP), (x, n, T)):
        assert call[1][0] == which and np.array_equal(call[1][1], grid)
    assert np.array_equal(lib.calls[3][1][0], v)
    call = lib.calls[4]
    assert call[1] == (0, 2.0, 0.01, 3.0) and call[2]["window"] == 2 and call[2]["gap_threshold"] == 0.2 and call[2]["edges"].size == 5
    assert {k: call[2][k] for k in ("dst_grid", "dst_what", "tau", "flux")} == {"dst_grid": None, "dst_what": _capi.LYA_FLUX, "tau": False, "flux": True}
    assert (f.N, f.los_axis, f.velocity, f.gap_threshold, f.window) == (N, 0, True, 0.2, 3) and f.flux.shape == (N, N, N) and f.tau is None
    assert f.pdf.tolist() == [128] * 4 and f.bin_edges.size == 5
    # the device grids where they lie: nothing is uploaded, nobody is asked to leave
    lib.calls.clear()
    f = M.lyman_alpha_forest(b_scale=0.01, tau_scale=3.0)
    assert lib.names() == ["lyman_alpha_forest"] and lib.calls[0][1] == (2, None, 0.01, 3.0) and lib.calls[0][2]["window"] == 0 and holder.left == 2
    assert not f.velocity and f.pdf.size == 20
    # into: a grid is about to be overwritten, so whoever keeps data on the device takes it home first
    lib.calls.clear()
    f = M.lyman_alpha_forest(temp=T, b_scale=0.01, tau_scale=3.0, into=_capi.GRID_XH_AV, into_what="tau", return_tau=True)
    assert lib.names() == ["grid_to_device", "lyman_alpha_forest"] and lib.calls[0][1][0] == _capi.GRID_TEMP and holder.left == 3
    assert lib.calls[1][2]["dst_grid"] == _capi.GRID_XH_AV and lib.calls[1][2]["dst_what"] == _capi.LYA_TAU and f.tau.shape == (N, N, N)
    lib.calls.clear()
    M.lyman_alpha_forest(b_scale=0.01, tau_scale=3.0, into=_capi.GRID_XH_AV)
    assert lib.names() == ["lyman_alpha_forest"] and holder.left == 4
    # a host array of another mesh than the device's
    with pytest.raises(ValueError, match="xh must have the shape \\(8, 8, 8\\)"):
        M.lyman_alpha_forest(np.ones((4, 4, 4)), b_scale=0.01, tau_scale=3.0)


def test_yaml_keys_the_scale_factors_and_the_forms_the_class_takes(tmp_path, monkeypatch):
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.c2ray_base as B
    from pyc2ray_amd import _capi
    # the two pinned tuples are as they were; the third holds the new name, and one helper walks all three
    assert B.C2Ray._STEP_STATISTICS == ("photon_budget", "bubble_stats", "region_stats", "topology_stats", "granulometry_stats",
                                        "power_spectrum_stats", "observed_stats")
    assert B.C2Ray._STEP_STATISTICS_APPENDED == ("redshift_space_stats",) and B.C2Ray._STEP_STATISTICS_FURTHER == ("lyman_alpha_stats",)
    assert B.C2Ray._step_statistics() == B.C2Ray._STEP_STATISTICS + ("redshift_space_stats", "lyman_alpha_stats")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 8
        plain = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        assert plain.lyman_alpha_stats is False and plain.last_lyman_alpha is None
        with pytest.raises(ValueError, match="C2Ray.lyman_alpha_stats: lyman_alpha_stats needs use_gpu=True"):
            plain.lyman_alpha_stats = True
        with pytest.raises(ValueError, match="lyman_alpha_stats must be a bool"):
            plain.lyman_alpha_stats = 1
        body = open(PLAIN_PARAMS).read()
        key = lambda text: body.replace("  logfile: pyC2Ray.log\n", f"  logfile: pyC2Ray.log\n{text}")
        for text, what in (("  lyman_alpha: 2\n", "Output: lyman_alpha must be 0 or 1"),
                           ("  lyman_alpha: 1\n", "Output: lyman_alpha: 1: lyman_alpha_stats needs use_gpu=True"),
                           ("  lyman_alpha_gap_threshold: .nan\n", "gap_threshold must be a finite number"),
                           ("  lyman_alpha_bins: 0\n", "bins as an int must be in"),
                           ("  lyman_alpha_bins: [0.5, 0.2]\n", "the edges of bins must be finite and non-decreasing")):
            with open("p.yml", "w") as f:
                f.write(key(text))
            with pytest.raises(ValueError, match=what):
                pc2r.C2Ray_Test("p.yml", N, False)
        with pytest.raises(ValueError, match="Output: lyman_alpha: 1: lyman_alpha_stats needs use_gpu=True"):
            pc2r.C2Ray_Test(LYA_PARAMS, N, False)
        # an object with use_gpu (as one constructed with use_gpu=True has it) reading its keys
        sim = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        sim.gpu = True
        sim._read_paramfile(LYA_PARAMS)
        sim._statistic_init("lyman_alpha_stats")
        assert sim.lyman_alpha_stats is True and sim.last_lyman_alpha is None
        assert B.C2Ray.lyman_alpha_stats.defaults(sim) == {"gap_threshold": 0.1, "bins": 8}
        # the scale factors against hand-computed values: sqrt(2 k_B / m_p) = 0.1284866 km/s per sqrt(K); I_alpha = pi e^2 f lambda /
        # (m_e c) = 1.34348e-7 cm^3 / s
        cs = sim._ld["Cosmology"]
        z = sim.zred
        assert sim.lyman_alpha_b_scale() / sim.velocity_scale() == pytest.approx(0.1284866, rel=2e-6)
        hubble = 100 * cs["h"] * math.sqrt(cs["Omega0"] * (1 + z) ** 3 + 1 - cs["Omega0"]) * 1.0e5 / 3.086e24      # 1/s (radiation: below 1e-2 at this z)
        assert sim.lyman_alpha_tau_scale() * hubble == pytest.approx(1.34348e-7, rel=1e-2)
        assert sim.lyman_alpha_tau_scale() * (100 * cs["h"] * float(sim.cosmology.efunc(z)) * 1.0e5 / B.Mpc) == pytest.approx(1.34348e-7, rel=2e-6)
        lib = _install(monkeypatch, LB.Counting(N))
        steps = []
        monkeypatch.setattr(B, "evolve3D_resident", lambda *a, **kw: steps.append("evolve3D_resident"))
        flux, pos = np.ones(1), np.ones((3, 1), dtype=int)
        sim.device_resident = True
        # no velocity: the gas at rest, and the line says so
        sim.evolve3D(2.0, flux, pos)
        assert steps == ["evolve3D_resident"] and lib.names() == ["lyman_alpha_forest"]
        call = lib.calls[0]
        assert call[1] == (2, None, sim.lyman_alpha_b_scale(), sim.lyman_alpha_tau_scale())
        assert call[2]["window"] == 0 and call[2]["gap_threshold"] == 0.1 and call[2]["edges"].size == 9 and call[2]["dst_grid"] is None
        first = sim.last_lyman_alpha
        assert (first.N, first.los_axis, first.velocity, first.gap_threshold) == (N, 2, False, 0.1) and first.pdf.size == 8
        assert sim._device_newer >= {"xh", "phi_ion"} and "xh" not in sim._host_newer
        # a velocity: uploaded once per assignment, not per step, and shared with the redshift-space calls
        v = np.full((N, N, N), 1.0)
        sim.los_velocity = v
        sim.los_axis = 0
        lib.calls.clear()
        sim.evolve3D(2.0, flux, pos)
        sim.evolve3D(2.0, flux, pos)
        assert lib.names() == ["los_velocity_to_device", "lyman_alpha_forest", "lyman_alpha_forest"]
        assert lib.calls[1][1] == (0, sim.velocity_scale(), sim.lyman_alpha_b_scale(), sim.lyman_alpha_tau_scale()) and sim.last_lyman_alpha.velocity
        log = open(sim.logfile).read()
        assert log.count("Lyman-alpha forest (line of sight 2, no velocity, W = 3): mean flux 5.000000e-01, ") == 1
        assert log.count("Lyman-alpha forest (line of sight 0, with peculiar velocities, W = 3): mean flux 5.000000e-01, ") == 2
        # a direct call: keywords over the keys; into uploads the object's grids afresh
        lib.calls.clear()
        f = sim.lyman_alpha_forest(window=2, bins=[0.0, 0.5, 1.0], b_scale=0.5, into=_capi.GRID_XH_AV, into_what="tau", return_tau=True)
        # (reclaimed: the object's device copies come down first, then every grid and the velocity go up again)
        assert lib.names()[-5:] == ["grid_to_device"] * 3 + ["los_velocity_to_device", "lyman_alpha_forest"]
        assert "grid_to_host" in lib.names()[:-5] and "grid_to_device" not in lib.names()[:-5]
        assert lib.calls[-1][1][2] == 0.5 and lib.calls[-1][2]["window"] == 2 and lib.calls[-1][2]["dst_what"] == _capi.LYA_TAU
        assert f.pdf.size == 2 and f.tau.shape == (N, N, N) and sim.last_lyman_alpha is not f
        for name in ("xh", "ndens", "temp", "velocity", "device_velocity"):
            with pytest.raises(ValueError, match=f"C2Ray.lyman_alpha_forest: {name} is not for the class"):
                sim.lyman_alpha_forest(**{name: None})
        lib.calls.clear()
        with pytest.raises(ValueError, match="C2Ray.lyman_alpha_forest: .*wider than the N = 8 cells of a line"):
            sim.lyman_alpha_forest(window=4)
        assert lib.calls == []
        # off: a step makes no library call of the feature's, and leaves the last result alone
        kept = sim.last_lyman_alpha
        sim.lyman_alpha_stats = False
        before = open(sim.logfile).read()
        sim.evolve3D(1.0, flux, pos)
        assert lib.calls == [] and sim.last_lyman_alpha is kept and open(sim.logfile).read() == before
    finally:
        os.chdir(cwd)
        if "sim" in locals():      # (nothing of this object lives on a device: a later step elsewhere must not ask it to fetch)
            sim._device_newer.clear()
            sim.device_resident = False
