"""CPU: the host side of the connected regions: the C-ABI symbol, RegionSizes' arithmetic, the argument
checks of region_sizes (before the library is touched), the YAML keys and attributes of the class, and which form of the call the
class takes (on a stand-in for the library)."""
import math
import os

import numpy as np
import pytest

import lls_standin_backend as SB
import regions_standin_backend as RB

HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_test.yml")
REGION_PARAMS = os.path.join(HERE, "data", "parameters_regions.yml")


@pytest.fixture(scope="module", autouse=True)
def no_leftover_device():
    """On a machine with a GPU an earlier test of the suite may have left the library initialised behind the package's back (the
    CPU-path cases of tests/test_integration_stubs.py do: c2ray_do_all_sources sets the device up on its own and nobody closes it).
    The code-2 check below needs a library without a device, so such a leftover is closed first; a device the package itself
    holds is left alone."""
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    lib = _capi.load()
    if lib.asora_device_ptr(_capi.GRID_NDENS) and not p.cuda_is_init():
        assert lib.asora_device_close() == 0
    yield


def _install(monkeypatch, backend, ready=True):
    import pyc2ray_amd.c2ray_base as B
    import pyc2ray_amd.regions as M
    for mod in (M, B):
        monkeypatch.setattr(mod, "load_asora", lambda: backend)
        monkeypatch.setattr(mod, "cuda_is_init", lambda: ready)
    return backend


def test_capi_symbol_and_header():
    from pyc2ray_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "asora_hip.h")).read()
    assert ("int asora_region_sizes(int which_grid, double threshold, int phase, int periodic, int connectivity, int n_bins, "
            "const double *edges,\n                       unsigned long long *counts, unsigned long long *cells, unsigned long long "
            "*tallies, uint32_t *labels);") in header
    # no selector, option or grid is added
    assert "ASORA_KERNEL_BUBBLE_RAYS = 6, ASORA_KERNEL_SLOTS = 7" in header and "ASORA_OPT_COUNT = 19" in header
    assert "ASORA_GRID_COUNT = 9" in header
    order = ("N_PHASE", "N_REGIONS", "SUM_V2", "V_LARGEST", "LABEL_LARGEST", "EXTENT_I", "EXTENT_J", "EXTENT_K", "V_SECOND", "LABEL_SECOND",
             "UNDERFLOW", "UNDERFLOW_CELLS", "OVERFLOW", "OVERFLOW_CELLS")
    for n, name in enumerate(order):
        assert f"ASORA_REGION_{name} = {n}," in header and getattr(_capi, f"REGION_{name}") == n
    assert "ASORA_REGION_TALLIES = 14" in header and _capi.REGION_TALLIES == 14
    assert "ASORA_REGION_MAX_N = 645" in header and _capi.REGION_MAX_N == 645 and 645 ** 3 < 2 ** 32 and 8 * 645 ** 3 <= 2 ** 31 < 8 * 646 ** 3
    assert len(_capi.SIGNATURES["asora_region_sizes"][1]) == 11
    lib = _capi.load()                    # (opening the library resolves every declared symbol)
    if not lib.asora_device_ptr(_capi.GRID_NDENS):      # no device initialised in this process: refused as every entry is
        out = np.full(14, 9, dtype=np.uint64)
        labels = np.full(8, 9, dtype=np.uint32)
        e = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
        u64 = lambda a: a.ctypes.data_as(_capi._u64p)
        import ctypes as C
        rc = lib.asora_region_sizes(_capi.GRID_XH, 0.5, 0, 1, 6, 4, _capi.dptr(e), u64(out), u64(out), u64(out),
                                    labels.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert rc == 2 and b"region_sizes" in lib.asora_last_error() and b"not initialised" in lib.asora_last_error()
        assert np.all(out == 9) and np.all(labels == 9)                 # (a refused call writes nothing)


def test_region_sizes_arithmetic():
    from pyc2ray_amd.regions import RegionSizes
    edges = np.array([1.0, 2.0, 8.0, 512.0])
    N = 8
    label = (3 * N + 4) * N + 5
    r = RegionSizes(edges, [4, 3, 1], [4, 16, 300], [400, 10, 90_300, 300, label, 8, 5, 7, 40, 9, 0, 0, 2, 80], N, threshold=0.3,
                    phase="neutral", connectivity=26, periodic=False, dr=2.0)
    assert (r.n_phase, r.n_regions, r.sum_v2, r.v_largest, r.label_largest, r.v_second, r.label_second) == (400, 10, 90_300, 300, label, 40, 9)
    assert (r.underflow, r.underflow_cells, r.overflow, r.overflow_cells) == (0, 0, 2, 80)
    assert r.counts.dtype == r.cells.dtype == np.uint64
    assert r.extent == (8, 5, 7) and r.largest_index == (3, 4, 5) and r.percolates is True
    assert r.fraction_largest == 0.75 and r.mean_volume == 40.0 and r.weighted_mean_volume == 225.75
    assert np.array_equal(r.volume_fraction, [0.01, 0.04, 0.75])
    assert np.allclose(r.radius_edges, (3 * edges / (4 * math.pi)) ** (1 / 3), rtol=1e-15)
    assert np.array_equal(r.edges_phys, 8.0 * edges) and np.array_equal(r.radius_edges_phys, 2.0 * r.radius_edges)
    assert (r.v_largest_phys, r.v_second_phys, r.mean_volume_phys, r.weighted_mean_volume_phys) == (2400.0, 320.0, 320.0, 1806.0)
    assert r.labels is None
    line = r.log_line()
    assert line.startswith("Regions (neutral, x < 0.3, 26 neighbours, open): 10 regions in 400 cells, largest 300 cells") and "\n" not in line
    assert "extent 8 x 5 x 7 of 8, percolates" in line and "in units of dr^3" in line
    short = RegionSizes(edges, [4, 3, 1], [4, 16, 300], [400, 10, 90_300, 300, label, 7, 5, 7, 40, 9, 0, 0, 2, 80], N)
    assert short.percolates is False and "does not percolate" in short.log_line() and short.v_largest_phys is None
    assert short.edges_phys is None and short.radius_edges_phys is None and "in units of dr^3" not in short.log_line()
    # the tie rule's fields: equal volumes, the smaller label the largest
    tie = RegionSizes(edges, [0, 0, 2], [0, 0, 54], [54, 2, 1458, 27, 73, 3, 3, 3, 27, 300, 0, 0, 0, 0], N)
    assert tie.v_largest == tie.v_second and tie.label_largest < tie.label_second and tie.largest_index == (1, 1, 1)
    empty = RegionSizes(edges, [0, 0, 0], [0, 0, 0], [0, 0, 0, 0, 0xFFFFFFFF, 0, 0, 0, 0, 0xFFFFFFFF, 0, 0, 0, 0], N)
    assert empty.fraction_largest == empty.mean_volume == empty.weighted_mean_volume == 0.0 and not empty.volume_fraction.any()
    assert empty.percolates is False and empty.largest_index is None and empty.extent == (0, 0, 0) and "\n" not in empty.log_line()
    with pytest.raises(ValueError, match="one count and one cell sum per bin"):
        RegionSizes(edges, [1, 2], [1, 2, 3], [0] * 14, N)
    with pytest.raises(ValueError, match="14 tallies"):
        RegionSizes(edges, [1, 2, 3], [1, 2, 3], [0] * 6, N)


def test_bad_arguments_are_refused_before_the_library_is_touched(monkeypatch):
    from pyc2ray_amd.regions import region_sizes
    _install(monkeypatch, SB.Untouchable())
    f = np.zeros((8, 8, 8))
    for kw, what in ((dict(threshold=np.nan), "threshold must be a finite number"), (dict(threshold="0.5"), "threshold must be"),
                     (dict(threshold=True), "threshold must be"), (dict(phase="ionized"), "phase must be 'ionised' or 'neutral'"),
                     (dict(phase=0), "phase must be"), (dict(connectivity=18), "connectivity must be 6"), (dict(connectivity=6.0), "connectivity must be"),
                     (dict(connectivity="6"), "connectivity must be"), (dict(connectivity=True), "connectivity must be"),
                     (dict(bins=12), "a number of bins has no natural upper edge"), (dict(bins=True), "a number of bins"),
                     (dict(bins="many"), "bins must be"), (dict(bins=[1.0]), "1-D array of 2 ... 257 values"), (dict(bins=np.ones((2, 2))), "1-D array"),
                     (dict(bins=[1.0, 1.0, 2.0]), "finite, > 0 and ascending"), (dict(bins=[0.0, 1.0]), "finite, > 0 and ascending"),
                     (dict(bins=[1.0, np.nan]), "finite, > 0 and ascending"), (dict(bins=np.geomspace(1, 9, 258)), "2 ... 257 values"),
                     (dict(periodic=1), "periodic must be a bool"), (dict(dr=0.0), "dr must be None or a finite number > 0"),
                     (dict(dr=np.nan), "dr must be"), (dict(labels=1), "labels must be a bool"),
                     (dict(grid=4), "grid selects a device grid and goes with field=None")):
        with pytest.raises(ValueError, match=f"region_sizes: .*{what}"):
            region_sizes(f, **kw)
        if "grid" not in kw:
            with pytest.raises(ValueError, match=f"region_sizes: .*{what}"):
                region_sizes(None, **kw)
    for bad in (np.zeros((8, 8)), np.zeros((8, 8, 4)), np.zeros((4, 4, 4), dtype=complex), [["a"]]):
        with pytest.raises(ValueError, match="field must be a real"):
            region_sizes(bad)
    for bad in (-1, 9, 1.0, "xh", True):
        with pytest.raises(ValueError, match="grid must be one of"):
            region_sizes(None, grid=bad)
    _install(monkeypatch, SB.Untouchable(), ready=False)
    with pytest.raises(RuntimeError, match="GPU not initialized"):
        region_sizes(f)


def test_the_two_forms_of_the_module_entry(monkeypatch):
    from pyc2ray_amd import _capi
    from pyc2ray_amd.regions import region_sizes, region_spec
    lib = _install(monkeypatch, RB.Labelling(8))
    f = np.random.default_rng(0).random((8, 8, 8))
    r = region_sizes(f, threshold=0.25, phase="neutral", connectivity=26, periodic=False, dr=3.0)
    assert lib.names() == ["grid_to_device", "region_sizes"]
    up, call = lib.calls
    assert up[1][0] == _capi.GRID_XH and np.array_equal(up[1][1], f)
    assert call[1][:5] == (_capi.GRID_XH, 0.25, 1, False, 26) and call[2] == {}
    # powers of two: floor(log2(8^3)) + 1 = 10 bins, so that 512 itself is in one
    assert np.array_equal(call[1][5], 2.0 ** np.arange(11)) and r.counts.size == 10
    assert np.array_equal(r.counts, RB.bins_for(10)[0]) and np.array_equal(r.cells, RB.bins_for(10)[1])
    assert (r.n_phase, r.n_regions, r.v_largest, r.label_largest, r.extent, r.dr, r.N) == (400, 12, 300, 73, (8, 5, 7), 3.0, 8)
    assert (r.phase, r.threshold, r.connectivity, r.periodic, r.labels, r.percolates) == ("neutral", 0.25, 26, False, None, True)
    lib.calls.clear()
    r = region_sizes(None, grid=_capi.GRID_XH_AV, bins=[1.0, 2.0, 3.0], labels=True)      # the device grid where it lies
    assert lib.names() == ["region_sizes"]
    assert lib.calls[0][1][:5] == (_capi.GRID_XH_AV, 0.5, 0, True, 6) and np.array_equal(lib.calls[0][1][5], [1.0, 2.0, 3.0])
    assert lib.calls[0][2] == {"labels": True} and r.labels.shape == (8, 8, 8) and r.labels.dtype == np.uint32
    lib.calls.clear()
    assert region_sizes(None).edges.size == 11 and lib.calls[0][1][0] == _capi.GRID_XH
    for N, nb in ((1, 1), (2, 4), (17, 13), (64, 19), (70, 19), (256, 25), (645, 28)):
        e = region_spec("x", N)["edges"]
        assert e.size == nb + 1 == math.floor(math.log2(N ** 3)) + 2 and e[0] == 1.0 and e[-2] <= N ** 3 < e[-1]
    with pytest.raises(ValueError, match="1 ... 645 cells a side"):
        region_spec("x", 646)


def test_yaml_keys_the_attribute_and_the_forms_the_class_takes(tmp_path, monkeypatch):
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.c2ray_base as B
    from pyc2ray_amd import _capi
    assert pc2r.region_sizes is pc2r.regions.region_sizes and pc2r.RegionSizes is pc2r.regions.RegionSizes
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 8
        plain = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        assert plain.region_stats is False and plain.last_regions is None
        with pytest.raises(ValueError, match="C2Ray.region_stats: region_stats needs use_gpu=True"):
            plain.region_stats = True
        plain.region_stats = False
        for bad in (1, 0, None, "on", 1.0):
            with pytest.raises(ValueError, match="region_stats must be a bool"):
                plain.region_stats = bad
        body = open(PLAIN_PARAMS).read()
        key = lambda text: body.replace("  logfile: pyC2Ray.log\n", f"  logfile: pyC2Ray.log\n{text}")
        assert key("x") != body
        for text, what in (("  region_sizes: 2\n", "Output: region_sizes must be 0 or 1"), ("  region_sizes: 'yes'\n", "must be 0 or 1"),
                           ("  region_sizes: 1.0\n", "must be 0 or 1"),
                           ("  region_sizes: 1\n", "Output: region_sizes: 1: region_stats needs use_gpu=True"),
                           ("  region_threshold: .nan\n", "threshold must be a finite number"), ("  region_threshold: half\n", "threshold must be"),
                           ("  region_connectivity: 18\n", "connectivity must be 6"), ("  region_connectivity: 6.0\n", "connectivity must be")):
            with open("p.yml", "w") as f:
                f.write(key(text))
            with pytest.raises(ValueError, match=what):
                pc2r.C2Ray_Test("p.yml", N, False)
        with open("p.yml", "w") as f:
            f.write(key("  region_sizes: 0\n  region_connectivity: 26\n"))
        assert pc2r.C2Ray_Test("p.yml", N, False).region_stats is False
        # the committed parameter file is refused without use_gpu, as the key says
        with pytest.raises(ValueError, match="Output: region_sizes: 1: region_stats needs use_gpu=True"):
            pc2r.C2Ray_Test(REGION_PARAMS, N, False)
        # an object with use_gpu (as one constructed with use_gpu=True has it) reading its keys
        sim = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        sim.gpu = True
        sim._read_paramfile(REGION_PARAMS)
        sim._statistic_init("region_stats")
        assert sim.region_stats is True and sim.last_regions is None
        lib = _install(monkeypatch, RB.Labelling(N))
        steps = []
        monkeypatch.setattr(B, "evolve3D", lambda *a, **kw: steps.append("evolve3D") or (np.full((N, N, N), 0.75), np.zeros((N, N, N))))
        monkeypatch.setattr(B, "evolve3D_resident", lambda *a, **kw: steps.append("evolve3D_resident"))
        flux, pos = np.ones(1), np.ones((3, 1), dtype=int)
        # the resident path: the device grid where it lies -- no upload, no download, the bookkeeping untouched
        sim.device_resident = True
        sim.evolve3D(2.0, flux, pos)
        assert steps == ["evolve3D_resident"] and lib.names() == ["region_sizes"]
        args = lib.calls[0][1]
        assert args[:5] == (_capi.GRID_XH, 0.4, 0, True, 26) and args[5].size == 11 and lib.calls[0][2] == {}
        first = sim.last_regions
        assert (first.n_regions, first.dr, first.periodic, first.connectivity, first.threshold) == (12, sim.dr, True, 26, 0.4)
        assert sim._device_newer >= {"xh", "phi_ion"} and "xh" not in sim._host_newer
        lib.calls.clear()
        r = sim.regions(connectivity=6, phase="neutral", bins=[1.0, 4.0], dr=None, periodic=False)      # keywords override keys and defaults
        assert lib.names() == ["region_sizes"] and lib.calls[0][1][:5] == (_capi.GRID_XH, 0.4, 1, False, 6)
        assert r.dr is None and r is not sim.last_regions and sim.last_regions is first
        assert sim._device_newer >= {"xh", "phi_ion"} and "xh" not in sim._host_newer
        for name in ("field", "grid"):
            with pytest.raises(ValueError, match=f"C2Ray.regions: {name} is not for the class"):
                sim.regions(**{name: None})
        with pytest.raises(ValueError, match="C2Ray.regions: connectivity must be"):
            sim.regions(connectivity=8)
        # otherwise: the host array goes up first
        lib.calls.clear()
        sim._device_newer.clear()
        sim.device_resident = False
        sim.evolve3D(3.0, flux, pos)
        assert steps[-1] == "evolve3D" and lib.names() == ["grid_to_device", "region_sizes"]
        assert lib.calls[0][1][0] == _capi.GRID_XH and np.all(lib.calls[0][1][1] == 0.75) and lib.calls[1][1][4] == 26
        assert sim.last_regions is not first
        assert open(sim.logfile).read().count("Regions (ionised, x >= 0.4, 26 neighbours, periodic): 12 regions in 400 cells") == 2
        # off: a step makes no library call of the feature's, and leaves the last result alone
        kept = sim.last_regions
        sim.region_stats = False
        for resident in (True, False):
            lib.calls.clear()
            sim._device_newer.clear()
            sim.device_resident = resident
            sim.evolve3D(1.0, flux, pos)
            assert lib.calls == [] and sim.last_regions is kept
        assert open(sim.logfile).read().count("Regions (") == 2
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
    assert lib.names() and not [n for n in lib.names() if "region" in n]
