"""CPU: the host side of the bubble-size distribution: the C-ABI symbols, BubbleSizes' arithmetic, the
argument checks of mfp_distribution (before the library is touched), the YAML keys and attributes of the class, and which form of
the call the class takes (on a stand-in for the library)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import bubble_standin_backend as BB
import lls_standin_backend as SB

HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_test.yml")


def _install(monkeypatch, backend, ready=True):
    import pyc2ray_amd.bubbles as M
    import pyc2ray_amd.c2ray_base as B
    for mod in (M, B):
        monkeypatch.setattr(mod, "load_asora", lambda: backend)
        monkeypatch.setattr(mod, "cuda_is_init", lambda: ready)
    return backend


def test_capi_symbols_and_header():
    from pyc2ray_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "asora_hip.h")).read()
    assert ("int asora_bubble_mfp(int which_grid, double threshold, int phase, int periodic, unsigned long long seed, long long n_rays, "
            "double l_max,") in header
    assert "int asora_bubble_mask(int which_grid, double threshold, int phase, uint64_t *mask_words, uint32_t *row_counts);" in header
    # the new kernel selectors are appended: the first four keep their numbers
    assert "ASORA_KERNEL_FINISH = 3, ASORA_KERNEL_COUNT = 4" in header
    assert "ASORA_KERNEL_BUBBLE_MASK = 4, ASORA_KERNEL_BUBBLE_SCAN = 5, ASORA_KERNEL_BUBBLE_RAYS = 6, ASORA_KERNEL_SLOTS = 7" in header
    assert (_capi.KERNEL_FINISH, _capi.KERNEL_BUBBLE_MASK, _capi.KERNEL_BUBBLE_SCAN, _capi.KERNEL_BUBBLE_RAYS) == (3, 4, 5, 6)
    assert (_capi.BUBBLE_ENDED, _capi.BUBBLE_CAPPED, _capi.BUBBLE_LEFT_BOX, _capi.BUBBLE_MAX_BINS) == (0, 1, 2, 256)
    assert len(_capi.SIGNATURES["asora_bubble_mfp"][1]) == 16 and len(_capi.SIGNATURES["asora_bubble_mask"][1]) == 5
    lib = _capi.load()                    # (opening the library resolves every declared symbol)
    ms, n = C.c_double(-1.0), C.c_long(-1)
    assert lib.asora_kernel_time_ms(_capi.KERNEL_BUBBLE_RAYS, C.byref(ms), C.byref(n)) == 0 and (ms.value, n.value) == (0.0, 0)
    assert lib.asora_kernel_time_ms(7, C.byref(ms), C.byref(n)) == 3
    if not lib.asora_device_ptr(_capi.GRID_NDENS):      # no device initialised in this process: refused as every entry is
        counts = np.full(4, 9, dtype=np.uint64)
        e = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
        u64 = lambda a: a.ctypes.data_as(_capi._u64p)
        rc = lib.asora_bubble_mfp(_capi.GRID_XH, 0.5, 0, 1, 0, 10, 8.0, 4, _capi.dptr(e), u64(counts), u64(counts), _capi.dptr(e),
                                  None, None, None, None)
        assert rc == 2 and b"bubble_mfp" in lib.asora_last_error() and b"not initialised" in lib.asora_last_error()
        assert lib.asora_bubble_mask(_capi.GRID_XH, 0.5, 0, None, None) == 2 and b"bubble_mask" in lib.asora_last_error()
        assert np.all(counts == 9)                      # (a refused call writes nothing)


def test_bubble_sizes_arithmetic():
    from pyc2ray_amd.bubbles import BubbleSizes
    edges = np.array([1.0, 2.0, 4.0, 16.0])
    b = BubbleSizes(edges, [10, 30, 20], [64, 5, 1, 3, 1, 1000], [256.0, 1600.0], 70, threshold=0.3, phase="neutral", seed=9, l_max=32.0,
                    periodic=False, dr=2.5)
    assert (b.ended, b.capped, b.left_box, b.underflow, b.overflow, b.n_phase, b.n_rays) == (64, 5, 1, 3, 1, 1000, 70)
    assert b.counts.dtype == np.uint64 and b.fraction_capped == 5 / 70
    assert b.mean == 4.0 and b.rms == 5.0 and b.mean_phys == 10.0 and b.rms_phys == 12.5
    assert np.array_equal(b.centres, [math.sqrt(2.0), math.sqrt(8.0), 8.0]) and np.array_equal(b.centres_phys, 2.5 * b.centres)
    assert np.array_equal(b.edges_phys, 2.5 * edges)
    dln = np.log([2.0, 2.0, 4.0])
    assert np.allclose(b.RdPdR, np.array([10, 30, 20]) / (60 * dln), rtol=1e-15) and np.sum(b.RdPdR * b.dlnR) == pytest.approx(1.0, rel=1e-15)
    assert b.peak_radius == math.sqrt(8.0) and b.peak_radius_phys == 2.5 * math.sqrt(8.0)
    line = b.log_line()
    assert line.startswith("Bubble sizes (neutral, x < 0.3): 70 rays from 1000 cells, mean 4.0000, rms 5.0000") and "\n" not in line
    cells = BubbleSizes(edges, [0, 0, 0], [0, 0, 0, 0, 0, 0], [0.0, 0.0], 0)
    assert cells.mean == cells.rms == cells.fraction_capped == cells.peak_radius == 0.0 and not cells.RdPdR.any()
    assert cells.mean_phys is None and cells.centres_phys is None and "in units of dr" not in cells.log_line()
    with pytest.raises(ValueError, match="one count per bin"):
        BubbleSizes(edges, [1, 2], [0] * 6, [0.0, 0.0], 0)


def test_bad_arguments_are_refused_before_the_library_is_touched(monkeypatch):
    from pyc2ray_amd.bubbles import mfp_distribution
    _install(monkeypatch, SB.Untouchable())
    f = np.zeros((8, 8, 8))
    for kw, what in ((dict(threshold=np.nan), "threshold must be a finite number"), (dict(threshold="0.5"), "threshold must be"),
                     (dict(threshold=True), "threshold must be"), (dict(phase="ionized"), "phase must be 'ionised' or 'neutral'"),
                     (dict(phase=0), "phase must be"), (dict(n_rays=-1), "n_rays must be an integer >= 0"), (dict(n_rays=1e5), "n_rays must be"),
                     (dict(seed=-1), "seed must be an integer in"), (dict(seed=2 ** 64), "seed must be"), (dict(seed=1.0), "seed must be"),
                     (dict(l_max=0.0), "l_max must be"), (dict(l_max=np.inf), "l_max must be"), (dict(l_max=0.25), "needs l_max > 0.5"),
                     (dict(bins=0), "bins must be 1 ... 256"), (dict(bins=257), "bins must be 1 ... 256"), (dict(bins="many"), "bins must be"),
                     (dict(bins=[1.0]), "1-D array of 2 ... 257 values"), (dict(bins=np.ones((2, 2))), "1-D array"),
                     (dict(bins=[1.0, 1.0, 2.0]), "finite, > 0 and ascending"), (dict(bins=[0.0, 1.0]), "finite, > 0 and ascending"),
                     (dict(bins=[1.0, np.nan]), "finite, > 0 and ascending"), (dict(bins=np.geomspace(1, 9, 258)), "2 ... 257 values"),
                     (dict(periodic=1), "periodic must be a bool"), (dict(dr=0.0), "dr must be None or a finite number > 0"),
                     (dict(dr=np.nan), "dr must be"), (dict(grid=4), "grid selects a device grid and goes with field=None")):
        with pytest.raises(ValueError, match=f"mfp_distribution: .*{what}"):
            mfp_distribution(f, **kw)
        if "grid" not in kw:
            with pytest.raises(ValueError, match=f"mfp_distribution: .*{what}"):
                mfp_distribution(None, **kw)
    for bad in (np.zeros((8, 8)), np.zeros((8, 8, 4)), np.zeros((4, 4, 4), dtype=complex), [["a"]]):
        with pytest.raises(ValueError, match="field must be a real"):
            mfp_distribution(bad)
    for bad in (-1, 9, 1.0, "xh", True):
        with pytest.raises(ValueError, match="grid must be one of"):
            mfp_distribution(None, grid=bad)
    _install(monkeypatch, SB.Untouchable(), ready=False)
    with pytest.raises(RuntimeError, match="GPU not initialized"):
        mfp_distribution(f)


def test_the_two_forms_of_the_module_entry(monkeypatch):
    from pyc2ray_amd import _capi
    from pyc2ray_amd.bubbles import mfp_distribution
    lib = _install(monkeypatch, BB.Bubbling(8))
    f = np.random.default_rng(0).random((8, 8, 8))
    b = mfp_distribution(f, threshold=0.25, phase="neutral", n_rays=100, seed=4, bins=5, periodic=False, dr=3.0)
    assert lib.names() == ["grid_to_device", "bubble_mfp"]
    up, call = lib.calls
    assert up[1][0] == _capi.GRID_XH and np.array_equal(up[1][1], f)
    assert call[1][:7] == (_capi.GRID_XH, 0.25, 1, False, 4, 100, 8.0) and np.array_equal(call[1][7], np.geomspace(0.5, 8.0, 6))
    assert np.array_equal(b.counts, BB.counts_for(5)) and (b.ended, b.n_phase, b.n_rays, b.dr) == (90, 4321, 100, 3.0)
    assert (b.mean, b.phase, b.threshold, b.seed, b.l_max, b.periodic) == (5.0, "neutral", 0.25, 4, 8.0, False)
    lib.calls.clear()
    b = mfp_distribution(None, grid=_capi.GRID_XH_AV, l_max=4.0, bins=[1.0, 2.0, 3.0])      # the device grid where it lies
    assert lib.names() == ["bubble_mfp"]
    assert lib.calls[0][1][:7] == (_capi.GRID_XH_AV, 0.5, 0, True, 0, 100_000, 4.0) and np.array_equal(lib.calls[0][1][7], [1.0, 2.0, 3.0])
    lib.calls.clear()
    assert mfp_distribution(None).l_max == 8.0 and lib.calls[0][1][0] == _capi.GRID_XH and lib.calls[0][1][7].size == 65


def test_yaml_keys_the_attribute_and_the_forms_the_class_takes(tmp_path, monkeypatch):
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.c2ray_base as B
    from pyc2ray_amd import _capi
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 8
        plain = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        assert plain.bubble_stats is False and plain.last_bubble_sizes is None
        with pytest.raises(ValueError, match="C2Ray.bubble_stats: bubble_stats needs use_gpu=True"):
            plain.bubble_stats = True
        plain.bubble_stats = False
        for bad in (1, 0, None, "on", 1.0):
            with pytest.raises(ValueError, match="bubble_stats must be a bool"):
                plain.bubble_stats = bad
        body = open(PLAIN_PARAMS).read()
        key = lambda text: body.replace("  logfile: pyC2Ray.log\n", f"  logfile: pyC2Ray.log\n{text}")
        assert key("x") != body
        for text, what in (("  bubble_sizes: 2\n", "Output: bubble_sizes must be 0 or 1"), ("  bubble_sizes: 'yes'\n", "must be 0 or 1"),
                           ("  bubble_sizes: 1.0\n", "must be 0 or 1"),
                           ("  bubble_sizes: 1\n", "Output: bubble_sizes: 1: bubble_stats needs use_gpu=True"),
                           ("  bubble_rays: -5\n", "n_rays must be an integer >= 0"), ("  bubble_rays: 1.5\n", "n_rays must be"),
                           ("  bubble_threshold: .nan\n", "threshold must be a finite number"), ("  bubble_threshold: half\n", "threshold must be"),
                           ("  bubble_seed: -1\n", "seed must be an integer in"), ("  bubble_seed: 0.5\n", "seed must be")):
            with open("p.yml", "w") as f:
                f.write(key(text))
            with pytest.raises(ValueError, match=what):
                pc2r.C2Ray_Test("p.yml", N, False)
        with open("p.yml", "w") as f:
            f.write(key("  bubble_sizes: 0\n  bubble_rays: 300\n"))
        assert pc2r.C2Ray_Test("p.yml", N, False).bubble_stats is False
        # an object with use_gpu (as one constructed with use_gpu=True has it) reading the keys
        with open("p.yml", "w") as f:
            f.write(key("  bubble_sizes: 1\n  bubble_rays: 300\n  bubble_threshold: 0.25\n  bubble_seed: 11\n"))
        sim = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        sim.gpu = True
        sim._read_paramfile("p.yml")
        sim._statistic_init("bubble_stats")
        assert sim.bubble_stats is True and sim.last_bubble_sizes is None
        lib = _install(monkeypatch, BB.Bubbling(N))
        steps = []
        monkeypatch.setattr(B, "evolve3D", lambda *a, **kw: steps.append("evolve3D") or (np.full((N, N, N), 0.75), np.zeros((N, N, N))))
        monkeypatch.setattr(B, "evolve3D_resident", lambda *a, **kw: steps.append("evolve3D_resident"))
        flux, pos = np.ones(1), np.ones((3, 1), dtype=int)
        # the resident path: the device grid where it lies -- no upload, no download, the bookkeeping untouched
        sim.device_resident = True
        sim.evolve3D(2.0, flux, pos)
        assert steps == ["evolve3D_resident"] and lib.names() == ["bubble_mfp"]
        args = lib.calls[0][1]
        assert args[:7] == (_capi.GRID_XH, 0.25, 0, True, 11, 300, float(N)) and args[7].size == 65
        first = sim.last_bubble_sizes
        assert (first.n_rays, first.dr, first.periodic, first.ended) == (300, sim.dr, True, 90)
        assert sim._device_newer >= {"xh", "phi_ion"} and "xh" not in sim._host_newer
        lib.calls.clear()
        b = sim.bubble_sizes(n_rays=50, phase="neutral", l_max=3.0, bins=4, dr=None)        # keywords override keys and defaults
        assert lib.names() == ["bubble_mfp"] and lib.calls[0][1][:7] == (_capi.GRID_XH, 0.25, 1, True, 11, 50, 3.0)
        assert b.dr is None and b is not sim.last_bubble_sizes and sim.last_bubble_sizes is first
        assert sim._device_newer >= {"xh", "phi_ion"} and "xh" not in sim._host_newer
        for name in ("field", "grid"):
            with pytest.raises(ValueError, match=f"C2Ray.bubble_sizes: {name} is not for the class"):
                sim.bubble_sizes(**{name: None})
        with pytest.raises(ValueError, match="C2Ray.bubble_sizes: n_rays must be"):
            sim.bubble_sizes(n_rays=-2)
        # otherwise: the host array goes up first
        lib.calls.clear()
        sim._device_newer.clear()
        sim.device_resident = False
        sim.evolve3D(3.0, flux, pos)
        assert steps[-1] == "evolve3D" and lib.names() == ["grid_to_device", "bubble_mfp"]
        assert lib.calls[0][1][0] == _capi.GRID_XH and np.all(lib.calls[0][1][1] == 0.75) and lib.calls[1][1][5] == 300
        assert sim.last_bubble_sizes is not first
        assert open(sim.logfile).read().count("Bubble sizes (ionised, x >= 0.25): 300 rays from 4321 cells") == 2
        # off: a step makes no library call of the feature's, and leaves the last result alone
        kept = sim.last_bubble_sizes
        sim.bubble_stats = False
        for resident in (True, False):
            lib.calls.clear()
            sim._device_newer.clear()
            sim.device_resident = resident
            sim.evolve3D(1.0, flux, pos)
            assert lib.calls == [] and sim.last_bubble_sizes is kept
        assert open(sim.logfile).read().count("Bubble sizes") == 2
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
    assert lib.names() and not [n for n in lib.names() if "bubble" in n]
