"""Per-source spectra, the parts that need no GPU: the checks of ``src_spectrum=`` and of ``spectra_to_device`` that run before
any GPU work, the spectrum of each source carried through the library's position sort and through the sharding of dist.py, and
the YAML list form of ``BlackBodySource: Teff``."""
import os

import numpy as np
import pytest

import cases


@pytest.fixture(scope="module")
def lib():
    from pyc2ray_amd.load_extensions import load_asora
    return load_asora()


def _evolve_args(N=8, ns=4, use_gpu=True):
    nd, xh, dr = cases.grid(N, "uniform", 1, 0.1)
    pos, flux = cases.sources(N, ns, 2)
    thin, thick, dlog = cases.soft_tables(50)
    T = np.full((N, N, N), 1e4)
    return (3e13, dr, flux, pos, use_gpu, 1000, N, 1e-2, T, nd, xh, thin, thick, cases.MINLOGTAU, dlog, 3.0, 1e-4, cases.SIG,
            cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)


@pytest.mark.parametrize("spec,use_gpu,match", [
    (np.array([0, 1, 0]), True, "one entry per source"),
    (np.array([[0, 1, 0, 1]]), True, "one entry per source"),
    (np.array([0.0, 1.0, 0.0, 1.0]), True, "integer array"),
    (np.array([True, False, False, True]), True, "integer array"),
    (np.array([0, -1, 0, 1]), True, "negative"),
    (np.array([0, 1, 0, 2]), False, "use_gpu=True"),
    (np.array([0, 1, 0, 7]), True, "index 7"),          # no table set on the device at all: num_spectra() = 0
])
def test_src_spectrum_is_checked_before_any_gpu_work(tmp_path, spec, use_gpu, match):
    import pyc2ray_amd as p
    args = _evolve_args(use_gpu=use_gpu)
    log = dict(logfile=str(tmp_path / "log"), quiet=True)
    with pytest.raises(ValueError, match=match):
        p.evolve3D(*args, src_spectrum=spec, **log)
    with pytest.raises(ValueError, match=match):
        p.evolve3D_MPI(*args[:8], None, None, 0, 1, *args[8:], src_spectrum=spec, **log)
    with pytest.raises(ValueError, match=match):
        p.evolve3D_resident(args[0], args[1], args[2], args[3], {}, args[6], args[11], args[13], args[14], args[15], args[16], args[17],
                            *args[18:], src_spectrum=spec, **log) if use_gpu else p.evolve3D(*args, src_spectrum=spec, **log)
    with pytest.raises(ValueError, match=match):
        p.do_raytracing(args[1], args[2], args[3], use_gpu, 1000, 8, 1e-2, args[9], args[10], args[11], args[12], None, None,
                        args[13], args[14], args[15], args[17], src_spectrum=spec, **log)


def test_all_zero_src_spectrum_is_no_spectrum():
    from pyc2ray_amd.spectra import source_spectrum_spec

    def never():
        raise AssertionError("asked for the number of table sets")
    assert source_spectrum_spec(None, 4, True, never) is None
    assert source_spectrum_spec(np.zeros(4, dtype=np.int64), 4, True, never) is None
    assert source_spectrum_spec(np.zeros(4, dtype=np.int64), 4, False, never) is None
    assert source_spectrum_spec(np.zeros(0, dtype=np.int32), 0, True, never) is None
    s = source_spectrum_spec(np.array([0, 2, 1], dtype=np.uint8), 3, True, lambda: 3)
    assert s.dtype == np.int32 and s.tolist() == [0, 2, 1]


def test_spectra_to_device_checks_shapes(lib):
    t = np.ones((3, 20))
    for bad, match in (((np.ones(20), np.ones(20)), "2-D"), ((t, np.ones((2, 20))), "shape"), ((t, t, t), "without the other"),
                       ((t, t, t, np.ones((3, 19))), "shape"), ((np.ones((17, 20)), np.ones((17, 20))), "17 spectra"),
                       ((np.ones((0, 20)), np.ones((0, 20))), "0 spectra")):
        with pytest.raises(ValueError, match=match):
            lib.spectra_to_device(*bad)
    with pytest.raises(ValueError, match="integer"):
        lib.source_spectra_to_device(np.array([0.0, 1.0]))
    with pytest.raises(RuntimeError):                    # well-formed, but there is no device here / nothing initialised
        if lib._N is None:
            lib.spectra_to_device(t, t)
        else:
            raise RuntimeError("initialised elsewhere")


def test_exports_are_declared_and_bound(lib):
    from pyc2ray_amd import _capi
    import pyc2ray_amd as p
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "asora_hip.h")).read()
    for name in ("asora_spectra_to_device", "asora_source_spectra_to_device", "asora_num_spectra"):
        assert name in _capi.SIGNATURES and f"int {name}(" in header and hasattr(lib._lib, name)
    for name in ("spectra_to_device", "source_spectra_to_device", "num_spectra", "photo_table_to_device"):
        assert callable(getattr(p, name))
    assert lib.num_spectra() in range(0, _capi.MAX_SPECTRA + 1)


def test_spectrum_follows_its_source_through_the_position_sort(lib):
    """The library's position-ordered copy of a source list (what whole-list launches and the pipelined call work from), through
    the host-only hook: the lexicographic stable order rebuilt in numpy, and every (position, flux, spectrum) triple preserved."""
    rng = np.random.RandomState(3)
    n, N = 257, 12                                      # many equal first (and second) coordinates; duplicates too
    pos1 = 1 + rng.randint(0, N, size=(3, n))
    pos1[:, 5] = pos1[:, 200]                           # two sources in one cell: the stable order keeps 5 before 200
    flux = rng.uniform(1, 2, n)
    spec = rng.randint(0, 16, n).astype(np.int32)
    p0, f0 = cases.flat_sources(pos1, flux)
    ps, fs, ss = lib.sort_sources(p0, f0, spec)
    xyz = p0.reshape(n, 3)
    order = np.lexsort((np.arange(n), xyz[:, 2], xyz[:, 1], xyz[:, 0]))
    assert np.array_equal(ps.reshape(n, 3), xyz[order])
    assert np.array_equal(fs, f0[order]) and np.array_equal(ss, spec[order])
    triples = lambda a, b, c: sorted(zip(map(tuple, a.reshape(n, 3).tolist()), b.tolist(), c.tolist()))
    assert triples(ps, fs, ss) == triples(p0, f0, spec)
    assert list(order).index(5) < list(order).index(200)
    ps2, fs2, none = lib.sort_sources(p0, f0)
    assert none is None and np.array_equal(ps2, ps) and np.array_equal(fs2, fs)


def test_spectrum_follows_its_source_through_the_sharding():
    from pyc2ray_amd.dist import TorchComm
    from pyc2ray_amd.evolve import _contiguous_shard
    rng = np.random.RandomState(4)
    n = 37
    pos = 1 + rng.randint(0, 20, size=(3, n))
    flux = rng.uniform(1, 2, n)
    spec = rng.randint(0, 3, n)
    key = {(tuple(pos[:, s]), flux[s]): spec[s] for s in range(n)}
    P, F, bounds, S = TorchComm.shard_sources_by_slab(pos, flux, 3, spec)
    assert bounds == [0, 12, 24, 37] and np.all(np.diff(P[0]) >= 0)
    assert all(key[(tuple(P[:, s]), F[s])] == S[s] for s in range(n))
    assert len(TorchComm.shard_sources_by_slab(pos, flux, 3)) == 3
    P, F, S = TorchComm.sort_sources_for_overlap(pos, flux, spec)
    assert all(key[(tuple(P[:, s]), F[s])] == S[s] for s in range(n))
    for rank in range(3):
        P, F, S = _contiguous_shard(pos, flux, ("mpi", object(), rank, 3), spec)
        assert F.shape == S.shape and all(key[(tuple(P[:, s]), F[s])] == S[s] for s in range(F.shape[0]))
    assert _contiguous_shard(pos, flux, (None, None, 0, 1), spec)[2] is spec


def test_teff_list_builds_one_table_set_per_temperature(tmp_path):
    """``BlackBodySource: Teff: [..]``: K table sets from the scalar form's builder; the first equals the scalar form's tables."""
    import yaml
    from pyc2ray_amd.c2ray_base import C2Ray
    base = yaml.safe_load(open(os.path.join(os.path.dirname(__file__), "data", "parameters_single_black_body.yml")))

    class _Radiation(C2Ray):
        """Only the radiation part of the constructor."""
        def __init__(self, ld):
            self._ld, self.rank, self.gpu = ld, 0, False
            self.logfile = str(tmp_path / "log")
            self.eth0, self.ethe1 = 13.598, 54.416
            self._radiation_init()

        def printlog(self, s, quiet=False):
            pass

    base["Photo"]["NumTau"] = 60
    base["Photo"]["compute_heating_rates"] = 1
    base["BlackBodySource"]["Teff"] = 5e4
    one = _Radiation(base)
    several = dict(base, BlackBodySource=dict(base["BlackBodySource"], Teff=[5e4, 2e5, 1e5]))
    many = _Radiation(several)
    assert many.spectra_photo_thin_table.shape == many.spectra_heat_thick_table.shape == (3, 61)
    for name in ("photo_thin_table", "photo_thick_table", "heat_thin_table", "heat_thick_table"):
        assert np.array_equal(getattr(many, "spectra_" + name)[0], getattr(one, name))
        assert np.array_equal(getattr(many, name), getattr(one, name))
        assert not np.allclose(getattr(many, "spectra_" + name)[1], getattr(one, name))
    assert not hasattr(one, "spectra_photo_thin_table")
    no_heat = _Radiation(dict(several, Photo=dict(base["Photo"], compute_heating_rates=0)))
    assert no_heat.spectra_heat_thin_table is None and not no_heat.heat_thin_table.any()
    with pytest.raises(ValueError, match="17 temperatures"):
        _Radiation(dict(base, BlackBodySource=dict(base["BlackBodySource"], Teff=[5e4] * 17)))
