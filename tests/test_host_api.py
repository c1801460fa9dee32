"""CPU: host-side logic of the product package and the C-ABI surface (no GPU compute calls)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from pyc2ray_amd import _capi
    return _capi


def test_library_exports_every_declared_symbol(built):
    header = open(os.path.join(ROOT, "include", "asora_hip.h")).read()
    declared = set(re.findall(r"\b((?:asora|c2ray)_[a-z0-9_]+)\s*\(", header))
    assert declared == set(built.SIGNATURES), declared ^ set(built.SIGNATURES)
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name


def test_library_is_built_for_gfx950(built):
    blob = open(built.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    assert b"raytrace_octant_kernel" in blob and b"chemistry_kernel" in blob


def test_product_package_never_touches_the_oracle():
    pkg = os.path.join(ROOT, "pyc2ray_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "liboracle" not in txt, f


def test_guards_before_device_init(built):
    import pyc2ray_amd as p
    assert not p.cuda_is_init()
    with pytest.raises(RuntimeError, match="GPU not initialized"):
        p.device_close()
    with pytest.raises(RuntimeError, match="GPU not initialized"):
        p.photo_table_to_device(np.ones(3), np.ones(3))
    N = 8
    g = np.ones((N, N, N))
    with pytest.raises(RuntimeError, match="GPU not initialized"):
        p.evolve3D(1.0, 1.0, np.ones(1), np.ones((3, 1)), True, 10, 4, 0.01, g, g, g, np.ones(5), np.ones(5),
                   -20.0, 0.1, 4.0, 1e-4, 1e-18, 1.0, 1.0, 1.0, 1.0, 1.0, quiet=True, logfile=None)
    with pytest.raises(RuntimeError, match="GPU not initialized"):
        p.do_raytracing(1.0, np.ones(1), np.ones((3, 1)), True, 10, 4, 0.01, g, g, np.ones(5), np.ones(5),
                        np.ones(5), np.ones(5), -20.0, 0.1, 4.0, 1e-18, quiet=True, logfile=None)


def _without_a_gpu(body):
    """Runs `body` (Python source, indented as a function body) in a fresh interpreter that sees no GPU
    (HIP_VISIBLE_DEVICES=-1), so that what the library does without one is checked on every machine, one with a GPU
    included.  An AssertionError there fails the test here, with the child's output."""
    import subprocess
    import sys
    import textwrap
    code = ("import sys\nsys.path.insert(0, %r)\nimport numpy as np\nimport pytest\n" % ROOT) + textwrap.dedent(body)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_cpu_semantics_path_has_no_cpu_fallback(built):
    """use_gpu=False selects the SEMANTICS of the reference's CPU raytracer (sub-boxes, photon loss); the work is
    still done by the HIP library.  Without a GPU the call fails loudly instead of computing on the host."""
    _without_a_gpu("""
        import pyc2ray_amd as p
        N = 8
        g = np.ones((N, N, N)) * 0.5
        with pytest.raises(RuntimeError, match="device_init_auto failed"):
            p.evolve3D(1.0, 1.0, np.ones(1), np.ones((3, 1)), False, 10, 4, 0.01, g, g, g, np.ones(5), np.ones(5),
                       -20.0, 0.1, 4.0, 1e-4, 1e-18, 1.0, 1.0, 1.0, 1.0, 1.0, quiet=True, logfile=None)
        with pytest.raises(RuntimeError, match="do_all_sources failed"):
            p.do_raytracing(1.0, np.ones(1), np.ones((3, 1)), False, 10, 4, 0.01, g, g, np.ones(5), np.ones(5),
                            np.ones(5), np.ones(5), -20.0, 0.1, 4.0, 1e-18, quiet=True, logfile=None)
    """)


def test_errors_come_back_as_runtime_errors_with_message(built):
    _without_a_gpu("""
        from pyc2ray_amd.load_extensions import load_asora
        lib = load_asora()
        with pytest.raises(RuntimeError, match="not initialised"):
            lib.density_to_device(np.zeros(8), 2)
        with pytest.raises(RuntimeError):          # no GPU here: hipSetDevice fails, message carried over
            lib.device_init(8, 1)
    """)


def test_live_buffers_before_any_device_init(built):
    """asora_debug_live_buffers reads the registry of the library's buffers on the host: callable with no device, and a process
    that never called device_init holds nothing of either lifetime."""
    _without_a_gpu("""
        from pyc2ray_amd.load_extensions import load_asora
        lib = load_asora()
        assert lib.live_buffers(0) == (0, 0)
        assert lib.live_buffers(1) == (0, 0)
        with pytest.raises(RuntimeError, match="lifetime"):
            lib.live_buffers(2)
        with pytest.raises(RuntimeError):          # no GPU here: a refused device_init leaves nothing of the mesh behind
            lib.device_init(8, 1)
        assert lib.live_buffers(0) == (0, 0)
    """)


def test_format_sources_layout():
    from pyc2ray_amd.utils.sourceutils import format_sources
    pos = np.array([[1, 4], [2, 5], [3, 6]], dtype=float)          # (3, 2), 1-based
    flat, flux = format_sources(pos, np.array([1, 2]))
    assert flat.dtype == np.int32 and flux.dtype == np.float64
    assert flat.tolist() == [0, 1, 2, 3, 4, 5]                     # x0,y0,z0,x1,y1,z1 zero-based
    with pytest.raises(ValueError):
        format_sources(np.ones((2, 3)), np.ones(3))


def test_source_file_round_trip(tmp_path):
    from pyc2ray_amd.utils.sourceutils import generate_test_sourcefile, read_test_sources
    fn = str(tmp_path / "src.txt")
    generate_test_sourcefile(fn, 64, 7, 5e52, seed=100)
    pos, flux = read_test_sources(fn, 5)
    rng = np.random.RandomState(100)
    want = (1 + rng.randint(0, 64, size=21)).reshape(7, 3)[:5].T
    assert np.array_equal(pos, want) and np.allclose(flux, 5e4)
    with pytest.raises(ValueError):
        read_test_sources(fn, 8)


def test_tau_and_blackbody_tables():
    from pyc2ray_amd.radiation import BlackBodySource, make_tau_table
    tau, dlog = make_tau_table(-20.0, 4.0, 200)
    assert tau.shape == (201,) and tau[0] == 0.0 and np.isclose(tau[1], 1e-20) and np.isclose(dlog, 0.12)
    ev2fr = 0.241838e15
    grey = BlackBodySource(5e4, True, ev2fr * 13.598, 2.8)
    thin, thick = grey.make_photo_table(tau, ev2fr * 13.598, 10 * ev2fr * 54.416, 1e48)
    # grey opacity: both tables are S_star * exp(-tau) in closed form
    np.testing.assert_allclose(thick, 1e48 * np.exp(-tau), rtol=1e-9, atol=1e-300)
    np.testing.assert_allclose(thin, 1e48 * np.exp(-tau), rtol=1e-9, atol=1e-300)
    pl = BlackBodySource(1e5, False, ev2fr * 13.598, 2.8)
    thin, thick = pl.make_photo_table(tau, ev2fr * 13.598, 10 * ev2fr * 54.416, 1e48)
    assert np.isclose(thick[0], 1e48) and np.all(np.diff(thick) <= 1e-9 * thick[0]) and thin[0] < thick[0]


def test_radiation_tables_equal_the_reference_python():
    """tests/golden/radiation.npz holds make_tau_table(-20, 4, 2000) and the photo-ionisation tables of Teff = 5e3, 5e4,
    1e5 K, grey and power-law cross sections, produced by the reference's own pyc2ray/radiation/{common,blackbody}.py
    (tests/golden/make_radiation_golden.py).  The benchmark, paper test 3 and the hackathon test all run on such tables."""
    from pyc2ray_amd.radiation import BlackBodySource, make_tau_table
    g = np.load(os.path.join(ROOT, "tests", "golden", "radiation.npz"))
    tau, dlog = make_tau_table(-20.0, 4.0, 2000)
    assert np.array_equal(tau, g["tau"]) and dlog == float(g["dlogtau"])
    ev2fr = 0.241838e15
    f1, f2 = ev2fr * 13.598, 10 * ev2fr * 54.416
    for teff in g["teffs"]:
        for grey in (True, False):
            src = BlackBodySource(float(teff), grey, f1, 2.8)
            thin, thick = src.make_photo_table(tau, f1, f2, 1e48)
            key = f"T{teff:g}_{'grey' if grey else 'pl'}"
            np.testing.assert_allclose(src.R_star, float(g[key + "_Rstar"]), rtol=1e-13)
            for got, name in ((thin, "_thin"), (thick, "_thick")):
                want = g[key + name]
                assert np.array_equal(got != 0, want != 0), key + name       # the table's cut-off (tau a > 700) in the same place
                np.testing.assert_allclose(got, want, rtol=1e-10, atol=0, err_msg=key + name)
            if not grey:      # the shape the grey closed form cannot see: harder photons are absorbed less
                assert thin[0] < 0.95 * thick[0] and thick[1500] > 1e48 * np.exp(-tau[1500])


def test_blackbody_heating_tables_grey_closed_form():
    """Grey opacity: every photon sees the same optical depth, so both heating tables are H0 * exp(-tau) with
    H0 = int h (nu - nu_HI) S(nu) dnu, and the mean energy per ionisation H0/S_star lies between 0 and
    h (nu_max - nu_HI)."""
    from scipy.integrate import quad
    from pyc2ray_amd.radiation import BlackBodySource, make_tau_table
    from pyc2ray_amd.radiation.blackbody import hplanck, ion_freq_HI
    tau, _ = make_tau_table(-20.0, 4.0, 120)
    ev2fr = 0.241838e15
    f1, f2 = ev2fr * 13.598, 10 * ev2fr * 54.416
    src = BlackBodySource(5e4, True, f1, 2.8)
    hthin, hthick = src.make_heat_table(tau, f1, f2, 1e48)
    H0 = quad(lambda f: hplanck * (f - ion_freq_HI) * src.SED(f), f1, f2, epsrel=1e-12)[0]
    assert 0.0 < H0 / 1e48 < hplanck * (f2 - ion_freq_HI)
    keep = tau < 600.0
    np.testing.assert_allclose(hthick[keep], H0 * np.exp(-tau[keep]), rtol=1e-8, atol=1e-300)
    np.testing.assert_allclose(hthin[keep], H0 * np.exp(-tau[keep]), rtol=1e-8, atol=1e-300)
    # non-grey: harder photons are absorbed less, so the thick table falls more slowly than exp(-tau)
    src2 = BlackBodySource(5e4, False, f1, 2.8)
    h2thin, h2thick = src2.make_heat_table(tau, f1, f2, 1e48)
    i = int(np.searchsorted(tau, 5.0))
    assert h2thick[i] / h2thick[0] > np.exp(-tau[i])
    assert np.all(np.diff(h2thick) <= 1e-9 * h2thick[0])


def test_printlog_lines_writes_what_printlog_would(tmp_path, capsys):
    """The batch form used by the loop of a time step: same file content, same terminal output as one printlog per line."""
    from pyc2ray_amd.utils.logutils import printlog, printlog_lines
    lines = [("Doing Raytracing...", ' '), ("took  0.0 s.", '\n'), ("Number of non-converged points: 3", '\n')]
    a, b = tmp_path / "a.log", tmp_path / "b.log"
    for text, end in lines:
        printlog(text, str(a), quiet=False, end=end)
    one = capsys.readouterr().out
    printlog_lines(lines, str(b), quiet=False)
    two = capsys.readouterr().out
    assert open(a).read() == open(b).read() == "Doing Raytracing... took  0.0 s.\nNumber of non-converged points: 3\n"
    assert one == two
    printlog_lines([], str(b), quiet=True)
    printlog_lines(lines, None, quiet=True)
    assert capsys.readouterr().out == ""


def test_bench_trip_counts_equal_the_oracles_do_chemistry():
    """bench.py's `evolving_state` prints a histogram of do_chemistry trip counts per cell, recomputed on the host with a
    vectorised restatement of chemistry.f90:146-203; here that restatement against the oracle's do_chemistry (which returns its
    trip count) on random cells, Gamma from 0 to huge, temperatures from 1e3 to 5e4 K."""
    import bench
    from oracle import oracle as O
    rng = np.random.default_rng(11)
    n = 400
    nd = 1e-3 * np.exp(rng.normal(size=n))
    T = 10 ** rng.uniform(3.0, 4.7, size=n)
    x0 = 10 ** rng.uniform(-4, -0.01, size=n)
    xav = np.clip(x0 * rng.uniform(0.5, 1.5, size=n), 1e-10, 1 - 1e-10)
    g = 10 ** rng.uniform(-20, -8, size=n)
    g[rng.uniform(size=n) < 0.2] = 0.0
    g[rng.uniform(size=n) < 0.05] = 1e-2
    dt = 3.15576e13
    mine = bench.trip_counts(dt, nd, T, x0, xav, g, bench.BH00, bench.ALBPOW, bench.COLH0, bench.TEMPH0, bench.ABU_C)
    ref = np.array([O.do_chemistry(dt, nd[q], T[q], x0[q], xav[q], g[q], bench.BH00, bench.ALBPOW, bench.COLH0, bench.TEMPH0,
                                   bench.ABU_C)[2] for q in range(n)])
    assert np.array_equal(mine, ref)
    assert ref.max() >= 3 and ref.min() == 1


# ---- round 6: host logic of the multi-rank batches and of the device-resident C2Ray grids (no GPU) ----------------------------
def test_next_batch_follows_the_distance_to_the_convergence_test():
    """evolve._next_batch: a multi-rank iteration's collectives are not gated by the device's `done` flag, so the batch shrinks as
    the test of evolve.py:232 comes within reach -- computed from the rows every rank polled, hence the same on every rank."""
    from pyc2ray_amd.evolve import _next_batch
    assert _next_batch([], 1, 3.0, 1e-4) == 1                       # gloo: always one
    assert _next_batch([], 8, 3.0, 1e-4) == 2                       # nothing to extrapolate from yet
    assert _next_batch([(1e5, 0, 0, 1.0, 1.0)], 8, 3.0, 1e-4) == 2
    # both criteria decay by 5 per iteration: rel 2e-2 -> 1e-4 needs ceil(log(200)/log(5)) = 4 more
    h = [(1e5, 0, 0, 1e-1, 1e-2), (2e4, 0, 0, 2e-2, 2e-3)]
    assert _next_batch(h, 8, 3.0, 1e-4) == 4
    assert _next_batch(h, 2, 3.0, 1e-4) == 2                        # never beyond the cap
    # the count criterion gets there first: 2e4 -> below 5e3 in one step of 5
    assert _next_batch(h, 8, 5e3, 1e-4) == 1
    # not decaying (or growing): no extrapolation, the full batch
    assert _next_batch([(10, 0, 0, 1e-2, 1e-3), (10, 0, 0, 2e-2, 2e-3)], 8, 3.0, 1e-4) == 8
    # conv_criterion = 0 (one source): only the relative changes count
    assert _next_batch(h, 8, 0, 1e-4) == 4
    # every simulated run ends without an iteration wasted once the decay is steady
    rows, rel, flag, wasted = [], 20.0, 3000.0, 0
    while True:
        b = _next_batch(rows, 8, 1.3, 1e-4)
        done_at = None
        for q in range(b):
            rows.append((flag, 0, 0, rel, 0.1 * rel))
            if done_at is None and (flag < 1.3 or rel < 1e-4):
                done_at = q
            rel *= 0.2
            flag *= 0.4
        if done_at is not None:
            wasted = b - 1 - done_at
            break
    assert wasted == 0 and len(rows) < 20


def test_comm_backend_of_foreign_communicators():
    from pyc2ray_amd.evolve import _comm_backend

    class WithProperty:
        backend = "nccl"

    class WithMethodOnly:
        def _backend(self):
            return "gloo"

    class Mpi4pyLike:
        pass

    assert _comm_backend(WithProperty()) == "nccl" and _comm_backend(WithMethodOnly()) == "gloo" and _comm_backend(Mpi4pyLike()) == "gloo"


def test_residency_registry_reclaims_every_other_holder():
    """pyc2ray_amd/_residency.py: whoever is about to overwrite the device grids first lets resident holders take their data home."""
    from pyc2ray_amd import _residency

    class Holder:
        def __init__(self):
            self.left = 0

        def _leave_device(self):
            self.left += 1

    a, b = Holder(), Holder()
    _residency.register(a)
    _residency.register(b)
    _residency.reclaim(except_for=a)
    assert (a.left, b.left) == (0, 1)
    _residency.reclaim()
    assert (a.left, b.left) == (1, 2)
    del b                                   # (weak references: a holder that is gone is not kept alive)
    import gc
    gc.collect()
    _residency.reclaim()
    assert a.left == 2


def test_grid_fingerprint_sees_rescalings_and_respects_storage_order():
    from pyc2ray_amd.c2ray_base import C2Ray
    g = np.asfortranarray(np.random.default_rng(0).random((48, 48, 48)))
    f0 = C2Ray._fingerprint(g)
    assert f0.base is None and f0.shape[0] >= min(C2Ray._FINGERPRINT_SAMPLES, g.size) // 2       # a copy, not a view
    assert np.array_equal(C2Ray._fingerprint(g), f0)
    g *= 3.0                                # what cosmo_evolve / a script does in place
    assert not np.array_equal(C2Ray._fingerprint(g), f0)
    c = np.ascontiguousarray(g)
    assert C2Ray._fingerprint(c).shape == C2Ray._fingerprint(g).shape
    assert C2Ray.device_resident is True
