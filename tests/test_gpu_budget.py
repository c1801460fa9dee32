"""GPU: the step budget (asora_step_budget, evolve3D(..., budget=), C2Ray.photon_budget).

* The kernel against the numpy statement (tests/budget_reference.py) at N = 17 (odd: a plane range begins on an odd element, and
  fewer cells than the persistent grid has threads) and N = 40 (several strides per thread), over every clumping mode, with and
  without the Lyman-limit absorbers and the end-of-step temperature, on plane ranges (0, N), (3, 5), (N - 1, 1), (0, 0).
* Two calls return the same bits, disjoint ranges add up, no grid is written.
* evolve3D / evolve3D_resident / the class / two ranks / the opt-in features together: the step is what it is without the budget,
  and the budget is the statement's on the step's own grids.

The tolerance of every sum is 1e-12 x (the sum of its terms' magnitudes): a term differs from numpy's by a few ulp (pow, exp, FMA
contraction), a thread adds 32 terms at most at 256^3 ahead of the tree, so the error is of order 1e-14 of that scale and 1e-12
leaves two decades.  CELLS is exact.  Across ranks the grids themselves agree with one GPU to 1e-10, the sums to 1e-9 of the scale.
The bit-for-bit comparisons of whole steps trace ONE source (tests/test_gpu_clumping.py says why)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import budget_reference as BR
import cases
from test_gpu_clumping import _cells, _clump_grid, _one_source

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BB_PARAMS = os.path.join(HERE, "data", "parameters_single_black_body.yml")
CHEM = (cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)
TOL, TOL_RANKS = 1e-12, 1e-9
LLS = (1e-3, 0.05)


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib, _capi
    lib.clumping(0)
    lib.lls_opacity(0.0, 0.0)
    if p.cuda_is_init():
        lib.thermal_params(False)
        p.device_close()


def _fresh(p, N, thin=None, thick=None):
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)
    if thin is not None:
        p.photo_table_to_device(thin, thick)


def _worst(got, ref, mag):
    """largest |got - ref| / sum |term| over the slots that have terms"""
    has = mag > 0.0
    assert np.array_equal(got[~has], ref[~has])
    return float(np.max(np.abs(got[has] - ref[has]) / mag[has])) if has.any() else 0.0


def _check(got, ref, mag, tol=TOL, what=""):
    worst = _worst(got, ref, mag)
    print(f"{what}: largest |dev - ref| / sum|term| = {worst:.2e}")
    assert got[BR.CELLS] == ref[BR.CELLS]
    assert np.all(np.abs(got - ref) <= tol * mag), (what, got, ref, mag)
    return worst


def _state(N, seed):
    """cells of a finished step: tests/test_gpu_clumping._cells plus an end-of-step ionised fraction and temperature"""
    n, T, x0, xav, gamma = _cells(N, seed)
    rng = np.random.default_rng(seed + 1000)
    x1 = np.clip(xav * 10 ** rng.uniform(-0.2, 0.2, (N, N, N)), 1e-14, 1.0)
    T1 = T * 10 ** rng.uniform(-0.3, 0.3, (N, N, N))
    return dict(n=n, T=T, x0=x0, x1=x1, xav=xav, gamma=gamma, T1=T1, clump=_clump_grid(N, seed + 2))


def _upload_state(lib, capi, s):
    for w, a in ((capi.GRID_NDENS, s["n"]), (capi.GRID_TEMP, s["T"]), (capi.GRID_XH, s["x0"]), (capi.GRID_XH_AV, s["xav"]),
                 (capi.GRID_PHI_ION, s["gamma"]), (capi.GRID_XH_INTERMED, s["x1"]), (capi.GRID_TEMP_END, s["T1"]),
                 (capi.GRID_CLUMP, s["clump"])):
        lib.grid_to_device(w, a)


def _ranges(N):
    return ((0, N), (3, 5), (N - 1, 1), (0, 0))


@pytest.mark.parametrize("N", [17, 40])
def test_kernel_against_numpy(asora, N):
    p, lib, capi = asora
    _fresh(p, N)
    s = _state(N, 500 + N)
    _upload_state(lib, capi, s)
    chem = (1.0,) + CHEM
    worst = 0.0
    try:
        for mode, const in ((0, 1.0), (1, 3.5), (2, 1.0)):
            lib.clumping(mode, const)
            clump = {0: 1.0, 1: const, 2: s["clump"]}[mode]
            for lls in ((0.0, 0.0), LLS):
                lib.lls_opacity(*lls)
                for tend in (False, True):
                    t = BR.terms(s["n"], s["x0"], s["x1"], s["xav"], s["gamma"], s["T"], CHEM, clump, lls, s["T1"] if tend else None)
                    for planes in _ranges(N):
                        ref, mag = BR.sums_of_terms(t, N, planes)
                        got = lib.step_budget(chem, use_temp_end=tend, planes=planes)
                        assert got.shape == (12,) and got.dtype == np.float64
                        worst = max(worst, _check(got, ref, mag, what=f"N={N} clumping {mode} lls {lls} temp_end {tend} planes {planes}"))
                        assert got[BR.CELLS] == planes[1] * N * N
                        if planes[1] == 0:
                            assert np.array_equal(got, np.zeros(12))
                    assert np.array_equal(lib.step_budget(chem, use_temp_end=tend), lib.step_budget(chem, use_temp_end=tend, planes=(0, N)))
    finally:
        lib.clumping(0)
        lib.lls_opacity(0.0, 0.0)
    print(f"N={N}: largest ratio over all cases {worst:.2e}")
    # what the C-ABI refuses: code 3 for a null pointer or a bad plane range, code 4 for a grid without data
    import ctypes as C
    raw = lib._lib
    out = np.zeros(12)
    ptr = out.ctypes.data_as(C.POINTER(C.c_double))
    assert raw.asora_step_budget(*CHEM, 0, 0, N, None) == 3
    for bad in ((-1, 2), (0, N + 1), (N, 1), (2, -1)):
        assert raw.asora_step_budget(*CHEM, 0, *bad, ptr) == 3 and b"step_budget" in raw.asora_last_error()
    _fresh(p, N)
    for w in (capi.GRID_NDENS, capi.GRID_TEMP, capi.GRID_XH, capi.GRID_XH_AV, capi.GRID_XH_INTERMED):
        lib.grid_to_device(w, s["n"])
    assert raw.asora_step_budget(*CHEM, 0, 0, N, ptr) == 4 and b"grid 2 holds no data" in raw.asora_last_error()      # PHI_ION
    lib.grid_to_device(capi.GRID_PHI_ION, s["gamma"])
    assert raw.asora_step_budget(*CHEM, 0, 0, N, ptr) == 0
    assert raw.asora_step_budget(*CHEM, 1, 0, N, ptr) == 4 and b"grid 7 holds no data" in raw.asora_last_error()      # TEMP_END


def test_same_bits_disjoint_ranges_and_no_grid_written(asora):
    p, lib, capi = asora
    N = 17
    _fresh(p, N)
    s = _state(N, 77)
    _upload_state(lib, capi, s)
    grids = (capi.GRID_NDENS, capi.GRID_TEMP, capi.GRID_XH, capi.GRID_XH_AV, capi.GRID_PHI_ION, capi.GRID_XH_INTERMED,
             capi.GRID_TEMP_END, capi.GRID_CLUMP)
    fetch = lambda: [lib.grid_to_host(w, np.empty((N, N, N))) for w in grids]
    before = fetch()
    chem = (1.0,) + CHEM
    lib.clumping(2)
    lib.lls_opacity(*LLS)
    try:
        whole = lib.step_budget(chem, use_temp_end=True)
        again = lib.step_budget(chem, use_temp_end=True)
        assert whole.tobytes() == again.tobytes()
        parts = [lib.step_budget(chem, use_temp_end=True, planes=pl) for pl in ((0, 6), (6, 1), (7, 10))]
        assert [lib.step_budget(chem, use_temp_end=True, planes=pl).tobytes() for pl in ((0, 6), (6, 1), (7, 10))] == [q.tobytes() for q in parts]
    finally:
        lib.clumping(0)
        lib.lls_opacity(0.0, 0.0)
    _, mag = BR.sums(s["n"], s["x0"], s["x1"], s["xav"], s["gamma"], s["T"], CHEM, s["clump"], LLS, s["T1"])
    total = parts[0] + parts[1] + parts[2]
    assert total[BR.CELLS] == whole[BR.CELLS] == N ** 3
    assert np.all(np.abs(total - whole) <= TOL * mag)
    for a, b in zip(before, fetch()):
        assert a.tobytes() == b.tobytes()


def _step(p, c, **kw):
    out = p.evolve3D(c["dt"], c["dr"], c["flux"], c["pos"], True, 1000, c["N"], 1e-2, c["temp"], c["ndens"], c["xh"], c["thin"], c["thick"],
                     cases.MINLOGTAU, c["dlogtau"], c["R"], c["convergence_fraction"], cases.SIG, *CHEM, logfile=None, quiet=True, **kw)
    return (p.evolve._evolve.last_niter,) + tuple(np.array(a) for a in out)


def _reference_of_step(lib, capi, c, x1, phi, dt, clump=1.0, lls=(0.0, 0.0), temp_end=None, keep=None):
    """(sums, magnitudes, xh_av) of the statement on the step's own grids: x0 and n as passed, the returned xh_new and phi_ion,
    and XH_AV as the device holds it."""
    N = c["N"]
    xav = lib.grid_to_host(capi.GRID_XH_AV, np.empty((N, N, N)))
    ref, mag = BR.sums(c["ndens"], c["xh"], x1, xav, phi, c["temp"], CHEM, clump, lls, temp_end, keep=keep)
    return ref, mag, xav


def test_evolve3D_with_the_budget(asora):
    p, lib, capi = asora
    from pyc2ray_amd.budget import StepBudget
    c = _one_source(cases.evolve_case("l24_gpu_F_37src"))
    N = c["N"]
    _fresh(p, N, c["thin"], c["thick"])
    plain = _step(p, c)
    b = StepBudget()
    with_budget = _step(p, c, budget=b)
    assert with_budget[0] == plain[0] >= 2
    for x, y in zip(with_budget[1:], plain[1:]):
        assert x.tobytes() == y.tobytes()
    _, x1, phi = with_budget
    ref, mag, xav = _reference_of_step(lib, capi, c, x1, phi, c["dt"])
    _check(b.sums, ref, mag, what="evolve3D")
    assert (b.dt, b.dr, b.N, b.steps) == (c["dt"], c["dr"], N, 1)
    assert b.emitted == c["flux"].sum() * 1e48 * c["dt"]
    assert b.mean_xh_mass == b.sums[BR.NX] / b.sums[BR.N_] and b.mean_xh_mass > b.mean_xh_mass_before > 0.0
    assert b.new_ions > 0.0 and 0.0 < b.absorbed < b.emitted and b.lls_absorbed == 0.0 and b.escaped > 0.0
    # the bound of the residual, DESIGN.md section 4.2c: cells clamped to 1e-14 taken out of both sides
    keep = (x1 > BR.EPS) & (xav > BR.EPS)
    dev = b.sums if keep.all() else BR.sums(c["ndens"], c["xh"], x1, xav, phi, c["temp"], CHEM, keep=keep)[0]
    res, bound = BR.residual(dev, c["dt"]), BR.residual_bound(c["ndens"], xav, c["temp"], c["dt"], CHEM, keep=keep)
    print(f"cells clamped {np.count_nonzero(~keep)}; residual / bound = {res / bound:.3f}; residual relative to the new ions "
          f"{res / dev[BR.DNX]:.2e}; escaped / emitted = {b.escaped / b.emitted:.4f}")
    assert bound > 0.0 and abs(res) <= bound
    if keep.all():
        assert b.residual == pytest.approx(res * c["dr"] ** 3, rel=1e-9)


def test_thermal_evolve3D_with_the_budget(asora):
    p, lib, capi = asora
    from pyc2ray_amd.budget import StepBudget
    from pyc2ray_amd.thermal import ThermalParams
    c = _one_source(cases.evolve_case("l24_gpu_F_37src"))
    N = c["N"]
    _fresh(p, N, c["thin"], c["thick"])
    th = ThermalParams(c["heat_thin"], c["heat_thick"])
    plain = _step(p, c, thermal=th)
    b = StepBudget()
    niter, x1, phi, temp_new = _step(p, c, thermal=th, budget=b)
    assert niter == plain[0]
    for x, y in zip((x1, phi, temp_new), plain[1:]):
        assert x.tobytes() == y.tobytes()
    assert not np.array_equal(temp_new, c["temp"])
    ref, mag, _ = _reference_of_step(lib, capi, c, x1, phi, c["dt"], temp_end=temp_new)
    _check(b.sums, ref, mag, what="thermal evolve3D")
    assert b.mean_temp == pytest.approx(0.5 * (c["temp"].mean() + temp_new.mean()), rel=1e-12)
    print(f"thermal step: residual relative to the new ions {b.residual / b.new_ions:.2e}")


def test_resident_class_with_photon_budget(asora, tmp_path):
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 24
        with open("src.txt", "w") as f:
            f.write("1\n12 12 12 5e50 1.0\n")
        if p.cuda_is_init():
            p.device_close()
        sim = pc2r.C2Ray_Test(BB_PARAMS, N, True)
        assert sim.device_resident and sim.photon_budget is False and sim.isothermal
        sim.photon_budget = True
        sim.density_init(0.0)
        srcpos, srcflux = sim.read_sources("src.txt", 1)
        dt = 3.15576e13
        chem = (sim.bh00, sim.albpow, sim.colh0, sim.temph0, sim.abu_c)
        x0 = np.array(sim.xh)                                   # (the test's own copy of the state before the step)
        g = lambda w: lib.grid_to_host(w, np.empty((N, N, N)))  # (the bare C-ABI: the class does not hear of these reads)
        budgets = []
        for step in range(2):
            sim.evolve3D(dt, srcflux, srcpos)
            b = sim.last_budget
            budgets.append(b)
            x1, xav, phi, n, T = g(capi.GRID_XH), g(capi.GRID_XH_AV), g(capi.GRID_PHI_ION), g(capi.GRID_NDENS), g(capi.GRID_TEMP)
            assert np.array_equal(x1, g(capi.GRID_XH_INTERMED))
            ref, mag = BR.sums(n, x0, x1, xav, phi, T, chem)
            _check(b.sums, ref, mag, what=f"class step {step + 1}")
            assert (b.dt, b.dr, b.N) == (dt, sim.dr, N) and b.emitted == srcflux.sum() * 1e48 * dt
            print(f"step {step + 1}: {b.log_line()}")
            x0 = x1
        assert budgets[0] is not budgets[1] and budgets[1].mean_xh_mass > budgets[0].mean_xh_mass
        t = sim.total_budget
        assert t.steps == 2 and t.dt == 2 * dt
        for k in ("emitted", "new_ions", "photoionisations", "recombinations", "collisional"):
            assert getattr(t, k) == getattr(budgets[0], k) + getattr(budgets[1], k)
        assert t.mean_xh_mass == budgets[1].mean_xh_mass and t.mean_xh_mass_before == budgets[0].mean_xh_mass_before
        assert sim._device_newer >= {"xh", "phi_ion"}          # nothing was fetched through the class
        assert open(sim.logfile).read().count("Photon budget: emitted") == 2
        sim.photon_budget = False
        sim.evolve3D(dt, srcflux, srcpos)
        assert sim.last_budget is budgets[1] and open(sim.logfile).read().count("Photon budget: emitted") == 2
    finally:
        if p.cuda_is_init():
            p.device_close()
        os.chdir(cwd)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def test_two_ranks(asora, tmp_path):
    """24^3, 37 sources, two gloo ranks on one GPU, the slab exchange (each rank reduces its own planes, the sums are added over
    the ranks) and the all-reduce loop (each rank reduces the whole grid): the ranks' budgets bit-identical, and the one-GPU
    budget's to 1e-9 of the scale."""
    p, lib, capi = asora
    import pyc2ray_amd.evolve as ev
    import _budget_dist_worker as W
    from pyc2ray_amd.budget import StepBudget
    world, port = 2, _free_port()
    outs = [str(tmp_path / f"r{r}.npz") for r in range(world)]
    env = dict(os.environ, PYC2RAY_AMD_NO_TORCH="0", OMP_NUM_THREADS="1")
    if p.cuda_is_init():
        p.device_close()
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_budget_dist_worker.py"), str(r), str(world), port, outs[r]],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = [q.communicate(timeout=300)[0].decode() for q in procs]
    for q, log in zip(procs, logs):
        assert q.returncode == 0, log
    res = [np.load(o) for o in outs]
    c = W.case()
    N = c["N"]
    _fresh(p, N, c["thin"], c["thick"])
    b = StepBudget()
    x1, phi, niter = W.evolve(ev, c, budget=b)
    ref, mag, _ = _reference_of_step(lib, capi, c, x1, phi, c["dt"])
    _check(b.sums, ref, mag, what="one GPU, 37 sources")
    for exchange in W.EXCHANGES:
        for k in ("xh", "phi", "sums", "fields"):
            assert res[0][f"{exchange}_{k}"].tobytes() == res[1][f"{exchange}_{k}"].tobytes(), (exchange, k)
        assert int(res[0][f"{exchange}_niter"]) == niter
        np.testing.assert_allclose(res[0][f"{exchange}_xh"], x1, rtol=1e-10, atol=0)
        np.testing.assert_allclose(res[0][f"{exchange}_phi"], phi, rtol=1e-10, atol=0)
        _check(res[0][f"{exchange}_sums"], b.sums, mag, tol=TOL_RANKS, what=f"two ranks, {exchange}")
        assert res[0][f"{exchange}_fields"][0] == b.emitted                      # (every rank counts the whole source list)


def test_features_together(asora):
    """One step at N = 24 with open boundaries, a face, Lyman-limit absorbers and a clumping grid."""
    p, lib, capi = asora
    from pyc2ray_amd.budget import StepBudget
    from pyc2ray_amd.lls import LLSOpacity
    from pyc2ray_amd.planeflux import PlaneFlux
    c = _one_source(cases.evolve_case("l24_gpu_F_37src"))
    N = c["N"]
    _fresh(p, N, c["thin"], c["thick"])
    clump = _clump_grid(N, 9)
    F = 3.0e-45
    lls = LLSOpacity(n_const=2e-5, per_density=0.05)
    b = StepBudget()
    niter, x1, phi = _step(p, c, budget=b, periodic=False, plane_flux=PlaneFlux("-x", F), lls=lls, clumping=clump)
    ref, mag, _ = _reference_of_step(lib, capi, c, x1, phi, c["dt"], clump=clump, lls=(lls.n_const, lls.per_density))
    _check(b.sums, ref, mag, what="features together")
    area = (N * c["dr"]) ** 2
    assert b.emitted == (c["flux"].sum() + F * area) * 1e48 * c["dt"] and F * area > 0.1 * c["flux"].sum()
    assert b.sums[BR.LLS] > 0.0 and b.lls_absorbed > 0.0 and b.absorbed == b.photoionisations + b.lls_absorbed
    assert lib.get_plane_flux() == [] and lib.get_lls_opacity() == (0.0, 0.0)
    print(f"features together: niter {niter}; {b.log_line()}")
