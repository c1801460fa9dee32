"""GPU: clumping of the recombination rate (asora_clumping, evolve3D(..., clumping=), C2Ray.clumping).

* A grid of ones is clumping off, and one constant C is clumping off with bh00 x C -- bit for bit, in every form of the pass.
* A log-normal grid against the numpy statement (tests/clumping_reference.py), the device loop against a host loop of
  isolated calls, the thermal pass, a Stroemgren sphere, two ranks, and the C2Ray class.
Sizes 17, 40, 197 and 200 cover the tile edges of the tiled pass and the odd last cell of chemistry_kernel.
The bit-for-bit comparisons of whole steps trace ONE source: the rates of several sources meet in a cell through atomic adds, in
an order that varies from run to run, so two runs of the same multi-source step agree to rounding only (each such test first
checks that its case repeats itself exactly)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import cases
import clumping_reference as CR
import thermal_reference as TR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BB_PARAMS = os.path.join(HERE, "data", "parameters_single_black_body.yml")
CHEM = (cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)
SIZES = (17, 40, 197, 200)
# the isothermal pass is compiled with FMA contraction, the statement is numpy: in the slow cells (delth dt small) an ulp is
# amplified as tests/test_gpu_thermal.py describes; those cells get its looser bounds
WELL_CONDITIONED, ILL_RTOL_XAV, ILL_RTOL = 1e-2, 1e-3, 1e-7


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib, _capi
    lib.clumping(0)
    if p.cuda_is_init():
        lib.thermal_params(False)
        p.device_close()


def _init(p, lib, N):
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)
    thin, thick, dlog = cases.soft_tables()
    p.photo_table_to_device(thin, thick)
    lib.heat_table_to_device(3e-11 * thin, 2.5e-11 * thick, thin.shape[0])
    return thin, thick, dlog


def _cells(N, seed, uniform_T=False):
    rng = np.random.default_rng(seed)
    s = (N, N, N)
    n = 10 ** rng.uniform(-4, 1, s)
    T = np.full(s, 1e4) if uniform_T else 10 ** rng.uniform(2, 5, s)
    xh = 10 ** rng.uniform(-4, 0, s) * 0.999
    xav = np.clip(xh * 10 ** rng.uniform(-0.3, 0.3, s), 1e-6, 0.999)
    gamma = np.where(rng.random(s) < 0.3, 0.0, 10 ** rng.uniform(-16, -11, s))
    return n, T, xh, xav, gamma


def _clump_grid(N, seed):
    """log-normal factors in [1, 50]"""
    return np.exp(np.random.default_rng(seed).normal(1.0, 0.8, (N, N, N))).clip(1.0, 50.0)


def _upload(lib, capi, n, T, xh, xav, gamma):
    for w, a in ((capi.GRID_NDENS, n), (capi.GRID_TEMP, T), (capi.GRID_XH, xh), (capi.GRID_XH_AV, xav), (capi.GRID_PHI_ION, gamma)):
        lib.grid_to_device(w, a)


def _isolated(lib, capi, N, cells, dt, bh00, mode=0, c=1.0):
    _upload(lib, capi, *cells)
    lib.clumping(mode, c)
    try:
        out = lib.chemistry_device(dt, bh00, *CHEM[1:])
    finally:
        lib.clumping(0)
    g = lambda w: lib.grid_to_host(w, np.empty((N, N, N)))
    return out, g(capi.GRID_XH_INTERMED), g(capi.GRID_XH_AV)


def _ranged(lib, capi, N, cells, dt, bh00, mode=0, c=1.0):
    """asora_chemistry_range over two slabs (the pipelined path's tiled pass)"""
    _upload(lib, capi, *cells)
    lib.clumping(mode, c)
    try:
        h = N // 2
        lib.chemistry_range(dt, bh00, *CHEM[1:], 0, h, 1)
        lib.chemistry_range(dt, bh00, *CHEM[1:], h, N - h, 0)
        out = lib.chemistry_finish()
    finally:
        lib.clumping(0)
    g = lambda w: lib.grid_to_host(w, np.empty((N, N, N)))
    return out, g(capi.GRID_XH_INTERMED), g(capi.GRID_XH_AV)


def _same(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("N", SIZES)
def test_isolated_and_ranged_passes_ones_constant_and_grid(asora, N):
    p, lib, capi = asora
    _init(p, lib, N)
    dt = 1e12
    cells = _cells(N, 300 + N)
    lib.grid_to_device(capi.GRID_CLUMP, np.ones((N, N, N)))
    for run in (_isolated, _ranged):
        off = run(lib, capi, N, cells, dt, cases.BH00)
        _same(run(lib, capi, N, cells, dt, cases.BH00, 2), off)                         # a grid of ones is off
        _same(run(lib, capi, N, cells, dt, cases.BH00, 1, 3.0), run(lib, capi, N, cells, dt, 3.0 * cases.BH00))   # C = bh00 C
    # a log-normal grid, in Fortran order
    clump = _clump_grid(N, N)
    lib.grid_to_device(capi.GRID_CLUMP, np.asfortranarray(clump))
    (conv, s1, _), xi, xa = _isolated(lib, capi, N, cells, dt, cases.BH00, 2)
    _, rxi, rxa = _ranged(lib, capi, N, cells, dt, cases.BH00, 2)
    np.testing.assert_allclose(rxi, xi, rtol=1e-12, atol=0)       # (the two passes: pair vs single loads, same arithmetic)
    if N != 200:
        ref_xi, ref_xa, ref_conv, ref_s1, delta = CR.chemistry_pass(dt, *cells, *CHEM, clump=clump, return_delta=True)
        well = delta > WELL_CONDITIONED
        assert well.sum() > 0.2 * N ** 3
        for got, ref, loose in ((xi, ref_xi, ILL_RTOL), (xa, ref_xa, ILL_RTOL_XAV)):
            np.testing.assert_allclose(got[well], ref[well], rtol=1e-10, atol=0)
            np.testing.assert_allclose(got, ref, rtol=loose, atol=0)
        assert abs(conv - ref_conv) <= max(2, 1e-4 * N ** 3) and s1 == pytest.approx(ref_s1, rel=1e-10)
        off_xa = _isolated(lib, capi, N, cells, dt, cases.BH00)[2]
        assert np.mean(xa < off_xa) > 0.5                          # more recombination, less ionisation
    # a grid filled with one constant against the constant form: c (bh00 ...) vs (C bh00) ... -- an ulp of brech0, amplified by
    # 1 / (delth dt) in the slow cells: 1e-12 where delth dt > 1 (1.5e-13 measured at most), 1e-10 where > 1e-2
    lib.grid_to_device(capi.GRID_CLUMP, np.full((N, N, N), 7.5))
    _, gxi, gxa = _isolated(lib, capi, N, cells, dt, cases.BH00, 2)
    _, cxi, cxa = _isolated(lib, capi, N, cells, dt, cases.BH00, 1, 7.5)
    if N != 200:
        delta = CR.chemistry_pass(dt, *cells, *CHEM, clump=7.5, return_delta=True)[4]
        assert (delta > 1.0).sum() > 0.1 * N ** 3
        np.testing.assert_allclose(gxi[delta > 1.0], cxi[delta > 1.0], rtol=1e-12, atol=0)
        np.testing.assert_allclose(gxi[delta > WELL_CONDITIONED], cxi[delta > WELL_CONDITIONED], rtol=1e-10, atol=0)
    np.testing.assert_allclose(gxi, cxi, rtol=ILL_RTOL, atol=0)
    np.testing.assert_allclose(gxa, cxa, rtol=ILL_RTOL_XAV, atol=0)


def _loop_case(N, seed=5, ns=4):
    rng = np.random.default_rng(seed)
    pos = rng.integers(1, N + 1, size=(3, ns))
    flux = 10 ** rng.uniform(-1.5, -0.5, ns) * (N / 32.0) ** 3
    n = 1e-3 * 10 ** rng.uniform(-0.3, 0.3, (N, N, N))
    xh = np.full((N, N, N), 1.2e-3)
    return pos, flux, n, xh


def _device_step(lib, capi, N, chem, R, dr, dlog, numtau, nsrc, mode=0, c=1.0):
    conv_frac = 1e-4
    crit = min(int(conv_frac * N ** 3), (nsrc - 1) / 3)
    lib.clumping(mode, c)
    try:
        lib.evolve_begin(*chem, R, cases.SIG, dr, cases.MINLOGTAU, dlog, numtau, 0, nsrc, crit, conv_frac)
        done, niter = False, 0
        while not done:
            lib.evolve_enqueue(4)
            niter, done, _ = lib.evolve_poll(0)
    finally:
        lib.clumping(0)
    g = lambda w: lib.grid_to_host(w, np.empty((N, N, N)))
    return niter, g(capi.GRID_XH_INTERMED), g(capi.GRID_XH_AV), g(capi.GRID_PHI_ION)


@pytest.mark.parametrize("uniform_T", [True, False])
@pytest.mark.parametrize("N", SIZES)
def test_fused_pass_ones_and_constant_are_bit_exact(asora, N, uniform_T):
    """The device loop (fused pass, uniform-temperature form or not): ones == off, C == bh00 C, iteration count included."""
    p, lib, capi = asora
    thin, _, dlog = _init(p, lib, N)
    pos, flux, n, xh = _loop_case(N, ns=1)
    lib.source_data_to_device(*cases.flat_sources(pos, flux), flux.shape[0])
    T = np.full((N, N, N), 1e4) if uniform_T else 10 ** np.random.default_rng(N).uniform(3.5, 4.5, (N, N, N))
    lib.grid_to_device(capi.GRID_NDENS, n)
    lib.grid_to_device(capi.GRID_TEMP, T)
    lib.grid_to_device(capi.GRID_CLUMP, np.ones((N, N, N)))
    dt, dr, R = 3.15576e13, 3.086e21 * 0.4, 12.0

    def step(bh00, mode=0, c=1.0):
        lib.grid_to_device(capi.GRID_XH, xh)
        return _device_step(lib, capi, N, (dt, bh00) + CHEM[1:], R, dr, dlog, thin.shape[0], flux.shape[0], mode, c)
    off = step(cases.BH00)
    assert off[0] > 1
    _same(step(cases.BH00), off)                                  # (the case repeats itself exactly)
    _same(step(cases.BH00, 2), off)
    const = step(cases.BH00, 1, 4.0)
    _same(const, step(4.0 * cases.BH00))
    assert not np.array_equal(const[1], off[1])


def test_device_loop_with_a_grid_equals_host_loop_of_isolated_calls(asora):
    p, lib, capi = asora
    N = 40
    thin, _, dlog = _init(p, lib, N)
    pos, flux, n, xh = _loop_case(N)
    lib.source_data_to_device(*cases.flat_sources(pos, flux), flux.shape[0])
    T = 10 ** np.random.default_rng(3).uniform(3.5, 4.5, (N, N, N))
    lib.grid_to_device(capi.GRID_NDENS, n)
    lib.grid_to_device(capi.GRID_TEMP, T)
    lib.grid_to_device(capi.GRID_CLUMP, _clump_grid(N, 9))
    dt, dr, R, conv_frac = 3.15576e13, 3.086e21 * 0.4, 12.0, 1e-4
    chem = (dt,) + CHEM
    lib.grid_to_device(capi.GRID_XH, xh)
    dev = _device_step(lib, capi, N, chem, R, dr, dlog, thin.shape[0], flux.shape[0], 2)
    lib.grid_to_device(capi.GRID_XH, xh)
    lib.grid_copy(capi.GRID_XH_AV, capi.GRID_XH)
    crit = min(int(conv_frac * N ** 3), (flux.shape[0] - 1) / 3)
    prev1 = prev0 = 2.0 * N ** 3
    niter, converged = 0, False
    lib.clumping(2)
    try:
        while not converged and niter < 100:
            niter += 1
            lib.raytrace_device(R, cases.SIG, dr, 0, flux.shape[0], cases.MINLOGTAU, dlog, thin.shape[0])
            conv, s1, s0 = lib.chemistry_device(*chem)
            rel1 = abs((s1 - prev1) / s1) if s1 > 0 else 1.0
            rel0 = abs((s0 - prev0) / s0) if s0 > 0 else 1.0
            converged = conv < crit or (rel1 < conv_frac and rel0 < conv_frac)
            prev1, prev0 = s1, s0
    finally:
        lib.clumping(0)
    g = lambda w: lib.grid_to_host(w, np.empty((N, N, N)))
    assert dev[0] == niter and niter > 1
    for a, b in zip(dev[1:], (g(capi.GRID_XH_INTERMED), g(capi.GRID_XH_AV), g(capi.GRID_PHI_ION))):
        np.testing.assert_allclose(a, b, rtol=1e-10, atol=0)


def _evolve(pc2r, c, use_gpu, clumping=None, bh00=cases.BH00, logfile=None, thermal=None):
    kw = {} if clumping is None else dict(clumping=clumping)
    if thermal is not None:
        kw["thermal"] = thermal
    out = pc2r.evolve3D(c["dt"], c["dr"], c["flux"], c["pos"], use_gpu, c["max_subbox"], c["subboxsize"], c["loss_fraction"],
                        c["temp"], c["ndens"], c["xh"], c["thin"], c["thick"], cases.MINLOGTAU, c["dlogtau"], c["R"],
                        c["convergence_fraction"], cases.SIG, bh00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C,
                        logfile=logfile, quiet=logfile is None, **kw)
    from pyc2ray_amd.evolve import _evolve as ev
    return (ev.last_niter,) + tuple(np.array(a) for a in out)


def _one_source(c):
    """the case's step with its sources merged into the first one (bit-exact runs, see the module docstring)"""
    c = dict(c)
    c["pos"], c["flux"] = c["pos"][:, :1], np.array([c["flux"].sum()])
    return c


@pytest.mark.parametrize("name", ["l16_gpu_F", "l16_cpu_F", "l24_gpu_F_37src"])
def test_evolve3D_step_ones_and_constant(asora, name, tmp_path):
    """Whole evolve3D steps (use_gpu=True and False): ones == off and C == bh00 C bit for bit; the log line appears only
    when clumping is on, and the library is left unclumped."""
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    c = _one_source(cases.evolve_case(name))
    N = c["N"]
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)
    p.photo_table_to_device(c["thin"], c["thick"])
    logs = {k: str(tmp_path / f"{k}.log") for k in ("off", "ones", "const")}
    off = _evolve(pc2r, c, c["use_gpu"], logfile=logs["off"])
    _same(_evolve(pc2r, c, c["use_gpu"]), off)                   # (the case repeats itself exactly)
    _same(_evolve(pc2r, c, c["use_gpu"], np.ones((N, N, N), order="F"), logfile=logs["ones"]), off)
    const = _evolve(pc2r, c, c["use_gpu"], 5.0, logfile=logs["const"])
    _same(const, _evolve(pc2r, c, c["use_gpu"], None, 5.0 * cases.BH00))
    assert not np.array_equal(const[1], off[1])
    _same(_evolve(pc2r, c, c["use_gpu"]), off)                     # (nothing carried into a call that did not ask)
    text = {k: open(v).read() for k, v in logs.items()}
    assert "Clumping factor" not in text["off"]
    assert "Clumping factor: grid, mean 1.000e+00" in text["ones"]
    assert "Clumping factor: constant 5.000e+00" in text["const"]
    assert text["off"].count("\n") + 1 == text["const"].count("\n")


def test_thermal_step_with_ones_is_the_thermal_step(asora):
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    from pyc2ray_amd.thermal import ThermalParams
    c = _one_source(cases.evolve_case("l16_gpu_F"))
    N = c["N"]
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)
    p.photo_table_to_device(c["thin"], c["thick"])
    th = ThermalParams(c["heat_thin"], c["heat_thick"])
    off = _evolve(pc2r, c, True, thermal=th)
    _same(_evolve(pc2r, c, True, thermal=th), off)
    _same(_evolve(pc2r, c, True, np.ones((N, N, N)), thermal=th), off)
    clumped = _evolve(pc2r, c, True, 6.0, thermal=th)
    assert clumped[0] >= 1 and not np.array_equal(clumped[1], off[1])


@pytest.mark.parametrize("mode", [1, 2])
def test_thermal_pass_with_clumping_matches_the_reference(asora, mode):
    """The isolated thermal pass, clumped (recombination rate and recombination cooling), against the numpy statement."""
    p, lib, capi = asora
    N = 24
    _init(p, lib, N)
    n, T, xh, xav, gamma = _cells(N, 77)
    heat = gamma * 10 ** np.random.default_rng(78).uniform(-12, -10.5, (N, N, N))
    clump = _clump_grid(N, 79) if mode == 2 else 6.0
    dt = 1e11
    prm = TR.Params(relative_denergy=0.1, t_floor=1.0, max_substeps=400, cooling_mask=31, compton=True, t_cmb=2.7255 * 11.0)
    _upload(lib, capi, n, T, xh, xav, gamma)
    lib.grid_to_device(capi.GRID_PHI_HEAT, heat)
    if mode == 2:
        lib.grid_to_device(capi.GRID_CLUMP, clump)
    lib.thermal_params(True, prm.relative_denergy, prm.t_floor, prm.max_substeps, prm.cooling_mask, prm.compton, prm.t_cmb)
    lib.clumping(mode, 6.0)
    try:
        conv, s1, _ = lib.chemistry_device(dt, *CHEM)
    finally:
        lib.clumping(0)
        lib.thermal_params(False)
    g = lambda w: lib.grid_to_host(w, np.empty((N, N, N)))
    xi, xa, te = g(capi.GRID_XH_INTERMED), g(capi.GRID_XH_AV), g(capi.GRID_TEMP_END)
    rxi, rxa, rte, rconv, delta, capped = CR.chemistry_thermal(prm, dt, n, T, xh, xav, gamma, heat, *CHEM, clump)
    well = (delta > WELL_CONDITIONED) & ~capped
    assert well.sum() > 1000
    for got, ref, loose in ((xi, rxi, ILL_RTOL), (xa, rxa, ILL_RTOL_XAV), (te, rte, ILL_RTOL)):
        np.testing.assert_allclose(got[well], ref[well], rtol=1e-10, atol=0)
        np.testing.assert_allclose(got, ref, rtol=loose, atol=0)
    assert conv == rconv


def _stroemgren_params(path, clumping):
    base = open(BB_PARAMS).read()
    # 13.2 kpc box, n = 1e-3, 10^4 K, a soft 2e4 K black body (a sharp front), R_max = half the box
    base = (base.replace("boxsize: 0.014", "boxsize: 0.0132").replace("avg_dens: 1.0e-6", "avg_dens: 1.0e-3")
                .replace("Teff: 5e4", "Teff: 2e4").replace("R_max_cMpc: 0.01640625", "R_max_cMpc: 0.0066")
                .replace("zred_0: 9.0", "zred_0: 0.0").replace("NumTau: 10000", "NumTau: 2000")
                .replace("Material:\n", f"Material:\n  clumping: {clumping}\n"))
    with open(path, "w") as f:
        f.write(base)
    return path


def test_stroemgren_volume_scales_with_one_over_clumping(asora, tmp_path):
    """One source, uniform isothermal medium, run to equilibrium: Q = C alpha_B n_e n_H V."""
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        vol = {}
        for C in (1, 8):
            if p.cuda_is_init():
                p.device_close()
            sim = pc2r.C2Ray_Test(_stroemgren_params(f"parameters_{C}.yml", C), 64, True)
            assert sim.clumping == float(C) and not sim.cosmological
            sim.density_init(0.0)
            with open("source.txt", "w") as f:
                f.write("1\n33 33 33 5e48 1.0\n")
            srcpos, srcflux = sim.read_sources("source.txt", 1)
            alpha, n = sim.bh00, 1e-3
            t_rec = 1.0 / (C * alpha * n)
            for _ in range(3):
                sim.evolve3D(10 * t_rec, srcflux, srcpos)
            x, phi = np.asarray(sim.xh), np.asarray(sim.phi_ion)
            dV = sim.dr ** 3
            # photons absorbed per second (the raytrace conserves them), and the volume whose recombinations balance them:
            # sum C alpha n_e n_HII dV = Q, i.e. V = sum x (x + abu_c) dV = Q / (C alpha n^2)
            q_abs = np.sum(phi * n * (1.0 - x)) * dV
            vol[C] = np.sum(x * (x + cases.ABU_C)) * dV
            expect = 5e48 / (C * alpha * n * n)
            print(f"C = {C}: Q_abs / Q = {q_abs / 5e48:.4f}, sum x (x + abu_c) dV / V_S = {vol[C] / expect:.4f}, "
                  f"sum x dV / V_S = {x.sum() * dV / expect:.4f}")
            assert q_abs == pytest.approx(5e48, rel=0.05)
            assert vol[C] == pytest.approx(expect, rel=0.05), (C, vol[C] / expect)
            assert x[0, 0, 0] < 1e-2                               # the sphere lies inside the box
        assert vol[1] / vol[8] == pytest.approx(8.0, rel=0.03)
    finally:
        if p.cuda_is_init():
            p.device_close()
        os.chdir(cwd)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


@pytest.mark.parametrize("exchange", ["slab", "allreduce"])
def test_two_ranks_with_a_clumping_grid(asora, tmp_path, exchange):
    """evolve3D_MPI with a clumping grid on two ranks sharing GPU 0 over gloo: identical grids on every rank, and the
    single-GPU evolve3D to 1e-10."""
    p, lib, capi = asora
    if p.cuda_is_init():
        p.device_close()
    world, port = 2, _free_port()
    outs = [str(tmp_path / f"r{r}.npz") for r in range(world)]
    env = dict(os.environ, PYC2RAY_AMD_NO_TORCH="0", OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_clumping_dist_worker.py"), str(r), str(world), port, outs[r],
                               exchange], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = [q.communicate(timeout=300)[0].decode() for q in procs]
    for q, log in zip(procs, logs):
        assert q.returncode == 0, log
    res = [np.load(o) for o in outs]
    assert np.array_equal(res[0]["xh"], res[1]["xh"]) and np.array_equal(res[0]["phi"], res[1]["phi"])
    assert int(res[0]["niter"]) == int(res[1]["niter"])
    import _clumping_dist_worker as W
    import pyc2ray_amd as pc2r
    c = W.case()
    p.device_init(c["N"], 8)
    p.photo_table_to_device(c["thin"], c["thick"])
    single = _evolve(pc2r, c, True, c["clump"])
    assert int(res[0]["niter"]) == single[0]
    np.testing.assert_allclose(res[0]["xh"], single[1], rtol=1e-10, atol=0)
    np.testing.assert_allclose(res[0]["phi"], single[2], rtol=1e-10, atol=0)
    off = _evolve(pc2r, c, True)
    assert not np.allclose(off[1], single[1], rtol=1e-3)


def _class_params(path):
    base = open(BB_PARAMS).read().replace("NumTau: 10000", "NumTau: 2000").replace("Material:\n", "Material:\n  clumping: 4\n")
    with open(path, "w") as f:
        f.write(base)
    return path


def test_resident_and_host_class_runs_agree(asora, tmp_path):
    """C2Ray_Test with `Material: clumping: 4`, two steps, then `sim.clumping = grid` between steps: the device-resident
    run against device_resident = False."""
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 24
        _class_params("parameters.yml")
        with open("src.txt", "w") as f:
            f.write("2\n12 12 12 6e50 1.0\n5 20 9 2e50 1.0\n")
        grid = _clump_grid(N, 41)
        runs = {}
        for resident in (True, False):
            if p.cuda_is_init():
                p.device_close()
            sim = pc2r.C2Ray_Test("parameters.yml", N, True)
            sim.device_resident = resident
            assert sim.clumping == 4.0
            sim.density_init(0.0)
            srcpos, srcflux = sim.read_sources("src.txt", 2)
            dt = 3.15576e13
            xs = []
            for step in range(5):
                if step == 2:
                    sim.clumping = grid
                if step == 4:
                    sim.clumping = 2.0 * sim.clumping         # (a read and an assignment: uploaded again)
                sim.evolve3D(dt, srcflux, srcpos)
                xs.append(np.array(sim.xh))
            runs[resident] = xs
        for a, b in zip(runs[True], runs[False]):
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)
        assert not np.allclose(runs[True][1], runs[True][2], rtol=1e-3)
    finally:
        if p.cuda_is_init():
            p.device_close()
        os.chdir(cwd)
