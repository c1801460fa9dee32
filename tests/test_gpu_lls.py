"""GPU: Lyman-limit-system opacity -- asora_lls_opacity and the ``lls=`` keyword -- against the CPU oracle
with the substitution of tests/lls_reference.py: the oracle's raytrace is given the absorber density n_abs as its density and
xh_av = 0, the chemistry the real density.  The tolerances are those of the tests without the feature (tests/test_gpu_parity.py:
GAMMA_RTOL for a raytrace, 1e-8 / 1e-7 for a step, the thermal step included, and 1e-10 in its well-conditioned cells)."""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import cases
import lls_reference as LR
from oracle import oracle as O
from test_gpu_parity import GAMMA_RTOL

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LLS_PARAMS = os.path.join(HERE, "data", "parameters_lls.yml")
CHEM = (cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)
RT_NAMES = ("l16_7src_R5.5", "l17_3src_Rbox", "l32_5src_R10")
# the thermal pass against its numpy statement (tests/test_gpu_thermal.py, tests/test_gpu_clumping.py): 1e-10 where delth dt >
# WELL_CONDITIONED and the integration did not hit max_substeps
WELL_CONDITIONED = 1e-2


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib, _capi
    lib.lls_opacity(0.0, 0.0)
    if p.cuda_is_init():
        for opt in (_capi.OPT_FORTRAN_CONSTANTS, _capi.OPT_PAIR_SOURCES, _capi.OPT_GLOBAL_ATOMICS):
            lib.set_option(opt, 0)
        lib.thermal_params(False)
        p.device_close()


def _ab(c, which):
    """(a, b) of a case: `a` worth an optical depth of 0.05 per cell -- comparable to a cell's own (0.05 ... 0.10 in these cases)
    -- and `b` half an absorber per atom."""
    a = 0.05 / (c["sig"] * c["dr"])
    return {"a": (a, 0.0), "b": (0.0, 0.5), "ab": (a, 0.5), "off": (0.0, 0.0)}[which]


@functools.lru_cache(maxsize=None)
def _rt_reference(name, which, fortran):
    c = cases.rt_case(name, "soft")
    pos0, flux = cases.flat_sources(c["pos"], c["flux"])
    a, b = _ab(c, which)
    ref = LR.raytrace(c["R"], c["sig"], c["dr"], c["ndens"], c["xh"], pos0, flux, c["thin"], c["thick"], c["minlogtau"], c["dlogtau"],
                      a, b, NumTau=c["thin"].shape[0] - 1, flags=O.PER_SOURCE_FLUX if fortran else O.ASORA_MODE)["phi_ion"]
    ref.setflags(write=False)
    return ref


def _setup(p, lib, capi, c, xh=None):
    N = c["N"]
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)
    p.photo_table_to_device(c["thin"], c["thick"])
    pos0, flux = cases.flat_sources(c["pos"], c["flux"])
    lib.source_data_to_device(pos0, flux, flux.shape[0])
    lib.grid_to_device(capi.GRID_NDENS, c["ndens"])
    lib.grid_to_device(capi.GRID_XH_AV, c["xh"] if xh is None else xh)
    return pos0, flux


def _trace(lib, capi, c, nsrc=None):
    N = c["N"]
    lib.raytrace_device(c["R"], c["sig"], c["dr"], 0, c["flux"].shape[0] if nsrc is None else nsrc, c["minlogtau"], c["dlogtau"],
                        c["thin"].shape[0] - 1)
    return lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))


@pytest.mark.parametrize("which", ["a", "b", "ab"])
@pytest.mark.parametrize("name", RT_NAMES)
def test_raytrace_with_lls_matches_the_substituted_oracle(asora, name, which):
    """asora_raytrace_device: both sets of constants, the single-source and the paired sweep, buffer and global atomics."""
    p, lib, capi = asora
    c = cases.rt_case(name, "soft")
    _setup(p, lib, capi, c)
    a, b = _ab(c, which)
    lib.lls_opacity(a, b)
    assert lib.get_lls_opacity() == (a, b)
    try:
        off = _rt_reference(name, "off", 0)
        for fortran in (0, 1):
            ref = _rt_reference(name, which, fortran)
            assert np.isfinite(ref).all() and not np.allclose(ref, off, rtol=1e-2, atol=0)
            lib.set_option(capi.OPT_FORTRAN_CONSTANTS, fortran)
            for pairs in (1, 2):
                for global_atomics in (0, 1):
                    lib.set_option(capi.OPT_PAIR_SOURCES, pairs)
                    lib.set_option(capi.OPT_GLOBAL_ATOMICS, global_atomics)
                    phi = _trace(lib, capi, c)
                    v = lib.last_raytrace_variant()
                    tag = str((name, which, fortran, pairs, global_atomics))
                    print(tag, "max rel. difference", np.max(np.abs(phi - ref)[ref != 0] / ref[ref != 0]), "paired", v["paired"],
                          "buffer atomics", v["buffer_atomics"])
                    assert not (v["paired"] and pairs == 1) and not (v["buffer_atomics"] and global_atomics), (tag, v)
                    assert np.array_equal(phi != 0, ref != 0), tag
                    np.testing.assert_allclose(phi, ref, rtol=GAMMA_RTOL, atol=0, err_msg=tag)
    finally:
        lib.lls_opacity(0.0, 0.0)
        for opt in (capi.OPT_FORTRAN_CONSTANTS, capi.OPT_PAIR_SOURCES, capi.OPT_GLOBAL_ATOMICS):
            lib.set_option(opt, 0)


@pytest.mark.parametrize("use_gpu", [True, False])
def test_do_raytracing_keyword(asora, use_gpu, tmp_path):
    """do_raytracing(lls=...): the ASORA path against the substituted oracle, the use_gpu=False path against the substituted
    sub-box oracle; the log line; the library left without LLS opacity."""
    p, lib, capi = asora
    from pyc2ray_amd.lls import LLSOpacity
    c = cases.rt_case("l16_7src_R5.5", "soft")
    N = c["N"]
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)
    p.photo_table_to_device(c["thin"], c["thick"])
    a, b = _ab(c, "ab")
    R = c["R"] if use_gpu else 1000.0          # (the sub-box cases of tests/cases.py: R beyond the box)
    log = str(tmp_path / "log")
    out = p.do_raytracing(c["dr"], c["flux"], c["pos"], use_gpu, 1000, 3, 1e-2, np.asfortranarray(c["ndens"]),
                          np.asfortranarray(c["xh"]), c["thin"], c["thick"], np.zeros_like(c["thin"]), np.zeros_like(c["thin"]),
                          c["minlogtau"], c["dlogtau"], R, c["sig"], logfile=log, quiet=True, lls=LLSOpacity(a, b))
    assert lib.get_lls_opacity() == (0.0, 0.0)
    assert "LLS opacity: n_const" in open(log).read()
    if use_gpu:
        pos0, flux = cases.flat_sources(c["pos"], c["flux"])
        ref = LR.raytrace(R, c["sig"], c["dr"], c["ndens"], c["xh"], pos0, flux, c["thin"], c["thick"], c["minlogtau"], c["dlogtau"],
                          a, b, NumTau=c["thin"].shape[0])["phi_ion"]
        np.testing.assert_allclose(out[0], ref, rtol=GAMMA_RTOL, atol=0)
    else:
        ref = O.do_all_sources(c["flux"], c["pos"], 1000, 3, c["sig"], c["dr"], LR.n_abs(c["ndens"], c["xh"], a, b), np.zeros((N, N, N)),
                               1e-2, c["thin"], c["thick"], c["minlogtau"], c["dlogtau"], R)["phi_ion"]
        np.testing.assert_allclose(out[0], ref, rtol=1e-7, atol=1e-14 * ref.max())     # (tests/test_gpu_subbox.py: _close)
    plain = p.do_raytracing(c["dr"], c["flux"], c["pos"], use_gpu, 1000, 3, 1e-2, np.asfortranarray(c["ndens"]),
                            np.asfortranarray(c["xh"]), c["thin"], c["thick"], np.zeros_like(c["thin"]), np.zeros_like(c["thin"]),
                            c["minlogtau"], c["dlogtau"], R, c["sig"], logfile=log, quiet=True)
    assert np.all(np.asarray(out[0]) <= np.asarray(plain[0])) and not np.allclose(out[0], plain[0], rtol=1e-2, atol=0)


def test_fully_ionised_patch_has_finite_rates_with_uniform_absorbers(asora):
    """x = 1 exactly in a block of cells: without LLS such a cell's rate is NaN (nHI = 0, as in the reference); with a > 0 it still
    has absorbers, and every rate is finite and the oracle's."""
    p, lib, capi = asora
    c = cases.rt_case("l16_7src_R5.5", "soft")
    N = c["N"]
    xh = c["xh"].copy()
    s = c["pos"][:, 0] - 1                               # a block around (and including) the first source, periodic
    idx = [np.arange(s[ax] - 1, s[ax] + 3) % N for ax in range(3)]
    xh[np.ix_(*idx)] = 1.0
    pos0, flux = _setup(p, lib, capi, c, xh=xh)
    assert not np.isfinite(_trace(lib, capi, c)).all()    # (the corner this feature removes)
    a, _ = _ab(c, "a")
    lib.lls_opacity(a, 0.0)
    try:
        phi = _trace(lib, capi, c)
    finally:
        lib.lls_opacity(0.0, 0.0)
    ref = LR.raytrace(c["R"], c["sig"], c["dr"], c["ndens"], xh, pos0, flux, c["thin"], c["thick"], c["minlogtau"], c["dlogtau"],
                      a, 0.0, NumTau=c["thin"].shape[0] - 1)["phi_ion"]
    assert np.isfinite(phi).all() and np.isfinite(ref).all()
    assert np.all(phi[np.ix_(*idx)] > 0)
    np.testing.assert_allclose(phi, ref, rtol=GAMMA_RTOL, atol=0)


@pytest.mark.parametrize("name", RT_NAMES)
def test_zeros_are_off_bit_for_bit_and_absorbers_only_lower_the_rates(asora, name):
    p, lib, capi = asora
    c = cases.rt_case(name, "soft")
    N = c["N"]
    one = dict(c, pos=c["pos"][:, :1], flux=c["flux"][:1])    # (one source: no two atomics meet in a cell, a trace repeats itself)
    _setup(p, lib, capi, one)
    never = _trace(lib, capi, one)
    assert np.array_equal(_trace(lib, capi, one), never)
    lib.lls_opacity(0.0, 0.0)
    assert np.array_equal(_trace(lib, capi, one), never)
    try:
        lib.lls_opacity(1e-3, 0.1)
        assert not np.array_equal(_trace(lib, capi, one), never)
        lib.lls_opacity(0.0, 0.0)
        assert np.array_equal(_trace(lib, capi, one), never)      # (nothing carried over)
        # all sources: Gamma(tau) falls and is convex, so more absorbers in front of and inside a cell lower its rate per absorber
        _setup(p, lib, capi, c)
        off = _trace(lib, capi, c)
        near = np.zeros((N, N, N), dtype=bool)
        for s in (c["pos"] - 1).T:
            near[np.ix_(*[np.arange(s[ax] - 1, s[ax] + 2) % N for ax in range(3)])] = True
        for which in ("a", "b", "ab"):
            lib.lls_opacity(*_ab(c, which))
            on = _trace(lib, capi, c)
            assert np.array_equal(on != 0, off != 0)
            assert np.all(on <= off), which
            far = ~near & (off != 0)
            assert far.sum() > 100 and np.all(on[far] < off[far]), which
    finally:
        lib.lls_opacity(0.0, 0.0)


def test_state_codes_and_lifetime(asora):
    """Code 3 for bad values, code 4 under grey opacity (setting it, and tracing with both on); device_init resets the state."""
    p, lib, capi = asora
    c = cases.rt_case("l16_7src_R5.5", "soft")
    _setup(p, lib, capi, c)
    for bad in ((-1.0, 0.0), (0.0, -1.0), (float("nan"), 0.0), (0.0, float("inf"))):
        with pytest.raises(RuntimeError, match="code 3"):
            lib.lls_opacity(*bad)
    lib.set_option(capi.OPT_GREY_NOTABLES, 1)
    try:
        with pytest.raises(RuntimeError, match="code 4"):
            lib.lls_opacity(1e-4, 0.0)
        lib.set_option(capi.OPT_GREY_NOTABLES, 0)
        lib.lls_opacity(1e-4, 0.0)
        lib.set_option(capi.OPT_GREY_NOTABLES, 1)
        with pytest.raises(RuntimeError, match="code 4"):
            _trace(lib, capi, c)
    finally:
        lib.set_option(capi.OPT_GREY_NOTABLES, 0)
    assert lib.get_lls_opacity() == (1e-4, 0.0)
    _setup(p, lib, capi, c)                                   # device_close + device_init
    assert lib.get_lls_opacity() == (0.0, 0.0)


def test_column_density_accumulates_the_lls_opacity(asora):
    """asora_debug_coldens: the column density through n_abs, against the oracle's with the substitution."""
    p, lib, capi = asora
    c = cases.rt_case("l17_3src_Rbox", "soft")
    N = c["N"]
    pos0, flux = _setup(p, lib, capi, c)
    a, b = _ab(c, "ab")
    lib.lls_opacity(a, b)
    try:
        cd = lib.debug_coldens(c["R"], c["sig"], c["dr"], flux.shape[0] - 1, N)
    finally:
        lib.lls_opacity(0.0, 0.0)
    ref = LR.raytrace(c["R"], c["sig"], c["dr"], c["ndens"], c["xh"], pos0, flux, c["thin"], c["thick"], c["minlogtau"], c["dlogtau"],
                      a, b, NumTau=c["thin"].shape[0] - 1, want_coldens=True)["coldens"]
    w = cd != 0
    assert w.sum() > 0
    np.testing.assert_allclose(cd[w], ref[w], rtol=1e-12)


# ---- whole steps ----------------------------------------------------------------------------------------------------------
def _step_case():
    """N = 16, seven sources, a = tau 0.05 per cell and b = 0.2: six outer iterations, 170 cells beyond x = 0.5 (255 without LLS)."""
    N = 16
    nd, xh, dr = cases.grid(N, "lognormal", 61, 0.2, xlo=1e-4, xhi=2e-3)
    pos, flux = cases.sources(N, 7, 62, flux=6e-5)
    thin, thick, dlog = cases.soft_tables()
    n = thin.shape[0]
    return dict(N=N, ndens=nd, xh=xh, dr=dr, temp=np.full((N, N, N), 1e4), pos=pos, flux=flux, thin=thin, thick=thick, dlogtau=dlog,
                R=5.5, dt=2 * cases.MYR, conv=1e-4, a=0.05 / (cases.SIG * dr), b=0.2,
                heat_thin=1e-11 * thin * np.linspace(1.0, 2.0, n), heat_thick=0.7e-11 * thick * np.linspace(2.0, 1.0, n))


def _evolve(p, c, use_gpu=True, lls=None, logfile=None, thermal=None, R=None, subboxsize=None):
    kw = {} if lls is None else dict(lls=lls)
    if thermal is not None:
        kw["thermal"] = thermal
    out = p.evolve3D(c["dt"], c["dr"], c["flux"], c["pos"], use_gpu, 1000, subboxsize or c["N"], 1e-2, c["temp"], c["ndens"], c["xh"],
                     c["thin"], c["thick"], cases.MINLOGTAU, c["dlogtau"], c["R"] if R is None else R, c["conv"], cases.SIG, *CHEM,
                     logfile=logfile, quiet=True, **kw)
    return (p.evolve._evolve.last_niter,) + tuple(np.array(a) for a in out)


def _fresh(p, c):
    if p.cuda_is_init():
        p.device_close()
    p.device_init(c["N"], 8)
    p.photo_table_to_device(c["thin"], c["thick"])


def test_evolve3D_with_lls_matches_the_substituted_oracle_loop(asora, tmp_path):
    p, lib, capi = asora
    from pyc2ray_amd.lls import LLSOpacity
    c = _step_case()
    _fresh(p, c)
    log = str(tmp_path / "log")
    niter, x, phi = _evolve(p, c, lls=LLSOpacity(c["a"], c["b"]), logfile=log)
    x_ref, phi_ref, niter_ref, _ = LR.evolve3D_lls_oracle(c["a"], c["b"], c["dt"], c["dr"], c["flux"], c["pos"], c["temp"], c["ndens"],
                                                          c["xh"], c["thin"], c["thick"], cases.MINLOGTAU, c["dlogtau"], c["R"],
                                                          c["conv"], cases.SIG, *CHEM)
    print("niter", niter, niter_ref, "max rel. difference x", np.max(np.abs(x - x_ref) / x_ref), "phi",
          np.max(np.abs(phi - phi_ref)[phi_ref != 0] / phi_ref[phi_ref != 0]))
    assert niter == niter_ref and niter >= 2
    np.testing.assert_allclose(x, x_ref, rtol=1e-8, atol=0)
    np.testing.assert_allclose(phi, phi_ref, rtol=1e-7, atol=0)
    assert x.max() > 0.5
    assert lib.get_lls_opacity() == (0.0, 0.0)
    text = open(log).read()
    assert f"LLS opacity: n_const {c['a']:.3e} cm^-3, per_density 2.000e-01" in text
    # off: the step without the feature, and its log without the line
    log_off = str(tmp_path / "off")
    off = _evolve(p, c, logfile=log_off)
    text_off = open(log_off).read()
    assert "LLS" not in text_off
    head = lambda t: t[:t.index("Convergence Criterion")]          # (the iteration counts differ: compare the headers)
    assert head(text).replace(f"LLS opacity: n_const {c['a']:.3e} cm^-3, per_density 2.000e-01\n", "") == head(text_off)
    assert off[1].mean() > 1.2 * x.mean()                           # the sink slows the fronts down
    zeros = _evolve(p, c, lls=LLSOpacity(0.0, 0.0))
    assert zeros[0] == off[0]
    np.testing.assert_allclose(zeros[1], off[1], rtol=1e-10, atol=0)   # (seven sources: the order of the atomics is free)


def test_thermal_evolve3D_with_lls(asora):
    p, lib, capi = asora
    import thermal_reference as TR
    from pyc2ray_amd.lls import LLSOpacity
    from pyc2ray_amd.thermal import ThermalParams
    c = _step_case()
    _fresh(p, c)
    prm = TR.Params(relative_denergy=0.1, t_floor=1.0, max_substeps=10000, cooling_mask=31, compton=False, t_cmb=0.0)
    tp = ThermalParams(c["heat_thin"], c["heat_thick"], relative_denergy=0.1, t_floor=1.0, max_substeps=10000, cooling=31, zred=None)
    niter, x, phi, T = _evolve(p, c, lls=LLSOpacity(c["a"], c["b"]), thermal=tp)
    heat = lib.grid_to_host(capi.GRID_PHI_HEAT, np.empty((c["N"],) * 3))
    x_ref, T_ref, phi_ref, heat_ref, niter_ref, delta, capped = LR.evolve3D_lls_thermal_oracle(
        c["a"], c["b"], prm, c["dt"], c["dr"], c["flux"], c["pos"], c["temp"], c["ndens"], c["xh"], c["thin"], c["thick"],
        c["heat_thin"], c["heat_thick"], cases.MINLOGTAU, c["dlogtau"], c["R"], c["conv"], cases.SIG, *CHEM)
    rel = lambda g, r: np.max(np.abs(g - r)[r != 0] / np.abs(r[r != 0]))
    print("niter", niter, niter_ref, "max rel. difference x", rel(x, x_ref), "T", rel(T, T_ref), "phi", rel(phi, phi_ref), "heat",
          rel(heat, heat_ref))
    assert niter == niter_ref and niter >= 2
    well = (delta > WELL_CONDITIONED) & ~capped
    assert well.sum() > 100
    for got, ref in ((x, x_ref), (T, T_ref)):
        np.testing.assert_allclose(got[well], ref[well], rtol=1e-10, atol=0)
        np.testing.assert_allclose(got, ref, rtol=1e-8, atol=0)          # (every cell: no ill-conditioned one in this case)
    for got, ref in ((phi, phi_ref), (heat, heat_ref)):
        assert np.array_equal(got != 0, ref != 0)
        np.testing.assert_allclose(got, ref, rtol=1e-7, atol=0)
    assert T.max() > 1.05e4 and T_ref.max() > 1.05e4 and lib.get_lls_opacity() == (0.0, 0.0)


def test_cpu_semantics_evolve3D_with_lls(asora):
    """use_gpu=False: the sub-box loop against the sub-box oracle with the substitution (tests/test_gpu_subbox.py's bounds)."""
    p, lib, capi = asora
    from pyc2ray_amd.lls import LLSOpacity
    c = _step_case()
    c = dict(c, temp=np.asfortranarray(c["temp"]), ndens=np.asfortranarray(c["ndens"]), xh=np.asfortranarray(c["xh"]))
    _fresh(p, c)
    niter, x, phi = _evolve(p, c, use_gpu=False, lls=LLSOpacity(c["a"], c["b"]), R=1000.0, subboxsize=3)
    x_ref, phi_ref, niter_ref = LR.evolve3d_lls_cpu_path(c["a"], c["b"], c["dt"], c["dr"], c["flux"], c["pos"], 1000, 3, 1e-2, c["temp"],
                                                         c["ndens"], c["xh"], c["thin"], c["thick"], cases.MINLOGTAU, c["dlogtau"],
                                                         1000.0, c["conv"], cases.SIG, *CHEM)
    print("niter", niter, niter_ref, "max rel. difference x", np.max(np.abs(x - x_ref) / x_ref))
    assert niter == niter_ref and niter >= 2
    np.testing.assert_allclose(x, x_ref, rtol=1e-7)
    np.testing.assert_allclose(phi, phi_ref, rtol=1e-7, atol=1e-14 * np.max(np.abs(phi_ref)))
    assert lib.get_lls_opacity() == (0.0, 0.0)


@pytest.mark.parametrize("N", [17, 40])
def test_fused_pass_and_prepare_form_the_same_absorber_density(asora, N):
    """One iteration of the device loop, xh_av downloaded; the second iteration traces through the nHI the fused pass emitted, a
    fresh asora_raytrace_device from that xh_av through prepare_nhi's: the same rates, bit for bit (one source: no two atomics meet
    in a cell).  N = 17: one tile, odd; N = 40: more than one tile of 32."""
    p, lib, capi = asora
    nd, xh, dr = cases.grid(N, "lognormal", 80 + N, 0.2, xlo=1e-4, xhi=2e-3)
    thin, thick, dlog = cases.soft_tables()
    pos, flux = np.array([[N // 2], [N // 3 + 1], [N - 2]]), np.array([4e-4 * (N / 16.0) ** 3])
    c = dict(N=N, ndens=nd, xh=xh, dr=dr, thin=thin, thick=thick, pos=pos, flux=flux)
    _fresh(p, c)
    lib.source_data_to_device(*cases.flat_sources(pos, flux), 1)
    for which, g in ((capi.GRID_NDENS, nd), (capi.GRID_TEMP, np.full((N, N, N), 1e4)), (capi.GRID_XH, xh)):
        lib.grid_to_device(which, g)
    a, b, R, numtau = 0.05 / (cases.SIG * dr), 0.2, 0.45 * N, thin.shape[0]
    grid = lambda w: lib.grid_to_host(w, np.empty((N, N, N)))
    lib.lls_opacity(a, b)
    try:
        lib.evolve_begin(2 * cases.MYR, *CHEM, R, cases.SIG, dr, cases.MINLOGTAU, dlog, numtau, 0, 1, 0.0, 1e-4)
        lib.evolve_enqueue(1)
        niter, done, _ = lib.evolve_poll(0)
        assert (niter, bool(done)) == (1, False)
        xh_av = grid(capi.GRID_XH_AV)
        assert xh_av.max() > 0.5 and not np.array_equal(xh_av, xh)
        lib.evolve_enqueue(1)
        niter, _, _ = lib.evolve_poll(0)
        assert niter == 2
        from_fused = grid(capi.GRID_PHI_ION)
        lib.grid_to_device(capi.GRID_XH_AV, xh_av)
        lib.raytrace_device(R, cases.SIG, dr, 0, 1, cases.MINLOGTAU, dlog, numtau)
        from_prepare = grid(capi.GRID_PHI_ION)
        assert np.array_equal(from_fused, from_prepare)
        lib.lls_opacity(0.0, 0.0)
        lib.raytrace_device(R, cases.SIG, dr, 0, 1, cases.MINLOGTAU, dlog, numtau)
        assert not np.array_equal(grid(capi.GRID_PHI_ION), from_prepare)
    finally:
        lib.lls_opacity(0.0, 0.0)


# ---- across ranks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", ["slab", "allreduce"])
def test_world1_rccl_step_with_lls_equals_the_one_gpu_loop(asora, tmp_path, monkeypatch, exchange):
    """The sharded and the all-reduce device loop over backend nccl (= RCCL) on one rank, as tests/test_gpu_parity.py drives them,
    with the LLS state set: same iteration count as evolve3D(lls=...), fields to 1e-10."""
    import torch.distributed as dist
    from pyc2ray_amd import dist as pd
    from pyc2ray_amd.lls import LLSOpacity
    from pyc2ray_amd.utils.sourceutils import format_sources
    p, lib, capi = asora
    monkeypatch.setenv("PYC2RAY_AMD_FORCE_COLLECTIVE", "1")
    c = _step_case()
    N, ns = c["N"], c["flux"].shape[0]
    _fresh(p, c)
    if not dist.is_initialized():
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        pd.init_process_group_from_env("nccl")
    n1, x1, phi1 = _evolve(p, c, lls=LLSOpacity(c["a"], c["b"]))
    n_off = _evolve(p, c)
    assert not np.allclose(n_off[1], x1, rtol=1e-3)
    comm = pd.TorchComm()
    comm.exchange = exchange
    pos, flux = c["pos"], c["flux"]
    plan = None
    if exchange == "slab":
        pos, flux, _ = comm.shard_sources_by_slab(c["pos"], c["flux"], 1)
        plan = pd.SlabPlan(N, 1, c["R"], [pos[0] - 1])
    lib.source_data_to_device(*format_sources(pos, flux), ns)
    for which, g in ((capi.GRID_NDENS, c["ndens"]), (capi.GRID_TEMP, c["temp"]), (capi.GRID_XH, c["xh"])):
        lib.grid_to_device(which, g)
    lib.grid_copy(capi.GRID_XH_AV, capi.GRID_XH)
    lib.grid_copy(capi.GRID_XH_INTERMED, capi.GRID_XH)
    chem = (c["dt"],) + CHEM
    crit = min(int(c["conv"] * N ** 3), (ns - 1) / 3)
    lib.lls_opacity(c["a"], c["b"])
    try:
        args = (N, c["R"], cases.SIG, c["dr"], ns, cases.MINLOGTAU, c["dlogtau"], c["thin"].shape[0], chem, crit, c["conv"])
        if exchange == "slab":
            comm.slab_begin(lib, plan, *args)
        else:
            comm.reduce_begin(lib, *args)
        done, n2 = False, 0
        while not done:
            comm.slab_enqueue(lib, 8)
            n2, done, _ = comm.slab_poll(lib, 8)
            assert n2 < 100
    finally:
        lib.lls_opacity(0.0, 0.0)
    x2 = lib.grid_to_host(capi.GRID_XH_INTERMED, np.empty((N, N, N)))
    phi2 = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
    assert n2 == n1
    np.testing.assert_allclose(x2, x1, rtol=1e-10, atol=0)
    np.testing.assert_allclose(phi2, phi1, rtol=1e-10, atol=0)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def test_two_ranks_with_lls_on_every_loop(asora, tmp_path):
    """evolve3D_MPI(lls=...) on two ranks sharing GPU 0 over gloo, through the slab, all-reduce, pipelined and three-call loops
    in one pair of processes: identical grids on both ranks, and the single-GPU evolve3D(lls=...) to 1e-10."""
    p, lib, capi = asora
    if p.cuda_is_init():
        p.device_close()
    world, port = 2, _free_port()
    outs = [str(tmp_path / f"r{r}.npz") for r in range(world)]
    env = dict(os.environ, PYC2RAY_AMD_NO_TORCH="0", OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_lls_dist_worker.py"), str(r), str(world), port, outs[r]],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = [q.communicate(timeout=300)[0].decode() for q in procs]
    for q, log in zip(procs, logs):
        assert q.returncode == 0, log
    res = [np.load(o) for o in outs]
    import _lls_dist_worker as W
    c = W.case()
    c["conv"] = c["convergence_fraction"]
    _fresh(p, c)
    single = _evolve(p, c, lls=c["lls"])
    off = _evolve(p, c)
    assert not np.allclose(off[1], single[1], rtol=1e-3)
    for loop in W.LOOPS:
        for k in ("xh", "phi"):
            assert np.array_equal(res[0][f"{loop}_{k}"], res[1][f"{loop}_{k}"]), (loop, k)
        assert int(res[0][f"{loop}_niter"]) == int(res[1][f"{loop}_niter"]) == single[0], loop
        np.testing.assert_allclose(res[0][f"{loop}_xh"], single[1], rtol=1e-10, atol=0, err_msg=loop)
        np.testing.assert_allclose(res[0][f"{loop}_phi"], single[2], rtol=1e-10, atol=0, err_msg=loop)


# ---- the simulation class -------------------------------------------------------------------------------------------------
def test_c2ray_class_with_the_yaml_keys(asora, tmp_path):
    """C2Ray_Test with `Photo: LLS_mfp_pMpc` in a cosmological configuration: two steps run, `a` follows the redshift between them,
    the run differs from the one without the keys, and the device-resident run equals the one through the host."""
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    from pyc2ray_amd.lls import MPC_CM
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 24
        with open("src.txt", "w") as f:
            f.write("2\n12 12 12 6e51 1.0\n5 20 9 2e51 1.0\n")
        with open("plain.yml", "w") as f:
            f.write("".join(l for l in open(LLS_PARAMS) if "LLS_" not in l))
        runs = {}
        for key, params, resident in (("lls", LLS_PARAMS, True), ("host", LLS_PARAMS, False), ("plain", "plain.yml", True)):
            if p.cuda_is_init():
                p.device_close()
            sim = pc2r.C2Ray_Test(params, N, True)
            sim.device_resident = resident
            assert sim.cosmological
            srcpos, srcflux = sim.read_sources("src.txt", 2)
            zs = sim.generate_redshift_array(2, 4e7)
            dt = sim.set_timestep(zs[0], zs[1], 2)
            sim.density_init(zs[0])
            a_seen, xs = [], []
            for step in range(2):
                sim.cosmo_evolve(dt)
                a_seen.append(None if sim.lls is None else sim.lls.n_const)
                sim.evolve3D(dt, srcflux, srcpos)
                xs.append(np.array(sim.xh))
            runs[key] = (a_seen, xs)
            assert lib.get_lls_opacity() == (0.0, 0.0)
            if key != "plain":
                a0 = 1.0 / (sim.sig * 0.135 * MPC_CM)
                assert a_seen[1] < a_seen[0] < a0 and a_seen[1] == pytest.approx(a0 * ((1 + sim.zred) / 10.0) ** 4.4, rel=1e-12)
                # sig a dr of the first step: about the 0.05 the file's header promises
                assert cases.SIG * a_seen[0] * sim.dr == pytest.approx(0.05, rel=0.1)
        assert runs["plain"][0] == [None, None]
        for a, b in zip(runs["lls"][1], runs["host"][1]):
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)
        assert np.all(np.isfinite(runs["lls"][1][1])) and runs["lls"][1][1].max() > 0.5
        assert runs["plain"][1][1].mean() > 1.02 * runs["lls"][1][1].mean()
    finally:
        if p.cuda_is_init():
            p.device_close()
        os.chdir(cwd)
