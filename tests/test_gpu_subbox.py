"""GPU parity tests of libc2ray.raytracing.do_all_sources -- the reference's CPU raytracer (cubic sub-boxes
grown until the photon loss is small, photon-loss statistics, heating rates, column densities of the last
source; src/c2ray/raytracing.f90:52-567) evaluated on the MI355X (csrc/subbox.hip).

Checkers: tests/golden/subbox.npz and raytrace.npz (outputs of the reference Fortran itself, flang-built) and
the oracle.  Tolerances: rates 1e-8 (same cancellation argument as test_gpu_parity.py), column densities
1e-11, sub-box counts exact, photon loss 1e-8.
"""
import os

import numpy as np
import pytest

import cases
from oracle import oracle as O

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RATE_RTOL = 1e-8


@pytest.fixture(scope="module")
def libs():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora, load_c2ray
    yield p, load_c2ray(), load_asora(), _capi
    if p.cuda_is_init():
        p.device_close()


def _fresh(p, N):
    """The entry point initialises the library itself; start each case from a closed device when N changes."""
    if p.cuda_is_init():
        p.device_close()


def _call(c2ray, c, max_subbox, subboxsize, loss_fraction, R, heat=True, numtau_minus=1):
    N = c["N"]
    phi = np.zeros((N, N, N), order="F")
    ph = np.zeros((N, N, N), order="F")
    cd = np.full((N, N, N), 7.0, order="F")          # the input content must not matter (f90:181)
    n = c["thin"].shape[0] - numtau_minus
    ht = c.get("heat_thin") if heat else None
    hk = c.get("heat_thick") if heat else None
    if ht is None:
        ht, hk = np.zeros(c["thin"].shape[0]), np.zeros(c["thin"].shape[0])
    nbox, loss = c2ray.raytracing.do_all_sources(c["flux"], c["pos"], max_subbox, subboxsize, cd, c["sig"], c["dr"],
                                                 c["ndens"], c["xh"], phi, ph, loss_fraction, c["thin"][:n],
                                                 c["thick"][:n], ht[:n], hk[:n], c["minlogtau"], c["dlogtau"], R)
    return phi, ph, cd, nbox, loss


def _close(a, b, rtol):
    scale = np.abs(b).max()
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-14 * scale)


@pytest.mark.parametrize("name", list(cases.SUBBOX_CASES))
def test_subbox_growth_matches_the_reference(libs, name):
    """Sub-box growth with early stop, unequal fluxes (the reference rates every source with the LAST source's
    flux, f90:500,503), heating tables: against the reference's own output."""
    p, c2ray, asora, capi = libs
    c = cases.subbox_case(name)
    _fresh(p, c["N"])
    # the f2py signature takes NumTau from the table length; the golden run passed NumTau = len - 1 with the full
    # tables (the benchmark's convention).  Hand over len - 1 entries: identical to the oracle called the same
    # way, and to the golden as long as tau stays below the last table entries (it does in these cases).
    g = np.load(os.path.join(G, "subbox.npz"))
    phi, heat, cd, nbox, loss = _call(c2ray, c, c["max_subbox"], c["subboxsize"], c["loss_fraction"], c["R"])
    n = c["thin"].shape[0] - 1
    ref = O.do_all_sources(c["flux"], c["pos"], c["max_subbox"], c["subboxsize"], c["sig"], c["dr"], c["ndens"],
                           c["xh"], c["loss_fraction"], c["thin"][:n], c["thick"][:n], c["minlogtau"], c["dlogtau"],
                           c["R"], heat_thin=c["heat_thin"][:n], heat_thick=c["heat_thick"][:n])
    assert nbox == ref["nsubbox"]
    _close(phi, ref["phi_ion"], RATE_RTOL)
    _close(heat, ref["phi_heat"], RATE_RTOL)
    assert np.array_equal(cd != 0, ref["coldens"] != 0)               # same cells reached by the last source
    np.testing.assert_allclose(cd, ref["coldens"], rtol=1e-11)
    np.testing.assert_allclose(loss, ref["photon_loss"], rtol=RATE_RTOL)
    # the reference's own numbers (tau never reaches the last table entries in these cases, so NumTau = len-1
    # with the full table and a table cut to len-1 entries give the same lookups)
    assert nbox == int(g[name + "__stats"][0])
    _close(phi, g[name + "__phi"], RATE_RTOL)
    _close(heat, g[name + "__heat"], RATE_RTOL)
    np.testing.assert_allclose(cd, g[name + "__cd"], rtol=1e-11)
    np.testing.assert_allclose(loss, g[name + "__stats"][1], rtol=RATE_RTOL)


@pytest.mark.parametrize("name", list(cases.RT_CASES))
@pytest.mark.parametrize("tables", ["grey", "soft"])
def test_full_box_matches_the_reference(libs, name, tables):
    """One box over the whole periodic cube (the golden raytracing cases): rates, column densities, counts."""
    p, c2ray, asora, capi = libs
    c = cases.rt_case(name, tables)
    N = c["N"]
    _fresh(p, N)
    g = np.load(os.path.join(G, "raytrace.npz"))
    phi, heat, cd, nbox, loss = _call(c2ray, c, 1000, N, 0.0, c["R"], heat=False)
    key = f"{name}__{tables}"
    _close(phi, g[key + "__phi"], RATE_RTOL)
    assert not heat.any()
    np.testing.assert_allclose(cd, g[key + "__cd"], rtol=1e-11)
    assert nbox == int(g[key + "__stats"][0]) == c["flux"].shape[0]
    if c["R"] >= 1000.0:
        # (with a finite radius, cells on the box faces beyond it deposit nothing and the reference adds an
        #  undefined phi_out to the loss there: not comparable)
        np.testing.assert_allclose(loss, g[key + "__stats"][1], rtol=RATE_RTOL)


def test_golden_subbox_case_of_round_one(libs):
    """The sub-box fixture that has been in raytrace.npz from the start (max_subbox 12, steps of 3)."""
    p, c2ray, asora, capi = libs
    c = cases.rt_case("l32_5src_R10", "grey")
    _fresh(p, c["N"])
    g = np.load(os.path.join(G, "raytrace.npz"))
    phi, heat, cd, nbox, loss = _call(c2ray, c, 12, 3, 1e-2, 1000.0, heat=False)
    _close(phi, g["subbox__phi"], RATE_RTOL)
    assert nbox == int(g["subbox__stats"][0])
    np.testing.assert_allclose(loss, g["subbox__stats"][1], rtol=RATE_RTOL)


def test_own_flux_option(libs):
    """ASORA_OPT_C2RAY_OWN_FLUX = 1 rates every source with its own flux (what the CUDA path does)."""
    p, c2ray, asora, capi = libs
    c = cases.subbox_case("sb32_mid")
    _fresh(p, c["N"])
    n = c["thin"].shape[0] - 1
    asora.set_option(capi.OPT_C2RAY_OWN_FLUX, 1)
    try:
        phi, heat, cd, nbox, loss = _call(c2ray, c, c["max_subbox"], c["subboxsize"], c["loss_fraction"], c["R"])
    finally:
        asora.set_option(capi.OPT_C2RAY_OWN_FLUX, 0)
    ref = O.do_all_sources(c["flux"], c["pos"], c["max_subbox"], c["subboxsize"], c["sig"], c["dr"], c["ndens"],
                           c["xh"], c["loss_fraction"], c["thin"][:n], c["thick"][:n], c["minlogtau"], c["dlogtau"],
                           c["R"], heat_thin=c["heat_thin"][:n], heat_thick=c["heat_thick"][:n],
                           flags=O.PER_SOURCE_FLUX)
    assert nbox == ref["nsubbox"]
    _close(phi, ref["phi_ion"], RATE_RTOL)
    _close(heat, ref["phi_heat"], RATE_RTOL)
    np.testing.assert_allclose(loss, ref["photon_loss"], rtol=RATE_RTOL)
    # and it differs from the default
    phi_last, *_ = _call(c2ray, c, c["max_subbox"], c["subboxsize"], c["loss_fraction"], c["R"])
    assert np.abs(phi_last - phi).max() > 1e-2 * phi.max()


def test_phi_heat_is_accumulated_onto_and_phi_ion_is_reset(libs):
    """phi_ion is zeroed by the call (f90:95), phi_heat is intent(inout) and only added to."""
    p, c2ray, asora, capi = libs
    c = cases.subbox_case("sb16_b7")
    N = c["N"]
    _fresh(p, N)
    n = c["thin"].shape[0] - 1
    phi0, heat0, *_ = _call(c2ray, c, 1000, 7, 1e-3, 1000.0)
    phi = np.full((N, N, N), 3.0, order="F")
    heat = np.full((N, N, N), 2.0e-16, order="F")
    cd = np.zeros((N, N, N), order="F")
    c2ray.raytracing.do_all_sources(c["flux"], c["pos"], 1000, 7, cd, c["sig"], c["dr"], c["ndens"], c["xh"], phi, heat,
                                    1e-3, c["thin"][:n], c["thick"][:n], c["heat_thin"][:n], c["heat_thick"][:n],
                                    c["minlogtau"], c["dlogtau"], 1000.0)
    _close(phi, phi0, 1e-12)
    _close(heat - 2.0e-16, heat0, 1e-6)


def test_no_box_at_all(libs):
    """loss_fraction >= 1, or max_subbox = 0: the while loop of do_source never runs (f90:193-195): no rates,
    no sub-boxes, every photon counted as lost."""
    p, c2ray, asora, capi = libs
    c = cases.subbox_case("sb16_b7")
    _fresh(p, c["N"])
    for max_subbox, lf in ((1000, 1.5), (0, 1e-2)):
        phi, heat, cd, nbox, loss = _call(c2ray, c, max_subbox, 7, lf, 1000.0)
        assert nbox == 0 and not phi.any() and not heat.any() and not cd.any()
        np.testing.assert_allclose(loss, c["flux"].sum() * 1e48, rtol=1e-14)


def test_error_paths(libs):
    p, c2ray, asora, capi = libs
    c = cases.subbox_case("sb16_b7")
    N = c["N"]
    _fresh(p, N)
    n = c["thin"].shape[0] - 1
    args = lambda pos, sub, cd: (c["flux"], pos, 1000, sub, cd, c["sig"], c["dr"], c["ndens"], c["xh"],
                                 np.zeros((N, N, N), order="F"), np.zeros((N, N, N), order="F"), 1e-2,
                                 c["thin"][:n], c["thick"][:n], c["heat_thin"][:n], c["heat_thick"][:n],
                                 c["minlogtau"], c["dlogtau"], 1000.0)
    good_cd = np.zeros((N, N, N), order="F")
    with pytest.raises(RuntimeError, match="subboxsize"):
        c2ray.raytracing.do_all_sources(*args(c["pos"], 0, good_cd))
    bad = c["pos"].copy()
    bad[1, 0] = N + 1
    with pytest.raises(RuntimeError, match="outside the mesh"):
        c2ray.raytracing.do_all_sources(*args(bad, 4, good_cd))
    with pytest.raises(ValueError, match="Fortran-contiguous"):
        c2ray.raytracing.do_all_sources(*args(c["pos"], 4, np.zeros((N, N, N))))
    # a library initialised for another mesh size refuses
    p.device_init(N + 2, 1)
    with pytest.raises(RuntimeError, match="does not match"):
        c2ray.raytracing.do_all_sources(*args(c["pos"], 4, good_cd))
    p.device_close()


def test_many_sources_larger_mesh_against_oracle(libs):
    """64^3, 12 sources, boxes of 6 cells, moderate opacity: sources stop after different numbers of boxes."""
    p, c2ray, asora, capi = libs
    N = 64
    nd, xh, dr = cases.grid(N, "lognormal", 31, 0.6)
    pos, flux = cases.sources(N, 12, 32, flux=2.0)
    flux = flux * (1.0 + 0.25 * np.arange(12))
    thin, thick, dlog = cases.soft_tables()
    c = dict(N=N, ndens=nd, xh=xh, dr=dr, pos=pos, flux=flux, thin=thin, thick=thick, dlogtau=dlog,
             minlogtau=cases.MINLOGTAU, sig=cases.SIG, heat_thin=1e-11 * thin, heat_thick=2e-11 * thick)
    _fresh(p, N)
    phi, heat, cd, nbox, loss = _call(c2ray, c, 1000, 6, 2e-2, 20.0)
    n = thin.shape[0] - 1
    # R_max_LLS = 20 < box: the reference's loss on the faces beyond the radius is undefined; the library adds 0 there, and so
    # does the oracle under STOPPED_CELLS_LOSE_NOTHING (tests/test_oracle_subbox_loss.py)
    ref = O.do_all_sources(flux, pos, 1000, 6, cases.SIG, dr, nd, xh, 2e-2, thin[:n], thick[:n], cases.MINLOGTAU, dlog,
                           20.0, heat_thin=c["heat_thin"][:n], heat_thick=c["heat_thick"][:n], flags=O.STOPPED_CELLS_LOSE_NOTHING)
    assert nbox == ref["nsubbox"]
    np.testing.assert_allclose(loss, ref["photon_loss"], rtol=RATE_RTOL)
    _close(phi, ref["phi_ion"], RATE_RTOL)
    _close(heat, ref["phi_heat"], RATE_RTOL)
    np.testing.assert_allclose(cd, ref["coldens"], rtol=1e-11)
    assert 12 <= nbox <= 12 * 6


def test_evolve3d_cpu_semantics(libs):
    """evolve3D(use_gpu=False): the reference's CPU branch (sub-box raytracer + global_pass per iteration)."""
    p, c2ray, asora, capi = libs
    import evolve_oracle as EO
    c = cases.rt_case("l16_7src_R5.5", "soft")
    N = c["N"]
    _fresh(p, N)
    rng = np.random.default_rng(5)
    temp = np.asfortranarray(10 ** rng.uniform(3.5, 4.5, size=(N, N, N)))
    nd = np.asfortranarray(c["ndens"])
    xh = np.asfortranarray(np.full((N, N, N), 2e-4))
    kw = dict(dt=3.15576e13, dr=c["dr"], src_flux=c["flux"], src_pos=c["pos"], max_subbox=1000, subboxsize=3,
              loss_fraction=1e-2, temp=temp, ndens=nd, xh=xh, thin=c["thin"], thick=c["thick"],
              minlogtau=c["minlogtau"], dlogtau=c["dlogtau"], R=1000.0, conv=1e-3, sig=c["sig"])
    xh_new, phi = p.evolve3D(kw["dt"], kw["dr"], kw["src_flux"], kw["src_pos"], False, kw["max_subbox"],
                             kw["subboxsize"], kw["loss_fraction"], temp, nd, xh, c["thin"], c["thick"],
                             c["minlogtau"], c["dlogtau"], kw["R"], kw["conv"], c["sig"], cases.BH00, cases.ALBPOW,
                             cases.COLH0, cases.TEMPH0, cases.ABU_C, logfile=os.devnull, quiet=True)
    ref_x, ref_phi, ref_iter = EO.evolve3d_cpu_path(**kw)
    assert p.evolve._evolve.last_niter == ref_iter
    assert phi.flags.f_contiguous and xh_new.flags.f_contiguous
    np.testing.assert_allclose(xh_new, ref_x, rtol=1e-7)
    _close(phi, ref_phi, 1e-7)


def test_do_raytracing_cpu_semantics_with_stats(libs):
    p, c2ray, asora, capi = libs
    c = cases.subbox_case("sb32_mid")
    _fresh(p, c["N"])
    g = np.load(os.path.join(G, "subbox.npz"))
    n = c["thin"].shape[0] - 1
    out = p.do_raytracing(c["dr"], c["flux"], c["pos"], False, c["max_subbox"], c["subboxsize"], c["loss_fraction"],
                          c["ndens"], c["xh"], c["thin"][:n], c["thick"][:n], c["heat_thin"][:n], c["heat_thick"][:n],
                          c["minlogtau"], c["dlogtau"], c["R"], c["sig"], logfile=os.devnull, quiet=True, stats=True)
    phi, nbox, loss = out
    _close(phi, g["sb32_mid__phi"], RATE_RTOL)
    assert nbox == int(g["sb32_mid__stats"][0])
    np.testing.assert_allclose(loss, g["sb32_mid__stats"][1], rtol=RATE_RTOL)
    phi2, heat2 = p.do_raytracing(c["dr"], c["flux"], c["pos"], False, c["max_subbox"], c["subboxsize"],
                                  c["loss_fraction"], c["ndens"], c["xh"], c["thin"][:n], c["thick"][:n],
                                  c["heat_thin"][:n], c["heat_thick"][:n], c["minlogtau"], c["dlogtau"], c["R"],
                                  c["sig"], logfile=os.devnull, quiet=True)
    _close(heat2, g["sb32_mid__heat"], RATE_RTOL)


def test_randomised_subbox_parameters_against_oracle(libs):
    """Seeded sweep over mesh sizes (odd and even), source counts and positions (corners included), ranges,
    box steps, loss fractions and opacities: box counts, loss, rates, heating and column densities against the
    oracle (R_max_LLS covers the boxes, so the loss is defined everywhere)."""
    p, c2ray, asora, capi = libs
    rng = np.random.default_rng(2027)
    thin, thick, dlog = cases.soft_tables(400)
    n = thin.shape[0]
    ht, hk = 1e-11 * thin[::-1].copy(), 3e-12 * thick
    seen_early_stop = seen_full = 0
    for trial in range(24):
        N = int(rng.choice([9, 12, 16, 20]))
        ns = int(rng.integers(1, 5))
        tau_cell = float(10 ** rng.uniform(-2.0, 0.7))
        nd, xh, dr = cases.grid(N, "lognormal", 100 + trial, tau_cell)
        pos = 1 + rng.integers(0, N, size=(3, ns))
        if trial % 5 == 0:
            pos[:, 0] = [1, N, 1]                                   # a corner source: the cube wraps on every axis
        flux = rng.uniform(0.5, 4.0, size=ns)
        max_subbox = int(rng.choice([1, 2, 3, N // 2 - 1, N // 2, 1000]))
        subboxsize = int(rng.integers(1, 7))
        lf = float(rng.choice([0.0, 1e-3, 0.05, 0.3, 0.9]))
        _fresh(p, N)
        phi = np.zeros((N, N, N), order="F"); heat = np.zeros((N, N, N), order="F"); cd = np.zeros((N, N, N), order="F")
        nbox, loss = c2ray.raytracing.do_all_sources(flux, pos, max_subbox, subboxsize, cd, cases.SIG, dr, nd, xh, phi, heat,
                                                     lf, thin, thick, ht, hk, cases.MINLOGTAU, dlog, 1000.0)
        ref = O.do_all_sources(flux, pos, max_subbox, subboxsize, cases.SIG, dr, nd, xh, lf, thin, thick, cases.MINLOGTAU,
                               dlog, 1000.0, heat_thin=ht, heat_thick=hk)
        tag = f"trial {trial}: N={N} ns={ns} max_subbox={max_subbox} subboxsize={subboxsize} lf={lf} tau={tau_cell:.3g}"
        assert nbox == ref["nsubbox"], tag
        np.testing.assert_allclose(loss, ref["photon_loss"], rtol=RATE_RTOL, err_msg=tag)
        assert np.array_equal(cd != 0, ref["coldens"] != 0), tag
        np.testing.assert_allclose(cd, ref["coldens"], rtol=1e-11, err_msg=tag)
        _close(phi, ref["phi_ion"], RATE_RTOL)
        _close(heat, ref["phi_heat"], RATE_RTOL)
        full = sum(-(-min(max_subbox, N // 2 - 1 + N % 2) // subboxsize) for _ in range(ns))
        seen_early_stop += nbox < full
        seen_full += nbox == full
    assert seen_early_stop >= 3 and seen_full >= 3            # the sweep exercises both outcomes


@pytest.mark.parametrize("name", ["sb32_b5", "sb32_mid", "sb17_b2"])
@pytest.mark.parametrize("heat", [True, False])
def test_shell_buffers_in_lds_and_in_global_memory_give_the_same(libs, name, heat):
    """The sweep keeps its two shell buffers in LDS when they fit and hands the trailing shell to the next sub-box's
    launch through global memory; with ASORA_OPT_SUBBOX_GLOBAL_SHELLS both stay in global memory (what large meshes
    use).  Same box counts and loss, rates and column densities equal up to the order of the atomic sums -- with and
    without heating tables (two kernel variants each)."""
    p, c2ray, asora, capi = libs
    c = cases.subbox_case(name)
    _fresh(p, c["N"])
    out = []
    for global_shells in (0, 1):
        asora.set_option(capi.OPT_SUBBOX_GLOBAL_SHELLS, global_shells)
        try:
            out.append(_call(c2ray, c, c["max_subbox"], c["subboxsize"], c["loss_fraction"], c["R"], heat=heat))
        finally:
            asora.set_option(capi.OPT_SUBBOX_GLOBAL_SHELLS, 0)
    (phi0, heat0, cd0, nbox0, loss0), (phi1, heat1, cd1, nbox1, loss1) = out
    assert nbox0 == nbox1
    np.testing.assert_allclose(loss0, loss1, rtol=1e-12)
    assert np.array_equal(cd0, cd1)
    _close(phi0, phi1, 1e-12)
    _close(heat0, heat1, 1e-12)
    assert heat or not heat0.any()
    g = np.load(os.path.join(G, "subbox.npz"))
    if heat:
        _close(phi1, g[name + "__phi"], RATE_RTOL)
        assert nbox1 == int(g[name + "__stats"][0])


# ---- the sweep on tabulated geometry (round 3: raytrace.hip SUBBOX) -----------------------------------------------------
@pytest.mark.parametrize("name", list(cases.SUBBOX_CASES))
def test_tabulated_sweep_matches_the_reference(libs, name):
    """ASORA_OPT_SUBBOX_TABLES = 2: every source but the last (whose column densities go back to the caller) is swept on
    the tabulated geometry of the ASORA kernel -- launch per sub-box, trailing shell through global memory, photon loss
    from the cells on the box faces.  Same fixtures of the reference Fortran as the on-the-fly kernel: box counts exact,
    rates, heating, loss and column densities."""
    p, c2ray, asora, capi = libs
    c = cases.subbox_case(name)
    _fresh(p, c["N"])
    g = np.load(os.path.join(G, "subbox.npz"))
    asora.set_option(capi.OPT_SUBBOX_TABLES, 2)
    try:
        phi, heat, cd, nbox, loss = _call(c2ray, c, c["max_subbox"], c["subboxsize"], c["loss_fraction"], c["R"])
    finally:
        asora.set_option(capi.OPT_SUBBOX_TABLES, 0)
    assert nbox == int(g[name + "__stats"][0])
    _close(phi, g[name + "__phi"], RATE_RTOL)
    _close(heat, g[name + "__heat"], RATE_RTOL)
    np.testing.assert_allclose(cd, g[name + "__cd"], rtol=1e-11)
    np.testing.assert_allclose(loss, g[name + "__stats"][1], rtol=RATE_RTOL)


def test_tabulated_sweep_randomised_against_oracle_and_on_the_fly_kernel(libs):
    """Seeded sweep: mesh sizes, source counts (corners included), ranges, box sizes, loss fractions, opacities, and radii
    both beyond the range (loss defined everywhere) and INSIDE it (the tables then hold the sphere only; cells on box faces
    beyond the radius add nothing on either GPU path, nor in the oracle under STOPPED_CELLS_LOSE_NOTHING): the two paths
    against each other and against the oracle -- box counts, loss, rates, heating."""
    p, c2ray, asora, capi = libs
    rng = np.random.default_rng(2031)
    thin, thick, dlog = cases.soft_tables(400)
    ht, hk = 1e-11 * thin[::-1].copy(), 3e-12 * thick
    seen_multi_box = 0
    for trial in range(28):
        N = int(rng.choice([12, 16, 20, 33]))
        ns = int(rng.integers(2, 7))
        tau_cell = float(10 ** rng.uniform(-2.0, 0.5))
        nd, xh, dr = cases.grid(N, "lognormal", 300 + trial, tau_cell)
        pos = 1 + rng.integers(0, N, size=(3, ns))
        if trial % 4 == 0:
            pos[:, 0] = [1, N, 1]
        flux = rng.uniform(0.5, 4.0, size=ns)
        max_subbox = int(rng.choice([3, N // 2 - 1, N // 2, 1000]))
        subboxsize = int(rng.integers(1, 6))
        lf = float(rng.choice([0.0, 1e-3, 0.05, 0.3]))
        R = float(rng.choice([1000.0, 1000.0, 2.5, 4.0, 5.0, N / 3.0]))
        use_heat = bool(trial % 2)
        own_flux = trial % 3 == 0                      # ASORA_OPT_C2RAY_OWN_FLUX: each source its own flux (default: the last one's)
        zeros = np.zeros(thin.shape[0])
        _fresh(p, N)
        out = {}
        # 1: the on-the-fly kernel; 2: the tabulated sweep, one source per workgroup; 3: the tabulated sweep with TWO sources
        # per workgroup (round 4; sources that stop growing after different numbers of boxes share workgroups, odd counts
        # leave one alone; with heating the library keeps one source per workgroup)
        for variant in (1, 2, 3):
            phi = np.zeros((N, N, N), order="F"); heat = np.zeros((N, N, N), order="F"); cd = np.zeros((N, N, N), order="F")
            asora.set_option(capi.OPT_SUBBOX_TABLES, min(variant, 2))
            asora.set_option(capi.OPT_PAIR_SOURCES, 2 if variant == 3 else 1)
            asora.set_option(capi.OPT_C2RAY_OWN_FLUX, 1 if own_flux else 0)
            try:
                nbox, loss = c2ray.raytracing.do_all_sources(flux, pos, max_subbox, subboxsize, cd, cases.SIG, dr, nd, xh, phi, heat,
                                                             lf, thin, thick, ht if use_heat else zeros, hk if use_heat else zeros,
                                                             cases.MINLOGTAU, dlog, R)
            finally:
                asora.set_option(capi.OPT_SUBBOX_TABLES, 0)
                asora.set_option(capi.OPT_PAIR_SOURCES, 0)
                asora.set_option(capi.OPT_C2RAY_OWN_FLUX, 0)
            out[variant] = (phi, heat, cd, nbox, loss)
        tag = f"trial {trial}: N={N} ns={ns} max_subbox={max_subbox} subboxsize={subboxsize} lf={lf} tau={tau_cell:.3g} R={R} heat={use_heat}"
        phi3, heat3, cd3, nbox3, loss3 = out[3]
        assert nbox3 == out[2][3], tag
        np.testing.assert_allclose(loss3, out[2][4], rtol=1e-12, err_msg=tag)
        assert np.array_equal(cd3, out[2][2]), tag
        _close(phi3, out[2][0], 1e-12)                              # (same arithmetic per source; sums in another order)
        _close(heat3, out[2][1], 1e-12)
        (phi1, heat1, cd1, nbox1, loss1), (phi2, heat2, cd2, nbox2, loss2) = out[1], out[2]
        assert nbox1 == nbox2, tag
        np.testing.assert_allclose(loss2, loss1, rtol=RATE_RTOL, err_msg=tag)
        assert np.array_equal(cd1, cd2), tag                       # the dumped source takes the same kernel on both paths
        _close(phi2, phi1, RATE_RTOL)
        _close(heat2, heat1, RATE_RTOL)
        ref = O.do_all_sources(flux, pos, max_subbox, subboxsize, cases.SIG, dr, nd, xh, lf, thin, thick, cases.MINLOGTAU,
                               dlog, R, heat_thin=ht if use_heat else None, heat_thick=hk if use_heat else None,
                               flags=O.STOPPED_CELLS_LOSE_NOTHING | (O.PER_SOURCE_FLUX if own_flux else 0))
        # (with the radius inside the range the faces hold cells that deposit nothing: 0 to the loss on the device and, under the
        #  flag, in the oracle; beyond the range the flag changes nothing)
        assert nbox2 == ref["nsubbox"], tag
        np.testing.assert_allclose(loss2, ref["photon_loss"], rtol=RATE_RTOL, err_msg=tag)
        _close(phi2, ref["phi_ion"], RATE_RTOL)
        _close(heat2, ref["phi_heat"], RATE_RTOL)
        seen_multi_box += nbox2 > ns
    assert seen_multi_box >= 8


@pytest.mark.parametrize("heat", [False, True])
def test_tabulated_sweep_on_line_aligned_tables(libs, heat):
    """Round 5: the sub-box sweep on the line-aligned form of its tables (eight forms of every sector table, by the source's
    position modulo 8 along the memory-contiguous axis of the sector's face; two sources share a workgroup only when they agree
    in it: pair lists) -- sectors of one face, i.e. radii from 25.5 cells.  N = 64, 41 sources (an odd count; corners of the box
    included), sub-boxes of 7 cells grown until the loss is small: aligned paired / aligned single / packed tables against each
    other (same arithmetic per cell) and against the oracle."""
    p, c2ray, asora, capi = libs
    N, ns, R = 64, 41, 28.0
    rng = np.random.default_rng(77)
    thin, thick, dlog = cases.soft_tables(400)
    ht, hk = 1e-11 * thin[::-1].copy(), 3e-12 * thick
    zeros = np.zeros(thin.shape[0])
    nd, xh, dr = cases.grid(N, "lognormal", 78, 0.08)
    pos = 1 + rng.integers(0, N, size=(3, ns))
    pos[:, 0], pos[:, 1] = [1, N, 1], [N, N, N]
    flux = rng.uniform(0.5, 4.0, size=ns)
    _fresh(p, N)
    out = {}
    for name, aligned, pairs in (("aligned_pairs", 2, 2), ("aligned_single", 2, 1), ("packed_pairs", 1, 2)):
        phi = np.zeros((N, N, N), order="F"); hgrid = np.zeros((N, N, N), order="F"); cd = np.zeros((N, N, N), order="F")
        asora.set_option(capi.OPT_SUBBOX_TABLES, 2)
        asora.set_option(capi.OPT_ALIGNED_ROWS, aligned)
        asora.set_option(capi.OPT_PAIR_SOURCES, pairs)
        try:
            nbox, loss = c2ray.raytracing.do_all_sources(flux, pos, 1000, 7, cd, cases.SIG, dr, nd, xh, phi, hgrid, 1e-3, thin, thick,
                                                         ht if heat else zeros, hk if heat else zeros, cases.MINLOGTAU, dlog, R)
            v = asora.last_raytrace_variant()
        finally:
            asora.set_option(capi.OPT_SUBBOX_TABLES, 0)
            asora.set_option(capi.OPT_ALIGNED_ROWS, 0)
            asora.set_option(capi.OPT_PAIR_SOURCES, 0)
        assert v["aligned"] == (aligned == 2) and v["units"] == 6 and v["paired"] == (pairs == 2 and not heat), (name, v)
        out[name] = (phi, hgrid, cd, nbox, loss)
    a, b, c = out["aligned_pairs"], out["aligned_single"], out["packed_pairs"]
    for other in (b, c):
        assert a[3] == other[3]
        np.testing.assert_allclose(a[4], other[4], rtol=1e-12)
        assert np.array_equal(a[2], other[2])
        _close(a[0], other[0], 1e-12)
        _close(a[1], other[1], 1e-12)
    ref = O.do_all_sources(flux, pos, 1000, 7, cases.SIG, dr, nd, xh, 1e-3, thin, thick, cases.MINLOGTAU, dlog, R,
                           heat_thin=ht if heat else None, heat_thick=hk if heat else None, flags=O.STOPPED_CELLS_LOSE_NOTHING)
    assert a[3] == ref["nsubbox"]
    np.testing.assert_allclose(a[4], ref["photon_loss"], rtol=RATE_RTOL)
    _close(a[0], ref["phi_ion"], RATE_RTOL)
    if heat:
        _close(a[1], ref["phi_heat"], RATE_RTOL)
    assert a[3] >= ns and np.isfinite(a[0]).all() and a[0].max() > 0


def test_tabulated_sweep_in_several_batches(libs, monkeypatch):
    """The trailing shells of the tabulated sweep live in a scratch of bounded size; more sources than it holds are swept
    in batches (the dumped source in the last one).  Forced here with a scratch of a few sources: same results."""
    p, c2ray, asora, capi = libs
    N = 24
    nd, xh, dr = cases.grid(N, "lognormal", 77, 0.3)
    pos, flux = cases.sources(N, 23, 78, flux=2.0)
    flux = flux * (1.0 + 0.1 * np.arange(23))
    thin, thick, dlog = cases.soft_tables()
    c = dict(N=N, ndens=nd, xh=xh, dr=dr, pos=pos, flux=flux, thin=thin, thick=thick, dlogtau=dlog,
             minlogtau=cases.MINLOGTAU, sig=cases.SIG, heat_thin=1e-11 * thin, heat_thick=2e-11 * thick)
    _fresh(p, N)
    out = []
    for budget in (None, "60000"):                 # 60 kB: about five sources per batch at this size
        if budget:
            monkeypatch.setenv("ASORA_SUBBOX_TRAIL_BUDGET", budget)
        asora.set_option(capi.OPT_SUBBOX_TABLES, 2)
        try:
            out.append(_call(c2ray, c, 1000, 3, 2e-2, 7.0))
        finally:
            asora.set_option(capi.OPT_SUBBOX_TABLES, 0)
            monkeypatch.delenv("ASORA_SUBBOX_TRAIL_BUDGET", raising=False)
    # the same without heating and with two sources per workgroup, whole and in batches of five (odd: a source sweeps alone)
    c_noheat = dict(c, heat_thin=np.zeros_like(thin), heat_thick=np.zeros_like(thick))
    paired = []
    for pairs, budget in ((1, None), (2, None), (2, "60000")):
        if budget:
            monkeypatch.setenv("ASORA_SUBBOX_TRAIL_BUDGET", budget)
        asora.set_option(capi.OPT_SUBBOX_TABLES, 2)
        asora.set_option(capi.OPT_PAIR_SOURCES, pairs)
        try:
            paired.append(_call(c2ray, c_noheat, 1000, 3, 2e-2, 7.0))
        finally:
            asora.set_option(capi.OPT_SUBBOX_TABLES, 0)
            asora.set_option(capi.OPT_PAIR_SOURCES, 0)
            monkeypatch.delenv("ASORA_SUBBOX_TRAIL_BUDGET", raising=False)
    for phi_p, _, cd_p, nbox_p, loss_p in paired[1:]:
        assert nbox_p == paired[0][3] and np.array_equal(cd_p, paired[0][2])
        np.testing.assert_allclose(loss_p, paired[0][4], rtol=1e-12)
        _close(phi_p, paired[0][0], 1e-12)
    _close(paired[0][0], out[0][0], 1e-12)          # (the rates do not depend on the heating tables)
    (phi0, heat0, cd0, nbox0, loss0), (phi1, heat1, cd1, nbox1, loss1) = out
    assert nbox0 == nbox1 and nbox0 > 23
    np.testing.assert_allclose(loss1, loss0, rtol=1e-12)
    assert np.array_equal(cd0, cd1)
    _close(phi1, phi0, 1e-12)
    _close(heat1, heat0, 1e-12)
    n = thin.shape[0] - 1
    ref = O.do_all_sources(flux, pos, 1000, 3, cases.SIG, dr, nd, xh, 2e-2, thin[:n], thick[:n], cases.MINLOGTAU, dlog, 7.0,
                           heat_thin=c["heat_thin"][:n], heat_thick=c["heat_thick"][:n], flags=O.STOPPED_CELLS_LOSE_NOTHING)
    assert nbox1 == ref["nsubbox"]
    np.testing.assert_allclose(loss1, ref["photon_loss"], rtol=RATE_RTOL)
    _close(phi1, ref["phi_ion"], RATE_RTOL)
    _close(heat1, ref["phi_heat"], RATE_RTOL)
