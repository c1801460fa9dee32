"""GPU: the photo-heating rates of the HEAT raytrace forms and the thermal device loop that consumes them, against the CPU
oracle (oracle_asora_do_all_sources with heating tables) and tests/thermal_reference.py.

Two kinds of check:
  * the power-of-two identity: heating tables = 2^-35 x photo tables.  The kernels form the heating rate exactly like the
    photo rate (the same table index and residual, pref (T_in - T_out) or pref dtau T), and scaling by a power of two
    commutes with every rounding there, so with sources whose spheres do not overlap (one addition per cell: no
    summation-order freedom) PHI_HEAT == 2^-35 PHI_ION bit for bit -- in every launch form, and after every step of the
    thermal loop, whatever was left in the accumulators before;
  * black-body heating tables (not proportional to the photo tables) against the oracle, and the thermal passes against
    the numpy statement of the scheme evaluated on the rates the pass read.
"""
import numpy as np
import pytest

import cases
import thermal_reference as TR
from oracle import oracle as O

pytestmark = pytest.mark.gpu

P2 = 2.0 ** -35                     # ~20 eV per ionisation
GAMMA_RTOL = 1e-8                   # the rate tolerance of tests/test_gpu_parity.py
CHEM = (cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)
# the conditioning split of tests/test_gpu_thermal.py
WELL_CONDITIONED = 1e-2
ILL_RTOL_XAV, ILL_RTOL = 1e-3, 1e-7


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib, _capi
    if p.cuda_is_init():
        lib.thermal_params(False)
        p.device_close()


def _fresh(p, N):
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)


def _set(lib, capi, opts):
    for k, v in opts.items():
        lib.set_option(getattr(capi, k), v)


def _reset(lib, capi, opts):
    for k in opts:
        lib.set_option(getattr(capi, k), 1 if k == "OPT_Z_TRANSPOSED" else 0)


def _form(lib, v):
    """The heating form the last launch took (variant table): family, workgroup size, table capacity -- read from the
    row the library says it launched (asora_debug_last_launch_form), which must be a heating row and agree with the variant word."""
    form, row = lib.last_launch_form()
    assert form is not None and lib.built_forms()[row] == form, (form, row)
    f = dict(zip(lib.FORM_FIELDS, form))
    assert f["heat"] and not f["dump"] and not f["grey"] and not f["skip_zero"] and f["nsrc"] == 1 and not f["subbox"], f
    assert (f["threads"], bool(f["bufatom"]), bool(f["split"]), bool(f["global_scratch"]), bool(f["open"])) == \
           (v["threads"], v["buffer_atomics"], v["split_descriptors"], v["global_shells"], v["open"]), (f, v)
    if f["split"]:
        family = "split"
    elif f["bufatom"]:
        family = "buffer"
    elif f["global_scratch"]:
        family = "global_shells"
    else:
        family = "global"
    return family, f["threads"], f["tabcap"]


def _lattice_sources(N, n, seed, spacing=12):
    lattice = np.array([(i, j, k) for i in range(1, N, spacing) for j in range(1, N, spacing) for k in range(1, N, spacing)]).T
    rng = np.random.RandomState(seed)
    pos = lattice[:, rng.permutation(lattice.shape[1])[:n]].copy()
    pos[:, 0] = [1, 1, 1]                                       # a corner: the periodic wrap is in play
    flux = rng.uniform(1.0, 5.0, n)
    return pos, flux


# ---- 3a: every heating form ------------------------------------------------------------------------------------------
def _identity_launch(lib, capi, N, R, n, dr, numtau, dlog, opts, seen):
    """One raytrace with heating under `opts`; asserts the identity and returns (phi, heat, variant)."""
    _set(lib, capi, dict(opts, OPT_HEATING=1))
    try:
        lib.raytrace_device(R, cases.SIG, dr, 0, n, cases.MINLOGTAU, dlog, numtau)
        v = lib.last_raytrace_variant()
        phi = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
        heat = lib.grid_to_host(capi.GRID_PHI_HEAT, np.empty((N, N, N)))
    finally:
        _reset(lib, capi, dict(opts, OPT_HEATING=1))
    seen.add(_form(lib, v))
    assert not v["paired"] and not v["skip_zero"], (R, opts, v)     # neither form exists with heating
    tag = f"N={N} R={R} n={n} {opts} {v}"
    assert phi.max() > 0, tag
    assert np.array_equal(heat, P2 * phi), tag
    assert not np.signbit(heat).any() and not np.signbit(phi).any(), tag
    return phi, heat, v


REQUIRED_FORMS = (
    # single source, buffer atomics: {64..1024} x 256 tables, {64,128} x 64 tables
    {("buffer", t, 256) for t in (64, 128, 256, 512, 1024)} | {("buffer", t, 64) for t in (64, 128)}
    # single source, global atomics (option), shells in LDS
    | {("global", t, 256) for t in (64, 128, 256, 512, 1024)} | {("global", t, 64) for t in (64, 128)})
# ... and the shells in global memory (family "global_shells", at whatever workgroup size the library picks).  Not reachable
# below N = 512: the per-layout descriptor form (SPLIT) and the 1024-entry tables (more than 256 shells), which
# tests/test_gpu_form_recipes.py runs row by row, as it does the sub-box sweep with heating.


def test_every_heating_form_by_identity_and_against_the_oracle(asora):
    """Heating tables = 2^-35 x photo tables, 80 sources on a lattice (spheres apart; one on a box corner), tiny radii to
    radii beyond the box (one source), an ordinary, an optically thin (thin-cell lookups at tau_out) and a thick medium
    (most cells beyond the last table entry: heat exactly +0 wherever the rate is), through every decomposition, workgroup
    size, both atomic families, both accumulator layouts and both constant sets: PHI_HEAT == 2^-35 PHI_ION bit for bit.
    The paired-source and exact-zero-skipping forms do not exist with heating: forcing them changes nothing.  Then
    overlapping spheres with black-body tables against the oracle, and the N = 168 set-up of
    test_large_shells_global_scratch_and_large_lds (shells in global memory, 256-entry tables at 64 / 128 threads).
    The forms seen must include every heating row of the variant table reachable at these sizes."""
    p, lib, capi = asora
    seen = set()
    N = 96
    thin, thick, dlog = cases.soft_tables(400)
    numtau = thin.shape[0]
    nd, xh, dr = cases.grid(N, "lognormal", 11, 0.4, xlo=1e-4, xhi=1e-2)
    _fresh(p, N)
    p.photo_table_to_device(thin, thick)
    lib.heat_table_to_device(P2 * thin, P2 * thick, numtau)
    pos, flux = _lattice_sources(N, 80, 3)
    p0, f0 = cases.flat_sources(pos, flux)
    lib.grid_to_device(capi.GRID_XH_AV, xh)
    combos = ([{}] + [{"OPT_SECTORS": m} for m in range(1, 10)]
              + [{"OPT_BLOCK_THREADS": t} for t in (64, 128, 256, 512, 1024)]
              + [{"OPT_SECTORS": 1, "OPT_BLOCK_THREADS": t} for t in (64, 128, 1024)]
              + [{"OPT_SECTORS": 3, "OPT_BLOCK_THREADS": 512}, {"OPT_Z_TRANSPOSED": 0}, {"OPT_FORTRAN_CONSTANTS": 1},
                 {"OPT_FORTRAN_CONSTANTS": 1, "OPT_SECTORS": 2}])
    media = {"ordinary": nd, "thin": nd * 2.5e-9, "thick": nd * 3.0e4}
    for medium, ndm in media.items():
        lib.grid_to_device(capi.GRID_NDENS, ndm)
        for R, n in ((0.5, 80), (1.0, 80), (5.5, 80), (1000.0, 1)):
            lib.source_data_to_device(p0[:3 * n], f0[:n], n)
            first = None
            for opts in combos:
                for glob in (0, 1):
                    phi, heat, v = _identity_launch(lib, capi, N, R, n, dr, numtau, dlog, dict(opts, OPT_GLOBAL_ATOMICS=glob), seen)
                    if first is None:
                        first = phi
                        if medium == "thick" and R > 1.0:
                            assert (phi == 0).sum() > (phi != 0).sum() > 0
                    elif "OPT_FORTRAN_CONSTANTS" not in opts:      # (the same rates: one addition per cell, then the twin fold)
                        np.testing.assert_allclose(phi, first, rtol=1e-13, atol=0, err_msg=f"{medium} R={R} {opts}")
            # the forms that do not exist with heating: forced, the library falls back to the single-source form -- same bits
            ref_phi = _identity_launch(lib, capi, N, R, n, dr, numtau, dlog, {"OPT_SKIP_ZERO_RATES": 2}, seen)[0]
            for opts in ({"OPT_SKIP_ZERO_RATES": 1}, {"OPT_SKIP_ZERO_RATES": 0}, {"OPT_PAIR_SOURCES": 2},
                         {"OPT_PAIR_SOURCES": 2, "OPT_SKIP_ZERO_RATES": 1, "OPT_SECTORS": 9}):
                phi = _identity_launch(lib, capi, N, R, n, dr, numtau, dlog, opts, seen)[0]
                if opts.get("OPT_SECTORS") is None:
                    assert np.array_equal(phi, ref_phi), (medium, R, opts)

    # overlapping spheres and black-body tables against the oracle (both constant sets, a few decompositions, both families)
    bthin, bthick, bhthin, bhthick, bdlog = cases.blackbody_photo_and_heat_tables(num_tau=400)
    p.photo_table_to_device(bthin, bthick)
    lib.heat_table_to_device(bhthin, bhthick, bthin.shape[0])
    lib.grid_to_device(capi.GRID_NDENS, nd)
    lib.source_data_to_device(p0, f0, 80)
    R = 9.0
    for fortran in (0, 1):
        flags = O.PER_SOURCE_FLUX if fortran else O.ASORA_MODE
        ref = O.asora_do_all_sources(R, cases.SIG, dr, nd, xh, p0, f0, bthin, bthick, cases.MINLOGTAU, bdlog,
                                     NumTau=bthin.shape[0], flags=flags, heat_thin=bhthin, heat_thick=bhthick)
        w = ref["phi_heat"] != 0
        assert np.array_equal(ref["phi_ion"] != 0, w) and w.sum() > 80 * 1000
        for opts in ({}, {"OPT_SECTORS": 1}, {"OPT_SECTORS": 3, "OPT_BLOCK_THREADS": 128}, {"OPT_SECTORS": 6},
                     {"OPT_SECTORS": 9, "OPT_GLOBAL_ATOMICS": 1}, {"OPT_Z_TRANSPOSED": 0}):
            opts = dict(opts, OPT_HEATING=1, OPT_FORTRAN_CONSTANTS=fortran)
            _set(lib, capi, opts)
            try:
                lib.raytrace_device(R, cases.SIG, dr, 0, 80, cases.MINLOGTAU, bdlog, bthin.shape[0])
                seen.add(_form(lib, lib.last_raytrace_variant()))
                phi = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
                heat = lib.grid_to_host(capi.GRID_PHI_HEAT, np.empty((N, N, N)))
            finally:
                _reset(lib, capi, opts)
            assert np.array_equal(heat != 0, w) and np.array_equal(phi != 0, w), opts
            np.testing.assert_allclose(heat[w], ref["phi_heat"][w], rtol=GAMMA_RTOL, atol=0, err_msg=str(opts))
            np.testing.assert_allclose(phi[w], ref["phi_ion"][w], rtol=GAMMA_RTOL, atol=0, err_msg=str(opts))

    # N = 168, one source, R beyond the box: the shells outgrow LDS for one workgroup per octant (global shell scratch);
    # 85 shells: the 256-entry tables also at 64 and 128 threads
    N = 168
    nd, xh, dr = cases.grid(N, "lognormal", 41, 0.02)
    pos, flux = cases.sources(N, 1, 42, flux=5.0)
    q0, g0 = cases.flat_sources(pos, flux)
    thin, thick, dlog = cases.grey_tables()
    _fresh(p, N)
    p.photo_table_to_device(thin, thick)
    lib.heat_table_to_device(P2 * thin, P2 * thick, thin.shape[0])
    lib.grid_to_device(capi.GRID_NDENS, nd)
    lib.grid_to_device(capi.GRID_XH_AV, xh)
    lib.source_data_to_device(q0, g0, 1)
    for opts in ({}, {"OPT_SECTORS": 1}, {"OPT_SECTORS": 2}, {"OPT_SECTORS": 4, "OPT_BLOCK_THREADS": 64},
                 {"OPT_SECTORS": 4, "OPT_BLOCK_THREADS": 128}, {"OPT_SECTORS": 2, "OPT_BLOCK_THREADS": 64},
                 {"OPT_SECTORS": 2, "OPT_BLOCK_THREADS": 128}):
        for glob in (0, 1):
            _identity_launch(lib, capi, N, 1000.0, 1, dr, thin.shape[0] - 1, dlog, dict(opts, OPT_GLOBAL_ATOMICS=glob), seen)
    # ... and black-body heating against the oracle on the global-shell form and the default one
    p.photo_table_to_device(bthin, bthick)
    lib.heat_table_to_device(bhthin, bhthick, bthin.shape[0])
    ref = O.asora_do_all_sources(1000.0, cases.SIG, dr, nd, xh, q0, g0, bthin, bthick, cases.MINLOGTAU, bdlog,
                                 NumTau=bthin.shape[0] - 1, flags=O.ASORA_MODE, heat_thin=bhthin, heat_thick=bhthick)
    for opts in ({"OPT_SECTORS": 1}, {}):
        _set(lib, capi, dict(opts, OPT_HEATING=1))
        try:
            lib.raytrace_device(1000.0, cases.SIG, dr, 0, 1, cases.MINLOGTAU, bdlog, bthin.shape[0] - 1)
            v = lib.last_raytrace_variant()
            heat = lib.grid_to_host(capi.GRID_PHI_HEAT, np.empty((N, N, N)))
        finally:
            _reset(lib, capi, dict(opts, OPT_HEATING=1))
        if opts:
            assert v["global_shells"], v
        np.testing.assert_allclose(heat, ref["phi_heat"], rtol=GAMMA_RTOL, atol=0, err_msg=str(opts))
    p.device_close()

    print("heating forms seen:", sorted(seen))
    missing = REQUIRED_FORMS - seen
    assert not missing, f"heating forms not run: {sorted(missing)}; seen: {sorted(seen)}"
    assert any(f[0] == "global_shells" for f in seen), sorted(seen)


# ---- 3b: the thermal fused pass in isolation ---------------------------------------------------------------------------
def _thermal_medium(N, seed):
    rng = np.random.default_rng(seed)
    s = (N, N, N)
    n = 1e-3 * np.exp(0.8 * rng.standard_normal(s) - 0.32)
    xh = 10 ** rng.uniform(-4, -1, s)
    T = 10 ** rng.uniform(2, 4.3, s)
    return n, xh, T


def _sample_cells(N, rng):
    """Whole j-planes (the middle index: a workgroup's trip of the j loop) -- the first, the last, some far beyond the first
    trip (j >= gridDim.y) -- and random cells."""
    planes = sorted({0, 1, N - 1, N // 2} | set(int(j) for j in rng.integers(0, N, 3)) | ({100, 150, 170} if N > 170 else set()))
    m = np.zeros((N, N, N), dtype=bool)
    m[:, planes, :] = True
    m.ravel()[rng.integers(0, N ** 3, 20000)] = True
    return m


def _nconv(xav, xav_in):
    y = 1.0 - xav_in
    return int(np.count_nonzero((np.abs(xav - xav_in) > TR.MIN_FRAC_CHANGE) & (np.abs((xav - xav_in) / y) > TR.MIN_FRAC_CHANGE)
                                & (y > TR.MIN_FRAC_ATOMS)))


@pytest.mark.parametrize("N,ns,R", [(17, 3, 2.5), (40, 4, 3.5), (197, 5, 4.5), (200, 4, 3.0), (17, 2, 1000.0), (200, 1, 1000.0)])
def test_thermal_fused_pass_against_the_reference_on_the_rates_it_read(asora, N, ns, R):
    """chemistry_tile_kernel<true,true,false,true>, one iteration at a time (evolve_enqueue(1) + evolve_poll, a step that
    never converges): after each, PHI_ION / PHI_HEAT hold exactly the folded rates that iteration's pass consumed, and
    its x_av input was XH (first iteration) or the previous XH_AV.  The numpy statement of the pass on those grids must give
    XH_AV, XH_INTERMED, TEMP_END, the history row's conv_flag and sums and asora_thermal_stats; the rates themselves are
    checked against the oracle on the same x_av -- three iterations, so the third traces into the heating pair the second
    pass had to zero.  N = 197 / 200: several j per workgroup (the second and later trips of the j loop, the barrier
    before the LDS tiles are refilled); 17 / 197: partial 32-tiles and partial 8-cell lines; small R: the reach mask (lines
    no source reaches are neither read nor zeroed); R beyond the box: no mask.  At N >= 197 the reference runs on whole
    j-planes and a random sample of cells (the rest of the grid enters through conv_flag and the sums)."""
    p, lib, capi = asora
    rng = np.random.default_rng(1000 + N + ns)
    n, xh, T = _thermal_medium(N, N + ns)
    thin, thick, hthin, hthick, dlog = cases.blackbody_photo_and_heat_tables(num_tau=600)
    numtau = thin.shape[0]
    pos = 1 + rng.integers(0, N, size=(3, ns))
    if ns > 1:
        pos[:, 0] = [1, 1, N]                                   # wraps
    flux = rng.uniform(0.5, 2.0, ns) * 1e-2
    dr = 3.086e21 * 0.1
    dt = 3.15576e13
    prm = TR.Params(relative_denergy=0.1, t_floor=1.0, max_substeps=400, cooling_mask=31, compton=True, t_cmb=2.7255 * 9.0)
    _fresh(p, N)
    p.photo_table_to_device(thin, thick)
    lib.heat_table_to_device(hthin, hthick, numtau)
    p0, f0 = cases.flat_sources(pos, flux)
    lib.source_data_to_device(p0, f0, ns)
    lib.grid_to_device(capi.GRID_NDENS, n)
    lib.grid_to_device(capi.GRID_TEMP, T)
    lib.grid_to_device(capi.GRID_XH, xh)
    g = lambda w: lib.grid_to_host(w, np.empty((N, N, N)))
    full = N <= 64
    sel = np.ones((N, N, N), dtype=bool) if full else _sample_cells(N, rng)
    lib.thermal_params(True, prm.relative_denergy, prm.t_floor, prm.max_substeps, prm.cooling_mask, prm.compton, prm.t_cmb)
    try:
        lib.evolve_begin(cases.MYR, *CHEM, R, cases.SIG, dr, cases.MINLOGTAU, dlog, numtau, 0, ns, -1.0, 0.0)
        xav_in = xh
        tot = [0, 0, 0]
        for it in range(3):
            lib.evolve_enqueue(1)
            niter, done, rows = lib.evolve_poll()
            assert niter == it + 1 and not done and len(rows) == 1
            stats = lib.thermal_stats()
            phi, heat = g(capi.GRID_PHI_ION), g(capi.GRID_PHI_HEAT)
            xa, xi, te = g(capi.GRID_XH_AV), g(capi.GRID_XH_INTERMED), g(capi.GRID_TEMP_END)
            tag = f"N={N} ns={ns} R={R} iteration {it + 1}"
            # the rates the pass read, against the oracle on the same x_av
            ref = O.asora_do_all_sources(R, cases.SIG, dr, n, xav_in, p0, f0, thin, thick, cases.MINLOGTAU, dlog, NumTau=numtau,
                                         flags=O.ASORA_MODE, heat_thin=hthin, heat_thick=hthick)
            w = ref["phi_ion"] != 0
            assert w.sum() > 0 and np.array_equal(phi != 0, w) and np.array_equal(heat != 0, w), tag
            np.testing.assert_allclose(phi[w], ref["phi_ion"][w], rtol=GAMMA_RTOL, atol=0, err_msg=tag)
            np.testing.assert_allclose(heat[w], ref["phi_heat"][w], rtol=GAMMA_RTOL, atol=0, err_msg=tag)
            # the pass on those rates
            rxi, rxa, rte, rconv, rstats, delta, capped = TR.chemistry_thermal(
                prm, dt, n[sel], T[sel], xh[sel], xav_in[sel], phi[sel], heat[sel], *CHEM, return_delta=True)
            well = (delta > WELL_CONDITIONED) & ~capped
            assert well.any(), tag
            for got, want, rtol in ((xi[sel], rxi, ILL_RTOL), (xa[sel], rxa, ILL_RTOL_XAV), (te[sel], rte, ILL_RTOL)):
                np.testing.assert_allclose(got[well], want[well], rtol=1e-10, atol=0, err_msg=tag)
                np.testing.assert_allclose(got, want, rtol=rtol, atol=0, err_msg=tag)
            conv, s1, s0 = rows[0][0], rows[0][1], rows[0][2]
            assert int(conv) == _nconv(xa, xav_in), tag            # the device's own count of its own fields
            assert s1 == pytest.approx(xi.sum(), rel=1e-12) and s0 == pytest.approx((1.0 - xi).sum(), rel=1e-12), tag
            tot = [tot[0] + rstats[0], tot[1] + rstats[1], max(tot[2], rstats[2])]
            if full:
                assert int(conv) == rconv, tag
                assert tuple(stats) == tuple(tot), (tag, stats, tot)
            else:
                assert stats[0] >= tot[0] and stats[1] >= tot[1] and stats[2] >= tot[2], (tag, stats, tot)
            assert np.any(te > T) and heat.max() > 0, tag
            xav_in = xa
    finally:
        lib.thermal_params(False)
    p.device_close()


# ---- 3c: whole thermal steps against the oracle loop -----------------------------------------------------------------
def _non_overlapping(N, ns, R, rng):
    """ns sources on the lattice of spacing N // 2 (one on a box corner), R small enough that no two spheres share a cell."""
    h = N // 2
    assert 2 * int(np.floor(R)) < h
    pts = np.array([(1 + a * h, 1 + b * h, 1 + c * h) for a in (0, 1) for b in (0, 1) for c in (0, 1)]).T
    pick = np.concatenate([[0], 1 + rng.permutation(7)[:ns - 1]])
    return pts[:, pick]


def test_randomised_thermal_steps_against_the_oracle_loop(asora, tmp_path):
    """Seeded sweep of whole thermal time steps through evolve3D(..., thermal=ThermalParams(...)) against
    evolve3D_thermal_oracle: odd and even meshes, 0-6 sources (0: cooling only), radii from one cell to beyond the box,
    cooling masks 0 ... 31, Compton on and off, a small max_substeps, two consecutive steps (the second with another source
    set or radius, from the first step's x and T).  Equal iteration counts; x, T and both rate grids to the tolerances of
    the thermal tests, split by conditioning.  In the same sweep, with 2^-35-scaled tables and non-overlapping sources:
    PHI_HEAT == 2^-35 PHI_ION bit for bit after every step (stale heating accumulators would show)."""
    from pyc2ray_amd.thermal import ThermalParams
    from evolve_oracle import evolve3D_thermal_oracle
    p, lib, capi = asora
    # (a seed whose steps all converge: the loop, the reference's as well, has no iteration limit -- with other draws a step
    #  can cycle for ever between two states of its capped cells, and evolve3D then never returns; the oracle runs first)
    rng = np.random.default_rng(4243)
    bb = cases.blackbody_photo_and_heat_tables(num_tau=600)
    checked_identity = 0
    max_iter_seen = 0
    for trial in range(10):
        identity = trial % 3 == 2
        N = int(rng.choice([17, 20, 24, 33, 40]))
        thin, thick, hthin, hthick, dlog = bb
        if identity:
            hthin, hthick = P2 * thin, P2 * thick
        mask = int(rng.choice([0, 31, 1, 3, 8, 24, 31]))
        compton = bool(rng.integers(0, 2))
        max_sub = int(rng.choice([10000, 40]))
        zred = 8.0 if compton else None
        prm = TR.Params(relative_denergy=0.1, t_floor=1.0, max_substeps=max_sub, cooling_mask=mask, compton=compton,
                        t_cmb=0.0 if zred is None else 2.7255 * (1.0 + zred))
        tp = ThermalParams(hthin, hthick, relative_denergy=0.1, t_floor=1.0, max_substeps=max_sub, cooling=mask, zred=zred)
        assert tp.t_cmb == prm.t_cmb
        nd, xh, dr = cases.grid(N, "lognormal", 900 + trial, float(10 ** rng.uniform(-1.5, 0.3)), xlo=1e-4, xhi=2e-3)
        temp = 10 ** rng.uniform(2.0, 4.0, size=(N, N, N))
        dt = 3.15576e13 * float(rng.choice([0.5, 2.0]))
        _fresh(p, N)
        p.photo_table_to_device(thin, thick)
        x, T, x_ref, T_ref = xh, temp, xh, temp
        for step in range(2):
            if identity:
                R = float(rng.choice([1.0, 2.5, (N // 2 - 1) / 2.0]))
                ns = int(rng.integers(1, 7))
                pos = _non_overlapping(N, ns, R, rng)
            else:
                ns = int(rng.integers(0, 7))
                R = float(rng.choice([1.0, 2.5, 4.0, N / 3.0, N * 0.8, 1000.0]))
                pos = 1 + rng.integers(0, N, size=(3, ns))
            flux = rng.uniform(0.5, 2.0, size=ns) * 3e-4 * (N / 16.0) ** 3 / max(ns, 1)
            if trial == 0 and step == 0:        # no source: cooling only
                ns, pos, flux = 0, pos[:, :0], flux[:0]
            tag = (f"trial {trial} step {step}: N={N} ns={ns} R={R:g} mask={mask} compton={compton} max_substeps={max_sub} "
                   f"identity={identity}")
            x_ref, T_ref, phi_ref, heat_ref, niter_ref, hist, delta, capped = evolve3D_thermal_oracle(
                prm, dt, dr, flux, pos, T_ref, nd, x_ref, thin, thick, hthin, hthick, cases.MINLOGTAU, dlog, R, 1e-4,
                cases.SIG, *CHEM, max_iter=100, return_delta=True)
            assert niter_ref < 100, tag
            x, phi, T = p.evolve3D(dt, dr, flux, pos, True, 1000, N, 1e-2, T, nd, x, thin, thick, cases.MINLOGTAU, dlog, R,
                                   1e-4, cases.SIG, *CHEM, logfile=str(tmp_path / "log"), quiet=True, thermal=tp)
            heat = lib.grid_to_host(capi.GRID_PHI_HEAT, np.empty((N, N, N)))
            niter = p.evolve._evolve.last_niter
            max_iter_seen = max(max_iter_seen, niter)
            assert niter == niter_ref, tag
            well = (delta > WELL_CONDITIONED) & ~capped
            np.testing.assert_allclose(x[well], x_ref[well], rtol=1e-10, atol=0, err_msg=tag)
            np.testing.assert_allclose(T[well], T_ref[well], rtol=1e-10, atol=0, err_msg=tag)
            np.testing.assert_allclose(x, x_ref, rtol=ILL_RTOL, atol=0, err_msg=tag)
            np.testing.assert_allclose(T, T_ref, rtol=ILL_RTOL, atol=0, err_msg=tag)
            if ns:
                for got, want in ((phi, phi_ref), (heat, heat_ref)):
                    w = want != 0
                    assert np.array_equal(got != 0, w), tag
                    np.testing.assert_allclose(got, want, rtol=1e-7, atol=1e-13 * want.max(), err_msg=tag)
            else:
                assert not phi.any() and not heat.any(), tag
            if identity:
                assert np.array_equal(heat, P2 * phi), tag
                checked_identity += 1
    assert checked_identity >= 4 and max_iter_seen >= 3, (checked_identity, max_iter_seen)
    p.device_close()
