"""GPU: the thermal (non-isothermal) mode -- asora_thermal_params, the thermal form of the chemistry pass, the device loop
with heating, and the C2Ray class with `Material: isothermal: false`.  The checker is the numpy statement of the scheme,
tests/thermal_reference.py; the kernel evaluates it without FMA contraction, so the differences are those of the device's
exp / pow / log10 against libm (a few ulps per call)."""
import os

import numpy as np
import pytest

import cases
import thermal_reference as TR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BB_PARAMS = os.path.join(HERE, "data", "parameters_single_black_body.yml")
CHEM = (cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)
# doric's x_av = eqxh + (x0 - eqxh) (1 - e^-D) / D, D = delth dt, loses log10(1/D) digits: in the slow cells of the random grids
# (D down to 1e-12) one ulp of the device's exp against libm's moves x_av by up to ~1e-4 relative, and x_intermed / T_end, which
# follow it through the inner iteration, by up to ~1e-8 (at D = 1e-3 x_av still shows 1.5e-10).  Cells with D > WELL_CONDITIONED
# are held to 1e-10; the rest to the tolerances below.  So are the cells whose integration hit max_substeps: their last substep
# jumps to the end of the step, (e + h r) cancels, and the difference of an ulp in r is amplified by h |r| / e.
WELL_CONDITIONED = 1e-2
ILL_RTOL_XAV, ILL_RTOL = 1e-3, 1e-7


def _compare(got, ref, well, rtol_ill):
    np.testing.assert_allclose(got[well], ref[well], rtol=1e-10, atol=0)
    np.testing.assert_allclose(got, ref, rtol=rtol_ill, atol=0)


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


def _init(p, lib, N):
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)
    thin, thick, dlog = cases.soft_tables()
    p.photo_table_to_device(thin, thick)
    lib.heat_table_to_device(3e-11 * thin, 2.5e-11 * thick, thin.shape[0])
    return thin, thick, dlog


def _random_cells(N, seed, zero_rates=False):
    rng = np.random.default_rng(seed)
    s = (N, N, N)
    n = 10 ** rng.uniform(-4, 1, s)
    T = 10 ** rng.uniform(1, 5, s)
    xh = 10 ** rng.uniform(-4, 0, s) * 0.999
    xav = np.clip(xh * 10 ** rng.uniform(-0.3, 0.3, s), 1e-6, 0.999)
    gamma = np.where(rng.random(s) < 0.3, 0.0, 10 ** rng.uniform(-16, -11, s))
    heat = gamma * 10 ** rng.uniform(-12, -10.5, s)
    if zero_rates:
        gamma, heat = np.zeros(s), np.zeros(s)
    return n, T, xh, xav, gamma, heat


def _upload(lib, capi, n, T, xh, xav, gamma, heat):
    lib.grid_to_device(capi.GRID_NDENS, n)
    lib.grid_to_device(capi.GRID_TEMP, T)
    lib.grid_to_device(capi.GRID_XH, xh)
    lib.grid_to_device(capi.GRID_XH_AV, xav)
    lib.grid_to_device(capi.GRID_PHI_ION, gamma)
    lib.grid_to_device(capi.GRID_PHI_HEAT, heat)


# name -> (cooling mask, compton, max_substeps, zero rates)
PASS_CASES = {
    "recombination": (1, False, 400, False),
    "collisional_ionisation": (2, False, 400, False),
    "collisional_excitation": (4, False, 400, False),
    "bremsstrahlung": (8, False, 400, False),
    "compton": (16, True, 400, False),
    "all": (31, True, 400, False),
    "all_no_rates": (31, True, 400, True),
    "all_capped": (31, True, 6, False),
}


@pytest.mark.parametrize("N,name", [(24, k) for k in PASS_CASES] + [(33, "all"), (33, "all_capped")])
def test_isolated_thermal_pass_matches_the_reference(asora, N, name):
    p, lib, capi = asora
    _init(p, lib, N)
    mask, compton, max_sub, zero = PASS_CASES[name]
    n, T, xh, xav, gamma, heat = _random_cells(N, 100 + N + len(name), zero)
    dt = 1e11
    prm = TR.Params(relative_denergy=0.1, t_floor=1.0, max_substeps=max_sub, cooling_mask=mask, compton=compton,
                    t_cmb=2.7255 * 11.0)
    _upload(lib, capi, n, T, xh, xav, gamma, heat)
    lib.thermal_params(True, prm.relative_denergy, prm.t_floor, prm.max_substeps, prm.cooling_mask, prm.compton, prm.t_cmb)
    try:
        conv, s1, s0 = lib.chemistry_device(dt, *CHEM)
        stats = lib.thermal_stats()
    finally:
        lib.thermal_params(False)
    xi = lib.grid_to_host(capi.GRID_XH_INTERMED, np.empty((N, N, N)))
    xa = lib.grid_to_host(capi.GRID_XH_AV, np.empty((N, N, N)))
    te = lib.grid_to_host(capi.GRID_TEMP_END, np.empty((N, N, N)))
    rxi, rxa, rte, rconv, rstats, delta, capped = TR.chemistry_thermal(prm, dt, n, T, xh, xav, gamma, heat, *CHEM,
                                                                       return_delta=True)
    well = (delta > WELL_CONDITIONED) & ~capped
    assert well.sum() > 1000
    _compare(xi, rxi, well, ILL_RTOL)
    _compare(xa, rxa, well, ILL_RTOL_XAV)
    _compare(te, rte, well, ILL_RTOL)
    assert conv == rconv
    assert tuple(stats) == rstats
    assert s1 == pytest.approx(rxi.sum(), rel=1e-12)
    if name == "all_capped":
        assert stats[0] > 0 and stats[2] == max_sub
    if name == "all":
        assert np.any(te > T) and np.any(te < T)                       # heated and cooled cells


def test_noop_thermal_pass_is_the_isothermal_pass(asora):
    """No cooling channel and no heating: the temperature stays, and the ionisation is the isothermal pass's."""
    p, lib, capi = asora
    N = 24
    _init(p, lib, N)
    n, T, xh, xav, gamma, _ = _random_cells(N, 7)
    heat = np.zeros_like(gamma)
    dt = 1e12
    out = {}
    for thermal in (False, True):
        _upload(lib, capi, n, T, xh, xav, gamma, heat)
        if thermal:
            lib.thermal_params(True, 0.1, 1.0, 10000, 0, False, 0.0)
        try:
            conv = lib.chemistry_device(dt, *CHEM)
        finally:
            lib.thermal_params(False)
        out[thermal] = (conv, lib.grid_to_host(capi.GRID_XH_INTERMED, np.empty((N, N, N))),
                        lib.grid_to_host(capi.GRID_XH_AV, np.empty((N, N, N))))
    te = lib.grid_to_host(capi.GRID_TEMP_END, np.empty((N, N, N)))
    np.testing.assert_allclose(te, T, rtol=1e-15, atol=0)        # (one substep: T = (c T) / c)
    assert out[True][0][0] == out[False][0][0]
    # (the isothermal pass is compiled with FMA contraction, the thermal one without: the same ill-conditioning as above)
    delta = TR.chemistry_thermal(TR.Params(cooling_mask=0), dt, n, T, xh, xav, gamma, heat, *CHEM, return_delta=True)[5]
    well = delta > 1e-1
    np.testing.assert_allclose(out[True][1][well], out[False][1][well], rtol=1e-13, atol=0)
    np.testing.assert_allclose(out[True][2][well], out[False][2][well], rtol=1e-13, atol=0)
    np.testing.assert_allclose(out[True][1], out[False][1], rtol=ILL_RTOL, atol=0)
    np.testing.assert_allclose(out[True][2], out[False][2], rtol=ILL_RTOL_XAV, atol=0)


def _loop_case(N=32, seed=5):
    rng = np.random.default_rng(seed)
    ns = 4
    pos = rng.integers(1, N + 1, size=(3, ns))
    flux = 10 ** rng.uniform(-1.5, -0.5, ns)
    n = 1e-3 * 10 ** rng.uniform(-0.3, 0.3, (N, N, N))
    xh = np.full((N, N, N), 1.2e-3)
    T = np.full((N, N, N), 100.0)
    return pos, flux, n, xh, T


def _device_step(lib, capi, N, chem, R, dr, dlog, numtau, nsrc, conv_frac, prm):
    crit = min(int(conv_frac * N ** 3), (nsrc - 1) / 3)
    lib.thermal_params(True, prm.relative_denergy, prm.t_floor, prm.max_substeps, prm.cooling_mask, prm.compton, prm.t_cmb)
    try:
        lib.evolve_begin(*chem, R, cases.SIG, dr, cases.MINLOGTAU, dlog, numtau, 0, nsrc, crit, conv_frac)
        done, niter = False, 0
        while not done:
            lib.evolve_enqueue(4)
            niter, done, _ = lib.evolve_poll(0)
        stats = lib.thermal_stats()
    finally:
        lib.thermal_params(False)
    g = lambda w: lib.grid_to_host(w, np.empty((N, N, N)))
    return niter, g(capi.GRID_XH_INTERMED), g(capi.GRID_XH_AV), g(capi.GRID_PHI_ION), g(capi.GRID_PHI_HEAT), g(capi.GRID_TEMP_END), stats


@pytest.mark.parametrize("mask", [31, 0])
def test_device_loop_equals_host_loop_of_isolated_calls(asora, mask):
    """The asora_evolve_* loop in thermal mode == the loop of evolve.py:168-240 over the isolated calls: a trace with heating
    (ASORA_OPT_HEATING), then the thermal asora_chemistry_device.  mask = 0 (cooling off) also checks the energy
    bookkeeping of a real traced step: the gas gains exactly the heat deposited by the last iteration's rates."""
    p, lib, capi = asora
    N = 32
    thin, thick, dlog = _init(p, lib, N)
    pos, flux, n, xh, T = _loop_case(N)
    pos0, f0 = cases.flat_sources(pos, flux)
    lib.source_data_to_device(pos0, f0, flux.shape[0])
    numtau = thin.shape[0]
    dt, dr, R, conv_frac = 3.15576e13, 3.086e21 * 0.4, 12.0, 1e-4
    chem = (dt,) + CHEM
    prm = TR.Params(cooling_mask=mask, compton=False)
    lib.grid_to_device(capi.GRID_NDENS, n)
    lib.grid_to_device(capi.GRID_TEMP, T)
    lib.grid_to_device(capi.GRID_XH, xh)
    dev = _device_step(lib, capi, N, chem, R, dr, dlog, numtau, flux.shape[0], conv_frac, prm)

    # host-driven loop over the isolated calls
    lib.grid_to_device(capi.GRID_XH, xh)
    lib.grid_copy(capi.GRID_XH_AV, capi.GRID_XH)
    crit = min(int(conv_frac * N ** 3), (flux.shape[0] - 1) / 3)
    prev1 = prev0 = 2.0 * N ** 3
    niter, converged = 0, False
    lib.set_option(capi.OPT_HEATING, 1)
    lib.thermal_params(True, prm.relative_denergy, prm.t_floor, prm.max_substeps, prm.cooling_mask, prm.compton, prm.t_cmb)
    try:
        while not converged and niter < 100:
            niter += 1
            lib.raytrace_device(R, cases.SIG, dr, 0, flux.shape[0], cases.MINLOGTAU, dlog, numtau)
            conv, s1, s0 = lib.chemistry_device(*chem)
            rel1 = abs((s1 - prev1) / s1) if s1 > 0 else 1.0
            rel0 = abs((s0 - prev0) / s0) if s0 > 0 else 1.0
            converged = conv < crit or (rel1 < conv_frac and rel0 < conv_frac)
            prev1, prev0 = s1, s0
    finally:
        lib.set_option(capi.OPT_HEATING, 0)
        lib.thermal_params(False)
    g = lambda w: lib.grid_to_host(w, np.empty((N, N, N)))
    host = (niter, g(capi.GRID_XH_INTERMED), g(capi.GRID_XH_AV), g(capi.GRID_PHI_ION), g(capi.GRID_PHI_HEAT), g(capi.GRID_TEMP_END))
    assert dev[0] == host[0] and dev[0] > 1
    for a, b in zip(dev[1:6], host[1:6]):
        np.testing.assert_allclose(a, b, rtol=1e-10, atol=0)
    te, xav, heat = dev[5], dev[2], dev[4]
    assert heat.max() > 0 and te.max() > 5e3
    if mask == 0:
        gained = np.sum(1.5 * TR.K_B * n * (1.0 + xav + cases.ABU_C) * (te - T))
        deposited = dt * np.sum(n * (1.0 - xav) * heat)
        # (1e-12: the per-cell differences T_end - T_start of barely heated cells carry the rounding of their energies)
        assert gained == pytest.approx(deposited, rel=1e-12)
    # an isothermal step afterwards is untouched by what the thermal one left behind
    lib.grid_to_device(capi.GRID_XH, xh)
    lib.evolve_begin(*chem, R, cases.SIG, dr, cases.MINLOGTAU, dlog, numtau, 0, flux.shape[0], crit, conv_frac)
    done = False
    while not done:
        lib.evolve_enqueue(4)
        _, done, _ = lib.evolve_poll(0)
    iso = g(capi.GRID_XH_INTERMED)
    assert np.all(np.isfinite(iso)) and not np.allclose(iso, dev[1], rtol=1e-3)


def test_thermal_mode_refusals(asora):
    p, lib, capi = asora
    N = 16
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)
    thin, thick, dlog = cases.soft_tables()
    p.photo_table_to_device(thin, thick)
    with pytest.raises(RuntimeError, match=r"code 4\).*heating tables"):
        lib.thermal_params(True)
    lib.heat_table_to_device(thin, thick, thin.shape[0])
    lib.thermal_params(True)
    try:
        with pytest.raises(RuntimeError, match="single-GPU"):
            lib.evolve_begin_slab(1e13, *CHEM, 4.0, cases.SIG, 1e21, cases.MINLOGTAU, dlog, thin.shape[0], 0, 0, 0, 1e-4, 0, N)
    finally:
        lib.thermal_params(False)
    assert lib.thermal_stats() == (0, 0, 0)


def _params_file(path, cosmological=False, iliev=False):
    base = open(BB_PARAMS).read()
    base = (base.replace("Material:\n", "Material:\n  isothermal: false\n").replace("compute_heating_rates: 0", "compute_heating_rates: 1")
                .replace("NumTau: 10000", "NumTau: 2000"))
    if iliev:   # Iliev et al. (2006) Test 2: n = 1e-3, T0 = 100 K, 1e5 K black body; 13.2 kpc box (the source in the middle)
        base = (base.replace("boxsize: 0.014", "boxsize: 0.0132").replace("avg_dens: 1.0e-6", "avg_dens: 1.0e-3")
                    .replace("temp0: 1e4", "temp0: 100.0").replace("Teff: 5e4", "Teff: 1e5")
                    .replace("R_max_cMpc: 0.01640625", "R_max_cMpc: 0.0066").replace("zred_0: 9.0", "zred_0: 0.0"))
    if cosmological:
        base = base.replace("cosmological: 0", "cosmological: 1")
    with open(path, "w") as f:
        f.write(base)
    return path


def test_iliev_test2_hii_region(asora, tmp_path):
    """A Test-2-style H II region (Iliev et al. 2006) with the temperature evolved: 64^3, 5e48 photons/s, ten 10 Myr steps."""
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        if p.cuda_is_init():
            p.device_close()
        N = 64
        _params_file("parameters.yml", iliev=True)
        with open("source.txt", "w") as f:
            f.write("1\n33 33 33 5e48 1.0\n")
        sim = pc2r.C2Ray_Test("parameters.yml", N, True)
        assert not sim.isothermal and not sim.cosmological
        sim.density_init(0.0)
        assert sim.ndens.mean() == pytest.approx(1e-3)
        srcpos, srcflux = sim.read_sources("source.txt", 1)
        myr = 1e6 * 3.15576e7
        for _ in range(10):
            sim.evolve3D(10 * myr, srcflux, srcpos)
        T, x = sim.temp, sim.xh
        assert np.all(np.isfinite(T)) and T.min() >= 1.0
        Tbar = T[x > 0.9].mean()
        assert 8e3 <= Tbar <= 4e4, Tbar
        alpha = sim.bh00 * (Tbar / 1e4) ** sim.albpow
        n = 1e-3
        r_s = (3 * 5e48 / (4 * np.pi * alpha * n * n)) ** (1 / 3)
        t_rec = 1.0 / (alpha * n)
        expect = r_s * (1 - np.exp(-100 * myr / t_rec)) ** (1 / 3)
        front = (3 / (4 * np.pi) * x.sum() * sim.dr ** 3) ** (1 / 3)
        assert front == pytest.approx(expect, rel=0.1), (front / expect, Tbar)
        assert T[x < 0.01].mean() < 1e3                  # the medium beyond the front stays cold
        p.device_close()
    finally:
        os.chdir(cwd)


@pytest.mark.parametrize("cosmological", [False, True])
def test_resident_and_host_class_runs_agree(asora, tmp_path, cosmological):
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 24
        _params_file("parameters.yml", cosmological=cosmological)
        with open("src.txt", "w") as f:
            f.write("2\n12 12 12 6e50 1.0\n5 20 9 2e50 1.0\n")
        runs = {}
        for resident in (False, True):
            if p.cuda_is_init():
                p.device_close()
            sim = pc2r.C2Ray_Test("parameters.yml", N, True)
            sim.device_resident = resident
            srcpos, srcflux = sim.read_sources("src.txt", 2)
            zs = sim.generate_redshift_array(2, 4e7)
            dt = sim.set_timestep(zs[0], zs[1], 3)
            sim.density_init(zs[0])
            snaps = []
            for step in range(3):
                sim.cosmo_evolve(dt)
                sim.evolve3D(dt, srcflux, srcpos)
                if step >= 1:
                    snaps.append((np.array(sim.xh, copy=True), np.array(sim.temp, copy=True)))
            runs[resident] = snaps
            p.device_close()
        for (x0, t0), (x1, t1) in zip(runs[False], runs[True]):
            np.testing.assert_allclose(x1, x0, rtol=1e-12, atol=0)
            np.testing.assert_allclose(t1, t0, rtol=1e-12, atol=0)
        x, T = runs[True][-1]
        assert x.max() > 0.5 and T.max() > 5e3 and T.min() >= 1.0
    finally:
        os.chdir(cwd)
