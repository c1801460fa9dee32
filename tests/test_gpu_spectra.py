"""GPU: per-source spectra -- several rate-table sets on the device, each source rated with its own.

The main check is a power-of-two identity.  The tables of spectrum s are 2^-s x the tables of spectrum 0.  Every operation
that forms a rate from a table value -- the interpolation fma(residual, T[i+1] - T[i], T[i]), pref (T_in - T_out), pref dtau T --
commutes with a scaling by a power of two, and with sources whose spheres do not overlap every cell receives one addition, so
inside the sphere of a source of spectrum s the rates are 2^-s x the rates of the same call with every source on spectrum 0,
bit for bit.  A wrong base pointer for the second source of a pair, a spectrum lost in the position sort or a heating block
taken from the wrong set all break it.  Then two black-body spectra against the CPU oracle, the one-spectrum regression, the
device loop against a host loop of isolated calls, and the refusals.
"""
import numpy as np
import pytest

import cases
from _spectra_dist_worker import hard_tables
from oracle import oracle as O

pytestmark = pytest.mark.gpu

K = 3
P2 = 2.0 ** -35                     # heating tables of the identity runs (tests/test_gpu_heating.py)
GAMMA_RTOL = 1e-8                   # the rate tolerance of tests/test_gpu_parity.py
CHEM = (cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)
N_ID = 96


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


def _scaled_sets(thin, thick, k=K):
    """(k, NumTau) tables, set s = 2^-s x set 0 (exact in FP64)."""
    f = (2.0 ** -np.arange(k))[:, None]
    return f * thin[None, :], f * thick[None, :]


def _apart_sources(N, R, seed):
    """Sources (3, n) 1-based whose spheres of radius R do not touch in the periodic box (centre distance >= 2 R + 1), as many as
    a cubic or body-centred lattice gives; one sits on the box corner, so the periodic wrap is in play."""
    m = max(1, N // int(2 * R + 1))                         # lattice points per axis
    h = N // m
    pts = [(1 + a * h, 1 + b * h, 1 + c * h) for a in range(m) for b in range(m) for c in range(m)]
    if np.sqrt(3.0) * (h // 2) >= 2 * R + 1:                # body centres fit as well
        pts += [(1 + a * h + h // 2, 1 + b * h + h // 2, 1 + c * h + h // 2) for a in range(m) for b in range(m) for c in range(m)]
    pos = np.array(pts).T
    rng = np.random.RandomState(seed)
    order = rng.permutation(pos.shape[1])
    order = np.concatenate(([0], order[order != 0]))        # the corner source first: it survives any truncation
    pos = pos[:, order]
    return pos, rng.uniform(1.0, 5.0, pos.shape[1])


def _scale_grid(N, pos, spec):
    """2^-spec of the nearest source (periodic), per cell."""
    ax = np.arange(N)
    best = np.full((N, N, N), np.inf)
    out = np.ones((N, N, N))
    for s in range(pos.shape[1]):
        d = [np.minimum(np.abs(ax - (pos[a, s] - 1)), N - np.abs(ax - (pos[a, s] - 1))) ** 2 for a in range(3)]
        d2 = d[0][:, None, None] + d[1][None, :, None] + d[2][None, None, :]
        near = d2 < best
        best[near] = d2[near]
        out[near] = 2.0 ** -int(spec[s])
    return out


def _trace(lib, capi, N, R, n, dr, dlog, numtau, opts, heat):
    o = dict(opts, OPT_HEATING=1) if heat else dict(opts)
    _set(lib, capi, o)
    try:
        lib.raytrace_device(R, cases.SIG, dr, 0, n, cases.MINLOGTAU, dlog, numtau)
        v = lib.last_raytrace_variant()
        phi = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
        h = lib.grid_to_host(capi.GRID_PHI_HEAT, np.empty((N, N, N))) if heat else None
    finally:
        _reset(lib, capi, o)
    return phi, h, v


def _pairs_with_two_spectra(lib, p0, f0, spec, aligned):
    """How many workgroups of a paired launch of the whole list hold two sources of different spectra: the launch works from the
    position-ordered list; consecutive entries share a workgroup, or -- line-aligned tables -- consecutive entries that agree
    modulo 8 along the axis of the unit's face (raytrace.hip, source_pairs_by_class)."""
    ps, _, ss = lib.sort_sources(p0, f0, spec)
    if not aligned:
        return int(np.sum(ss[0:len(ss) - 1:2] != ss[1::2]))
    mixed = 0
    for axis in (2, 0):
        open_ = {}
        for s in range(len(ss)):
            c = ps[3 * s + axis] & 7
            if c in open_:
                mixed += int(ss[open_.pop(c)] != ss[s])
            else:
                open_[c] = s
    return mixed


def _identity_runs(lib, capi, N, R, pos, flux, spec, dr, dlog, numtau, combos, seen, medium=""):
    p0, f0 = cases.flat_sources(pos, flux)
    n = flux.shape[0]
    scale = _scale_grid(N, pos, spec)
    for opts, heat in combos:
        tag = f"N={N} R={R} n={n} {medium} {opts} heat={heat}"
        lib.source_data_to_device(p0, f0, n)                      # every source back to spectrum 0
        ref, href, v0 = _trace(lib, capi, N, R, n, dr, dlog, numtau, opts, heat)
        lib.source_spectra_to_device(spec)
        phi, h, v = _trace(lib, capi, N, R, n, dr, dlog, numtau, opts, heat)
        same = ("paired", "buffer_atomics", "global_shells", "units", "threads")    # (zero-skipping and, left to the library, the
        assert [v[k] for k in same] == [v0[k] for k in same], tag                    #  line-aligned tables follow the launch history)
        assert ref.max() > 0 and (ref != 0).sum() >= n, tag
        assert np.array_equal(phi, scale * ref), tag
        assert not np.signbit(phi).any(), tag
        if heat:
            assert href.max() > 0 and np.array_equal(h, scale * href), tag
            assert np.array_equal(href, P2 * ref), tag
        family = ("paired" if v["paired"] else "single", "aligned" if v["aligned"] else "packed",
                  "buffer" if v["buffer_atomics"] else "global", "skip_zero" if v["skip_zero"] else "all", "heat" if heat else "")
        seen.add(family)
        if opts.get("OPT_PAIR_SOURCES") == 2 and not heat and n >= 2:
            assert v["paired"], tag
            assert _pairs_with_two_spectra(lib, p0, f0, spec, v["aligned"]) >= 1, tag
        if opts.get("OPT_ALIGNED_ROWS") == 2 and v["paired"]:
            assert v["aligned"], tag
        if opts.get("OPT_GLOBAL_ATOMICS") == 1:
            assert not v["buffer_atomics"], tag
        if opts.get("OPT_SKIP_ZERO_RATES") == 1 and not heat and v["buffer_atomics"]:
            assert v["skip_zero"], tag          # (the branching form of the global-atomic family does not report itself)
        if opts.get("OPT_SKIP_ZERO_RATES") == 2:
            assert not v["skip_zero"], tag


# option sets of tests/test_gpu_heating.py that reach the families, with and without heating tables in play
_COMBOS = [
    ({}, False),
    ({"OPT_PAIR_SOURCES": 2, "OPT_SKIP_ZERO_RATES": 2}, False),            # paired
    ({"OPT_PAIR_SOURCES": 2, "OPT_SKIP_ZERO_RATES": 1}, False),            # paired, exact zeros left out
    ({"OPT_PAIR_SOURCES": 2, "OPT_ALIGNED_ROWS": 2, "OPT_SECTORS": 9, "OPT_SKIP_ZERO_RATES": 2}, False),     # line-aligned pairs, six sectors
    ({"OPT_PAIR_SOURCES": 2, "OPT_ALIGNED_ROWS": 2, "OPT_SECTORS": 3, "OPT_SKIP_ZERO_RATES": 1}, False),   # ... twelve sector pairs
    ({"OPT_PAIR_SOURCES": 1, "OPT_SKIP_ZERO_RATES": 2}, False),            # single source, buffer atomics
    ({"OPT_PAIR_SOURCES": 1, "OPT_SKIP_ZERO_RATES": 1}, False),
    ({"OPT_GLOBAL_ATOMICS": 1}, False),                                    # single source, global atomics
    ({"OPT_GLOBAL_ATOMICS": 1, "OPT_SKIP_ZERO_RATES": 1}, False),          # ... the branching zero-skipping form
    ({"OPT_SECTORS": 1, "OPT_BLOCK_THREADS": 64}, False),
    ({"OPT_Z_TRANSPOSED": 0}, False),
    ({"OPT_FORTRAN_CONSTANTS": 1, "OPT_PAIR_SOURCES": 2}, False),
    ({}, True),                                                            # heating: single source, buffer atomics
    ({"OPT_GLOBAL_ATOMICS": 1}, True),
    ({"OPT_SECTORS": 3, "OPT_BLOCK_THREADS": 128}, True),
]


@pytest.fixture(scope="module")
def identity_setup(asora):
    p, lib, capi = asora
    thin, thick, dlog = cases.soft_tables(400)
    nd, xh, dr = cases.grid(N_ID, "lognormal", 11, 0.4, xlo=1e-4, xhi=1e-2)
    _fresh(p, N_ID)
    st, sk = _scaled_sets(thin, thick)
    lib.spectra_to_device(st, sk, P2 * st, P2 * sk)
    assert lib.num_spectra() == K
    lib.grid_to_device(capi.GRID_XH_AV, xh)
    lib.grid_to_device(capi.GRID_NDENS, nd)
    return dict(thin=thin, thick=thick, dlog=dlog, nd=nd, xh=xh, dr=dr, numtau=thin.shape[0], seen=set())


@pytest.mark.parametrize("R", [5, 9, 17, 30])
def test_power_of_two_identity_in_every_launch_form(asora, identity_setup, R):
    """N = 96, K = 3 spectra drawn at random per source, spheres apart: PHI_ION (and PHI_HEAT with heating) of a source of
    spectrum s == 2^-s x the all-spectrum-0 run of the same call, bit for bit, in the paired form (with a workgroup that holds two
    different spectra), the single-source forms with buffer and with global atomics, with the exact zeros left out and not, the
    line-aligned paired form, and for an odd source count.  R = 5 also runs a thick medium, where most cells lie beyond the last
    table entry and the zero-skipping forms actually skip.
    The per-layout descriptor forms (SPLIT) are reached only at N > 512, which no option forces below; they go through the same
    per-source table base as the forms covered here -- one line of the kernel, read where the position and the flux are read --
    and the paired one of them keeps, for launches without spectra, the code of before."""
    p, lib, capi = asora
    c = identity_setup
    pos, flux = _apart_sources(N_ID, R, 30 + R)
    n = pos.shape[1]
    if n > 2 and n % 2 == 0:
        pos, flux, n = pos[:, :n - 1], flux[:n - 1], n - 1        # an odd count: the last pair is half empty
    if n > 81:
        pos, flux, n = pos[:, :81], flux[:81], 81
    rng = np.random.RandomState(R)
    spec = rng.randint(0, K, n).astype(np.int32)
    spec[:min(n, 3)] = [1, 2, 0][:min(n, 3)]                       # every spectrum present, the first two sources differ
    assert n >= 2
    _identity_runs(lib, capi, N_ID, float(R), pos, flux, spec, c["dr"], c["dlog"], c["numtau"], _COMBOS, c["seen"])
    if R == 5:
        lib.grid_to_device(capi.GRID_NDENS, c["nd"] * 3.0e4)
        try:
            thick_combos = [cb for cb in _COMBOS if "OPT_SKIP_ZERO_RATES" in cb[0] or cb[1]]
            _identity_runs(lib, capi, N_ID, float(R), pos, flux, spec, c["dr"], c["dlog"], c["numtau"], thick_combos, c["seen"], "thick")
        finally:
            lib.grid_to_device(capi.GRID_NDENS, c["nd"])
    if R == 30:     # (the last radius: what the four radii reached together)
        seen = c["seen"]
        for want in (("paired", "packed", "buffer", "all", ""), ("paired", "packed", "buffer", "skip_zero", ""),
                     ("paired", "aligned", "buffer", "all", ""), ("paired", "aligned", "buffer", "skip_zero", ""),
                     ("single", "packed", "buffer", "all", ""), ("single", "packed", "buffer", "skip_zero", ""),
                     ("single", "packed", "global", "all", ""),
                     ("single", "packed", "buffer", "all", "heat"), ("single", "packed", "global", "all", "heat")):
            assert want in seen, (want, sorted(seen))


def test_identity_with_shells_in_global_scratch(asora):
    """N = 168, R beyond the box: the shells outgrow LDS and live in global memory (the set-up of
    test_large_shells_global_scratch_and_large_lds); two sources cannot be apart there, so each spectrum is traced alone and
    compared with the spectrum-0 trace of the same source."""
    p, lib, capi = asora
    N = 168
    thin, thick, dlog = cases.soft_tables(400)
    nd, xh, dr = cases.grid(N, "lognormal", 41, 0.02)
    pos, flux = cases.sources(N, 1, 42, flux=5.0)
    p0, f0 = cases.flat_sources(pos, flux)
    _fresh(p, N)
    st, sk = _scaled_sets(thin, thick)
    lib.spectra_to_device(st, sk, P2 * st, P2 * sk)
    lib.grid_to_device(capi.GRID_NDENS, nd)
    lib.grid_to_device(capi.GRID_XH_AV, xh)
    for heat in (False, True):
        lib.source_data_to_device(p0, f0, 1)
        ref, href, v = _trace(lib, capi, N, 1000.0, 1, dr, dlog, thin.shape[0], {"OPT_SECTORS": 1}, heat)
        assert v["global_shells"] and ref.max() > 0
        for s in (1, 2):
            lib.source_spectra_to_device(np.array([s], dtype=np.int32))
            phi, h, v = _trace(lib, capi, N, 1000.0, 1, dr, dlog, thin.shape[0], {"OPT_SECTORS": 1}, heat)
            assert v["global_shells"]
            assert np.array_equal(phi, 2.0 ** -s * ref)
            if heat:
                assert np.array_equal(h, 2.0 ** -s * href)


def test_two_black_bodies_against_the_oracle(asora):
    """Two black-body table sets (5e4 K and 2e5 K, not proportional to one another), 40 sources with overlapping spheres at
    N = 48, random spectra: rates are linear in the sources at fixed nHI, so the GPU's PHI_ION and PHI_HEAT equal the sum over
    the spectra of the oracle's trace of that spectrum's sources with its tables."""
    p, lib, capi = asora
    N, ns, R = 48, 40, 9.0
    sets = [cases.blackbody_photo_and_heat_tables(teff=t, num_tau=400) for t in (5e4, 2e5)]
    dlog = sets[0][4]
    numtau = sets[0][0].shape[0]
    nd, xh, dr = cases.grid(N, "lognormal", 12, 0.3, xlo=1e-4, xhi=1e-2)
    pos, flux = cases.sources(N, ns, 13, flux=2.0)
    flux = flux * np.random.RandomState(14).uniform(0.5, 2.0, ns)
    spec = np.random.RandomState(15).randint(0, 2, ns).astype(np.int32)
    assert 5 < spec.sum() < ns - 5
    p0, f0 = cases.flat_sources(pos, flux)
    ref_phi, ref_heat = np.zeros((N, N, N)), np.zeros((N, N, N))
    for s, (thin, thick, hthin, hthick, _) in enumerate(sets):
        sel = np.flatnonzero(spec == s)
        q0, g0 = cases.flat_sources(pos[:, sel], flux[sel])
        r = O.asora_do_all_sources(R, cases.SIG, dr, nd, xh, q0, g0, thin, thick, cases.MINLOGTAU, dlog, NumTau=numtau,
                                   heat_thin=hthin, heat_thick=hthick)
        ref_phi += r["phi_ion"]
        ref_heat += r["phi_heat"]
    _fresh(p, N)
    lib.spectra_to_device(np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets]),
                          np.stack([s[2] for s in sets]), np.stack([s[3] for s in sets]))
    lib.grid_to_device(capi.GRID_NDENS, nd)
    lib.grid_to_device(capi.GRID_XH_AV, xh)
    lib.source_data_to_device(p0, f0, ns)
    lib.source_spectra_to_device(spec)
    w = ref_phi != 0
    assert w.sum() > 20000
    for opts, heat in (({}, True), ({"OPT_GLOBAL_ATOMICS": 1}, True), ({"OPT_PAIR_SOURCES": 2}, False),
                       ({"OPT_PAIR_SOURCES": 2, "OPT_ALIGNED_ROWS": 2, "OPT_SECTORS": 9}, False), ({"OPT_PAIR_SOURCES": 1}, False)):
        phi, h, v = _trace(lib, capi, N, R, ns, dr, dlog, numtau, opts, heat)
        print(f"{opts} heat={heat}: max rel err phi {np.max(np.abs(phi[w] - ref_phi[w]) / ref_phi[w]):.2e}"
              + (f", heat {np.max(np.abs(h[w] - ref_heat[w]) / ref_heat[w]):.2e}" if heat else ""))
        assert np.array_equal(phi != 0, w), opts
        np.testing.assert_allclose(phi[w], ref_phi[w], rtol=GAMMA_RTOL, atol=0, err_msg=str(opts))
        if heat:
            np.testing.assert_allclose(h[w], ref_heat[w], rtol=GAMMA_RTOL, atol=0, err_msg=str(opts))
        if opts.get("OPT_PAIR_SOURCES") == 2:
            assert v["paired"]


def test_one_spectrum_is_the_plain_table_path(asora):
    """spectra_to_device with K = 1, K = 3 with every source on spectrum 0, and photo_table_to_device (+ heat_table_to_device):
    the same bits, with and without heating, paired and not."""
    p, lib, capi = asora
    N, R = 96, 9.0
    thin, thick, dlog = cases.soft_tables(400)
    numtau = thin.shape[0]
    nd, xh, dr = cases.grid(N, "lognormal", 11, 0.4, xlo=1e-4, xhi=1e-2)
    pos, flux = _apart_sources(N, R, 5)
    pos, flux = pos[:, :63], flux[:63]
    p0, f0 = cases.flat_sources(pos, flux)
    n = flux.shape[0]
    st, sk = _scaled_sets(thin, thick)
    _fresh(p, N)
    lib.grid_to_device(capi.GRID_NDENS, nd)
    lib.grid_to_device(capi.GRID_XH_AV, xh)
    lib.source_data_to_device(p0, f0, n)
    runs = {}
    for name in ("plain", "K=1", "K=3 all 0", "K=3 zeros uploaded"):
        if name == "plain":
            p.photo_table_to_device(thin, thick)
            lib.heat_table_to_device(P2 * thin, P2 * thick, numtau)
            assert lib.num_spectra() == 1
        elif name == "K=1":
            lib.spectra_to_device(st[:1], sk[:1], P2 * st[:1], P2 * sk[:1])
            assert lib.num_spectra() == 1
        elif name == "K=3 all 0":
            lib.spectra_to_device(st, sk, P2 * st, P2 * sk)
            assert lib.num_spectra() == 3
        else:
            lib.source_spectra_to_device(np.zeros(n, dtype=np.int32))
        runs[name] = [_trace(lib, capi, N, R, n, dr, dlog, numtau, o, h)[:2]
                      for o, h in (({}, False), ({"OPT_PAIR_SOURCES": 2}, False), ({"OPT_GLOBAL_ATOMICS": 1}, False), ({}, True))]
    for name in ("K=1", "K=3 all 0", "K=3 zeros uploaded"):
        for (phi, h), (phi0, h0) in zip(runs[name], runs["plain"]):
            assert phi0.max() > 0 and np.array_equal(phi, phi0), name
            assert (h is None) == (h0 is None) and (h is None or np.array_equal(h, h0)), name


def _host_loop(lib, capi, N, chem, R, dr, dlog, numtau, nsrc, conv_frac, xh, thermal_prm):
    """The loop of evolve.py:168-240 over the isolated calls (the construction of tests/test_gpu_thermal.py)."""
    lib.grid_to_device(capi.GRID_XH, xh)
    lib.grid_copy(capi.GRID_XH_AV, capi.GRID_XH)
    crit = min(int(conv_frac * N ** 3), (nsrc - 1) / 3)
    prev1 = prev0 = 2.0 * N ** 3
    niter, converged = 0, False
    if thermal_prm is not None:
        lib.set_option(capi.OPT_HEATING, 1)
        lib.thermal_params(True, *thermal_prm)
    try:
        while not converged and niter < 100:
            niter += 1
            lib.raytrace_device(R, cases.SIG, dr, 0, nsrc, cases.MINLOGTAU, dlog, numtau)
            conv, s1, s0 = lib.chemistry_device(*chem)
            rel1 = abs((s1 - prev1) / s1) if s1 > 0 else 1.0
            rel0 = abs((s0 - prev0) / s0) if s0 > 0 else 1.0
            converged = conv < crit or (rel1 < conv_frac and rel0 < conv_frac)
            prev1, prev0 = s1, s0
    finally:
        lib.set_option(capi.OPT_HEATING, 0)
        lib.thermal_params(False)
    g = lambda w: lib.grid_to_host(w, np.empty((N, N, N)))
    return niter, g(capi.GRID_XH_INTERMED), g(capi.GRID_PHI_ION), (g(capi.GRID_TEMP_END) if thermal_prm is not None else None)


@pytest.mark.parametrize("N,thermal", [(24, False), (33, False), (24, True)])
def test_evolve3D_with_two_spectra_equals_the_host_loop(asora, tmp_path, N, thermal):
    """evolve3D(src_spectrum=...) -- the device loop -- against a host-driven loop over raytrace_device + chemistry_device with
    the same sources and spectra: the same iteration count, xh and phi_ion (and temp with thermal=) to 1e-10.  And the spectra
    matter: the step differs from the one with every source on spectrum 0."""
    from pyc2ray_amd.thermal import ThermalParams
    p, lib, capi = asora
    rng = np.random.default_rng(5 + N)
    ns = 5
    pos = rng.integers(1, N + 1, size=(3, ns))
    flux = 10 ** rng.uniform(-1.5, -0.5, ns)
    spec = np.array([0, 1, 1, 0, 1], dtype=np.int64)
    nd = 1e-3 * 10 ** rng.uniform(-0.3, 0.3, (N, N, N))
    xh = np.full((N, N, N), 1.2e-3)
    T = np.full((N, N, N), 100.0 if thermal else 1e4)
    thin, thick, dlog = cases.soft_tables()
    numtau = thin.shape[0]
    hard_thin, hard_thick = hard_tables(numtau - 1)
    pt, pk = np.stack([thin, hard_thin]), np.stack([thick, hard_thick])
    ht, hk = np.stack([3e-11 * thin, 9e-11 * hard_thin]), np.stack([2.5e-11 * thick, 8e-11 * hard_thick])
    dt, dr, R, conv_frac = 3.15576e13, 3.086e21 * 0.4, 12.0, 1e-4
    _fresh(p, N)
    lib.spectra_to_device(pt, pk, ht, hk)
    tp = ThermalParams(ht, hk) if thermal else None
    args = (dt, dr, flux, pos, True, 1000, N, 1e-2, T, nd, xh, thin, thick, cases.MINLOGTAU, dlog, R, conv_frac, cases.SIG, *CHEM)
    out = p.evolve3D(*args, logfile=str(tmp_path / "log"), quiet=True, thermal=tp, src_spectrum=spec)
    niter = p.evolve._evolve.last_niter
    out0 = p.evolve3D(*args, logfile=str(tmp_path / "log0"), quiet=True, thermal=tp)
    assert not np.allclose(out[1], out0[1], rtol=1e-3, atol=0)
    # the host-driven loop: sources and spectra as evolve3D left them on the device
    lib.grid_to_device(capi.GRID_NDENS, nd)
    lib.grid_to_device(capi.GRID_TEMP, T)
    p0, f0 = cases.flat_sources(pos, flux)
    lib.source_data_to_device(p0, f0, ns)
    lib.source_spectra_to_device(spec)
    prm = (tp.relative_denergy, tp.t_floor, tp.max_substeps, int(tp.cooling), False, 0.0) if thermal else None
    h_niter, h_x, h_phi, h_T = _host_loop(lib, capi, N, (dt,) + CHEM, R, dr, dlog, numtau, ns, conv_frac, xh, prm)
    assert niter == h_niter and niter > 1
    np.testing.assert_allclose(out[0], h_x, rtol=1e-10, atol=0)
    np.testing.assert_allclose(out[1], h_phi, rtol=1e-10, atol=0)
    if thermal:
        np.testing.assert_allclose(out[2], h_T, rtol=1e-10, atol=0)
        assert out[2].max() > 5e3


def test_refusals_leave_the_library_usable(asora, tmp_path):
    """What is not extended fails with its documented error while a source has a spectrum other than 0 -- the sub-box raytracer,
    use_gpu=False, grey opacity -- and an index >= K is caught on the host; the library works afterwards."""
    p, lib, capi = asora
    N, R = 24, 6.0
    thin, thick, dlog = cases.soft_tables(400)
    numtau = thin.shape[0]
    nd, xh, dr = cases.grid(N, "lognormal", 3, 0.3)
    pos, flux = cases.sources(N, 4, 8, flux=2.0)
    p0, f0 = cases.flat_sources(pos, flux)
    st, sk = _scaled_sets(thin, thick)
    _fresh(p, N)
    lib.spectra_to_device(st, sk)
    lib.grid_to_device(capi.GRID_NDENS, nd)
    lib.grid_to_device(capi.GRID_XH_AV, xh)
    lib.source_data_to_device(p0, f0, 4)
    spec = np.array([0, 2, 1, 0], dtype=np.int32)

    def works():
        phi = _trace(lib, capi, N, R, 4, dr, dlog, numtau, {}, False)[0]
        assert phi.max() > 0
        return phi

    with pytest.raises(RuntimeError, match="outside"):                           # an index >= K at upload
        lib.source_spectra_to_device(np.array([0, 3, 1, 0], dtype=np.int32))
    with pytest.raises(RuntimeError, match="4 sources"):
        lib.source_spectra_to_device(np.array([0, 1], dtype=np.int32))
    base = works()                                                               # (a failed upload leaves every source on 0)
    lib.source_spectra_to_device(spec)
    mixed = works()
    assert not np.array_equal(mixed, base)
    with pytest.raises(RuntimeError, match="one spectrum"):                      # sub-box call
        lib.subbox_raytrace_device(1000, N, 1e-2, R, cases.SIG, dr, cases.MINLOGTAU, dlog, numtau, 0, 4)
    lib.set_option(capi.OPT_GREY_NOTABLES, 1)                                    # grey opacity
    try:
        with pytest.raises(RuntimeError, match="grey"):
            lib.raytrace_device(R, cases.SIG, dr, 0, 4, cases.MINLOGTAU, dlog, numtau)
    finally:
        lib.set_option(capi.OPT_GREY_NOTABLES, 0)
    assert np.array_equal(works(), mixed)
    p.photo_table_to_device(thin, thick)                                         # fewer table sets afterwards: the first launch fails
    with pytest.raises(RuntimeError, match="table set 2"):
        lib.raytrace_device(R, cases.SIG, dr, 0, 4, cases.MINLOGTAU, dlog, numtau)
    lib.spectra_to_device(st, sk)
    assert np.array_equal(works(), mixed)
    T = np.full((N, N, N), 1e4)
    args = (3e13, dr, flux, pos, False, 1000, N, 1e-2, T, nd, xh, thin, thick, cases.MINLOGTAU, dlog, R, 1e-4, cases.SIG, *CHEM)
    with pytest.raises(ValueError, match="use_gpu=True"):                        # use_gpu=False
        p.evolve3D(*args, logfile=str(tmp_path / "log"), quiet=True, src_spectrum=spec)
    with pytest.raises(ValueError, match="index 3"):
        p.evolve3D(*(args[:4] + (True,) + args[5:]), logfile=str(tmp_path / "log"), quiet=True, src_spectrum=np.array([0, 3, 0, 0]))
    lib.source_data_to_device(p0, f0, 4)
    assert np.array_equal(works(), base)


def test_class_with_a_teff_list_resident_and_through_the_host(asora, tmp_path):
    """C2Ray_Test with `BlackBodySource: Teff: [5e4, 2e5]` and a spectrum per source, two steps: the device-resident run against
    `device_resident = False`, at the tolerance of test_device_resident_grids_give_the_same_run_with_fewer_transfers (1e-11:
    atomic summation order only); and the second temperature matters."""
    import os
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    here = os.path.dirname(os.path.abspath(__file__))
    base = open(os.path.join(here, "data", "parameters_single_black_body.yml")).read()
    assert "Teff: 5e4" in base and "NumTau: 10000" in base
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 24
        with open("parameters.yml", "w") as f:
            f.write(base.replace("Teff: 5e4", "Teff: [5.0e+4, 2.0e+5]").replace("NumTau: 10000", "NumTau: 500"))
        with open("src.txt", "w") as f:
            f.write("3\n12 12 12 6e50 1.0\n5 20 9 2e50 1.0\n18 4 15 3e50 1.0\n")
        spec = np.array([0, 1, 1])
        runs = {}
        for resident, spectrum in ((True, spec), (False, spec), (True, None)):
            if p.cuda_is_init():
                p.device_close()
            sim = pc2r.C2Ray_Test("parameters.yml", N, True)
            sim.device_resident = resident
            assert lib.num_spectra() == 2 and sim.spectra_photo_thin_table.shape == (2, 501)
            sim.density_init(0.0)
            srcpos, srcflux = sim.read_sources("src.txt", 3)
            out = []
            for _ in range(2):
                sim.evolve3D(3.15576e13, srcflux, srcpos, spectrum)
                out.append((np.array(sim.xh), np.array(sim.phi_ion)))
            runs[(resident, spectrum is not None)] = out
        for (x1, g1), (x0, g0) in zip(runs[(True, True)], runs[(False, True)]):
            assert g0.max() > 0
            np.testing.assert_allclose(x1, x0, rtol=1e-11, atol=0)
            np.testing.assert_allclose(g1, g0, rtol=1e-11, atol=0)
        assert not np.allclose(runs[(True, True)][1][1], runs[(True, False)][1][1], rtol=1e-3, atol=0)
    finally:
        if p.cuda_is_init():
            p.device_close()
        os.chdir(cwd)
