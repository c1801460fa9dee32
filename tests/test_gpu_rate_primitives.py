"""GPU: the device functions every rate goes through (pyc2ray_amd/csrc/rates_device.hpp), evaluated on arrays by
asora_debug_rate_primitives and held against the high-precision references, input sets and bounds of
tests/rate_primitives_reference.py (whose preconditions tests/test_rate_primitives_reference.py shows on the CPU): log2_pos to its
stated error bound, the table lookup against the exact interpolant with its clamps and offsets, div_newton bit for bit against the
IEEE quotient, the products and sums that must not be fused, the rates as the composition of those, and one production kernel
(the plane-parallel sweep) bit for bit against the composition of the debug kernel's lookups.  Mesh: 8^3, nothing here depends on it."""
import numpy as np
import pytest

import cases
import plane_flux_reference as PF
import rate_primitives_reference as RP

pytestmark = pytest.mark.gpu

SIG = cases.SIG


@pytest.fixture(scope="module")
def dev():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib, _capi
    lib.plane_flux((), ())
    lib.set_option(_capi.OPT_FORTRAN_CONSTANTS, 0)
    if p.cuda_is_init():
        p.device_close()


def _fresh(p, N=8):
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)


_TABLES_ON_DEVICE = {}


def _with_tables(p, lib, table_len):
    """An 8^3 device holding the two table sets of RP.lookup_tables(table_len); uploaded again only when the length changes."""
    t = RP.lookup_tables(table_len)
    if not p.cuda_is_init() or _TABLES_ON_DEVICE.get("len") != table_len:
        _fresh(p)
        lib.spectra_to_device(t[:, 1], t[:, 0], t[:, 3], t[:, 2])         # (thin, thick, heat thin, heat thick)
        _TABLES_ON_DEVICE["len"] = table_len
    return t


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


# ---- the entry itself ---------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    """Code 2 before device_init, 4 without the tables an operation needs, 3 on null arrays and on an unknown operation."""
    p, lib, capi = dev
    if p.cuda_is_init():
        p.device_close()
    _TABLES_ON_DEVICE.clear()
    x = np.array([1.0, 2.0])
    with pytest.raises(RuntimeError, match=r"code 2.*not initialised"):
        lib.debug_rate_primitives("log2", x)
    _fresh(p)
    assert np.all(np.abs(lib.debug_rate_primitives("log2", x) - [0.0, 1.0]) < 1e-14)       # no tables needed
    assert lib.debug_rate_primitives("log2", np.zeros(0)).size == 0
    for op in ("lookup", "photo", "heat"):
        with pytest.raises(RuntimeError, match=r"code 4.*tables not on device"):
            lib.debug_rate_primitives(op, x, x, x, x, NumTau=5)
    lib.photo_table_to_device(np.ones(5), np.ones(5), 5)
    assert np.array_equal(lib.debug_rate_primitives("lookup", x, NumTau=5)[0], [1.0, 1.0])
    for kw in (dict(op="heat"), dict(op="lookup", which="heat_thin")):
        with pytest.raises(RuntimeError, match=r"code 4.*heating tables not on device"):
            lib.debug_rate_primitives(kw["op"], x, x, x, x, which=kw.get("which", 0), NumTau=5)
    with pytest.raises(RuntimeError, match=r"code 4.*table set 1"):
        lib.debug_rate_primitives("lookup", x, spectrum=1, NumTau=5)
    with pytest.raises(RuntimeError, match=r"code 3.*null input"):
        lib.debug_rate_primitives("div", x)
    with pytest.raises(RuntimeError, match=r"code 3.*null input"):
        lib.debug_rate_primitives("absorber", x, x, x)
    out = np.zeros(2)
    assert lib._lib.asora_debug_rate_primitives(capi.PRIM_LOG2, 2, capi.dptr(x), None, None, None, 0, 0, 1.0, -20.0, 1.0, 1, None, None) == 3
    assert lib._lib.asora_debug_rate_primitives(capi.PRIM_LOOKUP, 2, capi.dptr(x), None, None, None, 0, 0, 1.0, -20.0, 1.0, 5, capi.dptr(out), None) == 3
    for op in (-1, capi.PRIM_COUNT, 99):
        with pytest.raises(RuntimeError, match=r"code 3.*unknown operation"):
            lib.debug_rate_primitives(op, x, x, x, x)
    with pytest.raises(RuntimeError, match=r"code 3.*NumTau"):
        lib.debug_rate_primitives("lookup", x, NumTau=0)


# ---- log2 ---------------------------------------------------------------------------------------------------------------------
def test_log2_within_its_stated_bound(dev):
    """|log2_pos(x) - log2 x| <= E(x) = 8.2e-15 + 2^-51 + ulp(log2 x)/2 on 20 000 + 20 000 log-uniform points, both neighbours of
    every edge of the 256 mantissa intervals at six exponents, every power of two and the two clamps."""
    p, lib, capi = dev
    if not p.cuda_is_init():
        _fresh(p)
    ref = RP.log2_reference()
    got = lib.debug_rate_primitives("log2", ref["x"])
    share = RP.error_against(got, ref["hi"], ref["lo"]) / ref["bound"]
    w = int(np.argmax(share))
    tau_range = slice(20000, 40000)
    print(f"log2_pos: {share.max():.3f} of E at x = {ref['x'][w]!r} (|error| {share[w] * ref['bound'][w]:.3e}); "
          f"{share[tau_range].max():.3f} of E on [1e-8, 1e3]; points: {got.size}")
    sub = slice(40000, None)                # the interval edges, the powers of two, the clamps
    for contract in (False, True):
        emu = RP.log2_pos_emulated(ref["x"][sub], contract_last=contract)
        print(f"  differs from the float64 restatement (last product {'fused' if contract else 'rounded'}) at "
              f"{int((emu != got[sub]).sum())} of {emu.size} points")
    assert np.all(np.isfinite(got))
    assert share.max() <= 1.0
    p2 = RP.powers_of_two()
    got2 = lib.debug_rate_primitives("log2", p2)
    print(f"  powers of two returned as the exponent itself: {int((got2 == np.log2(p2)).sum())} of {p2.size}")
    if RP.log2_exact_at_powers_of_two():
        assert np.array_equal(got2, np.log2(p2))


# ---- table lookup -------------------------------------------------------------------------------------------------------------
LOOKUP_SETS = ["production", "short19", "short20", "short21"]
_LOOKUP_REFERENCE = {}


def _lookup_reference(name):
    """Parameters, optical depths (the log2 set and the table's knots with their neighbours) and the exact index of a parameter
    set, computed once."""
    if name not in _LOOKUP_REFERENCE:
        ps = RP.lookup_parameter_sets()[name]
        ref = RP.log2_reference()
        knots = RP.knots(ps["minlogtau"], ps["dlogtau"], ps["table_len"])
        tau = np.concatenate([ref["x"], knots])
        log2_hp = ref["hp"] + RP.log2_exact_hp(knots)
        index = RP.exact_index(tau, ps["minlogtau"], ps["dlogtau"], ps["NumTau"], ps["table_len"], log2_hp=log2_hp)
        r = dict(ps=ps, tau=tau, log2_hi=np.array([float(v) for v in log2_hp]), index=index,
                 kw=dict(sig=1.0, minlogtau=ps["minlogtau"], dlogtau=ps["dlogtau"], NumTau=ps["NumTau"]))
        for v in (tau, r["log2_hi"]) + index:
            v.setflags(write=False)
        _LOOKUP_REFERENCE[name] = r
    return _LOOKUP_REFERENCE[name]


@pytest.mark.parametrize("name", LOOKUP_SETS)
def test_lookup_against_the_exact_interpolant(dev, name):
    """Every table (thick, thin, heat thick, heat thin) of both sets within
    S (k1 E(tau) + ulp(real_i)) + 2 eps max(|T_i|, |T_i+1|) of the exact interpolant.

    This test found the index fma(log2 tau, k1, k0) of the production parameters 1.4e-13 off at tau = 1e-18 (1.28 of the bound; 83
    of 413 384 values over it, all below tau = 9.5e-19): the doubles k0 = 1667.67 and k1 are themselves off by 1.1e-13 and
    5.4e-16 (RP.index_constant_errors), and k0 cancels against k1 log2 tau where the index, and with it ulp(real_i), is small.
    lookup_issue now adds the term kc of lut_index_constants (csrc/asora_internal.hpp), which holds what the two roundings leave
    out; the figures printed here are with it."""
    p, lib, capi = dev
    r = _lookup_reference(name)
    ps, tau, kw = r["ps"], r["tau"], r["kw"]
    tables = _with_tables(p, lib, ps["table_len"])
    constants = RP.index_constant_errors(ps["minlogtau"], ps["dlogtau"])
    exact = r["index"][0] + r["index"][1]
    worst, over, index_off = 0.0, 0, 0.0
    for s in range(2):
        for k, which in enumerate(RP.TABLES):
            T = tables[s, k]
            got, real_i = lib.debug_rate_primitives("lookup", tau, which=which, spectrum=s, **kw)
            F = RP.interp_exact(T, tau, ps["minlogtau"], ps["dlogtau"], ps["NumTau"], index=r["index"])
            share = RP.error_against(got, F["hi"], F["lo"]) / RP.lookup_bound(F, tau, ps["dlogtau"], r["log2_hi"])
            w = int(np.argmax(share))
            print(f"{name} set {s} {which}: {share.max():.3f} of the bound at tau = {tau[w]!r} (exact index {F['index'][w]!r}, "
                  f"device index {real_i[w]!r}); {int((share > 1).sum())} points over it")
            worst, over = max(worst, share.max()), over + int((share > 1).sum())
            index_off = max(index_off, np.max(np.abs(real_i - exact)[tau < 1e-15]))
    print(f"{name}: worst share of the lookup bound {worst:.3f} over {tau.size} optical depths x 8 tables, {over} values over it; "
          f"the index below tau = 1e-15 is off by {index_off:.2e} at most (the doubles k0, k1 alone: dk0 = {constants[0]:.3e}, "
          f"dk1 = {constants[1]:.3e})")
    assert worst <= 1.0


@pytest.mark.parametrize("name", LOOKUP_SETS)
def test_lookup_offsets_clamps_and_table_end(dev, name):
    """Every table of both sets: the value lies in the selected table's own range (the eight ranges are disjoint: a wrong offset,
    2 x stride or set stride shows at once); tau = 0, -0, -1, 5e-324, 1e-30 and NaN give the bits of tau = 1e-20; +inf and every
    finite tau >= 10^(minlogtau + dlogtau numtau_f) give exactly the last entry in use; the index as formed stays in
    [0, numtau_f] and its integer part on the table."""
    p, lib, capi = dev
    r = _lookup_reference(name)
    ps, tau, kw = r["ps"], r["tau"], r["kw"]
    n = ps["table_len"]
    tables = _with_tables(p, lib, n)
    limit = RP.index_limit(ps["NumTau"], n)
    end = RP.end_threshold(**ps)
    assert end >= RP.table_end(**ps)
    beyond = np.concatenate([tau[tau >= end], [end, np.nextafter(end, np.inf), 1e300, np.finfo(np.float64).max, np.inf]])
    clamped, floor = RP.clamp_inputs()
    for s in range(2):
        for k, which in enumerate(RP.TABLES):
            T = tables[s, k]
            got, real_i = lib.debug_rate_primitives("lookup", tau, which=which, spectrum=s, **kw)
            assert T.min() <= got.min() and got.max() <= T.max(), (s, which)
            assert real_i.min() >= 0.0 and real_i.max() <= limit and np.floor(real_i).max() <= n - 1
            exact = r["index"][0] + r["index"][1]
            assert np.max(np.abs(real_i - exact)) < 1e-11, (s, which)          # (the index is the index: 4 ulp of 2048)
            low, _ = lib.debug_rate_primitives("lookup", np.concatenate([[floor], clamped]), which=which, spectrum=s, **kw)
            assert np.all(_same_bits(low[1:], low[0])) and np.isfinite(low[0]), (s, which, low)
            high, high_i = lib.debug_rate_primitives("lookup", beyond, which=which, spectrum=s, **kw)
            assert np.all(high == T[int(limit)]) and np.all(high_i == limit), (s, which)
    print(f"{name}: {tau.size} optical depths x 8 tables in range; {beyond.size} beyond the end return the entry {int(limit)}")


# ---- division -----------------------------------------------------------------------------------------------------------------
def test_division_is_correctly_rounded(dev):
    """div_newton(x, y) == the IEEE quotient, bit for bit, on 2e6 random pairs over 2^+-340, 1e5 divisors with mantissas within
    8 ulp of 1.0 and 2.0 and the callers' operand families; y = 0 gives NaN."""
    p, lib, capi = dev
    if not p.cuda_is_init():
        _fresh(p)
    for name, (x, y) in RP.division_inputs().items():
        got = lib.debug_rate_primitives("div", x, y)
        wrong = int((got != x / y).sum())
        print(f"div_newton, {name}: {wrong} of {x.size} quotients differ from IEEE")
        assert wrong == 0, name
    x = np.array([1.0, -1.0, 0.0, 1e300, 5e-324])
    for zero in (0.0, -0.0):
        assert np.all(np.isnan(lib.debug_rate_primitives("div", x, np.full(x.size, zero))))


# ---- products and sums that must not be fused ------------------------------------------------------------------------------------
def test_unfused_operations(dev):
    """On operands for which fusing changes the bits (shown on the CPU): the device returns the separately rounded ones."""
    p, lib, capi = dev
    ps = RP.lookup_parameter_sets()["production"]
    tables = _with_tables(p, lib, ps["table_len"])
    u = RP.unfused_operands()
    # cd + n dr of the marches: mul_unfused, then add_unfused
    cd, n, dr = u["march"]
    prod = lib.debug_rate_primitives("mul", n, dr)
    got = lib.debug_rate_primitives("add", cd, prod)
    assert np.array_equal(prod, n * dr) and np.array_equal(got, cd + n * dr) and np.all(got != RP.fused(n, dr, cd))
    # the absorber density with both Lyman-limit terms
    nd, x, a, b = u["absorber"]
    got = lib.debug_rate_primitives("absorber", nd, x, a, b)
    inner = (1.0 - x) + b
    assert np.array_equal(got, nd * inner + a) and np.all(got != RP.fused(nd, inner, a))
    # ... and without them: n (1 - x) bit for bit, x = 1, n = 0 and NaN included
    nd, x = RP.absorber_without_lls()
    got = lib.debug_rate_primitives("absorber", nd, x, np.zeros(nd.size), np.zeros(nd.size))
    assert np.all(_same_bits(got, nd * (1.0 - x)))
    # tau_out - tau_in inside rate_issue: thin cells, whose rate is (pref dtau) T_thin(tau_out) with dtau the difference of the two
    # ROUNDED optical depths
    cd_in, cd_out, sig = u["tau"]
    kw = dict(sig=sig[0], minlogtau=ps["minlogtau"], dlogtau=ps["dlogtau"], NumTau=ps["NumTau"])
    flux, vol = np.full(cd_in.size, 3.0), np.full(cd_in.size, 7.0)
    got = lib.debug_rate_primitives("photo", flux, cd_in, cd_out, vol, **kw)
    t_in, t_out = cd_in * sig, cd_out * sig
    assert np.array_equal(lib.debug_rate_primitives("mul", cd_out, sig), t_out)
    thin_value, _ = lib.debug_rate_primitives("lookup", t_out, which="thin", **kw)
    assert np.all(np.abs(t_out - t_in) <= 1e-7)
    separate = (flux / vol) * (t_out - t_in) * thin_value
    contracted = (flux / vol) * RP.fused(cd_out, sig, -t_in) * thin_value
    print(f"thin cells: {int((separate != contracted).sum())} of {cd_in.size} rates tell the fused dtau from the separately rounded one")
    assert (separate != contracted).sum() >= 0.9 * cd_in.size
    assert np.array_equal(got, separate)


# ---- rates ----------------------------------------------------------------------------------------------------------------------
def _compose(lib, kw, fortran_consts, flux, cd_in, cd_out, vol_nhi, heat):
    """rate_issue / rate_value (heat: heat_rate_per_atom) on the host from the device's own LOOKUP outputs: every step one IEEE
    operation.  Returns (rate, thick mask)."""
    sig = kw["sig"]
    tau_in, tau_out = cd_in * sig, cd_out * sig
    dtau = tau_out - tau_in
    thick = np.abs(dtau) > RP.tau_photo_limit(fortran_consts)
    look = lambda which, tau: lib.debug_rate_primitives("lookup", tau, which=which, **kw)[0]
    names = ("heat_thick", "heat_thin") if heat else ("thick", "thin")
    with np.errstate(all="ignore"):
        pref = flux / vol_nhi
        a, b = look(names[0], tau_in), look(names[0], tau_out)
        t = look(names[1], tau_in if fortran_consts else tau_out)
        return np.where(thick, pref * (a - b), pref * dtau * t), thick


@pytest.mark.parametrize("fortran_consts", [0, 1])
def test_photo_and_heat_rates_are_the_composition_of_the_primitives(dev, fortran_consts):
    """PHOTO and HEAT equal, bit for bit, flux / vol_nhi times (a - b) -- thin: (pref dtau) a -- with a, b the device's own lookups:
    random thick and thin cells, the cells at TAU_PHOTO_LIMIT (double 1e-7, or the single 1e-7 promoted under Fortran constants),
    thin cells whose tau_in and tau_out lie in different table intervals, a == b beyond the table's end, vol_nhi = 0."""
    p, lib, capi = dev
    ps = RP.lookup_parameter_sets()["production"]
    _with_tables(p, lib, ps["table_len"])
    lib.set_option(capi.OPT_FORTRAN_CONSTANTS, fortran_consts)
    try:
        rng = np.random.default_rng(11 + fortran_consts)
        n = 4000
        base = dict(minlogtau=ps["minlogtau"], dlogtau=ps["dlogtau"], NumTau=ps["NumTau"])
        # (a) random cells at the cross-section of the runs: tau 6e-4 ... 600, dtau/tau 1e-12 ... 1
        cd_in = 10.0 ** rng.uniform(14.0, 20.0, n)
        cd_out = cd_in * (1.0 + 10.0 ** rng.uniform(-12.0, 0.0, n))
        flux, vol = 10.0 ** rng.uniform(0.0, 8.0, n), 10.0 ** rng.uniform(60.0, 72.0, n)
        # (b) sig = 1: the limit, thin cells across table intervals, beyond the end, vol_nhi = 0
        lim_cd, lim_thick = RP.limit_cases(fortran_consts)
        cases_b = [(1.0, 0.0, c, 2.0) for c in lim_cd]
        cases_b += [(1.0, 1e-6, 1e-6 + 0.9e-7, 2.0), (1.0, 3e-3, 3e-3 + 0.99e-7, 2.0)]       # thin, 9 % and 0.003 % apart
        cases_b += [(5.0, 1e5, 2e5, 2.0), (5.0, 1e7, 1e300, 3.0), (5.0, 2e4, 2e4, 3.0)]                       # a == b
        cases_b += [(1.0, 1e-3, 2e-3, 0.0), (0.0, 1e-3, 2e-3, 0.0), (1.0, 1e5, 2e5, 0.0), (1.0, 1e-6, 1e-6 + 0.5e-7, 0.0)]   # vol_nhi = 0
        fb, ib, ob, vb = (np.array(c) for c in zip(*cases_b))
        for heat in (False, True):
            op = "heat" if heat else "photo"
            kw = dict(base, sig=SIG)
            got = lib.debug_rate_primitives(op, flux, cd_in, cd_out, vol, **kw)
            want, thick = _compose(lib, kw, fortran_consts, flux, cd_in, cd_out, vol, heat)
            print(f"{op}, fortran_consts = {fortran_consts}: {int(thick.sum())} thick and {int((~thick).sum())} thin random cells, "
                  f"{int((~_same_bits(got, want)).sum())} differ from the composition")
            assert thick.sum() > n // 4 and (~thick).sum() > n // 10
            assert np.all(_same_bits(got, want))
            kw = dict(base, sig=1.0)
            got = lib.debug_rate_primitives(op, fb, ib, ob, vb, **kw)
            want, thick = _compose(lib, kw, fortran_consts, fb, ib, ob, vb, heat)
            assert np.array_equal(thick[:3], lim_thick) and not thick[3] and not thick[4] and thick[5] and thick[6] and not thick[7]
            assert np.all(_same_bits(got, want)), (op, got, want)
            # exactly at the limit a cell is thin: its rate carries the thin table's value (sets of disjoint ranges), not a difference
            # of the thick one's
            thin_name = "heat_thin" if heat else "thin"
            t_at = lib.debug_rate_primitives("lookup", np.array([0.0 if fortran_consts else lim_cd[1]]), which=thin_name, **kw)[0][0]
            assert got[1] == 0.5 * lim_cd[1] * t_at
            # the thin table is read at tau_out, under Fortran constants at tau_in: different intervals, different values
            v_in, v_out = lib.debug_rate_primitives("lookup", np.array([ib[3], ob[3]]), which=thin_name, **kw)[0]
            assert v_in != v_out and got[3] == 0.5 * (ob[3] - ib[3]) * (v_in if fortran_consts else v_out)
            # a == b beyond the table's end: exactly +0
            assert np.all(got[5:8] == 0.0) and not np.signbit(got[5:8]).any()
            # vol_nhi = 0: what the same IEEE expression gives (inf, NaN)
            assert np.isinf(got[8]) and np.isnan(got[9]) and np.isnan(got[10]) and np.isinf(got[11])
    finally:
        lib.set_option(capi.OPT_FORTRAN_CONSTANTS, 0)


def test_grey_rates(dev):
    """grey_rate_per_atom against the exact formula (rates.cu:48-64) at the tolerance of exp: 2 ulp on each exponential."""
    p, lib, capi = dev
    if not p.cuda_is_init():
        _fresh(p)
    rng = np.random.default_rng(21)
    n = 3000
    cd_in = 10.0 ** rng.uniform(13.0, 19.0, n)                 # tau_out <= 265: e^-tau stays a normal double
    cd_out = cd_in * (1.0 + 10.0 ** rng.uniform(-10.0, 0.5, n))
    lim_cd, _ = RP.limit_cases(0)
    cd_in = np.concatenate([cd_in, np.zeros(3)])
    cd_out = np.concatenate([cd_out, lim_cd / SIG])
    flux, vol = 10.0 ** rng.uniform(0.0, 8.0, n + 3), 10.0 ** rng.uniform(60.0, 72.0, n + 3)
    got = lib.debug_rate_primitives("grey", flux, cd_in, cd_out, vol, sig=SIG)
    hi, lo, bound = RP.grey_exact(flux, cd_in, cd_out, vol, SIG, 0)
    share = RP.error_against(got, hi, lo) / bound
    thick = np.abs(cd_out * SIG - cd_in * SIG) > 1e-7
    print(f"grey rates: {share[thick].max():.3f} of 4 eps max(e^-tau_in, e^-tau_out) |pref| over {int(thick.sum())} thick cells, "
          f"{share[~thick].max():.3f} of the thin cells' bound over {int((~thick).sum())}")
    assert thick.sum() > n // 4 and (~thick).sum() > n // 10
    assert share.max() <= 1.0


# ---- one tie to a production kernel ---------------------------------------------------------------------------------------------
def test_plane_flux_kernel_is_the_composition_of_the_debug_lookups(dev):
    """N = 20, a flux through the -x face, no point sources, the checkerboard of thin and thick cells: phi_ion equals, bit for bit,
    the march formed in numpy as plane_flux_kernel forms it (cd += n dr, tau = cd sig, pref = flux / (n dr), the carried
    T_thick(tau_in)) with every table value taken from the debug kernel's LOOKUP.  Each step is one rounded operation, pinned above."""
    p, lib, capi = dev
    N, flux = 20, 2.5
    nd, xh, dr = PF.checkerboard_medium(N)
    thin, thick, dlog = cases.soft_tables()
    _fresh(p, N)
    _TABLES_ON_DEVICE.clear()
    p.photo_table_to_device(thin, thick)
    lib.source_data_to_device(np.zeros(0, dtype=np.int32), np.zeros(0), 0)
    lib.grid_to_device(capi.GRID_NDENS, nd)
    lib.grid_to_device(capi.GRID_XH_AV, xh)
    numtau = thin.shape[0]
    try:
        lib.plane_flux([PF.face_index("-x")], [flux], [0])
        lib.raytrace_device(6.0, SIG, dr, 0, 0, cases.MINLOGTAU, dlog, numtau)
        phi = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
    finally:
        lib.plane_flux((), ())
    kw = dict(sig=SIG, minlogtau=cases.MINLOGTAU, dlogtau=dlog, NumTau=numtau)
    n_abs = nd * (1.0 - xh)                                     # absorber_density(n, x, 0, 0)
    vn = n_abs * dr                                             # [m][a][b], m the march index
    cd = np.cumsum(vn, axis=0)                                  # sequential: cd(m) = cd(m - 1) + vn(m)
    for m in range(1, N):
        assert np.array_equal(cd[m], cd[m - 1] + vn[m])
    tau_out = cd * SIG
    tau_in = np.concatenate([np.zeros((1, N, N)), tau_out[:-1]])
    t_out = lib.debug_rate_primitives("lookup", tau_out, which="thick", **kw)[0].reshape(N, N, N)
    t_first = lib.debug_rate_primitives("lookup", np.zeros(1), which="thick", **kw)[0][0]
    t_in = np.concatenate([np.full((1, N, N), t_first), t_out[:-1]])
    t_thin = lib.debug_rate_primitives("lookup", tau_out, which="thin", **kw)[0].reshape(N, N, N)
    dtau = tau_out - tau_in
    is_thick = np.abs(dtau) > 1e-7
    pref = flux / vn
    want = 0.0 + np.where(is_thick, pref * (t_in - t_out), pref * dtau * t_thin)
    differ = int((~_same_bits(phi, want)).sum())
    print(f"plane-flux sweep against the composition of the debug lookups: {differ} of {N ** 3} cells differ; "
          f"{int(is_thick.sum())} thick, {int((~is_thick).sum())} thin")
    assert is_thick.sum() > N ** 3 // 4 and (~is_thick).sum() > N ** 3 // 4 and np.all(vn > 0)
    assert differ == 0
