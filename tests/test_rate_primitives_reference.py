"""CPU: the references, input sets and bounds of tests/rate_primitives_reference.py, and every precondition the GPU tests of the
rate primitives (tests/test_gpu_rate_primitives.py) rest on -- shown here, where no device is needed."""
import numpy as np

import rate_primitives_reference as RP


def test_high_precision_backends_agree():
    """mpmath (where it imports) and decimal give the same pairs of doubles."""
    x = np.array([1e-20, 3.7e-9, 0.5, 1.0, 1.0 + 2.0 ** -52, 2.0, 12345.678, 1e300])
    d = RP.log2_exact(x, RP.hp(use_mpmath=False))
    assert np.array_equal(d[0], np.log2(x)) or np.max(np.abs(d[0] - np.log2(x)) / np.spacing(np.abs(d[0]) + 1e-300)) <= 1
    assert d[0][3] == 0.0 and d[1][3] == 0.0 and d[0][5] == 1.0
    if RP._mp is None:
        return              # decimal is the only backend here
    m = RP.log2_exact(x, RP.hp(use_mpmath=True))
    assert np.array_equal(d[0], m[0])
    np.testing.assert_allclose(d[1], m[1], rtol=1e-12, atol=1e-45)


def test_log2_input_set():
    x = RP.log2_inputs()
    assert x.shape == (40000 + 3 * 256 * len(RP.LOG2_EDGE_EXPONENTS) + RP.powers_of_two().size + 2,)
    assert x.min() == 1e-20 and x.max() == 1e300 and np.all(np.isfinite(x))
    p2 = RP.powers_of_two()
    assert p2[0] / 2 < 1e-20 <= p2[0] and p2[-1] <= 1e300 < p2[-1] * 2 and np.all(np.frexp(p2)[0] == 0.5)
    # the edges: the lower edge opens interval i, the double below it closes interval i - 1
    e = RP.interval_edges().reshape(3, len(RP.LOG2_EDGE_EXPONENTS), 256)
    idx = lambda v: (np.frexp(v)[0].view(np.int64) >> 44) & 255
    assert np.array_equal(idx(e[1]), np.broadcast_to(np.arange(256), e[1].shape))
    assert np.array_equal(idx(e[2]), idx(e[1])) and np.array_equal(idx(e[0]), (idx(e[1]) - 1) % 256)


def test_emulated_log2_stays_within_the_bound():
    """The float64 restatement of log2_pos, with the last product rounded on its own and fused, on the full input set: inside
    E(x), |r| < 2^-9 at every point, and the share of E used (the GPU test prints the device's next to it)."""
    ref = RP.log2_reference()
    for contract in (False, True):
        got, r = RP.log2_pos_emulated(ref["x"], contract_last=contract, details=True)
        share = RP.error_against(got, ref["hi"], ref["lo"]) / ref["bound"]
        worst = int(np.argmax(share))
        print(f"emulated log2_pos (last product {'fused' if contract else 'rounded'}): {share.max():.3f} of E at x = {ref['x'][worst]!r}, "
              f"max |r| 2^9 = {np.max(np.abs(r)) * 512:.4f}")
        assert np.max(np.abs(r)) * 512 < 1.0
        assert share.max() <= 1.0


def test_emulated_log2_at_powers_of_two():
    """Whether log2_pos returns the exponent itself at a power of two is decided here: RP.log2_exact_at_powers_of_two()."""
    p2 = RP.powers_of_two()
    exact = [np.array_equal(RP.log2_pos_emulated(p2, contract_last=c), np.log2(p2)) for c in (False, True)]
    print("log2_pos(2^k) == k for every k, last product rounded / fused:", exact)
    assert RP.log2_exact_at_powers_of_two() == all(exact)


def test_dropped_term_and_index_claims():
    """The figures of the comments: r^5/(5 ln 2) at the largest |r| of the table, 1/513, is below 8.2e-15 (at 2^-9 it would not
    be: 8.2008e-15), and the production parameters are the ones the comments quote k0 for."""
    assert (1.0 / 513) ** 5 / (5 * np.log(2)) < 8.2e-15 < (2.0 ** -9) ** 5 / (5 * np.log(2))
    _, r = RP.log2_pos_emulated(RP.interval_edges(), details=True)
    assert 0.99 / 513 < np.max(np.abs(r)) <= (1.0 + 1e-12) / 513     # (2/c is a rounded double)
    p = RP.lookup_parameter_sets()["production"]
    assert (p["table_len"], p["NumTau"], p["minlogtau"], p["dlogtau"]) == (2001, 2001, -20.0, 0.012)
    k0 = 1.0 - p["minlogtau"] / p["dlogtau"]
    assert 1667 < k0 < 1668


def test_lookup_tables_are_disjoint():
    for n in (21, 2001):
        t = RP.lookup_tables(n)
        assert t.shape == (2, 4, n)
        ranges = [(t[s, k].min(), t[s, k].max()) for s in range(2) for k in range(4)]
        for a in range(8):
            lo = 10 * (a // 4) + 2 * (a % 4) + 1
            assert lo <= ranges[a][0] and ranges[a][1] < lo + 1
            for b in range(a + 1, 8):
                assert ranges[a][1] < ranges[b][0] or ranges[b][1] < ranges[a][0]


def test_parameter_sets_lie_on_the_three_sides_of_the_index_limit():
    s = RP.lookup_parameter_sets()
    assert [RP.index_limit(s[k]["NumTau"], s[k]["table_len"]) for k in ("short19", "short20", "short21")] == [19.0, 20.0, 20.0]
    assert RP.index_limit(2001, 2001) == 2000.0
    # the end of the table: at table_end the exact index has reached the limit, one double below it has not
    for k, p in s.items():
        end = RP.table_end(**p)
        i0, rh, rl = RP.exact_index(np.array([np.nextafter(end, 0.0), end]), **p)
        limit = RP.index_limit(p["NumTau"], p["table_len"])
        assert i0[1] + rh[1] == limit and rh[1] == 0.0 and i0[0] + rh[0] <= limit and (i0[0] < limit), k


def test_interp_exact_against_the_oracle():
    """interp_exact against the oracle's table_lookup (oracle/c2ray_oracle.c) through its photo-rates probe, on the tables and
    the range of optical depths of the raytracing cases, within the rounding of the oracle's own double index.  With a flux and a
    volume factor of 1, sig = 1 and cd_in = 0: phi_out of a thick cell is the thick table's value at tau_out, and phi_cell of a
    thin one is tau_out times the thin table's value at tau_out (one more product, undone by one division)."""
    import cases
    from oracle import oracle as O
    thin, thick, dlog = cases.soft_tables()
    rng = np.random.default_rng(1)
    tau_thick = np.concatenate([10.0 ** rng.uniform(-6.9, 5.0, 300), [1.0, 1e4, 1e5]])
    tau_thin = np.concatenate([10.0 ** rng.uniform(-21.0, -7.1, 200), [1e-20, 1e-30]])
    # the oracle's index: log10 of libm (1 ulp of |log10 tau| <= 32) and the subtraction, divided by dlogtau; the sum with 1
    index_error = 3 * np.spacing(32.0) / dlog + 2 * np.spacing(2048.0)
    for numtau in (thick.shape[0], thick.shape[0] - 1):
        probe = lambda t: O.photoion_rates(1.0, 0.0, t, 1.0, 1.0, thin, thick, cases.MINLOGTAU, dlog, NumTau=numtau, flags=O.ASORA_MODE)
        for name, table, tau, got, roundings in (("thick", thick, tau_thick, np.array([probe(t)[1] for t in tau_thick]), 4),
                                                 ("thin", thin, tau_thin, np.array([probe(t)[0] for t in tau_thin]) / tau_thin, 8)):
            F = RP.interp_exact(table, tau, cases.MINLOGTAU, dlog, numtau)
            tol = F["slope"] * index_error + roundings * RP.EPS * F["tmax"]
            err = RP.error_against(got, F["hi"], F["lo"])
            print(f"NumTau = {numtau}, {name}: interp_exact against the oracle, worst share of the oracle's own rounding {np.max(err / tol):.3f}")
            assert np.all(err <= tol)
    # and exactly, at an index formed without rounding: a table of 5 entries over minlogtau = 0, dlogtau = 1 at tau = 10^k
    t = np.array([3.0, 1.0, 4.0, 1.5, 9.0])
    F = RP.interp_exact(t, np.array([0.01, 1.0, 10.0, 100.0, 1000.0, 1e4, 1e9, np.sqrt(10.0)]), 0.0, 1.0, 5)
    assert np.array_equal(F["hi"][:7], [3.0, 1.0, 4.0, 1.5, 9.0, 9.0, 9.0]) and np.all(F["lo"][:7] == 0)
    assert abs(F["hi"][7] - 2.5) < 1e-15 and F["i0"][7] == 1


def test_knots_sit_on_integer_indices():
    p = RP.lookup_parameter_sets()["short20"]
    k = RP.knots(p["minlogtau"], p["dlogtau"], p["table_len"]).reshape(3, -1)
    i0, rh, rl = RP.exact_index(k.ravel(), **p)
    idx = (i0 + rh).reshape(3, -1)
    want = np.arange(1, p["table_len"])
    assert np.all(np.abs(idx[1] - want) < 1e-13)
    # the neighbouring doubles lie on either side: compared as (integer part, residual hi, lo), a double cannot tell them apart
    key = [[(int(a), float(b), float(c)) for a, b, c in zip(i0.reshape(3, -1)[q], rh.reshape(3, -1)[q], rl.reshape(3, -1)[q])] for q in range(3)]
    # (not at the first knot, the clamp 1e-20, nor at the last, the index limit)
    assert all(key[0][j] < key[1][j] < key[2][j] for j in range(1, want.size - 1))


def test_division_inputs():
    s = RP.division_inputs()
    x, y = s["random"]
    assert x.size == y.size == 2_000_000
    for a in (x, y):
        e = np.frexp(a)[1] - 1
        assert e.min() == -340 and e.max() == 340 and np.all(np.isfinite(a)) and np.all(a != 0) and (a < 0).any() and (a > 0).any()
    x, y = s["divisor_mantissa_at_1_and_2"]
    m = np.frexp(y)[0] * 2                      # in [1, 2)
    assert y.size == 100_000 and np.all((m - 1.0 <= 8 * 2.0 ** -52) | (2.0 - m <= 8 * 2.0 ** -52))
    assert (m == 1.0).any() and (m > 1.5).any() and (m - 1.0 == 8 * 2.0 ** -52).any()
    x, y = s["interpolation"]
    assert np.all(np.abs(y - 1.0) <= 4 * 2.0 ** -52) and (y != 1.0).any()
    x, y = s["flux_over_vol_nhi"]
    assert 1e48 <= x.min() and x.max() <= 1e56 and 1e60 <= y.min() and y.max() <= 1e72


def test_unfused_operands_differ_from_fused():
    """Every operand set the GPU test uses separates the separately rounded result from the fused one."""
    u = RP.unfused_operands()
    cd_in, cd_out, sig = u["tau"]
    t_in = cd_in * sig
    assert np.all(cd_out * sig - t_in != RP.fused(cd_out, sig, -t_in)) and cd_in.size == 2000
    cd, n, dr = u["march"]
    assert np.all(cd + n * dr != RP.fused(n, dr, cd))
    n, x, a, b = u["absorber"]
    inner = (1.0 - x) + b
    assert np.all(n * inner + a != RP.fused(n, inner, a)) and np.all(a != 0) and np.all(b != 0)
    n, x = RP.absorber_without_lls()
    assert (x == 1.0).any() and (n == 0.0).any() and np.isnan(n).any() and np.isnan(x).any()


def test_limit_cases_straddle_the_limit():
    assert RP.tau_photo_limit(False) == 1e-7 and RP.tau_photo_limit(True) == float(np.float32(1e-7)) != 1e-7
    for fc in (False, True):
        cd, thick = RP.limit_cases(fc)
        lim = RP.tau_photo_limit(fc)
        assert cd[0] < lim == cd[1] < cd[2] and np.array_equal(np.abs(cd * 1.0 - 0.0 * 1.0) > lim, thick)
        assert list(thick) == [False, False, True]
    # the two limits tell the two settings apart: a dtau between them is thick under one and thin under the other
    lo, hi = sorted((RP.tau_photo_limit(False), RP.tau_photo_limit(True)))
    assert lo < 0.5 * (lo + hi) < hi


def test_grey_reference():
    hi, lo, bound = RP.grey_exact([2.0, 2.0], [0.0, 1e17], [1e17, 1e17 * (1 + 1e-9)], [3e60, 3e60], 6.3e-18, False)
    want0 = 2.0 * 1e48 / 3e60 * (1.0 - np.exp(-0.63))
    assert abs(hi[0] - want0) <= 4 * np.spacing(want0) and bound[0] > 0 and bound[1] > 0
    assert abs(hi[1] / (2.0 * 1e48 / 3e60 * 0.63e-9 * np.exp(-0.63)) - 1) < 1e-6
