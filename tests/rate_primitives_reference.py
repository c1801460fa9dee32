"""TEST INFRASTRUCTURE: high-precision references, input sets and error bounds for the device functions every rate goes through
(pyc2ray_amd/csrc/rates_device.hpp), shared by tests/test_rate_primitives_reference.py (CPU) and
tests/test_gpu_rate_primitives.py (GPU, through asora_debug_rate_primitives).

High precision comes from mpmath where it imports (it travels with sympy) and from the standard library's ``decimal`` otherwise;
both are used at 50 digits.  A high-precision value v is handed to numpy as a pair of doubles (hi, lo) with hi = fl(v),
lo = fl(v - hi), so an error is formed as |(got - hi) - lo|: got - hi is exact where the two are close, and the pair carries
v to 2^-106 relative.

The bounds, and where their constants come from
-----------------------------------------------
``log2_bound``:  E(x) = 8.2e-15 + 2^-51 + ulp(log2 x)/2 for log2_pos(x) = e + ((log2 c - 1) + p(r)).
  * 8.2e-15: the series log2(1 + r) = r/ln2 (1 - r/2 + r^2/3 - r^3/4 + ...) is cut after four terms; the first one dropped is
    r^5/(5 ln 2), and |r| = |m'/c - 1| <= 2^-9 / c <= 1/513 on a table of 2^8 intervals of the mantissa m' in [1, 2) with
    centres c >= 1 + 2^-9: (1/513)^5 / (5 ln 2) = 8.12e-15 < 8.2e-15 (at |r| = 2^-9 itself it would be 8.2008e-15).  The terms
    after it alternate and shrink, so the first one bounds the tail.
  * 2^-51 = 4 x 2^-53: four roundings of values of magnitude <= 1 -- the table entries 2/c (it enters r as m x error, m < 1) and
    log2 c - 1, the fused r = fma(m, 2/c, -1) (|r| < 2^-9: far less than 2^-53, counted whole), and the sum (log2 c - 1) + p.
    The roundings inside p are of terms <= |r| and are covered by what the third allowance leaves over.
  * ulp(log2 x)/2: the final e + (...), rounded to nearest.
``lookup_bound``:  S (k1 E(tau) + ulp(real_i)) + 2 eps max(|T_i|, |T_i+1|), eps = 2^-53.
  * the table index is real_i = fma(log2 tau, k1, k0) + kc: the logarithm's error E enters times k1 = log10(2)/dlogtau; the
    fused multiply-add and the addition round once each, by at most ulp(real_i)/2.  kc (lut_index_constants of the library) is what
    the roundings of the doubles k1 and k0 themselves leave out (``index_constant_errors``): without it k0 = 1667.67, off by
    1.1e-13, cancels against k1 log2 tau at small optical depths (production parameters) and the index of 160 at tau = 1e-18 is
    off by five of its ulp -- which this bound has no room for, and which is how the term came to be.
  * F, the exact piecewise-linear interpolant, is continuous: an index that is off by d moves the value by at most S d, S the
    largest |T_j+1 - T_j| of the interval that holds the exact index and its nearer neighbour -- also when d carries the index
    across the knot between them.
  * 2 eps max|T|: the device forms T_i+1 - T_i (one rounding, <= eps |T_i+1 - T_i| <= eps max|T| for a table of one sign, times
    a residual < 1) and fma(residual, difference, T_i) (one rounding, <= eps |F| <= eps max|T|).
``grey_bound``:  4 eps' max(e^-tau_in, e^-tau_out) |pref| for thick cells, eps' = 2^-52 -- 2 ulp on each of the two exponentials,
  an ulp of e^-tau being at most 2^-52 e^-tau.  For thin cells, pref dtau e^-tau_in: 2 ulp on the one exponential and the
  roundings of the two products, (2 eps' + 2 eps) |pref dtau| e^-tau_in.
"""
import math
from fractions import Fraction

import numpy as np

try:
    import mpmath as _mp
except ImportError:             # pragma: no cover
    _mp = None
import decimal as _dec

DIGITS = 50
LOG_TABLE_BITS = 8
LOG_TABLE_SIZE = 1 << LOG_TABLE_BITS
C1, C2, C3, C4 = 1.4426950408889634074, -0.72134752044448170368, 0.48089834696298780245, -0.36067376022224085184
EPS = 2.0 ** -53
TAU_MIN, TAU_MAX = 1.0e-20, 1.0e300          # the clamps of lookup_issue
LOG2_EDGE_EXPONENTS = (-60, -1, 0, 1, 7, 900)
TABLES = ("thick", "thin", "heat_thick", "heat_thin")


# ---- high precision, on mpmath or decimal ------------------------------------------------------------------------------------
class _HP:
    """The few operations the references need, on mpmath (``use_mpmath``) or on decimal."""

    def __init__(self, use_mpmath):
        self.mp = _mp if use_mpmath else None
        if self.mp is not None:
            self.ctx = _mp.mp.clone()
            self.ctx.dps = DIGITS
        else:
            self.ctx = _dec.Context(prec=DIGITS)

    def num(self, v):
        """float, int or Fraction, exactly (a Fraction to DIGITS digits)."""
        if isinstance(v, Fraction):
            return self.num(v.numerator) / self.num(v.denominator)
        if self.mp is not None:
            return self.ctx.mpf(v)
        return self.ctx.create_decimal(_dec.Decimal(v))

    def log2(self, v):
        if self.mp is not None:
            return self.ctx.log(v, 2)
        return self.ctx.divide(self.ctx.ln(v), self.ctx.ln(_dec.Decimal(2)))

    def log10_2(self):
        return self.ctx.log10(self.num(2)) if self.mp is not None else self.ctx.log10(_dec.Decimal(2))

    def exp(self, v):
        return self.ctx.exp(v)

    def mul(self, a, b):
        return a * b if self.mp is not None else self.ctx.multiply(a, b)

    def add(self, a, b):
        return a + b if self.mp is not None else self.ctx.add(a, b)

    def sub(self, a, b):
        return a - b if self.mp is not None else self.ctx.subtract(a, b)

    def div(self, a, b):
        return a / b if self.mp is not None else self.ctx.divide(a, b)

    def floor(self, v):
        return int(self.ctx.floor(v)) if self.mp is not None else int(v.to_integral_value(rounding=_dec.ROUND_FLOOR))

    def pair(self, v):
        """(hi, lo) doubles of v."""
        hi = float(v)
        return hi, float(self.sub(v, self.num(hi)))


def hp(use_mpmath=None):
    return _HP(_mp is not None if use_mpmath is None else use_mpmath)


def _pairs(h, values):
    out = np.array([h.pair(v) for v in values], dtype=np.float64).reshape(-1, 2)
    return out[:, 0].copy(), out[:, 1].copy()


def error_against(got, hi, lo):
    """|got - (hi + lo)| in doubles."""
    return np.abs((np.asarray(got, dtype=np.float64) - hi) - lo)


# ---- log2 --------------------------------------------------------------------------------------------------------------------
def log2_exact_hp(x, h=None):
    """log2 of every element of x as high-precision numbers (a list)."""
    h = h or hp()
    return [h.log2(h.num(float(v))) for v in np.asarray(x, dtype=np.float64).ravel()]


def log2_exact(x, h=None):
    """(hi, lo): log2 x to twice the precision of a double."""
    h = h or hp()
    return _pairs(h, log2_exact_hp(x, h))


def log2_bound(x, log2_hi=None):
    """E(x) = 8.2e-15 + 2^-51 + ulp(log2 x)/2 (module docstring)."""
    l2 = np.log2(np.asarray(x, dtype=np.float64)) if log2_hi is None else log2_hi
    return 8.2e-15 + 2.0 ** -51 + 0.5 * np.spacing(np.abs(l2))


def _fma(a, b, c):
    """a b + c formed exactly and rounded once."""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


_LOGTAB = {}
_CACHE = {}


def log_table(h=None):
    """{2/c, log2 c - 1} for the centres c = 1 + (i + 1/2) / 2^8 of the mantissa intervals, each rounded once to a double
    (the library forms them in long double and rounds again: the same doubles but for rare double roundings, inside 2^-51)."""
    if "t" not in _LOGTAB:
        h = h or hp()
        tx, ty = np.empty(LOG_TABLE_SIZE), np.empty(LOG_TABLE_SIZE)
        for i in range(LOG_TABLE_SIZE):
            c = Fraction(2 * LOG_TABLE_SIZE + 2 * i + 1, 2 * LOG_TABLE_SIZE)
            tx[i] = float(Fraction(2) / c)          # (Fraction -> float rounds correctly)
            ty[i] = float(h.sub(h.log2(h.num(c)), h.num(1)))
        _LOGTAB["t"] = (tx, ty)
    return _LOGTAB["t"]


def log2_pos_emulated(x, contract_last=False, details=False):
    """log2_pos of rates_device.hpp restated in float64: frexp, the interval of the mantissa's leading 8 bits, r = fma(m, 2/c, -1),
    the four-term series by Horner with fused steps, e + ((log2 c - 1) + p).  contract_last: p = r q is not rounded on its own
    but fused into (log2 c - 1) + r q, as a compiler that contracts may do.  details: also r."""
    x = np.asarray(x, dtype=np.float64).ravel()
    tx, ty = log_table()
    m, e = np.frexp(x)
    idx = (m.view(np.int64) >> (52 - LOG_TABLE_BITS)) & (LOG_TABLE_SIZE - 1)
    out, rs = np.empty(x.shape), np.empty(x.shape)
    for j in range(x.size):
        t0, t1 = float(tx[idx[j]]), float(ty[idx[j]])
        r = _fma(float(m[j]), t0, -1.0)
        q = _fma(r, _fma(r, _fma(r, C4, C3), C2), C1)
        inner = _fma(r, q, t1) if contract_last else t1 + r * q
        out[j] = float(e[j]) + inner
        rs[j] = r
    return (out, rs) if details else out


def powers_of_two():
    """Every exact power of two in [1e-20, 1e300]."""
    lo, hi = math.ceil(math.log2(TAU_MIN)), math.floor(math.log2(TAU_MAX))
    return np.ldexp(1.0, np.arange(lo, hi + 1))


def log2_exact_at_powers_of_two():
    """Does log2_pos return the exponent itself at every power of two?  Decided by the restatement, in both forms the compiler may
    give the last product: only if both say yes does the GPU test assert it of the device."""
    if "p2" not in _CACHE:
        p2 = powers_of_two()
        _CACHE["p2"] = all(np.array_equal(log2_pos_emulated(p2, contract_last=c), np.log2(p2)) for c in (False, True))
    return _CACHE["p2"]


def interval_edges():
    """At each exponent of LOG2_EDGE_EXPONENTS: the 256 lower edges 2^e (1 + i/256) of the table's mantissa intervals, each with
    the double below and the double above."""
    i = np.arange(LOG_TABLE_SIZE, dtype=np.float64)
    edges = np.concatenate([np.ldexp(1.0 + i / LOG_TABLE_SIZE, e) for e in LOG2_EDGE_EXPONENTS])
    return np.concatenate([np.nextafter(edges, 0.0), edges, np.nextafter(edges, np.inf)])


def log2_inputs():
    """The input set of the log2 tests: 20 000 log-uniform in [1e-20, 1e300], 20 000 log-uniform in [1e-8, 1e3] (where tau lives),
    the interval edges, the powers of two, and the two clamps themselves."""
    rng = np.random.default_rng(20250)
    wide = 10.0 ** rng.uniform(-20.0, 300.0, 20000)
    tau = 10.0 ** rng.uniform(-8.0, 3.0, 20000)
    x = np.concatenate([wide, tau, interval_edges(), powers_of_two(), [TAU_MIN, TAU_MAX]])
    return np.clip(x, TAU_MIN, TAU_MAX)


def log2_reference():
    """The log2 input set with its references, computed once: dict(x, hp (list), hi, lo, bound)."""
    if "log2" not in _CACHE:
        h = hp()
        x = log2_inputs()
        vals = log2_exact_hp(x, h)
        hi, lo = _pairs(h, vals)
        r = dict(x=x, hp=vals, hi=hi, lo=lo, bound=log2_bound(x, hi))
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE["log2"] = r
    return _CACHE["log2"]


# ---- table lookup ------------------------------------------------------------------------------------------------------------
def lookup_tables(table_len, seed=7):
    """Two table sets of four tables with pairwise disjoint value ranges: (2, 4, table_len), set s table t random in
    [10 s + 2 t + 1, 10 s + 2 t + 2) -- thick [1,2), thin [3,4), heat thick [5,6), heat thin [7,8), set 1 the same + 10."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.0, 1.0, (2, 4, table_len))
    for s in range(2):
        for k in range(4):
            t[s, k] += 10 * s + 2 * k + 1
    return t


def lookup_parameter_sets():
    """name -> dict(minlogtau, dlogtau, NumTau, table_len): the production set of tests/data/parameters_test.yml (2000 intervals
    from 10^-20 to 10^4, tau = 0 in front: 2001 entries, and the table length passed as NumTau, as the package does), and short
    tables of 21 entries with NumTau on the three sides of the index limit (19 < table_len - 1, 20 = table_len - 1, 21 = table_len:
    the reference's read past the end)."""
    import os
    import yaml
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "parameters_test.yml")) as f:
        ph = yaml.safe_load(f)["Photo"]
    n = int(ph["NumTau"])
    lo, hi = float(ph["minlogtau"]), float(ph["maxlogtau"])
    sets = {"production": dict(minlogtau=lo, dlogtau=(hi - lo) / n, NumTau=n + 1, table_len=n + 1)}
    for numtau in (19, 20, 21):
        sets[f"short{numtau}"] = dict(minlogtau=-20.0, dlogtau=24.0 / 20, NumTau=numtau, table_len=21)
    return sets


def index_limit(NumTau, table_len):
    """The largest real index: float(NumTau) of the reference, and never past the last entry."""
    return min(float(np.float32(NumTau)), float(table_len - 1))


def knots(minlogtau, dlogtau, table_len):
    """tau at the integer indices 1 ... table_len - 1 (the doubles nearest 10^(minlogtau + (j - 1) dlogtau)), each with its two
    neighbouring doubles."""
    j = np.arange(1, table_len, dtype=np.float64)
    t = 10.0 ** (minlogtau + (j - 1.0) * dlogtau)
    return np.concatenate([np.nextafter(t, 0.0), t, np.nextafter(t, np.inf)])


def lookup_inputs(minlogtau, dlogtau, table_len):
    """The log2 set taken as optical depths, plus the knots of the table."""
    return np.concatenate([log2_inputs(), knots(minlogtau, dlogtau, table_len)])


def exact_index(tau, minlogtau, dlogtau, NumTau, table_len, log2_hp=None, h=None):
    """min(limit, max(0, 1 + (log10 max(1e-20, tau) - minlogtau)/dlogtau)) in high precision -> (integer part, residual hi, lo)."""
    h = h or hp()
    tau = np.clip(np.asarray(tau, dtype=np.float64).ravel(), TAU_MIN, None)
    l2 = log2_exact_hp(tau, h) if log2_hp is None else log2_hp
    k1 = h.div(h.log10_2(), h.num(dlogtau))
    k0 = h.sub(h.num(1), h.div(h.num(minlogtau), h.num(dlogtau)))
    limit = index_limit(NumTau, table_len)
    i0, rh, rl = np.empty(tau.size, dtype=np.int64), np.empty(tau.size), np.empty(tau.size)
    zero, top = h.num(0), h.num(limit)
    for j, v in enumerate(l2):
        x = h.add(k0, h.mul(k1, v))
        if x < zero:
            x = zero
        if x > top:
            x = top
        i = h.floor(x)
        i0[j] = i
        rh[j], rl[j] = h.pair(h.sub(x, h.num(i)))
    return i0, rh, rl


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    split = 134217729.0
    ca, cb = split * a, split * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def interp_exact(table, tau, minlogtau, dlogtau, NumTau, index=None):
    """The reference's photo_lookuptable (rates.cu:70-83) as the exact piecewise-linear function F of the exact index, an index
    past the last entry reading the last entry: dict(hi, lo: F as a pair of doubles; index: the exact real index (a double);
    i0; slope: the largest |T_j+1 - T_j| over the interval that holds the index and its nearer neighbour; tmax:
    max(|T_i0|, |T_i0+1|)).  index: (i0, residual hi, lo) of exact_index where it has been formed already."""
    table = np.asarray(table, dtype=np.float64)
    last = table.shape[0] - 1
    i0, rh, rl = exact_index(tau, minlogtau, dlogtau, NumTau, table.shape[0]) if index is None else index
    top = int(index_limit(NumTau, table.shape[0]))
    at = lambda j: table[np.clip(np.minimum(j, top), 0, last)]        # (the index never passes `top`: the table is flat behind it)
    t0, t1 = at(i0), at(i0 + 1)
    dh, dl = _two_sum(t1, -t0)
    ph, pl = _two_prod(rh, dh)
    sh, sl = _two_sum(t0, ph)
    lo = sl + (pl + rh * dl + rl * dh)
    hi, lo = _two_sum(sh, lo)
    near = np.where(rh < 0.5, i0 - 1, i0 + 1)
    slope = np.maximum(np.abs(t1 - t0), np.abs(at(near + 1) - at(near)))
    return dict(hi=hi, lo=lo, index=i0 + rh, i0=i0, slope=slope, tmax=np.maximum(np.abs(t0), np.abs(t1)))


def lookup_bound(F, tau, dlogtau, log2_hi=None):
    """S (k1 E(tau) + ulp(real_i)) + 2 eps max(|T_i|, |T_i+1|) (module docstring)."""
    k1 = 0.30102999566398119521 / dlogtau
    tau = np.clip(np.asarray(tau, dtype=np.float64), TAU_MIN, TAU_MAX)
    return F["slope"] * (k1 * log2_bound(tau, log2_hi) + np.spacing(F["index"])) + 2.0 * EPS * F["tmax"]


def index_constant_errors(minlogtau, dlogtau):
    """(k0 as the library forms it in doubles - k0, the same for k1): k0 = 1 - minlogtau/dlogtau, k1 = log10(2)/dlogtau.  The
    index fma(log2 tau, k1, k0) carries k0's error whole and k1's times log2 tau -- under the cancellation of k0 = 1667.67 against
    k1 log2 tau at small optical depths (production parameters) far more than an ulp of the index itself; the library's term kc
    takes it out again."""
    h = hp()
    k1 = h.div(h.log10_2(), h.num(dlogtau))
    k0 = h.sub(h.num(1), h.div(h.num(minlogtau), h.num(dlogtau)))
    return float(h.sub(h.num(1.0 - minlogtau / dlogtau), k0)), float(h.sub(h.num(0.30102999566398119521 / dlogtau), k1))


def table_end(minlogtau, dlogtau, NumTau, table_len):
    """The smallest double tau from which the exact index has reached the limit: 10^(minlogtau + dlogtau (limit - 1)), rounded up."""
    h = hp()
    limit = index_limit(NumTau, table_len)
    expo = h.add(h.num(minlogtau), h.mul(h.num(dlogtau), h.num(limit - 1.0)))
    ten = h.num(10)
    v = h.ctx.power(ten, expo)
    t = float(v)
    while h.num(t) < v:
        t = float(np.nextafter(t, np.inf))
    return t


def end_threshold(minlogtau, dlogtau, NumTau, table_len):
    """10^(minlogtau + dlogtau limit): from here on (one interval past table_end, so that no rounding of the index matters) a
    lookup returns the last entry of its table exactly."""
    return 10.0 ** (minlogtau + dlogtau * index_limit(NumTau, table_len))


def clamp_inputs():
    """(optical depths that must give the bits of tau = 1e-20, 1e-20 itself)."""
    return np.array([0.0, -0.0, -1.0, 5e-324, 1e-30, np.nan]), TAU_MIN


# ---- division ----------------------------------------------------------------------------------------------------------------
def _random_doubles(rng, n, emin, emax):
    mant = 1.0 + rng.integers(0, 1 << 52, n).astype(np.float64) * 2.0 ** -52
    sign = np.where(rng.integers(0, 2, n) == 1, -1.0, 1.0)
    return sign * np.ldexp(mant, rng.integers(emin, emax + 1, n))


def division_inputs():
    """name -> (x, y): 2e6 pairs with exponents uniform in 2^+-340 and random mantissas and signs; 1e5 pairs whose divisor's
    mantissa lies within 8 ulp of 1.0 and of 2.0; and the operand families of the callers -- the short-characteristics
    interpolation (a weighted sum of column densities over the sum of its weights, which is 1 to rounding) and
    flux / (vol nHI) at cgs magnitudes 1e48 ... 1e56 over 1e60 ... 1e72."""
    rng = np.random.default_rng(4711)
    sets = {"random": (_random_doubles(rng, 2_000_000, -340, 340), _random_doubles(rng, 2_000_000, -340, 340))}
    n = 100_000
    k = rng.integers(0, 9, n).astype(np.float64)
    near_one = 1.0 + k * 2.0 ** -52
    near_two = 2.0 - k * 2.0 ** -52           # (the doubles below 2.0 are 2^-52 apart)
    y = np.ldexp(np.where(rng.integers(0, 2, n) == 1, near_one, near_two), rng.integers(-340, 341, n))
    sets["divisor_mantissa_at_1_and_2"] = (_random_doubles(rng, n, -340, 340), y)
    n = 200_000
    w = rng.uniform(0.0, 1.0, (4, n))
    w[:, : n // 4] = rng.uniform(0.0, 1e-6, (4, n // 4))
    w[rng.integers(0, 4, n // 4), np.arange(n // 4)] = 1.0                 # one dominant corner
    w /= w.sum(axis=0)
    cd = 10.0 ** rng.uniform(10.0, 24.0, (4, n))
    sets["interpolation"] = ((w * cd).sum(axis=0), w.sum(axis=0))
    sets["flux_over_vol_nhi"] = (10.0 ** rng.uniform(48.0, 56.0, n), 10.0 ** rng.uniform(60.0, 72.0, n))
    return sets


# ---- products and sums that must not be fused ----------------------------------------------------------------------------------
def fused(a, b, c):
    """fl(a b + c) of every element, the product exact."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    return np.array([_fma(float(p), float(q), float(r)) for p, q, r in zip(a.ravel(), b.ravel(), c.ravel())]).reshape(a.shape)


def unfused_operands(n=2000):
    """Operands for which rounding each operation on its own and fusing give different bits (asserted by the host test):
    dict(tau=(cd_in, cd_out, sig): fl(cd_out sig) - fl(cd_in sig) against fma(cd_out, sig, -fl(cd_in sig));
         march=(cd, n, dr): cd + fl(n dr) against fma(n, dr, cd);
         absorber=(n, x, a, b): fl(fl(n fl(fl(1 - x) + b)) + a) against fma(n, fl(fl(1 - x) + b), a))."""
    rng = np.random.default_rng(99)

    def keep(args, separate, contracted, count):
        w = np.flatnonzero(separate != contracted)[:count]
        assert w.size == count
        return tuple(a[w] for a in args)

    m = 8 * n
    sig = np.full(m, 6.30e-18)
    cd_in = 10.0 ** rng.uniform(14.0, 16.0, m)                             # tau 6e-4 ... 6e-2, dtau < 2e-9: thin cells, whose
    cd_out = cd_in * (1.0 + 10.0 ** rng.uniform(-9.0, -7.5, m))            # rate carries dtau itself
    t_in = cd_in * sig
    tau = keep((cd_in, cd_out, sig), cd_out * sig - t_in, fused(cd_out, sig, -t_in), n)
    cd = 10.0 ** rng.uniform(14.0, 20.0, m)
    nn, dr = 10.0 ** rng.uniform(-6.0, -1.0, m), np.full(m, 2.3e21)
    march = keep((cd, nn, dr), cd + nn * dr, fused(nn, dr, cd), n)
    nd, x = 10.0 ** rng.uniform(-6.0, -1.0, m), rng.uniform(0.0, 1.0, m)
    a, b = 10.0 ** rng.uniform(-9.0, -5.0, m), 10.0 ** rng.uniform(-4.0, -1.0, m)
    inner = (1.0 - x) + b
    absorber = keep((nd, x, a, b), nd * inner + a, fused(nd, inner, a), n)
    return dict(tau=tau, march=march, absorber=absorber)


def absorber_without_lls():
    """(n, x) for absorber_density(n, x, 0, 0) == n (1 - x): random, x = 1, n = 0, NaN in either."""
    rng = np.random.default_rng(5)
    n = np.concatenate([10.0 ** rng.uniform(-8.0, 0.0, 1000), [1e-3, 0.0, 0.0, np.nan, 1e-3, 0.0]])
    x = np.concatenate([rng.uniform(0.0, 1.0, 1000), [1.0, 0.3, 1.0, 0.5, np.nan, np.nan]])
    return n, x


# ---- rates -------------------------------------------------------------------------------------------------------------------
def tau_photo_limit(fortran_consts):
    """TAU_PHOTO_LIMIT: the double 1e-7 (rates.cu:7), or the single 1e-7 promoted (photorates.f90:69)."""
    return float(np.float32(1.0e-7)) if fortran_consts else 1.0e-7


def limit_cases(fortran_consts):
    """cd_out (with cd_in = 0 and sig = 1, so dtau = cd_out) below, at and above the limit: (cd_out, thick?).  Exactly at the
    limit a cell is thin (the test is `>`)."""
    lim = tau_photo_limit(fortran_consts)
    cd = np.array([np.nextafter(lim, 0.0), lim, np.nextafter(lim, 1.0)])
    return cd, np.array([False, False, True])


def grey_exact(flux, cd_in, cd_out, vol_nhi, sig, fortran_consts, h=None):
    """photoion_rates_test (rates.cu:48-64) per atom: pref = flux 1e48 / vol_nhi in doubles as the device forms it, the
    exponentials and their difference in high precision -> (hi, lo, bound), bound as the module docstring derives it."""
    h = h or hp()
    flux, cd_in, cd_out, vol_nhi = (np.asarray(a, dtype=np.float64).ravel() for a in (flux, cd_in, cd_out, vol_nhi))
    tau_in, tau_out = cd_in * sig, cd_out * sig
    pref = flux * 1e48 / vol_nhi
    thick = np.abs(tau_out - tau_in) > tau_photo_limit(fortran_consts)
    vals, bound = [], np.empty(flux.size)
    for j in range(flux.size):
        ei, eo = h.exp(h.num(-float(tau_in[j]))), h.exp(h.num(-float(tau_out[j])))
        if thick[j]:
            v = h.mul(h.num(float(pref[j])), h.sub(ei, eo))
            bound[j] = 4.0 * 2.0 ** -52 * max(float(ei), float(eo)) * abs(pref[j])
        else:
            v = h.mul(h.mul(h.num(float(pref[j])), h.num(float(tau_out[j] - tau_in[j]))), ei)
            bound[j] = (2.0 * 2.0 ** -52 + 2.0 * EPS) * float(ei) * abs(pref[j] * (tau_out[j] - tau_in[j]))
        vals.append(v)
    hi, lo = _pairs(h, vals)
    return hi, lo, bound
