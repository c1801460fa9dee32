// Device functions shared by the raytracing kernels (raytrace.hip: ASORA path, subbox.hip: Fortran-path
// semantics): the table-based log2 and the photo_lookuptable of src/asora/rates.cu:70-83.
#pragma once
#include "asora_internal.hpp"

namespace asora {

constexpr double FOURPI = 12.566370614359172463991853874177;   // raytracing.cu:12
constexpr int LOG_TABLE_BITS = 8;
constexpr int LOG_TABLE_SIZE = 1 << LOG_TABLE_BITS;

// ---------------------------------------------------------------------------------------------
// Rates (src/asora/rates.cu)
// ---------------------------------------------------------------------------------------------

// log2 of a positive normal double: exponent + table (2^LOG_TABLE_BITS intervals of the mantissa, staged in LDS) + series in
// r = m/c - 1 around the interval centre c; it replaces log10 in the table lookup because two of them per cell dominated the
// instruction count.  8 bits (4 KiB of LDS; 7 bits with six terms until round 3a): |r| < 2^-9, FOUR terms; the first one
// dropped is r^5/(5 ln 2) < 8.2e-15, against an ulp of 3.5e-15 ... 7e-15 of log2(tau) itself for tau outside [2^-16, 2^16]
// and of 2.3e-13 ... 3.6e-12 of the table index k0 + k1 log2(tau) (k0 = 1 - minlogtau/dlogtau = 1668 ... 16668) that the
// logarithm is formed for: below the rounding of the index, like libm's log10 in the reference.
// Mantissa and exponent come through v_frexp_mant_f64 / v_frexp_exp_i32_f64 (x = m * 2^e, m in [0.5, 1)) rather than shifts and
// masks on the bit pattern (4 instead of 7 integer instructions per logarithm); the table therefore holds {2/c, log2(c) - 1} for
// the interval centres c in [1, 2) (ensure_logtab), so that r = m * (2/c) - 1 and log2 x = e + (log2 c - 1) + log2(1 + r).
// Asserted (tests/test_gpu_rate_primitives.py through asora_debug_rate_primitives, DESIGN.md section 3 "Rate primitives"): the
// result lies within 8.2e-15 + 2^-51 + ulp(log2 x)/2 of log2 x on both sides of every interval edge (|r| <= 1/513 there, the
// dropped term 8.12e-15).  The index carried more than that until the same tests measured it: the rounding of the doubles k0
// and k1 themselves, 1.4e-13 at tau = 1e-18 with k0 = 1668 -- five ulp of an index of 160.  lookup_issue now adds the term kc
// that holds what they leave out (lut_index_constants, asora_internal.hpp).
__device__ __forceinline__ double log2_pos(double x, const double2 *__restrict__ logtab)
{
    const double m = __builtin_amdgcn_frexp_mant(x);
    const int e = __builtin_amdgcn_frexp_exp(x);
    const int idx = (int)(__double_as_longlong(m) >> (52 - LOG_TABLE_BITS)) & (LOG_TABLE_SIZE - 1);
    const double2 t = logtab[idx];                 // {2/c, log2 c - 1}
    const double r = fma(m, t.x, -1.0);
    // log2(1+r) = r/ln2 * (1 - r/2 + r^2/3 - r^3/4)
    const double C1 = 1.4426950408889634074, C2 = -0.72134752044448170368, C3 = 0.48089834696298780245,
                 C4 = -0.36067376022224085184;
    const double p = r * fma(r, fma(r, fma(r, C4, C3), C2), C1);
    return (double)e + (t.y + p);
}

// photo_lookuptable, rates.cu:70-83 (== photorates.f90:130-147), in two halves so that the two
// dependent table loads can be in flight while other work is done.  The reference forms
// 1 + (log10(tau) - minlogtau)/dlogtau; here that is one fused multiply-add on log2(tau) with
// k1 = log10(2)/dlogtau, k0 = 1 - minlogtau/dlogtau, and one addition of kc.  Indices are clamped to the last table
// element (the reference reads one past the end when NumTau == len(table), tau >= 10^maxlogtau).
// Device layout of the rate tables (since round 4): each table as it is, T[0 .. len-1] plus one more element T[len] = T[len-1];
// a lookup is ONE 16-byte load of {T[i], T[i+1]} from an 8-byte-aligned address and the difference is formed in the kernel (one
// more v_add_f64).  The entries a wave's 64 lanes need then span half as many cache lines as with the pairs
// {T[i], T[i+1] - T[i]} of 16 bytes per entry used in rounds 1-3.  The lookups are the loop's only divergent accesses (LABNOTES
// round 4: 14 % of the trace on the quiet benchmark medium, 25 % on a field with ionisation fronts).  Same bits as the pairs:
// the host formed T[i+1] - T[i] with the same IEEE subtraction.
// The four tables of an allocation (thick, thin, heating thick, heating thin) follow each other at table_stride(len) entries.
constexpr int TABLE_ENTRY_SHIFT = 3;          // log2 of the bytes per entry
__host__ __device__ constexpr int table_stride(int table_len) { return table_len + 1; }
typedef double double2_a8 __attribute__((ext_vector_type(2), aligned(8)));      // a 16-byte load that may start on any double

struct Lookup { double2 t; double2 h; double residual; };   // h: the heating table at the same index
template <bool HEAT = false, typename Params = RtParams>
__device__ __forceinline__ Lookup lookup_issue(const double2 *__restrict__ table, double tau, const Params &p,
                                               const double2 *__restrict__ logtab, int offset = 0)
{   // offset: entries to skip in front (the thin table follows the thick one: a per-lane offset instead of a per-lane pointer)
    // (upper clamp: log2_pos is only defined for finite arguments -- for tau = +inf the mantissa/exponent split gives -inf, i.e.
    //  the FIRST table entry, where the reference's log10(inf) -> min(NumTau, .) reads the last one; any finite value beyond
    //  10^maxlogtau is clamped to the last entry by numtau_f below)
    const double l2 = log2_pos(fmin(fmax(1.0e-20, tau), 1.0e300), logtab);
    // numtau_f is clamped to table_len - 1 on the host (lut_index_limit): real_i >= table_len - 1 reads the last entry
    // (slope 0) whatever the residual, as the reference's i0 = i1 = NumTau does -- no integer clamp here
    // (lut_kc: what the roundings of the doubles k1 and k0 leave out, lut_index_constants -- one more v_add_f64)
    const double real_i = fmin(p.numtau_f, fmax(0.0, fma(l2, p.lut_k1, p.lut_k0) + p.lut_kc));
    const int i0 = (int)real_i;
    Lookup L;
    L.residual = __builtin_amdgcn_fract(real_i);          // real_i - (double)i0 for real_i >= 0, one instruction
    const unsigned i = (unsigned)(i0 + offset);
    // a 32-bit byte offset from the (wave-uniform) table base: one shift, and the load takes base + offset by itself
    const char *base = reinterpret_cast<const char *>(table);
    auto load16 = [](const char *q) -> double2 {
        const double2_a8 v = *reinterpret_cast<const double2_a8 *>(q);
        return double2{v.x, v.y};
    };
    L.t = load16(base + (i << TABLE_ENTRY_SHIFT));
    if (HEAT) L.h = load16(base + ((i + 2u * (unsigned)table_stride(p.table_len)) << TABLE_ENTRY_SHIFT)); else L.h = L.t;
    return L;
}
__device__ __forceinline__ double lookup_value(const Lookup &L) { return fma(L.residual, L.t.y - L.t.x, L.t.x); }
__device__ __forceinline__ double lookup_heat(const Lookup &L) { return fma(L.residual, L.h.y - L.h.x, L.h.x); }

// Host: table t (0 thick, 1 thin, 2 heating thick, 3 heating thin) of `len` entries into a buffer of 4 * len double2
// (4 * (len + 1) doubles fit for len >= 1)
inline void pack_rate_table(double2 *buffer, int t, const double *src, int len)
{
    double *d = reinterpret_cast<double *>(buffer) + (size_t)t * table_stride(len);
    for (int i = 0; i < len; ++i) d[i] = src[i];
    d[len] = src[len - 1];
}
// byte range of the tables [t0, t1) inside such a buffer
inline size_t rate_table_byte_offset(int t, int len) { return (size_t)t * table_stride(len) * ((size_t)1 << TABLE_ENTRY_SHIFT); }

// Products and sums that must NOT be contracted into a fused multiply-add, where the reference's result depends on
// each operation being rounded on its own (device code is compiled with -ffp-contract=fast, and HIP's __dmul_rn /
// __dadd_rn are plain operators that get contracted after inlining).  Instructions emitted under contract(off) carry
// no `contract` flag, so the backend leaves them alone wherever they are inlined.
__device__ __forceinline__ double mul_unfused(double a, double b)
{
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double add_unfused(double a, double b)
{
#pragma clang fp contract(off)
    return a + b;
}

// The absorber density the raytrace sees: neutral hydrogen plus the unresolved Lyman-limit systems of
// asora_lls_opacity, n_abs = n ((1 - x) + b) + a.  Written once, for prepare_nhi_kernel and the fused pass alike, and without
// contraction: each of the four operations is rounded on its own, so both sites -- and a host restatement -- form the same bits.
// a = b = 0 gives n (1 - x) exactly: (1 - x) + 0 and n (1 - x) + 0 change no bit of a value >= +0, and NaN stays NaN.
__device__ __forceinline__ double absorber_density(double n, double x, double a, double b)
{
#pragma clang fp contract(off)
    return n * ((1.0 - x) + b) + a;
}

// x / y for finite y != 0 of ordinary magnitude: hardware reciprocal, Newton on the reciprocal, one correction of the
// quotient -- 6 instructions instead of the 12 of the IEEE sequence (v_div_scale x 2, v_div_fmas, v_div_fixup guard against
// operands near the ends of the exponent range, which column densities, interpolation weights and cell volumes are not).
// ONE Newton step (two until the middle of round 3): v_rcp_f64 is good to 2^-24.4 (measured,
// tools/micro/div_accuracy.hip -> profiles/r03_div_accuracy.txt); a step squares that, and the correction q + r (x - y q)
// multiplies the quotient's error by the reciprocal's once more: 2^-73, far below half an ulp.  Over 6.7e7 random operand
// pairs both forms returned the correctly rounded (IEEE) quotient every time.  Asserted bit for bit on 2.5e6 pairs in every run
// of the suite (tests/test_gpu_rate_primitives.py: exponents over 2^+-340, divisors at the ends of the mantissa, the callers' operands).
// y = 0 gives NaN: callers that can meet it handle it themselves (see pref in raytrace.hip).
__device__ __forceinline__ double div_newton(double x, double y)
{
    double r = __builtin_amdgcn_rcp(y);
    r = fma(fma(-y, r, 1.0), r, r);
    const double q = x * r;
    return fma(fma(-y, q, x), r, q);
}

// photoion_rates_gpu rates.cu:16-41 divided by nHI (raytracing.cu:324), also in two halves.
// pref = flux/(vol*nHI) replaces the reference's two divisions by one.  A cell is "thick" when
// |tau_out - tau_in| > TAU_PHOTO_LIMIT: Gamma = pref*(T_thick(tau_in) - T_thick(tau_out)); else
// Gamma = pref*(tau_out - tau_in)*T_thin(tau_out) [rates.cu:37; photorates.f90:121 uses tau_in].
struct RateJob {
    double pref, dtau;       // dtau = tau_out - tau_in for thin cells, unused (0) for thick ones
    Lookup A, B;             // thick: T(tau_in), T(tau_out);  thin: T_thin(tau*), unused
    bool thick;
};
// `tab`: the [thick | thin | heat thick | heat thin] block of the source's table set (RtParams::src_spec)
__device__ __forceinline__ RateJob rate_issue(double flux, double cd_in, double cd_out, double vol_nhi,
                                              const RtParams &p, const double2 *__restrict__ logtab, const double2 *__restrict__ tab)
{
    // (un-fused products: tau_out - tau_in must be the difference of the two ROUNDED optical depths, as in the
    //  reference; fused into fma(cd_out, sig, -tau_in) it would carry the rounding error of one product -- a speck
    //  instead of 0 where nHI = 0, and a 1e-8 relative change of dtau for thin cells)
    const double tau_in = mul_unfused(cd_in, p.sig);
    const double tau_out = mul_unfused(cd_out, p.sig);
    // TAU_PHOTO_LIMIT: rates.cu:7 (double 1e-7) or photorates.f90:69 (single 1e-7 promoted)
    const double limit = p.fortran_consts ? (double)1.0e-7f : 1.0e-7;
    RateJob J;
    J.pref = flux / vol_nhi;
    J.thick = fabs(tau_out - tau_in) > limit;
    J.dtau = tau_out - tau_in;
    const double tau_thin = p.fortran_consts ? tau_in : tau_out;
    // one code path for both kinds of cell: per-lane table and arguments
    // thick table at [0, table_len), thin table at [table_len, 2*table_len) of one allocation
    const int toff = J.thick ? 0 : table_stride(p.table_len);
    J.A = lookup_issue(tab, J.thick ? tau_in : tau_thin, p, logtab, toff);
    J.B = lookup_issue(tab, J.thick ? tau_out : tau_thin, p, logtab, toff);
    return J;
}
__device__ __forceinline__ double rate_value(const RateJob &J)
{
    const double a = lookup_value(J.A), b = lookup_value(J.B);
    // (pref*(a - b), not pref*a - pref*b: the compiler would fuse the latter into fma(pref, a, -(pref*b)), which
    //  leaves the rounding error of pref*b -- a random-signed ~1e-16 relative speck -- where a == b, e.g. beyond the
    //  last table entry, where the reference's un-fused arithmetic gives exactly 0)
    return J.thick ? J.pref * (a - b) : J.pref * J.dtau * a;
}

// photoion_rates_test_gpu rates.cu:48-64 (analytic grey rates, GREY_NOTABLES builds), per atom
__device__ __forceinline__ double grey_rate_per_atom(double flux, double cd_in, double cd_out, double vol_nhi,
                                                     const RtParams &p)
{
    const double tau_in = mul_unfused(cd_in, p.sig), tau_out = mul_unfused(cd_out, p.sig);   // un-fused, see rate_issue
    const double limit = p.fortran_consts ? (double)1.0e-7f : 1.0e-7;
    const double pref = flux * 1e48 / vol_nhi;
    if (fabs(tau_out - tau_in) > limit) return pref * (exp(-tau_in) - exp(-tau_out));
    return pref * (tau_out - tau_in) * exp(-tau_in);
}

// heating rate of one cell per atom (photorates.f90:118,124), used for the source cell only
__device__ __forceinline__ double heat_rate_per_atom(double flux, double cd_in, double cd_out, double vol_nhi,
                                                     const RtParams &p, const double2 *__restrict__ logtab, const double2 *__restrict__ tab)
{
    const double tau_in = mul_unfused(cd_in, p.sig), tau_out = mul_unfused(cd_out, p.sig);   // un-fused, see rate_issue
    const double limit = p.fortran_consts ? (double)1.0e-7f : 1.0e-7;
    const double pref = flux / vol_nhi;
    const bool thick = fabs(tau_out - tau_in) > limit;
    const double tau_thin = p.fortran_consts ? tau_in : tau_out;
    const int toff = thick ? 0 : table_stride(p.table_len);
    const Lookup A = lookup_issue<true>(tab, thick ? tau_in : tau_thin, p, logtab, toff);
    const Lookup B = lookup_issue<true>(tab, thick ? tau_out : tau_thin, p, logtab, toff);
    return thick ? pref * (lookup_heat(A) - lookup_heat(B)) : pref * (tau_out - tau_in) * lookup_heat(A);
}

__device__ __forceinline__ double photo_rate_per_atom(double flux, double cd_in, double cd_out, double vol_nhi,
                                                      const RtParams &p, const double2 *__restrict__ logtab, const double2 *__restrict__ tab)
{
    if (p.grey) return grey_rate_per_atom(flux, cd_in, cd_out, vol_nhi, p);
    return rate_value(rate_issue(flux, cd_in, cd_out, vol_nhi, p, logtab, tab));
}

__device__ __forceinline__ int wrap_once(int x, int N)
{
    return x < 0 ? x + N : (x >= N ? x - N : x);
}

} // namespace asora
