// fft_device.hpp -- what the units that transform a field share (power_spectrum.hip, smooth_field.hip; DESIGN.md sections 4.2h, 4.2i):
// the line transform in LDS with its plan, tile and LDS layout, the forming of the field from the grids, and the double-double sums
// of fixed order.  Device functions and small host helpers only: every kernel lives in the unit that launches it.
// The line transform (line_fft) is a mixed-radix Stockham autosort between two LDS buffers: a stage of radix p reads element
// idx + j N/p, j = 0 ... p - 1 -- contiguous in the work-item index -- and writes r + p (idx - r) + s k with the twiddle
// tw[(idx - r) k], r = idx mod s, s the product of the radices so far.  Radices 4, 2, 3, 5 and 7 have butterflies in registers, any
// other prime factor p a generic one of p multiply-adds per output (one work item per OUTPUT, so a prime N still fills the
// workgroup): N = 1 ... 645 all work, and the cost of a line grows with the sum of N's prime factors beyond 7 (N = 43 p, or prime,
// is slow).  tw[r] = exp(-2 pi i r / N), r = 0 ... N - 1, is tabulated once per mesh on the host in extended precision; no index
// beyond N - 1 is formed, no angle is multiplied, no recurrence is used.  Lines are stored with an odd pitch.
// The butterflies have the forward sign baked in; the inverse of a line is conj(line_fft(conj(.))), with the conjugations made on the
// load into LDS and on the store out of it (smooth_field.hip).
#pragma once
#include "asora_internal.hpp"

namespace asora {

constexpr int PS_THREADS = 256;
constexpr int PS_WAVES = PS_THREADS / 64;
constexpr int PS_RED_BLOCKS = 512;          // the workgroups of the mean-density sum: a constant, so that the order is the mesh's alone
constexpr int PS_MAX_FACTORS = 12;          // (2^12 > 645)

struct PsPlan {
    int nf;
    int radix[PS_MAX_FACTORS];
};

// ---- double-double sums ------------------------------------------------------------------------------------------------------
struct dd { double hi, lo; };
__device__ __forceinline__ void dd_add(dd &a, double x)
{
    const double s = a.hi + x, b = s - a.hi;
    a.lo += (a.hi - (s - b)) + (x - b);
    a.hi = s;
}
__device__ __forceinline__ void dd_merge(dd &a, const dd &o)
{
    dd_add(a, o.hi);
    a.lo += o.lo;
}
// the sum of v over the workgroup in lane, then wave order; every thread calls it and gets the result
__device__ __forceinline__ dd ps_block_sum(dd v)
{
    __shared__ double sh[2 * PS_WAVES];
    for (int o = 32; o > 0; o >>= 1) {
        dd other;
        other.hi = __shfl_down(v.hi, o);
        other.lo = __shfl_down(v.lo, o);
        dd_merge(v, other);
    }
    if ((threadIdx.x & 63) == 0) { sh[2 * (threadIdx.x >> 6)] = v.hi; sh[2 * (threadIdx.x >> 6) + 1] = v.lo; }
    __syncthreads();
    dd r = {sh[0], sh[1]};
    for (int q = 1; q < PS_WAVES; ++q) {
        dd o = {sh[2 * q], sh[2 * q + 1]};
        dd_merge(r, o);
    }
    __syncthreads();
    return r;
}

// ---- the line transform --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cmul(double2 a, double2 w) { return make_double2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }

// cos and sin of 2 pi m / P, m = 1 ... (P - 1) / 2, for P = 3, 5, 7
template <int P> __device__ __forceinline__ constexpr double root_cos(int m)
{
    return P == 3 ? -0.5
         : P == 5 ? (m == 1 ? 0.30901699437494742410 : -0.80901699437494742410)
                  : (m == 1 ? 0.62348980185873353053 : m == 2 ? -0.22252093395631440429 : -0.90096886790241912624);
}
template <int P> __device__ __forceinline__ constexpr double root_sin(int m)
{
    return P == 3 ? 0.86602540378443864676
         : P == 5 ? (m == 1 ? 0.95105651629515357212 : 0.58778525229247312917)
                  : (m == 1 ? 0.78183148246802980871 : m == 2 ? 0.97492791218182360702 : 0.43388373911755812048);
}

template <int P> __device__ __forceinline__ void butterfly(double2 (&a)[P])
{
    if constexpr (P == 2) {
        const double2 t = a[1];
        a[1] = csub(a[0], t);
        a[0] = cadd(a[0], t);
    } else if constexpr (P == 4) {
        const double2 t0 = cadd(a[0], a[2]), t1 = csub(a[0], a[2]), t2 = cadd(a[1], a[3]), t3 = csub(a[1], a[3]);
        a[0] = cadd(t0, t2);
        a[2] = csub(t0, t2);
        a[1] = make_double2(t1.x + t3.y, t1.y - t3.x);      // t1 - i t3
        a[3] = make_double2(t1.x - t3.y, t1.y + t3.x);      // t1 + i t3
    } else {
        // odd P: b_k, b_(P-k) = a_0 + sum_j cos(2 pi j k / P) (a_j + a_(P-j)) -/+ i sum_j sin(2 pi j k / P) (a_j - a_(P-j))
        constexpr int H = (P - 1) / 2;
        double2 u[H], v[H];
#pragma unroll
        for (int j = 1; j <= H; ++j) { u[j - 1] = cadd(a[j], a[P - j]); v[j - 1] = csub(a[j], a[P - j]); }
        const double2 a0 = a[0];
        double2 sum = a0;
#pragma unroll
        for (int j = 0; j < H; ++j) sum = cadd(sum, u[j]);
        a[0] = sum;
#pragma unroll
        for (int k = 1; k <= H; ++k) {
            double re = a0.x, im = a0.y, sr = 0.0, si = 0.0;
#pragma unroll
            for (int j = 1; j <= H; ++j) {
                const int m = (j * k) % P;
                const double c = m <= H ? root_cos<P>(m) : root_cos<P>(P - m);
                const double s = m <= H ? root_sin<P>(m) : -root_sin<P>(P - m);
                re += c * u[j - 1].x; im += c * u[j - 1].y;
                sr += s * v[j - 1].x; si += s * v[j - 1].y;
            }
            a[k] = make_double2(re + si, im - sr);
            a[P - k] = make_double2(re - si, im + sr);
        }
    }
}

// one Stockham stage of radix P over nl lines of length N (pitch apart) from x to y; s: the product of the radices before it
template <int P> __device__ __forceinline__ void stage_fixed(const double2 *x, double2 *y, const double2 *tw, int N, int pitch, int nl, int s)
{
    const int L = N / P;
    for (int w = threadIdx.x; w < nl * L; w += PS_THREADS) {
        const int t = w / L, idx = w - t * L, base = idx - idx % s;
        const double2 *xl = x + t * pitch;
        double2 *yl = y + t * pitch + (idx - base) + P * base;
        double2 a[P];
#pragma unroll
        for (int j = 0; j < P; ++j) a[j] = xl[idx + L * j];
        butterfly<P>(a);
        yl[0] = a[0];
#pragma unroll
        for (int k = 1; k < P; ++k) yl[s * k] = cmul(a[k], tw[base * k]);      // (base k < N)
    }
}

// the same for any radix p: one work item per output k of a butterfly, p multiply-adds each; tw[m N/p] = exp(-2 pi i m / p)
__device__ __forceinline__ void stage_generic(const double2 *x, double2 *y, const double2 *tw, int N, int pitch, int nl, int s, int p)
{
    const int L = N / p;
    for (int w = threadIdx.x; w < nl * N; w += PS_THREADS) {
        const int t = w / N, rem = w - t * N, k = rem / L, idx = rem - k * L, base = idx - idx % s;
        const double2 *xl = x + t * pitch + idx;
        double2 acc = xl[0];
        int m = 0;
        for (int j = 1; j < p; ++j) {
            m += k;
            m = m >= p ? m - p : m;                                           // (j k) mod p
            acc = cadd(acc, cmul(xl[L * j], tw[m * L]));
        }
        y[t * pitch + (idx - base) + p * base + s * k] = cmul(acc, tw[base * k]);
    }
}

// the transform of nl lines of length N, line t at a[t pitch ...]; b: a second buffer of the same size; tw: the N roots of unity.
// Every thread of the workgroup calls it; returns the buffer that holds the result (a or b), synchronised
__device__ __forceinline__ double2 *line_fft(double2 *a, double2 *b, const double2 *tw, const PsPlan &plan, int N, int pitch, int nl)
{
    int s = 1;
    for (int f = 0; f < plan.nf; ++f) {
        const int p = plan.radix[f];
        __syncthreads();
        switch (p) {
        case 2: stage_fixed<2>(a, b, tw, N, pitch, nl, s); break;
        case 3: stage_fixed<3>(a, b, tw, N, pitch, nl, s); break;
        case 4: stage_fixed<4>(a, b, tw, N, pitch, nl, s); break;
        case 5: stage_fixed<5>(a, b, tw, N, pitch, nl, s); break;
        case 7: stage_fixed<7>(a, b, tw, N, pitch, nl, s); break;
        default: stage_generic(a, b, tw, N, pitch, nl, s, p); break;
        }
        double2 *t = a; a = b; b = t;
        s *= p;
    }
    __syncthreads();
    return a;
}

// the dynamic LDS of the transform kernels: the roots of unity [N], then the two line buffers [T pitch] each
__device__ __forceinline__ void ps_lds_layout(double2 *lds, const double2 *__restrict__ twiddle, int N, int pitch, int T, double2 *&tw,
                                              double2 *&a, double2 *&b)
{
    tw = lds;
    a = lds + N;
    b = a + (size_t)T * pitch;
    for (int r = threadIdx.x; r < N; r += PS_THREADS) tw[r] = twiddle[r];
}

// g of a cell (the header's order of operations; nothing here may be contracted into a fused multiply-add)
__device__ __forceinline__ double ps_form(int kind, size_t c, const double *__restrict__ x, const double *__restrict__ n,
                                          const double *__restrict__ temp, double nbar, double scale, double t_gamma)
{
#pragma clang fp contract(off)
    switch (kind) {
    case ASORA_PS_XH: return x[c];
    case ASORA_PS_XHI: return 1.0 - x[c];
    case ASORA_PS_DENSITY: return n[c] / nbar;
    default: {
        const double g = (scale * (1.0 - x[c])) * (n[c] / nbar);
        return t_gamma > 0.0 ? g * (1.0 - t_gamma / temp[c]) : g;
    }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// lines per workgroup: the most of 16, 8 whose two buffers and roots fit 72 KiB of LDS (two workgroups per CU), else 4 (N > 271;
// 91 KiB at N = 645)
static int ps_tile(int N)
{
    for (int T : {16, 8})
        if (((size_t)2 * T * (N | 1) + N) * sizeof(double2) <= (size_t)72 * 1024) return T;
    return 4;
}

static PsPlan ps_plan(int N)
{
    PsPlan plan{};
    int n = N;
    auto take = [&plan](int n, int p) {
        while (n > 1 && n % p == 0) { plan.radix[plan.nf++] = p; n /= p; }
        return n;
    };
    for (int p : {4, 2, 3, 5, 7}) n = take(n, p);
    for (int p = 11; n > 1; p += 2) n = take(n, p);
    return plan;
}

// a host-side stopwatch of STAGES stages: events on the library's stream, only with ASORA_OPT_TIMING
template <int STAGES> struct StageStopwatch {
    bool on;
    hipStream_t stream;
    hipEvent_t ev[STAGES + 1] = {};
    int n = 0;
    StageStopwatch(bool on_, hipStream_t s) : on(on_), stream(s) {}
    ~StageStopwatch() { for (int q = 0; q <= STAGES; ++q) if (ev[q]) (void)hipEventDestroy(ev[q]); }
    int mark()
    {
        if (!on || n > STAGES) return 0;
        ASORA_HIP_TRY(hipEventCreate(&ev[n]));
        ASORA_HIP_TRY(hipEventRecord(ev[n], stream));
        ++n;
        return 0;
    }
    void read(double *ms) const
    {
        if (!on || n != STAGES + 1) return;
        for (int q = 0; q < STAGES; ++q) {
            float t = 0.0f;
            ms[q] = hipEventElapsedTime(&t, ev[q], ev[q + 1]) == hipSuccess ? (double)t : 0.0;
        }
    }
};

} // namespace asora
