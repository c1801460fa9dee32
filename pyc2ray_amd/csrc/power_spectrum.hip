// power_spectrum.hip -- the spherically averaged power spectrum of a field formed from the device grids, and the cross-spectrum of two
// (asora_power_spectrum): a batched FP64 real-to-complex 3-D Fourier transform and a shell binning, both
// written here; nothing but the HIP runtime is linked.  Stages on the library's stream, none of which writes to a grid:
//   a. mean density : ps_sum_kernel over ASORA_GRID_NDENS (a fixed grid of PS_RED_BLOCKS workgroups) and ps_final_kernel, for the
//                     kinds that divide by it;
//   b. along k      : ps_row_kernel, one workgroup per T rows (i, j): it forms g from the grids in registers, adds g and g^2 to its
//                     partial moments, stores the field if asked, transforms the T rows in LDS -- a complex transform with a zero
//                     imaginary part -- and stores n_z = 0 ... N/2 of each into the complex buffer [i][j][n_z];
//   c. along j, i   : ps_line_kernel, in place: one workgroup per tile of T adjacent columns of the contiguous index (n_z for the
//                     pass along j; (j, n_z) flattened for the pass along i) takes all N elements of the strided axis into LDS
//                     (every global access is a fragment of T complex doubles, 64 ... 256 bytes; the last tile of a row may be
//                     narrower), transforms the T lines and writes them back;
//   d. binning      : ps_bin_kernel, one workgroup per plane i: a wave takes 64 consecutive n_z of one row, along which the bin is
//                     non-decreasing, reduces each run of equal bins by a segmented scan in lane order, and the last lane of a run
//                     adds into the wave's own LDS histogram by plain read-modify-write; the waves' histograms are combined in wave
//                     order into the plane's partial row, and ps_bin_final_kernel adds the planes in plane order.
// The line transform (line_fft) is a mixed-radix Stockham autosort between two LDS buffers: a stage of radix p reads element
// idx + j N/p, j = 0 ... p - 1 -- contiguous in the work-item index -- and writes r + p (idx - r) + s k with the twiddle
// tw[(idx - r) k], r = idx mod s, s the product of the radices so far.  Radices 4, 2, 3, 5 and 7 have butterflies in registers, any
// other prime factor p a generic one of p multiply-adds per output (one work item per OUTPUT, so a prime N still fills the
// workgroup): N = 1 ... 645 all work, and the cost of a line grows with the sum of N's prime factors beyond 7 (N = 43 p, or prime,
// is slow).  tw[r] = exp(-2 pi i r / N), r = 0 ... N - 1, is tabulated once per mesh on the host in extended precision; no index
// beyond N - 1 is formed, no angle is multiplied, no recurrence is used.  Lines are stored with an odd pitch.
// Every floating-point sum is formed in an order fixed by (N, thresholds): per thread in index order, per wave by a shuffle tree,
// per workgroup in wave order, over workgroups in index order -- the mean density and the moments in double-double (two-sum), so
// that they are correct to the last bit or two whatever the order.  No floating-point atomic anywhere.
#include "asora_internal.hpp"

namespace asora {

constexpr int PS_THREADS = 256;
constexpr int PS_WAVES = PS_THREADS / 64;
constexpr int PS_RED_BLOCKS = 512;          // the workgroups of the mean-density sum: a constant, so that the order is the mesh's alone
constexpr int PS_MAX_FACTORS = 12;          // (2^12 > 645)
constexpr int PS_VALUES = 5;                // per bin: count, sum_k, sum_aa, sum_bb, sum_ab
constexpr int PS_COUNT = 0, PS_SUM_K = 1, PS_SUM_AA = 2, PS_SUM_BB = 3, PS_SUM_AB = 4;
// the result words (doubles; the counts are uint64 in the same 8 bytes): the bins, the moments of a and of b, the mean density
constexpr int PS_RES_MOMENTS = PS_VALUES * ASORA_BUBBLE_MAX_BINS, PS_RES_NBAR = PS_RES_MOMENTS + 4, PS_RES_WORDS = PS_RES_NBAR + 1;
constexpr int PS_HOST_WORDS = PS_RES_WORDS + (ASORA_BUBBLE_MAX_BINS + 2) / 2;     // the thresholds (uint32) behind the results

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

// partial[2 b], [2 b + 1] = the double-double sum of a[] over the cells of workgroup b (grid-stride; the grid is PS_RED_BLOCKS)
__global__ void __launch_bounds__(PS_THREADS) ps_sum_kernel(const double *__restrict__ a, size_t n, double *__restrict__ partial)
{
    dd s = {0.0, 0.0};
    const size_t stride = (size_t)gridDim.x * PS_THREADS;
    for (size_t c = (size_t)blockIdx.x * PS_THREADS + threadIdx.x; c < n; c += stride) dd_add(s, a[c]);
    s = ps_block_sum(s);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = s.hi; partial[2 * blockIdx.x + 1] = s.lo; }
}

// out[q] = (the sum over e < count of the double-double partial[(e ncomp + q) 2 ...]) / divisor, q < ncomp; ONE workgroup
__global__ void __launch_bounds__(PS_THREADS) ps_final_kernel(const double *__restrict__ partial, int count, int ncomp, double divisor,
                                                               double *__restrict__ out)
{
    for (int q = 0; q < ncomp; ++q) {
        dd s = {0.0, 0.0};
        for (int e = threadIdx.x; e < count; e += PS_THREADS) {
            const double *p = partial + ((size_t)e * ncomp + q) * 2;
            dd o = {p[0], p[1]};
            dd_merge(s, o);
        }
        s = ps_block_sum(s);
        if (threadIdx.x == 0) out[q] = (s.hi + s.lo) / divisor;
    }
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

// the dynamic LDS of the two transform kernels: the roots of unity [N], then the two line buffers [T pitch] each
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

// the pass along k: workgroup b forms and transforms the rows b T ... b T + T - 1 of the N^2 rows (i, j)
__global__ void __launch_bounds__(PS_THREADS) ps_row_kernel(int kind, const double *__restrict__ x, const double *__restrict__ n,
                                                             const double *__restrict__ temp, const double *__restrict__ nbar_dev,
                                                             double scale, double t_gamma, int N, int pitch, int T, PsPlan plan,
                                                             const double2 *__restrict__ twiddle, double2 *__restrict__ modes,
                                                             double *__restrict__ moment_partial, double *__restrict__ field)
{
    extern __shared__ double2 ps_lds[];
    double2 *tw, *a, *b;
    ps_lds_layout(ps_lds, twiddle, N, pitch, T, tw, a, b);
    const int NZ = N / 2 + 1;
    const size_t rows = (size_t)N * N, row0 = (size_t)blockIdx.x * T;
    const int nl = (int)(rows - row0 < (size_t)T ? rows - row0 : (size_t)T);
    const double nbar = nbar_dev ? *nbar_dev : 1.0;
    dd s1 = {0.0, 0.0}, s2 = {0.0, 0.0};
    for (int w = threadIdx.x; w < nl * N; w += PS_THREADS) {
        const int t = w / N, k = w - t * N;
        const size_t c = (row0 + t) * (size_t)N + k;
        const double g = ps_form(kind, c, x, n, temp, nbar, scale, t_gamma);
        a[t * pitch + k] = make_double2(g, 0.0);
        dd_add(s1, g);
        dd_add(s2, g * g);
        if (field) field[c] = g;
    }
    s1 = ps_block_sum(s1);
    s2 = ps_block_sum(s2);
    if (threadIdx.x == 0) {
        double *p = moment_partial + (size_t)blockIdx.x * 4;
        p[0] = s1.hi; p[1] = s1.lo; p[2] = s2.hi; p[3] = s2.lo;
    }
    const double2 *res = line_fft(a, b, tw, plan, N, pitch, nl);
    for (int w = threadIdx.x; w < nl * NZ; w += PS_THREADS) {
        const int t = w / NZ, kz = w - t * NZ;
        modes[(row0 + t) * (size_t)NZ + kz] = res[t * pitch + kz];
    }
}

// a strided pass, in place: the buffer is n_outer blocks, outer_stride apart, of N lines elements line_stride apart, each ncols
// contiguous columns wide; workgroup b takes the columns c0 ... c0 + width - 1 of one block, c0 a multiple of T, width <= T
__global__ void __launch_bounds__(PS_THREADS) ps_line_kernel(double2 *__restrict__ modes, int N, int pitch, int T, PsPlan plan,
                                                              const double2 *__restrict__ twiddle, size_t outer_stride, size_t line_stride,
                                                              size_t ncols, unsigned tiles)
{
    extern __shared__ double2 ps_lds[];
    double2 *tw, *a, *b;
    ps_lds_layout(ps_lds, twiddle, N, pitch, T, tw, a, b);
    const unsigned outer = blockIdx.x / tiles;
    const size_t c0 = (size_t)(blockIdx.x - outer * tiles) * T;
    const int width = (int)(ncols - c0 < (size_t)T ? ncols - c0 : (size_t)T);
    double2 *g = modes + outer * outer_stride + c0;
    for (int w = threadIdx.x; w < width * N; w += PS_THREADS) {
        const int e = w / width, t = w - e * width;
        a[t * pitch + e] = g[e * line_stride + t];
    }
    const double2 *res = line_fft(a, b, tw, plan, N, pitch, width);
    for (int w = threadIdx.x; w < width * N; w += PS_THREADS) {
        const int e = w / width, t = w - e * width;
        g[e * line_stride + t] = res[t * pitch + e];
    }
}

// ---- binning -------------------------------------------------------------------------------------------------------------------
// v summed over the lanes start ... lane of the caller's run, in the order of a Hillis-Steele scan
template <typename V> __device__ __forceinline__ V ps_run_scan(V v, int lane, int start)
{
    for (int d = 1; d < 64; d <<= 1) {
        const V up = __shfl_up(v, d);
        if (lane - d >= start) v += up;
    }
    return v;
}

// partial[(plane PS_VALUES + q) n_bins + b] = value q of bin b summed over the stored modes of plane i = blockIdx.x; dynamic LDS:
// PS_WAVES histograms [PS_VALUES][n_bins] of 8-byte words, then thresholds[n_bins + 1]
template <bool CROSS>
__global__ void __launch_bounds__(PS_THREADS) ps_bin_kernel(const double2 *__restrict__ A, const double2 *__restrict__ B, int N, int n_bins,
                                                             const unsigned *__restrict__ thresholds, double *__restrict__ partial)
{
    extern __shared__ double ps_hist[];
    unsigned *thr = (unsigned *)(ps_hist + (size_t)PS_WAVES * PS_VALUES * n_bins);
    for (int q = threadIdx.x; q < PS_WAVES * PS_VALUES * n_bins; q += PS_THREADS) ps_hist[q] = 0.0;      // (+0.0 is the integer 0 too)
    for (int q = threadIdx.x; q <= n_bins; q += PS_THREADS) thr[q] = thresholds[q];
    __syncthreads();
    const int NZ = N / 2 + 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = blockIdx.x;
    const unsigned mi = (unsigned)min(i, N - i);
    volatile double *hist = ps_hist + (size_t)wave * PS_VALUES * n_bins;
    volatile unsigned long long *hist_n = (volatile unsigned long long *)hist;
    for (int j = wave; j < N; j += PS_WAVES) {
        const unsigned mj = (unsigned)min(j, N - j), n2_ij = mi * mi + mj * mj;
        const double2 *ra = A + ((size_t)i * N + j) * NZ, *rb = CROSS ? B + ((size_t)i * N + j) * NZ : nullptr;
        for (int kz0 = 0; kz0 < NZ; kz0 += 64) {
            const int kz = kz0 + lane;
            const bool stored = kz < NZ;
            const unsigned n2 = n2_ij + (unsigned)(kz * kz);
            // the bin: (the first threshold above n2) - 1; -1 below the first edge, n_bins at or above the last and in the lanes
            // past the row's end -- non-decreasing along the lanes either way
            int bin = n_bins;
            if (stored) {
                int lo = 0, hi = n_bins + 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (thr[mid] <= n2) lo = mid + 1; else hi = mid;
                }
                bin = lo - 1;
            }
            double wgt = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
            if (stored) {
                wgt = (kz == 0 || 2 * kz == N) ? 1.0 : 2.0;
                const double2 za = ra[kz];
                aa = wgt * fma(za.x, za.x, za.y * za.y);
                if (CROSS) {
                    const double2 zb = rb[kz];
                    bb = wgt * fma(zb.x, zb.x, zb.y * zb.y);
                    ab = wgt * fma(za.x, zb.x, za.y * zb.y);
                }
            }
            const int before = __shfl_up(bin, 1);
            const unsigned long long heads = __ballot(lane == 0 || bin != before);
            const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
            const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
            const unsigned long long cnt = ps_run_scan((unsigned long long)wgt, lane, start);
            const double sk = ps_run_scan(wgt * sqrt((double)n2), lane, start);
            aa = ps_run_scan(aa, lane, start);
            if (CROSS) { bb = ps_run_scan(bb, lane, start); ab = ps_run_scan(ab, lane, start); }
            if (last && bin >= 0 && bin < n_bins) {               // (one lane per bin in this instruction: runs are maximal)
                hist_n[PS_COUNT * n_bins + bin] += cnt;
                hist[PS_SUM_K * n_bins + bin] += sk;
                hist[PS_SUM_AA * n_bins + bin] += aa;
                if (CROSS) { hist[PS_SUM_BB * n_bins + bin] += bb; hist[PS_SUM_AB * n_bins + bin] += ab; }
            }
        }
    }
    __syncthreads();
    const int nv = CROSS ? PS_VALUES : PS_SUM_AA + 1;
    for (int q = threadIdx.x; q < nv * n_bins; q += PS_THREADS) {
        double *out = partial + (size_t)i * PS_VALUES * n_bins + q;
        if (q < n_bins) {
            unsigned long long s = 0ull;
            for (int u = 0; u < PS_WAVES; ++u) s += ((const unsigned long long *)ps_hist)[(size_t)u * PS_VALUES * n_bins + q];
            *(unsigned long long *)out = s;
        } else {
            double s = ps_hist[q];
            for (int u = 1; u < PS_WAVES; ++u) s += ps_hist[(size_t)u * PS_VALUES * n_bins + q];
            *out = s;
        }
    }
}

// result[q ASORA_BUBBLE_MAX_BINS + b] = the planes' partial rows added in plane order, q < nv
__global__ void __launch_bounds__(PS_THREADS) ps_bin_final_kernel(const double *__restrict__ partial, int N, int n_bins, int nv,
                                                                   double *__restrict__ result)
{
    const int t = blockIdx.x * PS_THREADS + threadIdx.x;
    if (t >= nv * n_bins) return;
    const int q = t / n_bins, b = t - q * n_bins;
    double *out = result + q * ASORA_BUBBLE_MAX_BINS + b;
    if (q == PS_COUNT) {
        unsigned long long s = 0ull;
        for (int i = 0; i < N; ++i) s += ((const unsigned long long *)partial)[(size_t)i * PS_VALUES * n_bins + t];
        *(unsigned long long *)out = s;
    } else {
        double s = 0.0;
        for (int i = 0; i < N; ++i) s += partial[(size_t)i * PS_VALUES * n_bins + t];
        *out = s;
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

// the words of ps_partial: [bins: N PS_VALUES MAX_BINS | moments of a, of b: row workgroups x 4 each | mean density: 2 PS_RED_BLOCKS
// | results: PS_RES_WORDS]
struct PsLayout {
    size_t row_blocks, bins, moments[2], nbar, result, words;
    explicit PsLayout(int N, int T)
    {
        row_blocks = ((size_t)N * N + T - 1) / T;
        bins = 0;
        moments[0] = bins + (size_t)N * PS_VALUES * ASORA_BUBBLE_MAX_BINS;
        moments[1] = moments[0] + 4 * row_blocks;
        nbar = moments[1] + 4 * row_blocks;
        result = nbar + 2 * PS_RED_BLOCKS;
        words = result + PS_RES_WORDS;
    }
};

static int ensure_ps_buffers(State &st, const PsLayout &lay, bool cross)
{
    const int N = st.N;
    const size_t nmodes = (size_t)N * N * (N / 2 + 1);
    for (int f = 0; f < (cross ? 2 : 1); ++f)
        if (!st.ps_modes[f]) ASORA_HIP_TRY(hipMalloc(&st.ps_modes[f], sizeof(double2) * nmodes));
    if (!st.ps_partial) ASORA_HIP_TRY(hipMalloc(&st.ps_partial, sizeof(double) * lay.words));
    if (!st.ps_thresholds) ASORA_HIP_TRY(hipMalloc(&st.ps_thresholds, sizeof(unsigned) * (ASORA_BUBBLE_MAX_BINS + 1)));
    if (!st.ps_host) ASORA_HIP_TRY(hipHostMalloc(&st.ps_host, sizeof(double) * PS_HOST_WORDS));
    if (!st.ps_twiddle) {
        // exp(-2 pi i r / N) from the first octant's cos and sin in extended precision, so that the symmetries hold to the bit
        std::vector<double2> tw((size_t)N);
        const long double two_pi = 6.283185307179586476925286766559005768L;
        for (int r = 0; r < N; ++r) {
            // the angle 2 pi r / N folded into [0, pi/4] by exact integer arithmetic on eighths of a turn: 8 r = o N + rest
            const long o = (8L * r) / N, rest = 8L * r - o * N;                  // octant o = 0 ... 7, rest / (8 N) of a turn into it
            const bool odd = o & 1;
            const long double ang = two_pi * (long double)(odd ? N - rest : rest) / (8.0L * N);   // in [0, pi/4]
            const long double c = cosl(ang), s = sinl(ang);
            // cos and sin of the angle o pi/4 + (odd ? pi/4 - ang : ang)
            long double co, si;
            switch (o) {
            case 0: co = c; si = s; break;
            case 1: co = s; si = c; break;
            case 2: co = -s; si = c; break;
            case 3: co = -c; si = s; break;
            case 4: co = -c; si = -s; break;
            case 5: co = -s; si = -c; break;
            case 6: co = s; si = -c; break;
            default: co = c; si = -s; break;
            }
            tw[r] = make_double2((double)co, (double)(0.0L - si));
        }
        ASORA_HIP_TRY(hipMalloc(&st.ps_twiddle, sizeof(double2) * N));
        ASORA_HIP_TRY(hipMemcpy(st.ps_twiddle, tw.data(), sizeof(double2) * N, hipMemcpyHostToDevice));
    }
    return 0;
}

// a host-side stopwatch of the stages: events on the library's stream, only with ASORA_OPT_TIMING
struct PsStopwatch {
    bool on;
    hipStream_t stream;
    hipEvent_t ev[ASORA_PS_STAGES + 1] = {};
    int n = 0;
    PsStopwatch(bool on_, hipStream_t s) : on(on_), stream(s) {}
    ~PsStopwatch() { for (int q = 0; q <= ASORA_PS_STAGES; ++q) if (ev[q]) (void)hipEventDestroy(ev[q]); }
    int mark()
    {
        if (!on || n > ASORA_PS_STAGES) return 0;
        ASORA_HIP_TRY(hipEventCreate(&ev[n]));
        ASORA_HIP_TRY(hipEventRecord(ev[n], stream));
        ++n;
        return 0;
    }
    void read(double *ms) const
    {
        if (!on || n != ASORA_PS_STAGES + 1) return;
        for (int q = 0; q < ASORA_PS_STAGES; ++q) {
            float t = 0.0f;
            ms[q] = hipEventElapsedTime(&t, ev[q], ev[q + 1]) == hipSuccess ? (double)t : 0.0;
        }
    }
};

struct PsFieldCopy {                     // the formed field on the device, for field_out: freed when the call ends, however it ends
    double *dev = nullptr;
    ~PsFieldCopy() { (void)hipFree(dev); }
};

static bool ps_kind_uses(int kind, int grid, double t_gamma)
{
    switch (grid) {
    case ASORA_GRID_XH: return kind == ASORA_PS_XH || kind == ASORA_PS_XHI || kind == ASORA_PS_HI;
    case ASORA_GRID_NDENS: return kind == ASORA_PS_DENSITY || kind == ASORA_PS_HI;
    default: return kind == ASORA_PS_HI && t_gamma > 0.0;       // ASORA_GRID_TEMP
    }
}

} // namespace asora

using namespace asora;

extern "C" {

int asora_power_spectrum(int kind_a, int kind_b, double scale, double t_gamma, int n_bins, const unsigned *thresholds,
                         unsigned long long *count, double *sum_k, double *sum_aa, double *sum_bb, double *sum_ab, double *moments_a,
                         double *moments_b, double *field_out, double *modes_out)
{
    clear_error();
    if (int rc = require_init("power_spectrum")) return rc;
    const bool cross = kind_b != -1;
    if (kind_a < 0 || kind_a >= ASORA_PS_KINDS || (cross && (kind_b < 0 || kind_b >= ASORA_PS_KINDS)))
        return fail(3, "power_spectrum: a kind must be one of ASORA_PS_* (kind_b: or -1)");
    if (!std::isfinite(scale)) return fail(3, "power_spectrum: scale must be finite");
    if (!std::isfinite(t_gamma) || t_gamma < 0.0) return fail(3, "power_spectrum: t_gamma must be finite and >= 0");
    if (n_bins < 1 || n_bins > ASORA_BUBBLE_MAX_BINS)
        return fail(3, "power_spectrum: n_bins must be in [1, " + std::to_string(ASORA_BUBBLE_MAX_BINS) + "]");
    if (!thresholds || !count || !sum_k || !sum_aa || !moments_a || (cross && (!sum_bb || !sum_ab || !moments_b)))
        return fail(3, "power_spectrum: null thresholds or output pointer");
    if (thresholds[0] < 1u) return fail(3, "power_spectrum: thresholds[0] must be >= 1 (the mode n = 0 is never binned)");
    for (int b = 0; b < n_bins; ++b)
        if (thresholds[b + 1] < thresholds[b]) return fail(3, "power_spectrum: the thresholds must be non-decreasing");
    State &st = state();
    const int kinds[2] = {kind_a, cross ? kind_b : kind_a};
    bool need[3] = {false, false, false};
    const int grids[3] = {ASORA_GRID_XH, ASORA_GRID_NDENS, ASORA_GRID_TEMP};
    for (int q = 0; q < 3; ++q) {
        need[q] = ps_kind_uses(kinds[0], grids[q], t_gamma) || ps_kind_uses(kinds[1], grids[q], t_gamma);
        if (need[q] && (!st.grid[grids[q]] || !st.grid_valid[grids[q]]))
            return fail(4, "power_spectrum: grid " + std::to_string(grids[q]) + " holds no data");
    }
    if (st.N > ASORA_REGION_MAX_N)
        return fail(4, "power_spectrum: not built for N > " + std::to_string(ASORA_REGION_MAX_N) + " (a line and its roots must fit LDS)");

    const int N = st.N, NZ = N / 2 + 1, T = ps_tile(N), pitch = N | 1;
    const size_t ncell = st.ncell, nmodes = (size_t)N * N * NZ;
    const PsLayout lay(N, T);
    const PsPlan plan = ps_plan(N);
    if (int rc = ensure_ps_buffers(st, lay, cross)) return rc;
    PsFieldCopy field;
    if (field_out) ASORA_HIP_TRY(hipMalloc(&field.dev, sizeof(double) * ncell));

    const size_t fft_lds = ((size_t)2 * T * pitch + N) * sizeof(double2);
    const size_t bin_lds = (size_t)PS_WAVES * PS_VALUES * n_bins * sizeof(double) + sizeof(unsigned) * (n_bins + 1);
    ASORA_HIP_TRY(hipFuncSetAttribute((const void *)ps_row_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fft_lds));
    ASORA_HIP_TRY(hipFuncSetAttribute((const void *)ps_line_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fft_lds));

    double *part = st.ps_partial, *res = part + lay.result;
    unsigned *thr_host = (unsigned *)(st.ps_host + PS_RES_WORDS);
    std::memcpy(thr_host, thresholds, sizeof(unsigned) * (n_bins + 1));
    ASORA_HIP_TRY(hipMemcpyAsync(st.ps_thresholds, thr_host, sizeof(unsigned) * (n_bins + 1), hipMemcpyHostToDevice, st.stream));
    ASORA_HIP_TRY(hipMemsetAsync(res, 0, sizeof(double) * PS_RES_WORDS, st.stream));
    const dim3 block(PS_THREADS);
    PsStopwatch watch(st.opt[ASORA_OPT_TIMING] != 0, st.stream);

    if (int rc = watch.mark()) return rc;
    if (need[1]) {
        hipLaunchKernelGGL(ps_sum_kernel, dim3(PS_RED_BLOCKS), block, 0, st.stream, (const double *)st.grid[ASORA_GRID_NDENS], ncell, part + lay.nbar);
        ASORA_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(ps_final_kernel, dim3(1), block, 0, st.stream, (const double *)(part + lay.nbar), PS_RED_BLOCKS, 1, (double)ncell,
                           res + PS_RES_NBAR);
        ASORA_HIP_TRY(hipGetLastError());
    }
    if (int rc = watch.mark()) return rc;
    for (int f = 0; f < (cross ? 2 : 1); ++f) {
        hipLaunchKernelGGL(ps_row_kernel, dim3((unsigned)lay.row_blocks), block, fft_lds, st.stream, kinds[f],
                           (const double *)st.grid[ASORA_GRID_XH], (const double *)st.grid[ASORA_GRID_NDENS],
                           (const double *)st.grid[ASORA_GRID_TEMP], need[1] ? (const double *)(res + PS_RES_NBAR) : (const double *)nullptr,
                           scale, t_gamma, N, pitch, T, plan, (const double2 *)st.ps_twiddle, st.ps_modes[f], part + lay.moments[f],
                           f == 0 ? field.dev : (double *)nullptr);
        ASORA_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(ps_final_kernel, dim3(1), block, 0, st.stream, (const double *)(part + lay.moments[f]), (int)lay.row_blocks, 2, 1.0,
                           res + PS_RES_MOMENTS + 2 * f);
        ASORA_HIP_TRY(hipGetLastError());
    }
    if (int rc = watch.mark()) return rc;
    const unsigned tiles_j = (unsigned)((NZ + T - 1) / T), tiles_i = (unsigned)(((size_t)N * NZ + T - 1) / T);
    for (int f = 0; f < (cross ? 2 : 1); ++f) {        // along j: N blocks (the planes i) of N lines, NZ columns wide
        hipLaunchKernelGGL(ps_line_kernel, dim3((unsigned)N * tiles_j), block, fft_lds, st.stream, st.ps_modes[f], N, pitch, T, plan,
                           (const double2 *)st.ps_twiddle, (size_t)N * NZ, (size_t)NZ, (size_t)NZ, tiles_j);
        ASORA_HIP_TRY(hipGetLastError());
    }
    if (int rc = watch.mark()) return rc;
    for (int f = 0; f < (cross ? 2 : 1); ++f) {        // along i: one block of N lines, N NZ columns wide
        hipLaunchKernelGGL(ps_line_kernel, dim3(tiles_i), block, fft_lds, st.stream, st.ps_modes[f], N, pitch, T, plan,
                           (const double2 *)st.ps_twiddle, (size_t)0, (size_t)N * NZ, (size_t)N * NZ, tiles_i);
        ASORA_HIP_TRY(hipGetLastError());
    }
    if (int rc = watch.mark()) return rc;
    const int nv = cross ? PS_VALUES : PS_SUM_AA + 1;
    if (cross)
        hipLaunchKernelGGL(ps_bin_kernel<true>, dim3((unsigned)N), block, bin_lds, st.stream, (const double2 *)st.ps_modes[0],
                           (const double2 *)st.ps_modes[1], N, n_bins, (const unsigned *)st.ps_thresholds, part + lay.bins);
    else
        hipLaunchKernelGGL(ps_bin_kernel<false>, dim3((unsigned)N), block, bin_lds, st.stream, (const double2 *)st.ps_modes[0],
                           (const double2 *)nullptr, N, n_bins, (const unsigned *)st.ps_thresholds, part + lay.bins);
    ASORA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ps_bin_final_kernel, dim3((unsigned)((nv * n_bins + PS_THREADS - 1) / PS_THREADS)), block, 0, st.stream,
                       (const double *)(part + lay.bins), N, n_bins, nv, res);
    ASORA_HIP_TRY(hipGetLastError());
    if (int rc = watch.mark()) return rc;

    ASORA_HIP_TRY(hipMemcpyAsync(st.ps_host, res, sizeof(double) * PS_RES_WORDS, hipMemcpyDeviceToHost, st.stream));
    if (field_out) ASORA_HIP_TRY(hipMemcpyAsync(field_out, field.dev, sizeof(double) * ncell, hipMemcpyDeviceToHost, st.stream));
    if (modes_out) ASORA_HIP_TRY(hipMemcpyAsync(modes_out, st.ps_modes[0], sizeof(double2) * nmodes, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    watch.read(st.ps_ms);

    const double *h = st.ps_host;
    std::memcpy(count, h + PS_COUNT * ASORA_BUBBLE_MAX_BINS, sizeof(unsigned long long) * n_bins);
    std::memcpy(sum_k, h + PS_SUM_K * ASORA_BUBBLE_MAX_BINS, sizeof(double) * n_bins);
    std::memcpy(sum_aa, h + PS_SUM_AA * ASORA_BUBBLE_MAX_BINS, sizeof(double) * n_bins);
    std::memcpy(moments_a, h + PS_RES_MOMENTS, sizeof(double) * 2);
    if (cross) {
        std::memcpy(sum_bb, h + PS_SUM_BB * ASORA_BUBBLE_MAX_BINS, sizeof(double) * n_bins);
        std::memcpy(sum_ab, h + PS_SUM_AB * ASORA_BUBBLE_MAX_BINS, sizeof(double) * n_bins);
        std::memcpy(moments_b, h + PS_RES_MOMENTS + 2, sizeof(double) * 2);
    }
    return 0;
}

int asora_debug_power_spectrum_ms(double *ms)
{
    clear_error();
    if (!ms) return fail(3, "debug_power_spectrum_ms: null pointer");
    for (int q = 0; q < ASORA_PS_STAGES; ++q) ms[q] = state().ps_ms[q];
    return 0;
}

} // extern "C"
