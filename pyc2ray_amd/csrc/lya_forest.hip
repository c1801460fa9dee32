// lya_forest.hip -- the Lyman-alpha forest of the state on the device: optical depth and transmitted flux along every line of one
// axis, their one-point statistics and the dark gaps (asora_lyman_alpha_forest).  The line geometry -- the
// tiles, the displaced cell edges, the gather over the 2 W + 1 cells that can reach a pixel -- is the redshift-space mapping's
// (redshift_space.hip, rs_map_kernel); what is new is the weight, a cell's top hat between its edges convolved with its Doppler
// profile, two erf per term.  The stages:
//   r. reach      : lya_line_kernel<true>, only with window = 0: the lines are staged as below and max reach is reduced as the
//                   maximum of the bit patterns (reach > 0: an integer maximum, any order gives the same bits; an infinity or a NaN
//                   has a larger pattern than every finite value).  The host reads it back and takes W from it;
//   t. lines      : lya_line_kernel<false>, one workgroup per tile of T lines along los_axis: g, bt and u of the tile go into LDS,
//                   the edge displacements d are formed there, and every work item gathers one pixel over o = -W ... W ascending, in
//                   the order of the specification: consecutive work items own consecutive pixels, so the LDS reads of q = p - o are
//                   consecutive addresses across a wave.  lo and hi are formed from d[q] and d[q + 1] where they are used (two LDS
//                   reads either way, and one array less).  A term is skipped where the specification makes it exactly zero: g[q] ==
//                   0 and outside the cut at 6 bt.  tau is staged in LDS (in the place of u) and stored in the order of the loads
//                   with F = exp(-tau); a pixel with F < gap_threshold sets its bit in the line's mask words (an integer LDS atomic),
//                   and one work item per line walks the runs of its mask with count-trailing-zeros: O(words + runs).  Tiles are T
//                   contiguous rows for los_axis = 2 (48 KiB of LDS, 256 work items) and T adjacent columns of the contiguous index
//                   for the axes 0 and 1 (T = 16 up to N = 307, 8 up to N = 611, else 4; 1024 work items), as there.  Reads and
//                   writes of a workgroup touch its own lines only, and every read is behind a barrier before the first write: a
//                   destination may be a grid the call reads;
//   s. statistics : lya_stats_kernel, PS_RED_BLOCKS workgroups stride over tau: F = exp(-tau) (the same bits as the line kernel's),
//                   sum F and sum F^2 as double-double sums in lane, wave, workgroup order, min and max of tau, the non-finite count,
//                   and the PDF by a binary search over the edges into an LDS histogram of integers;
//   f. fold       : lya_fold_kernel, one workgroup: the partials of both kernels in workgroup order.
// Every floating-point sum has an order fixed by (N, los_axis); the only atomics are integer ones (counts, maxima of bit patterns).
#include "asora_internal.hpp"
#include "fft_device.hpp"

namespace asora {

constexpr int LYA_THREADS_ROWS = 256, LYA_THREADS_COLUMNS = 1024, LYA_MAX_WAVES = LYA_THREADS_COLUMNS / 64;
constexpr double LYA_FLOOR = 0.0009765625;       // 2^-10: the floor of bt and the width below which a cell is degenerate
// the result words on the device (uint64 each; the first four hold doubles), then gaps [ASORA_REGION_MAX_N + 1], then pdf
constexpr int LYA_R_SUM_F = 0, LYA_R_SUM_F2 = 1, LYA_R_TAU_MIN = 2, LYA_R_TAU_MAX = 3, LYA_R_NONFINITE = 4, LYA_R_DEGENERATE = 5,
              LYA_R_CLIPPED = 6, LYA_R_N_DARK = 7, LYA_R_N_GAPS = 8, LYA_R_LONGEST = 9, LYA_R_FULL_LINES = 10, LYA_R_REACH = 11,
              LYA_R_HEAD = 16;
constexpr int LYA_R_GAPS = LYA_R_HEAD, LYA_R_PDF = LYA_R_GAPS + ASORA_REGION_MAX_N + 1, LYA_R_WORDS = LYA_R_PDF + ASORA_LYA_MAX_BINS;
// what a workgroup of the line kernel leaves: degenerate, clipped, dark pixels, gaps, the longest gap, full lines
constexpr int LYA_B_DEGENERATE = 0, LYA_B_CLIPPED = 1, LYA_B_N_DARK = 2, LYA_B_N_GAPS = 3, LYA_B_LONGEST = 4, LYA_B_FULL_LINES = 5,
              LYA_B_WORDS = 8;
// ... and one of the statistics kernel: sum F (hi, lo), sum F^2 (hi, lo), min tau, max tau, the non-finite count
constexpr int LYA_S_WORDS = 8;

// how the lines of the mesh are dealt to the workgroups (rs_map_kernel's scheme): workgroup b takes `width` <= T lines; cell e of its
// line t is base + t t_stride + e e_stride
struct LyaTiles {
    int N, pitch, T, contiguous, mask_words;
    size_t outer_stride, line_stride, ncols;
    unsigned tiles, blocks;
    size_t lds;
};
struct LyaTile { size_t base, t_stride, e_stride; int width; };

__device__ __forceinline__ LyaTile lya_tile(const LyaTiles &geo)
{
    LyaTile tl;
    if (geo.contiguous) {
        const size_t rows = (size_t)geo.N * geo.N, row0 = (size_t)blockIdx.x * geo.T;
        tl.width = (int)(rows - row0 < (size_t)geo.T ? rows - row0 : (size_t)geo.T);
        tl.base = row0 * geo.N; tl.t_stride = (size_t)geo.N; tl.e_stride = 1;
    } else {
        const unsigned outer = blockIdx.x / geo.tiles;
        const size_t c0 = (size_t)(blockIdx.x - outer * geo.tiles) * geo.T;
        tl.width = (int)(geo.ncols - c0 < (size_t)geo.T ? geo.ncols - c0 : (size_t)geo.T);
        tl.base = outer * geo.outer_stride + c0; tl.t_stride = 1; tl.e_stride = geo.line_stride;
    }
    return tl;
}

// v over the workgroup with `op`, in lane, then wave order; every thread calls it and gets the result.  sh: [LYA_MAX_WAVES]
template <typename V, typename Op> __device__ __forceinline__ V lya_block_reduce(V v, Op op, V *sh)
{
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_down(v, o));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    V r = sh[0];
    for (int q = 1; q < (int)(blockDim.x >> 6); ++q) r = op(r, sh[q]);
    __syncthreads();
    return r;
}
struct LyaSum { __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a + b; } };
struct LyaMaxU { __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a > b ? a : b; } };
struct LyaMin { __device__ double operator()(double a, double b) const { return fmin(a, b); } };      // (fmin, fmax: a NaN loses)
struct LyaMax { __device__ double operator()(double a, double b) const { return fmax(a, b); } };

// the edges of cell q of a line relative to q, and its reach (the header's order of operations)
__device__ __forceinline__ void lya_edges(const double *d, int q, int N, double &lo, double &hi)
{
#pragma clang fp contract(off)
    const int q1 = q + 1 == N ? 0 : q + 1;
    const double a = d[q], b = 1.0 + d[q1];
    lo = b < a ? b : a;
    hi = b < a ? a : b;
}
__device__ __forceinline__ double lya_reach(double lo, double hi, double bt)
{
#pragma clang fp contract(off)
    const double r1 = (6.0 * bt - lo) + 0.5, r2 = (hi + 6.0 * bt) - 0.5;
    return r2 > r1 ? r2 : r1;
}

// REACH: result[LYA_R_REACH] = max over the cells of the bit pattern of reach (zeroed beforehand), nothing else is read or written.
// Else the optical depth of the header into tau, with flux != NULL F into flux, and the workgroup's counts into block_partial and
// result's gaps.  Dynamic LDS: G, BT, D, U [T pitch] doubles each, the mask [T mask_words] and the reduction's scratch
// [LYA_MAX_WAVES] (uint64), the histogram of gap lengths [N + 1] (unsigned).  x, n, temp, tau and flux may alias:
// no __restrict__ on them
template <bool REACH>
__global__ void __launch_bounds__(LYA_THREADS_COLUMNS) lya_line_kernel(LyaTiles geo, const double *x, const double *n, const double *temp,
                                                                       const double *__restrict__ v, double vscale, double b_scale,
                                                                       double tau_scale, int W, double gap_threshold, double *tau,
                                                                       double *flux, unsigned long long *__restrict__ block_partial,
                                                                       unsigned long long *__restrict__ result)
{
    extern __shared__ double lya_lds[];
    const int N = geo.N, pitch = geo.pitch, T = geo.T, MW = geo.mask_words, threads = blockDim.x;
    double *G = lya_lds, *BT = G + (size_t)T * pitch, *D = BT + (size_t)T * pitch, *U = D + (size_t)T * pitch;
    unsigned long long *mask = (unsigned long long *)(U + (size_t)T * pitch), *red = mask + (size_t)T * MW;
    unsigned *hist = (unsigned *)(red + LYA_MAX_WAVES);
    const LyaTile tl = lya_tile(geo);
    const int items = tl.width * N;
    if (!REACH) {
        for (int q = threadIdx.x; q < T * MW; q += threads) mask[q] = 0ull;
        for (int q = threadIdx.x; q <= N; q += threads) hist[q] = 0u;
    }
    for (int w = threadIdx.x; w < items; w += threads) {
#pragma clang fp contract(off)
        int t, e;
        if (geo.contiguous) { t = w / N; e = w - t * N; } else { e = w / tl.width; t = w - e * tl.width; }
        const size_t c = tl.base + t * tl.t_stride + e * tl.e_stride;
        if (!REACH) G[t * pitch + e] = tau_scale * ((1.0 - x[c]) * n[c]);
        const double bt = b_scale * sqrt(temp[c]);
        BT[t * pitch + e] = bt > LYA_FLOOR ? bt : LYA_FLOOR;        // (a NaN, the root of a negative temperature, takes the floor)
        U[t * pitch + e] = v ? v[c] * vscale : 0.0;
    }
    __syncthreads();
    for (int w = threadIdx.x; w < items; w += threads) {
#pragma clang fp contract(off)
        const int t = w / N, q = w - t * N, qm = q == 0 ? N - 1 : q - 1;
        D[t * pitch + q] = 0.5 * (U[t * pitch + qm] + U[t * pitch + q]);
    }
    __syncthreads();
    // every cell's reach: the largest (REACH), or how many reach beyond W and how many are degenerate
    unsigned long long reach_bits = 0ull, degenerate = 0ull, clipped = 0ull;
    for (int w = threadIdx.x; w < items; w += threads) {
#pragma clang fp contract(off)
        const int t = w / N, q = w - t * N;
        double lo, hi;
        lya_edges(D + t * pitch, q, N, lo, hi);
        const double r = lya_reach(lo, hi, BT[t * pitch + q]);
        if (REACH) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(r) & 0x7FFFFFFFFFFFFFFFull;
            reach_bits = b > reach_bits ? b : reach_bits;
        } else {
            degenerate += hi - lo < LYA_FLOOR ? 1ull : 0ull;
            clipped += ceil(r) > (double)W ? 1ull : 0ull;
        }
    }
    if (REACH) {
        reach_bits = lya_block_reduce(reach_bits, LyaMaxU(), red);
        if (threadIdx.x == 0 && reach_bits) atomicMax(result + LYA_R_REACH, reach_bits);
        return;
    }
    for (int w = threadIdx.x; w < items; w += threads) {
#pragma clang fp contract(off)
        const int t = w / N, p = w - t * N;
        const double *g = G + t * pitch, *d = D + t * pitch, *btl = BT + t * pitch;
        double sum = 0.0;
        for (int o = -W; o <= W; ++o) {                            // (2 W + 1 <= N: q stays within one period of p)
            int q = p - o;
            q = q < 0 ? q + N : q;
            q = q >= N ? q - N : q;
            const double gq = g[q];
            if (gq == 0.0) continue;                               // (w is finite and >= 0: the term is a zero, and sum + 0 = sum)
            double lo, hi;
            lya_edges(d, q, N, lo, hi);
            const double bt = btl[q], wd = hi - lo, s = (double)o + 0.5;
            double wgt;
            if (wd >= LYA_FLOOR) {
                if ((s - hi) > 6.0 * bt || (lo - s) > 6.0 * bt) continue;
                wgt = 0.5 * (erf((s - lo) / bt) - erf((s - hi) / bt)) / wd;
            } else {
                const double c = 0.5 * (lo + hi), tt = (s - c) / bt;
                if (fabs(tt) > 6.0) continue;
                wgt = (0.5641895835477563 / bt) * exp(-(tt * tt));
            }
            sum = sum + wgt * gq;
        }
        U[t * pitch + p] = sum;                                    // (u is dead: d holds what the gather needs of it)
        if (exp(-sum) < gap_threshold) atomicOr(mask + (size_t)t * MW + (p >> 6), 1ull << (p & 63));
    }
    __syncthreads();
    for (int w = threadIdx.x; w < items; w += threads) {
        int t, e;
        if (geo.contiguous) { t = w / N; e = w - t * N; } else { e = w / tl.width; t = w - e * tl.width; }
        const size_t c = tl.base + t * tl.t_stride + e * tl.e_stride;
        const double tv = U[t * pitch + e];
        tau[c] = tv;
        if (flux) flux[c] = exp(-tv);
    }
    // the gaps of line t = threadIdx.x: the maximal runs of set bits of its mask, the run through the end joined to the one at 0
    unsigned long long n_dark = 0ull, n_gaps = 0ull, longest = 0ull, full = 0ull;
    if ((int)threadIdx.x < tl.width) {
        const unsigned long long *m = mask + (size_t)threadIdx.x * MW;
        for (int q = 0; q < MW; ++q) n_dark += (unsigned long long)__popcll(m[q]);
        if (n_dark == (unsigned long long)N) {
            n_gaps = 1ull; longest = (unsigned long long)N; full = 1ull;
            atomicAdd(hist + N, 1u);
        } else if (n_dark) {
            int pos = 0, first = 0;                                // first: the length of a run that starts at pixel 0
            while (pos < N) {
                // the first set bit at or behind pos, then the first clear bit behind it (the pad bits of the last word are clear)
                int wq = pos >> 6;
                unsigned long long bits = m[wq] & (~0ull << (pos & 63));
                while (!bits && ++wq < MW) bits = m[wq];
                if (!bits) break;
                const int start = (wq << 6) + __ffsll((long long)bits) - 1;
                wq = start >> 6;
                bits = ~m[wq] & (~0ull << (start & 63));
                while (!bits && ++wq < MW) bits = ~m[wq];
                int end = bits ? (wq << 6) + __ffsll((long long)bits) - 1 : N;
                end = end > N ? N : end;
                int len = end - start;
                pos = end;
                if (start == 0) { first = len; continue; }         // (recorded with the run through the end, or alone behind the loop)
                if (end == N) { len += first; first = 0; }
                atomicAdd(hist + len, 1u);
                n_gaps += 1ull;
                longest = (unsigned long long)len > longest ? (unsigned long long)len : longest;
            }
            if (first) {
                atomicAdd(hist + first, 1u);
                n_gaps += 1ull;
                longest = (unsigned long long)first > longest ? (unsigned long long)first : longest;
            }
        }
    }
    degenerate = lya_block_reduce(degenerate, LyaSum(), red);
    clipped = lya_block_reduce(clipped, LyaSum(), red);
    n_dark = lya_block_reduce(n_dark, LyaSum(), red);
    n_gaps = lya_block_reduce(n_gaps, LyaSum(), red);
    longest = lya_block_reduce(longest, LyaMaxU(), red);
    full = lya_block_reduce(full, LyaSum(), red);                  // (its barriers also put hist behind the gap pass)
    if (threadIdx.x == 0) {
        unsigned long long *p = block_partial + (size_t)blockIdx.x * LYA_B_WORDS;
        p[LYA_B_DEGENERATE] = degenerate; p[LYA_B_CLIPPED] = clipped; p[LYA_B_N_DARK] = n_dark; p[LYA_B_N_GAPS] = n_gaps;
        p[LYA_B_LONGEST] = longest; p[LYA_B_FULL_LINES] = full;
    }
    for (int q = threadIdx.x; q <= N; q += threads)
        if (hist[q]) atomicAdd(result + LYA_R_GAPS + q, (unsigned long long)hist[q]);
}

// the statistics of tau [ncell]: workgroup b leaves stat_partial[b LYA_S_WORDS ...] and adds its histogram of F into result's pdf
__global__ void __launch_bounds__(PS_THREADS) lya_stats_kernel(const double *__restrict__ tau, size_t ncell, int n_bins,
                                                               const double *__restrict__ edges, double *__restrict__ stat_partial,
                                                               unsigned long long *__restrict__ result)
{
    __shared__ double sh_edges[ASORA_LYA_MAX_BINS + 1];
    __shared__ unsigned sh_hist[ASORA_LYA_MAX_BINS];
    __shared__ double sh_d[LYA_MAX_WAVES];
    __shared__ unsigned long long sh_u[LYA_MAX_WAVES];
    for (int q = threadIdx.x; q < n_bins; q += PS_THREADS) sh_hist[q] = 0u;
    for (int q = threadIdx.x; q <= n_bins && n_bins; q += PS_THREADS) sh_edges[q] = edges[q];
    __syncthreads();
    dd s1 = {0.0, 0.0}, s2 = {0.0, 0.0};
    double lo = INFINITY, hi = -INFINITY;
    unsigned long long nonfinite = 0ull;
    const size_t stride = (size_t)gridDim.x * PS_THREADS;
    for (size_t c = (size_t)blockIdx.x * PS_THREADS + threadIdx.x; c < ncell; c += stride) {
#pragma clang fp contract(off)
        const double t = tau[c], f = exp(-t);
        dd_add(s1, f);
        dd_add(s2, f * f);
        lo = fmin(lo, t);
        hi = fmax(hi, t);
        nonfinite += isfinite(t) ? 0ull : 1ull;
        if (n_bins) {                                              // (the edges at or below F) - 1
            int a = 0, b = n_bins + 1;
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (sh_edges[mid] <= f) a = mid + 1; else b = mid;
            }
            if (a >= 1 && a <= n_bins) atomicAdd(sh_hist + (a - 1), 1u);
        }
    }
    s1 = ps_block_sum(s1);
    s2 = ps_block_sum(s2);
    lo = lya_block_reduce(lo, LyaMin(), sh_d);
    hi = lya_block_reduce(hi, LyaMax(), sh_d);
    nonfinite = lya_block_reduce(nonfinite, LyaSum(), sh_u);
    if (threadIdx.x == 0) {
        double *p = stat_partial + (size_t)blockIdx.x * LYA_S_WORDS;
        p[0] = s1.hi; p[1] = s1.lo; p[2] = s2.hi; p[3] = s2.lo; p[4] = lo; p[5] = hi;
        ((unsigned long long *)p)[6] = nonfinite;
    }
    for (int q = threadIdx.x; q < n_bins; q += PS_THREADS)
        if (sh_hist[q]) atomicAdd(result + LYA_R_PDF + q, (unsigned long long)sh_hist[q]);
}

// the partials of the two kernels in workgroup order into the result words; ONE workgroup
__global__ void __launch_bounds__(PS_THREADS) lya_fold_kernel(const double *__restrict__ stat_partial, int stat_count,
                                                              const unsigned long long *__restrict__ block_partial, unsigned block_count,
                                                              unsigned long long *__restrict__ result)
{
    __shared__ double sh_d[LYA_MAX_WAVES];
    __shared__ unsigned long long sh_u[LYA_MAX_WAVES];
    for (int q = 0; q < 2; ++q) {
        dd s = {0.0, 0.0};
        for (int e = threadIdx.x; e < stat_count; e += PS_THREADS) {
            const double *p = stat_partial + (size_t)e * LYA_S_WORDS + 2 * q;
            dd o = {p[0], p[1]};
            dd_merge(s, o);
        }
        s = ps_block_sum(s);
        if (threadIdx.x == 0) result[q == 0 ? LYA_R_SUM_F : LYA_R_SUM_F2] =(unsigned long long)__double_as_longlong(s.hi + s.lo);
    }
    double lo = INFINITY, hi = -INFINITY;
    unsigned long long nonfinite = 0ull;
    for (int e = threadIdx.x; e < stat_count; e += PS_THREADS) {
        const double *p = stat_partial + (size_t)e * LYA_S_WORDS;
        lo = fmin(lo, p[4]);
        hi = fmax(hi, p[5]);
        nonfinite += ((const unsigned long long *)p)[6];
    }
    lo = lya_block_reduce(lo, LyaMin(), sh_d);
    hi = lya_block_reduce(hi, LyaMax(), sh_d);
    nonfinite = lya_block_reduce(nonfinite, LyaSum(), sh_u);
    unsigned long long sums[LYA_B_WORDS] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    for (unsigned e = threadIdx.x; e < block_count; e += PS_THREADS) {
        const unsigned long long *p = block_partial + (size_t)e * LYA_B_WORDS;
        for (int q = 0; q < LYA_B_WORDS; ++q)
            sums[q] = q == LYA_B_LONGEST ? (p[q] > sums[q] ? p[q] : sums[q]) : sums[q] + p[q];
    }
    for (int q = 0; q < LYA_B_WORDS; ++q)
        sums[q] = q == LYA_B_LONGEST ? lya_block_reduce(sums[q], LyaMaxU(), sh_u) : lya_block_reduce(sums[q], LyaSum(), sh_u);
    if (threadIdx.x == 0) {
        result[LYA_R_TAU_MIN] = (unsigned long long)__double_as_longlong(lo);
        result[LYA_R_TAU_MAX] = (unsigned long long)__double_as_longlong(hi);
        result[LYA_R_NONFINITE] = nonfinite;
        result[LYA_R_DEGENERATE] = sums[LYA_B_DEGENERATE]; result[LYA_R_CLIPPED] = sums[LYA_B_CLIPPED];
        result[LYA_R_N_DARK] = sums[LYA_B_N_DARK]; result[LYA_R_N_GAPS] = sums[LYA_B_N_GAPS];
        result[LYA_R_LONGEST] = sums[LYA_B_LONGEST]; result[LYA_R_FULL_LINES] = sums[LYA_B_FULL_LINES];
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// the tiles of a mesh along los_axis: rows of los_axis 2 to 48 KiB of LDS (three workgroups per CU; 128 rows at the most); columns
// of the other axes 16, 8 or 4, the most whose four lines per column fit 156 KiB
static LyaTiles lya_tiles(int N, int los_axis)
{
    LyaTiles g{};
    g.N = N; g.pitch = N | 1; g.contiguous = los_axis == 2 ? 1 : 0; g.mask_words = (N + 63) / 64;
    const size_t line = 4 * (size_t)g.pitch * sizeof(double) + (size_t)g.mask_words * sizeof(unsigned long long);
    const size_t fixed = (size_t)LYA_MAX_WAVES * sizeof(unsigned long long) + (size_t)(N + 1) * sizeof(unsigned);
    if (g.contiguous)
        g.T = (int)std::max<size_t>(1, std::min<size_t>(128, ((size_t)48 * 1024 - fixed) / line));
    else
        g.T = 16 * line + fixed <= (size_t)156 * 1024 ? 16 : 8 * line + fixed <= (size_t)156 * 1024 ? 8 : 4;
    g.lds = (size_t)g.T * line + fixed;
    const size_t n2 = (size_t)N * N;
    g.outer_stride = 0; g.line_stride = 1; g.ncols = n2;
    if (g.contiguous) {
        g.tiles = (unsigned)((n2 + g.T - 1) / g.T); g.blocks = g.tiles;
    } else if (los_axis == 1) {
        g.outer_stride = n2; g.line_stride = (size_t)N; g.ncols = (size_t)N;
        g.tiles = (unsigned)((N + g.T - 1) / g.T); g.blocks = (unsigned)N * g.tiles;
    } else {
        g.line_stride = n2;
        g.tiles = (unsigned)((n2 + g.T - 1) / g.T); g.blocks = g.tiles;
    }
    return g;
}

// the two forms of the line kernel may take `lds` bytes of dynamic LDS on `device`: asked for when either changes (a new mesh,
// another axis), not per call
static int lya_allow_lds(int device, size_t lds)
{
    static size_t allowed = 0;
    static int allowed_on = -1;
    if (lds == allowed && device == allowed_on) return 0;
    ASORA_HIP_TRY(hipFuncSetAttribute((const void *)lya_line_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ASORA_HIP_TRY(hipFuncSetAttribute((const void *)lya_line_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    allowed = lds; allowed_on = device;
    return 0;
}

} // namespace asora

using namespace asora;

extern "C" {

int asora_lyman_alpha_forest(int los_axis, int use_velocity, double velocity_scale, double b_scale, double tau_scale, int window,
                             double gap_threshold, int n_bins, const double *edges, int dst_grid, int dst_what, double *stats,
                             unsigned long long *counts, unsigned long long *pdf, unsigned long long *gaps, double *tau_out,
                             double *flux_out)
{
    clear_error();
    if (int rc = require_init("lyman_alpha_forest")) return rc;
    State &st = state();
    const std::string me("lyman_alpha_forest");
    if (los_axis < 0 || los_axis > 2) return fail(3, me + ": los_axis must be 0, 1 or 2");
    if (!std::isfinite(b_scale) || !(b_scale > 0.0)) return fail(3, me + ": b_scale must be finite and > 0");
    if (!std::isfinite(tau_scale) || !(tau_scale > 0.0)) return fail(3, me + ": tau_scale must be finite and > 0");
    if (use_velocity) {
        if (!std::isfinite(velocity_scale)) return fail(3, me + ": velocity_scale must be finite");
        if (!st.redshift.velocity) return fail(3, me + ": use_velocity without a velocity on the device (asora_los_velocity_to_device)");
    }
    if (!std::isfinite(gap_threshold)) return fail(3, me + ": gap_threshold must be finite");
    if (n_bins < 0 || n_bins > ASORA_LYA_MAX_BINS) return fail(3, me + ": n_bins must be 0 ... " + std::to_string(ASORA_LYA_MAX_BINS));
    if (n_bins > 0) {
        if (!edges || !pdf) return fail(3, me + ": n_bins > 0 needs edges and pdf");
        for (int b = 0; b <= n_bins; ++b)
            if (!std::isfinite(edges[b]) || (b > 0 && edges[b] < edges[b - 1])) return fail(3, me + ": edges must be finite and non-decreasing");
    }
    if (!stats || !counts || !gaps) return fail(3, me + ": null output pointer (stats, counts, gaps)");
    if (dst_grid < -1 || dst_grid >= ASORA_GRID_COUNT) return fail(3, me + ": dst_grid must be -1 or a grid selector");
    if (dst_grid >= 0 && dst_what != ASORA_LYA_FLUX && dst_what != ASORA_LYA_TAU) return fail(3, me + ": dst_what must be ASORA_LYA_FLUX or ASORA_LYA_TAU");
    if (window < 0) return fail(3, me + ": window must be >= 0");
    if (window > 0 && 2LL * window + 1 > (long long)st.N)
        return fail(3, me + ": the window of 2 W + 1 = " + std::to_string(2LL * window + 1) + " cells is wider than the N = " +
                           std::to_string(st.N) + " cells of a line");
    if (int rc = require_grids("lyman_alpha_forest", {ASORA_GRID_XH, ASORA_GRID_NDENS, ASORA_GRID_TEMP})) return rc;
    if (st.N > ASORA_REGION_MAX_N)
        return fail(4, me + ": not built for N > " + std::to_string(ASORA_REGION_MAX_N) + " (the lines of a tile must fit LDS)");

    const int N = st.N;
    const LyaTiles geo = lya_tiles(N, los_axis);
    const bool tau_to_grid = dst_grid >= 0 && dst_what == ASORA_LYA_TAU, flux_to_grid = dst_grid >= 0 && dst_what == ASORA_LYA_FLUX;
    if (!tau_to_grid) { if (int rc = st.smoothing.field.allocate(st.ncell)) return rc; }
    if (flux_out && !flux_to_grid) { if (int rc = st.lyman.flux.allocate(st.ncell)) return rc; }
    if (int rc = st.lyman.result.allocate(LYA_R_WORDS)) return rc;
    if (int rc = st.lyman.edges.allocate(ASORA_LYA_MAX_BINS + 1)) return rc;
    if (int rc = st.lyman.stat_partial.allocate((size_t)PS_RED_BLOCKS * LYA_S_WORDS)) return rc;
    if (int rc = st.lyman.block_partial.reserve((size_t)geo.blocks * LYA_B_WORDS, st.stream)) return rc;
    if (int rc = st.lyman.host.allocate(LYA_R_WORDS + ASORA_LYA_MAX_BINS + 1)) return rc;
    if (dst_grid >= 0)
        if (int rc = ensure_optional_grid(dst_grid)) return rc;
    double *tau_dev = tau_to_grid ? st.grid[dst_grid] : (double *)st.smoothing.field;
    double *flux_dev = flux_to_grid ? st.grid[dst_grid] : flux_out ? (double *)st.lyman.flux : (double *)nullptr;
    unsigned long long *res = st.lyman.result, *host = st.lyman.host;
    const double *v = use_velocity ? (const double *)st.redshift.velocity : (const double *)nullptr;
    const double *x = st.grid[ASORA_GRID_XH], *n = st.grid[ASORA_GRID_NDENS], *temp = st.grid[ASORA_GRID_TEMP];
    const dim3 threads(geo.contiguous ? LYA_THREADS_ROWS : LYA_THREADS_COLUMNS);

    ASORA_HIP_TRY(hipMemsetAsync(res, 0, sizeof(unsigned long long) * LYA_R_WORDS, st.stream));
    if (n_bins > 0) {
        double *stage = (double *)(host + LYA_R_WORDS);
        std::memcpy(stage, edges, sizeof(double) * (n_bins + 1));
        ASORA_HIP_TRY(hipMemcpyAsync(st.lyman.edges, stage, sizeof(double) * (n_bins + 1), hipMemcpyHostToDevice, st.stream));
    }
    if (int rc = lya_allow_lds(st.device, geo.lds)) return rc;
    StageStopwatch<ASORA_LYA_STAGES> watch(st.opt[ASORA_OPT_TIMING] != 0, st.stream);
    if (int rc = watch.mark()) return rc;
    int W = window;
    if (window == 0) {
        hipLaunchKernelGGL(lya_line_kernel<true>, dim3(geo.blocks), threads, geo.lds, st.stream, geo, x, n, temp, v, velocity_scale, b_scale,
                           tau_scale, 0, gap_threshold, (double *)nullptr, (double *)nullptr, (unsigned long long *)nullptr, res);
        ASORA_HIP_TRY(hipGetLastError());
        ASORA_HIP_TRY(hipMemcpyAsync(host + LYA_R_REACH, res + LYA_R_REACH, sizeof(unsigned long long), hipMemcpyDeviceToHost, st.stream));
        ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
        double reach;
        std::memcpy(&reach, host + LYA_R_REACH, sizeof reach);
        const int cap = (N - 1) / 2;
        const double need = std::ceil(reach);
        W = !(need <= (double)cap) ? cap : std::max(1, (int)need);      // (an infinite or NaN reach: the whole line)
        W = std::min(W, cap);
    }
    if (int rc = watch.mark()) return rc;
    hipLaunchKernelGGL(lya_line_kernel<false>, dim3(geo.blocks), threads, geo.lds, st.stream, geo, x, n, temp, v, velocity_scale, b_scale,
                       tau_scale, W, gap_threshold, tau_dev, flux_dev, (unsigned long long *)st.lyman.block_partial, res);
    ASORA_HIP_TRY(hipGetLastError());
    if (dst_grid >= 0) {                                           // (as asora_grid_to_device leaves a grid)
        st.grid_valid[dst_grid] = true;
        st.zero.verdict.since_probe = std::max(st.zero.verdict.since_probe, 48);
        if (dst_grid == ASORA_GRID_TEMP) st.temp_probe.valid = false;
    }
    if (int rc = watch.mark()) return rc;
    hipLaunchKernelGGL(lya_stats_kernel, dim3(PS_RED_BLOCKS), dim3(PS_THREADS), 0, st.stream, (const double *)tau_dev, st.ncell, n_bins,
                       (const double *)st.lyman.edges, (double *)st.lyman.stat_partial, res);
    ASORA_HIP_TRY(hipGetLastError());
    if (int rc = watch.mark()) return rc;
    hipLaunchKernelGGL(lya_fold_kernel, dim3(1), dim3(PS_THREADS), 0, st.stream, (const double *)st.lyman.stat_partial, PS_RED_BLOCKS,
                       (const unsigned long long *)st.lyman.block_partial, geo.blocks, res);
    ASORA_HIP_TRY(hipGetLastError());
    if (int rc = watch.mark()) return rc;
    ASORA_HIP_TRY(hipMemcpyAsync(host, res, sizeof(unsigned long long) * LYA_R_WORDS, hipMemcpyDeviceToHost, st.stream));
    if (tau_out) ASORA_HIP_TRY(hipMemcpyAsync(tau_out, tau_dev, sizeof(double) * st.ncell, hipMemcpyDeviceToHost, st.stream));
    if (flux_out) ASORA_HIP_TRY(hipMemcpyAsync(flux_out, flux_dev, sizeof(double) * st.ncell, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    watch.read(st.lyman.ms);

    std::memcpy(stats, host + LYA_R_SUM_F, sizeof(double) * ASORA_LYA_STATS);
    counts[ASORA_LYA_NONFINITE] = host[LYA_R_NONFINITE];
    counts[ASORA_LYA_WINDOW] = (unsigned long long)W;
    counts[ASORA_LYA_CLIPPED] = host[LYA_R_CLIPPED];
    counts[ASORA_LYA_DEGENERATE] = host[LYA_R_DEGENERATE];
    counts[ASORA_LYA_N_DARK] = host[LYA_R_N_DARK];
    counts[ASORA_LYA_N_GAPS] = host[LYA_R_N_GAPS];
    counts[ASORA_LYA_LONGEST] = host[LYA_R_LONGEST];
    counts[ASORA_LYA_FULL_LINES] = host[LYA_R_FULL_LINES];
    std::memcpy(gaps, host + LYA_R_GAPS, sizeof(unsigned long long) * (N + 1));
    if (n_bins > 0) std::memcpy(pdf, host + LYA_R_PDF, sizeof(unsigned long long) * n_bins);
    return 0;
}

int asora_debug_lya_forest_tiles(int N, int los_axis, int *tiles)
{
    clear_error();
    if (!tiles) return fail(3, "debug_lya_forest_tiles: null pointer");
    if (N < 1 || N > ASORA_REGION_MAX_N || los_axis < 0 || los_axis > 2)
        return fail(3, "debug_lya_forest_tiles: N must be 1 ... " + std::to_string(ASORA_REGION_MAX_N) + " and los_axis 0, 1 or 2");
    const LyaTiles geo = lya_tiles(N, los_axis);
    tiles[0] = geo.T;
    tiles[1] = geo.contiguous ? LYA_THREADS_ROWS : LYA_THREADS_COLUMNS;
    tiles[2] = (int)geo.blocks;
    tiles[3] = (int)geo.lds;
    return 0;
}

int asora_debug_lya_forest_ms(double *ms)
{
    clear_error();
    if (!ms) return fail(3, "debug_lya_forest_ms: null pointer");
    for (int q = 0; q < ASORA_LYA_STAGES; ++q) ms[q] = state().lyman.ms[q];
    return 0;
}

} // extern "C"
