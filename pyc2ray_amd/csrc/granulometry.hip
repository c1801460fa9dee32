// granulometry.hip -- the exact squared Euclidean distance transform of the in-phase cells of a device grid, and the numbers of cells
// that survive an erosion and an opening by digital balls of growing radius (asora_granulometry).  All
// integers.  Stages on the library's stream, none of which writes to a grid:
//   a. threshold : bubble_mfp.hip's pass as it is (launch_bubble_mask): the bit mask, bit k & 63 of word (i N + j) W + (k >> 6);
//   b. transform : three separable min-plus passes, out[x] = min over x' of in[x'] + d(x, x')^2.
//                  along k  : gran_row_kernel, one thread per cell, straight from the words of its row: the nearest source bit at or
//                             below and at or above k by count-leading / -trailing-zeros, word by word, through the wrap (periodic)
//                             or to the exterior at distance k + 1 / N - k (open box).  The sources are the 0 bits of the mask --
//                             the pad bits of the tail word, 0 as well, are masked out -- or, for the second transform, the 1 bits;
//                  along j, then along i : gran_line_kernel, one thread per cell, lanes along k so that every load is a whole line:
//                             the scan goes outward, d = 1, 2, ..., on both sides and stops as soon as d^2 >= the best so far, so its
//                             cost is bounded by the local distance, not by N.  Lines are read through L2 (a line of 64 lanes of
//                             uint32 at N = 645 does not fit a workgroup's share of LDS at a useful occupancy).  The sums are formed
//                             in 64 bits: the sentinel 0xFFFFFFFF plus d^2 does not wrap, and loses every comparison;
//                  the open box's exterior enters the line passes as the bound min(x + 1, N - x)^2;
//   c. tallies   : gran_tally_kernel over D2: cells in phase (D2 > 0), the largest finite D2, the cells at the sentinel, the sum;
//   d. per radius: gran_erode_kernel packs D2 > r2 into a second bit mask, one wave per word (a ballot), and counts it: eroded[n];
//                  the second transform runs from the 1 bits of that mask -- the exterior is no source -- exact up to r2 (the outward
//                  scan stops at d^2 > r2), and its last pass stores nothing and counts D2' <= r2: opened[n].  Every kernel of a
//                  radius returns at once when the device already knows the eroded set to be empty (eroded[n - 1] for the erosion,
//                  eroded[n] for the transform): the sets only shrink with n, and the host is not asked.
// Every count is an integer sum: reduced per wave, per workgroup, then one 64-bit atomic per counter and workgroup; two calls
// return the same bits.  Memory: D2 lives in region_label, the passes go through region_volume and gran_work (a third uint32 grid);
// gran_mask is the eroded set; all allocated by the first call and kept until the device is closed.
#include "asora_internal.hpp"

namespace asora {

constexpr int GR_THREADS = 256;
constexpr int GR_WAVES = GR_THREADS / 64;
constexpr int GR_BLOCKS_PER_CU = 16;
constexpr unsigned GR_INF = ASORA_GRAN_UNBOUNDED;
// the result words: eroded[], opened[], the tallies
constexpr int GR_ERODED = 0, GR_OPENED = ASORA_BUBBLE_MAX_BINS, GR_TALLY = 2 * ASORA_BUBBLE_MAX_BINS, GR_WORDS = GR_TALLY + ASORA_GRAN_TALLIES;
static_assert(GR_WORDS <= BUBBLE_HOST_WORDS, "the pinned area holds the result words");

// result[slot] += the sum of `n` over the workgroup (every thread of the workgroup calls it, once)
__device__ __forceinline__ void gr_block_add(unsigned long long n, unsigned long long *slot)
{
    __shared__ unsigned long long sh[GR_WAVES];
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0ull;
        for (int q = 0; q < GR_WAVES; ++q) s += sh[q];
        if (s) atomicAdd(slot, s);
    }
}

// the pass along k.  out[c] = the squared distance along the row to its nearest source, GR_INF if it has none.  invert != 0: the
// sources are the 0 bits of the N valid bits of a row (the out-of-phase cells); else the 1 bits.  exterior != 0 (open box only): the
// cells at k = -1 and k = N are sources as well.  gate: the call returns at once if *gate == 0 (NULL: no gate)
__global__ void __launch_bounds__(GR_THREADS) gran_row_kernel(const unsigned long long *__restrict__ mask, int N, int W, int periodic, int exterior,
                                                              int invert, size_t ncell, const unsigned long long *__restrict__ gate,
                                                              unsigned *__restrict__ out)
{
    if (gate && *gate == 0ull) return;
    const unsigned long long tail = (N & 63) ? (1ull << (N & 63)) - 1ull : ~0ull;
    const size_t stride = (size_t)gridDim.x * GR_THREADS;
    for (size_t c = (size_t)blockIdx.x * GR_THREADS + threadIdx.x; c < ncell; c += stride) {
        const size_t row = c / (size_t)N;
        const int k = (int)(c - row * (size_t)N), w = k >> 6, b = k & 63;
        const unsigned long long *r = mask + row * (size_t)W;
        int down = -1, up = -1;
        // at or below k: word w down to word 0, then (periodic) from word W - 1 down to the upper bits of word w itself
        for (int t = 0; t <= W; ++t) {
            int wi = w - t;
            const bool wrapped = wi < 0;
            if (wrapped) {
                if (!periodic) break;
                wi += W;
            }
            unsigned long long s = invert ? ~r[wi] & (wi == W - 1 ? tail : ~0ull) : r[wi];
            if (t == 0) s &= b == 63 ? ~0ull : (2ull << b) - 1ull;
            if (s) {
                down = k - (64 * wi + 63 - __clzll((long long)s)) + (wrapped ? N : 0);
                break;
            }
        }
        // at or above k
        for (int t = 0; t <= W; ++t) {
            int wi = w + t;
            const bool wrapped = wi >= W;
            if (wrapped) {
                if (!periodic) break;
                wi -= W;
            }
            unsigned long long s = invert ? ~r[wi] & (wi == W - 1 ? tail : ~0ull) : r[wi];
            if (t == 0) s &= ~0ull << b;
            if (s) {
                up = 64 * wi + (__ffsll((long long)s) - 1) - k + (wrapped ? N : 0);
                break;
            }
        }
        if (exterior) {
            if (down < 0) down = k + 1;
            if (up < 0) up = N - k;
        }
        const int d = down < 0 ? up : (up < 0 ? down : min(down, up));
        out[c] = d < 0 ? GR_INF : (unsigned)(d * d);
    }
}

// a pass along j (axis 1, stride N) or along i (axis 0, stride N^2): best[c] = min over the line of in[c'] + d(c, c')^2, found by the
// outward scan; exterior != 0: also min(x + 1, N - x)^2; the scan ends at d^2 > cap (cap = GR_INF: no end), beyond which the result
// need not be exact.  COUNT: nothing is stored, *count += the cells with best <= cap; else out[c] = best
template <bool COUNT>
__global__ void __launch_bounds__(GR_THREADS) gran_line_kernel(const unsigned *__restrict__ in, int N, int axis, int periodic, int exterior,
                                                               unsigned cap, size_t ncell, const unsigned long long *__restrict__ gate,
                                                               unsigned *__restrict__ out, unsigned long long *__restrict__ count)
{
    if (gate && *gate == 0ull) return;
    const size_t nn = (size_t)N * N, step = axis == 0 ? nn : (size_t)N, stride = (size_t)gridDim.x * GR_THREADS;
    unsigned long long n = 0ull;
    for (size_t c = (size_t)blockIdx.x * GR_THREADS + threadIdx.x; c < ncell; c += stride) {
        const int i = (int)(c / nn), j = (int)((c - (size_t)i * nn) / (size_t)N);
        const int x = axis == 0 ? i : j;
        const unsigned *line = in + (c - (size_t)x * step);
        unsigned long long best = line[(size_t)x * step];
        if (exterior) {
            const unsigned long long e = (unsigned long long)min(x + 1, N - x);
            best = min(best, e * e);
        }
        const int dmax = periodic ? N / 2 : max(x, N - 1 - x);
        for (int d = 1; d <= dmax; ++d) {
            const unsigned long long dd = (unsigned long long)d * d;
            if (dd >= best || dd > cap) break;
            int lo = x - d, hi = x + d;
            if (periodic) {
                lo = lo < 0 ? lo + N : lo;
                hi = hi >= N ? hi - N : hi;
            }
            if (lo >= 0) best = min(best, (unsigned long long)line[(size_t)lo * step] + dd);
            if (hi < N) best = min(best, (unsigned long long)line[(size_t)hi * step] + dd);
        }
        if (COUNT) n += best <= cap ? 1ull : 0ull;
        else out[c] = (unsigned)best;           // (best <= in[c] <= 0xFFFFFFFF)
    }
    if (COUNT) gr_block_add(n, count);
}

// tally[N_PHASE] += cells with D2 > 0, [N_UNBOUNDED] += cells at the sentinel, [SUM_D2] += the finite D2, [D2_MAX] = their maximum
__global__ void __launch_bounds__(GR_THREADS) gran_tally_kernel(const unsigned *__restrict__ d2, size_t ncell, unsigned long long *__restrict__ tally)
{
    __shared__ unsigned long long sh[GR_WAVES][ASORA_GRAN_TALLIES];
    unsigned long long v[ASORA_GRAN_TALLIES] = {0ull, 0ull, 0ull, 0ull};
    const size_t stride = (size_t)gridDim.x * GR_THREADS;
    for (size_t c = (size_t)blockIdx.x * GR_THREADS + threadIdx.x; c < ncell; c += stride) {
        const unsigned d = d2[c];
        if (d) ++v[ASORA_GRAN_N_PHASE];
        if (d == GR_INF) ++v[ASORA_GRAN_N_UNBOUNDED];
        else {
            v[ASORA_GRAN_SUM_D2] += d;
            v[ASORA_GRAN_D2_MAX] = max(v[ASORA_GRAN_D2_MAX], (unsigned long long)d);
        }
    }
    for (int q = 0; q < ASORA_GRAN_TALLIES; ++q) {
        unsigned long long s = v[q];
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_down(s, o);
            s = q == ASORA_GRAN_D2_MAX ? max(s, other) : s + other;
        }
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][q] = s;
    }
    __syncthreads();
    if (threadIdx.x < ASORA_GRAN_TALLIES) {
        const int q = threadIdx.x;
        unsigned long long s = 0ull;
        for (int u = 0; u < GR_WAVES; ++u) s = q == ASORA_GRAN_D2_MAX ? max(s, sh[u][q]) : s + sh[u][q];
        if (s) {
            if (q == ASORA_GRAN_D2_MAX) atomicMax(&tally[q], s);
            else atomicAdd(&tally[q], s);
        }
    }
}

// the eroded set of a radius as a bit mask in the layout of the phase mask (pad bits 0), one wave per word; *eroded += its size
__global__ void __launch_bounds__(GR_THREADS) gran_erode_kernel(const unsigned *__restrict__ d2, int N, int W, unsigned r2, size_t nwords,
                                                                const unsigned long long *__restrict__ gate, unsigned long long *__restrict__ mask,
                                                                unsigned long long *__restrict__ eroded)
{
    if (gate && *gate == 0ull) return;
    const int lane = threadIdx.x & 63;
    const size_t nwaves = (size_t)gridDim.x * GR_WAVES;
    unsigned long long n = 0ull;
    for (size_t t = (size_t)blockIdx.x * GR_WAVES + (threadIdx.x >> 6); t < nwords; t += nwaves) {      // (the same t in all lanes of a wave)
        const size_t row = t / (size_t)W;
        const int k = 64 * (int)(t - row * (size_t)W) + lane;
        const bool in = k < N && d2[row * (size_t)N + k] > r2;
        const unsigned long long word = __ballot(in);
        if (lane == 0) {
            mask[t] = word;
            n += (unsigned long long)__popcll(word);
        }
    }
    gr_block_add(n, eroded);
}

static unsigned gran_blocks(const State &st, size_t items)
{
    return (unsigned)std::max<size_t>(1, std::min<size_t>((items + GR_THREADS - 1) / GR_THREADS, (size_t)st.cu_count * GR_BLOCKS_PER_CU));
}

static int ensure_gran_buffers(State &st)
{
    const size_t nwords = (size_t)st.N * st.N * (((size_t)st.N + 63) / 64);
    if (int rc = st.granulometry.work.allocate(st.ncell)) return rc;
    if (int rc = st.granulometry.mask.allocate(nwords)) return rc;
    if (int rc = st.granulometry.result.allocate(GR_WORDS)) return rc;
    return 0;
}

// the three passes of one transform from the sources of `mask`: the result goes to `out` (cap = GR_INF), or is counted against
// `cap` into *count (out = NULL); a and b are the two grids the passes go through (out may be neither)
static int launch_gran_transform(State &st, const unsigned long long *mask, int periodic, int exterior, int invert, unsigned cap,
                                 const unsigned long long *gate, unsigned *a, unsigned *b, unsigned *out, unsigned long long *count)
{
    const int N = st.N, W = (N + 63) / 64;
    const size_t ncell = st.ncell;
    const dim3 grid(gran_blocks(st, ncell)), block(GR_THREADS);
    hipLaunchKernelGGL(gran_row_kernel, grid, block, 0, st.stream, mask, N, W, periodic, exterior, invert, ncell, gate, a);
    ASORA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(gran_line_kernel<false>, grid, block, 0, st.stream, (const unsigned *)a, N, 1, periodic, exterior, cap, ncell, gate, b,
                       (unsigned long long *)nullptr);
    ASORA_HIP_TRY(hipGetLastError());
    if (out)
        hipLaunchKernelGGL(gran_line_kernel<false>, grid, block, 0, st.stream, (const unsigned *)b, N, 0, periodic, exterior, cap, ncell, gate, out,
                           (unsigned long long *)nullptr);
    else
        hipLaunchKernelGGL(gran_line_kernel<true>, grid, block, 0, st.stream, (const unsigned *)b, N, 0, periodic, exterior, cap, ncell, gate,
                           (unsigned *)nullptr, count);
    ASORA_HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace asora

using namespace asora;

extern "C" {

int asora_granulometry(int which_grid, double threshold, int phase, int periodic, int n_radii, const double *radii,
                       unsigned long long *eroded, unsigned long long *opened, unsigned long long *tallies, unsigned *dist2)
{
    clear_error();
    if (int rc = require_init("granulometry")) return rc;
    if (int rc = check_bubble_grid("granulometry", which_grid, threshold, phase)) return rc;
    if (n_radii < 1 || n_radii > ASORA_BUBBLE_MAX_BINS)
        return fail(3, "granulometry: n_radii must be in [1, " + std::to_string(ASORA_BUBBLE_MAX_BINS) + "]");
    if (!radii || !eroded || !opened || !tallies) return fail(3, "granulometry: null radii or output pointer");
    unsigned r2[ASORA_BUBBLE_MAX_BINS];
    for (int n = 0; n < n_radii; ++n) {
        if (!std::isfinite(radii[n])) return fail(3, "granulometry: the radii must be finite");
        if (radii[n] < 0.0) return fail(3, "granulometry: the radii must be >= 0");
        if (n > 0 && !(radii[n] > radii[n - 1])) return fail(3, "granulometry: the radii must be strictly ascending");
        const double rr = radii[n] * radii[n];
        if (!(rr < 2147483648.0)) return fail(3, "granulometry: the radii must have R^2 < 2^31");
        r2[n] = (unsigned)std::floor(rr);
    }
    State &st = state();
    if (st.N > ASORA_REGION_MAX_N)
        return fail(4, "granulometry: not built for N > " + std::to_string(ASORA_REGION_MAX_N) + " (8 bytes per cell: 2 GiB there)");
    if (int rc = ensure_bubble_buffers(st)) return rc;
    if (int rc = ensure_region_buffers(st)) return rc;
    if (int rc = ensure_gran_buffers(st)) return rc;
    const int N = st.N, W = (N + 63) / 64, per = periodic != 0;
    const size_t ncell = st.ncell, nwords = (size_t)N * N * W;
    unsigned *d2 = st.regions.label, *ga = st.regions.volume, *gb = st.granulometry.work;
    unsigned long long *res = st.granulometry.result;

    ASORA_HIP_TRY(hipMemsetAsync(res, 0, sizeof(unsigned long long) * GR_WORDS, st.stream));
    if (int rc = launch_bubble_mask(st, which_grid, threshold, phase, false)) return rc;
    if (int rc = launch_gran_transform(st, st.bubbles.mask, per, !per, 1, GR_INF, nullptr, ga, gb, d2, nullptr)) return rc;
    const dim3 block(GR_THREADS);
    hipLaunchKernelGGL(gran_tally_kernel, dim3(gran_blocks(st, ncell)), block, 0, st.stream, (const unsigned *)d2, ncell, res + GR_TALLY);
    ASORA_HIP_TRY(hipGetLastError());
    for (int n = 0; n < n_radii; ++n) {
        hipLaunchKernelGGL(gran_erode_kernel, dim3(gran_blocks(st, nwords * 64)), block, 0, st.stream, (const unsigned *)d2, N, W, r2[n], nwords,
                           n > 0 ? (const unsigned long long *)(res + GR_ERODED + n - 1) : (const unsigned long long *)nullptr, st.granulometry.mask,
                           res + GR_ERODED + n);
        ASORA_HIP_TRY(hipGetLastError());
        if (int rc = launch_gran_transform(st, st.granulometry.mask, per, 0, 0, r2[n], res + GR_ERODED + n, ga, gb, nullptr, res + GR_OPENED + n))
            return rc;
    }
    ASORA_HIP_TRY(hipMemcpyAsync(st.bubbles.host, res, sizeof(unsigned long long) * GR_WORDS, hipMemcpyDeviceToHost, st.stream));
    if (dist2) ASORA_HIP_TRY(hipMemcpyAsync(dist2, d2, sizeof(unsigned) * ncell, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));

    const unsigned long long *h = st.bubbles.host;
    for (int n = 0; n < n_radii; ++n) { eroded[n] = h[GR_ERODED + n]; opened[n] = h[GR_OPENED + n]; }
    for (int t = 0; t < ASORA_GRAN_TALLIES; ++t) tallies[t] = h[GR_TALLY + t];
    return 0;
}

} // extern "C"
