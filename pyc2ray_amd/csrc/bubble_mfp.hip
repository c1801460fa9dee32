// bubble_mfp.hip -- the size distribution of the ionised regions (or of the neutral islands) of a device grid by the mean-free-path
// method of Mesinger & Furlanetto (2007): rays from random in-phase cells in random directions, each marched to the first cell
// that is not in phase (asora_bubble_mfp, asora_bubble_mask).  Three stages on the library's stream, none
// of which writes to a grid:
//   a. threshold : one streaming read of the grid -> a bit mask (bit k & 63 of word (i N + j) W + (k >> 6), W = ceil(N / 64); pad
//                  bits 0) and one uint32 count per row (i, j).  The march reads the mask, not the grid: 2 MiB at 256^3 against
//                  128 MiB, which one XCD's L2 holds;
//   b. scan      : exclusive prefix sums of the N^2 row counts in uint64, the total n_phase behind them (one workgroup);
//   c. rays      : one thread per ray, grid-stride.  Start cell, direction and march are a pure function of (seed, ray index, mask):
//                  the specification is the comment above bubble_rays_kernel, its numpy statement tests/bubble_reference.py.
// The bin counts and tallies are integers (LDS atomics per workgroup, then global ones): order-independent.  sum L and sum L^2 are
// reduced in two stages in a fixed order like the sums of step_budget.hip: two calls return the same bits.
#include "asora_internal.hpp"

// The specification counts roundings (1 - mu mu is two of them, tMax = (m + 0.5) tDelta is one): nothing in this unit is contracted
// into a fused multiply-add.
#pragma clang fp contract(off)

namespace asora {

constexpr int BM_THREADS = 256;
constexpr int BM_WAVES = BM_THREADS / 64;
constexpr int BM_SCAN_THREADS = 1024;
constexpr int BM_SLOTS = ASORA_BUBBLE_MAX_BINS + 5;      // the bins, then underflow, overflow, ended, capped, left_box
constexpr int BM_UNDER = ASORA_BUBBLE_MAX_BINS, BM_OVER = BM_UNDER + 1, BM_ENDED = BM_UNDER + 2, BM_CAPPED = BM_UNDER + 3,
              BM_LEFT = BM_UNDER + 4;
constexpr int BM_RESULT = BM_SLOTS + 3;                  // ... then n_phase and the bits of sum L, sum L^2: what crosses PCIe
constexpr int BM_BLOCKS_PER_CU = 8;
static_assert(BM_RESULT + ASORA_BUBBLE_MAX_BINS + 1 <= BUBBLE_HOST_WORDS, "the pinned area holds the result words and the edges");

// ---- a. threshold ------------------------------------------------------------------------------------------------------------
// One wave per row (i, j), one __ballot per word of it: lane l of the ballot of word w holds cell k = 64 w + l; lanes beyond N vote
// false, so the pad bits are 0.  Both predicates are plain comparisons: a NaN is in neither phase.  Lane w keeps word w, so a row's
// words leave in one store instruction (W <= 64 for every mesh device_init accepts).
__global__ void __launch_bounds__(BM_THREADS) bubble_mask_kernel(const double *__restrict__ x, int N, int W, double threshold, int phase,
                                                                 unsigned long long *__restrict__ mask, unsigned *__restrict__ rows)
{
    const int lane = threadIdx.x & 63;
    const size_t nrows = (size_t)N * N, nwaves = (size_t)gridDim.x * BM_WAVES;
    for (size_t row = (size_t)blockIdx.x * BM_WAVES + (threadIdx.x >> 6); row < nrows; row += nwaves) {
        const double *q = x + row * (size_t)N;
        unsigned long long mine = 0;
        unsigned count = 0;
        for (int w = 0; w < W; ++w) {
            const int k = w * 64 + lane;
            bool in = false;
            if (k < N) {
                const double v = __builtin_nontemporal_load(q + k);
                in = phase == 0 ? v >= threshold : v < threshold;
            }
            const unsigned long long word = __ballot(in);
            count += (unsigned)__popcll(word);
            if (lane == w) mine = word;
        }
        if (lane < W) mask[row * (size_t)W + lane] = mine;
        if (lane == 0) rows[row] = count;
    }
}

// ---- b. scan -----------------------------------------------------------------------------------------------------------------
// scan[r] = rows[0] + ... + rows[r - 1], scan[nrows] = n_phase.  One workgroup walks the counts in tiles of 4 per thread (one 16-byte
// load): an inclusive scan of the threads' sums by lane shuffles inside a wave, the waves' totals through LDS, the running total of
// the tiles before in a register of every thread.
constexpr int BM_SCAN_TILE = 4 * BM_SCAN_THREADS;
__global__ void __launch_bounds__(BM_SCAN_THREADS) bubble_scan_kernel(const unsigned *__restrict__ rows, size_t nrows,
                                                                      unsigned long long *__restrict__ scan)
{
    __shared__ unsigned long long wave_total[BM_SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long carry = 0;
    for (size_t base = 0; base < nrows; base += BM_SCAN_TILE) {
        const size_t i0 = base + 4 * (size_t)threadIdx.x;
        unsigned v[4] = {0u, 0u, 0u, 0u};
        if (i0 + 3 < nrows) {
            const uint4 q = *reinterpret_cast<const uint4 *>(rows + i0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            for (int q = 0; q < 4; ++q) if (i0 + q < nrows) v[q] = rows[i0 + q];
        }
        const unsigned long long s = (unsigned long long)v[0] + v[1] + v[2] + v[3];
        unsigned long long inc = s;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long below = __shfl_up(inc, o);
            if (lane >= o) inc += below;
        }
        if (lane == 63) wave_total[wave] = inc;
        __syncthreads();
        unsigned long long run = carry + inc - s, total = 0;
        for (int w = 0; w < BM_SCAN_THREADS / 64; ++w) {
            if (w < wave) run += wave_total[w];
            total += wave_total[w];
        }
        for (int q = 0; q < 4; ++q) {
            if (i0 + q < nrows) scan[i0 + q] = run;
            run += v[q];
        }
        carry += total;
        __syncthreads();                   // (the waves' totals are overwritten by the next tile)
    }
    if (threadIdx.x == 0) scan[nrows] = carry;
}

// ---- c. rays -----------------------------------------------------------------------------------------------------------------
struct BubbleParams {
    int N, W, periodic, nb;
    unsigned long long seed;
    long long n_rays;
    double l_max;
    const unsigned long long *mask;      // [N^2 W]
    const unsigned long long *scan;      // [N^2 + 1]
    size_t nrows;
    const double *edges;                 // [nb + 1]
    unsigned long long *result;          // [BM_RESULT]
    double *partial;                     // [2][nblocks]: sum L, sum L^2 of each workgroup
    int nblocks;
    int32_t *ray_start;                  // the per-ray record, all four or none
    double *ray_dir, *ray_len;
    int32_t *ray_status;
};

// splitmix64 of the c-th state behind `seed`
__device__ __forceinline__ unsigned long long bubble_mix(unsigned long long seed, unsigned long long c)
{
    unsigned long long z = seed + (c + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ double bubble_u01(unsigned long long h) { return (double)(h >> 11) * 0x1p-53; }

__device__ __forceinline__ bool bubble_in_phase(const BubbleParams &p, int i, int j, int k)
{
    return (p.mask[((size_t)i * p.N + j) * (size_t)p.W + (k >> 6)] >> (k & 63)) & 1ull;
}

// Ray r of a call (all hashes in uint64 with wrap-around; u01(h) = (h >> 11) 2^-53):
//   start : the u-th in-phase cell in C order, u = mix(seed, 4 r) % n_phase -- its row by binary search in the scanned counts, its
//           word by walking the row's popcounts, its bit as the n-th set one of the word;
//   dir   : mu = 2 u01(mix(seed, 4 r + 1)) - 1, phi = 2 pi u01(mix(seed, 4 r + 2)), s = sqrt(1 - mu mu), d = (s cos phi, s sin phi, mu);
//   march : exact cell traversal (Amanatides & Woo) from the cell centre, in cell units.  Per axis step = sign(d), tDelta = 1 / |d|
//           (infinite for d = 0), crossings m = 0.  Loop: tMax_a = (m_a + 0.5) tDelta_a, a product, not a running sum; the axis of
//           the smallest tMax (ties: the lowest axis), t = its tMax; t > l_max: CAPPED, length l_max; else move one cell along the
//           axis, ++m; periodic: wrap; open: outside [0, N): LEFT_BOX, length t; the new cell not in phase: ENDED, length t.
//   bins  : an ENDED ray with E[b] <= L < E[b + 1] counts in bin b, L < E[0] is underflow, L >= E[nb] overflow; CAPPED and LEFT_BOX
//           rays are counted apart and are in no bin; sum L and sum L^2 run over the ENDED rays.
// A grid whose n_phase is 0 has no start cell: every workgroup returns at once.
__global__ void __launch_bounds__(BM_THREADS) bubble_rays_kernel(const BubbleParams p)
{
    __shared__ double edges[ASORA_BUBBLE_MAX_BINS + 1];
    __shared__ unsigned long long hist[BM_SLOTS];
    __shared__ double sh_sum[BM_WAVES][2];
    for (int t = threadIdx.x; t <= p.nb; t += BM_THREADS) edges[t] = p.edges[t];
    for (int t = threadIdx.x; t < BM_SLOTS; t += BM_THREADS) hist[t] = 0ull;
    __syncthreads();
    const unsigned long long n_phase = p.scan[p.nrows];
    double s1 = 0.0, s2 = 0.0;
    const int N = p.N;
    const long long stride = (long long)gridDim.x * BM_THREADS;
    for (long long r = (long long)blockIdx.x * BM_THREADS + threadIdx.x; n_phase > 0 && r < p.n_rays; r += stride) {
        const unsigned long long c4 = 4ull * (unsigned long long)r;
        // ---- start cell
        const unsigned long long u = bubble_mix(p.seed, c4) % n_phase;
        size_t lo = 0, hi = p.nrows;                 // scan[lo] <= u, and hi == nrows or scan[hi] > u
        while (hi - lo > 1) {
            const size_t mid = lo + (hi - lo) / 2;
            if (p.scan[mid] <= u) lo = mid; else hi = mid;
        }
        unsigned long long rem = u - p.scan[lo];     // < the row's count
        const unsigned long long *mw = p.mask + lo * (size_t)p.W;
        int w = 0;
        for (; w < p.W - 1; ++w) {
            const unsigned long long c = (unsigned long long)__popcll(mw[w]);
            if (rem < c) break;
            rem -= c;
        }
        unsigned long long word = mw[w];
        for (; rem > 0 && word; --rem) word &= word - 1ull;
        int ci = (int)(lo / (size_t)N), cj = (int)(lo % (size_t)N), ck = w * 64 + (word ? __ffsll((long long)word) - 1 : 0);
        if (ck > N - 1) ck = N - 1;                  // (cannot happen: the pad bits are 0)
        // ---- direction
        const double mu = 2.0 * bubble_u01(bubble_mix(p.seed, c4 + 1ull)) - 1.0;
        const double phi = 6.283185307179586 * bubble_u01(bubble_mix(p.seed, c4 + 2ull));
        const double mu2 = mu * mu;
        const double s = sqrt(1.0 - mu2);
        double sn, cs;
        sincos(phi, &sn, &cs);
        const double dx = s * cs, dy = s * sn, dz = mu;
        if (p.ray_start) {
            p.ray_start[3 * r] = ci; p.ray_start[3 * r + 1] = cj; p.ray_start[3 * r + 2] = ck;
            p.ray_dir[3 * r] = dx; p.ray_dir[3 * r + 1] = dy; p.ray_dir[3 * r + 2] = dz;
        }
        // ---- march
        const int sx = (dx > 0.0) - (dx < 0.0), sy = (dy > 0.0) - (dy < 0.0), sz = (dz > 0.0) - (dz < 0.0);
        const double tdx = sx ? 1.0 / fabs(dx) : INFINITY, tdy = sy ? 1.0 / fabs(dy) : INFINITY, tdz = sz ? 1.0 / fabs(dz) : INFINITY;
        double mx = 0.0, my = 0.0, mz = 0.0, L;
        int status;
        for (;;) {
            const double tx = (mx + 0.5) * tdx, ty = (my + 0.5) * tdy, tz = (mz + 0.5) * tdz;
            int axis = 0;
            double t = tx;
            if (ty < t) { axis = 1; t = ty; }
            if (tz < t) { axis = 2; t = tz; }
            if (!(t <= p.l_max)) { status = ASORA_BUBBLE_CAPPED; L = p.l_max; break; }
            if (axis == 0) { ci += sx; mx += 1.0; } else if (axis == 1) { cj += sy; my += 1.0; } else { ck += sz; mz += 1.0; }
            if (p.periodic) {
                ci = ci < 0 ? ci + N : (ci >= N ? ci - N : ci);
                cj = cj < 0 ? cj + N : (cj >= N ? cj - N : cj);
                ck = ck < 0 ? ck + N : (ck >= N ? ck - N : ck);
            } else if (ci < 0 || ci >= N || cj < 0 || cj >= N || ck < 0 || ck >= N) {
                status = ASORA_BUBBLE_LEFT_BOX; L = t; break;
            }
            if (!bubble_in_phase(p, ci, cj, ck)) { status = ASORA_BUBBLE_ENDED; L = t; break; }
        }
        if (p.ray_len) { p.ray_len[r] = L; p.ray_status[r] = status; }
        if (status == ASORA_BUBBLE_ENDED) {
            // the number of edges <= L, less one (np.searchsorted(E, L, 'right') - 1)
            int a = 0, b = p.nb + 1;
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (edges[mid] <= L) a = mid + 1; else b = mid;
            }
            const int bin = a - 1;
            atomicAdd(&hist[bin < 0 ? BM_UNDER : (bin >= p.nb ? BM_OVER : bin)], 1ull);
            atomicAdd(&hist[BM_ENDED], 1ull);
            s1 += L;
            s2 += L * L;
        } else
            atomicAdd(&hist[status == ASORA_BUBBLE_CAPPED ? BM_CAPPED : BM_LEFT], 1ull);
    }
    // the two moments: lane shuffles inside a wave, one row of LDS per wave added in the order of the waves, one partial per workgroup
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_down(s1, o); s2 += __shfl_down(s2, o); }
    if ((threadIdx.x & 63) == 0) { sh_sum[threadIdx.x >> 6][0] = s1; sh_sum[threadIdx.x >> 6][1] = s2; }
    __syncthreads();
    if (threadIdx.x < 2) {
        double t = sh_sum[0][threadIdx.x];
        for (int q = 1; q < BM_WAVES; ++q) t += sh_sum[q][threadIdx.x];
        p.partial[(size_t)threadIdx.x * p.nblocks + blockIdx.x] = t;
    }
    for (int t = threadIdx.x; t < BM_SLOTS; t += BM_THREADS)
        if (hist[t]) atomicAdd(&p.result[t], hist[t]);
}

// result[BM_SLOTS] = n_phase, the two behind it = the bits of the partials of each moment added in a fixed order (one workgroup, as
// step_budget_final_kernel; nblocks = 0: no ray was shot, two zeros)
__global__ void __launch_bounds__(BM_THREADS) bubble_final_kernel(const double *__restrict__ partial, int nblocks,
                                                                  const unsigned long long *__restrict__ scan, size_t nrows,
                                                                  unsigned long long *__restrict__ result)
{
    __shared__ double sh[BM_THREADS];
    for (int k = 0; k < 2; ++k) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nblocks; b += BM_THREADS) s += partial[(size_t)k * nblocks + b];
        sh[threadIdx.x] = s;
        __syncthreads();
        for (int off = BM_THREADS / 2; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x == 0) result[BM_SLOTS + 1 + k] = (unsigned long long)__double_as_longlong(sh[0]);
        __syncthreads();
    }
    if (threadIdx.x == 0) result[BM_SLOTS] = scan[nrows];
}

// The feature's own buffers, allocated by the first call for the mesh of device_init and kept until the device is closed: the mask,
// the row counts, their scan, the workgroups' partials, the result words and the edges on the device; the last two pinned on the host.
static int bubble_ray_blocks(const State &st) { return st.cu_count * BM_BLOCKS_PER_CU; }

int ensure_bubble_buffers(State &st)
{
    if (st.bubbles.mask && st.bubbles.rows && st.bubbles.scan && st.bubbles.partial && st.bubbles.result && st.bubbles.edges && st.bubbles.host)
        return 0;
    const size_t nrows = (size_t)st.N * st.N, W = ((size_t)st.N + 63) / 64;
    if (int rc = st.bubbles.mask.allocate(nrows * W)) return rc;
    if (int rc = st.bubbles.rows.allocate(nrows)) return rc;
    if (int rc = st.bubbles.scan.allocate((nrows + 1))) return rc;
    if (int rc = st.bubbles.partial.allocate(2 * (size_t)bubble_ray_blocks(st))) return rc;
    if (int rc = st.bubbles.result.allocate(BM_RESULT)) return rc;
    if (int rc = st.bubbles.edges.allocate((ASORA_BUBBLE_MAX_BINS + 1))) return rc;
    if (int rc = st.bubbles.host.allocate(BUBBLE_HOST_WORDS)) return rc;
    return 0;
}

// stages a and b
int launch_bubble_mask(State &st, int which, double threshold, int phase, bool scan)
{
    const size_t nrows = (size_t)st.N * st.N;
    const int W = (st.N + 63) / 64;
    {
        KernelTimer kt(ASORA_KERNEL_BUBBLE_MASK);
        const size_t want = (nrows + BM_WAVES - 1) / BM_WAVES;
        const unsigned blocks = (unsigned)std::min<size_t>(want, (size_t)st.cu_count * 32);
        hipLaunchKernelGGL(bubble_mask_kernel, dim3(blocks), dim3(BM_THREADS), 0, st.stream, (const double *)st.grid[which], st.N, W,
                           threshold, phase, st.bubbles.mask, st.bubbles.rows);
        ASORA_HIP_TRY(hipGetLastError());
    }
    if (!scan) return 0;
    KernelTimer kt(ASORA_KERNEL_BUBBLE_SCAN);
    hipLaunchKernelGGL(bubble_scan_kernel, dim3(1), dim3(BM_SCAN_THREADS), 0, st.stream, (const unsigned *)st.bubbles.rows, nrows,
                       st.bubbles.scan);
    ASORA_HIP_TRY(hipGetLastError());
    return 0;
}

int check_bubble_grid(const char *who, int which, double threshold, int phase)
{
    const State &st = state();
    if (which < 0 || which >= ASORA_GRID_COUNT) return fail(3, std::string(who) + ": bad grid selector");
    if (!st.grid[which] || !st.grid_valid[which]) return fail(4, std::string(who) + ": grid " + std::to_string(which) + " holds no data");
    if (!std::isfinite(threshold)) return fail(3, std::string(who) + ": the threshold must be finite");
    if (phase != 0 && phase != 1) return fail(3, std::string(who) + ": phase must be 0 (x >= threshold) or 1 (x < threshold)");
    return 0;
}

// the per-ray record of a call on the device: freed when the call ends, however it ends
struct BubbleRecord {
    Scoped<int32_t> start, status;
    Scoped<double> dir, len;
};

} // namespace asora

using namespace asora;

extern "C" {

int asora_bubble_mask(int which_grid, double threshold, int phase, uint64_t *mask_words, uint32_t *row_counts)
{
    clear_error();
    if (int rc = require_init("bubble_mask")) return rc;
    if (int rc = check_bubble_grid("bubble_mask", which_grid, threshold, phase)) return rc;
    if (!mask_words || !row_counts) return fail(3, "bubble_mask: null output pointer");
    State &st = state();
    if (int rc = ensure_bubble_buffers(st)) return rc;
    if (int rc = launch_bubble_mask(st, which_grid, threshold, phase, false)) return rc;
    const size_t nrows = (size_t)st.N * st.N, W = ((size_t)st.N + 63) / 64;
    ASORA_HIP_TRY(hipMemcpyAsync(mask_words, st.bubbles.mask, sizeof(unsigned long long) * nrows * W, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipMemcpyAsync(row_counts, st.bubbles.rows, sizeof(unsigned) * nrows, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    return 0;
}

int asora_bubble_mfp(int which_grid, double threshold, int phase, int periodic, unsigned long long seed, long long n_rays, double l_max,
                     int n_bins, const double *edges, unsigned long long *counts, unsigned long long *tallies, double *moments,
                     int32_t *ray_start, double *ray_dir, double *ray_len, int32_t *ray_status)
{
    clear_error();
    if (int rc = require_init("bubble_mfp")) return rc;
    if (int rc = check_bubble_grid("bubble_mfp", which_grid, threshold, phase)) return rc;
    if (n_rays < 0) return fail(3, "bubble_mfp: n_rays must be >= 0");
    if (!(std::isfinite(l_max) && l_max > 0.0)) return fail(3, "bubble_mfp: l_max must be finite and > 0");
    if (n_bins < 1 || n_bins > ASORA_BUBBLE_MAX_BINS)
        return fail(3, "bubble_mfp: n_bins must be in [1, " + std::to_string(ASORA_BUBBLE_MAX_BINS) + "]");
    if (!edges || !counts || !tallies || !moments) return fail(3, "bubble_mfp: null edges or output pointer");
    for (int b = 0; b <= n_bins; ++b) {
        if (!std::isfinite(edges[b])) return fail(3, "bubble_mfp: the bin edges must be finite");
        if (b > 0 && !(edges[b] > edges[b - 1])) return fail(3, "bubble_mfp: the bin edges must be ascending");
    }
    const int given = (ray_start != nullptr) + (ray_dir != nullptr) + (ray_len != nullptr) + (ray_status != nullptr);
    if (given != 0 && given != 4) return fail(3, "bubble_mfp: the per-ray record takes all four of its pointers or none");
    State &st = state();
    if (int rc = ensure_bubble_buffers(st)) return rc;

    const size_t rays = (size_t)n_rays;
    BubbleRecord rec;
    if (given && n_rays > 0) {
        if (int rc = rec.start.allocate(3 * rays)) return rc;
        if (int rc = rec.dir.allocate(3 * rays)) return rc;
        if (int rc = rec.len.allocate(rays)) return rc;
        if (int rc = rec.status.allocate(rays)) return rc;
        // (a grid without an in-phase cell shoots no ray: the record then comes back as zeros)
        ASORA_HIP_TRY(hipMemsetAsync(rec.start, 0, sizeof(int32_t) * 3 * rays, st.stream));
        ASORA_HIP_TRY(hipMemsetAsync(rec.dir, 0, sizeof(double) * 3 * rays, st.stream));
        ASORA_HIP_TRY(hipMemsetAsync(rec.len, 0, sizeof(double) * rays, st.stream));
        ASORA_HIP_TRY(hipMemsetAsync(rec.status, 0, sizeof(int32_t) * rays, st.stream));
    }
    double *edges_host = reinterpret_cast<double *>(st.bubbles.host + BM_RESULT);
    for (int b = 0; b <= n_bins; ++b) edges_host[b] = edges[b];
    ASORA_HIP_TRY(hipMemcpyAsync(st.bubbles.edges, edges_host, sizeof(double) * (n_bins + 1), hipMemcpyHostToDevice, st.stream));
    ASORA_HIP_TRY(hipMemsetAsync(st.bubbles.result, 0, sizeof(unsigned long long) * BM_RESULT, st.stream));
    if (int rc = launch_bubble_mask(st, which_grid, threshold, phase, true)) return rc;

    const size_t nrows = (size_t)st.N * st.N;
    int nblocks = 0;
    if (n_rays > 0) {
        KernelTimer kt(ASORA_KERNEL_BUBBLE_RAYS);
        BubbleParams p;
        p.N = st.N; p.W = (st.N + 63) / 64; p.periodic = periodic != 0; p.nb = n_bins;
        p.seed = seed; p.n_rays = n_rays; p.l_max = l_max;
        p.mask = st.bubbles.mask; p.scan = st.bubbles.scan; p.nrows = nrows; p.edges = st.bubbles.edges;
        p.result = st.bubbles.result; p.partial = st.bubbles.partial;
        nblocks = (int)std::min<size_t>((rays + BM_THREADS - 1) / BM_THREADS, (size_t)bubble_ray_blocks(st));
        p.nblocks = nblocks;
        p.ray_start = rec.start; p.ray_dir = rec.dir; p.ray_len = rec.len; p.ray_status = rec.status;
        hipLaunchKernelGGL(bubble_rays_kernel, dim3((unsigned)nblocks), dim3(BM_THREADS), 0, st.stream, p);
        ASORA_HIP_TRY(hipGetLastError());
    }
    {
        KernelTimer kt(ASORA_KERNEL_BUBBLE_RAYS);
        hipLaunchKernelGGL(bubble_final_kernel, dim3(1), dim3(BM_THREADS), 0, st.stream, (const double *)st.bubbles.partial, nblocks,
                           (const unsigned long long *)st.bubbles.scan, nrows, st.bubbles.result);
        ASORA_HIP_TRY(hipGetLastError());
    }
    ASORA_HIP_TRY(hipMemcpyAsync(st.bubbles.host, st.bubbles.result, sizeof(unsigned long long) * BM_RESULT, hipMemcpyDeviceToHost, st.stream));
    if (given && n_rays > 0) {
        ASORA_HIP_TRY(hipMemcpyAsync(ray_start, rec.start, sizeof(int32_t) * 3 * rays, hipMemcpyDeviceToHost, st.stream));
        ASORA_HIP_TRY(hipMemcpyAsync(ray_dir, rec.dir, sizeof(double) * 3 * rays, hipMemcpyDeviceToHost, st.stream));
        ASORA_HIP_TRY(hipMemcpyAsync(ray_len, rec.len, sizeof(double) * rays, hipMemcpyDeviceToHost, st.stream));
        ASORA_HIP_TRY(hipMemcpyAsync(ray_status, rec.status, sizeof(int32_t) * rays, hipMemcpyDeviceToHost, st.stream));
    }
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    const unsigned long long *h = st.bubbles.host;
    for (int b = 0; b < n_bins; ++b) counts[b] = h[b];
    tallies[0] = h[BM_ENDED]; tallies[1] = h[BM_CAPPED]; tallies[2] = h[BM_LEFT]; tallies[3] = h[BM_UNDER]; tallies[4] = h[BM_OVER];
    tallies[5] = h[BM_SLOTS];
    std::memcpy(moments, h + BM_SLOTS + 1, sizeof(double) * 2);
    return 0;
}

} // extern "C"
