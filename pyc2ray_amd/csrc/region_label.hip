// region_label.hip -- the connected in-phase regions of a device grid (the friends-of-friends view of the ionised bubbles or of the
// neutral islands): their volumes, how many there are, the largest and the second largest and whether the largest spans the box
// (asora_region_sizes).  All integers.  Stages on the library's stream, none of which writes to a grid, each a
// kernel of its own: the order between them is the order of the launches, no workgroup ever waits for another.
//   a. threshold : bubble_mfp.hip's pass as it is (launch_bubble_mask): the bit mask, bit k & 63 of word (i N + j) W + (k >> 6);
//   b. labelling : lock-free union-find on one uint32 label per cell (Komura 2015; Playne & Hawick 2018; ECL-CC, Jaiganesh &
//                  Burtscher 2018).  region_init_kernel reads a cell's run along k out of the mask's words, so a cell starts with the
//                  index of the first cell of its run: the k axis costs no union at all.  region_merge_kernel unites runs of
//                  neighbouring rows, one representative cell per pair of overlapping runs (with 26 neighbours the overlap is one bit
//                  wider each way), and the two ends of a row through the periodic wrap: a root is hooked under a smaller root with
//                  atomicMin.  region_flatten_kernel then gives every cell the root of its region, which is the region's smallest
//                  index -- hooks only ever lower a label, and the smallest cell of a region can hang under nothing;
//   c. volumes   : the first cell of every run adds the run's length onto its root (through a hash table in LDS per workgroup, so a
//                  region that holds most of the box does not serialise the chip on one address); region_roots_kernel bins the roots
//                  (LDS atomics per workgroup, then global ones) and finds the largest with one 64-bit atomicMax on (V << 32) | ~label,
//                  which encodes "greatest V, ties to the smaller label"; region_second_kernel repeats that without the largest and
//                  sets the 3 N plane flags of the largest's cells; region_final_kernel counts the flags.
// Memory: 4 bytes of label and 4 bytes of volume per cell (8 N^3: 128 MiB at 256^3, 2.0 GiB at N = 645, the largest mesh the entry
// accepts; cell indices fit uint32 well beyond), allocated by the first call and kept until the device is closed.
// Every label access of stage b that can race is a relaxed agent-scope atomic (the CUs' L1s are not coherent with each other).
#include "asora_internal.hpp"

namespace asora {

constexpr int RG_THREADS = 256;
constexpr int RG_BLOCKS_PER_CU = 8;
constexpr unsigned RG_NONE = 0xFFFFFFFFu;
// the result words on the device: counts, cells, then ...
constexpr int RG_COUNTS = 0, RG_CELLS = ASORA_BUBBLE_MAX_BINS, RG_SCALARS = 2 * ASORA_BUBBLE_MAX_BINS;
constexpr int RG_N_PHASE = RG_SCALARS, RG_N_REGIONS = RG_SCALARS + 1, RG_SUM_V2 = RG_SCALARS + 2, RG_UNDER_R = RG_SCALARS + 3,
              RG_UNDER_C = RG_SCALARS + 4, RG_OVER_R = RG_SCALARS + 5, RG_OVER_C = RG_SCALARS + 6, RG_KEY_1 = RG_SCALARS + 7,
              RG_KEY_2 = RG_SCALARS + 8, RG_EXTENT = RG_SCALARS + 9 /* three */, RG_WORDS = RG_SCALARS + 12;
constexpr int RG_LOCAL = RG_KEY_1 - RG_SCALARS;          // the scalars a workgroup of the roots pass sums in LDS
static_assert(RG_WORDS + ASORA_BUBBLE_MAX_BINS + 1 <= BUBBLE_HOST_WORDS, "the pinned area holds the result words and the edges");

__device__ __forceinline__ unsigned rg_load(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rg_store(unsigned *p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ bool rg_bit(const unsigned long long *__restrict__ mask, int W, size_t row, int k)
{
    return (mask[row * (size_t)W + (k >> 6)] >> (k & 63)) & 1ull;
}
// ... of a k that may lie outside the row: then no cell
__device__ __forceinline__ bool rg_bit_in(const unsigned long long *__restrict__ mask, int W, int N, size_t row, int k)
{
    return k >= 0 && k < N && rg_bit(mask, W, row, k);
}

// The root of x.  Terminates: label[x] <= x at all times (region_init_kernel writes the first cell of x's run, atomicMin only ever
// lowers a label, the compressing stores of region_flatten_kernel write a root found along the cell's own chain), so x strictly
// decreases from one turn to the next and the walk ends, at the latest at cell 0, on a cell that is its own label.
// (Path halving inside this walk -- each cell passed handed to its grandparent by an atomicMin -- was measured and not kept: at
// 256^3 the call became 1 ... 18 % slower on three fields of four, LABNOTES.  The paths are compressed once, by region_flatten_kernel.)
__device__ __forceinline__ unsigned rg_find(const unsigned *label, unsigned x)
{
    for (;;) {
        const unsigned p = rg_load(label + x);
        if (p == x) return x;
        x = p;
    }
}

// Unite the regions of cells a and b.  Terminates: a turn either returns or goes on with (a, b) replaced by two roots of which the
// larger is strictly smaller than before -- a failed hook means another thread lowered label[b] meanwhile, and `was` < b is what it
// held; indices are bounded below by 0.  No thread waits for another: a failed hook is retried with what it has learnt.
// Correct: atomicMin(label[b], a) with `was` < b either leaves the link b -> was (was < a) or replaces it by b -> a; in both cases
// going on with (a, was) restores what the overwritten link stated.
__device__ __forceinline__ void rg_unite(unsigned *label, unsigned a, unsigned b)
{
    for (;;) {
        a = rg_find(label, a);
        b = rg_find(label, b);
        if (a == b) return;
        if (a > b) { const unsigned t = a; a = b; b = t; }
        const unsigned was = atomicMin(label + b, a);
        if (was == b) return;                // b was a root still: hooked
        b = was;
    }
}

// ---- b.1 the runs ------------------------------------------------------------------------------------------------------------
// One thread per cell (so the stores are coalesced): label = the first cell of the cell's run of in-phase cells along k inside its
// row (no wrap here: the merge joins the two ends), RG_NONE out of phase; volume = 0.
__global__ void __launch_bounds__(RG_THREADS) region_init_kernel(const unsigned long long *__restrict__ mask, int N, int W, size_t ncell,
                                                                 unsigned *__restrict__ label, unsigned *__restrict__ volume)
{
    const size_t stride = (size_t)gridDim.x * RG_THREADS;
    for (size_t c = (size_t)blockIdx.x * RG_THREADS + threadIdx.x; c < ncell; c += stride) {
        const size_t row = c / (size_t)N;
        const int k = (int)(c - row * (size_t)N);
        const unsigned long long *mw = mask + row * (size_t)W;
        int w = k >> 6;
        const int b = k & 63;
        unsigned out = RG_NONE;
        if ((mw[w] >> b) & 1ull) {
            // the highest 0 bit below bit b of the word; none: the run began in an earlier word.  Terminates: w strictly decreases to 0.
            unsigned long long zeros = ~mw[w] & ((1ull << b) - 1ull);
            while (!zeros && w > 0) zeros = ~mw[--w];
            const int first = zeros ? w * 64 + 64 - __clzll((long long)zeros) : 0;
            out = (unsigned)(row * (size_t)N) + (unsigned)first;
        }
        label[c] = out;
        volume[c] = 0u;
    }
}

// ---- b.2 the unions ----------------------------------------------------------------------------------------------------------
// One thread per cell c = (i, j, k) in phase.  Of the 6 (26) neighbour offsets only the half that is lexicographically positive in
// (di, dj) is looked at -- the other half is the same pair seen from the other cell --: rows (i, j + 1), (i + 1, j) and with 26
// neighbours (i + 1, j - 1), (i + 1, j + 1) too; periodic: wrapped, open: left out beyond the faces.  Inside the row the run IS the
// region; only its two ends meet through the wrap (cell N - 1 with cell 0).
// Representatives.  A is c's row, B the other, both as bits inside [0, N).  Cell k unites with B's cell
//   k      unless A[k - 1] and B[k - 1]: then cell k - 1, in the same two runs, does it (or defers further down, and the lowest does);
//   k + 1  (26) unless B[k]: same run of B, and the pair (k, k) is made; or A[k + 1]: then that cell makes the pair (k + 1, k + 1);
//   k - 1  (26) unless B[k], or A[k - 1]: then that cell makes the pair (k - 1, k - 1), or the chain below it does.
// A neighbour reached through the wrap of k is united without such a test (two cells per row).  For N = 1, 2 a cell meets itself
// or one neighbour twice: rg_unite of equal roots returns at once.
struct RegionMergeParams {
    const unsigned long long *mask;
    unsigned *label;
    int N, W, periodic, nrows_fwd;
    int di[4], dj[4];
    size_t ncell;
};
__global__ void __launch_bounds__(RG_THREADS) region_merge_kernel(const RegionMergeParams p)
{
    const int N = p.N, W = p.W;
    const size_t stride = (size_t)gridDim.x * RG_THREADS;
    for (size_t c = (size_t)blockIdx.x * RG_THREADS + threadIdx.x; c < p.ncell; c += stride) {
        const size_t row = c / (size_t)N;
        const int k = (int)(c - row * (size_t)N);
        if (!rg_bit(p.mask, W, row, k)) continue;
        const int i = (int)(row / (size_t)N), j = (int)(row - (size_t)i * N);
        const bool a_m = rg_bit_in(p.mask, W, N, row, k - 1), a_p = rg_bit_in(p.mask, W, N, row, k + 1);
        if (p.periodic && k == N - 1 && rg_bit(p.mask, W, row, 0)) rg_unite(p.label, (unsigned)c, (unsigned)(row * (size_t)N));
        for (int q = 0; q < p.nrows_fwd; ++q) {
            int ii = i + p.di[q], jj = j + p.dj[q];
            if (p.periodic) {
                ii = ii < 0 ? ii + N : (ii >= N ? ii - N : ii);
                jj = jj < 0 ? jj + N : (jj >= N ? jj - N : jj);
            } else if (ii < 0 || ii >= N || jj < 0 || jj >= N)
                continue;
            const size_t row2 = (size_t)ii * N + jj;
            const unsigned base2 = (unsigned)(row2 * (size_t)N);
            const bool b_0 = rg_bit(p.mask, W, row2, k), b_m = rg_bit_in(p.mask, W, N, row2, k - 1), b_p = rg_bit_in(p.mask, W, N, row2, k + 1);
            if (b_0 && !(a_m && b_m)) rg_unite(p.label, (unsigned)c, base2 + (unsigned)k);
            if (p.nrows_fwd == 4) {
                if (k + 1 < N) {
                    if (b_p && !b_0 && !a_p) rg_unite(p.label, (unsigned)c, base2 + (unsigned)(k + 1));
                } else if (p.periodic && rg_bit(p.mask, W, row2, 0))
                    rg_unite(p.label, (unsigned)c, base2);
                if (k > 0) {
                    if (b_m && !b_0 && !a_m) rg_unite(p.label, (unsigned)c, base2 + (unsigned)(k - 1));
                } else if (p.periodic && rg_bit(p.mask, W, row2, N - 1))
                    rg_unite(p.label, (unsigned)c, base2 + (unsigned)(N - 1));
            }
        }
    }
}

// ---- b.3 / c.1 every cell its root; the volumes ------------------------------------------------------------------------------
// After the merge the roots are final.  One thread per cell in phase: label[c] = its root (the stores race with other threads' walks,
// which read either the old label or the root: both lie on the cell's chain).  The thread of the first cell of a run adds the run's
// length onto the root: into a table in LDS that the workgroup keeps over all its cells -- open addressing, RG_PROBES slots tried,
// then straight to global memory -- and empties into volume[] when it ends.
constexpr int RG_HASH = 2048, RG_PROBES = 8;
__global__ void __launch_bounds__(RG_THREADS) region_flatten_kernel(const unsigned long long *__restrict__ mask, int N, int W, size_t ncell,
                                                                    unsigned *label, unsigned *volume)
{
    __shared__ unsigned key[RG_HASH], sum[RG_HASH];
    for (int t = threadIdx.x; t < RG_HASH; t += RG_THREADS) { key[t] = RG_NONE; sum[t] = 0u; }
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * RG_THREADS;
    for (size_t c = (size_t)blockIdx.x * RG_THREADS + threadIdx.x; c < ncell; c += stride) {
        const size_t row = c / (size_t)N;
        const int k = (int)(c - row * (size_t)N);
        const unsigned long long *mw = mask + row * (size_t)W;
        int w = k >> 6;
        const int b = k & 63;
        if (!((mw[w] >> b) & 1ull)) continue;
        const unsigned root = rg_find(label, rg_load(label + c));
        rg_store(label + c, root);
        if (b ? (mw[w] >> (b - 1)) & 1ull : (w > 0 && (mw[w - 1] >> 63))) continue;      // not the first cell of its run
        // the run's length: the lowest 0 bit at or above bit b; none: the run goes on in the next word.  Terminates: w strictly
        // increases to W - 1 (the pad bits of the last word are 0, and a full last word ends the run at N).
        unsigned long long zeros = ~mw[w] & ~((1ull << b) - 1ull);
        while (!zeros && w < W - 1) zeros = ~mw[++w];
        const int end = zeros ? w * 64 + __ffsll((long long)zeros) - 1 : (w + 1) * 64;
        const unsigned len = (unsigned)(end - k);
        const unsigned h = (root * 2654435761u) >> 21;                                   // 11 bits
        bool placed = false;
        for (int t = 0; t < RG_PROBES && !placed; ++t) {                                 // (a counted loop)
            const unsigned s = (h + (unsigned)t) & (RG_HASH - 1);
            const unsigned was = atomicCAS(&key[s], RG_NONE, root);
            if (was == RG_NONE || was == root) { atomicAdd(&sum[s], len); placed = true; }
        }
        if (!placed) atomicAdd(volume + root, len);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < RG_HASH; t += RG_THREADS)
        if (key[t] != RG_NONE) atomicAdd(volume + key[t], sum[t]);
}

// ---- c.2 the roots -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long rg_key(unsigned v, unsigned label) { return ((unsigned long long)v << 32) | (unsigned)~label; }

// A cell that is its own label is a region, volume[c] its V: counts, cells, under- and overflow, n_regions, n_phase = sum V, sum V^2
// in LDS, then one global atomic per word the workgroup touched; the largest by atomicMax of the key.
__global__ void __launch_bounds__(RG_THREADS) region_roots_kernel(const unsigned *__restrict__ label, const unsigned *__restrict__ volume,
                                                                  size_t ncell, int nb, const double *__restrict__ edges_dev,
                                                                  unsigned long long *__restrict__ res)
{
    __shared__ double edges[ASORA_BUBBLE_MAX_BINS + 1];
    __shared__ unsigned long long hist[RG_SCALARS + RG_LOCAL];
    __shared__ unsigned long long best;
    for (int t = threadIdx.x; t <= nb; t += RG_THREADS) edges[t] = edges_dev[t];
    for (int t = threadIdx.x; t < RG_SCALARS + RG_LOCAL; t += RG_THREADS) hist[t] = 0ull;
    if (threadIdx.x == 0) best = 0ull;
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * RG_THREADS;
    for (size_t c = (size_t)blockIdx.x * RG_THREADS + threadIdx.x; c < ncell; c += stride) {
        if (label[c] != (unsigned)c) continue;
        const unsigned v = volume[c];
        const unsigned long long V = v;
        const double x = (double)v;
        int a = 0, b = nb + 1;                       // the number of edges <= V, less one.  Terminates: b - a shrinks every turn
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (edges[mid] <= x) a = mid + 1; else b = mid;
        }
        const int bin = a - 1;
        if (bin < 0) { atomicAdd(&hist[RG_UNDER_R], 1ull); atomicAdd(&hist[RG_UNDER_C], V); }
        else if (bin >= nb) { atomicAdd(&hist[RG_OVER_R], 1ull); atomicAdd(&hist[RG_OVER_C], V); }
        else { atomicAdd(&hist[RG_COUNTS + bin], 1ull); atomicAdd(&hist[RG_CELLS + bin], V); }
        atomicAdd(&hist[RG_N_REGIONS], 1ull);
        atomicAdd(&hist[RG_N_PHASE], V);
        atomicAdd(&hist[RG_SUM_V2], V * V);
        atomicMax(&best, rg_key(v, (unsigned)c));
    }
    __syncthreads();
    for (int t = threadIdx.x; t < RG_SCALARS + RG_LOCAL; t += RG_THREADS)
        if (hist[t]) atomicAdd(&res[t], hist[t]);
    if (threadIdx.x == 0 && best) atomicMax(&res[RG_KEY_1], best);
}

// The largest among the other regions, and the planes the largest has a cell in: flags[a N + plane], a = 0, 1, 2 for i, j, k (every
// writer stores the same 1).
__global__ void __launch_bounds__(RG_THREADS) region_second_kernel(const unsigned *__restrict__ label, const unsigned *__restrict__ volume,
                                                                   int N, size_t ncell, unsigned long long *__restrict__ res,
                                                                   unsigned *__restrict__ flags)
{
    __shared__ unsigned long long best;
    if (threadIdx.x == 0) best = 0ull;
    __syncthreads();
    const unsigned long long key1 = res[RG_KEY_1];
    const unsigned largest = (unsigned)~(unsigned)key1;      // RG_NONE while there is no region
    const size_t stride = (size_t)gridDim.x * RG_THREADS;
    for (size_t c = (size_t)blockIdx.x * RG_THREADS + threadIdx.x; key1 && c < ncell; c += stride) {
        const unsigned l = label[c];
        if (l == largest) {
            const size_t row = c / (size_t)N;
            const int k = (int)(c - row * (size_t)N), i = (int)(row / (size_t)N), j = (int)(row - (size_t)i * N);
            flags[i] = 1u; flags[N + j] = 1u; flags[2 * N + k] = 1u;
        } else if (l == (unsigned)c)
            atomicMax(&best, rg_key(volume[c], (unsigned)c));
    }
    __syncthreads();
    if (threadIdx.x == 0 && best) atomicMax(&res[RG_KEY_2], best);
}

__global__ void __launch_bounds__(RG_THREADS) region_final_kernel(const unsigned *__restrict__ flags, int N, unsigned long long *__restrict__ res)
{
    __shared__ unsigned count[3];
    if (threadIdx.x < 3) count[threadIdx.x] = 0u;
    __syncthreads();
    for (int t = threadIdx.x; t < 3 * N; t += RG_THREADS)
        if (flags[t]) atomicAdd(&count[t / N], 1u);
    __syncthreads();
    if (threadIdx.x < 3) res[RG_EXTENT + threadIdx.x] = count[threadIdx.x];
}

int ensure_region_buffers(State &st)
{
    if (st.regions.label && st.regions.volume && st.regions.result && st.regions.flags) return 0;
    if (int rc = st.regions.label.allocate(st.ncell)) return rc;
    if (int rc = st.regions.volume.allocate(st.ncell)) return rc;
    if (int rc = st.regions.result.allocate(RG_WORDS)) return rc;
    if (int rc = st.regions.flags.allocate(3 * (size_t)st.N)) return rc;
    return 0;
}

static unsigned region_blocks(const State &st)
{
    return (unsigned)std::min<size_t>((st.ncell + RG_THREADS - 1) / RG_THREADS, (size_t)st.cu_count * RG_BLOCKS_PER_CU);
}

// stage b, and the volumes of c.1 with it: the launches that leave every in-phase cell of `mask` with its root in region_label and
// every root with its volume in region_volume
int launch_region_label(State &st, const unsigned long long *mask, int periodic, int connectivity)
{
    const int N = st.N, W = (N + 63) / 64;
    const size_t ncell = st.ncell;
    const dim3 grid(region_blocks(st)), block(RG_THREADS);
    hipLaunchKernelGGL(region_init_kernel, grid, block, 0, st.stream, mask, N, W, ncell, st.regions.label, st.regions.volume);
    ASORA_HIP_TRY(hipGetLastError());
    RegionMergeParams mp;
    mp.mask = mask; mp.label = st.regions.label; mp.N = N; mp.W = W; mp.periodic = periodic != 0; mp.ncell = ncell;
    mp.nrows_fwd = connectivity == 6 ? 2 : 4;
    const int di[4] = {0, 1, 1, 1}, dj[4] = {1, 0, -1, 1};
    for (int q = 0; q < 4; ++q) { mp.di[q] = di[q]; mp.dj[q] = dj[q]; }
    hipLaunchKernelGGL(region_merge_kernel, grid, block, 0, st.stream, mp);
    ASORA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(region_flatten_kernel, grid, block, 0, st.stream, mask, N, W, ncell, st.regions.label, st.regions.volume);
    ASORA_HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace asora

using namespace asora;

extern "C" {

int asora_region_sizes(int which_grid, double threshold, int phase, int periodic, int connectivity, int n_bins, const double *edges,
                       unsigned long long *counts, unsigned long long *cells, unsigned long long *tallies, uint32_t *labels)
{
    clear_error();
    if (int rc = require_init("region_sizes")) return rc;
    if (int rc = check_bubble_grid("region_sizes", which_grid, threshold, phase)) return rc;
    if (connectivity != 6 && connectivity != 26) return fail(3, "region_sizes: connectivity must be 6 (faces) or 26 (faces, edges and corners)");
    if (n_bins < 1 || n_bins > ASORA_BUBBLE_MAX_BINS)
        return fail(3, "region_sizes: n_bins must be in [1, " + std::to_string(ASORA_BUBBLE_MAX_BINS) + "]");
    if (!edges || !counts || !cells || !tallies) return fail(3, "region_sizes: null edges or output pointer");
    for (int b = 0; b <= n_bins; ++b) {
        if (!std::isfinite(edges[b])) return fail(3, "region_sizes: the bin edges must be finite");
        if (b > 0 && !(edges[b] > edges[b - 1])) return fail(3, "region_sizes: the bin edges must be ascending");
    }
    State &st = state();
    if (st.N > ASORA_REGION_MAX_N)
        return fail(4, "region_sizes: not built for N > " + std::to_string(ASORA_REGION_MAX_N) + " (8 bytes per cell: 2 GiB there)");
    if (int rc = ensure_bubble_buffers(st)) return rc;
    if (int rc = ensure_region_buffers(st)) return rc;

    const int N = st.N;
    const size_t ncell = st.ncell;
    double *edges_host = reinterpret_cast<double *>(st.bubbles.host + RG_WORDS);
    for (int b = 0; b <= n_bins; ++b) edges_host[b] = edges[b];
    ASORA_HIP_TRY(hipMemcpyAsync(st.bubbles.edges, edges_host, sizeof(double) * (n_bins + 1), hipMemcpyHostToDevice, st.stream));
    ASORA_HIP_TRY(hipMemsetAsync(st.regions.result, 0, sizeof(unsigned long long) * RG_WORDS, st.stream));
    ASORA_HIP_TRY(hipMemsetAsync(st.regions.flags, 0, sizeof(unsigned) * 3 * (size_t)N, st.stream));
    if (int rc = launch_bubble_mask(st, which_grid, threshold, phase, false)) return rc;

    const dim3 grid(region_blocks(st)), block(RG_THREADS);
    if (int rc = launch_region_label(st, st.bubbles.mask, periodic, connectivity)) return rc;
    hipLaunchKernelGGL(region_roots_kernel, grid, block, 0, st.stream, (const unsigned *)st.regions.label, (const unsigned *)st.regions.volume,
                       ncell, n_bins, (const double *)st.bubbles.edges, st.regions.result);
    ASORA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(region_second_kernel, grid, block, 0, st.stream, (const unsigned *)st.regions.label, (const unsigned *)st.regions.volume,
                       N, ncell, st.regions.result, st.regions.flags);
    ASORA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(region_final_kernel, dim3(1), block, 0, st.stream, (const unsigned *)st.regions.flags, N, st.regions.result);
    ASORA_HIP_TRY(hipGetLastError());
    ASORA_HIP_TRY(hipMemcpyAsync(st.bubbles.host, st.regions.result, sizeof(unsigned long long) * RG_WORDS, hipMemcpyDeviceToHost, st.stream));
    if (labels) ASORA_HIP_TRY(hipMemcpyAsync(labels, st.regions.label, sizeof(uint32_t) * ncell, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));

    const unsigned long long *h = st.bubbles.host;
    for (int b = 0; b < n_bins; ++b) { counts[b] = h[RG_COUNTS + b]; cells[b] = h[RG_CELLS + b]; }
    tallies[ASORA_REGION_N_PHASE] = h[RG_N_PHASE];
    tallies[ASORA_REGION_N_REGIONS] = h[RG_N_REGIONS];
    tallies[ASORA_REGION_SUM_V2] = h[RG_SUM_V2];
    tallies[ASORA_REGION_V_LARGEST] = h[RG_KEY_1] >> 32;
    tallies[ASORA_REGION_LABEL_LARGEST] = (uint32_t)~(uint32_t)h[RG_KEY_1];
    tallies[ASORA_REGION_EXTENT_I] = h[RG_EXTENT];
    tallies[ASORA_REGION_EXTENT_J] = h[RG_EXTENT + 1];
    tallies[ASORA_REGION_EXTENT_K] = h[RG_EXTENT + 2];
    tallies[ASORA_REGION_V_SECOND] = h[RG_KEY_2] >> 32;
    tallies[ASORA_REGION_LABEL_SECOND] = (uint32_t)~(uint32_t)h[RG_KEY_2];
    tallies[ASORA_REGION_UNDERFLOW] = h[RG_UNDER_R];
    tallies[ASORA_REGION_UNDERFLOW_CELLS] = h[RG_UNDER_C];
    tallies[ASORA_REGION_OVERFLOW] = h[RG_OVER_R];
    tallies[ASORA_REGION_OVERFLOW_CELLS] = h[RG_OVER_C];
    return 0;
}

} // extern "C"
