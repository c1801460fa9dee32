// topology.hip -- the topology of the in-phase cells of a device grid: the numbers of lattice elements (cells, faces, edges, vertices)
// of the closed and of the open complex, from which the Euler characteristic and the Minkowski functionals follow, and the numbers of
// components, of components of the complement and of cavities, from which the Betti numbers follow (asora_topology; DESIGN.md section
// 4.2f).  All integers.  Stages on the library's stream, none of which writes to a grid:
//   a. threshold  : bubble_mfp.hip's pass as it is (launch_bubble_mask): the bit mask, bit k & 63 of word (i N + j) W + (k >> 6);
//   b. elements   : topology_count_kernel, one thread per word position (i, j, w).  The 64 anchors (i, j, 64 w ... 64 w + 63) have
//                   their eight incident cells in four rows -- (i, j), (i - 1, j), (i, j - 1), (i - 1, j - 1) -- at k and k - 1: the
//                   word of each row and that word shifted up by one bit, the carry out of word w - 1 (for w = 0: bit N - 1 of the
//                   row through the wrap, 0 in the open box).  An element's incident cells are a subset of the eight, so each count is
//                   the popcount of the OR (closed: at least one in phase) or of the AND (open: all in phase) of 2, 4 or 8 of these
//                   words.  Open box: cells outside are 0, and the anchors run to N on every axis -- one more plane, row and bit; an
//                   element that extends along an axis has all its incident cells at the anchor's index on that axis, so at index N
//                   it counts nothing and no range is cut by element type.  Bit N of a row lies in word N / 64, which for N a multiple
//                   of 64 the mask does not have: read as 0, its shifted form is the carry alone;
//   c. complement : topology_complement_kernel, the valid bits inverted, the pad bits 0, into a mask of its own;
//   d. components : launch_region_label (region_label.hip) on the mask, topology_roots_kernel counts the cells that are their own
//                   label; then the same on the complement with the dual connectivity.  In the open box topology_faces_kernel first
//                   marks the root of every complement cell on a face of the box, and the roots left unmarked are the cavities.  The
//                   mark is a 0 in volume[root]: after the labelling a root's volume is >= 1, and nobody reads the volumes here.
// Every count is an integer sum: reduced per wave, per workgroup, then one 64-bit atomic per counter and workgroup; two calls
// return the same bits.  Memory: the complement mask (N^2 W words: 2 MiB at 256^3), allocated by the first call and kept until the
// device is closed; labels, volumes and the result words are those of asora_region_sizes, used one call after the other.
#include "asora_internal.hpp"

namespace asora {

constexpr int TP_THREADS = 256;
constexpr int TP_WAVES = TP_THREADS / 64;
constexpr int TP_BLOCKS_PER_CU = 8;
constexpr int TP_ELEMENTS = 7;      // cells, closed faces / edges / vertices, open faces / edges / vertices: ASORA_TOPO_CELLS ... _OPEN_VERTICES
static_assert(ASORA_TOPO_CELLS == 0 && ASORA_TOPO_OPEN_VERTICES == TP_ELEMENTS - 1, "the element counts lead the tallies, in the kernel's order");
static_assert(ASORA_TOPO_TALLIES <= BUBBLE_HOST_WORDS, "the pinned area holds the result words");

struct TopoParams {
    const unsigned long long *mask;      // [N^2 W]
    unsigned long long *result;          // [ASORA_TOPO_TALLIES]
    int N, W, periodic;
    int span, WT;                        // anchors per axis (N, open: N + 1) and words per row of anchors (W, open: N / 64 + 1)
};

// word w of row (i, j); outside the mask: through the wrap (periodic), else 0
__device__ __forceinline__ unsigned long long tp_word(const TopoParams &p, int i, int j, int w)
{
    const int N = p.N;
    if (w < 0 || w >= p.W) return 0ull;
    if (p.periodic) {
        i = i < 0 ? i + N : i;
        j = j < 0 ? j + N : j;
    } else if (i < 0 || i >= N || j < 0 || j >= N)
        return 0ull;
    return p.mask[((size_t)i * N + j) * (size_t)p.W + w];
}

// the cells (i, j, 64 w + b - 1) of row (i, j) at bit b: `here` = tp_word(i, j, w) shifted up, bit 0 from word w - 1 or the wrap
__device__ __forceinline__ unsigned long long tp_below(const TopoParams &p, int i, int j, int w, unsigned long long here)
{
    unsigned long long carry;
    if (w > 0) carry = tp_word(p, i, j, w - 1) >> 63;
    else carry = p.periodic ? (tp_word(p, i, j, p.W - 1) >> ((p.N - 1) & 63)) & 1ull : 0ull;
    return (here << 1) | carry;
}

__global__ void __launch_bounds__(TP_THREADS) topology_count_kernel(const TopoParams p)
{
    __shared__ unsigned sh[TP_WAVES][TP_ELEMENTS];
    unsigned n[TP_ELEMENTS] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};       // (< 2^32: 192 per trip at most)
    const size_t total = (size_t)p.span * p.span * p.WT, stride = (size_t)gridDim.x * TP_THREADS;
    for (size_t t = (size_t)blockIdx.x * TP_THREADS + threadIdx.x; t < total; t += stride) {
        const size_t row = t / (size_t)p.WT;
        const int w = (int)(t - row * (size_t)p.WT), i = (int)(row / (size_t)p.span), j = (int)(row - (size_t)i * p.span);
        // the anchors of this word that exist: k < N, open: k <= N (the pad bits of the mask are 0, those of the shifted words are not)
        const int left = p.N + (p.periodic ? 0 : 1) - 64 * w;
        const unsigned long long valid = left >= 64 ? ~0ull : (1ull << left) - 1ull;
        const unsigned long long a = tp_word(p, i, j, w), b = tp_word(p, i - 1, j, w), c = tp_word(p, i, j - 1, w), d = tp_word(p, i - 1, j - 1, w);
        const unsigned long long a1 = tp_below(p, i, j, w, a), b1 = tp_below(p, i - 1, j, w, b), c1 = tp_below(p, i, j - 1, w, c),
                                 d1 = tp_below(p, i - 1, j - 1, w, d);
        n[0] += (unsigned)__popcll(a & valid);
        // faces: across k, across j, across i
        n[1] += (unsigned)(__popcll((a | a1) & valid) + __popcll((a | c) & valid) + __popcll((a | b) & valid));
        n[4] += (unsigned)(__popcll(a & a1 & valid) + __popcll(a & c & valid) + __popcll(a & b & valid));
        // edges: along i (rows j, j - 1 at k, k - 1), along j (rows i, i - 1 at k, k - 1), along k (the four rows at k)
        n[2] += (unsigned)(__popcll((a | c | a1 | c1) & valid) + __popcll((a | b | a1 | b1) & valid) + __popcll((a | b | c | d) & valid));
        n[5] += (unsigned)(__popcll(a & c & a1 & c1 & valid) + __popcll(a & b & a1 & b1 & valid) + __popcll(a & b & c & d & valid));
        // vertices
        n[3] += (unsigned)__popcll((a | b | c | d | a1 | b1 | c1 | d1) & valid);
        n[6] += (unsigned)__popcll(a & b & c & d & a1 & b1 & c1 & d1 & valid);
    }
    for (int q = 0; q < TP_ELEMENTS; ++q) {
        unsigned v = n[q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < TP_ELEMENTS) {
        unsigned long long s = 0ull;
        for (int q = 0; q < TP_WAVES; ++q) s += sh[q][threadIdx.x];
        if (s) atomicAdd(&p.result[threadIdx.x], s);
    }
}

__global__ void __launch_bounds__(TP_THREADS) topology_complement_kernel(const unsigned long long *__restrict__ mask, int N, int W, size_t nwords,
                                                                         unsigned long long *__restrict__ out)
{
    const unsigned long long tail = (N & 63) ? (1ull << (N & 63)) - 1ull : ~0ull;
    const size_t stride = (size_t)gridDim.x * TP_THREADS;
    for (size_t t = (size_t)blockIdx.x * TP_THREADS + threadIdx.x; t < nwords; t += stride)
        out[t] = ~mask[t] & ((int)(t % (size_t)W) == W - 1 ? tail : ~0ull);
}

// volume[root] = 0 for the root of every in-phase cell on a face of the box (every writer stores the same 0): one thread per cell
// of the six faces, f = face N^2 + u N + v
__global__ void __launch_bounds__(TP_THREADS) topology_faces_kernel(const unsigned *__restrict__ label, int N, unsigned *__restrict__ volume)
{
    const size_t nn = (size_t)N * N, total = 6 * nn, stride = (size_t)gridDim.x * TP_THREADS;
    for (size_t f = (size_t)blockIdx.x * TP_THREADS + threadIdx.x; f < total; f += stride) {
        const int face = (int)(f / nn);
        const size_t r = f - (size_t)face * nn;
        const size_t u = r / (size_t)N, v = r - u * (size_t)N, e = (face & 1) ? (size_t)(N - 1) : 0;
        const size_t c = face < 2 ? (e * N + u) * N + v : (face < 4 ? (u * N + e) * N + v : (u * N + v) * N + e);
        const unsigned l = label[c];
        if (l != 0xFFFFFFFFu) volume[l] = 0u;
    }
}

// result[slot_roots] += the cells that are their own label; slot_kept >= 0: result[slot_kept] += those of them whose volume is not 0
__global__ void __launch_bounds__(TP_THREADS) topology_roots_kernel(const unsigned *__restrict__ label, const unsigned *__restrict__ volume,
                                                                    size_t ncell, unsigned long long *__restrict__ result, int slot_roots,
                                                                    int slot_kept)
{
    __shared__ unsigned sh[TP_WAVES][2];
    unsigned roots = 0u, kept = 0u;
    const size_t stride = (size_t)gridDim.x * TP_THREADS;
    for (size_t c = (size_t)blockIdx.x * TP_THREADS + threadIdx.x; c < ncell; c += stride) {
        if (label[c] != (unsigned)c) continue;
        ++roots;
        if (slot_kept >= 0 && volume[c]) ++kept;
    }
    for (int o = 32; o > 0; o >>= 1) { roots += __shfl_down(roots, o); kept += __shfl_down(kept, o); }
    if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6][0] = roots; sh[threadIdx.x >> 6][1] = kept; }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long s = 0ull;
        for (int q = 0; q < TP_WAVES; ++q) s += sh[q][threadIdx.x];
        const int slot = threadIdx.x == 0 ? slot_roots : slot_kept;
        if (s && slot >= 0) atomicAdd(&result[slot], s);
    }
}

static unsigned topo_blocks(const State &st, size_t items)
{
    return (unsigned)std::max<size_t>(1, std::min<size_t>((items + TP_THREADS - 1) / TP_THREADS, (size_t)st.cu_count * TP_BLOCKS_PER_CU));
}

} // namespace asora

using namespace asora;

extern "C" {

int asora_topology(int which_grid, double threshold, int phase, int periodic, int connectivity, unsigned long long *tallies)
{
    clear_error();
    if (int rc = require_init("topology")) return rc;
    if (int rc = check_bubble_grid("topology", which_grid, threshold, phase)) return rc;
    if (connectivity != 6 && connectivity != 26) return fail(3, "topology: connectivity must be 6 (faces) or 26 (faces, edges and corners)");
    if (!tallies) return fail(3, "topology: null output pointer");
    State &st = state();
    if (st.N > ASORA_REGION_MAX_N)
        return fail(4, "topology: not built for N > " + std::to_string(ASORA_REGION_MAX_N) + " (8 bytes per cell: 2 GiB there)");
    if (int rc = ensure_bubble_buffers(st)) return rc;
    if (int rc = ensure_region_buffers(st)) return rc;
    const int N = st.N, W = (N + 63) / 64;
    const size_t ncell = st.ncell, nwords = (size_t)N * N * W;
    if (int rc = st.topology.complement.allocate(nwords)) return rc;

    unsigned long long *res = st.regions.result;
    ASORA_HIP_TRY(hipMemsetAsync(res, 0, sizeof(unsigned long long) * ASORA_TOPO_TALLIES, st.stream));
    if (int rc = launch_bubble_mask(st, which_grid, threshold, phase, false)) return rc;

    TopoParams p;
    p.mask = st.bubbles.mask; p.result = res; p.N = N; p.W = W; p.periodic = periodic != 0;
    p.span = p.periodic ? N : N + 1;
    p.WT = p.periodic ? W : N / 64 + 1;
    const dim3 block(TP_THREADS);
    hipLaunchKernelGGL(topology_count_kernel, dim3(topo_blocks(st, (size_t)p.span * p.span * p.WT)), block, 0, st.stream, p);
    ASORA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(topology_complement_kernel, dim3(topo_blocks(st, nwords)), block, 0, st.stream,
                       (const unsigned long long *)st.bubbles.mask, N, W, nwords, st.topology.complement);
    ASORA_HIP_TRY(hipGetLastError());

    const dim3 cells(topo_blocks(st, ncell));
    if (int rc = launch_region_label(st, st.bubbles.mask, p.periodic, connectivity)) return rc;
    hipLaunchKernelGGL(topology_roots_kernel, cells, block, 0, st.stream, (const unsigned *)st.regions.label, (const unsigned *)st.regions.volume,
                       ncell, res, (int)ASORA_TOPO_COMPONENTS, -1);
    ASORA_HIP_TRY(hipGetLastError());
    if (int rc = launch_region_label(st, st.topology.complement, p.periodic, connectivity == 6 ? 26 : 6)) return rc;
    if (!p.periodic) {
        hipLaunchKernelGGL(topology_faces_kernel, dim3(topo_blocks(st, 6 * (size_t)N * N)), block, 0, st.stream, (const unsigned *)st.regions.label,
                           N, st.regions.volume);
        ASORA_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(topology_roots_kernel, cells, block, 0, st.stream, (const unsigned *)st.regions.label, (const unsigned *)st.regions.volume,
                       ncell, res, (int)ASORA_TOPO_COMPLEMENT_COMPONENTS, p.periodic ? -1 : (int)ASORA_TOPO_CAVITIES);
    ASORA_HIP_TRY(hipGetLastError());
    ASORA_HIP_TRY(hipMemcpyAsync(st.bubbles.host, res, sizeof(unsigned long long) * ASORA_TOPO_TALLIES, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    for (int t = 0; t < ASORA_TOPO_TALLIES; ++t) tallies[t] = st.bubbles.host[t];
    return 0;
}

} // extern "C"
