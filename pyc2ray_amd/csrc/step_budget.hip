// step_budget.hip -- the photon budget and the mean ionised fractions of a time step, reduced on the device (asora_step_budget;
// DESIGN.md section 4.2c).  C2Ray closes every time step with its photon statistics: photons that ionised, photons that
// recombinations took back, the volume- and mass-weighted ionised fraction.  With the grids resident on the device the host
// would have to fetch four N^3 grids for that line; here ONE read-only streaming pass forms the twelve sums of
// ASORA_BUDGET_* over a range of planes and twelve doubles cross PCIe.
//
// The pass writes to no grid.  Its sums are two-stage and order-fixed like those of the chemistry passes (per-thread
// accumulators over a grid-stride loop, lane shuffles inside a wave, LDS across the waves, one partial per workgroup and slot,
// then one workgroup that adds the partials): no floating-point atomics, so two calls on the same grids return the same bits.
// Per cell it loads 6 grids (48 B), 7 with a clumping grid, one more with use_temp_end: memory-bound, a sixth of a fused pass.
#include "asora_internal.hpp"

namespace asora {

constexpr int CH_THREADS = 256;      // as the chemistry passes (chemistry.hip)
constexpr int BUDGET_WAVES = CH_THREADS / 64;

typedef double budget_d2 __attribute__((ext_vector_type(2)));     // (a native vector: one 16-byte non-temporal load)

struct BudgetParams {
    size_t begin, count;             // the cells [begin, begin + count) of the [i][j][k] grids
    const double *ndens, *xh, *xh_intermed, *xh_av, *phi, *temp, *temp_end, *clump;
    double clump_c;                  // the factor of every cell when there is no grid (1: clumping off)
    double lls_a, lls_b;             // asora_lls_opacity; both 0: off
    double bh00, albpow, colh0, temph0, abu_c;
    double *partial;                 // [ASORA_BUDGET_COUNT][nblocks]
    int nblocks;
};

// The temperature-only factors of the recombination and collisional-ionisation rates (doric, chemistry.f90:257-262).  Most grids
// are uniform in T, so a lane keeps the factors of the last temperature it saw, as temperature_factors of chemistry.hip does.
struct BudgetTemp {
    double T = -1.0;                 // (no cell has T = -1: the first use always computes)
    double rec = 0.0, col = 0.0;
};
__device__ __forceinline__ void budget_temp(const BudgetParams &p, double T, BudgetTemp &f)
{
    if (T == f.T) return;
    f.T = T;
    f.rec = p.bh00 * pow(T / 1e4, p.albpow);
    f.col = p.colh0 * sqrt(T) * exp(-p.temph0 / T);
}

// one cell's terms added to the twelve accumulators, in the order of the ASORA_BUDGET_* slots
__device__ __forceinline__ void budget_cell(const BudgetParams &p, double (&s)[ASORA_BUDGET_COUNT], BudgetTemp &tf, double n,
                                            double x0, double x1, double xav, double gamma, double T, double c)
{
    budget_temp(p, T, tf);
    const double ne = n * (xav + p.abu_c), nHI = n * (1.0 - xav);
    s[ASORA_BUDGET_CELLS] += 1.0;
    s[ASORA_BUDGET_N] += n;
    s[ASORA_BUDGET_X] += x1;
    s[ASORA_BUDGET_NX] += n * x1;
    s[ASORA_BUDGET_NX0] += n * x0;
    s[ASORA_BUDGET_DNX] += n * (x1 - x0);
    s[ASORA_BUDGET_PHOTO] += gamma * nHI;
    s[ASORA_BUDGET_LLS] += gamma * (n * p.lls_b + p.lls_a);
    s[ASORA_BUDGET_REC] += c * tf.rec * ne * (n * xav);
    s[ASORA_BUDGET_COL] += tf.col * ne * nHI;
    s[ASORA_BUDGET_T] += T;
    s[ASORA_BUDGET_NT] += n * T;
}

template <typename V> __device__ __forceinline__ V budget_load(const double *q)
{
    return __builtin_nontemporal_load(reinterpret_cast<const V *>(q));
}

template <bool CLUMP, bool TEMP_END>
__device__ __forceinline__ void budget_one(const BudgetParams &p, double (&s)[ASORA_BUDGET_COUNT], BudgetTemp &tf, size_t idx)
{
    double T = budget_load<double>(p.temp + idx);
    if (TEMP_END) T = 0.5 * (T + budget_load<double>(p.temp_end + idx));
    const double c = CLUMP ? budget_load<double>(p.clump + idx) : p.clump_c;
    budget_cell(p, s, tf, budget_load<double>(p.ndens + idx), budget_load<double>(p.xh + idx), budget_load<double>(p.xh_intermed + idx),
                budget_load<double>(p.xh_av + idx), budget_load<double>(p.phi + idx), T, c);
}

// A persistent grid with a grid-stride loop over PAIRS of cells (16-byte loads).  A plane range of an odd N begins on an odd
// element every other plane, where a pair would straddle a 16-byte boundary: the range's first cell (when its index is odd) and
// its last one (when what remains is odd) are taken with scalar loads by the grid's first thread, the pairs between them start
// on an even element.  Every grid starts on a 256-byte boundary at least (the arena's slots, hipMalloc).
template <bool CLUMP, bool TEMP_END>
__global__ void __launch_bounds__(CH_THREADS) step_budget_kernel(const BudgetParams p)
{
    double s[ASORA_BUDGET_COUNT];
#pragma unroll
    for (int k = 0; k < ASORA_BUDGET_COUNT; ++k) s[k] = 0.0;
    BudgetTemp tf;
    const size_t head = (p.count > 0 && (p.begin & 1)) ? 1 : 0;
    const size_t first = p.begin + head, npair = (p.count - head) / 2, tail = (p.count - head) & 1;
    const size_t gtid = (size_t)blockIdx.x * CH_THREADS + threadIdx.x, stride = (size_t)gridDim.x * CH_THREADS;
    if (gtid == 0) {
        if (head) budget_one<CLUMP, TEMP_END>(p, s, tf, p.begin);
        if (tail) budget_one<CLUMP, TEMP_END>(p, s, tf, first + 2 * npair);
    }
    for (size_t q = gtid; q < npair; q += stride) {
        const size_t idx = first + 2 * q;
        const budget_d2 n = budget_load<budget_d2>(p.ndens + idx), x0 = budget_load<budget_d2>(p.xh + idx),
                        x1 = budget_load<budget_d2>(p.xh_intermed + idx), xav = budget_load<budget_d2>(p.xh_av + idx),
                        g = budget_load<budget_d2>(p.phi + idx);
        budget_d2 T = budget_load<budget_d2>(p.temp + idx);
        if (TEMP_END) T = 0.5 * (T + budget_load<budget_d2>(p.temp_end + idx));
        budget_d2 c = {p.clump_c, p.clump_c};
        if (CLUMP) c = budget_load<budget_d2>(p.clump + idx);
        budget_cell(p, s, tf, n.x, x0.x, x1.x, xav.x, g.x, T.x, c.x);
        budget_cell(p, s, tf, n.y, x0.y, x1.y, xav.y, g.y, T.y, c.y);
    }
    // wave: lane shuffles; workgroup: one row of LDS per wave, added in the order of the waves
#pragma unroll
    for (int k = 0; k < ASORA_BUDGET_COUNT; ++k)
        for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_down(s[k], o);
    __shared__ double sh[BUDGET_WAVES][ASORA_BUDGET_COUNT];
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < ASORA_BUDGET_COUNT; ++k) sh[threadIdx.x >> 6][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < ASORA_BUDGET_COUNT) {
        double t = sh[0][threadIdx.x];
        for (int w = 1; w < BUDGET_WAVES; ++w) t += sh[w][threadIdx.x];
        p.partial[(size_t)threadIdx.x * p.nblocks + blockIdx.x] = t;
    }
}

// out[k] = the partials of slot k added in a fixed order (one workgroup, as grid_sum_final_kernel)
__global__ void __launch_bounds__(CH_THREADS) step_budget_final_kernel(const double *__restrict__ partial, int nblocks, double *__restrict__ out)
{
    __shared__ double sh[CH_THREADS];
    for (int k = 0; k < ASORA_BUDGET_COUNT; ++k) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nblocks; b += CH_THREADS) s += partial[(size_t)k * nblocks + b];
        sh[threadIdx.x] = s;
        __syncthreads();
        for (int off = CH_THREADS / 2; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[k] = sh[0];
        __syncthreads();
    }
}

// the feature's own buffers: [12][red_blocks] partials and the 12 results behind them on the device, 12 doubles pinned
static int ensure_budget_buffers(State &st)
{
    if (st.budget.partial && st.budget.host) return 0;
    const size_t entries = (size_t)ASORA_BUDGET_COUNT * ((size_t)st.red_blocks + 1);
    if (int rc = st.budget.partial.allocate(entries)) return rc;
    if (int rc = st.budget.host.allocate(ASORA_BUDGET_COUNT)) return rc;
    return 0;
}

static int launch_step_budget(State &st, BudgetParams &p, bool clump_grid, bool temp_end)
{
    KernelTimer kt(ASORA_KERNEL_FINISH);
    const dim3 grid((unsigned)p.nblocks), block(CH_THREADS);
    if (clump_grid && temp_end) hipLaunchKernelGGL((step_budget_kernel<true, true>), grid, block, 0, st.stream, p);
    else if (clump_grid)        hipLaunchKernelGGL((step_budget_kernel<true, false>), grid, block, 0, st.stream, p);
    else if (temp_end)          hipLaunchKernelGGL((step_budget_kernel<false, true>), grid, block, 0, st.stream, p);
    else                        hipLaunchKernelGGL((step_budget_kernel<false, false>), grid, block, 0, st.stream, p);
    ASORA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(step_budget_final_kernel, dim3(1), block, 0, st.stream, (const double *)p.partial, p.nblocks,
                       p.partial + (size_t)ASORA_BUDGET_COUNT * p.nblocks);
    ASORA_HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace asora

using namespace asora;

extern "C" {

int asora_step_budget(double bh00, double albpow, double colh0, double temph0, double abu_c, int use_temp_end, int i_begin,
                      int i_count, double *sums)
{
    clear_error();
    if (int rc = require_init("step_budget")) return rc;
    State &st = state();
    if (!sums) return fail(3, "step_budget: null output pointer");
    if (int rc = check_planes("step_budget", 3, "bad plane range", i_begin, i_count)) return rc;
    if (int rc = require_grids("step_budget", {ASORA_GRID_NDENS, ASORA_GRID_XH, ASORA_GRID_XH_INTERMED, ASORA_GRID_XH_AV,
                                               ASORA_GRID_PHI_ION, ASORA_GRID_TEMP})) return rc;
    if (use_temp_end) {
        if (int rc = require_grids("step_budget", {ASORA_GRID_TEMP_END})) return rc;
        if (!st.grid[ASORA_GRID_TEMP_END]) return fail(4, "step_budget: use_temp_end without ASORA_GRID_TEMP_END on the device");
    }
    if (st.medium.clump_mode == 2) {
        if (int rc = require_grids("step_budget", {ASORA_GRID_CLUMP})) return rc;
        if (!st.grid[ASORA_GRID_CLUMP]) return fail(4, "step_budget: clumping mode 2 without ASORA_GRID_CLUMP on the device");
    }
    for (int k = 0; k < ASORA_BUDGET_COUNT; ++k) sums[k] = 0.0;
    if (i_count == 0) return 0;
    if (int rc = ensure_budget_buffers(st)) return rc;
    BudgetParams p;
    const size_t plane = (size_t)st.N * st.N;
    p.begin = (size_t)i_begin * plane; p.count = (size_t)i_count * plane;
    p.ndens = st.grid[ASORA_GRID_NDENS]; p.xh = st.grid[ASORA_GRID_XH]; p.xh_intermed = st.grid[ASORA_GRID_XH_INTERMED];
    p.xh_av = st.grid[ASORA_GRID_XH_AV]; p.phi = st.grid[ASORA_GRID_PHI_ION]; p.temp = st.grid[ASORA_GRID_TEMP];
    p.temp_end = use_temp_end ? st.grid[ASORA_GRID_TEMP_END] : nullptr;
    p.clump = st.medium.clump_mode == 2 ? st.grid[ASORA_GRID_CLUMP] : nullptr;
    p.clump_c = st.medium.clump_mode == 1 ? st.medium.clump_c : 1.0;
    p.lls_a = st.medium.lls_a; p.lls_b = st.medium.lls_b;
    p.bh00 = bh00; p.albpow = albpow; p.colh0 = colh0; p.temph0 = temph0; p.abu_c = abu_c;
    p.partial = st.budget.partial; p.nblocks = st.red_blocks;
    if (int rc = launch_step_budget(st, p, p.clump != nullptr, use_temp_end != 0)) return rc;
    ASORA_HIP_TRY(hipMemcpyAsync(st.budget.host, p.partial + (size_t)ASORA_BUDGET_COUNT * p.nblocks, sizeof(double) * ASORA_BUDGET_COUNT,
                                 hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    for (int k = 0; k < ASORA_BUDGET_COUNT; ++k) sums[k] = st.budget.host[k];
    return 0;
}

} // extern "C"
