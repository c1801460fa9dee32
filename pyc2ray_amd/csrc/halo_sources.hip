// halo_sources.hip -- the source list of a time step from a halo catalogue, with the low-mass haloes suppressed where the gas is
// already ionised (asora_halo_catalogue_to_device, asora_halo_sources_build; the specification is in
// include/asora_hip.h, its numpy statement in tests/halo_sources_reference.py).  Everything that is summed is an integer, so the
// table, the list and the summary do not depend on the order of the haloes or of the workgroups, and no floating-point atomic enters.
// Per catalogue, on the library's stream:
//   u. upload : the positions, masses and weights of the n haloes into buffers of this call, and two zeroed N^3 grids of uint64;
//   b. bin    : halo_bin_kernel, one thread per halo, grid-stride: floor, wrap or drop, classify, quantise, one 64-bit unsigned
//               atomic add into the Q_hm or the Q_lm grid; the three drop counts per thread, per wave by shuffles, one atomic per wave;
//   c. count  : halo_rows_kernel, one wave per row (i, j): the occupied cells (Q_hm + Q_lm > 0) of the row by ballots; then
//               halo_scan_kernel, the exclusive scan of the N^2 counts in uint64 by one workgroup (the shape of bubble_scan_kernel);
//   a. room   : n_cells comes down (8 bytes, a synchronisation) and the table and the buffers of a build are allocated for it;
//   t. table  : halo_rows_kernel again, the same walk as c, which now writes (cell, Q_hm, Q_lm) of every occupied cell behind its row's
//               offset: ascending cell index.  The upload and the two grids are released before the call returns.
// Per step, over the table's rows in chunks of HS_THREADS (one row per thread, one chunk per workgroup):
//   f. flux   : halo_flux_kernel gathers x = grid[cell], forms the flux and stores it, counts the chunk's active rows and reduces
//               the integer summary per workgroup (one integer atomic per workgroup and word);
//   s. scan   : halo_scan_kernel over the chunk counts;
//   e. emit   : halo_emit_kernel writes the active rows behind their chunk's offset, in table order.
#include "asora_internal.hpp"
#include "fft_device.hpp"

// The specification counts the roundings of the flux (three products, a sum, a product): nothing in this unit is contracted.
#pragma clang fp contract(off)

namespace asora {

constexpr int HS_THREADS = 256;
constexpr int HS_WAVES = HS_THREADS / 64;
constexpr int HS_SCAN_THREADS = 1024;
constexpr int HS_SCAN_TILE = 4 * HS_SCAN_THREADS;
constexpr int HS_BIN_BLOCKS_PER_CU = 4;
constexpr int HS_SUMMARY = 4;                 // the words the flux kernel adds to: n_suppressed, sum Q_hm, sum Q_lm active, sum Q_lm suppressed
constexpr int HS_HOST_WORDS = 16;             // the pinned area: the drop counts and n_cells of a catalogue, the summary of a build

typedef unsigned long long u64;

// ---- b. bin ------------------------------------------------------------------------------------------------------------------
// drops[0] = outside, [1] = nonfinite, [2] = below.  The order of the tests is the specification's: position first, then mass.
__global__ void __launch_bounds__(HS_THREADS) halo_bin_kernel(const double *__restrict__ pos, const double *__restrict__ mass,
                                                              const double *__restrict__ weight, long long n, int N, int wrap, double m_lm,
                                                              double m_hm, int neg_exponent, u64 *__restrict__ q_hm, u64 *__restrict__ q_lm,
                                                              u64 *__restrict__ drops)
{
    unsigned outside = 0, nonfinite = 0, below = 0;          // (a thread sees fewer than 2^32 haloes)
    const long long stride = (long long)gridDim.x * HS_THREADS;
    for (long long h = (long long)blockIdx.x * HS_THREADS + threadIdx.x; h < n; h += stride) {
        const double px = pos[3 * h], py = pos[3 * h + 1], pz = pos[3 * h + 2];
        if (!(fabs(px) < 0x1p31 && fabs(py) < 0x1p31 && fabs(pz) < 0x1p31)) { ++nonfinite; continue; }     // (false for a NaN)
        long long ci = (long long)floor(px), cj = (long long)floor(py), ck = (long long)floor(pz);
        if (wrap) {
            ci %= N; cj %= N; ck %= N;
            if (ci < 0) ci += N;
            if (cj < 0) cj += N;
            if (ck < 0) ck += N;
        } else if (ci < 0 || ci >= N || cj < 0 || cj >= N || ck < 0 || ck >= N) { ++outside; continue; }
        const double m = mass[h];
        const bool hm = m >= m_hm, lm = !hm && m >= m_lm && m < m_hm;
        if (!hm && !lm) { ++below; continue; }
        const u64 q = (u64)rint(scalbn(weight[h], neg_exponent));
        if (q) atomicAdd((hm ? q_hm : q_lm) + ((size_t)ci * N + cj) * (size_t)N + ck, q);
    }
    for (int o = 32; o > 0; o >>= 1) {
        outside += __shfl_down(outside, o);
        nonfinite += __shfl_down(nonfinite, o);
        below += __shfl_down(below, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (outside) atomicAdd(&drops[0], (u64)outside);
        if (nonfinite) atomicAdd(&drops[1], (u64)nonfinite);
        if (below) atomicAdd(&drops[2], (u64)below);
    }
}

// ---- c. count, t. table ------------------------------------------------------------------------------------------------------
// One wave per row (i, j), 64 cells of it per trip: lanes beyond N vote false.  table == nullptr: rows[row] = the row's occupied
// cells.  Else the occupied cells are written behind scan[row]: a lane's slot is the set bits of the ballot below it.
__global__ void __launch_bounds__(HS_THREADS) halo_rows_kernel(const u64 *__restrict__ q_hm, const u64 *__restrict__ q_lm, int N,
                                                               unsigned *__restrict__ rows, const u64 *__restrict__ scan,
                                                               u64 *__restrict__ table, size_t n_cells)
{
    const int lane = threadIdx.x & 63;
    const size_t nrows = (size_t)N * N, nwaves = (size_t)gridDim.x * HS_WAVES;
    for (size_t row = (size_t)blockIdx.x * HS_WAVES + (threadIdx.x >> 6); row < nrows; row += nwaves) {
        u64 at = table ? scan[row] : 0ull;
        unsigned count = 0;
        for (int k0 = 0; k0 < N; k0 += 64) {
            const int k = k0 + lane;
            u64 a = 0, b = 0;
            if (k < N) {
                a = __builtin_nontemporal_load(q_hm + row * (size_t)N + k);
                b = __builtin_nontemporal_load(q_lm + row * (size_t)N + k);
            }
            const bool in = a + b > 0;               // (a + b < 2^62: the refusal of an overflowing exponent)
            const u64 word = __ballot(in);
            if (table && in) {
                const u64 slot = at + (u64)__popcll(word & ((1ull << lane) - 1ull));
                if (slot < n_cells) {                // (always: n_cells is this scan's total)
                    table[slot] = (u64)(row * (size_t)N + k);
                    table[n_cells + slot] = a;
                    table[2 * n_cells + slot] = b;
                }
            }
            at += (u64)__popcll(word);
            count += (unsigned)__popcll(word);
        }
        if (!table && lane == 0) rows[row] = count;
    }
}

// scan[r] = counts[0] + ... + counts[r - 1], scan[n] = the total.  One workgroup, tiles of 4 counts per thread: an inclusive scan of
// the threads' sums by lane shuffles inside a wave, the waves' totals through LDS, the tiles before in a register of every thread.
__global__ void __launch_bounds__(HS_SCAN_THREADS) halo_scan_kernel(const unsigned *__restrict__ counts, size_t n, u64 *__restrict__ scan)
{
    __shared__ u64 wave_total[HS_SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 carry = 0;
    for (size_t base = 0; base < n; base += HS_SCAN_TILE) {
        const size_t i0 = base + 4 * (size_t)threadIdx.x;
        unsigned v[4] = {0u, 0u, 0u, 0u};
        for (int q = 0; q < 4; ++q) if (i0 + q < n) v[q] = counts[i0 + q];
        const u64 s = (u64)v[0] + v[1] + v[2] + v[3];
        u64 inc = s;
        for (int o = 1; o < 64; o <<= 1) {
            const u64 lower = __shfl_up(inc, o);
            if (lane >= o) inc += lower;
        }
        if (lane == 63) wave_total[wave] = inc;
        __syncthreads();
        u64 run = carry + inc - s, total = 0;
        for (int w = 0; w < HS_SCAN_THREADS / 64; ++w) {
            if (w < wave) run += wave_total[w];
            total += wave_total[w];
        }
        for (int q = 0; q < 4; ++q) {
            if (i0 + q < n) scan[i0 + q] = run;
            run += v[q];
        }
        carry += total;
        __syncthreads();                   // (the waves' totals are overwritten by the next tile)
    }
    if (threadIdx.x == 0) scan[n] = carry;
}

// ---- f. flux -----------------------------------------------------------------------------------------------------------------
struct HaloBuild {
    const u64 *table;            // [3][n_cells]: cell, Q_hm, Q_lm
    size_t n_cells;
    const double *x;             // the grid the suppression reads, [N^3]
    double g_hm, g_lm, scale, x_suppress, f_suppressed;
    int model, N;
};

__global__ void __launch_bounds__(HS_THREADS) halo_flux_kernel(const HaloBuild p, double *__restrict__ flux_all,
                                                               unsigned *__restrict__ chunk_count, u64 *__restrict__ summary)
{
    __shared__ u64 sh[HS_WAVES][HS_SUMMARY + 1];
    const size_t r = (size_t)blockIdx.x * HS_THREADS + threadIdx.x;
    u64 v[HS_SUMMARY + 1] = {0, 0, 0, 0, 0};                 // n_suppressed, Q_hm, Q_lm active, Q_lm suppressed, active rows
    if (r < p.n_cells) {
        const u64 cell = p.table[r], qh = p.table[p.n_cells + r], ql = p.table[2 * p.n_cells + r];
        const double x = p.x[cell];
        const bool suppressed = p.model != ASORA_HALO_MODEL_NONE && x > p.x_suppress;       // (false for a NaN)
        const double s = suppressed ? (p.model == ASORA_HALO_MODEL_FULL ? 0.0 : p.f_suppressed) : 1.0;
        const double a = p.g_hm * (double)qh;
        const double b = p.g_lm * s;
        const double c = b * (double)ql;
        const double flux = (a + c) * p.scale;
        flux_all[r] = flux;
        v[0] = suppressed && ql > 0;
        v[1] = qh;
        v[2] = suppressed ? 0ull : ql;
        v[3] = suppressed ? ql : 0ull;
        v[4] = flux > 0.0;
    }
    for (int q = 0; q <= HS_SUMMARY; ++q)
        for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_down(v[q], o);
    if ((threadIdx.x & 63) == 0)
        for (int q = 0; q <= HS_SUMMARY; ++q) sh[threadIdx.x >> 6][q] = v[q];
    __syncthreads();
    if (threadIdx.x <= HS_SUMMARY) {
        u64 t = 0;
        for (int w = 0; w < HS_WAVES; ++w) t += sh[w][threadIdx.x];
        if (threadIdx.x == HS_SUMMARY) chunk_count[blockIdx.x] = (unsigned)t;
        else if (t) atomicAdd(&summary[threadIdx.x], t);
    }
}

// ---- e. emit -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(HS_THREADS) halo_emit_kernel(const u64 *__restrict__ table, size_t n_cells, int N,
                                                               const double *__restrict__ flux_all, const u64 *__restrict__ chunk_scan,
                                                               int32_t *__restrict__ out_pos, double *__restrict__ out_flux)
{
    __shared__ unsigned wave_count[HS_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t r = (size_t)blockIdx.x * HS_THREADS + threadIdx.x;
    double flux = 0.0;
    if (r < n_cells) flux = flux_all[r];
    const bool active = flux > 0.0;
    const u64 word = __ballot(active);
    if (lane == 0) wave_count[wave] = (unsigned)__popcll(word);
    __syncthreads();
    if (!active) return;
    u64 slot = chunk_scan[blockIdx.x] + (u64)__popcll(word & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) slot += wave_count[w];
    if (slot >= n_cells) return;                       // (never: the active rows are no more than the rows)
    const u64 cell = table[r];
    const u64 ij = cell / (u64)N;
    out_pos[3 * slot] = (int32_t)(ij / (u64)N);
    out_pos[3 * slot + 1] = (int32_t)(ij % (u64)N);
    out_pos[3 * slot + 2] = (int32_t)(cell % (u64)N);
    out_flux[slot] = flux;
}

// the transient buffers of a catalogue call: released on every way out of it
struct HaloTransient {
    State::HaloSources &hs;
    explicit HaloTransient(State::HaloSources &h) : hs(h) {}
    ~HaloTransient()
    {
        (void)hs.cat_pos.release(); (void)hs.cat_mass.release(); (void)hs.cat_weight.release();
        (void)hs.q_hm.release(); (void)hs.q_lm.release(); (void)hs.rows.release(); (void)hs.row_scan.release();
    }
};

static int halo_forget(State::HaloSources &hs)
{
    hs.loaded = {};
    if (int rc = hs.table.release()) return rc;
    if (int rc = hs.flux_all.release()) return rc;
    if (int rc = hs.chunk_count.release()) return rc;
    if (int rc = hs.chunk_scan.release()) return rc;
    if (int rc = hs.out_pos.release()) return rc;
    if (int rc = hs.out_flux.release()) return rc;
    if (int rc = hs.summary.release()) return rc;
    if (int rc = hs.host.release()) return rc;
    return 0;
}

static bool halo_has_catalogue(const State::HaloSources &hs) { return hs.loaded.has && hs.table; }

} // namespace asora

using namespace asora;

extern "C" {

int asora_halo_catalogue_to_device(const double *pos, const double *mass, const double *weight, long long n, double m_lm, double m_hm,
                                   int wrap, int unit_exponent, long long *counts_out)
{
    clear_error();
    if (int rc = require_init("halo_catalogue_to_device")) return rc;
    const std::string me("halo_catalogue_to_device");
    if (n < 0) return fail(3, me + ": n must be >= 0");
    if (!counts_out || (n > 0 && (!pos || !mass || !weight))) return fail(3, me + ": null pointer (pos, mass, weight, counts_out)");
    if (std::isnan(m_lm) || std::isnan(m_hm) || m_lm > m_hm) return fail(3, me + ": the mass thresholds must be numbers with m_lm <= m_hm");
    if (wrap != 0 && wrap != 1) return fail(3, me + ": wrap must be 0 or 1");
    if (unit_exponent < -1000 || unit_exponent > 1000) return fail(3, me + ": unit_exponent must lie in [-1000, 1000]");
    // one pass over the weights on the host: eight running sums, so that the adds do not wait for each other (the sum only feeds
    // the refusal below, which has a bit to spare); a weight that is negative or not finite makes its sum fail the test behind
    double part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool good = true;
    for (long long h = 0; h < n; ++h) {
        good &= weight[h] >= 0.0;                    // (false for a NaN)
        part[h & 7] += weight[h];
    }
    const double total = ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]));
    if (!good || !std::isfinite(total))
        for (long long h = 0; h < n; ++h)
            if (!(weight[h] >= 0.0) || !std::isfinite(weight[h]))
                return fail(3, me + ": weight[" + std::to_string(h) + "] is negative or not finite");
    if (!std::isfinite(total)) return fail(3, me + ": the sum of the weights is not finite");
    if (!(std::ldexp(total, -unit_exponent) + 0.5 * (double)n < 0x1p62))
        return fail(3, me + ": with unit 2^" + std::to_string(unit_exponent) + " a cell's integer sum could overflow (sum weight / unit + n / 2 "
                       "must stay below 2^62)");
    State &st = state();
    State::HaloSources &hs = st.halo;
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));          // (a build's download may still read the buffers that go now)
    if (int rc = halo_forget(hs)) return rc;
    HaloTransient transient(hs);

    const int N = st.N;
    const size_t nrows = (size_t)N * N, count = (size_t)n;
    if (int rc = hs.host.allocate(HS_HOST_WORDS)) return rc;
    if (int rc = hs.summary.allocate(HS_HOST_WORDS)) return rc;
    if (int rc = hs.cat_pos.allocate(std::max<size_t>(3 * count, 1))) return rc;
    if (int rc = hs.cat_mass.allocate(std::max<size_t>(count, 1))) return rc;
    if (int rc = hs.cat_weight.allocate(std::max<size_t>(count, 1))) return rc;
    if (int rc = hs.q_hm.allocate(st.ncell)) return rc;
    if (int rc = hs.q_lm.allocate(st.ncell)) return rc;
    if (int rc = hs.rows.allocate(nrows)) return rc;
    if (int rc = hs.row_scan.allocate(nrows + 1)) return rc;

    StageStopwatch<5> watch(st.opt[ASORA_OPT_TIMING] != 0, st.stream);
    if (int rc = watch.mark()) return rc;
    ASORA_HIP_TRY(hipMemsetAsync(hs.q_hm, 0, sizeof(u64) * st.ncell, st.stream));
    ASORA_HIP_TRY(hipMemsetAsync(hs.q_lm, 0, sizeof(u64) * st.ncell, st.stream));
    ASORA_HIP_TRY(hipMemsetAsync(hs.summary, 0, sizeof(u64) * HS_HOST_WORDS, st.stream));
    if (n > 0) {
        ASORA_HIP_TRY(hipMemcpyAsync(hs.cat_pos, pos, sizeof(double) * 3 * count, hipMemcpyHostToDevice, st.stream));
        ASORA_HIP_TRY(hipMemcpyAsync(hs.cat_mass, mass, sizeof(double) * count, hipMemcpyHostToDevice, st.stream));
        ASORA_HIP_TRY(hipMemcpyAsync(hs.cat_weight, weight, sizeof(double) * count, hipMemcpyHostToDevice, st.stream));
    }
    if (int rc = watch.mark()) return rc;
    if (n > 0) {
        const size_t want = (count + HS_THREADS - 1) / HS_THREADS;
        const unsigned blocks = (unsigned)std::min<size_t>(want, (size_t)st.cu_count * HS_BIN_BLOCKS_PER_CU);
        hipLaunchKernelGGL(halo_bin_kernel, dim3(blocks), dim3(HS_THREADS), 0, st.stream, (const double *)hs.cat_pos,
                           (const double *)hs.cat_mass, (const double *)hs.cat_weight, n, N, wrap, m_lm, m_hm, -unit_exponent,
                           (u64 *)hs.q_hm, (u64 *)hs.q_lm, (u64 *)hs.summary);
        ASORA_HIP_TRY(hipGetLastError());
    }
    if (int rc = watch.mark()) return rc;
    const unsigned row_blocks = (unsigned)std::min<size_t>((nrows + HS_WAVES - 1) / HS_WAVES, (size_t)st.cu_count * 32);
    hipLaunchKernelGGL(halo_rows_kernel, dim3(row_blocks), dim3(HS_THREADS), 0, st.stream, (const u64 *)hs.q_hm, (const u64 *)hs.q_lm, N,
                       (unsigned *)hs.rows, (const u64 *)nullptr, (u64 *)nullptr, (size_t)0);
    ASORA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(halo_scan_kernel, dim3(1), dim3(HS_SCAN_THREADS), 0, st.stream, (const unsigned *)hs.rows, nrows, (u64 *)hs.row_scan);
    ASORA_HIP_TRY(hipGetLastError());
    if (int rc = watch.mark()) return rc;
    u64 *host = hs.host;
    ASORA_HIP_TRY(hipMemcpyAsync(host, hs.summary, sizeof(u64) * 3, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipMemcpyAsync(host + 3, hs.row_scan.get() + nrows, sizeof(u64), hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));          // (the table is allocated for the cells that are occupied)
    const size_t n_cells = (size_t)host[3];
    const size_t room = std::max<size_t>(n_cells, 1), chunks = (n_cells + HS_THREADS - 1) / HS_THREADS;
    if (int rc = hs.table.allocate(3 * room)) return rc;
    if (int rc = hs.flux_all.allocate(room)) return rc;
    if (int rc = hs.out_flux.allocate(room)) return rc;
    if (int rc = hs.out_pos.allocate(3 * room)) return rc;
    if (int rc = hs.chunk_count.allocate(std::max<size_t>(chunks, 1))) return rc;
    if (int rc = hs.chunk_scan.allocate(chunks + 1)) return rc;
    if (int rc = watch.mark()) return rc;
    if (n_cells > 0) {
        hipLaunchKernelGGL(halo_rows_kernel, dim3(row_blocks), dim3(HS_THREADS), 0, st.stream, (const u64 *)hs.q_hm, (const u64 *)hs.q_lm, N,
                           (unsigned *)nullptr, (const u64 *)hs.row_scan, (u64 *)hs.table, n_cells);
        ASORA_HIP_TRY(hipGetLastError());
    }
    if (int rc = watch.mark()) return rc;
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));          // (the grids the table was read from are released on return)
    watch.read(hs.ms);
    hs.loaded.has = true;
    hs.generation += 1;
    hs.loaded.n_cells = (long long)n_cells;
    hs.loaded.unit_exponent = unit_exponent;
    counts_out[0] = (long long)n_cells;
    counts_out[1] = (long long)host[0];
    counts_out[2] = (long long)host[1];
    counts_out[3] = (long long)host[2];
    return 0;
}

int asora_halo_catalogue_clear(void)
{
    clear_error();
    State &st = state();
    if (st.init && st.stream) ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    return halo_forget(st.halo);
}

int asora_halo_catalogue_state(long long *n_cells, int *unit_exponent, long long *generation)
{
    clear_error();
    if (!n_cells || !unit_exponent || !generation) return fail(3, "halo_catalogue_state: null pointer");
    const State::HaloSources &hs = state().halo;
    const bool has = halo_has_catalogue(hs);
    *n_cells = has ? hs.loaded.n_cells : -1;
    *unit_exponent = has ? hs.loaded.unit_exponent : 0;
    *generation = has ? hs.generation : 0;
    return 0;
}

int asora_halo_table_to_host(int64_t *cell, uint64_t *q_hm, uint64_t *q_lm, long long capacity)
{
    clear_error();
    if (int rc = require_init("halo_table_to_host")) return rc;
    State &st = state();
    State::HaloSources &hs = st.halo;
    if (!halo_has_catalogue(hs)) return fail(3, "halo_table_to_host: no catalogue on the device (halo_catalogue_to_device)");
    const size_t n = (size_t)hs.loaded.n_cells;
    if (capacity < hs.loaded.n_cells) return fail(3, "halo_table_to_host: room for " + std::to_string(capacity) + " rows, the table has " +
                                                         std::to_string(hs.loaded.n_cells));
    if (n == 0) return 0;
    if (!cell || !q_hm || !q_lm) return fail(3, "halo_table_to_host: null output pointer");
    const u64 *t = hs.table;
    ASORA_HIP_TRY(hipMemcpyAsync(cell, t, sizeof(u64) * n, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipMemcpyAsync(q_hm, t + n, sizeof(u64) * n, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipMemcpyAsync(q_lm, t + 2 * n, sizeof(u64) * n, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    return 0;
}

int asora_halo_sources_build(int which_grid, double g_hm, double g_lm, double scale, int model, double x_suppress, double f_suppressed,
                             unsigned long long *summary_out, long long *n_active)
{
    clear_error();
    if (int rc = require_init("halo_sources_build")) return rc;
    const std::string me("halo_sources_build");
    State &st = state();
    State::HaloSources &hs = st.halo;
    if (which_grid < 0 || which_grid >= ASORA_GRID_COUNT) return fail(3, me + ": bad grid selector");
    if (model != ASORA_HALO_MODEL_NONE && model != ASORA_HALO_MODEL_FULL && model != ASORA_HALO_MODEL_PARTIAL)
        return fail(3, me + ": model must be 0 (none), 1 (full) or 2 (partial)");
    if (!(std::isfinite(g_hm) && g_hm >= 0.0 && std::isfinite(g_lm) && g_lm >= 0.0 && std::isfinite(scale) && scale >= 0.0))
        return fail(3, me + ": g_hm, g_lm and scale must be finite and >= 0");
    if (std::isnan(x_suppress)) return fail(3, me + ": x_suppress must be a number");
    if (!(f_suppressed >= 0.0 && f_suppressed <= 1.0)) return fail(3, me + ": f_suppressed must lie in [0, 1]");
    if (!summary_out || !n_active) return fail(3, me + ": null output pointer");
    if (!halo_has_catalogue(hs)) return fail(3, me + ": no catalogue on the device (halo_catalogue_to_device)");
    if (!st.grid[which_grid] || !st.grid_valid[which_grid]) return fail(4, me + ": grid " + std::to_string(which_grid) + " holds no data");

    const size_t n_cells = (size_t)hs.loaded.n_cells, chunks = (n_cells + HS_THREADS - 1) / HS_THREADS;
    hs.loaded.built = false;
    StageStopwatch<3> watch(st.opt[ASORA_OPT_TIMING] != 0, st.stream);
    ASORA_HIP_TRY(hipMemsetAsync(hs.summary, 0, sizeof(u64) * HS_HOST_WORDS, st.stream));
    if (int rc = watch.mark()) return rc;
    if (chunks > 0) {
        HaloBuild p{hs.table, n_cells, st.grid[which_grid], g_hm, g_lm, scale, x_suppress, f_suppressed, model, st.N};
        hipLaunchKernelGGL(halo_flux_kernel, dim3((unsigned)chunks), dim3(HS_THREADS), 0, st.stream, p, (double *)hs.flux_all,
                           (unsigned *)hs.chunk_count, (u64 *)hs.summary);
        ASORA_HIP_TRY(hipGetLastError());
    }
    if (int rc = watch.mark()) return rc;
    hipLaunchKernelGGL(halo_scan_kernel, dim3(1), dim3(HS_SCAN_THREADS), 0, st.stream, (const unsigned *)hs.chunk_count, chunks,
                       (u64 *)hs.chunk_scan);
    ASORA_HIP_TRY(hipGetLastError());
    if (int rc = watch.mark()) return rc;
    if (chunks > 0) {
        hipLaunchKernelGGL(halo_emit_kernel, dim3((unsigned)chunks), dim3(HS_THREADS), 0, st.stream, (const u64 *)hs.table, n_cells, st.N,
                           (const double *)hs.flux_all, (const u64 *)hs.chunk_scan, (int32_t *)hs.out_pos, (double *)hs.out_flux);
        ASORA_HIP_TRY(hipGetLastError());
    }
    if (int rc = watch.mark()) return rc;
    u64 *host = hs.host;
    ASORA_HIP_TRY(hipMemcpyAsync(host, hs.summary, sizeof(u64) * HS_SUMMARY, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipMemcpyAsync(host + HS_SUMMARY, hs.chunk_scan.get() + chunks, sizeof(u64), hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    watch.read(hs.ms + 5);
    hs.loaded.built = true;
    hs.loaded.n_active = (long long)host[HS_SUMMARY];
    summary_out[0] = host[HS_SUMMARY];
    for (int q = 0; q < HS_SUMMARY; ++q) summary_out[1 + q] = host[q];
    *n_active = hs.loaded.n_active;
    return 0;
}

int asora_halo_sources_to_host(int32_t *pos, double *flux, long long capacity)
{
    clear_error();
    if (int rc = require_init("halo_sources_to_host")) return rc;
    State &st = state();
    State::HaloSources &hs = st.halo;
    if (!halo_has_catalogue(hs)) return fail(3, "halo_sources_to_host: no catalogue on the device (halo_catalogue_to_device)");
    if (!hs.loaded.built) return fail(3, "halo_sources_to_host: no list has been built from this catalogue (halo_sources_build)");
    if (capacity < hs.loaded.n_active) return fail(3, "halo_sources_to_host: room for " + std::to_string(capacity) + " sources, the list has " +
                                                          std::to_string(hs.loaded.n_active));
    const size_t n = (size_t)hs.loaded.n_active;
    if (n == 0) return 0;
    if (!pos || !flux) return fail(3, "halo_sources_to_host: null output pointer");
    ASORA_HIP_TRY(hipMemcpyAsync(pos, hs.out_pos, sizeof(int32_t) * 3 * n, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipMemcpyAsync(flux, hs.out_flux, sizeof(double) * n, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    return 0;
}

int asora_debug_halo_sources_ms(double *ms)
{
    clear_error();
    if (!ms) return fail(3, "debug_halo_sources_ms: null pointer");
    for (int q = 0; q < ASORA_HALO_STAGES; ++q) ms[q] = state().halo.ms[q];
    return 0;
}

} // extern "C"
