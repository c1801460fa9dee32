// lightcone.hip -- slices of a light cone, emitted while a run advances (asora_lightcone_advance).  The library
// knows nothing of cosmology: per slot it keeps one formed field g_prev from the previous call and blends planes of it with planes
// of the field g_now formed from the present grids, out = (w_prev g_prev) + (w_now g_now).  The stages, all on the library's stream:
//   d. mean density : ps_mean_density (power_spectrum.hip), for the kinds that divide by it: the launches, so the bits, of
//                     asora_power_spectrum;
//   e. emit         : the slices into the staging buffer [n_slices][N][N].  lc_emit_kernel, one work item per output, the second of
//                     the two remaining axes fastest: for los_axis 0 a slice is N^2 contiguous cells, for los_axis 1 N rows of N --
//                     reads and writes are whole lines either way.  For los_axis 2 a slice takes one cell out of every row; there
//                     the host cuts plane[] into runs of consecutive planes (ascending or descending, LC_RUN_MIN ... LC_RUN_MAX
//                     long) and lc_emit_runs_kernel gives a workgroup one i, 64 j and one run: it reads each row's contiguous
//                     fragment of `len` cells once, blends on the way into LDS and writes out[t][i][j0 ... j0 + 63], 512 contiguous
//                     bytes per slice.  Slices in no such run (a shuffled list, a run cut short by the wrap) go through
//                     lc_emit_kernel with a list of their indices;
//   m. moments      : lc_moments_kernel, LC_RED workgroups per slice over the STAGED slice (so the order is (N)'s alone, whichever
//                     kernel emitted it): sum out and sum out^2 in double-double per work item in index order, per wave by a shuffle
//                     tree, per workgroup in wave order; lc_moments_fold_kernel adds the LC_RED partials in workgroup order;
//   r. refresh      : lc_refresh_kernel, g_prev <- g_now over the N^3 cells, formed by the same function as the emit's.
// The blend is two products, each rounded, and one sum; nothing is contracted.  No floating-point atomic anywhere.
#include "asora_internal.hpp"
#include "fft_device.hpp"

namespace asora {

constexpr int LC_RED = 16;                   // workgroups per slice of the moments: a constant, so that the order is the mesh's alone
constexpr int LC_RUN_MIN = 4, LC_RUN_MAX = 32, LC_RUN_PITCH = LC_RUN_MAX + 1, LC_TILE_J = 64;
constexpr unsigned LC_MAX_BLOCKS = 8192;     // of the grid-stride kernels
// the words (doubles) of State::lightcone.params / .host: the weights, the planes and the fallback's slice list (int32), the
// runs (int4), then -- device and pinned area alike -- the moments
constexpr size_t LC_P_WPREV = 0, LC_P_WNOW = ASORA_LC_MAX_SLICES, LC_P_PLANE = 2 * ASORA_LC_MAX_SLICES,
                 LC_P_LIST = LC_P_PLANE + ASORA_LC_MAX_SLICES / 2, LC_P_RUNS = LC_P_LIST + ASORA_LC_MAX_SLICES / 2,
                 LC_P_MOMENTS = LC_P_RUNS + 2 * (ASORA_LC_MAX_SLICES / LC_RUN_MIN), LC_P_WORDS = LC_P_MOMENTS + 2 * ASORA_LC_MAX_SLICES;

// what g_now is formed from: a grid verbatim (src), or a kind of ps_form from x, n, temp and the mean density at *nbar
struct LcSource {
    int kind;
    const double *x, *n, *temp, *src, *nbar;
    double t_gamma;
};

__device__ __forceinline__ double lc_form(const LcSource &s, size_t c, double nbar)
{
    return s.src ? s.src[c] : ps_form(s.kind, c, s.x, s.n, s.temp, nbar, 1.0, s.t_gamma);
}

__device__ __forceinline__ double lc_blend(double wp, double gp, double wn, double gn)
{
#pragma clang fp contract(off)
    const double a = wp * gp, b = wn * gn;
    return a + b;
}

// out[t][a][b] for the `count` slices t = list[q] (list = NULL: t = q), one work item per output, grid-stride
__global__ void __launch_bounds__(PS_THREADS) lc_emit_kernel(LcSource s, const double *__restrict__ prev, int N, int los_axis, int count,
                                                              const int32_t *__restrict__ list, const int32_t *__restrict__ plane,
                                                              const double *__restrict__ w_prev, const double *__restrict__ w_now,
                                                              double *__restrict__ out)
{
    const double nbar = s.nbar ? *s.nbar : 1.0;
    const size_t n2 = (size_t)N * N, total = (size_t)count * n2, stride = (size_t)gridDim.x * PS_THREADS;
    for (size_t o = (size_t)blockIdx.x * PS_THREADS + threadIdx.x; o < total; o += stride) {
        const size_t q = o / n2, r = o - q * n2;
        const int t = list ? list[q] : (int)q;
        const size_t a = r / N, b = r - a * N, p = (size_t)plane[t];
        const size_t c = los_axis == 0 ? p * n2 + r : los_axis == 1 ? (a * N + p) * N + b : r * N + p;
        out[(size_t)t * n2 + r] = lc_blend(w_prev[t], prev[c], w_now[t], lc_form(s, c, nbar));
    }
}

// los_axis 2: workgroup (x: tile of LC_TILE_J j, y: i, z: run).  runs[z] = {t0, len, k0, step}: the slices t0 ... t0 + len - 1 take
// the planes k0 ... k0 + len - 1, ascending (step 1: plane k0 + q is slice t0 + q) or descending (step -1: slice t0 + len - 1 - q)
__global__ void __launch_bounds__(PS_THREADS) lc_emit_runs_kernel(LcSource s, const double *__restrict__ prev, int N,
                                                                   const int4 *__restrict__ runs, const double *__restrict__ w_prev,
                                                                   const double *__restrict__ w_now, double *__restrict__ out)
{
    __shared__ double tile[LC_TILE_J * LC_RUN_PITCH];
    const double nbar = s.nbar ? *s.nbar : 1.0;
    const int4 run = runs[blockIdx.z];
    const int t0 = run.x, len = run.y, k0 = run.z, step = run.w, i = blockIdx.y, j0 = blockIdx.x * LC_TILE_J;
    const int width = N - j0 < LC_TILE_J ? N - j0 : LC_TILE_J;
    const size_t n2 = (size_t)N * N;
    for (int w = threadIdx.x; w < width * len; w += PS_THREADS) {
        const int jj = w / len, kk = w - jj * len, t = step > 0 ? t0 + kk : t0 + (len - 1 - kk);
        const size_t c = ((size_t)i * N + (j0 + jj)) * N + (k0 + kk);
        tile[jj * LC_RUN_PITCH + kk] = lc_blend(w_prev[t], prev[c], w_now[t], lc_form(s, c, nbar));
    }
    __syncthreads();
    for (int w = threadIdx.x; w < LC_TILE_J * len; w += PS_THREADS) {
        const int kk = w / LC_TILE_J, jj = w - kk * LC_TILE_J, t = step > 0 ? t0 + kk : t0 + (len - 1 - kk);
        if (jj < width) out[(size_t)t * n2 + (size_t)i * N + (j0 + jj)] = tile[jj * LC_RUN_PITCH + kk];
    }
}

// partial[(t LC_RED + r) 4 ...] = (sum out, sum out^2) of workgroup r = blockIdx.x of slice t = blockIdx.y, double-double
__global__ void __launch_bounds__(PS_THREADS) lc_moments_kernel(const double *__restrict__ slices, size_t n2, double *__restrict__ partial)
{
    const double *sl = slices + (size_t)blockIdx.y * n2;
    dd s1 = {0.0, 0.0}, s2 = {0.0, 0.0};
    for (size_t e = (size_t)blockIdx.x * PS_THREADS + threadIdx.x; e < n2; e += (size_t)LC_RED * PS_THREADS) {
#pragma clang fp contract(off)
        const double v = sl[e];
        dd_add(s1, v);
        dd_add(s2, v * v);
    }
    s1 = ps_block_sum(s1);
    s2 = ps_block_sum(s2);
    if (threadIdx.x == 0) {
        double *p = partial + ((size_t)blockIdx.y * LC_RED + blockIdx.x) * 4;
        p[0] = s1.hi; p[1] = s1.lo; p[2] = s2.hi; p[3] = s2.lo;
    }
}

// moments[2 t + q] = the LC_RED partials of slice t in workgroup order; one work item per (t, q)
__global__ void __launch_bounds__(PS_THREADS) lc_moments_fold_kernel(const double *__restrict__ partial, int n_slices, double *__restrict__ moments)
{
    const int e = blockIdx.x * PS_THREADS + threadIdx.x;
    if (e >= 2 * n_slices) return;
    const int t = e >> 1, q = e & 1;
    dd s = {0.0, 0.0};
    for (int r = 0; r < LC_RED; ++r) {
        const double *p = partial + ((size_t)t * LC_RED + r) * 4 + 2 * q;
        dd o = {p[0], p[1]};
        dd_merge(s, o);
    }
    moments[e] = s.hi + s.lo;
}

__global__ void __launch_bounds__(PS_THREADS) lc_refresh_kernel(LcSource s, size_t ncell, double *__restrict__ prev)
{
    const double nbar = s.nbar ? *s.nbar : 1.0;
    const size_t stride = (size_t)gridDim.x * PS_THREADS;
    for (size_t c = (size_t)blockIdx.x * PS_THREADS + threadIdx.x; c < ncell; c += stride) prev[c] = lc_form(s, c, nbar);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
static unsigned lc_blocks(size_t items)
{
    return (unsigned)std::max<size_t>(1, std::min<size_t>(LC_MAX_BLOCKS, (items + PS_THREADS - 1) / PS_THREADS));
}

// plane[0 ... n) cut for los_axis 2: maximal stretches in which consecutive slices take consecutive planes, in pieces of at most
// LC_RUN_MAX; those of LC_RUN_MIN or more become runs, every other slice goes on the list
static void lc_cut_runs(const int32_t *plane, int n, std::vector<int4> &runs, std::vector<int32_t> &list)
{
    int t = 0;
    while (t < n) {
        int len = 1, step = 0;
        if (t + 1 < n && (plane[t + 1] - plane[t] == 1 || plane[t + 1] - plane[t] == -1)) {
            step = plane[t + 1] - plane[t];
            while (t + len < n && len < LC_RUN_MAX && plane[t + len] - plane[t + len - 1] == step) ++len;
        }
        if (len >= LC_RUN_MIN)
            runs.push_back(make_int4(t, len, step > 0 ? plane[t] : plane[t + len - 1], step));
        else
            for (int q = 0; q < len; ++q) list.push_back(t + q);
        t += len;
    }
}

} // namespace asora

using namespace asora;

extern "C" {

int asora_lightcone_advance(int slot, int kind, int src_grid, double t_gamma, int los_axis, int n_slices, const int32_t *plane,
                            const double *w_prev, const double *w_now, int refresh, double *slices_out, double *moments)
{
    clear_error();
    if (int rc = require_init("lightcone_advance")) return rc;
    State &st = state();
    const std::string me("lightcone_advance");
    if (slot < 0 || slot >= ASORA_LC_SLOTS) return fail(3, me + ": slot must be 0 ... " + std::to_string(ASORA_LC_SLOTS - 1));
    if (src_grid < -1 || src_grid >= ASORA_GRID_COUNT) return fail(3, me + ": src_grid must be -1 or a grid selector");
    if (kind < 0 || kind >= ASORA_PS_KINDS || (src_grid >= 0 && kind != 0))
        return fail(3, me + ": kind must be one of ASORA_PS_* (0 with a src_grid)");
    if (los_axis < 0 || los_axis > 2) return fail(3, me + ": los_axis must be 0, 1 or 2");
    if (!std::isfinite(t_gamma) || t_gamma < 0.0) return fail(3, me + ": t_gamma must be finite and >= 0");
    if (n_slices < 0 || n_slices > ASORA_LC_MAX_SLICES)
        return fail(3, me + ": n_slices must be 0 ... " + std::to_string(ASORA_LC_MAX_SLICES));
    if (refresh != 0 && refresh != 1) return fail(3, me + ": refresh must be 0 or 1");
    if (n_slices > 0) {
        if (!plane || !w_prev || !w_now || !moments) return fail(3, me + ": null pointer (plane, w_prev, w_now, moments)");
        for (int t = 0; t < n_slices; ++t) {
            if (plane[t] < 0 || plane[t] >= st.N) return fail(3, me + ": plane[" + std::to_string(t) + "] lies outside [0, N)");
            if (!std::isfinite(w_prev[t]) || !std::isfinite(w_now[t])) return fail(3, me + ": the weights must be finite");
        }
    }
    State::Lightcone &lc = st.lightcone;
    State::Lightcone::Kept &kept = lc.kept[slot];
    const bool has_prev = kept.has && lc.prev[slot];
    if (!has_prev && (n_slices != 0 || refresh != 1))
        return fail(3, me + ": the first call on a slot stores the field: n_slices = 0 and refresh = 1");
    if (has_prev && (kept.kind != kind || kept.src_grid != src_grid))
        return fail(3, me + ": the slot's kept field was made with kind " + std::to_string(kept.kind) + " and src_grid " +
                           std::to_string(kept.src_grid) + " (asora_lightcone_reset forgets it)");
    if (src_grid >= 0) {
        if (!st.grid[src_grid] || !st.grid_valid[src_grid]) return fail(4, me + ": grid " + std::to_string(src_grid) + " holds no data");
    } else {
        for (int g : {ASORA_GRID_XH, ASORA_GRID_NDENS, ASORA_GRID_TEMP})
            if (ps_needs_grid(kind, g, t_gamma) && (!st.grid[g] || !st.grid_valid[g]))
                return fail(4, me + ": grid " + std::to_string(g) + " holds no data");
    }
    if (st.N > ASORA_REGION_MAX_N) return fail(4, me + ": not built for N > " + std::to_string(ASORA_REGION_MAX_N));
    if (n_slices == 0 && !refresh) return 0;                       // (nothing to emit, nothing to keep)

    const int N = st.N;
    const size_t n2 = (size_t)N * N;
    if (int rc = lc.prev[slot].allocate(st.ncell)) return rc;
    if (int rc = lc.params.allocate(LC_P_WORDS)) return rc;
    if (int rc = lc.host.allocate(LC_P_WORDS)) return rc;
    if (n_slices > 0) {
        if (int rc = lc.partial.allocate((size_t)ASORA_LC_MAX_SLICES * LC_RED * 4)) return rc;
        if (int rc = lc.stage.reserve((size_t)n_slices * n2, st.stream)) return rc;
    }
    const bool need_nbar = src_grid < 0 && ps_needs_grid(kind, ASORA_GRID_NDENS, t_gamma);

    double *host = lc.host, *dev = lc.params, *prev = lc.prev[slot], *stage = lc.stage;
    std::vector<int4> runs;
    std::vector<int32_t> list;
    if (n_slices > 0) {
        std::memcpy(host + LC_P_WPREV, w_prev, sizeof(double) * n_slices);
        std::memcpy(host + LC_P_WNOW, w_now, sizeof(double) * n_slices);
        std::memcpy(host + LC_P_PLANE, plane, sizeof(int32_t) * n_slices);
        if (los_axis == 2) {
            lc_cut_runs(plane, n_slices, runs, list);
            if (!list.empty()) std::memcpy(host + LC_P_LIST, list.data(), sizeof(int32_t) * list.size());
            if (!runs.empty()) std::memcpy(host + LC_P_RUNS, runs.data(), sizeof(int4) * runs.size());
        }
        ASORA_HIP_TRY(hipMemcpyAsync(dev, host, sizeof(double) * LC_P_MOMENTS, hipMemcpyHostToDevice, st.stream));
    }
    StageStopwatch<ASORA_LC_STAGES> watch(st.opt[ASORA_OPT_TIMING] != 0, st.stream);
    if (int rc = watch.mark()) return rc;
    LcSource s{kind, st.grid[ASORA_GRID_XH], st.grid[ASORA_GRID_NDENS], st.grid[ASORA_GRID_TEMP],
               src_grid >= 0 ? st.grid[src_grid] : (const double *)nullptr, (const double *)nullptr, t_gamma};
    if (need_nbar)
        if (int rc = ps_mean_density(st, &s.nbar)) return rc;
    if (int rc = watch.mark()) return rc;
    if (n_slices > 0) {
        const int32_t *plane_dev = (const int32_t *)(dev + LC_P_PLANE), *list_dev = (const int32_t *)(dev + LC_P_LIST);
        const double *wp = dev + LC_P_WPREV, *wn = dev + LC_P_WNOW;
        if (los_axis != 2) {
            hipLaunchKernelGGL(lc_emit_kernel, dim3(lc_blocks((size_t)n_slices * n2)), dim3(PS_THREADS), 0, st.stream, s, (const double *)prev,
                               N, los_axis, n_slices, (const int32_t *)nullptr, plane_dev, wp, wn, stage);
            ASORA_HIP_TRY(hipGetLastError());
        } else {
            if (!runs.empty()) {
                hipLaunchKernelGGL(lc_emit_runs_kernel, dim3((unsigned)((N + LC_TILE_J - 1) / LC_TILE_J), (unsigned)N, (unsigned)runs.size()),
                                   dim3(PS_THREADS), 0, st.stream, s, (const double *)prev, N, (const int4 *)(dev + LC_P_RUNS), wp, wn, stage);
                ASORA_HIP_TRY(hipGetLastError());
            }
            if (!list.empty()) {
                hipLaunchKernelGGL(lc_emit_kernel, dim3(lc_blocks(list.size() * n2)), dim3(PS_THREADS), 0, st.stream, s, (const double *)prev,
                                   N, los_axis, (int)list.size(), list_dev, plane_dev, wp, wn, stage);
                ASORA_HIP_TRY(hipGetLastError());
            }
        }
    }
    if (int rc = watch.mark()) return rc;
    if (n_slices > 0) {
        hipLaunchKernelGGL(lc_moments_kernel, dim3(LC_RED, (unsigned)n_slices), dim3(PS_THREADS), 0, st.stream, (const double *)stage, n2,
                           (double *)lc.partial);
        ASORA_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(lc_moments_fold_kernel, dim3((unsigned)((2 * n_slices + PS_THREADS - 1) / PS_THREADS)), dim3(PS_THREADS), 0, st.stream,
                           (const double *)lc.partial, n_slices, dev + LC_P_MOMENTS);
        ASORA_HIP_TRY(hipGetLastError());
    }
    if (int rc = watch.mark()) return rc;
    if (refresh) {
        hipLaunchKernelGGL(lc_refresh_kernel, dim3(lc_blocks(st.ncell)), dim3(PS_THREADS), 0, st.stream, s, st.ncell, prev);
        ASORA_HIP_TRY(hipGetLastError());
        kept.has = true; kept.kind = kind; kept.src_grid = src_grid;
    }
    if (int rc = watch.mark()) return rc;
    if (n_slices > 0) {
        ASORA_HIP_TRY(hipMemcpyAsync(host + LC_P_MOMENTS, dev + LC_P_MOMENTS, sizeof(double) * 2 * n_slices, hipMemcpyDeviceToHost, st.stream));
        if (slices_out)
            ASORA_HIP_TRY(hipMemcpyAsync(slices_out, stage, sizeof(double) * n_slices * n2, hipMemcpyDeviceToHost, st.stream));
    }
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    watch.read(lc.ms);
    if (n_slices > 0) std::memcpy(moments, host + LC_P_MOMENTS, sizeof(double) * 2 * n_slices);
    return 0;
}

int asora_lightcone_state(int slot, int *has_prev, int *kind, int *src_grid)
{
    clear_error();
    if (slot < 0 || slot >= ASORA_LC_SLOTS) return fail(3, "lightcone_state: slot must be 0 ... " + std::to_string(ASORA_LC_SLOTS - 1));
    if (!has_prev || !kind || !src_grid) return fail(3, "lightcone_state: null pointer");
    const State::Lightcone &lc = state().lightcone;
    const bool has = lc.kept[slot].has && lc.prev[slot];
    *has_prev = has ? 1 : 0;
    *kind = has ? lc.kept[slot].kind : 0;
    *src_grid = has ? lc.kept[slot].src_grid : -1;
    return 0;
}

int asora_lightcone_reset(int slot)
{
    clear_error();
    if (slot < 0 || slot >= ASORA_LC_SLOTS) return fail(3, "lightcone_reset: slot must be 0 ... " + std::to_string(ASORA_LC_SLOTS - 1));
    state().lightcone.kept[slot] = {};
    return 0;
}

int asora_debug_lightcone_ms(double *ms)
{
    clear_error();
    if (!ms) return fail(3, "debug_lightcone_ms: null pointer");
    for (int q = 0; q < ASORA_LC_STAGES; ++q) ms[q] = state().lightcone.ms[q];
    return 0;
}

} // extern "C"
