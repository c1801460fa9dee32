// smooth_field.hip -- a field formed from the device grids, filtered in Fourier space and transformed back, with the one-point
// statistics of the result (asora_smooth_field).  The forward half is the power spectrum's (ps_forward,
// power_spectrum.hip: mean density, the pass along k that forms the field, along j, along i); the complex buffer is its buffer,
// transformed in place and overwritten on the way back.  The stages written here, on the library's stream behind those:
//   e. back along i : sm_line_kernel<true>, ps_line_kernel's tiles and strides; on the load into LDS element (n_x, n_y, n_z) is
//                     multiplied by W(n) -- w_i, w_j, w_k staged in LDS behind the line buffers (3 x 8 N bytes), w_r read from global
//                     memory (2.5 MB at most: it stays in L2) -- and conjugated, and the result is conjugated on the store: the
//                     butterflies have the forward sign baked in, and conj(FFT(conj(.))) is the unnormalised inverse.  W is real,
//                     so it commutes with the conjugation;
//   f. back along j : sm_line_kernel<false>, the same without the filter;
//   g. back along k : sm_c2r_kernel, one workgroup per T rows (i, j), the simple form like the forward row pass: it loads the
//                     floor(N/2) + 1 stored values of a row, fills in a[N - n_z] = conj(a[n_z]), drops the imaginary parts of
//                     n_z = 0 and N/2, transforms, and stores Re / N^3 into h; sum h, min, max and the counts of finite and
//                     non-finite cells go to the workgroup's partials, and sm_first_kernel (one workgroup) folds them in index
//                     order and forms mu;
//   h. moments, pdf : sm_moment_kernel reads h a second time on a fixed grid of PS_RED_BLOCKS workgroups: (h - mu)^2, ^3, ^4 into
//                     double-double partials; the histogram by integer LDS atomics per workgroup (the bin by binary search of the
//                     edges in LDS), then one integer global atomic per non-empty bin and workgroup; sm_fold_kernel adds the
//                     partials in index order.
// Every floating-point sum has the order of the power spectrum's moments (per thread in index order, per wave by a shuffle tree, per
// workgroup in wave order, over workgroups in index order), in double-double; only integers are added atomically.
#include "asora_internal.hpp"
#include "fft_device.hpp"

namespace asora {

constexpr int SM_FIRST_WORDS = 6;           // a row workgroup's partials: sum h (hi, lo), min, max, finite cells, non-finite cells (uint64)
constexpr int SM_RES_MU = ASORA_SMOOTH_STATS, SM_RES_HIST = SM_RES_MU + 1, SM_RES_WORDS = SM_RES_HIST + ASORA_SMOOTH_MAX_BINS + 2;

// min and max of (lo, hi) and the sums of (n0, n1) over the workgroup, in lane, then wave order; every thread calls it and gets them
__device__ __forceinline__ void sm_block_range(double &lo, double &hi, unsigned long long &n0, unsigned long long &n1)
{
    __shared__ double sh[2 * PS_WAVES];
    __shared__ unsigned long long shn[2 * PS_WAVES];
    for (int o = 32; o > 0; o >>= 1) {
        lo = fmin(lo, __shfl_down(lo, o));
        hi = fmax(hi, __shfl_down(hi, o));
        n0 += __shfl_down(n0, o);
        n1 += __shfl_down(n1, o);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[2 * wave] = lo; sh[2 * wave + 1] = hi; shn[2 * wave] = n0; shn[2 * wave + 1] = n1; }
    __syncthreads();
    lo = sh[0]; hi = sh[1]; n0 = shn[0]; n1 = shn[1];
    for (int q = 1; q < PS_WAVES; ++q) {
        lo = fmin(lo, sh[2 * q]);
        hi = fmax(hi, sh[2 * q + 1]);
        n0 += shn[2 * q];
        n1 += shn[2 * q + 1];
    }
    __syncthreads();
}

// a strided pass of the inverse, in place, with ps_line_kernel's geometry (power_spectrum.hip): conj on the load, conj on the store.
// FILTER (the pass along i: one block, the columns are (n_y, n_z) flattened, NZ = N / 2 + 1 of n_z each): the element is multiplied
// by W on the load.  Dynamic LDS: roots [N], two line buffers [T pitch]; FILTER: then w_i, w_j, w_k [N] each (ones for a null
// table) and, per column of the tile, n_y, n_z and m_y^2 + m_z^2
template <bool FILTER>
__global__ void __launch_bounds__(PS_THREADS) sm_line_kernel(double2 *__restrict__ modes, int N, int pitch, int T, PsPlan plan,
                                                              const double2 *__restrict__ twiddle, size_t outer_stride, size_t line_stride,
                                                              size_t ncols, unsigned tiles, const double *__restrict__ w_i,
                                                              const double *__restrict__ w_j, const double *__restrict__ w_k,
                                                              const double *__restrict__ w_r, int subtract_mean)
{
    extern __shared__ double2 ps_lds[];
    double2 *tw, *a, *b;
    ps_lds_layout(ps_lds, twiddle, N, pitch, T, tw, a, b);
    const unsigned outer = blockIdx.x / tiles;
    const size_t c0 = (size_t)(blockIdx.x - outer * tiles) * T;
    const int width = (int)(ncols - c0 < (size_t)T ? ncols - c0 : (size_t)T);
    double2 *g = modes + outer * outer_stride + c0;
    if constexpr (FILTER) {
        double *wt = (double *)(b + (size_t)T * pitch);
        int *col = (int *)(wt + 3 * (size_t)N);
        for (int r = threadIdx.x; r < N; r += PS_THREADS) {
            wt[r] = w_i ? w_i[r] : 1.0;
            wt[N + r] = w_j ? w_j[r] : 1.0;
            wt[2 * N + r] = w_k ? w_k[r] : 1.0;
        }
        const int NZ = N / 2 + 1;
        for (int t = threadIdx.x; t < width; t += PS_THREADS) {
            const int c = (int)c0 + t, ny = c / NZ, nz = c - ny * NZ, my = min(ny, N - ny);      // (n_z <= N / 2: its own folded index)
            col[3 * t] = ny; col[3 * t + 1] = nz; col[3 * t + 2] = my * my + nz * nz;
        }
        __syncthreads();
        for (int w = threadIdx.x; w < width * N; w += PS_THREADS) {
#pragma clang fp contract(off)
            const int e = w / width, t = w - e * width, ny = col[3 * t], nz = col[3 * t + 1], mx = min(e, N - e);
            double W = (wt[e] * wt[N + ny]) * wt[2 * N + nz];
            if (w_r) W = W * w_r[mx * mx + col[3 * t + 2]];
            if (subtract_mean && e == 0 && ny == 0 && nz == 0) W = 0.0;
            const double2 v = g[e * line_stride + t];
            a[t * pitch + e] = make_double2(v.x * W, -(v.y * W));
        }
    } else {
        for (int w = threadIdx.x; w < width * N; w += PS_THREADS) {
            const int e = w / width, t = w - e * width;
            const double2 v = g[e * line_stride + t];
            a[t * pitch + e] = make_double2(v.x, -v.y);
        }
    }
    const double2 *res = line_fft(a, b, tw, plan, N, pitch, width);
    for (int w = threadIdx.x; w < width * N; w += PS_THREADS) {
        const int e = w / width, t = w - e * width;
        const double2 v = res[t * pitch + e];
        g[e * line_stride + t] = make_double2(v.x, -v.y);
    }
}

// the pass back along k: workgroup b takes the rows b T ... b T + T - 1 of the N^2 rows (i, j) of the half-space to N real cells each
__global__ void __launch_bounds__(PS_THREADS) sm_c2r_kernel(const double2 *__restrict__ modes, int N, int pitch, int T, PsPlan plan,
                                                             const double2 *__restrict__ twiddle, double *__restrict__ h,
                                                             double *__restrict__ partial)
{
    extern __shared__ double2 ps_lds[];
    double2 *tw, *a, *b;
    ps_lds_layout(ps_lds, twiddle, N, pitch, T, tw, a, b);
    const int NZ = N / 2 + 1;
    const size_t rows = (size_t)N * N, row0 = (size_t)blockIdx.x * T;
    const int nl = (int)(rows - row0 < (size_t)T ? rows - row0 : (size_t)T);
    for (int w = threadIdx.x; w < nl * NZ; w += PS_THREADS) {
        const int t = w / NZ, kz = w - t * NZ;
        const double2 v = modes[(row0 + t) * (size_t)NZ + kz];
        if (kz == 0 || 2 * kz == N) {
            a[t * pitch + kz] = make_double2(v.x, 0.0);        // its own partner: real
        } else {
            a[t * pitch + kz] = make_double2(v.x, -v.y);       // conj of the stored value
            a[t * pitch + N - kz] = v;                         // conj of its partner conj(v)
        }
    }
    const double2 *res = line_fft(a, b, tw, plan, N, pitch, nl);
    const double n3 = (double)N * (double)N * (double)N;
    dd s = {0.0, 0.0};
    double lo = INFINITY, hi = -INFINITY;
    unsigned long long n_fin = 0ull, n_non = 0ull;
    for (int w = threadIdx.x; w < nl * N; w += PS_THREADS) {
        const int t = w / N, k = w - t * N;
        const double v = res[t * pitch + k].x / n3;
        h[(row0 + t) * (size_t)N + k] = v;
        dd_add(s, v);
        if (isfinite(v)) { lo = fmin(lo, v); hi = fmax(hi, v); ++n_fin; } else ++n_non;
    }
    s = ps_block_sum(s);
    sm_block_range(lo, hi, n_fin, n_non);
    if (threadIdx.x == 0) {
        double *p = partial + (size_t)blockIdx.x * SM_FIRST_WORDS;
        p[0] = s.hi; p[1] = s.lo; p[2] = lo; p[3] = hi;
        ((unsigned long long *)p)[4] = n_fin; ((unsigned long long *)p)[5] = n_non;
    }
}

// the row workgroups' partials folded in index order into result[0 ... 3], [6] and mu; [4], [5]: the input's moments; ONE workgroup
__global__ void __launch_bounds__(PS_THREADS) sm_first_kernel(const double *__restrict__ partial, int count, double n3,
                                                               const double *__restrict__ input_moments, double *__restrict__ result)
{
    dd s = {0.0, 0.0};
    double lo = INFINITY, hi = -INFINITY;
    unsigned long long n_fin = 0ull, n_non = 0ull;
    for (int e = threadIdx.x; e < count; e += PS_THREADS) {
        const double *p = partial + (size_t)e * SM_FIRST_WORDS;
        dd o = {p[0], p[1]};
        dd_merge(s, o);
        lo = fmin(lo, p[2]); hi = fmax(hi, p[3]);
        n_fin += ((const unsigned long long *)p)[4]; n_non += ((const unsigned long long *)p)[5];
    }
    s = ps_block_sum(s);
    sm_block_range(lo, hi, n_fin, n_non);
    if (threadIdx.x == 0) {
        const double sum = s.hi + s.lo;
        result[0] = (double)n_fin; result[1] = (double)n_non; result[2] = lo; result[3] = hi;
        result[4] = input_moments[0]; result[5] = input_moments[1];
        result[6] = sum;
        result[SM_RES_MU] = sum / n3;
    }
}

// partial[6 b ...] = the double-double sums of (h - mu)^2, ^3, ^4 over the cells of workgroup b (grid-stride; the grid is
// PS_RED_BLOCKS); hist[...] += the workgroup's counts.  Dynamic LDS: edges [n_hist + 1], then uint32 counts [n_hist + 2]
__global__ void __launch_bounds__(PS_THREADS) sm_moment_kernel(const double *__restrict__ h, size_t n, const double *__restrict__ mu_dev,
                                                                int n_hist, const double *__restrict__ edges, double *__restrict__ partial,
                                                                unsigned long long *__restrict__ hist)
{
    extern __shared__ double sm_lds[];
    double *edge = sm_lds;
    unsigned *cnt = (unsigned *)(sm_lds + n_hist + 1);
    if (n_hist > 0) {
        for (int q = threadIdx.x; q <= n_hist; q += PS_THREADS) edge[q] = edges[q];
        for (int q = threadIdx.x; q < n_hist + 2; q += PS_THREADS) cnt[q] = 0u;
    }
    __syncthreads();
    const double mu = *mu_dev;
    dd s2 = {0.0, 0.0}, s3 = {0.0, 0.0}, s4 = {0.0, 0.0};
    const size_t stride = (size_t)gridDim.x * PS_THREADS;
    for (size_t c = (size_t)blockIdx.x * PS_THREADS + threadIdx.x; c < n; c += stride) {
#pragma clang fp contract(off)
        const double v = h[c], d = v - mu, d2 = d * d;
        dd_add(s2, d2);
        dd_add(s3, d2 * d);
        dd_add(s4, d2 * d2);
        if (n_hist > 0 && isfinite(v)) {
            int slot;
            if (v < edge[0]) slot = n_hist;
            else if (v >= edge[n_hist]) slot = n_hist + 1;
            else {
                int lo = 0, hi = n_hist;                           // edge[lo] <= v < edge[hi]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (edge[mid] <= v) lo = mid; else hi = mid;
                }
                slot = lo;
            }
            atomicAdd(&cnt[slot], 1u);
        }
    }
    s2 = ps_block_sum(s2);
    s3 = ps_block_sum(s3);
    s4 = ps_block_sum(s4);
    if (threadIdx.x == 0) {
        double *p = partial + (size_t)blockIdx.x * 6;
        p[0] = s2.hi; p[1] = s2.lo; p[2] = s3.hi; p[3] = s3.lo; p[4] = s4.hi; p[5] = s4.lo;
    }
    if (n_hist > 0)
        for (int q = threadIdx.x; q < n_hist + 2; q += PS_THREADS)
            if (cnt[q]) atomicAdd(&hist[q], (unsigned long long)cnt[q]);
}

// out[q] = the sum over e < count of the double-double partial[(e ncomp + q) 2 ...], q < ncomp, in index order; ONE workgroup
__global__ void __launch_bounds__(PS_THREADS) sm_fold_kernel(const double *__restrict__ partial, int count, int ncomp, double *__restrict__ out)
{
    for (int q = 0; q < ncomp; ++q) {
        dd s = {0.0, 0.0};
        for (int e = threadIdx.x; e < count; e += PS_THREADS) {
            const double *p = partial + ((size_t)e * ncomp + q) * 2;
            dd o = {p[0], p[1]};
            dd_merge(s, o);
        }
        s = ps_block_sum(s);
        if (threadIdx.x == 0) out[q] = s.hi + s.lo;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// the doubles of sm_tables (and of the pinned area behind its SM_RES_WORDS result words): w_i, w_j, w_k, w_r, the edges
struct SmLayout {
    size_t n_r, w[3], w_r, edges, words, row_blocks, first, moments, partial_words;
    explicit SmLayout(int N, int T)
    {
        n_r = 3 * (size_t)(N / 2) * (size_t)(N / 2) + 1;
        w[0] = 0; w[1] = (size_t)N; w[2] = 2 * (size_t)N;
        w_r = 3 * (size_t)N;
        edges = w_r + n_r;
        words = edges + ASORA_SMOOTH_MAX_BINS + 1;
        row_blocks = ((size_t)N * N + T - 1) / T;
        first = 0;
        moments = first + SM_FIRST_WORDS * row_blocks;
        partial_words = moments + 6 * (size_t)PS_RED_BLOCKS;
    }
};

static int ensure_sm_buffers(State &st, const SmLayout &lay, bool own_field)
{
    if (own_field) { if (int rc = st.smoothing.field.allocate(st.ncell)) return rc; }
    if (int rc = st.smoothing.tables.allocate(lay.words)) return rc;
    if (int rc = st.smoothing.partial.allocate(lay.partial_words)) return rc;
    if (int rc = st.smoothing.result.allocate(SM_RES_WORDS)) return rc;
    if (int rc = st.smoothing.host.allocate((SM_RES_WORDS + lay.words))) return rc;
    return 0;
}

static bool all_finite(const double *v, size_t n)
{
    for (size_t q = 0; q < n; ++q)
        if (!std::isfinite(v[q])) return false;
    return true;
}

} // namespace asora

using namespace asora;

extern "C" {

int asora_smooth_field(int kind, double scale, double t_gamma, const double *w_i, const double *w_j, const double *w_k, const double *w_r,
                       unsigned n_r, int subtract_mean, int n_hist, const double *edges, int dst_grid, double *stats, uint64_t *hist,
                       double *field_out)
{
    clear_error();
    if (int rc = require_init("smooth_field")) return rc;
    State &st = state();
    const int N = st.N;
    if (kind < 0 || kind >= ASORA_PS_KINDS) return fail(3, "smooth_field: kind must be one of ASORA_PS_*");
    if (!std::isfinite(scale)) return fail(3, "smooth_field: scale must be finite");
    if (!std::isfinite(t_gamma) || t_gamma < 0.0) return fail(3, "smooth_field: t_gamma must be finite and >= 0");
    const double *sep[3] = {w_i, w_j, w_k};
    for (int q = 0; q < 3; ++q) {
        if (!sep[q]) continue;
        if (!all_finite(sep[q], (size_t)N)) return fail(3, std::string("smooth_field: w_") + "ijk"[q] + " has a non-finite entry");
        if (q < 2)
            for (int n = 1; n < N; ++n)
                if (std::memcmp(sep[q] + n, sep[q] + N - n, sizeof(double)) != 0)
                    return fail(3, std::string("smooth_field: w_") + "ij"[q] + "[n] must equal w[N - n] bit for bit (the output would not be real)");
    }
    const size_t want_r = 3 * (size_t)(N / 2) * (size_t)(N / 2) + 1;
    if (w_r) {
        if ((size_t)n_r != want_r) return fail(3, "smooth_field: w_r must have 3 floor(N/2)^2 + 1 = " + std::to_string(want_r) + " entries");
        if (!all_finite(w_r, want_r)) return fail(3, "smooth_field: w_r has a non-finite entry");
    }
    if (n_hist < 0 || n_hist > ASORA_SMOOTH_MAX_BINS)
        return fail(3, "smooth_field: n_hist must be in [0, " + std::to_string(ASORA_SMOOTH_MAX_BINS) + "]");
    if (n_hist > 0) {
        if (!edges || !hist) return fail(3, "smooth_field: null edges or hist with n_hist > 0");
        if (!all_finite(edges, (size_t)n_hist + 1)) return fail(3, "smooth_field: the edges must be finite");
        for (int b = 0; b < n_hist; ++b)
            if (!(edges[b] < edges[b + 1])) return fail(3, "smooth_field: the edges must strictly ascend");
    }
    if (dst_grid < -1 || dst_grid >= ASORA_GRID_COUNT) return fail(3, "smooth_field: dst_grid must be -1 or a grid selector");
    if (!stats) return fail(3, "smooth_field: null stats");
    const int grids[3] = {ASORA_GRID_XH, ASORA_GRID_NDENS, ASORA_GRID_TEMP};
    for (int q = 0; q < 3; ++q)
        if (ps_needs_grid(kind, grids[q], t_gamma) && (!st.grid[grids[q]] || !st.grid_valid[grids[q]]))
            return fail(4, "smooth_field: grid " + std::to_string(grids[q]) + " holds no data");
    if (N > ASORA_REGION_MAX_N)
        return fail(4, "smooth_field: not built for N > " + std::to_string(ASORA_REGION_MAX_N) + " (a line and its roots must fit LDS)");

    const int NZ = N / 2 + 1, T = ps_tile(N), pitch = N | 1;
    const size_t ncell = st.ncell;
    const SmLayout lay(N, T);
    const PsPlan plan = ps_plan(N);
    if (int rc = ensure_sm_buffers(st, lay, dst_grid < 0)) return rc;
    if (dst_grid >= 0)
        if (int rc = ensure_optional_grid(dst_grid)) return rc;
    double *h = dst_grid >= 0 ? st.grid[dst_grid] : st.smoothing.field;

    const size_t fft_lds = ((size_t)2 * T * pitch + N) * sizeof(double2);
    const size_t filter_lds = fft_lds + 3 * (size_t)N * sizeof(double) + 3 * (size_t)T * sizeof(int);
    const size_t hist_lds = n_hist > 0 ? sizeof(double) * ((size_t)n_hist + 1) + sizeof(unsigned) * ((size_t)n_hist + 2) : sizeof(double);
    ASORA_HIP_TRY(hipFuncSetAttribute((const void *)sm_line_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)filter_lds));
    ASORA_HIP_TRY(hipFuncSetAttribute((const void *)sm_line_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fft_lds));
    ASORA_HIP_TRY(hipFuncSetAttribute((const void *)sm_c2r_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fft_lds));
    ASORA_HIP_TRY(hipFuncSetAttribute((const void *)sm_moment_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hist_lds));

    // the tables and the edges leave the host through the pinned area, one copy each
    double *stage = st.smoothing.host + SM_RES_WORDS, *tab = st.smoothing.tables;
    auto upload = [&](const double *src, size_t at, size_t n) -> int {
        std::memcpy(stage + at, src, sizeof(double) * n);
        ASORA_HIP_TRY(hipMemcpyAsync(tab + at, stage + at, sizeof(double) * n, hipMemcpyHostToDevice, st.stream));
        return 0;
    };
    for (int q = 0; q < 3; ++q)
        if (sep[q])
            if (int rc = upload(sep[q], lay.w[q], (size_t)N)) return rc;
    if (w_r)
        if (int rc = upload(w_r, lay.w_r, want_r)) return rc;
    if (n_hist > 0)
        if (int rc = upload(edges, lay.edges, (size_t)n_hist + 1)) return rc;
    double *res = st.smoothing.result, *part = st.smoothing.partial;
    unsigned long long *hist_dev = (unsigned long long *)(res + SM_RES_HIST);
    if (n_hist > 0) ASORA_HIP_TRY(hipMemsetAsync(hist_dev, 0, sizeof(unsigned long long) * ((size_t)n_hist + 2), st.stream));

    const dim3 block(PS_THREADS);
    StageStopwatch<ASORA_SMOOTH_STAGES> watch(st.opt[ASORA_OPT_TIMING] != 0, st.stream);
    if (int rc = watch.mark()) return rc;
    const double *input_moments = nullptr;
    if (int rc = ps_forward(st, kind, scale, t_gamma, [&watch]() { return watch.mark(); }, &input_moments)) return rc;

    double2 *modes = st.spectrum.modes[0];
    const double2 *twiddle = st.spectrum.twiddle;
    const unsigned tiles_j = (unsigned)((NZ + T - 1) / T), tiles_i = (unsigned)(((size_t)N * NZ + T - 1) / T);
    hipLaunchKernelGGL(sm_line_kernel<true>, dim3(tiles_i), block, filter_lds, st.stream, modes, N, pitch, T, plan, twiddle, (size_t)0,
                       (size_t)N * NZ, (size_t)N * NZ, tiles_i, w_i ? (const double *)(tab + lay.w[0]) : (const double *)nullptr,
                       w_j ? (const double *)(tab + lay.w[1]) : (const double *)nullptr,
                       w_k ? (const double *)(tab + lay.w[2]) : (const double *)nullptr,
                       w_r ? (const double *)(tab + lay.w_r) : (const double *)nullptr, subtract_mean ? 1 : 0);
    ASORA_HIP_TRY(hipGetLastError());
    if (int rc = watch.mark()) return rc;
    hipLaunchKernelGGL(sm_line_kernel<false>, dim3((unsigned)N * tiles_j), block, fft_lds, st.stream, modes, N, pitch, T, plan, twiddle,
                       (size_t)N * NZ, (size_t)NZ, (size_t)NZ, tiles_j, (const double *)nullptr, (const double *)nullptr,
                       (const double *)nullptr, (const double *)nullptr, 0);
    ASORA_HIP_TRY(hipGetLastError());
    if (int rc = watch.mark()) return rc;
    hipLaunchKernelGGL(sm_c2r_kernel, dim3((unsigned)lay.row_blocks), block, fft_lds, st.stream, (const double2 *)modes, N, pitch, T, plan,
                       twiddle, h, part + lay.first);
    ASORA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sm_first_kernel, dim3(1), block, 0, st.stream, (const double *)(part + lay.first), (int)lay.row_blocks, (double)ncell,
                       input_moments, res);
    ASORA_HIP_TRY(hipGetLastError());
    if (int rc = watch.mark()) return rc;
    hipLaunchKernelGGL(sm_moment_kernel, dim3(PS_RED_BLOCKS), block, hist_lds, st.stream, (const double *)h, ncell,
                       (const double *)(res + SM_RES_MU), n_hist, (const double *)(tab + lay.edges), part + lay.moments, hist_dev);
    ASORA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sm_fold_kernel, dim3(1), block, 0, st.stream, (const double *)(part + lay.moments), PS_RED_BLOCKS, 3, res + 7);
    ASORA_HIP_TRY(hipGetLastError());
    if (int rc = watch.mark()) return rc;
    if (dst_grid >= 0) {                                           // (as asora_grid_to_device leaves a grid)
        st.grid_valid[dst_grid] = true;
        st.zero.verdict.since_probe = std::max(st.zero.verdict.since_probe, 48);
        if (dst_grid == ASORA_GRID_TEMP) st.temp_probe.valid = false;
    }

    const size_t res_words = (size_t)SM_RES_HIST + (n_hist > 0 ? (size_t)n_hist + 2 : 0);
    ASORA_HIP_TRY(hipMemcpyAsync(st.smoothing.host, res, sizeof(double) * res_words, hipMemcpyDeviceToHost, st.stream));
    if (field_out) ASORA_HIP_TRY(hipMemcpyAsync(field_out, h, sizeof(double) * ncell, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    watch.read(st.smoothing.ms);

    std::memcpy(stats, st.smoothing.host, sizeof(double) * ASORA_SMOOTH_STATS);
    if (n_hist > 0) std::memcpy(hist, st.smoothing.host + SM_RES_HIST, sizeof(uint64_t) * ((size_t)n_hist + 2));
    return 0;
}

int asora_debug_smooth_field_ms(double *ms)
{
    clear_error();
    if (!ms) return fail(3, "debug_smooth_field_ms: null pointer");
    for (int q = 0; q < ASORA_SMOOTH_STAGES; ++q) ms[q] = state().smoothing.ms[q];
    return 0;
}

} // extern "C"
