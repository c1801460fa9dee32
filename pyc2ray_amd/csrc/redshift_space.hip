// redshift_space.hip -- the field of the power spectrum moved into redshift space along one axis by the line-of-sight velocity, and
// its power binned in two dimensions with Legendre-weighted sums (asora_los_velocity_to_device, asora_redshift_space_field,
// asora_power_spectrum_los).  The transform, the forming of the field and the double-double sums are the
// power spectrum's (fft_device.hpp; ps_mean_density and ps_transform of power_spectrum.hip).  The stages written here:
//   v. velocity     : rs_vmax_kernel, max |v| over the uploaded buffer as the maximum of the bit patterns of |v| (an integer maximum:
//                     any order gives the same bits, and a NaN or an infinity has a larger pattern than every finite value, so the
//                     same pass catches them);
//   m. mapping      : rs_map_kernel, one workgroup per tile of T lines along los_axis: g (formed from the grids) and u = v
//                     velocity_scale of the tile go into LDS, the edge displacements d are formed there, and every work item gathers
//                     one output cell over the 2 W + 1 source cells that can reach it, in the order of the specification: no scatter,
//                     no atomic.  For los_axis = 2 a tile is T contiguous rows (48 KiB of LDS, 256 work items); for the axes 0 and 1
//                     it is T adjacent columns of the contiguous index, with ps_line_kernel's strides, T = 16 (fragments of 128
//                     bytes) where three real lines per column fit LDS (N <= 415) and 8 beyond, and 1024 work items: such a tile
//                     leaves room for one workgroup on a CU at 256^3, and sixteen waves keep the loads in flight that four did
//                     not (DESIGN.md 4.2j has both timings).  The result is staged in LDS (in the place of u) and stored in the
//                     order of the loads.  Each cell of g is formed by exactly one workgroup, which also adds g and g^2 to its
//                     partial moments.  Reads and writes of a workgroup touch its own lines only, and every read is behind a
//                     barrier before the first write: the output may be a grid the kind reads;
//   n. binning      : rs_bin_kernel<MODE>, ps_bin_kernel's scheme with two bin indices: one workgroup per plane i, a wave takes 64
//                     consecutive n_z of one row, along which each of the two indices is monotone, so every two-dimensional bin is
//                     seen in one maximal run; runs are reduced by a segmented scan in lane order and the last lane of a run adds
//                     into the wave's own LDS histogram.  Six values per bin: with n_a n_b <= 512 the workgroup has four waves and
//                     four histograms, beyond that two of each (96 KiB), so the LDS need never passes 111 KiB.  The waves'
//                     histograms are combined in wave order into the plane's partial row, rs_bin_final_kernel adds the planes in
//                     plane order.
// Every floating-point sum has an order fixed by (N, los_axis, mode, thresholds); no floating-point atomic anywhere.
#include "asora_internal.hpp"
#include "fft_device.hpp"

namespace asora {

constexpr int RS_VALUES = 6;                // per bin: count, sum_1, sum_2, sum_aa, sum_l2, sum_l4
constexpr int RS_COUNT = 0, RS_SUM_1 = 1, RS_SUM_2 = 2, RS_SUM_AA = 3, RS_SUM_L2 = 4, RS_SUM_L4 = 5;
constexpr int RS_RES_BINS = 4;              // the result words: sum g, sum g^2, sum h, sum h^2, then [RS_VALUES][n_a n_b]
constexpr int RS_RES_WORDS = RS_RES_BINS + RS_VALUES * ASORA_ANISO_MAX_BINS;
constexpr int RS_THR_B = 0, RS_THR_A = ASORA_ANISO_MAX_BINS + 1;                     // (doubles) thr_b, then thr_a as uint32
constexpr int RS_THR_WORDS = RS_THR_A + (ASORA_ANISO_MAX_BINS + 2) / 2;
constexpr unsigned long long RS_INF_BITS = 0x7FF0000000000000ull;
// the mapping's workgroups: 256 work items on tiles of rows, three of which fit a CU; 1024 on tiles of 16 columns, whose LDS leaves
// room for one workgroup on a CU beyond N = 212, so that the waves which hide the latency of its loads come from the workgroup's
// size (measured both ways at 256^3)
constexpr int RS_MAP_THREADS_ROWS = 256, RS_MAP_THREADS_COLUMNS = 1024, RS_MAP_MAX_WAVES = RS_MAP_THREADS_COLUMNS / 64;

// ps_block_sum for a workgroup of blockDim.x work items: the sum of v in lane, then wave order; every thread calls it and gets the result
__device__ __forceinline__ dd rs_map_block_sum(dd v)
{
    __shared__ double sh[2 * RS_MAP_MAX_WAVES];
    for (int o = 32; o > 0; o >>= 1) {
        dd other;
        other.hi = __shfl_down(v.hi, o);
        other.lo = __shfl_down(v.lo, o);
        dd_merge(v, other);
    }
    if ((threadIdx.x & 63) == 0) { sh[2 * (threadIdx.x >> 6)] = v.hi; sh[2 * (threadIdx.x >> 6) + 1] = v.lo; }
    __syncthreads();
    dd r = {sh[0], sh[1]};
    for (int q = 1; q < (int)(blockDim.x >> 6); ++q) {
        dd o = {sh[2 * q], sh[2 * q + 1]};
        dd_merge(r, o);
    }
    __syncthreads();
    return r;
}

// *out = max over the cells of the bit pattern of |v| (out zeroed beforehand)
__global__ void __launch_bounds__(PS_THREADS) rs_vmax_kernel(const double *__restrict__ v, size_t n, unsigned long long *__restrict__ out)
{
    unsigned long long m = 0ull;
    const size_t stride = (size_t)gridDim.x * PS_THREADS;
    for (size_t c = (size_t)blockIdx.x * PS_THREADS + threadIdx.x; c < n; c += stride) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(v[c]) & 0x7FFFFFFFFFFFFFFFull;
        m = b > m ? b : m;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_down(m, o);
        m = other > m ? other : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// The mapping.  Workgroup b takes `width` <= T lines; cell e of its line t is base + t t_stride + e e_stride:
//   contiguous (los_axis 2): the rows b T ... of the N^2 rows, t_stride = N, e_stride = 1;
//   else                   : block b / tiles of outer_stride cells, the columns (b mod tiles) T ... of its ncols, t_stride = 1,
//                            e_stride = line_stride.
// v = NULL: h = g.  Dynamic LDS: g, u (later h), d, [T pitch] doubles each.  x, n, temp and h may alias: no __restrict__ on them
__global__ void __launch_bounds__(RS_MAP_THREADS_COLUMNS) rs_map_kernel(int kind, const double *x, const double *n, const double *temp,
                                                             const double *__restrict__ nbar_dev, double scale, double t_gamma,
                                                             const double *__restrict__ v, double vscale, int W, int N, int pitch, int T,
                                                             int contiguous, size_t outer_stride, size_t line_stride, size_t ncols,
                                                             unsigned tiles, double *h, double *__restrict__ moment_partial)
{
    extern __shared__ double rs_lds[];
    double *G = rs_lds, *U = G + (size_t)T * pitch, *D = U + (size_t)T * pitch;
    size_t base, t_stride, e_stride;
    int width;
    if (contiguous) {
        const size_t rows = (size_t)N * N, row0 = (size_t)blockIdx.x * T;
        width = (int)(rows - row0 < (size_t)T ? rows - row0 : (size_t)T);
        base = row0 * N; t_stride = (size_t)N; e_stride = 1;
    } else {
        const unsigned outer = blockIdx.x / tiles;
        const size_t c0 = (size_t)(blockIdx.x - outer * tiles) * T;
        width = (int)(ncols - c0 < (size_t)T ? ncols - c0 : (size_t)T);
        base = outer * outer_stride + c0; t_stride = 1; e_stride = line_stride;
    }
    const int items = width * N, threads = blockDim.x;
    const double nbar = nbar_dev ? *nbar_dev : 1.0;
    dd s1 = {0.0, 0.0}, s2 = {0.0, 0.0};
    for (int w = threadIdx.x; w < items; w += threads) {
#pragma clang fp contract(off)
        int t, e;
        if (contiguous) { t = w / N; e = w - t * N; } else { e = w / width; t = w - e * width; }
        const size_t c = base + t * t_stride + e * e_stride;
        const double g = ps_form(kind, c, x, n, temp, nbar, scale, t_gamma);
        G[t * pitch + e] = g;
        if (v) U[t * pitch + e] = v[c] * vscale;
        dd_add(s1, g);
        dd_add(s2, g * g);
    }
    s1 = rs_map_block_sum(s1);                  // (its barriers also put G and U behind the loads)
    s2 = rs_map_block_sum(s2);
    if (threadIdx.x == 0) {
        double *p = moment_partial + (size_t)blockIdx.x * 4;
        p[0] = s1.hi; p[1] = s1.lo; p[2] = s2.hi; p[3] = s2.lo;
    }
    const double *out = G;
    if (v) {
        for (int w = threadIdx.x; w < items; w += threads) {
#pragma clang fp contract(off)
            const int t = w / N, q = w - t * N, qm = q == 0 ? N - 1 : q - 1;
            D[t * pitch + q] = 0.5 * (U[t * pitch + qm] + U[t * pitch + q]);
        }
        __syncthreads();
        for (int w = threadIdx.x; w < items; w += threads) {
#pragma clang fp contract(off)
            const int t = w / N, p = w - t * N;
            const double *g = G + t * pitch, *d = D + t * pitch;
            double sum = 0.0;
            for (int o = -W; o <= W; ++o) {                        // (2 W + 1 <= N: q stays within one period of p)
                int q = p - o;
                q = q < 0 ? q + N : q;
                q = q >= N ? q - N : q;
                const int q1 = q + 1 == N ? 0 : q + 1;
                const double a = d[q], b = 1.0 + d[q1];
                const double lo = b < a ? b : a, hi = b < a ? a : b, wd = hi - lo, od = (double)o;
                double wgt;
                if (wd >= 0.0009765625) {                          // 2^-10
                    const double top = od + 1.0, r = hi < top ? hi : top, l = lo > od ? lo : od, ov = r - l;
                    wgt = ov > 0.0 ? ov / wd : 0.0;
                } else
                    wgt = od == floor(0.5 * (lo + hi)) ? 1.0 : 0.0;
                sum = sum + wgt * g[q];
            }
            U[t * pitch + p] = sum;                                // (u is dead: d holds what the gather needs of it)
        }
        __syncthreads();
        out = U;
    }
    for (int w = threadIdx.x; w < items; w += threads) {
        int t, e;
        if (contiguous) { t = w / N; e = w - t * N; } else { e = w / width; t = w - e * width; }
        h[base + t * t_stride + e * e_stride] = out[t * pitch + e];
    }
}

// out[q] = the sum over e < count of the double-double partial[(e ncomp + q) 2 ...], q < ncomp, in index order; ONE workgroup
__global__ void __launch_bounds__(PS_THREADS) rs_fold_kernel(const double *__restrict__ partial, int count, int ncomp, double *__restrict__ out)
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

// v summed over the lanes start ... lane of the caller's run, in the order of a Hillis-Steele scan
template <typename V> __device__ __forceinline__ V rs_run_scan(V v, int lane, int start)
{
    for (int d = 1; d < 64; d <<= 1) {
        const V up = __shfl_up(v, d);
        if (lane - d >= start) v += up;
    }
    return v;
}

// partial[(plane RS_VALUES + q) nb + b] = value q of the two-dimensional bin b = ia n_b + ib summed over the stored modes of plane
// i = blockIdx.x, nb = n_a n_b.  blockDim.x / 64 waves; dynamic LDS: a histogram [RS_VALUES][nb] of 8-byte words per wave, then
// thr_b [n_b + 1] (doubles), then thr_a [n_a + 1]
template <int MODE>
__global__ void __launch_bounds__(PS_THREADS) rs_bin_kernel(const double2 *__restrict__ A, int N, int axis, int n_a, int n_b,
                                                             const unsigned *__restrict__ thr_a, const double *__restrict__ thr_b,
                                                             double *__restrict__ partial)
{
    extern __shared__ double rs_hist[];
    const int nb = n_a * n_b, waves = blockDim.x >> 6, threads = blockDim.x;
    double *tb = rs_hist + (size_t)waves * RS_VALUES * nb;
    unsigned *ta = (unsigned *)(tb + n_b + 1);
    for (int q = threadIdx.x; q < waves * RS_VALUES * nb; q += threads) rs_hist[q] = 0.0;       // (+0.0 is the integer 0 too)
    for (int q = threadIdx.x; q <= n_b; q += threads) tb[q] = thr_b[q];
    for (int q = threadIdx.x; q <= n_a; q += threads) ta[q] = thr_a[q];
    __syncthreads();
    const int NZ = N / 2 + 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = blockIdx.x;
    const unsigned mi = (unsigned)min(i, N - i);
    volatile double *hist = rs_hist + (size_t)wave * RS_VALUES * nb;
    volatile unsigned long long *hist_n = (volatile unsigned long long *)hist;
    for (int j = wave; j < N; j += waves) {
        const unsigned mj = (unsigned)min(j, N - j);
        const double2 *ra = A + ((size_t)i * N + j) * NZ;
        for (int kz0 = 0; kz0 < NZ; kz0 += 64) {
#pragma clang fp contract(off)
            const int kz = kz0 + lane;
            const bool stored = kz < NZ;
            const unsigned mk = (unsigned)kz, mp = axis == 0 ? mi : axis == 1 ? mj : mk;
            const unsigned n2 = mi * mi + mj * mj + mk * mk, mp2 = mp * mp, nperp2 = n2 - mp2;
            const bool binned = stored && n2 != 0u;
            const double n2d = binned ? (double)n2 : 1.0, mp2d = (double)mp2;
            // each index: (the first threshold above the key) - 1; along the lanes each is monotone, in one direction or the other
            int bin = -1;
            if (binned) {
                const unsigned key = MODE == ASORA_ANISO_CYLINDRICAL ? nperp2 : n2;
                int lo = 0, hi = n_a + 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (ta[mid] <= key) lo = mid + 1; else hi = mid;
                }
                const int ia = lo - 1;
                lo = 0; hi = n_b + 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const double edge = MODE == ASORA_ANISO_CYLINDRICAL ? tb[mid] : tb[mid] * n2d;
                    if (edge <= mp2d) lo = mid + 1; else hi = mid;
                }
                const int ib = lo - 1;
                if (ia >= 0 && ia < n_a && ib >= 0 && ib < n_b) bin = ia * n_b + ib;
            }
            double wgt = 0.0, s1 = 0.0, s2 = 0.0, aa = 0.0, l2 = 0.0, l4 = 0.0;
            if (binned) {
                wgt = (kz == 0 || 2 * kz == N) ? 1.0 : 2.0;
                const double t = mp2d / n2d;
                if (MODE == ASORA_ANISO_CYLINDRICAL) { s1 = wgt * sqrt((double)nperp2); s2 = wgt * (double)mp; }
                else { s1 = wgt * sqrt(n2d); s2 = wgt * sqrt(t); }
                const double2 za = ra[kz];
                aa = wgt * fma(za.x, za.x, za.y * za.y);
                l2 = aa * (0.5 * (3.0 * t - 1.0));
                l4 = aa * (0.125 * ((35.0 * t - 30.0) * t + 3.0));
            }
            const int before = __shfl_up(bin, 1);
            const unsigned long long heads = __ballot(lane == 0 || bin != before);
            const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
            const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
            const unsigned long long cnt = rs_run_scan((unsigned long long)wgt, lane, start);
            s1 = rs_run_scan(s1, lane, start);
            s2 = rs_run_scan(s2, lane, start);
            aa = rs_run_scan(aa, lane, start);
            l2 = rs_run_scan(l2, lane, start);
            l4 = rs_run_scan(l4, lane, start);
            if (last && bin >= 0) {                                // (one lane per bin in this instruction: runs are maximal)
                hist_n[RS_COUNT * nb + bin] += cnt;
                hist[RS_SUM_1 * nb + bin] += s1;
                hist[RS_SUM_2 * nb + bin] += s2;
                hist[RS_SUM_AA * nb + bin] += aa;
                hist[RS_SUM_L2 * nb + bin] += l2;
                hist[RS_SUM_L4 * nb + bin] += l4;
            }
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < RS_VALUES * nb; q += threads) {
        double *out = partial + (size_t)i * RS_VALUES * nb + q;
        if (q < nb) {
            unsigned long long s = 0ull;
            for (int u = 0; u < waves; ++u) s += ((const unsigned long long *)rs_hist)[(size_t)u * RS_VALUES * nb + q];
            *(unsigned long long *)out = s;
        } else {
            double s = rs_hist[q];
            for (int u = 1; u < waves; ++u) s += rs_hist[(size_t)u * RS_VALUES * nb + q];
            *out = s;
        }
    }
}

// result[q nb + b] = the planes' partial rows added in plane order, q < RS_VALUES
__global__ void __launch_bounds__(PS_THREADS) rs_bin_final_kernel(const double *__restrict__ partial, int N, int nb, double *__restrict__ result)
{
    const int t = blockIdx.x * PS_THREADS + threadIdx.x;
    if (t >= RS_VALUES * nb) return;
    if (t < nb) {
        unsigned long long s = 0ull;
        for (int i = 0; i < N; ++i) s += ((const unsigned long long *)partial)[(size_t)i * RS_VALUES * nb + t];
        ((unsigned long long *)result)[t] = s;
    } else {
        double s = 0.0;
        for (int i = 0; i < N; ++i) s += partial[(size_t)i * RS_VALUES * nb + t];
        result[t] = s;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// the words of rs_partial: [bins: N RS_VALUES MAX_BINS | the mapping's moments: 4 per workgroup, N^2 at the most | results]
struct RsLayout {
    size_t bins, moments, result, words;
    explicit RsLayout(int N)
    {
        bins = 0;
        moments = bins + (size_t)N * RS_VALUES * ASORA_ANISO_MAX_BINS;
        result = moments + 4 * (size_t)N * N;
        words = result + RS_RES_WORDS;
    }
};

// lines per workgroup of the mapping: rows of los_axis 2 to 48 KiB (three workgroups per CU; 128 rows at the most); columns of the
// other axes 16, or 8 where 16 columns of three lines do not fit the 160 KiB of a CU (N > 415)
static int rs_tile(int N, bool contiguous)
{
    const size_t line = 3 * (size_t)(N | 1) * sizeof(double);
    if (contiguous) return (int)std::max<size_t>(1, std::min<size_t>(128, (size_t)48 * 1024 / line));
    return 16 * line <= (size_t)156 * 1024 ? 16 : 8;
}

static int ensure_rs_buffers(State &st, bool own_field)
{
    const RsLayout lay(st.N);
    if (own_field) { if (int rc = st.smoothing.field.allocate(st.ncell)) return rc; }
    if (int rc = st.redshift.partial.allocate(lay.words)) return rc;
    if (int rc = st.redshift.thresholds.allocate(RS_THR_WORDS)) return rc;
    if (int rc = st.redshift.host.allocate((RS_RES_WORDS + RS_THR_WORDS))) return rc;
    return 0;
}

// what the two entries check alike, in the order of the header: 3 for a bad argument, then 4 for the grids and the mesh; *W: the
// half-width of the window
static int rs_check(const char *who, State &st, int kind, double scale, double t_gamma, int los_axis, int use_velocity,
                    double velocity_scale, int *W)
{
    const std::string me(who);
    if (kind < 0 || kind >= ASORA_PS_KINDS) return fail(3, me + ": kind must be one of ASORA_PS_*");
    if (!std::isfinite(scale)) return fail(3, me + ": scale must be finite");
    if (!std::isfinite(t_gamma) || t_gamma < 0.0) return fail(3, me + ": t_gamma must be finite and >= 0");
    if (los_axis < 0 || los_axis > 2) return fail(3, me + ": los_axis must be 0, 1 or 2");
    *W = 0;
    if (use_velocity) {
        if (!std::isfinite(velocity_scale)) return fail(3, me + ": velocity_scale must be finite");
        if (!st.redshift.velocity) return fail(3, me + ": use_velocity without a velocity on the device (asora_los_velocity_to_device)");
        const double w = std::floor(st.redshift.vmax * std::fabs(velocity_scale)) + 1.0;
        if (!(2.0 * w + 1.0 <= (double)st.N))
            return fail(3, me + ": the window of 2 W + 1 cells, W = floor(max|v| |velocity_scale|) + 1, is wider than the N = " +
                               std::to_string(st.N) + " cells of a line");
        *W = (int)w;
    }
    return 0;
}

static int rs_check_grids(const char *who, State &st, int kind, double t_gamma)
{
    const int grids[3] = {ASORA_GRID_XH, ASORA_GRID_NDENS, ASORA_GRID_TEMP};
    for (int q = 0; q < 3; ++q)
        if (ps_needs_grid(kind, grids[q], t_gamma) && (!st.grid[grids[q]] || !st.grid_valid[grids[q]]))
            return fail(4, std::string(who) + ": grid " + std::to_string(grids[q]) + " holds no data");
    if (st.N > ASORA_REGION_MAX_N)
        return fail(4, std::string(who) + ": not built for N > " + std::to_string(ASORA_REGION_MAX_N) + " (a line and its roots must fit LDS)");
    return 0;
}

// the mapping of the field of `kind` into h on the library's stream (v = NULL: h = g), with the fold of its moments into
// moments_out[0 ... 1] (device)
static int rs_launch_map(State &st, int kind, const double *nbar_dev, double scale, double t_gamma, const double *v, double vscale, int W,
                         int los_axis, double *h, double *moment_partial, double *moments_out)
{
    const int N = st.N, pitch = N | 1;
    const bool contiguous = los_axis == 2;
    const int T = rs_tile(N, contiguous);
    const size_t lds = 3 * (size_t)T * pitch * sizeof(double), n2 = (size_t)N * N;
    size_t outer_stride = 0, line_stride = 1, ncols = n2;
    unsigned tiles, blocks;
    if (contiguous) {
        tiles = (unsigned)((n2 + T - 1) / T); blocks = tiles;
    } else if (los_axis == 1) {
        outer_stride = n2; line_stride = (size_t)N; ncols = (size_t)N;
        tiles = (unsigned)((N + T - 1) / T); blocks = (unsigned)N * tiles;
    } else {
        line_stride = n2; ncols = n2;
        tiles = (unsigned)((n2 + T - 1) / T); blocks = tiles;
    }
    ASORA_HIP_TRY(hipFuncSetAttribute((const void *)rs_map_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(rs_map_kernel, dim3(blocks), dim3(contiguous ? RS_MAP_THREADS_ROWS : RS_MAP_THREADS_COLUMNS), lds, st.stream, kind, (const double *)st.grid[ASORA_GRID_XH],
                       (const double *)st.grid[ASORA_GRID_NDENS], (const double *)st.grid[ASORA_GRID_TEMP], nbar_dev, scale, t_gamma, v,
                       vscale, W, N, pitch, T, contiguous ? 1 : 0, outer_stride, line_stride, ncols, tiles, h, moment_partial);
    ASORA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rs_fold_kernel, dim3(1), dim3(PS_THREADS), 0, st.stream, (const double *)moment_partial, (int)blocks, 2, moments_out);
    ASORA_HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace asora

using namespace asora;

extern "C" {

int asora_los_velocity_to_device(const double *v, int N, char order, double *max_abs)
{
    clear_error();
    if (int rc = require_init("los_velocity_to_device")) return rc;
    if (int rc = check_N("los_velocity_to_device", N)) return rc;
    if (!v) return fail(3, "los_velocity_to_device: null host pointer");
    const bool c_order = order == 'C' || order == 'c';
    if (!c_order && order != 'F' && order != 'f') return fail(3, "los_velocity_to_device: order must be 'C' or 'F'");
    State &st = state();
    const size_t bytes = st.ncell * sizeof(double);
    // into a buffer of its own first: a refused upload leaves the velocity of the last good one in place
    Scoped<double> fresh;
    if (int rc = fresh.allocate(st.ncell)) return rc;
    if (int rc = st.redshift.vmax_dev.allocate(1)) return rc;
    if (c_order) {
        ASORA_HIP_TRY(hipMemcpyAsync(fresh.get(), v, bytes, hipMemcpyHostToDevice, st.stream));
    } else {
        ASORA_HIP_TRY(hipMemcpyAsync(st.staging, v, bytes, hipMemcpyHostToDevice, st.stream));
        if (int rc = launch_transpose(st, st.staging, fresh.get(), N)) return rc;
    }
    ASORA_HIP_TRY(hipMemsetAsync(st.redshift.vmax_dev, 0, sizeof(unsigned long long), st.stream));
    hipLaunchKernelGGL(rs_vmax_kernel, dim3(PS_RED_BLOCKS), dim3(PS_THREADS), 0, st.stream, (const double *)fresh.get(), st.ncell, st.redshift.vmax_dev);
    ASORA_HIP_TRY(hipGetLastError());
    unsigned long long bits = 0ull;
    ASORA_HIP_TRY(hipMemcpyAsync(&bits, st.redshift.vmax_dev, sizeof bits, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    if (bits >= RS_INF_BITS) return fail(3, "los_velocity_to_device: the velocity has a non-finite entry");
    (void)st.redshift.velocity.release();
    st.redshift.velocity.adopt(fresh.give(), bytes);
    std::memcpy(&st.redshift.vmax, &bits, sizeof bits);
    if (max_abs) *max_abs = st.redshift.vmax;
    return 0;
}

int asora_los_velocity_clear(void)
{
    clear_error();
    State &st = state();
    (void)st.redshift.velocity.release();
    st.redshift.vmax = 0.0;
    return 0;
}

int asora_redshift_space_field(int kind, double scale, double t_gamma, int los_axis, int use_velocity, double velocity_scale, int dst_grid,
                               double *moments, double *field_out)
{
    clear_error();
    if (int rc = require_init("redshift_space_field")) return rc;
    State &st = state();
    int W = 0;
    if (int rc = rs_check("redshift_space_field", st, kind, scale, t_gamma, los_axis, use_velocity, velocity_scale, &W)) return rc;
    if (dst_grid < -1 || dst_grid >= ASORA_GRID_COUNT) return fail(3, "redshift_space_field: dst_grid must be -1 or a grid selector");
    if (int rc = rs_check_grids("redshift_space_field", st, kind, t_gamma)) return rc;
    if (int rc = ensure_rs_buffers(st, dst_grid < 0)) return rc;
    if (dst_grid >= 0)
        if (int rc = ensure_optional_grid(dst_grid)) return rc;
    double *h = dst_grid >= 0 ? st.grid[dst_grid] : st.smoothing.field;
    const RsLayout lay(st.N);
    double *part = st.redshift.partial, *res = part + lay.result;
    const double *nbar_dev = nullptr;
    if (ps_needs_grid(kind, ASORA_GRID_NDENS, t_gamma))
        if (int rc = ps_mean_density(st, &nbar_dev)) return rc;
    if (int rc = rs_launch_map(st, kind, nbar_dev, scale, t_gamma, use_velocity ? (const double *)st.redshift.velocity : (const double *)nullptr,
                               velocity_scale, W, los_axis, h, part + lay.moments, res))
        return rc;
    if (dst_grid >= 0) {                                           // (as asora_grid_to_device leaves a grid)
        st.grid_valid[dst_grid] = true;
        st.zero.verdict.since_probe = std::max(st.zero.verdict.since_probe, 48);
        if (dst_grid == ASORA_GRID_TEMP) st.temp_probe.valid = false;
    }
    ASORA_HIP_TRY(hipMemcpyAsync(st.redshift.host, res, sizeof(double) * 2, hipMemcpyDeviceToHost, st.stream));
    if (field_out) ASORA_HIP_TRY(hipMemcpyAsync(field_out, h, sizeof(double) * st.ncell, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    if (moments) std::memcpy(moments, st.redshift.host, sizeof(double) * 2);
    return 0;
}

int asora_power_spectrum_los(int kind, double scale, double t_gamma, int los_axis, int use_velocity, double velocity_scale, int mode,
                             int n_a, const unsigned *thr_a, int n_b, const double *thr_b, unsigned long long *count, double *sum_1,
                             double *sum_2, double *sum_aa, double *sum_l2, double *sum_l4, double *moments_real, double *moments_rs,
                             double *field_out, double *modes_out)
{
    clear_error();
    if (int rc = require_init("power_spectrum_los")) return rc;
    State &st = state();
    int W = 0;
    if (int rc = rs_check("power_spectrum_los", st, kind, scale, t_gamma, los_axis, use_velocity, velocity_scale, &W)) return rc;
    if (mode != ASORA_ANISO_CYLINDRICAL && mode != ASORA_ANISO_MU) return fail(3, "power_spectrum_los: mode must be one of ASORA_ANISO_*");
    if (n_a < 1 || n_b < 1 || (long long)n_a * n_b > ASORA_ANISO_MAX_BINS)
        return fail(3, "power_spectrum_los: n_a and n_b must be >= 1 with n_a n_b <= " + std::to_string(ASORA_ANISO_MAX_BINS));
    if (!thr_a || !thr_b || !count || !sum_1 || !sum_2 || !sum_aa || !sum_l2 || !sum_l4 || !moments_real || !moments_rs)
        return fail(3, "power_spectrum_los: null thresholds or output pointer");
    if (mode == ASORA_ANISO_MU && thr_a[0] < 1u)
        return fail(3, "power_spectrum_los: thr_a[0] must be >= 1 in mode ASORA_ANISO_MU (the mode n = 0 is never binned)");
    for (int b = 0; b < n_a; ++b)
        if (thr_a[b + 1] < thr_a[b]) return fail(3, "power_spectrum_los: thr_a must be non-decreasing");
    for (int b = 0; b <= n_b; ++b)
        if (!std::isfinite(thr_b[b]) || (b > 0 && thr_b[b] < thr_b[b - 1]))
            return fail(3, "power_spectrum_los: thr_b must be finite and non-decreasing");
    if (int rc = rs_check_grids("power_spectrum_los", st, kind, t_gamma)) return rc;

    const int N = st.N, NZ = N / 2 + 1, nb = n_a * n_b;
    const size_t ncell = st.ncell, nmodes = (size_t)N * N * NZ;
    if (int rc = ensure_rs_buffers(st, use_velocity || field_out)) return rc;
    const RsLayout lay(N);
    double *part = st.redshift.partial, *res = part + lay.result;
    double *stage = st.redshift.host + RS_RES_WORDS;
    std::memcpy(stage + RS_THR_B, thr_b, sizeof(double) * (n_b + 1));
    std::memcpy(stage + RS_THR_A, thr_a, sizeof(unsigned) * (n_a + 1));
    ASORA_HIP_TRY(hipMemcpyAsync(st.redshift.thresholds, stage, sizeof(double) * RS_THR_WORDS, hipMemcpyHostToDevice, st.stream));
    StageStopwatch<ASORA_PSLOS_STAGES> watch(st.opt[ASORA_OPT_TIMING] != 0, st.stream);
    auto mark = [&watch]() { return watch.mark(); };

    if (int rc = watch.mark()) return rc;
    const bool nbar = ps_needs_grid(kind, ASORA_GRID_NDENS, t_gamma);
    const double *nbar_dev = nullptr, *moments_dev = nullptr;
    if (nbar)
        if (int rc = ps_mean_density(st, &nbar_dev)) return rc;
    if (int rc = watch.mark()) return rc;
    if (use_velocity) {
        // the mapped field lies in sm_field and goes through the transform as kind ASORA_PS_XH
        if (int rc = rs_launch_map(st, kind, nbar_dev, scale, t_gamma, (const double *)st.redshift.velocity, velocity_scale, W, los_axis,
                                   st.smoothing.field, part + lay.moments, res))
            return rc;
        if (int rc = watch.mark()) return rc;
        if (int rc = ps_transform(st, ASORA_PS_XH, st.smoothing.field, false, 1.0, 0.0, nullptr, mark, &moments_dev)) return rc;
        ASORA_HIP_TRY(hipMemcpyAsync(res + 2, moments_dev, sizeof(double) * 2, hipMemcpyDeviceToDevice, st.stream));
    } else {
        if (int rc = watch.mark()) return rc;
        if (int rc = ps_transform(st, kind, st.grid[ASORA_GRID_XH], nbar, scale, t_gamma, field_out ? st.smoothing.field : (double *)nullptr, mark,
                                  &moments_dev))
            return rc;
        ASORA_HIP_TRY(hipMemcpyAsync(res, moments_dev, sizeof(double) * 2, hipMemcpyDeviceToDevice, st.stream));
        ASORA_HIP_TRY(hipMemcpyAsync(res + 2, moments_dev, sizeof(double) * 2, hipMemcpyDeviceToDevice, st.stream));
    }

    const int waves = nb <= ASORA_ANISO_MAX_BINS / 2 ? PS_WAVES : PS_WAVES / 2;
    const size_t bin_lds = (size_t)waves * RS_VALUES * nb * sizeof(double) + sizeof(double) * (n_b + 1) + sizeof(unsigned) * (n_a + 1);
    const unsigned *ta = (const unsigned *)(st.redshift.thresholds + RS_THR_A);
    const double *tb = st.redshift.thresholds + RS_THR_B;
    if (mode == ASORA_ANISO_CYLINDRICAL) {
        ASORA_HIP_TRY(hipFuncSetAttribute((const void *)rs_bin_kernel<ASORA_ANISO_CYLINDRICAL>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)bin_lds));
        hipLaunchKernelGGL(rs_bin_kernel<ASORA_ANISO_CYLINDRICAL>, dim3((unsigned)N), dim3(64 * waves), bin_lds, st.stream,
                           (const double2 *)st.spectrum.modes[0], N, los_axis, n_a, n_b, ta, tb, part + lay.bins);
    } else {
        ASORA_HIP_TRY(hipFuncSetAttribute((const void *)rs_bin_kernel<ASORA_ANISO_MU>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bin_lds));
        hipLaunchKernelGGL(rs_bin_kernel<ASORA_ANISO_MU>, dim3((unsigned)N), dim3(64 * waves), bin_lds, st.stream,
                           (const double2 *)st.spectrum.modes[0], N, los_axis, n_a, n_b, ta, tb, part + lay.bins);
    }
    ASORA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rs_bin_final_kernel, dim3((unsigned)((RS_VALUES * nb + PS_THREADS - 1) / PS_THREADS)), dim3(PS_THREADS), 0, st.stream,
                       (const double *)(part + lay.bins), N, nb, res + RS_RES_BINS);
    ASORA_HIP_TRY(hipGetLastError());
    if (int rc = watch.mark()) return rc;

    ASORA_HIP_TRY(hipMemcpyAsync(st.redshift.host, res, sizeof(double) * (RS_RES_BINS + (size_t)RS_VALUES * nb), hipMemcpyDeviceToHost, st.stream));
    if (field_out) ASORA_HIP_TRY(hipMemcpyAsync(field_out, st.smoothing.field, sizeof(double) * ncell, hipMemcpyDeviceToHost, st.stream));
    if (modes_out) ASORA_HIP_TRY(hipMemcpyAsync(modes_out, st.spectrum.modes[0], sizeof(double2) * nmodes, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    watch.read(st.redshift.ms);

    const double *h = st.redshift.host, *bins = h + RS_RES_BINS;
    std::memcpy(moments_real, h, sizeof(double) * 2);
    std::memcpy(moments_rs, h + 2, sizeof(double) * 2);
    std::memcpy(count, bins + (size_t)RS_COUNT * nb, sizeof(unsigned long long) * nb);
    std::memcpy(sum_1, bins + (size_t)RS_SUM_1 * nb, sizeof(double) * nb);
    std::memcpy(sum_2, bins + (size_t)RS_SUM_2 * nb, sizeof(double) * nb);
    std::memcpy(sum_aa, bins + (size_t)RS_SUM_AA * nb, sizeof(double) * nb);
    std::memcpy(sum_l2, bins + (size_t)RS_SUM_L2 * nb, sizeof(double) * nb);
    std::memcpy(sum_l4, bins + (size_t)RS_SUM_L4 * nb, sizeof(double) * nb);
    return 0;
}

int asora_debug_power_spectrum_los_ms(double *ms)
{
    clear_error();
    if (!ms) return fail(3, "debug_power_spectrum_los_ms: null pointer");
    for (int q = 0; q < ASORA_PSLOS_STAGES; ++q) ms[q] = state().redshift.ms[q];
    return 0;
}

} // extern "C"
