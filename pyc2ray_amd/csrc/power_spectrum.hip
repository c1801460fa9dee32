// power_spectrum.hip -- the spherically averaged power spectrum of a field formed from the device grids, and the cross-spectrum of two
// (asora_power_spectrum): a batched FP64 real-to-complex 3-D Fourier transform and a shell binning, both
// written here; nothing but the HIP runtime is linked.  Stages on the library's stream, none of which writes to a grid:
//   a. mean density : ps_sum_kernel over ASORA_GRID_NDENS (a fixed grid of PS_RED_BLOCKS workgroups) and ps_final_kernel, for the
//                     kinds that divide by it;
//   b. along k      : ps_row_kernel, one workgroup per T rows (i, j): it forms g from the grids in registers, adds g and g^2 to its
//                     partial moments, stores the field if asked, transforms the T rows in LDS -- a complex transform with a zero
//                     imaginary part -- and stores n_z = 0 ... N/2 of each into the complex buffer [i][j][n_z];
//   c. along j, i   : ps_line_kernel, in place: one workgroup per tile of T adjacent columns of the contiguous index (n_z for the
//                     pass along j; (j, n_z) flattened for the pass along i) takes all N elements of the strided axis into LDS
//                     (every global access is a fragment of T complex doubles, 64 ... 256 bytes; the last tile of a row may be
//                     narrower), transforms the T lines and writes them back;
//   d. binning      : ps_bin_kernel, one workgroup per plane i: a wave takes 64 consecutive n_z of one row, along which the bin is
//                     non-decreasing, reduces each run of equal bins by a segmented scan in lane order, and the last lane of a run
//                     adds into the wave's own LDS histogram by plain read-modify-write; the waves' histograms are combined in wave
//                     order into the plane's partial row, and ps_bin_final_kernel adds the planes in plane order.
// The line transform (line_fft), its plan, tile and LDS layout, the forming of the field and the double-double sums are shared with
// the smoothing (smooth_field.hip): fft_device.hpp.
// Every floating-point sum is formed in an order fixed by (N, thresholds): per thread in index order, per wave by a shuffle tree,
// per workgroup in wave order, over workgroups in index order -- the mean density and the moments in double-double (two-sum), so
// that they are correct to the last bit or two whatever the order.  No floating-point atomic anywhere.
#include "asora_internal.hpp"
#include "fft_device.hpp"

namespace asora {

constexpr int PS_VALUES = 5;                // per bin: count, sum_k, sum_aa, sum_bb, sum_ab
constexpr int PS_COUNT = 0, PS_SUM_K = 1, PS_SUM_AA = 2, PS_SUM_BB = 3, PS_SUM_AB = 4;
// the result words (doubles; the counts are uint64 in the same 8 bytes): the bins, the moments of a and of b, the mean density
constexpr int PS_RES_MOMENTS = PS_VALUES * ASORA_BUBBLE_MAX_BINS, PS_RES_NBAR = PS_RES_MOMENTS + 4, PS_RES_WORDS = PS_RES_NBAR + 1;
constexpr int PS_HOST_WORDS = PS_RES_WORDS + (ASORA_BUBBLE_MAX_BINS + 2) / 2;     // the thresholds (uint32) behind the results

// partial[2 b], [2 b + 1] = the double-double sum of a[] over the cells of workgroup b (grid-stride; the grid is PS_RED_BLOCKS)
__global__ void __launch_bounds__(PS_THREADS) ps_sum_kernel(const double *__restrict__ a, size_t n, double *__restrict__ partial)
{
    dd s = {0.0, 0.0};
    const size_t stride = (size_t)gridDim.x * PS_THREADS;
    for (size_t c = (size_t)blockIdx.x * PS_THREADS + threadIdx.x; c < n; c += stride) dd_add(s, a[c]);
    s = ps_block_sum(s);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = s.hi; partial[2 * blockIdx.x + 1] = s.lo; }
}

// out[q] = (the sum over e < count of the double-double partial[(e ncomp + q) 2 ...]) / divisor, q < ncomp; ONE workgroup
__global__ void __launch_bounds__(PS_THREADS) ps_final_kernel(const double *__restrict__ partial, int count, int ncomp, double divisor,
                                                               double *__restrict__ out)
{
    for (int q = 0; q < ncomp; ++q) {
        dd s = {0.0, 0.0};
        for (int e = threadIdx.x; e < count; e += PS_THREADS) {
            const double *p = partial + ((size_t)e * ncomp + q) * 2;
            dd o = {p[0], p[1]};
            dd_merge(s, o);
        }
        s = ps_block_sum(s);
        if (threadIdx.x == 0) out[q] = (s.hi + s.lo) / divisor;
    }
}

// the pass along k: workgroup b forms and transforms the rows b T ... b T + T - 1 of the N^2 rows (i, j)
__global__ void __launch_bounds__(PS_THREADS) ps_row_kernel(int kind, const double *__restrict__ x, const double *__restrict__ n,
                                                             const double *__restrict__ temp, const double *__restrict__ nbar_dev,
                                                             double scale, double t_gamma, int N, int pitch, int T, PsPlan plan,
                                                             const double2 *__restrict__ twiddle, double2 *__restrict__ modes,
                                                             double *__restrict__ moment_partial, double *__restrict__ field)
{
    extern __shared__ double2 ps_lds[];
    double2 *tw, *a, *b;
    ps_lds_layout(ps_lds, twiddle, N, pitch, T, tw, a, b);
    const int NZ = N / 2 + 1;
    const size_t rows = (size_t)N * N, row0 = (size_t)blockIdx.x * T;
    const int nl = (int)(rows - row0 < (size_t)T ? rows - row0 : (size_t)T);
    const double nbar = nbar_dev ? *nbar_dev : 1.0;
    dd s1 = {0.0, 0.0}, s2 = {0.0, 0.0};
    for (int w = threadIdx.x; w < nl * N; w += PS_THREADS) {
        const int t = w / N, k = w - t * N;
        const size_t c = (row0 + t) * (size_t)N + k;
        const double g = ps_form(kind, c, x, n, temp, nbar, scale, t_gamma);
        a[t * pitch + k] = make_double2(g, 0.0);
        dd_add(s1, g);
        dd_add(s2, g * g);
        if (field) field[c] = g;
    }
    s1 = ps_block_sum(s1);
    s2 = ps_block_sum(s2);
    if (threadIdx.x == 0) {
        double *p = moment_partial + (size_t)blockIdx.x * 4;
        p[0] = s1.hi; p[1] = s1.lo; p[2] = s2.hi; p[3] = s2.lo;
    }
    const double2 *res = line_fft(a, b, tw, plan, N, pitch, nl);
    for (int w = threadIdx.x; w < nl * NZ; w += PS_THREADS) {
        const int t = w / NZ, kz = w - t * NZ;
        modes[(row0 + t) * (size_t)NZ + kz] = res[t * pitch + kz];
    }
}

// a strided pass, in place: the buffer is n_outer blocks, outer_stride apart, of N lines elements line_stride apart, each ncols
// contiguous columns wide; workgroup b takes the columns c0 ... c0 + width - 1 of one block, c0 a multiple of T, width <= T
__global__ void __launch_bounds__(PS_THREADS) ps_line_kernel(double2 *__restrict__ modes, int N, int pitch, int T, PsPlan plan,
                                                              const double2 *__restrict__ twiddle, size_t outer_stride, size_t line_stride,
                                                              size_t ncols, unsigned tiles)
{
    extern __shared__ double2 ps_lds[];
    double2 *tw, *a, *b;
    ps_lds_layout(ps_lds, twiddle, N, pitch, T, tw, a, b);
    const unsigned outer = blockIdx.x / tiles;
    const size_t c0 = (size_t)(blockIdx.x - outer * tiles) * T;
    const int width = (int)(ncols - c0 < (size_t)T ? ncols - c0 : (size_t)T);
    double2 *g = modes + outer * outer_stride + c0;
    for (int w = threadIdx.x; w < width * N; w += PS_THREADS) {
        const int e = w / width, t = w - e * width;
        a[t * pitch + e] = g[e * line_stride + t];
    }
    const double2 *res = line_fft(a, b, tw, plan, N, pitch, width);
    for (int w = threadIdx.x; w < width * N; w += PS_THREADS) {
        const int e = w / width, t = w - e * width;
        g[e * line_stride + t] = res[t * pitch + e];
    }
}

// ---- binning -------------------------------------------------------------------------------------------------------------------
// v summed over the lanes start ... lane of the caller's run, in the order of a Hillis-Steele scan
template <typename V> __device__ __forceinline__ V ps_run_scan(V v, int lane, int start)
{
    for (int d = 1; d < 64; d <<= 1) {
        const V up = __shfl_up(v, d);
        if (lane - d >= start) v += up;
    }
    return v;
}

// partial[(plane PS_VALUES + q) n_bins + b] = value q of bin b summed over the stored modes of plane i = blockIdx.x; dynamic LDS:
// PS_WAVES histograms [PS_VALUES][n_bins] of 8-byte words, then thresholds[n_bins + 1]
template <bool CROSS>
__global__ void __launch_bounds__(PS_THREADS) ps_bin_kernel(const double2 *__restrict__ A, const double2 *__restrict__ B, int N, int n_bins,
                                                             const unsigned *__restrict__ thresholds, double *__restrict__ partial)
{
    extern __shared__ double ps_hist[];
    unsigned *thr = (unsigned *)(ps_hist + (size_t)PS_WAVES * PS_VALUES * n_bins);
    for (int q = threadIdx.x; q < PS_WAVES * PS_VALUES * n_bins; q += PS_THREADS) ps_hist[q] = 0.0;      // (+0.0 is the integer 0 too)
    for (int q = threadIdx.x; q <= n_bins; q += PS_THREADS) thr[q] = thresholds[q];
    __syncthreads();
    const int NZ = N / 2 + 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = blockIdx.x;
    const unsigned mi = (unsigned)min(i, N - i);
    volatile double *hist = ps_hist + (size_t)wave * PS_VALUES * n_bins;
    volatile unsigned long long *hist_n = (volatile unsigned long long *)hist;
    for (int j = wave; j < N; j += PS_WAVES) {
        const unsigned mj = (unsigned)min(j, N - j), n2_ij = mi * mi + mj * mj;
        const double2 *ra = A + ((size_t)i * N + j) * NZ, *rb = CROSS ? B + ((size_t)i * N + j) * NZ : nullptr;
        for (int kz0 = 0; kz0 < NZ; kz0 += 64) {
            const int kz = kz0 + lane;
            const bool stored = kz < NZ;
            const unsigned n2 = n2_ij + (unsigned)(kz * kz);
            // the bin: (the first threshold above n2) - 1; -1 below the first edge, n_bins at or above the last and in the lanes
            // past the row's end -- non-decreasing along the lanes either way
            int bin = n_bins;
            if (stored) {
                int lo = 0, hi = n_bins + 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (thr[mid] <= n2) lo = mid + 1; else hi = mid;
                }
                bin = lo - 1;
            }
            double wgt = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
            if (stored) {
                wgt = (kz == 0 || 2 * kz == N) ? 1.0 : 2.0;
                const double2 za = ra[kz];
                aa = wgt * fma(za.x, za.x, za.y * za.y);
                if (CROSS) {
                    const double2 zb = rb[kz];
                    bb = wgt * fma(zb.x, zb.x, zb.y * zb.y);
                    ab = wgt * fma(za.x, zb.x, za.y * zb.y);
                }
            }
            const int before = __shfl_up(bin, 1);
            const unsigned long long heads = __ballot(lane == 0 || bin != before);
            const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
            const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
            const unsigned long long cnt = ps_run_scan((unsigned long long)wgt, lane, start);
            const double sk = ps_run_scan(wgt * sqrt((double)n2), lane, start);
            aa = ps_run_scan(aa, lane, start);
            if (CROSS) { bb = ps_run_scan(bb, lane, start); ab = ps_run_scan(ab, lane, start); }
            if (last && bin >= 0 && bin < n_bins) {               // (one lane per bin in this instruction: runs are maximal)
                hist_n[PS_COUNT * n_bins + bin] += cnt;
                hist[PS_SUM_K * n_bins + bin] += sk;
                hist[PS_SUM_AA * n_bins + bin] += aa;
                if (CROSS) { hist[PS_SUM_BB * n_bins + bin] += bb; hist[PS_SUM_AB * n_bins + bin] += ab; }
            }
        }
    }
    __syncthreads();
    const int nv = CROSS ? PS_VALUES : PS_SUM_AA + 1;
    for (int q = threadIdx.x; q < nv * n_bins; q += PS_THREADS) {
        double *out = partial + (size_t)i * PS_VALUES * n_bins + q;
        if (q < n_bins) {
            unsigned long long s = 0ull;
            for (int u = 0; u < PS_WAVES; ++u) s += ((const unsigned long long *)ps_hist)[(size_t)u * PS_VALUES * n_bins + q];
            *(unsigned long long *)out = s;
        } else {
            double s = ps_hist[q];
            for (int u = 1; u < PS_WAVES; ++u) s += ps_hist[(size_t)u * PS_VALUES * n_bins + q];
            *out = s;
        }
    }
}

// result[q ASORA_BUBBLE_MAX_BINS + b] = the planes' partial rows added in plane order, q < nv
__global__ void __launch_bounds__(PS_THREADS) ps_bin_final_kernel(const double *__restrict__ partial, int N, int n_bins, int nv,
                                                                   double *__restrict__ result)
{
    const int t = blockIdx.x * PS_THREADS + threadIdx.x;
    if (t >= nv * n_bins) return;
    const int q = t / n_bins, b = t - q * n_bins;
    double *out = result + q * ASORA_BUBBLE_MAX_BINS + b;
    if (q == PS_COUNT) {
        unsigned long long s = 0ull;
        for (int i = 0; i < N; ++i) s += ((const unsigned long long *)partial)[(size_t)i * PS_VALUES * n_bins + t];
        *(unsigned long long *)out = s;
    } else {
        double s = 0.0;
        for (int i = 0; i < N; ++i) s += partial[(size_t)i * PS_VALUES * n_bins + t];
        *out = s;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// the words of ps_partial: [bins: N PS_VALUES MAX_BINS | moments of a, of b: row workgroups x 4 each | mean density: 2 PS_RED_BLOCKS
// | results: PS_RES_WORDS]
struct PsLayout {
    size_t row_blocks, bins, moments[2], nbar, result, words;
    explicit PsLayout(int N, int T)
    {
        row_blocks = ((size_t)N * N + T - 1) / T;
        bins = 0;
        moments[0] = bins + (size_t)N * PS_VALUES * ASORA_BUBBLE_MAX_BINS;
        moments[1] = moments[0] + 4 * row_blocks;
        nbar = moments[1] + 4 * row_blocks;
        result = nbar + 2 * PS_RED_BLOCKS;
        words = result + PS_RES_WORDS;
    }
};

static int ensure_ps_buffers(State &st, const PsLayout &lay, bool cross)
{
    const int N = st.N;
    const size_t nmodes = (size_t)N * N * (N / 2 + 1);
    for (int f = 0; f < (cross ? 2 : 1); ++f)
        if (int rc = st.spectrum.modes[f].allocate(nmodes)) return rc;
    if (int rc = st.spectrum.partial.allocate(lay.words)) return rc;
    if (int rc = st.spectrum.thresholds.allocate((ASORA_BUBBLE_MAX_BINS + 1))) return rc;
    if (int rc = st.spectrum.host.allocate(PS_HOST_WORDS)) return rc;
    if (!st.spectrum.twiddle) {
        // exp(-2 pi i r / N) from the first octant's cos and sin in extended precision, so that the symmetries hold to the bit
        std::vector<double2> tw((size_t)N);
        const long double two_pi = 6.283185307179586476925286766559005768L;
        for (int r = 0; r < N; ++r) {
            // the angle 2 pi r / N folded into [0, pi/4] by exact integer arithmetic on eighths of a turn: 8 r = o N + rest
            const long o = (8L * r) / N, rest = 8L * r - o * N;                  // octant o = 0 ... 7, rest / (8 N) of a turn into it
            const bool odd = o & 1;
            const long double ang = two_pi * (long double)(odd ? N - rest : rest) / (8.0L * N);   // in [0, pi/4]
            const long double c = cosl(ang), s = sinl(ang);
            // cos and sin of the angle o pi/4 + (odd ? pi/4 - ang : ang)
            long double co, si;
            switch (o) {
            case 0: co = c; si = s; break;
            case 1: co = s; si = c; break;
            case 2: co = -s; si = c; break;
            case 3: co = -c; si = s; break;
            case 4: co = -c; si = -s; break;
            case 5: co = -s; si = -c; break;
            case 6: co = s; si = -c; break;
            default: co = c; si = -s; break;
            }
            tw[r] = make_double2((double)co, (double)(0.0L - si));
        }
        if (int rc = st.spectrum.twiddle.allocate((size_t)N)) return rc;
        ASORA_HIP_TRY(hipMemcpy(st.spectrum.twiddle, tw.data(), sizeof(double2) * N, hipMemcpyHostToDevice));
    }
    return 0;
}

using PsStopwatch = StageStopwatch<ASORA_PS_STAGES>;

static bool ps_kind_uses(int kind, int grid, double t_gamma)
{
    switch (grid) {
    case ASORA_GRID_XH: return kind == ASORA_PS_XH || kind == ASORA_PS_XHI || kind == ASORA_PS_HI;
    case ASORA_GRID_NDENS: return kind == ASORA_PS_DENSITY || kind == ASORA_PS_HI;
    default: return kind == ASORA_PS_HI && t_gamma > 0.0;       // ASORA_GRID_TEMP
    }
}

bool ps_needs_grid(int kind, int grid, double t_gamma) { return ps_kind_uses(kind, grid, t_gamma); }

// The launches of stages a to c on the library's stream, for asora_power_spectrum and for ps_forward: field f of a kind goes into
// st.spectrum.modes[f], its moments into the result words
struct PsPasses {
    State &st;
    const int N, NZ, T, pitch;
    const PsLayout lay;
    const PsPlan plan;
    const size_t fft_lds;
    const dim3 block{PS_THREADS};
    explicit PsPasses(State &s)
        : st(s), N(s.N), NZ(s.N / 2 + 1), T(ps_tile(s.N)), pitch(s.N | 1), lay(s.N, ps_tile(s.N)), plan(ps_plan(s.N)),
          fft_lds(((size_t)2 * ps_tile(s.N) * (s.N | 1) + s.N) * sizeof(double2)) {}
    double *partial() const { return st.spectrum.partial; }
    double *result() const { return st.spectrum.partial + lay.result; }
    int prepare(bool cross)
    {
        if (int rc = ensure_ps_buffers(st, lay, cross)) return rc;
        ASORA_HIP_TRY(hipFuncSetAttribute((const void *)ps_row_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fft_lds));
        ASORA_HIP_TRY(hipFuncSetAttribute((const void *)ps_line_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fft_lds));
        return 0;
    }
    int mean_density()
    {
        hipLaunchKernelGGL(ps_sum_kernel, dim3(PS_RED_BLOCKS), block, 0, st.stream, (const double *)st.grid[ASORA_GRID_NDENS], st.ncell,
                           partial() + lay.nbar);
        ASORA_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(ps_final_kernel, dim3(1), block, 0, st.stream, (const double *)(partial() + lay.nbar), PS_RED_BLOCKS, 1,
                           (double)st.ncell, result() + PS_RES_NBAR);
        ASORA_HIP_TRY(hipGetLastError());
        return 0;
    }
    // along k, with the field and its moments; x: what the kinds read as the ionised fraction (the grid, or a caller's own buffer)
    int rows(int f, int kind, bool nbar, double scale, double t_gamma, double *field, const double *x)
    {
        hipLaunchKernelGGL(ps_row_kernel, dim3((unsigned)lay.row_blocks), block, fft_lds, st.stream, kind,
                           x, (const double *)st.grid[ASORA_GRID_NDENS],
                           (const double *)st.grid[ASORA_GRID_TEMP], nbar ? (const double *)(result() + PS_RES_NBAR) : (const double *)nullptr,
                           scale, t_gamma, N, pitch, T, plan, (const double2 *)st.spectrum.twiddle, st.spectrum.modes[f], partial() + lay.moments[f],
                           field);
        ASORA_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(ps_final_kernel, dim3(1), block, 0, st.stream, (const double *)(partial() + lay.moments[f]), (int)lay.row_blocks,
                           2, 1.0, result() + PS_RES_MOMENTS + 2 * f);
        ASORA_HIP_TRY(hipGetLastError());
        return 0;
    }
    int lines_j(int f)                  // N blocks (the planes i) of N lines, NZ columns wide
    {
        const unsigned tiles = (unsigned)((NZ + T - 1) / T);
        hipLaunchKernelGGL(ps_line_kernel, dim3((unsigned)N * tiles), block, fft_lds, st.stream, st.spectrum.modes[f], N, pitch, T, plan,
                           (const double2 *)st.spectrum.twiddle, (size_t)N * NZ, (size_t)NZ, (size_t)NZ, tiles);
        ASORA_HIP_TRY(hipGetLastError());
        return 0;
    }
    int lines_i(int f)                  // one block of N lines, N NZ columns wide
    {
        const unsigned tiles = (unsigned)(((size_t)N * NZ + T - 1) / T);
        hipLaunchKernelGGL(ps_line_kernel, dim3(tiles), block, fft_lds, st.stream, st.spectrum.modes[f], N, pitch, T, plan,
                           (const double2 *)st.spectrum.twiddle, (size_t)0, (size_t)N * NZ, (size_t)N * NZ, tiles);
        ASORA_HIP_TRY(hipGetLastError());
        return 0;
    }
};

// The forward half of asora_smooth_field (smooth_field.hip): stages a to c above for the one field of `kind`, into st.spectrum.modes[0] --
// the launches of an auto-spectrum, so the modes and the moments are its bits.  The caller has checked the kind and its grids.
// stage_done is called behind each of the four stages (mean density, along k, j, i); *moments_dev: where (sum g, sum g^2) lie on the
// device once the stream has got there
int ps_forward(State &st, int kind, double scale, double t_gamma, const std::function<int()> &stage_done, const double **moments_dev)
{
    const bool nbar = ps_kind_uses(kind, ASORA_GRID_NDENS, t_gamma);
    const double *nbar_dev = nullptr;
    if (nbar)
        if (int rc = ps_mean_density(st, &nbar_dev)) return rc;
    if (int rc = stage_done()) return rc;
    return ps_transform(st, kind, st.grid[ASORA_GRID_XH], nbar, scale, t_gamma, nullptr, stage_done, moments_dev);
}

// The same stages one by one, for the redshift-space unit (redshift_space.hip), which puts a stage of its own between the mean
// density and the pass along k.  ps_mean_density: stage a; *nbar_dev: where the mean lies on the device.  ps_transform: stages b and
// c for the field of `kind`, read with `x` in the place of the ionised-fraction grid (a mapped field goes through ASORA_PS_XH), with
// nbar as ps_mean_density left it if `nbar`; field: NULL, or where the formed field is stored; stage_done behind each of the three
int ps_mean_density(State &st, const double **nbar_dev)
{
    PsPasses pass(st);
    if (int rc = pass.prepare(false)) return rc;
    if (int rc = pass.mean_density()) return rc;
    *nbar_dev = pass.result() + PS_RES_NBAR;
    return 0;
}

int ps_transform(State &st, int kind, const double *x, bool nbar, double scale, double t_gamma, double *field,
                 const std::function<int()> &stage_done, const double **moments_dev)
{
    PsPasses pass(st);
    if (int rc = pass.prepare(false)) return rc;
    if (int rc = pass.rows(0, kind, nbar, scale, t_gamma, field, x)) return rc;
    if (int rc = stage_done()) return rc;
    if (int rc = pass.lines_j(0)) return rc;
    if (int rc = stage_done()) return rc;
    if (int rc = pass.lines_i(0)) return rc;
    if (int rc = stage_done()) return rc;
    *moments_dev = pass.result() + PS_RES_MOMENTS;
    return 0;
}

// Stage d for the auto-spectrum of what ps_forward left in st.spectrum.modes[0], for asora_bispectrum (bispectrum.hip): the thresholds
// leave through the pinned area as in asora_power_spectrum, and the two launches are its launches
int ps_bin_auto(State &st, int n_bins, const unsigned *thresholds, const unsigned long long **count_dev, const double **sum_k_dev,
                const double **sum_aa_dev)
{
    PsPasses pass(st);
    if (int rc = pass.prepare(false)) return rc;
    const int N = st.N;
    const size_t bin_lds = (size_t)PS_WAVES * PS_VALUES * n_bins * sizeof(double) + sizeof(unsigned) * (n_bins + 1);
    unsigned *thr_host = (unsigned *)(st.spectrum.host + PS_RES_WORDS);
    std::memcpy(thr_host, thresholds, sizeof(unsigned) * (n_bins + 1));
    ASORA_HIP_TRY(hipMemcpyAsync(st.spectrum.thresholds, thr_host, sizeof(unsigned) * (n_bins + 1), hipMemcpyHostToDevice, st.stream));
    double *part = pass.partial(), *res = pass.result();
    const int nv = PS_SUM_AA + 1;
    hipLaunchKernelGGL(ps_bin_kernel<false>, dim3((unsigned)N), pass.block, bin_lds, st.stream, (const double2 *)st.spectrum.modes[0],
                       (const double2 *)nullptr, N, n_bins, (const unsigned *)st.spectrum.thresholds, part + pass.lay.bins);
    ASORA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ps_bin_final_kernel, dim3((unsigned)((nv * n_bins + PS_THREADS - 1) / PS_THREADS)), pass.block, 0, st.stream,
                       (const double *)(part + pass.lay.bins), N, n_bins, nv, res);
    ASORA_HIP_TRY(hipGetLastError());
    *count_dev = (const unsigned long long *)(res + PS_COUNT * ASORA_BUBBLE_MAX_BINS);
    *sum_k_dev = res + PS_SUM_K * ASORA_BUBBLE_MAX_BINS;
    *sum_aa_dev = res + PS_SUM_AA * ASORA_BUBBLE_MAX_BINS;
    return 0;
}

} // namespace asora

using namespace asora;

extern "C" {

int asora_power_spectrum(int kind_a, int kind_b, double scale, double t_gamma, int n_bins, const unsigned *thresholds,
                         unsigned long long *count, double *sum_k, double *sum_aa, double *sum_bb, double *sum_ab, double *moments_a,
                         double *moments_b, double *field_out, double *modes_out)
{
    clear_error();
    if (int rc = require_init("power_spectrum")) return rc;
    const bool cross = kind_b != -1;
    if (kind_a < 0 || kind_a >= ASORA_PS_KINDS || (cross && (kind_b < 0 || kind_b >= ASORA_PS_KINDS)))
        return fail(3, "power_spectrum: a kind must be one of ASORA_PS_* (kind_b: or -1)");
    if (!std::isfinite(scale)) return fail(3, "power_spectrum: scale must be finite");
    if (!std::isfinite(t_gamma) || t_gamma < 0.0) return fail(3, "power_spectrum: t_gamma must be finite and >= 0");
    if (n_bins < 1 || n_bins > ASORA_BUBBLE_MAX_BINS)
        return fail(3, "power_spectrum: n_bins must be in [1, " + std::to_string(ASORA_BUBBLE_MAX_BINS) + "]");
    if (!thresholds || !count || !sum_k || !sum_aa || !moments_a || (cross && (!sum_bb || !sum_ab || !moments_b)))
        return fail(3, "power_spectrum: null thresholds or output pointer");
    if (thresholds[0] < 1u) return fail(3, "power_spectrum: thresholds[0] must be >= 1 (the mode n = 0 is never binned)");
    for (int b = 0; b < n_bins; ++b)
        if (thresholds[b + 1] < thresholds[b]) return fail(3, "power_spectrum: the thresholds must be non-decreasing");
    State &st = state();
    const int kinds[2] = {kind_a, cross ? kind_b : kind_a};
    bool need[3] = {false, false, false};
    const int grids[3] = {ASORA_GRID_XH, ASORA_GRID_NDENS, ASORA_GRID_TEMP};
    for (int q = 0; q < 3; ++q) {
        need[q] = ps_kind_uses(kinds[0], grids[q], t_gamma) || ps_kind_uses(kinds[1], grids[q], t_gamma);
        if (need[q] && (!st.grid[grids[q]] || !st.grid_valid[grids[q]]))
            return fail(4, "power_spectrum: grid " + std::to_string(grids[q]) + " holds no data");
    }
    if (st.N > ASORA_REGION_MAX_N)
        return fail(4, "power_spectrum: not built for N > " + std::to_string(ASORA_REGION_MAX_N) + " (a line and its roots must fit LDS)");

    PsPasses pass(st);
    const int N = st.N, nf = cross ? 2 : 1;
    const size_t ncell = st.ncell, nmodes = (size_t)N * N * pass.NZ;
    const PsLayout &lay = pass.lay;
    if (int rc = pass.prepare(cross)) return rc;
    Scoped<double> field;                // the formed field on the device, for field_out
    if (field_out) { if (int rc = field.allocate(ncell)) return rc; }

    const size_t bin_lds = (size_t)PS_WAVES * PS_VALUES * n_bins * sizeof(double) + sizeof(unsigned) * (n_bins + 1);
    double *part = pass.partial(), *res = pass.result();
    unsigned *thr_host = (unsigned *)(st.spectrum.host + PS_RES_WORDS);
    std::memcpy(thr_host, thresholds, sizeof(unsigned) * (n_bins + 1));
    ASORA_HIP_TRY(hipMemcpyAsync(st.spectrum.thresholds, thr_host, sizeof(unsigned) * (n_bins + 1), hipMemcpyHostToDevice, st.stream));
    ASORA_HIP_TRY(hipMemsetAsync(res, 0, sizeof(double) * PS_RES_WORDS, st.stream));
    const dim3 block(PS_THREADS);
    PsStopwatch watch(st.opt[ASORA_OPT_TIMING] != 0, st.stream);

    if (int rc = watch.mark()) return rc;
    if (need[1])
        if (int rc = pass.mean_density()) return rc;
    if (int rc = watch.mark()) return rc;
    for (int f = 0; f < nf; ++f)
        if (int rc = pass.rows(f, kinds[f], need[1], scale, t_gamma, f == 0 ? field.get() : (double *)nullptr, st.grid[ASORA_GRID_XH])) return rc;
    if (int rc = watch.mark()) return rc;
    for (int f = 0; f < nf; ++f)
        if (int rc = pass.lines_j(f)) return rc;
    if (int rc = watch.mark()) return rc;
    for (int f = 0; f < nf; ++f)
        if (int rc = pass.lines_i(f)) return rc;
    if (int rc = watch.mark()) return rc;
    const int nv = cross ? PS_VALUES : PS_SUM_AA + 1;
    if (cross)
        hipLaunchKernelGGL(ps_bin_kernel<true>, dim3((unsigned)N), block, bin_lds, st.stream, (const double2 *)st.spectrum.modes[0],
                           (const double2 *)st.spectrum.modes[1], N, n_bins, (const unsigned *)st.spectrum.thresholds, part + lay.bins);
    else
        hipLaunchKernelGGL(ps_bin_kernel<false>, dim3((unsigned)N), block, bin_lds, st.stream, (const double2 *)st.spectrum.modes[0],
                           (const double2 *)nullptr, N, n_bins, (const unsigned *)st.spectrum.thresholds, part + lay.bins);
    ASORA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ps_bin_final_kernel, dim3((unsigned)((nv * n_bins + PS_THREADS - 1) / PS_THREADS)), block, 0, st.stream,
                       (const double *)(part + lay.bins), N, n_bins, nv, res);
    ASORA_HIP_TRY(hipGetLastError());
    if (int rc = watch.mark()) return rc;

    ASORA_HIP_TRY(hipMemcpyAsync(st.spectrum.host, res, sizeof(double) * PS_RES_WORDS, hipMemcpyDeviceToHost, st.stream));
    if (field_out) ASORA_HIP_TRY(hipMemcpyAsync(field_out, field.get(), sizeof(double) * ncell, hipMemcpyDeviceToHost, st.stream));
    if (modes_out) ASORA_HIP_TRY(hipMemcpyAsync(modes_out, st.spectrum.modes[0], sizeof(double2) * nmodes, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    watch.read(st.spectrum.ms);

    const double *h = st.spectrum.host;
    std::memcpy(count, h + PS_COUNT * ASORA_BUBBLE_MAX_BINS, sizeof(unsigned long long) * n_bins);
    std::memcpy(sum_k, h + PS_SUM_K * ASORA_BUBBLE_MAX_BINS, sizeof(double) * n_bins);
    std::memcpy(sum_aa, h + PS_SUM_AA * ASORA_BUBBLE_MAX_BINS, sizeof(double) * n_bins);
    std::memcpy(moments_a, h + PS_RES_MOMENTS, sizeof(double) * 2);
    if (cross) {
        std::memcpy(sum_bb, h + PS_SUM_BB * ASORA_BUBBLE_MAX_BINS, sizeof(double) * n_bins);
        std::memcpy(sum_ab, h + PS_SUM_AB * ASORA_BUBBLE_MAX_BINS, sizeof(double) * n_bins);
        std::memcpy(moments_b, h + PS_RES_MOMENTS + 2, sizeof(double) * 2);
    }
    return 0;
}

int asora_debug_power_spectrum_ms(double *ms)
{
    clear_error();
    if (!ms) return fail(3, "debug_power_spectrum_ms: null pointer");
    for (int q = 0; q < ASORA_PS_STAGES; ++q) ms[q] = state().spectrum.ms[q];
    return 0;
}

} // extern "C"
