// bispectrum.hip -- the bispectrum of a field formed from the device grids by the FFT triangle estimator (asora_bispectrum; DESIGN.md
// section 4.2l): for every k-shell the field filtered to the shell is transformed back to a real cube, and the product of three
// cubes is summed over the cells for every triangle of shells; the same with the spectrum set to 1 counts the closed triples.
// The forward half and the per-shell sums are the power spectrum's (ps_forward, ps_bin_auto: power_spectrum.hip) and the spectrum
// stays where they leave it, State::spectrum.modes[0], read only.  The stages written here, on the library's stream behind those:
//   e. back along i : bs_back_i_kernel, out of place: a workgroup takes T columns (n_y, n_z) of the kept spectrum, multiplies by the
//                     shell's 0/1 indicator on the load, conjugates (fft_device.hpp: the butterflies have the forward sign), transforms
//                     and stores the conjugate into the work buffer.  Only the columns with m_y < lim and n_z < lim are visited, lim
//                     the smallest integer with lim^2 >= thresholds[a + 1]: every other column of the shell is zero;
//   f. back along j : bs_back_j_kernel, in place in the work buffer: only the tiles with n_z < lim, and of a line only the n_y with
//                     m_y < lim are loaded -- the rest enters LDS as zeros;
//   g. back along k : bs_c2r_kernel, the row pass of the smoothing without its statistics: n_z >= lim enters as zeros; Re / N^3 goes
//                     into the shell's cube;
//   h. products     : bs_product_kernel, a fixed grid of BS_BLOCKS workgroups over tiles of 256 cells: a tile's values of every
//                     shell the pass uses are loaded once into LDS, and each of the four waves accumulates its own BS_WAVE_CHUNK
//                     triangles in registers as double-double, so a pass over the cubes serves BS_CHUNK = 128 triangles; a wave's
//                     lanes are folded by a shuffle tree and bs_fold_kernel (one workgroup per triangle) adds the workgroups'
//                     partials in index order.
// For the counts the same stages run with 1 in the place of the spectrum (no forward transform, no load in stage e).
// Every sum is double-double in an order fixed by (N, thresholds, tri); no atomic of any kind.
#include "asora_internal.hpp"
#include "fft_device.hpp"

#include <cstring>

namespace asora {

constexpr int BS_WAVE_CHUNK = 32;                     // triangles a wave holds in registers (64 doubles of accumulators)
constexpr int BS_CHUNK = PS_WAVES * BS_WAVE_CHUNK;    // triangles of one pass over the cubes
constexpr int BS_BLOCKS = 512;                        // the workgroups of the product kernel: a constant, so that the order is the mesh's alone
constexpr int BS_TILE = PS_THREADS;                   // cells of a tile

// the smallest m in [0, floor(N/2) + 1] with m^2 >= hi (floor(N/2) + 1 if there is none): folded indices at or beyond it lie outside
static int bs_limit(unsigned hi, int N)
{
    int m = 0;
    while (m < N / 2 + 1 && (unsigned)(m * m) < hi) ++m;
    return m;
}

// the pass back along i for one shell, out of place: column c of the ny_cnt lim visited ones is (n_y, n_z) with n_z = c mod lim and
// n_y the (c / lim)-th of 0 ... lim - 1, N - (ny_cnt - lim) ... N - 1.  INDICATOR: the spectrum is 1.  Dynamic LDS: roots [N], two
// line buffers [T pitch], then per column of the tile its offset n_y NZ + n_z and m_y^2 + n_z^2
template <bool INDICATOR>
__global__ void __launch_bounds__(PS_THREADS) bs_back_i_kernel(const double2 *__restrict__ modes, double2 *__restrict__ work, int N, int pitch,
                                                                int T, PsPlan plan, const double2 *__restrict__ twiddle, unsigned lo,
                                                                unsigned hi, int lim, int ny_cnt)
{
    extern __shared__ double2 ps_lds[];
    double2 *tw, *a, *b;
    ps_lds_layout(ps_lds, twiddle, N, pitch, T, tw, a, b);
    int *col = (int *)(b + (size_t)T * pitch);
    const int NZ = N / 2 + 1, ncols = ny_cnt * lim, c0 = (int)blockIdx.x * T;
    const int width = ncols - c0 < T ? ncols - c0 : T;
    for (int t = threadIdx.x; t < width; t += PS_THREADS) {
        const int c = c0 + t, q = c / lim, nz = c - q * lim, ny = q < lim ? q : N - ny_cnt + q, my = min(ny, N - ny);
        col[2 * t] = ny * NZ + nz;
        col[2 * t + 1] = my * my + nz * nz;
    }
    __syncthreads();
    const size_t stride = (size_t)N * NZ;
    for (int w = threadIdx.x; w < width * N; w += PS_THREADS) {
        const int e = w / width, t = w - e * width, mx = min(e, N - e);
        const unsigned n2 = (unsigned)(mx * mx + col[2 * t + 1]);
        double2 v = make_double2(0.0, 0.0);
        if (n2 >= lo && n2 < hi) {
            if constexpr (INDICATOR) v = make_double2(1.0, 0.0);
            else {
                const double2 m = modes[e * stride + col[2 * t]];
                v = make_double2(m.x, -m.y);
            }
        }
        a[t * pitch + e] = v;
    }
    const double2 *res = line_fft(a, b, tw, plan, N, pitch, width);
    for (int w = threadIdx.x; w < width * N; w += PS_THREADS) {
        const int e = w / width, t = w - e * width;
        const double2 v = res[t * pitch + e];
        work[e * stride + col[2 * t]] = make_double2(v.x, -v.y);
    }
}

// the pass back along j, in place: plane x = blockIdx.x / tiles, the columns n_z = c0 ... c0 + width - 1 < lim; of the N elements
// of a line those with m_y >= lim are zero and are not read
__global__ void __launch_bounds__(PS_THREADS) bs_back_j_kernel(double2 *__restrict__ work, int N, int pitch, int T, PsPlan plan,
                                                                const double2 *__restrict__ twiddle, int lim, unsigned tiles)
{
    extern __shared__ double2 ps_lds[];
    double2 *tw, *a, *b;
    ps_lds_layout(ps_lds, twiddle, N, pitch, T, tw, a, b);
    const int NZ = N / 2 + 1;
    const unsigned plane = blockIdx.x / tiles;
    const int c0 = (int)(blockIdx.x - plane * tiles) * T;
    const int width = lim - c0 < T ? lim - c0 : T;
    double2 *g = work + (size_t)plane * N * NZ + c0;
    for (int w = threadIdx.x; w < width * N; w += PS_THREADS) {
        const int e = w / width, t = w - e * width, my = min(e, N - e);
        double2 v = make_double2(0.0, 0.0);
        if (my < lim) {
            const double2 m = g[(size_t)e * NZ + t];
            v = make_double2(m.x, -m.y);
        }
        a[t * pitch + e] = v;
    }
    const double2 *res = line_fft(a, b, tw, plan, N, pitch, width);
    for (int w = threadIdx.x; w < width * N; w += PS_THREADS) {
        const int e = w / width, t = w - e * width;
        const double2 v = res[t * pitch + e];
        g[(size_t)e * NZ + t] = make_double2(v.x, -v.y);
    }
}

// the pass back along k: workgroup b takes the rows b T ... b T + T - 1 of the N^2 rows (i, j) to N real cells each, d = Re / N^3;
// the stored values n_z >= lim are zero and are not read
__global__ void __launch_bounds__(PS_THREADS) bs_c2r_kernel(const double2 *__restrict__ work, int N, int pitch, int T, PsPlan plan,
                                                             const double2 *__restrict__ twiddle, int lim, double *__restrict__ cube)
{
    extern __shared__ double2 ps_lds[];
    double2 *tw, *a, *b;
    ps_lds_layout(ps_lds, twiddle, N, pitch, T, tw, a, b);
    const int NZ = N / 2 + 1;
    const size_t rows = (size_t)N * N, row0 = (size_t)blockIdx.x * T;
    const int nl = (int)(rows - row0 < (size_t)T ? rows - row0 : (size_t)T);
    for (int w = threadIdx.x; w < nl * NZ; w += PS_THREADS) {
        const int t = w / NZ, kz = w - t * NZ;
        const double2 v = kz < lim ? work[(row0 + t) * (size_t)NZ + kz] : make_double2(0.0, 0.0);
        if (kz == 0 || 2 * kz == N) {
            a[t * pitch + kz] = make_double2(v.x, 0.0);        // its own partner: real
        } else {
            a[t * pitch + kz] = make_double2(v.x, -v.y);       // conj of the stored value
            a[t * pitch + N - kz] = v;                         // conj of its partner conj(v)
        }
    }
    const double2 *res = line_fft(a, b, tw, plan, N, pitch, nl);
    const double n3 = (double)N * (double)N * (double)N;
    for (int w = threadIdx.x; w < nl * N; w += PS_THREADS) {
        const int t = w / N, k = w - t * N;
        cube[(row0 + t) * (size_t)N + k] = res[t * pitch + k].x / n3;
    }
}

// One pass over the cubes for the triangles first ... first + count - 1 (count <= BS_CHUNK) of tri, one word a | b << 8 | c << 16
// each.  Wave w of a workgroup takes the triangles first + w per ... of them, per = ceil(count / 4).  Workgroup g takes the tiles g,
// g + BS_BLOCKS, ... of 256 cells; thread t loads cell t of the tile of every shell in `used` into LDS [n_shells][256], and every
// wave then adds (d_a d_b) d_c of the cells lane, 64 + lane, 128 + lane, 192 + lane to its triangles' accumulators.  Cells past the
// end enter as 0.  partial[((triangle) BS_BLOCKS + g) 2 ...] = the wave's sum (hi, lo), its lanes folded by a shuffle tree
__global__ void __launch_bounds__(PS_THREADS) bs_product_kernel(const double *__restrict__ cubes, size_t ncell, int n_shells, unsigned used,
                                                                 const int32_t *__restrict__ tri, int first, int count,
                                                                 double *__restrict__ partial)
{
    extern __shared__ double bs_vals[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int per = (count + PS_WAVES - 1) / PS_WAVES, t0 = wave * per;
    const int mine = count - t0 < per ? (count - t0 > 0 ? count - t0 : 0) : per;
    int pk[BS_WAVE_CHUNK];
    dd acc[BS_WAVE_CHUNK];
#pragma unroll
    for (int q = 0; q < BS_WAVE_CHUNK; ++q) {
        pk[q] = q < mine ? __builtin_amdgcn_readfirstlane(tri[first + t0 + q]) : 0;
        acc[q].hi = 0.0; acc[q].lo = 0.0;
    }
    const size_t tiles = (ncell + BS_TILE - 1) / BS_TILE;
    for (size_t tile = blockIdx.x; tile < tiles; tile += BS_BLOCKS) {
        const size_t cell = tile * BS_TILE + threadIdx.x;
        __syncthreads();                                       // (the tile before has been read)
        for (int s = 0; s < n_shells; ++s)
            if ((used >> s) & 1u) bs_vals[s * BS_TILE + threadIdx.x] = cell < ncell ? cubes[(size_t)s * ncell + cell] : 0.0;
        __syncthreads();
        for (int sub = 0; sub < BS_TILE / 64; ++sub) {
            const double *v = bs_vals + sub * 64 + lane;
#pragma unroll
            for (int q = 0; q < BS_WAVE_CHUNK; ++q) {
#pragma clang fp contract(off)
                if (q < mine) {
                    const double da = v[(pk[q] & 0xff) * BS_TILE], db = v[((pk[q] >> 8) & 0xff) * BS_TILE], dc = v[((pk[q] >> 16) & 0xff) * BS_TILE];
                    dd_add(acc[q], (da * db) * dc);
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < BS_WAVE_CHUNK; ++q) {
        if (q < mine) {
            dd v = acc[q];
            for (int o = 32; o > 0; o >>= 1) {
                dd other;
                other.hi = __shfl_down(v.hi, o);
                other.lo = __shfl_down(v.lo, o);
                dd_merge(v, other);
            }
            if (lane == 0) {
                double *p = partial + ((size_t)(first + t0 + q) * BS_BLOCKS + blockIdx.x) * 2;
                p[0] = v.hi; p[1] = v.lo;
            }
        }
    }
}

// out[t] = ((the BS_BLOCKS partials of triangle t = blockIdx.x added in index order) N^3) N^3: sm_fold_kernel's order, one workgroup
// per triangle
__global__ void __launch_bounds__(PS_THREADS) bs_fold_kernel(const double *__restrict__ partial, double n3, double *__restrict__ out)
{
    const double *mine = partial + (size_t)blockIdx.x * BS_BLOCKS * 2;
    dd s = {0.0, 0.0};
    for (int e = threadIdx.x; e < BS_BLOCKS; e += PS_THREADS) {
        dd o = {mine[2 * e], mine[2 * e + 1]};
        dd_merge(s, o);
    }
    s = ps_block_sum(s);
    if (threadIdx.x == 0) out[blockIdx.x] = ((s.hi + s.lo) * n3) * n3;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// the doubles of the pinned area: sum_ggg, sum_iii [MAX_TRIANGLES each], count, sum_k, sum_aa [MAX_SHELLS each], the moments [2],
// then the packed triangles (int32)
constexpr size_t BS_HOST_GGG = 0, BS_HOST_III = ASORA_BISPEC_MAX_TRIANGLES, BS_HOST_COUNT = 2 * (size_t)ASORA_BISPEC_MAX_TRIANGLES,
                 BS_HOST_K = BS_HOST_COUNT + ASORA_BISPEC_MAX_SHELLS, BS_HOST_AA = BS_HOST_K + ASORA_BISPEC_MAX_SHELLS,
                 BS_HOST_MOMENTS = BS_HOST_AA + ASORA_BISPEC_MAX_SHELLS, BS_HOST_TRI = BS_HOST_MOMENTS + 2,
                 BS_HOST_WORDS = BS_HOST_TRI + ASORA_BISPEC_MAX_TRIANGLES / 2;

struct BsPlan {
    int passes;
    size_t tiles;
    BsPlan(int N, int n_tri) : passes((n_tri + BS_CHUNK - 1) / BS_CHUNK), tiles(((size_t)N * N * N + BS_TILE - 1) / BS_TILE) {}
};

// the shell fields of one side into st.bispectrum.cubes, then the triangles' sums into out_dev [n_tri]
static int bs_side(State &st, bool indicator, int n_shells, const unsigned *thr, unsigned used_any, int n_tri, const unsigned *pass_used,
                   double *out_dev, const std::function<int()> &stage_done)
{
    const int N = st.N, T = ps_tile(N), pitch = N | 1;
    const PsPlan plan = ps_plan(N);
    const size_t ncell = st.ncell, fft_lds = ((size_t)2 * T * pitch + N) * sizeof(double2), col_lds = fft_lds + 2 * (size_t)T * sizeof(int);
    const dim3 block(PS_THREADS);
    const double2 *twiddle = st.spectrum.twiddle;
    double2 *work = st.bispectrum.work;
    const unsigned row_blocks = (unsigned)(((size_t)N * N + T - 1) / T);
    for (int a = 0; a < n_shells; ++a) {
        if (!((used_any >> a) & 1u)) continue;                     // (no triangle reads it)
        double *cube = st.bispectrum.cubes + (size_t)a * ncell;
        if (thr[a] == thr[a + 1]) {                                // an empty shell: d = 0
            ASORA_HIP_TRY(hipMemsetAsync(cube, 0, sizeof(double) * ncell, st.stream));
            continue;
        }
        const int lim = bs_limit(thr[a + 1], N), ny_cnt = 2 * lim - 1 < N ? 2 * lim - 1 : N;
        const unsigned tiles_i = (unsigned)((ny_cnt * lim + T - 1) / T), tiles_j = (unsigned)((lim + T - 1) / T);
        if (indicator)
            hipLaunchKernelGGL(bs_back_i_kernel<true>, dim3(tiles_i), block, col_lds, st.stream, (const double2 *)nullptr, work, N, pitch, T,
                               plan, twiddle, thr[a], thr[a + 1], lim, ny_cnt);
        else
            hipLaunchKernelGGL(bs_back_i_kernel<false>, dim3(tiles_i), block, col_lds, st.stream, (const double2 *)st.spectrum.modes[0], work, N,
                               pitch, T, plan, twiddle, thr[a], thr[a + 1], lim, ny_cnt);
        ASORA_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(bs_back_j_kernel, dim3((unsigned)N * tiles_j), block, fft_lds, st.stream, work, N, pitch, T, plan, twiddle, lim,
                           tiles_j);
        ASORA_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(bs_c2r_kernel, dim3(row_blocks), block, fft_lds, st.stream, (const double2 *)work, N, pitch, T, plan, twiddle, lim,
                           cube);
        ASORA_HIP_TRY(hipGetLastError());
    }
    if (int rc = stage_done()) return rc;
    const BsPlan bp(N, n_tri);
    const size_t prod_lds = sizeof(double) * (size_t)n_shells * BS_TILE;
    for (int p = 0; p < bp.passes; ++p) {
        const int first = p * BS_CHUNK, count = n_tri - first < BS_CHUNK ? n_tri - first : BS_CHUNK;
        hipLaunchKernelGGL(bs_product_kernel, dim3(BS_BLOCKS), block, prod_lds, st.stream, (const double *)st.bispectrum.cubes, ncell, n_shells,
                           pass_used[p], (const int32_t *)st.bispectrum.tri, first, count, (double *)st.bispectrum.partial);
        ASORA_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(bs_fold_kernel, dim3((unsigned)n_tri), block, 0, st.stream, (const double *)st.bispectrum.partial,
                       (double)N * (double)N * (double)N, out_dev);
    ASORA_HIP_TRY(hipGetLastError());
    return stage_done();
}

} // namespace asora

using namespace asora;

extern "C" {

int asora_bispectrum(int kind, double scale, double t_gamma, int n_shells, const unsigned *thresholds, int n_tri, const int32_t *tri,
                     double *sum_ggg, double *sum_iii, unsigned long long *count, double *sum_k, double *sum_aa, double *moments)
{
    clear_error();
    if (int rc = require_init("bispectrum")) return rc;
    if (kind < 0 || kind >= ASORA_PS_KINDS) return fail(3, "bispectrum: kind must be one of ASORA_PS_*");
    if (!std::isfinite(scale)) return fail(3, "bispectrum: scale must be finite");
    if (!std::isfinite(t_gamma) || t_gamma < 0.0) return fail(3, "bispectrum: t_gamma must be finite and >= 0");
    if (n_shells < 1 || n_shells > ASORA_BISPEC_MAX_SHELLS)
        return fail(3, "bispectrum: n_shells must be in [1, " + std::to_string(ASORA_BISPEC_MAX_SHELLS) + "]");
    if (n_tri < 1 || n_tri > ASORA_BISPEC_MAX_TRIANGLES)
        return fail(3, "bispectrum: n_tri must be in [1, " + std::to_string(ASORA_BISPEC_MAX_TRIANGLES) + "]");
    if (!thresholds || !tri || !sum_ggg || !sum_iii || !count || !sum_k || !sum_aa || !moments)
        return fail(3, "bispectrum: null thresholds, tri or output pointer");
    if (thresholds[0] < 1u) return fail(3, "bispectrum: thresholds[0] must be >= 1 (the mode n = 0 belongs to no shell)");
    for (int b = 0; b < n_shells; ++b)
        if (thresholds[b + 1] < thresholds[b]) return fail(3, "bispectrum: the thresholds must be non-decreasing");
    for (int q = 0; q < 3 * n_tri; ++q)
        if (tri[q] < 0 || tri[q] >= n_shells)
            return fail(3, "bispectrum: tri[" + std::to_string(q) + "] = " + std::to_string(tri[q]) + " is no shell index in [0, " +
                               std::to_string(n_shells) + ")");
    State &st = state();
    const int grids[3] = {ASORA_GRID_XH, ASORA_GRID_NDENS, ASORA_GRID_TEMP};
    for (int q = 0; q < 3; ++q)
        if (ps_needs_grid(kind, grids[q], t_gamma) && (!st.grid[grids[q]] || !st.grid_valid[grids[q]]))
            return fail(4, "bispectrum: grid " + std::to_string(grids[q]) + " holds no data");
    if (st.N > ASORA_REGION_MAX_N)
        return fail(4, "bispectrum: not built for N > " + std::to_string(ASORA_REGION_MAX_N) + " (a line and its roots must fit LDS)");

    const int N = st.N, T = ps_tile(N), pitch = N | 1;
    const size_t ncell = st.ncell, nmodes = (size_t)N * N * (N / 2 + 1);
    State::Bispectrum &bs = st.bispectrum;
    const BsPlan bp(N, n_tri);
    if (int rc = bs.work.allocate(nmodes)) return rc;
    if (int rc = bs.cubes.reserve((size_t)n_shells * ncell, st.stream)) return rc;
    if (int rc = bs.partial.reserve((size_t)n_tri * BS_BLOCKS * 2, st.stream)) return rc;
    if (int rc = bs.result.allocate(2 * (size_t)ASORA_BISPEC_MAX_TRIANGLES)) return rc;
    if (int rc = bs.tri.allocate((size_t)ASORA_BISPEC_MAX_TRIANGLES)) return rc;
    if (int rc = bs.host.allocate(BS_HOST_WORDS)) return rc;
    const size_t fft_lds = ((size_t)2 * T * pitch + N) * sizeof(double2), col_lds = fft_lds + 2 * (size_t)T * sizeof(int);
    ASORA_HIP_TRY(hipFuncSetAttribute((const void *)bs_back_i_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)col_lds));
    ASORA_HIP_TRY(hipFuncSetAttribute((const void *)bs_back_i_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)col_lds));
    ASORA_HIP_TRY(hipFuncSetAttribute((const void *)bs_back_j_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fft_lds));
    ASORA_HIP_TRY(hipFuncSetAttribute((const void *)bs_c2r_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fft_lds));
    ASORA_HIP_TRY(hipFuncSetAttribute((const void *)bs_product_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)(sizeof(double) * ASORA_BISPEC_MAX_SHELLS * BS_TILE)));

    // the triangles, one word each, leave through the pinned area; the shells a pass reads, and those any pass reads
    int32_t *tri_host = (int32_t *)(bs.host + BS_HOST_TRI);
    std::vector<unsigned> pass_used((size_t)bp.passes, 0u);
    unsigned used_any = 0u;
    for (int t = 0; t < n_tri; ++t) {
        const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
        tri_host[t] = a | (b << 8) | (c << 16);
        pass_used[(size_t)(t / BS_CHUNK)] |= (1u << a) | (1u << b) | (1u << c);
    }
    for (unsigned u : pass_used) used_any |= u;
    ASORA_HIP_TRY(hipMemcpyAsync(bs.tri, tri_host, sizeof(int32_t) * n_tri, hipMemcpyHostToDevice, st.stream));

    State::Bispectrum::Cache &cache = bs.cache;
    const bool cached = cache.N == N && cache.thresholds.size() == (size_t)n_shells + 1 && cache.tri.size() == 3 * (size_t)n_tri &&
                        std::memcmp(cache.thresholds.data(), thresholds, sizeof(unsigned) * (n_shells + 1)) == 0 &&
                        std::memcmp(cache.tri.data(), tri, sizeof(int32_t) * 3 * n_tri) == 0;

    StageStopwatch<ASORA_BISPEC_STAGES> watch(st.opt[ASORA_OPT_TIMING] != 0, st.stream);
    auto mark = [&watch]() { return watch.mark(); };
    if (int rc = watch.mark()) return rc;
    const double *moments_dev = nullptr, *sum_k_dev = nullptr, *sum_aa_dev = nullptr;
    const unsigned long long *count_dev = nullptr;
    if (int rc = ps_forward(st, kind, scale, t_gamma, mark, &moments_dev)) return rc;
    if (int rc = ps_bin_auto(st, n_shells, thresholds, &count_dev, &sum_k_dev, &sum_aa_dev)) return rc;
    if (int rc = watch.mark()) return rc;
    double *res = bs.result;
    if (int rc = bs_side(st, false, n_shells, thresholds, used_any, n_tri, pass_used.data(), res, mark)) return rc;
    if (cached) {
        if (int rc = watch.mark()) return rc;
        if (int rc = watch.mark()) return rc;
    } else if (int rc = bs_side(st, true, n_shells, thresholds, used_any, n_tri, pass_used.data(), res + ASORA_BISPEC_MAX_TRIANGLES, mark))
        return rc;

    double *h = bs.host;
    ASORA_HIP_TRY(hipMemcpyAsync(h + BS_HOST_GGG, res, sizeof(double) * n_tri, hipMemcpyDeviceToHost, st.stream));
    if (!cached)
        ASORA_HIP_TRY(hipMemcpyAsync(h + BS_HOST_III, res + ASORA_BISPEC_MAX_TRIANGLES, sizeof(double) * n_tri, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipMemcpyAsync(h + BS_HOST_COUNT, count_dev, sizeof(double) * n_shells, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipMemcpyAsync(h + BS_HOST_K, sum_k_dev, sizeof(double) * n_shells, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipMemcpyAsync(h + BS_HOST_AA, sum_aa_dev, sizeof(double) * n_shells, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipMemcpyAsync(h + BS_HOST_MOMENTS, moments_dev, sizeof(double) * 2, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    watch.read(bs.ms);
    if (cached) bs.ms[ASORA_BISPEC_STAGES - 2] = bs.ms[ASORA_BISPEC_STAGES - 1] = 0.0;
    else {
        cache.N = N;
        cache.thresholds.assign(thresholds, thresholds + n_shells + 1);
        cache.tri.assign(tri, tri + 3 * (size_t)n_tri);
        cache.sum_iii.assign(h + BS_HOST_III, h + BS_HOST_III + n_tri);
    }

    std::memcpy(sum_ggg, h + BS_HOST_GGG, sizeof(double) * n_tri);
    std::memcpy(sum_iii, cache.sum_iii.data(), sizeof(double) * n_tri);
    std::memcpy(count, h + BS_HOST_COUNT, sizeof(unsigned long long) * n_shells);
    std::memcpy(sum_k, h + BS_HOST_K, sizeof(double) * n_shells);
    std::memcpy(sum_aa, h + BS_HOST_AA, sizeof(double) * n_shells);
    std::memcpy(moments, h + BS_HOST_MOMENTS, sizeof(double) * 2);
    return 0;
}

int asora_debug_bispectrum_ms(double *ms)
{
    clear_error();
    if (!ms) return fail(3, "debug_bispectrum_ms: null pointer");
    for (int q = 0; q < ASORA_BISPEC_STAGES; ++q) ms[q] = state().bispectrum.ms[q];
    return 0;
}

int asora_debug_bispectrum_plan(int N, int n_shells, int n_tri, int32_t *out)
{
    clear_error();
    if (!out) return fail(3, "debug_bispectrum_plan: null pointer");
    if (N < 2 || N > ASORA_REGION_MAX_N || n_shells < 1 || n_shells > ASORA_BISPEC_MAX_SHELLS || n_tri < 1 || n_tri > ASORA_BISPEC_MAX_TRIANGLES)
        return fail(3, "debug_bispectrum_plan: N, n_shells or n_tri outside what asora_bispectrum takes");
    const BsPlan bp(N, n_tri);
    out[0] = BS_CHUNK;
    out[1] = bp.passes;
    out[2] = BS_BLOCKS;
    out[3] = (int32_t)((bp.tiles + BS_BLOCKS - 1) / BS_BLOCKS);
    out[4] = (int32_t)(bp.tiles / BS_BLOCKS);
    out[5] = BS_WAVE_CHUNK;
    out[6] = BS_TILE;
    out[7] = bp.tiles < (size_t)BS_BLOCKS ? (int32_t)(BS_BLOCKS - bp.tiles) : 0;
    return 0;
}

} // extern "C"
