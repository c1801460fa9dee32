// plane_flux.hip -- plane-parallel ionising flux through a face of the box: the setting
// (asora_plane_flux / asora_get_plane_flux), its checks, and the sweep kernel -- a prefix march of the column density along a
// grid axis, one lane per ray, deposited into the rate accumulators of the point-source trace before any of its launches.
#include "rates_device.hpp"

namespace asora {

// One face's sweep.  A ray is (a, b): b runs along the memory-contiguous index of the layout the face uses, a along the
// other axis the march does not take; cell m of the ray (travel order) sits at a * stride_a + b + m' * stride_m, m' = m for
// a '-' face and N - 1 - m for a '+' face.
//   -x +x : the [i][j][k] grids, march i (stride N^2), a = j (stride N),   b = k
//   -y +y : the [i][j][k] grids, march j (stride N),   a = i (stride N^2), b = k
//   -z +z : the [k][j][i] twins, march k (stride N^2), a = j (stride N),   b = i  -- the x sweep on the twins
struct PlaneFluxParams {
    int N, reverse;
    unsigned stride_a, stride_m;       // elements; N^3 < 2^32 is checked by the launcher
    const double *nabs;                // absorber density of the layout
    double *phi, *heat;                // accumulators of the same layout (heat: HEAT form only)
    const double2 *tab;                // the face's table set: thick | thin | heat thick | heat thin
    const double2 *logtab;
    double flux, sig, dr, numtau_f, lut_k1, lut_k0, lut_kc;
    int table_len, fortran_consts;
    const int *done;                   // device loop: the step has converged -> nothing to do; or nullptr
};

constexpr int PF_ROWS = 4;             // rays (a) per workgroup: one wave each
constexpr int PF_UNROLL = 8;           // cells whose loads and lookups are in flight at once

// The rate of a cell is photoion_rates (rates.cu:16-41; raytrace.hip: rate_issue / rate_value) with the path dr for the
// shell volume: pref = flux / (dr n_abs), thick: pref (T(tau_in) - T(tau_out)), thin: pref (tau_out - tau_in) T_thin(tau*).
// T_thick(tau_out) is looked up once and carried to the next cell as its T_thick(tau_in): the absorbed photons of a ray
// telescope exactly.  The only loop-carried values are the column density (one add per cell) and that carried table value;
// the PF_UNROLL loads of n_abs and of the accumulators, and the lookups, of a batch are independent of each other.
// Every cell is written by exactly one lane of one launch: the deposit is a plain load-add-store.
template <bool HEAT>
__global__ void __launch_bounds__(64 * PF_ROWS) plane_flux_kernel(const PlaneFluxParams p)
{
    __shared__ double2 logtab[LOG_TABLE_SIZE];
    if (p.done && *p.done) return;                                  // (uniform over the launch)
    for (int t = threadIdx.y * 64 + threadIdx.x; t < LOG_TABLE_SIZE; t += 64 * PF_ROWS) logtab[t] = p.logtab[t];
    __syncthreads();
    const int N = p.N;
    const int b = blockIdx.x * 64 + threadIdx.x, a = blockIdx.y * PF_ROWS + threadIdx.y;
    if (b >= N || a >= N) return;

    const double limit = p.fortran_consts ? (double)1.0e-7f : 1.0e-7;       // TAU_PHOTO_LIMIT (rates.cu:7 / photorates.f90:69)
    const double maxcd = p.fortran_consts ? (double)2e30f : 2e30;           // MAX_COLDENSH (raytracing.cu:15)
    const int thin_off = table_stride(p.table_len);
    const unsigned first = (unsigned)a * p.stride_a + (unsigned)b + (p.reverse ? (unsigned)(N - 1) * p.stride_m : 0u);
    const unsigned step = p.reverse ? 0u - p.stride_m : p.stride_m;       // (indices wrap modulo 2^32: N^3 < 2^32)

    double cd = 0.0, tau_in = 0.0;
    const Lookup L0 = lookup_issue<HEAT>(p.tab, 0.0, p, logtab, 0);
    double t_in = lookup_value(L0), h_in = HEAT ? lookup_heat(L0) : 0.0;

    for (int m0 = 0; m0 < N; m0 += PF_UNROLL) {
        const int cnt = N - m0 < PF_UNROLL ? N - m0 : PF_UNROLL;            // (uniform)
        const unsigned idx0 = first + (unsigned)m0 * step;
        double n[PF_UNROLL], acc[PF_UNROLL], hacc[PF_UNROLL];
#pragma unroll
        for (int u = 0; u < PF_UNROLL; ++u) {
            n[u] = 0.0; acc[u] = 0.0; hacc[u] = 0.0;
            if (u < cnt) {
                const unsigned idx = idx0 + (unsigned)u * step;
                n[u] = p.nabs[idx];
                acc[u] = p.phi[idx];
                if (HEAT) hacc[u] = p.heat[idx];
            }
        }
        // the column densities of the batch, in march order, every product and sum rounded on its own
        double vn[PF_UNROLL], tau[PF_UNROLL + 1];
        bool rated[PF_UNROLL];
        Lookup Lo[PF_UNROLL];
        tau[0] = tau_in;
        bool any_thin = false;
#pragma unroll
        for (int u = 0; u < PF_UNROLL; ++u) {
            vn[u] = mul_unfused(n[u], p.dr);
            rated[u] = cd <= maxcd;
            if (u < cnt) cd = add_unfused(cd, vn[u]);
            tau[u + 1] = mul_unfused(cd, p.sig);
            Lo[u] = lookup_issue<HEAT>(p.tab, tau[u + 1], p, logtab, 0);
            any_thin = any_thin || (u < cnt && !(fabs(tau[u + 1] - tau[u]) > limit));     // (the padding of a last batch has dtau = 0)
        }
        const bool wave_thin = __builtin_amdgcn_ballot_w64(any_thin) != 0ull;
#pragma unroll
        for (int u = 0; u < PF_UNROLL; ++u) {
            const double dtau = tau[u + 1] - tau[u];
            const bool thick = fabs(dtau) > limit;
            const double t_out = lookup_value(Lo[u]);
            const double h_out = HEAT ? lookup_heat(Lo[u]) : 0.0;
            // (n_abs = 0 -- a fully ionised or empty cell: the reference divides by zero; flux / +0 = flux * inf, as pref in raytrace.hip)
            const double pref = vn[u] == 0.0 ? p.flux * INFINITY : div_newton(p.flux, vn[u]);
            double v = pref * (t_in - t_out), h = pref * (h_in - h_out);
            if (wave_thin) {        // thin cells: the thin table at tau_out (rates.cu:37) or tau_in (photorates.f90:121)
                const Lookup Lt = lookup_issue<HEAT>(p.tab, p.fortran_consts ? tau[u] : tau[u + 1], p, logtab, thin_off);
                if (!thick) {
                    v = pref * dtau * lookup_value(Lt);
                    if (HEAT) h = pref * dtau * lookup_heat(Lt);
                }
            }
            if (u < cnt) {
                const unsigned idx = idx0 + (unsigned)u * step;
                if (rated[u]) {
                    p.phi[idx] = add_unfused(acc[u], v);
                    if (HEAT) p.heat[idx] = add_unfused(hacc[u], h);
                }
                t_in = t_out; h_in = h_out;
            }
        }
        tau_in = tau[PF_UNROLL];    // (only read while cnt == PF_UNROLL)
    }
}

// The tables of a lookup as launch_raytrace sets them (lut_index_constants)
static void fill_lookup(PlaneFluxParams &k, const RtParams &p)
{
    k.numtau_f = p.numtau_f;
    const LutIndex lut = lut_index_constants(p.minlogtau, p.dlogtau);
    k.lut_k1 = lut.k1; k.lut_k0 = lut.k0; k.lut_kc = lut.kc;
    k.table_len = p.table_len;
    k.fortran_consts = p.fortran_consts;
}

int check_plane_flux(const State &st, const PlaneFluxSet &pf, const char *who, bool dump, bool heat)
{
    if (pf.count == 0) return 0;
    const std::string w = std::string(who) + ": a plane-parallel flux (asora_plane_flux) ";
    if (st.opt[ASORA_OPT_GREY_NOTABLES]) return fail(4, w + "needs table rates (grey opacity, ASORA_OPT_GREY_NOTABLES, is on)");
    if (dump) return fail(4, w + "has no column-density dump (the dump is of one point source)");
    if (!st.sources.tables) return fail(4, w + "needs the radiation tables on the device (photo_table_to_device)");
    if (heat && !st.sources.loaded.heat_tables) return fail(4, w + "with heating needs heating tables on the device (heat_table_to_device)");
    if (st.ncell >= ((size_t)1 << 32)) return fail(4, w + "is built for meshes below 2^32 cells");
    for (int q = 0; q < pf.count; ++q) {
        if (pf.spec[q] >= st.sources.loaded.num_spec)
            return fail(4, w + "has table set " + std::to_string(pf.spec[q]) + " but the device holds " + std::to_string(st.sources.loaded.num_spec) +
                               " (asora_spectra_to_device)");
        if (pf.face[q] >= 4 && !st.opt[ASORA_OPT_Z_TRANSPOSED])
            return fail(4, w + "through a z face needs the [k][j][i] twins (ASORA_OPT_Z_TRANSPOSED = 1)");
    }
    return 0;
}

int launch_plane_flux(State &st, const RtParams &p, double *phi, double *heat_acc, bool heat, const int *done)
{
    const PlaneFluxSet &pf = p.plane;
    if (pf.count == 0) return 0;
    if (int rc = check_plane_flux(st, pf, "raytrace", p.dump != nullptr, heat)) return rc;
    if (int rc = ensure_logtab(st)) return rc;
    KernelTimer kt(ASORA_KERNEL_RAYTRACE);
    const int N = p.N;
    for (int q = 0; q < pf.count; ++q) {
        const int axis = pf.face[q] >> 1;
        PlaneFluxParams k;
        std::memset(&k, 0, sizeof k);
        k.N = N; k.reverse = pf.face[q] & 1;
        k.stride_m = axis == 1 ? (unsigned)N : (unsigned)N * (unsigned)N;
        k.stride_a = axis == 1 ? (unsigned)N * (unsigned)N : (unsigned)N;
        const size_t twin = axis == 2 ? (size_t)p.ncell : 0;
        k.nabs = p.nhi + twin; k.phi = phi + twin; k.heat = heat ? heat_acc + twin : nullptr;
        k.tab = p.tables + (size_t)pf.spec[q] * p.spec_stride;
        k.logtab = st.logtab_dev;
        k.flux = pf.flux[q]; k.sig = p.sig; k.dr = p.dr;
        fill_lookup(k, p);
        k.done = done;
        const dim3 grid((N + 63) / 64, (N + PF_ROWS - 1) / PF_ROWS), block(64, PF_ROWS);
        if (heat) hipLaunchKernelGGL(plane_flux_kernel<true>, grid, block, 0, st.stream, k);
        else hipLaunchKernelGGL(plane_flux_kernel<false>, grid, block, 0, st.stream, k);
        ASORA_HIP_TRY(hipGetLastError());
    }
    return 0;
}

} // namespace asora

using namespace asora;

extern "C" {

int asora_plane_flux(int count, const int32_t *face, const double *flux, const int32_t *spectrum)
{
    clear_error();
    State &st = state();
    if (count < 0 || count > 6) return fail(3, "plane_flux: count must be 0 ... 6 (one entry per face at most)");
    if (count == 0) { st.medium.plane = PlaneFluxSet{}; return 0; }          // (also without a device: nothing to switch off)
    if (!face || !flux) return fail(3, "plane_flux: null face / flux");
    PlaneFluxSet pf{};
    for (int q = 0; q < count; ++q) {
        if (face[q] < 0 || face[q] > 5) return fail(3, "plane_flux: face must be 0 ... 5 (-x +x -y +y -z +z)");
        for (int r = 0; r < q; ++r) if (face[r] == face[q]) return fail(3, "plane_flux: a face is given twice");
        if (!(std::isfinite(flux[q]) && flux[q] >= 0.0)) return fail(3, "plane_flux: flux must be finite and >= 0");
        const int s = spectrum ? spectrum[q] : 0;
        if (s < 0 || s >= ASORA_MAX_SPECTRA) return fail(3, "plane_flux: spectrum index out of range");
        pf.face[q] = face[q]; pf.flux[q] = flux[q]; pf.spec[q] = s;
    }
    pf.count = count;
    if (int rc = require_init("plane_flux")) return rc;
    st.medium.plane = pf;
    return 0;
}

int asora_get_plane_flux(int *count, int32_t *face, double *flux, int32_t *spectrum)
{
    clear_error();
    const PlaneFluxSet &pf = state().medium.plane;
    if (count) *count = pf.count;
    for (int q = 0; q < pf.count; ++q) {
        if (face) face[q] = pf.face[q];
        if (flux) flux[q] = pf.flux[q];
        if (spectrum) spectrum[q] = pf.spec[q];
    }
    return 0;
}

} // extern "C"
