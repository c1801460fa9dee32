// chemistry_api.hip -- the chemistry passes as calls of their own (whole grid, a range of planes, the reference's global_pass),
// their reductions, and the switches of the pass: thermal mode, clumping and the Lyman-limit absorbers of the nHI it emits.
#include "asora_internal.hpp"

namespace asora {

// One temperature for the whole grid?  Probed once per upload of TEMP and set of chemistry constants (one pass over the
// grid + a 40-byte read-back); the tiled chemistry pass then needs neither the temperature loads nor pow/sqrt/exp.
// Clumping mode 1 (asora_clumping) folds its constant into bh00 first, as the launchers do for the per-cell path: brech0 =
// (C bh00) (T/1e4)^albpow, doric's order.
int ensure_temp_probe(double bh00, double albpow, double colh0, double temph0)
{
    State &st = state();
    const double clump = st.medium.clump_mode == 1 ? st.medium.clump_c : 1.0;
    const double b = clump * bh00;
    const double c[4] = {b, albpow, colh0, temph0};
    if (st.temp_probe.valid && std::memcmp(c, st.temp_probe.consts, sizeof c) == 0 && st.temp_probe.clump == clump) return 0;
    if (int rc = st.temp_probe.dev.allocate(8)) return rc;
    if (int rc = launch_temp_probe(st, st.grid[ASORA_GRID_TEMP], st.ncell, b, albpow, colh0, temph0, st.temp_probe.dev)) return rc;
    ASORA_HIP_TRY(hipMemcpyAsync(st.temp_probe.values, st.temp_probe.dev, sizeof(double) * 5, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    std::memcpy(st.temp_probe.consts, c, sizeof c);
    st.temp_probe.clump = clump;
    st.temp_probe.valid = true;
    return 0;
}

// What every tiled pass over the planes [i_begin, i_begin + i_count) is given, with or without a step of the device loop open:
// the constants chem[] = {dt, bh00, albpow, colh0, temph0, abu_c}, the grids of the medium, where the reductions go, and what
// the temperature probe found (ensure_temp_probe comes first).  Where the rates come from, and everything else, is the caller's.
ChemTileParams chem_tile_common(int i_begin, int i_count, const double chem[6])
{
    State &st = state();
    ChemTileParams p;
    p.N = st.N; p.i_begin = i_begin; p.i_end = i_begin + i_count;
    p.dt = chem[0]; p.bh00 = chem[1]; p.albpow = chem[2]; p.colh0 = chem[3]; p.temph0 = chem[4]; p.abu_c = chem[5];
    p.ndens = st.grid[ASORA_GRID_NDENS]; p.temp = st.grid[ASORA_GRID_TEMP]; p.xh = st.grid[ASORA_GRID_XH];
    p.xh_av = st.grid[ASORA_GRID_XH_AV]; p.xh_intermed = st.grid[ASORA_GRID_XH_INTERMED];
    p.red_partial = st.red_partial; p.red_final = st.red_final;
    p.uniform = (st.temp_probe.valid && st.temp_probe.values[0] != 0.0 && !st.opt[ASORA_OPT_NO_UNIFORM_T]) ? 1 : 0;
    p.uniform_T = st.temp_probe.values[1]; p.uniform_brech0 = st.temp_probe.values[2]; p.uniform_acolh0 = st.temp_probe.values[3];
    p.uniform_t_ok = st.temp_probe.values[4] != 0.0 ? 1 : 0;
    p.lls_a = st.medium.lls_a; p.lls_b = st.medium.lls_b;          // (the emit forms: nHI of the next trace as launch_prepare_nhi forms it)
    return p;
}

// the three reductions of the last pass, once it has run: blocking
static int read_reductions(int *conv_flag, double *sum_xh1, double *sum_xh0)
{
    State &st = state();
    ASORA_HIP_TRY(hipMemcpyAsync(st.red_host, st.red_final, sizeof(double) * 3, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    if (sum_xh1) *sum_xh1 = st.red_host[0];
    if (sum_xh0) *sum_xh0 = st.red_host[1];
    if (conv_flag) *conv_flag = (int)st.red_host[2];
    return 0;
}

// per-workgroup partial sums of the chemistry passes: room for `entries` doubles (what is enqueued may still write the old buffer)
int ensure_red_capacity(size_t entries) { return state().red_partial.reserve(entries, state().stream); }

} // namespace asora

using namespace asora;

extern "C" {

int asora_chemistry_device(double dt, double bh00, double albpow, double colh0, double temph0, double abu_c,
                           int *conv_flag, double *sum_xh1, double *sum_xh0)
{
    clear_error();
    if (int rc = require_init("chemistry_device")) return rc;
    State &st = state();
    if (int rc = require_grids("chemistry_device", {ASORA_GRID_NDENS, ASORA_GRID_TEMP, ASORA_GRID_XH, ASORA_GRID_XH_AV, ASORA_GRID_PHI_ION})) return rc;
    if (st.thermal.mode.on) {      // thermal form: the heating rates in, the end-of-step temperature out
        if (!st.grid[ASORA_GRID_PHI_HEAT] || !st.grid_valid[ASORA_GRID_PHI_HEAT])
            return fail(4, "chemistry_device: thermal mode needs the heating rates (ASORA_GRID_PHI_HEAT) on the device");
        if (int rc = ensure_optional_grid(ASORA_GRID_TEMP_END)) return rc;
    }
    st.grid_valid[ASORA_GRID_XH_INTERMED] = true;
    ChemParams p;
    p.ncell = st.ncell;
    p.dt = dt; p.bh00 = bh00; p.albpow = albpow; p.colh0 = colh0; p.temph0 = temph0; p.abu_c = abu_c;
    p.ndens = st.grid[ASORA_GRID_NDENS]; p.temp = st.grid[ASORA_GRID_TEMP]; p.xh = st.grid[ASORA_GRID_XH];
    p.phi = st.grid[ASORA_GRID_PHI_ION];
    p.xh_av = st.grid[ASORA_GRID_XH_AV]; p.xh_intermed = st.grid[ASORA_GRID_XH_INTERMED];
    p.red_partial = st.red_partial; p.red_final = st.red_final; p.red_blocks = st.red_blocks;
    if (st.thermal.mode.on) {
        p.thermal = true; p.th = st.thermal.mode.consts;
        p.phi_heat = st.grid[ASORA_GRID_PHI_HEAT]; p.temp_end = st.grid[ASORA_GRID_TEMP_END]; p.th_stats = st.thermal.stats_dev;
        ASORA_HIP_TRY(hipMemsetAsync(st.thermal.stats_dev, 0, 3 * sizeof(unsigned long long), st.stream));
        st.grid_valid[ASORA_GRID_TEMP_END] = true;
    }
    if (int rc = launch_chemistry(st, p, st.stream)) return rc;
    return read_reductions(conv_flag, sum_xh1, sum_xh0);
}

int asora_chemistry_range(double dt, double bh00, double albpow, double colh0, double temph0, double abu_c,
                          int i_begin, int i_count, int first)
{
    clear_error();
    if (int rc = require_init("chemistry_range")) return rc;
    State &st = state();
    if (st.thermal.mode.on) return fail(4, "chemistry_range: not available in thermal mode (single GPU: asora_chemistry_device or asora_evolve_*)");
    // (xh_intermed is only ever written by the pass: chemistry.f90:107)
    if (int rc = require_grids("chemistry_range", {ASORA_GRID_NDENS, ASORA_GRID_TEMP, ASORA_GRID_XH, ASORA_GRID_XH_AV, ASORA_GRID_PHI_ION})) return rc;
    st.grid_valid[ASORA_GRID_XH_INTERMED] = true;
    if (int rc = check_planes("chemistry_range", 4, "bad plane range", i_begin, i_count)) return rc;
    if (i_count == 0 && !first) return 0;
    if (i_count == 0) {       // an empty first slab still resets the reductions
        ASORA_HIP_TRY(hipMemsetAsync(st.red_final, 0, sizeof(double) * 3, st.stream));
        return 0;
    }
    if (int rc = ensure_red_capacity(3 * chemistry_tile_blocks(st, st.N, i_count))) return rc;    // (sized for every range at init)
    if (int rc = ensure_temp_probe(bh00, albpow, colh0, temph0)) return rc;
    const double chem[6] = {dt, bh00, albpow, colh0, temph0, abu_c};
    ChemTileParams p = chem_tile_common(i_begin, i_count, chem);
    p.xh_av_in = st.grid[ASORA_GRID_XH_AV];
    p.gamma = st.grid[ASORA_GRID_PHI_ION];
    p.accumulate = first ? 0 : 1;
    return launch_chemistry_tiles(st, p, st.stream);
}

int asora_chemistry_finish(int *conv_flag, double *sum_xh1, double *sum_xh0)
{
    clear_error();
    if (int rc = require_init("chemistry_finish")) return rc;
    return read_reductions(conv_flag, sum_xh1, sum_xh0);
}

void *asora_reduction_ptr(void) { return state().init ? (void *)state().red_final : nullptr; }

int c2ray_global_pass(double dt, const double *ndens, const double *temp, const double *xh, double *xh_av,
                      double *xh_intermed, const double *phi_ion, double bh00, double albpow, double colh0,
                      double temph0, double abu_c, int m1, int m2, int m3, int *conv_flag)
{
    clear_error();
    if (m1 < 1 || m2 < 1 || m3 < 1) return fail(3, "global_pass: bad mesh size");
    if (!ndens || !temp || !xh || !xh_av || !xh_intermed || !phi_ion) return fail(3, "global_pass: null grid");
    if (int rc = ensure_runtime()) return rc;
    State &st = state();
    const size_t ncell = (size_t)m1 * m2 * m3, bytes = ncell * sizeof(double);
    Scoped<double> d[6];
    const double *h[6] = {ndens, temp, xh, xh_av, xh_intermed, phi_ion};
    for (int g = 0; g < 6; ++g) {
        if (int rc = d[g].allocate(ncell)) return rc;
        hipError_t e = hipMemcpyAsync(d[g].get(), h[g], bytes, hipMemcpyHostToDevice, st.stream);
        if (e != hipSuccess) return fail(10, std::string("global_pass: ") + hipGetErrorString(e));
    }
    ChemParams p;
    p.ncell = ncell;
    p.dt = dt; p.bh00 = bh00; p.albpow = albpow; p.colh0 = colh0; p.temph0 = temph0; p.abu_c = abu_c;
    p.ndens = d[0].get(); p.temp = d[1].get(); p.xh = d[2].get(); p.xh_av = d[3].get(); p.xh_intermed = d[4].get(); p.phi = d[5].get();
    p.red_partial = st.red_partial; p.red_final = st.red_final; p.red_blocks = st.red_blocks;
    int rc = launch_chemistry(st, p, st.stream, false);     // (the reference's f2py boundary: no clumping argument)
    if (!rc) {
        hipError_t e = hipMemcpyAsync(xh_av, d[3].get(), bytes, hipMemcpyDeviceToHost, st.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(xh_intermed, d[4].get(), bytes, hipMemcpyDeviceToHost, st.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(st.red_host, st.red_final, sizeof(double) * 3, hipMemcpyDeviceToHost, st.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(st.stream);
        if (e != hipSuccess) rc = fail(10, std::string("global_pass: ") + hipGetErrorString(e));
    }
    if (!rc && conv_flag) *conv_flag = (int)st.red_host[2];
    return rc;
}

// ---------------------------------------------------------------------------------------------
// Thermal mode (include/asora_hip.h; chemistry.hip: chemistry_cell_thermal)
// ---------------------------------------------------------------------------------------------
int asora_thermal_params(int enable, double relative_denergy, double t_floor, int max_substeps, unsigned cooling_mask,
                         int compton, double t_cmb)
{
    clear_error();
    if (int rc = require_init("thermal_params")) return rc;
    State &st = state();
    if (!enable) { st.thermal.mode.on = false; return 0; }
    if (!st.sources.loaded.heat_tables || st.opt[ASORA_OPT_GREY_NOTABLES])
        return fail(4, "thermal_params: thermal mode needs heating tables on the device (heat_table_to_device) and table rates");
    if (!(relative_denergy > 0.0) || !(t_floor >= 0.0) || max_substeps < 1 || !(t_cmb >= 0.0) || cooling_mask > 31u)
        return fail(3, "thermal_params: need relative_denergy > 0, t_floor >= 0, max_substeps >= 1, t_cmb >= 0, cooling_mask < 32");
    if (!st.thermal.stats_dev) {
        if (int rc = st.thermal.stats_dev.allocate(3)) return rc;
        ASORA_HIP_TRY(hipMemsetAsync(st.thermal.stats_dev, 0, 3 * sizeof(unsigned long long), st.stream));
    }
    st.thermal.mode.consts.relative_denergy = relative_denergy; st.thermal.mode.consts.t_floor = t_floor; st.thermal.mode.consts.max_substeps = max_substeps;
    st.thermal.mode.consts.cooling_mask = cooling_mask; st.thermal.mode.consts.compton = compton ? 1 : 0; st.thermal.mode.consts.t_cmb = t_cmb;
    st.thermal.mode.on = true;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Clumping of the recombination rate (include/asora_hip.h; chemistry.hip: clumping_of)
// ---------------------------------------------------------------------------------------------
int asora_clumping(int mode, double constant)
{
    clear_error();
    State &st = state();
    if (mode == 0) { st.medium.clump_mode = 0; st.medium.clump_c = 1.0; return 0; }     // (also without a device: nothing to switch off)
    if (int rc = require_init("clumping")) return rc;
    if (mode == 1) {
        if (!(std::isfinite(constant) && constant > 0.0)) return fail(3, "clumping: the constant must be finite and > 0");
        st.medium.clump_mode = 1; st.medium.clump_c = constant;
        return 0;
    }
    if (mode == 2) {
        if (!st.grid[ASORA_GRID_CLUMP] || !st.grid_valid[ASORA_GRID_CLUMP])
            return fail(4, "clumping: mode 2 needs the factors on the device (asora_grid_to_device(ASORA_GRID_CLUMP, ...))");
        st.medium.clump_mode = 2; st.medium.clump_c = 1.0;
        return 0;
    }
    return fail(3, "clumping: mode must be 0 (off), 1 (constant) or 2 (per cell)");
}

// ---------------------------------------------------------------------------------------------
// Lyman-limit-system opacity (include/asora_hip.h; rates_device.hpp: absorber_density)
// ---------------------------------------------------------------------------------------------
int asora_lls_opacity(double n_const, double per_density)
{
    clear_error();
    State &st = state();
    if (!(std::isfinite(n_const) && n_const >= 0.0 && std::isfinite(per_density) && per_density >= 0.0))
        return fail(3, "lls_opacity: n_const and per_density must be finite and >= 0");
    if (n_const == 0.0 && per_density == 0.0) { st.medium.lls_a = st.medium.lls_b = 0.0; return 0; }   // (also without a device: nothing to switch off)
    if (int rc = require_init("lls_opacity")) return rc;
    if (st.opt[ASORA_OPT_GREY_NOTABLES])
        return fail(4, "lls_opacity: needs table rates (grey opacity, ASORA_OPT_GREY_NOTABLES, is on)");
    st.medium.lls_a = n_const; st.medium.lls_b = per_density;
    return 0;
}

int asora_get_lls_opacity(double *n_const, double *per_density)
{
    clear_error();
    if (n_const) *n_const = state().medium.lls_a;
    if (per_density) *per_density = state().medium.lls_b;
    return 0;
}

int asora_thermal_stats(long long *cells_max_substeps, long long *cells_floored, int *max_substeps_used)
{
    clear_error();
    if (int rc = require_init("thermal_stats")) return rc;
    State &st = state();
    unsigned long long h[3] = {0, 0, 0};
    if (st.thermal.stats_dev) {
        ASORA_HIP_TRY(hipMemcpyAsync(h, st.thermal.stats_dev, sizeof h, hipMemcpyDeviceToHost, st.stream));
        ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    }
    if (cells_max_substeps) *cells_max_substeps = (long long)h[0];
    if (cells_floored) *cells_floored = (long long)h[1];
    if (max_substeps_used) *max_substeps_used = (int)h[2];
    return 0;
}

} // extern "C"
