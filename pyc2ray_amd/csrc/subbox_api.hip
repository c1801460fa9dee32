// subbox_api.hip -- the raytrace with the reference's CPU semantics (cubic sub-boxes, photon loss): the host driver of the sweep,
// its f2py-shaped entry point c2ray_do_all_sources and the device-resident asora_subbox_raytrace_device.
#include "asora_internal.hpp"
#include "rates_device.hpp"


namespace asora {

// ---------------------------------------------------------------------------------------------
// Host driver of subbox.hip on device-resident inputs (do_all_sources / do_source,
// src/c2ray/raytracing.f90:52-249): NDENS and XH_AV on the device, tables and sources given as device pointers.
// ---------------------------------------------------------------------------------------------
struct SubboxCall {
    int max_subbox, subboxsize;
    float loss_fraction;
    double sig, dr, R, minlogtau, dlogtau;
    int NumTau, table_len;
    const double2 *tables;          // [thick | thin | heat thick | heat thin] pairs, table_len each
    const int32_t *src_pos;         // 0-based, xyz-interleaved
    const int32_t *host_pos;        // the same list on the host (pairing of sources for the line-aligned tables), or nullptr
    const double *src_flux;
    int src_begin, src_count;
    bool heat, keep_heat;           // keep_heat: add onto PHI_HEAT as it stands (f2py intent(inout)) instead of zeroing it
    double *dump;                   // N^3 grid receiving the column densities of the last source, or nullptr
};

// The sub-box semantics rate every source with the flux of the call's last one (f90:500,503): there is no meaningful spectrum
// per source, so the calls fail while the uploaded sources carry table sets of their own.
static int refuse_source_spectra(const char *who)
{
    if (!state().sources.spec) return 0;
    return fail(4, std::string(who) + ": the sub-box raytracer has one spectrum for all sources, and the sources on the device "
                                      "carry table sets of their own (source_spectra_to_device); use raytrace_device / evolve3D");
}

static int subbox_core(const SubboxCall &c, long long &total_nbox, double &total_loss)
{
    State &st = state();
    const int N = st.N;
    const size_t bytes = st.ncell * sizeof(double);
    const bool grey = st.opt[ASORA_OPT_GREY_NOTABLES] != 0;
    ASORA_HIP_TRY(hipMemsetAsync(st.grid[ASORA_GRID_PHI_ION], 0, 2 * bytes, st.stream));          // f90:95 (+ its [k][j][i] twin)
    if (c.heat) {
        if (!c.keep_heat) ASORA_HIP_TRY(hipMemsetAsync(st.grid[ASORA_GRID_PHI_HEAT], 0, bytes, st.stream));
        ASORA_HIP_TRY(hipMemsetAsync(st.heat_t, 0, bytes, st.stream));
    }
    if (c.dump) ASORA_HIP_TRY(hipMemsetAsync(c.dump, 0, bytes, st.stream));
    if (int rc = launch_prepare_nhi(st, true)) return rc;
    if (int rc = ensure_logtab(st)) return rc;

    // traversal range per axis side, f90:174-175
    int ext_r, ext_l;
    subbox_range(N, c.max_subbox, ext_r, ext_l);
    const int S_all = std::max(ext_r, ext_l);
    const bool range_open = ext_r > 0 && ext_l > 0;      // else the while loop of do_source never runs (f90:193-195)

    SubboxParams p;
    std::memset(&p, 0, sizeof p);
    p.N = N; p.W = std::max(S_all, 0) + 1;
    p.ext_r = ext_r; p.ext_l = ext_l;
    p.sig = c.sig; p.dr = c.dr; p.R = c.R;
    p.numtau_f = lut_index_limit(c.NumTau, c.table_len);                   // photorates.f90:141 real(NumTau)
    const LutIndex lut = lut_index_constants(c.minlogtau, c.dlogtau);
    p.lut_k1 = lut.k1; p.lut_k0 = lut.k0; p.lut_kc = lut.kc;
    p.table_len = c.table_len;
    p.grey = grey ? 1 : 0; p.heat = c.heat ? 1 : 0; p.add_zero = st.opt[ASORA_OPT_SKIP_ZERO_RATES] == 1 ? 0 : 1;
    const int last = c.src_begin + c.src_count - 1;
    p.flux_src = st.opt[ASORA_OPT_C2RAY_OWN_FLUX] ? -1 : last;            // f90:500,503
    p.dump_src = last;
    p.ncell = (unsigned)st.ncell;
    p.nhi = st.nhi; p.phi = st.grid[ASORA_GRID_PHI_ION]; p.heat_grid = st.grid[ASORA_GRID_PHI_HEAT];
    p.dump = c.dump;
    p.tables = c.tables; p.logtab = st.logtab_dev;
    p.src_pos = c.src_pos; p.src_flux = c.src_flux;
    p.unit_stride = (size_t)6 * p.W * p.W;

    total_nbox = 0;
    total_loss = 0.0;
    std::fill(st.sb_launch, st.sb_launch + ASORA_SUBBOX_LAUNCH_WORDS, 0);
    st.sb_launch[ASORA_SBL_VALID] = 1;
    // (pair lists are cached by the address of the source list: a caller's temporary list must not meet an older one's entries)
    struct DropPairs { State &s; bool on; ~DropPairs() { if (on) release_pair_lists(s); } } drop_pairs{st, c.src_pos != st.sources.pos};
    if (drop_pairs.on) release_pair_lists(st);
    // Round 3: the sources whose column densities do not go back to the caller are swept on the ASORA kernel's tabulated
    // geometry (cells within R_max_LLS only; raytrace.hip, SUBBOX) when that applies; the dumped source -- it needs the
    // whole cube -- and everything else stay with the on-the-fly kernel of subbox.hip
    RtParams tp;
    fill_rt_params(tp, c.R, c.sig, c.dr, c.minlogtau, c.dlogtau, c.NumTau, 1);
    tp.numtau_f = p.numtau_f; tp.lut_k1 = p.lut_k1; tp.lut_k0 = p.lut_k0; tp.lut_kc = p.lut_kc; tp.tau_zero = INFINITY;
    tp.table_len = c.table_len; tp.tables = c.tables;
    tp.fortran_consts = 1; tp.grey = grey ? 1 : 0; tp.z_transposed = 1;
    tp.logtab = st.logtab_dev;
    tp.src_pos = c.src_pos; tp.src_flux = c.src_flux;
    tp.src_spec = nullptr;                // (one spectrum: the entry points refuse sources with table sets of their own)
    tp.flux_src = p.flux_src;
    const bool has_dump = c.dump != nullptr;
    SubboxTables tab;
    const int table_sources = c.src_count - (has_dump ? 1 : 0);
    {
        if (range_open && table_sources > 0)
            if (int rc = subbox_tables_prepare(st, tp, ext_r, ext_l, c.subboxsize, table_sources, c.heat, tab, c.host_pos)) return rc;
    }

    // sources in batches bounded by the scratch: the on-the-fly kernel keeps 8 octants x 2 buffers x 3 W^2 doubles per source
    // (6.4 MB at 256^3), the tabulated sweep one trailing shell per source and unit (tab.max_batch)
    const size_t per_src = 8 * p.unit_stride * sizeof(double);
    const size_t budget = (size_t)4 << 30;
    // (one batch when the trailing shells of all tabulated sources fit: the dumped source then runs beside them)
    const int max_batch = tab.ok ? (tab.max_batch >= table_sources ? std::max(c.src_count, 1) : tab.max_batch)
                                 : (int)std::max<size_t>(8, std::min<size_t>((budget / per_src) / 8 * 8, 1 << 20));
    const int cap = std::min(std::max(c.src_count, 1), max_batch);
    // per-source bookkeeping of a batch, kept between calls
    if (int rc = st.subbox.active.reserve((size_t)cap)) return rc;
    if (int rc = st.subbox.nbox.reserve((size_t)cap)) return rc;
    if (int rc = st.subbox.loss.reserve((size_t)cap)) return rc;
    if (int rc = st.subbox.loss_final.reserve((size_t)cap)) return rc;
    if (int rc = st.subbox.nactive.allocate(1)) return rc;
    std::vector<int> h_nbox((size_t)cap);
    std::vector<double> h_loss((size_t)cap);

    for (int done = 0; done < c.src_count;) {
        const int batch = std::min(c.src_count - done, max_batch);
        // with the tables, the on-the-fly kernel only sweeps the dumped source (the last one of the call)
        const bool dump_here = has_dump && done + batch == c.src_count;
        const int fly_count = tab.ok ? (dump_here ? 1 : 0) : batch;
        const int fly_first = tab.ok ? batch - fly_count : 0;          // batch-local index of the first source swept on the fly
        const size_t need = (size_t)8 * ((std::max(fly_count, 1) + 7) / 8) * per_src;
        if (int rc = st.shell_scratch.reserve(need / sizeof(double))) return rc;
        const int first = c.src_begin + done;
        p.scratch = st.shell_scratch;
        p.src_begin = first + fly_first; p.src_count = fly_count;
        p.active = st.subbox.active + fly_first; p.loss = st.subbox.loss + fly_first;
        tp.src_begin = first; tp.src_count = batch - fly_count;
        tp.sb_active = st.subbox.active; tp.sb_loss = st.subbox.loss;
        int n_active = 0;
        if (int rc = launch_subbox_decide(st, 0, batch, c.src_flux, first, (double)c.loss_fraction, range_open ? 1 : 0,
                                          st.subbox.active, st.subbox.loss, st.subbox.loss_final, st.subbox.nbox, st.subbox.nactive)) return rc;
        ASORA_HIP_TRY(hipMemcpyAsync(&n_active, st.subbox.nactive, sizeof(int), hipMemcpyDeviceToHost, st.stream));
        ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
        long long box = 0;                                    // half-width of the current sub-box, f90:199-200
        while (n_active > 0) {
            const long long prev_box = box;
            box += c.subboxsize;
            p.s_begin = (int)std::min<long long>(prev_box, S_all);
            p.s_end = (int)std::min<long long>(box, S_all);
            p.edge_r = (int)std::min<long long>(box, ext_r);
            p.edge_l = (int)std::min<long long>(box, ext_l);
            // the dumped source's sweep (8 wide workgroups: as long as ONE workgroup lasts) runs beside the tabulated sweep of
            // all the others, on a side stream; both add into the same rate grids
            const bool beside = fly_count > 0 && tab.ok && tp.src_count > 0;
            if (beside) {
                ASORA_HIP_TRY(hipEventRecord(st.main_ready, st.stream));
                ASORA_HIP_TRY(hipStreamWaitEvent(st.side[0], st.main_ready, 0));
            }
            if (fly_count > 0) { if (int rc = launch_subbox_sweep(st, p, beside ? st.side[0] : nullptr)) return rc; }
            if (beside) ASORA_HIP_TRY(hipEventRecord(st.side_done[0], st.side[0]));
            if (tab.ok && tp.src_count > 0) {
                tp.sb_edge_r = p.edge_r; tp.sb_edge_l = p.edge_l;
                if (int rc = subbox_tables_sweep(st, tp, tab, p.s_begin, p.s_end, c.heat)) return rc;
            }
            if (beside) ASORA_HIP_TRY(hipStreamWaitEvent(st.stream, st.side_done[0], 0));
            const int more_range = (box < ext_r && box < ext_l) ? 1 : 0;          // f90:194-195
            if (int rc = launch_subbox_decide(st, 1, batch, c.src_flux, first, (double)c.loss_fraction, more_range,
                                              st.subbox.active, st.subbox.loss, st.subbox.loss_final, st.subbox.nbox, st.subbox.nactive)) return rc;
            ASORA_HIP_TRY(hipMemcpyAsync(&n_active, st.subbox.nactive, sizeof(int), hipMemcpyDeviceToHost, st.stream));
            ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
        }
        st.sb_launch[ASORA_SBL_BATCHES] += 1;
        ASORA_HIP_TRY(hipMemcpy(h_nbox.data(), st.subbox.nbox, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost));
        ASORA_HIP_TRY(hipMemcpy(h_loss.data(), st.subbox.loss_final, (size_t)batch * sizeof(double), hipMemcpyDeviceToHost));
        for (int s = 0; s < batch; ++s) { total_nbox += h_nbox[s]; total_loss += h_loss[s]; }   // f90:246-247, in source order
        done += batch;
    }

    // fold the [k][j][i] accumulators
    if (int rc = launch_finish_phi(st)) return rc;
    st.grid_valid[ASORA_GRID_PHI_ION] = true;
    if (c.heat) {
        if (int rc = launch_fold_transposed(st, st.heat_t, st.grid[ASORA_GRID_PHI_HEAT])) return rc;
        st.grid_valid[ASORA_GRID_PHI_HEAT] = true;
    }
    return 0;
}

} // namespace asora

using namespace asora;


extern "C" {

// ---------------------------------------------------------------------------------------------
// libc2ray.raytracing.do_all_sources: the host driver of subbox.hip (do_all_sources / do_source,
// src/c2ray/raytracing.f90:52-249)
// ---------------------------------------------------------------------------------------------
int c2ray_do_all_sources(const double *normflux, const int32_t *srcpos, int max_subbox, int subboxsize,
                         double *coldensh_out, double sig, double dr, const double *ndens, const double *xh_av,
                         double *phi_ion, double *phi_heat, float loss_fraction,
                         const double *photo_thin_table, const double *photo_thick_table,
                         const double *heat_thin_table, const double *heat_thick_table,
                         double minlogtau, double dlogtau, double R_max_LLS,
                         int NumTau, int NumSrc, int m1, int m2, int m3,
                         int *sum_nbox, double *photon_loss)
{
    clear_error();
    State &st = state();
    const char *who = "c2ray_do_all_sources";
    if (st.medium.plane.count > 0)
        return fail(4, std::string(who) + ": a plane-parallel flux (asora_plane_flux) has no sub-box sweep");
    if (st.opt[ASORA_OPT_OPEN_BOUNDARIES])
        return fail(4, std::string(who) + ": open boundaries (ASORA_OPT_OPEN_BOUNDARIES) have no sub-box sweep (the reference's Fortran has no such mode)");
    if (m1 != m2 || m1 != m3) return fail(3, std::string(who) + ": the mesh must be cubic (raytracing.f90:174-175 use m1 for every axis)");
    if (NumSrc < 0 || (NumSrc > 0 && (!normflux || !srcpos))) return fail(3, std::string(who) + ": bad source arguments");
    if (!ndens || !xh_av || !phi_ion || !coldensh_out) return fail(3, std::string(who) + ": null grid");
    if (subboxsize < 1) return fail(3, std::string(who) + ": subboxsize must be >= 1");
    const bool grey = st.opt[ASORA_OPT_GREY_NOTABLES] != 0;
    if (!grey && (NumTau < 1 || !photo_thin_table || !photo_thick_table))
        return fail(3, std::string(who) + ": empty photo-ionisation tables");
    if (int rc = refuse_source_spectra(who)) return rc;
    // Heating tables that are identically zero (what the reference's evolve3D passes, pyc2ray/evolve.py:193: "eventually
    // we'll add heating tables here") add exactly 0 to phi_heat: the grid is then neither uploaded, nor rated, nor
    // downloaded -- two 128 MiB transfers at 256^3 and the slower kernel variant for nothing.
    bool heat = !grey && phi_heat && heat_thin_table && heat_thick_table;
    if (heat) {
        bool any = false;
        for (int i = 0; i < NumTau && !any; ++i) any = heat_thin_table[i] != 0.0 || heat_thick_table[i] != 0.0;
        heat = any;
    }
    if (int rc = asora_device_init_auto(m1)) return rc;
    const int N = st.N;
    for (int s = 0; s < NumSrc; ++s)
        for (int ax = 0; ax < 3; ++ax)
            if (srcpos[3 * s + ax] < 1 || srcpos[3 * s + ax] > N)
                return fail(3, std::string(who) + ": source " + std::to_string(s + 1) + " lies outside the mesh (1-based " +
                                   std::to_string(srcpos[3 * s + ax]) + " on axis " + std::to_string(ax + 1) + ")");

    const size_t bytes = st.ncell * sizeof(double);
    // inputs: grids in Fortran order, sources 1-based
    if (int rc = asora_grid_to_device(ASORA_GRID_NDENS, ndens, N, 'F')) return rc;
    if (int rc = asora_grid_to_device(ASORA_GRID_XH_AV, xh_av, N, 'F')) return rc;
    if (heat) { if (int rc = asora_grid_to_device(ASORA_GRID_PHI_HEAT, phi_heat, N, 'F')) return rc; }

    Scoped<int32_t> d_pos; Scoped<double> d_flux; Scoped<double2> d_tables;     // (of this call: freed on every exit path)
    std::vector<int32_t> host_pos0;
    if (NumSrc > 0) {
        host_pos0.resize(3 * (size_t)NumSrc);
        std::vector<int32_t> &pos0 = host_pos0;
        for (size_t q = 0; q < pos0.size(); ++q) pos0[q] = srcpos[q] - 1;
        if (int rc = d_pos.allocate(pos0.size())) return rc;
        if (int rc = d_flux.allocate((size_t)NumSrc)) return rc;
        ASORA_HIP_TRY(hipMemcpy(d_pos, pos0.data(), pos0.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        ASORA_HIP_TRY(hipMemcpy(d_flux, normflux, (size_t)NumSrc * sizeof(double), hipMemcpyHostToDevice));
    }
    const int len = grey ? 1 : NumTau;
    {   // [thick | thin | heat thick | heat thin] as pairs {T[i], T[i+1]-T[i]} (see asora_photo_table_to_device)
        std::vector<double2> pairs(std::max<size_t>(4 * (size_t)len, 16), double2{0.0, 0.0});
        const double *src[4] = {photo_thick_table, photo_thin_table, heat ? heat_thick_table : nullptr,
                                heat ? heat_thin_table : nullptr};
        for (int t = 0; t < 4 && !grey; ++t)
            if (src[t]) pack_rate_table(pairs.data(), t, src[t], len);
        if (int rc = d_tables.allocate(pairs.size())) return rc;
        ASORA_HIP_TRY(hipMemcpy(d_tables, pairs.data(), pairs.size() * sizeof(double2), hipMemcpyHostToDevice));
    }

    SubboxCall c;
    c.max_subbox = max_subbox; c.subboxsize = subboxsize; c.loss_fraction = loss_fraction;
    c.sig = sig; c.dr = dr; c.R = R_max_LLS; c.minlogtau = minlogtau; c.dlogtau = dlogtau; c.NumTau = NumTau;
    c.table_len = len; c.tables = d_tables; c.src_pos = d_pos; c.src_flux = d_flux;
    c.host_pos = host_pos0.empty() ? nullptr : host_pos0.data();
    c.src_begin = 0; c.src_count = NumSrc;
    c.heat = heat; c.keep_heat = true;                  // phi_heat is intent(inout): added onto what was uploaded
    c.dump = st.staging;                                // column densities of the last source
    long long total_nbox = 0;
    double total_loss = 0.0;
    if (int rc = subbox_core(c, total_nbox, total_loss)) return rc;

    // the last source's column densities sit in the staging grid, which the 'F' download path below reuses:
    // take them out first, through nHI's transposed half (free once the sweep is over)
    if (int rc = launch_transpose(st, st.staging, st.nhi_t, N)) return rc;
    ASORA_HIP_TRY(hipMemcpyAsync(coldensh_out, st.nhi_t, bytes, hipMemcpyDeviceToHost, st.stream));
    if (int rc = asora_grid_to_host(ASORA_GRID_PHI_ION, phi_ion, N, 'F')) return rc;
    if (heat) { if (int rc = asora_grid_to_host(ASORA_GRID_PHI_HEAT, phi_heat, N, 'F')) return rc; }
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    if (sum_nbox) *sum_nbox = (int)total_nbox;
    if (photon_loss) *photon_loss = total_loss;
    return 0;
}

int asora_device_init_auto(int N)
{
    clear_error();
    State &st = state();
    if (!st.init || (st.auto_init && st.N != N)) {
        // stateless for the caller, like the f2py functions it serves: the library sets itself up for this mesh
        if (int rc = asora_device_init(N, 1)) return rc;
        st.auto_init = true;
        return 0;
    }
    return check_N("device_init_auto", N);
}

int asora_subbox_raytrace_device(int max_subbox, int subboxsize, float loss_fraction, double R_max_LLS, double sig, double dr,
                                 double minlogtau, double dlogtau, int NumTau, int src_begin, int src_count,
                                 int *sum_nbox, double *photon_loss)
{
    clear_error();
    if (int rc = require_init("subbox_raytrace_device")) return rc;
    State &st = state();
    const char *who = "subbox_raytrace_device";
    if (st.medium.plane.count > 0)
        return fail(4, std::string(who) + ": a plane-parallel flux (asora_plane_flux) has no sub-box sweep");
    if (st.opt[ASORA_OPT_OPEN_BOUNDARIES])
        return fail(4, std::string(who) + ": open boundaries (ASORA_OPT_OPEN_BOUNDARIES) have no sub-box sweep (the reference's Fortran has no such mode)");
    if (!st.grid_valid[ASORA_GRID_NDENS]) return fail(4, std::string(who) + ": density not on device");
    if (!st.grid_valid[ASORA_GRID_XH_AV]) return fail(4, std::string(who) + ": xh_av not on device");
    if (subboxsize < 1) return fail(3, std::string(who) + ": subboxsize must be >= 1");
    const bool grey = st.opt[ASORA_OPT_GREY_NOTABLES] != 0;
    if (!grey && (!st.sources.tables || NumTau < 1)) return fail(4, std::string(who) + ": radiation tables not on device");
    if (int rc = check_sources(who, 4, "source range outside the uploaded sources", src_begin, src_count)) return rc;
    if (int rc = refuse_source_spectra(who)) return rc;
    const bool heat = !grey && st.opt[ASORA_OPT_HEATING] != 0;
    if (heat && !st.sources.loaded.heat_tables) return fail(4, std::string(who) + ": heating requested but no heating tables on device");
    SubboxCall c;
    c.max_subbox = max_subbox; c.subboxsize = subboxsize; c.loss_fraction = loss_fraction;
    c.sig = sig; c.dr = dr; c.R = R_max_LLS; c.minlogtau = minlogtau; c.dlogtau = dlogtau; c.NumTau = NumTau;
    c.table_len = st.sources.loaded.table_len > 0 ? st.sources.loaded.table_len : 1; c.tables = st.sources.tables;
    c.src_pos = st.sources.pos; c.src_flux = st.sources.flux; c.src_begin = src_begin; c.src_count = src_count;
    c.host_pos = st.sources.loaded.pos_host.empty() ? nullptr : st.sources.loaded.pos_host.data();
    c.heat = heat; c.keep_heat = false; c.dump = nullptr;
    long long total_nbox = 0;
    double total_loss = 0.0;
    if (int rc = subbox_core(c, total_nbox, total_loss)) return rc;
    if (sum_nbox) *sum_nbox = (int)total_nbox;
    if (photon_loss) *photon_loss = total_loss;
    return 0;
}

int asora_debug_last_subbox_launch(int32_t *out)
{
    clear_error();
    if (!out) return fail(3, "debug_last_subbox_launch: null output");
    const State &st = state();
    for (int k = 0; k < ASORA_SUBBOX_LAUNCH_WORDS; ++k) out[k] = st.sb_launch[k];
    return 0;
}

int asora_debug_subbox_plan(int N, double R, int max_subbox, int src_count, int has_dump, int heat, int cu_count, int32_t *out)
{
    clear_error();
    if (N < 1 || src_count < 1 || !out) return fail(3, "debug_subbox_plan: bad arguments");
    const State &st = state();
    SubboxPlanInput in{};
    subbox_range(N, max_subbox, in.ext_r, in.ext_l);
    in.S_tab = subbox_table_extent(R, in.ext_r, in.ext_l);
    in.table_sources = src_count - (has_dump ? 1 : 0); in.has_dump = has_dump != 0; in.heat = heat != 0;
    // as subbox_core and subbox_tables_prepare read them (the sweep's grids always have their [k][j][i] twins)
    in.buffer_atomics = !st.opt[ASORA_OPT_GREY_NOTABLES] && !st.opt[ASORA_OPT_GLOBAL_ATOMICS] && 16ull * N * N * N <= 0x80000000ull;
    in.cu_count = cu_count > 0 ? cu_count : st.cu_count;
    in.opt_tables = st.opt[ASORA_OPT_SUBBOX_TABLES]; in.opt_pairs = st.opt[ASORA_OPT_PAIR_SOURCES]; in.opt_aligned = st.opt[ASORA_OPT_ALIGNED_ROWS];
    const SubboxPlan plan = plan_subbox(in);
    out[0] = plan.tables ? in.table_sources : 0;
    out[1] = plan.units; out[2] = plan.threads; out[3] = plan.tables ? plan.nsrc : 0; out[4] = plan.aligned ? 1 : 0;
    out[5] = plan.fly_sources; out[6] = plan.fly_threads; out[7] = in.S_tab;
    return 0;
}

} // extern "C"
