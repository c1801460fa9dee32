// grids_api.hip -- grids, rate tables and sources between the host and the device (asora_grid_*, asora_planes_to_*, the table and
// source uploads of src/asora/memory.cu).  An upload has left the host buffer when its call returns
// (a synchronise or a blocking copy: the buffer may be pageable).
#include "asora_internal.hpp"
#include "rates_device.hpp"


namespace asora {

// The grids that exist only once something needs them, allocated on first use:
//   PHI_HEAT  with its [k][j][i] twin (2 N^3 doubles: 2 GiB at 512^3): the heating tables are uploaded, or a caller hands the
//             grid over (evolve3D never does)
//   TEMP_END  thermal mode only (asora_thermal_params): the end-of-step temperature
//   CLUMP     clumping mode 2 only (asora_clumping): the per-cell factors, with their first upload
// Every other grid is a part of the arena.
int ensure_optional_grid(int which)
{
    State &st = state();
    if ((which != ASORA_GRID_PHI_HEAT && which != ASORA_GRID_TEMP_END && which != ASORA_GRID_CLUMP) || st.grid[which]) return 0;
    const bool twin = which == ASORA_GRID_PHI_HEAT;
    MeshBuffer<double> &own = twin ? st.phi_heat_grid : which == ASORA_GRID_TEMP_END ? st.temp_end_grid : st.clump_grid;
    if (int rc = own.allocate((twin ? 2 : 1) * st.ncell)) return rc;
    st.grid[which] = own;
    if (twin) st.heat_t = st.grid[which] + st.ncell;
    st.grid_valid[which] = false;
    return 0;
}

} // namespace asora

using namespace asora;

extern "C" {

int asora_grid_to_device(int which, const double *host, int N, char order)
{
    clear_error();
    if (int rc = require_init("grid_to_device")) return rc;
    if (int rc = check_N("grid_to_device", N)) return rc;
    if (which < 0 || which >= ASORA_GRID_COUNT) return fail(3, "grid_to_device: bad grid selector");
    if (!host) return fail(3, "grid_to_device: null host pointer");
    State &st = state();
    if (int rc = ensure_optional_grid(which)) return rc;
    st.zero.verdict.since_probe = std::max(st.zero.verdict.since_probe, 48);   // new medium: look again for cells beyond the table soon (decide_skip_zero: at 64)
    const size_t bytes = st.ncell * sizeof(double);
    if (order == 'C' || order == 'c') {
        ASORA_HIP_TRY(hipMemcpyAsync(st.grid[which], host, bytes, hipMemcpyHostToDevice, st.stream));
    } else if (order == 'F' || order == 'f') {
        ASORA_HIP_TRY(hipMemcpyAsync(st.staging, host, bytes, hipMemcpyHostToDevice, st.stream));
        if (int rc = launch_transpose(st, st.staging, st.grid[which], N)) return rc;
    } else
        return fail(3, "grid_to_device: order must be 'C' or 'F'");
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    st.grid_valid[which] = true;
    if (which == ASORA_GRID_TEMP) st.temp_probe.valid = false;
    return 0;
}

int asora_grid_to_host(int which, double *host, int N, char order)
{
    clear_error();
    if (int rc = require_init("grid_to_host")) return rc;
    if (int rc = check_N("grid_to_host", N)) return rc;
    if (which < 0 || which >= ASORA_GRID_COUNT) return fail(3, "grid_to_host: bad grid selector");
    if (!host) return fail(3, "grid_to_host: null host pointer");
    State &st = state();
    if (!st.grid[which] || !st.grid_valid[which]) return fail(3, "grid_to_host: grid " + std::to_string(which) + " holds no data");
    const size_t bytes = st.ncell * sizeof(double);
    if (order == 'C' || order == 'c') {
        ASORA_HIP_TRY(hipMemcpyAsync(host, st.grid[which], bytes, hipMemcpyDeviceToHost, st.stream));
    } else if (order == 'F' || order == 'f') {
        if (int rc = launch_transpose(st, st.grid[which], st.staging, N)) return rc;
        ASORA_HIP_TRY(hipMemcpyAsync(host, st.staging, bytes, hipMemcpyDeviceToHost, st.stream));
    } else
        return fail(3, "grid_to_host: order must be 'C' or 'F'");
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    return 0;
}

int asora_grid_copy(int dst, int src)
{
    clear_error();
    if (int rc = require_init("grid_copy")) return rc;
    if (dst < 0 || dst >= ASORA_GRID_COUNT || src < 0 || src >= ASORA_GRID_COUNT || dst == src)
        return fail(3, "grid_copy: bad grid selectors");
    State &st = state();
    if (!st.grid_valid[src]) return fail(3, "grid_copy: source grid holds no data");
    if (int rc = ensure_optional_grid(dst)) return rc;
    ASORA_HIP_TRY(hipMemcpyAsync(st.grid[dst], st.grid[src], st.ncell * sizeof(double), hipMemcpyDeviceToDevice,
                                 st.stream));
    st.grid_valid[dst] = true;
    if (dst == ASORA_GRID_TEMP) st.temp_probe.valid = false;
    return 0;
}

int asora_grid_scale(int which, double factor)
{
    clear_error();
    if (int rc = require_init("grid_scale")) return rc;
    if (which < 0 || which >= ASORA_GRID_COUNT) return fail(3, "grid_scale: bad grid selector");
    State &st = state();
    if (!st.grid_valid[which]) return fail(3, "grid_scale: grid " + std::to_string(which) + " holds no data");
    if (int rc = launch_scale(st, st.grid[which], st.ncell, factor)) return rc;
    if (which == ASORA_GRID_TEMP) st.temp_probe.valid = false;
    return 0;
}

int asora_grid_sum(int which, double *sum)
{
    clear_error();
    if (int rc = require_init("grid_sum")) return rc;
    if (which < 0 || which >= ASORA_GRID_COUNT) return fail(3, "grid_sum: bad grid selector");
    if (!sum) return fail(3, "grid_sum: null output pointer");
    State &st = state();
    if (!st.grid_valid[which]) return fail(3, "grid_sum: grid " + std::to_string(which) + " holds no data");
    if (int rc = st.temp_probe.dev.allocate(8)) return rc;
    if (int rc = launch_grid_sum(st, st.grid[which], st.ncell, st.temp_probe.dev + 5)) return rc;
    ASORA_HIP_TRY(hipMemcpyAsync(sum, st.temp_probe.dev + 5, sizeof(double), hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    return 0;
}

int asora_host_alloc(size_t bytes, void **host)
{
    clear_error();
    if (!host || bytes == 0) return fail(3, "host_alloc: null pointer or zero size");
    *host = nullptr;
    ASORA_HIP_TRY(hipHostMalloc(host, bytes, hipHostMallocDefault));
    return 0;
}

int asora_host_free(void *host)
{
    clear_error();
    if (!host) return 0;
    ASORA_HIP_TRY(hipHostFree(host));
    return 0;
}

void *asora_device_ptr(int which)
{
    if (!state().init || which < 0 || which >= ASORA_GRID_COUNT) return nullptr;
    return state().grid[which];
}

int asora_density_to_device(const double *ndens, int N)
{
    return asora_grid_to_device(ASORA_GRID_NDENS, ndens, N, 'C');
}

// One set's block on the device: rates_device.hpp (one 16-byte load serves the linear interpolation of photo_lookuptable,
// rates.cu:82), [thick | thin | heat thick | heat thin]; at least 16 entries: the kernels' pipeline-priming loads read a few fixed
// small offsets whatever the table's length.  Several sets (asora_spectra_to_device) are consecutive blocks.
static size_t rate_block_entries(int NumTau) { return std::max<size_t>(4 * (size_t)NumTau, 16); }

// heat_*: both null = no heating tables.  Arrays [NumSpec][NumTau].
static int upload_rate_tables(const char *who, int NumSpec, int NumTau, const double *thin, const double *thick, const double *heat_thin,
                              const double *heat_thick)
{
    State &st = state();
    const bool heat = heat_thin && heat_thick;
    if (heat) { if (int rc = ensure_optional_grid(ASORA_GRID_PHI_HEAT)) return rc; }
    st.zero.verdict.since_probe = std::max(st.zero.verdict.since_probe, 48);
    (void)st.sources.tables.release();
    st.sources.loaded.table_len = 0; st.sources.loaded.num_spec = 1; st.sources.loaded.spec_stride = 0; st.sources.loaded.heat_tables = false;
    const size_t block = rate_block_entries(NumTau);
    std::vector<double2> pairs(block * (size_t)NumSpec, double2{0.0, 0.0});
    for (int k = 0; k < NumSpec; ++k) {
        double2 *b = pairs.data() + block * (size_t)k;
        pack_rate_table(b, 0, thick + (size_t)k * NumTau, NumTau);
        pack_rate_table(b, 1, thin + (size_t)k * NumTau, NumTau);
        if (heat) {
            pack_rate_table(b, 2, heat_thick + (size_t)k * NumTau, NumTau);
            pack_rate_table(b, 3, heat_thin + (size_t)k * NumTau, NumTau);
        }
    }
    (void)who;
    if (int rc = st.sources.tables.allocate(pairs.size())) return rc;
    ASORA_HIP_TRY(hipMemcpy(st.sources.tables, pairs.data(), pairs.size() * sizeof(double2), hipMemcpyHostToDevice));
    st.sources.loaded.table_len = NumTau;
    st.sources.loaded.num_spec = NumSpec;
    st.sources.loaded.spec_stride = block;
    st.sources.loaded.heat_tables = heat;
    return 0;
}

int asora_photo_table_to_device(const double *thin_table, const double *thick_table, int NumTau)
{
    clear_error();
    if (int rc = require_init("photo_table_to_device")) return rc;
    if (NumTau < 1 || !thin_table || !thick_table) return fail(3, "photo_table_to_device: empty table");
    return upload_rate_tables("photo_table_to_device", 1, NumTau, thin_table, thick_table, nullptr, nullptr);
}

int asora_heat_table_to_device(const double *heat_thin_table, const double *heat_thick_table, int NumTau)
{
    clear_error();
    if (int rc = require_init("heat_table_to_device")) return rc;
    State &st = state();
    if (!st.sources.tables) return fail(4, "heat_table_to_device: upload the photo tables first (photo_table_to_device)");
    if (st.sources.loaded.num_spec != 1)
        return fail(4, "heat_table_to_device: " + std::to_string(st.sources.loaded.num_spec) + " table sets are on the device; their heating tables go "
                       "up with them (spectra_to_device)");
    if (NumTau != st.sources.loaded.table_len || !heat_thin_table || !heat_thick_table)
        return fail(3, "heat_table_to_device: the heating tables must have the length of the photo tables (" +
                           std::to_string(st.sources.loaded.table_len) + ")");
    if (int rc = ensure_optional_grid(ASORA_GRID_PHI_HEAT)) return rc;
    std::vector<double2> pairs(4 * (size_t)NumTau, double2{0.0, 0.0});
    pack_rate_table(pairs.data(), 2, heat_thick_table, NumTau);
    pack_rate_table(pairs.data(), 3, heat_thin_table, NumTau);
    const size_t lo = rate_table_byte_offset(2, NumTau), hi = rate_table_byte_offset(4, NumTau);
    ASORA_HIP_TRY(hipMemcpy(reinterpret_cast<char *>(st.sources.tables.get()) + lo, reinterpret_cast<const char *>(pairs.data()) + lo, hi - lo,
                            hipMemcpyHostToDevice));
    st.sources.loaded.heat_tables = true;
    return 0;
}

int asora_spectra_to_device(int NumSpec, int NumTau, const double *photo_thin, const double *photo_thick, const double *heat_thin,
                            const double *heat_thick)
{
    clear_error();
    if (int rc = require_init("spectra_to_device")) return rc;
    if (NumSpec < 1 || NumSpec > ASORA_MAX_SPECTRA)
        return fail(3, "spectra_to_device: NumSpec=" + std::to_string(NumSpec) + " outside [1, " + std::to_string(ASORA_MAX_SPECTRA) + "]");
    if (NumTau < 1 || !photo_thin || !photo_thick) return fail(3, "spectra_to_device: empty table");
    if ((heat_thin == nullptr) != (heat_thick == nullptr)) return fail(3, "spectra_to_device: one heating table without the other");
    return upload_rate_tables("spectra_to_device", NumSpec, NumTau, photo_thin, photo_thick, heat_thin, heat_thick);
}

int asora_num_spectra(void) { return state().sources.tables ? state().sources.loaded.num_spec : 0; }

} // extern "C"

namespace asora {

void sort_sources_by_position(const int32_t *pos, int NumSrc, std::vector<int> &order)
{
    order.resize((size_t)std::max(NumSrc, 0));
    for (int s = 0; s < NumSrc; ++s) order[s] = s;
    std::stable_sort(order.begin(), order.end(), [pos](int a, int b) {
        if (pos[3 * a] != pos[3 * b]) return pos[3 * a] < pos[3 * b];
        if (pos[3 * a + 1] != pos[3 * b + 1]) return pos[3 * a + 1] < pos[3 * b + 1];
        return pos[3 * a + 2] < pos[3 * b + 2];
    });
}

static void drop_source_spectra(State &st)
{
    (void)st.sources.spec.release(); (void)st.sources.spec_sorted.release();
    st.sources.loaded.spec_max = 0;
}

int check_source_spectra(const char *who)
{
    State &st = state();
    if (!st.sources.spec) return 0;
    if (st.opt[ASORA_OPT_GREY_NOTABLES])
        return fail(4, std::string(who) + ": grey opacity uses no tables, so sources cannot have table sets of their own "
                                          "(source_spectra_to_device with zeros, or ASORA_OPT_GREY_NOTABLES = 0)");
    if (st.sources.loaded.spec_max >= st.sources.loaded.num_spec)
        return fail(4, std::string(who) + ": a source has table set " + std::to_string(st.sources.loaded.spec_max) + " but the device holds " +
                           std::to_string(st.sources.loaded.num_spec) + " (spectra_to_device)");
    return 0;
}

} // namespace asora

extern "C" {

int asora_source_data_to_device(const int32_t *pos, const double *flux, int NumSrc)
{
    clear_error();
    if (int rc = require_init("source_data_to_device")) return rc;
    if (NumSrc < 0 || (NumSrc > 0 && (!pos || !flux))) return fail(3, "source_data_to_device: bad arguments");
    State &st = state();
    st.zero.verdict.since_probe = std::max(st.zero.verdict.since_probe, 48);
    // validate on the host before anything reaches a kernel: positions index the grid directly
    for (int s = 0; s < NumSrc; ++s)
        for (int ax = 0; ax < 3; ++ax)
            if (pos[3 * s + ax] < 0 || pos[3 * s + ax] >= st.N)
                return fail(3, "source_data_to_device: source " + std::to_string(s) + " lies outside the mesh (0-based " +
                                   std::to_string(pos[3 * s + ax]) + " on axis " + std::to_string(ax) + ")");
    (void)st.sources.pos.release(); (void)st.sources.flux.release();          // memory.cu:102-103
    (void)st.sources.pos_sorted.release(); (void)st.sources.flux_sorted.release();
    drop_source_spectra(st);              // every source back to table set 0
    st.sources.loaded.i0_sorted.clear();
    st.sources.loaded.pos_host.clear(); st.sources.loaded.pos_sorted_host.clear();
    release_pair_lists(st);
    st.sources.loaded.num = 0;
    if (NumSrc == 0) return 0;
    if (int rc = st.sources.pos.allocate(3 * (size_t)NumSrc)) return rc;
    if (int rc = st.sources.flux.allocate((size_t)NumSrc)) return rc;
    ASORA_HIP_TRY(hipMemcpy(st.sources.pos, pos, sizeof(int32_t) * 3 * (size_t)NumSrc, hipMemcpyHostToDevice));
    ASORA_HIP_TRY(hipMemcpy(st.sources.flux, flux, sizeof(double) * (size_t)NumSrc, hipMemcpyHostToDevice));
    {   // a second copy in lexicographic order of the position (the sum over sources does not depend on their order): what
        // a call that traces the WHOLE list works from -- sources that run side by side are then neighbours in space and
        // share nHI and rate lines (measured -2 % on the trace at r_RT = 16 and 32) -- and, ordered by the first
        // coordinate, what the pipelined asora_do_all_sources cuts into slabs
        std::vector<int> order;
        sort_sources_by_position(pos, NumSrc, order);
        std::vector<int32_t> ps(3 * (size_t)NumSrc);
        std::vector<double> fs((size_t)NumSrc);
        st.sources.loaded.i0_sorted.resize((size_t)NumSrc);
        for (int s = 0; s < NumSrc; ++s) {
            const int o = order[s];
            ps[3 * s] = pos[3 * o]; ps[3 * s + 1] = pos[3 * o + 1]; ps[3 * s + 2] = pos[3 * o + 2];
            fs[s] = flux[o];
            st.sources.loaded.i0_sorted[s] = pos[3 * o];
        }
        if (int rc = st.sources.pos_sorted.allocate(3 * (size_t)NumSrc)) return rc;
        if (int rc = st.sources.flux_sorted.allocate((size_t)NumSrc)) return rc;
        ASORA_HIP_TRY(hipMemcpy(st.sources.pos_sorted, ps.data(), sizeof(int32_t) * 3 * (size_t)NumSrc, hipMemcpyHostToDevice));
        ASORA_HIP_TRY(hipMemcpy(st.sources.flux_sorted, fs.data(), sizeof(double) * (size_t)NumSrc, hipMemcpyHostToDevice));
        st.sources.loaded.pos_sorted_host.swap(ps);
    }
    st.sources.loaded.pos_host.assign(pos, pos + 3 * (size_t)NumSrc);
    st.sources.loaded.num = NumSrc;
    st.src_generation += 1;
    return 0;
}

int asora_source_spectra_to_device(const int32_t *spec, int NumSrc)
{
    clear_error();
    if (int rc = require_init("source_spectra_to_device")) return rc;
    State &st = state();
    if (NumSrc != st.sources.loaded.num)
        return fail(3, "source_spectra_to_device: " + std::to_string(NumSrc) + " table sets for the " + std::to_string(st.sources.loaded.num) +
                           " sources on the device (source_data_to_device first)");
    drop_source_spectra(st);
    if (!spec || NumSrc == 0) return 0;
    // validated on the host: the index becomes an offset on the table pointer.  Against the sets on the device now, if any; a
    // table upload that follows is met by check_source_spectra before the first trace
    const int limit = st.sources.tables ? st.sources.loaded.num_spec : ASORA_MAX_SPECTRA;
    int top = 0;
    for (int s = 0; s < NumSrc; ++s) {
        if (spec[s] < 0 || spec[s] >= limit)
            return fail(3, "source_spectra_to_device: source " + std::to_string(s) + " has table set " + std::to_string(spec[s]) +
                               ", outside [0, " + std::to_string(limit) + ")");
        top = std::max(top, (int)spec[s]);
    }
    if (top == 0) return 0;               // all set 0: the launches carry no array at all
    std::vector<int> order;
    sort_sources_by_position(st.sources.loaded.pos_host.data(), NumSrc, order);
    std::vector<int32_t> sorted((size_t)NumSrc);
    for (int s = 0; s < NumSrc; ++s) sorted[s] = spec[order[s]];
    if (int rc = st.sources.spec.allocate((size_t)NumSrc)) return rc;
    if (int rc = st.sources.spec_sorted.allocate((size_t)NumSrc)) return rc;
    ASORA_HIP_TRY(hipMemcpy(st.sources.spec, spec, sizeof(int32_t) * (size_t)NumSrc, hipMemcpyHostToDevice));
    ASORA_HIP_TRY(hipMemcpy(st.sources.spec_sorted, sorted.data(), sizeof(int32_t) * (size_t)NumSrc, hipMemcpyHostToDevice));
    st.sources.loaded.spec_max = top;
    return 0;
}

int asora_debug_sort_sources(const int32_t *pos, const double *flux, const int32_t *spec, int NumSrc, int32_t *pos_out,
                             double *flux_out, int32_t *spec_out)
{
    clear_error();
    if (NumSrc < 0 || (NumSrc > 0 && (!pos || !flux || !pos_out || !flux_out))) return fail(3, "debug_sort_sources: bad arguments");
    std::vector<int> order;
    sort_sources_by_position(pos, NumSrc, order);
    for (int s = 0; s < NumSrc; ++s) {
        const int o = order[s];
        for (int ax = 0; ax < 3; ++ax) pos_out[3 * s + ax] = pos[3 * o + ax];
        flux_out[s] = flux[o];
        if (spec && spec_out) spec_out[s] = spec[o];
    }
    return 0;
}

// Contiguous runs of i-planes of a grid to / from the host (C order: plane i is N*N consecutive doubles).  What a
// multi-GPU rank exchanges are such runs (the planes its sources reach, the planes whose chemistry it owns).
int asora_planes_to_host(int which, int i_begin, int i_count, double *host)
{
    clear_error();
    if (int rc = require_init("planes_to_host")) return rc;
    State &st = state();
    if (which < 0 || which >= ASORA_GRID_COUNT) return fail(3, "planes_to_host: bad grid selector");
    if (int rc = check_planes("planes_to_host", 3, "bad plane range", i_begin, i_count)) return rc;
    if (i_count == 0) return 0;
    if (!host) return fail(3, "planes_to_host: null host pointer");
    if (!st.grid_valid[which]) return fail(3, "planes_to_host: grid " + std::to_string(which) + " holds no data");
    const size_t plane = (size_t)st.N * st.N;
    ASORA_HIP_TRY(hipMemcpyAsync(host, st.grid[which] + (size_t)i_begin * plane, (size_t)i_count * plane * sizeof(double),
                                 hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    return 0;
}

int asora_planes_to_device(int which, int i_begin, int i_count, const double *host)
{
    clear_error();
    if (int rc = require_init("planes_to_device")) return rc;
    State &st = state();
    if (which < 0 || which >= ASORA_GRID_COUNT) return fail(3, "planes_to_device: bad grid selector");
    if (int rc = check_planes("planes_to_device", 3, "bad plane range", i_begin, i_count)) return rc;
    if (i_count == 0) return 0;
    if (!host) return fail(3, "planes_to_device: null host pointer");
    if (int rc = ensure_optional_grid(which)) return rc;
    const size_t plane = (size_t)st.N * st.N;
    ASORA_HIP_TRY(hipMemcpyAsync(st.grid[which] + (size_t)i_begin * plane, host, (size_t)i_count * plane * sizeof(double),
                                 hipMemcpyHostToDevice, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    st.grid_valid[which] = true;             // (the caller vouches for the planes it did not write)
    if (which == ASORA_GRID_TEMP) st.temp_probe.valid = false;
    return 0;
}

} // extern "C"
