// raytrace_api.hip -- the whole-box raytrace of the uploaded sources: the three-part call (asora_raytrace_begin / _range / _fold),
// the reference's asora_do_all_sources with its PCIe copies pipelined behind the trace, the work counters of the last trace.
#include "asora_internal.hpp"

namespace asora {

int reset_counters()
{
    State &st = state();
    ASORA_HIP_TRY(hipMemsetAsync(st.counters, 0, sizeof(unsigned long long) * COUNTER_FIELDS * COUNTER_SLOTS, st.stream));
    return 0;
}

// What a trace of the uploaded sources needs on the device, for every entry point that starts one.  density / xh_av: the
// call reads these grids as they stand (the device loop checks its own grids, the drop-in call uploads xh_av itself).
int require_raytrace_inputs(const char *who, double R, int NumTau, bool density, bool xh_av)
{
    State &st = state();
    const std::string w = std::string(who) + ": ";
    // (a matter of the library's settings alone: said before anything about the data)
    if (int rc = check_open_boundaries(st, who, st.opt[ASORA_OPT_OPEN_BOUNDARIES] != 0, false)) return rc;
    if (density && !st.grid_valid[ASORA_GRID_NDENS]) return fail(4, w + "density not on device (density_to_device)");
    if (xh_av && !st.grid_valid[ASORA_GRID_XH_AV]) return fail(4, w + "xh_av not on device");
    if (!st.opt[ASORA_OPT_GREY_NOTABLES] && !st.sources.tables) return fail(4, w + "radiation tables not on device (photo_table_to_device)");
    if (!(R >= 0.0)) return fail(4, w + "R must be >= 0");
    if (NumTau < 1 && !st.opt[ASORA_OPT_GREY_NOTABLES]) return fail(4, w + "NumTau must be >= 1");
    return check_source_spectra(who);
}

static int check_rt_sources(int src_begin, int src_count)
{
    return check_sources("raytrace", 4, "source range [" + std::to_string(src_begin) + "," + std::to_string(src_begin + src_count) +
                         ") outside the " + std::to_string(state().sources.loaded.num) + " uploaded sources (source_data_to_device)", src_begin, src_count);
}

// The parameter block of a raytrace of the uploaded sources into PHI_ION (+ its [k][j][i] twin).  radius_path: which radius
// history the call belongs to (note_call_radius; exactly one call of it per API call: here) -- 0 the whole-box entry points,
// 1 the sub-box sweep
void fill_rt_params(RtParams &p, double R, double sig, double dr, double minlogtau, double dlogtau, int NumTau, int radius_path)
{
    State &st = state();
    std::memset(&p, 0, sizeof p);
    p.N = st.N;
    p.R = R; p.sig = sig; p.dr = dr;
    p.minlogtau = minlogtau; p.dlogtau = dlogtau;
    p.table_len = st.sources.loaded.table_len > 0 ? st.sources.loaded.table_len : 1;
    p.NumTau = NumTau; p.numtau_f = lut_index_limit(NumTau, p.table_len);
    p.fortran_consts = st.opt[ASORA_OPT_FORTRAN_CONSTANTS];
    p.grey = st.opt[ASORA_OPT_GREY_NOTABLES];
    p.z_transposed = st.opt[ASORA_OPT_Z_TRANSPOSED] != 0 ? 1 : 0;
    p.ncell = (unsigned)st.ncell;
    p.nhi = st.nhi;
    p.phi = st.grid[ASORA_GRID_PHI_ION];
    p.tables = st.sources.tables;
    p.heat = st.grid[ASORA_GRID_PHI_HEAT];
    // (per-source spectra: the two fields every entry point built on this block inherits)
    p.spec_stride = (unsigned)st.sources.loaded.spec_stride;
    use_source_list(p, st, false);
    p.counters = st.counters;
    p.radius_stays = note_call_radius(st, R, radius_path) ? 1 : 0;
    p.open_bc = st.opt[ASORA_OPT_OPEN_BOUNDARIES] != 0 ? 1 : 0;
    p.plane = st.medium.plane;
}

// A raytrace call in three parts, so that a caller can overlap the multi-GPU sum of finished slabs of the
// rate grid with the tracing of later sources (asora_raytrace_begin / _range / _fold):
//   rt_begin  checks, zeroes the accumulators (raytracing.cu:113), forms nHI, fixes the parameters;
//   rt_range  traces a range of the uploaded sources into the accumulators (asynchronous);
//   rt_fold   adds the [k][j][i] accumulator of the z-faces into phi_ion for a slab of i-planes.
static int rt_begin(double R, double sig, double dr, double minlogtau, double dlogtau, int NumTau, double *dump,
                    bool pipelined = false)
{
    State &st = state();
    st.rt.open = false;
    if (int rc = require_raytrace_inputs("raytrace", R, NumTau, true, true)) return rc;

    const bool zt = st.opt[ASORA_OPT_Z_TRANSPOSED] != 0;
    const bool heat = st.opt[ASORA_OPT_HEATING] != 0 && dump == nullptr;
    if (heat && (!st.sources.loaded.heat_tables || st.opt[ASORA_OPT_GREY_NOTABLES]))
        return fail(4, "raytrace: heating requested but no heating tables on device (heat_table_to_device)");
    if (int rc = check_plane_flux(st, st.medium.plane, "raytrace", dump != nullptr, heat)) return rc;
    const size_t bytes = st.ncell * sizeof(double);
    ASORA_HIP_TRY(hipMemsetAsync(st.grid[ASORA_GRID_PHI_ION], 0, bytes, st.stream));      // raytracing.cu:113
    if (zt) ASORA_HIP_TRY(hipMemsetAsync(st.phi_t, 0, bytes, st.stream));
    if (heat) {
        ASORA_HIP_TRY(hipMemsetAsync(st.grid[ASORA_GRID_PHI_HEAT], 0, bytes, st.stream));
        if (zt) ASORA_HIP_TRY(hipMemsetAsync(st.heat_t, 0, bytes, st.stream));
    }
    if (int rc = reset_counters()) return rc;
    if (int rc = launch_prepare_nhi(st, zt)) return rc;

    RtParams &p = st.rt_params;
    fill_rt_params(p, R, sig, dr, minlogtau, dlogtau, NumTau);
    p.dump = dump;
    // the faces' sweeps (asora_plane_flux): behind the zeroed accumulators and nHI, ahead of every point-source launch (and of
    // main_ready below, so the side streams of the pipelined form start behind them)
    if (int rc = launch_plane_flux(st, p, st.grid[ASORA_GRID_PHI_ION], st.grid[ASORA_GRID_PHI_HEAT], heat, nullptr)) return rc;
    st.rt_heat = heat;
    st.rt_pipelined = pipelined;
    st.rt_by_planes = false;
    if (pipelined) {       // the side streams start behind the zeroed accumulators and nHI
        ASORA_HIP_TRY(hipEventRecord(st.main_ready, st.stream));
        for (int q = 0; q < 2; ++q) {
            ASORA_HIP_TRY(hipStreamWaitEvent(st.side[q], st.main_ready, 0));
            st.side_pending[q] = false;
        }
        st.side_next = 0;
    }
    st.rt.open = true;
    return 0;
}

static int rt_range(int src_begin, int src_count)
{
    State &st = state();
    if (!st.rt.open) return fail(4, "raytrace_range: no raytrace in progress (call asora_raytrace_begin)");
    if (int rc = check_rt_sources(src_begin, src_count)) return rc;
    if (src_count == 0) return 0;
    RtParams p = st.rt_params;
    // the whole list: in the spatially ordered copy (a column-density dump is of the caller's LAST source: caller's order)
    use_source_list(p, st, src_begin == 0 && src_count == st.sources.loaded.num && st.sources.pos_sorted && !p.dump);
    p.src_begin = src_begin; p.src_count = src_count;
    // one launch shape (one set of geometry tables) per call: a call that traces its sources in several ranges (pipelined
    // all-reduce, chunked slab exchange) is sized by all of the rank's sources
    p.shape_src_count = (st.rt_pipelined || st.rt_by_planes) ? st.sources.loaded.num : src_count;
    if (!st.rt_pipelined) return launch_raytrace(st, p, p.dump != nullptr, st.rt_heat);
    const int q = st.side_next;
    st.side_next ^= 1;
    if (int rc = launch_raytrace(st, p, p.dump != nullptr, st.rt_heat, st.side[q])) return rc;
    ASORA_HIP_TRY(hipEventRecord(st.side_done[q], st.side[q]));
    st.side_pending[q] = true;
    return 0;
}

static int rt_fold(int i_begin, int i_count)
{
    State &st = state();
    if (!st.rt.open) return fail(4, "raytrace_fold: no raytrace in progress (call asora_raytrace_begin)");
    if (int rc = check_planes("raytrace_fold", 4, "bad plane range", i_begin, i_count)) return rc;
    for (int q = 0; q < 2; ++q)       // everything traced so far must have landed
        if (st.side_pending[q]) {
            ASORA_HIP_TRY(hipStreamWaitEvent(st.stream, st.side_done[q], 0));
            st.side_pending[q] = false;
        }
    if (st.rt_params.z_transposed && i_count > 0) {
        if (int rc = launch_fold_range(st, st.phi_t, st.grid[ASORA_GRID_PHI_ION], i_begin, i_count)) return rc;
        if (st.rt_heat)
            if (int rc = launch_fold_range(st, st.heat_t, st.grid[ASORA_GRID_PHI_HEAT], i_begin, i_count)) return rc;
    }
    st.grid_valid[ASORA_GRID_PHI_ION] = true;
    if (st.rt_heat) st.grid_valid[ASORA_GRID_PHI_HEAT] = true;
    return 0;
}

static int do_raytrace(double R, double sig, double dr, int src_begin, int src_count, double minlogtau,
                       double dlogtau, int NumTau, double *dump)
{
    State &st = state();
    if (int rc = check_rt_sources(src_begin, src_count)) return rc;
    if (int rc = rt_begin(R, sig, dr, minlogtau, dlogtau, NumTau, dump)) return rc;
    if (int rc = rt_range(src_begin, src_count)) return rc;
    if (int rc = rt_fold(0, st.N)) return rc;
    st.rt.open = false;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// The drop-in asora_do_all_sources with its two PCIe copies hidden behind the trace
// ---------------------------------------------------------------------------------------------
// The reference's call uploads xh_av (N^3 doubles), traces, downloads phi_ion (raytracing.cu:117-146): at 256^3 the two
// copies take 2 x 2.4 ms at the link's ~56 GB/s against 1.4 ms of tracing 1000 sources.  A source at plane i0 only needs
// nHI on, and only rates, the planes within R of it.  So the grid is cut into K slabs of planes; the slabs of xh_av are
// uploaded one after the other on a copy stream, nHI of a slab is formed as soon as it has arrived, the sources of a
// slab (a second copy of the source list, ordered by first coordinate) are traced as soon as the slabs they reach are
// there, and a slab of phi_ion is folded and sent to the host on a second copy stream as soon as the last source that
// reaches it has been traced -- upload, trace and download overlap (PCIe is full duplex).  The host buffers are
// registered (pinned) for the duration of the call so that the copies are asynchronous; re-registering a buffer the
// driver has seen before costs microseconds (tools/micro/pcie.hip).  done = false: conditions not met, nothing was
// started, the caller takes the plain path.
static int do_all_sources_pipelined(double R, double sig, double dr, const double *xh_av, double *phi_ion, int NumSrc,
                                    double minlogtau, double dlogtau, int NumTau, bool &done)
{
    State &st = state();
    done = false;
    const int N = st.N;
    constexpr int KMAX = 16;
    const char *kenv = getenv("ASORA_PIPELINE_SLABS");
    const int K = kenv ? std::max(2, std::min(KMAX, atoi(kenv))) : 8;
    if (!st.opt[ASORA_OPT_PIPELINED_COPIES] || !st.opt[ASORA_OPT_Z_TRANSPOSED] || st.opt[ASORA_OPT_HEATING]) return 0;
    if (st.medium.plane.count > 0) return 0;                       // a face's sweep needs nHI of the whole box before anything is traced
    if (NumSrc != st.sources.loaded.num || NumSrc < 1 || !st.sources.pos_sorted || N < 8 * K) return 0;
    if (!std::isfinite(R) || !(R >= 0.0)) return 0;
    const int m = (int)std::floor(R);                       // a source rates the planes i0 - floor(R) ... i0 + floor(R)
    if (2 * m + N / K >= N) return 0;                       // every slab of sources reaches (nearly) every plane
    if (int rc = require_raytrace_inputs("raytrace", R, NumTau, true, false)) return rc;     // (xh_av: uploaded below)

    const size_t bytes = st.ncell * sizeof(double);
    if (hipHostRegister((void *)xh_av, bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return 0; }
    if (hipHostRegister((void *)phi_ion, bytes, hipHostRegisterDefault) != hipSuccess) {
        (void)hipGetLastError(); (void)hipHostUnregister((void *)xh_av); return 0;
    }
    // on EVERY exit path -- also the error returns below, with copies into and out of the caller's buffers possibly still in
    // flight -- the three streams are drained before the buffers are unregistered and handed back
    struct Unpin {
        const void *a, *b;
        ~Unpin()
        {
            State &s = state();
            for (hipStream_t q : {s.side[0], s.side[1], s.stream}) if (q) (void)hipStreamSynchronize(q);
            (void)hipHostUnregister((void *)a); (void)hipHostUnregister((void *)b);
        }
    } unpin{xh_av, phi_ion};

    while ((int)st.pipe_events.size() < 2 * K) {
        hipEvent_t e = nullptr;
        ASORA_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        st.pipe_events.push_back(e);
    }
    hipStream_t up = st.side[0], down = st.side[1];
    const size_t plane = (size_t)N * N;
    int lo[KMAX + 1];
    for (int c = 0; c <= K; ++c) lo[c] = c * N / K;
    // sources of slab c: [sb[c], sb[c+1]) of the sorted list
    int sb[KMAX + 1];
    for (int c = 0; c <= K; ++c)
        sb[c] = (int)(std::lower_bound(st.sources.loaded.i0_sorted.begin(), st.sources.loaded.i0_sorted.end(), lo[c]) - st.sources.loaded.i0_sorted.begin());
    // reach[c][d]: do sources of slab c touch planes of slab d (within m planes, periodically)
    bool reach[KMAX][KMAX];
    for (int c = 0; c < K; ++c)
        for (int d = 0; d < K; ++d) {
            bool hit = false;
            if (sb[c + 1] > sb[c])
                for (int q = lo[d]; q < lo[d + 1] && !hit; ++q) {
                    // distance from plane q to the interval [lo[c], lo[c+1]) on the ring
                    int dist = 0;
                    if (q < lo[c]) dist = std::min(lo[c] - q, q + N - (lo[c + 1] - 1));
                    else if (q >= lo[c + 1]) dist = std::min(q - (lo[c + 1] - 1), lo[c] + N - q);
                    hit = dist <= m;
                }
            reach[c][d] = hit;
        }

    ASORA_HIP_TRY(hipMemsetAsync(st.grid[ASORA_GRID_PHI_ION], 0, 2 * bytes, st.stream));      // raytracing.cu:113 (+ twin)
    if (int rc = reset_counters()) return rc;
    RtParams base;
    fill_rt_params(base, R, sig, dr, minlogtau, dlogtau, NumTau);
    use_source_list(base, st, true);
    base.shape_src_count = NumSrc;
    st.rt.open = false;
    // the copy streams start behind whatever the main stream has done so far (earlier calls may still own the grids)
    ASORA_HIP_TRY(hipEventRecord(st.main_ready, st.stream));
    ASORA_HIP_TRY(hipStreamWaitEvent(up, st.main_ready, 0));
    ASORA_HIP_TRY(hipStreamWaitEvent(down, st.main_ready, 0));

    bool prepped[KMAX] = {}, traced[KMAX] = {}, sent[KMAX] = {};
    auto try_traces = [&]() -> int {
        for (int c = 0; c < K; ++c) {
            if (traced[c]) continue;
            bool ready = true;
            for (int d = 0; d < K; ++d) if (reach[c][d] && !prepped[d]) ready = false;
            if (!ready) continue;
            if (sb[c + 1] > sb[c]) {
                RtParams p = base;
                p.src_begin = sb[c]; p.src_count = sb[c + 1] - sb[c];
                if (int rc = launch_raytrace(st, p, false, false)) return rc;
            }
            traced[c] = true;
        }
        return 0;
    };
    // A device-to-host copy blocks the calling thread until it has run (measured; the uploads do not): so all uploads are
    // enqueued first, a slab's fold is enqueued as soon as the slab is final, and its download is only ISSUED one round
    // later, after the next round's kernels have been enqueued -- the host then waits in the copy while the GPU traces.
    // (Letting the fold kernel write the slab straight into the pinned host buffer instead was measured as well: 5.9 ms
    //  per call against 5.0 ms this way -- that kernel does not overlap with the uploads either.)
    bool folded[KMAX] = {};
    std::vector<int> to_send;
    auto try_folds = [&]() -> int {
        for (int d = 0; d < K; ++d) {
            if (folded[d]) continue;
            bool final_ = true;
            for (int c = 0; c < K; ++c) if (reach[c][d] && !traced[c]) final_ = false;
            if (!final_) continue;
            if (int rc = launch_fold_range(st, st.phi_t, st.grid[ASORA_GRID_PHI_ION], lo[d], lo[d + 1] - lo[d])) return rc;
            ASORA_HIP_TRY(hipEventRecord(st.pipe_events[K + d], st.stream));
            folded[d] = true;
            to_send.push_back(d);
        }
        return 0;
    };
    auto send = [&](int d) -> int {
        ASORA_HIP_TRY(hipStreamWaitEvent(down, st.pipe_events[K + d], 0));
        ASORA_HIP_TRY(hipMemcpyAsync(phi_ion + (size_t)lo[d] * plane, st.grid[ASORA_GRID_PHI_ION] + (size_t)lo[d] * plane,
                                     (size_t)(lo[d + 1] - lo[d]) * plane * sizeof(double), hipMemcpyDeviceToHost, down));   // cu:146
        sent[d] = true;
        return 0;
    };
    // upload order: the slabs the sources of slab 0 reach back into first (K-w ... K-1), then 0, 1, ...
    int w = 0;                                    // how many slabs back the sources of a slab reach
    for (int c = 0; c < K; ++c)
        for (int d = 0; d < K; ++d) {
            const int back = (c - d + K) % K;     // d lies `back` slabs behind c (more than half the ring: it lies ahead)
            if (reach[c][d] && back <= K / 2) w = std::max(w, back);
        }
    for (int q = 0; q < K; ++q) {
        const int c = (q + K - w) % K;
        ASORA_HIP_TRY(hipMemcpyAsync(st.grid[ASORA_GRID_XH_AV] + (size_t)lo[c] * plane, xh_av + (size_t)lo[c] * plane,
                                     (size_t)(lo[c + 1] - lo[c]) * plane * sizeof(double), hipMemcpyHostToDevice, up));   // cu:117
        ASORA_HIP_TRY(hipEventRecord(st.pipe_events[c], up));
    }
    for (int q = 0; q < K; ++q) {
        const int c = (q + K - w) % K;
        ASORA_HIP_TRY(hipStreamWaitEvent(st.stream, st.pipe_events[c], 0));
        if (int rc = launch_prepare_range(st, lo[c], lo[c + 1] - lo[c], false, nullptr)) return rc;
        prepped[c] = true;
        const std::vector<int> ready = to_send;       // final since the previous round: their folds are already enqueued
        to_send.clear();
        if (int rc = try_traces()) return rc;
        if (int rc = try_folds()) return rc;
        for (int d : ready) if (int rc = send(d)) return rc;
    }
    for (int d : to_send) if (int rc = send(d)) return rc;
    for (int c = 0; c < K; ++c) if (!traced[c] || !sent[c]) return fail(11, "do_all_sources: pipeline schedule incomplete (internal error)");
    ASORA_HIP_TRY(hipStreamSynchronize(down));
    ASORA_HIP_TRY(hipStreamSynchronize(up));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    st.grid_valid[ASORA_GRID_XH_AV] = true;
    st.grid_valid[ASORA_GRID_PHI_ION] = true;
    done = true;
    return 0;
}

} // namespace asora

using namespace asora;

extern "C" {

int asora_raytrace_device(double R, double sig, double dr, int src_begin, int src_count, double minlogtau,
                          double dlogtau, int NumTau)
{
    clear_error();
    if (int rc = require_init("raytrace_device")) return rc;
    return do_raytrace(R, sig, dr, src_begin, src_count, minlogtau, dlogtau, NumTau, nullptr);
}

int asora_raytrace_begin(double R, double sig, double dr, double minlogtau, double dlogtau, int NumTau)
{
    clear_error();
    if (int rc = require_init("raytrace_begin")) return rc;
    return rt_begin(R, sig, dr, minlogtau, dlogtau, NumTau, nullptr, true);
}

int asora_raytrace_begin_planes(double R, double sig, double dr, double minlogtau, double dlogtau, int NumTau,
                                const int *runs, int nruns)
{
    clear_error();
    if (int rc = require_init("raytrace_begin_planes")) return rc;
    State &st = state();
    st.rt.open = false;
    if (int rc = require_raytrace_inputs("raytrace_begin_planes", R, NumTau, true, true)) return rc;
    if (!st.opt[ASORA_OPT_Z_TRANSPOSED]) return fail(4, "raytrace_begin_planes: needs the [k][j][i] twins (ASORA_OPT_Z_TRANSPOSED = 1)");
    if (st.opt[ASORA_OPT_HEATING]) return fail(4, "raytrace_begin_planes: no heating rates on this path");
    if (nruns < 0 || (nruns > 0 && !runs)) return fail(3, "raytrace_begin_planes: bad plane runs");
    for (int q = 0; q < nruns; ++q)
        if (int rc = check_planes("raytrace_begin_planes", 3, "plane run outside the mesh", runs[2 * q], runs[2 * q + 1])) return rc;
    if (int rc = check_plane_flux(st, st.medium.plane, "raytrace_begin_planes", false, false)) return rc;
    if (int rc = reset_counters()) return rc;
    if (st.medium.plane.count > 0) {      // a face's sweep reads nHI of, and rates, every plane: the runs become the whole box
        if (int rc = launch_prepare_range(st, 0, st.N, true, st.grid[ASORA_GRID_PHI_ION])) return rc;
    } else
        for (int q = 0; q < nruns; ++q)
            if (int rc = launch_prepare_range(st, runs[2 * q], runs[2 * q + 1], true, st.grid[ASORA_GRID_PHI_ION])) return rc;
    fill_rt_params(st.rt_params, R, sig, dr, minlogtau, dlogtau, NumTau);
    if (int rc = launch_plane_flux(st, st.rt_params, st.grid[ASORA_GRID_PHI_ION], nullptr, false, nullptr)) return rc;
    st.rt_heat = false;
    st.rt_pipelined = false;
    st.rt_by_planes = true;
    st.rt.open = true;
    return 0;
}

int asora_raytrace_range(int src_begin, int src_count)
{
    clear_error();
    if (int rc = require_init("raytrace_range")) return rc;
    return rt_range(src_begin, src_count);
}

int asora_raytrace_fold(int i_begin, int i_count)
{
    clear_error();
    if (int rc = require_init("raytrace_fold")) return rc;
    return rt_fold(i_begin, i_count);
}

int asora_do_all_sources(double R, double *coldensh_out, double sig, double dr, const double *ndens,
                         const double *xh_av, double *phi_ion, int NumSrc, int m1, double minlogtau,
                         double dlogtau, int NumTau)
{
    (void)coldensh_out; (void)ndens;      // ignored by the reference too (raytracing.cu:116)
    clear_error();
    if (int rc = require_init("do_all_sources")) return rc;
    if (int rc = check_N("do_all_sources", m1)) return rc;
    if (!xh_av || !phi_ion) return fail(3, "do_all_sources: null xh_av / phi_ion");
    State &st = state();
    if (NumSrc > st.sources.loaded.num)
        return fail(3, "do_all_sources: NumSrc=" + std::to_string(NumSrc) + " exceeds the " +
                           std::to_string(st.sources.loaded.num) + " sources on the device");
    const size_t bytes = st.ncell * sizeof(double);
    {
        bool done = false;
        if (int rc = do_all_sources_pipelined(R, sig, dr, xh_av, phi_ion, NumSrc, minlogtau, dlogtau, NumTau, done)) return rc;
        if (done) return 0;
    }
    ASORA_HIP_TRY(hipMemcpyAsync(st.grid[ASORA_GRID_XH_AV], xh_av, bytes, hipMemcpyHostToDevice, st.stream)); // cu:117
    st.grid_valid[ASORA_GRID_XH_AV] = true;
    if (int rc = do_raytrace(R, sig, dr, 0, NumSrc, minlogtau, dlogtau, NumTau, nullptr)) return rc;
    ASORA_HIP_TRY(hipMemcpyAsync(phi_ion, st.grid[ASORA_GRID_PHI_ION], bytes, hipMemcpyDeviceToHost, st.stream)); // cu:146
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    return 0;
}

int asora_last_raytrace_counts(long long *gamma_cells, long long *evaluated_cells)
{
    clear_error();
    if (int rc = require_init("last_raytrace_counts")) return rc;
    long long zero = 0;
    return asora_last_raytrace_counts_ex(gamma_cells, evaluated_cells, &zero);
}

int asora_last_raytrace_counts_ex(long long *gamma_cells, long long *evaluated_cells, long long *zero_rates_left_out)
{
    clear_error();
    if (int rc = require_init("last_raytrace_counts")) return rc;
    std::vector<unsigned long long> h((size_t)COUNTER_FIELDS * COUNTER_SLOTS, 0ULL);
    ASORA_HIP_TRY(hipStreamSynchronize(state().stream));
    ASORA_HIP_TRY(hipMemcpy(h.data(), state().counters, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long tot[COUNTER_FIELDS] = {0ULL, 0ULL, 0ULL};
    for (int q = 0; q < COUNTER_SLOTS; ++q) for (int f = 0; f < COUNTER_FIELDS; ++f) tot[f] += h[(size_t)COUNTER_FIELDS * q + f];
    if (gamma_cells) *gamma_cells = (long long)tot[0];
    if (evaluated_cells) *evaluated_cells = (long long)tot[1];
    if (zero_rates_left_out) *zero_rates_left_out = (long long)tot[2];
    return 0;
}

int asora_last_raytrace_variant(void) { return state().last_variant; }

int asora_debug_launch_plan(int N, double R, int src_count, int shape_src_count, int cu_count, int flags, int shells, int max_cells,
                            int32_t *out)
{
    clear_error();
    if (N < 1 || src_count < 1 || !out || (shells >= 0 && max_cells < 0)) return fail(3, "debug_launch_plan: bad arguments");
    const State &st = state();
    RtPlanInput in{};
    plan_options(st, in);
    if (cu_count > 0) in.cu_count = cu_count;
    in.N = N; in.R = R; in.src_count = src_count; in.shape_src_count = shape_src_count;
    // as fill_rt_params reads them when a call begins
    in.grey = st.opt[ASORA_OPT_GREY_NOTABLES] != 0; in.open = st.opt[ASORA_OPT_OPEN_BOUNDARIES] != 0; in.z_transposed = in.z_transposed_opt;
    in.heat = flags & ASORA_PLAN_HEAT; in.dump = flags & ASORA_PLAN_DUMP; in.table_sets = flags & ASORA_PLAN_TABLE_SETS;
    in.host_positions = flags & ASORA_PLAN_HOST_POSITIONS; in.radius_stays = flags & ASORA_PLAN_RADIUS_STAYS;
    in.tau_zero_finite = (flags & ASORA_PLAN_RATE_TABLES) && in.skip_zero_rates != 2 && !in.grey;      // launch_raytrace: p.tau_zero
    for (int k = 0; k < ASORA_PLAN_WORDS; ++k) out[k] = 0;
    if (in.open) {
        const std::string why = open_boundaries_refusal(N, in.grey, in.global_atomics != 0, in.dump);
        if (!why.empty()) return fail(4, "raytrace: open boundaries (ASORA_OPT_OPEN_BOUNDARIES) " + why);
    }
    const RtShape sh = plan_shape(in);
    out[0] = sh.units; out[1] = sh.threads; out[2] = sh.aligned;
    if (shells < 0) return 0;
    RtPlan plan{};
    std::string why;
    if (int rc = plan_launch(in, sh, shells, max_cells, plan, why)) return fail(rc, why);
    plan_skip_zero(plan, plan.zero_form_exists && in.skip_zero_rates == 1);     // (left to the library, 0, the probes decide: not planned)
    const RtForm &f = plan.form;
    form_values(f, out + 3);
    out[16] = plan.use_lds; out[17] = (int32_t)plan.lds_bytes; out[18] = variant_word(f, sh.units, sh.aligned);
    out[19] = form_is_built(f); out[20] = plan.zero_form_exists; out[21] = 1;
    return 0;
}

int asora_debug_built_forms(int32_t *out, int capacity_rows, int *rows)
{
    clear_error();
    if (!rows || capacity_rows < 0 || (capacity_rows > 0 && !out)) return fail(3, "debug_built_forms: bad arguments");
    *rows = RT_FORM_COUNT;
    for (int r = 0; r < std::min(capacity_rows, RT_FORM_COUNT); ++r) {
        int v[13];
        form_values(RT_FORMS.row[r], v);
        std::copy(v, v + 13, out + 13 * (size_t)r);
    }
    return 0;
}

int asora_debug_form_launches(unsigned long long *counts, int capacity, int *rows)
{
    clear_error();
    if (!rows || capacity < 0 || (capacity > 0 && !counts)) return fail(3, "debug_form_launches: bad arguments");
    *rows = RT_FORM_COUNT;
    std::copy(form_launch_counts(), form_launch_counts() + std::min(capacity, RT_FORM_COUNT), counts);
    return 0;
}

int asora_debug_form_launches_reset(void)
{
    clear_error();
    reset_form_launch_counts();
    return 0;
}

int asora_debug_last_launch_form(int32_t form[13], int *row)
{
    clear_error();
    if (!form || !row) return fail(3, "debug_last_launch_form: null output");
    *row = last_launched_row();
    for (int k = 0; k < 13; ++k) form[k] = 0;
    if (*row >= 0) {
        int v[13];
        form_values(RT_FORMS.row[*row], v);
        std::copy(v, v + 13, form);
    }
    return 0;
}

int asora_debug_block_order(const int32_t *pos0, int begin, int count, int units, int nsrc, int aligned, int cu_count, int32_t *out,
                            size_t capacity, int *grid)
{
    clear_error();
    if (!pos0 || begin < 0 || count < 1 || units < 1 || units > MAX_UNITS || (nsrc != 1 && nsrc != 2) || !grid || (aligned && units != 6 && units != 12))
        return fail(3, "debug_block_order: bad arguments");
    const bool pairs = nsrc == 2;
    // as set_launch_grid (raytrace.hip) feeds the same functions
    std::vector<SrcPair> pl[2];
    std::vector<int> cls[2];
    int npairs[2] = {0, 0};
    int groups = pairs ? (count + 1) / 2 : count;
    if (pairs && aligned) {
        for (int ft = 0; ft < 2; ++ft) { pairs_by_class(pos0, begin, count, ft, pl[ft], cls[ft]); npairs[ft] = (int)pl[ft].size(); }
        groups = std::max(npairs[0], npairs[1]);
    }
    int spread = 0;
    if (cu_count <= 0) cu_count = state().cu_count;
    (void)launch_grid(groups, units, cu_count, spread);
    *grid = 0;
    if (spread) return 0;
    std::vector<int> face_type((size_t)units);
    for (int u = 0; u < units; ++u) face_type[(size_t)u] = unit_face(units, u) == 2 ? 1 : 0;
    const int *const pair_cls[2] = {cls[0].data(), cls[1].data()};
    std::vector<int32_t> order;
    const unsigned n = launch_block_order(pos0, begin, count, units, face_type.data(), pairs, aligned != 0, npairs, pair_cls, order);
    *grid = (int)n;
    if (!out || capacity < n) return 0;
    for (unsigned b = 0; b < n; ++b) {
        const int g = order[2 * (size_t)b], u = order[2 * (size_t)b + 1];
        int32_t *o = out + 4 * (size_t)b;
        o[0] = g; o[1] = u; o[2] = o[3] = -1;
        if (g < 0) continue;
        if (pairs && aligned) { const SrcPair &s = pl[face_type[(size_t)u]][(size_t)g]; o[2] = s.x; o[3] = s.y; }
        else if (pairs) { o[2] = begin + 2 * g; o[3] = 2 * g + 1 < count ? begin + 2 * g + 1 : -1; }
        else o[2] = begin + g;
    }
    return 0;
}

int asora_debug_coldens(double R, double sig, double dr, int source_index, double *coldens_out, int N)
{
    clear_error();
    if (int rc = require_init("debug_coldens")) return rc;
    if (int rc = check_N("debug_coldens", N)) return rc;
    if (!coldens_out) return fail(3, "debug_coldens: null output");
    State &st = state();
    if (int rc = check_open_boundaries(st, "debug_coldens", st.opt[ASORA_OPT_OPEN_BOUNDARIES] != 0, true)) return rc;
    const size_t bytes = st.ncell * sizeof(double);
    ASORA_HIP_TRY(hipMemsetAsync(st.staging, 0, bytes, st.stream));
    // the column density does not depend on the tables: trace with whatever is loaded
    const int numtau = st.sources.loaded.table_len > 0 ? st.sources.loaded.table_len : 1;
    const int grey_save = st.opt[ASORA_OPT_GREY_NOTABLES];
    if (!st.sources.tables) { st.opt[ASORA_OPT_GREY_NOTABLES] = 1; st.coldens_only = true; }
    int rc = do_raytrace(R, sig, dr, source_index, 1, -20.0, 1.0, numtau, st.staging);
    st.opt[ASORA_OPT_GREY_NOTABLES] = grey_save; st.coldens_only = false;
    if (rc) return rc;
    ASORA_HIP_TRY(hipMemcpyAsync(coldens_out, st.staging, bytes, hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    return 0;
}

} // extern "C"
