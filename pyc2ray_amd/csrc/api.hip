// api.hip -- the device state of libasora_hip.so, what sets it up and tears it down (the arena of the grids, device_init /
// device_close, options, timers), and the checks every entry point shares.  The entry points themselves are in the *_api.hip
// units beside this file, one per concern.  The reference counterparts are src/asora/memory.cu (state) and
// src/asora/python_module.cu (CPython wrappers); see include/asora_hip.h for the mapping.
#include "asora_internal.hpp"

#include <chrono>

namespace asora {

static State g_state;
static std::string g_error;

State &state() { return g_state; }
int fail(int code, const std::string &msg) { g_error = msg; return code; }
void clear_error() { g_error.clear(); }

// Kernel timing with HIP events on the library's stream.  Events are recorded without any host
// synchronisation (so that enabling the timers does not perturb what is being timed) and resolved
// when the totals are queried, or when the pool of pending pairs is full.
static int flush_timers()
{
    State &st = g_state;
    if (st.pending_timers.empty()) return 0;
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    for (hipStream_t s : st.side) if (s) ASORA_HIP_TRY(hipStreamSynchronize(s));
    for (auto &pt : st.pending_timers) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pt.e0, pt.e1) == hipSuccess) {
            st.k_ms[pt.which] += (double)ms;
            st.k_n[pt.which] += 1;
        }
        st.free_events.push_back(pt.e0);
        st.free_events.push_back(pt.e1);
    }
    st.pending_timers.clear();
    return 0;
}

static hipEvent_t take_event()
{
    State &st = g_state;
    if (!st.free_events.empty()) { hipEvent_t e = st.free_events.back(); st.free_events.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

KernelTimer::KernelTimer(int w, hipStream_t s)
    : which(w), on(g_state.opt[ASORA_OPT_TIMING] != 0 && g_state.stream != nullptr), stream(s ? s : g_state.stream)
{
    if (!on) return;
    if (g_state.pending_timers.size() >= 4096) (void)flush_timers();
    e0 = take_event();
    e1 = take_event();
    (void)hipEventRecord(e0, stream);
}
KernelTimer::~KernelTimer()
{
    if (!on) return;
    (void)hipEventRecord(e1, stream);
    g_state.pending_timers.push_back({which, e0, e1});
}

// stream, events and the chemistry reduction buffers: needed with or without device_init
int ensure_runtime()
{
    State &st = g_state;
    if (st.stream) return 0;
    ASORA_HIP_TRY(hipSetDevice(st.device));
    hipDeviceProp_t prop;
    ASORA_HIP_TRY(hipGetDeviceProperties(&prop, st.device));
    st.cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    ASORA_HIP_TRY(hipStreamCreateWithFlags(&st.stream, hipStreamNonBlocking));
    for (int q = 0; q < 2; ++q) {
        ASORA_HIP_TRY(hipStreamCreateWithFlags(&st.side[q], hipStreamNonBlocking));
        ASORA_HIP_TRY(hipEventCreateWithFlags(&st.side_done[q], hipEventDisableTiming));
    }
    ASORA_HIP_TRY(hipEventCreateWithFlags(&st.main_ready, hipEventDisableTiming));
    st.red_blocks = chemistry_reduction_blocks(st);
    if (int rc = st.red_partial.allocate(3 * (size_t)st.red_blocks)) return rc;
    if (int rc = st.red_final.allocate(3)) return rc;
    if (int rc = st.red_host.allocate(3)) return rc;
    if (int rc = st.counters.allocate((size_t)COUNTER_FIELDS * COUNTER_SLOTS)) return rc;
    ASORA_HIP_TRY(hipMemset(st.counters, 0, sizeof(unsigned long long) * COUNTER_FIELDS * COUNTER_SLOTS));
    return 0;
}

// What dies with the mesh.  The buffers know it themselves (MeshBuffer / MeshPinned fields of State, device_memory.hpp); the
// bookkeeping beside them goes back to what a fresh State holds.
static int release_all()
{
    State &st = g_state;
    OwnedMemory::release_all_of(LIFETIME_MESH);
    st.thermal.mode = {}; st.medium = {}; st.sources.loaded = {}; st.zero.verdict = {}; st.evolve.flags = {}; st.reach.d = {};
    st.rt = {}; st.redshift.vmax = 0.0; st.temp_probe.valid = false;
    for (int g = 0; g < ASORA_GRID_COUNT; ++g) { st.grid[g] = nullptr; st.grid_valid[g] = false; }     // (aliases of the arena and of the three grids beside it)
    st.nhi = st.staging = st.acc = nullptr;
    st.nhi_t = st.phi_t = st.heat_t = nullptr;    // second halves of nhi / phi_ion / phi_heat
    release_pair_lists(st);
    release_geometry(st);
    if (st.zero.done) { (void)hipEventDestroy(st.zero.done); st.zero.done = nullptr; }
    st.init = false; st.N = 0; st.ncell = 0;
    return 0;
}

int require_init(const char *who)
{
    if (!g_state.init) return fail(2, std::string(who) + ": device not initialised (call asora_device_init first)");
    return 0;
}

int check_N(const char *who, int N)
{
    if (N != g_state.N)
        return fail(3, std::string(who) + ": mesh size " + std::to_string(N) + " does not match device_init(" +
                           std::to_string(g_state.N) + ")");
    return 0;
}

int check_planes(const char *who, int code, const char *tail, int i_begin, int i_count)
{
    if (i_begin < 0 || i_count < 0 || i_begin + i_count > g_state.N) return fail(code, std::string(who) + ": " + tail);
    return 0;
}

int check_sources(const char *who, int code, const std::string &tail, int src_begin, int src_count)
{
    if (src_begin < 0 || src_count < 0 || src_begin + src_count > g_state.sources.loaded.num) return fail(code, std::string(who) + ": " + tail);
    return 0;
}

int require_grids(const char *who, std::initializer_list<int> grids)
{
    for (int g : grids)
        if (!g_state.grid_valid[g]) return fail(4, std::string(who) + ": grid " + std::to_string(g) + " holds no data");
    return 0;
}

} // namespace asora

using namespace asora;

extern "C" {

// ---------------------------------------------------------------------------------------------
// Where the grids lie.  The fused pass streams 5 grids in and 6-7 out at once, and how fast the memory side takes that mix depends
// on WHERE those grids lie physically: the same kernel on the same box moves 5.2-5.4 TB/s on most placements and 6.0-6.2 TB/s on
// a fifth to a third of them, stable for the life of the allocation (tools/micro/placement_probe.hip; some boxes offer one kind only;
// with one hipMalloc per grid the sets spread between the two, which is what earlier rounds recorded as the "state of the box":
// fused pass 0.25 ... 0.31 ms from run to run).  Nothing a process can read tells the two kinds apart beforehand, so device_init
// tries a FEW allocations of the whole arena, three launches of a kernel with the pass's stream mix on each, keeps the fastest and
// frees the others.  Round 6 bounds (round 5 tried up to 32 within a quarter of the free memory: 56 GB and 96 probe launches on a
// box of one kind, for a 4 % spread):
//   * at most ASORA_OPT_PLACEMENT_CANDIDATES allocations (0 = default 8; 1 = take the first; the environment variable
//     ASORA_PLACEMENT_CANDIDATES does the same for a process that cannot call asora_set_option before device_init);
//   * what is held during the probe stays within an EIGHTH of the free device memory (512^3: two candidates of 14 GiB);
//   * it stops as soon as it holds a candidate 7 % faster than another (both kinds seen, one of the fast kind in hand); a box of one
//     kind costs all eight (10 ms at 256^3: one placement in eight to one in three is of the fast kind where both occur, so fewer
//     tries would miss it too often).
// The losers are held until the probe ends: a freed arena's pages are what the next allocation of that size gets back, so
// freeing as it goes would time the same placement again and again.  Meshes below 128^3 take the first allocation (their grids
// sit in the caches).  asora_debug_placement reports what was tried and what the probe cost.
// On a box with both kinds, alternating processes (profiles/r05_ab_placement.txt): first allocation taken 1.392-1.395 ms per step
// in five runs of six (fused pass 0.282, trace 1.079), probed 1.333-1.337 in six of six (0.245, 1.060; 2-6 candidates tried).
// ---------------------------------------------------------------------------------------------
constexpr int ARENA_CANDIDATES = 8;        // default bound (one placement in eight to one in three is of the fast kind where both occur)
constexpr int ARENA_SLOTS = 14;            // ndens, xh, xh_av, temp, xh_intermed, 4 accumulators, nhi x 2, phi_ion x 2, staging
__global__ void __launch_bounds__(256) placement_probe_kernel(char *arena, size_t slot, size_t n)
{
    // 5 read streams (non-temporal, as the pass loads them) and 7 write streams over the first 12 slots
    const double *in[5]; double *out[7];
    for (int q = 0; q < 5; ++q) in[q] = reinterpret_cast<const double *>(arena + q * slot);
    for (int q = 0; q < 7; ++q) out[q] = reinterpret_cast<double *>(arena + (5 + q) * slot);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 5; ++q) s += __builtin_nontemporal_load(in[q] + i);
#pragma unroll
        for (int q = 0; q < 7; ++q) out[q][i] = s;
    }
}

static int choose_arena(State &st, size_t slot, int slots)
{
    const auto wall0 = std::chrono::steady_clock::now();
    const size_t total = slot * (size_t)slots;
    int want = st.opt[ASORA_OPT_PLACEMENT_CANDIDATES] > 0 ? st.opt[ASORA_OPT_PLACEMENT_CANDIDATES] : ARENA_CANDIDATES;
    if (const char *e = getenv("ASORA_PLACEMENT_CANDIDATES")) want = std::max(1, atoi(e));
    want = std::min(want, 32);
    if (st.N < 128) want = 1;
    size_t free_b = 0, all_b = 0;
    if (want > 1 && hipMemGetInfo(&free_b, &all_b) == hipSuccess && total > 0)
        want = (int)std::max<size_t>(1, std::min<size_t>((size_t)want, (size_t)(0.125 * (double)free_b) / total));     // (several ranks may share a GPU)
    st.arena_candidates = 0; st.arena_probe_ms = st.arena_probe_worst_ms = st.arena_probe_wall_ms = 0.0;
    if (want == 1) {
        if (int rc = st.arena.allocate(total)) return rc;
        st.arena_candidates = 1;
        return 0;
    }
    hipEvent_t t0, t1;
    ASORA_HIP_TRY(hipEventCreate(&t0)); ASORA_HIP_TRY(hipEventCreate(&t1));
    std::vector<char *> cand;
    std::vector<float> ms;
    int best = -1;
    float worst = 0.0f;
    const size_t n = st.ncell;
    for (int c = 0; c < want; ++c) {
        char *a = nullptr;
        if (hipMalloc(&a, total) != hipSuccess) { (void)hipGetLastError(); break; }
        cand.push_back(a);
        float t = 1e30f;
        for (int rep = 0; rep < 3; ++rep) {
            (void)hipEventRecord(t0, st.stream);
            hipLaunchKernelGGL(placement_probe_kernel, dim3(1024), dim3(256), 0, st.stream, a, slot, n);
            (void)hipEventRecord(t1, st.stream);
            if (hipEventSynchronize(t1) != hipSuccess) { t = 1e30f; break; }
            float e = 0.0f;
            (void)hipEventElapsedTime(&e, t0, t1);
            if (rep >= 1) t = std::min(t, e);              // (the first launch maps the pages)
        }
        ms.push_back(t);
        if (best < 0 || t < ms[(size_t)best]) best = c;
        worst = std::max(worst, t);
        if (c >= 1 && ms[(size_t)best] <= 0.93f * worst) break;     // both kinds seen, and one of the fast kind in hand
    }
    (void)hipEventDestroy(t0); (void)hipEventDestroy(t1);
    if (best < 0) return fail(2, "device_init: out of device memory for the grids");
    for (size_t c = 0; c < cand.size(); ++c) if ((int)c != best) (void)hipFree(cand[c]);
    st.arena.adopt(cand[(size_t)best], total);
    st.arena_candidates = (int)cand.size();
    st.arena_probe_ms = ms[(size_t)best]; st.arena_probe_worst_ms = worst;
    st.arena_probe_wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    return 0;
}

void asora_debug_placement(int *candidates, double *chosen_probe_ms, double *slowest_probe_ms)
{
    if (candidates) *candidates = g_state.arena_candidates;
    if (chosen_probe_ms) *chosen_probe_ms = g_state.arena_probe_ms;
    if (slowest_probe_ms) *slowest_probe_ms = g_state.arena_probe_worst_ms;
}

void asora_debug_init_cost(double *device_init_ms, double *placement_probe_ms)
{
    if (device_init_ms) *device_init_ms = g_state.device_init_wall_ms;
    if (placement_probe_ms) *placement_probe_ms = g_state.arena_probe_wall_ms;
}

int asora_debug_live_buffers(int lifetime, long long *buffers, unsigned long long *bytes)
{
    clear_error();
    if (lifetime != LIFETIME_MESH && lifetime != LIFETIME_PROCESS) return fail(3, "debug_live_buffers: lifetime must be 0 (mesh) or 1 (process)");
    long long n = 0; unsigned long long b = 0;
    OwnedMemory::live((Lifetime)lifetime, n, b);
    if (buffers) *buffers = n;
    if (bytes) *bytes = b;
    return 0;
}

const char *asora_last_error(void) { return g_error.c_str(); }

int asora_device_init_ex(int N, int num_src_par, int device_id)
{
    clear_error();
    State &st = g_state;
    const auto init_wall0 = std::chrono::steady_clock::now();
    // validate everything first: a refused re-initialisation leaves the working state as it was
    if (N < 2 || N > 1280) return fail(1, "device_init: N must be in [2, 1280] (32-bit cell indices over 2 N^3)");
    if (st.stream && device_id != st.device) return fail(1, "device_init: the device cannot change within a process");
    if (st.init) release_all();
    st.device = device_id;
    if (int rc = ensure_runtime()) return rc;
    st.N = N;
    st.ncell = (size_t)N * N * N;
    st.num_src_par = num_src_par;
    st.auto_init = false;
    const size_t bytes = st.ncell * sizeof(double);
    // ONE allocation for every N^3 grid of the hot loop (choose_arena); the rate grids and nHI carry their [k][j][i] twin directly
    // behind them (one 32-bit index reaches both)
    const size_t slot = (bytes + 4095) / 4096 * 4096;
    if (int rc = choose_arena(st, slot, ARENA_SLOTS)) return rc;
    {
        size_t at = 0;
        auto take = [&](size_t grids) { double *q = reinterpret_cast<double *>(st.arena + at); at += grids * slot; return q; };
        // (two-grid buffers: the second half starts ncell doubles behind the first -- inside the two slots either way)
        st.grid[ASORA_GRID_NDENS] = take(1); st.grid[ASORA_GRID_XH] = take(1); st.grid[ASORA_GRID_XH_AV] = take(1);
        st.grid[ASORA_GRID_TEMP] = take(1); st.grid[ASORA_GRID_XH_INTERMED] = take(1);
        st.acc = take(4);
        st.nhi = take(2);
        st.grid[ASORA_GRID_PHI_ION] = take(2);
        st.staging = take(1);
    }
    for (int g = 0; g < ASORA_GRID_COUNT; ++g)
        if (g != ASORA_GRID_PHI_HEAT && g != ASORA_GRID_TEMP_END && g != ASORA_GRID_CLUMP && !st.grid[g]) return fail(11, "device_init: a grid without a place in the arena (internal error)");
    st.nhi_t = st.nhi + st.ncell;
    st.phi_t = st.grid[ASORA_GRID_PHI_ION] + st.ncell;
    st.heat_t = nullptr;
    st.evolve.flags.sets_known = false;
    {   // per-workgroup partials of the tiled chemistry pass: the j-chunk count is rounded up per (k tile x i tile), so a
        // RANGE of planes (asora_chemistry_range: a multi-GPU rank's slab) can need more workgroups than the whole grid
        size_t worst = 0;
        for (int planes = 1; planes <= N; ++planes) worst = std::max(worst, chemistry_tile_blocks(st, N, planes));
        if (int rc = ensure_red_capacity(3 * worst)) return rc;
    }
    st.init = true;
    st.device_init_wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - init_wall0).count();
    return 0;
}

int asora_device_init(int N, int num_src_par)
{
    int dev = g_state.stream ? g_state.device : 0;
    if (!g_state.stream) {
        // the reference uses the current device (memory.cu:39)
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    }
    return asora_device_init_ex(N, num_src_par, dev);
}

int asora_device_close(void)
{
    clear_error();
    if (int rc = require_init("device_close")) return rc;
    ASORA_HIP_TRY(hipStreamSynchronize(g_state.stream));
    return release_all();
}

void *asora_stream(void) { return (void *)g_state.stream; }

int asora_set_option(int option, int value)
{
    clear_error();
    if (option < 0 || option >= ASORA_OPT_COUNT) return fail(3, "set_option: unknown option");
    g_state.opt[option] = value;
    return 0;
}

int asora_get_option(int option)
{
    if (option < 0 || option >= ASORA_OPT_COUNT) return -1;
    return g_state.opt[option];
}

int asora_kernel_time_ms(int kernel, double *total_ms, long *launches)
{
    clear_error();
    if (kernel < 0 || kernel >= ASORA_KERNEL_SLOTS) return fail(3, "kernel_time_ms: unknown kernel");
    if (int rc = flush_timers()) return rc;
    if (total_ms) *total_ms = g_state.k_ms[kernel];
    if (launches) *launches = g_state.k_n[kernel];
    return 0;
}

int asora_kernel_time_reset(void)
{
    (void)flush_timers();
    for (int k = 0; k < ASORA_KERNEL_SLOTS; ++k) { g_state.k_ms[k] = 0.0; g_state.k_n[k] = 0; }
    return 0;
}

int asora_synchronize(void)
{
    clear_error();
    if (!g_state.stream) return 0;
    ASORA_HIP_TRY(hipStreamSynchronize(g_state.stream));
    ASORA_HIP_TRY(hipDeviceSynchronize());
    return 0;
}

} // extern "C"
