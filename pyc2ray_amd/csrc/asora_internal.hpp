// Internal declarations shared by the translation units of libasora_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/asora_hip.h"
#include "device_memory.hpp"
#include "raytrace_plan.hpp"

namespace asora {

// Source-independent geometry of one octant, tabulated on the host (raytrace.hip), device pointers.
// A flat sequence of steps of workgroup-size entries; see the table description above the kernel.
struct OctGeomDev {
    const uint4 *cellA;          // { |di| | |dj|<<10 | |dk|<<20 | face<<30, own slot | flags, path (double) }
    const uint4 *cellB;          // shell-buffer slots of the four upstream corners in shell s-1
    int nsteps;
    int info;                    // sign bits of the unit | (merge axis + 1) << 3 | rates-the-source-cell << 5
    int inner;                   // tables that share their inner shells (geometry_device.hip): steps [0, inner >> 8) are read through
                                 // cellA / cellB of table (inner & 255) of the same array, the rest through this table's own
                                 // pointers (which are shifted: entry e of the table is cellA[e] on either side).  0: all its own
    int reserved_;
};

constexpr int MAX_UNITS = 96;   // workgroups per source: 8 octants, 12 mirrored sector pairs, 24 sectors or 96 sector wedges

// Parameters of one raytrace launch (raytrace.hip)
// The work counters of a trace (rated pairs, evaluated cells): every wave adds its share when it ends.  On TWO addresses those
// adds serialise in the memory-side atomic unit at ~12 ns each and set a floor of 25 ns per workgroup under the whole
// launch (0.2 ms for 8000 workgroups, whatever the radius); spread over COUNTER_SLOTS addresses by workgroup index they cost
// nothing, and asora_last_raytrace_counts sums the slots.
constexpr int COUNTER_SLOTS = 4096;
constexpr int ZERO_PROBE_SLOTS = 256;   // RtParams.zero_probe: {rated pairs, exact zeros left out} of ONE launch, spread over these slots
constexpr int COUNTER_FIELDS = 3;   // per slot: rated pairs, evaluated cells, rated pairs whose rate was exactly +0 and was not added

// Upper limit of the real table index in photo_lookuptable: min(float(NumTau), ...) of rates.cu:79 / real(NumTau) of
// photorates.f90:141, and never beyond the last element the device table holds (the reference reads one past the end when the
// caller passes NumTau = len(table), asora_core.py:54; index table_len - 1 is the pair {T[last], 0}).  With the limit applied to
// the REAL index the integer index needs no clamp of its own (rates_device.hpp, lookup_issue).
inline double lut_index_limit(int NumTau, int table_len)
{
    const double by_reference = (double)(float)NumTau, by_table = (double)(table_len > 0 ? table_len - 1 : 0);
    return by_reference < by_table ? by_reference : by_table;
}

// The constants of the real table index k0 + k1 log2(tau) + kc (rates_device.hpp, lookup_issue) for every launcher:
// k1 = log10(2)/dlogtau and k0 = 1 - minlogtau/dlogtau as the nearest doubles, and kc, what those two roundings leave out.  k0
// cancels against k1 log2(tau) at small optical depths (k0 = 1668, index 1 at tau = 10^minlogtau), so its rounding -- half an
// ulp of 1668, 1.1e-13 -- and k1's times log2(tau) weigh several ulp of a small index; (k0 - K0) + (k1 - K1) log2(tau) against
// the exact K0, K1 is linear in log2(tau), and its value where the index is 1, L0 = minlogtau/log10(2), serves the whole
// table: what remains, (k1 - K1)(log2 tau - L0) = 2e-17 (index - 1), is far below an ulp of the index everywhere.  Formed
// in doubles from the exact remainders of the divisions (fma) and of the sum (two-sum).
struct LutIndex { double k1, k0, kc; };
inline LutIndex lut_index_constants(double minlogtau, double dlogtau)
{
    const double log10_2 = 0.30102999566398119521, log10_2_lo = -2.8037281277851703e-18;     // hi + lo = log10(2) to 2^-106
    LutIndex c;
    c.k1 = log10_2 / dlogtau;
    const double q = minlogtau / dlogtau;
    c.k0 = 1.0 - q;
    const double k1_lo = (std::fma(-c.k1, dlogtau, log10_2) + log10_2_lo) / dlogtau;       // K1 = k1 + k1_lo
    const double q_lo = std::fma(-q, dlogtau, minlogtau) / dlogtau;                         // minlogtau/dlogtau = q + q_lo
    const double bb = c.k0 - 1.0, sum_lo = (1.0 - (c.k0 - bb)) + (-q - bb);                // 1 - q = k0 + sum_lo
    c.kc = (sum_lo - q_lo) + k1_lo * (minlogtau / log10_2);                                 // -((k0 - K0) + (k1 - K1) L0)
    if (!std::isfinite(c.kc)) c.kc = 0.0;
    return c;
}

// Plane-parallel flux through faces of the box (asora_plane_flux; plane_flux.hip)
struct PlaneFluxSet {
    int count;                         // 0: off
    int face[6];                       // 0 ... 5 = -x +x -y +y -z +z, the face the radiation enters through
    int spec[6];                       // table set of the face
    double flux[6];
};                                     // (a plain aggregate: RtParams stays trivial; PlaneFluxSet{} is "off")

struct RtParams {
    int N;
    int S;                 // last Chebyshev shell over all octants
    int max_cells;         // largest shell; slot max_cells of a shell buffer holds 0.0
    double R;
    double sig, dr;
    double minlogtau, dlogtau, numtau_f;
    double lut_k1, lut_k0; // table index = 1 + (log10 tau - minlogtau)/dlogtau = lut_k1*log2(tau) + lut_k0
    double tau_zero;       // ASORA_OPT_SKIP_ZERO_RATES: thick cells with tau_in >= tau_zero get exactly +0 (both lookups clamp) and are not added; +inf = add everything
    int NumTau, table_len;
    int fortran_consts, grey, z_transposed;
    int src_begin, src_count;
    int shape_src_count;   // source count the launch shape is chosen for (the whole call's, not a pipelined range's)
    int split_desc;        // 1: N > 512 -- the buffer descriptors of the rate atomics span ONE layout of the grid each (raytrace.hip)
    int radius_stays;      // decided once per call (note_call_radius): the line-aligned tables may be built for this radius
    OctGeomDev geom[MAX_UNITS]; // by value: pointers read from the kernarg segment are known-global to the compiler
    int units;                  // workgroups per source: 8 octants, 24 octant-sectors, 12 mirrored sector pairs, 96 sector wedges
    int spread;                 // 1: block b = (source b / units, unit b % units) -- a source's units on different XCDs
    const double2 *logtab;      // log2 table of log2_pos (ensure_logtab)
    unsigned ncell;             // N^3: the [k][j][i] copy of a grid starts ncell elements after its [i][j][k] form
    const double *nhi;          // nHI, [i][j][k] then [k][j][i]
    double *phi;                // Gamma accumulator, [i][j][k] then [k][j][i]
    const double2 *tables;      // thick, thin, heat thick, heat thin, each table_stride(len) doubles (pack_rate_table, rates_device.hpp)
    double *heat;               // heating accumulator (HEAT kernels), [i][j][k] then [k][j][i]
    const int32_t *src_pos;
    const double *src_flux;
    double *dump;               // debug: outgoing column density (N^3) or nullptr
    double *shell_scratch;      // global shell buffers when they do not fit LDS, else nullptr
    unsigned long long *counters;
    const int *done_flag;       // evolve loop: device flag "the step has converged" -> the launch does nothing; or nullptr
    unsigned long long *zero_probe;   // SKIP_ZERO kernels: where a probe launch sums what it rated and what it left out, or nullptr
    // ---- rows cut at 64-byte lines (ASORA_OPT_ALIGNED_ROWS; plan_shape) ----
    int aligned;                // 1: geom[] holds 8 x units tables, [class * units + unit], class = source position & 7 along the
                                //    memory-contiguous axis of the unit's face (k for the x- and y-sectors, i for the z-sector)
    const int2 *pairs[2];       // NSRC = 2 && aligned: the workgroup's two sources (indices into src_pos; .y < 0: only one) for
    int npairs[2];              //    [0] units of the x- / y-sector (equal k & 7), [1] units of the z-sector (equal i & 7)
    // ---- SUBBOX kernels only (the reference's CPU semantics on the tabulated geometry, raytrace.hip / subbox.hip) ----
    int sb_k0[12], sb_k1[12];   // per unit: this launch sweeps the table steps [k0, k1) = the shells of one sub-box (multiples of 3)
    int sb_first;               // 1: the launch starts at the source cell; 0: it continues from the trailing shell in sb_trail
    int sb_edge_r, sb_edge_l;   // faces of the current sub-box on the + / - side of every axis (raytracing.f90:199-200)
    int flux_src;               // >= 0: every source shines with the flux of this one (f90:500,503); -1: its own
    const int *sb_active;       // per source of the batch: still growing?
    double *sb_loss;            // per source of the batch: photons through the faces of the current sub-box
    double *sb_trail;           // per (source, unit): the last shell swept, handed to the next sub-box's launch
    // ---- per-source spectra (asora_spectra_to_device; appended, so the fields above keep their offsets) ----
    const int32_t *src_spec;    // table set of each source, indexed like src_pos / src_flux; nullptr: every source set 0
    unsigned spec_stride;       // double2 entries from one set's [thick | thin | heat thick | heat thin] block to the next
    // ---- dispatch order (block_order, raytrace_plan.hpp) ----
    const int2 *order;          // block b sweeps {group, unit} = order[b], {-1, -1}: nothing; nullptr: the arithmetic map of the prologue
    // ---- open boundaries (ASORA_OPT_OPEN_BOUNDARIES as it stood when the call began; read by the launcher, not by the kernels) ----
    int open_bc;
    // ---- plane-parallel flux (asora_plane_flux as it stood when the call began; read by launch_plane_flux, not by the kernels above) ----
    PlaneFluxSet plane;
    // ---- the table index's correction term (lut_index_constants; appended) ----
    double lut_kc;
};

// Constants of the thermal form of the chemistry pass (asora_thermal_params; chemistry.hip: thermal_integrate)
struct ThermalConsts {
    double relative_denergy = 0.1;   // largest relative change of the thermal energy per substep
    double t_floor = 1.0;            // K
    double t_cmb = 0.0;              // K, at the current redshift
    int max_substeps = 10000;
    unsigned cooling_mask = 31u;     // THERMAL_COOL_* bits
    int compton = 0;                 // Compton exchange only with a redshift
};
constexpr unsigned THERMAL_COOL_RECOMB = 1u, THERMAL_COOL_COLION = 2u, THERMAL_COOL_COLEXC = 4u, THERMAL_COOL_BREMS = 8u,
                   THERMAL_COOL_COMPTON = 16u;

// Device-side bookkeeping of the evolve loop (asora_evolve_begin / _enqueue / _poll): the convergence test of
// pyc2ray/evolve.py:216-236 is evaluated on the device right behind the chemistry reductions, so that several outer
// iterations can be enqueued at once; launches that come after convergence see `done` and do nothing.
constexpr int EVOLVE_HIST = 64;
struct EvolveStatus {
    int niter;                         // outer iterations carried out
    int done;                          // 1 once the test of evolve.py:231-232 has passed
    double prev1, prev0;               // sum(xh_intermed), sum(1 - xh_intermed) of the previous iteration (evolve.py:130-131,234-235)
    double conv_criterion, conv_fraction;
    double hist[EVOLVE_HIST][5];       // ring by iteration: conv_flag, sum1, sum0, rel_change_xh1, rel_change_xh0
};

// ---------------------------------------------------------------------------------------------
// Process-global device state (the role of src/asora/memory.cu:20-29).  Every buffer is an owning field (device_memory.hpp) of the
// unit it belongs to: MeshBuffer / MeshPinned die with the mesh, ProcessBuffer / ProcessPinned never.  The scalar bookkeeping that
// dies with the mesh stands in a plain aggregate beside its buffers, which release_all() (api.hip) resets by one assignment.
// ---------------------------------------------------------------------------------------------
struct State {
    bool init = false;
    bool auto_init = false;        // initialised by c2ray_do_all_sources on its own (may re-initialise for another N)
    int device = 0;
    int N = 0;
    size_t ncell = 0;
    int num_src_par = 0;           // accepted, unused (no per-source N^3 scratch in this build)
    int cu_count = 256;

    // every N^3 grid of the hot loop lives in ONE allocation (api.hip: choose_arena), picked among several candidates by a probe;
    // PHI_HEAT (with its [k][j][i] twin), TEMP_END and CLUMP are allocations of their own, made on first use (ensure_optional_grid).
    // grid[] aliases both kinds
    MeshBuffer<char> arena;
    MeshBuffer<double> phi_heat_grid, temp_end_grid, clump_grid;
    double *grid[ASORA_GRID_COUNT] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool grid_valid[ASORA_GRID_COUNT] = {false, false, false, false, false, false, false, false, false};
    int arena_candidates = 0;               // how many were tried
    double arena_probe_ms = 0.0, arena_probe_worst_ms = 0.0;     // the chosen one's probe time, the slowest candidate's
    double arena_probe_wall_ms = 0.0, device_init_wall_ms = 0.0; // host wall clock of the whole probe / of the last device_init

    // derived per raytrace call (aliases of the arena)
    // each of these is the second half of a 2 N^3 allocation whose first half is the [i][j][k] grid
    double *nhi = nullptr;     // ndens*(1-xh_av), [i][j][k]
    double *nhi_t = nullptr;   // = nhi + N^3: same, transposed [k][j][i]
    double *phi_t = nullptr;   // = grid[PHI_ION] + N^3: rate accumulator for z-faces, transposed [k][j][i]
    double *heat_t = nullptr;  // = grid[PHI_HEAT] + N^3: heating-rate accumulator for z-faces, transposed
    double *staging = nullptr; // N^3 staging grid for 'F'-order transfers / debug dumps
    // fused evolve loop (asora_evolve_*): raytrace accumulators of their own ([i][j][k] then [k][j][i]; the chemistry
    // kernel folds them into PHI_ION and zeroes them), device-side convergence bookkeeping
    // TWO sets of accumulators, each [i][j][k] then [k][j][i] (4 N^3 doubles).  Iteration k of a
    // time step traces into set (evolve.base + k - 1) & 1; its fused pass reads that set WITHOUT destroying it and zeroes the
    // other one for iteration k + 1.  The rates of the last iteration carried out therefore survive in their set until the
    // host asks for them (asora_evolve_poll folds them into PHI_ION): the pass writes no rate grid (88 instead of 96 B per cell).
    double *acc = nullptr;

    // the sources and their spectra: the rate tables, num_spec blocks of [thick | thin | heat thick | heat thin] (pack_rate_table),
    // spec_stride apart; the source list as uploaded and ordered by the first coordinate (pipelined asora_do_all_sources); the
    // table set of each source (asora_source_spectra_to_device) in both orders, null while every source has set 0
    struct Sources {
        MeshBuffer<double2> tables;
        MeshBuffer<int32_t> pos, pos_sorted, spec, spec_sorted;
        MeshBuffer<double> flux, flux_sorted;
        struct Loaded {
            int table_len = 0, num = 0;    // entries of a table; sources
            int num_spec = 1;              // table sets on the device (asora_spectra_to_device; the one-set uploads: 1)
            size_t spec_stride = 0;        // double2 entries of one set's block (rate_block_entries)
            bool heat_tables = false;
            int spec_max = 0;              // the largest table set uploaded for a source, checked against num_spec before every trace
            std::vector<int> i0_sorted;
            // host copies of the two source lists (as uploaded, and in lexicographic order of the position): who shares a
            // workgroup with whom on aligned tables is decided from them (source_pairs_by_class)
            std::vector<int32_t> pos_host, pos_sorted_host;
        } loaded;
    } sources;
    long src_generation = 0;                // counts asora_source_data_to_device calls
    std::vector<hipEvent_t> pipe_events;

    // raytracing geometry tables (built once per (N, R, dr), see raytrace.hip)
    std::vector<void *> geom_owned;
    size_t geom_bytes = 0;                  // device memory the current tables occupy (shells shared by several tables count once)
    OctGeomDev geom_host[MAX_UNITS];        // device pointers of the unit tables ([class * units + unit] when geom_aligned)
    bool geom_aligned = false;
    // exact-zero rates (ASORA_OPT_SKIP_ZERO_RATES = 0): decide_skip_zero takes the kernels that leave them out while its probes
    // find enough of them
    struct ZeroProbe {
        MeshBuffer<unsigned long long> dev;     // [2 * ZERO_PROBE_SLOTS]
        MeshPinned<unsigned long long> host;    // {rated, left out} of the last probe
        hipEvent_t done = nullptr;
        struct Verdict { bool pending = false, known = false, dark = false; int since_probe = 0; } verdict;
    } zero;
    int last_variant = 0;                   // ASORA_VARIANT_* bits | units << 8 | threads << 16 of the last raytrace launch
    int sb_launch[ASORA_SUBBOX_LAUNCH_WORDS] = {};   // what the last sub-box call launched (asora_debug_last_subbox_launch), written where the launches are made
    // a raytrace call in progress (asora_raytrace_begin ... _range ... _fold); how the radius has behaved across launches (plan_shape)
    struct RadiusHistory { double last_R = -1.0; long same_R_calls = 0; bool has_changed = false; };
    struct Trace { bool open = false; RadiusHistory radius[2]; } rt;   // radius: [0] whole-box traces and the evolve loop, [1] the sub-box sweep (note_call_radius)
    // for the paired-sources variant on aligned tables, who shares a workgroup with whom: built once per (list, range), see
    // source_pairs_by_class
    struct PairList { const void *list; int begin, count; int2 *dev[2]; int n[2]; std::vector<int> cls[2]; };   // cls: the class of each pair
    std::vector<PairList> pair_lists;      // (a sharded or chunked trace asks for the same few ranges every iteration)
    // ... and which (group, unit) every block of such a launch sweeps (block_order, raytrace_plan.hpp): built once per (list, range,
    // launch shape), released with the pair lists
    struct OrderList { const void *list; int begin, count, units, aligned, nsrc; int2 *dev; unsigned grid; };
    std::vector<OrderList> order_lists;
    int geom_units = 0;
    ProcessBuffer<double2> logtab_dev;      // log2 table (ensure_logtab), lives until the runtime is torn down
    bool geom_valid = false;
    bool geom_on_host = false;              // the cached tables were built by the host builder (ASORA_OPT_GEOMETRY_ON_HOST)
    // table entries of cells that sit (to rounding) exactly ON the sphere: whether such a cell gets a rate is decided by
    // the reference's floating-point distance test, whose outcome depends on dr.  They are always tabulated (evaluated);
    // their RATE bit is re-decided in place when dr changes (a cosmological run: every time step) -- no rebuild.
    struct SphereCell { uint32_t *dev_word; uint32_t word_without_rate; int a, b, c; };
    std::vector<SphereCell> geom_sphere;
    MeshBuffer<unsigned long long> geom_patch_dev;   // staging for the patch kernel: {address, value} pairs
    int geom_N = 0, geom_S = 0, geom_max_cells = 0, geom_threads = 0;
    // sub-box tables (subbox_tables_prepare): traversal range instead of the periodic window, no octahedron bound, every
    // sub-box boundary padded to whole triples of steps; step_after_shell[u][s] = first table step behind shell s of unit u
    int geom_subbox = 0, geom_ext_r = 0, geom_ext_l = 0, geom_boxsize = 0;
    std::vector<int> geom_step_after_shell[12];
    double geom_R = 0.0, geom_dr = 0.0;

    RtParams rt_params;
    bool rt_heat = false;
    // pipelined calls put consecutive source ranges on two side streams, so that the tail of one range and the
    // head of the next overlap; folds (main stream) wait for the ranges issued before them
    bool rt_pipelined = false;
    bool rt_by_planes = false;              // begun by asora_raytrace_begin_planes: ranges share one launch shape
    hipStream_t side[2] = {nullptr, nullptr};
    hipEvent_t side_done[2] = {nullptr, nullptr}, main_ready = nullptr;
    bool side_pending[2] = {false, false};
    int side_next = 0;

    // per-source bookkeeping of the sub-box raytracer (subbox.hip), sized for the largest batch so far, and, per (source, unit),
    // the trailing shell between two sub-box launches (table path)
    struct Subbox { MeshBuffer<int> active, nbox; MeshBuffer<double> loss, loss_final, trail; ProcessBuffer<int> nactive; } subbox;

    // shell scratch for traces whose shell buffers exceed LDS
    MeshBuffer<double> shell_scratch;

    // chemistry reductions
    ProcessBuffer<double> red_partial;      // per-workgroup partial sums: room for 3 red_blocks and for every tiled pass (ensure_red_capacity)
    ProcessBuffer<double> red_final;        // [3]
    ProcessPinned<double> red_host;         // [3]
    int red_blocks = 0;
    // the step budget's own buffers (asora_step_budget, step_budget.hip), allocated by the first call: per-workgroup partials
    // [ASORA_BUDGET_COUNT][red_blocks] with the twelve results behind them, and where those arrive on the host
    struct Budget { MeshBuffer<double> partial; MeshPinned<double> host; } budget;
    // the bubble-size distribution's own buffers (asora_bubble_mfp, bubble_mfp.hip), allocated by the first call for the mesh of
    // device_init: the bit mask [N^2 W], the row counts [N^2], their exclusive scan [N^2 + 1], the ray workgroups' partial moments,
    // the result words and the bin edges on the device; result words and edges on the host
    struct Bubbles {
        MeshBuffer<unsigned long long> mask, scan, result;
        MeshPinned<unsigned long long> host;
        MeshBuffer<unsigned> rows;
        MeshBuffer<double> partial, edges;
    } bubbles;
    // the connected regions' own buffers (asora_region_sizes, region_label.hip), allocated by the first call: one uint32 label and
    // one uint32 volume per cell, the result words, the 3 N plane flags of the largest region; mask, edges and the pinned area are
    // the bubble buffers above
    struct Regions { MeshBuffer<unsigned> label, volume, flags; MeshBuffer<unsigned long long> result; } regions;
    // the topology's own buffer (asora_topology, topology.hip), allocated by the first call: the bit mask of the complement [N^2 W];
    // everything else it uses is the bubble and region buffers above
    struct Topology { MeshBuffer<unsigned long long> complement; } topology;
    // the granulometry's own buffers (asora_granulometry, granulometry.hip), allocated by the first call: a third uint32 grid [N^3]
    // next to regions.label / regions.volume, the bit mask of an eroded set [N^2 W] and the result words
    struct Granulometry { MeshBuffer<unsigned> work; MeshBuffer<unsigned long long> mask, result; } granulometry;
    // the power spectrum's own buffers (asora_power_spectrum, power_spectrum.hip), allocated by the first call that needs them: the
    // complex half-space of field a [N N (N/2 + 1)] and, from the first cross call, of field b; the N roots of unity; the partial
    // sums (mean density, moments, the planes' bin sums) with the result words behind them, and where those arrive on the host.
    // ms: the stage times of the last call under ASORA_OPT_TIMING (asora_debug_power_spectrum_ms)
    struct Spectrum {
        MeshBuffer<double2> modes[2], twiddle;
        MeshBuffer<double> partial;
        MeshPinned<double> host;
        MeshBuffer<unsigned> thresholds;
        double ms[ASORA_PS_STAGES] = {0, 0, 0, 0, 0};
    } spectrum;
    // the smoothing's own buffers (asora_smooth_field, smooth_field.hip), allocated by the first call that needs them: the output
    // field [N^3] of a call without dst_grid; the filter tables w_i, w_j, w_k [N each], w_r [3 floor(N/2)^2 + 1] and the histogram's
    // edges behind them; the workgroups' partial statistics; the result words (stats, then the histogram); and the pinned area the
    // tables and edges leave the host through and the results arrive in.  The complex buffer, the roots and the forward pass's
    // partial sums are the power spectrum's.  ms: the stage times of the last call under ASORA_OPT_TIMING
    struct Smoothing {
        MeshBuffer<double> field, tables, partial, result;
        MeshPinned<double> host;
        double ms[ASORA_SMOOTH_STAGES] = {0, 0, 0, 0, 0, 0, 0, 0};
    } smoothing;
    // the redshift-space unit's own buffers (redshift_space.hip): the line-of-sight velocity [N^3] of asora_los_velocity_to_device
    // with max |v| kept on the host; the planes' partial bin sums with the moments' partials and the result words behind them; the
    // two threshold tables; the pinned area the thresholds leave through and the results arrive in.  The mapped field lies in
    // smoothing.field, the complex buffer, the roots and the mean density's partials are the power spectrum's.  ms: the stage times
    // of the last asora_power_spectrum_los call under ASORA_OPT_TIMING
    struct Redshift {
        MeshBuffer<double> velocity, partial, thresholds;
        MeshPinned<double> host;
        MeshBuffer<unsigned long long> vmax_dev;
        double vmax = 0.0;                  // dies with the velocity
        double ms[ASORA_PSLOS_STAGES] = {0, 0, 0, 0, 0, 0};
    } redshift;
    // the Lyman-alpha forest's own buffers (asora_lyman_alpha_forest, lya_forest.hip), allocated by the first call that needs them:
    // F [N^3] of a call that returns the flux to the host without writing it into a grid; the result words with the gap and PDF
    // counts behind them; the PDF's edges; the partials of the statistics' workgroups and of the line kernel's; the pinned area the
    // edges leave through and the results arrive in.  tau lies in smoothing.field (either call overwrites the other's), the
    // velocity is redshift.velocity.  ms: the stage times of the last call under ASORA_OPT_TIMING
    struct Lyman {
        MeshBuffer<double> flux, edges, stat_partial;
        MeshBuffer<unsigned long long> result, block_partial;
        MeshPinned<unsigned long long> host;
        double ms[ASORA_LYA_STAGES] = {0, 0, 0, 0};
    } lyman;
    // the bispectrum's own buffers (asora_bispectrum, bispectrum.hip), allocated by the first call that needs them: the complex
    // half-space a shell's lines are filtered into on the way back (the kept spectrum is spectrum.modes[0], read only); the shell
    // fields [n_shells][N^3]; the triangles, one packed word each; the workgroups' partial sums [n_tri][workgroups] (double-double)
    // and the folded sums [2][n_tri]; the pinned area the triangles leave through and the results arrive in.  cache: the last
    // call's sum_iii with the (N, thresholds, tri) it belongs to -- values, no device memory, so it may outlive the mesh.  ms: the
    // stage times of the last call under ASORA_OPT_TIMING
    struct Bispectrum {
        MeshBuffer<double2> work;
        MeshBuffer<double> cubes, partial, result;
        MeshBuffer<int32_t> tri;
        MeshPinned<double> host;
        struct Cache { int N = 0; std::vector<unsigned> thresholds; std::vector<int32_t> tri; std::vector<double> sum_iii; } cache;
        double ms[ASORA_BISPEC_STAGES] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    } bispectrum;
    // the light cone's own buffers (asora_lightcone_advance, lightcone.hip), allocated by the first call that needs them: per slot
    // the formed field of the previous call [N^3]; the slices of a call [n_slices][N^2], grown on demand; the weights, planes, slice
    // list and runs of a call with the moments behind them, on the device and in the pinned area they cross through; the moments'
    // partials.  kept: what a slot's field was made with -- it counts only while the slot's buffer is there, so it needs no reset
    // when the mesh goes.  ms: the stage times of the last call under ASORA_OPT_TIMING
    struct Lightcone {
        MeshBuffer<double> prev[ASORA_LC_SLOTS], stage, params, partial;
        MeshPinned<double> host;
        struct Kept { bool has = false; int kind = 0, src_grid = -1; } kept[ASORA_LC_SLOTS];
        double ms[ASORA_LC_STAGES] = {0, 0, 0, 0};
    } lightcone;
    // the halo catalogue's own buffers (asora_halo_catalogue_to_device, halo_sources.hip).  Of one catalogue call and released
    // before it returns: the uploaded catalogue, the two N^3 grids of integer sums, the row counts and their scan.  Kept until the
    // next catalogue, asora_halo_catalogue_clear or the end of the mesh: the table [3][n_cells] (cell, Q_hm, Q_lm) and, sized by
    // it, what a build writes -- the flux of every row, the counts of the chunks and their scan, the list that crosses PCIe; the
    // summary words on the device and in the pinned area.  loaded counts only while the table is there, so it needs no reset when
    // the mesh goes.  generation: how many catalogues have gone up in this process, the name of the one the device holds.
    // ms: the stage times of the last catalogue call ([0] ... [4]) and build ([5] ... [7]) under ASORA_OPT_TIMING
    struct HaloSources {
        MeshBuffer<double> cat_pos, cat_mass, cat_weight;
        MeshBuffer<unsigned long long> q_hm, q_lm, row_scan;
        MeshBuffer<unsigned> rows;
        MeshBuffer<unsigned long long> table, chunk_scan, summary;
        MeshBuffer<unsigned> chunk_count;
        MeshBuffer<double> flux_all, out_flux;
        MeshBuffer<int32_t> out_pos;
        MeshPinned<unsigned long long> host;
        struct Loaded { bool has = false, built = false; long long n_cells = 0, n_active = 0; int unit_exponent = 0; } loaded;
        long long generation = 0;
        double ms[ASORA_HALO_STAGES] = {0, 0, 0, 0, 0, 0, 0, 0};
    } halo;

    ProcessBuffer<unsigned long long> counters;  // [COUNTER_FIELDS * COUNTER_SLOTS]: gamma cells, evaluated cells, exact zeros left out, spread over the slots
    long long last_gamma_cells = 0, last_eval_cells = 0;

    // the evolve step (asora_evolve_*): which accumulator set is which, the device-side convergence bookkeeping, what the step was
    // begun with
    struct Evolve {
        struct Flags {
            bool clean[2] = {false, false}; // set known to be all zero (when nothing is enqueued)
            bool sets_known = false, open = false;   // sets_known: the line above is valid (a poll has happened since the last enqueue)
        } flags;
        int base = 0;                       // set of the first iteration of the current time step
        int folded_iter = -1;               // PHI_ION holds the rates of this iteration of the current step (0: none yet)
        ProcessBuffer<EvolveStatus> status;
        ProcessPinned<EvolveStatus> host;
        bool first = true;
        int reported = 0;                   // iterations already handed to the caller by asora_evolve_poll
        int enqueued = 0;                   // upper bound of the iterations carried out (enqueued) in this step
        double chem[6] = {0, 0, 0, 0, 0, 0}; // dt, bh00, albpow, colh0, temph0, abu_c
        int src_begin = 0, src_count = 0;
        RtParams rt;
        // multi-GPU form of the loop (asora_evolve_begin_slab): this rank runs the fused pass on the planes it owns only
        bool slab = false;
        int own_begin = 0, own_count = 0;
        bool slab_passed = false;           // the current iteration's pass has been enqueued (close comes next)
        bool folded_all = false;            // ... and this iteration's has been enqueued
        bool rates_in_outbox = false;       // asora_evolve_slab_fold_all: the passes of this step read the out-box and keep PHI_ION
        bool slab_thermal = false;          // begun with asora_evolve_begin_slab_thermal: every slab call carries the heating rates too
        bool plane_swept = false;           // the current iteration of a sharded step has had its plane-flux sweep (ahead of its first asora_evolve_slab_trace)
    } evolve;
    // temperature probe of the TEMP grid: valid for the upload and the constants in consts; clump: the clumping factor the probe
    // folded into its brech0 (the constant in mode 1, else 1)
    struct TempProbe {
        ProcessBuffer<double> dev;          // [8]: the probe's five results, [5] = asora_grid_sum's
        double values[5] = {0, 0, 0, 0, 0}; // host copy: uniform?, T, brech0, acolh0, t_ok
        bool valid = false;                 // dies with the mesh
        double consts[4] = {0, 0, 0, 0};
        double clump = 1.0;
    } temp_probe;
    // Which 64-byte lines of the rate accumulators the sources of the current step can touch at all (round 4): one byte per
    // line of 8 cells, [i][j][k >> 3] for the plain layout and, behind it, [k][j][i >> 3] for the transposed one.  The fused
    // pass neither reads nor zeroes the lines no source reaches (they are zero and stay zero): 32 of its 88 bytes per cell.
    // Valid for (source upload, source range, R); nullptr in the pass = every line is reachable.
    struct ReachMask {
        MeshBuffer<unsigned char> mask;     // both layouts, half each
        MeshBuffer<unsigned long long> count_dev;
        struct Decision {                   // dies with the mesh
            bool in_use = false;
            bool pays = false;              // enough lines out of reach for the mask to pay (counted when the mask is built)
            struct Key {                    // what `pays` (and the mask, where one was built) has been decided for
                bool valid = false;
                long src_generation = -1;
                int src_begin = 0, src_count = 0;
                double R = -1.0;
                bool operator==(const Key &o) const { return valid == o.valid && src_generation == o.src_generation && src_begin == o.src_begin && src_count == o.src_count && R == o.R; }
            } key;
        } d;
    } reach;

    // thermal mode (asora_thermal_params): TEMP_END and the heating accumulators of the device loop are allocated on first use
    struct Thermal {
        struct Mode { bool on = false; ThermalConsts consts; bool heat_clean[2] = {false, false}; } mode;   // heat_clean: pair known to be all zero
        MeshBuffer<double> heat_acc;        // two pairs like `acc`, [i][j][k] then [k][j][i] each (4 N^3 doubles)
        MeshBuffer<double> heat_outbox;     // thermal step across ranks: the heating planes to send / the summed heating (N^3 doubles,
                                            // the twin of `staging`'s role as rate out-box; allocated by the first such step)
        MeshBuffer<unsigned long long> stats_dev;   // [3]: cells at max_substeps, cells floored, most substeps
    } thermal;

    // what the raytrace and the chemistry are told about the medium, until the mesh goes:
    //  * sub-grid clumping of the recombination rate (asora_clumping): 0 off, 1 one constant, 2 per cell (ASORA_GRID_CLUMP).  The
    //    launchers of the chemistry passes apply it (chemistry.hip)
    //  * Lyman-limit-system opacity (asora_lls_opacity): the raytrace's absorber density is
    //    ndens ((1 - xh_av) + lls_b) + lls_a, formed wherever nHI is (launch_prepare_nhi*, launch_prepare_range, the emit forms of
    //    the fused pass through chem_tile_common).  Both 0: off
    //  * plane-parallel flux through faces of the box (asora_plane_flux)
    struct Medium { int clump_mode = 0; double clump_c = 1.0, lls_a = 0.0, lls_b = 0.0; PlaneFluxSet plane{}; } medium;
    bool coldens_only = false;              // asora_debug_coldens has borrowed the grey form

    hipStream_t stream = nullptr;
    struct PendingTimer { int which; hipEvent_t e0, e1; };
    std::vector<PendingTimer> pending_timers;     // recorded, not yet resolved
    std::vector<hipEvent_t> free_events;
    int opt[ASORA_OPT_COUNT] = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0};
    double k_ms[ASORA_KERNEL_SLOTS] = {0, 0, 0, 0, 0, 0, 0};
    long k_n[ASORA_KERNEL_SLOTS] = {0, 0, 0, 0, 0, 0, 0};
};

State &state();
void clear_error();

// Scoped HIP-event timer around kernel launches on the library stream.
struct KernelTimer {
    int which;
    bool on;
    hipStream_t stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    explicit KernelTimer(int w, hipStream_t s = nullptr);   // s = nullptr: the library's main stream
    ~KernelTimer();
};

// ---------------------------------------------------------------------------------------------
// Raytracing (raytrace.hip)
// ---------------------------------------------------------------------------------------------

// flag bits of a geometry-table entry (cellA.y; raytrace.hip describes the tables, geometry.hip builds them)
constexpr unsigned CELL_VALID = 1u << 30, CELL_LAST = 1u << 31, CELL_RATE = 1u << 29,
                   CELL_SPHERE = 1u << 28,            // host bookkeeping: the cell sits on the sphere, RATE depends on dr (the kernel ignores it)
                   CELL_ZERO_SHIFT = 25,              // bits 25..27: which of the offsets (a, b, c) are zero
                   CELL_NEG_SHIFT = 22,               // bits 22..24: the cell lies on the mirrored side of axis 0 / 1 / 2 (axes the unit merges)
                   CELL_SLOT_MASK = (1u << 22) - 1;

// What one geometry table holds (geometry.hip: UnitSpec + the alignment class): a dependency-closed part of the sphere
struct GeomTableSpec {
    int face = -1;            // -1: whole octant(s); 0 / 1 / 2: the x- / y- / z-sector
    int merge_mask = 0;       // bit ax: the unit covers BOTH signs of axis ax
    int ext[3] = {0, 0, 0};   // periodic-window extent of each axis on the side the unit looks at
    int ext_neg = 0;          // extent on the mirrored side of a merged axis
    int wedge = -1;           // 0..3: a quarter of the sector, -1: the whole unit
    int align_class = -1;     // 0..7: line-aligned form for sources at this position modulo 8; -1: densely packed
};
// geometry_device.hip: the DISTINCT tables of a launch shape built on the GPU (bit-identical to geometry.hip's host builder)
int build_geometry_on_device(State &st, const std::vector<GeomTableSpec> &specs, double R, double dr, int q_max, int threads,
                             int boxsize, std::vector<OctGeomDev> &out, std::vector<std::vector<int>> &step_after, int &S_all,
                             uint32_t &max_cells_all);
struct SubboxGeometry { int ext_r, ext_l, boxsize; };     // sub-box tables: the traversal range of raytracing.f90:174-175, the box size
// Build (or reuse) the geometry tables for (N, R, dr, threads, units): geometry.hip
int ensure_geometry(State &st, RtParams &p, int threads, int units, const SubboxGeometry *sbg = nullptr, bool aligned = false);
void release_geometry(State &st);
bool note_call_radius(State &st, double R, int path);   // once per API call: may the eight-fold aligned tables be built for this radius?
void release_pair_lists(State &st);     // with every change of the source lists
int launch_fold_range(State &st, const double *src_t, double *dst, int i_begin, int i_count);   // dst[i][j][k] += src_t[k][j][i], i in the range
int ensure_logtab(State &st);
int launch_prepare_nhi(State &st, bool need_transposed);
int launch_finish_phi(State &st);
// open boundaries: what they are not built for (N > 512, grey opacity, global atomics, the column-density dump), code 4
int check_open_boundaries(const State &st, const char *who, bool open, bool dump);
// plane_flux.hip: what a trace with faces set is not built for (grey opacity, the dump, heating without its tables, a table set
// the device does not hold, a z face without the twins), code 4; the sweeps of p.plane into phi (+ heat_acc), [i][j][k] then
// [k][j][i] each, on the library's stream (nothing without faces)
int check_plane_flux(const State &st, const PlaneFluxSet &pf, const char *who, bool dump, bool heat);
int launch_plane_flux(State &st, const RtParams &p, double *phi, double *heat_acc, bool heat, const int *done);
int launch_raytrace(State &st, RtParams &p, bool dump, bool heat, hipStream_t side = nullptr);   // side: stream to launch on when no shared scratch is needed
void plan_options(const State &st, RtPlanInput &in);    // cu_count and the options a launch plan reads (raytrace_plan.hpp)
// which rows of RT_FORMS have been launched, process-wide (raytrace.hip; asora_debug_form_launches, asora_debug_last_launch_form)
const unsigned long long *form_launch_counts();         // RT_FORM_COUNT counters
void reset_form_launch_counts();
int last_launched_row();                                // -1 before the first launch
// The sub-box sweep on tabulated geometry (raytrace.hip): prepare -> tables for (N, R, range, box size), then one launch per
// sub-box.  `shells` = (s_begin, s_end] of the box; returns without launching when the tables hold nothing there.
struct SubboxTables { int units = 0, threads = 0, S = 0, max_batch = 0, nsrc = 1; bool ok = false, aligned = false; const int32_t *host_pos = nullptr; };   // max_batch: sources per launch the trailing-shell scratch holds; nsrc: sources per workgroup (2: paired sweep); host_pos: the source positions on the host (0-based, xyz-interleaved; pairing for the aligned tables) or nullptr
int subbox_tables_prepare(State &st, RtParams &p, int ext_r, int ext_l, int subboxsize, int src_count, bool heat, SubboxTables &out,
                          const int32_t *host_pos);
int subbox_tables_sweep(State &st, const RtParams &p, const SubboxTables &tab, int s_begin, int s_end, bool heat);
int launch_fold_transposed(State &st, const double *src_t, double *dst);   // dst[i][j][k] += src_t[k][j][i]
int launch_fold_sum(State &st, const double *a, const double *b_t, double *dst);   // dst[i][j][k] = a[i][j][k] + b_t[k][j][i]
int launch_transpose(State &st, const double *src, double *dst, int N);   // dst[k][j][i] = src[i][j][k]

// ---------------------------------------------------------------------------------------------
// Raytracing with the reference's CPU semantics: cubic sub-boxes, photon loss (subbox.hip)
// ---------------------------------------------------------------------------------------------
struct SubboxParams {
    int N, W;                   // mesh size; row pitch of the shell-buffer slot layout (largest shell + 1)
    int ext_r, ext_l;           // traversal range on the + / - side of every axis (raytracing.f90:174-175)
    int s_begin, s_end;         // this launch sweeps the Chebyshev shells (s_begin, s_end]
    int edge_r, edge_l;         // faces of the current sub-box: last_r - src, src - last_l (f90:199-200)
    double sig, dr, R;          // R = R_max_LLS in cells
    double numtau_f, lut_k1, lut_k0;
    int table_len;
    int grey, heat, add_zero;   // add_zero = 0: ASORA_OPT_SKIP_ZERO_RATES
    int src_begin, src_count;   // batch of sources
    int flux_src;               // >= 0: every source shines with the flux of this one (f90:500,503); -1: its own
    int dump_src;               // source whose column densities are returned (the last one), or -1
    unsigned ncell;
    const double *nhi;          // [i][j][k] then [k][j][i]
    double *phi, *heat_grid;    // same layout
    double *dump;               // [i][j][k]
    const double2 *tables, *logtab;
    const int32_t *src_pos;
    const double *src_flux;
    double *scratch;            // per workgroup: two shell buffers of 3 W^2 doubles
    size_t unit_stride;         // = 6 W^2
    const int *active;          // per source of the batch
    double *loss;               // per source of the batch: photons through the current box faces
    double lut_kc;              // the table index's correction term (lut_index_constants)
};
int launch_subbox_sweep(State &st, const SubboxParams &p, hipStream_t side = nullptr);   // side: the stream to launch on (default: the library's)
int launch_subbox_decide(State &st, int mode, int count, const double *src_flux, int src_begin, double loss_fraction,
                         int more_range, int *active, double *loss, double *loss_final, int *nbox, int *n_active);

// ---------------------------------------------------------------------------------------------
// Chemistry (chemistry.hip)
// ---------------------------------------------------------------------------------------------
struct ChemParams {
    size_t ncell;
    double dt, bh00, albpow, colh0, temph0, abu_c;
    const double *ndens, *temp, *xh, *phi;
    double *xh_av, *xh_intermed;
    double *red_partial, *red_final;
    int red_blocks;
    int accumulate = 0;        // 1: add this launch's reductions to red_final (slab-wise passes) instead of replacing it
    // thermal form (launch_chemistry with `thermal`): heating rate per HI atom in, end-of-step temperature out
    bool thermal = false;
    const double *phi_heat = nullptr;
    double *temp_end = nullptr;
    unsigned long long *th_stats = nullptr;
    ThermalConsts th;
    // clumping (set by launch_chemistry from State::medium.clump_mode; appended, so the fields above keep their offsets): the per-cell
    // factors, or nullptr with the one factor clump_c (thermal form only: the isothermal constant scales bh00 instead)
    const double *clump = nullptr;
    double clump_c = 1.0;
};
// clumped = false: State::medium.clump_mode is not applied (c2ray_global_pass, the reference's f2py boundary, has no clumping argument)
int launch_chemistry(State &st, ChemParams &p, hipStream_t stream, bool clumped = true);
int chemistry_reduction_blocks(const State &st);

// The same pass over the planes [i_begin, i_end) of the N^3 grids, tiled so that the [k][j][i] twins can be read and
// written with contiguous rows as well (chemistry.hip: chemistry_tile_kernel).
//   fold   : the rate of a cell is gamma[i][j][k] + gamma_t[k][j][i] (the raytrace's two accumulators), written to phi_out
//   emit   : additionally form nHI = ndens (1 - xh_av) of the NEW xh_av in both layouts for the next raytrace and
//            zero both accumulators -- everything the host did between two iterations (pyc2ray/evolve.py:200-240)
//   status : evaluate the convergence test on the device behind the reductions; launches do nothing once it has passed
struct ChemTileParams {
    int N = 0, i_begin = 0, i_end = 0;
    double dt = 0, bh00 = 0, albpow = 0, colh0 = 0, temph0 = 0, abu_c = 0;
    const double *ndens = nullptr, *temp = nullptr, *xh = nullptr, *xh_av_in = nullptr;
    double *gamma = nullptr, *gamma_t = nullptr;     // rates [i][j][k] (+ [k][j][i] accumulator when fold)
    double *phi_out = nullptr;                       // fold: folded rates go here as well (nullptr: nowhere)
    double *zero_a = nullptr, *zero_t = nullptr;     // emit: the accumulator pair to zero for the next raytrace
    double *xh_av = nullptr, *xh_intermed = nullptr;
    double *nhi = nullptr, *nhi_t = nullptr;         // emit
    double *red_partial = nullptr, *red_final = nullptr;
    int red_stride = 0;                              // number of workgroups of the launch (set by the launcher)
    int accumulate = 0;
    EvolveStatus *status = nullptr;
    bool local_sums = false;                         // status only gates the launch: the reductions stop at red_final, the convergence
                                                     // test follows later, on the sums over all ranks (launch_convergence_test)
    const unsigned char *reach_a = nullptr, *reach_t = nullptr;   // fold + emit: lines of the accumulators any source reaches (State::reach), or nullptr
    bool fold = false, emit = false;
    // the grid has one temperature (launch_temp_probe): its factors, evaluated on the device, travel with the parameters
    int uniform = 0, uniform_t_ok = 0;
    double uniform_T = 0, uniform_brech0 = 0, uniform_acolh0 = 0;
    // thermal form (emit only): the heating accumulators are folded like the rates, the other heating pair zeroed
    bool thermal = false;
    double *heat = nullptr, *heat_t = nullptr;
    double *zero_ha = nullptr, *zero_ht = nullptr;
    double *temp_end = nullptr;
    unsigned long long *th_stats = nullptr;
    ThermalConsts th;
    // clumping: set by launch_chemistry_tiles from State::medium.clump_mode, as ChemParams::clump / clump_c
    const double *clump = nullptr;
    double clump_c = 1.0;
    // thermal form without fold (heating already summed over both layouts and over the ranks: the all-reduce loop): where the pass
    // keeps it, as phi_out keeps the rates (appended, so the fields above keep their offsets)
    double *heat_out = nullptr;
    // emit: the Lyman-limit absorbers in the next trace's nHI (State::medium.lls_a / lls_b, set by chem_tile_common)
    double lls_a = 0.0, lls_b = 0.0;
};
int launch_grid_sum(State &st, const double *a, size_t n, double *out_dev);
int launch_scale(State &st, double *a, size_t n, double factor);
int launch_temp_probe(State &st, const double *temp, size_t n, double bh00, double albpow, double colh0, double temph0,
                      double *out_dev);
int launch_chemistry_tiles(State &st, ChemTileParams &p, hipStream_t stream);
size_t chemistry_tile_blocks(const State &st, int N, int planes);
int launch_prepare_nhi_from(State &st, const double *xh_av, bool need_transposed);
int launch_prepare_range(State &st, int i_begin, int i_count, bool zero_acc, double *acc, const int *done = nullptr);
// multi-GPU device loop: foreign planes folded into the out-box (+ the other accumulator pair zeroed there); received planes added
int launch_fold_out(State &st, const double *a, const double *a_t, double *out, double *z_a, double *z_t, int i_begin, int i_count,
                    const int *done);
// the same for the rates and the heating rates of a thermal step in ONE launch (h, h_t -> hout; zh_a, zh_t zeroed)
int launch_fold_out_pair(State &st, const double *a, const double *a_t, double *out, double *z_a, double *z_t, const double *h,
                         const double *h_t, double *hout, double *zh_a, double *zh_t, int i_begin, int i_count, const int *done);
int launch_add_planes(State &st, double *dst, const double *src, size_t n, const int *done);
// the convergence test of evolve.py:216-236 on sums[3] = {sum x, sum 1-x, conv_flag} (summed over the ranks beforehand)
int launch_convergence_test(State &st, const double *sums, EvolveStatus *status);
// mask[0 .. N*N*NL) for [i][j][k >> 3], mask[N*N*NL .. ) for [k][j][i >> 3], NL = (N + 7) / 8: 1 where a source of the range reaches
int launch_reach_mask(State &st, const int32_t *src_pos, int src_begin, int src_count, double R, unsigned char *mask, size_t bytes_one_layout);
int launch_reach_count(State &st, const unsigned char *mask, size_t bytes_both_layouts, unsigned long long *out_dev);

// ---------------------------------------------------------------------------------------------
// Host API layer (api.hip and the *_api.hip units): what more than one of them needs
// ---------------------------------------------------------------------------------------------
// api.hip
int ensure_runtime();                           // stream, events, reduction buffers: needed with or without device_init
int require_init(const char *who);
int check_N(const char *who, int N);
// fail(code, who + ": " + tail) unless the planes lie in the mesh / the sources among the uploaded ones
int check_planes(const char *who, int code, const char *tail, int i_begin, int i_count);
int check_sources(const char *who, int code, const std::string &tail, int src_begin, int src_count);
int require_grids(const char *who, std::initializer_list<int> grids);     // code 4 unless every one of them holds data
// grids_api.hip
int ensure_optional_grid(int which);            // PHI_HEAT, TEMP_END, CLUMP: allocated on first use; any other grid: nothing to do
// raytrace_api.hip
int reset_counters();
int require_raytrace_inputs(const char *who, double R, int NumTau, bool density, bool xh_av);
void fill_rt_params(RtParams &p, double R, double sig, double dr, double minlogtau, double dlogtau, int NumTau, int radius_path = 0);
// the source list a trace works from: as uploaded, or its position-ordered copy -- positions, fluxes and table sets together
inline void use_source_list(RtParams &p, const State &st, bool sorted)
{
    p.src_pos = sorted ? st.sources.pos_sorted : st.sources.pos;
    p.src_flux = sorted ? st.sources.flux_sorted : st.sources.flux;
    p.src_spec = sorted ? st.sources.spec_sorted : st.sources.spec;
}
// code 4 while a source has a table set the device does not hold, or a set other than 0 under grey opacity (no tables)
int check_source_spectra(const char *who);
// grids_api.hip: order[s] = index of the s-th source in lexicographic order of the position (stable)
void sort_sources_by_position(const int32_t *pos, int NumSrc, std::vector<int> &order);
// chemistry_api.hip
int ensure_red_capacity(size_t entries);
int ensure_temp_probe(double bh00, double albpow, double colh0, double temph0);
ChemTileParams chem_tile_common(int i_begin, int i_count, const double chem[6]);
// bubble_mfp.hip: what asora_region_sizes (region_label.hip) shares with asora_bubble_mfp -- the argument checks of a thresholded
// grid (codes 3 and 4), the feature's buffers, the threshold pass (and, with `scan`, the scan of the row counts)
constexpr int BUBBLE_HOST_WORDS = 1024;         // uint64 words of State::bubbles.host (pinned): a call's result words, its edges behind them
int check_bubble_grid(const char *who, int which, double threshold, int phase);
int ensure_bubble_buffers(State &st);
int launch_bubble_mask(State &st, int which, double threshold, int phase, bool scan);
// region_label.hip: what asora_topology (topology.hip) shares with asora_region_sizes -- the labelling's buffers, and the launches
// that label the in-phase cells of a bit mask of the mesh (`mask`: the layout of State::bubbles.mask, pad bits 0): afterwards
// region_label holds every in-phase cell's root (the smallest index of its region; 0xFFFFFFFF out of phase) and region_volume every
// root's volume (0 elsewhere)
int ensure_region_buffers(State &st);
int launch_region_label(State &st, const unsigned long long *mask, int periodic, int connectivity);
// power_spectrum.hip: what asora_smooth_field (smooth_field.hip) shares with asora_power_spectrum -- which grids a kind reads, and
// the forward transform of one field into State::spectrum.modes[0] (the mean density, the pass along k with the moments, along j, along i)
bool ps_needs_grid(int kind, int grid, double t_gamma);
int ps_forward(State &st, int kind, double scale, double t_gamma, const std::function<int()> &stage_done, const double **moments_dev);
// the same stage by stage, for redshift_space.hip: the mean density alone, and the three passes with `x` read as the ionised fraction
int ps_mean_density(State &st, const double **nbar_dev);
int ps_transform(State &st, int kind, const double *x, bool nbar, double scale, double t_gamma, double *field,
                 const std::function<int()> &stage_done, const double **moments_dev);
// the binning of asora_power_spectrum's auto-spectrum for what lies in State::spectrum.modes[0] (bispectrum.hip): the same two launches,
// so count, sum_k and sum_aa are its bits; *count_dev, *sum_k_dev, *sum_aa_dev: where the n_bins values of each lie on the device
int ps_bin_auto(State &st, int n_bins, const unsigned *thresholds, const unsigned long long **count_dev, const double **sum_k_dev,
                const double **sum_aa_dev);

} // namespace asora
