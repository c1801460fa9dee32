// raytrace.hip -- short-characteristics raytracing for gfx950 (MI355X).
//
// What is computed is exactly what the reference's GPU path computes
// (src/asora/raytracing.cu:79-339: do_all_sources_gpu + evolve0D_gpu + cinterp_gpu, and
//  src/asora/rates.cu:16-83): for every source, the incoming/outgoing HI column density of
// every cell by short-characteristics interpolation and the photon-conserving rate Gamma,
// summed over sources into phi_ion.
//
// How it is computed is different:
//   * work item = (source, unit), unit = octant, octant sector or pair of mirrored sectors (pick_launch_shape).
//     The 8 sign-octants of a source only share the three
//     coordinate planes through the source, and a cell on such a plane depends only on cells
//     of the same plane (the "upstream" neighbour across a zero offset has bilinear weight
//     exactly 0, cinterp_gpu raytracing.cu:378-408 with sign(0)=+1), so each octant re-derives
//     its boundary planes and is otherwise independent: 8*NumSrc independent workgroups, no
//     inter-workgroup communication.
//   * inside an octant the sweep runs over CHEBYSHEV shells s = max(|di|,|dj|,|dk|) instead of
//     the reference's octahedral shells q = |di|+|dj|+|dk|.  The interpolation of a cell whose
//     dominant offset is s reads only cells whose dominant offset is s-1, so ONE trailing shell
//     is live (the octahedral order keeps three) and there are R+1 instead of ~sqrt(3)R+1
//     barriers.  Both orders are valid topological orders of the same dependency graph, so the
//     values are the same.
//   * the live shell is double-buffered in LDS; the reference's NUM_SRC_PAR x N^3 global scratch
//     (memory.cu:65) does not exist.
//   * only cells that can receive a rate are evaluated: |d|^2 <= R^2, inside the periodic window
//     and inside the reference's octahedron q <= q_max.  Every upstream neighbour of such a cell
//     is strictly closer to the source, so the pruned cells never feed a kept one and phi_ion is
//     unchanged (the reference evaluates them into scratch and then discards them,
//     raytracing.cu:311-315).
//   * what does not depend on the source or on the medium -- which cells a shell holds, their
//     path length and the shell-buffer slots of their four upstream corners -- is the same for
//     all sources.  It is tabulated ONCE per (N, R) on the host (build_unit_geometry in geometry.hip,
//     32 B per cell) and streamed from L2 by every workgroup, two steps ahead of its use.
//   * faces dj=s and di=s are rows along k, contiguous in the [i][j][k] grid.  Faces dk=s are
//     rows along i, so they read nHI and accumulate Gamma through [k][j][i] transposed copies
//     (rows contiguous again); the transposed accumulator is folded back once per call.
//   * nHI = ndens*(1-xh_av) is formed once per call (raytracing.cu:275-276 forms it per visit).
#include "asora_internal.hpp"
#include "rates_device.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <thread>
#include <utility>
#include <vector>

namespace asora {

// (the rates of a cell -- rate_issue / rate_value, grey_rate_per_atom, heat_rate_per_atom, photo_rate_per_atom -- live in
//  rates_device.hpp, where rate_primitives_debug.hip can call them too)

// ---------------------------------------------------------------------------------------------
// The octant kernel
// ---------------------------------------------------------------------------------------------
// Per-octant cell tables (built by build_unit_geometry, geometry.hip): a flat sequence of "steps" of RT_THREADS
// entries; the cells of a shell fill whole steps (the last one padded with invalid entries), so
// entry k*RT_THREADS + lane is what `lane` does in step k and the tables can be prefetched blindly.
//   cellA[e] = { abc, own slot | VALID | LAST_OF_SHELL, path (double, 2 words) }
//   cellB[e] = { slots of the four upstream corners in the previous shell's buffer }
// Dynamic LDS: [log table: LOG_TABLE_SIZE x {2/c, log2 c - 1}][1/s: TABCAP doubles][wrapped i(a), j(b), k(c), mirrored: 4*TABCAP ints]
//              [shell buffer 0: max_cells+1 doubles][shell buffer 1: same]   (the last two unless GLOBAL_SCRATCH)
// TABCAP = 64 (S <= 63, workgroups of 64 or 128 threads: small traces, where LDS decides how many workgroups a CU
// holds), 256 (S <= 255) or 1024.
// Slot max_cells of each shell buffer holds 0.0: upstream corners of weight 0 point there.

// buffer_atomic_add_f64 through a raw buffer descriptor: a lane whose offset lies beyond the descriptor's range is dropped
// by the hardware, so "this lane has nothing to add" is an offset of -1 and the instruction needs no branch around it
// (clang has no builtin for the f64 form; this binds the LLVM intrinsic).
// The offset of such a lane is 2 GiB, and the descriptors never span more than 2 GiB: the range check is
// offset + 8 > num_records in 32-bit arithmetic, so an offset near 2^32 would wrap around and pass it.
#define ASORA_OOB_OFFSET ((int)0x80000000u)
// OPEN kernels: mark of a wrapped-coordinate entry (and of the cell index made of three) whose unwrapped position is outside the box
constexpr unsigned WTAB_OUTSIDE = 0x80000000u;
extern "C" __device__ double asora_buffer_atomic_fadd_f64(double, __amdgpu_buffer_rsrc_t, int, int, int)
    __asm("llvm.amdgcn.raw.ptr.buffer.atomic.fadd.f64");

// Choices of the step loop, each measured on MI355X (LABNOTES; 1000 sources, 256^3 unless stated):
// - The table lookups of a step are CONSUMED in the next step (their rate is formed there, right before that step's own
//   lookups are issued, and added behind them): a whole step of arithmetic hides their latency.  Pays where the kernel is
//   latency-bound; costs 14 VGPRs (the kernel as a whole needs 96 with buffer atomics).  Round 2: R = 16 -1.0 %, 24 -3.5 %,
//   32 -1.9 %, 48 -1.7 %, 64 -1.7 %.
// - The rate atomic of a step is thereby issued in the NEXT step, right behind that step's table-lookup loads.  Vector
//   memory operations complete in issue order, so a lookup issued after an atomic cannot return before the atomic has
//   gone through the memory-side atomic unit (thousands of cycles under load); issued the other way round the lookup
//   only waits for the atomic of the step before.
// - Within a group of 8 sources the units are dispatched largest first (the z-sector units hold the most cells), so that
//   the workgroups still running when the grid drains are the short ones.  Round 2: R = 24 -2.6 %, 32 -1.8 %, 48 -1.7 %,
//   64 -0.5 %.
// - A wave whose 64 table entries of a step are all padding skips the interpolation only and issues the (unused) lookups
//   like every other wave.  Skipping the lookups as well makes the number of vector-memory operations in flight differ
//   between the two paths, and where they meet the compiler waits as the shorter one demands (three operations too early
//   on every wait of every step).
// - A scheduling barrier between the unrolled steps.  Without it the compiler hoists the decoding of a table entry (the
//   address of the NEXT step's nHI) into the step that loaded the entry, i.e. waits for a load issued 250 instructions ago
//   with two newer ones in flight instead of a whole step later.
// - The two divisions of a cell (interpolation, flux / volume) go through div_newton (rates_device.hpp) instead of the IEEE
//   sequence.  Pays since the work counters stopped serialising the launch and the kernel runs at ~80 % of VALU issue.
// - No minimum of waves per SIMD in __launch_bounds__ (1; workgroups of up to 512 threads).  Left alone the kernel takes
//   100 VGPRs (4 waves per SIMD); asked for 5 it fits 96 with three dwords spilled outside the loop, and is slower (R = 16
//   +5 %, R = 32 +2 %: profiles/r02_ab_work_counters.txt).  The paired-sources variant (NSRC = 2) left alone takes 134
//   VGPRs (3 waves per SIMD).

// (round 6: the thick and thin rate table in LDS -- NumTau <= 2048, 2 x 16 KB, lookups as ds_read2_b64 gathers -- was measured on
//  twelve sector pairs with two workgroups per CU and is 11-14 % SLOWER than the global-memory lookups on the quiet medium and on an
//  evolving field alike: the LDS pipe is already a third to a half busy with corner reads, the logarithm table and the wrapped
//  coordinates, and 8 more divergent 16-byte gathers per wave-step tip it over.  LABNOTES round 6, profiles/r06_ab_lds_tables.txt)
// (round 4: non-temporal loads for the table-entry and nHI streams were measured and are slower -- the workgroups of a CU and of an
//  XCD share those lines through the L1 and L2: LABNOTES.md)
// (the flag bits of a table entry, CELL_*: asora_internal.hpp)

// GREY (ASORA_OPT_GREY_NOTABLES) is a compile-time variant although its branch is wave-uniform: the compiler counts the
// vector-memory operations in flight per PATH and, where paths of different counts meet, waits as the shortest one
// demands -- with the grey branch (one atomic, no lookups) in the loop every wait of the table path was three operations
// too early, i.e. the lookups had to be back at the top of the next step.
// BUFATOM: the rate atomics go through buffer descriptors over [phi | phi_t] and [heat | heat_t] (possible while the
// pair of grids stays within 2 GiB, N <= 512): the atomic of a step is then ONE unconditional instruction -- with
// `if (lane has a rate) atomic` the compiler sees a path without the atomic and counts one operation too few in flight
// behind every earlier load, i.e. every wait for a lookup also waited for the atomic issued after it.
// NSRC = 2: one workgroup sweeps its unit for TWO sources at once (consecutive entries of the source list, which a whole-list
// call has ordered by position: neighbours).  Everything a step derives from the table entry alone -- offsets, face, shell,
// bilinear weights and their products, path, volume factor, owner bits, the shell barrier -- is then evaluated once per
// lane-step instead of once per source (~45 of ~230 VALU instructions), the tables are streamed once, and a wave carries
// two independent dependency chains (LDS reads -> interpolation -> LDS write) that interleave.  What stays per source:
// the shell buffers and wrapped-coordinate tables in LDS, nHI, the interpolation, the lookups and the atomic.  An odd
// source count leaves the last workgroup with a copy of its first source whose rates are dropped (`have`).
// SUBBOX: the semantics of the reference's CPU function (src/c2ray/raytracing.f90:52-567, see subbox.hip) on this kernel's
// machinery.  A launch sweeps ONE sub-box = a range of shells = the table steps [sb_k0, sb_k1) of its unit, for the sources
// that are still growing; it starts from the trailing shell the previous sub-box's launch left in global memory and leaves
// its own there; cells on the faces of the box add what passes through them (phi_out, photorates.f90:120-125) to the
// source's photon loss; every source is rated with the flux of `flux_src` (f90:500,503).  Fortran-flavoured constants.
//
// Which combinations exist: the rows of RT_FORMS (raytrace_plan.hpp, make_form_table), which is the source -- launch_form_row below
// instantiates exactly its rows, 152 of the 13 template parameters, and the static_asserts below check every one.  In summary
// (SPLIT, SPEC and OPEN are f, t, f unless the family says otherwise; DESIGN.md 4.1 has the launch shapes that select them):
//   family                         THREADS x TABCAP                               GS   DUMP HEAT SKIP_ZERO GREY BUFATOM NSRC SUBBOX   forms
//   paired production              {64,128,256,512}x256 {64,128,256}x64 256x32     f    f    f    f/t       f    t       2    f        16
//   single source, buffer atomics  {64..1024}x256 {64,128}x64                      f    f    f/t  f/t       f/t  t       1    f        28
//   single source, global atomics  same, and {256,512,1024}x1024 with GS=t (N > 512, option, shells in global memory) f/t  f    f/t  f (t: GS=f) f/t f       1    f        58
//   column-density dump            256 x {256, 1024 with GS=t}                     f/t  t    f    f         f/t  f       1    f        6
//   sub-box sweep                  {256,512} x 256                                 f    f    f/t  f         f    t       1|2  t        6
//   descriptors per layout (SPLIT) paired {256x32, 256x64, 256x256, 512x256}, SPEC f/t; single {256,512}x256   f    f    f/t  f/t       f/t  t       1|2  f        16 + 8
//   open boundaries (OPEN)         paired {256,512}x256; single {256,512}x{256, 1024 with GS=t} f/t(1) f    f/t(1) f       f    t       1|2  f        14
//   (the 1024-entry tables -- more than 256 shells -- only with the shells in global memory: raytrace_plan.hpp, at RT_FORM_COUNT)
//   (SKIP_ZERO with HEAT or GREY, NSRC = 2 with HEAT, DUMP, GREY or global atomics, SUBBOX with NSRC = 2 and HEAT: not built)
// OPEN (ASORA_OPT_OPEN_BOUNDARIES): a cell whose unwrapped position i0 +- a, j0 +- b, k0 +- c lies outside [0, N)
// on any axis is swept like every other -- its upstream neighbours and whatever reads it lie outside as well, since every
// upstream neighbour of an in-box cell lies in the bounding box of that cell and the source -- but receives no rate and is not
// counted (in_box_gpu of the reference's build without PERIODIC, raytracing.cu:264-267).  The per-source wrapped-coordinate
// tables carry the verdict per axis and offset in their top bit, nhi_address hands the OR of the three on in the top bit of the
// cell index, and the lane's pending atomic gets the out-of-range offset of a lane without a rate.  A compile-time variant: with
// OPEN = false every instantiation is what it was (register counts line for line); the last row of the table is all that is
// built with it -- 14 forms -- and plan_shape maps every launch shape onto them (64 ... 256 threads -> 256, 512 and 1024
// -> 512; 256-entry LDS tables unless there are more than 256 shells; no exact-zero skipping); N > 512, grey opacity, global
// atomics, the column-density dump and the sub-box sweep are refused (check_open_boundaries).  138 VGPRs paired (three waves
// per SIMD against four), 100 single (four against five), 108 with heating.
// SPEC: the kernel reads the table set of its source(s) (RtParams::src_spec; a scalar load and a scalar multiply-add per source).
// Every form is built with it, at no VGPR; only the paired SPLIT family tips from 128 to 129 VGPRs (four waves per SIMD to three),
// so that family alone is ALSO built without (SPEC = false) and launches without table sets take that form: plan_launch.
// split descriptors: does this unit's face write the [k][j][i] twin?  (the z-sector with the twins in use)
__device__ __forceinline__ bool ztr_desc(const RtParams &p, int uinfo) { return p.z_transposed != 0 && ((uinfo >> 8) & 3) == 3; }

template <int RT_THREADS, bool GLOBAL_SCRATCH, bool DUMP, bool HEAT, int TABCAP, bool SKIP_ZERO = false, bool GREY = false,
          bool BUFATOM = false, int NSRC = 1, bool SUBBOX = false, bool SPLIT = false, bool SPEC = true, bool OPEN = false>
__global__ void __launch_bounds__(RT_THREADS, 1) raytrace_octant_kernel(const RtParams p)
{
    extern __shared__ double lds_raw[];
    static_assert(NSRC == 1 || (!GLOBAL_SCRATCH && !DUMP && BUFATOM), "paired sources: production variant only");
    static_assert(!SUBBOX || (!GLOBAL_SCRATCH && !DUMP && !SKIP_ZERO && !GREY), "sub-box sweep: table rates, shells in LDS");
    static_assert(SPEC || (SPLIT && NSRC == 2), "the form without per-source table sets is kept for the paired SPLIT family only");
    static_assert(!SPLIT || (BUFATOM && !SUBBOX && !DUMP && (NSRC == 1 || (!HEAT && !GREY)) && !(SKIP_ZERO && (HEAT || GREY))),
                  "descriptors per layout: the production forms for 512 < N <= 645, and the single-source form with heating or grey opacity");
    static_assert(!OPEN || (BUFATOM && !DUMP && !SKIP_ZERO && !GREY && !SUBBOX && !SPLIT && SPEC && (NSRC == 1 || !HEAT)),
                  "open boundaries: table rates through buffer atomics over one descriptor (N <= 512), see the variant table");

    if (p.done_flag && *p.done_flag) return;   // evolve loop: an iteration enqueued beyond convergence does nothing
    const int blk = blockIdx.x;
    // blocks b and b+8 share an XCD (round-robin dispatch): keep the 8 octants of one source
    // on one XCD so that they share its L2 lines of nHI.  Speed only, never correctness.
    // p.units workgroups per source (8, 24, 12, 96 or 4: see ensure_geometry).
    // p.spread (a handful of sources): consecutive blocks are the units of ONE source, i.e. they go to different XCDs --
    // with the grouping above a single source would keep all its workgroups on one XCD's 32 CUs.
    int src_local, unit;      // src_local: index of the group of NSRC sources this workgroup sweeps
    // p.order (whole-list and sub-range traces that are not spread): the host has dealt the workgroups table-major per XCD
    // (block_order, raytrace_plan.hpp) -- the workgroups resident on an XCD then stream one or two geometry tables, which stay in
    // its L2, instead of one table each.  One scalar load; padding at the lanes' ends does nothing.
    if (p.order) {
        const int2 e = p.order[blk];
        if (e.x < 0) return;
        src_local = e.x;
        unit = e.y;
    } else {
        if (p.spread) {
            src_local = blk / p.units;
            unit = blk % p.units;
        } else {
            src_local = (blk & 7) + 8 * (blk / (8 * p.units));
            unit = (blk >> 3) % p.units;
        }
        unit = p.units - 1 - unit;   // sector units: z (most cells) first, x (fewest) last in dispatch order
    }
    const int uinfo = p.geom[unit].info;           // sign bits of the unit | merged axes << 3 | rates-source << 6 | (face + 1) << 8
    // p.aligned: the unit's tables come in eight forms, by the source's position modulo 8 along the memory-contiguous axis of
    // the unit's face; the two sources of a workgroup agree in it (the host paired them so: p.pairs)
    const bool by_class = p.aligned != 0;
    const int face_type = ((uinfo >> 8) & 3) == 3 ? 1 : 0;          // 1: z-sector (rows along i), 0: x- / y-sector (rows along k)
    const bool listed = by_class && NSRC == 2;
    if (listed ? src_local >= p.npairs[face_type] : src_local * NSRC >= p.src_count) return;

    const int N = p.N;
    int i0[NSRC], j0[NSRC], k0[NSRC];
    int loc[NSRC];            // SUBBOX: the source's index within the batch (activity, photon loss, trailing shell)
    double flux[NSRC];
    // the rate tables of each source: its table set's block (asora_spectra_to_device).  Workgroup-uniform like the source itself:
    // a scalar offset on a kernel argument, read where the position and the flux are read, by the same index
    const double2 *tab[NSRC];
    bool have[NSRC];
    unsigned nreal = 0;
    int2 listed_pair = {0, -1};
    if (listed) listed_pair = p.pairs[face_type][src_local];
#pragma unroll
    for (int q = 0; q < NSRC; ++q) {
        int ns;
        if (listed) {
            have[q] = q == 0 || listed_pair.y >= 0;
            ns = (q == 0 || listed_pair.y < 0) ? listed_pair.x : listed_pair.y;
        } else {
            have[q] = src_local * NSRC + q < p.src_count;
            ns = p.src_begin + (have[q] ? src_local * NSRC + q : src_local * NSRC);
        }
        loc[q] = ns - p.src_begin;
        // SUBBOX: a source that stopped growing after an earlier box is swept along with its partner, its rates and its
        // photon loss dropped like those of the copy that fills an odd count; a workgroup without a live source ends here
        if (SUBBOX) have[q] = have[q] && p.sb_active[loc[q]] != 0;
        i0[q] = p.src_pos[3 * ns + 0];
        j0[q] = p.src_pos[3 * ns + 1];
        k0[q] = p.src_pos[3 * ns + 2];
        flux[q] = p.src_flux[(SUBBOX && p.flux_src >= 0) ? p.flux_src : ns];
        tab[q] = p.tables;
        if (SPEC && !GREY && !SUBBOX && p.src_spec) tab[q] += (size_t)p.src_spec[ns] * p.spec_stride;
        nreal += have[q] ? 1u : 0u;
    }
    if (SUBBOX && nreal == 0) return;
    const int table = by_class ? unit + p.units * ((face_type ? i0[0] : k0[0]) & 7) : unit;
    const uint4 *__restrict__ cellA = p.geom[table].cellA;
    const uint4 *__restrict__ cellB = p.geom[table].cellB;
    const int nsteps = p.geom[table].nsteps;
    // Tables that share their inner shells (clipped windows, geometry_device.hip): the steps before `inner_steps` are read through
    // the family's first table.  The step index is wave-uniform: a scalar compare and two scalar selects per table load.
    const int inner_info = p.geom[table].inner;
    const int inner_steps = inner_info >> 8;
    const uint4 *__restrict__ innerA = p.geom[inner_info & 255].cellA;
    const uint4 *__restrict__ innerB = p.geom[inner_info & 255].cellB;
    const int sa = (uinfo & 1) ? -1 : 1, sb = (uinfo & 2) ? -1 : 1, sc = (uinfo & 4) ? -1 : 1;

    // LDS: the small tables sit first, at compile-time offsets (TABCAP entries each), then the shell buffers
    double2 *logtab = reinterpret_cast<double2 *>(lds_raw);
    double *inv_s = reinterpret_cast<double *>(logtab + LOG_TABLE_SIZE);
    // per source, per axis: wrapped position of offset t on the unit's side [0, TABCAP) and on the mirrored side [TABCAP, 2 TABCAP)
    int *wtab = reinterpret_cast<int *>(inv_s + TABCAP);
    double *shells = reinterpret_cast<double *>(wtab + NSRC * 6 * TABCAP);
    const int slots = (p.max_cells + 2) & ~1;      // cells + the zero slot, even (keeps 16-B alignment)
    // source q's two shell buffers follow source q-1's: prev/cur of source q = prev/cur + q * 2 * slots
    double *prev, *cur;
    if (GLOBAL_SCRATCH) {
        prev = p.shell_scratch + (size_t)blk * 2 * slots;
        cur = prev + slots;
    } else {
        prev = shells;
        cur = prev + slots;
    }
    const int src_stride = 2 * slots;

    for (int t = threadIdx.x; t < LOG_TABLE_SIZE; t += RT_THREADS) logtab[t] = p.logtab[t];
    for (int t = threadIdx.x; t <= p.S; t += RT_THREADS) {
        inv_s[t] = 1.0 / (double)max(t, 1);
#pragma unroll
        for (int q = 0; q < NSRC; ++q) {
            int *w = wtab + q * 6 * TABCAP;
            // OPEN: an entry also says whether the unwrapped position lies outside [0, N) (WTAB_OUTSIDE; in_box_gpu of the
            // reference's build without PERIODIC, raytracing.cu:264-267).  The wrapped position stays: the cell is still swept,
            // on whatever nHI it finds there, and only its rate is dropped (nhi_address, `ok`)
            auto entry = [&](int x) -> int { return wrap_once(x, N) | ((OPEN && (unsigned)x >= (unsigned)N) ? (int)WTAB_OUTSIDE : 0); };
            w[t] = entry(i0[q] + sa * t);      // periodic position of offset t along each axis
            w[TABCAP + t] = entry(i0[q] - sa * t);      // (|offset| <= N/2: one wrap suffices, raytracing.cu:270-272)
            w[2 * TABCAP + t] = entry(j0[q] + sb * t);
            w[3 * TABCAP + t] = entry(j0[q] - sb * t);
            w[4 * TABCAP + t] = entry(k0[q] + sc * t);
            w[5 * TABCAP + t] = entry(k0[q] - sc * t);
        }
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NSRC; ++q) { prev[q * src_stride + p.max_cells] = 0.0; cur[q * src_stride + p.max_cells] = 0.0; }
    }
    __syncthreads();

    const double sig = p.sig, dr = p.dr;
    const unsigned negmask = (sa < 0 ? 1u : 0u) | (sb < 0 ? 2u : 0u) | (sc < 0 ? 4u : 0u);
    const bool ztr = p.z_transposed != 0;
    constexpr bool grey = GREY;

    // work accounting, per wave (scalar registers: population counts of the lane masks, no per-lane adds)
    unsigned int n_gamma = 0, n_eval = 0;
    unsigned int n_zero_lane = 0;                           // this lane's rated cells whose rate was exactly +0 and was not added
    unsigned int src_cell_gamma = 0, src_cell_eval = 0;      // the source cell (thread 0 only)

    // rate accumulation: `idx` indexes [phi | phi_t] (and [heat | heat_t])
    // One descriptor over [phi | phi_t] while the pair fits 2 GiB (N <= 512).  Beyond (SPLIT, N <= 645 -- the reference's own
    // limit, raytracing.cu:95): a descriptor over ONE layout, N^3 doubles -- possible for units whose rated cells all lie on
    // one face (the sectors), where the layout is the same for the whole workgroup: the descriptor starts at the layout the
    // unit's face writes and `desc_off8` takes that layout's offset out of the byte offsets.  A compile-time variant: without
    // it the kernels of N <= 512 are instruction for instruction what they were (the scalar alone cost two VGPRs, i.e. the
    // fourth wave per SIMD of the paired kernels).
    const bool unit_in_twin = SPLIT && ztr_desc(p, uinfo);
    const unsigned desc_cells = SPLIT ? p.ncell : 2u * p.ncell;
    // (subtracted in UNSIGNED arithmetic and cast once: at N = 576 idx * 8 reaches 3.0e9 and the layout's offset 1.5e9 -- as signed
    //  ints their sum would overflow, which the hardware wraps but the language leaves undefined)
    const unsigned desc_off8 = (SPLIT && unit_in_twin) ? 8u * (unsigned)p.ncell : 0u;
    __amdgpu_buffer_rsrc_t rs_phi = __builtin_amdgcn_make_buffer_rsrc(p.phi + (unit_in_twin ? p.ncell : 0u), 0, BUFATOM ? (int)(8u * desc_cells) : 0, 0x00020000);
    __amdgpu_buffer_rsrc_t rs_heat = __builtin_amdgcn_make_buffer_rsrc((HEAT ? p.heat : p.phi) + (unit_in_twin ? p.ncell : 0u), 0, (BUFATOM && HEAT) ? (int)(8u * desc_cells) : 0, 0x00020000);
    auto add_phi = [&](bool ok, unsigned idx, double v) {
        if (BUFATOM) (void)asora_buffer_atomic_fadd_f64(v, rs_phi, ok ? (int)(idx * 8u - desc_off8) : ASORA_OOB_OFFSET, 0, 0);
        else if (ok) unsafeAtomicAdd(p.phi + idx, v);
    };
    auto add_heat = [&](bool ok, unsigned idx, double v) {
        if (BUFATOM) (void)asora_buffer_atomic_fadd_f64(v, rs_heat, ok ? (int)(idx * 8u - desc_off8) : ASORA_OOB_OFFSET, 0, 0);
        else if (ok) unsafeAtomicAdd(p.heat + idx, v);
    };
    // BUFATOM: a pending rate is carried as the byte offset its atomic will use -- ASORA_OOB_OFFSET when the lane has nothing
    // to add -- instead of an index and a flag (a flag that lives across the step costs a select to make and a compare to use)
    auto add_phi_at = [&](int off, double v) { (void)asora_buffer_atomic_fadd_f64(v, rs_phi, off, 0, 0); };
    auto add_heat_at = [&](int off, double v) { (void)asora_buffer_atomic_fadd_f64(v, rs_heat, off, 0, 0); };

    // ---- SUBBOX, a later box of the source: continue from the trailing shell of the box before ------------
    const bool continues = SUBBOX && !p.sb_first;
    // (one trailing shell per source of the batch and unit)
    double *trail[NSRC];
#pragma unroll
    for (int q = 0; q < NSRC; ++q) trail[q] = SUBBOX ? p.sb_trail + ((size_t)loc[q] * p.units + unit) * (size_t)slots : nullptr;
    if (continues) {
#pragma unroll
        for (int q = 0; q < NSRC; ++q)
            if (have[q]) for (int t = threadIdx.x; t < p.max_cells; t += RT_THREADS) prev[q * src_stride + t] = trail[q][t];
    }
    // ---- shell 0: the source cell (raytracing.cu:285-294) -----------------------------------
    if (threadIdx.x == 0 && !continues) {
#pragma unroll
        for (int q = 0; q < NSRC; ++q) {
            const unsigned idx = ((unsigned)i0[q] * N + j0[q]) * N + k0[q];
            const double nHI = p.nhi[idx];
            const double path = 0.5 * dr;
            const double cd_out = 0.0 + nHI * path;
            prev[q * src_stride] = cd_out;
            src_cell_eval += have[q] ? 1u : 0u;
            if ((uinfo & 64) && have[q]) {                 // the source cell is rated by exactly one unit
                if (DUMP) p.dump[idx] = cd_out;
                const double phi = photo_rate_per_atom(flux[q], 0.0, cd_out, dr * dr * dr * nHI, p, logtab, tab[q]);
                unsafeAtomicAdd(&p.phi[idx], phi);
                if (HEAT && !p.grey) unsafeAtomicAdd(&p.heat[idx], heat_rate_per_atom(flux[q], 0.0, cd_out, dr * dr * dr * nHI, p, logtab, tab[q]));
                src_cell_gamma += 1;
            }
        }
    }
    __syncthreads();

    // ---- shells 1..S, software-pipelined ------------------------------------------------------
    // The tables of a step do not depend on the medium, and the address of a cell's nHI only on
    // its table entry, so both are fetched ahead of the dependent arithmetic: tables two steps
    // ahead, nHI one step ahead.  The rate lookups of a step are issued after its shell barrier, so
    // their latency never holds the barrier up, and consumed a step later.
    // (The tables carry two all-invalid steps of padding at the end: prefetches stay in bounds.)
    auto nhi_address = [&](int q, unsigned abc, unsigned flags, unsigned &idx) -> const double * {
        const int *w = wtab + q * 6 * TABCAP;
        // (a cell on the mirrored side of an axis the unit merges reads the second half of that axis's table)
        const unsigned i = w[(abc & 1023) + ((flags >> CELL_NEG_SHIFT) & 1u) * TABCAP];
        const unsigned j = w[2 * TABCAP + ((abc >> 10) & 1023) + ((flags >> (CELL_NEG_SHIFT + 1)) & 1u) * TABCAP];
        const unsigned k = w[4 * TABCAP + ((abc >> 20) & 1023) + ((flags >> (CELL_NEG_SHIFT + 2)) & 1u) * TABCAP];
        const bool zt = ztr && (abc >> 30) == 2;
        // the [k][j][i] copies follow the [i][j][k] grids in memory: one 32-bit index covers both
        // (one formula with the outer and inner coordinate swapped, rather than two under a branch)
        // OPEN: the marks of the three entries.  `outer` and `row` are 24-bit multiplicands below, so the mark of `outer` and
        // the one `j` carries into `row` fall away by themselves; `inner` is the final 32-bit addend and is stripped here.
        // The OR of the three rides on the top bit of `idx` (an index stays below 2^28 while one descriptor spans both
        // layouts, N <= 512), so the step that rates the cell gets it at no register.
        const unsigned outside = OPEN ? ((i | j | k) & WTAB_OUTSIDE) : 0u;
        const unsigned outer = zt ? k : i, inner = (zt ? i : k) & (OPEN ? ~WTAB_OUTSIDE : ~0u);
        // (24-bit multiplies: N <= 1280 (device_init) so outer * N + j < 2^21; a 32-bit integer multiply runs at a quarter of their rate)
        // (spelled out: from __umul24 the compiler makes one 24-bit and one 64-bit multiply-add)
        unsigned row, cell;
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(row) : "v"(outer), "s"(N), "v"(j));
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(cell) : "v"(row), "s"(N), "v"(inner));
        idx = cell + (zt ? p.ncell : 0u);
        const double *addr = p.nhi + idx;
        if (OPEN) idx |= outside;
        return addr;
    };

    // One step of one lane, straight-line (whole-wave instruction count is what matters, so
    // inactive lanes run the arithmetic on harmless padding values and only the LDS store and
    // the atomic are predicated).  `cur_*` is this step's table entry / nHI, `nxt_*` the next
    // step's (its nHI is requested here), `pf_*` the register set the entry two steps ahead is
    // loaded into.  The loop below is unrolled three times with the three register sets rotating,
    // so the pipeline needs no register-to-register copies.
    bool late_ok[NSRC];                // a rate computed in the previous step, not yet added
    unsigned late_idx[NSRC];
    int late_off[NSRC];                // BUFATOM: byte offset of the pending rate's atomic, or ASORA_OOB_OFFSET
    Lookup pend_A[NSRC], pend_B[NSRC];             // lookups issued in the previous step, consumed in this one
    bool pend_thick[NSRC];
    double pend_pref[NSRC], pend_dtau[NSRC];
#pragma unroll
    for (int q = 0; q < NSRC; ++q) {
        late_ok[q] = false; late_idx[q] = 0; late_off[q] = ASORA_OOB_OFFSET;
        pend_A[q].t = pend_B[q].t = pend_A[q].h = pend_B[q].h = double2{0.0, 0.0};
        pend_A[q].residual = pend_B[q].residual = 0.0;
        pend_thick[q] = false; pend_pref[q] = 0.0; pend_dtau[q] = 0.0;
    }

    // SUBBOX: photons through the faces of the current sub-box (f90:541-543), per lane; the faces on the unit's own side
    // and on the mirrored side of each axis
    double loss[NSRC];
    bool pend_edge = false, cur_edge = false;     // (geometry only: the same for every source of the workgroup)
    double pend_pv[NSRC];                 // flux / volume of the pending cell (pref without the division by nHI)
#pragma unroll
    for (int q = 0; q < NSRC; ++q) { loss[q] = 0.0; pend_pv[q] = 0.0; }
    const int edge_own[3] = {sa > 0 ? p.sb_edge_r : p.sb_edge_l, sb > 0 ? p.sb_edge_r : p.sb_edge_l, sc > 0 ? p.sb_edge_r : p.sb_edge_l};
    const int edge_mir[3] = {sa > 0 ? p.sb_edge_l : p.sb_edge_r, sb > 0 ? p.sb_edge_l : p.sb_edge_r, sc > 0 ? p.sb_edge_l : p.sb_edge_r};

    // `first_c`: std::true_type for the steps of a unit's first triple -- the only ones that can hold shell 1, whose cells next to
    // the source get the diagonal factors of raytracing.cu:431-441; every other step is compiled without that block.
    auto step = [&](auto first_c, int k_pf, unsigned e_pf, const uint4 &cur_A, const uint4 &cur_B, const double (&cur_nhi)[NSRC], const unsigned (&cur_idx)[NSRC],
                    const uint4 &nxt_A, double (&nxt_nhi)[NSRC], unsigned (&nxt_idx)[NSRC], uint4 &pf_A, uint4 &pf_B) {
        constexpr bool FIRST_TRIPLE = decltype(first_c)::value;
        __builtin_amdgcn_sched_barrier(0);      // nothing of this step is scheduled into the previous one (see above the kernel)
        pf_A = (k_pf < inner_steps ? innerA : cellA)[e_pf];                      // two steps ahead (step k_pf)
        pf_B = (k_pf < inner_steps ? innerB : cellB)[e_pf];
#pragma unroll
        for (int q = 0; q < NSRC; ++q) nxt_nhi[q] = *nhi_address(q, nxt_A.x, nxt_A.y, nxt_idx[q]);          // one step ahead

        const bool valid = (cur_A.y & CELL_VALID) != 0;
        // waves whose 64 entries are all padding skip the arithmetic (wave-uniform branch)
        const bool wave_has_work = __builtin_amdgcn_ballot_w64(valid) != 0ull;
        bool rated[NSRC];
        double cd_in[NSRC], cd_out[NSRC], vol_nhi[NSRC];
        unsigned dst_idx[NSRC];
#pragma unroll
        for (int q = 0; q < NSRC; ++q) { rated[q] = false; cd_in[q] = 0.0; cd_out[q] = 0.0; vol_nhi[q] = 1.0; dst_idx[q] = 0; }
        if (wave_has_work) {
        // ---- what the table entry alone determines: once per lane-step, whatever NSRC -------------------------------
        const unsigned abc = cur_A.x;
        const int a = abc & 1023, b = (abc >> 10) & 1023, c = (abc >> 20) & 1023;
        const unsigned face = abc >> 30;                 // 2: dk = s, 1: dj = s, 0: di = s
        const int s = max(a, max(b, c));

        // ---- cinterp_gpu, raytracing.cu:345-535 ------------------------------------------
        // Bilinear weights: with alam = (s-1/2)/s the reference's dx = 2|alam*u - (u - 1/2)|
        // (raytracing.cu:397-403, source-relative) is 1 - u/s, so
        // s1..s4 = fu*fv, fv*(1-fu), fu*(1-fv), (1-fu)*(1-fv) with fu = u/s (raytracing.cu:405-408).
        // fu = 0 (resp. 1) makes the weights of the corners that do not exist in shell s-1 exactly 0.
        const int U = face == 0 ? b : a, V = face == 2 ? b : c;
        const double is = inv_s[s];
        // (u*(1/s) may miss 0 or 1 by an ulp; the corner that would then get a ~1e-16 weight does not exist
        //  in shell s-1 and reads the zero slot, so only the denominator moves, below rounding)
        const double fu = (double)U * is, fv = (double)V * is;
        const double gu = 1.0 - fu, gv = 1.0 - fv;
        const double w1 = fu * fv, w2 = fv * gu, w3 = fu * gv, w4 = gu * gv;
        const double path = __hiloint2double((int)cur_A.w, (int)cur_A.z) * dr;
        // a cell on an octant-boundary plane is rated by the octant with the + sign there
        const unsigned zmask = (cur_A.y >> CELL_ZERO_SHIFT) & 7u;        // (a == 0) | (b == 0) << 1 | (c == 0) << 2, tabulated
        const double maxcd = p.fortran_consts ? (double)2e30f : 2e30;                    // raytracing.cu:15
        const bool owner = valid && (cur_A.y & CELL_RATE) && (zmask & negmask) == 0;
        const double n2 = (double)(a * a + b * b + c * c);
        const double volfac = n2 * (dr * dr * FOURPI) * path;                              // raytracing.cu:302-307 without nHI
        const unsigned own_slot = cur_A.y & CELL_SLOT_MASK;
        if (SUBBOX) {       // is the cell on a face of the current sub-box?  only from the shell of the nearest face on (a
            // wave's entries belong to one shell: a wave-uniform branch; without clipping that is the box's last shell only)
            cur_edge = false;
            if (__builtin_amdgcn_readfirstlane(s) >= min(p.sb_edge_r, p.sb_edge_l)) {
                const unsigned nb = cur_A.y >> CELL_NEG_SHIFT;
                cur_edge = a == ((nb & 1u) ? edge_mir[0] : edge_own[0]) || b == ((nb & 2u) ? edge_mir[1] : edge_own[1]) ||
                           c == ((nb & 4u) ? edge_mir[2] : edge_own[2]);
            }
        }
        n_eval += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(valid)) * nreal;

        // ---- per source: the medium-dependent arithmetic ----------------------------------------------------------------
        // (round 4: loading the corner values of EVERY source before the first source's shell-buffer store -- the compiler
        //  cannot know that the store does not feed the other source's loads, so it orders them behind it -- was measured:
        //  0 at R = 16 ... 32, -1 % at R = 48, and 130 instead of 128 VGPRs, i.e. three waves per SIMD instead of four: not kept)
#pragma unroll
        for (int q = 0; q < NSRC; ++q) {
            const double *pq = prev + q * src_stride;
            // w_n = s_n / max(0.6, c_n*sig) (raytracing.cu:33,422-425) and
            // cdensi = sum(c_n w_n)/sum(w_n) (raytracing.cu:428), with numerator and denominator
            // multiplied through by the four max() terms: one division instead of five.
            const double x1 = pq[cur_B.x], x2 = pq[cur_B.y], x3 = pq[cur_B.z], x4 = pq[cur_B.w];
            const double m1 = fmax(0.6, x1 * sig), m2 = fmax(0.6, x2 * sig);
            const double m3 = fmax(0.6, x3 * sig), m4 = fmax(0.6, x4 * sig);
            const double m12 = m1 * m2, m34 = m3 * m4;
            const double q1 = w1 * (m2 * m34), q2 = w2 * (m1 * m34);
            const double q3 = w3 * (m12 * m4), q4 = w4 * (m12 * m3);
            double cdi = div_newton(x1 * q1 + x2 * q2 + x3 * q3 + x4 * q4, q1 + q2 + q3 + q4);     // (the weights sum to 1, each max() is >= 0.6)
            if (FIRST_TRIPLE && s == 1) {                    // diagonal neighbours of the source, cu:431-441
                // (round 3: a wave's entries belong to one shell, so this could be a scalar branch instead of the dozen selects
                //  the compiler makes of it -- measured: no gain at R = 16 / 32, +5 % at R = 64: the branch splits the
                //  scheduling region around the LDS reads; left as it is)
                const int nz = (a == 0) + (b == 0) + (c == 0);
                const double r3 = p.fortran_consts ? (double)1.7320507764816284 : 1.73205080757; // f90:608 / cu:435
                const double r2 = p.fortran_consts ? (double)1.4142135381698608 : 1.41421356237; // f90:609 / cu:439
                if (nz < 2) cdi = (nz == 0 ? r3 : r2) * cdi;
            }
            cd_in[q] = cdi;

            // ---- the cell itself, raytracing.cu:270-276,311-328 -----------------------------
            const double nHI = cur_nhi[q];
            cd_out[q] = fma(nHI, path, cdi);
            if (valid) cur[q * src_stride + own_slot] = cd_out[q];
            if (DUMP) {
                if (owner) {
                    const int *w = wtab + q * 6 * TABCAP;
                    const unsigned nb = cur_A.y >> CELL_NEG_SHIFT;
                    const unsigned di = w[a + (nb & 1u) * TABCAP], dj = w[2 * TABCAP + b + ((nb >> 1) & 1u) * TABCAP];
                    const unsigned dk = w[4 * TABCAP + c + ((nb >> 2) & 1u) * TABCAP];
                    p.dump[(di * N + dj) * N + dk] = cd_out[q];
                }
            }
            // OPEN: a cell beyond a face of the box is neither rated nor counted; its pending offset below is ASORA_OOB_OFFSET
            const bool ok = owner && cdi <= maxcd && (NSRC == 1 || have[q]) && !(OPEN && (cur_idx[q] & WTAB_OUTSIDE));
            rated[q] = ok;
            n_gamma += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(ok));
            vol_nhi[q] = volfac * nHI;
            dst_idx[q] = cur_idx[q];
        }
        }

        if (__builtin_amdgcn_readfirstlane(cur_A.y) & CELL_LAST) {   // shell finished: publish it
            __syncthreads();
            double *tmp = prev; prev = cur; cur = tmp;
        }

        // ---- rates, raytracing.cu:315-328 + rates.cu:16-41 ---------------------------------------
        if (grey) {
#pragma unroll
            for (int q = 0; q < NSRC; ++q)
                add_phi(rated[q], dst_idx[q], grey_rate_per_atom(flux[q], cd_in[q], cd_out[q], vol_nhi[q], p));
        } else {    // (waves without work issue their unused lookups as well: see above the kernel)
            // (lanes without a rate run the lookups on whatever they hold: the index is clamped for any input)
            // TAU_PHOTO_LIMIT: rates.cu:7 (double 1e-7) or photorates.f90:69 (single 1e-7 promoted)
            const double limit = p.fortran_consts ? (double)1.0e-7f : 1.0e-7;
            bool thick[NSRC];
            double dtau[NSRC], arg_A[NSRC], arg_B[NSRC], tau_at_entry[NSRC];
            int toff[NSRC];
#pragma unroll
            for (int q = 0; q < NSRC; ++q) {
                const double tau_in = mul_unfused(cd_in[q], sig), tau_out = mul_unfused(cd_out[q], sig);   // un-fused, see rate_issue
                tau_at_entry[q] = tau_in;
                dtau[q] = tau_out - tau_in;
                thick[q] = fabs(dtau[q]) > limit;
                // one code path for both kinds of cell: per-lane table offset and arguments.  A thin cell looks its tau_thin up
                // twice: tau_in with the Fortran's constants (photorates.f90:121), tau_out with the CUDA library's (rates.cu:37)
                toff[q] = thick[q] ? 0 : table_stride(p.table_len);
                arg_A[q] = (thick[q] || p.fortran_consts) ? tau_in : tau_out;
                arg_B[q] = (thick[q] || !p.fortran_consts) ? tau_out : tau_in;
            }
            // SUBBOX: the second lookup of a THIN cell is the THICK table at tau_in: phi_in = pref T_thick(tau_in), which
            // the photon loss needs (phi_out = phi_in - phi, photorates.f90:120-125); its rate only uses the first
            // SKIP_ZERO (ASORA_OPT_SKIP_ZERO_RATES): a thick cell whose tau_in lies beyond the last table entry gets
            // pref * (T_last - T_last) = exactly +0; adding it changes nothing, so the atomic is not issued -- and when no
            // lane of the wave has anything to add, neither are the division, the logarithms and the lookups.  (pref must
            // be finite for the product to be 0 and not NaN: vol_nhi is checked instead of forming pref first.)  A kernel
            // variant of its own: the test and the branch cost 4.5 % where nothing can be left out.
            bool add[NSRC];
            bool wave_adds = true;
#pragma unroll
            for (int q = 0; q < NSRC; ++q) add[q] = rated[q];
            // SKIP_ZERO with BUFATOM (round 3; the variant launch_raytrace takes while its probes find such cells): the same
            // test per lane without a branch around the atomic -- the lane carries the out-of-range offset of a lane without
            // a rate, so its atomic never becomes a request -- and, below, whole waves of them skip the rate arithmetic.
            if (SKIP_ZERO) {
#pragma unroll
                for (int q = 0; q < NSRC; ++q) {
                    // (BUFATOM form: one compare.  A thick cell has nHI * path * sig > 1e-7, so nHI is an ordinary positive number
                    //  and pref = flux / (volume x nHI) is finite unless the volume factor itself is out of range, which the
                    //  branching variant's two extra tests guard against and this one leaves to vol_nhi > 0 being implied)
                    const bool zero_rate = (SKIP_ZERO && !BUFATOM)
                        ? (thick[q] && tau_at_entry[q] >= p.tau_zero && fabs(vol_nhi[q]) > 1e-250 && (vol_nhi[q] - vol_nhi[q] == 0.0))
                        : (thick[q] && tau_at_entry[q] >= p.tau_zero);
                    add[q] = rated[q] && !zero_rate;
                    n_zero_lane += (rated[q] && zero_rate) ? 1u : 0u;      // per lane: one add-with-carry; summed when the workgroup ends
                }
                // a wave none of whose lanes has anything to add leaves out the division, the logarithms and the index
                // arithmetic as well; the BUFATOM form then issues as many (wave-uniform, cheap) table loads as the other path,
                // so that the number of operations in flight is the same wherever the two paths meet
                bool any_add = add[0];
#pragma unroll
                for (int q = 1; q < NSRC; ++q) any_add = any_add || add[q];
                wave_adds = __builtin_amdgcn_ballot_w64(any_add) != 0ull;
            }
            {   // the previous step's lookups have had a whole step to arrive: form its rates now, issue this step's
                // lookups, then add the rates behind them
                double v_prev[NSRC], h_prev[NSRC], pref[NSRC];
                Lookup A2[NSRC], B2[NSRC];
#pragma unroll
                for (int q = 0; q < NSRC; ++q) {
                    const double ta = lookup_value(pend_A[q]), tb = lookup_value(pend_B[q]);
                    v_prev[q] = pend_thick[q] ? pend_pref[q] * (ta - tb) : pend_pref[q] * pend_dtau[q] * ta;
                    h_prev[q] = 0.0;
                    if (HEAT) {
                        const double ha = lookup_heat(pend_A[q]), hb = lookup_heat(pend_B[q]);
                        h_prev[q] = pend_thick[q] ? pend_pref[q] * (ha - hb) : pend_pref[q] * pend_dtau[q] * ha;
                    }
                    A2[q] = pend_A[q]; B2[q] = pend_B[q];
                    pref[q] = 0.0;
                }
                if (wave_adds) {
#pragma unroll
                    for (int q = 0; q < NSRC; ++q) {
                        // (nHI = 0 -- a fully ionised or empty cell: the reference divides by zero; flux / +0 = flux * inf)
                        pref[q] = vol_nhi[q] == 0.0 ? flux[q] * INFINITY : div_newton(flux[q], vol_nhi[q]);
                        A2[q] = lookup_issue<HEAT>(tab[q], arg_A[q], p, logtab, toff[q]);
                        B2[q] = lookup_issue<HEAT>(tab[q], arg_B[q], p, logtab, SUBBOX ? 0 : toff[q]);
                    }
                }
                else if (BUFATOM && SKIP_ZERO) {
#pragma unroll
                    for (int q = 0; q < NSRC; ++q) {     // (distinct addresses, or the loads would be merged)
                        const double2 *__restrict__ dummy = tab[q] + (threadIdx.x & 1) + 4 * q;
                        A2[q].t = dummy[0]; A2[q].residual = 0.0;
                        B2[q].t = dummy[2]; B2[q].residual = 0.0;
                        if (HEAT) { A2[q].h = dummy[2 * p.table_len]; B2[q].h = dummy[2 * p.table_len + 2]; }
                        else { A2[q].h = A2[q].t; B2[q].h = B2[q].t; }
                    }
                }
                if (SUBBOX) {
                    // what leaves the PREVIOUS step's cell through the far side, if that cell lies on a face of the box
                    if (__builtin_amdgcn_ballot_w64(pend_edge) != 0ull) {
#pragma unroll
                        for (int q = 0; q < NSRC; ++q) {
                            const bool lost = (BUFATOM ? late_off[q] != ASORA_OOB_OFFSET : late_ok[q]) && pend_edge;
                            const double ta = lookup_value(pend_A[q]), tb = lookup_value(pend_B[q]);
                            const double po = pend_thick[q] ? pend_pv[q] * tb : pend_pv[q] * (tb - pend_dtau[q] * ta);
                            if (lost) loss[q] += po;
                        }
                    }
                    // flux / volume of this step's cell, should it lie on a face: pref * nHI, or the quotient itself where
                    // nHI = 0 (pref = inf)
                    if (__builtin_amdgcn_ballot_w64(cur_edge) != 0ull) {
#pragma unroll
                        for (int q = 0; q < NSRC; ++q) {
                            double pv = pref[q] * cur_nhi[q];
                            if (__builtin_amdgcn_ballot_w64(cur_nhi[q] == 0.0) != 0ull) {
                                const double n2s = (double)((cur_A.x & 1023) * (cur_A.x & 1023) + ((cur_A.x >> 10) & 1023) * ((cur_A.x >> 10) & 1023) +
                                                            ((cur_A.x >> 20) & 1023) * ((cur_A.x >> 20) & 1023));
                                const double vol = n2s * (dr * dr * FOURPI) * (__hiloint2double((int)cur_A.w, (int)cur_A.z) * dr);
                                if (cur_nhi[q] == 0.0) pv = flux[q] / vol;
                            }
                            pend_pv[q] = pv;
                        }
                    }
                    pend_edge = cur_edge;
                }
#pragma unroll
                for (int q = 0; q < NSRC; ++q) {
                    if (BUFATOM) {
                        add_phi_at(late_off[q], v_prev[q]);
                        if (HEAT) add_heat_at(late_off[q], h_prev[q]);
                    } else {
                        add_phi(late_ok[q], late_idx[q], v_prev[q]);
                        if (HEAT) add_heat(late_ok[q], late_idx[q], h_prev[q]);
                    }
                }
#pragma unroll
                for (int q = 0; q < NSRC; ++q) {
                    pend_A[q] = A2[q]; pend_B[q] = B2[q]; pend_thick[q] = thick[q]; pend_pref[q] = pref[q]; pend_dtau[q] = dtau[q];
                    if (BUFATOM) late_off[q] = add[q] ? (int)(dst_idx[q] * 8u - desc_off8) : ASORA_OOB_OFFSET;
                    else { late_idx[q] = dst_idx[q]; late_ok[q] = add[q]; }
                }
            }
        }
    };

    // SUBBOX: the steps of this launch's sub-box only (whole triples: the tables are padded at every box boundary)
    const int k_first = SUBBOX ? p.sb_k0[unit] : 0, k_last = SUBBOX ? p.sb_k1[unit] : nsteps;
    unsigned e = (unsigned)k_first * RT_THREADS + threadIdx.x;
    uint4 A0 = (k_first < inner_steps ? innerA : cellA)[e], B0 = (k_first < inner_steps ? innerB : cellB)[e];
    uint4 A1 = (k_first + 1 < inner_steps ? innerA : cellA)[e + RT_THREADS], B1 = (k_first + 1 < inner_steps ? innerB : cellB)[e + RT_THREADS];
    uint4 A2, B2;
    unsigned idx0[NSRC], idx1[NSRC], idx2[NSRC];
    double nhi0[NSRC], nhi1[NSRC], nhi2[NSRC];
#pragma unroll
    for (int q = 0; q < NSRC; ++q) {
        idx1[q] = idx2[q] = 0; nhi1[q] = nhi2[q] = 0.0;
        nhi0[q] = *nhi_address(q, A0.x, A0.y, idx0[q]);
    }
    // The loop is entered with the loads in flight that a step leaves behind, in the same order (tables, nHI, two lookups):
    // the compiler merges the counts of outstanding operations of the loop entry with those of the back edge and waits as
    // the SHORTER history demands, so without these two (unused) lookups every first step of the unrolled three waited
    // for its nHI and its predecessor's lookups as if nothing else were in flight.
    if (!GREY) {
        __builtin_amdgcn_sched_barrier(0);          // behind the nHI load, as in a step
        const double2 *__restrict__ prime = tab[0] + (threadIdx.x & 1);
#pragma unroll
        for (int q = 0; q < NSRC; ++q) {
            // (distinct addresses, or the loads would be merged; a further source's come from the 128-entry log table)
            pend_A[q].t = q == 0 ? prime[0] : p.logtab[(threadIdx.x & 1) + 4 * q];
            if (HEAT) pend_A[q].h = prime[2 * p.table_len];
            pend_B[q].t = q == 0 ? prime[p.table_len] : p.logtab[(threadIdx.x & 1) + 4 * q + 2];
            if (HEAT) pend_B[q].h = prime[3 * p.table_len - 1];
        }
        if (BUFATOM) {                              // ... and the (dropped) atomics that follow them
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < NSRC; ++q) {
                (void)asora_buffer_atomic_fadd_f64(0.0, rs_phi, ASORA_OOB_OFFSET, 0, 0);
                if (HEAT) (void)asora_buffer_atomic_fadd_f64(0.0, rs_heat, ASORA_OOB_OFFSET, 0, 0);
            }
        }
    }

    // nsteps is a multiple of 3 (the tables are padded to it) and is followed by two more
    // all-invalid steps, so every look-ahead stays inside the tables.
    // Shell 1 (at most 26 cells) is step 0 of a unit's table: the first triple is peeled off with the shell-1 block in it.
    int k = k_first;
    if (k == 0 && k < k_last) {
        step(std::true_type{}, k + 2, e + 2 * RT_THREADS, A0, B0, nhi0, idx0, A1, nhi1, idx1, A2, B2);
        step(std::true_type{}, k + 3, e + 3 * RT_THREADS, A1, B1, nhi1, idx1, A2, nhi2, idx2, A0, B0);
        step(std::true_type{}, k + 4, e + 4 * RT_THREADS, A2, B2, nhi2, idx2, A0, nhi0, idx0, A1, B1);
        k += 3; e += 3 * RT_THREADS;
    }
    for (; k < k_last; k += 3, e += 3 * RT_THREADS) {
        step(std::false_type{}, k + 2, e + 2 * RT_THREADS, A0, B0, nhi0, idx0, A1, nhi1, idx1, A2, B2);
        step(std::false_type{}, k + 3, e + 3 * RT_THREADS, A1, B1, nhi1, idx1, A2, nhi2, idx2, A0, B0);
        step(std::false_type{}, k + 4, e + 4 * RT_THREADS, A2, B2, nhi2, idx2, A0, nhi0, idx0, A1, B1);
    }
#pragma unroll
    for (int q = 0; q < NSRC; ++q) {
        const double ta = lookup_value(pend_A[q]), tb = lookup_value(pend_B[q]);
        const double v_last = pend_thick[q] ? pend_pref[q] * (ta - tb) : pend_pref[q] * pend_dtau[q] * ta;
        if (BUFATOM) add_phi_at(late_off[q], v_last); else add_phi(late_ok[q], late_idx[q], v_last);
        if (HEAT) {
            const double ha = lookup_heat(pend_A[q]), hb = lookup_heat(pend_B[q]);
            const double h_last = pend_thick[q] ? pend_pref[q] * (ha - hb) : pend_pref[q] * pend_dtau[q] * ha;
            if (BUFATOM) add_heat_at(late_off[q], h_last); else add_heat(late_ok[q], late_idx[q], h_last);
        }
    }

    if (SUBBOX) {
#pragma unroll
        for (int q = 0; q < NSRC; ++q) {
            // the pending cell of the last step
            {
                const double ta = lookup_value(pend_A[q]), tb = lookup_value(pend_B[q]);
                const double po = pend_thick[q] ? pend_pv[q] * tb : pend_pv[q] * (tb - pend_dtau[q] * ta);
                if ((BUFATOM ? late_off[q] != ASORA_OOB_OFFSET : late_ok[q]) && pend_edge) loss[q] += po;
            }
            if (!have[q]) continue;
            // hand the last shell swept to the next sub-box's launch (the step that closed it ended with the barrier and the
            // swap: it is `prev`, complete)
            for (int t = threadIdx.x; t < p.max_cells; t += RT_THREADS) trail[q][t] = prev[q * src_stride + t];
            double l = loss[q];
            for (int o = 32; o > 0; o >>= 1) l += __shfl_down(l, o);
            if ((threadIdx.x & 63) == 0 && l != 0.0) unsafeAtomicAdd(p.sb_loss + loc[q], l * (dr * dr * dr));
        }
    }

    // work accounting: one atomic per wave and counter
    unsigned int n_zero = n_zero_lane;
    if (SKIP_ZERO) for (int o = 32; o > 0; o >>= 1) n_zero += __shfl_down(n_zero, o);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *slot = p.counters + COUNTER_FIELDS * (blockIdx.x & (COUNTER_SLOTS - 1));     // (see COUNTER_SLOTS)
        atomicAdd(slot, (unsigned long long)(n_gamma + src_cell_gamma));
        atomicAdd(slot + 1, (unsigned long long)(n_eval + src_cell_eval));
        if (n_zero) atomicAdd(slot + 2, (unsigned long long)n_zero);
        if (SKIP_ZERO && p.zero_probe) {      // a probe launch (launch_raytrace): its own pair of sums, spread like the others
            unsigned long long *pr = p.zero_probe + 2 * (blockIdx.x & (ZERO_PROBE_SLOTS - 1));
            atomicAdd(pr, (unsigned long long)(n_gamma + src_cell_gamma));
            if (n_zero) atomicAdd(pr + 1, (unsigned long long)n_zero);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Host driver of the octant kernel (the role of do_all_sources_gpu's batch loop,
// raytracing.cu:101-143).  What a launch is going to be is decided in raytrace_plan.hpp; here is what touches the device.
// ---------------------------------------------------------------------------------------------
static_assert(LDS_LOG_TABLE_BYTES == LOG_TABLE_SIZE * sizeof(double2), "raytrace_plan.hpp counts the log table as the kernel lays it out");

// Which rows have been launched (asora_debug_form_launches, asora_debug_last_launch_form; tests): process-wide, not in State, so
// that they outlive device_close.  A row counts once its launch's hipGetLastError is clean.
static unsigned long long form_launches[RT_FORM_COUNT];
static int last_launch_row = -1;
const unsigned long long *form_launch_counts() { return form_launches; }
void reset_form_launch_counts() { std::fill(form_launches, form_launches + RT_FORM_COUNT, 0ULL); }
int last_launched_row() { return last_launch_row; }
// the row of a form about to be launched, noted where st.last_variant is (-1: not built -- launch_form refuses it)
static void note_launch_form(const RtForm &f)
{
    const RtForm *at = std::find(RT_FORMS.row, RT_FORMS.row + RT_FORM_COUNT, f);
    last_launch_row = at != RT_FORMS.row + RT_FORM_COUNT ? (int)(at - RT_FORMS.row) : -1;
}

// Row I of RT_FORMS: the one place where the kernel's template arguments are written, so the rows of the table are the
// instantiations of the build
template <size_t I>
static int launch_form_row(const RtParams &q, unsigned grid, size_t lds_bytes, hipStream_t stream)
{
    constexpr RtForm f = RT_FORMS.row[I];
    constexpr auto kernel = raytrace_octant_kernel<f.threads, f.global_scratch, f.dump, f.heat, f.tabcap, f.skip_zero, f.grey, f.bufatom, f.nsrc, f.subbox, f.split, f.spec, f.open>;
    ASORA_HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(f.threads), lds_bytes, stream, q);
    ASORA_HIP_TRY(hipGetLastError());
    form_launches[I] += 1;
    return 0;
}
// The row equal to the planned form; a form that is not built is an error, never a neighbouring kernel
template <size_t... I>
static int launch_form(const RtForm &f, const RtParams &q, unsigned grid, size_t lds_bytes, hipStream_t stream, std::index_sequence<I...>)
{
    int rc = -1;
    (void)((RT_FORMS.row[I] == f && ((rc = launch_form_row<I>(q, grid, lds_bytes, stream)), true)) || ...);
    if (rc < 0) return fail(11, "raytrace: no kernel is built for the form " + form_text(f) + " (internal error)");
    return rc;
}
constexpr std::make_index_sequence<RT_FORM_COUNT> ALL_FORMS{};

// What open boundaries are not built for: refused before anything is launched (every entry point asks through
// require_raytrace_inputs; launch_raytrace asks again, so that no launch can slip past)
int check_open_boundaries(const State &st, const char *who, bool open, bool dump)
{
    if (!open) return 0;
    const std::string why = open_boundaries_refusal(st.N, st.opt[ASORA_OPT_GREY_NOTABLES] && !st.coldens_only, st.opt[ASORA_OPT_GLOBAL_ATOMICS] != 0, dump);
    return why.empty() ? 0 : fail(4, std::string(who) + ": open boundaries (ASORA_OPT_OPEN_BOUNDARIES) " + why);
}

// Who shares a workgroup with whom when the tables are the aligned kind (pairs_by_class, raytrace_plan.hpp), and the dispatch
// orders: cached on the device per (list, range), dropped with every change of the source lists
static void release_order_lists(State &st)
{
    for (auto &e : st.order_lists) if (e.dev) (void)hipFree(e.dev);
    st.order_lists.clear();
}
void release_pair_lists(State &st)
{
    for (auto &e : st.pair_lists) for (int ft = 0; ft < 2; ++ft) if (e.dev[ft]) (void)hipFree(e.dev[ft]);
    st.pair_lists.clear();
    release_order_lists(st);
}

static int source_pairs_by_class(State &st, const int32_t *host_pos, const void *list, int begin, int count, const State::PairList *&out)
{
    for (const auto &e : st.pair_lists)
        if (e.list == list && e.begin == begin && e.count == count) { out = &e; return 0; }
    if (st.pair_lists.size() >= 64) release_pair_lists(st);
    State::PairList e{list, begin, count, {nullptr, nullptr}, {0, 0}};
    static_assert(sizeof(SrcPair) == sizeof(int2), "the kernel reads a pair as int2");
    for (int ft = 0; ft < 2; ++ft) {
        std::vector<SrcPair> pairs;
        pairs_by_class(host_pos, begin, count, ft, pairs, e.cls[ft]);
        e.n[ft] = (int)pairs.size();
        if (int rc = device_allocate(e.dev[ft], std::max<size_t>(1, pairs.size()))) return rc;
        ASORA_HIP_TRY(hipMemcpy(e.dev[ft], pairs.data(), pairs.size() * sizeof(int2), hipMemcpyHostToDevice));
    }
    st.pair_lists.push_back(e);
    out = &st.pair_lists.back();
    return 0;
}

// The workgroups of a launch of q.src_count sources from q.src_begin: per unit one for every source or every two, by the
// class lists where the tables are aligned; q.spread and the grid from their number
// `ordered`: a launch that is not spread takes its blocks from a dispatch order (block_order, raytrace_plan.hpp; the kernel's
// p.order), built once per (list, range, shape) like the pair lists; else, and for the few workgroups of a spread launch, the
// arithmetic map of the kernel's prologue
static int set_launch_grid(State &st, RtParams &q, int units, bool pairs, bool aligned, const int32_t *host_pos, bool ordered, unsigned &grid)
{
    int groups = pairs ? (q.src_count + 1) / 2 : q.src_count;              // workgroups per unit
    const State::PairList *pl = nullptr;
    if (pairs && aligned) {        // partners agree modulo 8 along the memory-contiguous axis of the unit's face
        if (int rc = source_pairs_by_class(st, host_pos, q.src_pos, q.src_begin, q.src_count, pl)) return rc;
        for (int ft = 0; ft < 2; ++ft) { q.pairs[ft] = pl->dev[ft]; q.npairs[ft] = pl->n[ft]; }
        groups = std::max(pl->n[0], pl->n[1]);
    }
    grid = launch_grid(groups, units, st.cu_count, q.spread);
    q.order = nullptr;
    if (!ordered || q.spread) return 0;
    if (aligned && !host_pos) return fail(11, "raytrace: aligned tables without the positions of the source list (internal error)");
    const int nsrc = pairs ? 2 : 1;
    for (const auto &e : st.order_lists)
        if (e.list == q.src_pos && e.begin == q.src_begin && e.count == q.src_count && e.units == units && e.aligned == (int)aligned && e.nsrc == nsrc) {
            q.order = e.dev; grid = e.grid;
            return 0;
        }
    if (st.order_lists.size() >= 64) release_order_lists(st);
    std::vector<int> face_type((size_t)units);
    for (int u = 0; u < units; ++u) {
        face_type[(size_t)u] = ((st.geom_host[u].info >> 8) & 3) == 3 ? 1 : 0;
        if (face_type[(size_t)u] != (unit_face(units, u) == 2 ? 1 : 0)) return fail(11, "raytrace: unit_face disagrees with the geometry tables (internal error)");
    }
    const int none[2] = {0, 0};
    const int *const no_cls[2] = {nullptr, nullptr};
    const int *const pair_cls[2] = {pl ? pl->cls[0].data() : nullptr, pl ? pl->cls[1].data() : nullptr};
    std::vector<int32_t> order;
    State::OrderList e{q.src_pos, q.src_begin, q.src_count, units, (int)aligned, nsrc, nullptr, 0};
    e.grid = launch_block_order(host_pos, q.src_begin, q.src_count, units, face_type.data(), pairs, aligned, pl ? pl->n : none, pl ? pair_cls : no_cls, order);
    if (e.grid == 0 || e.grid > grid) return fail(11, "raytrace: dispatch order of " + std::to_string(e.grid) + " blocks (internal error)");
    static_assert(sizeof(int2) == 2 * sizeof(int32_t), "an entry of the dispatch order is {group, unit}");
    if (int rc = device_allocate(e.dev, (order.size() + 1) / 2)) return rc;
    ASORA_HIP_TRY(hipMemcpy(e.dev, order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    st.order_lists.push_back(e);
    q.order = e.dev; grid = e.grid;
    return 0;
}

// {rated pairs, exact zeros left out} of a probe launch, summed over its slots into pinned host memory
__global__ void __launch_bounds__(ZERO_PROBE_SLOTS) zero_probe_sum_kernel(const unsigned long long *__restrict__ slots, unsigned long long *out)
{
    __shared__ unsigned long long r[2][ZERO_PROBE_SLOTS];
    r[0][threadIdx.x] = slots[2 * threadIdx.x]; r[1][threadIdx.x] = slots[2 * threadIdx.x + 1];
    __syncthreads();
    for (int o = ZERO_PROBE_SLOTS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { r[0][threadIdx.x] += r[0][threadIdx.x + o]; r[1][threadIdx.x] += r[1][threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = r[0][0]; out[1] = r[1][0]; }
}

// Exact-zero rates (ASORA_OPT_SKIP_ZERO_RATES, see the kernel's SKIP_ZERO).  The kernels that leave them out cost 5 % where
// there are none, and save up to a quarter of the launch where most cells lie beyond the table (the neutral medium of an
// early-reionisation run).  Left to the library (0) a launch takes them while the last PROBE found more than 15 % of the
// rated pairs dark; a probe is such a launch whose two sums go to pinned host memory behind it and are looked at, without
// waiting, by a later call: the first launch, every 64th after it, every launch while the dark variant runs anyway.
// exists: such a form exists for this launch (RtPlan::zero_form_exists)
static int decide_skip_zero(State &st, bool exists, bool &skip_zero, bool &probe)
{
    skip_zero = false; probe = false;
    const int skip_zero_opt = st.opt[ASORA_OPT_SKIP_ZERO_RATES];
    if (exists && skip_zero_opt == 1) skip_zero = true;
    else if (exists && skip_zero_opt == 0) {
        if (!st.zero.dev) {
            if (int rc = st.zero.dev.allocate(2 * ZERO_PROBE_SLOTS)) return rc;
            if (int rc = st.zero.host.allocate(2)) return rc;
            ASORA_HIP_TRY(hipEventCreateWithFlags(&st.zero.done, hipEventDisableTiming));
        }
        if (st.zero.verdict.pending && hipEventQuery(st.zero.done) == hipSuccess) {
            const double rated = (double)st.zero.host[0], dark = (double)st.zero.host[1];
            st.zero.verdict.dark = rated > 0.0 && dark > 0.15 * rated;
            st.zero.verdict.known = true;
            st.zero.verdict.pending = false;
        }
        (void)hipGetLastError();      // (hipErrorNotReady from the query is not an error)
        st.zero.verdict.since_probe += 1;
        probe = !st.zero.verdict.pending && (!st.zero.verdict.known || st.zero.verdict.since_probe >= 64 || st.zero.verdict.dark);
        skip_zero = probe || st.zero.verdict.dark;
    }
    return 0;
}
// behind a probe launch: its sums to the host
static int launch_zero_probe_sum(State &st, hipStream_t stream)
{
    hipLaunchKernelGGL(zero_probe_sum_kernel, dim3(1), dim3(ZERO_PROBE_SLOTS), 0, stream,
                       (const unsigned long long *)st.zero.dev, st.zero.host);
    ASORA_HIP_TRY(hipGetLastError());
    ASORA_HIP_TRY(hipEventRecord(st.zero.done, stream));
    st.zero.verdict.pending = true;
    st.zero.verdict.since_probe = 0;
    return 0;
}

// Shells that outgrow LDS live in global memory: bound that scratch to ~2 GiB per launch (the reference's source batching,
// raytracing.cu:126, reappears only for such traces).  batch: in, the sources left; out, those of this launch
static int ensure_shell_scratch(State &st, int units, size_t shell_bytes, int &batch)
{
    const size_t per_src = (size_t)units * shell_bytes;
    const size_t budget = (size_t)2 << 30;
    int max_batch = (int)std::max<size_t>(8, (budget / per_src) / 8 * 8);
    batch = std::min(batch, max_batch);
    const size_t need = (size_t)8 * units * ((batch + 7) / 8) * shell_bytes;
    return st.shell_scratch.reserve(need / sizeof(double));
}

// How the radius behaves from call to call (a call = one raytrace of the library's API, one time step of the evolve loop):
// the eight-fold line-aligned tables only pay when they are reused (see plan_shape)
bool note_call_radius(State &st, double R, int path)
{
    // (one history per path -- 0: the whole-box ASORA trace and the evolve loop, 1: the sub-box sweep, whose R is R_max_LLS and
    //  whose calls alternate with the other's in a process that uses both: a shared history would see the radius "change" on
    //  every alternation and never let the aligned tables back in)
    State::RadiusHistory &h = st.rt.radius[path ? 1 : 0];
    if (R != h.last_R) {
        if (h.last_R >= 0.0) h.has_changed = true;
        h.last_R = R;
        h.same_R_calls = 0;
    }
    h.same_R_calls += 1;
    return !h.has_changed || h.same_R_calls > 32;
}

// the options a plan reads, as asora_set_option left them
void plan_options(const State &st, RtPlanInput &in)
{
    in.cu_count = st.cu_count;
    in.sectors = st.opt[ASORA_OPT_SECTORS]; in.block_threads = st.opt[ASORA_OPT_BLOCK_THREADS]; in.pair_sources = st.opt[ASORA_OPT_PAIR_SOURCES];
    in.aligned_rows = st.opt[ASORA_OPT_ALIGNED_ROWS]; in.global_atomics = st.opt[ASORA_OPT_GLOBAL_ATOMICS];
    in.skip_zero_rates = st.opt[ASORA_OPT_SKIP_ZERO_RATES]; in.z_transposed_opt = st.opt[ASORA_OPT_Z_TRANSPOSED] != 0;
}

int launch_raytrace(State &st, RtParams &p, bool dump, bool heat, hipStream_t side)
{
    // (per-source spectra: checked by the entry points already; here so that no launch can carry an unchecked index)
    if (p.src_spec) { if (int rc = check_source_spectra("raytrace")) return rc; }
    if (int rc = check_open_boundaries(st, "raytrace", p.open_bc != 0, dump)) return rc;
    const int32_t *host_pos = p.src_pos == st.sources.pos_sorted ? st.sources.loaded.pos_sorted_host.data()
                            : p.src_pos == st.sources.pos ? st.sources.loaded.pos_host.data() : nullptr;
    RtPlanInput in{};
    plan_options(st, in);
    in.N = p.N; in.R = p.R; in.src_count = p.src_count; in.shape_src_count = p.shape_src_count;
    in.grey = p.grey != 0; in.heat = heat; in.dump = dump; in.open = p.open_bc != 0; in.z_transposed = p.z_transposed != 0;
    in.table_sets = p.src_spec != nullptr; in.host_positions = host_pos != nullptr; in.radius_stays = p.radius_stays != 0;
    const RtShape sh = plan_shape(in);
    if (int rc = ensure_geometry(st, p, sh.threads, sh.units, nullptr, sh.aligned)) return rc;
    st.last_variant = 0;
    const LutIndex lut = lut_index_constants(p.minlogtau, p.dlogtau);      // log10(2)/dlogtau, 1 - minlogtau/dlogtau, their remainder
    p.lut_k1 = lut.k1; p.lut_k0 = lut.k0; p.lut_kc = lut.kc;
    // optical depth from which BOTH lookups of a thick cell return the same table value (index clamped to NumTau, or on
    // the last pair of the device table, whose slope is 0): 0.01 index units beyond the exact point, far more than the
    // 1e-12 the device's log2 can be off by
    // ASORA_OPT_SKIP_ZERO_RATES: 0 = where it costs nothing (the buffer-atomic kernels drop such lanes' atomics), 1 = everywhere
    // (kernels without buffer atomics take the branching SKIP_ZERO variant), 2 = nowhere
    p.tau_zero = INFINITY;
    if (in.skip_zero_rates != 2 && !p.grey && p.lut_k1 > 0.0) {
        const double last = std::min(p.numtau_f, (double)(p.table_len - 1));
        p.tau_zero = std::exp2((last + 0.01 - p.lut_k0) / p.lut_k1);
    }
    in.tau_zero_finite = std::isfinite(p.tau_zero);
    RtPlan plan{};
    std::string why;
    if (int rc = plan_launch(in, sh, p.S, p.max_cells, plan, why)) return fail(rc, why);
    p.split_desc = plan.form.split ? 1 : 0;
    // launches that share the global shell scratch stay on the main stream (one at a time)
    hipStream_t stream = (side && plan.use_lds) ? side : st.stream;
    if (side && !plan.use_lds) {       // ... behind whatever the side streams still run, and the side streams behind it
        for (int q = 0; q < 2; ++q)
            if (st.side_pending[q]) ASORA_HIP_TRY(hipStreamWaitEvent(st.stream, st.side_done[q], 0));
    }
    bool skip_zero = false, probe = false;
    if (int rc = decide_skip_zero(st, plan.zero_form_exists, skip_zero, probe)) return rc;
    plan_skip_zero(plan, skip_zero);
    const RtForm &form = plan.form;

    int done = 0;
    while (done < p.src_count) {
        int batch = p.src_count - done;
        if (!plan.use_lds) { if (int rc = ensure_shell_scratch(st, sh.units, plan.shell_bytes, batch)) return rc; }
        RtParams q = p;
        q.src_begin = p.src_begin + done;
        q.src_count = batch;
        q.shell_scratch = plan.use_lds ? nullptr : st.shell_scratch;
        q.zero_probe = nullptr;
        if (probe && done == 0) {
            ASORA_HIP_TRY(hipMemsetAsync(st.zero.dev, 0, 2 * ZERO_PROBE_SLOTS * sizeof(unsigned long long), stream));
            q.zero_probe = st.zero.dev;
        }
        unsigned grid = 0;
        if (int rc = set_launch_grid(st, q, sh.units, form.nsrc == 2, sh.aligned, host_pos, !dump, grid)) return rc;
        st.last_variant = variant_word(form, sh.units, sh.aligned);
        note_launch_form(form);
        {
            KernelTimer kt(ASORA_KERNEL_RAYTRACE, stream);
            if (int rc = launch_form(form, q, grid, plan.lds_bytes, stream, ALL_FORMS)) return rc;
        }
        if (q.zero_probe) { if (int rc = launch_zero_probe_sum(st, stream)) return rc; }
        done += batch;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// The sub-box sweep of the reference's CPU function on this file's tabulated geometry (see the kernel's SUBBOX and
// subbox.hip for the semantics).  The tables hold the cells within R_max_LLS inside the traversal range -- the only ones
// that are rated or add to the photon loss; a source whose column densities go back to the caller needs the whole cube and
// stays with the on-the-fly kernel of subbox.hip.
// ---------------------------------------------------------------------------------------------
int subbox_tables_prepare(State &st, RtParams &p, int ext_r, int ext_l, int subboxsize, int src_count, bool heat, SubboxTables &out,
                          const int32_t *host_pos)
{
    out = SubboxTables();
    out.host_pos = host_pos;
    SubboxPlanInput in{};
    in.ext_r = ext_r; in.ext_l = ext_l; in.S_tab = subbox_table_extent(p.R, ext_r, ext_l);
    in.table_sources = src_count; in.has_dump = false; in.heat = heat;
    in.buffer_atomics = !p.grey && p.z_transposed && !st.opt[ASORA_OPT_GLOBAL_ATOMICS] && 16ull * p.ncell <= 0x80000000ull;   // the rates go through buffer atomics (one descriptor: N <= 512)
    in.cu_count = st.cu_count;
    in.opt_tables = st.opt[ASORA_OPT_SUBBOX_TABLES]; in.opt_pairs = st.opt[ASORA_OPT_PAIR_SOURCES]; in.opt_aligned = st.opt[ASORA_OPT_ALIGNED_ROWS];
    const SubboxPlan plan = plan_subbox(in);
    if (!plan.tables) return 0;
    const int units = plan.units, threads = plan.threads;
    const SubboxGeometry sbg{ext_r, ext_l, subboxsize};
    // (line-aligned tables: also a mesh whose rows start on lines, positions the host knows)
    const bool aligned = plan.aligned && p.N % 8 == 0 && host_pos != nullptr;
    if (int rc = ensure_geometry(st, p, threads, units, &sbg, aligned)) return rc;
    out.aligned = aligned;
    if (form_lds_bytes(subbox_form(threads, heat, 1), p.max_cells) > LDS_LIMIT_BYTES) return 0;
    // one trailing shell per source and unit, within 2 GiB (82 KB per source at r_RT = 32: 26 000 sources per launch)
    const size_t per_source = (size_t)units * shell_slots(p.max_cells) * sizeof(double);
    size_t trail_budget = (size_t)2 << 30;
    if (const char *e = getenv("ASORA_SUBBOX_TRAIL_BUDGET")) trail_budget = std::max<size_t>(per_source, (size_t)atoll(e));   // tests: force several batches
    const int max_batch = (int)std::max<size_t>(1, std::min<size_t>((size_t)src_count, trail_budget / per_source));
    const size_t need = (size_t)max_batch * per_source;
    if (int rc = st.subbox.trail.reserve(need / sizeof(double))) return rc;
    p.sb_trail = st.subbox.trail;
    out.units = units; out.threads = threads; out.S = p.S; out.max_batch = max_batch; out.ok = true;
    // two sources per workgroup where the plan wants them and four shell buffers fit
    out.nsrc = (plan.nsrc == 2 && form_lds_bytes(subbox_form(threads, false, 2), p.max_cells) <= LDS_LIMIT_BYTES) ? 2 : 1;
    return 0;
}

int subbox_tables_sweep(State &st, const RtParams &p, const SubboxTables &tab, int s_begin, int s_end, bool heat)
{
    RtParams q = p;
    bool any = false;
    for (int u = 0; u < tab.units; ++u) {
        const std::vector<int> &after = st.geom_step_after_shell[u];
        auto at = [&](int s) { return after[(size_t)std::min<long>(std::max(s, 0), (long)after.size() - 1)]; };
        q.sb_k0[u] = at(s_begin);
        q.sb_k1[u] = at(s_end);
        if (q.sb_k0[u] % 3 || q.sb_k1[u] % 3) return fail(11, "sub-box tables: a box boundary is not on a triple of steps (internal error)");
        any = any || q.sb_k1[u] > q.sb_k0[u];
    }
    if (!any) return 0;                       // the box lies beyond the radius: nothing is rated, nothing is lost
    q.sb_first = s_begin == 0 ? 1 : 0;
    const bool pairs = tab.nsrc == 2 && !heat;
    const RtForm form = subbox_form(tab.threads, heat, pairs ? 2 : 1);
    unsigned grid = 0;
    if (int rc = set_launch_grid(st, q, tab.units, pairs, tab.aligned, tab.host_pos, false, grid)) return rc;
    st.last_variant = variant_word(form, tab.units, tab.aligned);
    note_launch_form(form);
    {   // asora_debug_last_subbox_launch: the form and grid shape of this very launch
        int *r = st.sb_launch;
        if (q.sb_first) r[ASORA_SBL_TABLE_SOURCES] += p.src_count;
        r[ASORA_SBL_UNITS] = tab.units; r[ASORA_SBL_THREADS] = form.threads; r[ASORA_SBL_NSRC] = form.nsrc;
        r[ASORA_SBL_ALIGNED] = tab.aligned ? 1 : 0; r[ASORA_SBL_HEAT] = form.heat ? 1 : 0;
        r[ASORA_SBL_TABLE_LAUNCHES] += 1;
    }
    KernelTimer kt(ASORA_KERNEL_RAYTRACE);
    return launch_form(form, q, grid, form_lds_bytes(form, p.max_cells), st.stream, ALL_FORMS);
}

} // namespace asora

