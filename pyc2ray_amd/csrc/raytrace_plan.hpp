// raytrace_plan.hpp -- what a raytrace launch is going to be, decided by pure host functions: no HIP, no State.
//   stage 1 (plan_shape), before the geometry tables exist: workgroups per source, threads per workgroup, aligned rows;
//   stage 2 (plan_launch), from stage 1 and the tables' shell count and largest shell: the kernel form (RtForm, one field per
//   template parameter of raytrace_octant_kernel), LDS, and the ASORA_VARIANT_* word;
//   RT_FORMS: the forms that are built.  raytrace.hip instantiates exactly these rows and launches the row equal to the plan.
// raytrace.hip feeds them from State and RtParams, asora_debug_launch_plan from its arguments (tests/test_launch_forms_host.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/asora_hip.h"

namespace asora {

// One field per template parameter of raytrace_octant_kernel, in its order
struct RtForm {
    int threads; bool global_scratch, dump, heat; int tabcap; bool skip_zero, grey, bufatom; int nsrc; bool subbox, split, spec, open;
};
constexpr bool operator==(const RtForm &a, const RtForm &b)
{
    return a.threads == b.threads && a.global_scratch == b.global_scratch && a.dump == b.dump && a.heat == b.heat && a.tabcap == b.tabcap &&
           a.skip_zero == b.skip_zero && a.grey == b.grey && a.bufatom == b.bufatom && a.nsrc == b.nsrc && a.subbox == b.subbox &&
           a.split == b.split && a.spec == b.spec && a.open == b.open;
}
inline void form_values(const RtForm &f, int v[13])
{
    const int a[13] = {f.threads, f.global_scratch, f.dump, f.heat, f.tabcap, f.skip_zero, f.grey, f.bufatom, f.nsrc, f.subbox, f.split, f.spec, f.open};
    std::copy(a, a + 13, v);
}
inline std::string form_text(const RtForm &f)      // the template arguments, as DESIGN.md writes them
{
    int v[13];
    form_values(f, v);
    std::string s = "<";
    for (int k = 0; k < 13; ++k) s += (k ? "," : "") + std::to_string(v[k]);
    return s + ">";
}

// The forms that are built, family by family (kind: 0 table rates, 1 the same without the exact zeros, 2 with heating, 3 grey
// opacity); the kernel's static_asserts check every row.
// The 1024-entry LDS tables (more than 256 shells: N >= 512 with R >= 256) are built with the shells in global memory only: the
// smallest largest shell such a trace has -- N = 512, R = 256, cut into the 96 quarter sectors -- holds 12 445 cells, 199 KB of shell
// buffers against the 124 KB that LDS leaves beside those tables, so no launch of the library plans them with the shells in LDS
// (plan_launch, asked about shells that no geometry has, still names such a form; it is reported as not built).
constexpr int RT_FORM_COUNT = 152;
struct RtFormTable { RtForm row[RT_FORM_COUNT]; int n; };
constexpr RtFormTable make_form_table()
{
    RtFormTable t{};
    constexpr bool f = false, y = true;
    // single source, THREADS x TABCAP: 256-entry tables at every size, 64-entry ones for small workgroups, 1024-entry ones for large
    // (shells in global memory only).  Buffer atomics; global atomics (N > 512, option; the exact zeros left out by a branch) with
    // the shells in LDS or, without a zero-skipping form, in global memory
    constexpr int single[10][2] = {{64, 256}, {128, 256}, {256, 256}, {512, 256}, {1024, 256}, {64, 64}, {128, 64}, {256, 1024}, {512, 1024}, {1024, 1024}};
    for (const auto &s : single)
        for (int gs = 0; gs < 2; ++gs)
            for (int ba = 0; ba < 2; ++ba)
                for (int kind = 0; kind < 4; ++kind)
                    if (!(gs && (ba || kind == 1)) && (gs || s[1] != 1024)) t.row[t.n++] = RtForm{s[0], gs != 0, f, kind == 2, s[1], kind == 1, kind == 3, ba != 0, 1, f, f, y, f};
    // column-density dump: 256 threads (pick_launch_shape), shells in LDS or global memory, table or grey opacity
    for (int cap : {256, 1024})
        for (int gs = cap == 1024 ? 1 : 0; gs < 2; ++gs)
            for (int gr = 0; gr < 2; ++gr) t.row[t.n++] = RtForm{256, gs != 0, y, f, cap, f, gr != 0, f, 1, f, f, y, f};
    // two sources per workgroup (production): with and without the exact zeros
    constexpr int paired[8][2] = {{64, 256}, {128, 256}, {256, 256}, {512, 256}, {64, 64}, {128, 64}, {256, 64}, {256, 32}};
    for (const auto &s : paired)
        for (int sz = 0; sz < 2; ++sz) t.row[t.n++] = RtForm{s[0], f, f, f, s[1], sz != 0, f, y, 2, f, f, y, f};
    // descriptors per layout (512 < N <= 645), paired: also without per-source table sets (see the kernel's SPEC)
    constexpr int paired_split[4][2] = {{256, 32}, {256, 64}, {256, 256}, {512, 256}};
    for (const auto &s : paired_split)
        for (int sz = 0; sz < 2; ++sz)
            for (int sp = 0; sp < 2; ++sp) t.row[t.n++] = RtForm{s[0], f, f, f, s[1], sz != 0, f, y, 2, f, y, sp != 0, f};
    for (int th : {256, 512}) {
        // ... and single, every kind
        for (int kind = 0; kind < 4; ++kind) t.row[t.n++] = RtForm{th, f, f, kind == 2, 256, kind == 1, kind == 3, y, 1, f, y, y, f};
        // open boundaries: paired with the 256-entry tables; single with or without heating, shells in LDS or global memory
        t.row[t.n++] = RtForm{th, f, f, f, 256, f, f, y, 2, f, f, y, y};
        for (int cap : {256, 1024})
            for (int gs = cap == 1024 ? 1 : 0; gs < 2; ++gs)
                for (int ht = 0; ht < 2; ++ht) t.row[t.n++] = RtForm{th, gs != 0, f, ht != 0, cap, f, f, y, 1, f, f, y, y};
        // sub-box sweep: one source with or without heating, two without
        for (int k = 0; k < 3; ++k) t.row[t.n++] = RtForm{th, f, f, k == 1, 256, f, f, y, k == 2 ? 2 : 1, y, f, y, f};
    }
    return t;
}
constexpr RtFormTable RT_FORMS = make_form_table();
static_assert(RT_FORMS.n == RT_FORM_COUNT, "RT_FORM_COUNT is the number of rows make_form_table writes");
inline bool form_is_built(const RtForm &f) { return std::find(RT_FORMS.row, RT_FORMS.row + RT_FORM_COUNT, f) != RT_FORMS.row + RT_FORM_COUNT; }

// What the decisions read
struct RtPlanInput {
    int N;
    double R;
    int src_count, shape_src_count;   // sources of this launch; sources the launch shape is chosen for (the whole call's, not a pipelined range's)
    int cu_count;
    int sectors, block_threads, pair_sources, aligned_rows, global_atomics, skip_zero_rates;   // options as they stood when the call began
    bool z_transposed_opt;            // ASORA_OPT_Z_TRANSPOSED itself; z_transposed: what the launch's grids have
    bool grey, heat, dump, open, z_transposed;
    bool table_sets;                  // per-source table sets are attached (RtParams::src_spec)
    bool host_positions;              // the host knows the positions of the source list (pairing by alignment class)
    bool radius_stays;                // note_call_radius
    bool tau_zero_finite;             // an optical depth exists beyond which rates are exactly 0 (RtParams::tau_zero)
};

constexpr size_t LDS_LIMIT_BYTES = 160 * 1024;
constexpr size_t LDS_LOG_TABLE_BYTES = 256 * 2 * sizeof(double);     // LOG_TABLE_SIZE x double2 (rates_device.hpp)
constexpr size_t lds_table_bytes(int tabcap, int nsrc = 1) { return LDS_LOG_TABLE_BYTES + (size_t)tabcap * (sizeof(double) + (size_t)nsrc * 6 * sizeof(int)); }
constexpr size_t shell_slots(int max_cells) { return ((size_t)max_cells + 2) & ~(size_t)1; }   // a shell buffer: max_cells + zero slot, rounded to even (16-B alignment)
constexpr size_t shell_pair_bytes(int max_cells) { return 2 * shell_slots(max_cells) * sizeof(double); }   // the two shell buffers of one source

// Decomposition and workgroup size.  Shells of a small trace do not fill 256 lanes (R=16: <= 310 cells per
// octant shell); a large one needs so much LDS per octant that few workgroups fit a CU.  Three things pull:
//   * padding: every shell of every unit is padded to whole waves, so FEWER, LARGER units waste fewer lanes (R = 16:
//     1.41 lane-steps per rated cell with 8 octants, 1.04 with the whole sphere in one workgroup; R = 32: 1.17 with 12
//     sector pairs, 1.10 with 6 sectors whose transverse axes are both mirrored), and units that cover both signs of an
//     axis do not evaluate the plane between them twice;
//   * the rate atomics want long contiguous rows: units that mirror the memory-contiguous axis of a face sweep full
//     chords of the sphere (~15 % fewer 64-B atomic requests per rated cell than octants);
//   * LDS: a unit's two shell buffers must leave room for enough workgroups per CU, which is what stops the merging --
//     the whole sphere needs 39 KB at R = 16 and 157 KB at R = 32.
// Thresholds from sweeps on MI355X (1000 sources, 256^3; tools/sweep_units.sh, profiles/r03_sweep_units_run*.txt):
//   R < 11.5: whole sphere x 128 threads | < 15.5: x 256 | < 21.5: x 512 | < 23.5: half spheres x 256 | < 25.5: x 512 |
//   < 36.5: 6 sectors by sign of the dominant offset x 256 | < 52.5: 12 mirrored sector pairs x 256 | else x 512
// (round 2, without the merged kinds: R <= 12 octant pairs x 64 | 13..14 x 128 | 15..19 octants x 64 | 20..22 sector pairs
//  x 64 | 23..28 octant pairs x 256 | 29..35 sector pairs x 128 | 36..54 x 256 | >= 55 x 512 -- still what is used when the
//  merged kinds would leave CUs without a workgroup)
// the merged kinds by radius (mu = 0 beyond them); the sub-box sweep takes its shape from the same table
inline void merged_kind(double r, int &mu, int &mt)
{
    mu = 0; mt = 0;
    if (r < 11.5) { mu = 1; mt = 128; }
    else if (r < 15.5) { mu = 1; mt = 256; }
    else if (r < 21.5) { mu = 1; mt = 512; }
    else if (r < 23.5) { mu = 2; mt = 256; }
    else if (r < 25.5) { mu = 2; mt = 512; }
    else if (r < 36.5) { mu = 6; mt = 256; }
    else if (r < 52.5) { mu = 12; mt = 256; }
}
inline void pick_launch_shape(const RtPlanInput &in, int &units, int &threads)
{
    const double R = in.R;
    const int N = in.N, src_count = in.shape_src_count > 0 ? in.shape_src_count : in.src_count;
    const bool dump = in.dump;
    const double r = std::min(R, 0.87 * N);                 // the window cuts the trace at ~sqrt(3)/2 N
    const double est_cells = 1.2 * r * r;                   // largest shell of an octant
    if (r <= 12.5) { units = 4; threads = 64; }             // pairs of whole octants mirrored in x
    else if (r <= 14.5) { units = 4; threads = 128; }
    else if (est_cells <= 450.0) { units = 8; threads = 64; }        // r <= 19.4
    else if (r <= 22.5) { units = 12; threads = 64; }
    else if (r <= 28.5) { units = 4; threads = 256; }
    else if (est_cells <= 1500.0) { units = 12; threads = 128; }     // r <= 35.3
    else if (est_cells <= 3500.0) { units = 12; threads = 256; }     // r <= 54
    else { units = 12; threads = 512; }
    {   // the merged kinds, when they still give every CU a couple of workgroups
        int mu = 0, mt = 0;
        merged_kind(r, mu, mt);
        if (mu && (long)src_count * mu >= 2L * in.cu_count && !dump) { units = mu; threads = mt; }
        // Beyond N = 512 a buffer descriptor spans ONE layout of the rate grid (buffer_atomics_fit, `split`), so the production forms --
        // two sources per workgroup, buffer atomics -- need units whose rated cells all lie on one kind of face.  Where the radius
        // would take the whole sphere or the half spheres (cells of every face in one workgroup: the global-atomic family, one
        // source per workgroup), the three all-sign sectors take their place (round 6; the reference's meshes end at 645,
        // ref: src/asora/raytracing.cu:95).  Measured at N = 576, 1000 sources (profiles/r06_ab_576_small_radii.txt): r_RT = 16
        // 0.286 -> 0.241 ms, r_RT = 24 0.605 -> 0.589 ms; below the radius from which two sources share a workgroup (15.5) the
        // whole sphere stays (r_RT = 12: 0.137 against 0.140 ms).
        if ((units == 1 || units == 2) && units == mu && r >= 15.5 && N > 512 && N <= 645 && (long)src_count * 3 >= 2L * in.cu_count &&
            !in.global_atomics && in.z_transposed_opt) {
            units = 3;
            threads = r < 21.5 ? 256 : 512;
        }
    }
    // Few sources (fewer workgroups than CUs): the time of the call is the time of ONE workgroup, so cut a source
    // into more (24 sectors) and wider pieces.  One source, 128^3, R = 64: 0.235 -> 0.146 ms (tools/sweep_single_source.sh)
    // A few dozen sources (workgroups for half the CUs' slots at most): still one round, wider workgroups finish it sooner
    // (64 sources, R = 32: pairs x 256 threads 0.183 ms against 0.202 with 128; tools/sweep_mid_counts.sh)
    if ((long)src_count * 12 <= (long)in.cu_count * 4 && units == 12 && threads == 128) threads = 256;
    if ((long)src_count * 12 < (long)in.cu_count) {
        units = 24;
        if (est_cells > 900.0) threads = std::max(threads, 512);
        if (est_cells > 2500.0) threads = 1024;
    }
    // A handful of sources: 24 workgroups each still leave most CUs idle -- quarter the sectors (96 per source; each wedge
    // re-derives the inner part of its sector, so evaluations double, time about halves)
    // (measured, one source: 128^3 whole box 0.205 -> 0.157 ms, R = 32 0.051 -> 0.043 ms; the floor is the chain of shells,
    //  ~2 us each, not the work: tools/sweep_single_source.sh)
    if ((long)src_count * 48 <= (long)in.cu_count) {
        units = 96;
        threads = est_cells > 6000.0 ? 1024 : est_cells > 2500.0 ? 512 : 256;
    }
    const int want_sectors = in.sectors;
    if (want_sectors == 1) units = 8;
    if (want_sectors == 2) units = 24;
    if (want_sectors == 3) units = 12;
    if (want_sectors == 4) units = 96;
    if (want_sectors == 5) units = 4;
    if (want_sectors == 6) units = 1;
    if (want_sectors == 7) units = 2;
    if (want_sectors == 8) units = 3;
    if (want_sectors == 9) units = 6;
    const int forced = in.block_threads;
    if (forced == 64 || forced == 128 || forced == 256 || forced == 512 || forced == 1024) threads = forced;
    if (dump) threads = 256;                                // the column-density dump variant is built for 256 only
}

// Enough waves must be left to fill the chip (two per SIMD) when two sources share a workgroup
inline bool pairs_fill_chip(int src_count, int units, int threads, int cu_count)
{
    return (long)(src_count / 2) * units * (threads / 64) >= 8L * cu_count;
}
// Does sweeping two sources per workgroup pay?  (auto mode of ASORA_OPT_PAIR_SOURCES; from A/B runs on MI355X, 1000 sources,
// 256^3: profiles/r03_ab_two_sources.txt -- R = 16 -4 %, 20 -2 %, 26 -10 %, 28 -12 %, 32 -7 %, 40 -8 %, 48 -5 %, 56 and 64 0 %;
// nothing below R ~ 15, where the whole sphere is swept by few waves)
inline bool pair_sources_pays(const RtPlanInput &in, int units, int threads)
{
    const double r = std::min(in.R, 0.87 * in.N);
    if (!(r >= 15.5 && r < 52.5)) return false;
    return pairs_fill_chip(in.shape_src_count > 0 ? in.shape_src_count : in.src_count, units, threads, in.cu_count);
}

// ---- the sub-box sweep (subbox_api.hip): what it launches when left to itself --------------------------------------------------
// traversal range per axis side (raytracing.f90:174-175) and the last shell a table of the cells within R_max_LLS would hold
inline void subbox_range(int N, int max_subbox, int &ext_r, int &ext_l)
{
    ext_r = std::min(max_subbox, N / 2 - 1 + N % 2);
    ext_l = std::min(max_subbox, N / 2);
}
inline int subbox_table_extent(double R, int ext_r, int ext_l)
{
    const double R2hi = R * R * (1.0 + 1e-9) + 1e-9;
    const int range = std::max(ext_r, ext_l);
    return std::isfinite(R2hi) ? (int)std::min((double)range, std::floor(std::sqrt(R2hi))) : range;
}
// workgroup size of the on-the-fly kernel (subbox.hip) for a launch of `sources` sources whose shells have pitch W:
// fewer workgroups than CUs (a handful of sources): the launch lasts as long as one workgroup, so wider workgroups shorten it;
// enough sources to fill the chip: 256 threads per workgroup; small boxes: shells of a few hundred cells fill 128 threads
// better (+-16: 0.65 -> 0.59 ms per 1000 sources; +-32: 256)
inline int subbox_fly_threads(int sources, int W, int cu_count)
{
    if ((long)sources * 8 < (long)cu_count) return 1024;
    return W <= 20 ? 128 : 256;
}
struct SubboxPlanInput {
    int S_tab, ext_r, ext_l;          // subbox_table_extent, subbox_range
    int table_sources;                // the call's sources without the one whose column densities go back to the caller
    bool has_dump, heat;
    bool buffer_atomics;              // table rates through one buffer descriptor: not grey, [k][j][i] twins, N <= 512, no ASORA_OPT_GLOBAL_ATOMICS
    int cu_count;
    int opt_tables, opt_pairs, opt_aligned;     // ASORA_OPT_SUBBOX_TABLES, _PAIR_SOURCES, _ALIGNED_ROWS
};
// Decided before the geometry exists.  What needs the built tables stays with subbox_tables_prepare: the sweep falls back to the
// on-the-fly kernel when one source's shells exceed LDS, to one source per workgroup when two sources' do, and `aligned` further
// needs a mesh that is a multiple of 8 and positions the host knows.
struct SubboxPlan {
    bool tables;                      // the sources that are not dumped sweep on tabulated geometry
    int units, threads, nsrc;         // ... in this shape, nsrc sources per workgroup
    bool aligned;                     // ... on line-aligned tables
    int fly_sources, fly_threads;     // sources of a one-batch call swept by the on-the-fly kernel, and its workgroup size
};
inline SubboxPlan plan_subbox(const SubboxPlanInput &in)
{
    SubboxPlan out{false, 0, 0, 1, false, 0, 0};
    const int want = in.opt_tables, src_count = in.table_sources;
    const double r = (double)in.S_tab;
    auto decide = [&]() {
        if (want == 1 || !in.buffer_atomics || in.ext_r <= 0 || in.ext_l <= 0 || src_count < 1) return false;
        if (in.S_tab + 1 > 256) return false;                             // the variant is built with the 256-entry LDS tables
        // auto: when the radius, not the range, bounds the work (else the tables would hold the whole cube), and not beyond
        // what a table of a few tens of MB covers
        if (want == 0 && !(in.S_tab < std::min(in.ext_r, in.ext_l) && in.S_tab <= 96)) return false;
        // the merged kinds of the ASORA sweep, in the workgroup sizes the sub-box forms are built for (256 and 512: the whole sphere
        // below 11.5 takes 256), and the sector pairs x 512 beyond them
        merged_kind(r, out.units, out.threads);
        if (!out.units) { out.units = 12; out.threads = 512; }
        out.threads = std::max(out.threads, 256);
        if (want == 0 && (long)src_count * out.units < 2L * in.cu_count) return false;     // a handful of sources: subbox.hip's wide workgroups
        return true;
    };
    out.tables = decide();
    if (out.tables) {
        // Rows cut at 64-byte lines, as for the ASORA sweep (plan_shape): sectors of one face.  ON REQUEST ONLY
        // (ASORA_OPT_ALIGNED_ROWS = 2): measured on MI355X, 1000 sources, 256^3, r_RT = 32 (profiles/r05_ab_subbox_aligned.jsonl), the
        // aligned tables give this sweep nothing -- 1.136 / 1.151 ms aligned against 1.139 / 1.143 ms packed with two sources per
        // workgroup, 1.235 against 1.18 ms with one -- where they gave the ASORA sweep -1.5 ... -4.7 %: here the photon-loss
        // arithmetic and 141 VGPRs (three waves per SIMD), not the atomic requests, set the pace.
        out.aligned = (out.units == 6 || out.units == 12) && r <= 110.0 && in.opt_aligned == 2;
        // two sources per workgroup (the kernel's NSRC = 2, round 4): as for the ASORA sweep -- table entry decoded once, tables
        // streamed once, two dependency chains per wave -- where enough workgroups remain; not with heating (two more lookups per
        // source in flight)
        const bool pays = r >= 15.5 && pairs_fill_chip(src_count, out.units, out.threads, in.cu_count);
        out.nsrc = (!in.heat && src_count >= 2 && (in.opt_pairs == 2 || (in.opt_pairs == 0 && pays))) ? 2 : 1;
    } else {
        out.units = out.threads = 0;
    }
    // with the tables, the on-the-fly kernel only sweeps the dumped source
    out.fly_sources = out.tables ? (in.has_dump ? 1 : 0) : std::max(src_count, 0) + (in.has_dump ? 1 : 0);
    out.fly_threads = out.fly_sources > 0 ? subbox_fly_threads(out.fly_sources, std::max(std::max(in.ext_r, in.ext_l), 0) + 1, in.cu_count) : 0;
    return out;
}

// Can the rate atomics go through buffer descriptors (the kernel's BUFATOM)?  One descriptor over both layouts of the rate
// grid while the pair fits 2 GiB (N <= 512); one per layout (split) up to 2 GiB per layout (N <= 645) for units whose rated
// cells all lie on one face -- the sector kinds.
// The split form is built for the shapes such meshes take at ordinary radii: 256 or 512 threads, up to 256 shells; two sources
// per workgroup for table rates without heating, one source per workgroup also with heating or grey opacity (everything else
// beyond N = 512 -- column-density dump, more than 256 shells, whole spheres below r = 15.5 -- keeps the global-atomic family).
inline bool buffer_atomics_fit(const RtPlanInput &in, int units, int threads, bool plain_tables, bool &split)
{
    const unsigned long long ncell = (unsigned long long)in.N * in.N * in.N;
    split = false;
    if (in.global_atomics) return false;
    if (16ull * ncell <= 0x80000000ull) return true;
    const bool one_face = units == 3 || units == 6 || units == 12 || units == 24 || units == 96;
    if (8ull * ncell <= 0x80000000ull && one_face && in.z_transposed && (threads == 256 || threads == 512) && plain_tables) { split = true; return true; }
    return false;
}

// What open boundaries are not built for (check_open_boundaries, code 4): the reason, or "" when the launch may go on
inline std::string open_boundaries_refusal(int N, bool grey_rates, bool global_atomics, bool dump)
{
    if (16ull * N * N * N > 0x80000000ull) return "are built for N <= 512 (mesh of " + std::to_string(N) + ")";
    if (grey_rates) return "need table rates (grey opacity, ASORA_OPT_GREY_NOTABLES, is on)";
    if (global_atomics) return "need the buffer-atomic kernels (ASORA_OPT_GLOBAL_ATOMICS is on)";
    if (dump) return "have no column-density dump";
    return "";
}

// Stage 1: before the geometry tables are built
struct RtShape { int units, threads; bool aligned; };   // one workgroup per (source, octant) or per (source, octant, sector)
inline RtShape plan_shape(const RtPlanInput &in)
{
    RtShape sh{0, 0, false};
    int &units = sh.units, &threads = sh.threads;
    pick_launch_shape(in, units, threads);
    if (in.open) threads = threads <= 256 ? 256 : 512;      // the workgroup sizes the open forms are built for (RT_FORMS)
    {   // number of shells, known before the tables are built: the 1024-entry LDS tables exist for 256/512 threads
        const double R2hi = in.R * in.R * (1.0 + 1e-9) + 1e-9;
        const int Emax = in.N / 2;
        const int S_est = std::isfinite(R2hi) ? (int)std::min((double)Emax, std::floor(std::sqrt(R2hi))) : Emax;
        if (S_est + 1 > 256 && threads < 256) threads = 256;
    }
    // rows cut at 64-byte lines (ASORA_OPT_ALIGNED_ROWS): units of one face, a mesh whose rows start on lines, the [k][j][i]
    // twin for the z-faces, a source list whose positions the host knows (pairing), and eight times the tables.  By default
    // where two sources share a workgroup (r < 52.5: -1.5 ... -4.7 %; beyond, with one source per workgroup and 0.13-0.2 GB of
    // tables, nothing: profiles/r03_ab_aligned_rows.txt); on request up to r ~ 110
    // ... and, left to the library, a radius that stays: building eight forms costs eight times as long (12 ms instead of
    // 2.5 at r = 30), which a run whose r_RT changes with every time step (R_max_LLS in cells under cosmological expansion,
    // ref: c2ray_base.py:460; a dozen launches per step) would pay every step for 0.3 ms saved.  So: aligned from the first
    // call on until the radius changes for the first time, afterwards only once a radius has served 32 calls in a row.
    // Decided ONCE PER CALL (note_call_radius, from fill_rt_params), never per launch: every range of a pipelined or chunked
    // call and every iteration of an evolve batch sees the same tables.
    {
        const int want = in.aligned_rows;
        const double r = std::min(in.R, 0.87 * in.N);
        const bool possible = (units == 6 || units == 12) && !in.dump && in.N % 8 == 0 && in.z_transposed && in.host_positions && r <= 110.0;
        sh.aligned = possible && (want == 2 || (want == 0 && r < 52.5 && in.radius_stays));
    }
    return sh;
}

// Stage 2: from stage 1 and the tables' S (last shell) and max_cells (largest shell)
struct RtPlan {
    RtForm form;               // skip_zero: the branching form only; what decide_skip_zero decides goes in through plan_skip_zero
    bool use_lds;              // the shell buffers fit LDS (else global memory, one launch at a time)
    bool zero_form_exists;     // a form that drops exact zeros at no cost exists for this launch
    size_t lds_bytes;
    size_t shell_bytes;        // per source: its two shell buffers
};

// The ASORA_VARIANT_* word of a launch.  (SKIP_ZERO reports the forms that drop the zeros' atomics; the branching form under
// global atomics has never been reported.)
inline int variant_word(const RtForm &f, int units, bool aligned)
{
    return (f.nsrc == 2 ? ASORA_VARIANT_PAIRED : 0) | (aligned ? ASORA_VARIANT_ALIGNED : 0) |
           (f.bufatom ? ASORA_VARIANT_BUFFER_ATOMICS : 0) | (f.split ? ASORA_VARIANT_SPLIT_DESCRIPTORS : 0) |
           (f.open ? ASORA_VARIANT_OPEN_BOUNDARIES : 0) |
           ((f.skip_zero && f.bufatom) ? ASORA_VARIANT_SKIP_ZERO : 0) | (f.global_scratch ? ASORA_VARIANT_GLOBAL_SHELLS : 0) | (units << 8) | (f.threads << 16);
}
// the sub-box sweep's form: table rates through buffer atomics, 256-entry tables, shells in LDS
constexpr RtForm subbox_form(int threads, bool heat, int nsrc) { return RtForm{threads, false, false, heat, 256, false, false, true, nsrc, true, false, true, false}; }
inline size_t form_lds_bytes(const RtForm &f, int max_cells)
{
    return (f.global_scratch ? 0 : (size_t)f.nsrc * shell_pair_bytes(max_cells)) + lds_table_bytes(f.tabcap, f.nsrc);
}
// workgroups of a launch: `groups` per unit; few of them are spread, a source's units over the XCDs (RtParams::spread)
inline unsigned launch_grid(int groups, int units, int cu_count, int &spread)
{
    spread = (long)groups * units <= 2L * cu_count ? 1 : 0;
    return spread ? (unsigned)units * (unsigned)groups : 8u * (unsigned)units * (unsigned)((groups + 7) / 8);
}

// Who shares a workgroup with whom when the tables are the aligned kind (build_unit_geometry, align_class): two sources
// that agree modulo 8 in k (units of the x- and y-sector: face type 0) or in i (units of the z-sector: face type 1).  The list is
// walked in its order -- position-sorted for a whole-list call -- and a source waits for the next one of its class, so partners are
// neighbours in the list, hence in space; what is left over at the end sweeps alone (y = -1).  cls: the class of each pair.
struct SrcPair { int x, y; };
inline void pairs_by_class(const int32_t *host_pos, int begin, int count, int face_type, std::vector<SrcPair> &pairs, std::vector<int> &cls)
{
    const int axis = face_type ? 0 : 2;
    pairs.clear(); cls.clear();
    pairs.reserve((size_t)count / 2 + 8);
    int open[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    for (int s = begin; s < begin + count; ++s) {
        const int c = host_pos[3 * (size_t)s + axis] & 7;
        if (open[c] < 0) open[c] = s;
        else { pairs.push_back(SrcPair{open[c], s}); cls.push_back(c); open[c] = -1; }
    }
    for (int c = 0; c < 8; ++c) if (open[c] >= 0) { pairs.push_back(SrcPair{open[c], -1}); cls.push_back(c); }
}

// The face of unit u of a source cut into `units` (ensure_geometry): 0 x, 1 y, 2 z, -1 for units that hold cells of every face
inline int unit_face(int units, int u)
{
    return units == 6 ? u >> 1 : units == 12 ? u >> 2 : units == 3 ? u : units == 24 ? u >> 3 : units == 96 ? (u % 24) >> 3 : -1;
}
// Which (group, unit) a block index stands for, where the arithmetic map of the kernel's prologue is not used: block b sweeps entry b
// of `order`, {group, unit} or {-1, -1} for padding.  A group is what one workgroup sweeps per unit (a pair of the class lists, two
// consecutive sources, or one source).  Blocks b and b + 8 share an XCD, so blocks b & 7 = x form the "lane" of XCD x, and a lane is
// dealt TABLE-MAJOR: per unit (in dispatch order) the groups of the unit's face type are ordered stably by their table class and cut
// into 8 contiguous slices whose sizes differ by at most 1; lane x sweeps its slice of the first unit, then of the second, ...  A
// slice spans one or two classes (more only where a class holds fewer groups than a slice), so the workgroups resident on an XCD read
// one or two tables, four across a unit boundary, and those stay in its L2.
//   dispatch[d]: the unit dispatched d-th (largest first); face_type[u]: 1 for a z-sector unit, else 0;
//   ngroups[ft], cls[ft][g]: the groups of face type ft and the table class of each (cls[ft] == nullptr: all one class).
// Returns the grid: 8 x the longest lane.
inline unsigned block_order(int units, const int *dispatch, const int *face_type, const int ngroups[2], const int *const cls[2],
                            std::vector<int32_t> &order)
{
    std::vector<int> sorted[2];
    for (int ft = 0; ft < 2; ++ft) {
        sorted[ft].resize((size_t)std::max(ngroups[ft], 0));
        for (int g = 0; g < ngroups[ft]; ++g) sorted[ft][(size_t)g] = g;
        if (cls[ft]) std::stable_sort(sorted[ft].begin(), sorted[ft].end(), [&](int a, int b) { return cls[ft][a] < cls[ft][b]; });
    }
    auto cut = [](int n, int x) { return (int)((long long)n * x / 8); };       // slice x of n groups: [cut(n, x), cut(n, x + 1))
    size_t len = 0;
    for (int x = 0; x < 8; ++x) {
        size_t l = 0;
        for (int d = 0; d < units; ++d) { const int n = ngroups[face_type[dispatch[d]]]; l += (size_t)(cut(n, x + 1) - cut(n, x)); }
        len = std::max(len, l);
    }
    order.assign(16 * len, -1);
    for (int x = 0; x < 8; ++x) {
        size_t t = 0;
        for (int d = 0; d < units; ++d) {
            const int u = dispatch[d], ft = face_type[u], n = ngroups[ft];
            for (int k = cut(n, x); k < cut(n, x + 1); ++k, ++t) {
                order[2 * (8 * t + (size_t)x)] = sorted[ft][(size_t)k];
                order[2 * (8 * t + (size_t)x) + 1] = u;
            }
        }
    }
    return (unsigned)(8 * len);
}

// ... of a launch of `count` sources from `begin`: units dispatched largest first (the z-sector units hold the most cells: unit
// units - 1 first); groups = the pairs of the class lists (pairs && aligned: npairs, pair_cls from pairs_by_class), two consecutive
// sources (pairs), or single sources, whose class is their own where the tables are aligned
inline unsigned launch_block_order(const int32_t *host_pos, int begin, int count, int units, const int *face_type, bool pairs, bool aligned,
                                   const int npairs[2], const int *const pair_cls[2], std::vector<int32_t> &order)
{
    std::vector<int> dispatch((size_t)units), own[2];
    for (int d = 0; d < units; ++d) dispatch[(size_t)d] = units - 1 - d;
    int n[2] = {pairs ? (count + 1) / 2 : count, pairs ? (count + 1) / 2 : count};
    const int *cls[2] = {nullptr, nullptr};
    if (pairs && aligned) {
        for (int ft = 0; ft < 2; ++ft) { n[ft] = npairs[ft]; cls[ft] = pair_cls[ft]; }
    } else if (aligned) {
        for (int ft = 0; ft < 2; ++ft) {
            own[ft].resize((size_t)count);
            for (int g = 0; g < count; ++g) own[ft][(size_t)g] = host_pos[3 * (size_t)(begin + g) + (ft ? 0 : 2)] & 7;
            cls[ft] = own[ft].data();
        }
    }
    return block_order(units, dispatch.data(), face_type, n, cls, order);
}

// returns 0, or the launcher's error code with its message in `why`
inline int plan_launch(const RtPlanInput &in, const RtShape &sh, int S, int max_cells, RtPlan &out, std::string &why)
{
    const int units = sh.units, threads = sh.threads;
    const bool open = in.open, dump = in.dump, heat = in.heat, grey = in.grey;
    // small tables (log table, 1/s, three wrapped-coordinate tables) at fixed capacity, then the shell buffers
    const bool big_tables = S + 1 > 256;
    const bool small_tables = !open && S + 1 <= 64 && threads <= 128;
    if (S + 1 > 1024) { why = "raytrace: more than 1023 shells (mesh too large for this build)"; return 4; }
    const size_t fixed_bytes = lds_table_bytes(big_tables ? 1024 : small_tables ? 64 : 256);
    const size_t shell_bytes = shell_pair_bytes(max_cells);
    const bool use_lds = shell_bytes + fixed_bytes <= LDS_LIMIT_BYTES;
    bool split = false;
    // (beyond N = 512: per-layout descriptors also for the single-source form with heating or grey opacity, round 6)
    const bool bufatom_fits = buffer_atomics_fit(in, units, threads, use_lds && !dump && !big_tables, split);
    // Two sources per workgroup (see the kernel's NSRC): the variant exists for table rates without heating, column-density
    // dump or exact-zero skipping, with the shell buffers in LDS and the rates through buffer atomics, for 64..512 threads
    // and the two smaller LDS table capacities
    bool pairs = false;
    {
        const int want = in.pair_sources;
        const bool possible = use_lds && !dump && !heat && !grey && !big_tables && threads <= 512 &&
                              bufatom_fits && in.src_count >= 2 &&
                              2 * shell_bytes + lds_table_bytes(open ? 256 : (S + 1 <= 32 && threads == 256) ? 32 : (S + 1 <= 64 && threads <= 256) ? 64 : 256, 2) <= LDS_LIMIT_BYTES;
        pairs = possible && (want == 2 || (want == 0 && pair_sources_pays(in, units, threads)));
    }
    const bool pairs_small = !open && S + 1 <= 64 && threads <= 256;      // the paired variant has the 64-entry tables for 256 threads too
    // ... and 32-entry ones for 256 threads: at r_RT = 30 the 1.75 KB they save are what separates two workgroups per CU from
    // three (four shell buffers of 11.6 KB + tables: 53.9 KB against 52.2 KB; three per CU fit up to 53.3 KB; worth ~4 %)
    const bool pairs_tiny = !open && S + 1 <= 32 && threads == 256;

    const int tabcap = pairs ? (pairs_tiny ? 32 : pairs_small ? 64 : 256) : big_tables ? 1024 : small_tables ? 64 : 256;
    // rate atomics through buffer descriptors (see the kernel's BUFATOM): decided here, once
    const bool bufatom = bufatom_fits && (use_lds || open) && !dump;
    // ASORA_OPT_SKIP_ZERO_RATES = 1 where the buffer-atomic kernel (which drops exact zeros by itself) is not available: the
    // branching variant that leaves them out
    const bool branching = use_lds && !bufatom && !dump && !grey && !heat && in.tau_zero_finite && in.skip_zero_rates == 1;
    // (the grey and the dump forms have no heating; SPLIT without table sets per source: the form that does not read them -- see the kernel's SPEC)
    const RtForm &f = out.form = RtForm{threads, !use_lds, dump, heat && !grey && !dump, tabcap, branching, grey, bufatom, pairs ? 2 : 1, false, split,
                                        !(pairs && split && !in.table_sets), open};
    out.use_lds = use_lds;
    // (open boundaries: the forms that add exact zeros only)
    out.zero_form_exists = use_lds && !dump && !heat && !grey && in.tau_zero_finite && bufatom_fits && !open;
    out.shell_bytes = shell_bytes;
    out.lds_bytes = form_lds_bytes(f, max_cells);
    return 0;
}
// what decide_skip_zero decided for a launch whose zero_form_exists
inline void plan_skip_zero(RtPlan &plan, bool skip_zero) { if (skip_zero) plan.form.skip_zero = true; }

} // namespace asora
