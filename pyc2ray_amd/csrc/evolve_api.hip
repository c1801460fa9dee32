// evolve_api.hip -- the evolve loop on the device (asora_evolve_*): on one GPU, and with the sources sharded over several
// (the slab calls).  Both forms share the step's prologue (evolve_begin_impl), the two accumulator pairs and the parameter
// block of the fused pass (evolve_pass_params).
#include "asora_internal.hpp"

namespace asora {

// The two accumulator pairs (State::acc; State::thermal.heat_acc in thermal mode): pair `set` is 2 N^3 doubles, [i][j][k] then [k][j][i].
// Iteration k of a step traces into pair (evolve.base + k - 1) & 1, and its pass zeroes the other one.
static double *acc_pair(int set) { return state().acc + (size_t)set * 2 * state().ncell; }
static double *heat_pair(int set) { return state().thermal.heat_acc + (size_t)set * 2 * state().ncell; }

static int ensure_heat_acc()
{
    State &st = state();
    if (st.thermal.heat_acc) return 0;
    if (int rc = st.thermal.heat_acc.allocate(4 * st.ncell)) return rc;
    ASORA_HIP_TRY(hipMemsetAsync(st.thermal.heat_acc, 0, 4 * st.ncell * sizeof(double), st.stream));
    st.thermal.mode.heat_clean[0] = st.thermal.mode.heat_clean[1] = true;
    return 0;
}

// Make both pairs all zero, without storing where that is known already.  The rate pairs are zeroed in one piece (raytracing.cu:113)
// and count as dirty when iterations were enqueued and never polled: which pair holds what is then not known.  heating: the
// heating pairs instead, pair by pair (after a poll one of them is clean).
static int zero_pairs_unless_clean(bool heating = false)
{
    State &st = state();
    const size_t pair_bytes = 2 * st.ncell * sizeof(double);
    if (heating) {
        for (int q = 0; q < 2; ++q)
            if (!st.thermal.mode.heat_clean[q]) {
                ASORA_HIP_TRY(hipMemsetAsync(heat_pair(q), 0, pair_bytes, st.stream));
                st.thermal.mode.heat_clean[q] = true;
            }
        return 0;
    }
    if (!st.evolve.flags.sets_known) { st.evolve.flags.clean[0] = st.evolve.flags.clean[1] = false; st.evolve.flags.sets_known = true; }
    if (st.evolve.flags.clean[0] && st.evolve.flags.clean[1]) return 0;
    ASORA_HIP_TRY(hipMemsetAsync(acc_pair(0), 0, 2 * pair_bytes, st.stream));
    st.evolve.flags.clean[0] = st.evolve.flags.clean[1] = true;
    return 0;
}

// Which lines of the accumulators this step's sources can touch (State::reach): rebuilt when the sources, their range
// or the radius change, and USED while at least 45 % of the lines are out of reach (counted then).  Measured at 256^3 with 1000
// sources (profiles/r04_ab_reach_mask.txt): r_RT = 8 (20 % of the lines reached) pass -12 ... -19 %, 12 (46 %) -3 ... -7 %,
// 16 (74 %) +2 ... +5 %, 32 (100 %) +10 %: where the spheres cover the box the two mask bytes per cell only cost -- none of the
// BASELINE configurations gains, sparse runs (few sources, small radii) do.  Whenever the set of lines the
// passes zero changes, BOTH pairs are zeroed once: the dirty pair of the previous step may hold rates where the new
// sources do not reach.  Not for traces that cover (nearly) the whole box, nor with ASORA_REACH_MASK=0 (2: whenever built).
// Leaves State::reach.d.in_use set for the step (one GPU; a sharded step uses no mask).
// faces: the step has plane-parallel fluxes (asora_plane_flux), which reach every line -- no mask; going from a mask to none
// zeroes both pairs like any other change of the set of lines.
static int decide_reach_mask(int src_begin, int src_count, double R, bool faces)
{
    State &st = state();
    State::ReachMask::Decision &rm = st.reach.d;
    static const int mode = []() { const char *v = getenv("ASORA_REACH_MASK"); return v ? atoi(v) : 1; }();
    const bool possible = !faces && mode != 0 && std::isfinite(R) && 2.0 * R + 2.0 < (double)st.N && st.opt[ASORA_OPT_Z_TRANSPOSED] != 0;
    const State::ReachMask::Decision::Key now{true, st.src_generation, src_begin, src_count, R};
    const bool same = rm.key == now;
    // where the spheres together hold more cells than the box, (nearly) every line is reached: the mask can not pay and is
    // not built (in a cosmological run R changes every step, and every build ends with a blocking read-back)
    // (forced use, ASORA_REACH_MASK=2, always builds it: a mask in use must be the mask of THIS source set and radius)
    const bool covers = possible && mode != 2 && (double)src_count * (4.0 / 3.0) * 3.14159265358979 * R * R * R >= (double)st.ncell;
    if (possible && !same) {
        if (covers) rm.pays = false;
        else {
            const size_t one = (size_t)st.N * st.N * ((st.N + 7) / 8);
            if (int rc = st.reach.mask.allocate(2 * one)) return rc;
            if (int rc = st.reach.count_dev.allocate(1)) return rc;
            if (int rc = launch_reach_mask(st, st.sources.pos, src_begin, src_count, R, st.reach.mask, one)) return rc;
            if (int rc = launch_reach_count(st, st.reach.mask, 2 * one, st.reach.count_dev)) return rc;
            unsigned long long marked = 0;
            ASORA_HIP_TRY(hipMemcpyAsync(&marked, st.reach.count_dev, sizeof marked, hipMemcpyDeviceToHost, st.stream));
            ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
            rm.pays = (double)marked <= 0.55 * (double)(2 * one);
        }
        rm.key = now;
    }
    const bool wanted = possible && (rm.pays || mode == 2);
    if ((wanted && !same) || (wanted != rm.in_use))      // the set of lines the passes zero changes: start from zeroed pairs
        if (int rc = zero_pairs_unless_clean()) return rc;
    rm.in_use = wanted;
    return 0;
}

// The parameter block of a fused pass of the device loop over the planes [i_begin, i_begin + i_count): it reads the rates of
// pair `set`, zeroes the other pair for the next trace, forms the next nHI and is gated by the step's status block.  What
// only one form of the loop has is the caller's: the reach mask and the thermal block (one GPU), the out-box as the source
// of the rates and the rank-local sums (sharded).
static ChemTileParams evolve_pass_params(int i_begin, int i_count, int set)
{
    State &st = state();
    ChemTileParams c = chem_tile_common(i_begin, i_count, st.evolve.chem);
    c.xh_av_in = st.evolve.first ? st.grid[ASORA_GRID_XH] : st.grid[ASORA_GRID_XH_AV];
    c.gamma = acc_pair(set); c.gamma_t = c.gamma + st.ncell;
    c.zero_a = acc_pair(set ^ 1); c.zero_t = c.zero_a + st.ncell;
    c.nhi = st.nhi; c.nhi_t = st.nhi_t;
    c.status = st.evolve.status;
    c.fold = true; c.emit = true;
    return c;
}

// The thermal block of such a pass (one GPU, and the sharded step begun with asora_evolve_begin_slab_thermal): the heating pair of
// `set` is folded like the rates, the other heating pair zeroed, the end-of-step temperature and the substep counters written
static void evolve_pass_thermal(ChemTileParams &c, int set)
{
    State &st = state();
    c.thermal = true; c.uniform = 0; c.th = st.thermal.mode.consts;
    c.heat = heat_pair(set); c.heat_t = c.heat + st.ncell;
    c.zero_ha = heat_pair(set ^ 1); c.zero_ht = c.zero_ha + st.ncell;
    c.temp_end = st.grid[ASORA_GRID_TEMP_END]; c.th_stats = st.thermal.stats_dev;
}

} // namespace asora

using namespace asora;

extern "C" {

// ---------------------------------------------------------------------------------------------
// The evolve loop on the device (pyc2ray/evolve.py:168-240): raytrace -> fused chemistry -> convergence test,
// nothing in between and nothing on the host
// ---------------------------------------------------------------------------------------------
static int evolve_begin_impl(double dt, double bh00, double albpow, double colh0, double temph0, double abu_c,
                             double R, double sig, double dr, double minlogtau, double dlogtau, int NumTau,
                             int src_begin, int src_count, double conv_criterion, double convergence_fraction,
                             bool slab, int own_begin, int own_count, bool slab_thermal = false)
{
    clear_error();
    if (int rc = require_init("evolve_begin")) return rc;
    State &st = state();
    st.evolve.flags.open = false;
    // 1. what the step needs
    if (slab && st.thermal.mode.on && !slab_thermal)
        return fail(4, "evolve_begin_slab: thermal mode is on, and this entry begins an isothermal step (single-GPU thermal loop: "
                       "asora_evolve_begin; across ranks, with the heating rates exchanged as well: asora_evolve_begin_slab_thermal)");
    if (slab_thermal && (!st.sources.loaded.heat_tables || st.opt[ASORA_OPT_GREY_NOTABLES]))
        return fail(4, "evolve_begin_slab_thermal: needs heating tables on the device (heat_table_to_device)");
    if (slab_thermal && !st.thermal.mode.on)
        return fail(4, "evolve_begin_slab_thermal: needs the thermal mode (asora_thermal_params(1, ...) first)");
    if (slab) {
        if (int rc = check_planes("evolve_begin_slab", 4, "bad range of own planes", own_begin, own_count)) return rc;
        if (!st.opt[ASORA_OPT_Z_TRANSPOSED]) return fail(4, "evolve_begin_slab: needs the [k][j][i] twins (ASORA_OPT_Z_TRANSPOSED = 1)");
    }
    if (int rc = require_grids("evolve_begin", {ASORA_GRID_NDENS, ASORA_GRID_TEMP, ASORA_GRID_XH})) return rc;
    if (int rc = require_raytrace_inputs("evolve_begin", R, NumTau, false, false)) return rc;
    if (int rc = check_sources("evolve_begin", 4, "source range outside the " + std::to_string(st.sources.loaded.num) + " uploaded sources", src_begin, src_count)) return rc;
    if (st.opt[ASORA_OPT_HEATING]) return fail(4, "evolve_begin: the fused loop carries no heating rates (use raytrace_device)");
    if (st.thermal.mode.on) {
        if (!st.sources.loaded.heat_tables || st.opt[ASORA_OPT_GREY_NOTABLES])
            return fail(4, "evolve_begin: thermal mode needs heating tables on the device (heat_table_to_device)");
        if (!st.opt[ASORA_OPT_Z_TRANSPOSED]) return fail(4, "evolve_begin: thermal mode needs the [k][j][i] twins (ASORA_OPT_Z_TRANSPOSED = 1)");
        if (int rc = ensure_optional_grid(ASORA_GRID_PHI_HEAT)) return rc;
        if (int rc = ensure_optional_grid(ASORA_GRID_TEMP_END)) return rc;
        if (int rc = ensure_heat_acc()) return rc;
        // the heating out-box of a thermal step across ranks: N^3 doubles like the rate out-box (State::staging), with the first such step
        if (slab) { if (int rc = st.thermal.heat_outbox.allocate(st.ncell)) return rc; }
    }
    if (int rc = check_plane_flux(st, st.medium.plane, "evolve_begin", false, st.thermal.mode.on)) return rc;
    // a face's sweep rates every plane, and a step that owns only some of them folds out, sends and zeroes only the planes its
    // sources reach: the rates on the other foreign planes would never arrive and would pile up from iteration to iteration
    if (slab && st.medium.plane.count > 0 && !(own_begin == 0 && own_count == st.N))
        return fail(4, "evolve_begin_slab: a plane-parallel flux (asora_plane_flux) needs a step that owns every plane (the full-grid "
                       "exchange, asora_evolve_slab_fold_all): the slab exchange does not deliver a whole-box sweep");
    if (int rc = ensure_temp_probe(bh00, albpow, colh0, temph0)) return rc;

    // 2. which lines of the accumulators the passes sweep.  The first trace needs a zeroed pair; every fused pass zeroes the
    // pair the next trace adds into, iterations beyond convergence touch nothing.
    // multi-GPU: the pass sweeps the own planes only and the out-box folds zero the foreign ones (asora_evolve_slab_fold_out);
    // which planes those are changes with the plan, so a step simply starts from two zeroed pairs (256 MiB of stores at
    // 256^3, once per time step), and no reach mask
    if (!st.evolve.flags.sets_known || slab)
        if (int rc = zero_pairs_unless_clean()) return rc;
    if (slab) st.reach.d.in_use = false;
    else if (int rc = decide_reach_mask(src_begin, src_count, R, st.medium.plane.count > 0)) return rc;

    // 3. the accumulators and the status block of the step
    if (!st.evolve.flags.clean[0] && !st.evolve.flags.clean[1]) return fail(11, "evolve_begin: no clean accumulator pair (internal error)");
    st.evolve.base = st.evolve.flags.clean[0] ? 0 : 1;
    if (st.thermal.mode.on) {
        // the heating pairs start every thermal step all zero (the pass zeroes only the lines the step's sources reach)
        if (int rc = zero_pairs_unless_clean(true)) return rc;
        ASORA_HIP_TRY(hipMemsetAsync(st.thermal.stats_dev, 0, 3 * sizeof(unsigned long long), st.stream));
    }
    st.evolve.folded_iter = 0;
    if (int rc = st.evolve.status.allocate(1)) return rc;
    if (int rc = st.evolve.host.allocate(1)) return rc;
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));            // evolve.host may still be the target of an earlier poll
    std::memset(st.evolve.host, 0, sizeof(EvolveStatus));
    st.evolve.host->prev1 = 2.0 * (double)st.ncell;                // evolve.py:130-131
    st.evolve.host->prev0 = 2.0 * (double)st.ncell;
    st.evolve.host->conv_criterion = conv_criterion;
    st.evolve.host->conv_fraction = convergence_fraction;
    ASORA_HIP_TRY(hipMemcpyAsync(st.evolve.status, st.evolve.host, sizeof(EvolveStatus), hipMemcpyHostToDevice, st.stream));
    if (int rc = reset_counters()) return rc;
    // xh_av = copy(xh) (evolve.py:136) is not materialised: nHI of the first trace is formed from xh and the first
    // chemistry pass takes xh as its starting xh_av; xh_intermed (evolve.py:137) is only ever written
    if (int rc = launch_prepare_nhi_from(st, st.grid[ASORA_GRID_XH], st.opt[ASORA_OPT_Z_TRANSPOSED] != 0)) return rc;

    // 4. the step's parameters
    fill_rt_params(st.evolve.rt, R, sig, dr, minlogtau, dlogtau, NumTau);
    st.evolve.rt.phi = acc_pair(st.evolve.base);       // (each iteration sets its own pair, asora_evolve_enqueue)
    st.evolve.rt.done_flag = &st.evolve.status->done;
    st.evolve.rt.src_begin = src_begin; st.evolve.rt.src_count = src_count; st.evolve.rt.shape_src_count = src_count;
    if (src_begin == 0 && src_count == st.sources.loaded.num && st.sources.pos_sorted) use_source_list(st.evolve.rt, st, true);
    st.evolve.src_begin = src_begin; st.evolve.src_count = src_count;
    st.evolve.chem[0] = dt; st.evolve.chem[1] = bh00; st.evolve.chem[2] = albpow; st.evolve.chem[3] = colh0; st.evolve.chem[4] = temph0;
    st.evolve.chem[5] = abu_c;
    st.evolve.first = true;
    st.evolve.reported = 0;
    st.evolve.enqueued = 0;
    st.evolve.slab = slab; st.evolve.own_begin = own_begin; st.evolve.own_count = own_count; st.evolve.slab_passed = false;
    st.evolve.slab_thermal = slab && st.thermal.mode.on;
    st.evolve.rates_in_outbox = false; st.evolve.folded_all = false;
    st.evolve.plane_swept = false;
    st.evolve.flags.open = true;
    return 0;
}

int asora_evolve_begin(double dt, double bh00, double albpow, double colh0, double temph0, double abu_c,
                       double R, double sig, double dr, double minlogtau, double dlogtau, int NumTau,
                       int src_begin, int src_count, double conv_criterion, double convergence_fraction)
{
    return evolve_begin_impl(dt, bh00, albpow, colh0, temph0, abu_c, R, sig, dr, minlogtau, dlogtau, NumTau, src_begin, src_count,
                             conv_criterion, convergence_fraction, false, 0, 0);
}

// ---------------------------------------------------------------------------------------------
// The same loop when the sources are sharded over several GPUs (pyc2ray/evolve.py:249-498; pyc2ray_amd/dist.py SlabPlan): a
// rank traces ITS sources, owns the chemistry of ITS planes, and one iteration is the sequence
//   asora_evolve_slab_trace      (once, or per chunk of sources)     -> rates into the iteration's accumulator pair
//   asora_evolve_slab_fold_out   per run of foreign planes           -> out-box planes to send; the other pair zeroed there
//   asora_evolve_slab_add        per run received from another rank  -> added to the own planes of the pair
//   asora_evolve_slab_pass                                            -> the fused pass of the one-GPU loop on the own planes
//   asora_evolve_slab_nhi        per run of xh_av received           -> nHI of the halo planes for the next trace
//   asora_evolve_slab_close                                           -> convergence test on the sums over all ranks
// all asynchronous on the library's stream and all gated by the status block's `done`, so that -- as on one GPU -- a caller
// enqueues several iterations and reads the status back once (asora_evolve_poll; it folds the own rates into PHI_ION).
// ---------------------------------------------------------------------------------------------
int asora_evolve_begin_slab(double dt, double bh00, double albpow, double colh0, double temph0, double abu_c,
                            double R, double sig, double dr, double minlogtau, double dlogtau, int NumTau,
                            int src_begin, int src_count, double conv_criterion, double convergence_fraction,
                            int own_begin, int own_count)
{
    return evolve_begin_impl(dt, bh00, albpow, colh0, temph0, abu_c, R, sig, dr, minlogtau, dlogtau, NumTau, src_begin, src_count,
                             conv_criterion, convergence_fraction, true, own_begin, own_count);
}

// The same step in thermal mode (asora_thermal_params(1, ...), heating tables, the [k][j][i] twins: code 4 without).  Beginning
// through this entry is how a caller declares that it exchanges the heating rates with the photo-ionisation rates: every slab call
// then carries both fields (trace, fold_out, fold_all, pass, poll), and what arrives from other ranks is added with
// asora_evolve_slab_add (rates) AND asora_evolve_slab_add_heat (heating), from asora_evolve_slab_heat_outbox() on the sender's side.
int asora_evolve_begin_slab_thermal(double dt, double bh00, double albpow, double colh0, double temph0, double abu_c,
                                    double R, double sig, double dr, double minlogtau, double dlogtau, int NumTau,
                                    int src_begin, int src_count, double conv_criterion, double convergence_fraction,
                                    int own_begin, int own_count)
{
    return evolve_begin_impl(dt, bh00, albpow, colh0, temph0, abu_c, R, sig, dr, minlogtau, dlogtau, NumTau, src_begin, src_count,
                             conv_criterion, convergence_fraction, true, own_begin, own_count, true);
}

static int require_slab(const char *who)
{
    if (int rc = require_init(who)) return rc;
    if (!state().evolve.flags.open || !state().evolve.slab)
        return fail(4, std::string(who) + ": no multi-GPU evolve step in progress (call asora_evolve_begin_slab)");
    if (state().evolve.enqueued - state().evolve.reported + 1 > EVOLVE_HIST)
        return fail(4, std::string(who) + ": " + std::to_string(EVOLVE_HIST) + " iterations enqueued since the last asora_evolve_poll (poll first)");
    return 0;
}
static int slab_set() { return (state().evolve.base + state().evolve.enqueued) & 1; }     // the pair the current iteration traces into
static double *slab_pair(int which) { return acc_pair(slab_set() ^ which); }     // 0: that pair, 1: the other one
static double *slab_heat_pair(int which) { return heat_pair(slab_set() ^ which); }
static int require_slab_thermal(const char *who)
{
    if (int rc = require_slab(who)) return rc;
    if (!state().evolve.slab_thermal)
        return fail(4, std::string(who) + ": the step carries no heating rates (begin it with asora_evolve_begin_slab_thermal)");
    return 0;
}

int asora_evolve_slab_trace(int src_begin, int src_count)
{
    clear_error();
    if (int rc = require_slab("evolve_slab_trace")) return rc;
    State &st = state();
    if (st.evolve.slab_passed) return fail(4, "evolve_slab_trace: the iteration's pass has been enqueued already (close it first)");
    if (src_begin < st.evolve.src_begin || src_count < 0 || src_begin + src_count > st.evolve.src_begin + st.evolve.src_count)
        return fail(4, "evolve_slab_trace: source range outside the step's sources");
    if (st.evolve.rt.plane.count > 0 && !st.evolve.plane_swept) {      // the faces' sweeps: once per iteration, ahead of its first trace
        st.evolve.flags.sets_known = false;
        if (st.evolve.slab_thermal) st.thermal.mode.heat_clean[0] = st.thermal.mode.heat_clean[1] = false;
        if (int rc = launch_plane_flux(st, st.evolve.rt, slab_pair(0), st.evolve.slab_thermal ? slab_heat_pair(0) : nullptr, st.evolve.slab_thermal,
                                       &st.evolve.status->done)) return rc;
        st.evolve.plane_swept = true;
    }
    if (src_count == 0) return 0;
    st.evolve.flags.sets_known = false;
    RtParams p = st.evolve.rt;
    p.phi = slab_pair(0);
    p.src_begin = src_begin; p.src_count = src_count;          // (shape_src_count stays the rank's whole share: one launch shape)
    if (!(src_begin == 0 && src_count == st.sources.loaded.num)) use_source_list(p, st, false);
    if (st.evolve.slab_thermal) {                 // the HEAT forms, into the iteration's heating pair
        p.heat = slab_heat_pair(0);
        st.thermal.mode.heat_clean[0] = st.thermal.mode.heat_clean[1] = false;
    }
    return launch_raytrace(st, p, false, st.evolve.slab_thermal);
}

int asora_evolve_slab_fold_out(int i_begin, int i_count)
{
    clear_error();
    if (int rc = require_slab("evolve_slab_fold_out")) return rc;
    State &st = state();
    if (int rc = check_planes("evolve_slab_fold_out", 4, "bad plane range", i_begin, i_count)) return rc;
    if (i_count > 0 && i_begin < st.evolve.own_begin + st.evolve.own_count && st.evolve.own_begin < i_begin + i_count)
        return fail(4, "evolve_slab_fold_out: the range holds planes this rank owns (their rates stay: the pass folds them)");
    st.evolve.flags.sets_known = false;
    double *cur = slab_pair(0), *nxt = slab_pair(1);
    if (st.evolve.slab_thermal) {                 // both fields in one launch
        double *hcur = slab_heat_pair(0), *hnxt = slab_heat_pair(1);
        return launch_fold_out_pair(st, cur, cur + st.ncell, st.staging, nxt, nxt + st.ncell, hcur, hcur + st.ncell, st.thermal.heat_outbox,
                                    hnxt, hnxt + st.ncell, i_begin, i_count, &st.evolve.status->done);
    }
    return launch_fold_out(st, cur, cur + st.ncell, st.staging, nxt, nxt + st.ncell, i_begin, i_count, &st.evolve.status->done);
}

// The full-grid exchange (pyc2ray/evolve.py:433-437: every rank all-reduces the rate grid) on the same loop: ALL planes folded
// into the out-box, which the caller then sums over the ranks in place; the pass reads the out-box (one layout, nothing left to
// fold) and keeps the summed rates in PHI_ION itself.  (An all-reduce is not gated by `done`: iterations enqueued beyond convergence
// sum the stale out-box once more.  The pass is gated, so PHI_ION keeps what the last iteration carried out has read.)
int asora_evolve_slab_fold_all(void)
{
    clear_error();
    if (int rc = require_slab("evolve_slab_fold_all")) return rc;
    State &st = state();
    if (st.evolve.slab_passed) return fail(4, "evolve_slab_fold_all: the iteration's pass has been enqueued already");
    if (st.evolve.own_begin != 0 || st.evolve.own_count != st.N)
        return fail(4, "evolve_slab_fold_all: the step must own every plane (asora_evolve_begin_slab(..., 0, N)): the chemistry is replicated");
    st.evolve.flags.sets_known = false;
    st.evolve.rates_in_outbox = true; st.evolve.folded_all = true;
    double *cur = slab_pair(0), *nxt = slab_pair(1);
    // (the pass zeroes the other pair's [i][j][k] layout as it goes; the transposed layout is zeroed here)
    if (st.evolve.slab_thermal) {
        double *hcur = slab_heat_pair(0), *hnxt = slab_heat_pair(1);
        return launch_fold_out_pair(st, cur, cur + st.ncell, st.staging, nullptr, nxt + st.ncell, hcur, hcur + st.ncell, st.thermal.heat_outbox,
                                    nullptr, hnxt + st.ncell, 0, st.N, &st.evolve.status->done);
    }
    return launch_fold_out(st, cur, cur + st.ncell, st.staging, nullptr, nxt + st.ncell, 0, st.N, &st.evolve.status->done);
}

void *asora_evolve_slab_outbox(void) { return state().init ? (void *)state().staging : nullptr; }
// (nullptr until a thermal step across ranks has been begun: the heating out-box is allocated then)
void *asora_evolve_slab_heat_outbox(void) { return state().init ? (void *)state().thermal.heat_outbox : nullptr; }

// planes [i_begin, i_begin + i_count) of an out-box (`box`: the rate out-box, or the heating out-box) from / to the host
static int outbox_copy(const char *who, double *box, int i_begin, int i_count, double *host, bool to_host)
{
    clear_error();
    if (int rc = require_init(who)) return rc;
    State &st = state();
    if (i_begin < 0 || i_count < 0 || i_begin + i_count > st.N || (i_count > 0 && !host)) return fail(3, std::string(who) + ": bad arguments");
    if (i_count == 0) return 0;
    if (!box) return fail(4, std::string(who) + ": no heating out-box (begin a step with asora_evolve_begin_slab_thermal)");
    const size_t plane = (size_t)st.N * st.N;
    double *dev = box + (size_t)i_begin * plane;
    if (to_host) ASORA_HIP_TRY(hipMemcpyAsync(host, dev, (size_t)i_count * plane * sizeof(double), hipMemcpyDeviceToHost, st.stream));
    else         ASORA_HIP_TRY(hipMemcpyAsync(dev, host, (size_t)i_count * plane * sizeof(double), hipMemcpyHostToDevice, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));              // (the host buffer may be pageable)
    return 0;
}

int asora_evolve_slab_outbox_from_host(int i_begin, int i_count, const double *host)
{
    return outbox_copy("evolve_slab_outbox_from_host", state().staging, i_begin, i_count, const_cast<double *>(host), false);
}

int asora_evolve_slab_outbox_to_host(int i_begin, int i_count, double *host)
{
    return outbox_copy("evolve_slab_outbox_to_host", state().staging, i_begin, i_count, host, true);
}

int asora_evolve_slab_heat_outbox_from_host(int i_begin, int i_count, const double *host)
{
    return outbox_copy("evolve_slab_heat_outbox_from_host", state().thermal.heat_outbox, i_begin, i_count, const_cast<double *>(host), false);
}

int asora_evolve_slab_heat_outbox_to_host(int i_begin, int i_count, double *host)
{
    return outbox_copy("evolve_slab_heat_outbox_to_host", state().thermal.heat_outbox, i_begin, i_count, host, true);
}

// planes received from another rank added on the own planes of the iteration's pair: heating = false the rates, true the heating
static int slab_add(const char *who, bool heating, int i_begin, int i_count, const double *dev_planes)
{
    clear_error();
    if (int rc = heating ? require_slab_thermal(who) : require_slab(who)) return rc;
    State &st = state();
    if (i_begin < 0 || i_count < 0 || i_begin + i_count > st.N || (i_count > 0 && !dev_planes)) return fail(4, std::string(who) + ": bad arguments");
    if (st.evolve.slab_passed) return fail(4, std::string(who) + ": the iteration's pass has been enqueued already");
    if (i_count > 0 && (i_begin < st.evolve.own_begin || i_begin + i_count > st.evolve.own_begin + st.evolve.own_count))
        return fail(4, std::string(who) + ": rates received for planes this rank does not own");
    st.evolve.flags.sets_known = false;
    const size_t plane = (size_t)st.N * st.N;
    double *pair = heating ? slab_heat_pair(0) : slab_pair(0);
    return launch_add_planes(st, pair + (size_t)i_begin * plane, dev_planes, (size_t)i_count * plane, &st.evolve.status->done);
}

static int slab_add_host(const char *who, bool heating, int i_begin, int i_count, const double *host_planes)
{
    clear_error();
    if (int rc = heating ? require_slab_thermal(who) : require_slab(who)) return rc;
    State &st = state();
    if (i_begin < 0 || i_count < 0 || i_begin + i_count > st.N || (i_count > 0 && !host_planes)) return fail(4, std::string(who) + ": bad arguments");
    if (i_count == 0) return 0;
    // through the out-box: what is added belongs to planes this rank owns, what the out-box holds to planes it does not
    const size_t plane = (size_t)st.N * st.N;
    double *tmp = (heating ? st.thermal.heat_outbox : st.staging) + (size_t)i_begin * plane;
    ASORA_HIP_TRY(hipMemcpyAsync(tmp, host_planes, (size_t)i_count * plane * sizeof(double), hipMemcpyHostToDevice, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));              // (the host buffer may be pageable)
    return slab_add(who, heating, i_begin, i_count, tmp);
}

int asora_evolve_slab_add(int i_begin, int i_count, const double *dev_planes)
{
    return slab_add("evolve_slab_add", false, i_begin, i_count, dev_planes);
}

int asora_evolve_slab_add_host(int i_begin, int i_count, const double *host_planes)
{
    return slab_add_host("evolve_slab_add_host", false, i_begin, i_count, host_planes);
}

int asora_evolve_slab_add_heat(int i_begin, int i_count, const double *dev_planes)
{
    return slab_add("evolve_slab_add_heat", true, i_begin, i_count, dev_planes);
}

int asora_evolve_slab_add_heat_host(int i_begin, int i_count, const double *host_planes)
{
    return slab_add_host("evolve_slab_add_heat_host", true, i_begin, i_count, host_planes);
}

int asora_evolve_slab_pass(void)
{
    clear_error();
    if (int rc = require_slab("evolve_slab_pass")) return rc;
    State &st = state();
    if (st.evolve.slab_passed) return fail(4, "evolve_slab_pass: already enqueued for this iteration");
    if (st.evolve.rates_in_outbox && !st.evolve.folded_all)
        return fail(4, "evolve_slab_pass: this step exchanges whole grids (asora_evolve_slab_fold_all), and this iteration's fold has not been enqueued");
    st.evolve.flags.sets_known = false;
    st.evolve.slab_passed = true;
    st.grid_valid[ASORA_GRID_XH_AV] = st.grid_valid[ASORA_GRID_XH_INTERMED] = true;
    st.grid_valid[ASORA_GRID_PHI_ION] = false;
    if (st.evolve.slab_thermal) {
        st.thermal.mode.heat_clean[0] = st.thermal.mode.heat_clean[1] = false;     // until the poll tells which pair the last iteration used
        st.grid_valid[ASORA_GRID_TEMP_END] = true;
        st.grid_valid[ASORA_GRID_PHI_HEAT] = false;
    }
    if (st.evolve.own_count == 0) {           // nothing to own (more ranks than planes): this rank's share of the sums is zero
        ASORA_HIP_TRY(hipMemsetAsync(st.red_final, 0, sizeof(double) * 3, st.stream));
        return 0;
    }
    if (int rc = ensure_red_capacity(3 * chemistry_tile_blocks(st, st.N, st.evolve.own_count))) return rc;    // (sized for every range at init)
    ChemTileParams c = evolve_pass_params(st.evolve.own_begin, st.evolve.own_count, slab_set());
    c.local_sums = true;
    if (st.evolve.slab_thermal) evolve_pass_thermal(c, slab_set());
    if (st.evolve.rates_in_outbox) {
        c.gamma = st.staging; c.gamma_t = nullptr; c.phi_out = st.grid[ASORA_GRID_PHI_ION]; c.fold = false;
        // (thermal: the summed heating likewise from its out-box, kept in PHI_HEAT)
        if (st.evolve.slab_thermal) { c.heat = st.thermal.heat_outbox; c.heat_t = nullptr; c.heat_out = st.grid[ASORA_GRID_PHI_HEAT]; }
    }
    return launch_chemistry_tiles(st, c, st.stream);
}

int asora_evolve_slab_nhi(int i_begin, int i_count)
{
    clear_error();
    if (int rc = require_slab("evolve_slab_nhi")) return rc;
    State &st = state();
    if (int rc = check_planes("evolve_slab_nhi", 4, "bad plane range", i_begin, i_count)) return rc;
    return launch_prepare_range(st, i_begin, i_count, false, nullptr, &st.evolve.status->done);
}

int asora_evolve_slab_close(const double *host_sums)
{
    clear_error();
    if (int rc = require_slab("evolve_slab_close")) return rc;
    State &st = state();
    if (!st.evolve.slab_passed) return fail(4, "evolve_slab_close: the iteration's pass has not been enqueued");
    if (host_sums) {          // summed over the ranks on the host (gloo rehearsals, mpi4py): {sum x, sum 1-x, conv_flag}
        ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
        std::memcpy(st.red_host, host_sums, sizeof(double) * 3);
        ASORA_HIP_TRY(hipMemcpyAsync(st.red_final, st.red_host, sizeof(double) * 3, hipMemcpyHostToDevice, st.stream));
    }
    if (int rc = launch_convergence_test(st, st.red_final, st.evolve.status)) return rc;
    st.evolve.first = false;
    st.evolve.slab_passed = false; st.evolve.folded_all = false;
    st.evolve.plane_swept = false;
    st.evolve.enqueued += 1;
    return 0;
}

int asora_evolve_enqueue(int iterations)
{
    clear_error();
    if (int rc = require_init("evolve_enqueue")) return rc;
    State &st = state();
    if (!st.evolve.flags.open) return fail(4, "evolve_enqueue: no evolve step in progress (call asora_evolve_begin)");
    if (st.evolve.slab) return fail(4, "evolve_enqueue: the step was begun with asora_evolve_begin_slab (use the asora_evolve_slab_* calls)");
    if (iterations < 1 || iterations > EVOLVE_HIST / 2) return fail(3, "evolve_enqueue: between 1 and 32 iterations per call");
    // the per-iteration history is a ring of EVOLVE_HIST rows on the device: rows not yet handed out by asora_evolve_poll
    // must not be overwritten
    if (st.evolve.enqueued - st.evolve.reported + iterations > EVOLVE_HIST)
        return fail(4, "evolve_enqueue: " + std::to_string(st.evolve.enqueued - st.evolve.reported) + " iterations enqueued since the last "
                           "asora_evolve_poll; the history ring holds " + std::to_string(EVOLVE_HIST) + " (poll first)");
    st.evolve.flags.sets_known = false;                        // until the next poll tells how many of these were carried out
    for (int it = 0; it < iterations; ++it) {
        // iteration k = ev_enqueued + it + 1 of the step (as long as the step has not converged: then nothing runs anyway)
        const int set = (st.evolve.base + st.evolve.enqueued + it) & 1;
        // the faces' sweeps (asora_plane_flux) into the iteration's pairs, ahead of the point sources; a step may have only faces
        if (int rc = launch_plane_flux(st, st.evolve.rt, acc_pair(set), st.thermal.mode.on ? heat_pair(set) : nullptr, st.thermal.mode.on, &st.evolve.status->done))
            return rc;
        if (st.evolve.src_count > 0) {
            RtParams p = st.evolve.rt;
            p.phi = acc_pair(set);
            if (st.thermal.mode.on) p.heat = heat_pair(set);    // thermal mode: the HEAT forms, into the iteration's heating pair
            if (int rc = launch_raytrace(st, p, false, st.thermal.mode.on)) return rc;
        }
        ChemTileParams c = evolve_pass_params(0, st.N, set);
        if (st.reach.d.in_use) { c.reach_a = st.reach.mask; c.reach_t = st.reach.mask + st.reach.mask.bytes() / 2; }
        if (st.thermal.mode.on) evolve_pass_thermal(c, set);
        if (int rc = launch_chemistry_tiles(st, c, st.stream)) return rc;
        st.evolve.first = false;
    }
    if (st.thermal.mode.on) {
        st.thermal.mode.heat_clean[0] = st.thermal.mode.heat_clean[1] = false;     // until the poll tells which pair the last iteration used
        st.grid_valid[ASORA_GRID_TEMP_END] = true;
        st.grid_valid[ASORA_GRID_PHI_HEAT] = false;
    }
    st.evolve.enqueued += iterations;
    st.grid_valid[ASORA_GRID_XH_AV] = st.grid_valid[ASORA_GRID_XH_INTERMED] = true;
    st.grid_valid[ASORA_GRID_PHI_ION] = false;       // until asora_evolve_poll folds the last iteration's accumulators
    return 0;
}

int asora_evolve_poll(int *niter, int *converged, double *history, int history_rows, int *rows_written)
{
    clear_error();
    if (int rc = require_init("evolve_poll")) return rc;
    State &st = state();
    if (!st.evolve.flags.open) return fail(4, "evolve_poll: no evolve step in progress (call asora_evolve_begin)");
    ASORA_HIP_TRY(hipMemcpyAsync(st.evolve.host, st.evolve.status, sizeof(EvolveStatus), hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    const EvolveStatus &h = *st.evolve.host;
    const bool thermal = st.evolve.slab ? st.evolve.slab_thermal : st.thermal.mode.on;
    // The rates of the last iteration carried out sit, unfolded, in its accumulator pair; the other pair is zero (the pass
    // of that iteration zeroed it; iterations enqueued beyond convergence did nothing).  Fold them into PHI_ION now.
    if (h.niter > 0) {
        const int set = (st.evolve.base + h.niter - 1) & 1;
        if (st.evolve.slab && st.evolve.rates_in_outbox) st.evolve.folded_iter = h.niter;      // (the pass has kept the summed rates in PHI_ION, and the heating in PHI_HEAT)
        if (st.evolve.folded_iter != h.niter) {
            const double *a = acc_pair(set);
            if (int rc = launch_fold_sum(st, a, a + st.ncell, st.grid[ASORA_GRID_PHI_ION])) return rc;
            if (thermal) {       // thermal mode: the last iteration's heating as well (a sharded step: complete on the own planes)
                const double *hsum = heat_pair(set);
                if (int rc = launch_fold_sum(st, hsum, hsum + st.ncell, st.grid[ASORA_GRID_PHI_HEAT])) return rc;
            }
            st.evolve.folded_iter = h.niter;
        }
        st.grid_valid[ASORA_GRID_PHI_ION] = true;
        st.evolve.flags.clean[set] = false; st.evolve.flags.clean[set ^ 1] = true;
        if (thermal) {
            st.grid_valid[ASORA_GRID_PHI_HEAT] = true;
            st.thermal.mode.heat_clean[set] = false; st.thermal.mode.heat_clean[set ^ 1] = true;
        }
    }
    st.evolve.flags.sets_known = true;
    int rows = 0;
    for (int it = st.evolve.reported; it < h.niter && history && rows < history_rows; ++it, ++rows)
        for (int q = 0; q < 5; ++q) history[5 * rows + q] = h.hist[it % EVOLVE_HIST][q];
    // everything enqueued has run by now (iterations enqueued beyond convergence did nothing and never will)
    st.evolve.enqueued = h.niter;
    if (history) st.evolve.reported += rows;
    else st.evolve.reported = h.niter;           // a caller that does not ask for the rows gives them up
    if (rows_written) *rows_written = rows;
    if (niter) *niter = h.niter;
    if (converged) *converged = h.done;
    return 0;
}

} // extern "C"
