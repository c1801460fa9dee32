"""GPU: one rank of the sharded device loop (asora_evolve_slab_*) in a world computed on the CPU, at meshes of several
32 x 32 tiles with cut tiles and cut 8-cell lines.

tests/slab_world.py plays a world of P ranks on the C oracle and records it; here the HIP library replays each rank of that
world in turn, in this one process: its incoming rate messages, the foreign XH_AV planes and the totals of the sums are the
recorded ones.  The GPU rank is compared with the CPU rank in its place (messages, consumed rates: 1e-8, the suite's bar for a
trace against the oracle, and the same zero pattern) and its pass with the C statement of the pass on the rates it read (1e-9,
the bar of test_global_pass_matches_reference) -- never with a one-process result: splitting the sum over ranks alone moves
XH_AV by up to 9e-12 here and 7e-10 in a less well-conditioned world (tests/test_slab_world_host.py).

What runs here and nowhere else in the suite: fold_out_kernel / fold_out_pair_kernel / add_planes_kernel on ranges that start
inside a tile and span more than one (blockIdx > 0), chemistry_tile_kernel over a plane range with i_begin != 0, i_end not
tile-aligned and rank-local sums, the same with several j per workgroup (jc < N), and the no-fold emit forms of the all-reduce
loop with several j per workgroup."""
import numpy as np
import pytest

import cases
import slab_world as W
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GAMMA_RTOL = 1e-8                   # tests/test_gpu_parity.py: a trace against the oracle
PASS_RTOL = 1e-9                    # tests/test_gpu_parity.py::test_global_pass_matches_reference
ITERS = 3                           # the third traces into the accumulator pair the second's fold_out / pass had to zero

WORLDS = W.WORLDS
_CACHE = {}


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _freeze(v)


def _world(name):
    """(case, record of the CPU world): computed once per name, shared, never written to."""
    if name not in _CACHE:
        c = W.make_case(**WORLDS[name])
        rec = W.cpu_world(c, ITERS, "allreduce" if name.startswith("C") else "slab")
        _freeze(c)
        _freeze(rec)
        _CACHE[name] = (c, rec)
    return _CACHE[name]


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib
    if p.cuda_is_init():
        lib.thermal_params(False)
        p.device_close()


def _fresh(p, c):
    if p.cuda_is_init():
        p.device_close()
    p.device_init(c["N"], 8)
    p.photo_table_to_device(c["thin"], c["thick"])


def _jc(N, planes):
    """Workgroups along j of the tiled pass over `planes` planes (chemistry.hip, tile_pass_grid) on this chip."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = ((N + 31) // 32) * ((planes + 31) // 32)
    return max(1, min(N, (16 * cus + tiles - 1) // tiles))


def _assert_rates(got, want, tag):
    assert np.array_equal(got != 0, want != 0), tag
    np.testing.assert_allclose(got, want, rtol=GAMMA_RTOL, atol=0, err_msg=tag)


def _assert_pass(c, sl, rates, xav_in, xint_in, xav, xint, sums, tag):
    """The C statement of the pass on the rates the GPU pass read and on its own x_av input."""
    xa, xi, conv, _ = O.global_pass(c["dt"], c["ndens"][sl], c["temp"][sl], c["xh"][sl], xav_in, xint_in, rates, *W.CHEM)
    np.testing.assert_allclose(xav, xa, rtol=PASS_RTOL, atol=0, err_msg=tag)
    np.testing.assert_allclose(xint, xi, rtol=PASS_RTOL, atol=0, err_msg=tag)
    assert int(sums[0]) == conv, tag
    # the sums of the GPU's own planes (tests/test_gpu_heating.py: 1e-12)
    assert sums[1] == pytest.approx(xint.sum(), rel=1e-12) and sums[2] == pytest.approx((1.0 - xint).sum(), rel=1e-12), tag


def _replay_slab_rank(lib, c, world, r):
    """Rank r of the world on the GPU, and every check of an iteration."""
    plan, N = c["plan"], c["N"]
    a, b = plan.own[r]
    sl = slice(a, b)
    W.begin_rank(lib, c, r)
    got = W.slab_iterations({r: lib}, c, ITERS, record=world)
    xav_in = xint_in = c["xh"][sl]
    for it, (g, w) in enumerate(zip(got, world)):
        tag = f"rank {r} of {c['P']}, N={N}, iteration {it + 1}"
        assert sorted(g["msgs"]) == sorted(k for k in w["msgs"] if k[0] == r), tag
        for key, m in g["msgs"].items():
            _assert_rates(m, w["msgs"][key], f"{tag}, message {key}")
            # (the accumulators outside work_runs cannot be read: what leaves must be exactly zero where no source of the rank reaches)
            assert not m[~W.reached(c, r, key[2], key[3])].any(), f"{tag}, message {key}"
        _assert_rates(g["rates"][r], w["rates"][r], f"{tag}, consumed rates")
        assert g["rates"][r].max() > 0, tag
        _assert_pass(c, sl, g["rates"][r], xav_in, xint_in, g["xav"][r], g["xint"][r], g["sums"][r], tag)
        assert tuple(g["rows"][r][:3]) == tuple(float(v) for v in w["totals"]), tag       # the row holds the totals given to close
        xav_in, xint_in = g["xav"][r], g["xint"][r]
    return got


# ---- A: slab loop, several tiles with cut tiles and cut lines -----------------------------------------------------------
@pytest.mark.parametrize("name", ["A_P2_Rbox", "A_P2_Rbox_uniformT", "A_P3_R11"])
def test_every_rank_of_a_cpu_world_at_cut_tiles(asora, name):
    """N = 75, isothermal.  P = 2, R beyond the box: every rank reaches every plane, the foreign range ([37, 75) or [0, 37)) is
    folded out in two i-tiles of which the first starts inside a tile of the grid, the pass runs on 37 / 38 planes (i tiles of
    32 + 5 / 6); once with a uniform temperature grid (the UNIFORM_T form over a range).  P = 3, R = 11: own ranges of 25 planes,
    none tile-aligned, messages across plane boundaries inside the box and through plane 0.  Every rank is replayed in turn."""
    p, lib = asora
    c, world = _world(name)
    plan, N = c["plan"], c["N"]
    if c["P"] == 3:                  # the geometry this world is about: sends across both kinds of boundary
        assert plan.own == [(0, 25), (25, 50), (50, 75)]
        assert plan.reach[0][25] and plan.reach[1][24] and plan.reach[1][50] and plan.reach[2][49]          # inside the box
        assert plan.reach[0][N - 1] and plan.reach[2][0]                                                    # through plane 0
        assert not all(m.all() for m in plan.reach)
    else:
        assert plan.own == [(0, 37), (37, 75)] and all(m.all() for m in plan.reach)
    assert (np.ptp(c["temp"]) == 0) == name.endswith("uniformT")
    for r in range(c["P"]):
        _fresh(p, c)
        _replay_slab_rank(lib, c, world, r)
    p.device_close()


# ---- B: slab pass over a range with several j per workgroup --------------------------------------------------------------
def test_rank_1_of_a_cpu_world_with_several_j_per_workgroup(asora):
    """N = 200, P = 2, R = 9, the GPU as rank 1 (planes [100, 200)): 7 x 4 tiles, so the pass's workgroups take more than one j
    each (asserted from tile_pass_grid's formula and this chip's CU count: on another chip the test fails instead of testing
    nothing), with i_begin = 100 and rank-local sums.  Half the sources sit at j beyond the first trip, so the next iteration's
    trace reads nHI the later trips emitted."""
    p, lib = asora
    c, world = _world("B_200")
    N, (a, b) = c["N"], c["plan"].own[1]
    jc = _jc(N, b - a)
    assert (a, b) == (100, 200) and jc < N, (a, b, jc)
    lo, hi = c["bounds"][1], c["bounds"][2]
    assert (c["pos"][1, lo:hi] - 1 >= jc).any() and (c["pos"][1, lo:hi] - 1 < jc).any()
    assert any(k[0] == 1 for k in world[0]["msgs"]) and any(k[1] == 1 for k in world[0]["msgs"])      # it sends and receives
    _fresh(p, c)
    _replay_slab_rank(lib, c, world, 1)
    p.device_close()


# ---- C: all-reduce loop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C_75", "C_75_uniformT", "C_168"])
def test_a_rank_of_the_all_reduce_loop_in_a_cpu_world(asora, name):
    """asora_evolve_slab_fold_all, then the pass with fold = false (chemistry_tile_kernel<false, true, ...>: it reads the summed
    out-box, keeps it in PHI_ION, emits nHI in both layouts), P = 2, both ranks in turn (N = 168: rank 1).  At N = 168 the whole-grid pass has
    several j per workgroup (asserted).  The out-box after fold_all against the CPU rank's; PHI_ION == the sum the pass was given,
    bit for bit; the pass on the rates it read; and the trace of iterations 2 and 3 against the oracle on the GPU's own previous
    XH_AV -- the [k][j][i] twin of nHI that the previous pass emitted through its LDS tile enters there, as the rates of the
    z-face sectors.  That tile is reused across the trips of the j loop; the barrier that separates a trip's transposed store
    from the next trip's writes is justified by reading the kernel, and a race need not fire in any given run: what this test
    guards is the layout logic of the multi-trip path."""
    p, lib = asora
    c, world = _world(name)
    N = c["N"]
    if N == 168:
        jc = _jc(N, N)
        assert jc < N, jc
        assert (c["pos"][1] - 1 >= jc).any()
    assert (np.ptp(c["temp"]) == 0) == name.endswith("uniformT")
    sl = slice(0, N)
    for r in (range(c["P"]) if N < 100 else [1]):            # (N = 168 is about the pass, the same on every rank: one rank)
        _fresh(p, c)
        p0, f0, n = W.share(c, r)
        W.begin_rank(lib, c, r, own=(0, N))
        got = W.reduce_iterations({r: lib}, c, ITERS, record=world)
        xav_in = xint_in = c["xh"]
        for it, (g, w) in enumerate(zip(got, world)):
            tag = f"{name}, rank {r}, iteration {it + 1}"
            _assert_rates(g["box"][r], w["box"][r], f"{tag}, out-box")
            if it > 0:               # (the first trace reads nHI formed from XH: the CPU rank's out-box is that reference)
                ref = O.asora_do_all_sources(c["R"], cases.SIG, c["dr"], c["ndens"], xav_in, p0, f0, c["thin"], c["thick"],
                                             cases.MINLOGTAU, c["dlog"], NumTau=c["numtau"], flags=O.ASORA_MODE)["phi_ion"]
                _assert_rates(g["box"][r], ref, f"{tag}, trace on the GPU's own previous XH_AV")
            assert np.array_equal(g["rates"][r], g["total"]) and g["total"].max() > 0, tag
            _assert_pass(c, sl, g["rates"][r], xav_in, xint_in, g["xav"][r], g["xint"][r], g["rows"][r], tag)
            assert tuple(g["sums"][r]) == tuple(g["rows"][r][:3]), tag
            xav_in, xint_in = g["xav"][r], g["xint"][r]
    p.device_close()


# ---- D: thermal, slab loop ---------------------------------------------------------------------------------------------------
P2 = 2.0 ** -35                                            # tests/test_gpu_heating.py: the power-of-two identity
# the conditioning split and the tolerances of tests/test_gpu_heating.py::test_thermal_fused_pass_against_the_reference_on_the_rates_it_read
WELL_CONDITIONED = 1e-2
ILL_RTOL_XAV, ILL_RTOL = 1e-3, 1e-7


def _thermal_case(identity):
    """N = 75, P = 2, R = 11, six non-overlapping sources on the N // 2 lattice: spheres straddle plane 37 (the slab boundary, inside
    a tile) and wrap through plane 0.  Black-body photo tables; heating tables 2^-35 x those (identity) or the black-body ones."""
    thin, thick, hthin, hthick, dlog = cases.blackbody_photo_and_heat_tables(num_tau=600)
    if identity:
        hthin, hthick = P2 * thin, P2 * thick
    c = W.make_case(N=75, P=2, ns=6, R=11.0, seed=108, lattice=True, tables=(thin, thick, dlog), temp_decades=(2.0, 4.0),
                    dt_myr=5.0, flux_scale=1.0)
    c.update(hthin=hthin, hthick=hthick)
    first = c["pos"][0] - 1
    assert 2 * int(c["R"]) < c["N"] // 2 and (first == 0).any() and (first == c["N"] // 2).any()
    assert c["plan"].own == [(0, 37), (37, 75)]
    return c


def _thermal_params():
    import thermal_reference as TR
    return TR.Params(relative_denergy=0.1, t_floor=1.0, max_substeps=400, cooling_mask=31, compton=True, t_cmb=2.7255 * 9.0)


def _fresh_thermal(p, lib, c, prm):
    _fresh(p, c)
    lib.heat_table_to_device(c["hthin"], c["hthick"], c["hthin"].shape[0])
    lib.thermal_params(True, prm.relative_denergy, prm.t_floor, prm.max_substeps, prm.cooling_mask, prm.compton, prm.t_cmb)


def _trace(c, r, xav):
    """The oracle's rates and heating of rank r's share on the ionised fraction xav."""
    p0, f0, _ = W.share(c, r)
    return O.asora_do_all_sources(c["R"], cases.SIG, c["dr"], c["ndens"], xav, p0, f0, c["thin"], c["thick"], cases.MINLOGTAU,
                                  c["dlog"], NumTau=c["numtau"], flags=O.ASORA_MODE, heat_thin=c["hthin"], heat_thick=c["hthick"])


def _thermal_world(p, lib, c, prm, identity):
    """What OracleAsora cannot supply (it is isothermal).  The one-GPU thermal loop, one iteration at a time, gives the XH_AV of
    the foreign planes and the totals of the sums -- another entry point, whose pass is pinned to numpy at N = 197 / 200 by
    tests/test_gpu_heating.py: it supplies the world, not the verdict.  What rank q sends is the oracle's trace of q's share on
    the iteration's x_av (identity: the heating message is 2^-35 x the rate message by construction)."""
    from pyc2ray_amd import _capi
    N, plan = c["N"], c["plan"]
    _fresh_thermal(p, lib, c, prm)
    p0, f0 = cases.flat_sources(c["pos"], c["flux"])
    lib.source_data_to_device(p0, f0, c["ns"])
    for which, a in ((_capi.GRID_NDENS, c["ndens"]), (_capi.GRID_TEMP, c["temp"]), (_capi.GRID_XH, c["xh"])):
        lib.grid_to_device(which, a)
    lib.evolve_begin(c["dt"], *W.CHEM, c["R"], cases.SIG, c["dr"], cases.MINLOGTAU, c["dlog"], c["numtau"], 0, c["ns"], -1.0, 0.0)
    K = plan.common_chunks(W.CHUNKS)
    world, x_in = [], c["xh"]
    for it in range(ITERS):
        lib.evolve_enqueue(1)
        niter, done, rows = lib.evolve_poll()
        assert niter == it + 1 and not done and len(rows) == 1
        xav = lib.grid_to_host(_capi.GRID_XH_AV, np.empty((N, N, N)))
        rec = dict(msgs={}, hmsgs={}, xav={q: xav[slice(*plan.own[q])] for q in range(2)}, totals=tuple(float(v) for v in rows[0][:3]),
                   x_in=x_in, x_one=xav)
        for q in range(2):
            t = _trace(c, q, x_in)
            for k, pieces in enumerate(plan.send_schedule(q, K)):
                for dest, a, b in pieces:
                    rec["msgs"][(q, dest, a, b, k)] = t["phi_ion"][a:b].copy()
                    rec["hmsgs"][(q, dest, a, b, k)] = P2 * t["phi_ion"][a:b] if identity else t["phi_heat"][a:b].copy()
        world.append(rec)
        x_in = xav
    _freeze(world)
    return world


def _replay_thermal_rank(p, lib, c, prm, world, r):
    _fresh_thermal(p, lib, c, prm)
    W.begin_rank(lib, c, r, thermal=True)
    got = W.slab_iterations({r: lib}, c, ITERS, record=world, thermal=True)
    for g, w in zip(got, world):
        assert sorted(g["msgs"]) == sorted(g["hmsgs"]) == sorted(k for k in w["msgs"] if k[0] == r) and g["msgs"]
        assert any(k[1] == r for k in w["msgs"])                                                  # and it receives
        assert tuple(g["rows"][r][:3]) == w["totals"]
    return got


def test_thermal_rank_heating_lands_where_the_rates_land(asora):
    """Heating tables = 2^-35 x the photo tables, one contributing source per cell: every heating message a rank sends and the
    PHI_HEAT its pass consumed equal 2^-35 x the rate message / PHI_ION bit for bit, in all three iterations, on both ranks.
    Pins fold_out_pair_kernel and asora_evolve_slab_add_heat_host (add_planes_kernel on the heating pair) at cut tiles: heating
    folded from or added to other planes or cells than the rates, a heating pair not zeroed where the rate pair is, would show."""
    p, lib = asora
    c, prm = _thermal_case(True), _thermal_params()
    try:
        world = _thermal_world(p, lib, c, prm, True)
        for r in range(2):
            got = _replay_thermal_rank(p, lib, c, prm, world, r)
            for it, (g, w) in enumerate(zip(got, world)):
                tag = f"rank {r}, iteration {it + 1}"
                for key, m in g["msgs"].items():
                    assert m.max() > 0 and np.array_equal(g["hmsgs"][key], P2 * m), f"{tag}, message {key}"
                    assert not m[~W.reached(c, r, key[2], key[3])].any(), f"{tag}, message {key}"
                assert g["rates"][r].max() > 0 and np.array_equal(g["heat"][r], P2 * g["rates"][r]), tag
                # what arrived was added on the planes and cells it was meant for, once
                sl = slice(*c["plan"].own[r])
                mine, theirs = W.reached(c, r, sl.start, sl.stop), W.reached(c, 1 - r, sl.start, sl.stop)
                assert not (mine & theirs).any() and theirs.any()
                arrived = np.zeros_like(g["rates"][r])
                for (src, dest, a, b, k), m in w["msgs"].items():
                    if dest == r:
                        arrived[a - sl.start:b - sl.start] += m
                assert np.array_equal(g["rates"][r][theirs], arrived[theirs]) and not g["rates"][r][~(mine | theirs)].any(), tag
    finally:
        lib.thermal_params(False)
    p.device_close()


def _nconv(xav, xav_in):
    import thermal_reference as TR
    y = 1.0 - xav_in
    return int(np.count_nonzero((np.abs(xav - xav_in) > TR.MIN_FRAC_CHANGE) & (np.abs((xav - xav_in) / y) > TR.MIN_FRAC_CHANGE)
                                & (y > TR.MIN_FRAC_ATOMS)))


def test_thermal_rank_pass_against_the_reference_on_the_rates_it_read(asora):
    """Black-body photo and heating tables: chemistry_tile_kernel<true, true, false, true> over the plane ranges [0, 37) and
    [37, 75) with rank-local sums, against tests/thermal_reference.py on the rates and heating the pass read -- the assertions and
    tolerances of test_thermal_fused_pass_against_the_reference_on_the_rates_it_read; what the rank sends against the oracle's
    trace of its share on the ionised fraction it traced through."""
    import thermal_reference as TR
    p, lib = asora
    c, prm = _thermal_case(False), _thermal_params()
    try:
        world = _thermal_world(p, lib, c, prm, False)
        for r in range(2):
            got = _replay_thermal_rank(p, lib, c, prm, world, r)
            sl = slice(*c["plan"].own[r])
            n, T, xh = c["ndens"][sl], c["temp"][sl], c["xh"][sl]
            xav_in, tot = xh, [0, 0, 0]
            view = np.array(c["xh"])
            for it, (g, w) in enumerate(zip(got, world)):
                tag = f"rank {r}, iteration {it + 1}"
                ref = _trace(c, r, view)
                for key, m in g["msgs"].items():
                    _assert_rates(m, ref["phi_ion"][key[2]:key[3]], f"{tag}, message {key}")
                    _assert_rates(g["hmsgs"][key], ref["phi_heat"][key[2]:key[3]], f"{tag}, heating message {key}")
                phi, heat, xa, xi, te = (g[k][r] for k in ("rates", "heat", "xav", "xint", "temp_end"))
                rxi, rxa, rte, rconv, rstats, delta, capped = TR.chemistry_thermal(prm, c["dt"], n, T, xh, xav_in, phi, heat, *W.CHEM,
                                                                                   return_delta=True)
                well = (delta > WELL_CONDITIONED) & ~capped
                assert well.any(), tag
                for have, want, rtol in ((xi, rxi, ILL_RTOL), (xa, rxa, ILL_RTOL_XAV), (te, rte, ILL_RTOL)):
                    np.testing.assert_allclose(have[well], want[well], rtol=1e-10, atol=0, err_msg=tag)
                    np.testing.assert_allclose(have, want, rtol=rtol, atol=0, err_msg=tag)
                conv, s1, s0 = g["sums"][r]
                assert int(conv) == _nconv(xa, xav_in) == rconv, tag
                assert s1 == pytest.approx(xi.sum(), rel=1e-12) and s0 == pytest.approx((1.0 - xi).sum(), rel=1e-12), tag
                tot = [tot[0] + rstats[0], tot[1] + rstats[1], max(tot[2], rstats[2])]
                assert tuple(g["stats"][r]) == tuple(tot), (tag, g["stats"][r], tot)
                assert np.any(te > T) and heat.max() > 0, tag
                xav_in = xa
                view = np.array(w["x_one"])            # what the rank traces through next: its own planes, the owner's elsewhere
                view[sl] = xa
    finally:
        lib.thermal_params(False)
    p.device_close()
