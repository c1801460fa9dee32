"""CPU: what tests/test_gpu_launch_forms.py rests on (tests/launch_forms.py) -- the case table against a restatement of the
dispatcher's rules, the six properties of every upload list against a numpy restatement of the library's sort and against the
library's own, the oracle's indifference to zero-flux sources, and the media.  Then the launcher's own plan, which
asora_debug_launch_plan returns without a device: against that restatement, at the edges of its second stage, and enumerated over
the options against the table of built forms."""
import numpy as np
import pytest

import cases
import launch_forms as LF
import open_boundary_reference as OB
from oracle import oracle as O

NAMES = list(LF.CASES)


@pytest.fixture(scope="module")
def lib():
    from pyc2ray_amd.load_extensions import load_asora
    return load_asora()


def test_the_table_is_the_one_of_the_issue_and_follows_the_dispatcher():
    """The sixteen (N, NS, R) rows, and units x threads / paired / aligned as the restated rules give them at 256 compute units."""
    rows = [(c.N, c.NS, c.R) for c in LF.CASES.values()]
    assert rows == [(64, 1001, 8.0), (64, 1001, 13.0), (96, 1001, 18.0), (96, 1000, 22.5), (96, 1001, 24.5), (128, 1001, 30.0),
                    (128, 1000, 41.0), (128, 1001, 56.0), (64, 100, 20.0), (64, 64, 25.0), (128, 64, 32.0), (64, 20, 20.0), (64, 3, 20.0),
                    (64, 1000, 1000.0), (48, 1000, 1000.0), (33, 1001, 1000.0)]
    shapes = [(c.units, c.threads) for c in LF.CASES.values()]
    assert shapes == [(1, 128), (1, 256), (1, 512), (2, 256), (2, 512), (6, 256), (12, 256), (12, 512), (12, 64), (4, 256), (12, 256),
                      (24, 64), (96, 256), (12, 512), (12, 256), (6, 256)]
    for name, c in LF.CASES.items():
        assert LF.expected_shape(c.N, c.NS, c.R) == (c.units, c.threads, c.paired, c.aligned), name
    assert [n for n, c in LF.CASES.items() if c.extra] == ["n96_1001_R18", "n128_1001_R30", "n128_1000_R41", "n48_1000_Rbox"]
    # every production form the dispatcher knows above 2 x 256 workgroups is in the table
    assert {(c.units, c.threads) for c in LF.CASES.values() if c.NS >= 1000} == {(1, 128), (1, 256), (1, 512), (2, 256), (2, 512), (6, 256),
                                                                                 (12, 256), (12, 512)}
    # the modes: heating has no paired form; the open forms run 256 or 512 threads
    for name, c in LF.CASES.items():
        assert not LF.expected_variant(c, "heat")["paired"]
        v = LF.expected_variant(c, "open")
        assert v["open"] and v["threads"] == (512 if c.threads == 512 else 256), name
        if c.extra:                                     # (64 threads widened to 256 can bring the paired form in: no such case is run open)
            assert v["paired"] == c.paired and v["threads"] == c.threads, name
        assert LF.expected_variant(c, "tables") == LF.expected_variant(c, "spectra")


@pytest.mark.parametrize("name", NAMES)
def test_upload_list_has_the_six_properties(lib, name):
    case, src = LF.CASES[name], LF.build_sources(name)
    NS = case.NS
    K = 3 if NS == 3 else 12 if case.aligned else 8
    assert src.flux.shape == (NS,) and src.pos0.shape == (3 * NS,) and src.pos0.dtype == np.int32
    assert np.count_nonzero(src.flux) == K and np.array_equal(np.flatnonzero(src.flux), src.bright)
    assert np.all(src.flux[src.flux != 0] > 0) and not np.signbit(src.flux).any()          # the fillers: +0.0 exactly
    assert src.pos0.min() >= 0 and src.pos0.max() == case.N - 1
    # against the numpy restatement of the sort ...
    assert LF.check_properties(case, src.pos0, src.flux, src.pair) == []
    # ... and against the library's own sorted copy, which the restatement must reproduce entry for entry
    ps, fs, ss = lib.sort_sources(src.pos0, src.flux, src.spec)
    order = LF.sort_order(src.pos0)
    assert np.array_equal(ps.reshape(-1, 3), src.pos0.reshape(-1, 3)[order]) and np.array_equal(fs, src.flux[order])
    assert np.array_equal(ss, src.spec[order])
    assert LF.check_properties(case, src.pos0, src.flux, src.pair, ps, fs) == []
    # a list without one of them is noticed: the pair pulled apart (three sources stay consecutive, but no longer overlap), the
    # far corner dimmed
    moved = src.pos0.copy()
    moved[3 * src.pair[1]] = (moved[3 * src.pair[1]] + case.N // 2) % case.N
    assert any(m.startswith(("1", "4", "5")) for m in LF.check_properties(case, moved, src.flux, src.pair))
    dim = src.flux.copy()
    dim[NS - 1] = 0.0
    assert any(m.startswith("4") for m in LF.check_properties(case, src.pos0, dim, src.pair))
    # the two table sets: the pair on different ones, the fillers alternating, both sets among the bright sources
    assert src.spec[src.pair[0]] != src.spec[src.pair[1]]
    fill = np.setdiff1d(np.arange(NS), src.bright)
    assert np.array_equal(src.spec[fill], np.arange(fill.size) % 2)
    assert set(src.spec[src.bright].tolist()) == {0, 1}
    # the pair shares a workgroup: the same entry of the sorted list's pairing, (even, odd) where the tables are packed
    where = {int(u): s for s, u in enumerate(order)}
    sa, sb = where[src.pair[0]], where[src.pair[1]]
    if not case.aligned:
        assert sa % 2 == 0 and sb == sa + 1
    if NS % 2 and not case.aligned:
        assert where[NS - 1] == NS - 1 and (NS - 1) % 2 == 0          # the far corner sweeps with the dummy partner


@pytest.mark.parametrize("name", [n for n, c in LF.CASES.items() if c.extra])
def test_open_boundaries_lose_cells_the_periodic_trace_reaches(name):
    """What makes the open mode of a case differ from its periodic one: cells that only the wrap brings into a bright sphere."""
    case = LF.CASES[name]
    pos = LF.bright_positions(name)
    per, opn = LF.coverage(case.N, case.R, pos), LF.coverage(case.N, case.R, pos, periodic=False)
    assert np.all(opn <= per) and ((per > 0) & (opn == 0)).sum() > 100


def test_workgroups_restates_the_class_lists():
    """Eleven sources by hand: classes along k (list 0) and along i (list 1); a source waits for the next one of its class."""
    pos = np.array([(0, 0, 0), (0, 0, 8), (0, 1, 3), (1, 0, 16), (1, 2, 11), (8, 0, 1), (9, 9, 9), (9, 9, 17), (16, 0, 5), (17, 1, 7), (24, 0, 0)])
    by_k, by_i = LF.workgroups(pos, True)
    assert by_k == [(0, 1), (2, 4), (5, 6), (3, 10), (7, -1), (8, -1), (9, -1)]
    assert by_i == [(0, 1), (3, 4), (2, 5), (6, 7), (8, 10), (9, -1)]
    assert LF.workgroups(pos, False) == [[(0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, -1)]]


def test_reach_and_cells_within():
    from test_gpu_parity import _cells_within
    for name, c in LF.CASES.items():
        assert LF.cells_within(c.N, c.R) == _cells_within(c.N, c.R), name
    for N, R in ((64, 8.0), (33, 1000.0), (48, 1000.0), (64, 20.0), (32, 13.0)):
        for pos in ((0, 0, 0), (N - 1, N - 1, N - 1), (5, N - 2, N // 2)):
            assert LF.reach(N, R, pos).sum() == LF.cells_within(N, R), (N, R, pos)
            if R < N / 2 - 1:
                assert LF.reach(N, R, pos, periodic=False).sum() == OB.rated_pairs(N, R, pos, periodic=False), (N, R, pos)
    assert LF.reach(48, 1000.0, (0, 0, 0), periodic=False).sum() == 24 ** 3        # the window 0 ... 23 of each axis
    assert LF.reach(48, 1000.0, (47, 47, 47), periodic=False).sum() == 25 ** 3     # -24 ... 0
    assert LF.reach(33, 1000.0, (3, 3, 3)).all()                                   # an odd mesh: the window is the box


@pytest.mark.parametrize("name", NAMES)
def test_media_keep_nhi_positive_and_the_dense_one_holds_cells_beyond_the_table(name):
    case = LF.CASES[name]
    sets, dlog = LF.tables()
    last = 10.0 ** (cases.MINLOGTAU + (sets[0][0].shape[0] - 2) * dlog)        # optical depth of the last table entry
    for with_dense in (False, True):
        nd, xh, dr = LF.medium(name, with_dense)
        nhi = nd * (1.0 - xh)
        assert np.isfinite(nhi).all() and nhi.min() > 0.0
        assert xh.min() >= 1e-4 and xh.max() <= 1e-2
        assert dr == 2.0 ** round(np.log2(dr))                        # on-sphere lattice points are inside
        tau = cases.SIG * nhi * dr
        assert np.median(tau) < 0.1
        if not with_dense:
            assert tau.max() * 2 * case.N < 0.2 * last                # no path through the box comes near the tables' end
            continue
        dense = tau > 1.02 * last
        plate = np.arange(-LF.PLATE_HALF_WIDTH, LF.PLATE_HALF_WIDTH + 1) % case.N
        assert dense[np.ix_([LF.PLATE_PLANE], plate, plate)].all()     # the plate in front of the corner source, through the wrap
        scattered = dense.sum() - plate.size ** 2
        assert 0.3 * (case.N ** 3 // LF.DENSE_ONE_IN) < scattered <= case.N ** 3 // LF.DENSE_ONE_IN     # (drawn with repetition)
        assert tau.max() * 2 * case.N < 2e30 * cases.SIG               # far from the column-density cap
        assert np.array_equal(nd[~dense], LF.medium(name)[0][~dense])


@pytest.mark.parametrize("name", ["n64_1001_R8", "n64_1001_R13", "n33_1001_Rbox"])
def test_zero_flux_sources_change_no_bit_of_the_oracle(name):
    """The oracle over the whole upload list (fillers traced like any source) against the oracle over the bright sources alone:
    phi_ion and phi_heat bit for bit.  The lognormal medium leaves no rated cell at exactly 0; the dense one does, behind its plate,
    which is what ASORA_OPT_SKIP_ZERO_RATES leaves out, and most of its cells are lit well enough to be compared."""
    case, src = LF.CASES[name], LF.build_sources(name)
    nd, xh, dr = LF.medium(name)
    if name == "n33_1001_Rbox":                                      # (1001 whole-box traces: the first 60 of the list and the far corner)
        keep = np.concatenate((np.arange(60), [case.NS - 1]))
        pos0, flux = np.ascontiguousarray(src.pos0.reshape(-1, 3)[keep]).ravel(), np.ascontiguousarray(src.flux[keep])
        bright = np.flatnonzero(flux)
        bp, bf = np.ascontiguousarray(pos0.reshape(-1, 3)[bright]).ravel(), np.ascontiguousarray(flux[bright])
        ref = LF._oracle(case, nd, xh, dr, bp, bf, 0, True)
    else:
        pos0, flux = src.pos0, src.flux
        ref = LF.reference(name, "tables")
    full = LF._oracle(case, nd, xh, dr, pos0, flux, 0, True)
    assert np.array_equal(full["phi_ion"], ref["phi_ion"]) and np.array_equal(full["phi_heat"], ref["phi_heat"])
    assert not np.signbit(full["phi_ion"]).any() and np.isfinite(full["phi_ion"]).all()
    if name != "n33_1001_Rbox":
        cov = LF.coverage(case.N, case.R, LF.bright_positions(name))
        assert np.array_equal(ref["phi_ion"] != 0, ref["phi_heat"] != 0)
        assert not ref["phi_ion"][cov == 0].any()
        assert np.array_equal(ref["phi_ion"] != 0, cov > 0)
        dense = LF.reference(name, "dense")["phi_ion"]
        dark = (dense == 0) & (cov > 0)
        assert 0 < dark.sum() < 0.1 * (cov > 0).sum(), (int(dark.sum()), int((cov > 0).sum()))
        assert (dense >= LF.WELL_LIT * ref["phi_ion"])[dense != 0].mean() > 0.99
        assert (cov >= 2).sum() > 0.5 * LF.cells_within(case.N, case.R)             # property 5 in cells


def test_two_set_reference_is_linear_in_the_sources():
    """The sum of two traces, each set on its sources; with both sets the same tables it is the one trace (to the order of the sum)."""
    name = "n64_1001_R13"
    case, src = LF.CASES[name], LF.build_sources(name)
    nd, xh, dr = LF.medium(name)
    one = LF.reference(name, "tables")["phi_ion"]
    two = np.zeros_like(one)
    for s in (0, 1):
        sel = src.spec[src.bright] == s
        assert sel.any()
        two += LF._oracle(case, nd, xh, dr, *LF._bright(src, sel), 0, False)["phi_ion"]
    assert np.array_equal(two != 0, one != 0)
    np.testing.assert_allclose(two, one, rtol=1e-13, atol=0)
    assert not np.allclose(LF.reference(name, "spectra")["phi_ion"], one, rtol=1e-3, atol=0)


def test_open_trace_by_source_equals_open_trace_where_both_apply():
    """N = 24, R = 8 < N/2 - 1: the per-source composition on the mesh of 2 N against open_boundary_reference.open_trace; and at a
    radius beyond the box it leaves every cell outside a source's window alone."""
    N = 24
    nd, xh, _ = cases.grid(N, "lognormal", 5, 0.05, xlo=1e-4, xhi=1e-2)
    dr = 2.0 ** 63
    (thin, thick, _, _), dlog = LF.tables()[0][0], LF.tables()[1]
    pos0 = np.array([0, 0, 0, 23, 23, 23, 3, 20, 11, 12, 12, 13], dtype=np.int32)
    flux = np.array([1.0, 2.0, 3.0, 4.0])
    a = LF.open_trace_by_source(8.0, dr, nd, xh, pos0, flux, thin, thick, dlog)
    b = OB.open_trace(8.0, cases.SIG, dr, nd, xh, pos0, flux, thin, thick, cases.MINLOGTAU, dlog, NumTau=thin.shape[0] - 1)["phi_ion"]
    assert np.array_equal(a != 0, b != 0) and (b != 0).sum() > 3000
    np.testing.assert_allclose(a, b, rtol=1e-13, atol=0)
    far = LF.open_trace_by_source(1000.0, dr, nd, xh, pos0[:3], flux[:1], thin, thick, dlog)
    assert np.array_equal(far != 0, LF.reach(N, 1000.0, (0, 0, 0), periodic=False)) and (far != 0).sum() == 12 ** 3
    # inside the window the rates are those of the periodic trace of the N-box (the corner source: nothing wraps on the way)
    per = O.asora_do_all_sources(1000.0, cases.SIG, dr, nd, xh, pos0[:3], flux[:1], thin, thick, cases.MINLOGTAU, dlog,
                                 NumTau=thin.shape[0] - 1, flags=O.ASORA_MODE)["phi_ion"]
    w = far != 0
    np.testing.assert_allclose(far[w], per[w], rtol=1e-13, atol=0)


# ---- the launcher's own plan (asora_debug_launch_plan: csrc/raytrace_plan.hpp without a device) -----------------------------------
PLAN_OPTIONS = ("OPT_SECTORS", "OPT_BLOCK_THREADS", "OPT_PAIR_SOURCES", "OPT_ALIGNED_ROWS", "OPT_GLOBAL_ATOMICS", "OPT_SKIP_ZERO_RATES",
                "OPT_GREY_NOTABLES", "OPT_OPEN_BOUNDARIES")
LDS_LIMIT = 160 * 1024


@pytest.fixture
def plan(lib):
    """plan(N, R, NS, ..., **options): lib.launch_plan on 256 compute units under the named options, which go back to 0 afterwards."""
    from pyc2ray_amd import _capi

    def call(N, R, NS, shells=-1, max_cells=0, **kw):
        opts = {k: kw.pop(k) for k in list(kw) if k.startswith("OPT_")}
        assert set(opts) <= set(PLAN_OPTIONS)
        for k in PLAN_OPTIONS:
            lib.set_option(getattr(_capi, k), opts.get(k, 0))
        return lib.launch_plan(N, R, NS, cu_count=LF.CU_COUNT, shells=shells, max_cells=max_cells, **kw)

    yield call
    for k in PLAN_OPTIONS:
        lib.set_option(getattr(_capi, k), 0)


def _refused(plan, code, *a, **kw):
    with pytest.raises(RuntimeError, match=rf"\(code {code}\)") as e:
        plan(*a, **kw)
    return str(e.value)


def _shells(N, R):
    return min(int(np.floor(R)), N // 2)


#: the smallest largest shell a trace of more than 256 shells has (N = 512, R = 256, cut into the 96 quarter sectors): such shells
#: never fit LDS beside the 1024-entry tables, and RT_FORMS holds those tables with the shells in global memory only
MANY_SHELLS_MAX_CELLS = 12445


def _max_cells(N, R, max_cells):
    """A largest shell that a trace of this many shells can have: `max_cells`, or what more than 256 shells bring at least."""
    return max(max_cells, MANY_SHELLS_MAX_CELLS) if _shells(N, R) + 1 > 256 else max_cells


def _lds(max_cells, tabcap, nsrc):
    """Dynamic LDS of a form with its shells in LDS (the kernel's layout: log table, 1/s, 6 wrapped-coordinate tables and two shell
    buffers per source)."""
    return nsrc * 2 * ((max_cells + 2) & ~1) * 8 + 256 * 16 + tabcap * (8 + nsrc * 6 * 4)


def _largest_that_fits(tabcap, nsrc):
    mc = (LDS_LIMIT - 256 * 16 - tabcap * (8 + nsrc * 24)) // (16 * nsrc)
    while _lds(mc + 1, tabcap, nsrc) <= LDS_LIMIT:
        mc += 1
    while _lds(mc, tabcap, nsrc) > LDS_LIMIT:
        mc -= 1
    return mc


@pytest.mark.parametrize("name", NAMES)
def test_plan_of_the_sixteen_cases_is_the_table(lib, plan, name):
    """Stage 1 against expected_shape, the variant word against expected_variant, in every mode; the planned form is built."""
    c = LF.CASES[name]
    units, threads, paired, aligned = LF.expected_shape(c.N, c.NS, c.R)
    for mode in ("tables", "heat", "spectra", "open"):
        kw = {"heat": mode == "heat", "table_sets": mode == "spectra", "OPT_OPEN_BOUNDARIES": int(mode == "open"),
              "OPT_SKIP_ZERO_RATES": 0 if mode in ("heat", "open") else 2}
        want_threads = threads if mode != "open" else 256 if threads <= 256 else 512      # the sizes the open forms are built for
        s1 = plan(c.N, c.R, c.NS, **kw)
        assert (s1["units"], s1["threads"], s1["aligned"]) == (units, want_threads, aligned), (name, mode)
        s2 = plan(c.N, c.R, c.NS, shells=_shells(c.N, c.R), max_cells=1000, **kw)
        got = {k: v for k, v in lib.variant_fields(s2["variant"]).items() if k != "skip_zero"}
        assert got == LF.expected_variant(c, mode), (name, mode)
        assert s2["built"] and s2["use_lds"] and s2["form"]["threads"] == want_threads, (name, mode)
        assert s2["form"]["nsrc"] == (2 if got["paired"] else 1) and s2["form"]["heat"] == (mode == "heat") and s2["form"]["open"] == (mode == "open")
        if mode == "tables":
            assert paired == got["paired"], name


def test_plan_shape_sweep_against_expected_shape(plan):
    """No forced option, N <= 512, first radius: every threshold of pick_launch_shape and pair_sources_pays from either side."""
    radii = (11.5, 12.5, 14.5, 15.5, np.sqrt(450 / 1.2), 21.5, 22.5, 23.5, 25.5, 28.5, 35.3, 36.5, 52.5, np.sqrt(3500 / 1.2))
    radii = sorted({x for r in radii for x in (np.nextafter(r, 0), r, np.nextafter(r, 1e9), r - 0.25, r + 0.25)} | {1000.0})
    n = 0
    for N in (33, 48, 64, 96, 128, 256, 512):
        for NS in (1, 3, 5, 20, 21, 64, 85, 100, 1000, 1001):
            for R in radii:
                units, threads, paired, aligned = LF.expected_shape(N, NS, R)
                if _shells(N, R) + 1 > 256:
                    threads = max(threads, 256)           # more than 256 shells: the 1024-entry LDS tables, 256 threads at least
                s2 = plan(N, R, NS, shells=_shells(N, R), max_cells=_max_cells(N, R, 1000))
                assert (s2["units"], s2["threads"], s2["aligned"]) == (units, threads, aligned), (N, NS, R)
                # stage 2 on top: expected_shape's pairing rule, where a paired form exists (up to 512 threads and 256 shells)
                assert (s2["form"]["nsrc"] == 2) == (paired and threads <= 512 and _shells(N, R) + 1 <= 256), (N, NS, R)
                assert s2["built"], (N, NS, R, s2["form"])
                n += 1
    assert n == 7 * 10 * len(radii)


def test_plan_stage_two_edges(lib, plan):
    from pyc2ray_amd import _capi
    N, R, NS = 256, 30.0, 1000                                          # six sectors x 256 threads
    # LDS table capacities by the number of shells: paired, single x 256, single x 128
    for shells1, paired_cap, single_cap, small_cap in ((32, 32, 256, 64), (33, 64, 256, 64), (64, 64, 256, 64), (65, 256, 256, 256), (256, 256, 256, 256),
                                                       (257, None, 1024, None), (1024, None, 1024, None)):
        a = plan(N, R, NS, shells=shells1 - 1, max_cells=1000, OPT_PAIR_SOURCES=2)
        b = plan(N, R, NS, shells=shells1 - 1, max_cells=1000, OPT_PAIR_SOURCES=1)
        # (more than 256 shells with a largest shell of 1000 cells: shells no geometry has -- planned, but not among the built forms)
        assert a["built"] == b["built"] == (shells1 <= 256)
        assert (a["form"]["nsrc"], a["form"]["tabcap"]) == ((2, paired_cap) if paired_cap else (1, 1024)), shells1
        assert (b["form"]["nsrc"], b["form"]["tabcap"], b["form"]["threads"]) == (1, single_cap, 256), shells1
        assert a["lds_bytes"] == _lds(1000, a["form"]["tabcap"], a["form"]["nsrc"]) and b["lds_bytes"] == _lds(1000, single_cap, 1)
        if small_cap:
            s = plan(N, R, NS, shells=shells1 - 1, max_cells=1000, OPT_BLOCK_THREADS=128, OPT_PAIR_SOURCES=1)
            assert s["built"] and (s["form"]["threads"], s["form"]["tabcap"]) == (128, small_cap), shells1
        else:       # ... and with the largest shell such a trace has at least: the 1024-entry tables, the shells in global memory, built
            for q in (plan(512, 1000.0, 1, shells=shells1 - 1, max_cells=MANY_SHELLS_MAX_CELLS, OPT_PAIR_SOURCES=pair) for pair in (1, 2)):
                assert q["built"] and not q["use_lds"] and (q["form"]["nsrc"], q["form"]["tabcap"], q["form"]["global_scratch"]) == (1, 1024, True)
                assert q["lds_bytes"] == 256 * 16 + 1024 * 32
    assert _lds(MANY_SHELLS_MAX_CELLS, 1024, 1) > LDS_LIMIT
    assert "more than 1023 shells" in _refused(plan, 4, N, R, NS, shells=1024, max_cells=1000)
    # the LDS limit: the shells of a single source leave LDS, the four shell buffers of a pair leave it first
    mc = _largest_that_fits(256, 1)
    assert _lds(mc, 256, 1) <= LDS_LIMIT < _lds(mc + 1, 256, 1)
    fits, over = (plan(N, R, NS, shells=40, max_cells=m, OPT_PAIR_SOURCES=1) for m in (mc, mc + 1))
    assert fits["use_lds"] and not fits["form"]["global_scratch"] and fits["form"]["bufatom"] and fits["lds_bytes"] == _lds(mc, 256, 1)
    assert not over["use_lds"] and over["form"]["global_scratch"] and not over["form"]["bufatom"] and over["built"]
    assert over["lds_bytes"] == 256 * 16 + 256 * 32 and lib.variant_fields(over["variant"])["global_shells"]
    mc2 = _largest_that_fits(256, 2)
    assert mc2 < mc
    two, one = (plan(N, R, NS, shells=80, max_cells=m, OPT_PAIR_SOURCES=2) for m in (mc2, mc2 + 1))
    assert two["form"]["nsrc"] == 2 and two["lds_bytes"] == _lds(mc2, 256, 2) <= LDS_LIMIT
    assert one["form"]["nsrc"] == 1 and one["use_lds"] and one["built"] and not lib.variant_fields(one["variant"])["paired"]
    # one descriptor, one per layout, global atomics
    for n, split, bufatom in ((512, False, True), (520, True, True), (645, True, True), (648, False, False)):
        q = plan(n, R, NS, shells=30, max_cells=1000)
        assert (q["form"]["split"], q["form"]["bufatom"], q["built"]) == (split, bufatom, True), n
        v = lib.variant_fields(q["variant"])
        assert (v["split_descriptors"], v["buffer_atomics"], v["paired"]) == (split, bufatom, bufatom), n
    # per-source table sets: the paired split family alone has a form without them
    for n in (512, 520):
        for sets in (False, True):
            q = plan(n, R, NS, shells=30, max_cells=1000, table_sets=sets)
            assert q["form"]["nsrc"] == 2 and q["form"]["spec"] == (sets or n == 512) and q["built"], (n, sets)
    assert plan(520, R, NS, shells=30, max_cells=1000, heat=True)["form"]["spec"]
    # what open boundaries are not built for
    assert "N <= 512" in _refused(plan, 4, 520, R, NS, OPT_OPEN_BOUNDARIES=1)
    assert "table rates" in _refused(plan, 4, N, R, NS, OPT_OPEN_BOUNDARIES=1, OPT_GREY_NOTABLES=1)
    assert "buffer-atomic" in _refused(plan, 4, N, R, NS, OPT_OPEN_BOUNDARIES=1, OPT_GLOBAL_ATOMICS=1)
    assert "dump" in _refused(plan, 4, N, R, NS, OPT_OPEN_BOUNDARIES=1, dump=True)
    # heating, grey opacity and the dump each end pairing and zero-skipping
    base = plan(N, R, NS, shells=30, max_cells=1000, OPT_PAIR_SOURCES=2, OPT_SKIP_ZERO_RATES=1)
    assert base["form"]["nsrc"] == 2 and base["form"]["skip_zero"] and base["zero_form_exists"] and base["variant"] & _capi.VARIANT_SKIP_ZERO
    for kw in ({"heat": True}, {"OPT_GREY_NOTABLES": 1}, {"dump": True}):
        q = plan(N, R, NS, shells=30, max_cells=1000, OPT_PAIR_SOURCES=2, OPT_SKIP_ZERO_RATES=1, **kw)
        assert q["form"]["nsrc"] == 1 and not q["form"]["skip_zero"] and not q["zero_form_exists"] and q["built"], kw
        assert not q["variant"] & (_capi.VARIANT_SKIP_ZERO | _capi.VARIANT_PAIRED), kw
        assert (q["form"]["heat"], q["form"]["grey"], q["form"]["dump"]) == ("heat" in kw, "OPT_GREY_NOTABLES" in kw, "dump" in kw)
    assert plan(N, R, NS, shells=30, max_cells=1000, dump=True)["threads"] == 256
    assert not plan(N, R, NS, shells=30, max_cells=1000, OPT_SKIP_ZERO_RATES=2)["zero_form_exists"]
    # ASORA_OPT_SKIP_ZERO_RATES = 1 without buffer atomics: the branching form, which the variant word does not report
    q = plan(N, R, NS, shells=30, max_cells=1000, OPT_GLOBAL_ATOMICS=1, OPT_SKIP_ZERO_RATES=1)
    assert q["form"]["skip_zero"] and not q["form"]["bufatom"] and q["form"]["nsrc"] == 1 and q["built"] and not q["zero_form_exists"]
    assert not q["variant"] & (_capi.VARIANT_SKIP_ZERO | _capi.VARIANT_BUFFER_ATOMICS)
    assert not plan(N, R, NS, shells=30, max_cells=1000, OPT_GLOBAL_ATOMICS=1)["form"]["skip_zero"]


def test_every_plan_is_refused_or_built(plan):
    """The dispatcher's soundness: over the options that shape a launch, the modes and meshes on every side of the descriptor rules,
    radii of every launch shape and shells inside and outside LDS, a call is refused with a message or plans a form of the table.
    The product of the options, the modes and the meshes is complete; what is thinned is what each combination is run with: four of
    the eight radii (one per launch-shape regime of pick_launch_shape, one beyond the box), each with shells inside LDS and outside
    (more than 256 shells, N = 512 and 576 with the radius beyond the box: outside only, with the largest shell such a trace has at least),
    one of three source counts and of three ASORA_OPT_SKIP_ZERO_RATES, going round with a running count."""
    modes = ({}, {"heat": True}, {"OPT_GREY_NOTABLES": 1}, {"dump": True}, {"OPT_OPEN_BOUNDARIES": 1}, {"OPT_OPEN_BOUNDARIES": 1, "heat": True})
    radii = (8.0, 13.0, 18.0, 24.5, 30.0, 41.0, 56.0, 1000.0)
    planned = refused = k = 0
    seen, ran = set(), set()
    for sectors in range(10):
        for threads in (0, 64, 128, 256, 512, 1024):
            for pair in (0, 1, 2):
                for rows in (0, 1, 2):
                    for ga in (0, 1):
                        k += 1
                        for m, mode in enumerate(modes):
                            for N in (64, 512, 576):
                                for j in range(8):
                                    R, max_cells, NS = radii[(k + 2 * (j // 2)) % 8], (500, 12000)[j % 2], (1000, 3, 64)[(k // 16) % 3]
                                    in_lds = max_cells == 500 and _shells(N, R) + 1 <= 256       # (more than 256 shells never fit LDS)
                                    max_cells = _max_cells(N, R, max_cells)
                                    ran.add((m, N, R, in_lds))
                                    try:
                                        q = plan(N, R, NS, shells=_shells(N, R), max_cells=max_cells, table_sets=bool((k // 2) % 2),
                                                 OPT_SECTORS=sectors, OPT_BLOCK_THREADS=threads, OPT_PAIR_SOURCES=pair, OPT_ALIGNED_ROWS=rows,
                                                 OPT_GLOBAL_ATOMICS=ga, OPT_SKIP_ZERO_RATES=(k // 48) % 3, **mode)
                                    except RuntimeError as e:
                                        assert "open boundaries" in str(e) and "(code 4)" in str(e) and m >= 4 and (N == 576 or ga), str(e)
                                        refused += 1
                                        continue
                                    assert not (m >= 4 and (N == 576 or ga))
                                    assert q["built"], (sectors, threads, pair, rows, ga, N, R, NS, max_cells, mode, q["form"])
                                    assert q["use_lds"] == in_lds
                                    planned += 1
                                    seen.add(tuple(q["form"].values()))
    print(f"{planned} planned, {refused} refused, {len(seen)} distinct forms, {len(ran)} of {6 * 3 * 8 * 2} (mode, N, R, shells) run")
    total = 8 * 10 * 6 * 3 * 3 * 2 * 6 * 3
    assert planned + refused == total and refused == total // 3 * 4 // 6          # the two open modes, on N = 576 or under global atomics
    assert len(ran) == 6 * 3 * 8 * 2 - 12                    # (N = 512 and 576 with the radius beyond the box: 257 and 289 shells, outside LDS both times)
