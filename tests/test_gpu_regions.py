"""GPU: the connected regions (asora_region_sizes, region_sizes, C2Ray.regions) against their numpy
statement, tests/regions_reference.py.  Everything is integers: every comparison is for equality.

* Meshes: those of the mean-free-path tests with their seeds -- N = 17 (odd, one word per row, fewer cells than a workgroup has
  threads), 64 (rows of exactly one full word: a run ends on the word boundary, next to the wrap), 70 (two words per row, the second
  with a 6-bit tail: runs straddle the word boundary) and 136 (three words per row, the third with an 8-bit tail, and runs that begin
  in the first and end in the third: both word walks take two steps; 4.8 trips of every grid-stride loop on 256 CUs).
* N = 216, regions_reference.crowded: 4.6 million regions of 1, 5, 6 and 7 cells under 6 neighbours, one under 26; 19 trips, and
  every workgroup meets more roots than its LDS table holds, so run lengths go straight to global memory (asserted from the device's
  CU count); the threshold pass takes a second trip.
* Fields: bubble_reference.blob_field at (threshold, phase, connectivity) = (0.5, both, 6) -- one dominant region and thousands of
  specks --, (0.69, ionised, 6) near the site-percolation threshold of 6 neighbours, (0.9, ionised, 26) the same for 26; each
  periodic and open, which differ in every one of them (asserted), so a missing or a spurious wrap cannot pass.
* Crafted masks at N = 16 and 17: the hand-built ones of tests/test_regions_reference.py, a serpentine (the longest chain), two cubes
  of equal volume."""
import os

import numpy as np
import pytest

import bubble_reference as BR
import regions_reference as RR
from test_bubble_reference import GPU_FIELDS
from test_regions_reference import BLOB_CASES, CROWDED, crowded_condition, hand_cases, two_cubes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REGION_PARAMS = os.path.join(HERE, "data", "parameters_regions.yml")
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_single_black_body.yml")
T = {name: n for n, name in enumerate(RR.TALLIES)}


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib, _capi
    if p.cuda_is_init():
        p.device_close()


def _mesh(asora, N):
    p, lib, capi = asora
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)


@pytest.fixture(scope="module", params=GPU_FIELDS, ids=lambda f: f"N{f[0]}")
def box(request, asora):
    """A mesh with the blob field in GRID_XH, and the references of its cases, computed as they are first asked for and kept."""
    p, lib, capi = asora
    N, seed = request.param
    field = BR.blob_field(N, seed)
    _mesh(asora, N)
    lib.grid_to_device(capi.GRID_XH, field)
    kept = {}

    def reference(threshold, phase, connectivity, periodic):
        key = (threshold, phase, connectivity, periodic)
        if key not in kept:
            kept[key] = RR.sizes(BR.in_phase(field, threshold, phase), connectivity, periodic, RR.default_edges(N))
            kept[key][0].setflags(write=False)
        return kept[key]
    return N, field, reference


def _same(got, want, what):
    for g, w, name in zip(got, want, ("counts", "cells", "tallies")):
        assert g.dtype == np.uint64 and np.array_equal(g, w), (what, name, g.tolist(), w.tolist())


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "open"])
@pytest.mark.parametrize("case", BLOB_CASES, ids=lambda c: f"x{c[0]}-phase{c[1]}-{c[2]}")
def test_blob_fields(asora, box, case, periodic):
    p, lib, capi = asora
    N, field, reference = box
    threshold, phase, connectivity = case
    labels, counts, cells, tallies = reference(threshold, phase, connectivity, periodic)
    edges = RR.default_edges(N)
    got = lib.region_sizes(capi.GRID_XH, threshold, phase, periodic, connectivity, edges, labels=True)
    print(f"N {N}, {case}, periodic {periodic}: tallies {got[2].tolist()}, {int((got[0] > 0).sum())} bins occupied")
    assert got[3].dtype == np.uint32 and got[3].shape == (N, N, N)
    assert np.array_equal(got[3], labels)
    _same(got[:3], (counts, cells, tallies), "with labels")
    production = lib.region_sizes(capi.GRID_XH, threshold, phase, periodic, connectivity, edges)
    _same(production, (counts, cells, tallies), "production")
    again = lib.region_sizes(capi.GRID_XH, threshold, phase, periodic, connectivity, edges)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(production, again))
    # the case is what it is meant to be: the other boundary gives other regions, and the sums close
    other = reference(threshold, phase, connectivity, not periodic)
    assert other[3][T["n_regions"]] != tallies[T["n_regions"]] and not np.array_equal(other[0], labels)
    assert counts.sum() == tallies[T["n_regions"]] and cells.sum() == tallies[T["n_phase"]] == BR.in_phase(field, threshold, phase).sum()
    if case == (0.69, 0, 6) and N > 17:                      # near percolation: a third of the phase in the largest, twelve bins occupied
        assert tallies[T["n_regions"]] == {(64, False): 13_823, (70, False): 18_146, (136, False): 129_629,
                                           (64, True): 12_968, (70, True): 17_062, (136, True): 125_629}[N, periodic]
        assert 0.3 < tallies[T["v_largest"]] / tallies[T["n_phase"]] < 0.41 and tallies[T["v_second"]] > 1000
        assert (counts > 0).sum() == {64: 12, 70: 12, 136: 14}[N]      # (eight times the cells: fourteen)
        assert tallies[T["v_largest"]] > tallies[T["v_second"]] and tallies[T["extent_i"]] == tallies[T["extent_k"]] == N
    if case == (0.9, 0, 26) and N > 17 and not periodic:
        assert tallies[T["n_regions"]] == {64: 3616, 70: 4708, 136: 32_679}[N] and (counts > 0).sum() == {64: 11, 70: 12, 136: 13}[N]


def test_26_neighbours_at_one_half(asora, box):
    """One region or two: nearly everything is joined."""
    p, lib, capi = asora
    N, field, reference = box
    for periodic in (True, False):
        want = RR.sizes(field >= 0.5, 26, periodic, RR.default_edges(N))
        got = lib.region_sizes(capi.GRID_XH, 0.5, 0, periodic, 26, RR.default_edges(N), labels=True)
        assert np.array_equal(got[3], want[0])
        _same(got[:3], want[1:], periodic)
        assert 1 <= got[2][T["n_regions"]] <= 2


def _run_mask(asora, mask, connectivity, periodic, edges=None):
    """The library on a boolean mask (uploaded as 0 / 1 into GRID_XH_AV, threshold 0.5) next to the reference: both results."""
    p, lib, capi = asora
    N = mask.shape[0]
    edges = RR.default_edges(N) if edges is None else edges
    lib.grid_to_device(capi.GRID_XH_AV, mask.astype(np.float64))
    got = lib.region_sizes(capi.GRID_XH_AV, 0.5, 0, periodic, connectivity, edges, labels=True)
    want = RR.sizes(mask, connectivity, periodic, edges)
    assert np.array_equal(got[3], want[0]), (connectivity, periodic)
    _same(got[:3], want[1:], (connectivity, periodic))
    _same(lib.region_sizes(capi.GRID_XH_AV, 0.5, 0, periodic, connectivity, edges), want[1:], ("production", connectivity, periodic))
    return got, want


def test_explicit_edges_and_a_grid_with_nans(asora, box):
    p, lib, capi = asora
    N, field, reference = box
    labels = reference(0.69, 0, 6, True)[0]
    edges = np.array([2.0, 3.0, 10.0, 100.0])
    want = RR.tally(labels, edges)
    got = lib.region_sizes(capi.GRID_XH, 0.69, 0, True, 6, edges)
    _same(got, want, "explicit edges")
    t = got[2]
    assert t[T["underflow"]] > 0 and t[T["overflow"]] > 0 and t[T["underflow_cells"]] == t[T["underflow"]]
    assert got[0].sum() + t[T["underflow"]] + t[T["overflow"]] == t[T["n_regions"]]
    assert got[1].sum() + t[T["underflow_cells"]] + t[T["overflow_cells"]] == t[T["n_phase"]]
    one = lib.region_sizes(capi.GRID_XH, 0.69, 0, True, 6, np.array([1.0, 1.5]))         # one bin: the regions of one cell
    assert one[0][0] == one[1][0] == t[T["underflow"]] and one[2][T["underflow"]] == 0
    # NaNs are in neither phase
    holed = field.copy()
    holed[0, 0, 0] = holed[N - 1, N - 1, N - 1] = holed[N // 2, 1, N // 2] = np.nan
    holed[N // 2, N // 2, :] = np.nan
    lib.grid_to_device(capi.GRID_XH_AV, holed)
    with np.errstate(invalid="ignore"):
        for phase in (0, 1):
            mask = BR.in_phase(holed, 0.5, phase)
            assert not mask[0, 0, 0] and not mask[N // 2, N // 2].any()
            want = RR.sizes(mask, 6, True, RR.default_edges(N))
            got = lib.region_sizes(capi.GRID_XH_AV, 0.5, phase, True, 6, RR.default_edges(N), labels=True)
            assert np.array_equal(got[3], want[0])
            _same(got[:3], want[1:], ("nan", phase))


def test_no_grid_changes_and_the_mfp_call_is_undisturbed(asora, box):
    p, lib, capi = asora
    N, field, _ = box
    held = [capi.GRID_NDENS, capi.GRID_XH_AV, capi.GRID_PHI_ION, capi.GRID_TEMP, capi.GRID_XH, capi.GRID_XH_INTERMED]
    for g in held:                                           # every grid holds data of its own
        if g != capi.GRID_XH:
            lib.grid_to_device(g, np.roll(field, g + 1, axis=g % 3) + g)
    before = [lib.grid_sum(g) for g in held]
    snapshot = lib.grid_to_host(capi.GRID_XH, np.empty((N, N, N)))
    mfp = lambda: lib.bubble_mfp(capi.GRID_XH, 0.5, 0, True, 7, 3000, float(N), np.geomspace(0.5, N, 17), record=True)
    first = mfp()
    lib.region_sizes(capi.GRID_XH, 0.69, 0, True, 6, RR.default_edges(N))
    lib.region_sizes(capi.GRID_XH_AV, 0.3, 1, False, 26, np.array([1.0, 5.0, 50.0]), labels=True)
    second = mfp()                                           # (they share the mask, the edges and the pinned area)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:3], second[:3]))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first[3], second[3]))
    assert [lib.grid_sum(g) for g in held] == before
    assert np.array_equal(lib.grid_to_host(capi.GRID_XH, np.empty((N, N, N))), snapshot) and np.array_equal(snapshot, field)


def test_refusals_and_the_mask_timer(asora, box):
    p, lib, capi = asora
    N, _, _ = box
    e = RR.default_edges(N)
    ok = dict(which=capi.GRID_XH, threshold=0.5, phase=0, periodic=True, connectivity=6, edges=e)
    for change, what in ((dict(which=capi.GRID_CLUMP), "holds no data"), (dict(which=99), "bad grid selector"),
                         (dict(threshold=np.nan), "threshold must be finite"), (dict(threshold=np.inf), "threshold must be finite"),
                         (dict(phase=2), "phase must be"), (dict(connectivity=18), "connectivity must be 6"),
                         (dict(connectivity=0), "connectivity must be 6"), (dict(edges=np.array([1.0])), "n_bins must be"),
                         (dict(edges=np.geomspace(0.5, N, 258)), "n_bins must be"), (dict(edges=np.array([1.0, 1.0, 2.0])), "ascending"),
                         (dict(edges=np.array([2.0, 1.0])), "ascending"), (dict(edges=np.array([1.0, np.nan])), "finite")):
        with pytest.raises(RuntimeError, match=f"region_sizes: .*{what}"):
            lib.region_sizes(**{**ok, **change})
    raw = lib._lib.asora_region_sizes
    out = np.full(14, 9, dtype=np.uint64)
    u64 = lambda a: a.ctypes.data_as(capi._u64p)
    assert raw(capi.GRID_XH, 0.5, 0, 1, 6, 4, capi.dptr(e), u64(out), None, u64(out), None) == 3 and b"null" in lib._lib.asora_last_error()
    assert np.all(out == 9)                                  # (a refused call writes nothing)
    # with the timers on the threshold pass counts where it always has; no selector was added
    lib.set_option(capi.OPT_TIMING, 1)
    lib.kernel_time_reset()
    try:
        assert lib.region_sizes(**ok)[2][T["n_phase"]] > 0   # (and the call still works afterwards)
        times = [lib.kernel_time_ms(k) for k in (capi.KERNEL_BUBBLE_MASK, capi.KERNEL_BUBBLE_SCAN, capi.KERNEL_BUBBLE_RAYS)]
    finally:
        lib.set_option(capi.OPT_TIMING, 0)
    assert [t[1] for t in times] == [1, 0, 0] and times[0][0] > 0.0


def test_module_entry(asora, box):
    p, lib, capi = asora
    from pyc2ray_amd.regions import region_sizes
    N, field, reference = box
    labels, counts, cells, tallies = reference(0.69, 0, 6, False)
    r = region_sizes(field, threshold=0.69, periodic=False, dr=2.0, labels=True)
    assert np.array_equal(r.edges, RR.default_edges(N)) and np.array_equal(r.counts, counts) and np.array_equal(r.cells, cells)
    assert [getattr(r, name) for name in RR.TALLIES] == tallies.tolist() and np.array_equal(r.labels, labels)
    assert r.extent == tuple(tallies[[T["extent_i"], T["extent_j"], T["extent_k"]]].tolist()) and r.percolates == (N in r.extent)
    assert labels[r.largest_index] == r.label_largest and r.fraction_largest == r.v_largest / r.n_phase
    assert r.volume_fraction.sum() == pytest.approx(1.0, rel=1e-14) and r.v_largest_phys == 8.0 * r.v_largest
    same = region_sizes(None, threshold=0.69, periodic=False)          # the grid where it lies
    assert np.array_equal(same.counts, r.counts) and same.sum_v2 == r.sum_v2 and same.dr is None and same.labels is None
    neutral = region_sizes(None, grid=capi.GRID_XH, phase="neutral", threshold=0.69, periodic=False, connectivity=26)
    assert neutral.n_phase == N ** 3 - r.n_phase and neutral.connectivity == 26


@pytest.mark.parametrize("N", [16, 17])
def test_crafted_masks(asora, N):
    p, lib, capi = asora
    _mesh(asora, N)
    i, j, k = np.indices((N, N, N))
    masks = {name: mask for name, (mask, _) in hand_cases(N).items()}
    if N % 2 == 0:
        masks["checkerboard"] = (i + j + k) % 2 == 0
    snake = RR.serpentine(N)
    masks["serpentine"] = snake
    masks["serpentine_rolled"] = np.roll(snake, (3, 2, 5), axis=(0, 1, 2))
    masks["two_cubes"] = two_cubes(N)
    for name, mask in masks.items():
        for connectivity in (6, 26):
            for periodic in (True, False):
                got, want = _run_mask(asora, mask, connectivity, periodic)
                t = got[2]
                if name == "empty":
                    assert not got[0].any() and not got[1].any() and np.all(got[3] == RR.NO_LABEL)
                    assert t.tolist() == [0, 0, 0, 0, RR.NO_LABEL, 0, 0, 0, 0, RR.NO_LABEL, 0, 0, 0, 0]
                if name == "full":
                    assert (t[T["n_regions"]], t[T["v_largest"]], t[T["label_largest"]], t[T["sum_v2"]]) == (1, N ** 3, 0, N ** 6)
                    assert t[T["extent_i"]] == t[T["extent_j"]] == t[T["extent_k"]] == N and t[T["label_second"]] == RR.NO_LABEL
                if name == "checkerboard":
                    assert t[T["n_regions"]] == (N ** 3 // 2 if connectivity == 6 else 1)
                if name == "periodic_corner":
                    assert t[T["n_regions"]] == (1 if connectivity == 26 and periodic else 2)
                if name == "slabs":
                    assert t[T["n_regions"]] == (1 if periodic else 2)
                if name == "serpentine" and connectivity == 6:
                    assert t[T["n_regions"]] == 1 and t[T["label_largest"]] == 0 and t[T["v_largest"]] == snake.sum()
                if name == "serpentine_rolled" and connectivity == 6 and periodic:
                    assert t[T["n_regions"]] == 1 and t[T["label_largest"]] == np.flatnonzero(mask)[0] > 0
                if name == "two_cubes":
                    first, second = (1 * N + 1) * N + 1, (8 * N + 6) * N + 7
                    assert (t[T["v_largest"]], t[T["label_largest"]], t[T["v_second"]], t[T["label_second"]]) == (27, first, 27, second)
                    assert (t[T["extent_i"]], t[T["extent_j"]], t[T["extent_k"]]) == (3, 3, 3)


def _cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_crowded_mask_overflows_every_root_table(asora):
    """N = 216, regions_reference.crowded.  With 6 neighbours every workgroup of region_flatten_kernel meets more distinct roots
    than its LDS table has slots -- asserted for this device's launch by crowded_condition, which tests/test_regions_reference.py
    asserts for 256 CUs without a GPU --, so every workgroup adds run lengths straight onto volume[], beside the sums it empties out
    of the table at its end; every grid-stride loop of the six region kernels takes 19 trips; the regions of 7 have their runs in
    three planes, hence in several workgroups.  With 26 neighbours the same mask is ONE region, whose 4.7 million cells go through
    every workgroup's table: the reference is analytic."""
    p, lib, capi = asora
    N, seed = CROWDED
    _mesh(asora, N)
    cus = _cu_count()
    mask = RR.crowded(N, seed)
    edges = RR.default_edges(N)
    lib.grid_to_device(capi.GRID_XH_AV, mask.astype(np.float64))
    call = lambda connectivity, periodic, **kw: lib.region_sizes(capi.GRID_XH_AV, 0.5, 0, periodic, connectivity, edges, **kw)
    wanted = {}
    for periodic in (True, False):
        want = wanted[periodic] = RR.sizes(mask, 6, periodic, edges)
        fewest, most, trips = crowded_condition(want[0], mask, cus)
        print(f"{cus} CUs, periodic {periodic}: {fewest} ... {most} roots per workgroup for a table of 2048, {trips:.1f} trips")
        got = call(6, periodic, labels=True)
        print(f"    tallies {got[2].tolist()}, reference {want[3].tolist()}")
        assert got[3].dtype == np.uint32 and np.array_equal(got[3], want[0])
        _same(got[:3], want[1:], ("with labels", periodic))
        production = call(6, periodic)
        _same(production, want[1:], ("production", periodic))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(production, call(6, periodic)))
    assert wanted[True][3][T["n_regions"]] != wanted[False][3][T["n_regions"]] and not np.array_equal(wanted[True][0], wanted[False][0])
    assert not np.array_equal(wanted[True][1], wanted[False][1])             # (the open faces make regions of 6 and 5)
    # 26 neighbours: one region, label 0, all of the mask
    V = int(mask.sum())
    b = V.bit_length() - 1
    one = np.where(mask, 0, RR.NO_LABEL).astype(np.uint32)
    for periodic in (True, False):
        got = call(26, periodic, labels=True)
        assert np.array_equal(got[3], one)
        for out in (got[:3], call(26, periodic)):
            counts, cells, t = out
            assert t.tolist() == [V, 1, V * V, V, 0, N, N, N, 0, RR.NO_LABEL, 0, 0, 0, 0], (periodic, t.tolist())
            assert counts[b] == 1 and counts.sum() == 1 and cells[b] == V and cells.sum() == V


def test_threshold_pass_with_more_rows_than_waves(asora):
    """N = 216: the 46 656 rows are more than the waves bubble_mask_kernel is launched with (32 workgroups of 4 per CU), so waves take
    a second row; four words per row, the last with a 24-bit tail."""
    p, lib, capi = asora
    N, seed = CROWDED
    _mesh(asora, N)
    assert N * N > _cu_count() * 32 * 4
    field = BR.blob_field(N, seed)
    lib.grid_to_device(capi.GRID_XH, field)
    for phase in (0, 1):
        words, rows = lib.bubble_mask(capi.GRID_XH, 0.5, phase)
        ref_words, ref_rows = BR.mask_words(BR.in_phase(field, 0.5, phase))
        assert words.shape == (N, N, 4) and np.array_equal(words, ref_words), phase
        assert np.array_equal(rows, ref_rows) and rows.sum() == BR.in_phase(field, 0.5, phase).sum(), phase


def test_class(asora, tmp_path):
    """The single black-body run at its test mesh with the region keys: every step, resident or through the host, leaves its regions
    and one line in the log; regions() reads the ionised fraction where it lies and equals the module-level call on a downloaded
    copy; the steps are bit for bit what they are with the key off."""
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    from pyc2ray_amd.regions import region_sizes
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N, dt = 24, 3.15576e13
        with open("src.txt", "w") as f:
            f.write("1\n12 12 12 5e50 1.0\n")

        def run(params, resident):
            if p.cuda_is_init():
                p.device_close()
            sim = pc2r.C2Ray_Test(params, N, True)
            sim.device_resident = resident
            sim.density_init(0.0)
            srcpos, srcflux = sim.read_sources("src.txt", 1)
            results = []
            for _ in range(2):
                sim.evolve3D(dt, srcflux, srcpos)
                results.append(sim.last_regions)
            return sim, results

        off, off_results = run(PLAIN_PARAMS, True)
        assert off.device_resident and off.region_stats is False and off_results == [None, None]
        r = off.regions(connectivity=26)
        assert off._device_newer >= {"xh", "phi_ion"}          # nothing was fetched
        assert (r.periodic, r.dr, r.connectivity, r.threshold, r.N) == (True, off.dr, 26, 0.5, N) and 0 < r.n_phase < N ** 3
        x_off, phi_off = off.xh.copy(), off.phi_ion.copy()      # (downloads)
        m = region_sizes(x_off.copy(), connectivity=26, dr=off.dr)
        assert np.array_equal(m.counts, r.counts) and np.array_equal(m.cells, r.cells)
        assert [getattr(m, name) for name in RR.TALLIES] == [getattr(r, name) for name in RR.TALLIES]
        want = RR.sizes(x_off >= 0.5, 26, True, RR.default_edges(N))
        assert np.array_equal(m.counts, want[1]) and [getattr(m, name) for name in RR.TALLIES] == want[3].tolist()
        again = off.regions(connectivity=26)                    # the host copy is the newer one now: the upload form
        assert np.array_equal(again.counts, r.counts) and again.sum_v2 == r.sum_v2

        for resident in (True, False):
            on, on_results = run(REGION_PARAMS, resident)
            assert on.device_resident == resident and on.region_stats is True
            assert all(res is not None for res in on_results) and on_results[0] is not on_results[1]
            last = on_results[1]
            assert (last.threshold, last.connectivity, last.dr, last.periodic) == (0.4, 26, on.dr, True)
            assert open(on.logfile).read().count("Regions (ionised, x >= 0.4, 26 neighbours, periodic)") == 2
            x_on = on.xh.copy()
            if resident:                                        # the same path as `off`: the analysis changes nothing of the step
                assert np.array_equal(x_on, x_off) and np.array_equal(on.phi_ion, phi_off)
            want = RR.sizes(x_on >= 0.4, 26, True, RR.default_edges(N))
            assert np.array_equal(last.counts, want[1]) and [getattr(last, name) for name in RR.TALLIES] == want[3].tolist()
            assert last.n_regions == 1 and last.n_phase > on_results[0].n_phase     # one bubble around the source, and it grows
    finally:
        if p.cuda_is_init():
            p.device_close()
        os.chdir(cwd)
