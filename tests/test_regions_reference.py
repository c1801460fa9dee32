"""CPU: the numpy statement of the connected-region specification (tests/regions_reference.py) pinned on
hand-built masks, against scipy.ndimage.label where scipy is installed, and by the invariance of the volumes under a periodic shift.
The GPU tests compare the library with it for equality."""
import numpy as np
import pytest

import bubble_reference as BR
import regions_reference as RR

#: (threshold, phase, connectivity) of the blob fields the GPU tests label (bubble_reference.blob_field on GPU_FIELDS' meshes)
BLOB_CASES = [(0.5, 0, 6), (0.5, 1, 6), (0.69, 0, 6), (0.9, 0, 26)]

#: (N, seed) of regions_reference.crowded in the GPU test of the table overflow, and of the blob field whose mask it takes beside it
CROWDED = (216, 2)
#: the launch of the region kernels (csrc/region_label.hip): threads per workgroup, workgroups per CU, slots of the LDS root table
RG_THREADS, RG_BLOCKS_PER_CU, RG_HASH = 256, 8, 2048

T = {name: n for n, name in enumerate(RR.TALLIES)}


def _idx(N, i, j, k):
    return (i * N + j) * N + k


def hand_cases(N):
    """name -> (mask, {(connectivity, periodic): (sorted volumes, label of the largest, extent of the largest)}): the hand-built
    masks, shared with tests/test_gpu_regions.py.  N >= 4."""
    both = [(c, p) for c in (6, 26) for p in (True, False)]
    cases = {}
    single = np.zeros((N, N, N), dtype=bool)
    single[1, 2, 3] = True
    cases["single"] = (single, {cp: ([1], _idx(N, 1, 2, 3), (1, 1, 1)) for cp in both})
    cases["full"] = (np.ones((N, N, N), dtype=bool), {cp: ([N ** 3], 0, (N, N, N)) for cp in both})
    cases["empty"] = (np.zeros((N, N, N), dtype=bool), {cp: ([], RR.NO_LABEL, (0, 0, 0)) for cp in both})
    corner = np.zeros((N, N, N), dtype=bool)
    corner[1, 1, 1] = corner[2, 2, 2] = True
    cases["corner"] = (corner, {(c, p): (([1, 1], _idx(N, 1, 1, 1), (1, 1, 1)) if c == 6 else ([2], _idx(N, 1, 1, 1), (2, 2, 2)))
                                for c, p in both})
    wrap = np.zeros((N, N, N), dtype=bool)
    wrap[0, 0, 0] = wrap[N - 1, N - 1, N - 1] = True
    cases["periodic_corner"] = (wrap, {(c, p): (([2], 0, (2, 2, 2)) if (c == 26 and p) else ([1, 1], 0, (1, 1, 1))) for c, p in both})
    slabs = np.zeros((N, N, N), dtype=bool)
    slabs[0] = slabs[N - 1] = True
    cases["slabs"] = (slabs, {(c, p): (([2 * N * N], 0, (2, N, N)) if p else ([N * N, N * N], 0, (1, N, N))) for c, p in both})
    return cases


def _check(mask, connectivity, periodic, vols, label_largest, extent):
    N = mask.shape[0]
    labels, counts, cells, t = RR.sizes(mask, connectivity, periodic, RR.default_edges(N))
    roots, v = RR.volumes(labels)
    assert sorted(v.tolist()) == sorted(vols)
    assert labels.dtype == np.uint32 and np.array_equal(labels != RR.NO_LABEL, mask)
    assert np.all(labels.ravel()[roots] == roots)                    # a label is a cell of its region ...
    assert np.all(labels[mask] <= np.flatnonzero(mask))              # ... and the smallest of them
    assert t[T["n_phase"]] == mask.sum() == sum(vols) and t[T["n_regions"]] == len(vols) and t[T["sum_v2"]] == sum(x * x for x in vols)
    assert t[T["v_largest"]] == (max(vols) if vols else 0) and t[T["label_largest"]] == label_largest
    assert tuple(t[[T["extent_i"], T["extent_j"], T["extent_k"]]].tolist()) == extent
    assert counts.sum() == len(vols) and cells.sum() == sum(vols) and not t[T["underflow"]:].any()
    for b in np.flatnonzero(counts):                                 # bin b: 2^b <= V < 2^(b + 1)
        assert counts[b] == sum(1 for x in vols if 2 ** b <= x < 2 ** (b + 1))
        assert cells[b] == sum(x for x in vols if 2 ** b <= x < 2 ** (b + 1))
    return t


@pytest.mark.parametrize("N", [4, 5, 16, 17])
def test_hand_built_masks(N):
    for name, (mask, expect) in hand_cases(N).items():
        for (connectivity, periodic), (vols, first, extent) in expect.items():
            t = _check(mask, connectivity, periodic, vols, first, extent)
            if len(vols) == 2 and vols[0] == vols[1]:                # a tie: the smaller label is the largest, the other the second
                assert t[T["v_second"]] == vols[0] and t[T["label_largest"]] < t[T["label_second"]] != RR.NO_LABEL, name
            elif len(vols) < 2:
                assert t[T["v_second"]] == 0 and t[T["label_second"]] == RR.NO_LABEL, name


@pytest.mark.parametrize("N", [4, 16])
def test_checkerboard(N):
    i, j, k = np.indices((N, N, N))
    board = (i + j + k) % 2 == 0
    for periodic in (True, False):
        _check(board, 6, periodic, [1] * (N ** 3 // 2), 0, (1, 1, 1))
        _check(board, 26, periodic, [N ** 3 // 2], 0, (N, N, N))


def test_meshes_of_one_and_two_cells():
    """Through the wrap a cell is its own neighbour (N = 1) or meets the same neighbour twice (N = 2): harmless."""
    for periodic in (True, False):
        for connectivity in (6, 26):
            _check(np.ones((1, 1, 1), dtype=bool), connectivity, periodic, [1], 0, (1, 1, 1))
            _check(np.ones((2, 2, 2), dtype=bool), connectivity, periodic, [8], 0, (2, 2, 2))
            diag = np.zeros((2, 2, 2), dtype=bool)
            diag[0, 0, 0] = diag[1, 1, 1] = True
            if connectivity == 26:
                _check(diag, 26, periodic, [2], 0, (2, 2, 2))
            else:
                _check(diag, 6, periodic, [1, 1], 0, (1, 1, 1))


def test_serpentine_and_tie():
    for N in (16, 17):
        snake = RR.serpentine(N)
        assert snake[0, 0, 0] and not snake[1::2, 1::2].any()
        for periodic in (True, False):
            labels = RR.label(snake, 6, periodic)
            assert np.all(labels[snake] == 0)
            rolled = np.roll(snake, (3, 2, 5), axis=(0, 1, 2))           # (periodic: still one region, its smallest index elsewhere)
            if periodic:
                lr = RR.label(rolled, 6, True)
                assert np.unique(lr[rolled]).size == 1 and lr[rolled][0] == np.flatnonzero(rolled)[0]
        cubes = two_cubes(N)
        t = RR.tally(RR.label(cubes, 6, True), RR.default_edges(N))[2]
        assert (t[T["v_largest"]], t[T["label_largest"]], t[T["v_second"]], t[T["label_second"]]) == (27, _idx(N, 1, 1, 1), 27, _idx(N, 8, 6, 7))
        assert t[T["n_regions"]] == 2 and t[T["sum_v2"]] == 2 * 27 * 27


def two_cubes(N):
    """Two 3^3 cubes that do not touch: a tie in V (shared with the GPU tests)."""
    m = np.zeros((N, N, N), dtype=bool)
    m[1:4, 1:4, 1:4] = True
    m[8:11, 6:9, 7:10] = True
    return m


def test_explicit_edges_under_and_overflow():
    N = 17
    mask = BR.in_phase(BR.blob_field(N, 3), 0.69, 0)
    labels = RR.label(mask, 6, True)
    _, vols = RR.volumes(labels)
    edges = np.array([2.0, 3.0, 10.0, 100.0])
    counts, cells, t = RR.tally(labels, edges)
    assert counts.tolist() == [int(np.sum(vols == 2)), int(np.sum((vols >= 3) & (vols < 10))), int(np.sum((vols >= 10) & (vols < 100)))]
    assert cells.tolist() == [int(vols[vols == 2].sum()), int(vols[(vols >= 3) & (vols < 10)].sum()), int(vols[(vols >= 10) & (vols < 100)].sum())]
    assert t[T["underflow"]] == t[T["underflow_cells"]] == np.sum(vols == 1) > 0
    assert t[T["overflow"]] == np.sum(vols >= 100) > 0 and t[T["overflow_cells"]] == vols[vols >= 100].sum()
    assert counts.sum() + t[T["underflow"]] + t[T["overflow"]] == t[T["n_regions"]]
    assert cells.sum() + t[T["underflow_cells"]] + t[T["overflow_cells"]] == t[T["n_phase"]]


@pytest.mark.parametrize("N,seed", [(17, 3), (32, 4)])
def test_against_scipy_open_boundaries(N, seed):
    ndimage = pytest.importorskip("scipy.ndimage")
    field = BR.blob_field(N, seed)
    for threshold, phase, connectivity in BLOB_CASES + [(0.5, 0, 26)]:
        mask = BR.in_phase(field, threshold, phase)
        structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
        theirs, n = ndimage.label(mask, structure=structure)
        ours = RR.label(mask, connectivity, False)
        assert np.array_equal(RR.partition(ours), RR.partition(theirs))             # the same partition, whatever the labels are called
        roots, vols = RR.volumes(ours)
        assert roots.size == n and np.array_equal(np.sort(vols), np.sort(np.bincount(theirs.ravel())[1:]))


@pytest.mark.parametrize("N,seed", [(17, 3), (32, 4)])
def test_periodic_volumes_do_not_depend_on_the_origin(N, seed):
    field = BR.blob_field(N, seed)
    for threshold, phase, connectivity in BLOB_CASES:
        mask = BR.in_phase(field, threshold, phase)
        vols = np.sort(RR.volumes(RR.label(mask, connectivity, True))[1])
        rolled = np.roll(mask, (3, N - 1, 5), axis=(0, 1, 2))
        assert np.array_equal(np.sort(RR.volumes(RR.label(rolled, connectivity, True))[1]), vols)
        open_vols = np.sort(RR.volumes(RR.label(mask, connectivity, False))[1])
        assert open_vols.size > vols.size                       # (the wrap joins regions: open and periodic differ on these fields)


def launch_blocks(N, cus):
    """Workgroups of a region kernel at mesh N on a chip of `cus` compute units."""
    return min((N ** 3 + RG_THREADS - 1) // RG_THREADS, cus * RG_BLOCKS_PER_CU)


def crowded_condition(labels, mask, cus):
    """What makes the crowded mask a test of region_flatten_kernel's overflow on a chip of `cus` compute units (shared with
    tests/test_gpu_regions.py, which asserts it for the device it runs on): every workgroup meets more distinct roots than its
    table has slots, so by pigeonhole every workgroup adds some run straight to global memory, and every thread of the
    grid-stride loops takes more than 16 trips.  Returns (fewest, most) roots of a workgroup and the trips."""
    N = mask.shape[0]
    blocks = launch_blocks(N, cus)
    per = RR.roots_per_workgroup(labels, mask, RG_THREADS, blocks)
    trips = N ** 3 / (blocks * RG_THREADS)
    assert per.size == blocks and per.min() > RG_HASH, (cus, blocks, int(per.min()), int(per.max()))
    assert N ** 3 > 16 * blocks * RG_THREADS, (cus, blocks, trips)
    return int(per.min()), int(per.max()), trips


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "open"])
def test_crowded_mask_overflows_every_root_table_of_256_cus(periodic):
    N, seed = CROWDED
    mask = RR.crowded(N, seed)
    i, j, k = np.indices((N, N, N))
    odd = mask & ((i + j + k) % 2 == 1)
    filled = int(odd.sum())
    assert np.all(mask[(i + j + k) % 2 == 0]) and 0.45 * (N // 4) ** 3 < filled < 0.55 * (N // 4) ** 3
    assert np.all(i[odd] % 4 == 1) and np.all(j[odd] % 4 == 0) and np.all(k[odd] % 4 == 0)
    labels = RR.label(mask, 6, periodic)
    roots, vols = RR.volumes(labels)
    # a filled odd cell and its six neighbours (five or four of them where j = 0 or k = 0 lies on an open face); every other cell alone
    at_face = (j[odd] == 0).astype(int) + (k[odd] == 0).astype(int)
    joined = np.full(filled, 7) if periodic else 7 - at_face
    want = {int(v): int(c) for v, c in zip(*np.unique(joined, return_counts=True))}
    want[1] = N ** 3 // 2 - int((joined - 1).sum())
    assert {int(v): int(c) for v, c in zip(*np.unique(vols, return_counts=True))} == want
    assert len(want) == (2 if periodic else 4)                       # (the volumes are not all equal)
    # the runs of one region lie in several workgroups: the seven cells of the first filled site
    c = np.flatnonzero(odd)[0]
    members = np.flatnonzero(labels.ravel() == labels.ravel()[c - N * N])
    assert c in members and np.unique((members // RG_THREADS) % launch_blocks(N, 256)).size >= 3
    fewest, most, trips = crowded_condition(labels, mask, 256)
    print(f"crowded({N}, {seed}), periodic {periodic}: {roots.size} regions, {fewest} ... {most} roots per workgroup, {trips:.1f} trips")


def test_the_136_field_has_runs_through_three_mask_words():
    """At threshold 0.5 the ionised phase of the N = 136 field of the GPU tests holds runs along k that begin in word 0 and end in
    word 2: region_init_kernel walks back two words from their last cells, region_flatten_kernel forward two words from their first."""
    from test_bubble_reference import GPU_FIELDS
    (N, seed), = [f for f in GPU_FIELDS if f[0] > 128]
    assert (N + 63) // 64 == 3 and N % 64 == 8
    mask = BR.in_phase(BR.blob_field(N, seed), 0.5, 0)
    through = mask[:, :, 63:129].all(axis=2)                 # cells 63 ... 128 in phase: the run begins at k < 64 and ends at k >= 128
    print(f"blob_field({N}, {seed}) >= 0.5: {int(through.sum())} runs begin in word 0 and end in word 2")
    assert through.sum() >= 1
    # ... and one of them ends short of the row's end, one begins after its start: both walks stop on a bit, not on the row's edge
    assert np.any(through & ~mask[:, :, N - 1]) and np.any(through & ~mask[:, :, 0])
