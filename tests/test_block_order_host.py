"""CPU: which workgroup sweeps what in a raytrace launch that is not spread -- the dispatch order of `block_order`
(csrc/raytrace_plan.hpp) through asora_debug_block_order, which needs no device.

Blocks b and b + 8 share an XCD, so the blocks with b % 8 == x are the "lane" of XCD x.  Per unit, in dispatch order (the last unit
first), the groups of the unit's face type -- pairs of the class lists, two consecutive sources, or single sources -- are ordered
stably by their table class and cut into eight contiguous slices whose sizes differ by at most 1; lane x sweeps its slice of every
unit in turn.  Checked on every shape:
  * every (group, unit) exactly once, padding at the lanes' ends only, the grid 8 x the longest lane;
  * what a lane holds of a unit differs by at most 1 between lanes;
  * the units of a lane in dispatch order; within a unit the classes ascending, position order kept within a class;
  * the sources of every group are those of tests/launch_forms.py's restatement of the pairing (`workgroups`).
A launch of at most two workgroups per compute unit is spread and has no order, so the small shapes are asked for with a small
number of compute units.  The window property -- any 64 consecutive entries of a lane (the workgroups resident on an XCD) name at
most 4 distinct (unit, class) tables -- is a statement about lanes whose slice of a unit holds about 64 groups: a window then lies in two
neighbouring slices (two classes each), or takes one entry on either side of a whole slice.  It is asserted on every shape whose
slices hold at least 62 groups.  On the small shapes a lane's whole sequence is shorter than 64 x units / 2 and names every unit
within any 64 entries whatever the order, so there the ascending classes within a slice are what is checked."""
import numpy as np
import pytest

import launch_forms as LF


@pytest.fixture(scope="module")
def lib():
    from pyc2ray_amd.load_extensions import load_asora
    return load_asora()


def positions(seed, N, i_counts, k_counts):
    """A position-sorted source list whose classes along i (z-sector units) and along k (x- / y-sector units) hold the given numbers
    of sources; flat int32."""
    rng = np.random.default_rng(seed)
    n = sum(i_counts)
    assert n == sum(k_counts) and N % 8 == 0
    cols = []
    for counts in (i_counts, k_counts):
        c = np.repeat(np.arange(8), counts)
        cols.append(rng.permutation(c + 8 * rng.integers(0, N // 8, n)))
    p = np.stack([cols[0], rng.integers(0, N, n), cols[1]], axis=1)
    return np.ascontiguousarray(p[LF.sort_order(p)], dtype=np.int32).ravel()


def pair_count(counts):
    return sum((c + 1) // 2 for c in counts)


def face_type(units, u):
    return int({6: u >> 1, 12: u >> 2}.get(units, -1) == 2)


def check(lib, pos0, units, nsrc, aligned, cu_count, begin=0, count=None, window=None):
    p = pos0.reshape(-1, 3)
    count = p.shape[0] - begin if count is None else count
    order = lib.block_order(pos0, units, nsrc, aligned, begin=begin, count=count, cu_count=cu_count)
    assert order is not None and order.shape[0] % 8 == 0
    sub = p[begin:begin + count]
    if nsrc == 2:
        lists = LF.workgroups(sub, aligned)
        lists = [lists[0], lists[-1]]                       # by k (face type 0), by i (face type 1); packed: the one list twice
    else:
        lists = [[(s, -1) for s in range(count)]] * 2
    lists = [[(a + begin, b + begin if b >= 0 else -1) for a, b in l] for l in lists]
    real = order[order[:, 0] >= 0]
    assert np.all(order[order[:, 0] < 0] == -1)
    # every (group, unit) exactly once, with the sources of the restated pairing
    want = {(g, u) for u in range(units) for g in range(len(lists[face_type(units, u)]))}
    got = [(int(g), int(u)) for g, u in real[:, :2]]
    assert len(got) == len(want) and set(got) == want
    for g, u, a, b in real.tolist():
        assert lists[face_type(units, u)][g] == (a, b), (g, u, a, b)
    for u in range(units):
        assert {(a, b) for g, uu, a, b in real.tolist() if uu == u} == set(lists[face_type(units, u)])
    per_unit = np.zeros((8, units), dtype=int)
    longest = 0
    for x in range(8):
        lane = order[x::8]
        valid = lane[:, 0] >= 0
        n = int(valid.sum())
        assert valid[:n].all(), f"lane {x}: padding before its end"
        longest = max(longest, n)
        lane = lane[:n]
        per_unit[x] = np.bincount(lane[:, 1], minlength=units)
        assert np.all(np.diff(lane[:, 1]) <= 0), f"lane {x}: units out of dispatch order"
        cls = np.zeros(n, dtype=int)
        if aligned:
            axis = np.where(np.array([face_type(units, u) for u in lane[:, 1]]) == 1, 0, 2)
            cls = p[lane[:, 2], axis] & 7
            if nsrc == 2:                                  # partners agree in the class
                both = lane[:, 3] >= 0
                assert np.array_equal(p[lane[both, 3], axis[both]] & 7, cls[both])
        key = lane[:, 1] * 8 + cls
        for u in range(units):
            of_u = lane[:, 1] == u
            assert np.all(np.diff(cls[of_u]) >= 0), f"lane {x}, unit {u}: classes not ascending"
            for c in range(8):                             # position order within a class
                assert np.all(np.diff(lane[of_u & (cls == c), 0]) > 0)
        if window:
            for t in range(max(1, n - window + 1)):
                assert len(set(key[t:t + window].tolist())) <= 4, f"lane {x}, entries {t} ...: more than 4 tables"
    assert order.shape[0] == 8 * longest
    assert np.all(per_unit.max(axis=0) - per_unit.min(axis=0) <= 1), per_unit
    if window:
        assert per_unit.min() >= 62
    return order


EVEN = [126, 124, 126, 124, 126, 124, 126, 124]             # 500 pairs: classes of 63 and 62
ALIGNED = {
    # name: (classes along i, classes along k, compute units, window)
    "500_500": (EVEN, EVEN[::-1], 256, 64),
    "87_86": ([22, 22, 22, 22, 22, 22, 22, 18], [21, 21, 22, 22, 22, 22, 22, 20], 16, None),          # k: two odd leftovers
    "13_9": ([2, 2, 2, 2, 2, 2, 2, 4], [1, 1, 1, 1, 3, 3, 3, 5], 1, None),                          # k: eight odd leftovers
    "one_class_empty": ([142, 142, 142, 0, 142, 142, 142, 148], [148, 142, 142, 142, 142, 0, 142, 142], 256, 64),
    "odd_leftovers": ([125] * 8, [127, 123, 125, 125, 121, 129, 125, 125], 256, 64),
}


@pytest.mark.parametrize("units", [6, 12])
@pytest.mark.parametrize("name", list(ALIGNED))
def test_paired_aligned(lib, name, units):
    i_counts, k_counts, cu, window = ALIGNED[name]
    pos0 = positions(3, 64, i_counts, k_counts)
    order = check(lib, pos0, units, 2, True, cu, window=window)
    n_k, n_i = pair_count(k_counts), pair_count(i_counts)
    if name in ("500_500", "87_86", "13_9"):
        assert (n_k, n_i) == {"500_500": (500, 500), "87_86": (87, 86), "13_9": (13, 9)}[name]
    if name == "odd_leftovers":
        assert n_k == 504 and n_i == 504
    z_units = units // 3
    assert (order[:, 0] >= 0).sum() == n_i * z_units + n_k * (units - z_units)


@pytest.mark.parametrize("units", [1, 2])
@pytest.mark.parametrize("nsrc", [1, 2])
@pytest.mark.parametrize("count", [1001, 1000, 37])
def test_unaligned(lib, units, nsrc, count):
    pos0 = positions(4, 64, [count - 7 * (count // 8)] + [count // 8] * 7, [count // 8] * 7 + [count - 7 * (count // 8)])
    order = check(lib, pos0, units, nsrc, False, 32 if count > 37 else 1, window=64 if count > 37 else None)
    # one class: a lane's slice is a run of consecutive groups
    for x in range(8):
        lane = order[x::8]
        lane = lane[lane[:, 0] >= 0]
        for u in range(units):
            assert np.all(np.diff(lane[lane[:, 1] == u, 0]) == 1)


def test_single_sources_six_units(lib):
    """125 sources, one per workgroup, six sectors on line-aligned tables: a source's class is its own."""
    pos0 = positions(5, 64, [16, 16, 16, 16, 16, 15, 15, 15], [15, 16, 15, 16, 15, 16, 16, 16])
    order = check(lib, pos0, 6, 1, True, 64)
    assert (order[:, 0] >= 0).sum() == 750 and order.shape[0] == 8 * max(sum(np.bincount(order[x::8][order[x::8, 1] >= 0, 1])) for x in range(8))


def test_sub_range_and_small_launches(lib):
    """A range of the list (begin > 0, odd count) pairs within the range; a launch of few workgroups is spread and has no order."""
    pos0 = positions(6, 64, EVEN, EVEN)
    check(lib, pos0, 6, 2, True, 128, begin=301, count=499)
    check(lib, pos0, 12, 2, False, 128, begin=7, count=333)
    assert lib.block_order(pos0, 6, 2, True, begin=0, count=100, cu_count=256) is None        # 50-odd pairs x 6 <= 512
    assert lib.block_order(pos0, 6, 1, True, begin=0, count=86, cu_count=256) is not None     # 516 workgroups
    assert lib.block_order(pos0, 6, 1, True, begin=0, count=85, cu_count=256) is None         # 510
    with pytest.raises(RuntimeError, match="bad arguments"):
        lib.block_order(pos0, 8, 1, True)                                                     # aligned tables: 6 or 12 units
