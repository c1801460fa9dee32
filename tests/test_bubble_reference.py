"""CPU: the numpy statement of the mean-free-path bubble sizes (tests/bubble_reference.py) on itself -- the hash, the limiting
geometries, the chord length of a sphere, and the robustness of statuses and bins against the last bits of the directions, which is
what lets tests/test_gpu_bubbles.py compare integer counts without slack."""
import numpy as np
import pytest

import bubble_reference as BR

# (N, seed) of the fields tests/test_gpu_bubbles.py and tests/test_gpu_regions.py use.  The seed of N = 136 is the first of 20 000 at
# which the field has runs along k through all three words of a row (tests/test_regions_reference.py) AND the largest region at
# threshold 0.69 holds 0.3 ... 0.41 of the phase with open boundaries too, as test_gpu_regions.py asserts of every mesh (at this mesh
# the open fraction is 0.21 ... 0.28 for most seeds).
GPU_FIELDS = [(17, 3), (64, 5), (70, 9), (136, 2755)]
L_MAX = lambda N: (3.0, 4.0 * N)                  # ... and its two l_max: one that caps many rays, one beyond every ray
# Its many-ray test, on the first field's ionised phase: two full trips of a ray launch of 256 CUs (8 workgroups of 256 threads
# each: 524 288 threads), 4096 more and an odd tail; the ray seed; (periodic, l_max) of its runs.
MANY_RAYS = 2 * 524_288 + 4096 + 37
MANY_RAYS_SEED = 7
MANY_RAY_CASES = [(True, 3.0), (False, 3.0), (False, 4.0 * GPU_FIELDS[0][0])]


def _mix_int(seed, c):
    """The same hash in Python integers."""
    M = (1 << 64) - 1
    z = (seed + (c + 1) * 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def test_hash_against_hand_computed_values():
    # the first three outputs of splitmix64 seeded with 0 (the published test vector of the generator)
    assert [int(v) for v in BR.mix(0, [0, 1, 2])] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    # a seed and counters that wrap around
    for seed, c in ((12345, 0), (2 ** 64 - 1, 7), (0xDEADBEEFCAFEF00D, 4 * 999_999 + 2)):
        assert int(BR.mix(seed, c)[0]) == _mix_int(seed, c)
    assert BR.u01(np.array([0, 2 ** 64 - 1], dtype=np.uint64)).tolist() == [0.0, 1.0 - 2.0 ** -53]


def test_fully_in_phase_box():
    N, n = 12, 512
    mask = np.ones((N, N, N), dtype=bool)
    start, d = BR.rays(mask, 1, n)
    assert np.allclose(np.sum(d * d, axis=1), 1.0, rtol=0, atol=4e-16)
    L, st = BR.march(mask, start, d, 20.0, True)
    assert np.all(st == BR.CAPPED) and np.all(L == 20.0)
    L, st = BR.march(mask, start, d, 40.0, False)
    assert np.all(st == BR.LEFT_BOX) and np.all(L >= 0.5) and np.all(L <= np.sqrt(3.0) * N)
    counts, tallies, moments = BR.distribution(mask, 1, n, 40.0, False, np.geomspace(0.5, 40.0, 9))
    assert counts.sum() == 0 and tallies.tolist() == [0, 0, n, 0, 0, N ** 3] and moments.tolist() == [0.0, 0.0]


def test_single_in_phase_cell():
    N = 9
    mask = np.zeros((N, N, N), dtype=bool)
    mask[4, 7, 2] = True
    start, d = BR.rays(mask, 5, 2048)
    assert np.all(start == [4, 7, 2])
    for periodic in (True, False):
        L, st = BR.march(mask, start, d, 5.0, periodic)
        assert np.all(st == BR.ENDED) and L.min() >= 0.5 and L.max() <= np.sqrt(3.0) / 2.0
    assert L.min() < 0.51 and L.max() > 0.8            # (the range is used)


def test_selection_is_flatnonzero_order_and_axis_rays_end():
    N = 8
    mask = np.zeros((N, N, N), dtype=bool)
    mask[3, 5, :] = True                                # a line along k
    start, _ = BR.rays(mask, 2, 256)
    assert np.all(start[:, :2] == [3, 5]) and set(start[:, 2]) == set(range(N))
    d = np.tile([0.0, 0.0, -1.0], (4, 1))              # along the line, two components exactly zero
    L, st = BR.march(mask, start[:4], d, 20.0, True)
    assert np.all(st == BR.CAPPED) and np.all(L == 20.0)
    L, st = BR.march(mask, start[:4], d, 20.0, False)
    assert np.all(st == BR.LEFT_BOX) and np.array_equal(L, start[:4, 2] + 0.5)
    d = np.tile([1.0, 0.0, 0.0], (4, 1))               # off the line at the first crossing
    L, st = BR.march(mask, start[:4], d, 20.0, True)
    assert np.all(st == BR.ENDED) and np.all(L == 0.5)


def test_mean_chord_of_a_voxelised_sphere():
    """Rays from uniformly random points of a ball of radius R in isotropic directions reach its surface after 3R/4 on average."""
    N, R, n = 64, 20.0, 20_000
    g = np.arange(N) - 31.5
    mask = (g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2) <= R * R
    start, d = BR.rays(mask, 0, n)
    L, st = BR.march(mask, start, d, float(N), True)
    assert np.all(st == BR.ENDED)
    mean, sem = L.mean(), L.std() / np.sqrt(n)
    print(f"mean length {mean:.3f} +- {sem:.3f} against 3R/4 = {0.75 * R}")
    assert abs(mean - 0.75 * R) <= 0.03 * 0.75 * R


def _shift(d, ulps):
    out = d.copy()
    for _ in range(4):
        out = np.nextafter(out, np.where(ulps > 0, np.inf, -np.inf))
    return out


def _unmoved_by_four_ulp(mask, start, d, l_max, periodic, name):
    """Asserts that three patterns of 4-ulp shifts of every direction component leave the statuses and the bins (32 geometric ones
    up to l_max, as the GPU tests have them) of the rays as they are; the largest relative change of a length."""
    edges = np.geomspace(0.5, l_max, 33)
    L0, s0 = BR.march(mask, start, d, l_max, periodic)
    b0 = np.searchsorted(edges, L0, "right")
    rng = np.random.default_rng(1)
    worst = 0.0
    for ulps in (np.ones_like(d), -np.ones_like(d), rng.choice([-1.0, 1.0], size=d.shape)):
        L1, s1 = BR.march(mask, start, _shift(d, ulps), l_max, periodic)
        assert np.array_equal(s0, s1), name
        assert np.array_equal(b0, np.searchsorted(edges, L1, "right")), name
        worst = max(worst, float(np.max(np.abs(L1 - L0) / L0)))
    return worst


def _fields():
    rng = np.random.default_rng(24)
    plain = rng.random((24, 24, 24))
    yield "uniform 24^3, 0.5", plain, 0.5, 0
    yield "uniform 24^3, 0.9", plain, 0.9, 0
    for N, seed in GPU_FIELDS:
        f = BR.blob_field(N, seed)
        yield f"blob {N}^3, ionised", f, 0.5, 0
        yield f"blob {N}^3, neutral", f, 0.5, 1


@pytest.mark.parametrize("periodic", [True, False])
def test_four_ulp_of_the_directions_change_no_status_and_no_bin(periodic):
    """The device's cos, sin and sqrt may differ from numpy's in the last bits.  On the fields of the GPU tests (and on a plain
    uniform-random one) no ray passes so close to a cell corner, a bin edge or l_max that 4 ulp of every direction component decide
    where it ends or which bin it falls in: the statuses and the bins of 4096 rays stay as they are, for both seeds, both l_max
    and three patterns of shifts."""
    n = 4096
    worst = 0.0
    for name, field, thr, phase in _fields():
        mask = BR.in_phase(field, thr, phase)
        N = mask.shape[0]
        for seed in (0, 7):
            start, d = BR.rays(mask, seed, n)
            for l_max in L_MAX(N):
                worst = max(worst, _unmoved_by_four_ulp(mask, start, d, l_max, periodic, name))
    print(f"largest relative change of a length: {worst:.3e}")
    # 4 ulp of d are at most 8.9e-16 of it, and 1 / |d| and the product round once each, in both marches
    assert worst <= 4 * 2.0 ** -52 + 4 * 2.0 ** -53


@pytest.mark.parametrize("periodic,l_max", MANY_RAY_CASES, ids=lambda v: str(v))
def test_four_ulp_change_no_status_and_no_bin_of_the_many_rays(periodic, l_max):
    """The same for exactly the ray set of test_gpu_bubbles.py's many-ray test -- MANY_RAYS rays of seed MANY_RAYS_SEED in the ionised
    phase of the smallest field, at the boundaries and l_max that test runs --, which is what lets it compare the counts of a
    million rays with the all-CPU reference without slack."""
    N, seed = GPU_FIELDS[0]
    mask = BR.in_phase(BR.blob_field(N, seed), 0.5, 0)
    start, d = BR.rays(mask, MANY_RAYS_SEED, MANY_RAYS)
    worst = _unmoved_by_four_ulp(mask, start, d, l_max, periodic, f"{MANY_RAYS} rays")
    print(f"periodic {periodic}, l_max {l_max}: largest relative change of a length {worst:.3e}")
    assert worst <= 4 * 2.0 ** -52 + 4 * 2.0 ** -53


def test_lengths_move_by_1e_15_at_most():
    """A 24^3 uniform-random field at the thresholds 0.5 and 0.9, 4096 rays, every direction component moved by 4 ulp: no length
    changes by more than 1e-15 of itself.  The figure is the largest of 4096 errors whose supremum is 1.33e-15 (the test above):
    9.9e-16 and 9.5e-16 for the two thresholds with this field and ray seed; other ray seeds and the fields of the GPU tests give
    9.3e-16 ... 1.07e-15."""
    field = np.random.default_rng(24).random((24, 24, 24))
    for thr in (0.5, 0.9):
        mask = BR.in_phase(field, thr, 0)
        start, d = BR.rays(mask, 7, 4096)
        L0, s0 = BR.march(mask, start, d, 24.0, True)
        for sign in (1.0, -1.0):
            L1, s1 = BR.march(mask, start, _shift(d, sign * np.ones_like(d)), 24.0, True)
            worst = float(np.max(np.abs(L1 - L0) / L0))
            print(f"threshold {thr}, {sign:+.0f} x 4 ulp: largest relative change of a length {worst:.3e}")
            assert np.array_equal(s0, s1) and worst <= 1e-15
