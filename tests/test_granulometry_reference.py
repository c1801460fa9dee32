"""CPU: the numpy statement of the granulometry specification (tests/granulometry_reference.py) pinned on
the O(N^6) definitions at small meshes, on shapes whose distances and counts are known by hand, on the recorded non-monotone pair
of openings, and against scipy.ndimage where scipy is installed.  The GPU tests compare the library with it for equality."""
import numpy as np
import pytest

import bubble_reference as BR
import granulometry_reference as GR

#: (threshold, phase) of the blob fields the GPU tests analyse (bubble_reference.blob_field on GPU_FIELDS' meshes)
BLOB_CASES = [(0.5, 0), (0.5, 1), (0.69, 0), (0.9, 0)]
#: the radii of the GPU tests on the blob fields, and their r2 = floor(R^2)
BLOB_RADII = (1, 1.5, 2, 2.9, 3, 4, 5.5, 8, 12, 20)
#: the squared radii on which the two-transform definition was compared with scipy's binary_opening
CHECKED_R2 = (0, 1, 2, 3, 4, 5, 6, 8, 9, 12, 16, 25)


def test_r2_is_the_floor_of_the_square_in_double():
    assert GR.r2_of(BLOB_RADII).tolist() == [1, 2, 4, 8, 9, 16, 30, 64, 144, 400]
    assert GR.r2_of(GR.radii_of(CHECKED_R2)).tolist() == list(CHECKED_R2)
    assert GR.r2_of([0.0, 0.99, 1.0, 46340.9]).tolist() == [0, 0, 1, int(np.floor(46340.9 ** 2))]


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "open"])
@pytest.mark.parametrize("N", [5, 8, 9])
def test_against_the_definition(N, periodic):
    rng = np.random.default_rng(100 + N)
    masks = [rng.random((N, N, N)) < 0.8, rng.random((N, N, N)) < 0.97, BR.blob_field(N, 3) >= 0.4, GR.one_cell_out(N),
             ~GR.one_cell_out(N)]
    for mask in masks:
        for exterior in (True, False):
            assert np.array_equal(GR.dist2(mask, periodic, exterior), GR.brute_dist2(mask, periodic, exterior))
        r2s = (0, 1, 2, 3, 4, 5, 6, 8, 9)
        eroded, opened, tallies, d2 = GR.counts(mask, periodic, GR.radii_of(r2s))
        for n, r2 in enumerate(r2s):
            assert (int(eroded[n]), int(opened[n])) == GR.brute_opening(mask, periodic, r2), (r2, eroded[n], opened[n])
        assert tallies[0] == mask.sum() and tallies[2] == 0 and tallies[1] == d2.max() and tallies[3] == d2.sum(dtype=np.uint64)


def test_by_hand():
    N = 70
    g = np.arange(N)
    image = np.minimum(g, N - g) ** 2
    # all in phase but the cell (0, 0, 0), periodic: the minimum-image |c|^2
    d2 = GR.dist2(GR.one_cell_out(N), True)
    assert np.array_equal(d2, image[:, None, None] + image[None, :, None] + image[None, None, :]) and d2.max() == 3 * 35 ** 2 == 3675
    # ... open: additionally the bound of the faces
    face = np.minimum(g + 1, N - g) ** 2
    plain = (g ** 2)[:, None, None] + (g ** 2)[None, :, None] + (g ** 2)[None, None, :]
    want = np.minimum(plain, np.minimum(np.minimum(face[:, None, None], face[None, :, None]), face[None, None, :]))
    assert np.array_equal(GR.dist2(GR.one_cell_out(N), False), want)
    # the slab k in {67, 68, 69, 0, 1, 2}, periodic: six planes thick through the wrap
    eroded, opened, tallies, d2 = GR.counts(GR.wrap_slab(N), True, [0, 1, 2, 3])
    assert eroded.tolist() == [6 * N * N, 4 * N * N, 2 * N * N, 0] and opened.tolist() == [6 * N * N, 6 * N * N, 6 * N * N, 0]
    assert tallies.tolist() == [6 * N * N, 9, 0, 2 * (1 + 4 + 9) * N * N]
    # ... open: two slabs of three planes at the faces, where the exterior eats into them
    eroded_open = GR.counts(GR.wrap_slab(N), False, [0, 1, 2, 3])[0]
    assert eroded_open.tolist() == [6 * N * N, 2 * (N - 2) ** 2, 0, 0]
    # the full box: unbounded in the periodic box, the distance to the faces in the open one
    N = 16
    full = np.ones((N, N, N), dtype=bool)
    eroded, opened, tallies, d2 = GR.counts(full, True, [1, 5, 40])
    assert np.all(d2 == GR.UNBOUNDED) and tallies.tolist() == [N ** 3, 0, N ** 3, 0]
    assert eroded.tolist() == opened.tolist() == [N ** 3] * 3
    eroded, opened, tallies, d2 = GR.counts(full, False, [1, 5, 8])
    assert tallies[1] == (N // 2) ** 2 and tallies[2] == 0
    assert eroded.tolist() == [(N - 2) ** 3, (N - 10) ** 3, 0] and opened[2] == 0 and opened[0] < N ** 3     # (the corners go)
    # the empty phase
    eroded, opened, tallies, d2 = GR.counts(~full, True, [1, 2])
    assert not eroded.any() and not opened.any() and not tallies.any() and not d2.any()
    # a ball about the corner through the wrap: its opening by a smaller ball keeps most of it, in the open box far less
    ball = GR.corner_ball(70)
    periodic, opened_box = GR.counts(ball, True, [2, 6, 7]), GR.counts(ball, False, [2, 6, 7])
    assert periodic[0][1] == 1 and periodic[1][1] == ball.sum() and periodic[0][2] == periodic[1][2] == 0
    assert opened_box[0][1] == 0 and opened_box[1][0] < periodic[1][0]


def test_the_by_hand_distances_of_missing_planes():
    """``planes_dist2``, the expected transform of the GPU tests' word-boundary fields, is what ``dist2`` gives."""
    N = 20
    for periodic in (True, False):
        for planes in ((19,), (0,), (0, 19), (7,), (8,), (3, 11)):
            assert np.array_equal(GR.planes_dist2(N, planes, periodic), GR.dist2(GR.planes_out(N, planes), periodic)), (periodic, planes)


def test_the_recorded_non_monotone_pair():
    """Digital balls are no granulometry in the strict sense: on the N = 17 blob field, open box, the opening with r2 = 9 holds more
    cells than the one with r2 = 8.  The counts are reported as they are -- not clipped, not sorted."""
    N, seed = 17, 3
    mask = BR.in_phase(BR.blob_field(N, seed), 0.5, 0)
    opened = GR.counts(mask, False, GR.radii_of(CHECKED_R2))[1]
    assert (int(opened[CHECKED_R2.index(8)]), int(opened[CHECKED_R2.index(9)])) == (479, 482)
    assert np.any(np.diff(opened.astype(np.int64)) > 0)


def _ball(r2):
    reach = int(np.floor(np.sqrt(r2)))
    o = np.arange(-reach, reach + 1) ** 2
    return o[:, None, None] + o[None, :, None] + o[None, None, :] <= r2


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "open"])
def test_against_scipy(periodic):
    """distance_transform_edt on the box padded by one layer of exterior (open) or tiled three times (periodic), and binary_opening
    with the digital ball (its border_value = 0 is the open box's exterior; periodic: the middle tile of three)."""
    ndimage = pytest.importorskip("scipy.ndimage")
    N, seed = 17, 3
    field = BR.blob_field(N, seed)
    for threshold, phase in BLOB_CASES:
        mask = BR.in_phase(field, threshold, phase)
        eroded, opened, tallies, d2 = GR.counts(mask, periodic, GR.radii_of(CHECKED_R2))
        middle = (slice(N, 2 * N),) * 3
        if periodic:
            big = np.tile(mask, (3, 3, 3))
            edt = ndimage.distance_transform_edt(big)[middle]
        else:
            big = mask
            edt = ndimage.distance_transform_edt(np.pad(mask, 1))[1:-1, 1:-1, 1:-1]
        assert np.array_equal(d2, np.rint(edt ** 2).astype(np.uint32))
        for n, r2 in enumerate(CHECKED_R2):
            theirs = ndimage.binary_opening(big, structure=_ball(r2))
            theirs_eroded = ndimage.binary_erosion(big, structure=_ball(r2))
            if periodic:
                theirs, theirs_eroded = theirs[middle], theirs_eroded[middle]
            assert (eroded[n], opened[n]) == (theirs_eroded.sum(), theirs.sum()), (threshold, phase, r2)
