"""CPU: the numpy statement of the topology specification (tests/topology_reference.py) pinned on shapes
whose element counts, Euler characteristics and Betti numbers are known by hand, on the full box, by two identities on the blob
fields, and against scipy.ndimage.label where scipy is installed.  The GPU tests compare the library with it for equality."""
import numpy as np
import pytest

import bubble_reference as BR
import topology_reference as TR

T = TR.T
#: (threshold, phase) of the blob fields the GPU tests analyse (bubble_reference.blob_field on GPU_FIELDS' meshes)
BLOB_CASES = [(0.5, 0), (0.5, 1), (0.69, 0), (0.9, 0)]


def _vefc(t):
    """(closed, open) counts in the order vertices, edges, faces, cells"""
    t = [int(v) for v in t]
    return ([t[T["closed_vertices"]], t[T["closed_edges"]], t[T["closed_faces"]], t[T["cells"]]],
            [t[T["open_vertices"]], t[T["open_edges"]], t[T["open_faces"]], t[T["cells"]]])


def test_known_answers_in_the_open_box():
    N = 9
    for connectivity in (6, 26):
        t = TR.tallies(TR.hollow_cube(N), connectivity, False)          # a 5^3 cube with its centre removed
        assert _vefc(t) == ([216, 540, 450, 124], [56, 228, 294, 124])
        assert TR.euler(t, 6) == TR.euler(t, 26) == 2 and TR.betti(t, connectivity) == (1, 0, 1)
        assert t[T["complement_components"]] == 2
        t = TR.tallies(TR.ring(N), connectivity, False)                 # a 5 x 5 ring, one cell thick, with a 3 x 3 hole
        assert _vefc(t) == ([64, 128, 80, 16], [0, 0, 16, 16])
        assert TR.euler(t, 6) == TR.euler(t, 26) == 0 and TR.betti(t, connectivity) == (1, 1, 0)
        t = TR.tallies(TR.one_cell(N), connectivity, False)
        assert _vefc(t) == ([8, 12, 6, 1], [0, 0, 0, 1]) and TR.euler(t, 6) == TR.euler(t, 26) == 1
        assert TR.betti(t, connectivity) == (1, 0, 0)
    # two cells that touch at a corner: two components of open cubes, one of closed cubes
    t6, t26 = TR.tallies(TR.corner_pair(N), 6, False), TR.tallies(TR.corner_pair(N), 26, False)
    assert TR.euler(t6, 6) == 2 and TR.euler(t26, 26) == 1
    assert t6[T["components"]] == 2 and t26[T["components"]] == 1
    assert np.array_equal(t6[:7], t26[:7])                              # (both sets of counts, whatever the connectivity)
    assert TR.betti(t6, 6) == (2, 0, 0) and TR.betti(t26, 26) == (1, 0, 0)


@pytest.mark.parametrize("N", TR.FULL_BOXES)
def test_full_box(N):
    full = np.ones((N, N, N), dtype=bool)
    for connectivity in (6, 26):
        t = TR.tallies(full, connectivity, True)
        closed, opened = _vefc(t)
        assert closed == opened == [N ** 3, 3 * N ** 3, 3 * N ** 3, N ** 3]
        assert TR.euler(t, 6) == TR.euler(t, 26) == 0
        assert (t[T["components"]], t[T["complement_components"]], t[T["cavities"]]) == (1, 0, 0)
        t = TR.tallies(full, connectivity, False)
        closed, opened = _vefc(t)
        assert closed == [(N + 1) ** 3, 3 * N * (N + 1) ** 2, 3 * N * N * (N + 1), N ** 3]
        assert opened == [(N - 1) ** 3, 3 * N * (N - 1) ** 2, 3 * N * N * (N - 1), N ** 3]
        assert TR.euler(t, 6) == TR.euler(t, 26) == 1 and TR.betti(t, connectivity) == (1, 0, 0)
        empty = TR.tallies(~full, connectivity, False)
        assert not empty[:8].any() and empty[T["complement_components"]] == 1 and empty[T["cavities"]] == 0


@pytest.mark.parametrize("N,seed", [(17, 3), (33, 4)])
def test_identities_on_the_blob_fields(N, seed):
    """Periodic: every element of the torus' lattice is in the closed complex of the phase or in the open complex of the complement
    and never in both, and the lattice of the whole torus has chi = 0; with the signs of the two definitions that makes chi under a
    connectivity of the phase EQUAL to chi under the dual connectivity of the complement.  Open: the first Betti number is a count,
    so >= 0."""
    field = BR.blob_field(N, seed)
    for threshold in (0.3, 0.5, 0.69, 0.9):
        mask = BR.in_phase(field, threshold, 0)
        for connectivity in (6, 26):
            t, tc = TR.tallies(mask, connectivity, True), TR.tallies(~mask, TR.dual(connectivity), True)
            assert TR.euler(t, connectivity) == TR.euler(tc, TR.dual(connectivity)), (threshold, connectivity)
            assert t[T["complement_components"]] == tc[T["components"]] and t[T["cells"]] + tc[T["cells"]] == N ** 3
            to = TR.tallies(mask, connectivity, False)
            assert TR.betti(to, connectivity)[1] >= 0, (threshold, connectivity)
            assert not np.array_equal(to[:7], t[:7])                    # (the boundary matters on these fields)


def test_shared_reference_is_the_plain_statement():
    """The economy of the GPU tests (one labelling per phase, connectivity and boundary, used as a phase's components and as the
    other phase's complement) gives what ``tallies`` gives."""
    N, seed = 17, 3
    field = BR.blob_field(N, seed)
    reference = TR.shared_reference(field)
    for threshold, phase in BLOB_CASES:
        for connectivity in (6, 26):
            for periodic in (True, False):
                want = TR.tallies(BR.in_phase(field, threshold, phase), connectivity, periodic)
                assert np.array_equal(reference(threshold, phase, connectivity, periodic), want), (threshold, phase, connectivity, periodic)
    holed = field.copy()
    holed[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="no labelling is shared"):
        TR.shared_reference(holed)


def test_periodic_counts_do_not_depend_on_the_origin():
    N = 17
    mask = BR.in_phase(BR.blob_field(N, 3), 0.69, 0)
    rolled = np.roll(mask, (3, N - 1, 5), axis=(0, 1, 2))
    for connectivity in (6, 26):
        assert np.array_equal(TR.tallies(mask, connectivity, True), TR.tallies(rolled, connectivity, True))


@pytest.mark.parametrize("N,seed", [(17, 3), (32, 4)])
def test_components_against_scipy_open_boundaries(N, seed):
    ndimage = pytest.importorskip("scipy.ndimage")
    field = BR.blob_field(N, seed)
    for threshold, phase in BLOB_CASES:
        mask = BR.in_phase(field, threshold, phase)
        for connectivity in (6, 26):
            t = TR.tallies(mask, connectivity, False)
            rank = {6: 1, 26: 3}
            assert t[T["components"]] == ndimage.label(mask, structure=ndimage.generate_binary_structure(3, rank[connectivity]))[1]
            theirs, n = ndimage.label(~mask, structure=ndimage.generate_binary_structure(3, rank[TR.dual(connectivity)]))
            assert t[T["complement_components"]] == n
            on_faces = np.unique(np.concatenate([theirs[0].ravel(), theirs[-1].ravel(), theirs[:, 0].ravel(), theirs[:, -1].ravel(),
                                                 theirs[:, :, 0].ravel(), theirs[:, :, -1].ravel()]))
            assert t[T["cavities"]] == n - np.count_nonzero(on_faces)
