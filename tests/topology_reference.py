"""TEST INFRASTRUCTURE: the numpy statement of the topology specification (include/asora_hip.h, asora_topology; DESIGN.md section
4.2f) -- the lattice elements of a mask and their closed and open counts, the components of the mask and of its complement, the
cavities.

An element is an anchor and a set E of axes; its incident cells lie at the anchor, and one step down along every axis NOT in E.
``elements`` ORs (closed count) and ANDs (open count) the ``np.roll``\\ s of the mask over those offsets and sums over the anchors the
specification names.  In the open box the mask gets one out-of-phase layer behind every axis first: rolled by one, that layer is also
what lies below index 0.  `mask` is a boolean (N, N, N) array, True where a cell is in phase (``bubble_reference.in_phase`` makes
it from a field).  Pure numpy: no scipy is assumed."""
import itertools

import numpy as np

import regions_reference as RR

TALLIES = ("cells", "closed_faces", "closed_edges", "closed_vertices", "open_faces", "open_edges", "open_vertices", "components",
           "complement_components", "cavities")
T = {name: n for n, name in enumerate(TALLIES)}


def elements(mask, periodic):
    """The seven element counts, int64, in the order of the tallies: cells, closed faces, edges, vertices, open faces, edges, vertices."""
    m = np.asarray(mask, dtype=bool)
    N = m.shape[0]
    if not periodic:
        m = np.pad(m, ((0, 1),) * 3)                       # indices N and, through the roll, -1: outside the box, out of phase
    closed, opened = [0] * 4, [0] * 4                      # by dimension |E|
    for E in itertools.chain.from_iterable(itertools.combinations(range(3), n) for n in range(4)):
        free = [ax for ax in range(3) if ax not in E]
        any_in, all_in = np.zeros_like(m), np.ones_like(m)
        for step in itertools.product((0, 1), repeat=len(free)):
            cell = np.roll(m, step, axis=free) if free else m       # cell[anchor] = m[anchor - step]
            any_in |= cell
            all_in &= cell
        # the anchors: periodic 0 ... N - 1 on every axis; open 0 ... N - 1 on the axes in E and 0 ... N on the others
        cut = tuple(slice(0, N) if (periodic or ax in E) else slice(0, N + 1) for ax in range(3))
        closed[len(E)] += int(any_in[cut].sum())
        opened[len(E)] += int(all_in[cut].sum())
    assert closed[3] == opened[3] == int(np.asarray(mask, dtype=bool).sum())
    return np.array([closed[3], closed[2], closed[1], closed[0], opened[2], opened[1], opened[0]], dtype=np.int64)


def dual(connectivity):
    return {6: 26, 26: 6}[connectivity]


def regions(mask, connectivity, periodic):
    """(the regions of the mask, those of them that hold no cell on one of the six faces of the box)"""
    labels = RR.label(mask, connectivity, periodic)
    roots = np.unique(labels[labels != RR.NO_LABEL])
    faces = np.concatenate([labels[0].ravel(), labels[-1].ravel(), labels[:, 0].ravel(), labels[:, -1].ravel(), labels[:, :, 0].ravel(),
                            labels[:, :, -1].ravel()])
    return int(roots.size), int(np.setdiff1d(roots, faces).size)


def tallies(mask, connectivity, periodic):
    """What asora_topology returns for the mask: uint64 [10]."""
    mask = np.asarray(mask, dtype=bool)
    out = np.zeros(len(TALLIES), dtype=np.uint64)
    out[:7] = elements(mask, periodic)
    out[T["components"]] = regions(mask, connectivity, periodic)[0]
    out[T["complement_components"]], enclosed = regions(~mask, dual(connectivity), periodic)
    out[T["cavities"]] = 0 if periodic else enclosed
    return out


def shared_reference(field):
    """``reference(threshold, phase, connectivity, periodic)`` = ``tallies`` of that phase of a field WITHOUT NaNs, computed as it
    is first asked for and kept.  Without NaNs the complement of a phase is the other phase at the same threshold, so one labelling
    serves as a phase's components and as the other phase's complement: half the work on the large meshes of the GPU tests."""
    if np.isnan(field).any():
        raise ValueError("a NaN is in the complement of both phases: no labelling is shared")
    import bubble_reference as BR
    counted, labelled = {}, {}

    def labelling(threshold, phase, connectivity, periodic):
        key = (threshold, phase, connectivity, periodic)
        if key not in labelled:
            labelled[key] = regions(BR.in_phase(field, threshold, phase), connectivity, periodic)
        return labelled[key]

    def reference(threshold, phase, connectivity, periodic):
        if (threshold, phase, periodic) not in counted:
            counted[threshold, phase, periodic] = elements(BR.in_phase(field, threshold, phase), periodic)
        out = np.zeros(len(TALLIES), dtype=np.uint64)
        out[:7] = counted[threshold, phase, periodic]
        out[T["components"]] = labelling(threshold, phase, connectivity, periodic)[0]
        out[T["complement_components"]], enclosed = labelling(threshold, 1 - phase, dual(connectivity), periodic)
        out[T["cavities"]] = 0 if periodic else enclosed
        return out
    return reference


def euler(t, connectivity):
    """chi_26 = V - E + F - C of the closed counts, chi_6 = C - F + E - V of the open ones."""
    t = [int(v) for v in t]
    if connectivity == 26:
        return t[T["closed_vertices"]] - t[T["closed_edges"]] + t[T["closed_faces"]] - t[T["cells"]]
    return t[T["cells"]] - t[T["open_faces"]] + t[T["open_edges"]] - t[T["open_vertices"]]


def betti(t, connectivity):
    """(b0, b1, b2) in the open box: components, b0 + b2 - chi, cavities."""
    b0, b2 = int(t[T["components"]]), int(t[T["cavities"]])
    return b0, b0 + b2 - euler(t, connectivity), b2


# ---- the hand shapes of tests/test_topology_reference.py, shared with tests/test_gpu_topology.py (N = 9, open box) -----------------
def hollow_cube(N=9):
    m = np.zeros((N, N, N), dtype=bool)
    m[2:7, 2:7, 2:7] = True
    m[4, 4, 4] = False
    return m


def ring(N=9):
    m = np.zeros((N, N, N), dtype=bool)
    m[4, 2:7, 2:7] = True
    m[4, 3:6, 3:6] = False
    return m


def one_cell(N=9):
    m = np.zeros((N, N, N), dtype=bool)
    m[4, 4, 4] = True
    return m


def corner_pair(N=9):
    m = np.zeros((N, N, N), dtype=bool)
    m[3, 3, 3] = m[4, 4, 4] = True
    return m


HAND_SHAPES = {"hollow_cube": hollow_cube, "ring": ring, "one_cell": one_cell, "corner_pair": corner_pair}
FULL_BOXES = (1, 2, 3, 5)
