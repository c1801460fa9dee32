"""TEST INFRASTRUCTURE: the numpy statement of the connected-region specification (include/asora_hip.h, asora_region_sizes; DESIGN.md
section 4.2e) -- neighbours, regions and their labels, the histogram of the volumes, the tallies.

``label(mask, connectivity, periodic)`` is a union-find over the cells: every pair of neighbouring in-phase cells is an edge, the
larger root of an edge is hooked under the smaller one (``np.minimum.at``: of several hooks on one root the smallest wins, the
others are met again in the next round), the parents are compressed by pointer jumping, until every edge has both ends under one
root.  Roots only ever hang under smaller cells, so a region's root is its smallest C-order index: its label.
``sizes`` adds what the library call returns.  `mask` is a boolean (N, N, N) array, True where a cell is in phase
(``bubble_reference.in_phase`` makes it from a field).  Pure numpy: no scipy is assumed."""
import itertools

import numpy as np

NO_LABEL = 0xFFFFFFFF
TALLIES = ("n_phase", "n_regions", "sum_v2", "v_largest", "label_largest", "extent_i", "extent_j", "extent_k", "v_second",
           "label_second", "underflow", "underflow_cells", "overflow", "overflow_cells")


def offsets(connectivity):
    """One of each pair of opposite neighbour offsets: 3 of the 6, 13 of the 26."""
    if connectivity == 6:
        return [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    if connectivity == 26:
        return [d for d in itertools.product((-1, 0, 1), repeat=3) if d > (0, 0, 0)]
    raise ValueError("connectivity is 6 or 26")


def edges_of(mask, connectivity, periodic):
    """(a, b): the C-order indices of every pair of neighbouring in-phase cells (a pair may come twice, or join a cell with itself,
    through the wrap of a mesh of 1 or 2 cells: harmless)."""
    N = mask.shape[0]
    idx = np.arange(N ** 3, dtype=np.int64).reshape(N, N, N)
    ea, eb = [], []
    for d in offsets(connectivity):
        if periodic:
            other, other_in = np.roll(idx, [-s for s in d], axis=(0, 1, 2)), np.roll(mask, [-s for s in d], axis=(0, 1, 2))
            both = mask & other_in
            ea.append(idx[both])
            eb.append(other[both])
        else:
            here = tuple(slice(max(0, -s), N - max(0, s)) for s in d)          # cells whose neighbour at +d is in the box
            there = tuple(slice(max(0, s), N - max(0, -s)) for s in d)
            both = mask[here] & mask[there]
            ea.append(idx[here][both])
            eb.append(idx[there][both])
    return np.concatenate(ea), np.concatenate(eb)


def label(mask, connectivity, periodic):
    """The label grid, (N, N, N) uint32: the smallest C-order index of the cell's region, NO_LABEL out of phase."""
    mask = np.asarray(mask, dtype=bool)
    n = mask.size
    parent = np.arange(n, dtype=np.int64)
    a, b = edges_of(mask, connectivity, periodic)
    while True:
        while True:                                   # compress: every cell points at its root
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
        ra, rb = parent[a], parent[b]
        open_ = ra != rb
        if not open_.any():
            break
        a, b, ra, rb = a[open_], b[open_], ra[open_], rb[open_]
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))
    out = np.where(mask.ravel(), parent, NO_LABEL).astype(np.uint32)
    return out.reshape(mask.shape)


def volumes(labels):
    """(labels of the regions ascending, their volumes) of a label grid."""
    flat = labels.ravel()
    roots, vols = np.unique(flat[flat != NO_LABEL], return_counts=True)
    return roots.astype(np.int64), vols.astype(np.int64)


def tally(labels, edges):
    """(counts, cells, tallies) of a label grid: what asora_region_sizes returns next to it."""
    N = labels.shape[0]
    e = np.asarray(edges, dtype=np.float64)
    nb = e.size - 1
    roots, vols = volumes(labels)
    b = np.searchsorted(e, vols.astype(np.float64), "right") - 1
    inside = (b >= 0) & (b < nb)
    counts = np.bincount(b[inside], minlength=nb).astype(np.uint64)
    cells = np.zeros(nb, dtype=np.uint64)
    np.add.at(cells, b[inside], vols[inside].astype(np.uint64))
    t = dict.fromkeys(TALLIES, 0)
    t["label_largest"] = t["label_second"] = NO_LABEL
    t["n_phase"], t["n_regions"] = int(vols.sum()), int(vols.size)
    t["sum_v2"] = sum(int(v) ** 2 for v in vols)
    t["underflow"], t["underflow_cells"] = int(np.sum(b < 0)), int(vols[b < 0].sum())
    t["overflow"], t["overflow_cells"] = int(np.sum(b >= nb)), int(vols[b >= nb].sum())
    if vols.size:
        order = np.lexsort((roots, -vols))              # greatest V first, ties: the smaller label first
        first = order[0]
        t["v_largest"], t["label_largest"] = int(vols[first]), int(roots[first])
        i, j, k = np.nonzero(labels == roots[first])
        t["extent_i"], t["extent_j"], t["extent_k"] = np.unique(i).size, np.unique(j).size, np.unique(k).size
        if vols.size > 1:
            t["v_second"], t["label_second"] = int(vols[order[1]]), int(roots[order[1]])
    return counts, cells, np.array([t[name] for name in TALLIES], dtype=np.uint64)


def sizes(mask, connectivity, periodic, edges):
    """(labels, counts, cells, tallies): everything the library call returns for the mask, all on the CPU."""
    labels = label(mask, connectivity, periodic)
    return (labels,) + tally(labels, edges)


def default_edges(N):
    """The powers of two of region_sizes(bins=None): bin b holds 2^b <= V < 2^(b + 1), and N^3 < 2^nb."""
    return 2.0 ** np.arange((N ** 3).bit_length() + 1)


def partition(labels):
    """A label grid as a canonical partition, whatever the labels are called: every cell gets the smallest C-order index of the cells
    that share its label (the background is one more label)."""
    flat = np.asarray(labels).ravel()
    _, first, inverse = np.unique(flat, return_index=True, return_inverse=True)
    return first[inverse.ravel()].reshape(np.shape(labels))


def crowded(N, seed):
    """The checkerboard (i + j + k even) plus a seeded random half of the odd cells with i % 4 == 1, j % 4 == 0, k % 4 == 0.  Under 6
    neighbours every even cell is a region of its own, except where a filled odd cell joins its six neighbours (five or four
    where j = 0 or k = 0 lies on an open face) into one region of 7 (6, 5): nearly as many regions as a mask can hold, of unequal
    volumes, and the runs of a region of 7 lie in five rows of three planes.  Under 26 neighbours it is one region.  Boolean
    (N, N, N); N a multiple of 4, so that the pattern is the same through the wrap."""
    if N % 4:
        raise ValueError("N is a multiple of 4")
    i, j, k = np.indices((N, N, N))
    sites = (i % 4 == 1) & (j % 4 == 0) & (k % 4 == 0)
    filled = np.zeros((N, N, N), dtype=bool)
    filled[sites] = np.random.default_rng(seed).random(int(sites.sum())) < 0.5
    return ((i + j + k) % 2 == 0) | filled


def run_firsts(mask):
    """True at the first cell of every run of in-phase cells along k inside its row (no wrap)."""
    first = mask.copy()
    first[:, :, 1:] &= ~mask[:, :, :-1]
    return first


def roots_per_workgroup(labels, mask, threads, blocks):
    """(blocks,) int64: how many distinct roots the run-first cells of workgroup (c // threads) % blocks carry, c the C-order
    index -- what a grid-stride launch of `blocks` workgroups of `threads` threads, one thread per cell, puts into one workgroup's
    table of roots."""
    cells = np.flatnonzero(run_firsts(np.asarray(mask, dtype=bool)))
    group = (cells // threads) % blocks
    pairs = np.unique((group.astype(np.int64) << 32) | labels.ravel()[cells].astype(np.int64))
    return np.bincount(pairs >> 32, minlength=blocks)


def serpentine(N):
    """A one-cell-wide path through every second row (i, j even) of the box, rows joined by single cells at alternating ends and
    planes by a single cell: one region under 6 neighbours, open or periodic for odd N, whose union-find chain is the longest a
    mesh can offer.  Boolean (N, N, N), cell (0, 0, 0) in it."""
    m = np.zeros((N, N, N), dtype=bool)
    end = N - 1                              # the k at which the next link sits
    js = list(range(0, N, 2))
    forward = True
    for i in range(0, N, 2):
        order = js if forward else js[::-1]
        for n, j in enumerate(order):
            m[i, j, :] = True
            if n + 1 < len(order):
                m[i, (j + order[n + 1]) // 2, end] = True
                end = 0 if end else N - 1
        if i + 2 < N:
            m[i + 1, order[-1], end] = True
            end = 0 if end else N - 1
        forward = not forward
    return m
