"""TEST INFRASTRUCTURE: the numpy statement of the granulometry specification (include/asora_hip.h, asora_granulometry; DESIGN.md
section 4.2g) -- the exact squared Euclidean distance transform and the erosion and opening counts that follow from it.

``dist2(mask, periodic)`` is the transform, ``counts(mask, periodic, radii)`` what the library call returns.  `mask` is a boolean
(N, N, N) array, True where a cell is in phase (``bubble_reference.in_phase`` makes it from a field).  No scipy: three min-plus
passes, ``out[x] = min over x' of in[x'] + d(x, x')^2``, one axis after the other, int64 inside.  ``brute_dist2`` and
``brute_opening`` are the O(N^6) definitions, for small meshes (tests/test_granulometry_reference.py)."""
import numpy as np

UNBOUNDED = 0xFFFFFFFF
TALLIES = ("n_phase", "d2_max", "n_unbounded", "sum_d2")
_INF = np.int64(1) << np.int64(40)           # "no source yet": above every finite value (< 2^31 + 2^20), far from wrapping


def r2_of(radii):
    """floor(R^2), formed in double."""
    r = np.asarray(radii, dtype=np.float64)
    return np.floor(r * r).astype(np.int64)


def radii_of(r2):
    """Radii whose floor(R^2) is `r2`, safely: the root of r2 + 1/2."""
    return np.sqrt(np.asarray(r2, dtype=np.float64) + 0.5)


def _pass(g, axis, periodic, exterior, cap):
    """One min-plus pass of the int64 grid `g` along `axis`.  The shifts go outward, d = 1, 2, ..., and end as soon as d^2 reaches
    the largest value left (no candidate in[x'] + d^2 >= d^2 can lower anything then) or exceeds `cap` (None: no cap; values above
    the cap need not be exact).  `exterior`: the cells at index -1 and N are sources (open box)."""
    N = g.shape[axis]
    g = np.moveaxis(g, axis, 0)
    out = g.copy()
    if exterior:
        x = np.arange(N, dtype=np.int64)
        face = np.minimum(x + 1, N - x) ** 2
        np.minimum(out, face[:, None, None], out=out)
    for d in range(1, (N // 2 if periodic else N - 1) + 1):
        dd = d * d
        if dd >= out.max() or (cap is not None and dd > cap):
            break
        if periodic:
            np.minimum(out, np.roll(g, d, axis=0) + dd, out=out)
            np.minimum(out, np.roll(g, -d, axis=0) + dd, out=out)
        else:
            np.minimum(out[d:], g[:-d] + dd, out=out[d:])
            np.minimum(out[:-d], g[d:] + dd, out=out[:-d])
    return np.moveaxis(out, 0, axis)


def _transform(sources, periodic, exterior, cap=None):
    """int64 squared distance to the nearest True cell of `sources` (>= _INF where there is none)."""
    g = np.where(sources, np.int64(0), _INF)
    for axis in (2, 1, 0):
        g = _pass(g, axis, periodic, exterior and not periodic, cap)
    return g


def dist2(mask, periodic, exterior_is_source=True):
    """D2 of every cell, (N, N, N) uint32: the squared distance to the nearest cell that is NOT in `mask` (minimum image in a periodic
    box; in an open one the exterior counts as such cells if `exterior_is_source`), UNBOUNDED where no such cell exists."""
    g = _transform(~np.asarray(mask, dtype=bool), periodic, exterior_is_source)
    return np.where(g >= _INF, np.int64(UNBOUNDED), g).astype(np.uint32)


def opened_mask(eroded_mask, periodic, r2):
    """The union of the digital balls of squared radius r2 about the cells of `eroded_mask`: D2' <= r2, the exterior no source."""
    if not eroded_mask.any():
        return np.zeros_like(eroded_mask)
    return _transform(eroded_mask, periodic, False, cap=int(r2)) <= int(r2)


def tallies_of(d2):
    finite = d2[d2 != UNBOUNDED].astype(np.uint64)
    return np.array([np.count_nonzero(d2), finite.max() if finite.size else 0, np.count_nonzero(d2 == UNBOUNDED), finite.sum(dtype=np.uint64)],
                    dtype=np.uint64)


def counts_from_dist2(d2, periodic, radii):
    """(eroded, opened, tallies) of the library call, uint64 arrays, from the transform `d2`."""
    r2 = r2_of(radii)
    eroded, opened = np.zeros(r2.size, dtype=np.uint64), np.zeros(r2.size, dtype=np.uint64)
    for n, r in enumerate(r2):
        e = d2.astype(np.int64) > r
        eroded[n] = np.count_nonzero(e)
        opened[n] = np.count_nonzero(opened_mask(e, periodic, r))
    return eroded, opened, tallies_of(d2)


def counts(mask, periodic, radii):
    """(eroded, opened, tallies, dist2) for a mask."""
    d2 = dist2(mask, periodic)
    return counts_from_dist2(d2, periodic, radii) + (d2,)


# ---- the definitions, O(N^6) ----
def _axis_d2(N, periodic):
    x = np.arange(N, dtype=np.int64)
    d = np.abs(x[:, None] - x[None, :])
    return (np.minimum(d, N - d) if periodic else d) ** 2


def _pair_d2(N, periodic):
    a = _axis_d2(N, periodic)
    return (a[:, None, None, :, None, None] + a[None, :, None, None, :, None] + a[None, None, :, None, None, :]).reshape(N ** 3, N ** 3)


def brute_dist2(mask, periodic, exterior_is_source=True):
    """D2 by the definition: the minimum over every out-of-phase cell, those of one layer of exterior included (open box: the nearest
    exterior cell of c lies in that layer)."""
    mask = np.asarray(mask, dtype=bool)
    N = mask.shape[0]
    if not periodic and exterior_is_source:
        padded = np.zeros((N + 2,) * 3, dtype=bool)
        padded[1:-1, 1:-1, 1:-1] = mask
        return brute_dist2(padded, False, False)[1:-1, 1:-1, 1:-1]
    pair = _pair_d2(N, periodic)
    out = np.flatnonzero(~mask.ravel())
    if out.size == 0:
        return np.full((N, N, N), UNBOUNDED, dtype=np.uint32)
    return pair[:, out].min(axis=1).reshape(N, N, N).astype(np.uint32)


def brute_opening(mask, periodic, r2):
    """(eroded, opened) by the definition: the centres at which the digital ball lies wholly in the phase (open box: and in the box),
    and the union of the balls about them."""
    mask = np.asarray(mask, dtype=bool)
    N = mask.shape[0]
    ball = _pair_d2(N, periodic) <= r2                     # ball[c, x]: x lies in the ball about c, clipped to the box
    inside = ~(ball & ~mask.ravel()[None, :]).any(axis=1)
    if not periodic:                                        # ... and the unclipped ball has to fit: |o|^2 <= r2 per axis
        x = np.arange(N)
        reach = int(np.floor(np.sqrt(r2)))
        fits = (x - reach >= 0) & (x + reach <= N - 1)
        inside &= (fits[:, None, None] & fits[None, :, None] & fits[None, None, :]).ravel()
    opened = ball[inside].any(axis=0) if inside.any() else np.zeros(N ** 3, dtype=bool)
    return int(inside.sum()), int(opened.sum())


# ---- fields of the GPU tests ----
def one_cell_out(N):
    m = np.ones((N, N, N), dtype=bool)
    m[0, 0, 0] = False
    return m


def wrap_slab(N, half=3):
    """The slab k in {N - half ... N - 1, 0 ... half - 1}: one slab through the wrap, two at the faces of an open box."""
    m = np.zeros((N, N, N), dtype=bool)
    m[:, :, :half] = True
    m[:, :, N - half:] = True
    return m


def corner_ball(N, radius=6):
    """The cells within `radius` of the corner (0, 0, 0), by the minimum image: one ball through the wrap, eight octants in an open box."""
    x = np.arange(N)
    d = np.minimum(x, N - x) ** 2
    return d[:, None, None] + d[None, :, None] + d[None, None, :] <= radius * radius


def planes_out(N, planes):
    m = np.ones((N, N, N), dtype=bool)
    m[:, :, list(planes)] = False
    return m


def planes_dist2(N, planes, periodic):
    """D2 of ``planes_out`` by hand: the distance along k to the nearest missing plane (periodic: cyclic; open: or to the exterior),
    and in the open box the distance to the faces along i and j as well."""
    k = np.arange(N, dtype=np.int64)
    d = np.abs(k[:, None] - np.asarray(planes, dtype=np.int64)[None, :])
    if periodic:
        return np.broadcast_to((np.minimum(d, N - d).min(axis=1) ** 2).astype(np.uint32), (N, N, N)).copy()
    face = np.minimum(k + 1, N - k)
    along_k = np.minimum(d.min(axis=1), face)
    return (np.minimum(np.minimum(face[:, None, None], face[None, :, None]), along_k[None, None, :]) ** 2).astype(np.uint32)
