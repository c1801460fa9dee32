"""TEST INFRASTRUCTURE: the numpy statement of the halo-catalogue sources (include/asora_hip.h, asora_halo_catalogue_to_device and
asora_halo_sources_build), operation by operation: floor, Python's %, rint, integer sums with np.add.at, a walk
over the occupied cells in ascending index, three products, a sum and a product.  ``table_loop`` says the same with a plain Python
loop over the haloes and exact Python integers (tests/test_halo_sources_reference.py compares the two)."""
import math

import numpy as np

NONE, FULL, PARTIAL = range(3)
MODELS = {"none": NONE, "full": FULL, "partial": PARTIAL}


def unit_exponent(weights):
    """ceil(log2(sum of the weights)) - 61; 0 for a sum of 0"""
    total = float(np.sum(np.asarray(weights, dtype=np.float64)))
    if not total > 0.0:
        return 0
    m, ex = math.frexp(total)
    return (ex - 1 if m == 0.5 else ex) - 61


def table(pos, mass, weight, N, m_lm, m_hm, wrap, e):
    """(cell int64, Q_hm uint64, Q_lm uint64) of the occupied cells in ascending index, and the counts
    dict(n_cells, outside, nonfinite, below)"""
    pos, mass, weight = (np.asarray(a, dtype=np.float64) for a in (pos, mass, weight))
    with np.errstate(invalid="ignore"):
        finite = np.all(np.abs(pos) < 2.0 ** 31, axis=1)             # (False for a NaN and for an infinity)
    c = np.floor(np.where(finite[:, None], pos, 0.0)).astype(np.int64)
    if wrap:
        c = c % N
        inside = finite
    else:
        inside = finite & np.all((c >= 0) & (c < N), axis=1)
    with np.errstate(invalid="ignore"):
        hm = inside & (mass >= m_hm)
        lm = inside & ~hm & (mass >= m_lm) & (mass < m_hm)
    counts = dict(outside=int(np.sum(finite & ~inside)), nonfinite=int(np.sum(~finite)), below=int(np.sum(inside & ~hm & ~lm)))
    q = np.rint(np.ldexp(weight, -e)).astype(np.uint64)
    index = (c[:, 0] * N + c[:, 1]) * N + c[:, 2]
    q_hm, q_lm = np.zeros(N ** 3, dtype=np.uint64), np.zeros(N ** 3, dtype=np.uint64)
    np.add.at(q_hm, index[hm], q[hm])
    np.add.at(q_lm, index[lm], q[lm])
    cell = np.flatnonzero(q_hm + q_lm > 0).astype(np.int64)
    counts["n_cells"] = int(cell.size)
    return cell, q_hm[cell], q_lm[cell], counts


def table_loop(pos, mass, weight, N, m_lm, m_hm, wrap, e):
    """The same with a Python loop over the haloes and Python integers: ({cell: [Q_hm, Q_lm]}, counts)"""
    cells, counts = {}, dict(outside=0, nonfinite=0, below=0)
    for p, m, w in zip(np.asarray(pos, dtype=np.float64), np.asarray(mass, dtype=np.float64), np.asarray(weight, dtype=np.float64)):
        if not all(math.isfinite(v) and abs(v) < 2.0 ** 31 for v in p):
            counts["nonfinite"] += 1
            continue
        c = [math.floor(v) for v in p]
        if wrap:
            c = [v % N for v in c]
        elif not all(0 <= v < N for v in c):
            counts["outside"] += 1
            continue
        kind = 0 if m >= m_hm else (1 if m_lm <= m < m_hm else None)
        if kind is None:
            counts["below"] += 1
            continue
        scaled = math.ldexp(float(w), -e)
        q = round(scaled)                                            # (Python's round of a float is half-even too)
        if q:
            cells.setdefault((c[0] * N + c[1]) * N + c[2], [0, 0])[kind] += q
    counts["n_cells"] = len(cells)
    return cells, counts


def build(cell, q_hm, q_lm, x, g_hm, g_lm, scale, model, x_suppress, f_suppressed):
    """(pos (n_active, 3) int32 0-based, flux, summary [n_active, n_suppressed, sum Q_hm, sum Q_lm not suppressed, sum Q_lm
    suppressed] as Python ints) for the table and the grid `x` (N, N, N)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    N = x.shape[0]
    model = MODELS.get(model, model)
    xs = x.ravel()[cell]
    with np.errstate(invalid="ignore"):
        suppressed = (xs > x_suppress) if model != NONE else np.zeros(cell.size, dtype=bool)
    s = np.where(suppressed, 0.0 if model == FULL else float(f_suppressed), 1.0)
    a = np.float64(g_hm) * q_hm.astype(np.float64)
    b = np.float64(g_lm) * s
    c = b * q_lm.astype(np.float64)
    flux = (a + c) * np.float64(scale)
    active = flux > 0.0
    ij, k = np.divmod(cell[active], N)
    i, j = np.divmod(ij, N)
    pos = np.stack([i, j, k], axis=1).astype(np.int32).reshape(-1, 3)
    total = lambda q, mask: sum(int(v) for v in q[mask])
    everything = np.ones(cell.size, dtype=bool)
    summary = [int(np.sum(active)), int(np.sum(suppressed & (q_lm > 0))), total(q_hm, everything), total(q_lm, ~suppressed),
               total(q_lm, suppressed)]
    return pos, flux[active], summary


def source_list(pos, mass, weight, x, m_lm, m_hm, wrap, e, g_hm, g_lm, scale, model, x_suppress, f_suppressed):
    """table and build in one: (src_pos (3, n) 1-based, src_flux), what C2Ray.evolve3D takes"""
    cell, q_hm, q_lm, _ = table(pos, mass, weight, x.shape[0], m_lm, m_hm, wrap, e)
    p, flux, _ = build(cell, q_hm, q_lm, x, g_hm, g_lm, scale, model, x_suppress, f_suppressed)
    return np.ascontiguousarray(p.T + 1), flux


def clustered(N, n, seed, sigma=1.5):
    """A clustered catalogue: positions drawn in proportion to a log-normal density on the mesh (exp(sigma g), g standard normal
    per cell) and uniform inside the cell; masses from dn/dM ~ M^-2 between 1e8 and 1e13.  (pos (n, 3), mass (n))"""
    rng = np.random.default_rng(seed)
    density = np.exp(sigma * rng.standard_normal(N ** 3))
    index = rng.choice(N ** 3, size=n, p=density / density.sum())
    ij, k = np.divmod(index, N)
    i, j = np.divmod(ij, N)
    pos = np.stack([i, j, k], axis=1) + rng.random((n, 3))
    u = rng.random(n)
    mass = 1.0 / (1.0e-8 - u * (1.0e-8 - 1.0e-13))
    return pos, mass
