"""TEST INFRASTRUCTURE: a numpy/scipy statement of the C-ABI of asora_lyman_alpha_forest (include/asora_hip.h):
the per-line quantities, the weight with its cut at six Doppler widths, the optical depth summed over o = -W ... W ascending, the
window, the PDF and the dark gaps, operation by operation in the header's order.  ``erf`` and ``exp`` are scipy's and numpy's, the
device's are the device library's: the optical depths agree to the bound of :func:`bound`, not bit for bit.  Nothing here runs on a
device; tests/test_lyman_alpha_reference.py checks it against a 40-digit evaluation and known answers."""
import math

import numpy as np
from scipy.special import erf

FLOOR = 2.0 ** -10
INV_SQRT_PI = 0.5641895835477563
EPS = 2.0 ** -52
MAX_BINS = 1024
FLUX, TAU = 0, 1


def line_quantities(x, n, T, v, velocity_scale, b_scale, tau_scale):
    """lo, hi, bt, g of every cell; the arrays hold lines along their LAST axis.  v = None: u = 0."""
    u = np.zeros_like(x, dtype=np.float64) if v is None else v * velocity_scale
    d = 0.5 * (np.roll(u, 1, axis=-1) + u)
    a, b = d, 1.0 + np.roll(d, -1, axis=-1)
    lo, hi = np.where(b < a, b, a), np.where(b < a, a, b)
    with np.errstate(invalid="ignore"):
        bt = b_scale * np.sqrt(T)
        bt = np.where(bt > FLOOR, bt, FLOOR)
    g = tau_scale * ((1.0 - x) * n)
    return lo, hi, bt, g


def reach_of(lo, hi, bt):
    r1, r2 = (6.0 * bt - lo) + 0.5, (hi + 6.0 * bt) - 0.5
    return np.where(r2 > r1, r2, r1)


def window_of(reach_max, N, window=0):
    """W: `window` itself, or the automatic one from the largest reach."""
    if window > 0:
        return int(window)
    cap = (N - 1) // 2
    need = math.ceil(reach_max) if math.isfinite(reach_max) else math.inf
    return cap if not need <= cap else min(max(1, int(need)), cap)


def weight(lo, hi, bt, o):
    """(w of every cell on the pixel o cells behind it, is the term left out) -- left out: outside the cut"""
    s = float(o) + 0.5
    width = hi - lo
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        cut = ((s - hi) > 6.0 * bt) | ((lo - s) > 6.0 * bt)
        wide = 0.5 * (erf((s - lo) / bt) - erf((s - hi) / bt)) / width
        t = (s - 0.5 * (lo + hi)) / bt
        cut_d = np.abs(t) > 6.0
        narrow = (INV_SQRT_PI / bt) * np.exp(-(t * t))
    is_wide = width >= FLOOR
    return np.where(is_wide, wide, narrow), np.where(is_wide, cut, cut_d)


def optical_depth(lo, hi, bt, g, W):
    """tau of every pixel, lines along the last axis: the sum over o ascending, from +0.0; a term outside the cut or with g == 0
    is left out"""
    tau = np.zeros_like(g)
    for o in range(-W, W + 1):
        w, out = weight(lo, hi, bt, o)
        with np.errstate(invalid="ignore", over="ignore"):
            term = np.where(out | (g == 0.0), 0.0, w * g)
        tau = tau + np.roll(term, o, axis=-1)          # (pixel p takes cell q = p - o)
    return tau


def bound(lo, hi, bt, g, W):
    """(2 W + 16) eps S[p], S[p] = the sum over the window of |g[q]| m[q], m = 1 / width or 0.5641895835477563 / bt: at most one rounding
    per addition of 2 W + 1 terms of magnitude <= g m, plus a few ulp per erf and per division"""
    width = hi - lo
    with np.errstate(divide="ignore"):
        m = np.where(width >= FLOOR, 1.0 / np.where(width >= FLOOR, width, 1.0), INV_SQRT_PI / bt)
    gm = np.abs(g) * m
    S = np.zeros_like(g)
    for o in range(-W, W + 1):
        S = S + np.roll(gm, o, axis=-1)
    return (2 * W + 16) * EPS * S


def gaps_of_line(dark):
    """The lengths of the maximal runs of True on a periodic line (a wholly dark line: one run of its length)."""
    dark = np.asarray(dark, dtype=bool)
    N = dark.size
    if dark.all():
        return [N]
    if not dark.any():
        return []
    first_bright = int(np.argmin(dark))
    rolled = np.roll(dark, -first_bright)              # starts bright: no run wraps
    edges = np.diff(np.r_[0, rolled.astype(np.int8), 0])
    return (np.nonzero(edges == -1)[0] - np.nonzero(edges == 1)[0]).tolist()


def gap_statistics(flux, gap_threshold):
    """dict of gaps [N + 1], n_dark, n_gaps, longest, full_lines for lines along the last axis of `flux`"""
    N = flux.shape[-1]
    dark = (flux < gap_threshold).reshape(-1, N)
    counts = np.zeros(N + 1, dtype=np.uint64)
    full = 0
    for line in dark:
        for length in gaps_of_line(line):
            counts[length] += 1
        full += bool(line.all())
    lengths = np.nonzero(counts)[0]
    return dict(gaps=counts, n_dark=int(dark.sum()), n_gaps=int(counts.sum()), longest=int(lengths.max()) if lengths.size else 0,
                full_lines=full)


def pdf_of(flux, edges):
    """uint64 [n_bins]: edges[i] <= F < edges[i + 1]; a cell outside every bin (a NaN too) is dropped"""
    edges = np.asarray(edges, dtype=np.float64)
    idx = np.searchsorted(edges, np.ravel(flux), side="right") - 1
    idx = idx[(idx >= 0) & (idx < edges.size - 1)]
    return np.bincount(idx, minlength=edges.size - 1).astype(np.uint64)


def pick_lines(a, los_axis, lines):
    """(len(lines), N): the lines along `los_axis` of the (N, N, N) array `a` with the flat indices `lines` (C order of the two other
    axes)"""
    r, c = np.divmod(np.asarray(lines), a.shape[0])
    index = [r, c]
    index.insert(los_axis, slice(None))
    out = a[tuple(index)]
    return out.T if los_axis == 0 else out


def forest(x, n, T, v, los_axis, velocity_scale, b_scale, tau_scale, window=0, gap_threshold=0.05, edges=None, lines=None):
    """The call on (N, N, N) arrays in C order: a dict of tau, flux (N, N, N), bound (of tau), window, reach_max, clipped, degenerate,
    nonfinite, sum_f, sum_f2, tau_min, tau_max, pdf (with edges) and the entries of :func:`gap_statistics`.  `lines`: indices into
    the N^2 lines (:func:`pick_lines`) to evaluate alone -- tau, flux and bound are then (len(lines), N), window, reach_max, clipped
    and degenerate those of the chosen lines, and no other statistic is returned."""
    N = x.shape[0]
    if lines is not None:
        to_lines = lambda a: None if a is None else pick_lines(np.asarray(a, dtype=np.float64), los_axis, lines)
    else:
        to_lines = lambda a: None if a is None else np.moveaxis(np.asarray(a, dtype=np.float64), los_axis, -1)
    lo, hi, bt, g = line_quantities(to_lines(x), to_lines(n), to_lines(T), to_lines(v), velocity_scale, b_scale, tau_scale)
    reach = reach_of(lo, hi, bt)
    reach_max = float(np.max(reach))
    W = window_of(reach_max, N, window)
    out = dict(window=W, reach_max=reach_max, clipped=int(np.sum(np.ceil(reach) > W)), degenerate=int(np.sum(hi - lo < FLOOR)))
    tau = optical_depth(lo, hi, bt, g, W)
    flux = np.exp(-tau)
    if lines is not None:
        out.update(tau=tau, flux=flux, bound=bound(lo, hi, bt, g, W))
        return out
    out.update(gap_statistics(flux, gap_threshold))
    back = lambda a: np.ascontiguousarray(np.moveaxis(a, -1, los_axis))
    out.update(tau=back(tau), flux=back(flux), bound=back(bound(lo, hi, bt, g, W)), nonfinite=int(np.sum(~np.isfinite(tau))),
               sum_f=math.fsum(flux.ravel()), sum_f2=math.fsum((flux * flux).ravel()), tau_min=float(np.nanmin(tau)),
               tau_max=float(np.nanmax(tau)), pdf=None if edges is None else pdf_of(flux, edges))
    return out


def fields(N, seed, degenerate=True):
    """The fields of the device tests, (x, n, T, v) with velocity_scale = 0.5 in mind: a log-normal density; x between exact 0 and exact
    1 with neutral islands, so that tau spans about 1e-2 ... 1e2; T from 1 K to 3e4 K with exact zeros (the floor of bt); a dyadic
    velocity (multiples of 1/4, |u| <= 3 cells) with inverted cells and, with `degenerate`, cells of width exactly 0 on every axis."""
    rng = np.random.default_rng(seed)
    i, j, k = np.meshgrid(*[np.arange(N, dtype=np.float64)] * 3, indexing="ij")
    wave = 0.5 + 0.5 * np.sin(2 * np.pi * (2 * i + 0.3) / N) * np.sin(2 * np.pi * (j + 0.7) / N) * np.sin(2 * np.pi * (3 * k + 0.1) / N)
    neutral = 10.0 ** (-3.0 + 3.3 * np.clip(wave + 0.25 * rng.standard_normal((N, N, N)), 0.0, 1.0))
    x = 1.0 - np.minimum(neutral, 1.0)
    x[rng.random((N, N, N)) < 0.02] = 1.0
    x[rng.random((N, N, N)) < 0.02] = 0.0
    n = 3.0 * np.exp(rng.standard_normal((N, N, N)))
    T = 10.0 ** rng.uniform(0.0, math.log10(3.0e4), (N, N, N))
    T[rng.random((N, N, N)) < 0.02] = 0.0
    v = np.round(rng.uniform(-6.0, 6.0, (N, N, N)) * 4.0) / 4.0       # u = v / 2: multiples of 1/8 up to 3 cells
    if degenerate:                                                     # d[q + 1] - d[q] = -1: u[q + 1] = u[q - 1] - 2
        for axis in range(3):
            idx = [slice(None)] * 3
            at = lambda q: tuple(idx[:axis] + [q % N] + idx[axis + 1:])
            sel = rng.random((N, N)) < 0.2
            for q in (5, 11):
                line_m, line_p = v[at(q - 1)], v[at(q + 1)]
                here = sel & (line_m >= -2.0)                          # (|u| stays <= 3)
                line_p[here] = line_m[here] - 4.0
    return x, n, T, v
