"""TEST INFRASTRUCTURE: a numpy/scipy statement of the C-ABI of asora_lyman_alpha_forest (include/asora_hip.h):
the per-line quantities, the weight with its cut at six Doppler widths, the optical depth summed over o = -W ... W ascending, the
window, the PDF and the dark gaps, operation by operation in the header's order.  ``erf`` and ``exp`` are scipy's and numpy's, the
device's are the device library's: the optical depths agree to the bound of :func:`bound`, not bit for bit.  Nothing here runs on a
device; tests/test_lyman_alpha_reference.py checks it against a 40-digit evaluation and known answers."""
import fractions
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


def gap_statistics_fast(flux, gap_threshold):
    """:func:`gap_statistics` without a Python loop over the lines, for meshes of 10^5 lines: every line that is neither wholly dark
    nor wholly bright is rolled to its first bright pixel, so that no run wraps, and the runs of all lines come from one difference
    of the masks: a run starts where it rises and ends where it falls, and in row-major order the q-th rise belongs to the q-th fall."""
    N = flux.shape[-1]
    dark = (flux < gap_threshold).reshape(-1, N)
    full = dark.all(axis=1)
    mixed = dark[dark.any(axis=1) & ~full]
    counts = np.zeros(N + 1, dtype=np.uint64)
    counts[N] = int(full.sum())
    if mixed.shape[0]:
        first_bright = np.argmin(mixed, axis=1).astype(np.int32)
        index = (np.arange(N, dtype=np.int32)[None, :] + first_bright[:, None]) % np.int32(N)
        rolled = np.zeros((mixed.shape[0], N + 2), dtype=np.int8)
        rolled[:, 1:-1] = np.take_along_axis(mixed, index, axis=1)
        edges = np.diff(rolled, axis=1)
        rise, fall = np.nonzero(edges == 1), np.nonzero(edges == -1)
        assert np.array_equal(rise[0], fall[0])
        counts += np.bincount(fall[1] - rise[1], minlength=N + 1).astype(np.uint64)
    lengths = np.nonzero(counts)[0]
    return dict(gaps=counts, n_dark=int(dark.sum()), n_gaps=int(counts.sum()), longest=int(lengths.max()) if lengths.size else 0,
                full_lines=int(full.sum()))


def fsum_of_values(a, values):
    """math.fsum(a) for an array that holds nothing but the few `values`: the exact sum, counts times values in rational arithmetic,
    correctly rounded once (as math.fsum rounds it), without a pass of Python floats over 10^7 cells"""
    a = np.ravel(a)
    counts = [int(np.count_nonzero(a == v)) for v in values]
    assert sum(counts) == a.size and len(set(values)) == len(values)
    return float(sum(fractions.Fraction(float(v)) * c for v, c in zip(values, counts)))


def crafted_lines(N):
    """Dark masks (True: dark) of a line of N pixels in mask words of 64, made for the word arithmetic of a gap walk: wholly dark and
    wholly bright; all dark but one pixel and all bright but one pixel at 0, 63, 64 and N - 1 (one run of N - 1, joined through the wrap
    unless the bright pixel is at an end); the runs [63, 64], [0, 63], [64, 127] and [1, N - 2]; from N = 192 on a run from inside
    word 0 to inside word 2, word 1 wholly dark; a run from N - 3 through the wrap to 2; alternating pixels starting dark and starting
    bright (at odd N the first and last join).  What does not fit a line of N (pixel 64 at N = 64) is left out."""
    lines = [np.ones(N, dtype=bool), np.zeros(N, dtype=bool)]
    places = [p for p in (0, 63, 64, N - 1) if 0 <= p < N]
    places = [p for q, p in enumerate(places) if p not in places[:q]]
    for base in (True, False):
        for p in places:
            line = np.full(N, base)
            line[p] = not base
            lines.append(line)
    for a, b in ((63, 64), (0, 63), (64, 127), (1, N - 2)):
        if 0 <= a <= b < N:
            line = np.zeros(N, dtype=bool)
            line[a:b + 1] = True
            lines.append(line)
    if N >= 192:
        line = np.zeros(N, dtype=bool)
        line[40:151] = True
        lines.append(line)
    if N >= 7:
        line = np.zeros(N, dtype=bool)
        line[[N - 3, N - 2, N - 1, 0, 1, 2]] = True
        lines.append(line)
    lines.append(np.arange(N) % 2 == 0)
    lines.append(np.arange(N) % 2 == 1)
    return lines


def mask_field(N, axis, lines_at, seed=0):
    """(x, n, T, dark): fields whose forest along `axis` has a known answer.  dark (N^2, N) is the designed mask of the lines in the
    order of :func:`pick_lines`: line ``lines_at[q]`` is crafted line q mod their number, every other line is a Bernoulli line with
    p = 0.02, 0.5 or 0.98 in turn.  x = 0 where dark and 1 where bright, n = 1, T = 0, no velocity: with tau_scale = 5 and any b_scale
    every bt is the floor 2^-10 and every cell is one pixel wide, a cell's weight on its own pixel is (erf(512) - erf(-512)) / 2 = 1
    and its neighbours lie outside the cut, so tau = 5 on the dark pixels and exactly 0 on the bright ones, W = 1, clipped = 0,
    degenerate = 0, and F is exp(-5) or exactly 1: gap_threshold = 0.5 gives back the designed mask."""
    rng = np.random.default_rng(1000 * N + 10 * axis + seed)
    p = np.array([0.02, 0.5, 0.98])[np.arange(N * N) % 3]
    dark = rng.random((N * N, N)) < p[:, None]
    crafted = crafted_lines(N)
    for q, at in enumerate(lines_at):
        dark[at] = crafted[q % len(crafted)]
    x = np.ascontiguousarray(np.moveaxis(np.where(dark, 0.0, 1.0).reshape(N, N, N), -1, axis))
    return x, np.ones((N, N, N)), np.zeros((N, N, N)), dark


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
