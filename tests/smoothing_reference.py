"""TEST INFRASTRUCTURE: a numpy statement of the C-ABI of asora_smooth_field (include/asora_hip.h): W from the
four tables in the library's order, ``np.fft.irfftn(W * np.fft.rfftn(g))``, and the one-point statistics by exact summation.  Nothing
here runs on a device; tests/test_smoothing_reference.py checks it against answers that owe nothing to a transform."""
import numpy as np

import powerspec_reference as PR

(N_FINITE, N_NONFINITE, MIN, MAX, INPUT_SUM, INPUT_SUM2, SUM, S2, S3, S4) = range(10)


def n_radial(N):
    """the length of the radial table: every |m|^2 of the mesh, 0 ... 3 floor(N/2)^2"""
    return 3 * (N // 2) ** 2 + 1


def filter_on_mesh(N, tables, subtract_mean=False):
    """W(n) of the stored half-space, (N, N, N // 2 + 1): ((w_i[n_x] w_j[n_y]) w_k[n_z]) w_r[|m|^2], an absent table all ones; with
    subtract_mean the mode n = 0 is 0 instead"""
    w_i, w_j, w_k, w_r = tables
    one = np.ones(N)
    W = ((one if w_i is None else np.asarray(w_i))[:, None, None] * (one if w_j is None else np.asarray(w_j))[None, :, None]) \
        * (one if w_k is None else np.asarray(w_k))[None, None, :N // 2 + 1]
    if w_r is not None:
        assert len(w_r) == n_radial(N)
        W = W * np.asarray(w_r)[PR.mode_n2(N)]
    W = np.array(np.broadcast_to(W, (N, N, N // 2 + 1)), dtype=np.float64)
    if subtract_mean:
        W[0, 0, 0] = 0.0
    return W


def smooth(g, tables=(None, None, None, None), subtract_mean=False):
    """h = irfftn(W rfftn(g)), (N, N, N)"""
    g = np.asarray(g, dtype=np.float64)
    N = g.shape[0]
    return np.fft.irfftn(filter_on_mesh(N, tables, subtract_mean) * np.fft.rfftn(g), s=(N, N, N), axes=(0, 1, 2))


def histogram(h, edges):
    """uint64 [n + 2]: the finite cells with edges[b] <= h < edges[b + 1], then those below edges[0], then those at or above
    edges[n]"""
    e = np.asarray(edges, dtype=np.float64)
    v = np.asarray(h, dtype=np.float64).ravel()
    v = v[np.isfinite(v)]
    b = np.searchsorted(e, v, side="right") - 1
    inside = (b >= 0) & (b < e.size - 1)
    out = np.zeros(e.size + 1, dtype=np.uint64)
    out[:e.size - 1] = np.bincount(b[inside], minlength=e.size - 1)
    out[e.size - 1] = np.count_nonzero(v < e[0])
    out[e.size] = np.count_nonzero(v >= e[-1])
    return out


def statistics(h, g=None):
    """the ten stats of the ABI for the field h (g: the field before the filter, for [4] and [5]; None: zeros): the terms formed in
    double in the header's order, the sums in extended precision"""
    h = np.asarray(h, dtype=np.float64)
    finite = np.isfinite(h)
    out = np.zeros(10)
    out[N_FINITE], out[N_NONFINITE] = np.count_nonzero(finite), h.size - np.count_nonzero(finite)
    out[MIN] = h[finite].min() if finite.any() else np.inf
    out[MAX] = h[finite].max() if finite.any() else -np.inf
    if g is not None:
        g = np.asarray(g, dtype=np.float64)
        out[INPUT_SUM], out[INPUT_SUM2] = float(PR.exact_sum(g)), float(PR.exact_sum(g * g))
    with np.errstate(invalid="ignore", over="ignore"):
        out[SUM] = float(PR.exact_sum(h))
        mu = out[SUM] / float(h.size)
        d = h - mu
        d2 = d * d
        out[S2], out[S3], out[S4] = float(PR.exact_sum(d2)), float(PR.exact_sum(d2 * d)), float(PR.exact_sum(d2 * d2))
    return out


def moving_average(g, width, axis):
    """the periodic moving average over `width` (odd) cells along `axis`: no transform anywhere"""
    assert width % 2 == 1
    g = np.asarray(g, dtype=np.float64)
    out = np.zeros_like(g)
    for s in range(-(width // 2), width // 2 + 1):
        out += np.roll(g, s, axis=axis)
    return out / width
