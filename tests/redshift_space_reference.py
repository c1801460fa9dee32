"""TEST INFRASTRUCTURE: a numpy statement of the C-ABI of asora_redshift_space_field and asora_power_spectrum_los (include/asora_hip.h;
DESIGN.md section 4.2j), written from the specification there and not from the kernels: the mapping loops over the offsets of the
SOURCE cells and scatters each cell's share onto the cell it lands on (the kernel gathers), the sums bin ``np.fft.rfftn`` output mode
by mode.  Nothing here runs on a device; tests/test_redshift_space_reference.py checks it against known answers."""
import numpy as np

import powerspec_reference as PR

CYLINDRICAL, MU = range(2)
MAX_BINS = 1024
DEGENERATE = 2.0 ** -10


def library_window(max_abs_v, velocity_scale):
    """W as the library takes it: floor(max|v| |velocity_scale|) + 1"""
    return int(np.floor(float(max_abs_v) * abs(float(velocity_scale)))) + 1


def map_lines(g, v, velocity_scale, los_axis, W=None):
    """h of the header: every line along `los_axis` of g regridded between its displaced cell edges.  Every step is one IEEE double
    operation on whole arrays (numpy contracts nothing); for each output cell the terms arrive in ascending o."""
    g = np.moveaxis(np.asarray(g, dtype=np.float64), los_axis, -1)
    v = np.moveaxis(np.asarray(v, dtype=np.float64), los_axis, -1)
    N = g.shape[-1]
    if W is None:
        W = library_window(np.max(np.abs(v)), velocity_scale)
    assert 2 * W + 1 <= N, "the window would wrap onto itself"
    u = v * float(velocity_scale)
    d = 0.5 * (np.roll(u, 1, axis=-1) + u)                      # d[q] = 0.5 (u[q - 1] + u[q])
    a, b = d, 1.0 + np.roll(d, -1, axis=-1)                     # b[q] = 1 + d[q + 1]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    width = hi - lo
    degenerate = width < DEGENERATE
    centre = np.floor(0.5 * (lo + hi))
    safe = np.where(degenerate, 1.0, width)
    h = np.zeros(g.shape)                                       # +0.0
    for o in range(-W, W + 1):
        od = float(o)
        ov = np.minimum(hi, od + 1.0) - np.maximum(lo, od)
        w = np.where(degenerate, np.where(centre == od, 1.0, 0.0), np.where(ov > 0.0, ov / safe, 0.0))
        h = h + np.roll(w * g, o, axis=-1)                      # cell q lands on p = q + o
    return np.ascontiguousarray(np.moveaxis(h, -1, los_axis))


def count_inverted(v, velocity_scale, los_axis):
    """how many cells have b < a (a shell crossing)"""
    u = np.moveaxis(np.asarray(v, dtype=np.float64), los_axis, -1) * float(velocity_scale)
    d = 0.5 * (np.roll(u, 1, axis=-1) + u)
    return int(np.sum(1.0 + np.roll(d, -1, axis=-1) < d))


def mode_parts(N, los_axis):
    """(m_par, n2) of the stored modes, (N, N, N // 2 + 1) int64 each"""
    m = PR.folded(N).astype(np.int64)
    parts = [m[:, None, None], m[None, :, None], np.arange(N // 2 + 1, dtype=np.int64)[None, None, :]]
    shape = (N, N, N // 2 + 1)
    return np.broadcast_to(parts[los_axis], shape), PR.mode_n2(N)


def bin_indices(N, los_axis, mode, thr_a, thr_b):
    """(ia, ib) of every stored mode; -1 or n: outside"""
    thr_a = np.asarray(thr_a, dtype=np.int64)
    thr_b = np.asarray(thr_b, dtype=np.float64)
    assert np.all(np.diff(thr_a) >= 0) and np.all(np.isfinite(thr_b)) and np.all(np.diff(thr_b) >= 0)
    mpar, n2 = mode_parts(N, los_axis)
    mp2 = (mpar * mpar).astype(np.float64)
    if mode == CYLINDRICAL:
        ia = np.searchsorted(thr_a, n2 - mpar * mpar, side="right") - 1
        ib = np.searchsorted(thr_b, mp2, side="right") - 1
    else:
        assert thr_a[0] >= 1
        ia = np.searchsorted(thr_a, n2, side="right") - 1
        n2d = n2.astype(np.float64)
        ib = np.full(n2.shape, -1, dtype=np.int64)
        for e in thr_b:                                        # thr_b[b] n2 <= m_par^2: each product one rounding
            ib += (e * n2d <= mp2)
    return ia, ib


def _sum_per_bin(idx, terms, nb):
    """terms (longdouble) summed per bin in extended precision"""
    order = np.argsort(idx, kind="stable")
    idx, terms = idx[order], terms[order]
    out = np.zeros(nb, dtype=np.longdouble)
    if idx.size:
        starts = np.flatnonzero(np.r_[True, idx[1:] != idx[:-1]])
        out[idx[starts]] = np.add.reduceat(terms, starts)
    return out.astype(np.float64)


def binned(N, los_axis, mode, thr_a, thr_b, hhat):
    """dict of count (uint64), sum_1, sum_2, sum_aa, sum_l2, sum_l4, each (n_a, n_b), and total_aa: the weighted power of every mode
    but n = 0"""
    n_a, n_b = len(thr_a) - 1, len(thr_b) - 1
    assert n_a >= 1 and n_b >= 1 and n_a * n_b <= MAX_BINS
    ia, ib = bin_indices(N, los_axis, mode, thr_a, thr_b)
    mpar, n2 = mode_parts(N, los_axis)
    w = np.broadcast_to(PR.mode_weights(N)[None, None, :], n2.shape)
    keep = (n2 > 0) & (ia >= 0) & (ia < n_a) & (ib >= 0) & (ib < n_b)
    idx = (ia * n_b + ib)[keep]
    wk = w[keep].astype(np.float64)
    n2k, mk = n2[keep], mpar[keep]
    ld = np.longdouble
    if mode == CYLINDRICAL:
        s1 = wk.astype(ld) * np.sqrt((n2k - mk * mk).astype(ld))
        s2 = wk.astype(ld) * mk.astype(ld)
    else:
        s1 = wk.astype(ld) * np.sqrt(n2k.astype(ld))
        s2 = wk.astype(ld) * np.sqrt((mk * mk).astype(ld) / n2k.astype(ld))
    t = (mk * mk).astype(np.float64) / n2k.astype(np.float64)
    L2 = 0.5 * (3.0 * t - 1.0)
    L4 = 0.125 * ((35.0 * t - 30.0) * t + 3.0)
    power = wk * np.abs(hhat[keep]) ** 2
    nb = n_a * n_b
    shape = (n_a, n_b)
    not0 = n2 > 0
    return dict(count=np.bincount(idx, weights=wk, minlength=nb).astype(np.uint64).reshape(shape),
                sum_1=_sum_per_bin(idx, s1, nb).reshape(shape), sum_2=_sum_per_bin(idx, s2, nb).reshape(shape),
                sum_aa=np.bincount(idx, weights=power, minlength=nb).reshape(shape),
                sum_l2=np.bincount(idx, weights=power * L2, minlength=nb).reshape(shape),
                sum_l4=np.bincount(idx, weights=power * L4, minlength=nb).reshape(shape),
                total_aa=float(np.sum(w[not0] * np.abs(hhat[not0]) ** 2)))


def kaiser_field(N, seed, rms=0.02, continuum=False):
    """A white Gaussian density contrast of rms `rms` and its linear-theory displacement (f = 1) along each axis in cells.  Linear theory is the continuity equation, div u = -delta, with u a gradient; to first order in u the mapping turns
    it into delta_s = delta - C u, C the CENTRED difference (u[q + 1] - u[q - 1]) / 2 that the edge displacements d of the
    specification amount to.  The velocities here satisfy the continuity equation with that operator, the one the mesh has:
    u_a(k) = i k_a^2 / (k^2 sin k_a) delta(k), so that C_a u_a = -(k_a^2 / k^2) delta mode by mode and the redshift-space field is
    (1 + mu^2) delta up to terms of second order.  `continuum`: u_a(k) = i k_a / k^2 delta(k) instead, the derivative of the
    continuum sampled at the cell centres, on which the centred difference loses sin(k_a) / k_a (the figure is printed by the
    test; it is no property of the implementation).  Returns (delta, [u_0, u_1, u_2])."""
    rng = np.random.default_rng(seed)
    white = np.fft.rfftn(rng.normal(size=(N, N, N)))
    k1 = 2.0 * np.pi * np.fft.fftfreq(N)
    kz = 2.0 * np.pi * np.fft.rfftfreq(N)
    kk = [k1[:, None, None], k1[None, :, None], kz[None, None, :]]
    k2 = kk[0] ** 2 + kk[1] ** 2 + kk[2] ** 2
    k2[0, 0, 0] = 1.0
    dk = white.copy()        # (white: a redder field's bulk flows carry the small scales about, second order but not small)
    dk[0, 0, 0] = 0.0
    if N % 2 == 0:                                             # the Nyquist planes carry no velocity of definite sign: drop them
        dk[N // 2, :, :] = 0.0
        dk[:, N // 2, :] = 0.0
        dk[:, :, N // 2] = 0.0
    delta = np.fft.irfftn(dk, s=(N, N, N), axes=(0, 1, 2))
    scale = rms / delta.std()
    delta, dk = delta * scale, dk * scale
    u = []
    for a in range(3):
        s = np.sin(kk[a])
        window = np.ones_like(s) if continuum else np.where(np.abs(s) > 1e-12, kk[a] / np.where(np.abs(s) > 1e-12, s, 1.0), 0.0)
        u.append(np.fft.irfftn(1j * kk[a] * window / k2 * dk, s=(N, N, N), axes=(0, 1, 2)))
    return delta, u


def kaiser_deviation(N, los_axis, delta, h):
    """the median over the modes with 0 < |n| < N / 4 of | |hhat|^2 / ((1 + mu^2)^2 |deltahat|^2) - 1 |"""
    mpar, n2 = mode_parts(N, los_axis)
    dhat, hhat = np.fft.rfftn(delta), np.fft.rfftn(h)
    pick = (n2 > 0) & (n2 < (N / 4.0) ** 2)
    mu2 = (mpar[pick] ** 2) / n2[pick].astype(np.float64)
    ratio = np.abs(hhat[pick]) ** 2 / ((1.0 + mu2) ** 2 * np.abs(dhat[pick]) ** 2)
    return float(np.median(np.abs(ratio - 1.0)))
