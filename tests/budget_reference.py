"""TEST INFRASTRUCTURE: the twelve sums of the step budget (include/asora_hip.h, asora_step_budget)
restated in numpy, each summed exactly (``math.fsum``), together with the sum of the terms' magnitudes per slot -- the scale a
floating-point sum's error is measured against."""
import math

import numpy as np

SLOTS = ("CELLS", "N", "X", "NX", "NX0", "DNX", "PHOTO", "LLS", "REC", "COL", "T", "NT")
CELLS, N_, X, NX, NX0, DNX, PHOTO, LLS, REC, COL, T_, NT = range(12)
EPS = 1e-14              # doric's floor of the ionised fraction (chemistry.f90:8)
MIN_FRAC_CHANGE = float(np.float32(1.0e-3))


def terms(n, x0, x1, xav, gamma, temp, chem, clump=1.0, lls=(0.0, 0.0), temp_end=None):
    """The twelve per-cell terms, a (12, cells) array; chem = (bh00, albpow, colh0, temph0, abu_c), `clump` a scalar or a grid,
    lls = (n_const, per_density), temp_end: T = (temp + temp_end) / 2."""
    bh00, albpow, colh0, temph0, abu_c = chem
    f = lambda a: np.ravel(np.asarray(a, dtype=np.float64))
    n, x0, x1, xav, g, T = f(n), f(x0), f(x1), f(xav), f(gamma), f(temp)
    if temp_end is not None:
        T = 0.5 * (T + f(temp_end))
    c = np.broadcast_to(np.asarray(clump, dtype=np.float64), np.shape(temp)).ravel() if np.ndim(clump) else np.full(n.shape, float(clump))
    a, b = lls
    ne, nHI = n * (xav + abu_c), n * (1.0 - xav)
    return np.stack([np.ones_like(n), n, x1, n * x1, n * x0, n * (x1 - x0), g * nHI, g * (n * b + a),
                     c * (bh00 * (T / 1e4) ** albpow) * ne * (n * xav), colh0 * np.sqrt(T) * np.exp(-temph0 / T) * ne * nHI, T, n * T])


def sums(n, x0, x1, xav, gamma, temp, chem, clump=1.0, lls=(0.0, 0.0), temp_end=None, planes=None, keep=None):
    """(sums[12], sum of |term| [12]) over the planes (i_begin, i_count) of the (N, N, N) C-ordered grids (None: all);
    `keep`: a boolean (N, N, N) mask of the cells that count (None: all)."""
    return sums_of_terms(terms(n, x0, x1, xav, gamma, temp, chem, clump, lls, temp_end), np.shape(n)[0], planes, keep)


def sums_of_terms(t, N, planes=None, keep=None):
    """:func:`sums` of the (12, N^3) array :func:`terms` returned (several plane ranges of one set of grids)."""
    sel = np.ones(t.shape[1], dtype=bool) if keep is None else np.ravel(keep).copy()
    if planes is not None:
        a, cnt = planes
        inside = np.zeros(t.shape[1], dtype=bool)
        inside[a * N * N:(a + cnt) * N * N] = True
        sel &= inside
    t = t[:, sel]
    return (np.array([math.fsum(row) for row in t]), np.array([math.fsum(np.abs(row)) for row in t]))


def residual_bound(n, xav, temp, dt, chem, clump=1.0, keep=None):
    """1e-3 dt sum n nHI (brech0 xav + acolh0 (1 - xav)): what the inner iteration's exit test leaves of the identity
    x1 - x0 = dt [(Gamma + de acolh0)(1 - xav) - de brech0 xav] when `de` is evaluated at the final xav (per unit volume)."""
    bh00, albpow, colh0, temph0, _ = chem
    f = lambda a: np.ravel(np.asarray(a, dtype=np.float64))
    n, xav, T = f(n), f(xav), f(temp)
    c = np.broadcast_to(np.asarray(clump, dtype=np.float64), np.shape(temp)).ravel() if np.ndim(clump) else float(clump)
    brech0 = c * (bh00 * (T / 1e4) ** albpow)
    acolh0 = colh0 * np.sqrt(T) * np.exp(-temph0 / T)
    t = n * (n * (1.0 - xav)) * (brech0 * xav + acolh0 * (1.0 - xav))
    if keep is not None:
        t = t[np.ravel(keep)]
    return MIN_FRAC_CHANGE * dt * math.fsum(t)


def residual(s, dt):
    """DNX - dt (PHOTO + COL - REC) of a sums vector (per unit volume)."""
    return s[DNX] - dt * (s[PHOTO] + s[COL] - s[REC])
