"""TEST INFRASTRUCTURE: the clumped chemistry restated in numpy.

* ``doric`` / ``do_chemistry``: the reference's doric (src/c2ray/chemistry.f90:221-316) with its clumping argument filled in,
  in its own operation order, brech0 = (C bh00) (T/1e4)^albpow, one cell at a time with libm's functions (``math``), as
  oracle/c2ray_oracle.c evaluates it.
* ``chemistry_pass``: the isolated pass (asora_chemistry_device) vectorised over cells, with the per-cell factor of the
  grid form, brech0 = c (bh00 (T/1e4)^albpow).
* ``chemistry_thermal``: the clumped thermal pass -- tests/thermal_reference.py's scheme with the recombination rate and the
  case-B recombination cooling times c (the kernel: chemistry_cell_thermal<CLUMP>, without FMA contraction)."""
import math

import numpy as np

import thermal_reference as TR

MIN_FRAC_CHANGE, MIN_FRAC_ATOMS, EPS = TR.MIN_FRAC_CHANGE, TR.MIN_FRAC_ATOMS, TR.EPS
_AVG_LIMIT = float(np.float32(1.0e-8))


def doric(xh_old, dt, temp, rhe, phi, bh00, albpow, colh0, temph0, clumping=1.0):
    """(xh, xh_av) of one cell, chemistry.f90:257-306."""
    brech0 = clumping * bh00 * math.pow(temp / 1e4, albpow)
    acolh0 = colh0 * math.sqrt(temp) * math.exp(-temph0 / temp)
    aih0 = phi + rhe * acolh0
    delth = aih0 + rhe * brech0
    eqxh = aih0 / delth
    deltht = delth * dt
    ee = math.exp(-deltht)
    x = (xh_old - eqxh) * ee + eqxh
    x = EPS if x < EPS else x
    avg = 1.0 if deltht < _AVG_LIMIT else (1.0 - ee) / deltht
    xa = eqxh + (xh_old - eqxh) * avg
    xa = EPS if xa < EPS else xa
    return x, xa


def do_chemistry(dt, ndens, temp, xh, xh_av, phi, bh00, albpow, colh0, temph0, abu_c, clumping=1.0):
    """(xh_intermed, xh_av, inner iterations) of one cell, chemistry.f90:146-203 with the clumping factor."""
    nit = 0
    while True:
        nit += 1
        xav_old = xh_av
        de = ndens * (xh_av + abu_c)
        xi, xh_av = doric(xh, dt, temp, de, phi, bh00, albpow, colh0, temph0, clumping)
        if abs((xh_av - xav_old) / (1.0 - xh_av)) < MIN_FRAC_CHANGE or 1.0 - xh_av < MIN_FRAC_ATOMS or nit > 400:
            return xi, xh_av, nit


def chemistry_pass(dt, ndens, temp, xh, xh_av, phi, bh00, albpow, colh0, temph0, abu_c, clump=1.0, return_delta=False):
    """The isolated isothermal pass on N^3 (or flat) grids with the clumping factors `clump` (a scalar or a grid):
    (xh_intermed, xh_av, conv_flag, sum xh_intermed) [+ delth dt of the last inner iteration per cell]."""
    shape = np.shape(ndens)
    n = np.ravel(ndens).astype(np.float64)
    T = np.ravel(temp).astype(np.float64)
    x0 = np.ravel(xh).astype(np.float64)
    g = np.ravel(phi).astype(np.float64)
    c = np.broadcast_to(np.asarray(clump, dtype=np.float64), shape).ravel()
    xav = np.ravel(xh_av).astype(np.float64).copy()
    xav_start, yh_av = xav.copy(), 1.0 - xav
    xint, delta = np.zeros_like(xav), np.zeros_like(xav)
    brech0 = c * (bh00 * (T / 1e4) ** albpow)
    acolh0 = colh0 * np.sqrt(T) * np.exp(-temph0 / T)
    t_ok = np.abs((T - T) / T) < MIN_FRAC_CHANGE
    nit = np.zeros(xav.shape, dtype=np.int64)
    idx = np.arange(xav.size)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        while idx.size:
            nit[idx] += 1
            xav_old = xav[idx]
            de = n[idx] * (xav_old + abu_c)
            aih0 = g[idx] + de * acolh0[idx]
            delth = aih0 + de * brech0[idx]
            eqxh = aih0 / delth
            deltht = delth * dt
            ee = np.exp(-deltht)
            xi = (x0[idx] - eqxh) * ee + eqxh
            xi = np.where(xi < EPS, EPS, xi)
            avg = np.where(deltht < _AVG_LIMIT, 1.0, (1.0 - ee) / deltht)
            xa = eqxh + (x0[idx] - eqxh) * avg
            xa = np.where(xa < EPS, EPS, xa)
            done = ((((np.abs((xa - xav_old) / (1.0 - xa)) < MIN_FRAC_CHANGE) | (1.0 - xa < MIN_FRAC_ATOMS)) & t_ok[idx])
                    | (nit[idx] > 400))
            xav[idx], xint[idx], delta[idx] = xa, xi, deltht
            idx = idx[~done]
        nconv = int(np.count_nonzero((np.abs(xav - xav_start) > MIN_FRAC_CHANGE) &
                                     (np.abs((xav - xav_start) / yh_av) > MIN_FRAC_CHANGE) & (yh_av > MIN_FRAC_ATOMS)))
    out = (xint.reshape(shape), xav.reshape(shape), nconv, float(xint.sum()))
    return out + (delta.reshape(shape),) if return_delta else out


def cooling(p, T, n_e, n_HII, n_HI, colh0, temph0, clump):
    """TR.cooling with the case-B recombination channel times `clump` (last), channel order as in the kernel."""
    L = np.zeros_like(T)
    if p.cooling_mask & 1:
        lam = 2.0 * 157807.0 / T
        L = L + 3.435e-30 * T * lam ** 1.970 / (1.0 + (lam / 2.25) ** 0.376) ** 3.720 * n_e * n_HII * clump
    rest = TR.Params(p.relative_denergy, p.t_floor, p.max_substeps, p.cooling_mask & ~1, p.compton, p.t_cmb)
    if rest.cooling_mask == 0:
        return L
    # (the other channels unchanged; summed in one go they differ from the kernel's running sum by an ulp of L at most)
    return L + TR.cooling(rest, T, n_e, n_HII, n_HI, colh0, temph0)


def thermal(p, dt, abu_c, colh0, temph0, n, x, phi_heat, T_start, clump):
    """TR.thermal with clumped recombination cooling."""
    n = np.asarray(n, dtype=np.float64)
    n_e, n_HII, n_HI = n * (x + abu_c), n * x, n * (1.0 - x)
    cv = 1.5 * TR.K_B * n * (1.0 + x + abu_c)
    H = n_HI * phi_heat
    T = np.array(T_start, dtype=np.float64, copy=True)
    e = cv * T
    t, intT = np.zeros_like(T), np.zeros_like(T)
    k = np.zeros(T.shape, dtype=np.int64)
    floored = np.zeros(T.shape, dtype=bool)
    idx = np.arange(T.size)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        while idx.size:
            Ti, ei, ti = T[idx], e[idx], t[idx]
            k[idx] += 1
            r = H[idx] - cooling(p, Ti, n_e[idx], n_HII[idx], n_HI[idx], colh0, temph0, clump[idx])
            h = dt - ti
            hl = p.relative_denergy * ei / np.abs(r)
            use = (k[idx] < p.max_substeps) & (r != 0.0) & (hl < h)
            h = np.where(use, hl, h)
            Tn = (ei + h * r) / cv[idx]
            fl = Tn < p.t_floor
            Tn = np.where(fl, p.t_floor, Tn)
            floored[idx] |= fl
            e[idx] = cv[idx] * Tn
            intT[idx] = intT[idx] + h * (Ti + Tn) * 0.5
            T[idx] = Tn
            t[idx] = np.where(use, ti + h, ti)
            idx = idx[use]
    return T, intT / dt, k, floored


def chemistry_thermal(p, dt, ndens, temp, xh, xh_av, phi_ion, phi_heat, bh00, albpow, colh0, temph0, abu_c, clump):
    """The isolated thermal pass with the clumping factors `clump` (scalar or grid): (xh_intermed, xh_av, T_end, conv_flag,
    delth dt of the last inner iteration, cells at max_substeps), as TR.chemistry_thermal(..., return_delta=True)."""
    shape = np.shape(temp)
    n_all = np.ravel(ndens).astype(np.float64)
    x0 = np.ravel(xh).astype(np.float64)
    T0 = np.ravel(temp).astype(np.float64)
    g_all = np.ravel(phi_ion).astype(np.float64)
    hr_all = np.ravel(phi_heat).astype(np.float64)
    c_all = np.broadcast_to(np.asarray(clump, dtype=np.float64), shape).ravel()
    xav = np.ravel(xh_av).astype(np.float64).copy()
    xav_start, yh_av = xav.copy(), 1.0 - xav
    T_av, T_end = T0.copy(), T0.copy()
    xint, delta = np.zeros_like(xav), np.zeros_like(xav)
    nit = np.zeros(xav.shape, dtype=np.int64)
    capped = np.zeros(xav.shape, dtype=bool)
    idx = np.arange(xav.size)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        while idx.size:
            nit[idx] += 1
            xav_old, T_prev = xav[idx], T_end[idx]
            n, c = n_all[idx], c_all[idx]
            de = n * (xav_old + abu_c)
            Ta = T_av[idx]
            brech0 = c * (1.0 * bh00 * (Ta / 1e4) ** albpow)
            acolh0 = colh0 * np.sqrt(Ta) * np.exp(-temph0 / Ta)
            aih0 = g_all[idx] + de * acolh0
            delth = aih0 + de * brech0
            eqxh = aih0 / delth
            deltht = delth * dt
            ee = np.exp(-deltht)
            xi = (x0[idx] - eqxh) * ee + eqxh
            xi = np.where(xi < EPS, EPS, xi)
            avg = np.where(deltht < _AVG_LIMIT, 1.0, (1.0 - ee) / deltht)
            xa = eqxh + (x0[idx] - eqxh) * avg
            xa = np.where(xa < EPS, EPS, xa)
            Te, Tav, k, _fl = thermal(p, dt, abu_c, colh0, temph0, n, xa, hr_all[idx], T0[idx], c)
            capped[idx] |= k >= p.max_substeps
            t_ok = np.abs((Te - T_prev) / Te) < MIN_FRAC_CHANGE
            done = (((np.abs((xa - xav_old) / (1.0 - xa)) < MIN_FRAC_CHANGE) | (1.0 - xa < MIN_FRAC_ATOMS)) & t_ok) | (nit[idx] > 400)
            xav[idx], xint[idx], T_end[idx], T_av[idx], delta[idx] = xa, xi, Te, Tav, deltht
            idx = idx[~done]
        nconv = int(np.count_nonzero((np.abs(xav - xav_start) > MIN_FRAC_CHANGE) &
                                     (np.abs((xav - xav_start) / yh_av) > MIN_FRAC_CHANGE) & (yh_av > MIN_FRAC_ATOMS)))
    return (xint.reshape(shape), xav.reshape(shape), T_end.reshape(shape), nconv, delta.reshape(shape),
            capped.reshape(shape))
