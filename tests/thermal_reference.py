"""TEST INFRASTRUCTURE: the thermal form of the chemistry pass (pyc2ray_amd/csrc/chemistry.hip: thermal_cooling,
thermal_integrate, chemistry_cell_thermal) restated in numpy, vectorised over cells, in the kernel's operation order
(the kernel evaluates these functions without FMA contraction)."""
import numpy as np

K_B = 1.381e-16
# Compton coupling 4 sigma_T a_rad k_B / (m_e c) from CODATA 2018 (cgs)
_SIGMA_T, _SIGMA_SB, _C, _KB, _ME = 6.6524587321e-25, 5.670374419e-5, 2.99792458e10, 1.380649e-16, 9.1093837015e-28
_A_RAD = 4.0 * _SIGMA_SB / _C
COMPTON_C = 4.0 * _SIGMA_T * _A_RAD * _KB / (_ME * _C)

MIN_FRAC_CHANGE = float(np.float32(1.0e-3))
MIN_FRAC_ATOMS = float(np.float32(1.0e-8))
EPS = 1e-14


class Params:
    """The constants of asora_thermal_params."""

    def __init__(self, relative_denergy=0.1, t_floor=1.0, max_substeps=10000, cooling_mask=31, compton=False, t_cmb=0.0):
        self.relative_denergy, self.t_floor, self.max_substeps = relative_denergy, t_floor, max_substeps
        self.cooling_mask, self.compton, self.t_cmb = cooling_mask, compton, t_cmb


def cooling(p, T, n_e, n_HII, n_HI, colh0, temph0):
    """Lambda(T) in erg s^-1 cm^-3."""
    L = np.zeros_like(T)
    if p.cooling_mask & 1:
        lam = 2.0 * 157807.0 / T
        L = L + 3.435e-30 * T * lam ** 1.970 / (1.0 + (lam / 2.25) ** 0.376) ** 3.720 * n_e * n_HII
    if p.cooling_mask & 2:
        L = L + K_B * temph0 * colh0 * np.sqrt(T) * np.exp(-temph0 / T) * n_e * n_HI
    if p.cooling_mask & 4:
        L = L + 7.5e-19 * np.exp(-118348.0 / T) / (1.0 + np.sqrt(T / 1e5)) * n_e * n_HI
    if p.cooling_mask & 8:
        u = 5.5 - np.log10(T)
        gff = 1.1 + 0.34 * np.exp(-(u * u) / 3.0)
        L = L + 1.42e-27 * gff * np.sqrt(T) * n_e * n_HII
    if (p.cooling_mask & 16) and p.compton:
        tg = p.t_cmb
        L = L + COMPTON_C * ((tg * tg) * (tg * tg)) * (T - tg) * n_e
    return L


def thermal(p, dt, abu_c, colh0, temph0, n, x, phi_heat, T_start):
    """thermal(T_start, x, phi_heat) -> (T_end, T_av, substeps, floored) per cell."""
    n = np.asarray(n, dtype=np.float64)
    n_e = n * (x + abu_c)
    n_HII = n * x
    n_HI = n * (1.0 - x)
    n_p = n * (1.0 + x + abu_c)
    cv = 1.5 * K_B * n_p
    H = n_HI * phi_heat
    T = np.array(T_start, dtype=np.float64, copy=True)
    e = cv * T
    t = np.zeros_like(T)
    intT = np.zeros_like(T)
    k = np.zeros(T.shape, dtype=np.int64)
    floored = np.zeros(T.shape, dtype=bool)
    idx = np.arange(T.size)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        while idx.size:
            Ti, ei, ti = T[idx], e[idx], t[idx]
            k[idx] += 1
            r = H[idx] - cooling(p, Ti, n_e[idx], n_HII[idx], n_HI[idx], colh0, temph0)
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


def chemistry_thermal(p, dt, ndens, temp, xh, xh_av, phi_ion, phi_heat, bh00, albpow, colh0, temph0, abu_c, return_delta=False):
    """The isolated thermal pass (asora_chemistry_device in thermal mode) on flat or N^3 grids.
    Returns (xh_intermed, xh_av, T_end, conv_flag, (cells at max_substeps, cells floored, most substeps)) [+ doric's
    delth * dt of the last inner iteration per cell and the cells that hit max_substeps, with return_delta]."""
    shape = np.shape(temp)
    n_all = np.ravel(ndens).astype(np.float64)
    x0 = np.ravel(xh).astype(np.float64)
    T0 = np.ravel(temp).astype(np.float64)
    g_all = np.ravel(phi_ion).astype(np.float64)
    hr_all = np.ravel(phi_heat).astype(np.float64)
    xav = np.ravel(xh_av).astype(np.float64).copy()
    xav_start = xav.copy()
    yh_av = 1.0 - xav
    T_av = T0.copy()
    T_end = T0.copy()
    xint = np.zeros_like(xav)
    delta = np.zeros_like(xav)
    nit = np.zeros(xav.shape, dtype=np.int64)
    capped = np.zeros(xav.shape, dtype=bool)
    floored = np.zeros(xav.shape, dtype=bool)
    most = 0
    idx = np.arange(xav.size)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        while idx.size:
            nit[idx] += 1
            xav_old, T_prev = xav[idx], T_end[idx]
            n = n_all[idx]
            de = n * (xav_old + abu_c)
            Ta = T_av[idx]
            brech0 = 1.0 * bh00 * (Ta / 1e4) ** albpow
            acolh0 = colh0 * np.sqrt(Ta) * np.exp(-temph0 / Ta)
            aih0 = g_all[idx] + de * acolh0
            delth = aih0 + de * brech0
            eqxh = aih0 / delth
            deltht = delth * dt
            ee = np.exp(-deltht)
            xi = (x0[idx] - eqxh) * ee + eqxh
            xi = np.where(xi < EPS, EPS, xi)
            avg = np.where(deltht < float(np.float32(1.0e-8)), 1.0, (1.0 - ee) / deltht)
            xa = eqxh + (x0[idx] - eqxh) * avg
            xa = np.where(xa < EPS, EPS, xa)
            Te, Tav, k, fl = thermal(p, dt, abu_c, colh0, temph0, n, xa, hr_all[idx], T0[idx])
            capped[idx] |= k >= p.max_substeps
            floored[idx] |= fl
            most = max(most, int(k.max()))
            t_ok = np.abs((Te - T_prev) / Te) < MIN_FRAC_CHANGE
            done = (((np.abs((xa - xav_old) / (1.0 - xa)) < MIN_FRAC_CHANGE) | (1.0 - xa < MIN_FRAC_ATOMS)) & t_ok) | (nit[idx] > 400)
            xav[idx], xint[idx], T_end[idx], T_av[idx], delta[idx] = xa, xi, Te, Tav, deltht
            idx = idx[~done]
        nconv = int(np.count_nonzero((np.abs(xav - xav_start) > MIN_FRAC_CHANGE) &
                                     (np.abs((xav - xav_start) / yh_av) > MIN_FRAC_CHANGE) & (yh_av > MIN_FRAC_ATOMS)))
    stats = (int(capped.sum()), int(floored.sum()), most)
    out = (xint.reshape(shape), xav.reshape(shape), T_end.reshape(shape), nconv, stats)
    return out + (delta.reshape(shape), capped.reshape(shape)) if return_delta else out
