"""TEST INFRASTRUCTURE: Lyman-limit-system opacity on the CPU, without a change to the oracle.

The raytrace reads the medium only as an absorber density.  So for a given xh_av the oracle's raytrace is called with
``ndens := n_abs(ndens, xh_av, a, b)`` and ``xh_av := 0`` -- its nHI = n_abs * (1 - 0) is n_abs bit for bit -- and the chemistry
with the real ``ndens``.  ``evolve3D_lls_oracle`` is the loop of tests/evolve_oracle.py with that substitution,
``evolve3D_lls_thermal_oracle`` its thermal twin, ``evolve3d_lls_cpu_path`` the use_gpu=False loop on the sub-box oracle."""
import numpy as np

from oracle import oracle as O


def n_abs(ndens, xh_av, a, b):
    """ndens ((1 - xh_av) + b) + a in IEEE double, every operation rounded on its own: the bits of the device helper
    (rates_device.hpp: absorber_density)."""
    n = np.asarray(ndens, dtype=np.float64)
    x = np.asarray(xh_av, dtype=np.float64)
    return n * ((1.0 - x) + np.float64(b)) + np.float64(a)


def raytrace(R, sig, dr, ndens, xh_av, pos0, flux, thin, thick, minlogtau, dlogtau, a, b, **kw):
    """O.asora_do_all_sources of the medium with LLS opacity (a, b)."""
    return O.asora_do_all_sources(R, sig, dr, n_abs(ndens, xh_av, a, b), np.zeros(np.shape(ndens)), pos0, flux, thin, thick,
                                  minlogtau, dlogtau, **kw)


def _loop(trace, chemistry, xh, NumSrc, convergence_fraction, max_iter):
    NumCells = xh.size
    conv_criterion = min(int(convergence_fraction * NumCells), (NumSrc - 1) / 3)
    prev1 = prev0 = 2 * NumCells
    xh_av = np.array(xh, dtype=np.float64, order="C", copy=True)
    state, niter, converged, history = None, 0, False, []
    while not converged and niter < max_iter:
        niter += 1
        rates = trace(xh_av)
        xh_av, xh_intermed, conv_flag, state = chemistry(xh_av, rates, state)
        s1, s0 = np.sum(xh_intermed), np.sum(1.0 - xh_intermed)
        rel1 = abs((s1 - prev1) / s1) if s1 > 0 else 1.0
        rel0 = abs((s0 - prev0) / s0) if s0 > 0 else 1.0
        history.append((conv_flag, rel1, rel0))
        converged = (conv_flag < conv_criterion) or (rel1 < convergence_fraction and rel0 < convergence_fraction)
        prev1, prev0 = s1, s0
    return xh_intermed, rates, niter, history, state


def evolve3D_lls_oracle(a, b, dt, dr, src_flux, src_pos, temp, ndens, xh, thin, thick, minlogtau, dlogtau, R_max_LLS,
                        convergence_fraction, sig, bh00, albpow, colh0, temph0, abu_c, flags=O.ASORA_MODE, max_iter=100):
    """evolve_oracle.evolve3D_oracle with LLS opacity (a, b): (xh_intermed, phi_ion, niter, history)."""
    pos0 = np.ravel((np.asarray(src_pos) - 1).astype("int32"), order="F")
    NumTau = thin.shape[0]

    def trace(xh_av):
        return raytrace(R_max_LLS, sig, dr, ndens, xh_av, pos0, src_flux, thin, thick, minlogtau, dlogtau, a, b, NumTau=NumTau,
                        flags=flags)["phi_ion"]

    def chemistry(xh_av, phi, xh_intermed):
        xh_intermed = xh_av.copy() if xh_intermed is None else xh_intermed
        xh_av, xh_intermed, conv_flag, _ = O.global_pass(dt, ndens, temp, xh, xh_av, xh_intermed, phi, bh00, albpow, colh0, temph0,
                                                         abu_c)
        return xh_av, xh_intermed, conv_flag, xh_intermed

    x, phi, niter, history, _ = _loop(trace, chemistry, xh, src_flux.shape[0], convergence_fraction, max_iter)
    return x, phi, niter, history


def evolve3D_lls_thermal_oracle(a, b, thermal_params, dt, dr, src_flux, src_pos, temp, ndens, xh, thin, thick, heat_thin, heat_thick,
                                minlogtau, dlogtau, R_max_LLS, convergence_fraction, sig, bh00, albpow, colh0, temph0, abu_c,
                                flags=O.ASORA_MODE, max_iter=100):
    """evolve_oracle.evolve3D_thermal_oracle with LLS opacity (a, b): (xh_intermed, T_end, phi_ion, phi_heat, niter, delth dt of
    the last pass, cells at max_substeps in it)."""
    import thermal_reference as TR
    pos0 = np.ravel((np.asarray(src_pos) - 1).astype("int32"), order="F")
    NumTau = thin.shape[0]

    def trace(xh_av):
        r = raytrace(R_max_LLS, sig, dr, ndens, xh_av, pos0, src_flux, thin, thick, minlogtau, dlogtau, a, b, NumTau=NumTau,
                     flags=flags, heat_thin=heat_thin, heat_thick=heat_thick)
        return r["phi_ion"], r["phi_heat"]

    def chemistry(xh_av, rates, _state):
        xh_intermed, xh_av, T_end, conv_flag, _stats, delta, capped = TR.chemistry_thermal(
            thermal_params, dt, ndens, temp, xh, xh_av, rates[0], rates[1], bh00, albpow, colh0, temph0, abu_c, return_delta=True)
        return xh_av, xh_intermed, conv_flag, (T_end, delta, capped)

    x, (phi, heat), niter, _, (T_end, delta, capped) = _loop(trace, chemistry, xh, src_flux.shape[0], convergence_fraction, max_iter)
    return x, T_end, phi, heat, niter, delta, capped


def evolve3d_lls_cpu_path(a, b, dt, dr, src_flux, src_pos, max_subbox, subboxsize, loss_fraction, temp, ndens, xh, thin, thick,
                          minlogtau, dlogtau, R, conv, sig, bh00, albpow, colh0, temph0, abu_c, max_iter=100):
    """evolve_oracle.evolve3d_cpu_path (the use_gpu=False branch on the sub-box oracle) with LLS opacity (a, b)."""
    def trace(xh_av):
        return O.do_all_sources(src_flux, src_pos, max_subbox, subboxsize, sig, dr, n_abs(ndens, xh_av, a, b), np.zeros(np.shape(ndens)),
                                loss_fraction, thin, thick, minlogtau, dlogtau, R)["phi_ion"]

    def chemistry(xh_av, phi, xh_intermed):
        xh_intermed = xh_av.copy() if xh_intermed is None else xh_intermed
        xh_av, xh_intermed, conv_flag, _ = O.global_pass(dt, ndens, temp, xh, xh_av, xh_intermed, phi, bh00, albpow, colh0, temph0,
                                                         abu_c)
        return xh_av, xh_intermed, conv_flag, xh_intermed

    x, phi, niter, _, _ = _loop(trace, chemistry, xh, src_flux.shape[0], conv, max_iter)
    return x, phi, niter
