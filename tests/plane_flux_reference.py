"""TEST INFRASTRUCTURE: the plane-parallel flux through a face of the box on the CPU, in numpy.

``plane_trace`` restates the semantics the sweep kernel implements: the column density is a cumulative sum of n_abs dr along the
axis in travel order (the bits of the device's un-fused march), the rate is the reference's photoion_rates (rates.cu:16-41, the
table lookup of rates.cu:70-83 with numpy's log10) with the cell size for the path, divided by n_abs and kept where
cd_in <= MAX_COLDENSH.  The faces are handled by moving the march axis to the front and flipping it, so the six faces are images
of one computation.  ``evolve3D_plane_oracle`` is the loop of tests/evolve_oracle.py with the plane trace added to the oracle's
point-source trace, faces counting as sources in the convergence criterion."""
import numpy as np

from oracle import oracle as O

FACES = ("-x", "+x", "-y", "+y", "-z", "+z")
TAU_PHOTO_LIMIT = 1.0e-7       # rates.cu:7 (the library's default constants, O.ASORA_MODE)
MAX_COLDENSH = 2e30            # raytracing.cu:15


def face_index(face):
    return FACES.index(face) if isinstance(face, str) else int(face)


def to_march_order(a, face):
    """View of the (N, N, N) grid `a` with the face's march axis first, in travel order."""
    f = face_index(face)
    v = np.moveaxis(a, f >> 1, 0)
    return v[::-1] if f & 1 else v


def table_lookup(table, tau, minlogtau, dlogtau, NumTau):
    """photo_lookuptable (rates.cu:70-83; oracle/c2ray_oracle.c: table_lookup), vectorised."""
    table = np.asarray(table, dtype=np.float64)
    logtau = np.log10(np.maximum(1.0e-20, tau))
    real_i = np.minimum(float(np.float32(NumTau)), np.maximum(0.0, 1.0 + (logtau - minlogtau) / dlogtau))
    i0 = real_i.astype(np.int64)
    i1 = np.minimum(NumTau, i0 + 1)
    residual = real_i - i0
    last = table.shape[0] - 1
    i0, i1 = np.minimum(i0, last), np.minimum(i1, last)
    return table[i0] + residual * (table[i1] - table[i0])


def column_densities(n_abs, dr, face):
    """(cd_in, cd_out) of every cell in march order of the face (axis 0 = travel order)."""
    inc = to_march_order(np.asarray(n_abs, dtype=np.float64), face) * np.float64(dr)
    cd_out = np.cumsum(inc, axis=0)            # sequential along the axis: cd_out(m) = cd_out(m-1) + n_abs(m) dr
    cd_in = np.concatenate([np.zeros((1,) + cd_out.shape[1:]), cd_out[:-1]], axis=0)
    return cd_in, cd_out


def plane_trace(face, flux, n_abs, dr, sig, thin, thick, minlogtau, dlogtau, NumTau=None, heat_thin=None, heat_thick=None,
                details=False):
    """Rates per absorber of one face: phi_ion (N, N, N) in the grid's own index order, and phi_heat when both heating tables are
    given (else None).  details=True: also a dict of the march-ordered cd_in, cd_out, thick mask, rated mask and n_abs."""
    n_abs = np.asarray(n_abs, dtype=np.float64)
    NumTau = np.shape(thin)[0] if NumTau is None else NumTau
    nm = to_march_order(n_abs, face)
    cd_in, cd_out = column_densities(n_abs, dr, face)
    tau_in, tau_out = cd_in * sig, cd_out * sig
    dtau = tau_out - tau_in
    is_thick = np.abs(dtau) > TAU_PHOTO_LIMIT
    rated = cd_in <= MAX_COLDENSH
    prefact = np.float64(flux) / np.float64(dr)
    look = lambda t, tau: table_lookup(t, tau, minlogtau, dlogtau, NumTau)

    def rate(t_thick, t_thin):
        phi = np.where(is_thick, prefact * (look(t_thick, tau_in) - look(t_thick, tau_out)), prefact * dtau * look(t_thin, tau_out))
        with np.errstate(divide="ignore", invalid="ignore"):
            per_atom = np.where(rated, phi / nm, 0.0)
        out = np.empty(n_abs.shape)
        to_march_order(out, face)[...] = per_atom           # (a view: written back in the grid's own order)
        return out

    phi_ion = rate(thick, thin)
    phi_heat = rate(heat_thick, heat_thin) if heat_thin is not None and heat_thick is not None else None
    if details:
        return phi_ion, phi_heat, dict(cd_in=cd_in, cd_out=cd_out, thick=is_thick, rated=rated, n_abs=nm)
    return phi_ion, phi_heat


def absorbed_per_ray(phi_ion, n_abs, dr, face):
    """sum over the ray of phi n_abs dr, in march order: the photons s^-1 cm^-2 (x 1e-48) the ray's cells absorb."""
    return np.sum(to_march_order(phi_ion * n_abs, face) * dr, axis=0)


def telescoped_per_ray(flux, n_abs, dr, sig, thick, minlogtau, dlogtau, face, NumTau=None):
    """flux (T_thick(0) - T_thick(tau_total)) of every ray, and the share of the flux that is absorbed."""
    NumTau = np.shape(thick)[0] if NumTau is None else NumTau
    _, cd_out = column_densities(n_abs, dr, face)
    t0 = table_lookup(thick, np.zeros(cd_out.shape[1:]), minlogtau, dlogtau, NumTau)
    t1 = table_lookup(thick, cd_out[-1] * sig, minlogtau, dlogtau, NumTau)
    return flux * (t0 - t1), (t0 - t1) / t0


def faces_trace(faces, n_abs, dr, sig, tables, minlogtau, dlogtau, NumTau=None, heat=False):
    """Sum over `faces`, (face, flux, spectrum) triples; tables[spectrum] = (thin, thick[, heat_thin, heat_thick])."""
    phi = np.zeros(np.shape(n_abs))
    h = np.zeros(np.shape(n_abs)) if heat else None
    for face, flux, spectrum in faces:
        t = tables[spectrum]
        kw = dict(heat_thin=t[2], heat_thick=t[3]) if heat else {}
        a, b = plane_trace(face, flux, n_abs, dr, sig, t[0], t[1], minlogtau, dlogtau, NumTau=NumTau, **kw)
        phi += a
        if heat:
            h += b
    return phi, h


def evolve3D_plane_oracle(faces, dt, dr, src_flux, src_pos, temp, ndens, xh, thin, thick, minlogtau, dlogtau, R_max_LLS,
                          convergence_fraction, sig, bh00, albpow, colh0, temph0, abu_c, thermal_params=None, heat_thin=None,
                          heat_thick=None, clumping=None, max_iter=100):
    """evolve3D(..., plane_flux=faces) on the CPU: per iteration the oracle's point-source trace (skipped without point sources)
    plus the plane trace, then O.global_pass -- or, with `thermal_params` (a thermal_reference.Params) and the heating tables,
    thermal_reference.chemistry_thermal.  faces: (face, flux) pairs, all on the one table set.  The convergence criterion counts
    the faces as sources.  With `clumping` (a factor or a grid) the step is step_reference.reference_step's, which has the clumped
    passes; without, this loop stays as it is: it is one of the restatements that anchor that function.
    Returns (xh_intermed, phi_ion, niter, history[, T_end, phi_heat])."""
    if clumping is not None:
        from step_reference import reference_step
        case = dict(dt=dt, dr=dr, flux=np.asarray(src_flux, dtype=np.float64).ravel(), pos=np.asarray(src_pos).reshape(3, -1), temp=temp,
                    ndens=ndens, xh=xh, thin=thin, thick=thick, heat_thin=heat_thin, heat_thick=heat_thick, minlogtau=minlogtau,
                    dlogtau=dlogtau, R=R_max_LLS, conv=convergence_fraction, sig=sig, chem=(bh00, albpow, colh0, temph0, abu_c))
        r = reference_step(case, thermal=thermal_params, clump=clumping, faces=[(f, x, 0) for f, x in faces], max_iter=max_iter)
        out = (r["xh_intermed"], r["phi_ion"], r["niter"], r["history"])
        return out + (r["T_end"], r["phi_heat"]) if thermal_params is not None else out
    NumSrc = int(np.size(src_flux))
    NumCells = ndens.size
    NumTau = thin.shape[0]
    thermal = thermal_params is not None
    tables = {0: (thin, thick, heat_thin, heat_thick)}
    triples = [(f, x, 0) for f, x in faces]
    conv_criterion = min(int(convergence_fraction * NumCells), (NumSrc + len(triples) - 1) / 3)
    prev1 = prev0 = 2 * NumCells
    xh_av = np.array(xh, dtype=np.float64, order="C", copy=True)
    xh_intermed = xh_av.copy()
    nd = np.ascontiguousarray(ndens, dtype=np.float64)
    T_end = heat = None
    pos0 = np.ravel((np.asarray(src_pos).reshape(3, -1) - 1).astype("int32"), order="F") if NumSrc else None
    history, niter, converged = [], 0, False
    while not converged and niter < max_iter:
        niter += 1
        phi, heat = faces_trace(triples, nd * (1.0 - xh_av), dr, sig, tables, minlogtau, dlogtau, NumTau=NumTau, heat=thermal)
        if NumSrc:
            kw = dict(heat_thin=heat_thin, heat_thick=heat_thick) if thermal else {}
            r = O.asora_do_all_sources(R_max_LLS, sig, dr, nd, xh_av, pos0, np.asarray(src_flux, dtype=np.float64), thin, thick,
                                       minlogtau, dlogtau, NumTau=NumTau, **kw)
            phi = phi + r["phi_ion"]
            if thermal:
                heat = heat + r["phi_heat"]
        if thermal:
            import thermal_reference as TR
            xh_intermed, xh_av, T_end, conv_flag, _stats = TR.chemistry_thermal(thermal_params, dt, nd, temp, xh, xh_av, phi, heat,
                                                                                bh00, albpow, colh0, temph0, abu_c)
        else:
            xh_av, xh_intermed, conv_flag, _ = O.global_pass(dt, nd, temp, xh, xh_av, xh_intermed, phi, bh00, albpow, colh0,
                                                             temph0, abu_c)
        s1, s0 = np.sum(xh_intermed), np.sum(1.0 - xh_intermed)
        rel1 = abs((s1 - prev1) / s1) if s1 > 0 else 1.0
        rel0 = abs((s0 - prev0) / s0) if s0 > 0 else 1.0
        history.append((conv_flag, rel1, rel0))
        converged = (conv_flag < conv_criterion) or (rel1 < convergence_fraction and rel0 < convergence_fraction)
        prev1, prev0 = s1, s0
    if thermal:
        return xh_intermed, phi, niter, history, T_end, heat
    return xh_intermed, phi, niter, history


def checkerboard_xh(xh, block=4, value=1.0 - 1e-7):
    """`xh` with `value` on the "black" blocks of a checkerboard of block^3 cells: cells there are optically thin."""
    N = xh.shape[0]
    i = np.arange(N) // block
    black = ((i[:, None, None] + i[None, :, None] + i[None, None, :]) & 1) == 1
    out = np.array(xh, copy=True)
    out[black] = value
    return out


def checkerboard_medium(N, seed=3):
    """(ndens, xh, dr) of the thin / thick case: cases.grid(N, "lognormal", seed, tau_cell) with xh = 1 - 1e-7 on the black blocks.
    tau_cell is chosen from the density field alone, so that the densest black cell has tau_out - tau_in = 0.9e-7, below
    TAU_PHOTO_LIMIT: every black cell is thin, every white one thick by a wide margin (at N = 67: 8e-6 and more).  The reason: a
    cell that is thick by a small dtau takes the difference T(tau_in) - T(tau_out) of two nearly equal table values, whose own
    rounding -- 1e-16 from the two products prefact T of the reference where this restatement forms prefact (T - T), 5e-14 from
    the last place of the table index -- is divided by dtau; cells with dtau between 1e-7 and a few 1e-6 therefore differ between
    any two correct evaluations by more than the 1e-10 (CPU) and 1e-8 (device) the comparisons assert, the reference's CUDA and
    Fortran forms among them.  The lognormal field spans five decades; this tau_cell keeps every cell out of that band."""
    import cases
    nd, xh, _ = cases.grid(N, "lognormal", seed, 1.0)
    tau_cell = 0.9 / (nd.max() / 1e-3)
    return nd, checkerboard_xh(xh), tau_cell / (cases.SIG * 1e-3)


# ---- the planar ionisation front shared by the CPU test and the GPU test ---------------------------------------------------------
def ifront_case():
    """A planar I-front in a uniform medium: N = 32, n = 1e-3 cm^-3 at 1e4 K, cells of optical depth 2, grey tables, a flux through
    the -x face whose Stroemgren length F / (alpha_B n^2) is 40 cells; ten steps of a tenth of a recombination time each."""
    import cases
    N, n, tau_cell = 32, 1.0e-3, 2.0
    dr = tau_cell / (cases.SIG * n)
    thin, thick, dlog = cases.grey_tables()
    photons = 40.0 * dr * cases.BH00 * n * n                 # photons s^-1 cm^-2
    t_rec = 1.0 / (cases.BH00 * n)
    return dict(N=N, n=n, dr=dr, thin=thin, thick=thick, dlogtau=dlog, flux=photons / thick[0], photons=photons, dt=0.1 * t_rec,
                steps=10, t_rec=t_rec, ndens=np.full((N, N, N), n), temp=np.full((N, N, N), 1.0e4), xh0=np.full((N, N, N), 1.0e-4),
                convergence_fraction=1e-4)


def ifront_analytic_cells(c, t):
    """x_f(t) = (F / (alpha_B n^2)) (1 - exp(-alpha_B n t)), in cells."""
    return c["photons"] / (c["n"] ** 2 * 2.59e-13) * (1.0 - np.exp(-t / c["t_rec"])) / c["dr"]


def front_position_cells(xh_ray):
    """Where the ionised fraction along a ray (cell centres at m + 0.5) falls through 0.5, by linear interpolation."""
    below = np.nonzero(xh_ray < 0.5)[0]
    m = int(below[0])
    if m == 0:
        return 0.0
    return (m - 0.5) + (xh_ray[m - 1] - 0.5) / (xh_ray[m - 1] - xh_ray[m])


_IFRONT = {}


def ifront_reference():
    """The ten steps on the CPU, computed once: list of (xh, phi_ion, niter) per step."""
    import cases
    if "steps" not in _IFRONT:
        c = ifront_case()
        xh, out = c["xh0"], []
        for _ in range(c["steps"]):
            xh, phi, niter, _h = evolve3D_plane_oracle([("-x", c["flux"])], c["dt"], c["dr"], np.zeros(0), np.zeros((3, 0), dtype=int),
                                                       c["temp"], c["ndens"], xh, c["thin"], c["thick"], cases.MINLOGTAU, c["dlogtau"],
                                                       1000.0, c["convergence_fraction"], cases.SIG, cases.BH00, cases.ALBPOW,
                                                       cases.COLH0, cases.TEMPH0, cases.ABU_C)
            out.append((xh, phi, niter))
        _IFRONT["steps"] = out
    return _IFRONT["steps"]
