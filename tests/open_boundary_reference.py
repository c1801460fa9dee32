"""TEST INFRASTRUCTURE: the CPU reference of a raytrace with open (non-periodic) boundaries, made of
the periodic oracle alone.

An open trace on an N-box equals the oracle's periodic ``asora_do_all_sources`` on a padded M-box, cropped to the N-box:
with M >= N + ceil(R) no sphere of radius R around a source of the embedded N-box reaches around the M-box back into it, so
what the open trace drops lands in the padding and is cropped away; and with R < N/2 - 1 neither box's periodic window
(offsets -N/2 ... N/2 - 1 + N % 2) clips the sphere, so both traces have the same reach.  Every upstream neighbour of an in-box
cell lies between that cell and the source, inside the N-box, so what the padding holds never reaches a cropped value: the
result does not depend on the padding's density and ionised fraction (`pad`), which the helper's own test asserts -- a wrong
embedding cannot pass that."""
import math

import numpy as np

from oracle import oracle as O


def padded_size(N, R):
    """The smallest padded mesh for an N-box traced to radius R."""
    return N + int(math.ceil(R))


def _check(N, R, M, offset):
    if not R < N / 2 - 1:
        raise ValueError(f"open-boundary reference: R = {R} must be below N/2 - 1 = {N / 2 - 1} (the periodic window must not clip)")
    if M < N + math.ceil(R):
        raise ValueError(f"open-boundary reference: padded mesh {M} smaller than N + ceil(R) = {N + math.ceil(R)}")
    if not 0 <= offset <= M - N:
        raise ValueError(f"open-boundary reference: offset {offset} leaves the N-box outside the padded mesh")


def embed(grid, M, offset, fill):
    """`grid` (N, N, N) at `offset` along every axis of an (M, M, M) mesh filled with `fill`."""
    N = grid.shape[0]
    out = np.full((M, M, M), float(fill))
    out[offset:offset + N, offset:offset + N, offset:offset + N] = grid
    return out


def crop(grid, N, offset):
    return np.ascontiguousarray(grid[offset:offset + N, offset:offset + N, offset:offset + N])


def open_trace(R, sig, dr, ndens, xh_av, src_pos0, src_flux, thin, thick, minlogtau, dlogtau, NumTau=None, flags=O.ASORA_MODE,
               heat_thin=None, heat_thick=None, M=None, offset=0, pad=(1e-2, 0.0)):
    """The open-boundary trace of the N-box: arguments as oracle.asora_do_all_sources (src_pos0: flat, 0-based, xyz-interleaved).
    M: padded mesh (default the smallest), offset: where the N-box sits in it, pad = (density, ionised fraction) of the padding.
    Returns {"phi_ion": (N, N, N)[, "phi_heat"]}."""
    N = ndens.shape[0]
    M = padded_size(N, R) if M is None else int(M)
    _check(N, R, M, offset)
    pos = np.asarray(src_pos0, dtype=np.int32) + np.int32(offset)
    r = O.asora_do_all_sources(R, sig, dr, embed(ndens, M, offset, pad[0]), embed(xh_av, M, offset, pad[1]), pos, src_flux, thin,
                               thick, minlogtau, dlogtau, NumTau=NumTau, flags=flags, heat_thin=heat_thin, heat_thick=heat_thick)
    out = {"phi_ion": crop(r["phi_ion"], N, offset)}
    if heat_thin is not None:
        out["phi_heat"] = crop(r["phi_heat"], N, offset)
    return out


def rated_pairs(N, R, src_pos0, periodic=False, dr=None):
    """(source, cell) pairs that receive a rate: lattice points within R of a source (inside the box when not periodic).  For
    R < N/2 - 1, where the periodic window does not clip.  With `dr` the distance test is the reference's, in its floating-point
    arithmetic (raytracing.cu:302-305,315: dist2 / dr^2 <= R^2 with dist2 from the cell's physical offsets), which decides the
    lattice points that sit exactly on the sphere -- for most cell sizes they fall outside by an ulp; dr a power of two keeps them."""
    pos = np.asarray(src_pos0).reshape(-1, 3)
    m = int(math.floor(R))
    d = np.arange(-m, m + 1)
    di, dj, dk = np.meshgrid(d, d, d, indexing="ij")
    if dr is None:
        inside = di * di + dj * dj + dk * dk <= R * R
    else:
        dr = np.float64(dr)
        xs, ys, zs = dr * di, dr * dj, dr * dk
        inside = ((xs * xs + ys * ys) + zs * zs) / (dr * dr) <= R * R
    total = 0
    for s in pos:
        ok = inside.copy()
        if not periodic:
            for ax, off in enumerate((di, dj, dk)):
                ok &= (s[ax] + off >= 0) & (s[ax] + off < N)
        total += int(ok.sum())
    return total


def evolve3D_open_oracle(dt, dr, src_flux, src_pos, temp, ndens, xh, thin, thick, minlogtau, dlogtau, R_max_LLS,
                         convergence_fraction, sig, bh00, albpow, colh0, temph0, abu_c, flags=O.ASORA_MODE, max_iter=100,
                         M=None, offset=0):
    """tests/evolve_oracle.py:evolve3D_oracle with open boundaries: per iteration the padded trace, cropped, then global_pass
    on the N-box.  src_pos (3, numsrc), 1-based.  Returns (xh_intermed, phi_ion, niter, history)."""
    NumSrc = src_flux.shape[0]
    N = temp.shape[0]
    NumCells = N ** 3
    NumTau = thin.shape[0]                                     # evolve.py:124
    conv_criterion = min(int(convergence_fraction * NumCells), (NumSrc - 1) / 3)
    prev1 = prev0 = 2 * NumCells
    xh_av = np.array(xh, dtype=np.float64, order="C", copy=True)
    xh_intermed = xh_av.copy()
    pos0 = np.ravel((np.asarray(src_pos) - 1).astype("int32"), order="F")
    history = []
    converged = False
    niter = 0
    phi = None
    while not converged and niter < max_iter:
        niter += 1
        phi = open_trace(R_max_LLS, sig, dr, np.ascontiguousarray(ndens), xh_av, pos0, src_flux, thin, thick, minlogtau, dlogtau,
                         NumTau=NumTau, flags=flags, M=M, offset=offset)["phi_ion"]
        xh_av, xh_intermed, conv_flag, _ = O.global_pass(dt, ndens, temp, xh, xh_av, xh_intermed, phi,
                                                         bh00, albpow, colh0, temph0, abu_c)
        s1 = np.sum(xh_intermed)
        s0 = np.sum(1.0 - xh_intermed)
        rel1 = abs((s1 - prev1) / s1) if s1 > 0 else 1.0
        rel0 = abs((s0 - prev0) / s0) if s0 > 0 else 1.0
        history.append((conv_flag, rel1, rel0))
        converged = (conv_flag < conv_criterion) or (rel1 < convergence_fraction and rel0 < convergence_fraction)
        prev1, prev0 = s1, s0
    return xh_intermed, phi, niter, history
