"""TEST INFRASTRUCTURE: one composable CPU reference of a time step, and the inputs of the feature-combination matrix.

``reference_step`` is evolve3D(..., thermal=, clumping=, src_spectrum=, lls=, periodic=, plane_flux=, budget=) on the CPU with
any subset of the keywords on at once.  It is composed of the pieces the single-feature references are made of, and of nothing
else:

* the absorber density of every trace is ``lls_reference.n_abs`` (a = b = 0 without LLS), handed to the oracle as its density with
  an ionised fraction of 0, as ``lls_reference.raytrace`` does;
* the point sources are traced one spectrum at a time -- the oracle on that spectrum's sources with its tables -- and the rates
  added up (they are linear in the sources at fixed nHI: tests/test_gpu_spectra.py, test_two_black_bodies_against_the_oracle);
  periodic: ``oracle.asora_do_all_sources``, open: ``open_boundary_reference.open_trace`` on the padded mesh;
* the faces are ``plane_flux_reference.faces_trace`` of the same absorber density;
* the chemistry is ``oracle.global_pass``, ``clumping_reference.chemistry_pass``, ``thermal_reference.chemistry_thermal`` or
  ``clumping_reference.chemistry_thermal``;
* the loop and its convergence test are ``lls_reference._loop``, faces counting as sources in the criterion
  (``plane_flux_reference.evolve3D_plane_oracle``).

With exactly one feature on it returns the bits of that feature's own restatement (tests/test_step_reference_host.py), which
stay as they are: they are what anchors this one.

The second half holds the inputs of the matrix (tests/test_gpu_feature_matrix.py): the rows of a two-level orthogonal array of
strength 2 over the seven keywords plus the all-on row, and the case they run on."""
import functools

import numpy as np

import budget_reference as BR
import cases
import clumping_reference as CR
import lls_reference as LR
import open_boundary_reference as OB
import plane_flux_reference as PF
import thermal_reference as TR
from oracle import oracle as O

CHEM = (cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)


def _table_sets(case, spectra):
    """(spectrum of every source, [(thin, thick, heat_thin, heat_thick) per set]); heating tables None where the case has none."""
    ns = int(np.size(case["flux"]))
    if spectra is None:
        return np.zeros(ns, dtype=np.int64), [(case["thin"], case["thick"], case.get("heat_thin"), case.get("heat_thick"))]
    src_spectrum, sets = spectra
    src_spectrum = np.asarray(src_spectrum, dtype=np.int64)
    if src_spectrum.shape != (ns,):
        raise ValueError(f"reference_step: {ns} sources, spectra for {src_spectrum.shape}")
    return src_spectrum, [tuple(s) + (None,) * (4 - len(s)) for s in sets]


def reference_step(case, *, thermal=None, clump=None, spectra=None, lls=None, periodic=True, faces=(), budget=False, max_iter=100):
    """One time step on the CPU.

    case: dict(dt, dr, flux (ns), pos (3, ns) 1-based, temp, ndens, xh, thin, thick, dlogtau, R, conv), and optionally heat_thin /
    heat_thick (the heating tables of table set 0), M (the padded mesh of an open step; default the smallest), minlogtau, sig,
    chem = (bh00, albpow, colh0, temph0, abu_c).
    thermal: None or a thermal_reference.Params.  clump: None, a factor or an (N, N, N) grid.  spectra: None (every source on the
    case's own tables) or (spectrum per source, [(thin, thick[, heat_thin, heat_thick]) per table set]).  lls: None or (n_const,
    per_density).  periodic=False: open boundaries.  faces: (face, flux[, spectrum]) tuples.  budget: also the twelve sums.

    Returns a dict: xh_intermed, phi_ion, niter, history (rows (conv_flag, rel1, rel0)), xh_av (of the last pass) and
    conv_criterion; with thermal T_end and phi_heat; with budget budget_sums and budget_mag (budget_reference.sums of the
    reference's own grids: x0 = the case's xh, x1 = xh_intermed, the last xh_av, phi_ion, the case's temp and -- thermal -- T_end)."""
    dt, dr, R, conv = case["dt"], case["dr"], case["R"], case["conv"]
    sig, minlogtau, dlogtau = case.get("sig", cases.SIG), case.get("minlogtau", cases.MINLOGTAU), case["dlogtau"]
    chem = tuple(case.get("chem", CHEM))
    ndens, temp, xh = case["ndens"], case["temp"], case["xh"]
    flux = np.asarray(case["flux"], dtype=np.float64)
    NumSrc = int(flux.size)
    pos = np.asarray(case["pos"]).reshape(3, -1)
    heat = thermal is not None
    src_spectrum, sets = _table_sets(case, spectra)
    NumTau = sets[0][0].shape[0]                                  # (the table LENGTH is what the loops pass, evolve.py:124)
    triples = [(f[0], f[1], f[2] if len(f) > 2 else 0) for f in faces]
    used = sorted(set(src_spectrum.tolist()) | {s for _, _, s in triples})
    if used and not 0 <= used[0] <= used[-1] < len(sets):
        raise ValueError(f"reference_step: spectra {used} with {len(sets)} table set(s)")
    if heat and any(sets[s][2] is None or sets[s][3] is None for s in used):
        raise ValueError("reference_step: thermal needs the heating tables of every table set in use")
    a, b = (0.0, 0.0) if lls is None else lls
    nd = np.ascontiguousarray(ndens, dtype=np.float64)
    zeros = np.zeros(nd.shape)
    sources = []                                                  # (flat 0-based positions, fluxes, table set) per spectrum
    for s in sorted(set(src_spectrum.tolist())):
        sel = np.flatnonzero(src_spectrum == s)
        sources.append((np.ravel((pos[:, sel] - 1).astype("int32"), order="F"), flux[sel], sets[s]))

    def trace(xh_av):
        nabs = LR.n_abs(nd, xh_av, a, b)
        phi = h = None
        for pos0, f, (thin, thick, ht, hk) in sources:
            kw = dict(heat_thin=ht, heat_thick=hk) if heat else {}
            if periodic:
                r = O.asora_do_all_sources(R, sig, dr, nabs, zeros, pos0, f, thin, thick, minlogtau, dlogtau, NumTau=NumTau, **kw)
            else:
                r = OB.open_trace(R, sig, dr, nabs, zeros, pos0, f, thin, thick, minlogtau, dlogtau, NumTau=NumTau, M=case.get("M"), **kw)
            phi = r["phi_ion"] if phi is None else phi + r["phi_ion"]
            if heat:
                h = r["phi_heat"] if h is None else h + r["phi_heat"]
        if triples:
            fp, fh = PF.faces_trace(triples, nabs, dr, sig, dict(enumerate(sets)), minlogtau, dlogtau, NumTau=NumTau, heat=heat)
            phi = fp if phi is None else fp + phi
            if heat:
                h = fh if h is None else fh + h
        if phi is None:
            phi, h = np.zeros(nd.shape), (np.zeros(nd.shape) if heat else None)
        return phi, h

    def chemistry(xh_av, rates, state):
        phi, h = rates
        if heat and clump is None:
            x, xh_av, T_end, conv_flag, _stats = TR.chemistry_thermal(thermal, dt, nd, temp, xh, xh_av, phi, h, *chem)
            return xh_av, x, conv_flag, T_end
        if heat:
            x, xh_av, T_end, conv_flag, _delta, _capped = CR.chemistry_thermal(thermal, dt, nd, temp, xh, xh_av, phi, h, *chem, clump)
            return xh_av, x, conv_flag, T_end
        if clump is None:
            x = xh_av.copy() if state is None else state
            xh_av, x, conv_flag, _ = O.global_pass(dt, nd, temp, xh, xh_av, x, phi, *chem)
            return xh_av, x, conv_flag, x
        x, xh_av, conv_flag, _sum = CR.chemistry_pass(dt, nd, temp, xh, xh_av, phi, *chem, clump)
        return xh_av, x, conv_flag, x

    last = {}

    def chemistry_keeping_xav(xh_av, rates, state):
        out = chemistry(xh_av, rates, state)
        last["xh_av"] = out[0]
        return out

    x, (phi, h), niter, history, state = LR._loop(trace, chemistry_keeping_xav, xh, NumSrc + len(triples), conv, max_iter)
    out = dict(xh_intermed=x, phi_ion=phi, niter=niter, history=[tuple(row[:3]) for row in history], xh_av=last["xh_av"],
               conv_criterion=min(int(conv * xh.size), (NumSrc + len(triples) - 1) / 3))
    if heat:
        out.update(T_end=state, phi_heat=h)
    if budget:
        s, mag = BR.sums(nd, xh, x, last["xh_av"], phi, temp, chem, 1.0 if clump is None else clump, (a, b), out.get("T_end"))
        out.update(budget_sums=s, budget_mag=mag)
    return out


# ---- the feature-combination matrix ------------------------------------------------------------------------------------------
FEATURES = ("thermal", "clumping", "spectra", "lls", "open", "faces", "budget")
#: the eight rows of the two-level orthogonal array of strength 2 over seven columns (every pair of features occurs on/on, on/off,
#: off/on and off/off), then the all-on row
ROWS = ("0000000", "1010101", "0110011", "1100110", "0001111", "1011010", "0111100", "1101001", "1111111")
#: (row, N): the nine rows at N = 24, and the all-on row once more at N = 17 (an odd cell count)
MATRIX = tuple((row, 24) for row in ROWS) + (("1111111", 17),)
RANK_ROWS = ("1111111", "1010101", "0111100")
#: max_substeps = 400: on the rows without LLS two source cells cool to the floor and stay there substep after substep until the
#: cap; every other cell needs fewer than 20 substeps.  With the library's default of 10000 the numpy pass takes 2 s instead of 10 ms
#: for the same temperatures, and at 400 the last-substep path of the integrator is part of the matrix.
THERMAL = dict(relative_denergy=0.1, t_floor=1.0, max_substeps=400, cooling_mask=31, compton=False, t_cmb=0.0)
#: the flux of every point source (1e48 photons/s).  The issue of the matrix leaves it open; it is chosen on the CPU reference
#: alone, so that every case meets the decision margin of tests/test_step_reference_host.py (no outer iteration within 2 cells or
#: 1e-3 of the convergence test's thresholds): with one value for all ten cases a scan of 1.5e-4 ... 6.8e-4 finds none that does,
#: 3.3e-4 leaves out one row, and that row takes 3.15e-4.
SOURCE_FLUX = 3.3e-4
ROW_SOURCE_FLUX = {"1100110": 3.15e-4}
_SOURCES = {24: ((0, 7, 9), (15, 6, 23), (11, 12, 13), (23, 23, 0)), 17: ((0, 7, 9), (8, 6, 16), (16, 16, 0))}


def features_of(row):
    return {name: bit == "1" for name, bit in zip(FEATURES, row)}


@functools.lru_cache(maxsize=None)
def matrix_case(N):
    """The case of the matrix at mesh N (24 or 17), every array read-only.  R = 6, dt = 2 Myr, the lognormal medium of the other
    step tests with the soft tables; sources on the first and last planes of every axis, alternating between two table sets; the
    second set is a mix of the first set's thin and thick tables, and its heating tables have the opposite slope along tau, so
    neither is proportional to the first set's.  The heating tables are a hundredth of those of the thermal step tests
    (tests/test_gpu_plane_flux.py, test_thermal_evolve3D_against_the_oracle_loop, says why)."""
    nd, xh, dr = cases.grid(N, "lognormal", 61, 0.2, xlo=1e-4, xhi=2e-3)
    thin, thick, dlog = cases.soft_tables()
    n = thin.shape[0]
    src = np.array(_SOURCES[N], dtype=np.int32)
    thin2, thick2 = 0.5 * thin + 0.3 * thick, 0.25 * thick + 0.2 * thin
    up, down = np.linspace(1.0, 2.0, n), np.linspace(2.0, 1.0, n)
    sets = ((thin, thick, 0.01 * 1e-11 * thin * up, 0.01 * 0.7e-11 * thick * down),
            (thin2, thick2, 0.01 * 1.5e-11 * thin2 * down, 0.01 * 1e-11 * thick2 * up))
    c = dict(N=N, ndens=nd, xh=xh, dr=dr, temp=np.full((N, N, N), 1e4), pos=(src + 1).T.copy(), flux=np.full(len(src), SOURCE_FLUX),
             spectrum=np.array([0, 1, 0, 1][:len(src)], dtype=np.int32), thin=thin, thick=thick, heat_thin=sets[0][2],
             heat_thick=sets[0][3], sets=sets, dlogtau=dlog, R=6.0, dt=2 * cases.MYR, conv=1e-4, M=N + 6,
             faces=(("-x", 3.0e-45, 0), ("+z", 1.5e-45, 1)), lls=(0.05 / (cases.SIG * dr), 0.2),
             clump=np.exp(np.random.default_rng(9).normal(1.0, 0.8, (N, N, N))).clip(1.0, 50.0))
    for v in list(c.values()) + [t for s in sets for t in s]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def case_of(row, N):
    """matrix_case(N) with the row's own source flux where it has one (ROW_SOURCE_FLUX)."""
    c = matrix_case(N)
    if row in ROW_SOURCE_FLUX:
        flux = np.full(c["flux"].shape, ROW_SOURCE_FLUX[row])
        flux.setflags(write=False)
        c = dict(c, flux=flux)
    return c


def reference_options(row, c):
    """The keywords of reference_step for a row on the case `c`.  Without the spectra column every source and every face is on
    table set 0."""
    f = features_of(row)
    faces = tuple((face, x, s if f["spectra"] else 0) for face, x, s in c["faces"]) if f["faces"] else ()
    return dict(thermal=TR.Params(**THERMAL) if f["thermal"] else None, clump=c["clump"] if f["clumping"] else None,
                spectra=(c["spectrum"], c["sets"]) if f["spectra"] else None, lls=c["lls"] if f["lls"] else None,
                periodic=not f["open"], faces=faces, budget=f["budget"])


def _frozen(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def matrix_reference(row, N, step=1):
    """The reference of step `step` (1 or 2) of a row: computed once per process and shared, read-only.  Step 2 starts from step
    1's xh_intermed and, on thermal rows, T_end."""
    c = case_of(row, N)
    if step > 1:
        before = matrix_reference(row, N, step - 1)
        c = dict(c, xh=before["xh_intermed"], temp=before.get("T_end", c["temp"]))
    return _frozen(reference_step(c, **reference_options(row, c)))
