"""CPU: the composable reference of a time step (tests/step_reference.py) and the inputs of the feature-combination matrix.

* Anchoring: with exactly one feature on, ``reference_step`` returns the bits of that feature's own restatement, on that
  restatement's own test case.
* The rows are an orthogonal array of strength 2.
* Fixed conditions on the matrix inputs, on the reference alone, for every case of tests/test_gpu_feature_matrix.py:
  (a) conditioning, (b) decision margin, (c) every feature of the row matters, (d) open rows differ from periodic ones.
  They are conditions on the inputs, not measurements of the device: a case that misses one gets other inputs.

Measured (a), the largest relative answer of xh_intermed / T_end to a relative change of 1e-11 of every flux, and the outer
iterations: 0000000 3.4e-11 (8), 1010101 1.7e-11 / 1.2e-11 (8), 0110011 1.5e-10 (8), 1100110 7.8e-11 / 1.3e-11 (8), 0001111 2.1e-11
(6), 1011010 2.2e-11 / 1.2e-12 (6), 0111100 1.7e-11 (6), 1101001 1.9e-11 / 8.9e-13 (6), 1111111 2.2e-11 / 1.2e-12 (6), 1111111 at
N = 17 1.6e-11 / 1.2e-12 (6)."""
import itertools

import numpy as np
import pytest

import cases
import lls_reference as LR
import open_boundary_reference as OB
import plane_flux_reference as PF
import step_reference as SR
import thermal_reference as TR
from evolve_oracle import evolve3D_oracle, evolve3D_thermal_oracle

CHEM = SR.CHEM
IDS = [f"{row}-N{N}" for row, N in SR.MATRIX]


# ---- anchoring ---------------------------------------------------------------------------------------------------------------
def _same(got, ref, keys):
    """got: reference_step's dict; ref: {key: array or count} of the restatement"""
    for k in keys:
        if k == "niter":
            assert got[k] == ref[k], (k, got[k], ref[k])
        else:
            assert np.array_equal(got[k], ref[k]), k


def _case(c, conv="conv"):
    out = dict(dt=c["dt"], dr=c["dr"], flux=c["flux"], pos=c["pos"], temp=c["temp"], ndens=c["ndens"], xh=c["xh"], thin=c["thin"],
               thick=c["thick"], dlogtau=c["dlogtau"], R=c["R"], conv=c[conv])
    for k in ("heat_thin", "heat_thick"):
        if k in c:
            out[k] = c[k]
    return out


def _tail(c, conv="conv"):
    return (cases.MINLOGTAU, c["dlogtau"], c["R"], c[conv], cases.SIG) + CHEM


def test_plain_and_thermal_steps_are_the_evolve_oracles():
    """tests/evolve_oracle.py on the golden case l16_gpu_F (tests/test_evolve_golden.py), isothermal and with its heating tables."""
    c = cases.evolve_case("l16_gpu_F")
    args = (c["dt"], c["dr"], c["flux"], c["pos"], c["temp"], c["ndens"], c["xh"], c["thin"], c["thick"])
    x, phi, niter, _ = evolve3D_oracle(*args, *_tail(c, "convergence_fraction"))
    got = SR.reference_step(_case(c, "convergence_fraction"))
    _same(got, dict(xh_intermed=x, phi_ion=phi, niter=niter), ("xh_intermed", "phi_ion", "niter"))
    assert niter >= 2 and "T_end" not in got
    prm = TR.Params()
    x, T, phi, heat, niter, _ = evolve3D_thermal_oracle(prm, *args, c["heat_thin"], c["heat_thick"], *_tail(c, "convergence_fraction"))
    got = SR.reference_step(_case(c, "convergence_fraction"), thermal=prm)
    _same(got, dict(xh_intermed=x, T_end=T, phi_ion=phi, phi_heat=heat, niter=niter), ("xh_intermed", "T_end", "phi_ion", "phi_heat", "niter"))
    assert niter >= 2 and T.max() > 1.05e4


def test_lls_steps_are_the_substituted_oracle_loops():
    """tests/lls_reference.py on the step case of tests/test_gpu_lls.py, isothermal and thermal."""
    from test_gpu_lls import _step_case
    c = _step_case()
    args = (c["dt"], c["dr"], c["flux"], c["pos"], c["temp"], c["ndens"], c["xh"], c["thin"], c["thick"])
    x, phi, niter, _ = LR.evolve3D_lls_oracle(c["a"], c["b"], *args, *_tail(c))
    got = SR.reference_step(_case(c), lls=(c["a"], c["b"]))
    _same(got, dict(xh_intermed=x, phi_ion=phi, niter=niter), ("xh_intermed", "phi_ion", "niter"))
    prm = TR.Params()
    x, T, phi, heat, niter, _, _ = LR.evolve3D_lls_thermal_oracle(c["a"], c["b"], prm, *args, c["heat_thin"], c["heat_thick"], *_tail(c))
    got = SR.reference_step(_case(c), lls=(c["a"], c["b"]), thermal=prm)
    _same(got, dict(xh_intermed=x, T_end=T, phi_ion=phi, phi_heat=heat, niter=niter), ("xh_intermed", "T_end", "phi_ion", "phi_heat", "niter"))
    assert niter >= 2


def test_open_step_is_the_padded_oracle_loop():
    """tests/open_boundary_reference.py on the step case of tests/test_gpu_open_boundaries.py (sources on corners, an edge, a face)."""
    from test_gpu_open_boundaries import _step_case
    c = _step_case(interior=False)
    x, phi, niter, _ = OB.evolve3D_open_oracle(c["dt"], c["dr"], c["flux"], c["pos"], c["temp"], c["ndens"], c["xh"], c["thin"], c["thick"],
                                               *_tail(c), M=24)
    got = SR.reference_step(dict(_case(c), M=24), periodic=False)
    _same(got, dict(xh_intermed=x, phi_ion=phi, niter=niter), ("xh_intermed", "phi_ion", "niter"))
    assert niter >= 2 and not np.array_equal(SR.reference_step(_case(c))["phi_ion"], phi)


def test_steps_with_faces_are_the_plane_oracle_loop_and_its_clumping_is_honoured():
    """tests/plane_flux_reference.py on the step case of tests/test_gpu_plane_flux.py, plain and thermal (with that test's heating
    tables); and evolve3D_plane_oracle(clumping=) now changes the result."""
    from test_gpu_plane_flux import _step_case
    c = _step_case()
    args = (c["dt"], c["dr"], c["flux"], c["pos"], c["temp"], c["ndens"], c["xh"], c["thin"], c["thick"])
    x, phi, niter, _ = PF.evolve3D_plane_oracle(c["faces"], *args, *_tail(c))
    got = SR.reference_step(_case(c), faces=c["faces"])
    _same(got, dict(xh_intermed=x, phi_ion=phi, niter=niter), ("xh_intermed", "phi_ion", "niter"))
    ht, hk = 0.01 * c["heat_thin"], 0.01 * c["heat_thick"]
    prm = TR.Params()
    xt, phit, nitert, _, T, heat = PF.evolve3D_plane_oracle(c["faces"], *args, *_tail(c), thermal_params=prm, heat_thin=ht, heat_thick=hk)
    got = SR.reference_step(dict(_case(c), heat_thin=ht, heat_thick=hk), faces=c["faces"], thermal=prm)
    _same(got, dict(xh_intermed=xt, T_end=T, phi_ion=phit, phi_heat=heat, niter=nitert), ("xh_intermed", "T_end", "phi_ion", "phi_heat", "niter"))
    assert niter >= 2 and nitert >= 2
    # faces only, no point source: the empty source list
    none = (np.zeros(0), np.zeros((3, 0), dtype=int))
    x0, phi0, n0, _ = PF.evolve3D_plane_oracle(c["faces"], c["dt"], c["dr"], *none, *args[4:], *_tail(c))
    got = SR.reference_step(dict(_case(c), flux=none[0], pos=none[1]), faces=c["faces"])
    _same(got, dict(xh_intermed=x0, phi_ion=phi0, niter=n0), ("xh_intermed", "phi_ion", "niter"))
    # clumping=: a factor of 1 is the unclumped step to rounding (another statement of the same pass), a grid is not
    one = PF.evolve3D_plane_oracle(c["faces"], *args, *_tail(c), clumping=1.0)
    assert one[2] == niter
    np.testing.assert_allclose(one[0], x, rtol=1e-9, atol=0)
    clump = np.exp(np.random.default_rng(9).normal(1.0, 0.8, c["xh"].shape)).clip(1.0, 50.0)
    xc, phic, _, _ = PF.evolve3D_plane_oracle(c["faces"], *args, *_tail(c), clumping=clump)
    assert np.max(np.abs(xc - x) / x) > 1e-3 and xc.mean() < x.mean()                      # more recombinations, fewer ions
    xtc = PF.evolve3D_plane_oracle(c["faces"], *args, *_tail(c), thermal_params=prm, heat_thin=ht, heat_thick=hk, clumping=clump)
    assert len(xtc) == 6 and np.max(np.abs(xtc[0] - xt) / xt) > 1e-3


# ---- the array ---------------------------------------------------------------------------------------------------------------
def test_rows_are_an_orthogonal_array_of_strength_two_plus_the_all_on_row():
    rows = SR.ROWS[:8]
    assert all(len(r) == len(SR.FEATURES) == 7 for r in SR.ROWS) and SR.ROWS[8] == "1111111" and len(set(SR.ROWS)) == 9
    for i, j in itertools.combinations(range(7), 2):
        pairs = sorted(r[i] + r[j] for r in rows)
        assert pairs == ["00", "00", "01", "01", "10", "10", "11", "11"], (i, j, pairs)
    assert SR.MATRIX[:9] == tuple((r, 24) for r in SR.ROWS) and SR.MATRIX[9] == ("1111111", 17)
    # across the rows the ranks run every feature is on at least once, and all but spectra and open boundaries also off once
    for k, name in enumerate(SR.FEATURES):
        assert {r[k] for r in SR.RANK_ROWS} == ({"1"} if name in ("spectra", "open") else {"0", "1"}), name


# ---- conditions on the matrix inputs -----------------------------------------------------------------------------------------
def _scaled(c, opts, factor):
    return (dict(c, flux=c["flux"] * factor), dict(opts, faces=tuple((f, x * factor, s) for f, x, s in opts["faces"])))


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


@pytest.mark.parametrize("row,N", SR.MATRIX, ids=IDS)
def test_conditioning_and_decision_margin(row, N):
    """(a) every flux times 1 + 1e-11: xh_intermed and T_end answer with 1e-9 at most, niter stays.  (b) at every outer iteration
    the decision stays when conv_flag moves by +-2 and rel1, rel0 by +-1e-3 relative; at least 3 iterations."""
    c = SR.case_of(row, N)
    opts = SR.reference_options(row, c)
    r = SR.matrix_reference(row, N)
    c2, opts2 = _scaled(c, opts, 1.0 + 1e-11)
    r2 = SR.reference_step(c2, **opts2)
    dx = _rel(r2["xh_intermed"], r["xh_intermed"])
    dT = _rel(r2["T_end"], r["T_end"]) if "T_end" in r else 0.0
    print(f"{row} N={N}: response of xh {dx:.2e}, of T {dT:.2e}; niter {r['niter']}; conv_flag per iteration {[h[0] for h in r['history']]}; "
          f"last rel1 {r['history'][-1][1]:.2e} rel0 {r['history'][-1][2]:.2e}")
    assert r2["niter"] == r["niter"]
    assert dx <= 1e-9 and dT <= 1e-9
    assert (r2["phi_ion"] != 0).sum() == (r["phi_ion"] != 0).sum() > 0
    crit, cf = r["conv_criterion"], c["conv"]
    decide = lambda flag, rel1, rel0: (flag < crit) or (rel1 < cf and rel0 < cf)
    assert r["niter"] >= 3 and len(r["history"]) == r["niter"]
    for it, (flag, rel1, rel0) in enumerate(r["history"]):
        base = decide(flag, rel1, rel0)
        assert base == (it == r["niter"] - 1)
        for d, f1, f0 in itertools.product((-2, 0, 2), (1 - 1e-3, 1.0, 1 + 1e-3), (1 - 1e-3, 1.0, 1 + 1e-3)):
            assert decide(flag + d, rel1 * f1, rel0 * f0) == base, (it, flag, rel1, rel0, d, f1, f0)


@pytest.mark.parametrize("row,N", SR.MATRIX, ids=IDS)
def test_every_feature_of_the_row_matters(row, N):
    """(c) turning any one feature of the row off moves xh_intermed by more than 1e-3 somewhere; the budget, which moves nothing,
    has ions, photo-ionisations and recombinations to count, and LLS absorptions exactly when the row has LLS.  (d) open rows:
    sources on first and last planes, every spectrum with a source within R of a face, and rates that the periodic step has and
    the open one has not."""
    c = SR.case_of(row, N)
    on = SR.features_of(row)
    r = SR.matrix_reference(row, N)
    for k, name in enumerate(SR.FEATURES):
        if not on[name] or name == "budget":
            continue
        off = row[:k] + "0" + row[k + 1:]
        other = SR.reference_step(c, **SR.reference_options(off, c))
        moved = _rel(other["xh_intermed"], r["xh_intermed"])
        print(f"{row} N={N}: without {name} xh_intermed moves by {moved:.2e}")
        assert moved > 1e-3, name
        if name == "open":
            wrapped = (other["phi_ion"] != 0) & (r["phi_ion"] == 0) if not on["faces"] else other["phi_ion"] > r["phi_ion"] * (1 + 1e-6)
            assert wrapped.sum() > 100
    if on["thermal"]:
        assert r["T_end"].max() > 1.05e4 and r["phi_heat"].max() > 0
    if on["budget"]:
        s = r["budget_sums"]
        assert s[SR.BR.CELLS] == N ** 3 and s[SR.BR.DNX] > 0 and s[SR.BR.PHOTO] > 0 and s[SR.BR.REC] > 0
        assert (s[SR.BR.LLS] > 0) == on["lls"] and (on["lls"] or s[SR.BR.LLS] == 0)
    else:
        assert "budget_sums" not in r
    if on["open"]:
        pos0 = c["pos"].T - 1
        assert (pos0 == 0).any() and (pos0 == N - 1).any() and c["R"] < N / 2 - 1 and c["M"] >= N + c["R"]
        near = np.min(np.minimum(pos0, N - 1 - pos0), axis=1) < c["R"]
        spec = c["spectrum"] if on["spectra"] else np.zeros(len(near), dtype=int)
        for s in set(spec.tolist()):
            assert near[spec == s].any(), s
