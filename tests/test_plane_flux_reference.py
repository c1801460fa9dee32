"""CPU: the numpy restatement of the plane-parallel flux (tests/plane_flux_reference.py) against the
oracle's photoion_rates, its photon conservation, the symmetry of the six faces, and a planar ionisation front against the
analytic solution.  Runs without a GPU; the GPU tests (tests/test_gpu_plane_flux.py) compare the kernel with this restatement."""
import functools

import numpy as np
import pytest

import cases
import plane_flux_reference as PF
from oracle import oracle as O

TAU_CELL = 0.1          # optical depth of a mean cell: every cell thick, and every ray of every face absorbs more than half the flux
FLUX = 2.5
SAMPLES = 2000


@functools.lru_cache(maxsize=None)
def _medium(N, checkerboard=False):
    nd, xh, dr = PF.checkerboard_medium(N) if checkerboard else cases.grid(N, "lognormal", 3, TAU_CELL)
    n_abs = nd * (1.0 - xh)
    n_abs.setflags(write=False)
    return n_abs, dr


def _tables(heat=False):
    thin, thick, dlog = cases.soft_tables()
    n = thin.shape[0]
    if heat:
        return thin, thick, dlog, 1e-11 * thin * np.linspace(1.0, 2.0, n), 0.7e-11 * thick * np.linspace(2.0, 1.0, n)
    return thin, thick, dlog, None, None


def _worst_against_oracle(N, face, checkerboard, heat, seed):
    """Worst relative difference between the restatement and the oracle's photoion_rates / n_abs over SAMPLES cells, the share of
    bit-equal samples and the share of thin cells among all cells."""
    n_abs, dr = _medium(N, checkerboard)
    thin, thick, dlog, ht, hk = _tables(heat)
    phi, h, d = PF.plane_trace(face, FLUX, n_abs, dr, cases.SIG, thin, thick, cases.MINLOGTAU, dlog, heat_thin=ht, heat_thick=hk,
                               details=True)
    phi_m, h_m = PF.to_march_order(phi, face), (PF.to_march_order(h, face) if heat else None)
    rng = np.random.default_rng(seed)
    picks = rng.choice(N ** 3, size=SAMPLES, replace=False)
    worst, equal = 0.0, 0
    for flat in picks:
        idx = np.unravel_index(flat, (N, N, N))
        a, _b, c = O.photoion_rates(FLUX, d["cd_in"][idx], d["cd_out"][idx], dr, cases.SIG, thin, thick, cases.MINLOGTAU, dlog,
                                    heat_thin=ht, heat_thick=hk, flags=O.ASORA_MODE)
        pairs = [(phi_m[idx], a / d["n_abs"][idx])] + ([(h_m[idx], c / d["n_abs"][idx])] if heat else [])
        for got, ref in pairs:
            assert ref > 0.0
            worst = max(worst, abs(got - ref) / ref)
            equal += got == ref
    return worst, equal / (SAMPLES * (2 if heat else 1)), 1.0 - d["thick"].mean()


@pytest.mark.parametrize("N", [24, 67])
def test_restatement_equals_the_oracles_rates(N):
    """Every face, 2000 sampled cells each, against oracle.photoion_rates(flux, cd_in, cd_out, dr, ...)[0] / n_abs to 1e-10.
    Measured: worst relative difference 6.1e-12 (N = 24 and 67, all six faces; 4.6e-12 at N = 24): numpy's log10 and libm's
    differ in the last place here and there, and the difference is multiplied by the table index (~1.7e4).  The bound is a factor
    of about 20 over that.  (About 9 % of the samples are bit-equal: the oracle forms prefact T(tau_in) - prefact T(tau_out), the
    restatement prefact (T(tau_in) - T(tau_out)) as the kernels do, which differ in the last place or two.)"""
    for f, face in enumerate(PF.FACES):
        worst, equal, thin_share = _worst_against_oracle(N, face, False, False, 100 + f)
        print(f"N={N} face {face}: worst {worst:.3e}, bit-equal {equal:.4f}, thin cells {thin_share:.3f}")
        assert thin_share == 0.0
        assert worst <= 1e-10


@pytest.mark.parametrize("N", [24, 67])
def test_thin_branch_and_heating(N):
    """The same on the checkerboard of 4^3 blocks with xh = 1 - 1e-7 (between 10 % and 90 % of the cells thin: a condition of the
    test), with the heating output; the cell size as PF.checkerboard_medium chooses it (and says why).  Measured: thin share 0.500 at both N,
    worst relative difference 9.6e-12 (N = 67, +y)."""
    for f, face in enumerate(("-x", "+y", "+z")):
        worst, equal, thin_share = _worst_against_oracle(N, face, True, True, 200 + f)
        print(f"N={N} face {face}: worst {worst:.3e}, bit-equal {equal:.4f}, thin cells {thin_share:.3f}")
        assert 0.1 <= thin_share <= 0.9
        assert worst <= 1e-10


@pytest.mark.parametrize("N", [24, 67])
def test_reference_conserves_photons(N):
    """Per ray, sum phi n_abs dr = flux (T_thick(0) - T_thick(tau_total)) on the all-thick medium, to 1e-13 relative (measured:
    1.5e-15 worst), and every ray of every face absorbs at least half of the flux (measured minimum: 0.59 at N = 24)."""
    n_abs, dr = _medium(N)
    thin, thick, dlog, _, _ = _tables()
    for face in PF.FACES:
        phi, _ = PF.plane_trace(face, FLUX, n_abs, dr, cases.SIG, thin, thick, cases.MINLOGTAU, dlog)
        absorbed = PF.absorbed_per_ray(phi, n_abs, dr, face)
        expected, share = PF.telescoped_per_ray(FLUX, n_abs, dr, cases.SIG, thick, cases.MINLOGTAU, dlog, face)
        worst = np.max(np.abs(absorbed - expected) / expected)
        print(f"N={N} face {face}: conservation {worst:.3e}, least absorbed share {share.min():.3f}")
        assert share.min() >= 0.5
        assert worst <= 1e-13


def test_faces_are_images_of_each_other():
    """The six faces under the matching transposes and flips of the input are bit-identical."""
    N = 24
    n_abs, dr = _medium(N)
    thin, thick, dlog, ht, hk = _tables(True)
    ref, ref_h = PF.plane_trace("-x", FLUX, n_abs, dr, cases.SIG, thin, thick, cases.MINLOGTAU, dlog, heat_thin=ht, heat_thick=hk)
    for face in PF.FACES[1:]:
        # the medium whose march order along `face` is the -x march order of n_abs
        moved = np.empty((N, N, N))
        PF.to_march_order(moved, face)[...] = n_abs
        phi, h = PF.plane_trace(face, FLUX, moved, dr, cases.SIG, thin, thick, cases.MINLOGTAU, dlog, heat_thin=ht, heat_thick=hk)
        assert np.array_equal(PF.to_march_order(phi, face), ref), face
        assert np.array_equal(PF.to_march_order(h, face), ref_h), face


def test_planar_ionisation_front_follows_the_analytic_solution():
    """A planar front in a uniform medium (N = 32, -x face, ten steps of a tenth of a recombination time, with recombination)
    against x_f(t) = (F / (alpha_B n^2)) (1 - exp(-alpha_B n t)), the front taken where x = 0.5.  Measured: the numerical front
    leads the analytic one by 0.05 cells after the first step, growing to 0.81 cells after the tenth (26.09 against 25.28
    cells; the analytic solution is that of a sharp front, which a front a few cells wide is not).  Asserted: within 1.81 cells at every step -- the measured value and one cell width."""
    c = PF.ifront_case()
    steps = PF.ifront_reference()
    worst = 0.0
    for s, (xh, _phi, niter) in enumerate(steps):
        assert np.array_equal(xh, np.broadcast_to(xh[:, :1, :1], xh.shape))         # planar: every ray the same
        got = PF.front_position_cells(xh[:, 0, 0])
        want = PF.ifront_analytic_cells(c, (s + 1) * c["dt"])
        print(f"step {s + 1}: front at {got:.3f} cells, analytic {want:.3f}, {niter} iterations")
        worst = max(worst, abs(got - want))
    assert steps[-1][0][:, 0, 0][20] > 0.9 and steps[-1][0][:, 0, 0][31] < 0.01    # the front is inside the box
    assert worst <= 1.81
