"""CPU: the oracle's restatement of the ASORA (GPU-path) shell traversal against the golden
Fortran-path results.  With the Fortran constants selected (flags=0) the two traversals must
agree to summation-order rounding wherever ASORA writes (|d| <= R inside the periodic window);
with the CUDA constants (ASORA_MODE) the documented ~1e-7 differences appear
(sqrt literals 1.8e-8, thin-cell tau argument ~1e-7)."""
import os

import numpy as np
import pytest

import cases
from oracle import oracle as O

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _run(name, tables, flags, want_cd=False):
    c = cases.rt_case(name, tables)
    pos0, flux = cases.flat_sources(c["pos"], c["flux"])
    return c, O.asora_do_all_sources(c["R"], c["sig"], c["dr"], c["ndens"], c["xh"], pos0, flux,
                                     c["thin"], c["thick"], c["minlogtau"], c["dlogtau"],
                                     NumTau=c["thin"].shape[0] - 1, flags=flags, want_coldens=want_cd)


@pytest.mark.parametrize("name", list(cases.RT_CASES))
@pytest.mark.parametrize("tables", ["grey", "soft"])
def test_shell_traversal_equals_cubic_traversal(name, tables):
    g = np.load(os.path.join(G, "raytrace.npz"))
    c, r = _run(name, tables, flags=0, want_cd=True)
    ref = g[f"{name}__{tables}__phi"]
    np.testing.assert_allclose(r["phi_ion"], ref, rtol=1e-10, atol=0)
    # column density of the last source: compare where the shell traversal wrote
    cd_ref = g[f"{name}__{tables}__cd"]
    w = r["coldens"] != 0
    assert w.sum() > 0
    np.testing.assert_allclose(r["coldens"][w], cd_ref[w], rtol=1e-12)


@pytest.mark.parametrize("name", ["u16_1src_R8", "l16_7src_R5.5", "l32_5src_R10", "l16_thin"])
def test_cuda_constants_within_north_star_tolerance(name):
    g = np.load(os.path.join(G, "raytrace.npz"))
    c, r = _run(name, "soft", flags=O.ASORA_MODE)
    ref = g[f"{name}__soft__phi"]
    np.testing.assert_allclose(r["phi_ion"], ref, rtol=1e-5, atol=0)
    assert np.abs(r["phi_ion"] - ref).max() > 0      # the two modes are genuinely different


def test_visited_count_is_clipped_octahedron():
    # R=4 on 16^3: q_max = ceil(1.73205080757*4) = 7, no clipping: 1 + sum_{1<=q<=7}(4q^2+2)
    # (shell 0 is the single source cell, raytracing.cu:211)
    c, r = _run("u16_1src_R4", "grey", flags=O.ASORA_MODE)
    assert r["visited"] == 1 + sum(4 * q * q + 2 for q in range(1, 8))


# ---- heating on the ASORA path -------------------------------------------------------------------------------------
P2 = 2.0 ** -35          # ~20 eV per ionisation: heating tables = P2 x photo tables hold 1e28 ... 1e48 x 2^-35, far from subnormal


def _heat_tables(c, kind):
    """(thin, thick, heat_thin, heat_thick): kind "ramp" the sub-box cases' heating tables on the case's photo tables,
    "bb" the black-body photo and heating tables (make_photo_table / make_heat_table)."""
    if kind == "bb":
        thin, thick, hthin, hthick, _ = cases.blackbody_photo_and_heat_tables()
        return thin, thick, hthin, hthick
    n = c["thin"].shape[0]
    return c["thin"], c["thick"], 1e-11 * c["thin"] * np.linspace(1.0, 2.0, n), 0.7e-11 * c["thick"] * np.linspace(2.0, 1.0, n)


def _asora(c, thin, thick, hthin, hthick, flags):
    pos0, flux = cases.flat_sources(c["pos"], c["flux"])
    return O.asora_do_all_sources(c["R"], c["sig"], c["dr"], c["ndens"], c["xh"], pos0, flux, thin, thick, c["minlogtau"],
                                  c["dlogtau"], NumTau=thin.shape[0] - 1, flags=flags, heat_thin=hthin, heat_thick=hthick)


@pytest.mark.parametrize("name", list(cases.RT_CASES))
@pytest.mark.parametrize("tables", ["ramp", "bb"])
def test_shell_traversal_heating_equals_cubic_traversal(name, tables):
    """With the Fortran constants (flags=0) the ASORA-path heating equals the Fortran-path oracle's (raytracing.f90:532,537)
    wherever the shell traversal writes, to the tolerances of the photo rates above; and the photo rates of a call with
    heating tables are those of a call without."""
    c = cases.rt_case(name, "soft")
    thin, thick, hthin, hthick = _heat_tables(c, tables)
    r = _asora(c, thin, thick, hthin, hthick, 0)
    bare = _asora(c, thin, thick, None, None, 0)
    assert "phi_heat" not in bare
    assert np.array_equal(r["phi_ion"], bare["phi_ion"])
    N = c["N"]
    f = O.do_all_sources(c["flux"], c["pos"], 1000, N, c["sig"], c["dr"], c["ndens"], c["xh"], 1e-2, thin, thick,
                         c["minlogtau"], c["dlogtau"], c["R"], heat_thin=hthin, heat_thick=hthick, NumTau=thin.shape[0] - 1)
    w = r["phi_ion"] != 0
    assert w.sum() > 0
    # (where the shell traversal does not write, the cubic one may: |d| > R inside the periodic window holds zeros in both,
    #  so the whole grids are compared)
    np.testing.assert_allclose(r["phi_ion"], f["phi_ion"], rtol=1e-10, atol=0)
    np.testing.assert_allclose(r["phi_heat"], f["phi_heat"], rtol=1e-10, atol=0)
    assert np.array_equal(r["phi_heat"] != 0, w)


@pytest.mark.parametrize("name", list(cases.RT_CASES))
@pytest.mark.parametrize("tables", ["soft", "bb"])
@pytest.mark.parametrize("flags", [0, O.ASORA_MODE])
def test_heating_of_power_of_two_scaled_tables_is_the_scaled_photo_rate(name, tables, flags):
    """Heating tables = 2^-35 x photo tables.  The scaling commutes with every rounding of a heating rate (table differences,
    the interpolation, the prefactor products, the division by nHI), so where the oracle forms photo rate and heating rate
    alike -- thin cells, pref dtau T(tau) -- phi_heat == 2^-35 phi_ion bit for bit, with either thin-cell optical depth.
    Thick cells: the oracle keeps the reference's photo rate phi_in - phi_out = pref T(tau_in) - pref T(tau_out)
    (photorates.f90, rates.cu), but forms the heating as pref (H(tau_in) - H(tau_out)) (photorates.f90:118, and the
    kernels' form of both): the two differ by the rounding of the two products, measured at most 1.0e-12 relative over
    these cases (the difference of nearly equal table values).  (On the GPU both are pref (T_in - T_out): bit for bit
    everywhere, tests/test_gpu_heating.py.)"""
    if tables == "bb":
        thin, thick = cases.blackbody_photo_and_heat_tables()[:2]
    else:
        thin, thick, _ = cases.soft_tables()
    c = cases.rt_case(name, "soft")
    r = _asora(c, thin, thick, P2 * thin, P2 * thick, flags)
    phi, heat = r["phi_ion"], r["phi_heat"]
    assert phi.max() > 0
    thin_cells = _asora(c, thin, thick, P2 * thin, 0.0 * thick, flags)["phi_heat"] != 0      # only thin cells get heating here
    thick_cells = (phi != 0) & ~thin_cells
    assert np.array_equal(heat[~thick_cells], P2 * phi[~thick_cells])
    assert not np.signbit(heat).any()
    np.testing.assert_allclose(heat[thick_cells], P2 * phi[thick_cells], rtol=4e-12, atol=0)
    if name == "l16_thin":
        assert thin_cells.sum() == phi.size
    if name == "l16_thick":
        assert thick_cells.sum() == phi.size


def test_thin_heating_uses_the_photo_rates_optical_depth():
    """Thin cells: the heating lookup is at the photo rate's optical depth -- tau_out with the CUDA constants
    (THIN_TAU_OUT), tau_in otherwise.  On the optically thin case the two choices differ in the last digits, and the
    black-body heating table has a different slope from the photo table, so a mixed choice shows."""
    c = cases.rt_case("l16_thin", "soft")
    thin, thick, hthin, hthick = _heat_tables(c, "bb")
    modes = {f: _asora(c, thin, thick, hthin, hthick, f) for f in (O.ASORA_MODE, O.ASORA_MODE & ~O.THIN_TAU_OUT)}
    a, b = modes[O.ASORA_MODE], modes[O.ASORA_MODE & ~O.THIN_TAU_OUT]
    w = a["phi_ion"] != 0
    assert not np.array_equal(a["phi_heat"][w], b["phi_heat"][w])
    # the relative change of heating and photo rate from one optical depth to the other is the table's logarithmic slope
    # times the same d tau: both tiny, and different from each other (the tables are not proportional)
    dh = a["phi_heat"][w] / b["phi_heat"][w] - 1.0
    dp = a["phi_ion"][w] / b["phi_ion"][w] - 1.0
    assert np.abs(dh).max() < 1e-6 and np.abs(dp).max() < 1e-6
    assert not np.allclose(dh, dp, rtol=1e-3, atol=0)


def test_thermal_oracle_loop_without_heating_or_cooling_is_the_isothermal_loop():
    """evolve3D_thermal_oracle with the cooling mask 0 and zero heating tables keeps T = T_start, so it must take as many outer
    iterations as evolve3D_oracle and reach the same ionised fraction.  The two passes are different statements of doric
    (numpy here, C in the oracle; the same libm): x to 1e-9, which is far looser than what they show."""
    import evolve_oracle as EO
    import thermal_reference as TR
    for name in ("l16_gpu_F", "l32_gpu_F_5src"):
        c = cases.evolve_case(name)
        temp = np.full_like(c["temp"], 3e3) * (1.0 + 0.5 * np.random.default_rng(3).random(c["temp"].shape))
        args = (c["dt"], c["dr"], c["flux"], c["pos"], temp, c["ndens"], c["xh"])
        tail = (cases.MINLOGTAU, c["dlogtau"], c["R"], c["convergence_fraction"], cases.SIG, cases.BH00, cases.ALBPOW,
                cases.COLH0, cases.TEMPH0, cases.ABU_C)
        x_iso, phi_iso, n_iso, _ = EO.evolve3D_oracle(*args, c["thin"], c["thick"], *tail)
        z = np.zeros_like(c["thin"])
        x, T, phi, heat, n, hist = EO.evolve3D_thermal_oracle(TR.Params(cooling_mask=0), *args, c["thin"], c["thick"], z, z, *tail)
        assert n == n_iso and n >= 2, (name, n, n_iso)
        np.testing.assert_allclose(T, temp, rtol=1e-15, atol=0)          # (one substep: T = (c T) / c)
        assert not heat.any()
        np.testing.assert_allclose(x, x_iso, rtol=1e-9, atol=0)
        np.testing.assert_allclose(phi, phi_iso, rtol=1e-9, atol=0)
        assert x.max() > 10 * c["xh"].max()
