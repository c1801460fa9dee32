"""CPU: the statement of the clumped chemistry (tests/clumping_reference.py) against the C oracle's and the reference Fortran's
doric with their clumping argument, and the host side of the clumping feature: argument checks that come before any GPU
work, the YAML key of the C2Ray class, the C-ABI symbol and grid selector."""
import os

import numpy as np
import pytest

import cases
import clumping_reference as CR

HERE = os.path.dirname(os.path.abspath(__file__))
BB_PARAMS = os.path.join(HERE, "data", "parameters_single_black_body.yml")
CHEM = (cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0)


def _random_doric_cells(seed, m=400):
    rng = np.random.default_rng(seed)
    return (10 ** rng.uniform(-5, -1e-3, m), 10 ** rng.uniform(9, 14, m), 10 ** rng.uniform(2, 5, m),
            10 ** rng.uniform(-5, 1, m), np.where(rng.random(m) < 0.2, 0.0, 10 ** rng.uniform(-18, -10, m)))


@pytest.mark.parametrize("clumping", [1.0, 2.0, 7.5, 30.0])
def test_doric_restatement_matches_the_c_oracle_bit_for_bit(clumping):
    from oracle import oracle
    for x0, dt, T, rhe, phi in zip(*_random_doric_cells(int(clumping * 10))):
        got = CR.doric(x0, dt, T, rhe, phi, *CHEM, clumping)
        want = oracle.doric(x0, dt, T, rhe, phi, *CHEM, clumping=clumping)
        assert got == want, (x0, dt, T, rhe, phi)


@pytest.mark.parametrize("clumping", [1.0, 2.0, 7.5, 30.0])
def test_doric_restatement_matches_the_reference_fortran(clumping):
    from oracle import ref_fortran
    if not ref_fortran.available():        # (built by build() where the reference tree exists, as test_oracle_vs_reference.py)
        pytest.skip("oracle/_ref/libc2ray_ref.so not built here")
    for x0, dt, T, rhe, phi in zip(*_random_doric_cells(int(clumping * 10) + 1)):
        got = CR.doric(x0, dt, T, rhe, phi, *CHEM, clumping)
        want = ref_fortran.doric(x0, dt, T, rhe, phi, *CHEM, clumping=clumping)
        np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)


def test_clumping_raises_the_recombination_rate_only():
    """Doubling C is doubling bh00 (doric's order: (C bh00) ...), bit for bit; and it lowers the equilibrium fraction."""
    for x0, dt, T, rhe, phi in zip(*_random_doric_cells(5, 100)):
        b = cases.BH00
        assert CR.doric(x0, dt, T, rhe, phi, b, *CHEM[1:], 2.0) == CR.doric(x0, dt, T, rhe, phi, 2.0 * b, *CHEM[1:], 1.0)
    x1 = CR.doric(0.5, 1e16, 1e4, 1e-3, 1e-12, *CHEM, 1.0)[0]
    x8 = CR.doric(0.5, 1e16, 1e4, 1e-3, 1e-12, *CHEM, 8.0)[0]
    assert x8 < x1


def test_vectorised_pass_agrees_with_the_cell_loop():
    """chemistry_pass (vectorised, grid form c x (bh00 ...)) against do_chemistry per cell (reference order) -- and with
    C = 1 against the oracle's do_chemistry."""
    from oracle import oracle
    c = cases.chem_case(6, 11)
    clump = np.exp(np.random.default_rng(2).normal(1.0, 0.8, (6, 6, 6))).clip(1.0, 50.0)
    args = (c["ndens"], c["temp"], c["xh"], c["xh_av"], c["phi_ion"], *CHEM, cases.ABU_C)
    xi, xa, _, _, delta = CR.chemistry_pass(c["dt"], *args, clump=clump, return_delta=True)
    xi1, xa1, _, _, delta1 = CR.chemistry_pass(c["dt"], *args, clump=1.0, return_delta=True)
    # (c (bh00 ...) against (c bh00) ..., numpy's vector exp / pow against libm: an ulp, amplified in the slow cells as
    # tests/test_gpu_thermal.py describes -- 1e-10 where delth dt > 1e-2, its looser bounds elsewhere)
    for idx in np.ndindex(6, 6, 6):
        cell = [a[idx] for a in args[:5]]
        for got, d, want in (((xi[idx], xa[idx]), delta[idx], CR.do_chemistry(c["dt"], *cell, *CHEM, cases.ABU_C, clump[idx])),
                             ((xi1[idx], xa1[idx]), delta1[idx], oracle.do_chemistry(c["dt"], *cell, *CHEM, cases.ABU_C))):
            rtol = (1e-10, 1e-10) if d > 1e-2 else (1e-7, 1e-3)
            assert got[0] == pytest.approx(want[0], rel=rtol[0]) and got[1] == pytest.approx(want[1], rel=rtol[1])


def test_clumping_keyword_limits_raise_before_any_gpu_work():
    import pyc2ray_amd as pc2r
    from pyc2ray_amd.evolve import _clumping_spec
    g = np.ones((4, 4, 4))
    bad = [0.0, -1.0, np.nan, np.inf, "3", True, np.ones((4, 4)), np.ones((3, 3, 3)), np.zeros((4, 4, 4)),
           np.full((4, 4, 4), np.nan), -np.ones((4, 4, 4)), np.ones((4, 4, 4), dtype=np.float32), [1.0, 2.0]]
    for c in bad:
        with pytest.raises(ValueError, match="clumping"):
            pc2r.evolve3D(1.0, 1.0, np.ones(1), np.ones((3, 1)), True, 10, 4, 0.01, g, g, g, np.ones(5), np.ones(5),
                          -20.0, 0.1, 4.0, 1e-4, 1e-18, 1.0, 1.0, 1.0, 1.0, 1.0, quiet=True, logfile=None, clumping=c)
        with pytest.raises(ValueError, match="clumping"):
            pc2r.evolve3D(1.0, 1.0, np.ones(1), np.ones((3, 1)), False, 10, 4, 0.01, g, g, g, np.ones(5), np.ones(5),
                          -20.0, 0.1, 4.0, 1e-4, 1e-18, 1.0, 1.0, 1.0, 1.0, 1.0, quiet=True, logfile=None, clumping=c)
        with pytest.raises(ValueError, match="clumping"):
            pc2r.evolve3D_MPI(1.0, 1.0, np.ones(1), np.ones((3, 1)), True, 10, 4, 0.01, None, None, 0, 2, g, g, g,
                              np.ones(5), np.ones(5), -20.0, 0.1, 4.0, 1e-4, 1e-18, 1.0, 1.0, 1.0, 1.0, 1.0, quiet=True,
                              logfile=None, clumping=c)
        with pytest.raises(ValueError, match="clumping"):
            pc2r.evolve3D_resident(1.0, 1.0, np.ones(1), np.ones((3, 1)), {8: c} if isinstance(c, np.ndarray) else {}, 4,
                                   np.ones(5), -20.0, 0.1, 4.0, 1e-4, 1e-18, 1.0, 1.0, 1.0, 1.0, 1.0, quiet=True,
                                   logfile=None, clumping=c)
    # off, constant, grid (either storage order)
    assert _clumping_spec(None, 4) is None and _clumping_spec(1.0, 4) is None and _clumping_spec(1, 4) is None
    assert _clumping_spec(np.float64(3.0), 4).constant == 3.0 and _clumping_spec(np.array(2.5), 4).constant == 2.5
    for order in "CF":
        grid = np.asarray(np.full((4, 4, 4), 2.0), order=order)
        assert _clumping_spec(grid, 4).grid is grid
    # the thermal refusals stay as they are, clumped or not
    from pyc2ray_amd.thermal import ThermalParams
    th = ThermalParams(np.zeros(5), np.zeros(5))
    with pytest.raises(ValueError, match="single-GPU"):
        pc2r.evolve3D_MPI(1.0, 1.0, np.ones(1), np.ones((3, 1)), True, 10, 4, 0.01, None, None, 0, 2, g, g, g, np.ones(5),
                          np.ones(5), -20.0, 0.1, 4.0, 1e-4, 1e-18, 1.0, 1.0, 1.0, 1.0, 1.0, quiet=True, logfile=None,
                          thermal=th, clumping=2.0)


def test_capi_grid_selector_and_symbol():
    from pyc2ray_amd import _capi
    assert _capi.GRID_CLUMP == 8
    assert "asora_clumping" in _capi.SIGNATURES
    header = open(os.path.join(os.path.dirname(HERE), "include", "asora_hip.h")).read()
    assert "ASORA_GRID_CLUMP = 8" in header and "ASORA_GRID_COUNT = 9" in header
    assert "int asora_clumping(int mode, double constant);" in header
    lib = _capi.load()                    # (opening the library resolves every declared symbol)
    assert hasattr(lib, "asora_clumping")


def _write_params(tmp_path, clumping=None):
    base = open(BB_PARAMS).read()
    if clumping is not None:
        base = base.replace("Material:\n", f"Material:\n  clumping: {clumping}\n")
    path = tmp_path / "parameters.yml"
    path.write_text(base)
    return str(path)


def test_yaml_clumping_key(tmp_path):
    import pyc2ray_amd as pc2r
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        sim = pc2r.C2Ray_Test(_write_params(tmp_path), 8, False)
        assert sim.clumping == 1.0                                    # absent: the reference's behaviour
        sim = pc2r.C2Ray_Test(_write_params(tmp_path, 4), 8, False)
        assert sim.clumping == 4.0 and isinstance(sim.clumping, float)
        for bad in ("0", "-2.0", "abc", ".nan"):
            with pytest.raises(ValueError, match="clumping"):
                pc2r.C2Ray_Test(_write_params(tmp_path, bad), 8, False)
        grid = np.full((8, 8, 8), 3.0)
        sim.clumping = grid
        assert sim.clumping is grid
        sim.clumping = None
        assert sim.clumping == 1.0
        for bad in (np.ones((4, 4, 4)), 0.0, np.full((8, 8, 8), -1.0)):
            with pytest.raises(ValueError, match="clumping"):
                sim.clumping = bad
    finally:
        os.chdir(cwd)
