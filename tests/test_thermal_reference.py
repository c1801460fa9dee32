"""CPU: the statement of the thermal scheme (tests/thermal_reference.py) against physics it must obey, and the
parameter-file checks of the non-isothermal mode of C2Ray."""
import os

import numpy as np
import pytest

import thermal_reference as TR

HERE = os.path.dirname(os.path.abspath(__file__))
BB_PARAMS = os.path.join(HERE, "data", "parameters_single_black_body.yml")
BH00, ALBPOW, COLH0, TEMPH0, ABU_C = 2.59e-13, -0.7, 1.3e-8 * 0.83 * 1.0 / 13.598 ** 2, 13.598 / 8.617e-05, 7.1e-7


def test_compton_constant_from_codata():
    assert TR.COMPTON_C == pytest.approx(1.0178e-37, rel=2e-4)
    from pyc2ray_amd import thermal
    assert thermal.COMPTON_C == TR.COMPTON_C and thermal.K_B == TR.K_B


def test_heating_only_conserves_energy():
    """Cooling off: the thermal energy gained is exactly the heat deposited, sum 1.5 k_B n_p(x_av) (T_end - T_start) =
    dt sum n (1 - x_av) phi_heat, through the whole coupled pass."""
    rng = np.random.default_rng(3)
    M = 4000
    n = 10 ** rng.uniform(-4, 1, M)
    T = 10 ** rng.uniform(1, 3, M)
    xh = 10 ** rng.uniform(-4, -0.5, M)
    gamma = 10 ** rng.uniform(-15, -12, M)
    heat = gamma * 3e-11                      # ~20 eV per photo-ionisation
    dt = 3e12
    p = TR.Params(cooling_mask=0)
    xint, xav, T_end, nconv, stats = TR.chemistry_thermal(p, dt, n, T, xh, xh.copy(), gamma, heat, BH00, ALBPOW, COLH0,
                                                          TEMPH0, ABU_C)
    assert stats[0] == 0 and stats[1] == 0
    gained = np.sum(1.5 * TR.K_B * n * (1.0 + xav + ABU_C) * (T_end - T))
    deposited = dt * np.sum(n * (1.0 - xav) * heat)
    assert gained == pytest.approx(deposited, rel=1e-13)
    assert np.all(T_end > T)


def test_compton_cooling_follows_the_exponential_approach_to_the_cmb():
    """Ionised gas, Compton exchange only: dT/dt = -(T - T_g)/tau with tau = 1.5 k_B n_p / (C_C T_g^4 n_e)."""
    zred, tcmb0 = 10.0, 2.7255
    tg = tcmb0 * (1 + zred)
    n = np.array([1e-4, 1e-3, 1e-2])
    x = np.ones(3)
    T0 = np.array([1e4, 2e3, 5.0])                              # the last one is HEATED towards T_g
    n_e, n_p = n * (x + ABU_C), n * (1.0 + x + ABU_C)
    tau = 1.5 * TR.K_B * n_p / (TR.COMPTON_C * tg ** 4 * n_e)
    dt = 0.5 * tau[0]
    p = TR.Params(relative_denergy=1e-4, cooling_mask=16, compton=True, t_cmb=tg, max_substeps=10 ** 7)
    T_end, T_av, k, fl = TR.thermal(p, dt, ABU_C, COLH0, TEMPH0, n, x, np.zeros(3), T0)
    expect = tg + (T0 - tg) * np.exp(-dt / tau)
    np.testing.assert_allclose(T_end, expect, rtol=1e-3)
    assert not fl.any() and T_end[2] > T0[2]
    expect_av = tg + (T0 - tg) * tau / dt * (1.0 - np.exp(-dt / tau))
    np.testing.assert_allclose(T_av, expect_av, rtol=1e-3)


def test_max_substeps_caps_the_integration():
    p = TR.Params(max_substeps=7)
    n, x = np.array([1.0]), np.array([0.999])
    T_end, T_av, k, fl = TR.thermal(p, 3e13, ABU_C, COLH0, TEMPH0, n, x, np.zeros(1), np.array([1e5]))
    assert k[0] == 7 and T_end[0] >= p.t_floor


def _write_params(tmp_path, isothermal=None, heating=None):
    base = open(BB_PARAMS).read()
    if heating is not None:
        base = base.replace("compute_heating_rates: 0", f"compute_heating_rates: {heating}")
    if isothermal is not None:
        base = base.replace("Material:\n", f"Material:\n  isothermal: {isothermal}\n")
    path = tmp_path / "parameters.yml"
    path.write_text(base)
    return str(path)


class _FakeMPI:
    class COMM_WORLD:
        @staticmethod
        def Get_rank():
            return 0

        @staticmethod
        def Get_size():
            return 2


def test_yaml_without_the_key_is_isothermal(tmp_path):
    import pyc2ray_amd as pc2r
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        sim = pc2r.C2Ray_Test(_write_params(tmp_path), 8, False)
        assert sim.isothermal is True and sim._thermal_params() is None
    finally:
        os.chdir(cwd)


def test_yaml_non_isothermal_needs_heating_rates(tmp_path):
    import pyc2ray_amd as pc2r
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        with pytest.raises(ValueError, match="compute_heating_rates"):
            pc2r.C2Ray_Test(_write_params(tmp_path, isothermal="false"), 8, True)
    finally:
        os.chdir(cwd)


def test_yaml_non_isothermal_refuses_mpi(tmp_path):
    import pyc2ray_amd as pc2r
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        with pytest.raises(ValueError, match="single-GPU"):
            pc2r.C2Ray_Test(_write_params(tmp_path, isothermal="false", heating=1), 8, True, _FakeMPI)
        with pytest.raises(ValueError, match="use_gpu"):
            pc2r.C2Ray_Test(_write_params(tmp_path, isothermal="false", heating=1), 8, False)
    finally:
        os.chdir(cwd)


def test_thermal_keyword_limits_raise_before_any_gpu_work():
    import pyc2ray_amd as pc2r
    from pyc2ray_amd.thermal import ThermalParams
    th = ThermalParams(np.zeros(5), np.zeros(5))
    g = np.ones((4, 4, 4))
    with pytest.raises(ValueError, match="use_gpu=True"):
        pc2r.evolve3D(1.0, 1.0, np.ones(1), np.ones((3, 1)), False, 10, 4, 0.01, g, g, g, np.ones(5), np.ones(5),
                      -20.0, 0.1, 4.0, 1e-4, 1e-18, 1.0, 1.0, 1.0, 1.0, 1.0, quiet=True, logfile=None, thermal=th)
    with pytest.raises(ValueError, match="single-GPU"):
        pc2r.evolve3D_MPI(1.0, 1.0, np.ones(1), np.ones((3, 1)), True, 10, 4, 0.01, None, None, 0, 2, g, g, g, np.ones(5),
                          np.ones(5), -20.0, 0.1, 4.0, 1e-4, 1e-18, 1.0, 1.0, 1.0, 1.0, 1.0, quiet=True, logfile=None,
                          thermal=th)
    assert th.t_cmb == 0.0 and ThermalParams(None, None, zred=9.0, tcmb0=2.0).t_cmb == 20.0
