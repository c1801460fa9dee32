"""CPU: the host side of the Lyman-limit-system opacity: LLSOpacity and its checks, the mean free path,
the YAML keys and lambda(z), the numpy statement of the absorber density, the C-ABI symbols, and -- on a stand-in for the library
-- that bad input is refused before the library is touched, that the state is set after the uploads and reset whatever happens."""
import os

import numpy as np
import pytest

import cases
import lls_reference as LR
import lls_standin_backend as SB

HERE = os.path.dirname(os.path.abspath(__file__))
LLS_PARAMS = os.path.join(HERE, "data", "parameters_lls.yml")
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_test.yml")


def test_lls_opacity_validation():
    from pyc2ray_amd.lls import LLSOpacity, lls_spec
    o = LLSOpacity()
    assert (o.n_const, o.per_density, o.on) == (0.0, 0.0, False)
    o = LLSOpacity(n_const=2e-6, per_density=np.float64(0.25))
    assert (o.n_const, o.per_density, o.on) == (2e-6, 0.25, True) and o == LLSOpacity(2e-6, 0.25)
    assert LLSOpacity(per_density=1).on and LLSOpacity(1e-9).on
    for bad in (-1e-9, float("nan"), float("inf"), -float("inf"), "1", None, True, [1.0]):
        with pytest.raises(ValueError, match="LLSOpacity"):
            LLSOpacity(n_const=bad)
        with pytest.raises(ValueError, match="LLSOpacity"):
            LLSOpacity(per_density=bad)
    assert lls_spec(None, "t") is None and lls_spec(LLSOpacity(), "t") is None          # both zero: off
    assert lls_spec(o, "t") == o
    for bad in (1.0, (1.0, 0.0), "on", {"n_const": 1.0}):
        with pytest.raises(ValueError, match="lls"):
            lls_spec(bad, "t")
    o.n_const = -1.0                                                                     # (assigned behind the constructor)
    with pytest.raises(ValueError, match="LLSOpacity"):
        lls_spec(o, "t")


def test_from_mean_free_path():
    from pyc2ray_amd.lls import LLSOpacity
    for mfp, sig in ((3.086e24, 6.30e-18), (1.5e23, 6.30e-18), (7.0e25, 1.0e-17)):
        o = LLSOpacity.from_mean_free_path(mfp, sig)
        assert o.n_const == 1.0 / (sig * mfp) and o.per_density == 0.0
        assert sig * o.n_const * mfp == pytest.approx(1.0, rel=1e-15)                    # one optical depth per mean free path
    assert LLSOpacity.from_mean_free_path(1e24, 6.3e-18, per_density=0.5).per_density == 0.5
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="mean_free_path"):
            LLSOpacity.from_mean_free_path(bad, 6.3e-18)
        with pytest.raises(ValueError, match="mean_free_path"):
            LLSOpacity.from_mean_free_path(1e24, bad)


def test_n_abs_with_zeros_is_nhi_bit_for_bit():
    rng = np.random.default_rng(3)
    n = 10 ** rng.uniform(-8, 2, 5000)
    x = np.concatenate([rng.uniform(0, 1, 4000), 1.0 - 10 ** rng.uniform(-16, -1, 990), np.zeros(5), np.ones(5)])
    got = LR.n_abs(n, x, 0.0, 0.0)
    assert np.array_equal(got, n * (1.0 - x)) and not np.signbit(got).any()
    # and with absorbers: every cell has some, the fully ionised ones included; more of either constant, more absorbers
    a, b = 3e-7, 0.02
    full = LR.n_abs(n, x, a, b)
    assert np.all(full > got) and np.all(full[-5:] == n[-5:] * b + a)
    assert np.all(LR.n_abs(n, x, 2 * a, b) > full) and np.all(LR.n_abs(n, x, a, 2 * b) > full)


def test_substituted_oracle_loop_with_zeros_is_the_oracle_loop():
    """evolve3D_lls_oracle(a = b = 0) is tests/evolve_oracle.py's loop bit for bit; with absorbers the fronts are slower."""
    from evolve_oracle import evolve3D_oracle
    N = 12
    nd, xh, dr = cases.grid(N, "lognormal", 61, 0.2, xlo=1e-4, xhi=2e-3)
    pos, flux = cases.sources(N, 3, 62, flux=6e-5)
    thin, thick, dlog = cases.soft_tables()
    args = (2 * cases.MYR, dr, flux, pos, np.full((N, N, N), 1e4), nd, xh, thin, thick, cases.MINLOGTAU, dlog, 5.5, 1e-4, cases.SIG,
            cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)
    x0, phi0, n0, _ = evolve3D_oracle(*args)
    x1, phi1, n1, _ = LR.evolve3D_lls_oracle(0.0, 0.0, *args)
    assert n0 == n1 and np.array_equal(x0, x1) and np.array_equal(phi0, phi1)
    x2, phi2, _, _ = LR.evolve3D_lls_oracle(0.05 / (cases.SIG * dr), 0.2, *args)
    assert np.isfinite(phi2).all() and x2.mean() < x0.mean()


def _photo(text):
    import yaml
    return yaml.safe_load(text)["Photo"]


def test_yaml_keys_and_mean_free_path_at_two_redshifts():
    from pyc2ray_amd.lls import MPC_CM, LLSOpacity, LLSSchedule
    sig = 6.30e-18
    assert LLSSchedule.from_photo_keys(_photo("Photo:\n  R_max_cMpc: 15.0\n"), sig, 9.0) is None      # no key: nothing changes
    s = LLSSchedule.from_photo_keys(_photo("Photo:\n  LLS_mfp_pMpc: 8.0\n  LLS_mfp_zref: 6.0\n  LLS_mfp_index: 4.4\n"
                                           "  LLS_per_density: 0.02\n"), sig, 9.0)
    assert (s.mfp_pMpc, s.zref, s.index, s.per_density) == (8.0, 6.0, 4.4, 0.02)
    assert s.mfp_cm(6.0) == 8.0 * MPC_CM
    assert s.mfp_cm(9.0) == pytest.approx(8.0 * MPC_CM * (10.0 / 7.0) ** -4.4, rel=1e-15)
    assert s.at(6.0) == LLSOpacity(1.0 / (sig * 8.0 * MPC_CM), 0.02)
    assert s.at(9.0).n_const == pytest.approx(s.at(6.0).n_const * (10.0 / 7.0) ** 4.4, rel=1e-14)
    # defaults: the reference redshift is the run's starting redshift, beta = 0 (the same at every redshift), b = 0
    s = LLSSchedule.from_photo_keys(_photo("Photo:\n  LLS_mfp_pMpc: 2.5\n"), sig, 9.0)
    assert (s.zref, s.index, s.per_density) == (9.0, 0.0, 0.0) and s.at(9.0) == s.at(5.0) == LLSOpacity.from_mean_free_path(2.5 * MPC_CM, sig)
    s = LLSSchedule.from_photo_keys(_photo("Photo:\n  LLS_per_density: 0.3\n"), sig, 9.0)
    assert s.mfp_cm(7.0) is None and s.at(7.0) == LLSOpacity(0.0, 0.3)
    for bad in ("LLS_mfp_pMpc: 0", "LLS_mfp_pMpc: -2", "LLS_mfp_pMpc: abc", "LLS_per_density: -0.1", "LLS_mfp_index: .nan",
                "LLS_mfp_zref: -1.5", "LLS_mfp_pMpc: true"):
        with pytest.raises(ValueError, match="LLS"):
            LLSSchedule.from_photo_keys(_photo(f"Photo:\n  {bad}\n"), sig, 9.0)


def test_c2ray_class_reads_the_keys_and_follows_the_redshift(tmp_path):
    import pyc2ray_amd as pc2r
    from pyc2ray_amd.lls import MPC_CM, LLSOpacity
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        plain = pc2r.C2Ray_Test(PLAIN_PARAMS, 8, False)
        assert plain.lls is None and plain.lls_schedule is None
        log_plain = open(plain.logfile).read()
        assert "LLS opacity" not in log_plain
        sim = pc2r.C2Ray_Test(LLS_PARAMS, 8, False)
        assert sim.cosmological and sim.zred_0 == 9.0
        a0 = 1.0 / (sim.sig * 0.135 * MPC_CM)
        assert sim.lls == LLSOpacity(a0, 0.01)
        assert "LLS opacity at z = 9.000" in open(sim.logfile).read()
        zs = sim.generate_redshift_array(2, 4e7)
        dt = sim.set_timestep(zs[0], zs[1], 2)
        sim.density_init(zs[0])
        sim.cosmo_evolve(dt)                                   # z falls: the proper mean free path grows, `a` falls
        assert sim.zred < 9.0
        assert sim.lls.n_const == pytest.approx(a0 * ((1 + sim.zred) / 10.0) ** 4.4, rel=1e-14) and sim.lls.n_const < a0
        assert sim.lls.per_density == 0.01
        # assignable between steps; what evolve3D would refuse is refused at the assignment
        sim.lls = LLSOpacity(5e-7)
        assert sim.lls == LLSOpacity(5e-7)
        sim.lls = None
        assert sim.lls is None
        for bad in (1.0, "x"):
            with pytest.raises(ValueError, match="lls"):
                sim.lls = bad
        sim.cosmo_evolve(dt)                                   # (the schedule takes over again ...)
        assert sim.lls is not None
        sim.lls_schedule = None                                # (... unless it is switched off)
        sim.lls = LLSOpacity(5e-7)
        sim.cosmo_evolve(dt)
        assert sim.lls == LLSOpacity(5e-7)
    finally:
        os.chdir(cwd)


def _evolve_args(N=4):
    g = np.ones((N, N, N))
    return (1.0, 1.0, np.ones(1), np.ones((3, 1)), True, 10, N, 0.01, g, g, g, np.ones(5), np.ones(5), -20.0, 0.1, 4.0, 1e-4, 1e-18,
            1.0, 1.0, 1.0, 1.0, 1.0)


def test_bad_lls_is_refused_before_the_library_is_touched(monkeypatch):
    import pyc2ray_amd as pc2r
    from pyc2ray_amd.lls import LLSOpacity
    SB.install(monkeypatch, SB.Untouchable())
    a = _evolve_args()
    broken = LLSOpacity(1e-6)
    broken.per_density = float("nan")
    for bad in (1e-6, (1e-6, 0.0), "on", broken):
        for use_gpu in (True, False):
            with pytest.raises(ValueError, match="(?i)lls"):
                pc2r.evolve3D(*a[:4], use_gpu, *a[5:], quiet=True, logfile=None, lls=bad)
        with pytest.raises(ValueError, match="(?i)lls"):
            pc2r.evolve3D_MPI(*a[:8], None, None, 0, 2, *a[8:], quiet=True, logfile=None, lls=bad)
        with pytest.raises(ValueError, match="(?i)lls"):
            pc2r.evolve3D_resident(a[0], a[1], a[2], a[3], {}, 4, np.ones(5), *a[13:], quiet=True, logfile=None, lls=bad)
        with pytest.raises(ValueError, match="(?i)lls"):
            pc2r.do_raytracing(a[1], a[2], a[3], True, 10, 4, 0.01, a[9], a[10], a[11], a[12], None, None, -20.0, 0.1, 4.0, 1e-18,
                               quiet=True, logfile=None, lls=bad)
    for bad in (-1.0, float("inf")):
        with pytest.raises(ValueError, match="LLSOpacity"):
            pc2r.evolve3D(*a, quiet=True, logfile=None, lls=LLSOpacity(bad))


@pytest.mark.parametrize("entry", ["evolve3D", "evolve3D_cpu", "evolve3D_resident", "do_raytracing"])
def test_state_is_set_after_the_uploads_and_reset_whatever_happens(monkeypatch, tmp_path, entry):
    import pyc2ray_amd as pc2r
    from pyc2ray_amd.lls import LLSOpacity
    a = _evolve_args()

    def run(lls, log):
        lib = SB.install(monkeypatch, SB.Recorder())
        kw = dict(quiet=True, logfile=str(log))
        if lls is not False:
            kw["lls"] = lls
        with pytest.raises(SB.Stop):
            if entry == "evolve3D":
                pc2r.evolve3D(*a, **kw)
            elif entry == "evolve3D_cpu":
                pc2r.evolve3D(*a[:4], False, *a[5:], **kw)
            elif entry == "evolve3D_resident":
                pc2r.evolve3D_resident(a[0], a[1], a[2], a[3], {0: a[9], 3: a[8], 4: a[10]}, 4, np.ones(5), *a[13:], **kw)
            else:
                pc2r.do_raytracing(a[1], a[2], a[3], True, 10, 4, 0.01, a[9], a[10], a[11], a[12], None, None, -20.0, 0.1, 4.0,
                                   1e-18, **kw)
        return lib, open(log).read()

    lib, text = run(LLSOpacity(2e-6, 0.5), tmp_path / "on.log")
    names = lib.names()
    sets = [c for c in lib.calls if c[0] == "lls_opacity"]
    assert [c[1] for c in sets] == [(2e-6, 0.5), (0.0, 0.0)]                 # set once, reset in the finally
    first = names.index("lls_opacity")
    assert max(i for i, n in enumerate(names) if n == "grid_to_device") < first          # after the uploads
    assert first < next(i for i, n in enumerate(names) if n in ("evolve_begin", "raytrace_device", "subbox_raytrace_device"))
    assert names[-1] == "lls_opacity"
    assert text.count("LLS opacity: n_const 2.000e-06 cm^-3, per_density 5.000e-01") == 1
    # off (no keyword, None, both zero): the library never hears of it and the log is the log without the feature
    logs = []
    for k, off in enumerate((False, None, LLSOpacity())):
        lib, text_off = run(off, tmp_path / f"off{k}.log")
        assert "lls_opacity" not in lib.names() and "LLS" not in text_off
        logs.append(text_off)
    assert logs[0] == logs[1] == logs[2]
    assert text.replace("LLS opacity: n_const 2.000e-06 cm^-3, per_density 5.000e-01\n", "") == logs[0]


def test_capi_symbols_and_header():
    from pyc2ray_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "asora_hip.h")).read()
    assert "int asora_lls_opacity(double n_const, double per_density);" in header
    assert "int asora_get_lls_opacity(double *n_const, double *per_density);" in header
    assert {"asora_lls_opacity", "asora_get_lls_opacity"} <= set(_capi.SIGNATURES)
    lib = _capi.load()                    # (opening the library resolves every declared symbol)
    # the state exists without a device: (0, 0) is accepted and read back, bad values are code 3, values > 0 want a device
    assert lib.asora_lls_opacity(0.0, 0.0) == 0
    import ctypes as C
    a, b = C.c_double(1.0), C.c_double(1.0)
    assert lib.asora_get_lls_opacity(C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0.0, 0.0)
    for bad in ((-1.0, 0.0), (0.0, -1e-300), (float("nan"), 0.0), (0.0, float("inf"))):
        assert lib.asora_lls_opacity(*bad) == 3
