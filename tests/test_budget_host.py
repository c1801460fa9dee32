"""CPU: the host side of the step budget: the C-ABI symbol, StepBudget's arithmetic, the checks of the
``budget=`` keyword and of the class's ``photon_budget``, where the call sits in a step (on a stand-in for the library), the numpy
statement on itself, and the bound of the residual on the statement of the chemistry pass."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import budget_reference as BR
import budget_standin_backend as BS
import cases
import clumping_reference as CR
import lls_standin_backend as SB

HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_test.yml")
CHEM = (cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)
YEAR = 3.15576e7


def test_capi_symbol_and_header():
    from pyc2ray_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "asora_hip.h")).read()
    assert ("int asora_step_budget(double bh00, double albpow, double colh0, double temph0, double abu_c, int use_temp_end, "
            "int i_begin, int i_count, double *sums);") in header
    assert "ASORA_BUDGET_CELLS = 0" in header and "ASORA_BUDGET_NT = 11" in header and "ASORA_BUDGET_COUNT = 12" in header
    assert "asora_step_budget" in _capi.SIGNATURES
    assert (_capi.BUDGET_CELLS, _capi.BUDGET_DNX, _capi.BUDGET_NT, _capi.BUDGET_COUNT) == (0, 5, 11, 12)
    # the selectors the issue pins stay where they are
    assert (_capi.GRID_CLUMP, len(_capi.SIGNATURES["asora_step_budget"][1])) == (8, 9)
    assert "ASORA_GRID_COUNT = 9" in header and "ASORA_KERNEL_COUNT = 4" in header
    lib = _capi.load()                    # (opening the library resolves every declared symbol)
    sums = np.full(12, -1.0)
    if not lib.asora_device_ptr(_capi.GRID_NDENS):      # no device initialised in this process: refused as every entry is
        rc = lib.asora_step_budget(*[1.0] * 5, 0, 0, 0, sums.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc != 0 and b"step_budget" in lib.asora_last_error() and b"not initialised" in lib.asora_last_error()
    else:                                               # (the whole suite in one process, a device left open: the null pointer)
        assert lib.asora_step_budget(*[1.0] * 5, 0, 0, 0, None) == 3 and b"step_budget" in lib.asora_last_error()
    assert np.all(sums == -1.0)                                          # (a refused call writes nothing)


def _filled(scale=1.0, dt=2.0, dr=3.0, N=4, flux=(1.5, 0.5), faces=()):
    from pyc2ray_amd.budget import StepBudget
    #        CELLS  N     X     NX    NX0   DNX  PHOTO  LLS  REC  COL   T      NT
    sums = [64.0, 32.0, 16.0, 12.0, 4.0, 8.0, 5.0, 0.5, 1.25, 0.25, 6.4e5, 3.2e5]
    return StepBudget().fill(np.array(sums) * [1, 1, 1, 1, 1, scale, scale, scale, scale, scale, 1, 1], dt, dr, N, np.array(flux), faces), sums


def test_step_budget_arithmetic():
    from pyc2ray_amd.budget import SLOTS, StepBudget
    from pyc2ray_amd.planeflux import PlaneFlux
    assert SLOTS == BR.SLOTS and len(SLOTS) == 12
    empty = StepBudget()
    assert empty.steps == 0 and np.all(empty.sums == 0.0) and empty.emitted == 0.0 and empty.residual == 0.0
    b, sums = _filled()
    V, dt = 27.0, 2.0
    assert np.array_equal(b.sums, sums) and (b.dt, b.dr, b.N, b.steps) == (2.0, 3.0, 4, 1)
    assert b.emitted == 2.0 * 1e48 * dt
    assert b.mean_xh_volume == 16.0 / 64.0 and b.mean_xh_mass == 12.0 / 32.0 and b.mean_xh_mass_before == 4.0 / 32.0
    assert b.mean_temp == 6.4e5 / 64.0 and b.mean_temp_mass == 3.2e5 / 32.0
    assert b.new_ions == 8.0 * V and b.photoionisations == 5.0 * V * dt and b.lls_absorbed == 0.5 * V * dt
    assert b.recombinations == 1.25 * V * dt and b.collisional == 0.25 * V * dt
    assert b.absorbed == (5.0 + 0.5) * V * dt and b.escaped == b.emitted - b.absorbed
    assert b.residual == 8.0 * V - (5.0 + 0.25 - 1.25) * V * dt == 0.0
    # faces: flux x the area of the box's face, with and without point sources
    faces = (PlaneFlux("-x", 0.25), PlaneFlux("+z", 1.0))
    area = (4 * 3.0) ** 2
    assert _filled(faces=faces)[0].emitted == (2.0 + 1.25 * area) * 1e48 * dt
    assert _filled(flux=(), faces=faces[:1])[0].emitted == 0.25 * area * 1e48 * dt
    # sums of steps: the counts, dt and steps add up; the means are the later step's, the mass-weighted start the earlier one's
    c, _ = _filled(scale=3.0, dt=5.0)
    c.mean_xh_mass_before, c.mean_xh_mass = 0.375, 0.5
    t = b + c
    assert (t.steps, t.dt) == (2, 7.0) and t.emitted == b.emitted + c.emitted
    for name in ("new_ions", "photoionisations", "lls_absorbed", "recombinations", "collisional", "absorbed", "escaped"):
        assert getattr(t, name) == pytest.approx(getattr(b, name) + getattr(c, name), rel=1e-15)
    assert t.residual == pytest.approx(b.residual + c.residual, abs=1e-12 * t.new_ions)
    assert t.mean_xh_mass == 0.5 and t.mean_xh_mass_before == 4.0 / 32.0 and np.array_equal(t.sums, c.sums)
    assert b.steps == 1 and b.dt == 2.0 and c.steps == 1                      # (the operands are left as they were)
    for s in (empty + b, b + empty):
        assert s is not b and s.__dict__.keys() == b.__dict__.keys()
        assert all(np.array_equal(getattr(s, k), getattr(b, k)) for k in b.__dict__)
    with pytest.raises(TypeError):
        b + 1.0
    line = b.log_line()
    assert line.startswith("Photon budget: emitted 4.0000e+48") and "<x>_mass 3.750000e-01" in line and "\n" not in line


def _evolve_args(N=4, nsrc=1):
    g = np.ones((N, N, N))
    return (1.0, 1.0, np.ones(nsrc), np.ones((3, nsrc)), True, 10, N, 0.01, g, g, g, np.ones(5), np.ones(5), -20.0, 0.1, 4.0, 1e-4, 1e-18,
            1.0, 1.0, 1.0, 1.0, 1.0)


def test_bad_budget_is_refused_before_the_library_is_touched(monkeypatch):
    import pyc2ray_amd as pc2r
    from pyc2ray_amd.budget import StepBudget
    SB.install(monkeypatch, SB.Untouchable())
    a = _evolve_args()
    for bad in (True, 1.0, "yes", {}, StepBudget, np.zeros(12)):
        with pytest.raises(ValueError, match="budget must be None or a pyc2ray_amd.budget.StepBudget"):
            pc2r.evolve3D(*a, quiet=True, logfile=None, budget=bad)
        with pytest.raises(ValueError, match="budget must be None"):
            pc2r.evolve3D_MPI(*a[:8], None, None, 0, 2, *a[8:], quiet=True, logfile=None, budget=bad)
        with pytest.raises(ValueError, match="budget must be None"):
            pc2r.evolve3D_resident(a[0], a[1], a[2], a[3], {}, 4, np.ones(5), *a[13:], quiet=True, logfile=None, budget=bad)
    with pytest.raises(ValueError, match="budget needs use_gpu=True"):
        pc2r.evolve3D(*a[:4], False, *a[5:], quiet=True, logfile=None, budget=StepBudget())
    with pytest.raises(ValueError, match="budget needs use_gpu=True"):
        pc2r.evolve3D_MPI(*a[:4], False, *a[5:8], None, None, 0, 2, *a[8:], quiet=True, logfile=None, budget=StepBudget())


@pytest.mark.parametrize("entry", ["evolve3D", "evolve3D_resident"])
def test_the_call_sits_behind_the_loop_and_ahead_of_the_results(monkeypatch, tmp_path, entry):
    """One call per step, after convergence, before XH is overwritten and before anything is fetched; without the keyword the
    library never hears of it and the step is call for call what it is with it."""
    import pyc2ray_amd as pc2r
    from pyc2ray_amd import _capi
    from pyc2ray_amd.budget import StepBudget
    from pyc2ray_amd.planeflux import PlaneFlux
    a = _evolve_args(nsrc=2)

    def run(**kw):
        lib = SB.install(monkeypatch, BS.Converging())
        kw.update(quiet=True, logfile=str(tmp_path / "log"))
        if entry == "evolve3D":
            pc2r.evolve3D(*a, **kw)
        else:
            pc2r.evolve3D_resident(a[0], a[1], a[2], a[3], {0: a[9], 3: a[8], 4: a[10]}, 4, np.ones(5), *a[13:], **kw)
        return lib

    off = run()
    assert "step_budget" not in off.names() and run(budget=None).names() == off.names()
    b = StepBudget()
    on = run(budget=b, plane_flux=PlaneFlux("-x", 0.5))
    names = on.names()
    assert names.count("step_budget") == 1
    at = names.index("step_budget")
    assert max(i for i, n in enumerate(names) if n == "evolve_poll") < at
    assert [n for n in names if n not in ("step_budget", "plane_flux")] == off.names()
    call = on.calls[at]
    assert call[1] == ((1.0, 1.0, 1.0, 1.0, 1.0, 1.0),) and call[2] == dict(use_temp_end=False, planes=None)
    assert np.array_equal(b.sums, BS.SUMS) and (b.dt, b.dr, b.N, b.steps) == (1.0, 1.0, 4, 1)
    assert b.emitted == (2.0 + 0.5 * 16.0) * 1e48
    if entry == "evolve3D_resident":           # XH <- XH_INTERMED comes after the budget has read both
        assert names.index("grid_copy") > at and on.calls[names.index("grid_copy")][1] == (_capi.GRID_XH, _capi.GRID_XH_INTERMED)
    else:
        assert "grid_to_host" not in names[:at] and names[at + 1:].count("grid_to_host") == 2


def test_yaml_key_and_the_attribute(tmp_path, monkeypatch):
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.c2ray_base as B
    from pyc2ray_amd.budget import StepBudget
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        plain = pc2r.C2Ray_Test(PLAIN_PARAMS, 8, False)
        assert plain.photon_budget is False and plain.last_budget is None and plain.total_budget.steps == 0
        with pytest.raises(ValueError, match="C2Ray.photon_budget: photon_budget needs use_gpu=True"):
            plain.photon_budget = True
        plain.photon_budget = False
        for bad in (1, 0, None, "on", 1.0):
            with pytest.raises(ValueError, match="photon_budget must be a bool"):
                plain.photon_budget = bad
        body = open(PLAIN_PARAMS).read()
        key = lambda v: body.replace("  logfile: pyC2Ray.log\n", f"  logfile: pyC2Ray.log\n  photon_budget: {v}\n")
        assert key(1) != body
        for v, what in ((2, "Output: photon_budget must be 0 or 1"), ("'yes'", "must be 0 or 1"), (1.0, "must be 0 or 1"),
                        (1, "Output: photon_budget: 1: photon_budget needs use_gpu=True")):
            with open("p.yml", "w") as f:
                f.write(key(v))
            with pytest.raises(ValueError, match=what):
                pc2r.C2Ray_Test("p.yml", 8, False)
        with open("p.yml", "w") as f:
            f.write(key(0))
        assert pc2r.C2Ray_Test("p.yml", 8, False).photon_budget is False
        # an object with use_gpu (as one constructed with use_gpu=True has it) reading the key
        with open("p.yml", "w") as f:
            f.write(key(1))
        sim = pc2r.C2Ray_Test(PLAIN_PARAMS, 8, False)
        sim.gpu = True
        sim._read_paramfile("p.yml")
        sim._statistic_init("photon_budget")
        assert sim.photon_budget is True
        # the class hands a fresh StepBudget to the entry, keeps it, adds it up and logs one line per step; off: no keyword at all
        seen = []

        def spy(name, result):
            def f(*args, **kw):
                seen.append((name, kw.get("budget", "absent")))
                if isinstance(kw.get("budget"), StepBudget):
                    kw["budget"].fill(np.arange(1.0, 13.0), args[0], args[1], 8, args[2])
                return result
            return f
        N = 8
        monkeypatch.setattr(B, "evolve3D", spy("evolve3D", (np.zeros((N, N, N)), np.zeros((N, N, N)))))
        monkeypatch.setattr(B, "evolve3D_resident", spy("evolve3D_resident", 1))
        flux, pos = np.ones(1), np.ones((3, 1), dtype=int)
        sim.device_resident = False
        sim.evolve3D(2.0, flux, pos)
        first = sim.last_budget
        sim.device_resident = True
        sim.evolve3D(3.0, flux, pos)
        assert [s[0] for s in seen] == ["evolve3D", "evolve3D_resident"] and seen[0][1] is first and seen[1][1] is sim.last_budget
        assert first is not sim.last_budget and (first.dt, sim.last_budget.dt) == (2.0, 3.0)
        assert sim.total_budget.steps == 2 and sim.total_budget.dt == 5.0
        assert sim.total_budget.emitted == first.emitted + sim.last_budget.emitted == pytest.approx(5e48, rel=1e-15)
        assert sim._device_newer >= {"xh", "phi_ion"}
        assert open(sim.logfile).read().count("Photon budget: emitted") == 2
        sim.photon_budget = False
        sim.evolve3D(1.0, flux, pos)
        assert seen[-1] == ("evolve3D_resident", "absent") and sim.total_budget.steps == 2
        assert open(sim.logfile).read().count("Photon budget: emitted") == 2
    finally:
        os.chdir(cwd)
        if "sim" in locals():      # (nothing of this object lives on a device: a later step elsewhere must not ask it to fetch)
            sim._device_newer.clear()
            sim.device_resident = False


def _cpu_case(N, seed, dt, uniform_T):
    from test_gpu_clumping import _cells, _clump_grid
    n, T, x0, xav_in, gamma = _cells(N, seed, uniform_T=uniform_T)
    clump = _clump_grid(N, seed + 1)
    x1, xav, _, _ = CR.chemistry_pass(dt, n, T, x0, xav_in, gamma, *CHEM, clump=clump)
    return n, T, x0, x1, xav, gamma, clump


def test_reference_on_itself_disjoint_ranges_add_up():
    N = 9
    n, T, x0, x1, xav, gamma, clump = _cpu_case(N, 11, 1e5 * YEAR, False)
    args = (n, x0, x1, xav, gamma, T, CHEM)
    kw = dict(clump=clump, lls=(1e-3, 0.05), temp_end=1.5 * T)
    whole, mag = BR.sums(*args, **kw)
    assert whole[BR.CELLS] == N ** 3 and np.all(mag >= np.abs(whole)) and whole[BR.LLS] > 0.0
    assert whole[BR.T_] == pytest.approx(1.25 * math.fsum(T.ravel()), rel=1e-14)
    a, _ = BR.sums(*args, planes=(0, 4), **kw)
    b, _ = BR.sums(*args, planes=(4, 5), **kw)
    assert np.all(np.abs(a + b - whole) <= 4e-16 * mag)
    assert np.array_equal(BR.sums(*args, planes=(3, 0), **kw)[0], np.zeros(12))
    keep = x1 > 0.01
    k, _ = BR.sums(*args, keep=keep, **kw)
    assert k[BR.CELLS] == keep.sum() and k[BR.N_] == pytest.approx(n[keep].sum(), rel=1e-13)
    # DNX is formed per cell: the same number as NX - NX0 to the rounding of the two big sums
    assert whole[BR.DNX] == pytest.approx(whole[BR.NX] - whole[BR.NX0], abs=4e-16 * (mag[BR.NX] + mag[BR.NX0]))


def test_residual_bound_on_the_chemistry_pass():
    """doric's solution obeys x1 - x0 = dt [(Gamma + de acolh0)(1 - xav) - de brech0 xav] with `de` of the PREVIOUS inner
    iteration; the budget evaluates it at the final xav, and the exit test |d xav| < 1e-3 (1 - xav) bounds the difference.  N = 24,
    dt = 1e5 yr, T = 1e4 K, a log-normal clumping grid: no cell is clamped to 1e-14, every cell left by the exit test."""
    N, dt = 24, 1e5 * YEAR
    n, T, x0, x1, xav, gamma, clump = _cpu_case(N, 7, dt, True)
    assert x1.min() > BR.EPS and xav.min() > BR.EPS and (1.0 - xav).min() >= 1e-8
    s, mag = BR.sums(n, x0, x1, xav, gamma, T, CHEM, clump=clump)
    res, bound = BR.residual(s, dt), BR.residual_bound(n, xav, T, dt, CHEM, clump=clump)
    print(f"residual / bound = {res / bound:.3f} (residual {res:.3e}, bound {bound:.3e})")
    assert bound > 0.0 and abs(res) <= 1.0 * bound
    # ... and the bound is not idle: the rounding of the sums lies orders below it
    assert 1e-13 * (mag[BR.DNX] + dt * (mag[BR.PHOTO] + mag[BR.COL] + mag[BR.REC])) < 1e-3 * bound
