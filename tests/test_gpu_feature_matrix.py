"""GPU: whole steps with several opt-in keywords on at once -- thermal=, clumping=, src_spectrum=, lls=, periodic=False,
plane_flux=, budget= -- against ONE composed CPU reference (tests/step_reference.py: reference_step, anchored bit for bit to
the single-feature restatements and conditioned in tests/test_step_reference_host.py).

The rows are the eight of a two-level orthogonal array of strength 2 over the seven keywords (every pair of them occurs on/on,
on/off, off/on and off/off) plus the all-on row, at N = 24 (R = 6, 2 Myr, four sources on first and last planes, two table sets,
two faces); the all-on row once more at N = 17, whose odd cell count exercises the scalar tail of the chemistry pass and the head
and tail of the budget kernel.  Three entry forms: evolve3D on host grids, two consecutive evolve3D_resident steps on one device
state, and evolve3D_MPI on two gloo ranks sharing GPU 0, on both device loops.

Tolerances: the project's own for single-feature steps (tests/test_gpu_plane_flux.py: _assert_step, and the thermal step
tests): xh and T to 1e-8, phi_ion and phi_heat to 1e-7, all relative with atol 0, equal iteration counts, and phi != 0 in the
reference's pattern; ranks identical bits and 1e-10 against one GPU; the budget to tests/test_gpu_budget.TOL of the statement on
the device's own grids and to 1e-7 of the scale against the composed reference's sums (they are linear in the grids), `emitted`
exact.  No tolerance is widened for a row: a row that misses one while the host file's conditions hold is a finding.

Measured on the MI355X over all cases (the table per case: LABNOTES.md, "Feature-combination matrix"): xh and phi_ion 2e-13 ...
6e-12, T 2e-14 ... 2e-13, phi_heat up to 2e-11; in the second resident step phi_ion up to 9e-10; the budget 6e-16 ... 1e-13 of the
scale from the reference's and 2e-16 from the statement on the device's grids; two ranks against one GPU 0 ... 6e-13."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import _matrix_dist_worker as W
import budget_reference as BR
import cases
import step_reference as SR
from test_gpu_budget import TOL, TOL_RANKS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHEM = SR.CHEM
IDS = [f"{row}-N{N}" for row, N in SR.MATRIX]
X_RTOL, PHI_RTOL, T_RTOL, HEAT_RTOL, RANKS_RTOL, BUDGET_RTOL = 1e-8, 1e-7, 1e-8, 1e-7, 1e-10, 1e-7


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib, _capi
    lib.plane_flux((), ())
    lib.set_option(_capi.OPT_OPEN_BOUNDARIES, 0)
    lib.lls_opacity(0.0, 0.0)
    if p.cuda_is_init():
        lib.thermal_params(False)
        lib.clumping(0)
        p.device_close()


def _device(p, N):
    """A device state for mesh N: the one the previous test left when it has this mesh (nothing is closed between rows)."""
    if p.cuda_is_init() and _device.N != N:
        p.device_close()
    if not p.cuda_is_init():
        p.device_init(N, 8)
    _device.N = N


_device.N = None


def _rel(got, ref):
    w = ref != 0
    return float(np.max(np.abs(got - ref)[w] / np.abs(ref[w]))) if w.any() else 0.0


def _defaults(lib, capi):
    """The library as it is before any keyword: periodic, no LLS opacity, no faces."""
    assert lib.get_option(capi.OPT_OPEN_BOUNDARIES) == 0 and lib.get_lls_opacity() == (0.0, 0.0) and lib.get_plane_flux() == []


def _assert_step(tag, on, got, ref):
    """got: dict(niter, xh, phi[, T, heat]) of the device; ref: reference_step's dict."""
    devs = dict(xh=_rel(got["xh"], ref["xh_intermed"]), phi=_rel(got["phi"], ref["phi_ion"]))
    if on["thermal"]:
        devs.update(T=_rel(got["T"], ref["T_end"]), heat=_rel(got["heat"], ref["phi_heat"]))
    print(tag, "niter", got["niter"], ref["niter"], "largest rel. deviation:", " ".join(f"{k} {v:.2e}" for k, v in devs.items()))
    assert got["niter"] == ref["niter"] >= 3, tag
    for k in ("xh", "phi") + (("T", "heat") if on["thermal"] else ()):
        assert np.all(np.isfinite(got[k])), (tag, k)
    np.testing.assert_allclose(got["xh"], ref["xh_intermed"], rtol=X_RTOL, atol=0, err_msg=tag)
    assert np.array_equal(got["phi"] != 0, ref["phi_ion"] != 0), tag
    np.testing.assert_allclose(got["phi"], ref["phi_ion"], rtol=PHI_RTOL, atol=0, err_msg=tag)
    if on["thermal"]:
        np.testing.assert_allclose(got["T"], ref["T_end"], rtol=T_RTOL, atol=0, err_msg=tag)
        assert np.array_equal(got["heat"] != 0, ref["phi_heat"] != 0), tag
        np.testing.assert_allclose(got["heat"], ref["phi_heat"], rtol=HEAT_RTOL, atol=0, err_msg=tag)
    return devs


def _assert_budget(tag, on, c, kw, got, ref, x0, temp0, xav):
    """The budget of a row with the budget column: against the statement on the device's own grids (x0, temp0: the step's start;
    xav: the device's XH_AV), against the composed reference's sums, and `emitted` exactly."""
    b = kw["budget"]
    own, mag = BR.sums(c["ndens"], x0, got["xh"], xav, got["phi"], temp0, CHEM, c["clump"] if on["clumping"] else 1.0,
                       c["lls"] if on["lls"] else (0.0, 0.0), got["T"] if on["thermal"] else None)
    has = mag > 0
    d_own = float(np.max(np.abs(b.sums - own)[has] / mag[has]))
    d_ref = float(np.max(np.abs(b.sums - ref["budget_sums"])[has] / ref["budget_mag"][has]))
    print(tag, f"budget: largest |dev - statement on the device's grids| / scale {d_own:.2e}, |dev - reference| / scale {d_ref:.2e}")
    assert b.sums[BR.CELLS] == own[BR.CELLS] == c["N"] ** 3
    assert np.all(np.abs(b.sums - own) <= TOL * mag), (tag, b.sums, own, mag)
    assert np.array_equal(ref["budget_mag"] > 0, has)
    assert np.all(np.abs(b.sums - ref["budget_sums"]) <= BUDGET_RTOL * ref["budget_mag"]), (tag, b.sums, ref["budget_sums"])
    assert b.emitted == W.emitted(c, kw) and b.steps == 1
    assert (b.sums[BR.LLS] > 0) == on["lls"]
    return d_own, d_ref


def _evolve3D(p, lib, capi, row, c, N):
    """One evolve3D call of a row on the current device state: (got, keywords, the device's XH_AV)."""
    on = SR.features_of(row)
    W.load_tables(p, lib, row, c)
    kw = W.library_options(row, c)
    out = p.evolve3D(c["dt"], c["dr"], c["flux"], c["pos"], True, 1000, N, 1e-2, c["temp"], c["ndens"], c["xh"], c["thin"], c["thick"],
                     cases.MINLOGTAU, c["dlogtau"], c["R"], c["conv"], cases.SIG, *CHEM, logfile=None, quiet=True, **kw)
    assert len(out) == (3 if on["thermal"] else 2)
    got = dict(niter=p.evolve._evolve.last_niter, xh=np.array(out[0]), phi=np.array(out[1]))
    g = lambda which: lib.grid_to_host(which, np.empty((N, N, N)))
    if on["thermal"]:
        got.update(T=np.array(out[2]), heat=g(capi.GRID_PHI_HEAT))
    assert bool(lib.last_raytrace_variant()["open"]) == on["open"], row
    _defaults(lib, capi)
    return got, kw, g(capi.GRID_XH_AV)


# ---- (i) evolve3D ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,N", SR.MATRIX, ids=IDS)
def test_evolve3D_row(asora, row, N):
    """The row against its reference, and then the row 0000000 on the same device state against its own: after every row, the
    last one included, the plain step is still the plain step -- the clumping mode, the thermal mode, the LLS opacity, the open
    boundaries, the faces, the second table set and the sources' spectra all left with the call that set them."""
    p, lib, capi = asora
    c, on, ref = SR.case_of(row, N), SR.features_of(row), SR.matrix_reference(row, N)
    _device(p, N)
    got, kw, xav = _evolve3D(p, lib, capi, row, c, N)
    _assert_step(f"evolve3D {row} N={N}:", on, got, ref)
    if on["budget"]:
        _assert_budget(f"evolve3D {row} N={N}:", on, c, kw, got, ref, c["xh"], c["temp"], xav)
    plain = SR.ROWS[0]
    if row != plain:
        got, _, _ = _evolve3D(p, lib, capi, plain, SR.case_of(plain, N), N)
        _assert_step(f"evolve3D {plain} N={N} after {row}:", SR.features_of(plain), got, SR.matrix_reference(plain, N))


# ---- (ii) evolve3D_resident, two steps on one device state -------------------------------------------------------------------
@pytest.mark.parametrize("row,N", SR.MATRIX, ids=IDS)
def test_two_resident_steps_of_a_row(asora, row, N):
    """The second step starts from the first's result on the device; the reference is chained the same way, from its own first
    step (step_reference.matrix_reference(row, N, 2))."""
    p, lib, capi = asora
    c, on = SR.case_of(row, N), SR.features_of(row)
    _device(p, N)
    W.load_tables(p, lib, row, c)
    g = lambda which: lib.grid_to_host(which, np.empty((N, N, N)))
    uploads = {capi.GRID_NDENS: c["ndens"], capi.GRID_TEMP: c["temp"], capi.GRID_XH: c["xh"]}
    if on["clumping"]:
        uploads[capi.GRID_CLUMP] = c["clump"]
    x0, temp0 = c["xh"], c["temp"]
    for step in (1, 2):
        kw = W.library_options(row, c)
        niter = p.evolve3D_resident(c["dt"], c["dr"], c["flux"], c["pos"], uploads, N, c["thin"], cases.MINLOGTAU, c["dlogtau"], c["R"],
                                    c["conv"], cases.SIG, *CHEM, logfile=None, quiet=True, **kw)
        assert bool(lib.last_raytrace_variant()["open"]) == on["open"], row
        _defaults(lib, capi)
        got = dict(niter=niter, xh=g(capi.GRID_XH), phi=g(capi.GRID_PHI_ION))
        assert np.array_equal(got["xh"], g(capi.GRID_XH_INTERMED))
        if on["thermal"]:
            got.update(T=g(capi.GRID_TEMP), heat=g(capi.GRID_PHI_HEAT))
            assert np.array_equal(got["T"], g(capi.GRID_TEMP_END))
        ref = SR.matrix_reference(row, N, step)
        tag = f"resident {row} N={N} step {step}:"
        _assert_step(tag, on, got, ref)
        if on["budget"]:
            _assert_budget(tag, on, c, kw, got, ref, x0, temp0, g(capi.GRID_XH_AV))
        x0, temp0, uploads = got["xh"], got.get("T", temp0), {}


# ---- (iii) two ranks on one GPU ----------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def test_two_ranks_on_both_device_loops(asora, tmp_path):
    """The rows 1111111, 1010101 and 0111100 through evolve3D_MPI on two gloo ranks sharing GPU 0, with a communicator set up for
    the slab exchange (the row with faces then runs the all-reduce loop, as designed) and on the all-reduce loop: identical bits
    on both ranks, the one-GPU evolve3D of the row to 1e-10 with the same iteration count, the composed reference at the
    tolerances of the other forms, and the budget -- the ranks' identical, the one-GPU budget to test_gpu_budget.TOL_RANKS of the
    scale, the reference's to 1e-7 of it."""
    p, lib, capi = asora
    if p.cuda_is_init():
        p.device_close()
    world, port = 2, _free_port()
    outs = [str(tmp_path / f"r{r}.npz") for r in range(world)]
    env = dict(os.environ, PYC2RAY_AMD_NO_TORCH="0", OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_matrix_dist_worker.py"), str(r), str(world), port, outs[r]],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = [q.communicate(timeout=300)[0].decode() for q in procs]
    for q, log in zip(procs, logs):
        assert q.returncode == 0, log
    res = [np.load(o) for o in outs]
    N = W.N
    _device(p, N)
    for row in SR.RANK_ROWS:
        c, on, ref = SR.case_of(row, N), SR.features_of(row), SR.matrix_reference(row, N)
        single, kw, _ = _evolve3D(p, lib, capi, row, c, N)
        keys = ("xh", "phi") + (("T", "heat") if on["thermal"] else ())
        for loop in W.LOOPS:
            tag = f"{row}_{loop}"
            for k in keys + (("sums", "emitted") if on["budget"] else ()):
                assert res[0][f"{tag}_{k}"].tobytes() == res[1][f"{tag}_{k}"].tobytes(), (tag, k)
            got = dict(niter=int(res[0][f"{tag}_niter"]), **{k: res[0][f"{tag}_{k}"] for k in keys})
            assert got["niter"] == int(res[1][f"{tag}_niter"]) == single["niter"], tag
            print(f"two ranks {row} {loop}: against one GPU", " ".join(f"{k} {_rel(got[k], single[k]):.2e}" for k in keys))
            for k in keys:
                assert np.array_equal(got[k] != 0, single[k] != 0), (tag, k)
                np.testing.assert_allclose(got[k], single[k], rtol=RANKS_RTOL, atol=0, err_msg=f"{tag} {k}")
            _assert_step(f"two ranks {row} {loop}:", on, got, ref)
            if on["budget"]:
                sums, mag = res[0][f"{tag}_sums"], ref["budget_mag"]
                has = mag > 0
                print(f"two ranks {row} {loop}: budget against one GPU {np.max(np.abs(sums - kw['budget'].sums)[has] / mag[has]):.2e}, "
                      f"against the reference {np.max(np.abs(sums - ref['budget_sums'])[has] / mag[has]):.2e} of the scale")
                assert sums[BR.CELLS] == N ** 3
                assert np.all(np.abs(sums - kw["budget"].sums) <= TOL_RANKS * mag), tag
                assert np.all(np.abs(sums - ref["budget_sums"]) <= BUDGET_RTOL * mag), tag
                assert float(res[0][f"{tag}_emitted"]) == W.emitted(c, kw) == kw["budget"].emitted
