"""GPU: the thermal mode across ranks -- evolve3D_MPI(thermal=...) on the slab and the all-reduce device loops of a TorchComm,
the heating rates exchanged with the photo-ionisation rates -- against the CPU oracle loop, the
power-of-two identity of tests/test_gpu_heating.py, and the one-GPU thermal loop.  Two ranks share GPU 0 over gloo
(tests/_thermal_dist_worker.py); one rank over RCCL covers the device-pointer views and the batches of eight iterations."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import cases
import _thermal_dist_worker as W
from oracle import oracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N = W.N
CHEM = (cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)
# the conditioning split and the tolerances of tests/test_gpu_heating.py::test_randomised_thermal_steps_against_the_oracle_loop
WELL_CONDITIONED = 1e-2
ILL_RTOL = 1e-7


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib, _capi
    if p.cuda_is_init():
        lib.thermal_params(False)
        lib.clumping(0)
        p.device_close()


def _oracle_steps(kind):
    """The two steps of W.case(kind) through the CPU oracle loop, max_iter = 100: the device loop has no iteration limit, so this
    runs FIRST and must converge.  kind = "clumped": the same loop with the clumped thermal pass of tests/clumping_reference.py."""
    from evolve_oracle import evolve3D_thermal_oracle
    c, prm = W.case(kind), W.reference_params()
    x, T, out = c["xh"], c["temp"], []
    for s in c["steps"]:
        if kind == "clumped":
            x, T, phi, heat, niter, delta, capped = _clumped_oracle_step(prm, c, s, x, T)
        else:
            x, T, phi, heat, niter, _, delta, capped = evolve3D_thermal_oracle(
                prm, c["dt"], c["dr"], s["flux"], s["pos"], T, c["ndens"], x, c["thin"], c["thick"], c["hthin"], c["hthick"],
                cases.MINLOGTAU, c["dlog"], s["R"], 1e-4, cases.SIG, *CHEM, max_iter=100, return_delta=True)
        assert 3 <= niter < 100, (kind, niter)
        out.append(dict(xh=x, temp=T, phi=phi, heat=heat, niter=niter, well=(delta > WELL_CONDITIONED) & ~capped))
    return out


def _clumped_oracle_step(prm, c, s, xh, temp):
    """evolve_oracle.evolve3D_thermal_oracle with clumping_reference.chemistry_thermal (one constant factor) as its pass."""
    import clumping_reference as CR
    ncell, ns = N ** 3, s["flux"].shape[0]
    crit = min(int(1e-4 * ncell), (ns - 1) / 3)
    prev1 = prev0 = 2 * ncell
    xav = np.array(xh, dtype=np.float64, order="C", copy=True)
    pos0 = np.ravel((np.asarray(s["pos"]) - 1).astype("int32"), order="F")
    niter, converged = 0, False
    while not converged and niter < 100:
        niter += 1
        r = O.asora_do_all_sources(s["R"], cases.SIG, c["dr"], c["ndens"], xav, pos0, s["flux"], c["thin"], c["thick"], cases.MINLOGTAU,
                                   c["dlog"], NumTau=c["thin"].shape[0], flags=O.ASORA_MODE, heat_thin=c["hthin"], heat_thick=c["hthick"])
        xi, xav, te, conv, delta, capped = CR.chemistry_thermal(prm, c["dt"], c["ndens"], temp, xh, xav, r["phi_ion"],
                                                                        r["phi_heat"], *CHEM, W.CLUMP)
        s1, s0 = np.sum(xi), np.sum(1.0 - xi)
        rel1, rel0 = abs((s1 - prev1) / s1), abs((s0 - prev0) / s0)
        converged = conv < crit or (rel1 < 1e-4 and rel0 < 1e-4)
        prev1, prev0 = s1, s0
    return xi, te, r["phi_ion"], r["phi_heat"], niter, delta, capped


_ORACLE = {}


def _reference(kind):
    """Computed once per kind, shared by the tests, never written to."""
    if kind not in _ORACLE:
        _ORACLE[kind] = _oracle_steps(kind)
        for st in _ORACLE[kind]:
            for a in st.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    return _ORACLE[kind]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def _run_ranks(tmp_path, world, exchange, kind, backend="gloo", **env):
    """The ranks as child processes; on a timeout or a failing rank all of them are killed and the test fails with their logs."""
    port = _free_port()
    outs = [str(tmp_path / f"{kind}_{exchange}_r{r}.npz") for r in range(world)]
    e = dict(os.environ, PYC2RAY_AMD_NO_TORCH="0", OMP_NUM_THREADS="1", **env)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_thermal_dist_worker.py"), str(r), str(world), port, outs[r],
                               exchange, kind, backend], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs, failed = [], False
    for q in procs:
        try:
            logs.append(q.communicate(timeout=300)[0].decode(errors="replace"))
        except subprocess.TimeoutExpired:
            failed = True
            break
    if failed or any(q.returncode != 0 for q in procs):
        for q in procs:
            if q.poll() is None:
                q.kill()
        logs = [q.communicate()[0].decode(errors="replace") if i >= len(logs) else logs[i] for i, q in enumerate(procs)]
        pytest.fail("a rank failed or timed out:\n" + "\n----\n".join(log[-3000:] for log in logs))
    return [np.load(o) for o in outs]


def _assert_step_equals(got, ref, k, tag, prefix=""):
    """The assertions of test_randomised_thermal_steps_against_the_oracle_loop for step k of `got` (a rank's npz) against `ref`."""
    x, T, phi, heat = (got[f"{prefix}{name}{k}"] for name in ("xh", "temp", "phi", "heat"))
    well = ref["well"]
    assert well.any(), tag
    np.testing.assert_allclose(x[well], ref["xh"][well], rtol=1e-10, atol=0, err_msg=tag)
    np.testing.assert_allclose(T[well], ref["temp"][well], rtol=1e-10, atol=0, err_msg=tag)
    np.testing.assert_allclose(x, ref["xh"], rtol=ILL_RTOL, atol=0, err_msg=tag)
    np.testing.assert_allclose(T, ref["temp"], rtol=ILL_RTOL, atol=0, err_msg=tag)
    for g, want in ((phi, ref["phi"]), (heat, ref["heat"])):
        assert np.array_equal(g != 0, want != 0), tag
        np.testing.assert_allclose(g, want, rtol=1e-7, atol=1e-13 * want.max(), err_msg=tag)


def _assert_ranks_identical(res, keys=("xh", "temp", "phi", "heat")):
    for k in range(2):
        for name in keys:
            assert np.array_equal(res[0][f"{name}{k}"], res[1][f"{name}{k}"]), (name, k)
        assert int(res[0][f"niter{k}"]) == int(res[1][f"niter{k}"])
        assert tuple(res[0][f"stats{k}"]) == tuple(res[1][f"stats{k}"])


# ---- 1: two ranks against the CPU oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", ["slab", "allreduce"])
def test_two_ranks_against_the_oracle_loop(asora, tmp_path, exchange):
    """Two consecutive evolve3D_MPI(thermal=tp) steps on two ranks: black-body photo and heating tables, a log-normal density,
    temperatures over 1e2 - 1e4 K, eight and nine overlapping sources (R = 4 and 5) whose spheres cross the slab boundary at plane
    N / 2 from both sides and wrap through plane 0, all five cooling channels, Compton at z = 8.  Both ranks return bit-identical
    x, T and rate grids and equal iteration counts; against evolve3D_thermal_oracle: equal iteration counts, and the tolerances
    of the one-GPU sweep."""
    p, lib, capi = asora
    ref = _reference("oracle")
    c = W.case("oracle")
    from pyc2ray_amd.dist import SlabPlan, TorchComm
    for s in c["steps"]:             # the geometry the test is about: both ranks send across plane N / 2, and a sphere wraps
        assert s["flux"].shape[0] >= 8 and s["R"] >= 4
        spos, _, b = TorchComm.shard_sources_by_slab(s["pos"], s["flux"], 2)
        plan = SlabPlan(N, 2, s["R"], [spos[0, b[r]:b[r + 1]] - 1 for r in range(2)])
        assert plan.reach[0][N // 2] and plan.reach[1][N // 2 - 1] and plan.reach[0][N - 1] and plan.reach[1][0]
    if p.cuda_is_init():
        p.device_close()
    res = _run_ranks(tmp_path, 2, exchange, "oracle")
    _assert_ranks_identical(res)
    for k in range(2):
        tag = f"{exchange} step {k}"
        assert int(res[0][f"niter{k}"]) == ref[k]["niter"], tag
        _assert_step_equals(res[0], ref[k], k, tag)


# ---- 2: heating lands where the rates land ------------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", ["slab", "allreduce"])
def test_heating_lands_where_the_rates_land(asora, tmp_path, exchange):
    """Heating tables = 2^-35 x the photo tables, non-overlapping sources on the N / 2 lattice (every cell has ONE contributing
    source, so the sums over layouts and ranks are exact): PHI_HEAT == 2^-35 PHI_ION bit for bit on every rank after BOTH steps.
    Heating planes added to the wrong planes, a heating pair not zeroed on foreign planes, a stale pair in the second step
    would all show."""
    p, lib, capi = asora
    ref = _reference("identity")
    c = W.case("identity")
    for s in c["steps"]:
        first = s["pos"][0] - 1
        assert 2 * int(np.floor(s["R"])) < N // 2 and (first == N // 2).any() and (first == 0).any()     # straddles N / 2; wraps
    if p.cuda_is_init():
        p.device_close()
    res = _run_ranks(tmp_path, 2, exchange, "identity")
    _assert_ranks_identical(res)
    for r in res:
        for k in range(2):
            assert int(r[f"niter{k}"]) == ref[k]["niter"]
            assert r[f"phi{k}"].max() > 0 and np.array_equal(r[f"heat{k}"], W.P2 * r[f"phi{k}"]), (exchange, k)
            assert np.array_equal(r[f"phi{k}"] != 0, ref[k]["phi"] != 0)


# ---- 3: one process owning every plane ----------------------------------------------------------------------------------
def _upload(p, lib, capi, n, c, s, tp):
    if p.cuda_is_init():
        p.device_close()
    p.device_init(n, 8)
    p.photo_table_to_device(c["thin"], c["thick"])
    p0, f0 = cases.flat_sources(s["pos"], s["flux"])
    lib.source_data_to_device(p0, f0, s["flux"].shape[0])
    for which, a in ((capi.GRID_NDENS, c["ndens"]), (capi.GRID_TEMP, c["temp"]), (capi.GRID_XH, c["xh"])):
        lib.grid_to_device(which, a)
    tp.apply(lib)


def _small_case(n):
    rng = np.random.default_rng(700 + n)
    thin, thick, hthin, hthick, dlog = cases.blackbody_photo_and_heat_tables(num_tau=600)
    nd, xh, dr = cases.grid(n, "lognormal", 700 + n, 0.3, xlo=1e-4, xhi=2e-3)
    h = n // 2
    pts = np.array([(1 + a * h, 1 + b * h, 1 + cc * h) for a in (0, 1) for b in (0, 1) for cc in (0, 1)]).T
    pos = pts[:, [0, 3, 5, 6, 7]]
    flux = rng.uniform(0.5, 2.0, size=5) * 3e-4 * (n / 16.0) ** 3 / 5
    c = dict(thin=thin, thick=thick, hthin=hthin, hthick=hthick, dlog=dlog, ndens=nd, xh=xh, dr=dr,
             temp=10 ** rng.uniform(2.0, 4.0, size=(n, n, n)))
    return c, dict(pos=pos, flux=flux, R=2.5)


@pytest.mark.parametrize("n", [17, 24])
def test_one_process_owning_every_plane_equals_the_one_gpu_loop(asora, n):
    """asora_evolve_begin_slab_thermal(..., 0, N) and four iterations of trace -> pass -> close, no communicator, against
    asora_evolve_begin + evolve_enqueue(4) in thermal mode on the same non-overlapping sources (rates bit-reproducible): the
    thermal pass over a plane range with rank-local sums.  Bit-identical XH_INTERMED, XH_AV, TEMP_END, PHI_ION and PHI_HEAT,
    equal conv_flag per history row and thermal statistics; the sums to 1e-13 (the reduction trees may differ)."""
    p, lib, capi = asora
    c, s = _small_case(n)
    tp = W.thermal_params(c)
    ns, numtau = 5, c["thin"].shape[0]
    args = (3.15576e13, *CHEM, s["R"], cases.SIG, c["dr"], cases.MINLOGTAU, c["dlog"], numtau, 0, ns, -1.0, 0.0)
    grids = (capi.GRID_XH_INTERMED, capi.GRID_XH_AV, capi.GRID_TEMP_END, capi.GRID_PHI_ION, capi.GRID_PHI_HEAT)
    g = lambda: [lib.grid_to_host(w, np.empty((n, n, n))) for w in grids]
    try:
        _upload(p, lib, capi, n, c, s, tp)
        lib.evolve_begin(*args)
        lib.evolve_enqueue(4)
        niter1, done1, rows1 = lib.evolve_poll(8)
        one, stats1 = g(), lib.thermal_stats()
        _upload(p, lib, capi, n, c, s, tp)
        lib.evolve_begin_slab_thermal(*args, 0, n)
        for _ in range(4):
            lib.evolve_slab_trace(0, ns)
            lib.evolve_slab_pass()
            lib.evolve_slab_close(None)
        niter2, done2, rows2 = lib.evolve_poll(8)
        two, stats2 = g(), lib.thermal_stats()
        assert (niter1, done1, len(rows1)) == (4, False, 4) == (niter2, done2, len(rows2))
        for a, b, which in zip(one, two, grids):
            assert np.array_equal(a, b), which
        assert one[4].max() > 0 and np.any(one[2] != c["temp"])
        for r1, r2 in zip(rows1, rows2):
            assert r1[0] == r2[0]
            assert abs(r1[1] - r2[1]) <= 1e-13 * abs(r1[1]) and abs(r1[2] - r2[2]) <= 1e-13 * abs(r1[2])
        assert stats1 == stats2 and stats1[2] >= 1
        # the counters are reset by the next begin
        lib.evolve_begin_slab_thermal(*args, 0, n)
        assert lib.thermal_stats() == (0, 0, 0)
    finally:
        lib.thermal_params(False)
    p.device_close()


# ---- 4: one rank over RCCL ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", ["slab", "allreduce"])
def test_world1_rccl_thermal_step_equals_the_one_gpu_step(asora, tmp_path, exchange):
    """A thermal step through TorchComm on the nccl backend (= RCCL), one rank, as a child process: the zero-copy views of both
    out-boxes, the all-reduce of both (forced: PYC2RAY_AMD_FORCE_COLLECTIVE), TEMP_END and PHI_HEAT through slab_gather, batches
    of eight iterations per poll.  Equal iteration counts, and the one-GPU evolve3D(thermal=) step of the same process under the
    tolerances of the oracle comparison (the conditioning split is the oracle's)."""
    p, lib, capi = asora
    ref = _reference("oracle")
    if p.cuda_is_init():
        p.device_close()
    (r,) = _run_ranks(tmp_path, 1, exchange, "oracle", backend="nccl", PYC2RAY_AMD_FORCE_COLLECTIVE="1")
    for k in range(2):
        tag = f"{exchange} step {k}"
        assert int(r[f"niter{k}"]) == int(r[f"one_niter{k}"]) == ref[k]["niter"], tag
        one = dict(xh=r[f"one_xh{k}"], temp=r[f"one_temp{k}"], phi=r[f"one_phi{k}"], heat=r[f"one_heat{k}"], well=ref[k]["well"])
        _assert_step_equals(r, one, k, tag)
        assert tuple(r[f"stats{k}"]) == tuple(r[f"one_stats{k}"]), tag


# ---- 5: refusals and hygiene ------------------------------------------------------------------------------------------------
def test_begin_slab_thermal_refusals(asora):
    p, lib, capi = asora
    c, s = _small_case(17)
    if p.cuda_is_init():
        p.device_close()
    p.device_init(17, 8)
    p.photo_table_to_device(c["thin"], c["thick"])
    args = (3.15576e13, *CHEM, s["R"], cases.SIG, c["dr"], cases.MINLOGTAU, c["dlog"], c["thin"].shape[0], 0, 0, -1.0, 0.0, 0, 17)
    with pytest.raises(RuntimeError, match=r"code 4\).*heating tables"):
        lib.evolve_begin_slab_thermal(*args)
    lib.heat_table_to_device(c["hthin"], c["hthick"], c["hthin"].shape[0])
    with pytest.raises(RuntimeError, match=r"code 4\).*asora_thermal_params"):
        lib.evolve_begin_slab_thermal(*args)
    p.device_close()


def test_an_isothermal_step_after_thermal_steps_is_the_fresh_one(asora, tmp_path):
    """After thermal sharded steps the library is isothermal again (the worker begins an isothermal slab step after each, which
    fails in thermal mode), and an isothermal evolve3D_MPI step on the same processes gives what fresh processes give."""
    p, lib, capi = asora
    _reference("oracle")
    if p.cuda_is_init():
        p.device_close()
    after = _run_ranks(tmp_path, 2, "slab", "iso_after")
    fresh = _run_ranks(tmp_path, 2, "slab", "iso_fresh")
    for a in after:
        assert int(a["iso_niter"]) == int(fresh[0]["iso_niter"])
        # (the same kernels on the same inputs; the order of the trace's atomics is free)
        np.testing.assert_allclose(a["iso_xh"], fresh[0]["iso_xh"], rtol=1e-10, atol=0)
        np.testing.assert_allclose(a["iso_phi"], fresh[0]["iso_phi"], rtol=1e-10, atol=0)
        assert not np.allclose(a["iso_xh"], a["xh0"], rtol=1e-3)


# ---- 6: clumping ------------------------------------------------------------------------------------------------------------
def test_two_ranks_with_a_constant_clumping_factor(asora, tmp_path):
    """One two-rank case with a constant clumping factor against the one-GPU clumped thermal step, under the tolerances of the
    oracle comparison (conditioning split: the clumped CPU loop's)."""
    p, lib, capi = asora
    ref = _reference("clumped")
    if p.cuda_is_init():
        p.device_close()
    res = _run_ranks(tmp_path, 2, "slab", "clumped")
    _assert_ranks_identical(res)
    c = W.case("clumped")
    p.device_init(N, 8)
    p.photo_table_to_device(c["thin"], c["thick"])
    one = W._one_gpu(p, lib, capi, c, W.thermal_params(c))
    p.device_close()
    unclumped = _reference("oracle")
    for k in range(2):
        tag = f"clumped step {k}"
        assert int(res[0][f"niter{k}"]) == int(one[f"one_niter{k}"]) == ref[k]["niter"], tag
        want = dict(xh=one[f"one_xh{k}"], temp=one[f"one_temp{k}"], phi=one[f"one_phi{k}"], heat=one[f"one_heat{k}"], well=ref[k]["well"])
        _assert_step_equals(res[0], want, k, tag)
        assert not np.allclose(res[0][f"xh{k}"], unclumped[k]["xh"], rtol=1e-3), tag
