"""GPU: open (non-periodic) box boundaries of the raytrace -- ASORA_OPT_OPEN_BOUNDARIES and the
``periodic=`` keyword -- against the CPU oracle's periodic trace on a padded mesh, cropped (tests/open_boundary_reference.py).
The tolerances are those of the tests without the feature (tests/test_gpu_parity.py: GAMMA_RTOL for a raytrace, 1e-8 / 1e-7 for
a step, 1e-10 between ranks and one GPU)."""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import cases
import open_boundary_reference as OB
from oracle import oracle as O
from test_gpu_parity import GAMMA_RTOL

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_test.yml")
CHEM = (cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)
SHAPE_OPTS = ("OPT_SECTORS", "OPT_BLOCK_THREADS", "OPT_PAIR_SOURCES", "OPT_HEATING", "OPT_GREY_NOTABLES", "OPT_GLOBAL_ATOMICS",
              "OPT_OPEN_BOUNDARIES")

#: 0-based source positions.  N = 16, R = 6: two opposite corners, an edge, the centre, a face
SRC16 = np.array([(0, 0, 0), (15, 15, 15), (0, 7, 15), (8, 8, 8), (3, 15, 0)], dtype=np.int32)
#: N = 48, R = 20: a corner, an edge, a face, inside, and a second face (an odd count: the paired form's last workgroup is half empty)
SRC48 = np.array([(0, 0, 0), (47, 0, 21), (17, 30, 47), (24, 23, 25), (5, 40, 9)], dtype=np.int32)
#: N = 76, R = 36 (one workgroup per source: the shells outgrow LDS): a corner and a face
SRC76 = np.array([(75, 0, 75), (30, 41, 2)], dtype=np.int32)
CASES = {"n16": (16, 6.0, 24, SRC16, 3, 0.08), "n48": (48, 20.0, 72, SRC48, 5, 0.05), "n76": (76, 36.0, 112, SRC76, 6, 0.03)}


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib, _capi
    for name in SHAPE_OPTS:
        lib.set_option(getattr(_capi, name), 0)
    lib.lls_opacity(0.0, 0.0)
    if p.cuda_is_init():
        lib.thermal_params(False)
        lib.clumping(0)
        p.device_close()


@functools.lru_cache(maxsize=None)
def _case(name):
    N, R, M, src, seed, tau_cell = CASES[name]
    nd, xh, dr = cases.grid(N, "lognormal", seed, tau_cell)
    if name == "n16":
        # a power of two (a mean cell of tau = 0.058): the reference's floating-point distance test (raytracing.cu:315) then keeps
        # the lattice points that sit exactly on the sphere of radius 6, and the rated pairs are the lattice points (rated_pairs)
        dr = 2.0 ** 63
    thin, thick, dlog = cases.soft_tables()
    n = thin.shape[0]
    flux = 3.0 * (1.0 + 0.25 * np.arange(len(src)))
    pos1 = (src + 1).T.copy()                                                     # (3, ns), 1-based: what the entry points take
    c = dict(N=N, R=R, M=M, pos0=src.ravel().copy(), pos=pos1, flux=flux, ndens=nd, xh=xh, dr=dr, thin=thin, thick=thick, dlogtau=dlog,
             heat_thin=1e-11 * thin * np.linspace(1.0, 2.0, n), heat_thick=0.7e-11 * thick * np.linspace(2.0, 1.0, n))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _reference(name, nsrc, numtau_minus, heat):
    """The padded oracle's cropped trace of the first `nsrc` sources of a case, computed once and shared."""
    c = _case(name)
    kw = dict(heat_thin=c["heat_thin"], heat_thick=c["heat_thick"]) if heat else {}
    r = OB.open_trace(c["R"], cases.SIG, c["dr"], c["ndens"], c["xh"], c["pos0"][:3 * nsrc], c["flux"][:nsrc], c["thin"], c["thick"],
                      cases.MINLOGTAU, c["dlogtau"], NumTau=c["thin"].shape[0] - numtau_minus, M=c["M"], **kw)
    for a in r.values():
        a.setflags(write=False)
    return r


def _fresh(p, N, thin, thick):
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)
    p.photo_table_to_device(thin, thick)


def _setup(p, lib, capi, c, heat=False):
    _fresh(p, c["N"], c["thin"], c["thick"])
    if heat:
        lib.heat_table_to_device(c["heat_thin"], c["heat_thick"], c["thin"].shape[0])
    lib.source_data_to_device(c["pos0"], c["flux"], c["flux"].shape[0])
    lib.grid_to_device(capi.GRID_NDENS, c["ndens"])
    lib.grid_to_device(capi.GRID_XH_AV, c["xh"])


def _trace(lib, capi, c, nsrc=None, opts=None, heat=False):
    """asora_raytrace_device under `opts` ({option name: value}), all of them back to 0 afterwards.  (phi_ion, phi_heat, variant)"""
    N = c["N"]
    opts = dict(opts or {})
    if heat:
        opts["OPT_HEATING"] = 1
    try:
        for k, v in opts.items():
            lib.set_option(getattr(capi, k), v)
        lib.raytrace_device(c["R"], cases.SIG, c["dr"], 0, c["flux"].shape[0] if nsrc is None else nsrc, cases.MINLOGTAU, c["dlogtau"],
                            c["thin"].shape[0] - 1)
        phi = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
        h = lib.grid_to_host(capi.GRID_PHI_HEAT, np.empty((N, N, N))) if heat else None
    finally:
        for k in opts:
            lib.set_option(getattr(capi, k), 0)
    return phi, h, lib.last_raytrace_variant()


def _rel(got, ref):
    w = ref != 0
    return np.max(np.abs(got - ref)[w] / np.abs(ref[w])) if w.any() else 0.0


def _assert_matches(got, ref, tag):
    print(tag, "max rel. difference", _rel(got, ref), "cells at exactly 0:", int((ref == 0).sum()))
    assert np.array_equal(got != 0, ref != 0), tag                  # what the reference leaves at exactly 0 is exactly 0
    np.testing.assert_allclose(got, ref, rtol=GAMMA_RTOL, atol=0, err_msg=tag)


def _do_raytracing(p, c, heat=False, **kw):
    zeros = np.zeros_like(c["thin"])
    return p.do_raytracing(c["dr"], c["flux"], c["pos"], True, 1000, c["N"], 1e-2, c["ndens"], c["xh"], c["thin"], c["thick"],
                           c["heat_thin"] if heat else zeros, c["heat_thick"] if heat else zeros, cases.MINLOGTAU, c["dlogtau"], c["R"],
                           cases.SIG, logfile=None, quiet=True, **kw)


# ---- 1. traces against the padded oracle, 2. the exact pair count ------------------------------------------------------------
def test_do_raytracing_keyword_against_the_padded_oracle(asora):
    """N = 16, R = 6, five sources on corners, an edge, a face and inside, through do_raytracing(periodic=False), without and with
    heating tables (the single-source HEAT form); the pair counts of the open and of the periodic call."""
    p, lib, capi = asora
    c = _case("n16")
    _fresh(p, c["N"], c["thin"], c["thick"])
    phi, none = _do_raytracing(p, c, periodic=False)
    assert none is None and lib.get_option(capi.OPT_OPEN_BOUNDARIES) == 0
    v = lib.last_raytrace_variant()
    assert v["open"] and v["buffer_atomics"], v
    ref = _reference("n16", 5, 0, True)              # (do_raytracing passes NumTau = len(table), raytracing.py:64)
    _assert_matches(phi, ref["phi_ion"], "do_raytracing n16")
    assert lib.last_raytrace_counts()[0] == OB.rated_pairs(16, 6.0, c["pos0"]) == 1797
    phi_p, _ = _do_raytracing(p, c)
    assert not lib.last_raytrace_variant()["open"]
    assert lib.last_raytrace_counts()[0] == OB.rated_pairs(16, 6.0, c["pos0"], periodic=True) == 5 * 925
    changed = phi_p != phi
    assert changed.sum() > 1000 and np.all(phi[changed] < phi_p[changed]) and np.any((phi == 0) & (phi_p != 0))
    phi_h, heat = _do_raytracing(p, c, heat=True, periodic=False)
    v = lib.last_raytrace_variant()
    assert v["open"] and not v["paired"], v
    _assert_matches(phi_h, ref["phi_ion"], "do_raytracing n16 with heating: phi_ion")
    _assert_matches(heat, ref["phi_heat"], "do_raytracing n16 with heating: phi_heat")
    assert lib.last_raytrace_counts()[0] == 1797


#: (options, heating, sources traced) -> the forms built with OPEN at 256-entry LDS tables and the shells in LDS: two sources per
#: workgroup at 256 and 512 threads (five sources: the last workgroup carries a filler; four: none does), one source per workgroup
#: at 256 and 512 threads without and with heating; over the decompositions of a source (units per source in the comment)
RUNS48 = [
    ({"OPT_PAIR_SOURCES": 2}, False, 5),                                                  # library's choice of units
    ({"OPT_PAIR_SOURCES": 2}, False, 4),
    ({"OPT_PAIR_SOURCES": 2, "OPT_BLOCK_THREADS": 512, "OPT_SECTORS": 3}, False, 5),      # 12 mirrored sector pairs
    ({"OPT_PAIR_SOURCES": 2, "OPT_BLOCK_THREADS": 64, "OPT_SECTORS": 9}, False, 5),       # 6 sectors; 64 threads become 256
    ({"OPT_PAIR_SOURCES": 2, "OPT_SECTORS": 6}, False, 5),                                # the whole sphere
    ({"OPT_PAIR_SOURCES": 1}, False, 5),
    ({"OPT_PAIR_SOURCES": 1, "OPT_BLOCK_THREADS": 512, "OPT_SECTORS": 1}, False, 5),      # 8 octants
    ({"OPT_PAIR_SOURCES": 1, "OPT_BLOCK_THREADS": 1024, "OPT_SECTORS": 5}, False, 5),     # 4 octant pairs; 1024 threads become 512
    ({"OPT_PAIR_SOURCES": 1, "OPT_SECTORS": 2}, False, 5),                                # 24 sectors
    ({"OPT_SECTORS": 7}, True, 5),                                                        # 2 half spheres
    ({"OPT_BLOCK_THREADS": 512, "OPT_SECTORS": 8}, True, 5),                              # 3 all-sign sectors
    ({"OPT_SECTORS": 4}, True, 4),                                                        # 96 wedges
]


def test_every_open_form_with_shells_in_lds_against_the_padded_oracle(asora):
    """N = 48, R = 20, M = 72."""
    p, lib, capi = asora
    c = _case("n48")
    _setup(p, lib, capi, c, heat=True)
    seen = set()
    for opts, heat, nsrc in RUNS48:
        ref = _reference("n48", nsrc, 1, True)
        phi, h, v = _trace(lib, capi, c, nsrc, dict(opts, OPT_OPEN_BOUNDARIES=1), heat)
        tag = f"n48 {opts} heat={heat} nsrc={nsrc} -> {v}"
        assert v["open"] and v["buffer_atomics"] and not v["global_shells"] and not v["skip_zero"] and v["threads"] in (256, 512), tag
        assert v["paired"] == (opts.get("OPT_PAIR_SOURCES") == 2), tag
        seen.add((v["paired"], v["threads"], heat))
        _assert_matches(phi, ref["phi_ion"], tag)
        if heat:
            _assert_matches(h, ref["phi_heat"], tag + " heat")
        assert lib.last_raytrace_counts()[0] == OB.rated_pairs(48, 20.0, c["pos0"][:3 * nsrc], dr=c["dr"]), tag
    assert seen == {(True, 256, False), (True, 512, False), (False, 256, False), (False, 512, False), (False, 256, True),
                    (False, 512, True)}
    # and the periodic trace of the same state differs: most of four spheres wrap
    per, _, v = _trace(lib, capi, c, 5, {"OPT_PAIR_SOURCES": 2})
    assert not v["open"] and (per != _reference("n48", 5, 1, True)["phi_ion"]).sum() > 10000


@pytest.mark.parametrize("threads", [256, 512])
def test_open_forms_with_shells_in_global_memory(asora, threads):
    """N = 76, R = 36, one workgroup per source: its shells (194 KB) outgrow LDS, the rates still go through buffer atomics."""
    p, lib, capi = asora
    c = _case("n76")
    _setup(p, lib, capi, c, heat=True)
    for heat in (False, True):
        ref = _reference("n76", 2, 1, True)
        phi, h, v = _trace(lib, capi, c, 2, {"OPT_SECTORS": 6, "OPT_BLOCK_THREADS": threads, "OPT_OPEN_BOUNDARIES": 1}, heat)
        tag = f"n76 threads={threads} heat={heat} -> {v}"
        assert v["open"] and v["global_shells"] and v["buffer_atomics"] and v["units"] == 1 and v["threads"] == threads, tag
        _assert_matches(phi, ref["phi_ion"], tag)
        if heat:
            _assert_matches(h, ref["phi_heat"], tag + " heat")
        assert lib.last_raytrace_counts()[0] == OB.rated_pairs(76, 36.0, c["pos0"], dr=c["dr"]), tag


# ---- 3. where open equals periodic -------------------------------------------------------------------------------------------
def test_sources_far_from_every_face_give_the_periodic_rates(asora):
    """Two sources at least R from every face (two: their sum does not depend on the order of the atomics)."""
    p, lib, capi = asora
    c = dict(_case("n16"))
    c["pos0"] = np.array([6, 7, 9, 9, 6, 8], dtype=np.int32)
    c["pos"] = (c["pos0"].reshape(2, 3) + 1).T.copy()
    c["flux"] = c["flux"][:2]
    _fresh(p, c["N"], c["thin"], c["thick"])
    per, _ = _do_raytracing(p, c, periodic=True)
    n_per = lib.last_raytrace_counts()[0]
    opn, _ = _do_raytracing(p, c, periodic=False)
    assert lib.last_raytrace_variant()["open"] and lib.last_raytrace_counts()[0] == n_per == 2 * 925
    assert np.array_equal(per, opn) and per.max() > 0


def test_whole_box_window_of_an_odd_mesh_has_no_cell_outside(asora):
    """N = 17, one source at the centre, R = 20: the window -8 ... 8 is the whole box, clipped-window tables in open mode."""
    p, lib, capi = asora
    N = 17
    nd, xh, dr = cases.grid(N, "lognormal", 4, 0.05)
    thin, thick, dlog = cases.soft_tables()
    c = dict(N=N, R=20.0, ndens=nd, xh=xh, dr=dr, thin=thin, thick=thick, dlogtau=dlog, pos0=np.array([8, 8, 8], dtype=np.int32),
             flux=np.array([3.0]))
    _setup(p, lib, capi, c)
    per, _, v0 = _trace(lib, capi, c)
    n_per = lib.last_raytrace_counts()[0]
    opn, _, v1 = _trace(lib, capi, c, opts={"OPT_OPEN_BOUNDARIES": 1})
    assert v1["open"] and not v0["open"] and lib.last_raytrace_counts()[0] == n_per
    assert np.array_equal(per, opn) and np.all(per > 0)


def test_the_largest_mesh_takes_the_1024_entry_tables(asora):
    """N = 512 with the source at (256, 256, 256) and R beyond the box: 257 shells, so the forms with 1024-entry LDS tables run,
    their shells in global memory; the window -256 ... 255 is the whole box and no cell is outside: the periodic rates.  The only
    mesh at which those forms exist (257 shells need N = 512, beyond it open boundaries are refused); uniform grids made with
    np.full, one source: 1.9 s on the MI355X."""
    p, lib, capi = asora
    N = 512
    thin, thick, dlog = cases.soft_tables()
    c = dict(N=N, R=1000.0, ndens=np.full((N, N, N), 1e-3), xh=np.full((N, N, N), 2e-4), dr=0.002 / (cases.SIG * 1e-3), thin=thin,
             thick=thick, dlogtau=dlog, pos0=np.array([256, 256, 256], dtype=np.int32), flux=np.array([3.0]))
    lib.set_option(capi.OPT_PLACEMENT_CANDIDATES, 1)
    try:
        _setup(p, lib, capi, c)
    finally:
        lib.set_option(capi.OPT_PLACEMENT_CANDIDATES, 0)
    per, _, v0 = _trace(lib, capi, c)
    n_per = lib.last_raytrace_counts()[0]
    opn, _, v1 = _trace(lib, capi, c, opts={"OPT_OPEN_BOUNDARIES": 1})
    assert v1["open"] and v1["buffer_atomics"] and v1["global_shells"], v1
    assert lib.last_raytrace_counts()[0] == n_per
    assert np.array_equal(per, opn) and per.min() > 0
    p.device_close()


# ---- 4. switching in one process ---------------------------------------------------------------------------------------------
def test_mode_switching_and_option_restored_after_a_failure(asora):
    p, lib, capi = asora
    c = dict(_case("n16"))
    c["pos0"], c["pos"], c["flux"] = c["pos0"][:3], c["pos"][:, :1], c["flux"][:1]       # (one source: a trace repeats itself)
    _fresh(p, c["N"], c["thin"], c["thick"])
    first, _ = _do_raytracing(p, c)
    opn, _ = _do_raytracing(p, c, periodic=False)
    third, _ = _do_raytracing(p, c, periodic=True)
    assert np.array_equal(first, third) and not np.array_equal(first, opn)
    _assert_matches(opn, _reference("n16", 1, 0, True)["phi_ion"], "one corner source")
    # a call that fails inside the library (a negative radius) leaves the library periodic
    with pytest.raises(RuntimeError):
        p.do_raytracing(c["dr"], c["flux"], c["pos"], True, 1000, 16, 1e-2, c["ndens"], c["xh"], c["thin"], c["thick"], None, None,
                        cases.MINLOGTAU, c["dlogtau"], -1.0, cases.SIG, logfile=None, quiet=True, periodic=False)
    assert lib.get_option(capi.OPT_OPEN_BOUNDARIES) == 0
    assert np.array_equal(_do_raytracing(p, c)[0], first)


# ---- 5. whole steps ----------------------------------------------------------------------------------------------------------
def _step_case(interior):
    N = 16
    nd, xh, dr = cases.grid(N, "lognormal", 61, 0.2, xlo=1e-4, xhi=2e-3)
    thin, thick, dlog = cases.soft_tables()
    src = np.array([(6, 7, 9), (9, 6, 8)], dtype=np.int32) if interior else SRC16
    return dict(N=N, ndens=nd, xh=xh, dr=dr, temp=np.full((N, N, N), 1e4), pos=(src + 1).T.copy(), flux=np.full(len(src), 1.5e-4),
                thin=thin, thick=thick, dlogtau=dlog, R=6.0, dt=2 * cases.MYR, conv=1e-4)


def _evolve(p, c, **kw):
    out = p.evolve3D(c["dt"], c["dr"], c["flux"], c["pos"], True, 1000, c["N"], 1e-2, c["temp"], c["ndens"], c["xh"], c["thin"],
                     c["thick"], cases.MINLOGTAU, c["dlogtau"], c["R"], c["conv"], cases.SIG, *CHEM, logfile=None, quiet=True, **kw)
    return (p.evolve._evolve.last_niter,) + tuple(np.array(a) for a in out)


def test_evolve3D_against_the_padded_oracle_loop(asora):
    p, lib, capi = asora
    c = _step_case(interior=False)
    _fresh(p, c["N"], c["thin"], c["thick"])
    niter, x, phi = _evolve(p, c, periodic=False)
    assert lib.get_option(capi.OPT_OPEN_BOUNDARIES) == 0
    x_ref, phi_ref, niter_ref, _ = OB.evolve3D_open_oracle(c["dt"], c["dr"], c["flux"], c["pos"], c["temp"], c["ndens"], c["xh"], c["thin"],
                                                           c["thick"], cases.MINLOGTAU, c["dlogtau"], c["R"], c["conv"], cases.SIG, *CHEM,
                                                           M=24)
    print("niter", niter, niter_ref, "max rel. difference x", np.max(np.abs(x - x_ref) / x_ref), "phi", _rel(phi, phi_ref))
    assert niter == niter_ref and niter >= 2 and x.max() > 0.5
    np.testing.assert_allclose(x, x_ref, rtol=1e-8, atol=0)
    assert np.array_equal(phi != 0, phi_ref != 0)
    np.testing.assert_allclose(phi, phi_ref, rtol=1e-7, atol=0)
    per = _evolve(p, c)
    assert (per[2] != 0).sum() > (phi != 0).sum() + 1000 and per[1].mean() > x.mean()


def test_evolve3D_with_interior_sources_is_the_periodic_step(asora):
    p, lib, capi = asora
    c = _step_case(interior=True)
    _fresh(p, c["N"], c["thin"], c["thick"])
    per = _evolve(p, c, periodic=True)
    opn = _evolve(p, c, periodic=False)
    assert per[0] == opn[0] >= 2 and np.array_equal(per[1], opn[1]) and np.array_equal(per[2], opn[2])


def test_evolve3D_with_every_opt_in_at_once(asora):
    """thermal=, clumping=, lls= and two spectra together, interior sources: the open forms with heating are reached and give the
    periodic step's bits."""
    from pyc2ray_amd.lls import LLSOpacity
    from pyc2ray_amd.thermal import ThermalParams
    p, lib, capi = asora
    c = _step_case(interior=True)
    thin, thick = c["thin"], c["thick"]
    n = thin.shape[0]
    pt, pk = np.stack([thin, 0.5 * thin]), np.stack([thick, 0.5 * thick])
    ht = np.stack([1e-11 * thin * np.linspace(1.0, 2.0, n), 2e-11 * thin])
    hk = np.stack([0.7e-11 * thick * np.linspace(2.0, 1.0, n), 1.5e-11 * thick])
    _fresh(p, c["N"], thin, thick)
    lib.spectra_to_device(pt, pk, ht, hk)
    kw = dict(thermal=ThermalParams(ht, hk), clumping=2.5, lls=LLSOpacity(0.05 / (cases.SIG * c["dr"]), 0.2),
              src_spectrum=np.array([0, 1], dtype=np.int32))
    per = _evolve(p, c, **kw)
    opn = _evolve(p, c, periodic=False, **kw)
    v = lib.last_raytrace_variant()
    assert v["open"] and not v["paired"], v
    assert lib.get_option(capi.OPT_OPEN_BOUNDARIES) == 0 and lib.get_lls_opacity() == (0.0, 0.0)
    assert per[0] == opn[0] >= 2
    for a, b in zip(per[1:], opn[1:]):
        assert np.array_equal(a, b)
    assert opn[3].max() > 1.05e4                                   # (the temperature moved: the heating rates arrived)
    plain = _evolve(p, c, periodic=False)
    assert not np.allclose(plain[1], opn[1], rtol=1e-3)           # (and the opt-ins matter)


# ---- 6. two ranks on one GPU -------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def test_two_ranks_on_the_slab_and_all_reduce_loops(asora, tmp_path):
    """evolve3D_MPI(periodic=False) on two ranks sharing GPU 0 over gloo: identical grids on both ranks, and the single-GPU
    evolve3D(periodic=False) to 1e-10 with the same iteration count.  Sources on the first and the last plane: the planes their
    periodic trace would wrap into belong to the other rank and arrive as zeros."""
    p, lib, capi = asora
    if p.cuda_is_init():
        p.device_close()
    world, port = 2, _free_port()
    outs = [str(tmp_path / f"r{r}.npz") for r in range(world)]
    env = dict(os.environ, PYC2RAY_AMD_NO_TORCH="0", OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_open_dist_worker.py"), str(r), str(world), port, outs[r]],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = [q.communicate(timeout=300)[0].decode() for q in procs]
    for q, log in zip(procs, logs):
        assert q.returncode == 0, log
    res = [np.load(o) for o in outs]
    import _open_dist_worker as W
    c = W.case()
    _fresh(p, c["N"], c["thin"], c["thick"])
    single = _evolve(p, c, periodic=False)
    per = _evolve(p, c)
    N = c["N"]
    for cell in ((N - 1, 6, 6), (0, 15, 15)):      # next to the sources on the first and the last plane, through the wrap only
        assert single[2][cell] == 0 and per[2][cell] > 0, cell
    for loop in W.LOOPS:
        for k in ("xh", "phi"):
            assert np.array_equal(res[0][f"{loop}_{k}"], res[1][f"{loop}_{k}"]), (loop, k)
        assert int(res[0][f"{loop}_niter"]) == int(res[1][f"{loop}_niter"]) == single[0], loop
        np.testing.assert_allclose(res[0][f"{loop}_xh"], single[1], rtol=1e-10, atol=0, err_msg=loop)
        assert np.array_equal(res[0][f"{loop}_phi"] != 0, single[2] != 0), loop
        np.testing.assert_allclose(res[0][f"{loop}_phi"], single[2], rtol=1e-10, atol=0, err_msg=loop)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def test_refused_combinations_launch_nothing_and_leave_the_library_working(asora):
    p, lib, capi = asora
    c = _case("n16")
    _setup(p, lib, capi, c)
    lib.grid_to_device(capi.GRID_XH, c["xh"])
    lib.grid_to_device(capi.GRID_TEMP, np.full((16, 16, 16), 1e4))
    good, _, _ = _trace(lib, capi, c)
    counts = lib.last_raytrace_counts()
    launches = lambda: lib.kernel_time_ms(0)[1]
    lib.set_option(capi.OPT_TIMING, 1)
    try:
        lib.kernel_time_reset()
        for opts, word in (({"OPT_GREY_NOTABLES": 1}, "grey"), ({"OPT_GLOBAL_ATOMICS": 1}, "ASORA_OPT_GLOBAL_ATOMICS")):
            with pytest.raises(RuntimeError, match=f"code 4.*open boundaries.*{word}"):
                _trace(lib, capi, c, opts=dict(opts, OPT_OPEN_BOUNDARIES=1))
            with pytest.raises(RuntimeError, match="code 4.*open boundaries"):
                try:
                    for k, v in dict(opts, OPT_OPEN_BOUNDARIES=1).items():
                        lib.set_option(getattr(capi, k), v)
                    lib.evolve_begin(cases.MYR, *CHEM, c["R"], cases.SIG, c["dr"], cases.MINLOGTAU, c["dlogtau"], c["thin"].shape[0], 0, 5,
                                     1.0, 1e-4)
                finally:
                    for k in dict(opts, OPT_OPEN_BOUNDARIES=1):
                        lib.set_option(getattr(capi, k), 0)
        lib.set_option(capi.OPT_OPEN_BOUNDARIES, 1)
        with pytest.raises(RuntimeError, match="code 4.*open boundaries.*column-density dump"):
            lib.debug_coldens(c["R"], cases.SIG, c["dr"], 0, 16)
        with pytest.raises(RuntimeError, match="code 4.*open boundaries.*sub-box"):
            lib.subbox_raytrace_device(1000, 3, 1e-2, 1000.0, cases.SIG, c["dr"], cases.MINLOGTAU, c["dlogtau"], c["thin"].shape[0] - 1,
                                       0, 5)
        from pyc2ray_amd.load_extensions import load_c2ray
        F = lambda a: np.asfortranarray(a)
        z = lambda: np.zeros((16, 16, 16), order="F")
        with pytest.raises(RuntimeError, match="code 4.*open boundaries.*sub-box"):
            load_c2ray().raytracing.do_all_sources(c["flux"], c["pos"], 1000, 3, z(), cases.SIG, c["dr"], F(c["ndens"]), F(c["xh"]), z(),
                                                   z(), 1e-2, c["thin"], c["thick"], 0 * c["thin"], 0 * c["thin"], cases.MINLOGTAU,
                                                   c["dlogtau"], 1000.0)
        lib.set_option(capi.OPT_OPEN_BOUNDARIES, 0)
        assert launches() == 0                                     # nothing of the above reached a raytrace launch
    finally:
        lib.set_option(capi.OPT_OPEN_BOUNDARIES, 0)
        lib.set_option(capi.OPT_TIMING, 0)
    # ... and nothing was zeroed or counted: the grids and counters of the last good call stand, and the next one repeats it
    assert lib.last_raytrace_counts() == counts
    again, _, _ = _trace(lib, capi, c)
    np.testing.assert_allclose(again, good, rtol=1e-12, atol=0)
    # the keyword with use_gpu=False never reaches the library
    with pytest.raises(ValueError, match="sub-box"):
        p.do_raytracing(c["dr"], c["flux"], c["pos"], False, 1000, 3, 1e-2, c["ndens"], c["xh"], c["thin"], c["thick"], None, None,
                        cases.MINLOGTAU, c["dlogtau"], 1000.0, cases.SIG, logfile=None, quiet=True, periodic=False)


def test_meshes_beyond_512_are_refused(asora):
    p, lib, capi = asora
    N = 513
    thin, thick, dlog = cases.soft_tables()
    lib.set_option(capi.OPT_PLACEMENT_CANDIDATES, 1)
    try:
        _fresh(p, N, thin, thick)
    finally:
        lib.set_option(capi.OPT_PLACEMENT_CANDIDATES, 0)
    lib.source_data_to_device(np.array([0, 0, 0], dtype=np.int32), np.array([1.0]), 1)
    try:
        lib.set_option(capi.OPT_OPEN_BOUNDARIES, 1)
        with pytest.raises(RuntimeError, match="code 4.*open boundaries.*N <= 512"):      # (said before anything about the grids)
            lib.raytrace_device(8.0, cases.SIG, 1e20, 0, 1, cases.MINLOGTAU, dlog, thin.shape[0] - 1)
    finally:
        lib.set_option(capi.OPT_OPEN_BOUNDARIES, 0)
        p.device_close()


# ---- 8. the simulation class -------------------------------------------------------------------------------------------------
def test_c2ray_class_with_the_yaml_key_and_the_attribute(asora, tmp_path):
    """C2Ray_Test with `Raytracing: periodic: 0`, one step at 24^3 with a source on the face i = 0: no rate in the planes its
    periodic trace wraps into, and the fields of the direct evolve3D(periodic=False) call; `sim.periodic = True` gives the
    periodic step."""
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N, R = 24, 6.0
        with open("src.txt", "w") as f:
            f.write("1\n1 12 13 5e50 1.0\n")
        with open("open.yml", "w") as f:
            f.write(open(PLAIN_PARAMS).read().rstrip("\n") + "\n  periodic: 0\n")
        runs = {}
        for key in ("open", "switched", "plain"):
            if p.cuda_is_init():
                p.device_close()
            sim = pc2r.C2Ray_Test(PLAIN_PARAMS if key == "plain" else "open.yml", N, True)
            assert sim.periodic == (key == "plain")
            if key == "switched":
                sim.periodic = True
            sim.R_max_LLS = R
            sim.density_init(sim.zred_0)
            srcpos, srcflux = sim.read_sources("src.txt", 1)
            dt = 1e7 * 3.15576e7
            before = [np.array(g) for g in (sim.temp, sim.ndens, sim.xh)]
            sim.evolve3D(dt, srcflux, srcpos)
            runs[key] = (np.array(sim.xh), np.array(sim.phi_ion))
            assert lib.get_option(capi.OPT_OPEN_BOUNDARIES) == 0
            if key == "open":
                assert "Open (non-periodic) boundaries" in open(sim.logfile).read()
                x, phi = p.evolve3D(dt, sim.dr, srcflux, srcpos, True, 1000, N, 1e-2, *before, sim.photo_thin_table,
                                    sim.photo_thick_table, sim.minlogtau, sim.dlogtau, R, sim.convergence_fraction, sim.sig, sim.bh00,
                                    sim.albpow, sim.colh0, sim.temph0, sim.abu_c, logfile=None, quiet=True, periodic=False)
                assert np.array_equal(x, runs[key][0]) and np.array_equal(phi, runs[key][1])
        m = int(R)
        phi_open, phi_plain = runs["open"][1], runs["plain"][1]
        assert np.all(phi_open[N - m:] == 0) and np.any(phi_plain[N - m:] > 0)
        assert phi_open[:m + 1].min() >= 0 and phi_open[0, 11, 12] > 0
        assert np.array_equal(runs["switched"][1], phi_plain) and np.array_equal(runs["switched"][0], runs["plain"][0])
    finally:
        if p.cuda_is_init():
            p.device_close()
        os.chdir(cwd)
