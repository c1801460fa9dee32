"""GPU: the plane-parallel flux through faces of the box -- asora_plane_flux and the ``plane_flux=``
keyword -- against the numpy restatement of tests/plane_flux_reference.py (itself checked against the oracle on the CPU,
tests/test_plane_flux_reference.py).  Meshes: N = 24 (a partial wave per row), 64 (exactly one wave per row), 67 (odd, prime, more
than one wave per row, with a tail).  The tolerances are those of the tests without the feature (tests/test_gpu_parity.py:
GAMMA_RTOL for a raytrace, 1e-8 / 1e-7 for a step)."""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import cases
import lls_reference as LR
import plane_flux_reference as PF
from evolve_oracle import evolve3D_oracle
from test_gpu_parity import GAMMA_RTOL

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHEM = (cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)
OPTS = ("OPT_HEATING", "OPT_GREY_NOTABLES", "OPT_OPEN_BOUNDARIES")
FLUX = 2.5
MESHES = (24, 64, 67)
#: 0-based source positions at N = 24 for R = 6: a corner, an edge, a face, inside, and a second face
SRC24 = np.array([(0, 0, 0), (23, 0, 10), (8, 15, 23), (12, 11, 12), (2, 20, 4)], dtype=np.int32)


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib, _capi
    lib.plane_flux((), ())
    for name in OPTS:
        lib.set_option(getattr(_capi, name), 0)
    lib.set_option(_capi.OPT_Z_TRANSPOSED, 1)
    lib.lls_opacity(0.0, 0.0)
    if p.cuda_is_init():
        lib.thermal_params(False)
        lib.clumping(0)
        p.device_close()


@functools.lru_cache(maxsize=None)
def _case(N, checkerboard=False):
    nd, xh, dr = PF.checkerboard_medium(N) if checkerboard else cases.grid(N, "lognormal", 3, 0.1)
    thin, thick, dlog = cases.soft_tables()
    n = thin.shape[0]
    c = dict(N=N, ndens=nd, xh=xh, dr=dr, thin=thin, thick=thick, dlogtau=dlog, n_abs=nd * (1.0 - xh),
             heat_thin=1e-11 * thin * np.linspace(1.0, 2.0, n), heat_thick=0.7e-11 * thick * np.linspace(2.0, 1.0, n))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _reference(N, face, checkerboard, numtau_minus, heat):
    """The restatement's trace of one face of a case, computed once and shared."""
    c = _case(N, checkerboard)
    kw = dict(heat_thin=c["heat_thin"], heat_thick=c["heat_thick"]) if heat else {}
    r = PF.plane_trace(face, FLUX, c["n_abs"], c["dr"], cases.SIG, c["thin"], c["thick"], cases.MINLOGTAU, c["dlogtau"],
                       NumTau=c["thin"].shape[0] - numtau_minus, **kw)
    for a in r:
        if a is not None:
            a.setflags(write=False)
    return r


def _fresh(p, N, thin, thick):
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)
    p.photo_table_to_device(thin, thick)


def _setup(p, lib, capi, c, heat=False, pos0=None, flux=None, ndens=None, xh=None):
    _fresh(p, c["N"], c["thin"], c["thick"])
    if heat:
        lib.heat_table_to_device(c["heat_thin"], c["heat_thick"], c["thin"].shape[0])
    _sources(lib, pos0, flux)
    lib.grid_to_device(capi.GRID_NDENS, c["ndens"] if ndens is None else ndens)
    lib.grid_to_device(capi.GRID_XH_AV, c["xh"] if xh is None else xh)


def _sources(lib, pos0=None, flux=None):
    if pos0 is None:
        lib.source_data_to_device(np.zeros(0, dtype=np.int32), np.zeros(0), 0)
    else:
        lib.source_data_to_device(np.ascontiguousarray(pos0.ravel()), flux, flux.shape[0])


def _trace(lib, capi, c, faces, nsrc=0, R=6.0, numtau_minus=1, heat=False, opts=None):
    """asora_raytrace_device of `nsrc` point sources with `faces` ((face, flux[, spectrum]) tuples) set; faces off and the options
    back to 0 afterwards.  (phi_ion, phi_heat)"""
    N = c["N"]
    opts = dict(opts or {})
    if heat:
        opts["OPT_HEATING"] = 1
    try:
        for k, v in opts.items():
            lib.set_option(getattr(capi, k), v)
        lib.plane_flux([PF.face_index(f[0]) for f in faces], [f[1] for f in faces], [f[2] if len(f) > 2 else 0 for f in faces])
        lib.raytrace_device(R, cases.SIG, c["dr"], 0, nsrc, cases.MINLOGTAU, c["dlogtau"], c["thin"].shape[0] - numtau_minus)
        phi = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
        h = lib.grid_to_host(capi.GRID_PHI_HEAT, np.empty((N, N, N))) if heat else None
    finally:
        lib.plane_flux((), ())
        for k in opts:
            lib.set_option(getattr(capi, k), 0)
    return phi, h


def _rel(got, ref):
    w = ref != 0
    return np.max(np.abs(got - ref)[w] / np.abs(ref[w])) if w.any() else 0.0


def _assert_matches(got, ref, tag, rtol=GAMMA_RTOL):
    print(tag, "max rel. difference", _rel(got, ref))
    assert np.all(np.isfinite(got)), tag
    assert np.array_equal(got != 0, ref != 0), tag
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=0, err_msg=tag)


# ---- 1. traces with no point sources against the restatement -----------------------------------------------------------------
@pytest.mark.parametrize("N", MESHES)
def test_each_face_against_the_reference(asora, N):
    """Six faces, NumTau = len - 1, no point source."""
    p, lib, capi = asora
    c = _case(N)
    _setup(p, lib, capi, c)
    for face in PF.FACES:
        phi, _ = _trace(lib, capi, c, [(face, FLUX)])
        assert lib.get_plane_flux() == []
        ref = _reference(N, face, False, 1, False)[0]
        assert ref.min() > 0
        _assert_matches(phi, ref, f"N={N} face {face}")


@pytest.mark.parametrize("N", MESHES)
def test_each_face_with_heating(asora, N):
    """Six faces with the heating tables (OPT_HEATING), NumTau = len."""
    p, lib, capi = asora
    c = _case(N)
    _setup(p, lib, capi, c, heat=True)
    for face in PF.FACES:
        phi, h = _trace(lib, capi, c, [(face, FLUX)], numtau_minus=0, heat=True)
        ref, ref_h = _reference(N, face, False, 0, True)
        _assert_matches(phi, ref, f"N={N} face {face} rates")
        _assert_matches(h, ref_h, f"N={N} face {face} heating")


@pytest.mark.parametrize("N", [24, 67])
def test_thin_and_thick_cells(asora, N):
    """The checkerboard of thin and thick cells (PF.checkerboard_medium), rates and heating, every face."""
    p, lib, capi = asora
    c = _case(N, True)
    _setup(p, lib, capi, c, heat=True)
    for face in PF.FACES:
        phi, h = _trace(lib, capi, c, [(face, FLUX)], numtau_minus=0, heat=True)
        ref, ref_h = _reference(N, face, True, 0, True)
        _assert_matches(phi, ref, f"N={N} face {face} rates")
        _assert_matches(h, ref_h, f"N={N} face {face} heating")


# ---- 2. symmetry and conservation on the device -------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [24, 67])
def test_faces_are_bit_identical_images_on_the_device(asora, N):
    """Each face on the input moved so that its march sees what the -x march sees: the same bits after moving back.  (+-z go
    through the [k][j][i] twins and the fold, which adds to exact zeros.)"""
    p, lib, capi = asora
    c = _case(N)
    _setup(p, lib, capi, c)
    base, _ = _trace(lib, capi, c, [("-x", FLUX)])
    for face in PF.FACES[1:]:
        nd, xh = np.empty((N, N, N)), np.empty((N, N, N))
        PF.to_march_order(nd, face)[...] = c["ndens"]
        PF.to_march_order(xh, face)[...] = c["xh"]
        lib.grid_to_device(capi.GRID_NDENS, nd)
        lib.grid_to_device(capi.GRID_XH_AV, xh)
        phi, _ = _trace(lib, capi, c, [(face, FLUX)])
        back = np.ascontiguousarray(PF.to_march_order(phi, face))
        print(f"N={N} face {face}: cells that differ from the -x image: {int((back != base).sum())}")
        assert np.array_equal(back, base), face


@pytest.mark.parametrize("N", [24, 67])
def test_photon_conservation_on_the_device(asora, N):
    """Per ray, sum phi n_abs dr = flux (T_thick(0) - T_thick(tau_total)) to 1e-9 relative on the all-thick medium (the bound:
    N eps_lookup / absorbed share = 67 x 1e-12 / 0.5 = 1.4e-10, rounded up; with the lookup reused it sits near 1e-14)."""
    p, lib, capi = asora
    c = _case(N)
    _setup(p, lib, capi, c)
    for face in PF.FACES:
        phi, _ = _trace(lib, capi, c, [(face, FLUX)], numtau_minus=0)
        absorbed = PF.absorbed_per_ray(phi, c["n_abs"], c["dr"], face)
        expected, share = PF.telescoped_per_ray(FLUX, c["n_abs"], c["dr"], cases.SIG, c["thick"], cases.MINLOGTAU, c["dlogtau"], face)
        worst = np.max(np.abs(absorbed - expected) / expected)
        print(f"N={N} face {face}: conservation {worst:.3e}, least absorbed share {share.min():.3f}")
        assert share.min() >= 0.5
        assert worst <= 1e-9


# ---- 3. with point sources ----------------------------------------------------------------------------------------------------
def test_superposition_with_point_sources(asora):
    """Five point sources (N = 24, R = 6) plus two faces in one call = the point-only trace + the face-only traces, to 1e-13
    (equal up to the order of the additions); the faces' contribution is the same bits with periodic and with open boundaries."""
    p, lib, capi = asora
    c = _case(24)
    flux = 3.0 * (1.0 + 0.25 * np.arange(len(SRC24)))
    _setup(p, lib, capi, c, pos0=SRC24, flux=flux)
    faces = [("-x", FLUX), ("+z", 0.5 * FLUX)]
    both, _ = _trace(lib, capi, c, faces, nsrc=5)
    points, _ = _trace(lib, capi, c, [], nsrc=5)
    fa, _ = _trace(lib, capi, c, faces[:1])
    fb, _ = _trace(lib, capi, c, faces[1:])
    assert (points != 0).sum() > 1000 and (points == 0).sum() > 1000
    total = points + fa + fb
    print("superposition: max rel. difference", _rel(both, total))
    np.testing.assert_allclose(both, total, rtol=1e-13, atol=0)
    two, _ = _trace(lib, capi, c, faces)
    two_open, _ = _trace(lib, capi, c, faces, opts={"OPT_OPEN_BOUNDARIES": 1})
    assert np.array_equal(two, two_open)
    both_open, _ = _trace(lib, capi, c, faces, nsrc=5, opts={"OPT_OPEN_BOUNDARIES": 1})
    points_open, _ = _trace(lib, capi, c, [], nsrc=5, opts={"OPT_OPEN_BOUNDARIES": 1})
    np.testing.assert_allclose(both_open, points_open + fa + fb, rtol=1e-13, atol=0)
    # the counters keep counting point-source pairs only
    _trace(lib, capi, c, faces, nsrc=5)
    with_faces = lib.last_raytrace_counts()
    _trace(lib, capi, c, [], nsrc=5)
    assert with_faces == lib.last_raytrace_counts() and with_faces[0] > 0


def test_lls_opacity_and_a_second_spectrum(asora):
    """With asora_lls_opacity the sweep sees n_abs; with two table sets on the device a face on set 1 takes set 1's tables."""
    p, lib, capi = asora
    c = _case(24)
    _setup(p, lib, capi, c)
    a, b = 0.05 / (cases.SIG * c["dr"]), 0.2
    lib.lls_opacity(a, b)
    try:
        phi, _ = _trace(lib, capi, c, [("+y", FLUX)])
    finally:
        lib.lls_opacity(0.0, 0.0)
    ref, _ = PF.plane_trace("+y", FLUX, LR.n_abs(c["ndens"], c["xh"], a, b), c["dr"], cases.SIG, c["thin"], c["thick"], cases.MINLOGTAU,
                            c["dlogtau"], NumTau=c["thin"].shape[0] - 1)
    _assert_matches(phi, ref, "lls, face +y")
    assert not np.allclose(ref, _reference(24, "+y", False, 1, False)[0], rtol=1e-3)
    thin2, thick2 = 0.5 * c["thin"] + 0.3 * c["thick"], 0.25 * c["thick"] + 0.2 * c["thin"]
    lib.spectra_to_device(np.stack([c["thin"], thin2]), np.stack([c["thick"], thick2]))
    for spectrum, (tn, tk) in enumerate(((c["thin"], c["thick"]), (thin2, thick2))):
        phi, _ = _trace(lib, capi, c, [("-z", FLUX, spectrum)])
        ref, _ = PF.plane_trace("-z", FLUX, c["n_abs"], c["dr"], cases.SIG, tn, tk, cases.MINLOGTAU, c["dlogtau"],
                                NumTau=tn.shape[0] - 1)
        _assert_matches(phi, ref, f"spectrum {spectrum}, face -z")
    # a spectrum the device does not hold: refused at use
    with pytest.raises(RuntimeError, match="code 4"):
        _trace(lib, capi, c, [("-z", FLUX, 2)])


# ---- 4. whole steps ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _step_case():
    N = 24
    nd, xh, dr = cases.grid(N, "lognormal", 61, 0.2, xlo=1e-4, xhi=2e-3)
    thin, thick, dlog = cases.soft_tables()
    n = thin.shape[0]
    src = np.array([(6, 7, 9), (15, 6, 18)], dtype=np.int32)
    c = dict(N=N, ndens=nd, xh=xh, dr=dr, temp=np.full((N, N, N), 1e4), pos=(src + 1).T.copy(), flux=np.full(len(src), 1.5e-4),
             thin=thin, thick=thick, dlogtau=dlog, R=6.0, dt=2 * cases.MYR, conv=1e-4,
             heat_thin=1e-11 * thin * np.linspace(1.0, 2.0, n), heat_thick=0.7e-11 * thick * np.linspace(2.0, 1.0, n),
             faces=(("-x", 3.0e-45), ("+z", 1.5e-45)))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def _plane_flux(c):
    from pyc2ray_amd.planeflux import PlaneFlux
    return [PlaneFlux(f, x) for f, x in c["faces"]]


def _evolve(p, c, sources=True, xh=None, R=None, **kw):
    flux, pos = (c["flux"], c["pos"]) if sources else (np.zeros(0), np.zeros((3, 0), dtype=int))
    out = p.evolve3D(c["dt"], c["dr"], flux, pos, True, 1000, c["N"], 1e-2, c["temp"], c["ndens"], c["xh"] if xh is None else xh,
                     c["thin"], c["thick"], cases.MINLOGTAU, c["dlogtau"], c["R"] if R is None else R, c["conv"], cases.SIG, *CHEM,
                     logfile=None, quiet=True, **kw)
    return (p.evolve._evolve.last_niter,) + tuple(np.array(a) for a in out)


def _oracle(c, sources=True, faces=None, R=None, **kw):
    flux, pos = (c["flux"], c["pos"]) if sources else (np.zeros(0), np.zeros((3, 0), dtype=int))
    return PF.evolve3D_plane_oracle(c["faces"] if faces is None else faces, c["dt"], c["dr"], flux, pos, c["temp"], c["ndens"], c["xh"],
                                    c["thin"], c["thick"], cases.MINLOGTAU, c["dlogtau"], c["R"] if R is None else R, c["conv"],
                                    cases.SIG, *CHEM, **kw)


def _assert_step(tag, niter, x, phi, ref):
    x_ref, phi_ref, niter_ref = ref[:3]
    print(tag, "niter", niter, niter_ref, "max rel. difference x", np.max(np.abs(x - x_ref) / x_ref), "phi", _rel(phi, phi_ref))
    assert niter == niter_ref and niter >= 2
    np.testing.assert_allclose(x, x_ref, rtol=1e-8, atol=0)
    assert np.array_equal(phi != 0, phi_ref != 0)
    np.testing.assert_allclose(phi, phi_ref, rtol=1e-7, atol=0)


@pytest.mark.parametrize("sources", [False, True])
def test_evolve3D_against_the_oracle_loop(asora, sources):
    """evolve3D(plane_flux=) with faces only (an empty source list) and with faces plus point sources."""
    p, lib, capi = asora
    c = _step_case()
    _fresh(p, c["N"], c["thin"], c["thick"])
    niter, x, phi = _evolve(p, c, sources, plane_flux=_plane_flux(c))
    assert lib.get_plane_flux() == []
    _assert_step(f"sources={sources}", niter, x, phi, _oracle(c, sources))
    print("mean x of the planes 0, 12 and of the box:", x[0].mean(), x[12].mean(), x.mean())
    assert x.max() > 0.5


def test_thermal_evolve3D_against_the_oracle_loop(asora):
    """evolve3D(plane_flux=, thermal=) with faces and point sources.  The heating tables are a hundredth of those of the other
    thermal tests: with the full ones this step's cells reach 4e6 K and the CPU loop itself answers a change of 1e-11 in the
    fluxes with 1 % in xh (whole j-planes: both faces' rays lie in them, and the iterations feed a cell's change to the cells
    behind it); with these it answers with 1.2e-10, and the temperature still rises to 5e4 K (faces alone) and 2e6 K."""
    p, lib, capi = asora
    import thermal_reference as TR
    from pyc2ray_amd.thermal import ThermalParams
    c = _step_case()
    ht, hk = 0.01 * c["heat_thin"], 0.01 * c["heat_thick"]
    _fresh(p, c["N"], c["thin"], c["thick"])
    prm = TR.Params(relative_denergy=0.1, t_floor=1.0, max_substeps=10000, cooling_mask=31, compton=False, t_cmb=0.0)
    tp = ThermalParams(ht, hk, relative_denergy=0.1, t_floor=1.0, max_substeps=10000, cooling=31, zred=None)
    niter, x, phi, T = _evolve(p, c, plane_flux=_plane_flux(c), thermal=tp)
    heat = lib.grid_to_host(capi.GRID_PHI_HEAT, np.empty((c["N"],) * 3))
    x_ref, phi_ref, niter_ref, _h, T_ref, heat_ref = _oracle(c, thermal_params=prm, heat_thin=ht, heat_thick=hk)
    _assert_step("thermal", niter, x, phi, (x_ref, phi_ref, niter_ref))
    print("max rel. difference T", _rel(T, T_ref), "heat", _rel(heat, heat_ref))
    np.testing.assert_allclose(T, T_ref, rtol=1e-8, atol=0)
    np.testing.assert_allclose(heat, heat_ref, rtol=1e-7, atol=0)
    assert T.max() > 1.05e4 and lib.get_plane_flux() == []


def reach_mask_steps(p):
    """A step without faces, one with, one without again, on one device state: [(niter, xh, phi_ion)] (also run by
    tests/_plane_flux_reach_worker.py)."""
    c = _step_case()
    _fresh(p, c["N"], c["thin"], c["thick"])
    return [_evolve(p, c, R=3.0), _evolve(p, c, R=3.0, plane_flux=_plane_flux(c)), _evolve(p, c, R=3.0)]


@pytest.mark.parametrize("mask", ["default", "forced"])
def test_reach_mask_steps_around_a_step_with_faces(asora, tmp_path, mask):
    """Two sources with R = 3 at 24^3: a step without faces, one with, one without again, each against its oracle -- the switch
    leaves no rates behind on lines the mask skips.  default: the library decides about the reach mask of the fused pass itself
    (here the two spheres reach a small share of the lines, far below the 55 % up to which it is used).  forced: a child process with
    ASORA_REACH_MASK=2, where the mask is in use in every step without faces whatever that decision would be."""
    p, lib, capi = asora
    c = _step_case()
    if mask == "default":
        steps = reach_mask_steps(p)
    else:
        if p.cuda_is_init():
            p.device_close()
        out = str(tmp_path / "reach.npz")
        q = subprocess.run([sys.executable, os.path.join(HERE, "_plane_flux_reach_worker.py"), out],
                           env=dict(os.environ, ASORA_REACH_MASK="2"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert q.returncode == 0, q.stdout.decode()
        r = np.load(out)
        assert str(r["mode"]) == "2"
        steps = [(int(r[f"niter{k}"]), r[f"xh{k}"], r[f"phi{k}"]) for k in range(3)]
    plain_ref = evolve3D_oracle(c["dt"], c["dr"], c["flux"], c["pos"], c["temp"], c["ndens"], c["xh"], c["thin"], c["thick"],
                                cases.MINLOGTAU, c["dlogtau"], 3.0, c["conv"], cases.SIG, *CHEM)
    for tag, (niter, x, phi), ref in zip(("before", "with faces", "after"), steps, (plain_ref, _oracle(c, R=3.0), plain_ref)):
        _assert_step(f"{mask}: {tag}", niter, x, phi, ref)
    assert (steps[2][2] == 0).sum() > c["N"] ** 3 // 2


def test_planar_ionisation_front(asora):
    """The ten steps of the CPU test's planar front through evolve3D, each from the reference's previous state: xh per step to the
    step tolerance with equal iteration counts, so the analytic check of tests/test_plane_flux_reference.py carries over."""
    from pyc2ray_amd.planeflux import PlaneFlux
    p, lib, capi = asora
    c = PF.ifront_case()
    _fresh(p, c["N"], c["thin"], c["thick"])
    xh = c["xh0"]
    for s, (x_ref, phi_ref, niter_ref) in enumerate(PF.ifront_reference()):
        x, phi = p.evolve3D(c["dt"], c["dr"], np.zeros(0), np.zeros((3, 0), dtype=int), True, 1000, c["N"], 1e-2, c["temp"], c["ndens"],
                            xh, c["thin"], c["thick"], cases.MINLOGTAU, c["dlogtau"], 1000.0, c["convergence_fraction"], cases.SIG,
                            *CHEM, logfile=None, quiet=True, plane_flux=PlaneFlux("-x", c["flux"]))
        niter = p.evolve._evolve.last_niter
        print(f"step {s + 1}: niter {niter} {niter_ref}, max rel. difference x {np.max(np.abs(x - x_ref) / x_ref):.3e}")
        assert niter == niter_ref
        np.testing.assert_allclose(x, x_ref, rtol=1e-8, atol=0)
        xh = x_ref


# ---- 5. two ranks on one GPU -------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def test_two_ranks_share_the_sources_and_rank_zero_holds_the_faces(asora, tmp_path):
    """evolve3D_MPI(plane_flux=) on two ranks sharing GPU 0 over gloo -- a communicator set up for the slab exchange (it runs the
    all-reduce device loop), the all-reduce device loop, the three-call loop: identical grids on both ranks, and the single-GPU
    evolve3D(plane_flux=) to 1e-10 with the same iteration count."""
    from pyc2ray_amd.planeflux import PlaneFlux
    p, lib, capi = asora
    if p.cuda_is_init():
        p.device_close()
    world, port = 2, _free_port()
    outs = [str(tmp_path / f"r{r}.npz") for r in range(world)]
    env = dict(os.environ, PYC2RAY_AMD_NO_TORCH="0", OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_plane_flux_dist_worker.py"), str(r), str(world), port, outs[r]],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = [q.communicate(timeout=300)[0].decode() for q in procs]
    for q, log in zip(procs, logs):
        assert q.returncode == 0, log
    res = [np.load(o) for o in outs]
    import _plane_flux_dist_worker as W
    c = W.case()
    _fresh(p, c["N"], c["thin"], c["thick"])
    single = _evolve(p, c, plane_flux=[PlaneFlux(f, x) for f, x in c["faces"]])
    without = _evolve(p, c)
    assert single[0] >= 2 and single[1].mean() > 1.5 * without[1].mean()                 # (the faces matter in this case)
    for loop in W.LOOPS:
        for k in ("xh", "phi"):
            assert np.array_equal(res[0][f"{loop}_{k}"], res[1][f"{loop}_{k}"]), (loop, k)
        print(loop, "niter", int(res[0][f"{loop}_niter"]), single[0], "max rel. difference x",
              np.max(np.abs(res[0][f"{loop}_xh"] - single[1]) / single[1]), "phi", _rel(res[0][f"{loop}_phi"], single[2]))
        assert int(res[0][f"{loop}_niter"]) == int(res[1][f"{loop}_niter"]) == single[0], loop
        np.testing.assert_allclose(res[0][f"{loop}_xh"], single[1], rtol=1e-10, atol=0, err_msg=loop)
        np.testing.assert_allclose(res[0][f"{loop}_phi"], single[2], rtol=1e-10, atol=0, err_msg=loop)


def test_world1_rccl_step_with_faces_equals_the_one_gpu_step(asora, tmp_path):
    """The all-reduce device loop over backend nccl (= RCCL) on one rank, as a child process, once with a communicator set up for
    the slab exchange (it falls back to the all-reduce loop): several iterations are enqueued per poll (evolve._next_batch, up to
    eight), so the sweep ahead of each iteration's first trace is stream-ordered behind the previous iteration and gated by the
    device's `done` flag like the rest of the loop, and the out-box with the faces' rates is all-reduced in place (forced: PYC2RAY_AMD_FORCE_COLLECTIVE).  The one-GPU evolve3D(plane_flux=) step of
    the same process to 1e-10, equal iteration counts."""
    p, lib, capi = asora
    if p.cuda_is_init():
        p.device_close()
    out = str(tmp_path / "w1.npz")
    env = dict(os.environ, PYC2RAY_AMD_NO_TORCH="0", OMP_NUM_THREADS="1", PYC2RAY_AMD_FORCE_COLLECTIVE="1")
    q = subprocess.run([sys.executable, os.path.join(HERE, "_plane_flux_dist_worker.py"), "0", "1", _free_port(), out, "nccl"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert q.returncode == 0, q.stdout.decode()
    r = np.load(out)
    assert int(r["one_niter"]) >= 2
    for loop in ("slab", "allreduce"):
        print(loop, "niter", int(r[f"{loop}_niter"]), int(r["one_niter"]), "max rel. difference x",
              np.max(np.abs(r[f"{loop}_xh"] - r["one_xh"]) / r["one_xh"]), "phi", _rel(r[f"{loop}_phi"], r["one_phi"]))
        assert int(r[f"{loop}_niter"]) == int(r["one_niter"]), loop
        np.testing.assert_allclose(r[f"{loop}_xh"], r["one_xh"], rtol=1e-10, atol=0, err_msg=loop)
        np.testing.assert_allclose(r[f"{loop}_phi"], r["one_phi"], rtol=1e-10, atol=0, err_msg=loop)


# ---- 6. refusals, and off is off ---------------------------------------------------------------------------------------------
def test_an_existing_open_boundary_trace_keeps_its_bits_around_a_face_call(asora):
    """The one-source n16 open-boundary trace of tests/test_gpu_open_boundaries.py (one source: no two atomics meet in a cell, so
    it is deterministic) before and after a trace with faces in the same process: the same bits, and the open-boundary reference."""
    import test_gpu_open_boundaries as OBT
    p, lib, capi = asora
    c16 = OBT._case("n16")
    OBT._setup(p, lib, capi, c16)
    before, _, _ = OBT._trace(lib, capi, c16, nsrc=1, opts={"OPT_OPEN_BOUNDARIES": 1})
    OBT._assert_matches(before, OBT._reference("n16", 1, 1, False)["phi_ion"], "one corner source, before")
    lib.plane_flux([1, 4], [FLUX, 0.5 * FLUX])
    try:
        lib.raytrace_device(c16["R"], cases.SIG, c16["dr"], 0, 5, cases.MINLOGTAU, c16["dlogtau"], c16["thin"].shape[0] - 1)
        with_faces = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((16, 16, 16)))
    finally:
        lib.plane_flux((), ())
    assert with_faces.min() > 0                                    # (the faces reach every cell)
    after, _, _ = OBT._trace(lib, capi, c16, nsrc=1, opts={"OPT_OPEN_BOUNDARIES": 1})
    assert np.array_equal(after, before)


def test_refusals_and_off_is_off(asora):
    from pyc2ray_amd.planeflux import PlaneFlux
    p, lib, capi = asora
    c = _case(24)
    flux = 3.0 * (1.0 + 0.25 * np.arange(len(SRC24)))
    _setup(p, lib, capi, c, pos0=SRC24, flux=flux)
    lib.grid_to_device(capi.GRID_XH, c["xh"])
    lib.grid_to_device(capi.GRID_TEMP, np.full((24, 24, 24), 1e4))
    _trace(lib, capi, c, [], nsrc=5)
    counts = lib.last_raytrace_counts()
    launches = lambda: lib.kernel_time_ms(capi.KERNEL_RAYTRACE)[1]
    # what the setter refuses (code 3) leaves the setting alone
    for bad in (([6], [1.0]), ([0, 0], [1.0, 1.0]), ([0], [-1.0]), ([0], [np.inf]), ([-1], [1.0])):
        with pytest.raises(RuntimeError, match="code 3"):
            lib.plane_flux(*bad)
        assert lib.get_plane_flux() == []
    assert lib.last_raytrace_counts() == counts
    lib.plane_flux([4, 1], [2.0, 3.0], [0, 0])
    assert lib.get_plane_flux() == [(4, 2.0, 0), (1, 3.0, 0)]
    lib.set_option(capi.OPT_TIMING, 1)
    lib.kernel_time_reset()
    try:
        # grey opacity, the dump, both sub-box entries: code 4, nothing launched
        lib.set_option(capi.OPT_GREY_NOTABLES, 1)
        with pytest.raises(RuntimeError, match="code 4"):
            lib.raytrace_device(6.0, cases.SIG, c["dr"], 0, 5, cases.MINLOGTAU, c["dlogtau"], c["thin"].shape[0])
        lib.set_option(capi.OPT_GREY_NOTABLES, 0)
        with pytest.raises(RuntimeError, match="code 4"):
            lib.debug_coldens(6.0, cases.SIG, c["dr"], 0, c["N"])
        with pytest.raises(RuntimeError, match="code 4"):
            lib.subbox_raytrace_device(1000, 3, 1e-2, 1000.0, cases.SIG, c["dr"], cases.MINLOGTAU, c["dlogtau"], c["thin"].shape[0], 0, 5)
        zeros = np.zeros_like(c["thin"])
        with pytest.raises(RuntimeError, match="code 4"):
            pos1 = (SRC24 + 1).T.copy()
            p.load_extensions.load_c2ray().raytracing.do_all_sources(
                flux, pos1, 1000, 3, np.zeros((24,) * 3, order="F"), cases.SIG, c["dr"], np.asfortranarray(c["ndens"]),
                np.asfortranarray(c["xh"]), np.zeros((24,) * 3, order="F"), np.zeros((24,) * 3, order="F"), 1e-2, c["thin"], c["thick"],
                zeros, zeros, cases.MINLOGTAU, c["dlogtau"], 1000.0)
        # heating without heating tables
        lib.set_option(capi.OPT_HEATING, 1)
        with pytest.raises(RuntimeError, match="code 4"):
            lib.raytrace_device(6.0, cases.SIG, c["dr"], 0, 5, cases.MINLOGTAU, c["dlogtau"], c["thin"].shape[0])
        lib.set_option(capi.OPT_HEATING, 0)
        # a z face without the [k][j][i] twins (an x face alone is fine there, below)
        lib.set_option(capi.OPT_Z_TRANSPOSED, 0)
        with pytest.raises(RuntimeError, match="code 4.*z face"):
            lib.raytrace_device(6.0, cases.SIG, c["dr"], 0, 5, cases.MINLOGTAU, c["dlogtau"], c["thin"].shape[0])
        with pytest.raises(RuntimeError, match="code 4.*z face"):
            lib.evolve_begin(2 * cases.MYR, *CHEM, 6.0, cases.SIG, c["dr"], cases.MINLOGTAU, c["dlogtau"], c["thin"].shape[0], 0, 5, 0.0, 1e-4)
        lib.set_option(capi.OPT_Z_TRANSPOSED, 1)
        # a sharded step that owns only some of the planes: the slab exchange does not deliver a whole-box sweep
        with pytest.raises(RuntimeError, match="code 4.*owns every plane"):
            lib.evolve_begin_slab(2 * cases.MYR, *CHEM, 6.0, cases.SIG, c["dr"], cases.MINLOGTAU, c["dlogtau"], c["thin"].shape[0], 0, 5,
                                  0.0, 1e-4, 0, 12)
        assert launches() == 0                                     # nothing of the above reached a launch, sweep or raytrace
        assert lib.last_raytrace_counts() == counts                # ... nor zeroed the counters of the last good call
        lib.evolve_begin_slab(2 * cases.MYR, *CHEM, 6.0, cases.SIG, c["dr"], cases.MINLOGTAU, c["dlogtau"], c["thin"].shape[0], 0, 5,
                              0.0, 1e-4, 0, 24)                    # (owning every plane: accepted)
    finally:
        lib.set_option(capi.OPT_GREY_NOTABLES, 0)
        lib.set_option(capi.OPT_HEATING, 0)
        lib.set_option(capi.OPT_Z_TRANSPOSED, 1)
        lib.set_option(capi.OPT_TIMING, 0)
        lib.plane_flux((), ())
    # without the twins an x face alone is swept as with them
    with_twins, _ = _trace(lib, capi, c, [("+x", FLUX)])
    lib.set_option(capi.OPT_Z_TRANSPOSED, 0)
    try:
        without_twins, _ = _trace(lib, capi, c, [("+x", FLUX)])
    finally:
        lib.set_option(capi.OPT_Z_TRANSPOSED, 1)
    assert np.array_equal(with_twins, without_twins)
    # use_gpu=False never reaches the library
    kw = dict(logfile=None, quiet=True)
    pos1 = (SRC24 + 1).T.copy()
    with pytest.raises(ValueError, match="use_gpu=True"):
        p.do_raytracing(c["dr"], flux, pos1, False, 1000, 3, 1e-2, c["ndens"], c["xh"], c["thin"], c["thick"], None, None,
                        cases.MINLOGTAU, c["dlogtau"], 1000.0, cases.SIG, plane_flux=PlaneFlux("-x", 1.0), **kw)
    # plane_flux=None and [] are the call without the keyword
    zeros = np.zeros_like(c["thin"])
    one = SRC24[3:4]
    args = (c["dr"], flux[:1], (one + 1).T.copy(), True, 1000, 24, 1e-2, c["ndens"], c["xh"], c["thin"], c["thick"], zeros, zeros,
            cases.MINLOGTAU, c["dlogtau"], 6.0, cases.SIG)
    plain = p.do_raytracing(*args, **kw)[0]
    for off in (None, [], ()):
        assert np.array_equal(p.do_raytracing(*args, plane_flux=off, **kw)[0], plain)
    with_face = p.do_raytracing(*args, plane_flux=[PlaneFlux("-y", FLUX)], **kw)[0]
    ref = _reference(24, "-y", False, 0, False)[0]
    np.testing.assert_allclose(with_face - plain, ref, rtol=1e-6, atol=0)
    assert lib.get_plane_flux() == []
