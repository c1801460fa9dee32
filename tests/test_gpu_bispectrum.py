"""GPU: the bispectrum (asora_bispectrum, pyc2ray_amd.bispectrum, C2Ray.bispectrum) against an answer with no
transform in it, against the direct sum over closed triples and against the numpy FFT route (tests/bispectrum_reference.py).  Every
call is made twice and compared byte for byte.

The tolerance is derived, not tuned; tests/bispectrum_reference.py carries the derivation.  With E = 2.5 c(N) ||g||_2 the bound of
a shell field's error in the 2-norm (the smoothing's bound with max |W| = 1; c(N) of tests/powerspec_reference.py),

    |sum_ggg - exact| <= N^6 ( E (||d_b d_c|| + ||d_a d_c|| + ||d_a d_b||) + E^2 (max|d_a| + max|d_b| + max|d_c|) + E^3
                               + 5 eps sum |d_a d_b d_c| ),

the norms from the reference's cubes; for sum_iii the same with the indicator's cubes and ||g||_2 = 1.  Every test prints the
largest share of the bound it uses.

* Meshes of the shell inverse: 17, 30, 43, 64, 96 (generic butterfly, mixed radices, odd and even) with six shells, two of them
  pruned to a few columns and one reaching the Nyquist plane; 121, 169, 273 of tests/fft_meshes.py with two shells: a pruned one
  (28 columns: a tail tile at 16 and at 8 lines per workgroup) and one that reaches floor(N/2) and is not pruned at all (the tail
  tile of the full pass at 16, 8 and 4 lines).
* The product kernel's edges come from asora_debug_bispectrum_plan: chunk - 1, chunk, chunk + 1 and a prime number of triangles (one,
  two and three passes, waves with unequal and with no triangles), N = 30 (part of the fixed grid takes no tile) and N = 72 (workgroups
  with three tiles and with two)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import bispectrum_reference as BR
import powerspec_reference as PR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POWER_PARAMS = os.path.join(HERE, "data", "parameters_power_spectrum.yml")
KEYS = ("sum_ggg", "sum_iii", "count", "sum_k", "sum_aa", "moments")


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib, _capi
    if p.cuda_is_init():
        p.device_close()


def _mesh(asora, N):
    p, lib, capi = asora
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)


def _twice(lib, *args):
    got, again = lib.bispectrum(*args), lib.bispectrum(*args)
    for key in KEYS:
        assert got[key].tobytes() == again[key].tobytes(), key
    return got


def _bounds(N, ref, tri, g):
    """the derived bounds of sum_ggg and sum_iii for every triangle; the norms from the cubes of `ref`"""
    return BR.bound(N, ref["d"], tri, np.linalg.norm(np.ravel(g))), BR.bound(N, ref["i"], tri, 1.0)


def _check(what, N, got, tri, want_ggg, want_iii, ref, g, bounds=None):
    """sum_ggg and sum_iii within the derived bound of `want_*`"""
    b_g, b_i = _bounds(N, ref, tri, g) if bounds is None else bounds
    share_g = float(np.max(np.abs(got["sum_ggg"] - want_ggg) / b_g))
    share_i = float(np.max(np.abs(got["sum_iii"] - want_iii) / b_i))
    resid = float(np.max(np.abs(got["sum_iii"] - np.rint(got["sum_iii"]))))
    print(f"{what}: sum_ggg uses {share_g:.3e} of its bound, sum_iii {share_i:.3e}; count residual {resid:.3e}")
    assert share_g <= 1.0 and share_i <= 1.0, (what, share_g, share_i)
    return share_g, share_i


def _shells_to_nyquist(N):
    edges = np.arange(0, N // 2 + 1) + 0.5
    return edges, PR.thresholds_of(edges)


def test_three_waves(asora):
    """1. The known answer with no transform in it: three cosines that close, N = 12."""
    p, lib, capi = asora
    N = 12
    _mesh(asora, N)
    A, phi = (1.3, 0.7, 2.1), (0.4, -1.1, 2.5)
    thr = PR.thresholds_of(np.arange(0, 5) + 0.5)
    tri = np.array([(a, b, c) for a in range(4) for b in range(4) for c in range(4)], dtype=np.int32)
    want = 2.0 * (N ** 3 / 2.0) ** 3 * A[0] * A[1] * A[2] * math.cos(sum(phi))
    for flip, sign in ((0.0, 1.0), (math.pi, -1.0)):
        g = BR.three_waves(N, A, (phi[0] + flip, phi[1], phi[2]))
        lib.grid_to_device(capi.GRID_XH, g)
        got = _twice(lib, capi.PS_XH, 1.0, 0.0, thr, tri)
        ref = BR.fft_route(g, thr, tri)
        exact = np.array([sign * want if sorted(t) == [0, 1, 2] else 0.0 for t in tri.tolist()])
        _check(f"three waves, phase + {flip:.2f}", N, got, tri, exact, ref["sum_iii"], ref, g)
        t012 = tri.tolist().index([0, 1, 2])
        print(f"sum_ggg(0, 1, 2) = {got['sum_ggg'][t012]:.6e}, exact {sign * want:.6e}")


@pytest.mark.parametrize("N", (6, 8, 9, 12))
def test_direct_sum(asora, N):
    """2. Every triangle a <= b <= c of shells up to the Nyquist mode against the direct sum over ordered closed triples modulo N;
    the counts exactly."""
    p, lib, capi = asora
    _mesh(asora, N)
    g = PR.noise_with_block(N, 7000 + N)
    lib.grid_to_device(capi.GRID_XH, g)
    edges, thr = _shells_to_nyquist(N)
    tri = BR.all_triangles(edges)
    G, Cn = BR.direct_sums(g, thr)
    want_g = np.array([G[a, b, c].real for a, b, c in tri])
    want_c = np.array([Cn[a, b, c] for a, b, c in tri])
    got = _twice(lib, capi.PS_XH, 1.0, 0.0, thr, tri)
    ref = BR.fft_route(g, thr, tri)
    _check(f"N {N}, direct sum, {len(tri)} triangles", N, got, tri, want_g, want_c.astype(np.float64), ref, g)
    assert np.array_equal(np.rint(got["sum_iii"]).astype(np.int64), want_c)
    assert float(np.max(np.abs(got["sum_iii"] - np.rint(got["sum_iii"])))) < 0.5
    assert np.array_equal(lib.grid_to_host(capi.GRID_XH, np.empty((N, N, N))), g)             # no grid is written


def _six_shells(N):
    h = N // 2
    return np.array([0.5, 1.5, 2.5, max(3.5, 0.35 * h), 0.6 * h, 0.85 * h, h + 0.5])


@pytest.mark.parametrize("N", (17, 30, 43, 64, 96))
def test_shell_inverse_against_numpy(asora, N):
    """3. The numpy FFT route on the brightness temperature with the spin factor: six shells, every triangle that can close."""
    p, lib, capi = asora
    _mesh(asora, N)
    rng = np.random.default_rng(900 + N)
    x = np.clip(0.5 + 0.25 * PR.noise_with_block(N, 3000 + N), 0.0, 1.0)
    n = 1e-4 * np.exp(0.7 * rng.normal(size=(N, N, N)))
    T = 200.0 + 2e4 * rng.random((N, N, N))
    for which, grid in ((capi.GRID_XH, x), (capi.GRID_NDENS, n), (capi.GRID_TEMP, T)):
        lib.grid_to_device(which, grid)
    edges = _six_shells(N)
    thr = PR.thresholds_of(edges)
    tri = BR.all_triangles(edges)
    g = lib.power_spectrum(capi.PS_HI, None, 27.3, 30.0, thr, field=True)["field"]          # (tests/test_gpu_powerspec.py checks the forming)
    got = _twice(lib, capi.PS_HI, 27.3, 30.0, thr, tri)
    ref = BR.fft_route(g, thr, tri)
    _check(f"N {N}, {len(tri)} triangles", N, got, tri, ref["sum_ggg"], ref["sum_iii"], ref, g)


@pytest.mark.parametrize("N", (121, 169, 273))
def test_shell_inverse_at_the_tail_tiles(asora, N):
    """3. Two shells at the meshes with tail tiles at 16, 8 and 4 lines per workgroup: [1.5, 3.5) is pruned to 7 x 4 columns, the
    other reaches floor(N/2) and is transformed in full."""
    p, lib, capi = asora
    _mesh(asora, N)
    g = PR.noise_with_block(N, 4000 + N)
    lib.grid_to_device(capi.GRID_XH, g)
    h = N // 2
    thr = np.array([3, 13, (h - 2) ** 2, h * h + 1], dtype=np.uint32)       # shell 1 lies between the two and is used by no triangle
    tri = np.array([(0, 0, 0), (0, 0, 2), (2, 0, 2), (2, 2, 2)], dtype=np.int32)
    got = _twice(lib, capi.PS_XH, 1.0, 0.0, thr, tri)
    ref = BR.fft_route(g, thr, tri)
    _check(f"N {N}, two shells", N, got, tri, ref["sum_ggg"], ref["sum_iii"], ref, g)


def test_product_kernel_edges(asora):
    """4. Triangle counts around the chunk, repeated shells, an unsorted list with duplicates, an empty shell; N = 72: workgroups
    with unequal trips."""
    p, lib, capi = asora
    N = 72
    _mesh(asora, N)
    g = PR.noise_with_block(N, 72)
    lib.grid_to_device(capi.GRID_XH, g)
    thr = np.array([1, 3, 7, 7, 40, 36 * 36 + 1], dtype=np.uint32)         # shell 2 is empty
    ns = thr.size - 1
    every = np.array([(a, b, c) for a in range(ns) for b in range(ns) for c in range(ns)], dtype=np.int32)
    ref = BR.fft_route(g, thr, every)
    b_g, b_i = _bounds(N, ref, every, g)
    index = {tuple(t): q for q, t in enumerate(every.tolist())}
    plan = lib.bispectrum_plan(N, ns, 1)
    chunk = plan["chunk"]
    assert plan["trips_max"] == plan["trips_min"] + 1 and plan["idle_workgroups"] == 0 and plan["workgroups"] * plan["tile_cells"] < N ** 3
    rng = np.random.default_rng(4)
    for n_tri in (chunk - 1, chunk, chunk + 1, 2 * chunk + 1, 1):
        pick = rng.integers(0, len(every), n_tri)
        pick[:min(n_tri, 3)] = [index[(1, 1, 1)], index[(1, 1, 4)], index[(4, 0, 3)]][:min(n_tri, 3)]
        if n_tri > 10:
            pick[-1] = pick[5] = pick[0]                               # duplicates, in the first and in the last pass
        tri = every[pick]
        assert lib.bispectrum_plan(N, ns, n_tri)["passes"] == -(-n_tri // chunk)
        got = _twice(lib, capi.PS_XH, 1.0, 0.0, thr, tri)
        _check(f"N {N}, {n_tri} triangles", N, got, tri, ref["sum_ggg"][pick], ref["sum_iii"][pick], ref, g, (b_g[pick], b_i[pick]))
        empty = np.any(tri == 2, axis=1)
        assert np.all(got["sum_ggg"][empty] == 0.0) and np.all(got["sum_iii"][empty] == 0.0)
        assert got["count"][2] == 0 and got["sum_aa"][2] == 0.0
        if n_tri > 10:
            for key in ("sum_ggg", "sum_iii"):
                assert got[key][0].tobytes() == got[key][5].tobytes() == got[key][-1].tobytes(), key
    assert 2 * chunk + 1 == 257                                        # (a prime number of triangles)


def test_thirty_two_shells(asora):
    """4. 32 shells, all the ABI allows, at N = 30, where part of the product kernel's fixed grid takes no tile; 200 triangles
    drawn at random, in any order."""
    p, lib, capi = asora
    N = 30
    _mesh(asora, N)
    g = PR.noise_with_block(N, 30)
    lib.grid_to_device(capi.GRID_XH, g)
    thr = PR.thresholds_of(np.linspace(0.5, 15.5, 33))
    assert thr.size == 33 and lib.bispectrum_plan(N, 32, 200)["idle_workgroups"] > 0
    tri = np.random.default_rng(32).integers(0, 32, (200, 3)).astype(np.int32)
    tri[0] = (31, 31, 31)
    tri[1] = (0, 31, 31)
    got = _twice(lib, capi.PS_XH, 1.0, 0.0, thr, tri)
    ref = BR.fft_route(g, thr, tri)
    _check(f"N {N}, 32 shells", N, got, tri, ref["sum_ggg"], ref["sum_iii"], ref, g)


def test_shell_sums_are_the_power_spectrums(asora):
    """5. count, sum_k, sum_aa and moments are the power spectrum's bytes; the power spectrum and the smoothing return their earlier
    bytes after a bispectrum call; no grid is written."""
    p, lib, capi = asora
    N = 30
    _mesh(asora, N)
    rng = np.random.default_rng(5)
    x, n = rng.random((N, N, N)), 1e-4 * np.exp(0.7 * rng.normal(size=(N, N, N)))
    lib.grid_to_device(capi.GRID_XH, x)
    lib.grid_to_device(capi.GRID_NDENS, n)
    edges = _six_shells(N)
    thr = PR.thresholds_of(edges)
    tri = BR.all_triangles(edges)
    ps = lib.power_spectrum(capi.PS_HI, None, 27.3, 0.0, thr)
    w_r = np.zeros(3 * (N // 2) ** 2 + 1)
    w_r[thr[1]:thr[2]] = 1.0
    sm = lib.smooth_field(capi.PS_HI, 27.3, 0.0, w_r=w_r, field=True)
    got = _twice(lib, capi.PS_HI, 27.3, 0.0, thr, tri)
    for key, other in (("count", "count"), ("sum_k", "sum_k"), ("sum_aa", "sum_aa"), ("moments", "moments_a")):
        assert got[key].tobytes() == ps[other].tobytes(), key
    after = lib.power_spectrum(capi.PS_HI, None, 27.3, 0.0, thr)
    for key in ("count", "sum_k", "sum_aa", "moments_a"):
        assert after[key].tobytes() == ps[key].tobytes(), key
    sm_after = lib.smooth_field(capi.PS_HI, 27.3, 0.0, w_r=w_r, field=True)
    assert sm_after["field"].tobytes() == sm["field"].tobytes() and sm_after["stats"].tobytes() == sm["stats"].tobytes()
    # the shell field of the header is the smoothing's for that table: sum_ggg of (1, 1, 1) from its cube, within the bound
    d = sm["field"]
    want = float(np.sum((d * d) * d, dtype=np.longdouble)) * float(N) ** 6
    t = tri.tolist().index([1, 1, 1])
    g = lib.power_spectrum(capi.PS_HI, None, 27.3, 0.0, thr, field=True)["field"]
    ref = BR.fft_route(g, thr, tri[t:t + 1])
    b = BR.bound(N, ref["d"], tri[t:t + 1], np.linalg.norm(g.ravel()))[0]
    print(f"sum_ggg(1, 1, 1) from the smoothing's cube uses {abs(got['sum_ggg'][t] - want) / (2.0 * b):.3e} of twice the bound")
    assert abs(got["sum_ggg"][t] - want) <= 2.0 * b                    # (two computed cubes, each within the bound of the exact one)
    assert np.array_equal(lib.grid_to_host(capi.GRID_XH, np.empty((N, N, N))), x)
    assert np.array_equal(lib.grid_to_host(capi.GRID_NDENS, np.empty((N, N, N))), n)


def test_count_cache(asora):
    """6. A second call with the same (N, thresholds, tri) returns the kept counts -- count-stage times 0, the same bytes --, whatever
    the field; a changed threshold, a changed triangle and another mesh recompute."""
    p, lib, capi = asora
    N = 30
    _mesh(asora, N)
    rng = np.random.default_rng(6)
    lib.grid_to_device(capi.GRID_XH, rng.random((N, N, N)))
    edges = _six_shells(N)
    thr = PR.thresholds_of(edges)
    tri = BR.all_triangles(edges)
    lib.set_option(capi.OPT_TIMING, 1)
    try:
        thr0 = thr.copy()
        thr0[-1] += 1
        lib.bispectrum(capi.PS_XH, 1.0, 0.0, thr0, tri)                 # (whatever was kept before is not this)
        first = lib.bispectrum(capi.PS_XH, 1.0, 0.0, thr, tri)
        ms_first = lib.bispectrum_ms()
        lib.grid_to_device(capi.GRID_XH, rng.random((N, N, N)))
        second = lib.bispectrum(capi.PS_XH, 1.0, 0.0, thr, tri)
        ms_second = lib.bispectrum_ms()
        print(f"stage times at N {N}: computed {ms_first.tolist()} ms, kept {ms_second.tolist()} ms")
        assert ms_first.shape == (capi.BISPEC_STAGES,) and np.all(ms_first[1:] > 0.0)
        assert np.all(ms_second[1:7] > 0.0) and ms_second[7] == 0.0 and ms_second[8] == 0.0
        assert second["sum_iii"].tobytes() == first["sum_iii"].tobytes()
        assert second["sum_ggg"].tobytes() != first["sum_ggg"].tobytes()
        third = lib.bispectrum(capi.PS_XH, 1.0, 0.0, thr0, tri)
        assert np.all(lib.bispectrum_ms()[7:] > 0.0) and third["sum_iii"].tobytes() != first["sum_iii"].tobytes()
        tri2 = tri.copy()
        tri2[0] = tri[-1]
        lib.bispectrum(capi.PS_XH, 1.0, 0.0, thr0, tri2)
        assert np.all(lib.bispectrum_ms()[7:] > 0.0)
        back = lib.bispectrum(capi.PS_XH, 1.0, 0.0, thr, tri)
        assert np.all(lib.bispectrum_ms()[7:] > 0.0) and back["sum_iii"].tobytes() == first["sum_iii"].tobytes()
        _mesh(asora, 24)
        lib.set_option(capi.OPT_TIMING, 1)
        lib.grid_to_device(capi.GRID_XH, rng.random((24, 24, 24)))
        other = lib.bispectrum(capi.PS_XH, 1.0, 0.0, thr[:4], tri[:1] * 0)
        assert np.all(lib.bispectrum_ms()[7:] > 0.0) and other["sum_iii"][0] > 0
    finally:
        lib.set_option(capi.OPT_TIMING, 0)


def test_refusals_leave_the_outputs_untouched(asora):
    """7."""
    p, lib, capi = asora
    raw = capi.load()
    N, ns, nt = 8, 3, 2
    SENT = 12345.0

    def call(kind=capi.PS_XH, scale=1.0, t_gamma=0.0, n_shells=ns, thr=(1, 4, 9, 16), n_tri=nt, tri=(0, 1, 2, 1, 1, 1), null=()):
        thr, tri = np.array(thr, dtype=np.uint32), np.array(tri, dtype=np.int32)
        out = dict(sum_ggg=np.full(nt, SENT), sum_iii=np.full(nt, SENT), count=np.full(ns, 12345, dtype=np.uint64), sum_k=np.full(ns, SENT),
                   sum_aa=np.full(ns, SENT), moments=np.full(2, SENT))
        ptr = lambda name: None if name in null else (out[name].ctypes.data_as(capi._u64p) if name == "count" else capi.dptr(out[name]))
        rc = raw.asora_bispectrum(kind, scale, t_gamma, n_shells, None if "thresholds" in null else thr.ctypes.data_as(C.POINTER(C.c_uint32)),
                                  n_tri, None if "tri" in null else capi.iptr(tri), ptr("sum_ggg"), ptr("sum_iii"), ptr("count"), ptr("sum_k"),
                                  ptr("sum_aa"), ptr("moments"))
        untouched = all(np.all(v == 12345) for v in out.values())
        return rc, untouched, raw.asora_last_error() or b""

    if p.cuda_is_init():
        p.device_close()
    rc, untouched, msg = call()
    assert rc == 2 and untouched and b"bispectrum" in msg
    p.device_init(N, 8)
    assert call()[:2] == (4, True)
    lib.grid_to_device(capi.GRID_XH, np.random.default_rng(1).random((N, N, N)))
    assert call(kind=capi.PS_DENSITY)[:2] == (4, True) and call(kind=capi.PS_HI)[:2] == (4, True)
    lib.grid_to_device(capi.GRID_NDENS, np.full((N, N, N), 2.0))
    rc, untouched, msg = call(kind=capi.PS_HI, t_gamma=30.0)
    assert rc == 4 and untouched and b"holds no data" in msg
    for kw in (dict(kind=-1), dict(kind=4), dict(scale=np.nan), dict(scale=np.inf), dict(t_gamma=np.nan), dict(t_gamma=np.inf),
               dict(t_gamma=-1.0), dict(n_shells=0), dict(n_shells=-1), dict(n_shells=33), dict(n_tri=0), dict(n_tri=-1), dict(n_tri=8193),
               dict(thr=(0, 4, 9, 16)), dict(thr=(1, 9, 4, 16)), dict(thr=(1, 4, 9, 8)), dict(tri=(0, 1, 3, 1, 1, 1)),
               dict(tri=(0, 1, 2, 1, -1, 1)), dict(null=("thresholds",)), dict(null=("tri",)), dict(null=("sum_ggg",)),
               dict(null=("sum_iii",)), dict(null=("count",)), dict(null=("sum_k",)), dict(null=("sum_aa",)), dict(null=("moments",))):
        rc, untouched, msg = call(**kw)
        assert rc == 3 and untouched and b"bispectrum" in msg, kw
    assert call()[:2] == (0, False) and call(thr=(1, 4, 4, 16))[0] == 0 and call(kind=capi.PS_HI, scale=-3.0)[0] == 0
    for bad in (dict(N=1), dict(N=646), dict(n_shells=0), dict(n_shells=33), dict(n_tri=0), dict(n_tri=8193)):
        args = {**dict(N=8, n_shells=3, n_tri=2), **bad}
        assert raw.asora_debug_bispectrum_plan(args["N"], args["n_shells"], args["n_tri"], capi.iptr(np.zeros(8, dtype=np.int32))) == 3
    assert raw.asora_debug_bispectrum_plan(8, 3, 2, None) == 3 and raw.asora_debug_bispectrum_ms(None) == 3


def test_class(asora, tmp_path):
    """8. sim.bispectrum() after one step equals pyc2ray_amd.bispectrum(field=None, ...) with the same scale, bit for bit."""
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N, dt = 24, 3.15576e13
        with open("src.txt", "w") as f:
            f.write("1\n12 12 12 5e50 1.0\n")
        if p.cuda_is_init():
            p.device_close()
        sim = pc2r.C2Ray_Test(POWER_PARAMS, N, True)
        sim.density_init(0.0)
        srcpos, srcflux = sim.read_sources("src.txt", 1)
        sim.evolve3D(dt, srcflux, srcpos)
        got = sim.bispectrum()
        assert sim._device_newer >= {"xh", "phi_ion"}             # nothing was fetched
        from pyc2ray_amd.c2ray_base import Mpc
        box, scale = sim.boxsize_c / Mpc, sim.brightness_temperature_scale()
        assert (got.kind, got.N, got.box_len, got.aliased) == ("dtb", N, box, False)
        assert got.edges.tolist() == (np.arange(0, 8) + 0.5).tolist() and got.triangles.tolist() == BR.all_triangles(got.edges).tolist()
        m = pc2r.bispectrum(None, kind="dtb", scale=scale, box_len=box)
        for key in ("sum_ggg", "sum_iii", "n_modes", "sum_k", "sum_aa", "moments"):
            assert getattr(m, key).tobytes() == getattr(got, key).tobytes(), key
        assert got.count_residual < 1e-3 and np.all(np.isfinite(got.B[np.rint(got.sum_iii) > 0]))
        ps = sim.power_spectrum(bins=got.edges)
        assert ps.sum_aa.tobytes() == got.sum_aa.tobytes() and np.array_equal(ps.P, got.P)
        eq = sim.bispectrum(triangles="equilateral", shells=4, spin="kinetic")
        assert eq.triangles.tolist() == [[a, a, a] for a in range(4)] and "Bispectrum (dtb, 4 shells" in eq.log_line()
        print(got.log_line())
    finally:
        os.chdir(cwd)
