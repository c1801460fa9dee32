"""Every BASELINE.json configuration at its full size, on the GPU, through the C-ABI (pytest -m gpu).

  configs[0]  64^3, one source, r_RT = 32, Fortran CPU path ............ tests/test_evolve_golden.py::cfg0_64
  configs[1]  128^3, one source, r_RT = 64 (Stroemgren sphere) ........... test_config1_* below
  configs[2]  256^3 uniform, 1000 RandomState(100) sources, r_RT = 16 / 32 / 64: against sparse fixtures produced
              by the REFERENCE Fortran at this size (tests/golden/make_fullsize_golden.py)
  configs[3]  256^3 log-normal density, sources on the densest cells (adjacent sources, same-address atomics):
              ALL 1000 sources against a sparse fixture produced by the REFERENCE Fortran (tests/golden/
              make_bigconfig_golden.py); ONE WHOLE TIME STEP of evolve3D (the device-resident loop) against the reference's
              kernels driven by the reference's loop (make_fullsize_evolve_golden.py); 96 of them (plus coincident ones) against the oracle on the host cores of the GPU box
  configs[4]  512^3 (indices beyond 2^31 bytes): ALL 1e5 sources on the densest cells through two iterations of the evolve
              loop (counts, finiteness, fused loop == separate calls), 256 of them against a sparse fixture produced by the
              REFERENCE Fortran, superposition; corner sources, exact pair counts, one source against the oracle
  a-7         libc2ray.raytracing.do_all_sources (sub-box semantics) on configs[2] itself: 256^3, 1000 sources, r_RT = 32
"""
import os
import sys

import numpy as np
import pytest

import cases
from oracle import oracle as O

pytestmark = pytest.mark.gpu

# what north_star asks of the library's DEFAULT constants (the CUDA library's sqrt literals and thin-cell optical depth,
# ref: src/asora/raytracing.cu:435,439, rates.cu:37) against the reference Fortran: every full-size fixture test runs both
# constant sets -- the Fortran's at 1e-8 ... 1e-10, the default ones at this bar
DEFAULT_MODE_RTOL = 1e-5
_TOL = {1: dict(), 0: dict(rtol_vals=DEFAULT_MODE_RTOL, rtol_sums=DEFAULT_MODE_RTOL, rtol_total=DEFAULT_MODE_RTOL)}

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, G)


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib, _capi
    if p.cuda_is_init():
        p.device_close()


@pytest.fixture(scope="module")
def bench_tables():
    import bench
    return bench.make_tables()


def _fresh(p, N):
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 64)


def _lattice_points_within(R):
    m = int(np.floor(R))
    r = np.arange(-m, m + 1)
    return int(((r[:, None, None] ** 2 + r[None, :, None] ** 2 + r[None, None, :] ** 2) <= R * R).sum())


# ---- configs[2] ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [16, 32, 64])
def test_config2_256_uniform_1000_sources_against_reference_fortran(asora, bench_tables, R):
    """The benchmark workload itself.  R selects three different launch shapes (R = 16 the whole sphere in one
    workgroup of 512 threads, two sources each; R = 32 six sectors x 256 threads, two sources each, line-aligned tables;
    R = 64 twelve sector pairs x 512 threads, one source, the form that leaves exact zeros out)."""
    import bench
    import make_fullsize_golden as MG
    p, lib, capi = asora
    N, NS = 256, 1000
    g = np.load(os.path.join(G, f"fullsize_uniform_R{R}.npz"))
    thin, thick, dlog = bench_tables
    np.testing.assert_allclose([thin.sum(), thick.sum()], g["table_sums"], rtol=1e-13)     # same tables as the fixture's
    ndens, xh, temp, dr, pos, flux = bench.make_workload("uniform", N, NS)
    _fresh(p, N)
    p.photo_table_to_device(thin, thick)
    p0, f0 = cases.flat_sources(pos, flux)
    lib.source_data_to_device(p0, f0, NS)
    lib.grid_to_device(capi.GRID_NDENS, ndens)
    lib.grid_to_device(capi.GRID_XH_AV, xh)
    src_flat = ((pos[0] - 1) * N + (pos[1] - 1)) * N + (pos[2] - 1)
    # the fixture is the Fortran path.  With ITS constants (sqrt literals, thin-cell tau: DESIGN section 2) the comparison is
    # tight; with the library's DEFAULT constants -- the CUDA library's, the mode bench.py times and evolve3D runs -- the bar is
    # north_star's 1e-5 against the same digests
    for fortran_constants, rtol_vals, rtol_sums, rtol_total in ((1, 1e-8, 1e-9, 1e-10), (0, DEFAULT_MODE_RTOL, DEFAULT_MODE_RTOL, DEFAULT_MODE_RTOL)):
        lib.set_option(capi.OPT_FORTRAN_CONSTANTS, fortran_constants)
        try:
            lib.raytrace_device(float(R), bench.SIG, dr, 0, NS, bench.MINLOGTAU, dlog, thin.shape[0] - 1)
        finally:
            lib.set_option(capi.OPT_FORTRAN_CONSTANTS, 0)
        phi = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
        gam, ev = lib.last_raytrace_counts()
        assert gam == NS * _lattice_points_within(float(R))      # R < N/2: no source is clipped by the periodic window
        flat = phi.ravel()
        np.testing.assert_allclose(flat[MG.sample_indices(R)], g["vals"], rtol=rtol_vals, atol=0)
        np.testing.assert_allclose(flat[src_flat], g["src_vals"], rtol=rtol_vals, atol=0)
        d = MG.digest(phi)
        assert int(d["nonzero"]) == int(g["nonzero"])
        np.testing.assert_allclose(d["plane_sums"], g["plane_sums"], rtol=rtol_sums)
        np.testing.assert_allclose(d["block_sums"], g["block_sums"], rtol=rtol_sums)
        np.testing.assert_allclose(float(d["total"]), float(g["total"]), rtol=rtol_total)


# ---- configs[3] ---------------------------------------------------------------------------------------------------
def test_config3_256_lognormal_clustered_sources_against_oracle(asora, bench_tables):
    """The cosmological-like workload of bench.py: log-normal density, sources ON the densest cells -- neighbouring
    and near-coincident sources whose spheres overlap almost completely (many atomics on the same addresses), fluxes
    proportional to the density.  96 of them against the oracle's restatement of the ASORA kernel."""
    import bench
    p, lib, capi = asora
    N, NS, R = 256, 96, 32.0
    thin, thick, dlog = bench_tables
    ndens, xh, temp, dr, pos, flux = bench.make_workload("cosmo", N, 1000)
    # the 88 densest cells, plus the densest one three more times (coincident sources: every atomic of theirs hits an
    # address another workgroup is adding to) and its neighbours along each axis and the diagonal
    top = pos[:, 0]
    extra = np.array([top, top, top, top + [1, 0, 0], top + [0, 1, 0], top + [0, 0, 1], top + [1, 1, 1], top - [1, 1, 0]]).T
    extra = (extra - 1) % N + 1
    pos = np.concatenate([pos[:, :NS - 8], extra], axis=1)
    flux = np.concatenate([flux[:NS - 8], flux[0] * np.array([1.0, 0.5, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0])])
    d = np.abs(pos[:, :, None] - pos[:, None, :])
    d = np.minimum(d, N - d).max(axis=0)
    assert ((d <= 1).sum() - NS) // 2 >= 20                  # adjacent or coincident pairs
    assert ((d <= 32).sum() - NS) // 2 >= 100                # pairs whose spheres overlap by more than half
    _fresh(p, N)
    p.photo_table_to_device(thin, thick)
    p0, f0 = cases.flat_sources(pos, flux)
    lib.source_data_to_device(p0, f0, NS)
    lib.grid_to_device(capi.GRID_NDENS, ndens)
    lib.grid_to_device(capi.GRID_XH_AV, xh)
    numtau = thin.shape[0] - 1
    lib.raytrace_device(R, bench.SIG, dr, 0, NS, bench.MINLOGTAU, dlog, numtau)
    phi = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
    gam, _ = lib.last_raytrace_counts()
    assert gam == NS * _lattice_points_within(R)
    ref = O.asora_do_all_sources(R, bench.SIG, dr, ndens, xh, p0, f0, thin, thick, bench.MINLOGTAU, dlog, NumTau=numtau,
                                 flags=O.ASORA_MODE)["phi_ion"]
    w = ref != 0
    assert np.array_equal(phi != 0, w) and w.sum() > 1e5
    np.testing.assert_allclose(phi[w], ref[w], rtol=1e-8, atol=0)
    # and the step the benchmark times: one outer iteration of the device-resident loop on this workload equals
    # raytrace + chemistry done separately
    lib.grid_to_device(capi.GRID_TEMP, temp)
    lib.grid_to_device(capi.GRID_XH, xh)
    chem = (bench.MYR, bench.BH00, bench.ALBPOW, bench.COLH0, bench.TEMPH0, bench.ABU_C)
    lib.grid_copy(capi.GRID_XH_AV, capi.GRID_XH)
    lib.grid_copy(capi.GRID_XH_INTERMED, capi.GRID_XH)
    lib.raytrace_device(R, bench.SIG, dr, 0, NS, bench.MINLOGTAU, dlog, numtau)
    conv, s1, s0 = lib.chemistry_device(*chem)
    x_sep = lib.grid_to_host(capi.GRID_XH_INTERMED, np.empty((N, N, N)))
    lib.evolve_begin(*chem, R, bench.SIG, dr, bench.MINLOGTAU, dlog, numtau, 0, NS, -1.0, 0.0)
    lib.evolve_enqueue(1)
    n_done, done, rows = lib.evolve_poll()
    assert n_done == 1 and not done and int(rows[0][0]) == conv
    np.testing.assert_allclose(rows[0][1:3], [s1, s0], rtol=1e-12)
    x_fused = lib.grid_to_host(capi.GRID_XH_INTERMED, np.empty((N, N, N)))
    np.testing.assert_allclose(x_fused, x_sep, rtol=1e-11, atol=0)
    np.testing.assert_allclose(lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))[w], phi[w], rtol=1e-11)


def _against_bigconfig_fixture(phi, g, MB, N, pos, rtol_vals=1e-8, rtol_sums=1e-9, rtol_total=1e-10):
    flat = phi.ravel()
    np.testing.assert_allclose(flat[MB.sample_indices(N, pos, 20260300 + N)], g["vals"], rtol=rtol_vals, atol=0)
    src_flat = ((pos[0] - 1) * N + (pos[1] - 1)) * N + (pos[2] - 1)
    np.testing.assert_allclose(flat[src_flat], g["src_vals"], rtol=rtol_vals, atol=0)
    d = MB.digest(phi)
    assert int(d["nonzero"]) == int(g["nonzero"])
    np.testing.assert_allclose(d["plane_sums"], g["plane_sums"], rtol=rtol_sums)
    np.testing.assert_allclose(d["block_sums"], g["block_sums"], rtol=rtol_sums, atol=1e-12 * float(np.abs(g["block_sums"]).max()))
    np.testing.assert_allclose(float(d["total"]), float(g["total"]), rtol=rtol_total)


def test_config3_256_lognormal_all_1000_sources_against_reference_fortran(asora, bench_tables):
    """BASELINE configs[3] at its full workload: every one of the 1000 sources on the densest cells of the log-normal
    256^3 density, fluxes proportional to the density, against the reference Fortran (one call per source: its
    do_all_sources rates every source with the LAST source's flux, raytracing.f90:500)."""
    import bench
    import make_bigconfig_golden as MB
    p, lib, capi = asora
    N, NS, R = 256, 1000, 32.0
    g = np.load(os.path.join(G, "fullsize_cosmo256_R32.npz"))
    thin, thick, dlog = bench_tables
    np.testing.assert_allclose([thin.sum(), thick.sum()], g["table_sums"], rtol=1e-13)
    ndens, xh, temp, dr, pos, flux = bench.make_workload("cosmo", N, NS)
    chk = MB.input_checksums(ndens, pos, flux)      # the regenerated inputs are the fixture's inputs
    assert int(chk["pos_sum"]) == int(g["pos_sum"])
    np.testing.assert_allclose([float(chk["ndens_sum"]), float(chk["flux_sum"])], [float(g["ndens_sum"]), float(g["flux_sum"])], rtol=1e-12)
    _fresh(p, N)
    p.photo_table_to_device(thin, thick)
    p0, f0 = cases.flat_sources(pos, flux)
    lib.source_data_to_device(p0, f0, NS)
    lib.grid_to_device(capi.GRID_NDENS, ndens)
    lib.grid_to_device(capi.GRID_XH_AV, xh)
    for fortran_constants in (1, 0):           # the Fortran's constants: tight; the library's default ones: north_star's 1e-5
        lib.set_option(capi.OPT_FORTRAN_CONSTANTS, fortran_constants)
        try:
            lib.raytrace_device(R, bench.SIG, dr, 0, NS, bench.MINLOGTAU, dlog, thin.shape[0] - 1)
        finally:
            lib.set_option(capi.OPT_FORTRAN_CONSTANTS, 0)
        phi = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
        gam, _ = lib.last_raytrace_counts()
        assert gam == NS * _lattice_points_within(R)
        _against_bigconfig_fixture(phi, g, MB, N, pos, **_TOL[fortran_constants])


def test_config3_256_one_whole_time_step_against_the_reference_kernels(asora, bench_tables, tmp_path):
    """BASELINE configs[3] through `evolve3D` itself -- the device-resident loop: raytrace of all 1000 sources, fused pass,
    convergence test on the device, batches of iterations -- for one whole time step at full size, against the reference
    Fortran's kernels driven by the reference's loop (tests/golden/make_fullsize_evolve_golden.py): same number of outer
    iterations, the same count of non-converged cells in every iteration (to a handful of cells that sit on the 1e-3
    threshold), ionised fraction to 1e-8, last iteration's rates to 1e-7."""
    import re
    import bench
    import make_bigconfig_golden as MB
    p, lib, capi = asora
    N, NS, R = 256, 1000, 32.0
    g = np.load(os.path.join(G, "fullsize_evolve_cosmo256.npz"))
    thin, thick, dlog = bench_tables
    np.testing.assert_allclose([thin.sum(), thick.sum()], g["table_sums"], rtol=1e-13)
    ndens, xh, temp, dr, pos, flux = bench.make_workload("cosmo", N, NS)
    chk = MB.input_checksums(ndens, pos, flux)
    assert int(chk["pos_sum"]) == int(g["pos_sum"])
    np.testing.assert_allclose([float(chk["ndens_sum"]), float(chk["flux_sum"])], [float(g["ndens_sum"]), float(g["flux_sum"])], rtol=1e-12)
    _fresh(p, N)
    p.photo_table_to_device(thin, thick)
    niter = int(g["niter"])
    idx = MB.sample_indices(N, pos, 20260400)
    src_flat = ((pos[0] - 1) * N + (pos[1] - 1)) * N + (pos[2] - 1)
    want = g["rows"][:, 0]
    # the fixture is the Fortran path: with its constants tight; with the library's default constants (what evolve3D runs with)
    # the same number of outer iterations, the same counts to the cells on the threshold, fields within north_star's 1e-5
    for fortran_constants in (1, 0):
        log = str(tmp_path / f"log{fortran_constants}.txt")
        lib.set_option(capi.OPT_FORTRAN_CONSTANTS, fortran_constants)
        try:
            x, phi = p.evolve3D(float(g["dt"]), dr, flux * float(g["flux_scale"]), pos, True, 1000, N, 1e-2, temp, ndens, xh, thin, thick, bench.MINLOGTAU, dlog,
                                R, 1e-4, bench.SIG, bench.BH00, bench.ALBPOW, bench.COLH0, bench.TEMPH0, bench.ABU_C, logfile=log, quiet=True)
        finally:
            lib.set_option(capi.OPT_FORTRAN_CONSTANTS, 0)
        assert p.evolve._evolve.last_niter == niter and niter >= 5
        flags = [int(v) for v in re.findall(r"Number of non-converged points: (\d+) of", open(log).read())]
        assert len(flags) == niter
        assert np.all(np.abs(np.array(flags) - want) <= np.maximum(5, 1e-4 * want)), (flags, want)
        np.testing.assert_allclose(float(x.mean()), float(g["x_mean"]), rtol=1e-10 if fortran_constants else DEFAULT_MODE_RTOL)
        for name, grid, rtol in (("x", x, 1e-8), ("phi", phi, 1e-7)):
            if not fortran_constants:
                rtol = DEFAULT_MODE_RTOL
            flat = np.ascontiguousarray(grid).ravel()
            np.testing.assert_allclose(flat[idx], g[f"{name}_vals"], rtol=rtol, atol=0, err_msg=name)
            np.testing.assert_allclose(flat[src_flat], g[f"{name}_src_vals"], rtol=rtol, atol=0, err_msg=name)
            d = MB.digest(np.ascontiguousarray(grid))
            np.testing.assert_allclose(d["plane_sums"], g[f"{name}_plane_sums"], rtol=rtol)
            np.testing.assert_allclose(d["block_sums"], g[f"{name}_block_sums"], rtol=rtol, atol=1e-12 * float(np.abs(g[f"{name}_block_sums"]).max()))
    assert 1e-3 < float(x.mean()) < 0.5 and float(x.max()) > 0.9           # ionised bubbles in a mostly neutral box


# ---- configs[4] ---------------------------------------------------------------------------------------------------
def test_config4_512_corner_sources_and_large_indices(asora):
    """512^3: the [k][j][i] twins of the grids start 2^30 bytes in and end beyond 2^31 bytes.  Sources on the first
    and the last cell (every octant wraps), in the middle and on a face; one of them against the oracle."""
    p, lib, capi = asora
    N, R = 512, 32.0
    thin, thick, dlog = cases.soft_tables(20000)
    rng = np.random.default_rng(4)
    nd = 1e-3 * np.exp(0.8 * rng.standard_normal((N, N, N), dtype=np.float32).astype(np.float64) - 0.32)
    xh = np.full((N, N, N), 2e-4)
    dr = 0.02 / (cases.SIG * 1e-3)
    pos = np.array([[512, 512, 512], [1, 1, 1], [256, 256, 256], [512, 300, 1], [17, 512, 400], [300, 1, 512]]).T
    flux = np.array([1.0, 2.0, 3.0, 1.5, 0.5, 2.5])
    NS = flux.shape[0]
    _fresh(p, N)
    p.photo_table_to_device(thin, thick)
    p0, f0 = cases.flat_sources(pos, flux)
    lib.grid_to_device(capi.GRID_NDENS, nd)
    lib.grid_to_device(capi.GRID_XH_AV, xh)
    numtau = thin.shape[0] - 1

    def trace(sel):
        q0, g0 = cases.flat_sources(pos[:, sel], flux[sel])
        lib.source_data_to_device(q0, g0, g0.shape[0])
        lib.raytrace_device(R, cases.SIG, dr, 0, g0.shape[0], cases.MINLOGTAU, dlog, numtau)
        return lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))

    full = trace(np.arange(NS))
    gam, ev = lib.last_raytrace_counts()
    assert gam == NS * _lattice_points_within(R)
    assert np.isfinite(full).all() and (full >= 0).all()
    # the last cell of the grid (largest index of both layouts) is a source cell: it holds the largest rate there
    assert full[511, 511, 511] > 0 and full[0, 0, 0] > 0
    # the corner source alone against the oracle: its sphere wraps onto all eight corners of the box
    one = trace(np.array([0]))
    ref = O.asora_do_all_sources(R, cases.SIG, dr, nd, xh, p0[:3], f0[:1], thin, thick, cases.MINLOGTAU, dlog,
                                 NumTau=numtau, flags=O.ASORA_MODE)["phi_ion"]
    w = ref != 0
    assert np.array_equal(one != 0, w)
    np.testing.assert_allclose(one[w], ref[w], rtol=1e-8, atol=0)
    for corner in [(0, 0, 0), (511, 0, 0), (0, 511, 511), (511, 511, 511), (490, 5, 500)]:
        assert one[corner] > 0
    # superposition at this size: the sources one by one add up to the joint trace
    acc = one.copy()
    for s in range(1, NS):
        acc += trace(np.array([s]))
    np.testing.assert_allclose(acc, full, rtol=1e-11, atol=0)
    p.device_close()


def test_config4_512_all_1e5_sources_evolve_loop_and_reference_subset(asora, bench_tables):
    """BASELINE configs[4] at its workload: 512^3 log-normal density (seed of bench.make_workload), 1e5 sources on the
    densest cells, r_RT = 32.
      (a) 256 of the sources (spread from the densest cell to the 1e5-th densest) against the reference Fortran's sparse
          fixture; the two halves of that subset add up to the whole (superposition at this size);
      (b) all 1e5 sources -- 1.2 M workgroups per launch -- through TWO outer iterations of the device-resident evolve
          loop (1 GiB grids, the fused pass, the reduction buffers): exact pair counts, every field finite, and the same
          convergence numbers, ionised fraction and rates as raytrace_device + chemistry_device called separately."""
    import bench
    import make_bigconfig_golden as MB
    p, lib, capi = asora
    N, NS, R = 512, 100000, 32.0
    g = np.load(os.path.join(G, "fullsize_cosmo512_R32.npz"))
    thin, thick, dlog = bench_tables
    np.testing.assert_allclose([thin.sum(), thick.sum()], g["table_sums"], rtol=1e-13)
    ndens, xh, temp, dr, pos, flux = bench.make_workload("cosmo", N, NS)
    chk = MB.input_checksums(ndens, pos, flux)
    assert int(chk["pos_sum"]) == int(g["pos_sum"])
    np.testing.assert_allclose([float(chk["ndens_sum"]), float(chk["flux_sum"])], [float(g["ndens_sum"]), float(g["flux_sum"])], rtol=1e-12)
    numtau = thin.shape[0] - 1
    _fresh(p, N)
    p.photo_table_to_device(thin, thick)
    lib.grid_to_device(capi.GRID_NDENS, ndens)
    lib.grid_to_device(capi.GRID_XH_AV, xh)

    # (a) the fixture's subset, with the Fortran's constants
    sub = MB.subset_indices(NS, int(g["nsub"]))
    spos, sflux = pos[:, sub], flux[sub]

    def trace(sel):
        q0, g0 = cases.flat_sources(spos[:, sel], sflux[sel])
        lib.source_data_to_device(q0, g0, g0.shape[0])
        lib.raytrace_device(R, bench.SIG, dr, 0, g0.shape[0], bench.MINLOGTAU, dlog, numtau)
        return lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))

    lib.set_option(capi.OPT_FORTRAN_CONSTANTS, 1)
    try:
        both = trace(np.arange(sub.size))
        gam, _ = lib.last_raytrace_counts()
        assert gam == sub.size * _lattice_points_within(R)
        _against_bigconfig_fixture(both, g, MB, N, spos)
        half = trace(np.arange(sub.size // 2))
        half += trace(np.arange(sub.size // 2, sub.size))
    finally:
        lib.set_option(capi.OPT_FORTRAN_CONSTANTS, 0)
    w = both != 0
    assert np.array_equal(half != 0, w)
    np.testing.assert_allclose(half[w], both[w], rtol=1e-11, atol=0)
    del both, half, w
    # the same subset with the library's default constants: north_star's 1e-5 against the same fixture
    both = trace(np.arange(sub.size))
    _against_bigconfig_fixture(both, g, MB, N, spos, **_TOL[0])
    del both

    # (b) the whole list through the loop
    p0, f0 = cases.flat_sources(pos, flux)
    lib.source_data_to_device(p0, f0, NS)
    lib.grid_to_device(capi.GRID_TEMP, temp)
    lib.grid_to_device(capi.GRID_XH, xh)
    chem = (1e13, bench.BH00, bench.ALBPOW, bench.COLH0, bench.TEMPH0, bench.ABU_C)     # dt of SURVEY 8d(5)
    lib.grid_copy(capi.GRID_XH_AV, capi.GRID_XH)
    lib.grid_copy(capi.GRID_XH_INTERMED, capi.GRID_XH)
    sep = []
    for it in range(2):
        lib.raytrace_device(R, bench.SIG, dr, 0, NS, bench.MINLOGTAU, dlog, numtau)
        gam, ev = lib.last_raytrace_counts()
        assert gam == NS * _lattice_points_within(R) and ev > gam
        sep.append(lib.chemistry_device(*chem))
    x_sep = lib.grid_to_host(capi.GRID_XH_INTERMED, np.empty((N, N, N)))
    phi_sep = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
    assert np.isfinite(x_sep).all() and np.isfinite(phi_sep).all() and (phi_sep >= 0).all()
    assert 0 <= sep[0][0] <= N ** 3 and x_sep.min() > 0.0 and x_sep.max() <= 1.0
    lib.evolve_begin(*chem, R, bench.SIG, dr, bench.MINLOGTAU, dlog, numtau, 0, NS, -1.0, 1e-4)
    lib.evolve_enqueue(2)
    n_done, done, rows = lib.evolve_poll()
    assert n_done == 2 and len(rows) == 2
    gam, _ = lib.last_raytrace_counts()
    assert gam == 2 * NS * _lattice_points_within(R)            # the loop's counters run on from evolve_begin
    for it in range(2):
        assert int(rows[it][0]) == sep[it][0]
        np.testing.assert_allclose(rows[it][1:3], sep[it][1:3], rtol=1e-12)
    # (two launches add a cell's up to ~1e4 contributions in different orders: rounding of the sum, ~1e-16 x sqrt(count);
    #  measured: 6 of 1.3e8 cells beyond 1e-11, the largest 2.5e-11)
    x_fused = lib.grid_to_host(capi.GRID_XH_INTERMED, np.empty((N, N, N)))
    np.testing.assert_allclose(x_fused, x_sep, rtol=1e-9, atol=0)
    del x_fused, x_sep
    phi_fused = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
    w = phi_sep != 0
    assert np.array_equal(phi_fused != 0, w)
    np.testing.assert_allclose(phi_fused[w], phi_sep[w], rtol=1e-9, atol=0)
    p.device_close()


# ---- meshes beyond the buffer descriptors' range -----------------------------------------------------------------------
def test_mesh_576_both_atomic_families_at_real_size(asora):
    """N > 512: [phi | phi_t] no longer fits the 2 GiB a raw buffer descriptor spans, so the rates go through
    global_atomic_add_f64 with one 32-bit cell index over both layouts (2 x 576^3 = 3.8e8 < 2^32) formed by two 24-bit
    multiply-adds (raytrace.hip, nhi_address), and neither the paired-sources variant nor the line-aligned tables exist.
    Until round 4 that family only ran at N <= 96 behind an option switch; the reference works up to
    N = 645 (src/asora/raytracing.cu:95).  Here at N = 576 (1.5 GB grids, the [k][j][i] twins end 3.06e9 bytes in):
    a corner source whose sphere wraps onto all eight corners against the oracle, superposition of five sources, exact pair
    counts, and one iteration of the device-resident loop (fused pass on 1.5 GB grids, both accumulator pairs) against
    raytrace_device + chemistry_device called separately."""
    p, lib, capi = asora
    N, R = 576, 20.0
    thin, thick, dlog = cases.soft_tables(20000)
    rng = np.random.default_rng(576)
    nd = 1e-3 * np.exp(0.8 * rng.standard_normal((N, N, N), dtype=np.float32).astype(np.float64) - 0.32)
    xh = np.full((N, N, N), 2e-4)
    temp = np.full((N, N, N), 1e4)
    dr = 0.03 / (cases.SIG * 1e-3)
    pos = np.array([[576, 576, 576], [1, 1, 1], [288, 300, 17], [576, 400, 1], [530, 576, 575]]).T
    flux = np.array([1.0e3, 2.0e3, 3.0e3, 1.5e3, 0.5e3])
    NS = flux.shape[0]
    _fresh(p, N)
    p.photo_table_to_device(thin, thick)
    p0, f0 = cases.flat_sources(pos, flux)
    lib.grid_to_device(capi.GRID_NDENS, nd)
    lib.grid_to_device(capi.GRID_XH_AV, xh)
    numtau = thin.shape[0] - 1

    def trace(sel):
        q0, g0 = cases.flat_sources(pos[:, sel], flux[sel])
        lib.source_data_to_device(q0, g0, g0.shape[0])
        lib.raytrace_device(R, cases.SIG, dr, 0, g0.shape[0], cases.MINLOGTAU, dlog, numtau)
        return lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))

    full = trace(np.arange(NS))
    gam, ev = lib.last_raytrace_counts()
    assert gam == NS * _lattice_points_within(R) and ev >= gam
    assert np.isfinite(full).all() and (full >= 0).all()
    assert full[N - 1, N - 1, N - 1] > 0 and full[0, 0, 0] > 0        # the largest index of both layouts is a source cell
    one = trace(np.array([0]))
    ref = O.asora_do_all_sources(R, cases.SIG, dr, nd, xh, p0[:3], f0[:1], thin, thick, cases.MINLOGTAU, dlog,
                                 NumTau=numtau, flags=O.ASORA_MODE)["phi_ion"]
    w = ref != 0
    assert np.array_equal(one != 0, w) and int(w.sum()) == _lattice_points_within(R)
    np.testing.assert_allclose(one[w], ref[w], rtol=1e-8, atol=0)
    for corner in [(0, 0, 0), (N - 1, 0, 0), (0, N - 1, N - 1), (N - 1, N - 1, N - 1), (N - 12, 5, N - 8)]:
        assert one[corner] > 0
    del ref, w
    acc = one
    for s in range(1, NS):
        acc += trace(np.array([s]))
    np.testing.assert_allclose(acc, full, rtol=1e-11, atol=0)
    del acc, one, full

    # many sources: the launch shapes of a full chip against the oracle on the host -- at this radius the three all-sign sectors with
    # two sources per workgroup and a buffer descriptor per layout (round 6; the whole sphere in one workgroup, which N <= 512 takes
    # here, holds cells of every face and could only use global atomics) -- and the global-atomic family forced onto the same launch
    NM = 600
    mpos = 1 + rng.integers(0, N, size=(3, NM))
    mflux = rng.uniform(0.5e3, 2.0e3, size=NM)
    m0, mf0 = cases.flat_sources(mpos, mflux)
    lib.source_data_to_device(m0, mf0, NM)
    lib.raytrace_device(R, cases.SIG, dr, 0, NM, cases.MINLOGTAU, dlog, numtau)
    v = lib.last_raytrace_variant()
    assert v["units"] == 3 and v["paired"] and v["buffer_atomics"] and v["split_descriptors"], v
    many = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
    gam, ev = lib.last_raytrace_counts()
    assert gam == NM * _lattice_points_within(R)
    ref = O.asora_do_all_sources(R, cases.SIG, dr, nd, xh, m0, mf0, thin, thick, cases.MINLOGTAU, dlog,
                                 NumTau=numtau, flags=O.ASORA_MODE)["phi_ion"]
    w = ref != 0
    assert np.array_equal(many != 0, w)
    np.testing.assert_allclose(many[w], ref[w], rtol=1e-8, atol=0)
    del ref
    lib.set_option(capi.OPT_GLOBAL_ATOMICS, 1)              # the whole sphere x 512 threads, one source per workgroup
    lib.raytrace_device(R, cases.SIG, dr, 0, NM, cases.MINLOGTAU, dlog, numtau)
    v = lib.last_raytrace_variant()
    lib.set_option(capi.OPT_GLOBAL_ATOMICS, 0)
    assert v["units"] == 1 and not v["buffer_atomics"] and not v["paired"], v
    glob = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
    assert np.array_equal(glob != 0, w)
    np.testing.assert_allclose(glob[w], many[w], rtol=1e-11, atol=0)
    del many, glob

    # heating and grey opacity beyond N = 512 (round 6): one source per workgroup, a buffer descriptor per layout of the rate grid AND
    # of the heating grid -- the same arithmetic as the global-atomic family, so the two must agree to the order of the additions
    # (the rates of both against the oracle above and in tests/test_gpu_parity.py; heating against the oracle below N = 512 in
    # tests/test_gpu_heating.py, and here by the power-of-two identity after this block)
    lib.heat_table_to_device(2e-11 * thin * np.linspace(1.0, 3.0, thin.shape[0]), 1e-11 * thick, thin.shape[0])
    for opt, grids in ((capi.OPT_HEATING, (capi.GRID_PHI_ION, capi.GRID_PHI_HEAT)), (capi.OPT_GREY_NOTABLES, (capi.GRID_PHI_ION,))):
        res = {}
        for glob_atomics in (0, 1):
            lib.set_option(opt, 1)
            lib.set_option(capi.OPT_GLOBAL_ATOMICS, glob_atomics)
            try:
                lib.raytrace_device(R, cases.SIG, dr, 0, NM, cases.MINLOGTAU, dlog, numtau)
                v = lib.last_raytrace_variant()
                res[glob_atomics] = [lib.grid_to_host(g, np.empty((N, N, N))) for g in grids]
            finally:
                lib.set_option(opt, 0)
                lib.set_option(capi.OPT_GLOBAL_ATOMICS, 0)
            assert v["buffer_atomics"] == (not glob_atomics) and v["split_descriptors"] == (not glob_atomics) and not v["paired"], (opt, v)
        for a, b in zip(res[0], res[1]):
            assert np.array_equal(a != 0, w) and np.array_equal(b != 0, w)
            np.testing.assert_allclose(a[w], b[w], rtol=1e-11, atol=0)
        del res
    del w
    # the power-of-two identity at this size: heating tables = 2^-35 x photo tables and 27 sources whose spheres do not overlap
    # (one on the corner, so that they wrap) -> PHI_HEAT == 2^-35 PHI_ION bit for bit in both families (the three all-sign
    # sectors x 512 threads with SPLIT descriptors, the form the 600 sources above take; and global atomics)
    p2 = 2.0 ** -35
    lpos = np.array([(i, j, k) for i in (1, 193, 385) for j in (1, 193, 385) for k in (1, 193, 385)]).T
    l0, lf0 = cases.flat_sources(lpos, np.linspace(0.5e3, 2.0e3, lpos.shape[1]))
    lib.source_data_to_device(l0, lf0, lpos.shape[1])
    lib.heat_table_to_device(p2 * thin, p2 * thick, thin.shape[0])
    for glob_atomics in (0, 1):
        lib.set_option(capi.OPT_HEATING, 1)
        lib.set_option(capi.OPT_GLOBAL_ATOMICS, glob_atomics)
        lib.set_option(capi.OPT_SECTORS, 8)
        lib.set_option(capi.OPT_BLOCK_THREADS, 512)
        try:
            lib.raytrace_device(R, cases.SIG, dr, 0, lpos.shape[1], cases.MINLOGTAU, dlog, numtau)
            v = lib.last_raytrace_variant()
            lphi = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
            lheat = lib.grid_to_host(capi.GRID_PHI_HEAT, np.empty((N, N, N)))
        finally:
            lib.set_option(capi.OPT_HEATING, 0)
            lib.set_option(capi.OPT_GLOBAL_ATOMICS, 0)
            lib.set_option(capi.OPT_SECTORS, 0)
            lib.set_option(capi.OPT_BLOCK_THREADS, 0)
        assert v["units"] == 3 and v["threads"] == 512 and v["split_descriptors"] == (not glob_atomics) and not v["paired"], v
        assert int((lphi != 0).sum()) == lpos.shape[1] * _lattice_points_within(R)
        assert np.array_equal(lheat, p2 * lphi) and not np.signbit(lheat).any()
        del lphi, lheat

    # the production forms beyond N = 512 (round 5).  At r_RT = 30 a source is cut into six sectors, whose rated cells lie on one
    # face each, so the rate atomics of a workgroup go through a buffer descriptor over ONE layout of the grid (8 N^3 bytes
    # <= 2 GiB up to N = 645, the reference's own limit, raytracing.cu:95) -- and with buffer atomics come two sources per
    # workgroup and the line-aligned tables.  Against the oracle, and against the global-atomic family forced onto the same launch.
    R2, NM2 = 30.0, 320
    lib.source_data_to_device(m0[:3 * NM2], mf0[:NM2], NM2)
    lib.set_option(capi.OPT_ALIGNED_ROWS, 2)      # (left to itself the library waits for a radius to settle: it has just changed)
    lib.raytrace_device(R2, cases.SIG, dr, 0, NM2, cases.MINLOGTAU, dlog, numtau)
    lib.set_option(capi.OPT_ALIGNED_ROWS, 0)
    v = lib.last_raytrace_variant()
    assert v["paired"] and v["aligned"] and v["buffer_atomics"] and v["split_descriptors"] and v["units"] == 6, v
    prod = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
    gam, ev = lib.last_raytrace_counts()
    assert gam == NM2 * _lattice_points_within(R2)
    ref = O.asora_do_all_sources(R2, cases.SIG, dr, nd, xh, m0[:3 * NM2], mf0[:NM2], thin, thick, cases.MINLOGTAU, dlog,
                                 NumTau=numtau, flags=O.ASORA_MODE)["phi_ion"]
    w = ref != 0
    assert np.array_equal(prod != 0, w)
    np.testing.assert_allclose(prod[w], ref[w], rtol=1e-8, atol=0)
    del ref
    lib.set_option(capi.OPT_GLOBAL_ATOMICS, 1)
    lib.raytrace_device(R2, cases.SIG, dr, 0, NM2, cases.MINLOGTAU, dlog, numtau)
    v = lib.last_raytrace_variant()
    assert not v["buffer_atomics"] and not v["paired"] and not v["split_descriptors"], v
    lib.set_option(capi.OPT_GLOBAL_ATOMICS, 0)
    glob = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
    assert np.array_equal(glob != 0, w)
    np.testing.assert_allclose(glob[w], prod[w], rtol=1e-11, atol=0)
    del glob, prod, w

    # one iteration of the device-resident loop against the separate calls
    lib.source_data_to_device(p0, f0, NS)
    lib.grid_to_device(capi.GRID_TEMP, temp)
    lib.grid_to_device(capi.GRID_XH, xh)
    chem = (3.15576e13, cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)
    lib.grid_copy(capi.GRID_XH_AV, capi.GRID_XH)
    lib.grid_copy(capi.GRID_XH_INTERMED, capi.GRID_XH)
    sep = []
    for it in range(2):
        lib.raytrace_device(R, cases.SIG, dr, 0, NS, cases.MINLOGTAU, dlog, numtau)
        sep.append(lib.chemistry_device(*chem))
    x_sep = lib.grid_to_host(capi.GRID_XH_INTERMED, np.empty((N, N, N)))
    phi_sep = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
    assert np.isfinite(x_sep).all() and x_sep.max() > 10 * 2e-4          # the sources ionise their surroundings
    lib.evolve_begin(*chem, R, cases.SIG, dr, cases.MINLOGTAU, dlog, numtau, 0, NS, -1.0, 1e-4)
    lib.evolve_enqueue(2)
    n_done, done, rows = lib.evolve_poll()
    assert n_done == 2 and len(rows) == 2
    for it in range(2):
        assert int(rows[it][0]) == sep[it][0]
        np.testing.assert_allclose(rows[it][1:3], sep[it][1:3], rtol=1e-12)
    x_fused = lib.grid_to_host(capi.GRID_XH_INTERMED, np.empty((N, N, N)))
    np.testing.assert_allclose(x_fused, x_sep, rtol=1e-10, atol=0)
    del x_fused, x_sep
    phi_fused = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
    w = phi_sep != 0
    assert np.array_equal(phi_fused != 0, w)
    np.testing.assert_allclose(phi_fused[w], phi_sep[w], rtol=1e-10, atol=0)
    p.device_close()


# ---- a-7 at the benchmark's size ----------------------------------------------------------------------------------------
def test_c2ray_do_all_sources_256_uniform_1000_sources_against_reference_fortran(asora, bench_tables):
    """libc2ray.raytracing.do_all_sources -- the reference's CPU function, evaluated by the sub-box kernels -- on the
    benchmark workload itself (256^3, 1000 sources, one sub-box of +-32 cells, R_max_LLS = 32: the call of
    raytracing_benchmark/run_test.py:88), host arrays in and out, against the reference Fortran's fixture."""
    import bench
    import make_fullsize_golden as MG
    from pyc2ray_amd.load_extensions import load_c2ray
    p, lib, capi = asora
    N, NS, R = 256, 1000, 32
    g = np.load(os.path.join(G, f"fullsize_uniform_R{R}.npz"))
    thin, thick, dlog = bench_tables
    ndens, xh, temp, dr, pos, flux = bench.make_workload("uniform", N, NS)
    if p.cuda_is_init():
        p.device_close()
    f = lambda a: np.asfortranarray(a)
    cd, phi, heat = (np.zeros((N, N, N), order="F") for _ in range(3))
    zeros = np.zeros(thin.shape[0])
    nbox, loss = load_c2ray().raytracing.do_all_sources(flux, pos.astype(np.int32), R, R, cd, bench.SIG, dr, f(ndens), f(xh), phi,
                                                        heat, 0.0, thin, thick, zeros, zeros, bench.MINLOGTAU, dlog, float(R))
    assert nbox == int(g["nsubbox"]) == NS
    flat = np.ascontiguousarray(phi).ravel()
    np.testing.assert_allclose(flat[MG.sample_indices(R)], g["vals"], rtol=1e-8, atol=0)
    src_flat = ((pos[0] - 1) * N + (pos[1] - 1)) * N + (pos[2] - 1)
    np.testing.assert_allclose(flat[src_flat], g["src_vals"], rtol=1e-8, atol=0)
    d = MG.digest(np.ascontiguousarray(phi))
    assert int(d["nonzero"]) == int(g["nonzero"])
    np.testing.assert_allclose(d["plane_sums"], g["plane_sums"], rtol=1e-9)
    np.testing.assert_allclose(d["block_sums"], g["block_sums"], rtol=1e-9)
    np.testing.assert_allclose(float(d["total"]), float(g["total"]), rtol=1e-10)
    # the column densities that come back are the LAST source's, over its whole +-32 cube (raytracing.f90:181,488): against
    # the reference Fortran's own coldensh_out of this call (tests/golden/make_fullsize_coldens_golden.py)
    assert np.count_nonzero(cd) == (2 * R + 1) ** 3 and np.isfinite(cd).all() and not heat.any()
    _coldens_cube_against_fixture(cd, "u32", pos[:, -1], rtol=1e-11)


def _coldens_cube_against_fixture(cd, case, src, rtol, rated_only=False):
    """cd: (N,N,N) column densities of ONE source (logical [i,j,k]); against the reference Fortran's cube of that source.
    rated_only: cd holds the cells within r_RT only (what the ASORA path evaluates: asora_debug_coldens), zero elsewhere."""
    import make_fullsize_coldens_golden as MC
    g = np.load(os.path.join(G, "fullsize_coldens.npz"))
    r = MC.CASES[case][1]
    assert np.array_equal(np.asarray(src), g[f"{case}_src"])
    cube = MC.cube_of(cd, src, r)
    if not rated_only:
        d = MC.digest(cube, case)
        assert int(d[f"{case}_nonzero"]) == int(g[f"{case}_nonzero"]) == (2 * r + 1) ** 3
        for key in ("vals", "plane_sums", "row_sums", "total"):
            np.testing.assert_allclose(d[f"{case}_{key}"], g[f"{case}_{key}"], rtol=rtol, atol=0, err_msg=f"{case} {key}")
        return
    off = MC.sample_offsets(case)
    inside = (off ** 2).sum(axis=0) <= r * r
    assert inside.sum() > 5000
    rr = np.arange(-r, r + 1)
    sphere = (rr[:, None, None] ** 2 + rr[None, :, None] ** 2 + rr[None, None, :] ** 2) <= r * r
    assert np.array_equal(cube != 0, sphere) and np.count_nonzero(cd) == int(sphere.sum())       # exactly the rated cells
    got = cube[off[0] + r, off[1] + r, off[2] + r]
    np.testing.assert_allclose(got[inside], g[f"{case}_vals"][inside], rtol=rtol, atol=0, err_msg=case)


@pytest.mark.parametrize("case", ["u32", "u64", "c32"])
def test_column_density_at_full_size_against_reference_fortran(asora, bench_tables, case):
    """north_star: "ionized fraction AND column density within 1e-5".  256^3, the last source of configs[2] (r_RT = 32, 64) and
    of configs[3] (log-normal density): the column densities the ASORA path evaluates (asora_debug_coldens: the cells within
    r_RT, the DUMP kernels 256 x {256, 1024}) against the reference Fortran's coldensh_out -- with the Fortran's constants at
    1e-9, with the library's default ones (sqrt literals of raytracing.cu:435,439) at 1e-5 -- and the whole cube as
    c2ray_do_all_sources hands it back (sub-box kernels; for u32 inside the 1000-source call of the a-7 test above)."""
    import bench
    import make_fullsize_coldens_golden as MC
    from pyc2ray_amd.load_extensions import load_c2ray
    p, lib, capi = asora
    kind, R = MC.CASES[case]
    N, NS = MC.N, MC.NS
    g = np.load(os.path.join(G, "fullsize_coldens.npz"))
    thin, thick, dlog = bench_tables
    np.testing.assert_allclose([thin.sum(), thick.sum()], g["table_sums"], rtol=1e-13)
    ndens, xh, temp, dr, pos, flux = bench.make_workload(kind, N, NS)
    _fresh(p, N)
    p.photo_table_to_device(thin, thick)
    p0, f0 = cases.flat_sources(pos, flux)
    lib.source_data_to_device(p0, f0, NS)
    lib.grid_to_device(capi.GRID_NDENS, ndens)
    lib.grid_to_device(capi.GRID_XH_AV, xh)
    for fortran_constants, rtol in ((1, 1e-9), (0, DEFAULT_MODE_RTOL)):
        lib.set_option(capi.OPT_FORTRAN_CONSTANTS, fortran_constants)
        try:
            cd = lib.debug_coldens(float(R), bench.SIG, dr, NS - 1, N)
        finally:
            lib.set_option(capi.OPT_FORTRAN_CONSTANTS, 0)
        _coldens_cube_against_fixture(cd, case, pos[:, -1], rtol, rated_only=True)
    if case == "u32":
        return
    # the whole cube through the reference's CPU-function API: the last eight sources of the list, host arrays in and out
    p.device_close()
    f = lambda a: np.asfortranarray(a)
    cd, phi, heat = (np.zeros((N, N, N), order="F") for _ in range(3))
    zeros = np.zeros(thin.shape[0])
    nbox, loss = load_c2ray().raytracing.do_all_sources(flux[-8:], pos[:, -8:].astype(np.int32), R, R, cd, bench.SIG, dr, f(ndens), f(xh),
                                                        phi, heat, 0.0, thin, thick, zeros, zeros, bench.MINLOGTAU, dlog, float(R))
    assert nbox == 8
    _coldens_cube_against_fixture(cd, case, pos[:, -1], rtol=1e-11)


# ---- configs[1] ---------------------------------------------------------------------------------------------------
def test_config1_128_single_source_R64_against_oracle(asora):
    """Test 1 geometry: 128^3 uniform, ONE source at (64,64,64), r_RT = 64 (the sphere touches the periodic window:
    24 sector workgroups of 1024 threads).  Raytrace against the oracle, then three steps of the device-resident
    loop against the oracle's restatement of the reference loop (same iteration counts)."""
    import evolve_oracle as EO
    p, lib, capi = asora
    N, R = 128, 64.0
    nd = np.full((N, N, N), 1.87e-4)
    xh = np.full((N, N, N), 1.2e-3)
    temp = np.full((N, N, N), 1e4)
    dr = 5e24 / N
    pos = np.array([[64], [64], [64]])
    flux = np.array([1e6])
    thin, thick, dlog = cases.grey_tables(2000)
    _fresh(p, N)
    p.photo_table_to_device(thin, thick)
    p0, f0 = cases.flat_sources(pos, flux)
    lib.source_data_to_device(p0, f0, 1)
    lib.grid_to_device(capi.GRID_NDENS, nd)
    lib.grid_to_device(capi.GRID_XH_AV, xh)
    lib.raytrace_device(R, cases.SIG, dr, 0, 1, cases.MINLOGTAU, dlog, thin.shape[0])
    phi = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
    ref = O.asora_do_all_sources(R, cases.SIG, dr, nd, xh, p0, f0, thin, thick, cases.MINLOGTAU, dlog,
                                 NumTau=thin.shape[0], flags=O.ASORA_MODE)["phi_ion"]
    # tau = 46 per cell: beyond ~16 cells the grey table's exp(-tau) is denormal, then 0; a rate that is a difference of
    # denormals has no relative accuracy, so the comparison is made where the reference is a normal number
    w = ref > 1e-290
    assert w.sum() > 1000 and np.all(phi[~w] <= 1e-289) and np.all(phi >= 0)
    np.testing.assert_allclose(phi[w], ref[w], rtol=1e-8, atol=0)
    dt = 1.578e15 / 10
    x = xh
    x_ref = xh
    for step in range(2):
        x, _ = p.evolve3D(dt, dr, flux, pos, True, 1000, N, 1e-2, temp, nd, x, thin, thick, cases.MINLOGTAU, dlog, R,
                          1e-4, cases.SIG, cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C,
                          logfile=os.devnull, quiet=True)
        x_ref, _, niter_ref, _ = EO.evolve3D_oracle(dt, dr, flux, pos, temp, nd, x_ref, thin, thick, cases.MINLOGTAU,
                                                    dlog, R, 1e-4, cases.SIG, cases.BH00, cases.ALBPOW, cases.COLH0,
                                                    cases.TEMPH0, cases.ABU_C)
        assert p.evolve._evolve.last_niter == niter_ref
        np.testing.assert_allclose(x, x_ref, rtol=1e-8, atol=0)
