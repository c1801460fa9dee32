"""GPU: device_close frees what the mesh owned, whatever has been used, and a re-initialised library computes what a fresh one does.

Three cycles in one process at meshes 24, 16 and 24.  Each cycle uploads every kind of input, calls every entry point that allocates
on first use once, and closes.  The descending step comes first: a buffer that wrongly survived a close is then larger than the next
mesh needs, not smaller, and the assertion that nothing is live stands before every re-initialisation -- a buffer left behind fails
an assertion and never reaches a kernel.  Between the closes the process-lifetime memory (asora_debug_live_buffers(1)) must not grow.

The third cycle is compared with the first, both at mesh 24: the analyses form every sum in a fixed order and must agree bit for bit;
the rates of the evolve steps come from atomics and agree to rtol = 1e-10, the tolerance of
test_gpu_parity.py::test_grids_placed_by_probe_give_the_same_results for the same comparison.  The first cycle's analyses are also
checked against their CPU references, under the bounds of their own test files, so that a result cannot pass by being wrong twice."""
import numpy as np
import pytest

import bubble_reference as BR
import cases
import granulometry_reference as GR
import powerspec_reference as PR
import redshift_space_reference as RS
import regions_reference as RG
import topology_reference as TR

pytestmark = pytest.mark.gpu

MESHES = (24, 16, 24)
CHEM = (cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)
DT = 3.15576e13
N_RAYS, RAY_SEED, LOS_AXIS = 2000, 5, 1
RADII = np.array([1.0, 1.5, 2.0, 3.0])
ARENA_GRIDS = 14            # api.hip: ARENA_SLOTS
RATE_KEYS = ("evolve_xh", "evolve_phi_ion", "evolve_phi_heat", "slab_xh", "slab_phi_ion", "slab_phi_heat", "trace_phi_ion",
             "trace_phi_heat", "subbox_phi_ion")


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib, _capi
    lib.set_option(_capi.OPT_HEATING, 0)
    if p.cuda_is_init():
        lib.thermal_params(False)
        lib.clumping(0)
        p.device_close()


def _inputs(N):
    """Everything a cycle uploads, a function of N alone."""
    rng = np.random.default_rng(4100 + N)
    thin, thick, hthin, hthick, dlog = cases.blackbody_photo_and_heat_tables(num_tau=600)
    nd, xh, dr = cases.grid(N, "lognormal", 4100 + N, 0.3, xlo=1e-4, xhi=2e-3)
    h = N // 2
    pts = np.array([(1 + a * h, 1 + b * h, 1 + c * h) for a in (0, 1) for b in (0, 1) for c in (0, 1)]).T
    two = lambda t: np.stack([t, 0.5 * t])                  # the second table set: half the first
    return dict(N=N, ndens=nd, xh=xh, dr=dr, dlog=dlog, temp=10 ** rng.uniform(2.0, 4.0, size=(N, N, N)),
                tables=(two(thin), two(thick), two(hthin), two(hthick)), numtau=thin.shape[0],
                pos=pts[:, [0, 3, 5, 6, 7]], flux=rng.uniform(0.5, 2.0, size=5) * 3e-4 * (N / 16.0) ** 3 / 5,
                spec=np.array([0, 1, 0, 1, 1], dtype=np.int32), clump=1.0 + rng.random((N, N, N)),
                velocity=rng.uniform(-0.999, 0.999, size=(N, N, N)) * 40.0, velocity_scale=1.0 / 40.0,
                field=BR.blob_field(N, 4100 + N), R=2.5,
                thr=PR.thresholds_of(np.arange(0, N // 2 + 1) + 0.5), thr_mu=np.array([0.0, 0.5, 2.0]))


def _cycle(asora, c):
    """device_init(N) ... every lazily allocating entry point once ... what they returned, with the device still open."""
    p, lib, capi = asora
    N, ns = c["N"], c["flux"].shape[0]
    grid = lambda which: lib.grid_to_host(which, np.empty((N, N, N)))
    out = {}
    p.device_init(N, 8)
    # ---- 1. the uploads
    for which, a in ((capi.GRID_NDENS, c["ndens"]), (capi.GRID_XH, c["xh"]), (capi.GRID_TEMP, c["temp"]), (capi.GRID_CLUMP, c["clump"])):
        lib.grid_to_device(which, a)
    thin1, thick1, hthin1, hthick1 = (t[0] for t in c["tables"])
    lib.photo_table_to_device(thin1, thick1, c["numtau"])
    lib.heat_table_to_device(hthin1, hthick1, c["numtau"])
    lib.spectra_to_device(*c["tables"])                     # (replaces the one set by two)
    lib.source_data_to_device(*cases.flat_sources(c["pos"], c["flux"]), ns)
    lib.clumping(2)
    assert lib.los_velocity_to_device(c["velocity"]) == float(np.max(np.abs(c["velocity"])))
    lib.thermal_params(True, 0.1, 1.0, 200, 31, False, 0.0)
    trace = (c["R"], cases.SIG, c["dr"], cases.MINLOGTAU, c["dlog"], c["numtau"])
    step = (DT, *CHEM, *trace, 0, ns, -1.0, 0.0)
    # ---- 2. the sub-box sweep: it has one spectrum for all sources, so it runs before the sources get table sets of their own
    lib.grid_copy(capi.GRID_XH_AV, capi.GRID_XH)
    lib.set_option(capi.OPT_HEATING, 1)
    out["subbox"] = lib.subbox_raytrace_device(1000, 5, 1e-2, *trace, 0, ns)
    out["subbox_phi_ion"] = grid(capi.GRID_PHI_ION)
    lib.source_spectra_to_device(c["spec"])
    # ---- the whole-box trace with heating
    lib.raytrace_device(c["R"], cases.SIG, c["dr"], 0, ns, cases.MINLOGTAU, c["dlog"], c["numtau"])
    out["trace_phi_ion"], out["trace_phi_heat"] = grid(capi.GRID_PHI_ION), grid(capi.GRID_PHI_HEAT)
    lib.set_option(capi.OPT_HEATING, 0)
    # ---- one thermal step of the device loop, and its budget
    lib.evolve_begin(*step)
    lib.evolve_enqueue(2)
    niter, _, rows = lib.evolve_poll(8)
    assert niter == 2 and len(rows) == 2
    out["evolve_xh"], out["evolve_phi_ion"], out["evolve_phi_heat"] = (grid(g) for g in (capi.GRID_XH_INTERMED, capi.GRID_PHI_ION, capi.GRID_PHI_HEAT))
    out["budget"] = lib.step_budget((DT, *CHEM), use_temp_end=True)
    # ---- one thermal step of the sharded loop that owns every plane: the heating out-box
    lib.evolve_begin_slab_thermal(*step, 0, N)
    lib.evolve_slab_trace(0, ns)
    lib.evolve_slab_fold_all()
    lib.evolve_slab_pass()
    lib.evolve_slab_close(None)
    assert lib.evolve_poll(8)[0] == 1
    out["slab_xh"], out["slab_phi_ion"], out["slab_phi_heat"] = (grid(g) for g in (capi.GRID_XH_INTERMED, capi.GRID_PHI_ION, capi.GRID_PHI_HEAT))
    # ---- the analyses, on a field with structure
    lib.grid_to_device(capi.GRID_XH, c["field"])
    out["bubbles"] = lib.bubble_mfp(capi.GRID_XH, 0.5, 0, True, RAY_SEED, N_RAYS, 0.45 * N, np.geomspace(0.5, 0.45 * N, 17), record=True)
    out["regions"] = lib.region_sizes(capi.GRID_XH, 0.5, 0, True, 6, RG.default_edges(N), labels=True)
    out["topology"] = lib.topology(capi.GRID_XH, 0.5, 0, True, 6)
    out["granulometry"] = lib.granulometry(capi.GRID_XH, 0.5, 0, True, RADII, distances=True)
    out["power"] = lib.power_spectrum(capi.PS_XH, capi.PS_DENSITY, 1.0, 0.0, c["thr"])
    out["smooth"] = lib.smooth_field(capi.PS_XH, 1.0, 0.0, field=True)
    out["los"] = lib.power_spectrum_los(capi.PS_XH, 1.0, 0.0, LOS_AXIS, c["velocity_scale"], capi.ANISO_MU, c["thr"], c["thr_mu"], field=True)
    out["rs_field"] = lib.redshift_space_field(capi.PS_XH, 1.0, 0.0, LOS_AXIS, c["velocity_scale"], field=True)
    return out


def _flat(value):
    """the arrays of a result, whatever it is made of"""
    if isinstance(value, dict):
        return [a for key in sorted(value) for a in _flat(value[key])]
    if isinstance(value, (tuple, list)):
        return [a for v in value for a in _flat(v)]
    return [] if value is None else [np.asarray(value)]


def _against_references(c, out):
    N, field, x = c["N"], c["field"], c["field"]
    mask = BR.in_phase(field, 0.5, 0)
    edges = np.geomspace(0.5, 0.45 * N, 17)
    # bubbles: counts and tallies exactly, the moments as tests/test_gpu_bubbles.py bounds them
    counts, tallies, moments, rec = out["bubbles"]
    w_counts, w_tallies, w_moments = BR.distribution(mask, RAY_SEED, N_RAYS, 0.45 * N, True, edges)
    assert np.array_equal(counts, w_counts) and np.array_equal(tallies[:5], w_tallies[:5]) and tallies[5] == mask.sum()
    assert np.all(np.abs(moments - w_moments) <= 1e-12 * np.abs(w_moments))
    L, status = BR.march(mask, rec[0].astype(np.int64), rec[1], 0.45 * N, True)
    assert np.array_equal(rec[3], status) and np.array_equal(rec[2], L)
    # regions, topology, granulometry: integers
    w_labels, w_counts, w_cells, w_tallies = RG.sizes(mask, 6, True, RG.default_edges(N))
    got = out["regions"]
    assert np.array_equal(got[3], w_labels) and all(np.array_equal(g, w) for g, w in zip(got[:3], (w_counts, w_cells, w_tallies)))
    assert np.array_equal(out["topology"], TR.tallies(mask, 6, True))
    want = GR.counts(mask, True, RADII)
    assert len(want) == 4 and all(np.array_equal(g, w) for g, w in zip(out["granulometry"], want))
    # the power sums, under the bounds of tests/test_gpu_powerspec.py
    cN = PR.c_of_N(N)
    got, want = out["power"], PR.power_sums(x, c["thr"], PR.form_field(PR.DENSITY, n=c["ndens"]))
    assert np.array_equal(got["count"], want["count"]) and np.all(np.abs(got["sum_k"] - want["sum_k"]) <= 1e-13 * want["sum_k"])
    for key, tot in (("sum_aa", "total_aa"), ("sum_bb", "total_bb")):
        assert np.all(np.abs(got[key] - want[key]) <= 4.0 * cN * np.sqrt(want[key] * want[tot])), key
    bound = 4.0 * cN * (np.sqrt(want["sum_aa"] * want["total_bb"]) + np.sqrt(want["sum_bb"] * want["total_aa"]))
    assert np.all(np.abs(got["sum_ab"] - want["sum_ab"]) <= bound)
    # smoothing without a filter is the round trip (tests/test_gpu_smoothing.py)
    h = out["smooth"]["field"]
    assert np.linalg.norm((h - x).ravel()) <= 2.5 * cN * np.linalg.norm(x.ravel())
    # redshift space: the mapping bit for bit, the sums under the bounds of tests/test_gpu_redshift_space.py
    mapped = RS.map_lines(x, c["velocity"], c["velocity_scale"], LOS_AXIS)
    assert out["los"]["field"].tobytes() == mapped.tobytes() == out["rs_field"]["field"].tobytes()
    got, want = out["los"], RS.binned(N, LOS_AXIS, RS.MU, c["thr"], c["thr_mu"], np.fft.rfftn(mapped))
    assert np.array_equal(got["count"], want["count"])
    for key in ("sum_1", "sum_2"):
        assert np.all(np.abs(got[key] - want[key]) <= 1e-13 * want[key]), key
    for key in ("sum_aa", "sum_l2", "sum_l4"):
        assert np.all(np.abs(got[key] - want[key]) <= 4.0 * cN * np.sqrt(want["sum_aa"] * want["total_aa"])), key


def test_close_and_reinitialise_with_every_feature_used(asora):
    p, lib, capi = asora
    if p.cuda_is_init():
        p.device_close()
    assert lib.live_buffers(0) == (0, 0)
    results, process = [], []
    for cycle, N in enumerate(MESHES):
        c = _inputs(N)
        try:
            out = _cycle(asora, c)
            count, nbytes = lib.live_buffers(0)
            print(f"cycle {cycle}, N {N}: {count} mesh buffers of {nbytes} bytes, process {lib.live_buffers(1)}")
            assert count > 0 and nbytes >= ARENA_GRIDS * N ** 3 * 8
        finally:
            lib.set_option(capi.OPT_HEATING, 0)
            if p.cuda_is_init():
                p.device_close()
        assert lib.live_buffers(0) == (0, 0)                # before anything else runs
        process.append(lib.live_buffers(1))
        assert process[-1][0] > 0 and process[-1] == process[0], process
        if cycle == 0:
            _against_references(c, out)
        results.append(out)
    first, third = results[0], results[2]
    assert first["subbox"][0] == third["subbox"][0]
    for key in RATE_KEYS:
        assert np.any(first[key] > 0), key
        np.testing.assert_allclose(third[key], first[key], rtol=1e-10, atol=0, err_msg=key)
    for key in ("bubbles", "regions", "topology", "granulometry", "power", "smooth", "los", "rs_field"):
        a, b = _flat(first[key]), _flat(third[key])
        assert len(a) == len(b) > 0 and all(u.tobytes() == v.tobytes() for u, v in zip(a, b)), key
