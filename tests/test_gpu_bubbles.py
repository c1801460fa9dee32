"""GPU: the mean-free-path bubble sizes (asora_bubble_mfp, asora_bubble_mask, mfp_distribution, C2Ray.bubble_sizes; DESIGN.md
section 4.2d) against their numpy statement, tests/bubble_reference.py.

* Meshes: N = 17 (odd, one word per row, fewer cells than a launch has threads), 64 (rows of exactly one full word), 70 (two
  words per row, the second with a 6-bit tail) and 136 (three words per row, the third with an 8-bit tail: the popcount walk to a
  start cell passes two words, lane 2 keeps a mask word; 18 496 row counts are five tiles of the scan).  The field is
  uniform-random with a smooth blob laid over it (bubble_reference.blob_field): short rays in the noise, long ones in the blob.
* 4096 rays per call, which is one trip of the ray kernel's grid-stride loop and 16 partial sums; test_many_rays shoots 1 052 709 at
  N = 17: two and three trips per thread, 2048 partials on 256 CUs.
* The mask and the row counts are compared bit for bit; so are the start cells of the rays, and the lengths and statuses of the
  reference march fed the DEVICE's directions (one correctly rounded division and one multiplication per crossing: nothing may
  differ).  The directions themselves agree with numpy's to 4 ulp per component (sqrt, cos, sin and one product).
* The counts and tallies of the production call equal the binning of the per-ray record AND the all-CPU reference with numpy's own
  directions exactly: tests/test_bubble_reference.py shows that 4 ulp of the directions move no ray of these fields across a
  corner, a bin edge or l_max.  The two moments agree to 1e-12 (a sum of n terms in another order: n 2^-53 of the sum of
  magnitudes at worst, 5e-13 for 4096 rays, and far less in practice)."""
import os

import numpy as np
import pytest

import bubble_reference as BR
from test_bubble_reference import GPU_FIELDS, L_MAX, MANY_RAY_CASES, MANY_RAYS, MANY_RAYS_SEED

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BB_PARAMS = os.path.join(HERE, "data", "parameters_single_black_body.yml")
N_RAYS = 4096
SEED = 7


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib, _capi
    if p.cuda_is_init():
        p.device_close()


@pytest.fixture(scope="module", params=GPU_FIELDS, ids=lambda f: f"N{f[0]}")
def box(request, asora):
    """A mesh with the blob field in GRID_XH, and the reference's rays of both phases (computed once, left unchanged)."""
    p, lib, capi = asora
    N, seed = request.param
    field = BR.blob_field(N, seed)
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)
    lib.grid_to_device(capi.GRID_XH, field)
    ref = {}
    for phase in (0, 1):
        mask = BR.in_phase(field, 0.5, phase)
        start, d = BR.rays(mask, SEED, N_RAYS)
        ref[phase] = (mask, start, d)
    return N, field, ref


def _ulps(a, b):
    """the distance of two float64 arrays in units of the spacing at the larger magnitude"""
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_mask_and_row_counts(asora, box):
    p, lib, capi = asora
    N, field, _ = box
    exact = float(field[N // 2, N // 3, N - 1])              # a threshold that equals a cell's value
    for thr in (0.5, exact):
        for phase in (0, 1):
            words, rows = lib.bubble_mask(capi.GRID_XH, thr, phase)
            ref_words, ref_rows = BR.mask_words(BR.in_phase(field, thr, phase))
            assert words.shape == (N, N, (N + 63) // 64) and np.array_equal(words, ref_words), (thr, phase)
            assert np.array_equal(rows, ref_rows), (thr, phase)
    assert lib.bubble_mask(capi.GRID_XH, exact, 0)[0][N // 2, N // 3, (N - 1) >> 6] >> np.uint64((N - 1) & 63) & np.uint64(1) == 1


def test_mask_of_a_grid_with_nans(asora, box):
    p, lib, capi = asora
    N, field, _ = box
    holed = field.copy()
    holed[0, 0, 0] = holed[N - 1, N - 1, N - 1] = holed[N // 2, 1, N // 2] = np.nan
    lib.grid_to_device(capi.GRID_XH_AV, holed)
    with np.errstate(invalid="ignore"):
        for phase in (0, 1):
            words, rows = lib.bubble_mask(capi.GRID_XH_AV, 0.5, phase)
            mask = BR.in_phase(holed, 0.5, phase)
            assert not mask[0, 0, 0] and not mask[N // 2, 1, N // 2]
            ref_words, ref_rows = BR.mask_words(mask)
            assert np.array_equal(words, ref_words) and np.array_equal(rows, ref_rows)


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "open"])
@pytest.mark.parametrize("phase", [0, 1], ids=["ionised", "neutral"])
def test_rays_and_the_production_call(asora, box, phase, periodic):
    p, lib, capi = asora
    N, field, ref = box
    mask, start, d = ref[phase]
    for l_max in L_MAX(N):                                   # below the longest ray, and above it
        edges = np.geomspace(0.5, l_max, 33)
        counts, tallies, moments, rec = lib.bubble_mfp(capi.GRID_XH, 0.5, phase, periodic, SEED, N_RAYS, l_max, edges, record=True)
        r_start, r_dir, r_len, r_status = rec
        # ---- the per-ray record
        assert np.array_equal(r_start, start)
        worst = float(_ulps(r_dir, d).max())
        print(f"N {N}, phase {phase}, periodic {periodic}, l_max {l_max}: directions within {worst:.2f} ulp")
        assert worst <= 4.0
        L, status = BR.march(mask, start, r_dir, l_max, periodic)
        assert np.array_equal(r_status, status)
        assert np.array_equal(r_len, L)                      # bit for bit
        if l_max < N:
            assert np.any(status == BR.CAPPED) and np.any(status == BR.ENDED)
        else:
            assert not np.any(status == BR.CAPPED) and np.any(status == BR.LEFT_BOX) == (not periodic)
        # ---- the binning of the record, and the production call without it
        b_counts, b_tallies, b_moments = BR.bin_lengths(edges, r_len, r_status)
        assert np.array_equal(counts, b_counts) and np.array_equal(tallies[:5], b_tallies) and tallies[5] == mask.sum()
        assert int(tallies[0] + tallies[1] + tallies[2]) == N_RAYS
        p_counts, p_tallies, p_moments = lib.bubble_mfp(capi.GRID_XH, 0.5, phase, periodic, SEED, N_RAYS, l_max, edges)
        assert np.array_equal(p_counts, counts) and np.array_equal(p_tallies, tallies)
        assert p_moments.tobytes() == moments.tobytes()      # two calls, the same bits
        # ---- the all-CPU reference, numpy's own directions
        c_counts, c_tallies, c_moments = BR.distribution(mask, SEED, N_RAYS, l_max, periodic, edges)
        assert np.array_equal(p_counts, c_counts) and np.array_equal(p_tallies, c_tallies)
        rel = np.abs(p_moments - c_moments) / np.abs(c_moments)
        rel_record = np.abs(p_moments - b_moments) / np.abs(b_moments)
        print(f"    moments within {rel.max():.2e} of the reference's and {rel_record.max():.2e} of the record's (relative)")
        assert np.all(rel <= 1e-12) and np.all(rel_record <= 1e-12)


def test_no_grid_changes(asora, box):
    p, lib, capi = asora
    N, field, _ = box
    held = [capi.GRID_NDENS, capi.GRID_XH_AV, capi.GRID_PHI_ION, capi.GRID_TEMP, capi.GRID_XH, capi.GRID_XH_INTERMED]
    for g in held:                                           # every grid holds data of its own
        if g != capi.GRID_XH:
            lib.grid_to_device(g, np.roll(field, g + 1, axis=g % 3) + g)
    before = [lib.grid_sum(g) for g in held]
    snapshot = lib.grid_to_host(capi.GRID_XH, np.empty((N, N, N)))
    lib.bubble_mfp(capi.GRID_XH, 0.5, 0, True, 1, 3000, float(N), np.geomspace(0.5, N, 9))
    lib.bubble_mfp(capi.GRID_XH_AV, 0.3, 1, False, 2, 3000, float(N), np.geomspace(0.5, N, 9), record=True)
    lib.bubble_mask(capi.GRID_XH, 0.7, 1)
    assert [lib.grid_sum(g) for g in held] == before
    assert np.array_equal(lib.grid_to_host(capi.GRID_XH, np.empty((N, N, N))), snapshot) and np.array_equal(snapshot, field)


def test_edge_cases(asora, box):
    p, lib, capi = asora
    N, field, _ = box
    edges = np.geomspace(0.5, N, 17)
    # no in-phase cell: nothing is marched, every output zero but n_phase -- and n_phase = 0 too
    for record in (False, True):
        out = lib.bubble_mfp(capi.GRID_XH, 5.0, 0, True, 3, 1000, float(N), edges, record=record)
        assert not out[0].any() and not out[1].any() and not out[2].any()
        if record:
            assert all(not a.any() for a in out[3])
    # no rays: n_phase alone
    counts, tallies, moments = lib.bubble_mfp(capi.GRID_XH, 0.5, 0, True, 3, 0, float(N), edges)
    assert not counts.any() and tallies.tolist() == [0, 0, 0, 0, 0, int((field >= 0.5).sum())] and not moments.any()
    # ray counts around the workgroup size, one bin, under- and overflow
    mask = field >= 0.5
    for n in (1, 63, 255, 257, 1000):
        e2 = np.array([1.0, 3.0])
        got = lib.bubble_mfp(capi.GRID_XH, 0.5, 0, False, 11, n, float(N), e2)
        want = BR.distribution(mask, 11, n, float(N), False, e2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), n
        assert np.all(np.abs(got[2] - want[2]) <= 1e-12 * np.abs(want[2]))
        assert int(got[0][0] + got[1][3] + got[1][4]) == int(got[1][0])
    assert got[1][3] > 0 and got[1][4] > 0


def test_rays_along_an_axis(asora, box):
    """The in-phase cells form one line along k: every start lies on it.  Whatever the directions, every ray ends, leaves or is
    capped at the finite l_max -- and the call returns; statuses and lengths are the reference's on the device's directions."""
    p, lib, capi = asora
    N, _, _ = box
    line = np.zeros((N, N, N))
    line[N // 2, N // 3, :] = 1.0
    lib.grid_to_device(capi.GRID_XH_AV, line)
    mask = line >= 0.5
    for periodic in (True, False):
        counts, tallies, moments, rec = lib.bubble_mfp(capi.GRID_XH_AV, 0.5, 0, periodic, 0, 2000, 3.0 * N, np.geomspace(0.5, 3.0 * N, 9),
                                                       record=True)
        assert tallies[5] == N and np.all(rec[0][:, :2] == [N // 2, N // 3]) and set(rec[0][:, 2]) == set(range(N))
        L, status = BR.march(mask, rec[0].astype(np.int64), rec[1], 3.0 * N, periodic)
        assert np.array_equal(rec[3], status) and np.array_equal(rec[2], L)
        assert int(tallies[0] + tallies[1] + tallies[2]) == 2000


def test_refusals(asora, box):
    p, lib, capi = asora
    N, _, _ = box
    e = np.geomspace(0.5, N, 5)
    ok = dict(which=capi.GRID_XH, threshold=0.5, phase=0, periodic=True, seed=0, n_rays=10, l_max=float(N), edges=e)
    for change, what in ((dict(which=capi.GRID_CLUMP), "holds no data"), (dict(which=99), "bad grid selector"),
                         (dict(threshold=np.nan), "threshold must be finite"), (dict(threshold=np.inf), "threshold must be finite"),
                         (dict(phase=2), "phase must be"), (dict(n_rays=-1), "n_rays must be"), (dict(l_max=0.0), "l_max must be"),
                         (dict(l_max=np.inf), "l_max must be"), (dict(edges=np.array([1.0])), "n_bins must be"),
                         (dict(edges=np.geomspace(0.5, N, 258)), "n_bins must be"), (dict(edges=np.array([1.0, 1.0, 2.0])), "ascending"),
                         (dict(edges=np.array([2.0, 1.0])), "ascending"), (dict(edges=np.array([1.0, np.nan])), "finite")):
        with pytest.raises(RuntimeError, match=f"bubble_mfp: .*{what}"):
            lib.bubble_mfp(**{**ok, **change})
    import ctypes as C
    raw = lib._lib.asora_bubble_mfp
    cnt, tal, mom = np.zeros(4, dtype=np.uint64), np.zeros(6, dtype=np.uint64), np.zeros(2)
    some = np.zeros(10)
    u64 = lambda a: a.ctypes.data_as(capi._u64p)
    rc = raw(capi.GRID_XH, 0.5, 0, 1, 0, 10, float(N), 4, capi.dptr(e), u64(cnt), u64(tal), capi.dptr(mom), None, None, capi.dptr(some), None)
    assert rc == 3 and b"all four" in lib._lib.asora_last_error()
    assert lib.bubble_mfp(**ok)[1][5] > 0                    # (and the call still works afterwards)


def test_module_entry_and_kernel_timers(asora, box):
    p, lib, capi = asora
    from pyc2ray_amd.bubbles import mfp_distribution
    N, field, ref = box
    lib.set_option(capi.OPT_TIMING, 1)
    lib.kernel_time_reset()
    try:
        b = mfp_distribution(field, n_rays=N_RAYS, seed=SEED, bins=32, l_max=0.45 * N, dr=2.0)
        times = [lib.kernel_time_ms(k) for k in (capi.KERNEL_BUBBLE_MASK, capi.KERNEL_BUBBLE_SCAN, capi.KERNEL_BUBBLE_RAYS)]
    finally:
        lib.set_option(capi.OPT_TIMING, 0)
    assert [t[1] for t in times] == [1, 1, 2] and all(t[0] > 0.0 for t in times)
    counts, tallies, moments = BR.distribution(ref[0][0], SEED, N_RAYS, 0.45 * N, True, np.geomspace(0.5, 0.45 * N, 33))
    assert np.array_equal(b.counts, counts) and [b.ended, b.capped, b.left_box, b.underflow, b.overflow, b.n_phase] == tallies.tolist()
    assert b.mean == pytest.approx(moments[0] / tallies[0], rel=1e-12) and b.mean_phys == 2.0 * b.mean
    assert np.sum(b.RdPdR * b.dlnR) == pytest.approx(1.0, rel=1e-13)
    same = mfp_distribution(None, n_rays=N_RAYS, seed=SEED, bins=32, l_max=0.45 * N)      # the grid where it lies
    assert np.array_equal(same.counts, b.counts) and same.sum_length == b.sum_length and same.dr is None
    neutral = mfp_distribution(None, grid=capi.GRID_XH, phase="neutral", n_rays=500, periodic=False)
    assert neutral.n_phase == N ** 3 - b.n_phase and neutral.l_max == N and neutral.edges.size == 65


def test_many_rays(asora):
    """MANY_RAYS = 1 052 709 rays of the N = 17 field's ionised phase: more than twice the threads of the launch (asserted from the
    device's CU count), so every thread of bubble_rays_kernel carries its two sums and its workgroup's histogram over two rays and
    some over three; and more than 256 workgroups, so bubble_final_kernel's strided loop over the partials takes further turns.
    The structure of test_rays_and_the_production_call; tests/test_bubble_reference.py shows for exactly these rays that 4 ulp of
    the directions move no status and no bin.  Moments: a sum of n positive terms in another order differs by (n - 1) 2^-53 of it
    at most, 1.17e-10."""
    import torch
    p, lib, capi = asora
    N, seed = GPU_FIELDS[0]
    n = MANY_RAYS
    blocks = torch.cuda.get_device_properties(0).multi_processor_count * 8       # bubble_mfp.hip: BM_BLOCKS_PER_CU workgroups of 256
    assert n > 2 * blocks * 256 and (n + 255) // 256 >= blocks > 256, (n, blocks)
    field = BR.blob_field(N, seed)
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)
    lib.grid_to_device(capi.GRID_XH, field)
    mask = BR.in_phase(field, 0.5, 0)
    start, d = BR.rays(mask, MANY_RAYS_SEED, n)
    bound = (n - 1) * 2.0 ** -53
    for periodic, l_max in MANY_RAY_CASES:
        edges = np.geomspace(0.5, l_max, 33)
        counts, tallies, moments, rec = lib.bubble_mfp(capi.GRID_XH, 0.5, 0, periodic, MANY_RAYS_SEED, n, l_max, edges, record=True)
        r_start, r_dir, r_len, r_status = rec
        # ---- the per-ray record
        assert r_start.shape == (n, 3) and np.array_equal(r_start, start)
        worst = float(_ulps(r_dir, d).max())
        print(f"{n} rays, periodic {periodic}, l_max {l_max}: directions within {worst:.2f} ulp")
        assert worst <= 4.0
        L, status = BR.march(mask, start, r_dir, l_max, periodic)
        assert np.array_equal(r_status, status)
        assert np.array_equal(r_len, L)                      # bit for bit
        # ---- the binning of the record, and the production call without it
        b_counts, b_tallies, b_moments = BR.bin_lengths(edges, r_len, r_status)
        assert np.array_equal(counts, b_counts) and np.array_equal(tallies[:5], b_tallies) and tallies[5] == mask.sum()
        assert int(tallies[0] + tallies[1] + tallies[2]) == n and tallies[0] > 0
        p_counts, p_tallies, p_moments = lib.bubble_mfp(capi.GRID_XH, 0.5, 0, periodic, MANY_RAYS_SEED, n, l_max, edges)
        assert np.array_equal(p_counts, counts) and np.array_equal(p_tallies, tallies)
        assert p_moments.tobytes() == moments.tobytes()      # two calls, the same bits
        # ---- the all-CPU reference, numpy's own directions (BR.distribution, its rays computed once for the three runs)
        c_counts, c_tallies, c_moments = BR.bin_lengths(edges, *BR.march(mask, start, d, l_max, periodic))
        assert np.array_equal(p_counts, c_counts) and np.array_equal(p_tallies[:5], c_tallies)
        rel = np.abs(p_moments - c_moments) / np.abs(c_moments)
        rel_record = np.abs(p_moments - b_moments) / np.abs(b_moments)
        print(f"    moments within {rel.max():.2e} of the reference's and {rel_record.max():.2e} of the record's (relative); bound {bound:.2e}")
        assert np.all(rel <= bound) and np.all(rel_record <= bound)


def test_class(asora, tmp_path):
    """The single black-body run at its test mesh, two resident steps: bubble_sizes() reads the ionised fraction where it lies and
    equals the module-level call on a downloaded copy; with the key on every step leaves its result, and the steps are bit for bit
    what they are with the key off."""
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    from pyc2ray_amd.bubbles import mfp_distribution
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N, dt = 24, 3.15576e13
        with open("src.txt", "w") as f:
            f.write("1\n12 12 12 5e50 1.0\n")
        body = open(BB_PARAMS).read()
        marker = [ln for ln in body.splitlines() if ln.strip().startswith("logfile:")][0]
        with open("on.yml", "w") as f:
            f.write(body.replace(marker, marker + "\n  bubble_sizes: 1\n  bubble_rays: 5000\n  bubble_threshold: 0.4\n  bubble_seed: 3"))

        def run(params):
            if p.cuda_is_init():
                p.device_close()
            sim = pc2r.C2Ray_Test(params, N, True)
            sim.density_init(0.0)
            srcpos, srcflux = sim.read_sources("src.txt", 1)
            results = []
            for _ in range(2):
                sim.evolve3D(dt, srcflux, srcpos)
                results.append(sim.last_bubble_sizes)
            return sim, results

        off, off_results = run(BB_PARAMS)
        assert off.device_resident and off.bubble_stats is False and off_results == [None, None]
        kw = dict(n_rays=6000, seed=5, threshold=0.3, bins=24)
        b = off.bubble_sizes(**kw)
        assert off._device_newer >= {"xh", "phi_ion"}          # nothing was fetched
        assert b.periodic is True and b.dr == off.dr and b.n_rays == 6000 and 0 < b.n_phase < N ** 3 and b.ended > 0
        x_off, phi_off = off.xh.copy(), off.phi_ion.copy()      # (downloads)
        m = mfp_distribution(x_off.copy(), dr=off.dr, **kw)
        assert np.array_equal(m.counts, b.counts) and m.sum_length == b.sum_length and m.sum_length2 == b.sum_length2
        assert [m.ended, m.capped, m.left_box, m.underflow, m.overflow, m.n_phase] == [b.ended, b.capped, b.left_box, b.underflow,
                                                                                        b.overflow, b.n_phase]
        assert np.array_equal(m.counts, BR.distribution(x_off >= 0.3, 5, 6000, float(N), True, b.edges)[0])
        again = off.bubble_sizes(**kw)                          # the host copy is the newer one now: the upload form
        assert np.array_equal(again.counts, b.counts) and again.sum_length == b.sum_length

        on, on_results = run("on.yml")
        assert on.bubble_stats is True and all(r is not None for r in on_results) and on_results[0] is not on_results[1]
        last = on_results[1]
        assert (last.n_rays, last.threshold, last.seed, last.dr, last.periodic) == (5000, 0.4, 3, on.dr, True)
        assert on._device_newer >= {"xh", "phi_ion"}
        assert open(on.logfile).read().count("Bubble sizes (ionised") == 2
        assert np.array_equal(on.xh, x_off) and np.array_equal(on.phi_ion, phi_off)
        assert np.array_equal(last.counts, BR.distribution(x_off >= 0.4, 3, 5000, float(N), True, last.edges)[0])
        assert on_results[1].n_phase > on_results[0].n_phase    # the bubble grows
    finally:
        if p.cuda_is_init():
            p.device_close()
        os.chdir(cwd)
