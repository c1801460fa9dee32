"""GPU: the granulometry (asora_granulometry, granulometry, C2Ray.granulometry) against its numpy statement,
tests/granulometry_reference.py.  Everything is integers: every comparison is for equality of arrays, the squared distance transform
is downloaded and compared whole, and every call is made twice and compared byte for byte.

* Meshes: those of the mean-free-path, region and topology tests with their seeds -- N = 17 (one word per row), 64 (rows of exactly
  one full word), 70 (two words with a tail) and 136 (three words, and several trips of the grid-stride loops over the cells).
* Fields: bubble_reference.blob_field at (threshold, phase) = (0.5, both), (0.69, ionised), (0.9, ionised) with both boundaries.
  On these the two boundaries differ in few cells only, so the wrap has fields of its own at N = 70 -- all in phase but one cell, a
  slab through the wrap, a ball about the corner -- each asserted to differ between the boundaries.
* The full box (periodic: unbounded) and the empty phase at N = 64 and 128; N = 128 with single planes out of phase at the word
  boundaries.
* No opened[] is asserted to be monotone: it is not (tests/test_granulometry_reference.py)."""
import os

import numpy as np
import pytest

import bubble_reference as BR
import granulometry_reference as GR
import regions_reference as RR
from test_bubble_reference import GPU_FIELDS
from test_granulometry_reference import BLOB_CASES, BLOB_RADII

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GRANULOMETRY_PARAMS = os.path.join(HERE, "data", "parameters_granulometry.yml")
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_single_black_body.yml")
SMALL_FIELDS = [f for f in GPU_FIELDS if f[0] in (17, 64, 70)]
LARGE_FIELD = [f for f in GPU_FIELDS if f[0] == 136][0]
LARGE_RADII = (1, 2.5, 7, 20)


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


def _call(lib, grid, threshold, phase, periodic, radii):
    """(eroded, opened, tallies, dist2) of the library, made twice and compared byte for byte, and once without the download."""
    got = lib.granulometry(grid, threshold, phase, periodic, radii, distances=True)
    again = lib.granulometry(grid, threshold, phase, periodic, radii, distances=True)
    plain = lib.granulometry(grid, threshold, phase, periodic, radii)
    assert len(got) == 4 and len(plain) == 3
    assert [a.dtype for a in got] == [np.uint64, np.uint64, np.uint64, np.uint32] and got[2].shape == (4,)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(got, plain):
        assert a.tobytes() == b.tobytes()
    return got


def _check(got, want, what=""):
    """`want`: (eroded, opened, tallies, dist2) of the reference"""
    print(f"{what}: eroded {got[0].tolist()}, opened {got[1].tolist()}, tallies {got[2].tolist()}; reference {want[0].tolist()}, "
          f"{want[1].tolist()}, {want[2].tolist()}")
    assert np.array_equal(got[3], want[3]), (what, "dist2", int(np.count_nonzero(got[3] != want[3])))
    for name, g, w in zip(("eroded", "opened", "tallies"), got, want):
        assert np.array_equal(g, w), (what, name, g.tolist(), w.tolist())


def _run_mask(asora, mask, periodic, radii, want=None, what=""):
    """The library on a boolean mask (uploaded as 0 / 1 into GRID_XH_AV, threshold 0.5) next to the reference."""
    p, lib, capi = asora
    lib.grid_to_device(capi.GRID_XH_AV, mask.astype(np.float64))
    got = _call(lib, capi.GRID_XH_AV, 0.5, 0, periodic, radii)
    _check(got, GR.counts(mask, periodic, radii) if want is None else want, what)
    return got


@pytest.fixture(scope="module", params=SMALL_FIELDS, ids=lambda f: f"N{f[0]}")
def box(request, asora):
    """A mesh with the blob field in GRID_XH; the references of its cases are computed as they are first asked for and kept."""
    p, lib, capi = asora
    N, seed = request.param
    field = BR.blob_field(N, seed)
    _mesh(asora, N)
    lib.grid_to_device(capi.GRID_XH, field)
    kept = {}

    def reference(threshold, phase, periodic, radii=BLOB_RADII):
        key = (threshold, phase, periodic, tuple(radii))
        if key not in kept:
            kept[key] = GR.counts(BR.in_phase(field, threshold, phase), periodic, radii)
        return kept[key]
    return N, field, reference


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "open"])
@pytest.mark.parametrize("case", BLOB_CASES, ids=lambda c: f"x{c[0]}-phase{c[1]}")
def test_blob_fields(asora, box, case, periodic):
    p, lib, capi = asora
    N, field, reference = box
    threshold, phase = case
    want = reference(threshold, phase, periodic)
    got = _call(lib, capi.GRID_XH, threshold, phase, periodic, BLOB_RADII)
    _check(got, want, f"N {N}, {case}, periodic {periodic}")
    assert want[2][0] == BR.in_phase(field, threshold, phase).sum() and want[0][0] > 0 and want[2][2] == 0
    assert np.all(want[1] <= want[2][0]) and np.all(want[0] <= want[1])         # (centres lie in their balls, balls in the phase)


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "open"])
def test_blob_field_of_three_words_and_several_trips(asora, periodic):
    p, lib, capi = asora
    N, seed = LARGE_FIELD
    assert N == 136
    field = BR.blob_field(N, seed)
    _mesh(asora, N)
    lib.grid_to_device(capi.GRID_XH, field)
    got = _call(lib, capi.GRID_XH, 0.5, 0, periodic, LARGE_RADII)
    _check(got, GR.counts(BR.in_phase(field, 0.5, 0), periodic, LARGE_RADII), f"N {N}, periodic {periodic}")
    assert got[0][-1] > 0                                                   # (the blob holds a ball of radius 20)


def test_wrap_all_in_phase_but_one_cell(asora):
    """N = 70: D2 is the minimum-image |c|^2 in the periodic box, d2_max = 3 * 35^2; in the open box the faces bound it."""
    N = 70
    _mesh(asora, N)
    mask = GR.one_cell_out(N)
    g = np.arange(N)
    image = np.minimum(g, N - g) ** 2
    by_hand = (image[:, None, None] + image[None, :, None] + image[None, None, :]).astype(np.uint32)
    radii = (1, 5, 34.9, 35, 60)
    got = _run_mask(asora, mask, True, radii, GR.counts_from_dist2(by_hand, True, radii) + (by_hand,), "one cell out, periodic")
    assert got[2].tolist() == [N ** 3 - 1, 3675, 0, int(by_hand.sum())]
    assert got[0][-1] == np.count_nonzero(by_hand > 3600) > 0
    other = _run_mask(asora, mask, False, radii, None, "one cell out, open")
    assert other[2][1] == 35 ** 2 and other[0][-2] == 0 and np.count_nonzero(other[3] != got[3]) > N ** 3 // 2


def test_wrap_slab(asora):
    """N = 70, the slab k in {67, 68, 69, 0, 1, 2}: six planes thick through the wrap, two slabs of three planes in the open box."""
    N = 70
    _mesh(asora, N)
    mask = GR.wrap_slab(N)
    got = _run_mask(asora, mask, True, (0, 1, 2, 3), None, "slab, periodic")
    assert got[0].tolist() == [6 * N * N, 4 * N * N, 2 * N * N, 0]
    assert got[1].tolist() == [6 * N * N, 6 * N * N, 6 * N * N, 0]
    assert got[2].tolist() == [6 * N * N, 9, 0, 28 * N * N]
    other = _run_mask(asora, mask, False, (0, 1, 2, 3), None, "slab, open")
    assert other[0].tolist() == [6 * N * N, 2 * (N - 2) ** 2, 0, 0] and other[2][1] == 4


def test_wrap_ball_about_the_corner(asora):
    N = 70
    _mesh(asora, N)
    mask = GR.corner_ball(N, 6)
    radii = (1, 2, 3.5, 6, 7)
    got = _run_mask(asora, mask, True, radii, None, "corner ball, periodic")
    assert got[2][1] == 37 and got[0][3] == 1 and got[1][3] == mask.sum() and got[0][4] == got[1][4] == 0
    other = _run_mask(asora, mask, False, radii, None, "corner ball, open")
    assert other[2][1] < 37 and other[0][3] == 0 and other[1][1] < got[1][1]


@pytest.mark.parametrize("N", [64, 128])
def test_full_and_empty_box(asora, N):
    p, lib, capi = asora
    _mesh(asora, N)
    full = np.ones((N, N, N), dtype=bool)
    radii = (1, 3, 20, 31.9, N / 2)
    # periodic: no cell outside the phase -- unbounded, and every opening keeps everything
    everything = np.full(len(radii), N ** 3, dtype=np.uint64)
    want = (everything, everything, np.array([N ** 3, 0, N ** 3, 0], dtype=np.uint64), np.full((N, N, N), GR.UNBOUNDED, dtype=np.uint32))
    _run_mask(asora, full, True, radii, want, "full, periodic")
    # open: the distance to the nearest face
    g = np.arange(N)
    face = np.minimum(g + 1, N - g)
    by_hand = (np.minimum(np.minimum(face[:, None, None], face[None, :, None]), face[None, None, :]) ** 2).astype(np.uint32)
    got = _run_mask(asora, full, False, radii, GR.counts_from_dist2(by_hand, False, radii) + (by_hand,), "full, open")
    assert got[2][1] == (N // 2) ** 2 and got[0].tolist() == [max(N - 2 * int(r), 0) ** 3 for r in radii]
    # the empty phase
    nothing = np.zeros(len(radii), dtype=np.uint64)
    for periodic in (True, False):
        want = (nothing, nothing, np.zeros(4, dtype=np.uint64), np.zeros((N, N, N), dtype=np.uint32))
        _run_mask(asora, ~full, periodic, radii, want, "empty")


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "open"])
def test_word_boundary(asora, periodic):
    """N = 128: two full words per row, all in phase but single planes of k at the ends of the words -- the carry between the words,
    the carry through the wrap and, in the open box, the exterior behind the last bit."""
    N = 128
    _mesh(asora, N)
    radii = (1, 2, 5)
    for planes in ((127,), (0,), (0, 127), (63,), (64,)):
        by_hand = GR.planes_dist2(N, planes, periodic)
        want = GR.counts_from_dist2(by_hand, periodic, radii) + (by_hand,)
        got = _run_mask(asora, GR.planes_out(N, planes), periodic, radii, want, f"planes {planes}, periodic {periodic}")
        assert got[2][0] == N * N * (N - len(planes))
        if periodic:
            assert got[2][1] == {1: 64 ** 2, 2: 63 ** 2}[len(planes)]


def test_a_nan_cell_is_in_neither_phase_and_the_grid_is_unchanged(asora):
    p, lib, capi = asora
    N, seed = GPU_FIELDS[0]
    assert N == 17
    _mesh(asora, N)
    field = BR.blob_field(N, seed)
    field[8, 8, 8] = np.nan
    lib.grid_to_device(capi.GRID_XH, field)
    before = lib.grid_to_host(capi.GRID_XH, np.empty((N, N, N))).tobytes()
    assert before == field.tobytes()
    with np.errstate(invalid="ignore"):
        for phase in (0, 1):
            mask = BR.in_phase(field, 0.5, phase)
            assert not mask[8, 8, 8]
            for periodic in (True, False):
                got = _call(lib, capi.GRID_XH, 0.5, phase, periodic, (1, 2, 3))
                _check(got, GR.counts(mask, periodic, (1, 2, 3)), f"NaN, phase {phase}, periodic {periodic}")
                assert got[3][8, 8, 8] == 0
    assert lib.grid_to_host(capi.GRID_XH, np.empty((N, N, N))).tobytes() == before


def test_the_calls_that_share_its_buffers_are_undisturbed(asora, box):
    """region_sizes and topology use the two uint32 grids the transform goes through: their results before a granulometry call are
    their results after it, and no grid changes."""
    p, lib, capi = asora
    N, field, reference = box
    edges = RR.default_edges(N)
    before = lib.grid_to_host(capi.GRID_XH, np.empty((N, N, N))).tobytes()
    regions = lib.region_sizes(capi.GRID_XH, 0.69, 0, True, 6, edges, labels=True)
    topo = [lib.topology(capi.GRID_XH, 0.5, 0, periodic, 26) for periodic in (True, False)]
    got = lib.granulometry(capi.GRID_XH, 0.5, 0, False, BLOB_RADII, distances=True)
    for a, b in zip(regions, lib.region_sizes(capi.GRID_XH, 0.69, 0, True, 6, edges, labels=True)):
        assert a.tobytes() == b.tobytes()
    lib.granulometry(capi.GRID_XH, 0.9, 0, True, BLOB_RADII)
    for a, periodic in zip(topo, (True, False)):
        assert a.tobytes() == lib.topology(capi.GRID_XH, 0.5, 0, periodic, 26).tobytes()
    # ... and the other way round
    for a, b in zip(got, lib.granulometry(capi.GRID_XH, 0.5, 0, False, BLOB_RADII, distances=True)):
        assert a.tobytes() == b.tobytes()
    assert got[2][0] == topo[0][0] == BR.in_phase(field, 0.5, 0).sum()
    assert lib.grid_to_host(capi.GRID_XH, np.empty((N, N, N))).tobytes() == before == field.tobytes()


def test_module_entry(asora, box):
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    N, field, reference = box
    g = pc2r.granulometry(field, threshold=0.69, periodic=False, radii=BLOB_RADII, dr=2.0, distances=True)
    want = reference(0.69, 0, False)
    assert isinstance(g, pc2r.Granulometry)
    for mine, theirs in zip((g.eroded, g.opened, g.tallies, g.dist2), want):
        assert np.array_equal(mine, theirs)
    assert g.r2.tolist() == GR.r2_of(BLOB_RADII).tolist() and g.N == N and g.dr == 2.0 and g.periodic is False
    assert g.n_phase == want[2][0] and g.max_inscribed_r2 == int(want[2][1]) - 1 and g.mean_radius_phys == 2.0 * g.mean_radius
    assert np.array_equal(g.cumulative, 1.0 - want[1] / float(want[2][0])) and abs(g.dF.sum() + g.unresolved - 1.0) < 1e-12
    same = pc2r.granulometry(None, threshold=0.69, periodic=False, radii=BLOB_RADII)           # the grid where it lies
    assert np.array_equal(same.opened, g.opened) and np.array_equal(same.tallies, g.tallies) and same.dr is None and same.dist2 is None
    default = pc2r.granulometry(None, grid=capi.GRID_XH, phase="neutral", threshold=0.69)
    n = max(1, min(N // 4, 32))
    assert default.radii.tolist() == list(range(1, n + 1)) and default.n_phase == N ** 3 - g.n_phase
    few = pc2r.granulometry(None, phase="neutral", threshold=0.69, radii=3)
    assert few.radii.tolist() == [1.0, 2.0, 3.0] and np.array_equal(few.opened, default.opened[:3])
    assert np.array_equal(few.opened, GR.counts(BR.in_phase(field, 0.69, 1), True, (1, 2, 3))[1])


def test_refusals(asora, box):
    p, lib, capi = asora
    ok = dict(which=capi.GRID_XH, threshold=0.5, phase=0, periodic=True, radii=(1.0, 2.0))
    for change, what in ((dict(which=capi.GRID_CLUMP), "holds no data"), (dict(which=99), "bad grid selector"),
                         (dict(threshold=np.nan), "threshold must be finite"), (dict(threshold=np.inf), "threshold must be finite"),
                         (dict(phase=2), "phase must be"), (dict(radii=()), "n_radii must be in"),
                         (dict(radii=np.arange(1.0, 258.0)), "n_radii must be in"), (dict(radii=(1.0, np.nan)), "radii must be finite"),
                         (dict(radii=(1.0, np.inf)), "radii must be finite"), (dict(radii=(-1.0, 2.0)), "radii must be >= 0"),
                         (dict(radii=(1.0, 1.0)), "strictly ascending"), (dict(radii=(2.0, 1.0)), "strictly ascending"),
                         (dict(radii=(1.0, 46341.0)), "R\\^2 < 2\\^31")):
        with pytest.raises(RuntimeError, match=f"granulometry: .*{what}"):
            lib.granulometry(**{**ok, **change})
    raw = lib._lib.asora_granulometry
    u64 = lambda a: a.ctypes.data_as(capi._u64p)
    radii = np.array([1.0, 2.0])
    e, o, t = np.full(2, 9, dtype=np.uint64), np.full(2, 9, dtype=np.uint64), np.full(4, 9, dtype=np.uint64)
    untouched = lambda: np.all(e == 9) and np.all(o == 9) and np.all(t == 9)
    for args in ((None, u64(e), u64(o), u64(t)), (capi.dptr(radii), None, u64(o), u64(t)), (capi.dptr(radii), u64(e), None, u64(t)),
                 (capi.dptr(radii), u64(e), u64(o), None)):
        assert raw(capi.GRID_XH, 0.5, 0, 1, 2, *args, None) == 3 and b"null" in lib._lib.asora_last_error()
    assert raw(capi.GRID_XH, 0.5, 0, 1, 0, capi.dptr(radii), u64(e), u64(o), u64(t), None) == 3 and untouched()
    assert raw(capi.GRID_XH, 0.5, 3, 1, 2, capi.dptr(radii), u64(e), u64(o), u64(t), None) == 3 and untouched()
    assert raw(capi.GRID_CLUMP, 0.5, 0, 1, 2, capi.dptr(radii), u64(e), u64(o), u64(t), None) == 4 and untouched()
    assert lib.granulometry(**ok)[2][0] > 0                            # (and the call still works afterwards)
    largest = lib.granulometry(**{**ok, "radii": (0.0, 46340.9)})       # R = 0 and the largest R^2 below 2^31 are taken
    assert largest[0][0] == largest[1][0] == largest[2][0] and largest[0][1] == largest[1][1] == 0
    p.device_close()                                                    # before device_init: code 2
    assert raw(capi.GRID_XH, 0.5, 0, 1, 2, capi.dptr(radii), u64(e), u64(o), u64(t), None) == 2 and untouched()
    assert b"granulometry" in lib._lib.asora_last_error()
    N, field, reference = box                                           # (the mesh and its field back for whoever comes next)
    _mesh(asora, N)
    lib.grid_to_device(capi.GRID_XH, field)


def test_class(asora, tmp_path):
    """The single black-body run at its test mesh with the granulometry keys: every step on the resident path leaves its granulometry
    and one line in the log; granulometry() reads the ionised fraction where it lies and equals the module-level call on a
    downloaded copy."""
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N, dt = 24, 3.15576e13
        with open("src.txt", "w") as f:
            f.write("1\n12 12 12 5e50 1.0\n")

        def run(params, resident):
            if p.cuda_is_init():
                p.device_close()
            sim = pc2r.C2Ray_Test(params, N, True)
            sim.device_resident = resident
            sim.density_init(0.0)
            srcpos, srcflux = sim.read_sources("src.txt", 1)
            results = []
            for _ in range(2):
                sim.evolve3D(dt, srcflux, srcpos)
                results.append(sim.last_granulometry)
            return sim, results

        off, off_results = run(PLAIN_PARAMS, True)
        assert off.device_resident and off.granulometry_stats is False and off_results == [None, None]
        for periodic in (True, False):
            g = off.granulometry(radii=4, periodic=periodic, distances=True)
            assert off._device_newer >= {"xh", "phi_ion"}       # nothing was fetched
            assert (g.periodic, g.dr, g.threshold, g.N) == (periodic, off.dr, 0.5, N) and 0 < g.n_phase < N ** 3
            assert g.radii.tolist() == [1.0, 2.0, 3.0, 4.0] and g.dist2.shape == (N, N, N)
            if not periodic:
                resident_open = g
        assert off.granulometry().radii.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]       # (the default: 1 ... N // 4)
        x_off = off.xh.copy()                                   # (downloads)
        m = pc2r.granulometry(x_off.copy(), radii=4, periodic=False, dr=off.dr, distances=True)
        want = GR.counts(x_off >= 0.5, False, (1, 2, 3, 4))
        for mine, resident, theirs in zip((m.eroded, m.opened, m.tallies, m.dist2),
                                          (resident_open.eroded, resident_open.opened, resident_open.tallies, resident_open.dist2), want):
            assert np.array_equal(mine, theirs) and np.array_equal(resident, theirs)
        again = off.granulometry(radii=4, periodic=False)       # the host copy is the newer one now: the upload form
        assert np.array_equal(again.opened, m.opened) and again.dist2 is None

        on, on_results = run(GRANULOMETRY_PARAMS, True)
        assert on.device_resident and on.granulometry_stats is True
        assert all(res is not None for res in on_results) and on_results[0] is not on_results[1]
        last = on_results[1]
        assert (last.threshold, last.dr, last.periodic, last.radii.tolist()) == (0.4, on.dr, True, [1.0, 2.0, 3.0, 4.0, 5.0])
        assert open(on.logfile).read().count("Granulometry (ionised, x >= 0.4, periodic, 5 radii to 5): ") == 2
        x_on = on.xh.copy()
        assert np.array_equal(x_on, x_off)                      # the analysis changes nothing of the step
        want = GR.counts(x_on >= 0.4, True, (1, 2, 3, 4, 5))
        assert np.array_equal(last.eroded, want[0]) and np.array_equal(last.opened, want[1]) and np.array_equal(last.tallies, want[2])
        assert last.n_phase > on_results[0].n_phase and last.d2_max >= on_results[0].d2_max      # one bubble around the source, and it grows
    finally:
        if p.cuda_is_init():
            p.device_close()
        os.chdir(cwd)
