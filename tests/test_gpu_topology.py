"""GPU: the topology (asora_topology, topology, C2Ray.topology) against its numpy statement,
tests/topology_reference.py.  Everything is integers: every comparison is for equality of uint64 arrays.

* Meshes: those of the mean-free-path and region tests with their seeds -- N = 17 (one word per row), 64 (rows of exactly one full
  word: the open box's bit N falls into a word the mask does not have), 70 (two words with a tail) and 136 (three words, and several
  trips of the grid-stride loops over the cells).
* Fields: bubble_reference.blob_field at (threshold, phase) = (0.5, both), (0.69, ionised), (0.9, ionised), each with both
  connectivities and both boundaries, which differ in every one of them (asserted), so a missing or a spurious wrap cannot pass.
* N = 128, all in phase but the plane k = 127: the word boundary, the carry through the wrap and bit N together.
* The hand shapes of tests/test_topology_reference.py and the full box at N = 2, 3, 5 (N = 1 is not a mesh of device_init)."""
import os

import numpy as np
import pytest

import bubble_reference as BR
import regions_reference as RR
import topology_reference as TR
from test_bubble_reference import GPU_FIELDS
from test_topology_reference import BLOB_CASES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOPOLOGY_PARAMS = os.path.join(HERE, "data", "parameters_topology.yml")
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_single_black_body.yml")
T = TR.T


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


@pytest.fixture(scope="module", params=GPU_FIELDS, ids=lambda f: f"N{f[0]}")
def box(request, asora):
    """A mesh with the blob field in GRID_XH, and the references of its cases, computed as they are first asked for and kept
    (topology_reference.shared_reference, which tests/test_topology_reference.py checks against the plain statement)."""
    p, lib, capi = asora
    N, seed = request.param
    field = BR.blob_field(N, seed)
    _mesh(asora, N)
    lib.grid_to_device(capi.GRID_XH, field)
    return N, field, TR.shared_reference(field)


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "open"])
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("case", BLOB_CASES, ids=lambda c: f"x{c[0]}-phase{c[1]}")
def test_blob_fields(asora, box, case, connectivity, periodic):
    p, lib, capi = asora
    N, field, reference = box
    threshold, phase = case
    want = reference(threshold, phase, connectivity, periodic)
    got = lib.topology(capi.GRID_XH, threshold, phase, periodic, connectivity)
    print(f"N {N}, {case}, {connectivity} neighbours, periodic {periodic}: {got.tolist()}, reference {want.tolist()}")
    assert got.dtype == np.uint64 and got.shape == (10,)
    assert np.array_equal(got, want)
    again = lib.topology(capi.GRID_XH, threshold, phase, periodic, connectivity)
    assert again.tobytes() == got.tobytes()
    # the case is what it is meant to be: the other boundary gives other counts and other components
    other = reference(threshold, phase, connectivity, not periodic)
    assert want[T["cells"]] == other[T["cells"]] == BR.in_phase(field, threshold, phase).sum()
    assert all(want[n] != other[n] for n in (T["closed_faces"], T["closed_edges"], T["closed_vertices"], T["open_faces"])), (want.tolist(), other.tolist())
    assert (want[T["components"]], want[T["complement_components"]]) != (other[T["components"]], other[T["complement_components"]])


def _run_mask(asora, mask, connectivity, periodic, want=None):
    """The library on a boolean mask (uploaded as 0 / 1 into GRID_XH_AV, threshold 0.5) next to the reference."""
    p, lib, capi = asora
    lib.grid_to_device(capi.GRID_XH_AV, mask.astype(np.float64))
    got = lib.topology(capi.GRID_XH_AV, 0.5, 0, periodic, connectivity)
    want = TR.tallies(mask, connectivity, periodic) if want is None else want
    assert got.dtype == np.uint64 and np.array_equal(got, want), (connectivity, periodic, got.tolist(), want.tolist())
    assert lib.topology(capi.GRID_XH_AV, 0.5, 0, periodic, connectivity).tobytes() == got.tobytes()
    return got


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "open"])
def test_word_boundary_wrap_carry_and_bit_N_together(asora, periodic):
    """N = 128: two full words per row, all in phase but the plane k = 127 -- the last bit of the last word.  The carry into word 1
    comes out of bit 63 of word 0, the carry into word 0 through the wrap is a 0 next to 127 ones, and in the open box bit N = 128
    lies in a third word that the mask does not have.  The phase is one slab, the complement one plane that lies on the faces."""
    N = 128
    _mesh(asora, N)
    mask = np.ones((N, N, N), dtype=bool)
    mask[:, :, N - 1] = False
    want = np.zeros(10, dtype=np.uint64)
    want[:7] = TR.elements(mask, periodic)
    want[T["components"]], want[T["complement_components"]], want[T["cavities"]] = 1, 1, 0
    # the element counts by hand: a slab of N x N x (N - 1) cells
    M = N - 1
    if periodic:
        by_hand = [N * N * M, N * N * (M + 1) + 2 * N * N * M, 2 * N * N * (M + 1) + N * N * M, N * N * (M + 1),
                   N * N * (M - 1) + 2 * N * N * M, 2 * N * N * (M - 1) + N * N * M, N * N * (M - 1)]
    else:
        by_hand = [N * N * M, N * N * (M + 1) + 2 * N * (N + 1) * M, 2 * N * (N + 1) * (M + 1) + (N + 1) ** 2 * M, (N + 1) ** 2 * (M + 1),
                   N * N * (M - 1) + 2 * N * (N - 1) * M, 2 * N * (N - 1) * (M - 1) + (N - 1) ** 2 * M, (N - 1) ** 2 * (M - 1)]
    assert want[:7].tolist() == by_hand
    for connectivity in (6, 26):
        _run_mask(asora, mask, connectivity, periodic, want)
    # ... and the plane at the other end of the row, and the row's two ends both out of phase
    for planes in ((0,), (0, N - 1), (63,), (64,)):
        other = np.ones((N, N, N), dtype=bool)
        other[:, :, list(planes)] = False
        want = np.zeros(10, dtype=np.uint64)
        want[:7] = TR.elements(other, periodic)
        joined = periodic or planes in ((0,), (0, N - 1))             # one slab, or two that only the wrap joins
        want[T["components"]] = 1 if joined else 2
        want[T["complement_components"]] = 1 if (len(planes) == 1 or periodic) else 2
        _run_mask(asora, other, 6, periodic, want)


def test_hand_shapes(asora):
    N = 9
    _mesh(asora, N)
    for name, make in TR.HAND_SHAPES.items():
        mask = make(N)
        for connectivity in (6, 26):
            for periodic in (True, False):
                got = _run_mask(asora, mask, connectivity, periodic)
                if not periodic and name != "corner_pair":
                    chi, betti = {"hollow_cube": (2, (1, 0, 1)), "ring": (0, (1, 1, 0)), "one_cell": (1, (1, 0, 0))}[name]
                    assert TR.euler(got, 6) == TR.euler(got, 26) == chi and TR.betti(got, connectivity) == betti, name
                if name == "corner_pair":
                    assert TR.euler(got, 6) == 2 and TR.euler(got, 26) == 1 and got[T["components"]] == (2 if connectivity == 6 else 1)
    got = _run_mask(asora, TR.hollow_cube(N), 6, False)
    assert got.tolist() == [124, 450, 540, 216, 294, 228, 56, 1, 2, 1]


@pytest.mark.parametrize("N", [N for N in TR.FULL_BOXES if N >= 2])
def test_full_and_empty_box(asora, N):
    """N = 2, 3, 5 (device_init takes no mesh of one cell: N = 1 is pinned on the reference alone, tests/test_topology_reference.py).
    At N = 2 the periodic lattice meets every cell twice, and the counts follow the formula through the wrap."""
    _mesh(asora, N)
    full = np.ones((N, N, N), dtype=bool)
    for connectivity in (6, 26):
        got = _run_mask(asora, full, connectivity, True)
        assert got.tolist() == [N ** 3, 3 * N ** 3, 3 * N ** 3, N ** 3, 3 * N ** 3, 3 * N ** 3, N ** 3, 1, 0, 0]
        got = _run_mask(asora, full, connectivity, False)
        assert got[T["closed_vertices"]] == (N + 1) ** 3 and TR.euler(got, 6) == TR.euler(got, 26) == 1
        assert got[7:].tolist() == [1, 0, 0]
        for periodic in (True, False):
            got = _run_mask(asora, ~full, connectivity, periodic)
            assert got.tolist() == [0] * 8 + [1, 0]
    if N > 1:                                                           # one cell missing in a corner: no cavity, it lies on the faces
        holed = full.copy()
        holed[0, 0, 0] = False
        for connectivity in (6, 26):
            for periodic in (True, False):
                _run_mask(asora, holed, connectivity, periodic)


def test_a_nan_cell_is_in_the_complement_of_both_phases(asora):
    p, lib, capi = asora
    N, seed = GPU_FIELDS[0]
    assert N == 17
    _mesh(asora, N)
    field = BR.blob_field(N, seed)
    field[8, 8, 8] = np.nan
    lib.grid_to_device(capi.GRID_XH_AV, field)
    cells = 0
    with np.errstate(invalid="ignore"):
        for phase in (0, 1):
            mask = BR.in_phase(field, 0.5, phase)
            assert not mask[8, 8, 8]
            for connectivity in (6, 26):
                for periodic in (True, False):
                    got = lib.topology(capi.GRID_XH_AV, 0.5, phase, periodic, connectivity)
                    assert np.array_equal(got, TR.tallies(mask, connectivity, periodic)), (phase, connectivity, periodic)
            cells += int(got[T["cells"]])
    assert cells == N ** 3 - 1


def test_components_are_the_regions_and_the_region_call_is_undisturbed(asora, box):
    """COMPONENTS is n_regions of asora_region_sizes with the same arguments; a region_sizes call behind a topology call -- which
    has left the complement's labels and marked volumes in the buffers the two share -- returns its reference, labels included;
    no grid changes."""
    p, lib, capi = asora
    N, field, reference = box
    edges = RR.default_edges(N)
    n_regions = list(RR.TALLIES).index("n_regions")
    before = lib.grid_sum(capi.GRID_XH)
    for threshold, phase in BLOB_CASES:
        for connectivity in (6, 26):
            for periodic in (True, False):
                t = lib.topology(capi.GRID_XH, threshold, phase, periodic, connectivity)
                r = lib.region_sizes(capi.GRID_XH, threshold, phase, periodic, connectivity, edges)
                assert t[T["components"]] == r[2][n_regions] and t[T["cells"]] == r[2][0], (threshold, phase, connectivity, periodic)
    lib.topology(capi.GRID_XH, 0.5, 0, False, 26)
    want = RR.sizes(BR.in_phase(field, 0.69, 0), 6, True, edges)
    got = lib.region_sizes(capi.GRID_XH, 0.69, 0, True, 6, edges, labels=True)
    assert np.array_equal(got[3], want[0])
    for g, w in zip(got[:3], want[1:]):
        assert np.array_equal(g, w)
    assert lib.grid_sum(capi.GRID_XH) == before
    assert np.array_equal(lib.grid_to_host(capi.GRID_XH, np.empty((N, N, N))), field)


def test_module_entry(asora, box):
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    N, field, reference = box
    t = pc2r.topology(field, threshold=0.69, periodic=False, dr=2.0)
    want = reference(0.69, 0, 6, False)
    assert isinstance(t, pc2r.Topology) and np.array_equal(t.tallies, want)
    assert t.euler == t.euler_6 == TR.euler(want, 6) and t.euler_26 == TR.euler(want, 26) and t.betti == TR.betti(want, 6)
    assert t.betti[1] >= 0 and t.volume_phys == 8.0 * t.cells and t.surface_phys == 4.0 * t.surface
    same = pc2r.topology(None, threshold=0.69, periodic=False)         # the grid where it lies
    assert np.array_equal(same.tallies, t.tallies) and same.dr is None
    neutral = pc2r.topology(None, grid=capi.GRID_XH, phase="neutral", threshold=0.69, connectivity=26)
    assert np.array_equal(neutral.tallies, reference(0.69, 1, 26, True)) and neutral.betti is None
    assert neutral.cells == N ** 3 - t.cells
    # the periodic identity, from the device: chi of the phase = chi of the complement under the dual connectivity
    ionised = pc2r.topology(None, threshold=0.69, connectivity=6)
    assert ionised.euler == neutral.euler and ionised.complement_components == neutral.components


def test_refusals(asora, box):
    p, lib, capi = asora
    ok = dict(which=capi.GRID_XH, threshold=0.5, phase=0, periodic=True, connectivity=6)
    for change, what in ((dict(which=capi.GRID_CLUMP), "holds no data"), (dict(which=99), "bad grid selector"),
                         (dict(threshold=np.nan), "threshold must be finite"), (dict(threshold=np.inf), "threshold must be finite"),
                         (dict(phase=2), "phase must be"), (dict(connectivity=18), "connectivity must be 6"),
                         (dict(connectivity=0), "connectivity must be 6")):
        with pytest.raises(RuntimeError, match=f"topology: .*{what}"):
            lib.topology(**{**ok, **change})
    raw = lib._lib.asora_topology
    assert raw(capi.GRID_XH, 0.5, 0, 1, 6, None) == 3 and b"null" in lib._lib.asora_last_error()
    out = np.full(10, 9, dtype=np.uint64)
    assert raw(capi.GRID_XH, 0.5, 0, 1, 7, out.ctypes.data_as(capi._u64p)) == 3 and np.all(out == 9)     # (a refused call writes nothing)
    assert raw(capi.GRID_CLUMP, 0.5, 0, 1, 6, out.ctypes.data_as(capi._u64p)) == 4 and np.all(out == 9)
    assert lib.topology(**ok)[T["cells"]] > 0                           # (and the call still works afterwards)


def test_class(asora, tmp_path):
    """The single black-body run at its test mesh with the topology keys: every step on the resident path leaves its topology and one
    line in the log; topology() reads the ionised fraction where it lies and equals the module-level call on a downloaded copy."""
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
                results.append(sim.last_topology)
            return sim, results

        off, off_results = run(PLAIN_PARAMS, True)
        assert off.device_resident and off.topology_stats is False and off_results == [None, None]
        for periodic in (True, False):
            t = off.topology(connectivity=26, periodic=periodic)
            assert off._device_newer >= {"xh", "phi_ion"}       # nothing was fetched
            assert (t.periodic, t.dr, t.connectivity, t.threshold, t.N) == (periodic, off.dr, 26, 0.5, N) and 0 < t.cells < N ** 3
            if not periodic:
                resident_open = t
        x_off = off.xh.copy()                                   # (downloads)
        m = pc2r.topology(x_off.copy(), connectivity=26, periodic=False, dr=off.dr)
        assert np.array_equal(m.tallies, resident_open.tallies) and m.betti == resident_open.betti and m.betti[0] == 1
        assert np.array_equal(m.tallies, TR.tallies(x_off >= 0.5, 26, False))
        again = off.topology(connectivity=26, periodic=False)   # the host copy is the newer one now: the upload form
        assert np.array_equal(again.tallies, m.tallies)

        on, on_results = run(TOPOLOGY_PARAMS, True)
        assert on.device_resident and on.topology_stats is True
        assert all(res is not None for res in on_results) and on_results[0] is not on_results[1]
        last = on_results[1]
        assert (last.threshold, last.connectivity, last.dr, last.periodic) == (0.4, 26, on.dr, True)
        assert open(on.logfile).read().count("Topology (ionised, x >= 0.4, 26 neighbours, periodic): Euler characteristic ") == 2
        x_on = on.xh.copy()
        assert np.array_equal(x_on, x_off)                      # the analysis changes nothing of the step
        assert np.array_equal(last.tallies, TR.tallies(x_on >= 0.4, 26, True))
        assert last.components == 1 and last.cells > on_results[0].cells      # one bubble around the source, and it grows
    finally:
        if p.cuda_is_init():
            p.device_close()
        os.chdir(cwd)
