"""GPU: the Lyman-alpha forest (asora_lyman_alpha_forest, lyman_alpha_forest, C2Ray.lyman_alpha_forest) against
its numpy/scipy statement, tests/lyman_alpha_reference.py.  Every call is made twice and compared byte for byte.

The optical depth carries the bound of the reference, (2 W + 16) eps S[p] (derived there: the device's erf and exp are the device
library's, scipy's are the reference's); what is made of integers -- the window, clipped, degenerate, the PDF, the gaps -- is
compared exactly, the PDF and the gaps with numpy on the device's own downloaded F; sum F and sum F^2 within (N^3 + 4) eps relative,
the worst case of any summation order of non-negative terms plus exp.

A second pass (tests/untested_trips.py; DESIGN.md 4.2k, "Which trips the second pass reaches") runs fields with a known answer made
from crafted dark masks at N = 64, 128, 129, 192 and 320, the strict < of the threshold at equality, the PDF's limits, and a
non-finite reach."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import lyman_alpha_reference as R
import untested_trips as UT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LYA_PARAMS = os.path.join(HERE, "data", "parameters_lyman_alpha.yml")
VSCALE, B_SCALE, TAU_SCALE = 0.5, 0.5 / math.sqrt(3.0e4), 1.0     # u in multiples of 1/8 up to 3 cells; bt from 2^-10 to 0.5 cells
EDGES = np.linspace(0.0, 1.0, 11)
EDGES[-1] = np.nextafter(1.0, 2.0)
# 24, 33 and 70 on all three axes: 70 is above one wave and a multiple of nothing; a tile of 16 columns of 70 cells (1120) holds more
# cells than its workgroup has work items (1024), and so does every tile of rows (60, 45 and 21 rows against 256 work items)
CASES = [(N, axis) for N in (24, 33, 70) for axis in (0, 1, 2)]
N_TILES_OF_8 = 320        # from N = 308 to N = 611 a tile of columns has 8 lines; a line of 320 is also longer than a workgroup of axis 2
KEYS = ("stats", "counts", "gaps", "pdf", "tau", "flux")


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib, _capi
    if p.cuda_is_init():
        p.device_close()


@functools.lru_cache(maxsize=None)
def _fields(N):
    return R.fields(N, 100 + N)


@functools.lru_cache(maxsize=None)
def _reference(N, axis, window=0):
    x, n, T, v = _fields(N)
    return R.forest(x, n, T, v, axis, VSCALE, B_SCALE, TAU_SCALE, window=window, edges=EDGES)


def _mesh(asora, N, fields=None):
    p, lib, capi = asora
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)
    if fields is not None:
        x, n, T, v = fields
        for which, grid in ((capi.GRID_XH, x), (capi.GRID_NDENS, n), (capi.GRID_TEMP, T)):
            lib.grid_to_device(which, grid)
        lib.los_velocity_to_device(v)


def _twice(lib, *args, **kw):
    got, again = lib.lyman_alpha_forest(*args, **kw), lib.lyman_alpha_forest(*args, **kw)
    for key in KEYS:
        assert (got[key] is None) == (again[key] is None), key
        if got[key] is not None:
            assert got[key].tobytes() == again[key].tobytes(), key
    assert got["counts"].dtype == np.uint64 and got["gaps"].dtype == np.uint64
    return got


def _within_bound(tau, ref, what):
    err, bound = np.abs(tau - ref["tau"]), ref["bound"]
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
    print(f"{what}: worst |tau - reference| = {worst:.4f} of the bound (W = {ref['window']})")
    assert np.all(err <= bound), (what, worst)


@pytest.mark.parametrize("N,axis", CASES)
def test_optical_depth_and_windows(asora, N, axis):
    """The device's tau against the reference within its bound, with the automatic window, with a window smaller than the reach
    (clipped says so) and with one larger (the same bits as the automatic one)."""
    p, lib, capi = asora
    x, n, T, v = _fields(N)
    ref = _reference(N, axis)
    # the fields test something: exact 0 and 1 in x, exact 0 in T, degenerate and inverted cells, tau over four decades, at least three
    # occupied bins of the PDF and gaps of at least three lengths
    u = np.moveaxis(v, axis, -1) * VSCALE
    d = 0.5 * (np.roll(u, 1, axis=-1) + u)
    assert np.any(x == 0.0) and np.any(x == 1.0) and np.any(T == 0.0) and np.any(1.0 + np.roll(d, -1, axis=-1) < d)
    assert ref["degenerate"] >= 1 and np.max(np.abs(u)) <= ref["window"] - 1 and ref["clipped"] == 0
    assert np.sum(ref["tau"] < 1e-2) > 0 and np.sum(ref["tau"] > 1e2) > 0
    assert np.count_nonzero(ref["pdf"]) >= 3 and np.count_nonzero(ref["gaps"]) >= 3
    _mesh(asora, N, (x, n, T, v))
    auto = _twice(lib, axis, VSCALE, B_SCALE, TAU_SCALE, edges=EDGES, tau=True, flux=True)
    counts = auto["counts"]
    assert int(counts[capi.LYA_WINDOW]) == ref["window"] and int(counts[capi.LYA_CLIPPED]) == 0
    assert int(counts[capi.LYA_DEGENERATE]) == ref["degenerate"] and int(counts[capi.LYA_NONFINITE]) == 0
    _within_bound(auto["tau"], ref, f"N = {N}, axis {axis}, automatic")
    assert np.all(np.abs(auto["flux"] - np.exp(-auto["tau"])) <= 4.0 * R.EPS * auto["flux"])
    # larger than the reach: terms beyond the cut are left out, the bits are the same
    wide = _twice(lib, axis, VSCALE, B_SCALE, TAU_SCALE, window=(N - 1) // 2, edges=EDGES, tau=True, flux=True)
    assert int(wide["counts"][capi.LYA_WINDOW]) == (N - 1) // 2 > ref["window"] and int(wide["counts"][capi.LYA_CLIPPED]) == 0
    for key in ("stats", "gaps", "pdf", "tau", "flux"):
        assert wide[key].tobytes() == auto[key].tobytes(), key
    # smaller: clipped counts the cells cut off, and tau is the reference's with that W
    small = _reference(N, axis, 2)
    assert small["clipped"] > 0
    got = _twice(lib, axis, VSCALE, B_SCALE, TAU_SCALE, window=2, edges=EDGES, tau=True)
    assert int(got["counts"][capi.LYA_WINDOW]) == 2 and int(got["counts"][capi.LYA_CLIPPED]) == small["clipped"]
    _within_bound(got["tau"], small, f"N = {N}, axis {axis}, W = 2")
    # at rest: use_velocity = 0 is u = 0
    rest = R.forest(x, n, T, None, axis, VSCALE, B_SCALE, TAU_SCALE)
    got = _twice(lib, axis, None, B_SCALE, TAU_SCALE, tau=True)
    assert int(got["counts"][capi.LYA_WINDOW]) == rest["window"] and int(got["counts"][capi.LYA_DEGENERATE]) == 0 and got["pdf"] is None
    _within_bound(got["tau"], rest, f"N = {N}, axis {axis}, at rest")


@pytest.mark.parametrize("N", [24, 33, 70])
def test_axis_a_equals_axis_2_on_transposed_inputs(asora, N):
    p, lib, capi = asora
    fields = _fields(N)
    _mesh(asora, N, fields)
    along = {axis: _twice(lib, axis, VSCALE, B_SCALE, TAU_SCALE, edges=EDGES, tau=True, flux=True) for axis in (0, 1)}
    for axis in (0, 1):
        _mesh(asora, N, tuple(np.ascontiguousarray(np.moveaxis(a, axis, -1)) for a in fields))
        moved = _twice(lib, 2, VSCALE, B_SCALE, TAU_SCALE, edges=EDGES, tau=True, flux=True)
        for key in ("tau", "flux"):
            assert np.ascontiguousarray(np.moveaxis(moved[key], -1, axis)).tobytes() == along[axis][key].tobytes(), (axis, key)
        for key in ("counts", "gaps", "pdf"):
            assert moved[key].tobytes() == along[axis][key].tobytes(), (axis, key)


@pytest.mark.parametrize("N,axis", [(24, 0), (33, 1), (33, 2), (70, 0), (70, 2)])
def test_statistics_against_numpy_on_the_devices_own_fields(asora, N, axis):
    p, lib, capi = asora
    x, n, T, v = _fields(N)
    n, T = n.copy(), T.copy()
    n[1, 2, 3], T[1, 2, 3] = np.nan, 3.0e4                         # a non-finite tau on the lines through it (a cell cold and narrow enough
                                                                   # to lie between two pixel centres would add to no pixel at all)
    _mesh(asora, N, (x, n, T, v))
    cells = float(N) ** 3
    for threshold in (0.05, 2.0, -1.0):                            # the forest; every line wholly dark; no dark pixel
        got = _twice(lib, axis, VSCALE, B_SCALE, TAU_SCALE, gap_threshold=threshold, edges=EDGES, tau=True, flux=True)
        tau, flux, stats, counts = got["tau"], got["flux"], got["stats"], got["counts"]
        finite = np.isfinite(flux)
        assert int(counts[capi.LYA_NONFINITE]) == int(np.sum(~np.isfinite(tau))) > 0
        assert stats[capi.LYA_TAU_MIN] == np.nanmin(tau) and stats[capi.LYA_TAU_MAX] == np.nanmax(tau)
        assert np.isnan(stats[capi.LYA_SUM_F]) and np.isnan(stats[capi.LYA_SUM_F2])       # (a NaN among the terms)
        assert got["pdf"].tobytes() == R.pdf_of(flux, EDGES).tobytes() and int(got["pdf"].sum()) == int(np.sum(finite))
        want = R.gap_statistics(np.moveaxis(flux, axis, -1), threshold)
        assert got["gaps"].tobytes() == want["gaps"].tobytes() and got["gaps"][0] == 0
        assert (int(counts[capi.LYA_N_DARK]), int(counts[capi.LYA_N_GAPS]), int(counts[capi.LYA_LONGEST]), int(counts[capi.LYA_FULL_LINES])) == \
               (want["n_dark"], want["n_gaps"], want["longest"], want["full_lines"]), threshold
        if threshold == 2.0:                                       # (NaN < 2 is false: the lines through the NaN are not wholly dark)
            assert 0 < want["full_lines"] < N * N and want["gaps"][N] == want["full_lines"]
        if threshold == -1.0:
            assert want["n_gaps"] == 0
    # the sums, on fields without the NaN
    x, n, T, v = _fields(N)
    lib.grid_to_device(capi.GRID_NDENS, n)
    lib.grid_to_device(capi.GRID_TEMP, T)
    got = _twice(lib, axis, VSCALE, B_SCALE, TAU_SCALE, gap_threshold=2.0, edges=EDGES, tau=True, flux=True)
    flux = got["flux"]
    for key, exact in ((capi.LYA_SUM_F, math.fsum(flux.ravel())), (capi.LYA_SUM_F2, math.fsum((flux * flux).ravel()))):
        rel = abs(got["stats"][key] - exact) / exact
        print(f"N = {N}, axis {axis}: sum {key} off by {rel / R.EPS:.3f} eps relative")
        assert rel <= (cells + 4.0) * R.EPS
    assert int(got["counts"][capi.LYA_NONFINITE]) == 0 and int(got["counts"][capi.LYA_FULL_LINES]) == N * N == int(got["gaps"][N])
    assert int(got["counts"][capi.LYA_N_DARK]) == N ** 3 and int(got["counts"][capi.LYA_LONGEST]) == N


def test_tiles_of_8_columns(asora):
    """From N = 308 on a tile of the axes 0 and 1 has 8 columns, not 16 (the library says which it takes), and on axis 2 a line is
    longer than its workgroup of 256: some lines of such a mesh against the reference on every axis, with a small window
    (the reference takes 2 W + 1 passes of two erf over its cells)."""
    p, lib, capi = asora
    N = N_TILES_OF_8
    rng = np.random.default_rng(77)
    shape = (N, N, N)
    x = np.where(rng.random(shape) < 0.3, 1.0 - 10.0 ** rng.uniform(-2.0, 0.0, shape), 1.0)
    n = 3.0 * np.exp(rng.standard_normal(shape))
    T = 10.0 ** rng.uniform(0.0, 4.0, shape)
    v = np.round(rng.uniform(-2.0, 2.0, shape) * 4.0) / 4.0
    _mesh(asora, N, (x, n, T, v))
    rows = N * N
    lines = np.unique(np.r_[np.arange(24), np.arange(rows - 24, rows), rng.integers(0, rows, size=200)])
    assert [lib.lyman_alpha_forest_tiles(N, axis)["lines"] for axis in (0, 1, 2)] == [8, 8, 4]
    assert [lib.lyman_alpha_forest_tiles(70, axis)["lines"] for axis in (0, 1, 2)] == [16, 16, 21]      # (the meshes of CASES: 16 columns)
    for axis in (0, 1, 2):
        got = lib.lyman_alpha_forest(axis, VSCALE, B_SCALE, TAU_SCALE, window=1, tau=True)
        ref = R.forest(x, n, T, v, axis, VSCALE, B_SCALE, TAU_SCALE, window=1, lines=lines)
        tau = R.pick_lines(got["tau"], axis, lines)
        assert int(got["counts"][capi.LYA_WINDOW]) == 1 and int(got["counts"][capi.LYA_CLIPPED]) > 0
        _within_bound(tau, ref, f"N = {N}, axis {axis}, {lines.size} lines")
        assert np.count_nonzero(ref["tau"]) > 0.2 * ref["tau"].size


# ---- the second pass: the word arithmetic of the gap walk, the PDF's limits, whole meshes of other tile forms (tests/untested_trips.py)
MASK_B_SCALE, MASK_TAU_SCALE, MASK_THRESHOLD = 0.37, 5.0, 0.5      # (b_scale is arbitrary: T = 0, every bt is the floor)
GAP_COUNTS = ("n_dark", "n_gaps", "longest", "full_lines")


def _mask_mesh(asora, N, axis):
    """The crafted field of R.mask_field on the device, its crafted lines where the library's tiles of (N, axis) differ: (x, n, T,
    dark, the placement).  Asserts, from the tiles the library reports, that the placement reaches what it is there for."""
    p, lib, capi = asora
    tiles = lib.lyman_alpha_forest_tiles(N, axis)
    place = UT.lya_placement(N, axis, tiles["lines"], len(R.crafted_lines(N)))
    starts, at = place["starts"], set(place["lines_at"])
    assert len(starts) == tiles["workgroups"] and starts[0] == 0
    assert {0, N * N - 1} <= at and set(range(starts[-1], N * N)) <= at               # the first tile's first line; the whole last tile
    assert len(place["boundaries"]) >= 3 and all(b in starts and b - 1 in at and b in at for b in place["boundaries"])
    ragged = N % tiles["lines"] if axis == 1 else N * N % tiles["lines"]
    assert place["last_width"] == (ragged or tiles["lines"])
    x, n, T, dark = R.mask_field(N, axis, place["lines_at"])
    _mesh(asora, N)
    for which, grid in ((capi.GRID_XH, x), (capi.GRID_NDENS, n), (capi.GRID_TEMP, T)):
        lib.grid_to_device(which, grid)
    return x, n, T, dark, place


def _gaps_are(got, capi, want, what):
    counts = got["counts"]
    assert got["gaps"].tobytes() == want["gaps"].tobytes(), what
    assert (int(counts[capi.LYA_N_DARK]), int(counts[capi.LYA_N_GAPS]), int(counts[capi.LYA_LONGEST]), int(counts[capi.LYA_FULL_LINES])) == \
           tuple(want[k] for k in GAP_COUNTS), what


def _known_answer(asora, got, N, axis, dark, what):
    """What every crafted field gives: W = 1, nothing clipped, degenerate or non-finite; tau exactly 0 and F exactly 1 on the bright
    pixels; F below the threshold on the dark ones.  Prints whether tau == g holds bit for bit (the device's erf(+-512) decides)."""
    p, lib, capi = asora
    counts = got["counts"]
    assert int(counts[capi.LYA_WINDOW]) == 1 and int(counts[capi.LYA_CLIPPED]) == 0 and int(counts[capi.LYA_DEGENERATE]) == 0
    assert int(counts[capi.LYA_NONFINITE]) == 0
    cube = np.moveaxis(dark.reshape(N, N, N), -1, axis)
    assert np.all(got["tau"][~cube] == 0.0) and np.all(got["flux"][~cube] == 1.0)
    assert np.array_equal(got["flux"] < MASK_THRESHOLD, cube)
    exact = bool(np.all(got["tau"][cube] == MASK_TAU_SCALE))
    print(f"{what}: tau == g bit for bit on the device: {exact}")
    return cube


@pytest.mark.parametrize("N,axis", [(N, axis) for N in UT.LYA_MESHES for axis in (0, 1, 2)])
def test_crafted_masks_across_words_and_tiles(asora, N, axis):
    """Lines of one, two, two and a bit, and three mask words with runs made for the gap walk (R.crafted_lines) in the first tile, the
    last and either side of tile boundaries: tau against the statement, the gaps against the statement's on the DESIGNED mask and
    against numpy on the device's own F."""
    p, lib, capi = asora
    x, n, T, dark, place = _mask_mesh(asora, N, axis)
    assert UT.mask_words(N) == {64: 1, 128: 2, 129: 3, 192: 3}[N] and (UT.pad_bits(N) == 0) == (N % 64 == 0)
    ref = R.forest(x, n, T, None, axis, 0.0, MASK_B_SCALE, MASK_TAU_SCALE, gap_threshold=MASK_THRESHOLD)
    assert (ref["window"], ref["clipped"], ref["degenerate"]) == (1, 0, 0)
    assert np.array_equal(np.moveaxis(ref["flux"], axis, -1).reshape(-1, N) < MASK_THRESHOLD, dark)      # its gaps are the designed mask's
    got = _twice(lib, axis, None, MASK_B_SCALE, MASK_TAU_SCALE, gap_threshold=MASK_THRESHOLD, tau=True, flux=True)
    what = f"crafted masks, N = {N}, axis {axis}"
    _within_bound(got["tau"], ref, what)
    _known_answer(asora, got, N, axis, dark, what)
    _gaps_are(got, capi, ref, what)
    _gaps_are(got, capi, R.gap_statistics_fast(np.moveaxis(got["flux"], axis, -1), MASK_THRESHOLD), what + ", its own F")
    assert ref["full_lines"] >= 2 and ref["longest"] == N and ref["gaps"][N - 1] >= 4 and ref["gaps"][1] > N


def test_threshold_equality_and_pdf_limits(asora):
    """The strict < of the dark mask at equality; the PDF with values ON its edges, with repeated edges and with one bin; and with
    the 1024 bins of the limit on the forest of N = 70."""
    p, lib, capi = asora
    N, axis = 64, 2
    x, n, T, dark, place = _mask_mesh(asora, N, axis)
    call = lambda **kw: _twice(lib, axis, None, MASK_B_SCALE, MASK_TAU_SCALE, tau=True, flux=True, **kw)
    plain = call(gap_threshold=MASK_THRESHOLD)
    cube = _known_answer(asora, plain, N, axis, dark, "N = 64, axis 2")
    values = np.unique(plain["flux"][cube])
    assert values.size == 1 and 0.0 < values[0] < 0.01                 # one F for every dark pixel: exp(-5) as the device has it
    f_dark = float(values[0])
    n_dark, n_bright = int(dark.sum()), int((~dark).sum())
    designed = R.gap_statistics(np.where(dark, 0.0, 1.0), MASK_THRESHOLD)
    _gaps_are(plain, capi, designed, "threshold 0.5")
    at = call(gap_threshold=f_dark)                                    # F < F is false: no dark pixel
    _gaps_are(at, capi, dict(gaps=np.zeros(N + 1, dtype=np.uint64), n_dark=0, n_gaps=0, longest=0, full_lines=0), "threshold == F")
    _gaps_are(call(gap_threshold=float(np.nextafter(f_dark, 1.0))), capi, designed, "threshold the next double above F")
    # a value on an edge belongs to the bin above; between repeated edges lies nothing; F = 1 is outside [..., 1.0]
    for edges, want in (([0.0, f_dark, 1.0, float(np.nextafter(1.0, 2.0))], [0, n_dark, n_bright]), ([f_dark, f_dark, 1.0], [0, n_dark]),
                        ([f_dark, 1.0], [n_dark]), ([1.0, 2.0], [n_bright]), ([0.0, f_dark], [0])):
        got = call(gap_threshold=MASK_THRESHOLD, edges=edges)
        assert got["pdf"].tolist() == want == R.pdf_of(got["flux"], edges).tolist(), edges
        assert got["tau"].tobytes() == plain["tau"].tobytes()
    # the most bins the entry takes, on a forest whose F fills them
    N = 70
    _mesh(asora, N, _fields(N))
    edges = np.linspace(0.0, 1.0, capi.LYA_MAX_BINS + 1)
    assert edges.size - 1 == UT.LYA_MAX_BINS == R.MAX_BINS
    got = _twice(lib, 0, VSCALE, B_SCALE, TAU_SCALE, edges=edges, flux=True)
    flux = got["flux"]
    assert got["pdf"].shape == (1024,) and got["pdf"].tobytes() == R.pdf_of(flux, edges).tobytes()
    inside = np.isfinite(flux) & (flux >= edges[0]) & (flux < edges[-1])
    assert int(got["pdf"].sum()) == int(inside.sum()) < N ** 3 and np.count_nonzero(got["pdf"]) > 1000 and got["pdf"][-1] > 0
    assert any(np.any(flux == e) for e in edges[:-1])                  # (an F on an edge: exact 0 at the least)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_whole_mesh_of_8_column_and_4_row_tiles(asora, axis):
    """The crafted field at N = 320 -- five exact mask words, tiles of 8 columns (axes 0 and 1) and of 4 rows (axis 2) -- with every
    whole-mesh result: the gaps and counts against the vectorised statement on the designed mask, the sums against math.fsum of the
    device's own F; tau against the statement on the crafted lines."""
    p, lib, capi = asora
    N = UT.LYA_MESH_OF_8_COLUMNS
    assert lib.lyman_alpha_forest_tiles(N, axis)["lines"] == (4 if axis == 2 else 8) and UT.mask_words(N) == 5 and UT.pad_bits(N) == 0
    x, n, T, dark, place = _mask_mesh(asora, N, axis)
    got = _twice(lib, axis, None, MASK_B_SCALE, MASK_TAU_SCALE, gap_threshold=MASK_THRESHOLD, tau=True, flux=True)
    what = f"crafted masks, N = {N}, axis {axis}"
    _known_answer(asora, got, N, axis, dark, what)
    lines = np.array(place["lines_at"])
    ref = R.forest(x, n, T, None, axis, 0.0, MASK_B_SCALE, MASK_TAU_SCALE, lines=lines)
    assert (ref["window"], ref["clipped"], ref["degenerate"]) == (1, 0, 0)
    _within_bound(R.pick_lines(got["tau"], axis, lines), ref, what)
    want = R.gap_statistics_fast(np.where(dark, 0.0, 1.0), MASK_THRESHOLD)
    _gaps_are(got, capi, want, what)
    assert want["full_lines"] >= 2 and want["longest"] == N and want["gaps"][111] >= 2 and want["gaps"][N - 1] >= 8
    # math.fsum of the device's own F, which holds two values (_known_answer): the exact sum from their counts, rounded once
    flux = got["flux"].ravel()
    f_dark = float(flux.min())
    assert 0.0 < f_dark < 0.01
    sums = (R.fsum_of_values(flux, [f_dark, 1.0]), R.fsum_of_values(flux * flux, [f_dark * f_dark, 1.0]))
    for key, exact in ((capi.LYA_SUM_F, sums[0]), (capi.LYA_SUM_F2, sums[1])):
        rel = abs(got["stats"][key] - exact) / exact
        print(f"{what}: sum {key} off by {rel / R.EPS:.3f} eps relative")
        assert rel <= (float(N) ** 3 + 4.0) * R.EPS
    assert got["stats"][capi.LYA_TAU_MIN] == 0.0 and got["stats"][capi.LYA_TAU_MAX] == got["tau"].max()


@pytest.mark.parametrize("axis", [0, 2])
def test_a_non_finite_reach_takes_the_whole_line(asora, axis):
    """One cell at T = +inf: the largest reach is infinite, the automatic window falls back to the cap (N - 1) / 2 = 16, the cell
    counts as clipped, and -- its weight being (erf(0) - erf(0)) / 2 = 0 everywhere -- tau stays finite."""
    p, lib, capi = asora
    N = 33
    x, n, T, v = _fields(N)
    T = T.copy()
    T[4, 5, 6] = np.inf
    ref = R.forest(x, n, T, v, axis, VSCALE, B_SCALE, TAU_SCALE, edges=EDGES)
    assert ref["reach_max"] == math.inf and ref["window"] == 16 == (N - 1) // 2 and ref["clipped"] >= 1
    assert _reference(N, axis)["window"] < 16 and _reference(N, axis)["clipped"] == 0      # (without the cell: no fallback)
    _mesh(asora, N, (x, n, T, v))
    got = _twice(lib, axis, VSCALE, B_SCALE, TAU_SCALE, edges=EDGES, tau=True, flux=True)
    counts = got["counts"]
    assert int(counts[capi.LYA_WINDOW]) == 16 and int(counts[capi.LYA_CLIPPED]) == ref["clipped"]
    assert int(counts[capi.LYA_DEGENERATE]) == ref["degenerate"]
    assert int(counts[capi.LYA_NONFINITE]) == int(np.sum(~np.isfinite(got["tau"]))) == ref["nonfinite"] == 0
    finite = np.isfinite(ref["bound"])
    assert np.all(finite)
    _within_bound(got["tau"], ref, f"N = {N}, axis {axis}, one cell at T = inf")
    assert got["pdf"].tobytes() == R.pdf_of(got["flux"], EDGES).tobytes()
    _gaps_are(got, capi, R.gap_statistics(np.moveaxis(got["flux"], axis, -1), 0.05), "T = inf")


def test_into_a_grid(asora):
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    N, axis = 24, 1
    fields = _fields(N)
    _mesh(asora, N, fields)
    plain = _twice(lib, axis, VSCALE, B_SCALE, TAU_SCALE, edges=EDGES, tau=True, flux=True)
    for grid, what, key in ((capi.GRID_XH_AV, capi.LYA_FLUX, "flux"), (capi.GRID_PHI_ION, capi.LYA_TAU, "tau"), (capi.GRID_TEMP_END, capi.LYA_FLUX, "flux")):
        got = _twice(lib, axis, VSCALE, B_SCALE, TAU_SCALE, edges=EDGES, dst_grid=grid, dst_what=what, tau=True, flux=True)
        for k in KEYS:
            assert got[k].tobytes() == plain[k].tobytes(), (grid, k)
        assert lib.grid_to_host(grid, np.empty((N, N, N))).tobytes() == plain[key].tobytes(), grid
    sizes = pc2r.region_sizes(None, grid=capi.GRID_XH_AV, threshold=0.5)
    assert sizes.log_line()
    # into a grid the call reads: every workgroup has read its lines before it writes them
    got = lib.lyman_alpha_forest(axis, VSCALE, B_SCALE, TAU_SCALE, edges=EDGES, dst_grid=capi.GRID_TEMP, dst_what=capi.LYA_TAU, tau=True, flux=True)
    for k in KEYS:
        assert got[k].tobytes() == plain[k].tobytes(), k
    assert lib.grid_to_host(capi.GRID_TEMP, np.empty((N, N, N))).tobytes() == plain["tau"].tobytes()
    # the module's entry: host arrays up, F left in a grid
    res = pc2r.lyman_alpha_forest(fields[0], fields[1], fields[2], velocity=fields[3], velocity_scale=VSCALE, b_scale=B_SCALE, tau_scale=TAU_SCALE,
                                  los_axis=axis, bins=EDGES, into=capi.GRID_XH_AV, return_tau=True)
    assert res.tau.tobytes() == plain["tau"].tobytes() and res.pdf.tobytes() == plain["pdf"].tobytes() and res.flux is None
    assert res.mean_flux == plain["stats"][capi.LYA_SUM_F] / N ** 3 and res.window == int(plain["counts"][capi.LYA_WINDOW])


def _raw(lib, capi, N, los_axis=2, use_velocity=1, velocity_scale=VSCALE, b_scale=B_SCALE, tau_scale=TAU_SCALE, window=0, gap_threshold=0.05,
         n_bins=10, edges=EDGES, dst_grid=-1, dst_what=0, null=()):
    """The C entry with sentinels in every output: (code, are all outputs untouched)"""
    out = dict(stats=np.full(capi.LYA_STATS, 9.0), counts=np.full(capi.LYA_COUNTS, 9, dtype=np.uint64), pdf=np.full(1024, 9, dtype=np.uint64),
               gaps=np.full(N + 1, 9, dtype=np.uint64), tau=np.full((N, N, N), 9.0), flux=np.full((N, N, N), 9.0))
    dp = lambda a: a.ctypes.data_as(capi._dp)
    up = lambda a: a.ctypes.data_as(capi._u64p)
    ptr = {k: (None if k in null else (dp(a) if a.dtype == np.float64 else up(a))) for k, a in out.items()}
    e = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64)
    rc = lib._lib.asora_lyman_alpha_forest(los_axis, use_velocity, velocity_scale, b_scale, tau_scale, window, gap_threshold, n_bins,
                                           None if e is None else dp(e), dst_grid, dst_what, ptr["stats"], ptr["counts"], ptr["pdf"], ptr["gaps"],
                                           ptr["tau"], ptr["flux"])
    return rc, all(np.all(a == 9) for a in out.values())


def test_refusals(asora):
    p, lib, capi = asora
    N = 24
    fields = _fields(N)
    _mesh(asora, N)
    for which, grid in ((capi.GRID_XH, fields[0]), (capi.GRID_NDENS, fields[1])):
        lib.grid_to_device(which, grid)
    lib.los_velocity_to_device(fields[3])
    assert _raw(lib, capi, N) == (4, True) and b"holds no data" in lib._lib.asora_last_error()     # no temperature yet
    assert _raw(lib, capi, N, los_axis=3) == (3, True)              # (3 comes before 4)
    lib.grid_to_device(capi.GRID_TEMP, fields[2])
    marker = np.full((N, N, N), 7.0)
    lib.grid_to_device(capi.GRID_XH_AV, marker)
    nan, inf = math.nan, math.inf
    down = EDGES.copy()
    down[3] = down[2] - 0.01
    holed = EDGES.copy()
    holed[4] = nan
    bad = [dict(los_axis=-1), dict(los_axis=3), dict(b_scale=0.0), dict(b_scale=nan), dict(b_scale=inf), dict(tau_scale=-1.0), dict(tau_scale=nan),
           dict(tau_scale=inf), dict(velocity_scale=nan), dict(velocity_scale=inf), dict(gap_threshold=nan), dict(gap_threshold=inf),
           dict(n_bins=-1), dict(n_bins=1025), dict(edges=down), dict(edges=holed), dict(edges=None), dict(null=("pdf",)), dict(null=("stats",)),
           dict(null=("counts",)), dict(null=("gaps",)), dict(dst_grid=capi.GRID_COUNT), dict(dst_grid=-2), dict(dst_grid=capi.GRID_XH_AV, dst_what=2),
           dict(dst_grid=capi.GRID_XH_AV, dst_what=-1), dict(window=-1), dict(window=12), dict(window=2 ** 30)]
    for kw in bad:
        kw = {"dst_grid": capi.GRID_XH_AV, **kw} if "dst_grid" not in kw else kw
        assert _raw(lib, capi, N, **kw) == (3, True), kw
        assert lib._lib.asora_last_error().startswith(b"lyman_alpha_forest: "), kw
    assert lib.grid_to_host(capi.GRID_XH_AV, np.empty((N, N, N))).tobytes() == marker.tobytes()
    assert _raw(lib, capi, N, window=11, dst_grid=capi.GRID_XH_AV)[0] == 0     # 2 W + 1 = 23 <= 24; and now the grid is written
    assert lib.grid_to_host(capi.GRID_XH_AV, np.empty((N, N, N))).tobytes() != marker.tobytes()
    assert _raw(lib, capi, N, n_bins=0, edges=None, null=("pdf", "tau", "flux"))[0] == 0
    assert _raw(lib, capi, N, use_velocity=0, velocity_scale=nan)[0] == 0      # (not looked at)
    lib.los_velocity_clear()
    assert _raw(lib, capi, N) == (3, True) and b"without a velocity on the device" in lib._lib.asora_last_error()
    assert _raw(lib, capi, N, use_velocity=0)[0] == 0
    with pytest.raises(RuntimeError, match="lyman_alpha_forest failed \\(code 3\\)"):
        lib.lyman_alpha_forest(2, VSCALE, B_SCALE, TAU_SCALE)


def test_stage_times(asora):
    p, lib, capi = asora
    N = 33
    _mesh(asora, N, _fields(N))
    lib.set_option(capi.OPT_TIMING, 1)
    try:
        lib.lyman_alpha_forest(0, VSCALE, B_SCALE, TAU_SCALE, edges=EDGES)
        ms = lib.lyman_alpha_forest_ms()
        assert ms.shape == (capi.LYA_STAGES,) and np.all(ms > 0.0)
        lib.lyman_alpha_forest(0, VSCALE, B_SCALE, TAU_SCALE, window=3)
        ms = lib.lyman_alpha_forest_ms()
        assert np.all(ms[1:] > 0.0) and ms[0] < ms[1]              # (an explicit window: no pass for the reach)
    finally:
        lib.set_option(capi.OPT_TIMING, 0)


def test_class(asora, tmp_path):
    """A run at N = 24 with the Lyman-alpha keys: a step on the resident path leaves its forest and one line in the log, and nothing
    is fetched; the result equals a direct call on the same state and the module-level call on the downloaded grids."""
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
        sim = pc2r.C2Ray_Test(LYA_PARAMS, N, True)
        assert sim.device_resident and sim.lyman_alpha_stats is True and sim.last_lyman_alpha is None and sim.los_axis == 2
        sim.density_init(0.0)
        srcpos, srcflux = sim.read_sources("src.txt", 1)
        rng = np.random.default_rng(21)
        v = np.round(rng.uniform(-2.0, 2.0, (N, N, N)) * 8.0) / 8.0 / sim.velocity_scale()      # km/s: up to 2 cells
        sim.los_velocity = v
        sim.los_axis = 1
        sim.evolve3D(dt, srcflux, srcpos)
        first = sim.last_lyman_alpha
        assert first is not None and first.velocity and (first.los_axis, first.N, first.gap_threshold) == (1, N, 0.1) and first.pdf.size == 8
        assert sim._device_newer >= {"xh", "phi_ion"}             # nothing was fetched
        log = open(sim.logfile).read()
        assert log.count("Lyman-alpha forest (line of sight 1, with peculiar velocities, W = ") == 1 and first.log_line() in log
        assert first.nonfinite == 0 and 0.0 <= first.mean_flux <= 1.0 and first.n_gaps >= 1
        again = sim.lyman_alpha_forest(return_tau=True)
        assert sim._device_newer >= {"xh", "phi_ion"}
        for key in ("stats", "counts", "gap_counts", "pdf"):
            assert getattr(again, key).tobytes() == getattr(first, key).tobytes(), key
        x, n, T = sim.xh.copy(), np.array(sim.ndens, dtype=np.float64), np.array(sim.temp, dtype=np.float64)
        m = pc2r.lyman_alpha_forest(x, n, T, velocity=v, velocity_scale=sim.velocity_scale(), b_scale=sim.lyman_alpha_b_scale(),
                                    tau_scale=sim.lyman_alpha_tau_scale(), los_axis=1, gap_threshold=0.1, bins=8, return_tau=True)
        for key in ("stats", "counts", "gap_counts", "pdf", "tau"):
            assert getattr(m, key).tobytes() == getattr(again, key).tobytes(), key
        ref = R.forest(x, n, T, v, 1, sim.velocity_scale(), sim.lyman_alpha_b_scale(), sim.lyman_alpha_tau_scale(), gap_threshold=0.1)
        # (a box of 14 kpc: the Doppler width is many cells, the window is capped at (N - 1) / 2 and clipped says so)
        assert ref["window"] == first.window == (N - 1) // 2 and ref["clipped"] == first.clipped == N ** 3
        assert ref["degenerate"] == first.degenerate
        _within_bound(again.tau, ref, "C2Ray_Test, N = 24")
        sim.lyman_alpha_stats = False
        sim.evolve3D(dt, srcflux, srcpos)
        assert sim.last_lyman_alpha is first and open(sim.logfile).read().count("Lyman-alpha forest (") == 1
    finally:
        if p.cuda_is_init():
            p.device_close()
        os.chdir(cwd)
