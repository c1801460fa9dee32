"""GPU: the sources of a halo catalogue (asora_halo_catalogue_to_device, asora_halo_sources_build) against the
numpy statement of tests/halo_sources_reference.py.  Every comparison is exact: the table, the positions, the bits of the fluxes
and the summary.  Every build is made twice and compared byte for byte, and every catalogue goes up a second time permuted."""
import importlib
import os

import numpy as np
import pytest

import halo_sources_reference as R
import untested_trips as UT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CLASS_PARAMS = os.path.join(HERE, "data", "parameters_halo_sources.yml")
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_test.yml")
M_LM, M_HM = 1.0e8, 1.0e9
MODELS = (("none", 0.0), ("full", 0.0), ("partial", 0.25), ("partial", 0.0))


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


def _random_catalogue(N, n, seed):
    """Haloes in the box and a quarter of them around it, masses across both thresholds and below"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, N, size=(n, 3))
    far = rng.random(n) < 0.25
    pos[far] = rng.uniform(-1.5 * N, 2.5 * N, size=(int(far.sum()), 3))
    mass = 10.0 ** rng.uniform(7.5, 11.0, size=n)
    return pos, mass


def _field(N, seed):
    """An ionised fraction with both sides of 0.1 well filled"""
    return np.random.default_rng(seed).random((N, N, N)) ** 3


def _table(asora, N, pos, mass, weight, wrap, e, m_lm=M_LM, m_hm=M_HM, permute=True):
    """Uploads the catalogue and compares table and counts with the statement; then once more permuted: the same bytes."""
    p, lib, capi = asora
    want = R.table(pos, mass, weight, N, m_lm, m_hm, wrap, e)
    counts = lib.halo_catalogue_to_device(pos, mass, weight, m_lm, m_hm, wrap, e)
    got = lib.halo_table_to_host()
    assert counts == want[3], (counts, want[3])
    assert lib.halo_catalogue_state() == (want[3]["n_cells"], e)
    for a, b, name in zip(got, want[:3], ("cell", "q_hm", "q_lm")):
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    if permute and len(mass) > 1:
        order = np.random.default_rng(len(mass)).permutation(len(mass))
        assert lib.halo_catalogue_to_device(pos[order], mass[order], weight[order], m_lm, m_hm, wrap, e) == counts
        for a, b in zip(lib.halo_table_to_host(), got):
            assert a.tobytes() == b.tobytes()
    return want


def _build(asora, table, x, g_hm, g_lm, scale, model, x_suppress, f, grid=None):
    """Builds the list twice from the grid where it lies and compares it with the statement"""
    p, lib, capi = asora
    grid = capi.GRID_XH if grid is None else grid
    want = R.build(*table[:3], x, g_hm, g_lm, scale, model, x_suppress, f)
    got = lib.halo_sources_build(grid, g_hm, g_lm, scale, R.MODELS[model], x_suppress, f)
    again = lib.halo_sources_build(grid, g_hm, g_lm, scale, R.MODELS[model], x_suppress, f)
    assert got["pos"].tobytes() == again["pos"].tobytes() and got["flux"].tobytes() == again["flux"].tobytes()
    assert got["summary"] == again["summary"] == want[2], (got["summary"], want[2])
    assert got["pos"].dtype == np.int32 and np.array_equal(got["pos"], want[0])
    assert got["flux"].tobytes() == want[1].tobytes()
    # the order of the list is the one the source upload sorts into
    if got["flux"].size:
        sorted_pos, sorted_flux, _ = lib.sort_sources(got["pos"].ravel(), got["flux"])
        assert sorted_pos.tobytes() == got["pos"].tobytes() and sorted_flux.tobytes() == got["flux"].tobytes()
    got["statement"] = want
    return got


def _all_models(asora, table, x, scale=1.25e-9):
    out = []
    for model, f in MODELS:
        out.append(_build(asora, table, x, 2.0, 30.0, scale, model, 0.1, f))
    return out


@pytest.mark.parametrize("n", [0, 1, 5000])
def test_mesh_of_8(asora, n):
    """No halo, one, and 5000: every cell occupied, tens of haloes in each"""
    p, lib, capi = asora
    N = 8
    _mesh(asora, N)
    rng = np.random.default_rng(80 + n)
    pos = rng.uniform(0.0, N, size=(n, 3))
    if n >= N ** 3:                                    # (one halo at the centre of every cell, the others wherever they fall)
        pos[:N ** 3] = np.stack(np.unravel_index(np.arange(N ** 3), (N, N, N)), axis=1) + 0.5
    mass = 10.0 ** rng.uniform(8.0, 9.3, size=n)
    e = R.unit_exponent(mass)
    table = _table(asora, N, pos, mass, mass, True, e)
    assert table[3]["n_cells"] == (0, 1, N ** 3)[(0, 1, 5000).index(n)]
    x = _field(N, 81)
    lib.grid_to_device(capi.GRID_XH, x)
    lists = _all_models(asora, table, x)
    if n == 0:
        assert all(got["summary"] == [0, 0, 0, 0, 0] and got["flux"].size == 0 for got in lists)
    if n == 5000:
        assert lists[0]["summary"][0] == N ** 3 and 0 < lists[1]["summary"][0] < N ** 3 and lists[1]["summary"][1] > 0


@pytest.mark.parametrize("wrap", [True, False])
def test_mesh_of_20(asora, wrap):
    """No power of two, rows shorter than a wave; a quarter of the haloes outside the box"""
    p, lib, capi = asora
    N = 20
    _mesh(asora, N)
    pos, mass = _random_catalogue(N, 4000, 200)
    weight = mass * np.random.default_rng(201).uniform(0.5, 2.0, size=mass.size)
    table = _table(asora, N, pos, mass, weight, wrap, R.unit_exponent(weight))
    assert table[3]["below"] > 0 and (table[3]["outside"] > 0) == (not wrap)
    x = _field(N, 202)
    lib.grid_to_device(capi.GRID_XH, x)
    _all_models(asora, table, x)


def test_mesh_of_67_many_haloes(asora):
    """A row longer than a wave, 4489 rows (more than one trip of the scan), 300 000 haloes (more than one grid-stride trip of the
    bin kernel), some 170 000 table rows (several hundred build workgroups)"""
    p, lib, capi = asora
    N = 67
    _mesh(asora, N)
    pos, mass = _random_catalogue(N, 300_000, 670)
    table = _table(asora, N, pos, mass, mass, True, R.unit_exponent(mass))
    assert table[3]["n_cells"] > 100_000
    x = _field(N, 671)
    lib.grid_to_device(capi.GRID_XH, x)
    for model, f in (("full", 0.0), ("partial", 0.25)):
        got = _build(asora, table, x, 2.0, 30.0, 1.25e-9, model, 0.1, f)
    assert 0 < got["summary"][1] < table[3]["n_cells"]


def test_mesh_of_67_clustered(asora):
    """50 000 haloes drawn from a log-normal density, 10 000 of them in one cell: thousands of atomic adds to one address"""
    p, lib, capi = asora
    N = 67
    _mesh(asora, N)
    pos, mass = R.clustered(N, 50_000, 672)
    pos[:10_000] = np.array([33.0, 66.0, 1.0]) + np.random.default_rng(673).random((10_000, 3))
    table = _table(asora, N, pos, mass, mass, True, R.unit_exponent(mass))
    crowded = (33 * N + 66) * N + 1
    at = int(np.searchsorted(table[0], crowded))
    assert table[0][at] == crowded and int(table[1][at]) + int(table[2][at]) > 0
    x = _field(N, 674)
    lib.grid_to_device(capi.GRID_XH, x)
    _build(asora, table, x, 2.0, 30.0, 1.25e-9, "full", 0.1, 0.0)


def test_mesh_of_192_second_tile_of_the_chunk_scan(asora):
    """N = 192 with a halo in every fifth cell and 300 000 more (tests/untested_trips.py): more than 4096 x 256 occupied cells, so the
    scan of the chunk counts carries into a second tile and the emit kernel writes behind offsets taken from it; 36 864 rows of three
    trips of 64 cells, more rows than the row kernel has waves where the device has fewer than 288 compute units."""
    p, lib, capi = asora
    import torch
    N = UT.HS_MESH
    _mesh(asora, N)
    pos, mass = UT.halo_catalogue(N)
    table = _table(asora, N, pos, mass, mass, True, R.unit_exponent(mass))
    n_cells = table[3]["n_cells"]
    assert lib.halo_catalogue_state()[0] == n_cells > UT.HS_CHUNK_SCAN_NEEDS == 4096 * 256      # the library's own count
    chunks = -(-n_cells // UT.HS_THREADS)
    assert UT.HS_SCAN_TILE < chunks < 2 * UT.HS_SCAN_TILE and N * N > 2 * UT.HS_SCAN_TILE       # two tiles of chunks; nine of rows
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if UT.rows_second_trip(N, cus):
        print(f"{cus} compute units: {N * N} rows for {cus * UT.HS_ROW_BLOCKS_PER_CU * UT.HS_WAVES} waves, a wave takes a second row")
    else:
        print(f"{cus} compute units: every wave of the row kernel has one row at the most; a wave's second row is NOT reached here")
    assert N % 64 == 0 and N // 64 == 3
    x = _field(N, 1921)
    lib.grid_to_device(capi.GRID_XH, x)
    edge = UT.HS_SCAN_TILE * UT.HS_THREADS                     # the first table row of chunk 4096
    for model, f in (("none", 0.0), ("full", 0.0), ("partial", 0.25)):
        got = _build(asora, table, x, 2.0, 30.0, 1.25e-9, model, 0.1, f)
        want_pos, want_flux, _ = got["statement"]
        # the last source before chunk 4096 of the table and the first one of it: where the list passes the carry of the scan
        cells = (want_pos[:, 0].astype(np.int64) * N + want_pos[:, 1]) * N + want_pos[:, 2]
        at = int(np.searchsorted(cells, table[0][edge]))
        assert 0 < at < got["summary"][0] == cells.size and cells[at - 1] < table[0][edge] <= cells[at]
        for q in (at - 1, at):
            assert np.array_equal(got["pos"][q], want_pos[q]) and got["flux"][q] == want_flux[q] > 0.0, (model, q)
        if model == "full":
            assert 0 < got["summary"][1] and got["summary"][0] < n_cells


@pytest.mark.parametrize("wrap", [True, False])
def test_positions_and_masses_on_the_edges(asora, wrap):
    """Exact integers, N - 2^-40, -1e-20 (floors to -1, wraps to N - 1), exactly N, -3.5, 2 N + 0.5, infinities, a NaN, 3e9; masses
    exactly m_lm and m_hm, a NaN and one just below m_lm"""
    p, lib, capi = asora
    N = 20
    _mesh(asora, N)
    special = [0.0, 7.0, N - 1.0, N - 2.0 ** -40, -1e-20, float(N), -3.5, 2 * N + 0.5, np.inf, -np.inf, np.nan, 3e9, -3e9, 2.0 ** 31,
               np.nextafter(2.0 ** 31, 0.0), -2.0 ** 31]
    rows = []
    for axis in range(3):
        for v in special:
            row = [3.25, 4.5, 5.75]
            row[axis] = v
            rows.append(row)
    pos = np.array(rows)
    n = pos.shape[0]
    mass = np.full(n, 5e9)
    mass[::5] = 5e8
    table = _table(asora, N, pos, mass, mass, wrap, R.unit_exponent(mass))
    # what the statement says of each special value, counted by hand
    nonfinite = 3 * sum(1 for v in special if not (abs(v) < 2.0 ** 31))
    outside = 0 if wrap else 3 * sum(1 for v in special if abs(v) < 2.0 ** 31 and not 0 <= np.floor(v) < N)
    assert (nonfinite, outside) == (3 * 7, 0 if wrap else 3 * 5)
    assert (table[3]["nonfinite"], table[3]["outside"], table[3]["below"]) == (nonfinite, outside, 0)
    cells = set(int(c) for c in table[0])
    assert ((N - 1) * N + 4) * N + 5 in cells and (3 * N + 4) * N + (N - 1) in cells      # N - 2^-40 on axis 0, on axis 2
    assert ((0 * N + 4) * N + 5 in cells)                                                # exactly 0 (and, wrapped, exactly N)
    # the masses
    pos = np.tile([[2.5, 3.5, 4.5]], (6, 1)) + np.arange(6)[:, None]
    mass = np.array([M_LM, M_HM, np.nan, np.nextafter(M_LM, 0.0), np.nextafter(M_HM, 0.0), np.inf])
    weight = np.array([3.0, 5.0, 7.0, 11.0, 13.0, 17.0])
    cell, q_hm, q_lm, counts = _table(asora, N, pos, mass, weight, wrap, 0)
    assert counts == dict(n_cells=4, outside=0, nonfinite=0, below=2)
    assert [int(v) for v in q_hm] == [0, 5, 0, 17] and [int(v) for v in q_lm] == [3, 0, 13, 0]


def test_sums_are_64_bit_integers(asora):
    """One cell's Q beyond 2^53 and odd (no double holds it), another's 2^32 (its low 32 bits are zero), a unit of the caller's at the
    edge of the overflow refusal"""
    p, lib, capi = asora
    M = importlib.import_module("pyc2ray_amd.halo_sources")
    N = 8
    _mesh(asora, N)
    pos = np.array([[1.5, 1.5, 1.5]] * 3 + [[2.5, 2.5, 2.5]] * 2 + [[3.5, 3.5, 3.5]] * 2)
    weight = np.array([2.0 ** 52 + 1, 2.0 ** 52 + 3, 2.0 ** 52 + 5, 2.0 ** 31, 2.0 ** 31, 2.0 ** 52 + 1, 2.0 ** 52 + 3])
    mass = np.array([5e9, 5e9, 5e9, 5e9, 5e9, 5e8, 5e8])
    cell, q_hm, q_lm, counts = _table(asora, N, pos, mass, weight, True, 0)
    assert [int(v) for v in q_hm] == [3 * 2 ** 52 + 9, 2 ** 32, 0] and [int(v) for v in q_lm] == [0, 0, 2 ** 53 + 4]
    x = np.zeros((N, N, N))
    lib.grid_to_device(capi.GRID_XH, x)
    got = _build(asora, (cell, q_hm, q_lm), x, 1.0, 1.0, 1.0, "none", 0.1, 0.0)
    assert got["summary"] == [3, 0, 3 * 2 ** 52 + 9 + 2 ** 32, 2 ** 53 + 4, 0]
    # the edge of the refusal: sum weight / unit + n / 2 < 2^62 holds for 2^62 - 512 (the last double below 2^62), not for 2^62
    edge = 2.0 ** 62 - 512.0
    one = np.array([[4.5, 4.5, 4.5]])
    cat = M.HaloCatalogue(one, [5e9], [edge], unit=1.0)
    assert cat.unit_exponent == 0 and cat.unit == 1.0
    cell, q_hm, q_lm, counts = _table(asora, N, one, np.array([5e9]), np.array([edge]), True, 0)
    assert [int(v) for v in q_hm] == [2 ** 62 - 512]
    with pytest.raises(ValueError, match="HaloCatalogue: with unit 2\\^0 a cell's integer sum could overflow"):
        M.HaloCatalogue(one, [5e9], [2.0 ** 62], unit=1.0)
    with pytest.raises(RuntimeError, match="halo_catalogue_to_device failed \\(code 3\\).*could overflow"):
        lib.halo_catalogue_to_device(one, [5e9], [2.0 ** 62], M_LM, M_HM, True, 0)
    assert lib.halo_catalogue_state() == (1, 0)          # (a call refused for its arguments leaves the catalogue there as it was)
    # the same weights with the unit of the rule: one step is 2, the sums are exact to (haloes in the cell) units / 2
    _table(asora, N, pos, mass, weight, True, R.unit_exponent(weight))


def test_suppression_on_the_edges(asora):
    """x exactly x_suppress (not suppressed), the next double above it (suppressed) and a NaN (not suppressed) in cells with LM haloes
    only, with HM ones only and with both; the three models; f_suppressed 0 -- rows leave the list -- and 0.25; everything
    suppressed without an HM halo: an empty list; a grid other than the ionised fraction"""
    p, lib, capi = asora
    N = 8
    _mesh(asora, N)
    xs = 0.1
    values = [xs, np.nextafter(xs, 1.0), np.nan, 0.0, 1.0, np.nextafter(xs, 0.0)]
    pos, mass = [], []
    for q, _ in enumerate(values):
        for kind, masses in enumerate(([5e8], [5e9], [5e8, 5e9, 7e8])):
            for m in masses:
                pos.append([q + 0.5, kind + 0.5, 3.5])
                mass.append(m)
    pos, mass = np.array(pos), np.array(mass)
    x = np.full((N, N, N), 0.5)
    for q, v in enumerate(values):
        x[q, :3, 3] = v
    table = _table(asora, N, pos, mass, mass, True, R.unit_exponent(mass))
    assert table[3]["n_cells"] == 18
    lib.grid_to_device(capi.GRID_XH, x)
    none, full, partial, partial0 = _all_models(asora, table, x)
    assert none["summary"][:2] == [18, 0]
    # suppressed: the next double above and 1.0, in the 2 kinds of cells with LM haloes each; with full suppression the 2 cells
    # with LM haloes only leave the list
    assert full["summary"][:2] == [16, 4] and partial["summary"][:2] == [18, 4] and partial0["summary"][:2] == [16, 4]
    assert partial0["flux"].tobytes() == full["flux"].tobytes() and partial["flux"].tobytes() != none["flux"].tobytes()
    # another grid, another threshold: everything suppressed, and without HM haloes nothing is left
    y = np.full((N, N, N), 0.75)
    lib.grid_to_device(capi.GRID_XH_AV, y)
    got = _build(asora, table, y, 2.0, 30.0, 1.25e-9, "full", 0.7, 0.0, grid=capi.GRID_XH_AV)
    assert got["summary"][:2] == [12, 12]
    got = _build(asora, table, y, 0.0, 30.0, 1.25e-9, "full", 0.7, 0.0, grid=capi.GRID_XH_AV)
    assert got["summary"][:2] == [0, 12] and got["pos"].shape == (0, 3) and got["flux"].shape == (0,)
    got = _build(asora, table, y, 0.0, 30.0, 1.25e-9, "full", 0.75, 0.0, grid=capi.GRID_XH_AV)      # x == x_suppress everywhere
    assert got["summary"][:2] == [12, 0]


def test_refusals_stage_times_and_lifetime(asora):
    p, lib, capi = asora
    M = importlib.import_module("pyc2ray_amd.halo_sources")
    N = 20
    if p.cuda_is_init():
        p.device_close()
    base = lib.live_buffers(0)[0]
    pos, mass = _random_catalogue(N, 2000, 900)
    with pytest.raises(RuntimeError, match="halo_catalogue_to_device failed \\(code 2\\)"):
        lib.halo_catalogue_to_device(pos, mass, mass, M_LM, M_HM, True, 0)
    with pytest.raises(RuntimeError, match="halo_sources_build failed \\(code 2\\)"):
        lib.halo_sources_build(capi.GRID_XH, 1.0, 1.0, 1.0, 0, 0.1, 0.0)
    p.device_init(N, 8)
    lib.grid_to_device(capi.GRID_XH, _field(N, 901))
    mesh_only = lib.live_buffers(0)[0]
    with pytest.raises(RuntimeError, match="halo_sources_build failed \\(code 3\\).*no catalogue on the device"):
        lib.halo_sources_build(capi.GRID_XH, 1.0, 1.0, 1.0, 0, 0.1, 0.0)
    with pytest.raises(RuntimeError, match="halo_table_to_host failed \\(code 3\\).*no catalogue on the device"):
        lib.halo_table_to_host()
    import ctypes as C
    counts = (C.c_longlong * 4)()
    raw = lib._lib
    assert raw.asora_halo_catalogue_to_device(None, None, None, -1, M_LM, M_HM, 1, 0, counts) == 3 and b"n must be >= 0" in raw.asora_last_error()
    assert raw.asora_halo_catalogue_to_device(None, None, None, 0, M_LM, M_HM, 1, 2000, counts) == 3
    assert raw.asora_halo_catalogue_to_device(None, None, None, 0, M_HM, M_LM, 1, 0, counts) == 3
    assert raw.asora_halo_catalogue_to_device(None, None, None, 0, M_LM, M_HM, 2, 0, counts) == 3
    with pytest.raises(RuntimeError, match="code 3.*weight\\[1\\] is negative or not finite"):
        lib.halo_catalogue_to_device(pos[:3], mass[:3], [1.0, -1.0, 1.0], M_LM, M_HM, True, 0)
    assert lib.live_buffers(0)[0] == mesh_only               # (a refusal allocates nothing)

    lib.set_option(capi.OPT_TIMING, 1)
    try:
        e = R.unit_exponent(mass)
        lib.halo_catalogue_to_device(pos, mass, mass, M_LM, M_HM, True, e)
        kept = lib.live_buffers(0)[0]
        assert kept == mesh_only + 8                          # the table, five work buffers of a build, the summary and the pinned words
        lib.halo_sources_build(capi.GRID_XH, 2.0, 30.0, 1e-9, capi.HALO_MODEL_FULL, 0.1, 0.0)
        ms = lib.halo_sources_ms()
        assert ms.shape == (capi.HALO_STAGES,) and np.all(ms > 0.0), ms
        assert lib.live_buffers(0)[0] == kept                 # (a build allocates nothing; the transient grids are gone)
    finally:
        lib.set_option(capi.OPT_TIMING, 0)
    for args, what in (((capi.GRID_COUNT, 1.0, 1.0, 1.0, 0, 0.1, 0.0), "bad grid selector"), ((-1, 1.0, 1.0, 1.0, 0, 0.1, 0.0), "bad grid selector"),
                       ((capi.GRID_XH, 1.0, 1.0, 1.0, 3, 0.1, 0.0), "model must be 0"), ((capi.GRID_XH, -1.0, 1.0, 1.0, 0, 0.1, 0.0), "g_hm, g_lm and scale"),
                       ((capi.GRID_XH, 1.0, 1.0, np.inf, 0, 0.1, 0.0), "g_hm, g_lm and scale"), ((capi.GRID_XH, 1.0, 1.0, 1.0, 2, np.nan, 0.0), "x_suppress"),
                       ((capi.GRID_XH, 1.0, 1.0, 1.0, 2, 0.1, 1.5), "f_suppressed must lie in")):
        with pytest.raises(RuntimeError, match="halo_sources_build failed \\(code 3\\).*" + what):
            lib.halo_sources_build(*args)
    with pytest.raises(RuntimeError, match="halo_sources_build failed \\(code 4\\).*holds no data"):
        lib.halo_sources_build(capi.GRID_TEMP_END, 1.0, 1.0, 1.0, 0, 0.1, 0.0)
    # too little room for the list
    pos_out, flux_out = np.zeros((1, 3), dtype=np.int32), np.zeros(1)
    lib.halo_sources_build(capi.GRID_XH, 2.0, 30.0, 1e-9, 0, 0.1, 0.0)
    assert raw.asora_halo_sources_to_host(capi.iptr(pos_out), capi.dptr(flux_out), 1) == 3 and b"room for 1 sources" in raw.asora_last_error()
    # the class of the catalogue: uploaded when first used, again after another object's upload and after a new device_init
    cat = M.HaloCatalogue(pos, mass)
    other = M.HaloCatalogue(pos[:500], mass[:500])
    model = M.SourceModel(2.0, 30.0, 3.0, suppression="full")
    assert cat.n_cells is None and not cat.on_device(lib)
    first = M.halo_sources(cat, model, scale=1e-9)
    assert cat.on_device(lib) and cat.n_cells == lib.halo_catalogue_state()[0] and (cat.outside, cat.nonfinite) == (0, 0) and cat.below > 0
    M.halo_sources(other, model, scale=1e-9)
    assert other.on_device(lib) and not cat.on_device(lib)
    again = M.halo_sources(cat, model, scale=1e-9)
    assert cat.on_device(lib) and again.src_flux.tobytes() == first.src_flux.tobytes() and again.src_pos.tobytes() == first.src_pos.tobytes()
    # a catalogue that went up through the bare entry is another one: the object's table is gone, and it goes up again
    lib.halo_catalogue_to_device(pos[:500], mass[:500], mass[:500], M_LM, M_HM, True, 0)
    assert not cat.on_device(lib) and not other.on_device(lib)
    again = M.halo_sources(cat, model, scale=1e-9)
    assert cat.on_device(lib) and again.src_flux.tobytes() == first.src_flux.tobytes() and again.src_pos.tobytes() == first.src_pos.tobytes()
    want = R.source_list(pos, mass, cat.weights, _field(N, 901), M_LM, M_HM, True, cat.unit_exponent, 2.0, 30.0, cat.unit * 1e-9, "full", 0.1, 0.0)
    assert np.array_equal(first.src_pos, want[0]) and first.src_flux.tobytes() == want[1].tobytes() and first.src_pos.shape[0] == 3
    lib.halo_catalogue_clear()
    assert lib.live_buffers(0)[0] == mesh_only and lib.halo_catalogue_state() is None and not cat.on_device(lib)
    x = _field(N, 902)
    third = M.halo_sources(cat, model, scale=1e-9, xh=x)      # (a host array: uploaded to the ionised-fraction grid)
    assert cat.on_device(lib) and third.n_suppressed > 0 and third.src_flux.tobytes() != first.src_flux.tobytes()
    p.device_close()
    assert lib.live_buffers(0)[0] == base and lib.halo_catalogue_state() is None
    p.device_init(N, 8)
    assert not cat.on_device(lib)
    lib.grid_to_device(capi.GRID_XH, x)
    fourth = M.halo_sources(cat, model, scale=1e-9)
    assert fourth.src_flux.tobytes() == third.src_flux.tobytes() and fourth.log_line() == third.log_line()


def _class_run(pc2r, M, N, mode, catalogue, steps, params=None):
    """Steps of C2Ray_Test with the catalogue and the source model of the parameter file; mode 'resident', 'host' (device_resident =
    False) or 'numpy': the list of every step built by the statement from the downloaded ionised fraction and handed to
    evolve3D(dt, flux, pos)"""
    pos, mass = catalogue
    sim = pc2r.C2Ray_Test(params or CLASS_PARAMS, N, True)
    if params is not None:                             # (a parameter file without the Sources: keys)
        sim.source_model = M.SourceModel(30.0, 130.0, 0.03, suppression="full", x_suppress=0.1)
        sim.halo_mass_thresholds = {"m_lm": M_LM, "m_hm": M_HM}
    sim.device_resident = mode == "resident"
    sim.density_init(sim.zred_0)
    x0 = np.full((N, N, N), 1.2e-3)
    x0[:N // 2] = 0.5                                  # half of the box is ionised already: its LM haloes are off from the first step
    sim.xh = x0
    model = sim.source_model
    assert (model.fgamma_hm, model.fgamma_lm, model.ts_myr, model.suppression, model.x_suppress) == (30.0, 130.0, 0.03, "full", 0.1)
    cat = M.HaloCatalogue(pos, mass, **sim.halo_mass_thresholds)
    scale = M.source_scale(model.ts_myr, float(sim.cosmology.Ob0), float(sim.cosmology.Om0), sim.mean_molecular)
    lists, suppressed = [], []
    if mode != "numpy":
        sim.halo_catalogue = cat
    for dt in steps:
        if mode == "numpy":
            x = np.array(sim.xh, dtype=np.float64)
            src_pos, src_flux = R.source_list(pos, mass, cat.weights, x, cat.m_lm, cat.m_hm, True, cat.unit_exponent, model.fgamma_hm,
                                              model.fgamma_lm, cat.unit * scale, "full", model.x_suppress, 0.0)
            sim.evolve3D(dt, src_flux, src_pos)
        else:
            sim.evolve3D(dt)
            if mode == "resident":
                assert sim._device_newer >= {"xh", "phi_ion"}
            src_pos, src_flux = sim.last_halo_sources.src_pos, sim.last_halo_sources.src_flux
            suppressed.append(sim.last_halo_sources.n_suppressed)
        lists.append((np.array(src_pos), np.array(src_flux)))
    xh = np.array(sim.xh, dtype=np.float64)
    log = open(sim.logfile).read()
    assert log.count("Halo sources (suppression full): ") == (0 if mode == "numpy" else len(steps))
    return xh, lists, suppressed


def test_class_three_steps(asora, tmp_path):
    """C2Ray_Test at N = 16 with a catalogue and full suppression (tests/data/parameters_halo_sources.yml): the resident path, the
    host path and a run fed with the statement's lists give the same lists and the same ionised fraction, bit for bit.  The
    raytrace adds the rates of its sources with floating-point atomics, so two runs agree bit for bit only where no cell is reached
    by two sources (elsewhere to 1e-11, tests/test_c2ray_class.py): the haloes sit in eight cells 8 apart and the photons are
    followed for 2.5 cells."""
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    M = importlib.import_module("pyc2ray_amd.halo_sources")
    N = 16
    rng = np.random.default_rng(1600)
    cells = np.array([[i, j, k] for i in (4, 12) for j in (4, 12) for k in (4, 12)], dtype=np.float64)
    pos = np.repeat(cells, 6, axis=0) + rng.random((48, 3))
    mass = np.tile([2e10, 5e9, 6e8, 3e8, 2e8, 5e7], 8) * rng.uniform(0.8, 1.25, size=48)      # two HM, three LM, one below
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        runs = {}
        for mode in ("resident", "host", "numpy"):
            if p.cuda_is_init():
                p.device_close()
            runs[mode] = _class_run(pc2r, M, N, mode, (pos, mass), (1.0e11, 3.0e11, 1.0e11))
        xh, lists, _ = runs["numpy"]
        assert np.all(np.isfinite(xh)) and np.any(xh[N // 2:] != 1.2e-3)
        for mode in ("resident", "host"):
            assert all(4 <= s <= 8 for s in runs[mode][2]), runs[mode][2]        # the four cells of the ionised half, at the least
            for (pa, fa), (pb, fb) in zip(runs[mode][1], lists):
                assert np.array_equal(pa, pb) and fa.tobytes() == fb.tobytes(), mode
            assert runs[mode][0].tobytes() == xh.tobytes(), mode
        assert all(l[0].shape == (3, 8) for l in lists)
    finally:
        if p.cuda_is_init():
            p.device_close()
        os.chdir(cwd)


def test_class_overlapping_sources(asora, tmp_path):
    """The realistic case the exact test above leaves out: 300 haloes all over the box, photons followed across it
    (tests/data/parameters_test.yml), so that every cell is reached by many sources.  The rates of overlapping sources are added
    with floating-point atomics in no fixed order: the three runs agree to 1e-11, the tolerance of
    test_device_resident_grids_give_the_same_run_with_fewer_transfers for the same reason.  The list of the first step depends on
    the initial state alone and is equal bit for bit; the later ones agree in their cells and, as the fluxes are functions of the
    integer sums and of which side of x_suppress a cell lies on, in their bits too."""
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    M = importlib.import_module("pyc2ray_amd.halo_sources")
    N = 16
    rng = np.random.default_rng(1600)
    catalogue = (rng.uniform(0.0, N, size=(300, 3)), 10.0 ** rng.uniform(7.8, 11.0, size=300))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        runs = {}
        for mode in ("resident", "host", "numpy"):
            if p.cuda_is_init():
                p.device_close()
            runs[mode] = _class_run(pc2r, M, N, mode, catalogue, (1.0e11, 3.0e11, 1.0e11), params=PLAIN_PARAMS)
        xh, lists, _ = runs["numpy"]
        assert np.all(np.isfinite(xh)) and lists[0][0].shape[1] > 100
        for mode in ("resident", "host"):
            assert all(s > 0 for s in runs[mode][2])
            for (pa, fa), (pb, fb) in zip(runs[mode][1], lists):
                assert np.array_equal(pa, pb) and fa.tobytes() == fb.tobytes(), mode
            np.testing.assert_allclose(runs[mode][0], xh, rtol=1e-11, atol=0)
    finally:
        if p.cuda_is_init():
            p.device_close()
        os.chdir(cwd)
