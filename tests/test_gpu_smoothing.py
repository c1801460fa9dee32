"""GPU: the smoothing (asora_smooth_field, smoothed_field, C2Ray.observed_map) against its numpy statement,
tests/smoothing_reference.py, and against answers that owe nothing to a transform.  Every call is made twice and compared byte for
byte.

The tolerance is derived, not tuned.  The forward transform errs by at most c(N) ||ghat||_2, c(N) = 8 eps (log2 N^3 + p) of
tests/powerspec_reference.py; the inverse of W ghat by at most c(N) ||W ghat||_2; the multiplication by W costs 4 eps per mode.  With
Parseval, ||h - h_ref||_2 <= 2.5 c(N) max|W| ||g||_2.  Every test prints the share of that bound it uses.

* Meshes: every specialised radix alone (2, 3, 4, 5, 7), the generic butterfly (17, 43, 129 = 3 x 43), repeated and mixed radices, odd
  and even N, tail tiles of the strided passes (N / 2 + 1 no multiple of the tile); 144 takes 8 lines per workgroup and 280 takes 4 (the
  round trip only, which needs no numpy transform).
* The meshes of tests/fft_meshes.py (121, 139, 140, 169, 243, 256, 271, 272, 273; each row says what it is there for, and
  tests/test_fft_meshes_host.py checks that it is so): the round trip at all nine -- both edges of the tile rule, tails in every pass
  at 16, 8 and 4 lines per workgroup, two generic stages, five stages, primes up to 271, 256^3; the filter pass against numpy at 121,
  169 and 273 (a tail tile at each tile size); the boxcar at 140 and 272; the statistics at 121 (four trips of the one-workgroup
  fold, the last partial).
* Statistics at N = 30 (a part of the second pass's fixed grid of 512 workgroups holds no cell) and at N = 72: 72^2 / 16 = 324 row
  workgroups, so the one-workgroup fold of their partials makes two trips, and 72^3 = 373 248 cells are 2.85 trips of the second
  pass's 131 072 threads, so some threads make three and some two."""
import ctypes as C
import os

import numpy as np
import pytest

import bubble_reference as BR
import fft_meshes as FM
import powerspec_reference as PR
import smoothing_reference as SR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OBSERVED_PARAMS = os.path.join(HERE, "data", "parameters_observed_map.yml")
ROUND_TRIP_MESHES = (2, 3, 4, 5, 7, 8, 9, 17, 30, 43, 64, 96, 129, 136, 144, 280)
FILTER_MESHES = (8, 9, 17, 30, 43, 64, 96)
FILTER_TAIL_MESHES = (121, 169, 273)        # 16, 8 and 4 lines per workgroup, each with a tail tile in the pass along i


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


def _twice(lib, *args, **kw):
    got, again = lib.smooth_field(*args, **kw), lib.smooth_field(*args, **kw)
    for key in ("stats", "hist", "field"):
        assert (got[key] is None) == (again[key] is None), key
        if got[key] is not None:
            assert got[key].tobytes() == again[key].tobytes(), key
    assert got["stats"].shape == (10,) and (got["hist"] is None or got["hist"].dtype == np.uint64)
    return got


def _norm(a):
    return float(np.linalg.norm(np.asarray(a).ravel()))


def _check_field(what, N, h, want, max_w, g):
    bound = 2.5 * PR.c_of_N(N) * max_w * _norm(g)
    err = _norm(h - want)
    print(f"{what}: ||h - h_ref|| = {err:.3e} uses {err / bound:.3e} of its bound")
    assert err <= bound, (what, err, bound)
    return err / bound


def _same_power_spectrum(a, b):
    for key in ("count", "sum_k", "sum_aa", "moments_a"):
        assert a[key].tobytes() == b[key].tobytes(), key


@pytest.mark.parametrize("N", ROUND_TRIP_MESHES)
def test_round_trip(asora, N):
    """1. Without a table h is g again, within 2.5 c(N) ||g||: no reference is involved.  The input moments are the power spectrum's,
    bit for bit.  6. The power spectrum after a smoothing call returns the bytes it returned before: they share the complex buffer."""
    p, lib, capi = asora
    _mesh(asora, N)
    g = PR.noise_with_block(N, 2000 + N)
    lib.grid_to_device(capi.GRID_XH, g)
    thr = PR.thresholds_of(np.arange(0, max(N // 2, 1) + 1) + 0.5)
    before = lib.power_spectrum(capi.PS_XH, None, 1.0, 0.0, thr)
    got = _twice(lib, capi.PS_XH, 1.0, 0.0, field=True)
    _check_field(f"N {N}, round trip", N, got["field"], g, 1.0, g)
    s = got["stats"]
    assert s[capi.SMOOTH_INPUT_SUM:capi.SMOOTH_INPUT_SUM2 + 1].tobytes() == before["moments_a"].tobytes()
    assert s[capi.SMOOTH_N_FINITE] == N ** 3 and s[capi.SMOOTH_N_NONFINITE] == 0
    assert s[capi.SMOOTH_MIN] == got["field"].min() and s[capi.SMOOTH_MAX] == got["field"].max()
    _same_power_spectrum(before, lib.power_spectrum(capi.PS_XH, None, 1.0, 0.0, thr))
    assert np.array_equal(lib.grid_to_host(capi.GRID_XH, np.empty((N, N, N))), g)             # no grid is written


@pytest.mark.parametrize("N", FM.MESHES)
def test_round_trip_at_the_meshes_of_the_table(asora, N):
    """The same at the meshes of tests/fft_meshes.py: every pass of the inverse at both edges of the tile rule, with tails at 16, 8
    and 4 lines per workgroup, two generic stages, five stages, primes up to 271, and 256^3."""
    test_round_trip(asora, N)


@pytest.mark.parametrize("N", FILTER_MESHES)
def test_filters_against_the_numpy_statement(asora, N):
    """2. Five filters with the mean kept and removed on the ionised fraction; the brightness temperature with and without the
    spin-temperature factor through the telescope's filter (mean removed) and a product of a separable and a radial one (kept)."""
    p, lib, capi = asora
    import pyc2ray_amd.smoothing as S
    _mesh(asora, N)
    rng = np.random.default_rng(500 + N)
    x = np.clip(0.5 + 0.25 * PR.noise_with_block(N, 3000 + N), 0.0, 1.0)
    n = 1e-4 * np.exp(0.7 * rng.normal(size=(N, N, N)))
    T = 200.0 + 2e4 * rng.random((N, N, N))
    for which, grid in ((capi.GRID_XH, x), (capi.GRID_NDENS, n), (capi.GRID_TEMP, T)):
        lib.grid_to_device(which, grid)
    product = S.gaussian(2.0, axes=(0, 2)) * S.spherical_tophat(1.5)
    filters = {"telescope": S.telescope(2.5, 3), "gaussian": S.gaussian(3.0), "tophat": S.spherical_tophat(2.0), "sharp_k": S.sharp_k(N / 4),
               "product": product}
    thr = PR.thresholds_of([0.5, N])
    cases = [(capi.PS_XH, 1.0, 0.0, name, sub) for name in filters for sub in (False, True)]
    cases += [(capi.PS_HI, 27.3, t_gamma, name, sub) for t_gamma in (0.0, 30.0) for name, sub in (("telescope", True), ("product", False))]
    formed, worst = {}, 0.0
    for kind, scale, t_gamma, name, sub in cases:
        key = (kind, scale, t_gamma)
        if key not in formed:           # the field as the device forms it (tests/test_gpu_powerspec.py checks the forming), and its transform
            ps = lib.power_spectrum(kind, None, scale, t_gamma, thr, field=True)
            formed[key] = (ps["field"], np.fft.rfftn(ps["field"]), ps["moments_a"])
        g, ghat, moments = formed[key]
        tables = filters[name].tables(N)
        got = _twice(lib, kind, scale, t_gamma, *tables, subtract_mean=sub, field=True)
        W = SR.filter_on_mesh(N, tables, sub)
        want = np.fft.irfftn(W * ghat, s=(N, N, N), axes=(0, 1, 2))
        worst = max(worst, _check_field(f"N {N}, kind {kind}, t_gamma {t_gamma}, {name}, subtract_mean {sub}", N, got["field"], want,
                                        float(np.abs(W).max()), g))
        assert got["stats"][capi.SMOOTH_INPUT_SUM:capi.SMOOTH_INPUT_SUM2 + 1].tobytes() == moments.tobytes()
        if sub:                          # the mean is gone: what is left of it is rounding, far below the field's spread
            assert abs(got["stats"][capi.SMOOTH_SUM]) <= 2.5 * PR.c_of_N(N) * N ** 1.5 * _norm(g)
    print(f"N {N}: the largest share of the bound used is {worst:.3e}")


@pytest.mark.parametrize("N", FILTER_TAIL_MESHES)
def test_filters_beyond_sixteen_lines(asora, N):
    """2. at 121, 169 and 273 (tests/fft_meshes.py): the filter pass with a tail tile at 16, 8 and 4 lines per workgroup -- its three
    tables and its per-column indices behind line buffers of another size, w_r looked up at |m|^2 up to 3 x 136^2.  A product with
    all four tables on the ionised fraction, mean kept and removed; the telescope's filter on the brightness temperature with the
    spin-temperature factor, mean removed."""
    p, lib, capi = asora
    import pyc2ray_amd.smoothing as S
    _mesh(asora, N)
    rng = np.random.default_rng(500 + N)
    x = np.clip(0.5 + 0.25 * PR.noise_with_block(N, 3000 + N), 0.0, 1.0)
    n = 1e-4 * np.exp(0.7 * rng.normal(size=(N, N, N)))
    T = 200.0 + 2e4 * rng.random((N, N, N))
    for which, grid in ((capi.GRID_XH, x), (capi.GRID_NDENS, n), (capi.GRID_TEMP, T)):
        lib.grid_to_device(which, grid)
    filters = {"product": S.gaussian(2.0, axes=(0, 2)) * S.boxcar(3, 1) * S.spherical_tophat(1.5), "telescope": S.telescope(2.5, 3)}
    assert all(w is not None for w in filters["product"].tables(N))
    thr = PR.thresholds_of([0.5, N])
    worst = 0.0
    for kind, scale, t_gamma, name, subs in ((capi.PS_XH, 1.0, 0.0, "product", (False, True)), (capi.PS_HI, 27.3, 30.0, "telescope", (True,))):
        ps = lib.power_spectrum(kind, None, scale, t_gamma, thr, field=True)
        g, ghat = ps["field"], np.fft.rfftn(ps["field"])
        tables = filters[name].tables(N)
        for sub in subs:
            got = _twice(lib, kind, scale, t_gamma, *tables, subtract_mean=sub, field=True)
            W = SR.filter_on_mesh(N, tables, sub)
            want = np.fft.irfftn(W * ghat, s=(N, N, N), axes=(0, 1, 2))
            worst = max(worst, _check_field(f"N {N}, kind {kind}, t_gamma {t_gamma}, {name}, subtract_mean {sub}", N, got["field"], want,
                                            float(np.abs(W).max()), g))
            assert got["stats"][capi.SMOOTH_INPUT_SUM:capi.SMOOTH_INPUT_SUM2 + 1].tobytes() == ps["moments_a"].tobytes()
            if sub:
                assert abs(got["stats"][capi.SMOOTH_SUM]) <= 2.5 * PR.c_of_N(N) * N ** 1.5 * _norm(g)
    print(f"N {N}: the largest share of the bound used is {worst:.3e}")


@pytest.mark.parametrize("N", [9, 16, 140, 272])
def test_boxcar_is_the_moving_average(asora, N):
    """3. boxcar(3, axis) per axis against the periodic three-cell moving average: an answer that owes nothing to a transform, at
    16, 8 (N = 140) and 4 (N = 272) lines per workgroup."""
    p, lib, capi = asora
    import pyc2ray_amd.smoothing as S
    _mesh(asora, N)
    g = PR.noise_with_block(N, 4000 + N)
    lib.grid_to_device(capi.GRID_XH, g)
    for axis in (0, 1, 2):
        tables = S.boxcar(3, axis).tables(N)
        got = _twice(lib, capi.PS_XH, 1.0, 0.0, *tables, field=True)
        _check_field(f"N {N}, boxcar(3, {axis})", N, got["field"], SR.moving_average(g, 3, axis), 1.0, g)


def _edge_sets(h):
    """1, 7 and 4096 bins whose edges are cell values: cells below the first, at or above the last, and exactly on every edge"""
    q = np.unique(h[np.isfinite(h)])
    assert q.size >= 4200
    pick = lambda count: q[np.unique(np.linspace(q.size // 10, q.size - q.size // 10, count).astype(int))]
    return {1: pick(2), 7: pick(8), 4096: pick(4097)}


@pytest.mark.parametrize("N", [30, 72])
def test_statistics_against_the_downloaded_field(asora, N, bins=(1, 7, 4096)):
    """4. Counts, min, max and the histogram equal numpy's on the field the device returns; the sums are within 1e-13 of exact
    summation of the same terms."""
    p, lib, capi = asora
    import pyc2ray_amd.smoothing as S
    _mesh(asora, N)
    lib.grid_to_device(capi.GRID_XH, PR.noise_with_block(N, 5000 + N))
    tables = S.telescope(2.5, 3).tables(N)
    first = _twice(lib, capi.PS_XH, 1.0, 0.0, *tables, field=True)
    h = first["field"]
    want = SR.statistics(h)
    for edges in [None] + [e for count, e in _edge_sets(h).items() if count in bins]:
        got = _twice(lib, capi.PS_XH, 1.0, 0.0, *tables, edges=edges, field=True)
        assert got["field"].tobytes() == h.tobytes() and got["stats"].tobytes() == first["stats"].tobytes()
        if edges is not None:
            ref = SR.histogram(h, edges)
            assert got["hist"].shape == (edges.size + 1,) and np.array_equal(got["hist"], ref), edges.size
            assert ref[-2] > 0 and ref[-1] > 0 and int(ref.sum()) == N ** 3 and np.all(np.isin(edges, h))
    s = first["stats"]
    for key in (capi.SMOOTH_N_FINITE, capi.SMOOTH_N_NONFINITE, capi.SMOOTH_MIN, capi.SMOOTH_MAX):
        assert s[key] == want[key], key
    for key in (capi.SMOOTH_SUM, capi.SMOOTH_S2, capi.SMOOTH_S3, capi.SMOOTH_S4):
        print(f"N {N}, stats[{key}]: {s[key]!r} against {want[key]!r}: off by {abs(s[key] - want[key]) / abs(want[key]):.2e}")
        assert abs(s[key] - want[key]) <= 1e-13 * abs(want[key]), key


def test_statistics_with_a_partial_fourth_trip_of_the_fold(asora):
    """4. at N = 121: 121^2 / 16 = 916 row workgroups, so the one-workgroup fold of their partials makes four trips, the last of 148,
    and the last row workgroup holds one line; 121^3 cells are 13.5 trips of the second pass.  The 7 and the 4096 bins only."""
    test_statistics_against_the_downloaded_field(asora, 121, bins=(7, 4096))


def test_non_finite_cells_are_counted_apart(asora):
    """4. Kind 'hi' with t_gamma > 0 and one cell of temperature 0: that cell of g is -inf, and the transform mixes every cell into
    every other, so h is non-finite throughout.  The counts and the histogram are numpy's on the downloaded field; min and max are
    those of no cell; the sums are not finite."""
    p, lib, capi = asora
    N = 30
    _mesh(asora, N)
    rng = np.random.default_rng(9)
    T = 200.0 + 2e4 * rng.random((N, N, N))
    T[3, 4, 5] = 0.0
    for which, grid in ((capi.GRID_XH, 0.5 * rng.random((N, N, N))), (capi.GRID_NDENS, 1e-4 * (1.0 + rng.random((N, N, N)))), (capi.GRID_TEMP, T)):
        lib.grid_to_device(which, grid)
    edges = np.linspace(-100.0, 100.0, 8)
    got = _twice(lib, capi.PS_HI, 27.3, 30.0, subtract_mean=True, edges=edges, field=True)
    h, s = got["field"], got["stats"]
    want = SR.statistics(h)
    assert s[capi.SMOOTH_N_NONFINITE] == want[SR.N_NONFINITE] >= 1 and s[capi.SMOOTH_N_FINITE] == want[SR.N_FINITE]
    print(f"one cell of temperature 0: {int(s[capi.SMOOTH_N_FINITE])} finite and {int(s[capi.SMOOTH_N_NONFINITE])} non-finite cells")
    assert s[capi.SMOOTH_N_FINITE] == 0 and s[capi.SMOOTH_N_NONFINITE] == N ** 3
    assert s[capi.SMOOTH_MIN] == want[SR.MIN] and s[capi.SMOOTH_MAX] == want[SR.MAX]
    assert np.array_equal(got["hist"], SR.histogram(h, edges)) and int(got["hist"].sum()) == int(want[SR.N_FINITE])
    assert not np.isfinite(s[capi.SMOOTH_INPUT_SUM]) and not np.isfinite(s[capi.SMOOTH_SUM]) and not np.isfinite(s[capi.SMOOTH_S2])


def test_the_result_in_a_grid(asora):
    """5. dst_grid: the grid holds the field of field_out, the threshold pass of the mask analyses takes it by its selector, and a
    grid that is both source and target gives the bytes of a call without one."""
    p, lib, capi = asora
    import pyc2ray_amd.smoothing as S
    N = 43
    _mesh(asora, N)
    g = np.clip(0.5 + 0.4 * PR.noise_with_block(N, 6000), 0.0, 1.0)
    lib.grid_to_device(capi.GRID_XH, g)
    tables = S.gaussian(3.0).tables(N)
    plain = _twice(lib, capi.PS_XH, 1.0, 0.0, *tables, field=True)
    with pytest.raises(RuntimeError, match="holds no data"):
        lib.grid_to_host(capi.GRID_XH_AV, np.empty((N, N, N)))
    into = _twice(lib, capi.PS_XH, 1.0, 0.0, *tables, dst_grid=capi.GRID_XH_AV, field=True)
    assert into["field"].tobytes() == plain["field"].tobytes() and into["stats"].tobytes() == plain["stats"].tobytes()
    assert lib.grid_to_host(capi.GRID_XH_AV, np.empty((N, N, N))).tobytes() == into["field"].tobytes()
    assert np.array_equal(lib.grid_to_host(capi.GRID_XH, np.empty((N, N, N))), g)
    for phase in (0, 1):
        words, rows = lib.bubble_mask(capi.GRID_XH_AV, 0.5, phase)
        ref_words, ref_rows = BR.mask_words(BR.in_phase(into["field"], 0.5, phase))
        assert np.array_equal(words, ref_words) and np.array_equal(rows, ref_rows), phase
    assert 0 < int(lib.bubble_mask(capi.GRID_XH_AV, 0.5, 0)[1].sum()) < N ** 3
    # the source is the target: the whole forward transform is ordered before the first write
    own = lib.smooth_field(capi.PS_XH, 1.0, 0.0, *tables, dst_grid=capi.GRID_XH, field=True)
    assert own["field"].tobytes() == plain["field"].tobytes() and own["stats"].tobytes() == plain["stats"].tobytes()
    assert lib.grid_to_host(capi.GRID_XH, np.empty((N, N, N))).tobytes() == plain["field"].tobytes()
    # the package's call: into a grid, the histogram of an int in two calls
    import pyc2ray_amd as pc2r
    sf = pc2r.smoothed_field(g, filter=S.gaussian(3.0), bins=16, into=capi.GRID_XH_AV, return_field=True)
    assert sf.field.tobytes() == plain["field"].tobytes() and sf.stats.tobytes() == plain["stats"].tobytes()
    assert int(sf.hist.sum()) == N ** 3 and (sf.below, sf.above) == (0, 0) and sf.edges[0] == sf.min and sf.edges[-1] > sf.max
    assert np.array_equal(np.concatenate([sf.hist, [0, 0]]).astype(np.uint64), SR.histogram(sf.field, sf.edges))
    assert abs(sf.variance - sf.field.var()) <= 1e-12 * sf.variance and sf.variance < sf.input_variance


def test_refusals_leave_the_outputs_untouched(asora):
    """7. Every code of the header's list (10, a failed allocation, cannot be provoked); a refused call writes nothing."""
    p, lib, capi = asora
    raw = capi.load()
    N, nb = 8, 3
    SENT = 12345.0
    n_r = SR.n_radial(N)
    sym = np.array([1.0, 0.9, 0.8, 0.7, 0.6, 0.7, 0.8, 0.9])

    def call(kind=capi.PS_XH, scale=1.0, t_gamma=0.0, w_i=None, w_j=None, w_k=None, w_r=None, n_r=0, n_hist=nb, edges=(0.0, 0.3, 0.6, 0.9),
             dst_grid=-1, null=()):
        arrays = [None if w is None else np.array(w, dtype=np.float64) for w in (w_i, w_j, w_k, w_r)]
        e = None if edges is None else np.array(edges, dtype=np.float64)
        out = dict(stats=np.full(10, SENT), hist=np.full(nb + 2, 12345, dtype=np.uint64), field=np.full(N ** 3, SENT))
        ptr = lambda a: None if a is None else capi.dptr(a)
        rc = raw.asora_smooth_field(kind, scale, t_gamma, *[ptr(a) for a in arrays], n_r, 0, n_hist, ptr(e), dst_grid,
                                    None if "stats" in null else capi.dptr(out["stats"]),
                                    None if "hist" in null else out["hist"].ctypes.data_as(capi._u64p), capi.dptr(out["field"]))
        untouched = all(np.all(v == 12345) for v in out.values())
        return rc, untouched, raw.asora_last_error() or b""

    if p.cuda_is_init():
        p.device_close()
    rc, untouched, msg = call()
    assert rc == 2 and untouched and b"smooth_field" in msg
    p.device_init(N, 8)
    # 4: a grid the kind needs holds no data
    assert call()[:2] == (4, True)
    x = np.random.default_rng(1).random((N, N, N))
    lib.grid_to_device(capi.GRID_XH, x)
    assert call(kind=capi.PS_DENSITY)[:2] == (4, True) and call(kind=capi.PS_HI)[:2] == (4, True)
    lib.grid_to_device(capi.GRID_NDENS, np.full((N, N, N), 2.0))
    rc, untouched, msg = call(kind=capi.PS_HI, t_gamma=30.0, dst_grid=capi.GRID_XH)
    assert rc == 4 and untouched and b"holds no data" in msg
    # 3: the arguments
    bad_sym, nan_tab, inf_r = sym.copy(), sym.copy(), np.ones(n_r)
    bad_sym[2] = np.nextafter(bad_sym[2], 1.0)
    nan_tab[4] = np.nan
    inf_r[n_r - 1] = np.inf
    for kw in (dict(kind=-1), dict(kind=4), dict(scale=np.nan), dict(scale=np.inf), dict(t_gamma=np.nan), dict(t_gamma=np.inf),
               dict(t_gamma=-1.0), dict(w_i=nan_tab), dict(w_j=nan_tab), dict(w_k=nan_tab), dict(w_r=inf_r, n_r=n_r), dict(w_i=bad_sym),
               dict(w_j=bad_sym), dict(w_r=np.ones(n_r), n_r=n_r - 1), dict(w_r=np.ones(n_r + 1), n_r=n_r + 1), dict(w_r=np.ones(n_r), n_r=0),
               dict(n_hist=-1), dict(n_hist=4097, edges=np.arange(4098.0)), dict(edges=(0.0, 0.6, 0.3, 0.9)), dict(edges=(0.0, 0.3, 0.3, 0.9)),
               dict(edges=(0.0, 0.3, 0.6, np.inf)), dict(edges=(np.nan, 0.3, 0.6, 0.9)), dict(edges=None), dict(null=("hist",)),
               dict(dst_grid=-2), dict(dst_grid=9), dict(null=("stats",))):
        rc, untouched, msg = call(dst_grid=kw.pop("dst_grid", capi.GRID_XH), **kw)
        assert rc == 3 and untouched and b"smooth_field" in msg, kw
    # ... on the device neither: the grid a refused call named as its target is what it was, and no other grid has come to be
    assert np.array_equal(lib.grid_to_host(capi.GRID_XH, np.empty((N, N, N))), x)
    with pytest.raises(RuntimeError, match="holds no data"):
        lib.grid_to_host(capi.GRID_XH_AV, np.empty((N, N, N)))
    # accepted: w_k need not be symmetric (it is read at the stored half only); no histogram without edges and hist; a negative scale;
    # kind 'hi' without t_gamma needs no temperature; the stage times of a call under the timing option
    assert call(w_i=sym, w_j=sym, w_k=np.arange(1.0, 9.0), w_r=np.ones(n_r), n_r=n_r)[:2] == (0, False)
    assert call(n_hist=0, edges=None, null=("hist",))[0] == 0 and call(kind=capi.PS_HI, scale=-3.0)[0] == 0
    lib.set_option(capi.OPT_TIMING, 1)
    try:
        lib.smooth_field(capi.PS_HI, 1.0, 0.0, edges=[0.0, 0.5, 1.0])
        ms = lib.smooth_field_ms()
        print(f"stage times at N {N}: {ms.tolist()} ms")
        assert ms.shape == (capi.SMOOTH_STAGES,) and np.all(ms > 0.0)
    finally:
        lib.set_option(capi.OPT_TIMING, 0)


def test_class(asora, tmp_path):
    """8. The single black-body run at its test mesh with the observed-map keys: every step on the resident path leaves its map's
    statistics and one line in the log; observed_map() reads the grids where they lie and equals, bit for bit, the module-level call
    on the downloaded grids; so does the upload form."""
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.smoothing as S
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N, dt = 24, 3.15576e13
        with open("src.txt", "w") as f:
            f.write("1\n12 12 12 5e50 1.0\n")
        if p.cuda_is_init():
            p.device_close()
        sim = pc2r.C2Ray_Test(OBSERVED_PARAMS, N, True)
        assert sim.device_resident and sim.observed_stats is True and sim.last_observed is None
        sim.density_init(0.0)
        srcpos, srcflux = sim.read_sources("src.txt", 1)
        results = []
        for _ in range(2):
            sim.evolve3D(dt, srcflux, srcpos)
            results.append(sim.last_observed)
        assert all(r is not None for r in results) and results[0] is not results[1]
        assert sim._device_newer >= {"xh", "phi_ion"}             # nothing was fetched
        last = results[1]
        width = sim.beam_fwhm_cells(8000.0)
        assert 2.0 < width < 5.0 and last.kind == "dtb" and last.N == N and last.subtract_mean and last.hist.size == 5
        assert int(last.hist.sum()) == N ** 3 and last.n_nonfinite == 0 and abs(last.mean) <= 1e-10 * last.max
        assert last.variance > 0 and last.variance < last.input_variance and last.min < 0 < last.max
        assert open(sim.logfile).read().count("Smoothed field (dtb, gaussian(") == 2
        again = sim.observed_map()
        kin = sim.observed_map(spin="kinetic", bins=[-50.0, 0.0, 50.0], return_field=True)
        assert sim._device_newer >= {"xh", "phi_ion"}
        assert again.stats.tobytes() == last.stats.tobytes() and again.hist.tobytes() == last.hist.tobytes()
        scale, t_gamma = sim.brightness_temperature_scale(), 2.726 * (1 + sim.zred)
        # the downloaded grids, and the module-level call on them
        x, n, T = sim.xh.copy(), np.array(sim.ndens, dtype=np.float64), np.array(sim.temp, dtype=np.float64) * np.ones((N, N, N))
        for which, grid in ((capi.GRID_XH, x), (capi.GRID_NDENS, n), (capi.GRID_TEMP, T)):
            lib.grid_to_device(which, grid)
        filt = S.telescope(width, width, los_axis=1)
        m = pc2r.smoothed_field(None, kind="dtb", filter=filt, subtract_mean=True, scale=scale, bins=5)
        assert m.stats.tobytes() == last.stats.tobytes() and m.hist.tobytes() == last.hist.tobytes() and m.edges.tobytes() == last.edges.tobytes()
        m = pc2r.smoothed_field(None, kind="dtb", filter=filt, subtract_mean=True, scale=scale, t_gamma=t_gamma, bins=[-50.0, 0.0, 50.0],
                                return_field=True)
        assert m.stats.tobytes() == kin.stats.tobytes() and m.hist.tobytes() == kin.hist.tobytes() and m.field.tobytes() == kin.field.tobytes()
        g = PR.form_field(PR.HI, x, n, T, scale, t_gamma)
        W = SR.filter_on_mesh(N, filt.tables(N), True)
        _check_field("class", N, kin.field, SR.smooth(g, filt.tables(N), True), float(np.abs(W).max()), g)
        fallback = sim.observed_map()                              # the host copies are the newer ones now: the upload form
        assert fallback.stats.tobytes() == last.stats.tobytes() and fallback.hist.tobytes() == last.hist.tobytes()
    finally:
        if p.cuda_is_init():
            p.device_close()
        os.chdir(cwd)
