"""GPU: the redshift-space mapping and the anisotropic power sums (asora_los_velocity_to_device, asora_redshift_space_field,
asora_power_spectrum_los, power_spectrum_los, C2Ray.power_spectrum_los) against their numpy statement,
tests/redshift_space_reference.py.  Every call is made twice and compared byte for byte.

The mapping is specified operation by operation, so the device's field is compared with the reference's bit for bit.  The sums
carry the bounds of tests/test_gpu_powerspec.py: counts exactly; the sums that hang on integers alone (sum_1, sum_2) to 1e-13
relative; the power sums within 4 c(N) sqrt(sum_aa total_aa), c(N) of tests/powerspec_reference.py -- |L_2|, |L_4| <= 1 on
0 <= mu^2 <= 1, so the Cauchy-Schwarz argument for sum_aa bounds the Legendre-weighted sums of the same modes as well."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import powerspec_reference as PR
import redshift_space_reference as RR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RS_PARAMS = os.path.join(HERE, "data", "parameters_redshift_space.yml")
SUM_KEYS = ("count", "sum_1", "sum_2", "sum_aa", "sum_l2", "sum_l4")
KEYS = SUM_KEYS + ("moments_real", "moments_rs", "field", "modes")
# all three axes at 4, 17 and 30; 17 and 129 leave a ragged last tile on either tiling; at (65, 0), (129, 1) and from (64, 2) on a tile
# holds more cells than its workgroup has work items (16 x 65 and 16 x 129 against 1024; 31 x 64 and 15 x 129 against 256), with a
# last tile of one column at the first two
MAP_CASES = [(3, 2), (4, 0), (4, 1), (4, 2), (8, 2), (17, 0), (17, 1), (17, 2), (30, 0), (30, 1), (30, 2), (64, 2), (65, 0), (129, 1), (129, 2)]
N_TRIPS = 169         # NZ = 85: the binning's loop over n_z makes two trips
SUM_CASES = [(N, axis) for N in (4, 5, 8, 17, 30) for axis in (0, 1, 2)] + [(64, 2), (64, 0), (N_TRIPS, 2), (N_TRIPS, 0)]


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


def _same(got, again, keys):
    for key in keys:
        assert (got[key] is None) == (again[key] is None), key
        if got[key] is not None:
            assert got[key].tobytes() == again[key].tobytes(), key
    return got


def _spectrum_twice(lib, *args, **kw):
    got = _same(lib.power_spectrum_los(*args, **kw), lib.power_spectrum_los(*args, **kw), KEYS)
    assert got["count"].dtype == np.uint64
    return got


def _field_twice(lib, *args, **kw):
    return _same(lib.redshift_space_field(*args, field=True, **kw), lib.redshift_space_field(*args, field=True, **kw), ("moments", "field"))


def _velocities(N, axis, seed):
    """name -> (v, velocity_scale); u = v velocity_scale"""
    rng = np.random.default_rng(seed)
    shape = (N, N, N)
    top = (N - 1) // 2                      # the widest window the library takes: W = top
    cases = {"zero": (np.zeros(shape), 1.0),
             "one cell": (rng.uniform(-0.999, 0.999, size=shape) * 40.0, 1.0 / 40.0),
             "widest": (rng.uniform(-0.999 * top, 0.999 * top, size=shape), -1.0)}
    if N >= 5:
        cases["plus"] = (np.full(shape, 0.5), 2.0)
        cases["minus"] = (np.full(shape, 4.0), -0.25)
    if N >= 8:                               # the degenerate cell: u[3] = -2 on every line collapses cell 2
        v = np.zeros(shape)
        index = [slice(None)] * 3
        index[axis] = 3
        v[tuple(index)] = -2.0
        cases["degenerate"] = (v, 1.0)
    return cases


def _some_lines(N, axis, rng, count=1500):
    """flat indices of lines along `axis`: the first and the last 40 (whole first and last tiles) and random ones between"""
    rows = N * N
    return np.unique(np.r_[np.arange(40), np.arange(rows - 40, rows), rng.integers(0, rows, size=count)])


@pytest.mark.parametrize("N,axis", MAP_CASES)
def test_mapping_bit_for_bit(asora, N, axis):
    p, lib, capi = asora
    _mesh(asora, N)
    rng = np.random.default_rng(500 + 3 * N + axis)
    g = rng.random((N, N, N)) + 0.25
    lib.grid_to_device(capi.GRID_XH, g)
    thr_a, thr_b = PR.thresholds_of(np.arange(0, max(N // 2, 1) + 1) + 0.5), np.array([0.0, 2.0])
    for name, (v, vscale) in _velocities(N, axis, 900 + N).items():
        vmax = lib.los_velocity_to_device(v)
        assert vmax == float(np.max(np.abs(v))), name
        W = RR.library_window(vmax, vscale)
        assert 2 * W + 1 <= N, name
        got = _spectrum_twice(lib, capi.PS_XH, 1.0, 0.0, axis, vscale, capi.ANISO_MU, thr_a, thr_b, field=True)
        if name == "widest" and N > 64:      # (the reference takes 2 W + 1 passes over its cells: some of the lines)
            pick = _some_lines(N, axis, rng)
            lines = lambda a: np.moveaxis(a, axis, -1).reshape(N * N, N)[pick]
            want, mine = RR.map_lines(lines(g), lines(v), vscale, -1), lines(got["field"])
        else:
            want, mine = RR.map_lines(g, v, vscale, axis), got["field"]
        assert mine.tobytes() == want.tobytes(), (name, int(np.sum(mine != want)))
        if name == "zero":
            assert got["field"].tobytes() == g.tobytes()
        elif name in ("plus", "minus"):
            assert np.array_equal(got["field"], np.roll(g, 1 if name == "plus" else -1, axis=axis))
        elif name == "widest" and N >= 8:
            assert RR.count_inverted(v, vscale, axis) >= 1
        elif name == "degenerate":
            line = np.moveaxis(got["field"], axis, -1)[1, N - 1], np.moveaxis(g, axis, -1)[1, N - 1]
            assert line[0][2] == line[1][3] + line[1][2] and line[0][3] == 0.5 * line[1][4] == line[0][4]
        # the mapping conserves: the sums of the field before and after it
        m_real, m_rs = got["moments_real"], got["moments_rs"]
        want_real = np.array([float(PR.exact_sum(g)), float(PR.exact_sum(g * g))])
        assert np.all(np.abs(m_real - want_real) <= 1e-13 * want_real), name
        bound = 4 * (2 * W + 3) * PR.EPS * float(np.sum(np.abs(g)))
        print(f"N {N}, axis {axis}, {name}: W {W}, sum h - sum g = {m_rs[0] - m_real[0]:.3e} (bound {bound:.3e})")
        assert abs(m_rs[0] - m_real[0]) <= bound, name
        if name in ("one cell", "degenerate"):
            # the field entry alone: the same field, in its own buffer and in a grid, and the moments of g
            alone = _field_twice(lib, capi.PS_XH, 1.0, 0.0, axis, vscale)
            assert alone["field"].tobytes() == got["field"].tobytes() and alone["moments"].tobytes() == m_real.tobytes()
            into = _field_twice(lib, capi.PS_XH, 1.0, 0.0, axis, vscale, dst_grid=capi.GRID_XH_AV)
            assert into["field"].tobytes() == got["field"].tobytes()
            assert lib.grid_to_host(capi.GRID_XH_AV, np.empty((N, N, N))).tobytes() == got["field"].tobytes()
    assert np.array_equal(lib.grid_to_host(capi.GRID_XH, np.empty((N, N, N))), g)               # no grid of the kind is written
    # the source is the target: a workgroup has read its lines before it writes them
    own = lib.redshift_space_field(capi.PS_XH, 1.0, 0.0, axis, vscale, dst_grid=capi.GRID_XH, field=True)
    assert own["field"].tobytes() == got["field"].tobytes()
    assert lib.grid_to_host(capi.GRID_XH, np.empty((N, N, N))).tobytes() == got["field"].tobytes()
    # without a velocity the field entry forms the field and no more
    assert lib.redshift_space_field(capi.PS_XHI, 1.0, 0.0, axis, None, field=True)["field"].tobytes() == (1.0 - got["field"]).tobytes()


def test_mapping_the_brightness_temperature(asora):
    """kind 'dtb' with t_gamma > 0 at N = 17: h is the reference's mapping of the field a plain power_spectrum call returns; and a
    velocity in Fortran order"""
    p, lib, capi = asora
    N = 17
    _mesh(asora, N)
    rng = np.random.default_rng(41)
    x = rng.random((N, N, N))
    n = 1e-4 * np.exp(0.7 * rng.normal(size=(N, N, N)))
    T = 200.0 + 2e4 * rng.random((N, N, N))
    for which, grid in ((capi.GRID_XH, x), (capi.GRID_NDENS, n), (capi.GRID_TEMP, T)):
        lib.grid_to_device(which, grid)
    g = lib.power_spectrum(capi.PS_HI, None, 27.3, 30.0, [1, 4, 9], field=True)["field"]
    v = rng.uniform(-3.0, 3.0, size=(N, N, N))
    for axis in (0, 1, 2):
        assert lib.los_velocity_to_device(np.asfortranarray(v)) == float(np.max(np.abs(v)))
        got = _field_twice(lib, capi.PS_HI, 27.3, 30.0, axis, 1.1)
        assert got["field"].tobytes() == RR.map_lines(g, v, 1.1, axis).tobytes(), axis
        want_m = np.array([float(PR.exact_sum(g)), float(PR.exact_sum(g * g))])
        assert np.all(np.abs(got["moments"] - want_m) <= 1e-13 * np.abs(want_m))
    for which, grid in ((capi.GRID_XH, x), (capi.GRID_NDENS, n), (capi.GRID_TEMP, T)):
        assert np.array_equal(lib.grid_to_host(which, np.empty((N, N, N))), grid)


def _bin_sets(N):
    """name -> (mode, thr_a, thr_b), with modes on the edges: integer edges, thr_a[0] = 0 in the cylindrical mode, edges of mu^2 at
    exactly 0.25 and 0.5, a last edge of mu^2 of 1.0 (mu = 1 left out) and of 2.0 (taken in)"""
    h = max(N // 2, 1)
    squares = np.arange(0, min(h, 30) + 2, dtype=np.int64) ** 2          # (31 x 31 bins at the most)
    coarse = np.unique(np.r_[0, 1, 2, 4, 9, np.linspace(10, 2 * h * h + 1, 6).astype(np.int64)])
    return {"cylindrical": (RR.CYLINDRICAL, squares.astype(np.uint32), squares.astype(np.float64)),
            "cylindrical, coarse": (RR.CYLINDRICAL, coarse.astype(np.uint32), np.array([0.0, 1.0, 2.5, float(h * h), float(h * h + 1)])),
            "mu, mu = 1 left out": (RR.MU, squares[1:].astype(np.uint32), np.array([0.0, 0.25, 0.5, 1.0])),
            "mu": (RR.MU, squares[1:].astype(np.uint32), np.array([0.0, 0.25, 0.5, 2.0])),
            "multipoles": (RR.MU, PR.thresholds_of(np.arange(0, h + 1) + 0.5), np.array([0.0, 2.0]))}


def _check_sums(N, got, want, what):
    c = PR.c_of_N(N)
    assert np.array_equal(got["count"], want["count"]), (what, got["count"].tolist(), want["count"].tolist())
    for key in ("sum_1", "sum_2"):
        err = np.abs(got[key] - want[key])
        assert np.all(err <= 1e-13 * want[key]), (what, key, float(err.max()))
    bound = 4.0 * c * np.sqrt(want["sum_aa"] * want["total_aa"])
    used = {}
    for key in ("sum_aa", "sum_l2", "sum_l4"):
        err = np.abs(got[key] - want[key])
        used[key] = float(np.max(err / np.where(bound > 0, bound, 1.0))) if err.size else 0.0
        assert np.all(err <= bound), (what, key, float(err.max()))
    print(f"{what}: {got['count'].size} bins, " + ", ".join(f"{key} uses {u:.3e}" for key, u in used.items()) + " of the bound")


@functools.lru_cache(maxsize=2)
def _field_and_transform(N):
    """the test field of the transform and numpy's transform of it (computed once per mesh; treat as read-only)"""
    field = PR.noise_with_block(N, 2000 + N)
    return field, np.fft.rfftn(field)


@pytest.mark.parametrize("N,axis", SUM_CASES)
def test_transform_and_sums(asora, N, axis):
    p, lib, capi = asora
    _mesh(asora, N)
    field, ref = _field_and_transform(N)
    lib.grid_to_device(capi.GRID_XH, field)
    sets = _bin_sets(N)
    if N >= 64:                              # (the reference's binning takes a second per set there)
        sets = {name: sets[name] for name in (("cylindrical", "mu") if axis == 2 else ("mu, mu = 1 left out", "multipoles"))}
    first = True
    for name, (mode, thr_a, thr_b) in sets.items():
        got = _spectrum_twice(lib, capi.PS_XH, 1.0, 0.0, axis, None, mode, thr_a, thr_b, field=first, modes=first)
        if first:
            # without a velocity the field and its transform have the bytes of asora_power_spectrum's for the same kind
            plain = lib.power_spectrum(capi.PS_XH, None, 1.0, 0.0, PR.thresholds_of([0.5, N]), field=True, modes=True)
            assert got["modes"].tobytes() == plain["modes"].tobytes() and got["field"].tobytes() == plain["field"].tobytes() == field.tobytes()
            assert got["moments_real"].tobytes() == got["moments_rs"].tobytes() == plain["moments_a"].tobytes()
            first = False
        want = RR.binned(N, axis, mode, thr_a, thr_b, ref)
        _check_sums(N, got, want, f"N {N}, axis {axis}, {name}")
        if name == "mu":
            # summed over mu, the counts are those of the plain power spectrum for the same thr_a
            plain = lib.power_spectrum(capi.PS_XH, None, 1.0, 0.0, thr_a)
            assert np.array_equal(got["count"].sum(axis=1), plain["count"])
            left_out = _spectrum_twice(lib, capi.PS_XH, 1.0, 0.0, axis, None, mode, thr_a, np.array([0.0, 0.25, 0.5, 1.0]))
            assert np.array_equal(left_out["count"][:, :2], got["count"][:, :2]) and int(got["count"].sum() - left_out["count"].sum()) > 0
        if name == "multipoles":
            # one bin of mu: sum_aa is the plain power spectrum's to the bound, the counts exactly
            plain = lib.power_spectrum(capi.PS_XH, None, 1.0, 0.0, thr_a)
            assert np.array_equal(got["count"][:, 0], plain["count"])
            assert np.all(np.abs(got["sum_aa"][:, 0] - plain["sum_aa"]) <= 8.0 * PR.c_of_N(N) * np.sqrt(want["sum_aa"][:, 0] * want["total_aa"]))


def test_sums_of_a_mapped_field(asora):
    """The whole chain at N = 30: the sums of a call with a velocity against the reference's binning of the reference's mapping"""
    p, lib, capi = asora
    N = 30
    _mesh(asora, N)
    field, _ = _field_and_transform(N)
    lib.grid_to_device(capi.GRID_XH, field)
    v = np.random.default_rng(8).uniform(-2.5, 2.5, size=(N, N, N))
    lib.los_velocity_to_device(v)
    for axis in (0, 1, 2):
        h = RR.map_lines(field, v, 0.8, axis)
        ref = np.fft.rfftn(h)
        for name in ("cylindrical, coarse", "mu"):
            mode, thr_a, thr_b = _bin_sets(N)[name]
            got = _spectrum_twice(lib, capi.PS_XH, 1.0, 0.0, axis, 0.8, mode, thr_a, thr_b, field=True, modes=True)
            assert got["field"].tobytes() == h.tobytes()
            err = np.linalg.norm((got["modes"] - ref).ravel()) / np.linalg.norm(ref.ravel())
            assert err <= PR.c_of_N(N)
            _check_sums(N, got, RR.binned(N, axis, mode, thr_a, thr_b, ref), f"N {N}, axis {axis}, mapped, {name}")
            want_m = np.array([float(PR.exact_sum(h)), float(PR.exact_sum(h * h))])
            assert np.all(np.abs(got["moments_rs"] - want_m) <= 1e-13 * np.abs(want_m))


def test_the_bin_limit(asora):
    """1024 two-dimensional bins, all the ABI allows, as 32 x 32 and as 1024 x 1 (two histograms per workgroup instead of four), at a
    mesh with two trips of the loop over n_z; 1025 are refused"""
    p, lib, capi = asora
    N = N_TRIPS
    _mesh(asora, N)
    field, ref = _field_and_transform(N)
    lib.grid_to_device(capi.GRID_XH, field)
    edges = np.linspace(0.0, N // 2 + 0.5, 33)
    thr = np.ceil(edges * edges)
    got = _spectrum_twice(lib, capi.PS_XH, 1.0, 0.0, 1, None, capi.ANISO_CYLINDRICAL, thr.astype(np.uint32), thr)
    assert got["count"].shape == (32, 32)
    _check_sums(N, got, RR.binned(N, 1, RR.CYLINDRICAL, thr.astype(np.uint32), thr, ref), f"N {N}, 32 x 32 bins")
    q = np.unique(PR.mode_n2(N))
    thr_a = q[np.linspace(1, q.size - 40, 1025).astype(int)].astype(np.uint32)
    got = _spectrum_twice(lib, capi.PS_XH, 1.0, 0.0, 2, None, capi.ANISO_MU, thr_a, np.array([0.0, 2.0]))
    assert got["count"].shape == (1024, 1) and np.all(got["count"] > 0)
    _check_sums(N, got, RR.binned(N, 2, RR.MU, thr_a, np.array([0.0, 2.0]), ref), f"N {N}, 1024 x 1 bins")
    for n_a, n_b in ((1025, 1), (41, 25), (1, 1025)):
        with pytest.raises(RuntimeError, match="code 3.*n_a n_b <= 1024"):
            lib.power_spectrum_los(capi.PS_XH, 1.0, 0.0, 2, None, capi.ANISO_CYLINDRICAL, np.arange(n_a + 1), np.arange(n_b + 1.0))


def test_refusals_leave_the_outputs_untouched(asora):
    p, lib, capi = asora
    raw = capi.load()
    N, na, nb = 8, 3, 2
    SENT = 12345.0

    def call(kind=capi.PS_XH, scale=1.0, t_gamma=0.0, los_axis=2, use_velocity=0, velocity_scale=1.0, mode=capi.ANISO_MU, n_a=na, thr_a=(1, 4, 9, 16),
             n_b=nb, thr_b=(0.0, 0.5, 2.0), null=(), extra=False):
        ta, tb = np.array(thr_a, dtype=np.uint32), np.array(thr_b, dtype=np.float64)
        out = dict(count=np.full(na * nb, 12345, dtype=np.uint64), field=np.full(N ** 3, SENT), modes=np.full(2 * N * N * (N // 2 + 1), SENT))
        for key in ("sum_1", "sum_2", "sum_aa", "sum_l2", "sum_l4"):
            out[key] = np.full(na * nb, SENT)
        out["moments_real"], out["moments_rs"] = np.full(2, SENT), np.full(2, SENT)
        ptr = lambda name: None if name in null else (out[name].ctypes.data_as(capi._u64p) if name == "count" else capi.dptr(out[name]))
        rc = raw.asora_power_spectrum_los(kind, scale, t_gamma, los_axis, use_velocity, velocity_scale, mode, n_a,
                                          None if "thr_a" in null else ta.ctypes.data_as(C.POINTER(C.c_uint32)), n_b,
                                          None if "thr_b" in null else capi.dptr(tb), ptr("count"), ptr("sum_1"), ptr("sum_2"), ptr("sum_aa"),
                                          ptr("sum_l2"), ptr("sum_l4"), ptr("moments_real"), ptr("moments_rs"), ptr("field") if extra else None,
                                          ptr("modes") if extra else None)
        untouched = all(np.all(v == 12345) for v in out.values())
        return rc, untouched, raw.asora_last_error() or b""

    def field_call(dst_grid=-1, **kw):
        m, f = np.full(2, SENT), np.full(N ** 3, SENT)
        args = dict(kind=capi.PS_XH, scale=1.0, t_gamma=0.0, los_axis=2, use_velocity=0, velocity_scale=1.0)
        args.update(kw)
        rc = raw.asora_redshift_space_field(args["kind"], args["scale"], args["t_gamma"], args["los_axis"], args["use_velocity"],
                                            args["velocity_scale"], dst_grid, capi.dptr(m), capi.dptr(f))
        return rc, bool(np.all(m == SENT) and np.all(f == SENT))

    if p.cuda_is_init():
        p.device_close()
    rc, untouched, msg = call()
    assert rc == 2 and untouched and b"power_spectrum_los" in msg and field_call() == (2, True)
    assert raw.asora_los_velocity_to_device(capi.dptr(np.zeros(N ** 3)), N, b"C", None) == 2
    p.device_init(N, 8)
    # 4: a grid the kind needs holds no data
    assert call(extra=True)[:2] == (4, True) and field_call(dst_grid=capi.GRID_XH_AV) == (4, True)
    x = np.random.default_rng(1).random((N, N, N))
    lib.grid_to_device(capi.GRID_XH, x)
    assert call(kind=capi.PS_DENSITY)[:2] == (4, True) and call(kind=capi.PS_HI)[:2] == (4, True)
    lib.grid_to_device(capi.GRID_NDENS, np.full((N, N, N), 2.0))
    rc, untouched, msg = call(kind=capi.PS_HI, t_gamma=30.0, extra=True)
    assert rc == 4 and untouched and b"holds no data" in msg
    # 3: use_velocity without an upload; a NaN or an infinity in the velocity, which leaves the velocity of the last good upload
    rc, untouched, msg = call(use_velocity=1, extra=True)
    assert rc == 3 and untouched and b"without a velocity on the device" in msg
    assert field_call(use_velocity=1, dst_grid=capi.GRID_XH) == (3, True)
    good = np.full((N, N, N), 0.5)
    good[3, 4, 5] = -2.9
    assert lib.los_velocity_to_device(good) == 2.9
    for poison in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad[7, 7, 7] = poison
        with pytest.raises(RuntimeError, match="code 3.*non-finite entry"):
            lib.los_velocity_to_device(bad)
    assert call(use_velocity=1)[:2] == (0, False)                                              # (W = 3: 7 <= 8)
    # the window: 2 W + 1 = N + 1 is refused, 2 W + 1 = N - 1 taken
    rc, untouched, msg = call(use_velocity=1, velocity_scale=-3.1 / 2.9, extra=True)
    assert rc == 3 and untouched and b"window" in msg and field_call(use_velocity=1, velocity_scale=3.1 / 2.9, dst_grid=capi.GRID_XH) == (3, True)
    # 3: the other arguments
    for kw in (dict(kind=-1), dict(kind=4), dict(scale=np.nan), dict(t_gamma=np.inf), dict(t_gamma=-1.0), dict(los_axis=-1), dict(los_axis=3),
               dict(use_velocity=1, velocity_scale=np.nan), dict(mode=-1), dict(mode=2), dict(n_a=0), dict(n_b=0), dict(n_a=-3),
               dict(n_a=1025, n_b=1), dict(n_a=513, n_b=2), dict(thr_a=(0, 4, 9, 16)), dict(thr_a=(1, 9, 4, 16)), dict(thr_b=(0.0, 0.6, 0.5)),
               dict(thr_b=(0.0, np.nan, 2.0)), dict(thr_b=(-np.inf, 0.5, 2.0)), dict(null=("thr_a",)), dict(null=("thr_b",)),
               dict(null=("count",)), dict(null=("sum_1",)), dict(null=("sum_2",)), dict(null=("sum_aa",)), dict(null=("sum_l2",)),
               dict(null=("sum_l4",)), dict(null=("moments_real",)), dict(null=("moments_rs",))):
        rc, untouched, msg = call(extra=True, **kw)
        assert rc == 3 and untouched and b"power_spectrum_los" in msg, kw
    for kw in (dict(kind=7), dict(los_axis=4), dict(dst_grid=-2), dict(dst_grid=9), dict(scale=np.inf)):
        assert field_call(**{"dst_grid": capi.GRID_XH, **kw}) == (3, True), kw
    # ... on the device neither: the grid a refused call named as its target is what it was, and no other grid has come to be
    assert np.array_equal(lib.grid_to_host(capi.GRID_XH, np.empty((N, N, N))), x)
    with pytest.raises(RuntimeError, match="holds no data"):
        lib.grid_to_host(capi.GRID_XH_AV, np.empty((N, N, N)))
    # accepted: thr_a[0] = 0 in the cylindrical mode; equal thresholds are empty bins; the stage times under the timing option
    assert call(mode=capi.ANISO_CYLINDRICAL, thr_a=(0, 4, 4, 16))[0] == 0 and call(thr_b=(0.5, 0.5, 2.0))[0] == 0
    got = lib.power_spectrum_los(capi.PS_XH, 1.0, 0.0, 0, None, capi.ANISO_CYLINDRICAL, [0, 4, 4, 16], [0.0, 1.0, 1.0, 17.0])
    assert np.all(got["count"][1] == 0) and np.all(got["count"][:, 1] == 0) and got["count"][0, 0] > 0 and got["sum_aa"][1, 2] == 0.0
    lib.set_option(capi.OPT_TIMING, 1)
    try:
        lib.power_spectrum_los(capi.PS_HI, 1.0, 0.0, 1, 1.0, capi.ANISO_MU, [1, 4, 9, 16], [0.0, 2.0])
        ms = lib.power_spectrum_los_ms()
        print(f"stage times at N {N}: {ms.tolist()} ms")
        assert ms.shape == (6,) and np.all(ms >= 0.0) and np.all(ms > 0.0)
        lib.power_spectrum_los(capi.PS_XH, 1.0, 0.0, 1, None, capi.ANISO_MU, [1, 4, 9, 16], [0.0, 2.0])
        ms = lib.power_spectrum_los_ms()
        assert np.all(ms[2:] > 0.0)
    finally:
        lib.set_option(capi.OPT_TIMING, 0)
    lib.los_velocity_clear()
    assert call(use_velocity=1)[:2] == (3, True)
    # the spec of the package refuses N > 645 (no device could be asked: the mesh of device_init is the limit's own)
    from pyc2ray_amd.redshift_space import redshift_space_spec
    with pytest.raises(ValueError, match="the mesh must have 1 ... 645 cells a side"):
        redshift_space_spec("power_spectrum_los", 646)


def test_the_kaiser_factor_on_the_device(asora):
    """The N = 32 field of tests/test_redshift_space_reference.py on the device: the mapped field is the reference's bit for bit,
    and P2 / P0 of every bin of k agrees with the reference's within the bound of the sums, propagated: with S0, S2 the two sums of a
    bin and b their common bound, |S2 / S0 - S2' / S0'| <= b (1 + |S2 / S0|) / (S0 - b)."""
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    N = 32
    _mesh(asora, N)
    delta, u = RR.kaiser_field(N, 5)
    c = PR.c_of_N(N)
    for axis in (0, 1, 2):
        sp = pc2r.power_spectrum_los(1.0 + delta, velocity=u[axis], los_axis=axis, binning="multipoles", bins=8, return_field=True)
        again = pc2r.power_spectrum_los(1.0 + delta, velocity=u[axis], los_axis=axis, binning="multipoles", bins=8, return_field=True)
        for key in ("n_modes", "sum_1", "sum_2", "sum_aa", "sum_l2", "sum_l4", "moments_real", "moments_rs", "field"):
            assert getattr(sp, key).tobytes() == getattr(again, key).tobytes(), key
        h = RR.map_lines(1.0 + delta, u[axis], 1.0, axis)
        assert sp.field.tobytes() == h.tobytes()
        assert RR.kaiser_deviation(N, axis, delta, sp.field) < 0.02
        from pyc2ray_amd.powerspec import _edges_to_thresholds
        want = RR.binned(N, axis, RR.MU, _edges_to_thresholds(sp.edges_a), np.array([0.0, 2.0]), np.fft.rfftn(h))
        s0, s2 = want["sum_aa"][:, 0], want["sum_l2"][:, 0]
        b = 4.0 * c * np.sqrt(s0 * want["total_aa"])
        ratio, ratio_ref = sp.P2 / sp.P0, 5.0 * s2 / s0
        bound = 5.0 * b * (1.0 + np.abs(s2 / s0)) / (s0 - b)
        print(f"axis {axis}: P2 / P0 = {np.round(ratio, 4).tolist()}, off the reference's by {float(np.max(np.abs(ratio - ratio_ref) / bound)):.3e} of the bound")
        assert np.all(np.abs(ratio - ratio_ref) <= bound)
        # linear theory with f = 1: P2 / P0 = (4/3 + 4/7) / (1 + 2/3 + 1/5) = 1.0204, within the scatter of a white field's 1400 to
        # 4700 modes per bin (the reference's own ratios there lie between 0.84 and 1.07)
        assert np.all(np.abs(ratio[3:7] - 1.0204) < 0.25)
        assert abs(sp.mean_rs - sp.mean_real) <= 1e-13 and sp.variance_rs > sp.variance_real


def test_class(asora, tmp_path):
    """A run at N = 16 with the redshift-space keys: a step on the resident path with a velocity assigned leaves its multipoles and
    one line in the log, and nothing is fetched; the spectrum equals the module-level call on the downloaded grids; the mapped cube
    written into a grid is there for the analyses of a grid."""
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N, dt = 16, 3.15576e13
        with open("src.txt", "w") as f:
            f.write("1\n8 8 8 5e50 1.0\n")
        if p.cuda_is_init():
            p.device_close()
        sim = pc2r.C2Ray_Test(RS_PARAMS, N, True)
        assert sim.device_resident and sim.redshift_space_stats is True and sim.last_redshift_space is None and sim.los_axis == 1
        sim.density_init(0.0)
        srcpos, srcflux = sim.read_sources("src.txt", 1)
        rng = np.random.default_rng(12)
        v = rng.normal(size=(N, N, N)) * 1.5 / sim.velocity_scale()          # km/s: a displacement of 1.5 cells rms
        v = np.clip(v, -6.5 / sim.velocity_scale(), 6.5 / sim.velocity_scale())
        sim.los_velocity = v
        sim.evolve3D(dt, srcflux, srcpos)
        first = sim.last_redshift_space
        assert first is not None and first.velocity and (first.binning, first.kind, first.los_axis, first.N) == ("multipoles", "dtb", 1, N)
        assert sim._device_newer >= {"xh", "phi_ion"}             # nothing was fetched
        from pyc2ray_amd.c2ray_base import Mpc
        box = sim.boxsize_c / Mpc
        head = f"Redshift-space spectrum (dtb, multipoles, 4 x 1 bins, line of sight 1, redshift space, L = {box:g} units of box_len): "
        assert open(sim.logfile).read().count(head) == 1
        assert first.variance_rs > 0 and first.variance_real > 0 and abs(first.mean_rs - first.mean_real) <= 1e-12 * abs(first.mean_real)
        again = sim.power_spectrum_los()
        mu = sim.power_spectrum_los(binning="mu", bins=3, mu_bins=4, return_field=True)
        other = sim.power_spectrum_los(los_axis=2)
        assert sim._device_newer >= {"xh", "phi_ion"}
        for key in ("n_modes", "sum_1", "sum_aa", "sum_l2", "sum_l4", "moments_rs"):
            assert getattr(again, key).tobytes() == getattr(first, key).tobytes(), key
        assert other.los_axis == 2 and other.sum_l2.tobytes() != first.sum_l2.tobytes()
        # the downloaded grids: the reference's mapping of the reference's field, and the module-level call on them
        scale, vscale = sim.brightness_temperature_scale(), sim.velocity_scale()
        x, n = sim.xh.copy(), np.array(sim.ndens, dtype=np.float64)
        g = PR.form_field(PR.HI, x, n, None, scale, 0.0)
        assert np.all(np.abs(mu.field - RR.map_lines(g, v, vscale, 1)) <= 256.0 * PR.EPS * np.max(np.abs(g)))
        for which, grid in ((capi.GRID_XH, x), (capi.GRID_NDENS, n)):
            lib.grid_to_device(which, grid)
        m = pc2r.power_spectrum_los(None, velocity=v, velocity_scale=vscale, los_axis=1, binning="mu", bins=3, mu_bins=4, kind="dtb", scale=scale,
                                    box_len=box, return_field=True)
        for key in ("n_modes", "sum_1", "sum_2", "sum_aa", "sum_l2", "sum_l4", "moments_real", "moments_rs", "field"):
            assert getattr(m, key).tobytes() == getattr(mu, key).tobytes(), key
        # the mapped cube, and the same into a grid, where the analyses of a grid take it
        cube = sim.redshift_space_field()
        assert cube.tobytes() == mu.field.tobytes()
        assert sim.redshift_space_field(kind="xh", into=capi.GRID_XH_AV) is None
        mapped_x = lib.grid_to_host(capi.GRID_XH_AV, np.empty((N, N, N)))
        assert mapped_x.tobytes() == RR.map_lines(x, v, vscale, 1).tobytes()
        sizes = pc2r.mfp_distribution(None, grid=capi.GRID_XH_AV, n_rays=2000, threshold=0.5)
        assert sizes.log_line().startswith("Bubble sizes (")
        # no velocity: the real-space spectrum, and the line says so
        sim.los_velocity = None
        sim.evolve3D(dt, srcflux, srcpos)
        assert sim.last_redshift_space is not first and not sim.last_redshift_space.velocity
        assert open(sim.logfile).read().count("line of sight 1, real space: no velocity, ") == 1
        assert sim.last_redshift_space.moments_rs.tobytes() == sim.last_redshift_space.moments_real.tobytes()
    finally:
        if p.cuda_is_init():
            p.device_close()
        os.chdir(cwd)
