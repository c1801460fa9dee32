"""GPU: the power spectrum (asora_power_spectrum, power_spectrum, C2Ray.power_spectrum) against its numpy
statement, tests/powerspec_reference.py.  Every call is made twice and compared byte for byte.

The tolerances are derived, not tuned.  c(N) = 8 eps (log2 N^3 + p), p the largest prime factor of N beyond 7, bounds the relative
error of the transform in the 2-norm (the backward-error bound of a mixed-radix FFT whose generic butterfly sums p terms, with
head room 8; numpy itself stays 5 to 25 times inside it against an 80-bit transform).  For a bin's power sum S_b, Cauchy-Schwarz on
that bound gives |S_b - S_b^ref| <= 4 c(N) sqrt(S_b^ref S_tot), S_tot the weighted power of every mode but n = 0; for a cross sum
the same argument on a conj(b) gives 4 c(N) (sqrt(S_aa,b T_bb) + sqrt(S_bb,b T_aa)).  Where the exact answer of a bin is 0 (a
constant field at a mesh with a radix that is not exact on it, the bins beside a cosine's), the same bound is taken around the
whole spectrum's norm, which the error of the transform is relative to: sqrt(S_b) <= sqrt(2) c(N) ||ghat||, so S_b <= 2 c(N)^2
||ghat||^2, ||ghat||^2 = N^3 sum g^2.

* Transform meshes: every specialised radix alone (2, 3, 4, 5, 7), the generic butterfly (17, 43, 129 = 3 x 43), repeated and
  mixed radices, odd and even N, tail tiles of the strided passes (N / 2 + 1 no multiple of the tile), several lines per workgroup
  and several trips of the mean-density sum; N = 250 and 280 with the binned sums only.
* The meshes of tests/fft_meshes.py (121, 139, 140, 169, 243, 256, 271, 272, 273; each row says what it is there for, and
  tests/test_fft_meshes_host.py checks that it is so): the generic stage twice in one plan, five stages, primes up to 271, both
  edges of the tile rule (139 | 140, 271 | 272), tail tiles and a tail row workgroup at 16, 8 and 4 lines per workgroup, and
  256^3 -- the modes against numpy, the sums, Parseval, the moments.  At 169 (two trips of the binning's loop over n_z) the cross
  form with two different fields and both forms with 256 bins; 121 and 273 form every kind of field (uneven trips of the
  mean-density sum)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import fft_meshes as FM
import powerspec_reference as PR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POWER_PARAMS = os.path.join(HERE, "data", "parameters_power_spectrum.yml")
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_single_black_body.yml")
MESHES = (2, 3, 4, 5, 7, 8, 9, 16, 17, 30, 43, 49, 64, 96, 129, 136)      # (N = 1: test_a_single_cell_is_no_mesh_of_the_library)
KEYS = ("count", "sum_k", "sum_aa", "sum_bb", "sum_ab", "moments_a", "moments_b", "field", "modes")


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
    got, again = lib.power_spectrum(*args, **kw), lib.power_spectrum(*args, **kw)
    for key in KEYS:
        assert (got[key] is None) == (again[key] is None), key
        if got[key] is not None:
            assert got[key].tobytes() == again[key].tobytes(), key
    assert got["count"].dtype == np.uint64
    return got


def _bin_sets(N):
    """default bins; integer edges (modes on the edges); a last edge that cuts off the corners of a coarse set; one bin with all"""
    h = max(N // 2, 1)
    return {"default": np.arange(0, min(h, 256) + 1) + 0.5,
            "integer": np.arange(1, h + 2, dtype=np.float64),
            "cut": np.array([0.5, 0.5 + h / 3.0, 0.5 + h / 1.5, float(h)]) if h >= 3 else np.array([0.5, float(h) + 0.25]),
            "all": np.array([0.5, np.sqrt(3.0) * h + 1.0])}


def _check_sums(N, got, want, what):
    c = PR.c_of_N(N)
    assert np.array_equal(got["count"], want["count"]), (what, got["count"].tolist(), want["count"].tolist())
    err_k = np.abs(got["sum_k"] - want["sum_k"])
    assert np.all(err_k <= 1e-13 * want["sum_k"]), (what, "sum_k", float(err_k.max()))
    bound = 4.0 * c * np.sqrt(want["sum_aa"] * want["total_aa"])
    err = np.abs(got["sum_aa"] - want["sum_aa"])
    used = float(np.max(err / np.where(bound > 0, bound, 1.0))) if err.size else 0.0
    print(f"{what}: {len(err)} bins, sum_aa uses {used:.3e} of its bound")
    assert np.all(err <= bound), (what, "sum_aa", err.tolist(), bound.tolist())


@pytest.mark.parametrize("N", MESHES)
def test_transform_sums_and_parseval(asora, N, only=None):
    p, lib, capi = asora
    _mesh(asora, N)
    field = PR.noise_with_block(N, 1000 + N)
    lib.grid_to_device(capi.GRID_XH, field)
    c = PR.c_of_N(N)
    sets = {name: edges for name, edges in _bin_sets(N).items() if only is None or name in only}
    got = _twice(lib, capi.PS_XH, None, 1.0, 0.0, PR.thresholds_of(sets["default"]), field=True, modes=True)
    # 6. the formed field of kind xh is the grid, bit for bit; 1. its transform against numpy's of the downloaded field
    assert got["field"].tobytes() == field.tobytes() and got["modes"].shape == (N, N, N // 2 + 1)
    ref = np.fft.rfftn(got["field"])
    err = np.linalg.norm((got["modes"] - ref).ravel()) / np.linalg.norm(ref.ravel())
    print(f"N {N}: transform error {err:.3e}, c(N) {c:.3e} ({err / c:.3f} of it)")
    assert err <= c
    # 2. the binned sums
    for name, edges in sets.items():
        thr = PR.thresholds_of(edges)
        mine = got if name == "default" else _twice(lib, capi.PS_XH, None, 1.0, 0.0, thr)
        want = PR.binned(N, thr, ref)
        _check_sums(N, mine, want, f"N {N}, bins {name}")
        if name == "default":
            plain = lib.power_spectrum(capi.PS_XH, None, 1.0, 0.0, thr)       # the downloads change nothing
            for key in ("count", "sum_k", "sum_aa", "moments_a"):
                assert plain[key].tobytes() == got[key].tobytes()
        if name == "all":
            # 3. Parseval: the bin holds every mode but n = 0
            assert mine["count"].tolist() == [N ** 3 - 1]
            m = mine["moments_a"]
            spread = m[1] - m[0] ** 2 / N ** 3
            power = mine["sum_aa"][0] / N ** 3
            if N == 1:
                assert power == 0.0
            else:
                print(f"N {N}: Parseval residual {abs(power - spread) / spread:.3e}, bound {4 * c:.3e}")
                assert abs(power - spread) <= 4.0 * c * spread
    want_m = np.array([float(PR.exact_sum(field)), float(PR.exact_sum(field * field))])
    assert np.all(np.abs(got["moments_a"] - want_m) <= 1e-13 * np.abs(want_m)), (got["moments_a"].tolist(), want_m.tolist())


@pytest.mark.parametrize("N", FM.MESHES)
def test_transform_at_the_meshes_of_the_table(asora, N):
    """The same assertions at the meshes of tests/fft_meshes.py: two generic stages, five stages, primes beyond a workgroup's work
    items, both edges of the tile rule, tails at 8 and at 4 lines per workgroup, 256^3.  From N = 243 on the `default` and `all` bin
    sets only (numpy's transform and the reference's binning take a second each there)."""
    test_transform_sums_and_parseval(asora, N, only=("default", "all") if N >= FM.FEW_BIN_SETS_FROM else None)


def test_a_single_cell_is_no_mesh_of_the_library(asora):
    """N = 1 has a transform (the cell itself) and the kernels take it, but device_init refuses meshes below 2 cells a side, so no
    call can reach them: that refusal is what there is to test."""
    p, lib, capi = asora
    if p.cuda_is_init():
        p.device_close()
    with pytest.raises(RuntimeError, match="N must be in"):
        p.device_init(1, 8)
    assert not p.cuda_is_init()


@pytest.mark.parametrize("N", [250, 280])
def test_large_mesh_binned_sums(asora, N):
    """N = 250 = 2 x 5^3, the published protocol's mesh (8 lines per workgroup), and N = 280 = 2^3 x 5 x 7, at which a workgroup
    takes 4 lines, the tile of every mesh beyond 271: the binned sums only"""
    p, lib, capi = asora
    _mesh(asora, N)
    field = PR.noise_with_block(N, 1000 + N)
    lib.grid_to_device(capi.GRID_XH, field)
    thr = PR.thresholds_of(np.arange(0, N // 2 + 1) + 0.5)
    got = _twice(lib, capi.PS_XH, None, 1.0, 0.0, thr)
    _check_sums(N, got, PR.binned(N, thr, np.fft.rfftn(field)), f"N {N}")


@pytest.mark.parametrize("N", [16, 15])
def test_known_answers(asora, N):
    p, lib, capi = asora
    _mesh(asora, N)
    c = PR.c_of_N(N)
    sets = _bin_sets(N)
    thr = PR.thresholds_of(sets["integer"])
    # a constant field: no power beside n = 0
    const = np.full((N, N, N), 0.375)
    lib.grid_to_device(capi.GRID_XH, const)
    got = _twice(lib, capi.PS_XH, None, 1.0, 0.0, thr)
    want = PR.power_sums(const, thr)
    if N == 16:          # radices 4 and 2 are exact on it: the bound of the binned sums around the reference's (its own are 0 too)
        assert np.all(np.abs(got["sum_aa"] - want["sum_aa"]) <= 4.0 * c * np.sqrt(want["sum_aa"] * want["total_aa"]))
    norm2 = N ** 3 * float(np.sum(const * const))
    print(f"N {N}: constant field, largest power sum {got['sum_aa'].max():.3e}, bound {2 * c * c * norm2:.3e}")
    assert np.all(got["sum_aa"] <= 2.0 * c * c * norm2) and np.array_equal(got["count"], want["count"])
    assert got["moments_a"].tolist() == [0.375 * N ** 3, 0.375 ** 2 * N ** 3]
    # a single cosine along a: all its power, N^6 / 2, in the bin of |a|
    idx = np.arange(N)
    for a in ((1, 2, 2), (3, 0, 0), (0, 2, 0), (2, N - 1, 0), (N - 3, 1, N - 2)):
        phase = (a[0] * idx[:, None, None] + a[1] * idx[None, :, None] + a[2] * idx[None, None, :]) % N
        lib.grid_to_device(capi.GRID_XH, np.cos(2.0 * np.pi * phase / N))
        got = _twice(lib, capi.PS_XH, None, 1.0, 0.0, thr)
        m = [min(v, N - v) for v in a]
        n2 = sum(v * v for v in m)
        peak = int(np.searchsorted(thr, n2, side="right")) - 1
        assert 0 <= peak < len(thr) - 1
        total = float(N) ** 6 / 2
        others = np.delete(got["sum_aa"], peak)
        print(f"N {N}, cosine {a}: peak off by {abs(got['sum_aa'][peak] - total) / total:.3e} (bound {4 * c:.3e}), beside it {others.max():.3e}")
        assert abs(got["sum_aa"][peak] - total) <= 4.0 * c * total
        assert np.all(others <= 2.0 * c * c * total)
    # a single cell set to 1: |ghat| = 1 everywhere
    one = np.zeros((N, N, N))
    one[3, N - 2, 5] = 1.0
    lib.grid_to_device(capi.GRID_XH, one)
    for edges in sets.values():
        got = _twice(lib, capi.PS_XH, None, 1.0, 0.0, PR.thresholds_of(edges))
        count = got["count"].astype(np.float64)
        assert np.all(np.abs(got["sum_aa"] - count) <= c * count) and got["moments_a"].tolist() == [1.0, 1.0]


def test_cross_spectra(asora):
    p, lib, capi = asora
    N = 30
    _mesh(asora, N)
    c = PR.c_of_N(N)
    rng = np.random.default_rng(77)
    x = rng.random((N, N, N))
    n = 1e-4 * np.exp(0.5 * rng.normal(size=(N, N, N)))
    lib.grid_to_device(capi.GRID_XH, x)
    lib.grid_to_device(capi.GRID_NDENS, n)
    thr = PR.thresholds_of(_bin_sets(N)["default"])
    same = _twice(lib, capi.PS_XH, capi.PS_XH, 1.0, 0.0, thr)
    assert same["sum_ab"].tobytes() == same["sum_aa"].tobytes() == same["sum_bb"].tobytes()
    assert same["moments_a"].tobytes() == same["moments_b"].tobytes()
    auto = _twice(lib, capi.PS_XH, None, 1.0, 0.0, thr)
    assert auto["sum_aa"].tobytes() == same["sum_aa"].tobytes() and auto["sum_bb"] is None and auto["sum_ab"] is None
    want = PR.power_sums(x, thr, PR.form_field(PR.XHI, x))
    anti = _twice(lib, capi.PS_XH, capi.PS_XHI, 1.0, 0.0, thr)
    bound = 4.0 * c * np.sqrt(want["sum_aa"] * want["total_aa"])
    assert np.all(np.abs(anti["sum_ab"] + anti["sum_aa"]) <= 2.0 * bound)
    assert np.all(np.abs(anti["sum_bb"] - want["sum_bb"]) <= 4.0 * c * np.sqrt(want["sum_bb"] * want["total_bb"]))
    # two different fields, both ways round
    ab = _twice(lib, capi.PS_XH, capi.PS_DENSITY, 1.0, 0.0, thr)
    ba = _twice(lib, capi.PS_DENSITY, capi.PS_XH, 1.0, 0.0, thr)
    assert ab["sum_aa"].tobytes() == ba["sum_bb"].tobytes() and ab["sum_bb"].tobytes() == ba["sum_aa"].tobytes()
    assert ab["sum_ab"].tobytes() == ba["sum_ab"].tobytes() and ab["count"].tobytes() == ba["count"].tobytes()
    assert ab["moments_a"].tobytes() == ba["moments_b"].tobytes() and ab["moments_b"].tobytes() == ba["moments_a"].tobytes()
    dens = PR.form_field(PR.DENSITY, n=n)
    want = PR.power_sums(x, thr, dens)
    for key, tot in (("sum_aa", "total_aa"), ("sum_bb", "total_bb")):
        assert np.all(np.abs(ab[key] - want[key]) <= 4.0 * c * np.sqrt(want[key] * want[tot])), key
    bound = 4.0 * c * (np.sqrt(want["sum_aa"] * want["total_bb"]) + np.sqrt(want["sum_bb"] * want["total_aa"]))
    print(f"cross: sum_ab uses {float(np.max(np.abs(ab['sum_ab'] - want['sum_ab']) / bound)):.3e} of its bound")
    assert np.all(np.abs(ab["sum_ab"] - want["sum_ab"]) <= bound)
    for key in ("moments_a", "moments_b"):
        assert np.all(np.abs(ab[key] - want[key]) <= 1e-13 * np.abs(want[key])), key


N_TRIPS = 169         # NZ = 85: the binning's loop over n_z makes two trips, 21 lanes in the second (tests/fft_meshes.py)


@functools.lru_cache(maxsize=1)
def _two_fields():
    """x, n and numpy's transforms of x, 1 - x and n / nbar at N_TRIPS (computed once; treat as read-only)"""
    N = N_TRIPS
    rng = np.random.default_rng(78)
    x = rng.random((N, N, N))
    n = 1e-4 * np.exp(0.5 * rng.normal(size=(N, N, N)))
    xi, dens = PR.form_field(PR.XHI, x), PR.form_field(PR.DENSITY, n=n)
    moments = {name: np.array([float(PR.exact_sum(g)), float(PR.exact_sum(g * g))]) for name, g in (("x", x), ("xi", xi), ("dens", dens))}
    return dict(x=x, n=n, xhat=np.fft.rfftn(x), xihat=np.fft.rfftn(xi), denshat=np.fft.rfftn(dens), moments=moments)


def _upload_two_fields(asora):
    p, lib, capi = asora
    f = _two_fields()
    _mesh(asora, N_TRIPS)
    lib.grid_to_device(capi.GRID_XH, f["x"])
    lib.grid_to_device(capi.GRID_NDENS, f["n"])
    return f


def _check_cross_sums(N, got, want, what):
    """count and sum_k of _check_sums, and the three bounds of test_cross_spectra"""
    c = PR.c_of_N(N)
    _check_sums(N, got, want, what)
    err = np.abs(got["sum_bb"] - want["sum_bb"])
    assert np.all(err <= 4.0 * c * np.sqrt(want["sum_bb"] * want["total_bb"])), (what, "sum_bb")
    bound = 4.0 * c * (np.sqrt(want["sum_aa"] * want["total_bb"]) + np.sqrt(want["sum_bb"] * want["total_aa"]))
    err = np.abs(got["sum_ab"] - want["sum_ab"])
    print(f"{what}: sum_ab uses {float(np.max(err / np.where(bound > 0, bound, 1.0))):.3e} of its bound")
    assert np.all(err <= bound), (what, "sum_ab")


def test_the_bin_limit(asora):
    """n_bins = 256, all the ABI allows (the cross form then asks for 42 KB of LDS for its four histograms), at a mesh with two trips
    of the loop over n_z.  The 257 thresholds are values of |n|^2 that occur on the mesh, so every bin holds modes, but for two pairs
    of equal neighbours: two bins that are empty on purpose.  Modes below the first and at or above the last threshold are dropped."""
    p, lib, capi = asora
    N = N_TRIPS
    n2 = PR.mode_n2(N)
    q = np.unique(n2)
    assert q[0] == 0 and q[1] == 1 and q[-1] == 3 * (N // 2) ** 2
    pick = q[np.linspace(4, q.size - 40, 255).astype(int)]
    thr = np.insert(pick, [40, 200], pick[[40, 200]]).astype(np.uint32)
    f = _two_fields()
    want = PR.binned(N, thr, f["xhat"], f["denshat"])
    # the conditions, on the reference alone
    assert thr.size == 257 and np.all(np.diff(thr.astype(np.int64)) >= 0) and 1 < thr[0] and thr[-1] < 3 * (N // 2) ** 2
    assert int(np.sum(np.diff(thr.astype(np.int64)) == 0)) == 2
    assert int(np.sum(want["count"] == 0)) == 2 and want["count"][40] == 0 and want["count"][201] == 0
    w = np.broadcast_to(PR.mode_weights(N)[None, None, :], n2.shape)
    below, above = int(w[(n2 >= 1) & (n2 < thr[0])].sum()), int(w[n2 >= thr[-1]].sum())
    assert below > 0 and above > 0 and int(want["count"].sum()) + below + above == N ** 3 - 1
    print(f"N {N}, 256 bins: {below} modes dropped below the first threshold, {above} at or above the last")
    _upload_two_fields(asora)
    auto = _twice(lib, capi.PS_XH, None, 1.0, 0.0, thr)
    _check_sums(N, auto, want, f"N {N}, 256 bins")
    assert auto["sum_aa"][40] == 0.0 and auto["sum_aa"][201] == 0.0 and auto["sum_k"][40] == 0.0
    cross = _twice(lib, capi.PS_XH, capi.PS_DENSITY, 1.0, 0.0, thr)
    _check_cross_sums(N, cross, want, f"N {N}, 256 bins, cross")
    for key in ("count", "sum_k", "sum_aa", "moments_a"):
        assert cross[key].tobytes() == auto[key].tobytes(), key
    for key in ("sum_aa", "sum_bb", "sum_ab"):
        assert cross[key][40] == 0.0 and cross[key][201] == 0.0, key


def test_cross_spectra_across_trips(asora):
    """test_cross_spectra's two different fields where a row of the second field, too, takes a second, partly filled trip of the loop
    over n_z (NZ = 85); the density's mean is summed over 36.8 trips of the fixed grid."""
    p, lib, capi = asora
    N = N_TRIPS
    f = _upload_two_fields(asora)
    c = PR.c_of_N(N)
    thr = PR.thresholds_of(_bin_sets(N)["default"])
    ab = _twice(lib, capi.PS_XH, capi.PS_DENSITY, 1.0, 0.0, thr)
    ba = _twice(lib, capi.PS_DENSITY, capi.PS_XH, 1.0, 0.0, thr)
    assert ab["sum_aa"].tobytes() == ba["sum_bb"].tobytes() and ab["sum_bb"].tobytes() == ba["sum_aa"].tobytes()
    assert ab["sum_ab"].tobytes() == ba["sum_ab"].tobytes() and ab["count"].tobytes() == ba["count"].tobytes()
    assert ab["sum_k"].tobytes() == ba["sum_k"].tobytes()
    assert ab["moments_a"].tobytes() == ba["moments_b"].tobytes() and ab["moments_b"].tobytes() == ba["moments_a"].tobytes()
    want = PR.binned(N, thr, f["xhat"], f["denshat"])
    _check_cross_sums(N, ab, want, f"N {N}, xh x density")
    for key, name in (("moments_a", "x"), ("moments_b", "dens")):
        assert np.all(np.abs(ab[key] - f["moments"][name]) <= 1e-13 * np.abs(f["moments"][name])), key
    # a field against 1 - itself: every binned mode of the second is minus the first's
    anti = _twice(lib, capi.PS_XH, capi.PS_XHI, 1.0, 0.0, thr)
    want = PR.binned(N, thr, f["xhat"], f["xihat"])
    bound = 4.0 * c * np.sqrt(want["sum_aa"] * want["total_aa"])
    err = np.abs(anti["sum_ab"] + anti["sum_aa"])
    print(f"N {N}, xh x xhi: sum_ab + sum_aa uses {float(np.max(err / (2.0 * bound))):.3e} of its bound")
    assert np.all(err <= 2.0 * bound)
    _check_cross_sums(N, anti, want, f"N {N}, xh x xhi")
    assert anti["sum_aa"].tobytes() == ab["sum_aa"].tobytes()
    assert np.all(np.abs(anti["moments_b"] - f["moments"]["xi"]) <= 1e-13 * np.abs(f["moments"]["xi"]))


@pytest.mark.parametrize("N", [17, 64, 121, 273])
def test_forming_the_field(asora, N):
    """(121 and 273: uneven trips of the mean-density sum, 13.5 and 155.2, and a last row workgroup with one line at 16 and at 4
    lines per workgroup.  At 273 three kinds, so that the case stays within seconds: 'xhi', 'density' and 'hi' with t_gamma, one
    of each arithmetic form of the cell -- 'xh' is a copy, which the transform test asserts bit for bit at that mesh -- and the
    binned sums of the two that divide by the mean density)"""
    p, lib, capi = asora
    _mesh(asora, N)
    rng = np.random.default_rng(300 + N)
    x = rng.random((N, N, N))
    n = 1e-4 * np.exp(0.7 * rng.normal(size=(N, N, N)))
    T = 200.0 + 2e4 * rng.random((N, N, N))                  # (far from t_gamma: 1 - t_gamma / T loses no digits)
    for which, grid in ((capi.GRID_XH, x), (capi.GRID_NDENS, n), (capi.GRID_TEMP, T)):
        lib.grid_to_device(which, grid)
    thr = PR.thresholds_of(_bin_sets(N)["default"])
    kinds = ((capi.PS_XH, 1.0, 0.0), (capi.PS_XHI, 1.0, 0.0), (capi.PS_DENSITY, 1.0, 0.0), (capi.PS_HI, 1.0, 0.0),
             (capi.PS_HI, 27.3, 0.0), (capi.PS_HI, 27.3, 30.0), (capi.PS_XHI, 5.0, 30.0))
    binned_kinds = kinds
    if N >= FM.FEW_BIN_SETS_FROM:
        kinds, binned_kinds = (kinds[1], kinds[2], kinds[5]), (kinds[2], kinds[5])
    for kind, scale, t_gamma in kinds:
        got = _twice(lib, kind, None, scale, t_gamma, thr, field=True)
        hi = kind == capi.PS_HI
        want = PR.form_field(kind, x, n, T, scale if hi else 1.0, t_gamma if hi else 0.0)     # (scale and t_gamma are for 'hi' alone)
        err = float(np.max(np.abs(got["field"] - want) / np.abs(want)))
        print(f"N {N}, kind {kind}, scale {scale}, t_gamma {t_gamma}: field off by {err / PR.EPS:.2f} eps")
        assert err <= 4.0 * PR.EPS
        if kind in (capi.PS_XH, capi.PS_XHI):
            assert np.array_equal(got["field"], want)
        want_m = np.array([float(PR.exact_sum(got["field"])), float(PR.exact_sum(got["field"] ** 2))])
        assert np.all(np.abs(got["moments_a"] - want_m) <= 1e-13 * np.abs(want_m))
        if (kind, scale, t_gamma) in binned_kinds:
            _check_sums(N, got, PR.binned(N, thr, np.fft.rfftn(got["field"])), f"N {N}, kind {kind}")
    # no grid is written
    for which, grid in ((capi.GRID_XH, x), (capi.GRID_NDENS, n), (capi.GRID_TEMP, T)):
        assert np.array_equal(lib.grid_to_host(which, np.empty((N, N, N))), grid)


def test_refusals_leave_the_outputs_untouched(asora):
    p, lib, capi = asora
    raw = capi.load()
    N, nb = 8, 3
    SENT = 12345.0

    def call(kind_a=capi.PS_XH, kind_b=-1, scale=1.0, t_gamma=0.0, n_bins=nb, thr=(1, 4, 9, 16), null=(), extra=False):
        thr = np.array(thr, dtype=np.uint32)
        out = dict(count=np.full(nb, 12345, dtype=np.uint64), sum_k=np.full(nb, SENT), sum_aa=np.full(nb, SENT), sum_bb=np.full(nb, SENT),
                   sum_ab=np.full(nb, SENT), moments_a=np.full(2, SENT), moments_b=np.full(2, SENT), field=np.full(N ** 3, SENT),
                   modes=np.full(2 * N * N * (N // 2 + 1), SENT))
        ptr = lambda name: None if name in null else (out[name].ctypes.data_as(capi._u64p) if name == "count" else capi.dptr(out[name]))
        rc = raw.asora_power_spectrum(kind_a, kind_b, scale, t_gamma, n_bins,
                                      None if "thresholds" in null else thr.ctypes.data_as(C.POINTER(C.c_uint32)), ptr("count"), ptr("sum_k"),
                                      ptr("sum_aa"), ptr("sum_bb"), ptr("sum_ab"), ptr("moments_a"), ptr("moments_b"),
                                      ptr("field") if extra else None, ptr("modes") if extra else None)
        untouched = all(np.all(v == 12345) for v in out.values())
        return rc, untouched, raw.asora_last_error() or b""

    if p.cuda_is_init():
        p.device_close()
    rc, untouched, msg = call()
    assert rc == 2 and untouched and b"power_spectrum" in msg
    p.device_init(N, 8)
    # 4: a grid the kinds need holds no data
    assert call(extra=True)[:2] == (4, True)
    lib.grid_to_device(capi.GRID_XH, np.random.default_rng(1).random((N, N, N)))
    assert call(kind_a=capi.PS_DENSITY)[:2] == (4, True) and call(kind_a=capi.PS_HI)[:2] == (4, True)
    assert call(kind_b=capi.PS_DENSITY)[:2] == (4, True)
    lib.grid_to_device(capi.GRID_NDENS, np.full((N, N, N), 2.0))
    rc, untouched, msg = call(kind_a=capi.PS_HI, t_gamma=30.0, extra=True)
    assert rc == 4 and untouched and b"holds no data" in msg
    # 3: the arguments
    for kw in (dict(kind_a=-1), dict(kind_a=4), dict(kind_b=-2), dict(kind_b=4), dict(scale=np.nan), dict(scale=np.inf), dict(t_gamma=np.nan),
               dict(t_gamma=np.inf), dict(t_gamma=-1.0), dict(n_bins=0), dict(n_bins=-1), dict(n_bins=257), dict(thr=(0, 4, 9, 16)),
               dict(thr=(1, 9, 4, 16)), dict(thr=(1, 4, 9, 8)), dict(null=("thresholds",)), dict(null=("count",)), dict(null=("sum_k",)),
               dict(null=("sum_aa",)), dict(null=("moments_a",)), dict(kind_b=capi.PS_XHI, null=("sum_bb",)),
               dict(kind_b=capi.PS_XHI, null=("sum_ab",)), dict(kind_b=capi.PS_XHI, null=("moments_b",))):
        rc, untouched, msg = call(extra=True, **kw)
        assert rc == 3 and untouched and b"power_spectrum" in msg, kw
    # accepted: the second field's outputs may be NULL without one; equal thresholds are an empty bin; kind 'hi' without t_gamma
    # needs no temperature; the stage times of a call under the timing option
    assert call(null=("sum_bb", "sum_ab", "moments_b"))[:2] == (0, False)
    assert call(thr=(1, 4, 4, 16))[0] == 0 and call(kind_a=capi.PS_HI, kind_b=capi.PS_DENSITY, scale=-3.0)[0] == 0
    got = lib.power_spectrum(capi.PS_XH, None, 1.0, 0.0, [1, 4, 4, 16])
    assert got["count"][1] == 0 and got["sum_aa"][1] == 0.0 and got["count"][0] > 0 and got["count"][2] > 0
    lib.set_option(capi.OPT_TIMING, 1)
    try:
        lib.power_spectrum(capi.PS_HI, capi.PS_DENSITY, 1.0, 0.0, [1, 4, 9, 16])
        ms = lib.power_spectrum_ms()
        print(f"stage times at N {N}: {ms.tolist()} ms")
        assert ms.shape == (5,) and np.all(ms >= 0.0) and np.all(ms[1:] > 0.0)
    finally:
        lib.set_option(capi.OPT_TIMING, 0)


def test_class(asora, tmp_path):
    """The single black-body run at its test mesh with the power-spectrum keys: every step on the resident path leaves its power
    spectrum and one line in the log; power_spectrum() reads the grids where they lie and equals, bit for bit, the module-level
    call on the downloaded grids."""
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
        assert sim.device_resident and sim.power_spectrum_stats is True and sim.last_power_spectrum is None
        sim.density_init(0.0)
        srcpos, srcflux = sim.read_sources("src.txt", 1)
        results = []
        for _ in range(2):
            sim.evolve3D(dt, srcflux, srcpos)
            results.append(sim.last_power_spectrum)
        assert all(r is not None for r in results) and results[0] is not results[1]
        assert sim._device_newer >= {"xh", "phi_ion"}             # nothing was fetched
        last = results[1]
        from pyc2ray_amd.c2ray_base import Mpc
        box = sim.boxsize_c / Mpc
        assert (last.kind, last.kind_b, last.N, last.box_len) == ("dtb", None, N, box) and last.edges.tolist() == np.linspace(0.5, 12.5, 7).tolist()
        assert open(sim.logfile).read().count(f"Power spectrum (dtb, 6 bins to |n| = 12.5, L = {box:g} units of box_len): ") == 2
        assert last.variance > results[0].variance > 0           # one bubble around the source, and it grows
        kw = dict(bins=[1, 2, 3.5, 6], return_field=True)
        kin = sim.power_spectrum(spin="kinetic", kind_b="density", **kw)
        xh_res = sim.power_spectrum(kind="xh", bins=5, box_len=None)
        again = sim.power_spectrum()
        assert sim._device_newer >= {"xh", "phi_ion"}
        for key in ("n_modes", "sum_k", "sum_aa", "moments"):
            assert getattr(again, key).tobytes() == getattr(last, key).tobytes()
        scale, t_gamma = sim.brightness_temperature_scale(), 2.726 * (1 + sim.zred)
        # the downloaded grids: the reference's field, and the module-level call on them
        x, n, T = sim.xh.copy(), np.array(sim.ndens, dtype=np.float64), np.array(sim.temp, dtype=np.float64) * np.ones((N, N, N))
        want = PR.form_field(PR.HI, x, n, T, scale, t_gamma)
        assert np.all(np.abs(kin.field - want) <= 4.0 * PR.EPS * np.abs(want))
        _check_sums(N, dict(count=kin.n_modes, sum_k=kin.sum_k, sum_aa=kin.sum_aa), PR.binned(N, kin.thresholds, np.fft.rfftn(kin.field)), "class")
        m = pc2r.power_spectrum(x, kind="xh", bins=5)
        for key in ("n_modes", "sum_k", "sum_aa", "moments"):
            assert getattr(m, key).tobytes() == getattr(xh_res, key).tobytes(), key
        for which, grid in ((capi.GRID_XH, x), (capi.GRID_NDENS, n), (capi.GRID_TEMP, T)):
            lib.grid_to_device(which, grid)
        m = pc2r.power_spectrum(None, kind="dtb", kind_b="density", scale=scale, t_gamma=t_gamma, box_len=box, **kw)
        for key in ("n_modes", "sum_k", "sum_aa", "sum_bb", "sum_ab", "moments", "moments_b", "field"):
            assert getattr(m, key).tobytes() == getattr(kin, key).tobytes(), key
        m = pc2r.power_spectrum(None, kind="dtb", scale=scale, box_len=box, bins=6)
        for key in ("n_modes", "sum_k", "sum_aa", "moments"):
            assert getattr(m, key).tobytes() == getattr(last, key).tobytes(), key
        fallback = sim.power_spectrum()                            # the host copies are the newer ones now: the upload form
        assert fallback.sum_aa.tobytes() == last.sum_aa.tobytes()
        plain = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        with pytest.raises(ValueError, match="power_spectrum_stats needs use_gpu=True"):
            plain.power_spectrum_stats = True
    finally:
        if p.cuda_is_init():
            p.device_close()
        os.chdir(cwd)
