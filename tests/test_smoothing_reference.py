"""CPU: the numpy statement of asora_smooth_field (tests/smoothing_reference.py) and the filter builders of pyc2ray_amd.smoothing
against answers that owe nothing to a transform: a moving average, constant fields, a delta, a projection, the symmetry of the
tables.  The bound is the GPU tests' own, 2.5 c(N) max|W| ||g||_2 (tests/test_gpu_smoothing.py), which numpy stays far inside."""
import numpy as np
import pytest

import powerspec_reference as PR
import smoothing_reference as SR


def _S():
    import pyc2ray_amd.smoothing as S
    return S


def _filters(S, N):
    return {"telescope": S.telescope(2.5, 3), "gaussian": S.gaussian(3.0), "tophat": S.spherical_tophat(2.0), "sharp_k": S.sharp_k(N / 4),
            "product": S.gaussian(2.0, axes=(0, 2)) * S.spherical_tophat(1.5), "boxcar even": S.boxcar(4, 1), "boxcar real": S.boxcar(2.5, 0),
            "identity": S.Filter()}


def _bound(N, W, g):
    return 2.5 * PR.c_of_N(N) * float(np.max(np.abs(W))) * float(np.linalg.norm(g.ravel()))


@pytest.mark.parametrize("N", [9, 16])
def test_boxcar_of_three_is_the_moving_average(N):
    S = _S()
    g = PR.noise_with_block(N, 40 + N)
    for axis in (0, 1, 2):
        tables = S.boxcar(3, axis).tables(N)
        assert sum(t is not None for t in tables) == 1 and tables[axis] is not None
        h = SR.smooth(g, tables)
        want = SR.moving_average(g, 3, axis)
        err = float(np.linalg.norm((h - want).ravel()))
        assert err <= _bound(N, SR.filter_on_mesh(N, tables), g), (N, axis, err)
    h5 = SR.smooth(g, S.boxcar(5, 2).tables(N))
    assert np.linalg.norm((h5 - SR.moving_average(g, 5, 2)).ravel()) <= _bound(N, np.ones(1), g)


@pytest.mark.parametrize("N", [8, 9, 30])
def test_constant_fields_deltas_projections_and_symmetry(N):
    S = _S()
    const = np.full((N, N, N), 0.375)
    delta = np.zeros((N, N, N))
    delta[1, N - 1, 2] = 1.0
    g = PR.noise_with_block(N, 7 + N)
    for name, f in _filters(S, N).items():
        tables = f.tables(N)
        W = SR.filter_on_mesh(N, tables)
        assert W[0, 0, 0] == 1.0, name                                       # every filter is 1 at n = 0 ...
        assert np.array_equal(W, f.on_mesh(N)), name
        # ... so it maps a constant field to itself and, with subtract_mean, to 0
        tol = _bound(N, W, const)
        assert np.linalg.norm((SR.smooth(const, tables) - const).ravel()) <= tol, name
        assert np.linalg.norm(SR.smooth(const, tables, subtract_mean=True).ravel()) <= tol, name
        # the separable tables are symmetric to the bit, the radial one has every |m|^2 of the mesh
        for q in range(3):
            if tables[q] is not None:
                assert tables[q].shape == (N,) and tables[q][1:].tobytes() == tables[q][1:][::-1].tobytes(), (name, q)
        assert tables[3] is None or tables[3].shape == (SR.n_radial(N),)
        assert all(t is None or np.all(np.isfinite(t)) for t in tables)
    # a Gaussian of a delta sums to 1 (W(0) = 1) and is positive where it matters
    h = SR.smooth(delta, S.gaussian(3.0).tables(N))
    assert abs(float(PR.exact_sum(h)) - 1.0) <= 2.5 * PR.c_of_N(N) * N ** 1.5 and h[1, N - 1, 2] == h.max() > 0
    # a sharp cut is a projection: twice is once
    tables = S.sharp_k(N / 4).tables(N)
    once = SR.smooth(g, tables)
    twice = SR.smooth(once, tables)
    assert set(np.unique(tables[3]).tolist()) <= {0.0, 1.0} and tables[3][0] == 1.0
    assert np.linalg.norm((twice - once).ravel()) <= _bound(N, np.ones(1), g)
    assert np.linalg.norm((once - g).ravel()) > 0.1 * np.linalg.norm(g.ravel())       # (and it does cut)
    # the identity is a round trip
    assert np.linalg.norm((SR.smooth(g) - g).ravel()) <= _bound(N, np.ones(1), g)


def test_filter_values():
    S = _S()
    N = 16
    w = S.gaussian(4.0, axes=1).tables(N)
    sigma = 4.0 / (2 * np.sqrt(2 * np.log(2)))
    m = np.minimum(np.arange(N), N - np.arange(N))
    assert w[0] is None and w[2] is None and w[3] is None and np.allclose(w[1], np.exp(-0.5 * (2 * np.pi * m / N) ** 2 * sigma ** 2), rtol=1e-15)
    x = np.pi * m * 2.5 / N
    assert np.allclose(S.boxcar(2.5, 0).tables(N)[0][1:], np.sin(x[1:]) / x[1:], rtol=1e-15) and S.boxcar(2.5, 0).tables(N)[0][0] == 1.0
    d = S.boxcar(5, 2).tables(N)[2]
    assert np.allclose(d[1:], np.sin(np.pi * m[1:] * 5 / N) / (5 * np.sin(np.pi * m[1:] / N)), rtol=1e-13, atol=1e-16)
    assert np.array_equal(S.boxcar(1, 0).tables(N)[0], np.ones(N))           # a one-cell average is the identity, to the bit
    r = S.spherical_tophat(3.0).tables(N)[3]
    xs = 2 * np.pi * np.sqrt(np.arange(1, r.size)) * 3.0 / N
    assert r[0] == 1.0 and np.allclose(r[1:], 3 * (np.sin(xs) - xs * np.cos(xs)) / xs ** 3, rtol=1e-9)
    small = S.spherical_tophat(0.01).tables(N)[3]                             # the series below x = 0.1 joins the closed form
    xs = 2 * np.pi * np.sqrt(np.arange(small.size)) * 0.01 / N
    assert np.all(np.abs(small - (1 - xs ** 2 / 10)) <= 1e-6) and np.all(np.diff(small) < 0)
    k = S.sharp_k(2.5).tables(N)[3]
    assert k[:7].tolist() == [1.0] * 7 and not k[7:].any()                    # floor(2.5^2) = 6
    t = S.telescope(2.0, 3.0, los_axis=0).tables(N)
    assert np.array_equal(t[0], S.boxcar(3, 0).tables(N)[0]) and np.array_equal(t[1], S.gaussian(2.0, axes=(1,)).tables(N)[1])
    assert np.array_equal(t[2], t[1]) and t[3] is None
    prod = (S.gaussian(2.0) * S.boxcar(3, 0) * S.sharp_k(3)).tables(N)
    assert np.array_equal(prod[0], S.gaussian(2.0).tables(N)[0] * S.boxcar(3, 0).tables(N)[0]) and prod[3] is not None
    assert "gaussian(2" in repr(S.gaussian(2.0) * S.sharp_k(3)) and "sharp_k(3)" in repr(S.gaussian(2.0) * S.sharp_k(3))
    for bad, what in ((lambda: S.gaussian(-1.0), "fwhm must be"), (lambda: S.gaussian(1.0, axes=(0, 0)), "must not repeat"),
                      (lambda: S.boxcar(3, 3), "axis must be 0, 1 or 2"), (lambda: S.boxcar(np.nan, 0), "width must be"),
                      (lambda: S.spherical_tophat(np.inf), "R must be"), (lambda: S.sharp_k("3"), "m_max must be"),
                      (lambda: S.telescope(1.0, 1.0, los_axis=-1), "axis must be")):
        with pytest.raises(ValueError, match=what):
            bad()


def test_statistics_and_histogram_of_the_statement():
    h = np.array([[[-1.0, 0.0], [0.5, 1.0]], [[1.0, 2.0], [3.0, 1.5]]])
    s = SR.statistics(h, g=h)
    mu = h.mean()
    assert s[SR.N_FINITE] == 8 and s[SR.N_NONFINITE] == 0 and s[SR.MIN] == -1.0 and s[SR.MAX] == 3.0 and s[SR.SUM] == 8.0
    assert s[SR.INPUT_SUM] == 8.0 and s[SR.INPUT_SUM2] == float(np.sum(h * h))
    for p, key in ((2, SR.S2), (3, SR.S3), (4, SR.S4)):
        assert abs(s[key] - np.sum((h - mu) ** p)) <= 1e-14 * np.sum(np.abs(h - mu) ** p)
    # cells below, above and exactly on an edge: on an edge goes to the upper bin, on the last edge counts as above
    assert SR.histogram(h, [0.0, 1.0, 2.0]).tolist() == [2, 3, 1, 2]
    assert SR.histogram(h, [-5.0, 5.0]).tolist() == [8, 0, 0]
    h[0, 0, 0] = np.nan
    h[1, 1, 1] = np.inf
    s = SR.statistics(h)
    assert s[SR.N_FINITE] == 6 and s[SR.N_NONFINITE] == 2 and s[SR.MIN] == 0.0 and s[SR.MAX] == 3.0 and np.isnan(s[SR.SUM])
    assert SR.histogram(h, [0.0, 1.0, 2.0]).tolist() == [2, 2, 0, 2]
