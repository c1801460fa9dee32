"""CPU: the numpy statement of the redshift-space mapping and of the anisotropic sums (tests/redshift_space_reference.py; DESIGN.md
section 4.2j) against known answers: the identity, whole-cell shifts, conservation, independence of the window, the degenerate cell,
inverted cells, the Kaiser factor of linear theory, and the sums against a loop over the modes."""
import numpy as np
import pytest

import powerspec_reference as PR
import redshift_space_reference as RR

MESHES = (3, 4, 8, 17, 32)


def _lines(N, seed):
    rng = np.random.default_rng(seed)
    return rng.random((N, N, N)) + 0.5


@pytest.mark.parametrize("N", MESHES)
def test_identity_and_whole_cell_shifts(N):
    g = _lines(N, 10 + N)
    for axis in (0, 1, 2):
        assert RR.map_lines(g, np.zeros((N, N, N)), 1.0, axis).tobytes() == g.tobytes()
        for shift in (1.0, -1.0):
            if 2 * RR.library_window(1.0, shift) + 1 > N:       # (N = 3, 4: a shift of a whole cell is wider than the library takes)
                h = RR.map_lines(g, np.full((N, N, N), shift), 1.0, axis, W=1)
            else:
                h = RR.map_lines(g, np.full((N, N, N), 0.5), 2.0 * shift, axis)
            assert np.array_equal(h, np.roll(g, int(shift), axis=axis))


@pytest.mark.parametrize("N", MESHES)
def test_conservation_and_independence_of_the_window(N):
    g = _lines(N, 20 + N)
    rng = np.random.default_rng(30 + N)
    top = 0.999 * ((N - 1) // 2)
    v = rng.uniform(-top, top, size=(N, N, N))
    for axis in (0, 1, 2):
        W = RR.library_window(np.max(np.abs(v)), 1.0)
        assert 2 * W + 1 <= N
        h = RR.map_lines(g, v, 1.0, axis)
        assert abs(float(PR.exact_sum(h) - PR.exact_sum(g))) <= 4 * (2 * W + 3) * PR.EPS * float(np.sum(np.abs(g)))
        lines = np.moveaxis(h, axis, -1).sum(axis=-1) - np.moveaxis(g, axis, -1).sum(axis=-1)       # every line conserves alone
        assert np.max(np.abs(lines)) <= 4 * (2 * W + 3) * PR.EPS * N * 1.5
        if N >= 8:
            assert RR.count_inverted(v, 1.0, axis) >= 1
        if 2 * (W + 1) + 1 <= N:
            assert RR.map_lines(g, v, 1.0, axis, W=W + 1).tobytes() == h.tobytes()
    small = 0.4 * v / top                                           # W = 1; a wider window gives the same bits
    h = RR.map_lines(g, small, 1.0, 2)
    if N >= 5:
        assert RR.map_lines(g, small, 1.0, 2, W=2).tobytes() == h.tobytes()


def test_the_degenerate_cell():
    """N = 8, u[3] = -2: d[3] = d[4] = -1, so cell 2 = [0, 1 + d[3]] collapses to a point and cell 3 = [-1, 0] moves one cell down"""
    N = 8
    g = np.broadcast_to(np.arange(1.0, 9.0), (N, N, N)).copy()
    v = np.zeros((N, N, N))
    v[:, :, 3] = -2.0
    h = RR.map_lines(g, v, 1.0, 2)
    assert np.all(h == np.array([1.0, 2.0, 7.0, 2.5, 2.5, 6.0, 7.0, 8.0]))
    assert h.sum() == g.sum()
    h = RR.map_lines(np.moveaxis(g, 2, 0), np.moveaxis(v, 2, 0), 1.0, 0)
    assert np.all(np.moveaxis(h, 0, 2) == np.array([1.0, 2.0, 7.0, 2.5, 2.5, 6.0, 7.0, 8.0]))


def test_the_kaiser_factor():
    """A white Gaussian field of rms 0.02 at N = 32 with the velocities of linear theory, f = 1: the power of the mapped field over
    (1 + mu^2)^2 times the real-space power, mode by mode below half the Nyquist frequency.  The velocities satisfy the continuity
    equation with the centred difference, the derivative the mapping takes of them (kaiser_field): what is left is second order, a
    median of 0.005 to 0.007 (three seeds, three axes).  With the continuum's derivative sampled at the cell centres the centred
    difference loses sin(k) / k of the velocity term and the median is 0.018 to 0.025: printed, not asserted."""
    N = 32
    for seed in (5, 6):
        delta, u = RR.kaiser_field(N, seed)
        assert abs(delta.std() - 0.02) < 1e-12
        _, uc = RR.kaiser_field(N, seed, continuum=True)
        for axis in (0, 1, 2):
            dev = RR.kaiser_deviation(N, axis, delta, RR.map_lines(1.0 + delta, u[axis], 1.0, axis))
            cont = RR.kaiser_deviation(N, axis, delta, RR.map_lines(1.0 + delta, uc[axis], 1.0, axis))
            print(f"seed {seed}, axis {axis}: median deviation {dev:.4f} (continuum velocities: {cont:.4f})")
            assert dev < 0.02
            # the sign convention s = x + u: with the velocities reversed the factor is (1 - mu^2)^2, far from this one
            wrong = RR.kaiser_deviation(N, axis, delta, RR.map_lines(1.0 + delta, -u[axis], 1.0, axis))
            assert wrong > 0.2


@pytest.mark.parametrize("N", (4, 5, 8))
def test_sums_against_a_loop_over_the_modes(N):
    rng = np.random.default_rng(40 + N)
    hhat = np.fft.rfftn(rng.normal(size=(N, N, N)))
    h = max(N // 2, 1)
    thr_sets = {RR.CYLINDRICAL: (np.array([0, 1, 2, 5]), np.array([0.0, 1.0, 4.0])),
                RR.MU: (np.array([1, 2, 5, 3 * h * h + 1]), np.array([0.0, 0.25, 0.5, 1.0]))}
    m = PR.folded(N)
    for mode, (thr_a, thr_b) in thr_sets.items():
        for axis in (0, 1, 2):
            got = RR.binned(N, axis, mode, thr_a, thr_b, hhat)
            n_a, n_b = len(thr_a) - 1, len(thr_b) - 1
            want = {key: np.zeros((n_a, n_b)) for key in ("count", "sum_1", "sum_2", "sum_aa", "sum_l2", "sum_l4")}
            for i in range(N):
                for j in range(N):
                    for kz in range(N // 2 + 1):
                        mm = (int(m[i]), int(m[j]), kz)
                        n2 = sum(q * q for q in mm)
                        if n2 == 0:
                            continue
                        mp = mm[axis]
                        w = 1.0 if kz == 0 or 2 * kz == N else 2.0
                        if mode == RR.CYLINDRICAL:
                            ia = int(np.searchsorted(thr_a, n2 - mp * mp, side="right")) - 1
                            ib = int(np.searchsorted(thr_b, float(mp * mp), side="right")) - 1
                            s1, s2 = np.sqrt(n2 - mp * mp), float(mp)
                        else:
                            ia = int(np.searchsorted(thr_a, n2, side="right")) - 1
                            ib = sum(1 for e in thr_b if e * float(n2) <= float(mp * mp)) - 1
                            s1, s2 = np.sqrt(n2), np.sqrt(mp * mp / n2)
                        if not (0 <= ia < n_a and 0 <= ib < n_b):
                            continue
                        t = float(mp * mp) / float(n2)
                        p = w * abs(hhat[i, j, kz]) ** 2
                        for key, val in (("count", w), ("sum_1", w * s1), ("sum_2", w * s2), ("sum_aa", p),
                                         ("sum_l2", p * 0.5 * (3 * t - 1)), ("sum_l4", p * 0.125 * ((35 * t - 30) * t + 3))):
                            want[key][ia, ib] += val
            assert np.array_equal(got["count"], want["count"].astype(np.uint64))
            for key in ("sum_1", "sum_2", "sum_aa", "sum_l2", "sum_l4"):
                assert np.allclose(got[key], want[key], rtol=1e-12, atol=1e-12 * float(np.max(np.abs(want["sum_aa"])))), (mode, axis, key)
            if mode == RR.MU:       # mu^2 = 1 on the last edge is left out; a last edge of 2 takes it in
                full = RR.binned(N, axis, mode, thr_a, np.array([0.0, 0.25, 0.5, 2.0]), hhat)
                on_axis = full["count"][:, 2].sum() - got["count"][:, 2].sum()
                assert on_axis == 2 * h - (1 if N % 2 == 0 else 0) - int(np.sum(np.arange(1, h + 1) ** 2 < thr_a[0]))
                # summed over mu, the counts are the spherical ones
                assert np.array_equal(full["count"].sum(axis=1), PR.binned(N, thr_a.astype(np.uint32), hhat)["count"])
