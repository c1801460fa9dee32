"""CPU: the two numpy statements of the bispectrum (tests/bispectrum_reference.py) against each other and against an answer that owes
nothing to a transform.  The GPU tests (tests/test_gpu_bispectrum.py) hold the device to these."""
import math

import numpy as np
import pytest

import bispectrum_reference as BR
import powerspec_reference as PR


def _shells_to_nyquist(N):
    edges = np.arange(0, N // 2 + 1) + 0.5
    return edges, PR.thresholds_of(edges)


@pytest.mark.parametrize("N", (6, 8, 9))
def test_fft_route_equals_the_direct_sum(N):
    """Shells up to the Nyquist mode (N = 6 and 8 put it in the last shell), every ordered triangle of shells: the estimator's sums
    are the direct sums over closed triples modulo N, and its counts are their number."""
    g = PR.noise_with_block(N, 7000 + N)
    edges, thr = _shells_to_nyquist(N)
    ns = thr.size - 1
    tri = np.array([(a, b, c) for a in range(ns) for b in range(ns) for c in range(ns)], dtype=np.int32)
    got = BR.fft_route(g, thr, tri)
    G, C = BR.direct_sums(g, thr)
    want_g = np.array([G[a, b, c].real for a, b, c in tri])
    want_c = np.array([C[a, b, c] for a, b, c in tri])
    assert np.abs(G.imag).max() <= 1e-9 * np.abs(G.real).max()
    assert want_c.min() >= 0 and want_c.max() > 0
    assert np.array_equal(np.rint(got["sum_iii"]).astype(np.int64), want_c)
    assert np.abs(got["sum_iii"] - want_c).max() < 1e-6
    scale = np.abs(want_g).max()
    assert np.abs(got["sum_ggg"] - want_g).max() <= 1e-11 * scale
    # aliased triples are among them once a shell reaches beyond (N - 1) / 3: the counts of the unaliased definition are smaller
    assert 3 * math.isqrt(int(thr[-1]) - 1) > N - 1


def test_counts_are_symmetric_under_permutation():
    N = 8
    edges, thr = _shells_to_nyquist(N)
    G, C = BR.direct_sums(PR.noise_with_block(N, 11), thr)
    for perm in ((1, 0, 2), (2, 1, 0), (0, 2, 1)):
        assert np.array_equal(C, np.transpose(C, perm))
        assert np.allclose(G.real, np.transpose(G.real, perm), rtol=0, atol=1e-9 * np.abs(G.real).max())


def test_three_waves():
    """Three cosines at q = (1,0,0), (1,2,0), (-2,-2,0), which close: sum_ggg of the triangle of their shells is
    2 (N^3 / 2)^3 A1 A2 A3 cos(phi1 + phi2 + phi3), every triangle not made of these three shells is 0, and a phase flipped by pi
    flips the sign."""
    N = 12
    A, phi = (1.3, 0.7, 2.1), (0.4, -1.1, 2.5)
    thr = PR.thresholds_of(np.arange(0, 5) + 0.5)
    assert list(thr) == [1, 3, 7, 13, 21]
    tri = np.array([(a, b, c) for a in range(4) for b in range(4) for c in range(4)], dtype=np.int32)
    want = 2.0 * (N ** 3 / 2.0) ** 3 * A[0] * A[1] * A[2] * math.cos(sum(phi))
    got = BR.fft_route(BR.three_waves(N, A, phi), thr, tri)["sum_ggg"]
    flipped = BR.fft_route(BR.three_waves(N, A, (phi[0] + math.pi, phi[1], phi[2])), thr, tri)["sum_ggg"]
    G, _ = BR.direct_sums(BR.three_waves(N, A, phi), thr)
    for t, (a, b, c) in enumerate(tri):
        exact = want if sorted((a, b, c)) == [0, 1, 2] else 0.0
        assert abs(got[t] - exact) <= 1e-10 * abs(want), (a, b, c)
        assert abs(flipped[t] + exact) <= 1e-10 * abs(want), (a, b, c)
        assert abs(G[a, b, c].real - exact) <= 1e-10 * abs(want), (a, b, c)


def test_bound_is_small_against_the_sums():
    """The derived bound is a few thousand eps of the natural scale: it is a bound on rounding, not a licence."""
    N = 9
    g = PR.noise_with_block(N, 5)
    edges, thr = _shells_to_nyquist(N)
    tri = BR.all_triangles(edges)
    ref = BR.fft_route(g, thr, tri)
    b = BR.bound(N, ref["d"], tri, np.linalg.norm(g.ravel()))
    scale = float(N) ** 6 * np.array([np.sum(np.abs(ref["d"][a] * ref["d"][b_] * ref["d"][c])) for a, b_, c in tri])
    assert np.all(b > 0) and np.all(b <= 1e-10 * np.maximum(scale, scale.max() * 1e-3))
