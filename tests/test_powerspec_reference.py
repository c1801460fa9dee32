"""CPU: the numpy statement of asora_power_spectrum (tests/powerspec_reference.py) against a brute-force transform and against what
the header says of weights, folding and edges."""
import numpy as np
import pytest

import fft_meshes as FM
import powerspec_reference as PR


@pytest.mark.parametrize("N", [5, 6])
def test_reference_against_a_brute_force_transform(N):
    g = PR.noise_with_block(N, 100 + N)
    full = PR.brute_force_dft(g)                                   # every n, extended precision
    half = np.fft.rfftn(g)
    assert half.shape == (N, N, N // 2 + 1)
    want = full[:, :, :N // 2 + 1].astype(np.complex128)
    err = np.linalg.norm((half - want).ravel()) / np.linalg.norm(want.ravel())
    print(f"N {N}: rfftn against the brute-force transform {err:.3e}, c(N) {PR.c_of_N(N):.3e}")
    assert err <= PR.c_of_N(N)
    # the binned sums of the stored half-space with its weights are those over ALL modes, folded, each counted once
    edges = np.arange(0, N // 2 + 2) + 0.5
    thr = PR.thresholds_of(edges)
    got = PR.binned(N, thr, half)
    m = PR.folded(N).astype(np.int64)
    n2 = m[:, None, None] ** 2 + m[None, :, None] ** 2 + m[None, None, :] ** 2
    power = np.abs(full.astype(np.complex128)) ** 2
    for b in range(len(thr) - 1):
        inside = (n2 >= thr[b]) & (n2 < thr[b + 1])
        assert got["count"][b] == inside.sum()
        assert abs(got["sum_k"][b] - np.sqrt(n2[inside]).sum()) <= 1e-13 * max(1.0, np.sqrt(n2[inside]).sum())
        assert abs(got["sum_aa"][b] - power[inside].sum()) <= 1e-12 * power.sum()
    assert abs(got["total_aa"] - (power.sum() - power[0, 0, 0])) <= 1e-12 * power.sum()
    # Parseval: the power of every mode but n = 0 over N^3 is sum g^2 - (sum g)^2 / N^3
    sums = PR.power_sums(g, np.array([1, 3 * N * N], dtype=np.uint32))
    spread = sums["moments_a"][1] - sums["moments_a"][0] ** 2 / N ** 3
    assert abs(sums["sum_aa"][0] / N ** 3 - spread) <= 1e-12 * spread and sums["count"][0] == N ** 3 - 1


@pytest.mark.parametrize("N", FM.MESHES)
def test_numpy_serves_as_the_reference_at_the_meshes_of_the_table(N):
    """The bounds of the GPU tests, c(N) = 8 eps (log2 N^3 + p), rest on numpy's own error being far inside them.  Along one axis:
    np.fft.fft of 32 random real lines against the DFT matrix in extended precision ((r c) mod N reduced before the angle is formed,
    as brute_force_dft does), in the relative 2-norm, within a tenth of the per-axis share c(N) / 3."""
    lines = np.random.default_rng(7000 + N).normal(size=(32, N))
    r = (np.arange(N)[:, None] * np.arange(N)[None, :]) % N
    ang = -2.0 * np.pi * r.astype(np.longdouble) / N
    W = np.cos(ang) + 1j * np.sin(ang)
    want = lines.astype(np.clongdouble) @ W                           # (W is symmetric)
    got = np.fft.fft(lines, axis=1)
    diff = got.astype(np.clongdouble) - want
    err = float(np.sqrt(np.sum(np.abs(diff) ** 2) / np.sum(np.abs(want) ** 2)))
    share = PR.c_of_N(N) / 3.0
    print(f"N {N}: np.fft.fft against the extended-precision DFT {err / PR.EPS:.2f} eps, c(N) / 3 = {share / PR.EPS:.0f} eps: "
          f"{100.0 * err / share:.2f} % of it")
    assert err <= 0.1 * share


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17])
def test_weights_sum_to_all_modes_but_one(N):
    w = np.broadcast_to(PR.mode_weights(N)[None, None, :], (N, N, N // 2 + 1))
    assert w.sum() == N ** 3                                        # the half-space with its weights is the whole space
    got = PR.binned(N, np.array([1, 3 * N * N + 1], dtype=np.uint32), np.ones((N, N, N // 2 + 1), dtype=complex))
    assert got["count"].tolist() == [N ** 3 - 1] and got["sum_aa"][0] == N ** 3 - 1
    assert PR.mode_n2(N)[0, 0, 0] == 0 and PR.bin_of(N, [1, 2])[0, 0, 0] == -1      # n = 0 is never binned
    assert PR.mode_n2(N).max() == 3 * (N // 2) ** 2


def test_a_mode_on_an_edge_goes_to_the_upper_bin():
    N = 8
    thr = PR.thresholds_of([1, 2, 3])
    assert thr.tolist() == [1, 4, 9]
    b = PR.bin_of(N, thr)
    assert b[2, 0, 0] == 1 and b[0, 2, 0] == 1 and b[0, 0, 2] == 1 and b[N - 2, 0, 0] == 1      # |n| = 2, folded too
    assert b[1, 0, 0] == 0 and b[1, 1, 1] == 0 and b[2, 2, 0] == 1 and b[0, 0, 3] == -1 and b[2, 2, 1] == -1    # |n|^2 = 1, 3, 8, 9, 9
    # edges that are no integers: ceil(edge^2); below the first edge and at or above the last: dropped
    assert PR.thresholds_of([0.5, 1.5, 2.5]).tolist() == [1, 3, 7] and PR.thresholds_of([1e-200, 1e30]).tolist() == [1, 2 ** 32 - 1]
    ones = np.ones((N, N, N // 2 + 1), dtype=complex)
    got = PR.binned(N, thr, ones)
    n2 = PR.mode_n2(N)
    w = np.broadcast_to(PR.mode_weights(N)[None, None, :], n2.shape)
    assert got["count"].tolist() == [w[(n2 >= 1) & (n2 < 4)].sum(), w[(n2 >= 4) & (n2 < 9)].sum()]
    # equal thresholds: an empty bin
    assert PR.binned(N, np.array([1, 4, 4, 9]), ones)["count"].tolist() == [got["count"][0], 0, got["count"][1]]


def test_forming_the_field_and_the_bound():
    rng = np.random.default_rng(5)
    x, n, T = rng.random((4, 4, 4)), 1e-4 * (1 + rng.random((4, 4, 4))), 50.0 + 100.0 * rng.random((4, 4, 4))
    nbar = PR.mean_density(n)
    assert abs(nbar - n.mean()) <= 2 * PR.EPS * nbar
    assert np.array_equal(PR.form_field(PR.XH, x), x) and np.array_equal(PR.form_field(PR.XHI, x), 1.0 - x)
    assert np.array_equal(PR.form_field(PR.DENSITY, n=n), n / nbar)
    assert np.array_equal(PR.form_field(PR.HI, x, n, scale=3.0), (3.0 * (1.0 - x)) * (n / nbar))
    assert np.array_equal(PR.form_field(PR.HI, x, n, T, scale=3.0, t_gamma=30.0), ((3.0 * (1.0 - x)) * (n / nbar)) * (1.0 - 30.0 / T))
    assert [PR.largest_prime_factor(N) for N in (1, 2, 8, 30, 43, 49, 129, 136, 250, 645)] == [1, 2, 2, 5, 43, 7, 43, 17, 5, 43]
    assert [PR.largest_prime_factor(N) for N in FM.MESHES] == [11, 139, 7, 13, 3, 2, 271, 17, 13]
    assert PR.c_of_N(64) == 8 * PR.EPS * 18 and PR.c_of_N(43) == 8 * PR.EPS * (3 * np.log2(43.0) + 43)
