"""TEST INFRASTRUCTURE: two numpy statements of the C-ABI of asora_bispectrum (include/asora_hip.h), and the
error bound the GPU tests hold the device to.  Nothing here runs on a device; tests/test_bispectrum_reference.py checks the two
statements against each other.

* :func:`fft_route`: shells by the integer thresholds on the folded |n|^2, one inverse transform per shell, products of three cubes
  summed over the cells -- the estimator itself, in numpy.
* :func:`direct_sums`: the definition -- the sum of ghat(n1) ghat(n2) ghat(n3) over the ORDERED triples n1 in S_a, n2 in S_b, n3 in
  S_c with n1 + n2 + n3 = 0 modulo N on every axis, and the number of those triples -- with no transform in it: for every n1, n3 =
  -(n1 + n2) mod N of every n2 is looked up.  N^6 operations: affordable up to N = 16.

The bound (:func:`bound`), derived, not tuned.  The device's shell field is d_a + e_a with ||e_a||_2 <= E = 2.5 c(N) ||g||_2, the
smoothing's bound (tests/test_gpu_smoothing.py) with max |W| = 1, c(N) of tests/powerspec_reference.py.  Then

    sum (d_a + e_a)(d_b + e_b)(d_c + e_c) - sum d_a d_b d_c
        = [sum e_a d_b d_c + two more]  +  [sum e_a e_b d_c + two more]  +  sum e_a e_b e_c,

and by Cauchy-Schwarz |sum e_a d_b d_c| <= E ||d_b d_c||_2, |sum e_a e_b d_c| <= E^2 max|d_c|, |sum e_a e_b e_c| <= E^3 (the maximum of
e_c is at most its 2-norm).  The arithmetic behind the cubes: (d_a d_b) d_c costs two roundings per cell, 2 eps sum |d_a d_b d_c|; the
double-double accumulation costs eps^2 per term, which is dropped; the sum is rounded to a double once and multiplied by N^3 twice,
3 eps |sum| <= 3 eps sum |d_a d_b d_c|.  Together, times the N^6 of the definition:

    |sum_ggg - exact| <= N^6 ( E (||d_b d_c|| + ||d_a d_c|| + ||d_a d_b||) + E^2 (max|d_a| + max|d_b| + max|d_c|) + E^3
                               + 5 eps sum |d_a d_b d_c| ).

The norms come from the reference's cubes.  For sum_iii the field is the one whose transform is 1 everywhere, g = 1 at the origin
and 0 elsewhere: ||g||_2 = 1, E = 2.5 c(N).  Where the exact answer is 0 the bound is what is left: it is absolute."""
import numpy as np

import powerspec_reference as PR

EPS = PR.EPS


def shell_map(N, thresholds):
    """the shell of every mode of the full cube, (N, N, N) int64; -1: in no shell"""
    thr = np.asarray(thresholds, dtype=np.int64)
    assert thr[0] >= 1 and np.all(np.diff(thr) >= 0)
    m = PR.folded(N).astype(np.int64)
    n2 = m[:, None, None] ** 2 + m[None, :, None] ** 2 + m[None, None, :] ** 2
    s = np.searchsorted(thr, n2, side="right") - 1
    s[s >= thr.size - 1] = -1
    return s


def shell_cubes(g, thresholds, only=None):
    """(d, i): the shell fields of g and of the indicator, (n_shells, N, N, N) float64 each; only: the shells to form (the others
    stay zero), None for all"""
    g = np.asarray(g, dtype=np.float64)
    N = g.shape[0]
    half = shell_map(N, thresholds)[:, :, :N // 2 + 1]
    ghat = np.fft.rfftn(g)
    ns = len(thresholds) - 1
    d, i = np.zeros((ns, N, N, N)), np.zeros((ns, N, N, N))
    for a in (range(ns) if only is None else sorted(only)):
        mask = half == a
        d[a] = np.fft.irfftn(np.where(mask, ghat, 0.0), s=(N, N, N), axes=(0, 1, 2))
        i[a] = np.fft.irfftn(mask.astype(np.complex128), s=(N, N, N), axes=(0, 1, 2))
    return d, i


def triangle_sums(cubes, triangles):
    """N^6 sum over the cells of (c_a c_b) c_c for every triangle, the sum in extended precision"""
    n6 = float(cubes.shape[1]) ** 6
    return np.array([float(np.sum((cubes[a] * cubes[b]) * cubes[c], dtype=np.longdouble)) * n6 for a, b, c in triangles])


def fft_route(g, thresholds, triangles):
    """dict of sum_ggg, sum_iii (one per triangle) and the cubes d, i they were formed from"""
    d, i = shell_cubes(g, thresholds, set(int(q) for q in np.ravel(triangles)))
    return dict(sum_ggg=triangle_sums(d, triangles), sum_iii=triangle_sums(i, triangles), d=d, i=i)


def direct_sums(g, thresholds):
    """(G, C): G[a, b, c] the sum of ghat(n1) ghat(n2) ghat(n3) over the ordered closed triples of the shells (complex: the imaginary
    part is rounding), C[a, b, c] their number (int64).  ghat by numpy's transform of the small cube; the triples by looking up."""
    g = np.asarray(g, dtype=np.float64)
    N = g.shape[0]
    ns = len(thresholds) - 1
    shell = shell_map(N, thresholds).ravel()
    ghat = np.fft.fftn(g).ravel()
    X, Y, Z = (v.ravel() for v in np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij"))
    inside = np.flatnonzero(shell >= 0)
    sh2, g2 = shell[inside], ghat[inside]
    G = np.zeros((ns, ns, ns), dtype=np.complex128)
    Cn = np.zeros((ns, ns, ns), dtype=np.int64)
    for n1 in inside:
        n3 = ((-X[n1] - X[inside]) % N) * N * N + ((-Y[n1] - Y[inside]) % N) * N + (-Z[n1] - Z[inside]) % N
        sh3 = shell[n3]
        ok = sh3 >= 0
        key = sh2[ok] * ns + sh3[ok]
        w = g2[ok] * ghat[n3[ok]]
        a = shell[n1]
        G[a] += ghat[n1] * (np.bincount(key, weights=w.real, minlength=ns * ns)
                            + 1j * np.bincount(key, weights=w.imag, minlength=ns * ns)).reshape(ns, ns)
        Cn[a] += np.bincount(key, minlength=ns * ns).reshape(ns, ns)
    return G, Cn


def all_triangles(edges):
    """every a <= b <= c whose shells can close: the lower edge of c below the sum of the upper edges of a and b"""
    e = np.asarray(edges, dtype=np.float64)
    ns = e.size - 1
    return np.array([(a, b, c) for a in range(ns) for b in range(a, ns) for c in range(b, ns) if e[c] < e[a + 1] + e[b + 1]],
                    dtype=np.int32).reshape(-1, 3)


def bound(N, cubes, triangles, norm_g):
    """the module docstring's bound for every triangle; norm_g: ||g||_2 of the field behind the cubes (1 for the indicator)"""
    E = 2.5 * PR.c_of_N(N) * float(norm_g)
    n6 = float(N) ** 6
    peak = np.array([float(np.abs(c).max()) for c in cubes])
    out = []
    for a, b, c in triangles:
        da, db, dc = cubes[a], cubes[b], cubes[c]
        first = np.linalg.norm((db * dc).ravel()) + np.linalg.norm((da * dc).ravel()) + np.linalg.norm((da * db).ravel())
        out.append(n6 * (E * first + E * E * (peak[a] + peak[b] + peak[c]) + E ** 3 + 5.0 * EPS * float(np.sum(np.abs(da * db * dc)))))
    return np.array(out)


def three_waves(N, amplitudes, phases, q=((1, 0, 0), (1, 2, 0), (-2, -2, 0))):
    """sum of A cos(2 pi q.c / N + phi) over the three waves, (N, N, N)"""
    c = np.arange(N)
    g = np.zeros((N, N, N))
    for A, phi, (qx, qy, qz) in zip(amplitudes, phases, q):
        g += A * np.cos(2.0 * np.pi * (qx * c[:, None, None] + qy * c[None, :, None] + qz * c[None, None, :]) / N + phi)
    return g
