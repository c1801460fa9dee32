"""TEST INFRASTRUCTURE: a stand-in for the HIP library that answers ``bispectrum`` (tests/test_bispectrum_host.py).

``Counting(N)`` records every call like ``budget_standin_backend.Converging``; ``bispectrum`` hands out sums made from what it is
given: shell s holds 10 (s + 1) modes of |n| = s + 1 with |ghat|^2 = 4 N^6 each; triangle t = (a, b, c) has (a + 1)(b + 1)(c + 1)
closed triples -- none where a + b + c is 7, and a count off by 0.25 at triangle 0 -- with ghat ghat ghat = -2 N^9 each."""
import numpy as np

import budget_standin_backend as BS

MOMENTS = np.array([512.0, 2048.0])


def answer(N, thresholds, triangles):
    ns = len(thresholds) - 1
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    count = 10 * np.arange(1, ns + 1, dtype=np.uint64)
    c = count.astype(np.float64)
    iii = np.prod(tri + 1, axis=1).astype(np.float64)
    iii[tri.sum(axis=1) == 7] = 0.0
    ggg = -2.0 * float(N) ** 9 * iii
    iii[0] += 0.25
    return dict(sum_ggg=ggg, sum_iii=iii, count=count, sum_k=c * np.arange(1, ns + 1), sum_aa=4.0 * float(N) ** 6 * c, moments=MOMENTS.copy())


class Counting(BS.Converging):
    def __init__(self, N):
        super().__init__()
        self._N = N

    def __getattr__(self, name):
        inner = super().__getattr__(name)
        if name != "bispectrum":
            return inner

        def method(*args, **kwargs):
            inner(*args, **kwargs)
            return answer(self._N, args[3], args[4])
        return method
