"""TEST INFRASTRUCTURE: a stand-in for the HIP library that answers ``smooth_field`` (tests/test_smoothing_host.py).

``Counting(N)`` records every call like ``budget_standin_backend.Converging`` and lets a one-GPU step run to its end;
``smooth_field`` hands out the ten numbers of ``STATS`` scaled to the mesh -- N^3 finite cells between -1 and 3 with mean 0.5,
variance 4, skewness 0.25 and excess kurtosis -1 -- and, with edges, a histogram of 10 (b + 1) cells in bin b, 3 below and 4 above."""
import numpy as np

import budget_standin_backend as BS


def stats(N):
    n = float(N) ** 3
    #                finite non-finite min  max  sum g     sum g^2    sum h    S2       S3              S4
    return np.array([n, 0.0, -1.0, 3.0, 0.25 * n, 2.0625 * n, 0.5 * n, 4.0 * n, 0.25 * 8.0 * n, 2.0 * 16.0 * n])


def histogram(edges):
    nb = len(edges) - 1
    return np.concatenate([10 * np.arange(1, nb + 1), [3, 4]]).astype(np.uint64)


class Counting(BS.Converging):
    def __init__(self, N):
        super().__init__()
        self._N = N

    def __getattr__(self, name):
        inner = super().__getattr__(name)
        if name != "smooth_field":
            return inner

        def method(*args, **kwargs):
            inner(*args, **kwargs)
            edges = kwargs.get("edges")
            return dict(stats=stats(self._N), hist=None if edges is None else histogram(edges),
                        field=np.zeros((self._N,) * 3) if kwargs.get("field") else None)
        return method
