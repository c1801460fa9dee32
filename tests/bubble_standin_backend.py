"""TEST INFRASTRUCTURE: a stand-in for the HIP library that answers ``bubble_mfp`` (tests/test_bubbles_host.py).

``Bubbling(N)`` records every call like ``budget_standin_backend.Converging`` and lets a one-GPU step run to its end;
``bubble_mfp`` hands out ``COUNTS`` spread over the bins it is asked for, ``TALLIES`` and ``MOMENTS``."""
import numpy as np

import budget_standin_backend as BS

TALLIES = np.array([90, 7, 3, 2, 1, 4321], dtype=np.uint64)       # ended, capped, left_box, underflow, overflow, n_phase
MOMENTS = np.array([450.0, 3600.0])


def counts_for(nbins):
    """87 rays in the bins (the 90 ended ones less under- and overflow), all in the last bin but one in the first"""
    c = np.zeros(nbins, dtype=np.uint64)
    c[-1], c[0] = 86, c[0] + 1
    if nbins == 1:
        c[0] = 87
    return c


class Bubbling(BS.Converging):
    def __init__(self, N):
        super().__init__()
        self._N = N

    def __getattr__(self, name):
        inner = super().__getattr__(name)
        if name != "bubble_mfp":
            return inner

        def method(*args, **kwargs):
            inner(*args, **kwargs)
            return counts_for(len(args[7]) - 1), TALLIES.copy(), MOMENTS.copy()
        return method
