"""TEST INFRASTRUCTURE: a stand-in for the HIP library that answers ``granulometry`` (tests/test_granulometry_host.py).

``Counting()`` records every call like ``budget_standin_backend.Converging`` and lets a one-GPU step run to its end; ``granulometry``
hands out counts made from the radii it is given: ``n_phase`` = 400 cells, of which an opening of radius R keeps 400 - 40 R."""
import numpy as np

import budget_standin_backend as BS

TALLIES = np.array([400, 50, 0, 3000], dtype=np.uint64)


def answer(radii):
    r = np.asarray(radii, dtype=np.float64)
    opened = np.maximum(400 - 40 * r, 0).astype(np.uint64)
    return opened // np.uint64(2), opened, TALLIES.copy()


class Counting(BS.Converging):
    def __init__(self, N):
        super().__init__()
        self._N = N

    def __getattr__(self, name):
        inner = super().__getattr__(name)
        if name != "granulometry":
            return inner

        def method(*args, **kwargs):
            inner(*args, **kwargs)
            got = answer(args[4])
            return got + (np.zeros((self._N,) * 3, dtype=np.uint32),) if kwargs.get("distances") else got
        return method
