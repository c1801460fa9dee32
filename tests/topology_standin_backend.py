"""TEST INFRASTRUCTURE: a stand-in for the HIP library that answers ``topology`` (tests/test_topology_host.py).

``Counting()`` records every call like ``budget_standin_backend.Converging`` and lets a one-GPU step run to its end; ``topology``
hands out ``TALLIES``."""
import numpy as np

import budget_standin_backend as BS

#: cells, closed faces / edges / vertices, open faces / edges / vertices, components, complement components, cavities
TALLIES = np.array([124, 450, 540, 216, 294, 228, 56, 1, 2, 1], dtype=np.uint64)


class Counting(BS.Converging):
    def __init__(self, N):
        super().__init__()
        self._N = N

    def __getattr__(self, name):
        inner = super().__getattr__(name)
        if name != "topology":
            return inner

        def method(*args, **kwargs):
            inner(*args, **kwargs)
            return TALLIES.copy()
        return method
