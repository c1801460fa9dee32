"""TEST INFRASTRUCTURE: a stand-in for the HIP library that answers ``region_sizes`` (tests/test_regions_host.py).

``Labelling(N)`` records every call like ``budget_standin_backend.Converging`` and lets a one-GPU step run to its end;
``region_sizes`` hands out ``TALLIES`` and counts and cells spread over the bins it is asked for, and with ``labels=True`` a label
grid of zeros behind them."""
import numpy as np

import budget_standin_backend as BS

#: n_phase, n_regions, sum_v2, v_largest, label_largest, extents i j k, v_second, label_second, under- and overflow in regions and cells
TALLIES = np.array([400, 12, 90_000, 300, 73, 8, 5, 7, 40, 9, 2, 3, 1, 50], dtype=np.uint64)


def bins_for(nbins):
    """(counts, cells): 9 regions with 347 cells in the bins (the 12 and 400 less under- and overflow), all in the last bin but one
    region of one cell in the first"""
    counts, cells = np.zeros(nbins, dtype=np.uint64), np.zeros(nbins, dtype=np.uint64)
    if nbins == 1:
        counts[0], cells[0] = 9, 347
    else:
        counts[0], cells[0], counts[-1], cells[-1] = 1, 1, 8, 346
    return counts, cells


class Labelling(BS.Converging):
    def __init__(self, N):
        super().__init__()
        self._N = N

    def __getattr__(self, name):
        inner = super().__getattr__(name)
        if name != "region_sizes":
            return inner

        def method(*args, **kwargs):
            inner(*args, **kwargs)
            out = bins_for(len(args[5]) - 1) + (TALLIES.copy(),)
            return out + (np.zeros((self._N,) * 3, dtype=np.uint32),) if kwargs.get("labels") else out
        return method
