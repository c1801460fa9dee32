"""TEST INFRASTRUCTURE: a stand-in for the HIP library that answers ``lyman_alpha_forest`` and ``los_velocity_to_device``
(tests/test_lyman_alpha_host.py).

``Counting(N)`` records every call like ``budget_standin_backend.Converging`` and lets a one-GPU step run to its end.  The answer is
made from the mesh: sum F = N^3 / 2, sum F^2 = N^3 / 3, tau in [0.25, 8], W = 3, 5 cells clipped, 2 degenerate, N dark pixels in
two gaps of length 2 and N - 2; the PDF puts N^3 / n_bins cells into every bin; the upload answers max |v|."""
import numpy as np

import budget_standin_backend as BS


def answer(N, edges=None, tau=False, flux=False):
    cells = float(N) ** 3
    gaps = np.zeros(N + 1, dtype=np.uint64)
    gaps[2], gaps[N - 2] = gaps[2] + 1, gaps[N - 2] + 1
    counts = np.array([0, 3, 5, 2, N, 2, max(2, N - 2), 0], dtype=np.uint64)
    return dict(stats=np.array([cells / 2.0, cells / 3.0, 0.25, 8.0]), counts=counts, gaps=gaps,
                pdf=None if edges is None else np.full(len(edges) - 1, N ** 3 // (len(edges) - 1), dtype=np.uint64),
                tau=np.zeros((N,) * 3) if tau else None, flux=np.ones((N,) * 3) if flux else None)


class Counting(BS.Converging):
    def __init__(self, N):
        super().__init__()
        self._N = N

    def __getattr__(self, name):
        inner = super().__getattr__(name)
        if name not in ("lyman_alpha_forest", "los_velocity_to_device"):
            return inner

        def method(*args, **kwargs):
            inner(*args, **kwargs)
            if name == "los_velocity_to_device":
                return float(np.max(np.abs(args[0])))
            return answer(self._N, kwargs.get("edges"), kwargs.get("tau"), kwargs.get("flux"))
        return method
