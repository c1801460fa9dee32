"""TEST INFRASTRUCTURE: a stand-in for the HIP library whose device loop converges at once (tests/test_budget_host.py).

``Converging()`` records every call like ``lls_standin_backend.Recorder``, but lets a one-GPU step run to its end: ``evolve_poll``
reports one iteration and convergence, ``step_budget`` hands out the twelve numbers of ``SUMS``, the grid fetches return what
they are given."""
import numpy as np

SUMS = np.arange(1.0, 13.0)


class Converging:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def method(*args, **kwargs):
            self.calls.append((name, args, kwargs))
            if name == "evolve_poll":
                return 1, True, [(0, 1.0, 1.0, 0.0, 0.0)]
            if name == "step_budget":
                return SUMS.copy()
            if name == "grid_to_host":
                return args[1]
            if name == "host_empty":
                return np.zeros(args[0])
            return 0.0
        return method

    def names(self):
        return [c[0] for c in self.calls]
