"""TEST INFRASTRUCTURE: a stand-in for the HIP library that answers ``power_spectrum`` (tests/test_powerspec_host.py).

``Counting(N)`` records every call like ``budget_standin_backend.Converging`` and lets a one-GPU step run to its end;
``power_spectrum`` hands out sums made from the thresholds it is given: bin b holds 10 (b + 1) modes of |n| = b + 1 with
|ahat|^2 = 4 N^6 each, and with a second field |bhat|^2 = 9 N^6 and Re(ahat conj(bhat)) = -3 N^6."""
import numpy as np

import budget_standin_backend as BS

MOMENTS_A = np.array([512.0, 2048.0])
MOMENTS_B = np.array([256.0, 4096.0])


def answer(N, thresholds, cross):
    nb = len(thresholds) - 1
    count = 10 * np.arange(1, nb + 1, dtype=np.uint64)
    n6 = float(N) ** 6
    c = count.astype(np.float64)
    return dict(count=count, sum_k=c * np.arange(1, nb + 1), sum_aa=4.0 * n6 * c, moments_a=MOMENTS_A.copy(),
                sum_bb=9.0 * n6 * c if cross else None, sum_ab=-3.0 * n6 * c if cross else None,
                moments_b=MOMENTS_B.copy() if cross else None, field=None, modes=None)


class Counting(BS.Converging):
    def __init__(self, N):
        super().__init__()
        self._N = N

    def __getattr__(self, name):
        inner = super().__getattr__(name)
        if name != "power_spectrum":
            return inner

        def method(*args, **kwargs):
            inner(*args, **kwargs)
            got = answer(self._N, args[4], args[1] is not None)
            if kwargs.get("field"):
                got["field"] = np.zeros((self._N,) * 3)
            if kwargs.get("modes"):
                got["modes"] = np.zeros((self._N, self._N, self._N // 2 + 1), dtype=complex)
            return got
        return method
