"""TEST INFRASTRUCTURE: a stand-in for the HIP library that answers ``power_spectrum_los``, ``redshift_space_field`` and
``los_velocity_to_device`` (tests/test_redshift_space_host.py).

``Counting(N)`` records every call like ``budget_standin_backend.Converging`` and lets a one-GPU step run to its end.  The sums are
made from the thresholds: bin (a, b) holds 10 (a + 1) modes with sum_1 = count (a + 1), sum_2 = count / 2, |hhat|^2 = 4 N^6 each,
sum_l2 = sum_aa / 2 and sum_l4 = sum_aa / 8; the upload answers max |v|."""
import numpy as np

import budget_standin_backend as BS

MOMENTS_REAL = np.array([512.0, 2048.0])
MOMENTS_RS = np.array([512.0, 3072.0])


def answer(N, thr_a, thr_b):
    n_a, n_b = len(thr_a) - 1, len(thr_b) - 1
    count = np.repeat(10 * np.arange(1, n_a + 1, dtype=np.uint64)[:, None], n_b, axis=1)
    c = count.astype(np.float64)
    aa = 4.0 * float(N) ** 6 * c
    return dict(count=count, sum_1=c * np.arange(1, n_a + 1)[:, None], sum_2=0.5 * c, sum_aa=aa, sum_l2=0.5 * aa, sum_l4=0.125 * aa,
                moments_real=MOMENTS_REAL.copy(), moments_rs=MOMENTS_RS.copy(), field=None, modes=None)


class Counting(BS.Converging):
    def __init__(self, N):
        super().__init__()
        self._N = N

    def __getattr__(self, name):
        inner = super().__getattr__(name)
        if name not in ("power_spectrum_los", "redshift_space_field", "los_velocity_to_device"):
            return inner

        def method(*args, **kwargs):
            inner(*args, **kwargs)
            if name == "los_velocity_to_device":
                return float(np.max(np.abs(args[0])))
            if name == "redshift_space_field":
                return dict(moments=MOMENTS_REAL.copy(), field=np.zeros((self._N,) * 3) if kwargs.get("field") else None)
            got = answer(self._N, args[6], args[7])
            if kwargs.get("field"):
                got["field"] = np.zeros((self._N,) * 3)
            if kwargs.get("modes"):
                got["modes"] = np.zeros((self._N, self._N, self._N // 2 + 1), dtype=complex)
            return got
        return method
