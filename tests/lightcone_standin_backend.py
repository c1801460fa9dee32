"""TEST INFRASTRUCTURE: a numpy stand-in for the HIP library's three light-cone calls (tests/test_lightcone_host.py).

``Numpy(N)`` records every call like ``budget_standin_backend.Converging`` and lets a one-GPU step run to its end.  It keeps the grids
that ``grid_to_device`` hands it (a grid never uploaded is all ones) and answers ``lightcone_advance`` from them with the numpy
statement (tests/lightcone_reference.py), slot by slot, as the library would: the first call on a slot only stores, a call with more
than ``max_slices`` slices or on a slot of another kind raises."""
import numpy as np

import budget_standin_backend as BS
import lightcone_reference as R


class Numpy(BS.Converging):
    def __init__(self, N, max_slices=1024):
        super().__init__()
        self._N, self.max_slices = N, max_slices
        self.grids, self.slots = {}, {}

    def _grid(self, which):
        return self.grids.get(which, np.ones((self._N,) * 3))

    def _now(self, kind, src_grid, t_gamma):
        if src_grid is not None:
            return np.array(self._grid(src_grid), dtype=np.float64)
        x, n, T = self._grid(4), self._grid(0), self._grid(3)           # GRID_XH, GRID_NDENS, GRID_TEMP
        return R.form(kind, x, n, T, float(np.mean(n)), t_gamma)

    def __getattr__(self, name):
        inner = super().__getattr__(name)
        if name not in ("lightcone_advance", "lightcone_state", "lightcone_reset", "grid_to_device"):
            return inner

        def method(*args, **kwargs):
            inner(*args, **kwargs)
            if name == "grid_to_device":
                self.grids[args[0]] = np.array(args[1], dtype=np.float64, order="C")
                return None
            if name == "lightcone_reset":
                self.slots.pop(args[0], None)
                return None
            if name == "lightcone_state":
                kept = self.slots.get(args[0])
                return dict(has_prev=kept is not None, kind=kept[0] if kept else 0, src_grid=kept[1] if kept else None)
            slot, kind, src_grid, t_gamma, axis, planes, w_prev, w_now, refresh = args
            n = len(planes)
            kept = self.slots.get(slot)
            if n > self.max_slices:
                raise RuntimeError(f"lightcone_advance failed (code 3): {n} slices are more than {self.max_slices}")
            if kept is None and (n != 0 or not refresh):
                raise RuntimeError("lightcone_advance failed (code 3): the first call on a slot stores the field")
            if kept is not None and kept[:2] != (kind, src_grid):
                raise RuntimeError("lightcone_advance failed (code 3): the slot's kept field was made with another kind")
            now = self._now(kind, src_grid, t_gamma)
            slices = R.blend(kept[2], now, planes, w_prev, w_now, axis) if n else np.zeros((0, self._N, self._N))
            if refresh:
                self.slots[slot] = (kind, src_grid, now)
            moments = np.stack([slices.sum(axis=(1, 2)), (slices * slices).sum(axis=(1, 2))], axis=1)
            return dict(slices=slices if kwargs.get("slices", True) else None, moments=moments)
        return method
