"""TEST INFRASTRUCTURE: a numpy stand-in for the HIP library's halo-source calls (tests/test_halo_sources_host.py).

``Numpy(N)`` records every call like ``budget_standin_backend.Converging`` and lets a one-GPU step run to its end.  It keeps the grids
that ``grid_to_device`` hands it (a grid never uploaded is all zeros) and answers ``halo_catalogue_to_device``, ``halo_catalogue_state``,
``halo_catalogue_generation``, ``halo_catalogue_clear``, ``halo_table_to_host`` and ``halo_sources_build`` with the numpy statement
(tests/halo_sources_reference.py), as the library would: a build without a catalogue raises; ``new_mesh()`` is what a ``device_init``
does to the catalogue."""
import itertools

import numpy as np

import budget_standin_backend as BS
import halo_sources_reference as R

_OWN = ("grid_to_device", "halo_catalogue_to_device", "halo_catalogue_state", "halo_catalogue_generation", "halo_catalogue_clear",
        "halo_table_to_host", "halo_sources_build")
_GENERATIONS = itertools.count(1)          # (one numbering for all stand-ins of a process, as the library has one)


class Numpy(BS.Converging):
    def __init__(self, N):
        super().__init__()
        self._N = N
        self.grids, self.catalogue = {}, None

    def new_mesh(self):
        self.catalogue = None

    def __getattr__(self, name):
        inner = super().__getattr__(name)
        if name not in _OWN:
            return inner

        def method(*args, **kwargs):
            inner(*args, **kwargs)
            if name == "grid_to_device":
                self.grids[args[0]] = np.array(args[1], dtype=np.float64, order="C")
                return None
            if name == "halo_catalogue_clear":
                self.catalogue = None
                return None
            if name == "halo_catalogue_state":
                return None if self.catalogue is None else (int(self.catalogue[0].size), self.catalogue[3])
            if name == "halo_catalogue_generation":
                return None if self.catalogue is None else self.catalogue[4]
            if name == "halo_catalogue_to_device":
                pos, mass, weight, m_lm, m_hm, wrap, e = args
                cell, q_hm, q_lm, counts = R.table(pos, mass, weight, self._N, m_lm, m_hm, wrap, e)
                self.catalogue = (cell, q_hm, q_lm, e, next(_GENERATIONS))
                return counts
            if self.catalogue is None:
                raise RuntimeError(f"{name} failed (code 3): {name}: no catalogue on the device (halo_catalogue_to_device)")
            if name == "halo_table_to_host":
                return self.catalogue[:3]
            grid, g_hm, g_lm, scale, model, x_suppress, f = args
            x = self.grids.get(grid, np.zeros((self._N,) * 3))
            pos, flux, summary = R.build(*self.catalogue[:3], x, g_hm, g_lm, scale, model, x_suppress, f)
            return dict(pos=pos, flux=flux, summary=summary)
        return method
