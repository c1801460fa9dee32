"""TEST INFRASTRUCTURE: a stand-in for the HIP library that only records what it is asked (tests/test_open_boundaries_host.py).

``Recorder()`` takes any method call, appends (name, args) to ``calls`` and returns 0.0.  With ``stop=True`` the calls that begin
the work of a step (``evolve_begin``, ``raytrace_device``, ``subbox_raytrace_device``) raise :class:`Stop`, so the test sees what
the ``finally`` blocks do after a failure; with ``stop=False`` the step runs through: ``evolve_poll`` reports convergence after one
iteration.  ``Untouchable()`` fails the test on any use: for checks that must come before the library is touched."""


class Stop(Exception):
    pass


class Recorder:
    def __init__(self, stop=True):
        self.calls = []
        self.stop = stop

    def __getattr__(self, name):
        def method(*args, **kwargs):
            self.calls.append((name, args))
            if self.stop and name in ("evolve_begin", "raytrace_device", "subbox_raytrace_device"):
                raise Stop(name)
            if name == "evolve_poll":
                return 1, True, [(0, 1.0, 1.0, 0.0, 0.0)]
            return 0.0
        return method

    def names(self):
        return [c[0] for c in self.calls]


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the arguments were checked")


def install(monkeypatch, backend):
    """Every way the step functions reach the library now leads to `backend`."""
    import pyc2ray_amd.evolve as E
    import pyc2ray_amd.raytracing as R
    for mod in (E, R):
        monkeypatch.setattr(mod, "load_asora", lambda: backend)
        monkeypatch.setattr(mod, "cuda_is_init", lambda: True)
    return backend
