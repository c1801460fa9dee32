"""TEST INFRASTRUCTURE: a stand-in for the HIP library that only records what it is asked (tests/test_lls_host.py).

``Recorder()`` takes any method call, appends (name, args) to ``calls`` and returns 0.0; ``evolve_begin`` and ``raytrace_device``
raise :class:`Stop`, so a step ends where its loop would begin and the test sees the prologue and what the ``finally`` blocks do.
``Untouchable()`` fails the test on any use: for checks that must come before the library is touched."""


class Stop(Exception):
    pass


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def method(*args, **kwargs):
            self.calls.append((name, args))
            if name in ("evolve_begin", "raytrace_device", "subbox_raytrace_device"):
                raise Stop(name)
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
    import pyc2ray_amd.lls  # noqa: F401  (lls_reset is handed the module's load_asora at call time)
    return backend
