"""CPU: the host side of the plane-parallel flux: PlaneFlux and plane_flux_spec, the C-ABI symbols, the
YAML keys and the ``plane_flux`` attribute of the simulation class, and -- on a stand-in for the library -- that bad input is
refused before the library is touched, that the state is set before the loop and cleared whatever happens, that only rank 0 holds
the faces, that faces count as sources in the convergence criterion and move a slab-exchange communicator to the all-reduce loop."""
import ctypes as C
import os

import numpy as np
import pytest

import lls_standin_backend as SB

HERE = os.path.dirname(os.path.abspath(__file__))
PLANE_PARAMS = os.path.join(HERE, "data", "parameters_plane_flux.yml")
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_test.yml")


def _install(monkeypatch, backend):
    SB.install(monkeypatch, backend)
    return backend


def test_plane_flux_and_spec_validation():
    from pyc2ray_amd.planeflux import FACES, PlaneFlux, plane_flux_spec
    assert FACES == ("-x", "+x", "-y", "+y", "-z", "+z")
    f = PlaneFlux("+y", 2, spectrum=np.int32(1))
    assert (f.face, f.flux, f.spectrum, f.name) == (3, 2.0, 1, "+y") and f == PlaneFlux(3, 2.0, 1) and "+y" in repr(f)
    assert PlaneFlux(0, 0.0).flux == 0.0 and PlaneFlux(np.int64(5), np.float64(1.5)).name == "+z"
    for bad in ("x", "-w", 6, -1, 1.0, None, True, [0]):
        with pytest.raises(ValueError, match="PlaneFlux: face"):
            PlaneFlux(bad, 1.0)
    for bad in (-1.0, float("nan"), float("inf"), "1", None, True, [1.0]):
        with pytest.raises(ValueError, match="PlaneFlux: flux"):
            PlaneFlux("-x", bad)
    for bad in (-1, 16, 1.0, "0", None, True):
        with pytest.raises(ValueError, match="PlaneFlux: spectrum"):
            PlaneFlux("-x", 1.0, bad)
    # the keyword: off, one, several
    assert plane_flux_spec(None, "t") == () and plane_flux_spec([], "t") == () and plane_flux_spec((), "t", use_gpu=False) == ()
    assert plane_flux_spec(f, "t") == (f,)
    both = plane_flux_spec([PlaneFlux("-x", 1.0), f], "t", True, lambda: 2)
    assert both == (PlaneFlux("-x", 1.0), f)
    for bad in (1.0, "-x", ("-x", 1.0), [("-x", 1.0)], {"face": 0}, [f, None]):
        with pytest.raises(ValueError, match="plane_flux"):
            plane_flux_spec(bad, "t")
    with pytest.raises(ValueError, match="twice"):
        plane_flux_spec([PlaneFlux("-x", 1.0), PlaneFlux(0, 2.0)], "t")
    with pytest.raises(ValueError, match="use_gpu=True"):
        plane_flux_spec(f, "t", use_gpu=False)
    with pytest.raises(ValueError, match="table set"):
        plane_flux_spec(f, "t", True, lambda: 1)                       # spectrum 1 with one set on the device
    broken = PlaneFlux("-x", 1.0)
    broken.flux = -1.0                                                  # (assigned behind the constructor)
    with pytest.raises(ValueError, match="PlaneFlux: flux"):
        plane_flux_spec(broken, "t")


def test_capi_symbols_and_header():
    from pyc2ray_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "asora_hip.h")).read()
    assert "int asora_plane_flux(int count, const int32_t *face, const double *flux, const int32_t *spectrum);" in header
    assert "int asora_get_plane_flux(int *count, int32_t *face, double *flux, int32_t *spectrum);" in header
    assert {"asora_plane_flux", "asora_get_plane_flux"} <= set(_capi.SIGNATURES)
    lib = _capi.load()                    # (opening the library resolves every declared symbol)
    # the state exists without a device: "off" is accepted and read back, bad values are code 3, faces want a device
    assert lib.asora_plane_flux(0, None, None, None) == 0
    n = C.c_int(7)
    assert lib.asora_get_plane_flux(C.byref(n), None, None, None) == 0 and n.value == 0
    face = lambda *v: np.array(v, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    flux = lambda *v: np.array(v, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    assert lib.asora_plane_flux(7, face(*range(7)), flux(*[1.0] * 7), None) == 3
    assert lib.asora_plane_flux(-1, None, None, None) == 3
    assert lib.asora_plane_flux(1, face(6), flux(1.0), None) == 3
    assert lib.asora_plane_flux(1, face(-1), flux(1.0), None) == 3
    assert lib.asora_plane_flux(2, face(2, 2), flux(1.0, 1.0), None) == 3
    for bad in (-1.0, float("nan"), float("inf")):
        assert lib.asora_plane_flux(1, face(0), flux(bad), None) == 3
    assert lib.asora_plane_flux(1, face(0), flux(1.0), face(16)) == 3
    assert lib.asora_plane_flux(1, None, flux(1.0), None) == 3
    assert b"plane_flux" in lib.asora_last_error()
    assert lib.asora_get_plane_flux(C.byref(n), None, None, None) == 0 and n.value == 0


def _evolve_args(N=4, nsrc=1):
    g = np.ones((N, N, N))
    return (1.0, 1.0, np.ones(nsrc), np.ones((3, nsrc)), True, 10, N, 0.01, g, g, g, np.ones(5), np.ones(5), -20.0, 0.1, 4.0, 1e-4, 1e-18,
            1.0, 1.0, 1.0, 1.0, 1.0)


def test_bad_plane_flux_is_refused_before_the_library_is_touched(monkeypatch):
    import pyc2ray_amd as pc2r
    from pyc2ray_amd.planeflux import PlaneFlux
    _install(monkeypatch, SB.Untouchable())
    a = _evolve_args()
    ok = PlaneFlux("-x", 1.0)
    for bad in (1.0, "-x", [("-x", 1.0)], [ok, PlaneFlux(0, 2.0)]):
        with pytest.raises(ValueError, match="plane_flux"):
            pc2r.evolve3D(*a, quiet=True, logfile=None, plane_flux=bad)
        with pytest.raises(ValueError, match="plane_flux"):
            pc2r.evolve3D_MPI(*a[:8], None, None, 0, 2, *a[8:], quiet=True, logfile=None, plane_flux=bad)
        with pytest.raises(ValueError, match="plane_flux"):
            pc2r.evolve3D_resident(a[0], a[1], a[2], a[3], {}, 4, np.ones(5), *a[13:], quiet=True, logfile=None, plane_flux=bad)
        with pytest.raises(ValueError, match="plane_flux"):
            pc2r.do_raytracing(a[1], a[2], a[3], True, 10, 4, 0.01, a[9], a[10], a[11], a[12], None, None, -20.0, 0.1, 4.0, 1e-18,
                               quiet=True, logfile=None, plane_flux=bad)
    # use_gpu=False has no faces
    with pytest.raises(ValueError, match="use_gpu=True"):
        pc2r.evolve3D(*a[:4], False, *a[5:], quiet=True, logfile=None, plane_flux=ok)
    with pytest.raises(ValueError, match="use_gpu=True"):
        pc2r.evolve3D_MPI(*a[:4], False, *a[5:8], None, None, 0, 2, *a[8:], quiet=True, logfile=None, plane_flux=[ok])
    with pytest.raises(ValueError, match="use_gpu=True"):
        pc2r.do_raytracing(a[1], a[2], a[3], False, 10, 4, 0.01, a[9], a[10], a[11], a[12], None, None, -20.0, 0.1, 4.0, 1e-18,
                           quiet=True, logfile=None, plane_flux=ok)


@pytest.mark.parametrize("entry", ["evolve3D", "evolve3D_resident", "do_raytracing"])
@pytest.mark.parametrize("nsrc", [1, 0])
def test_state_is_set_before_the_loop_and_cleared_whatever_happens(monkeypatch, tmp_path, entry, nsrc):
    """The stand-in's evolve_begin / raytrace_device raise: the step ends where its loop would begin, and the finally has run.
    nsrc = 0: an empty source list is accepted with faces."""
    import pyc2ray_amd as pc2r
    from pyc2ray_amd.planeflux import PlaneFlux
    a = _evolve_args(nsrc=nsrc)
    faces = [PlaneFlux("-x", 2.0), PlaneFlux("+z", 0.5, 0)]

    def run(plane_flux, log):
        lib = _install(monkeypatch, SB.Recorder())
        kw = dict(quiet=True, logfile=str(log))
        if plane_flux is not False:
            kw["plane_flux"] = plane_flux
        with pytest.raises(SB.Stop):
            if entry == "evolve3D":
                pc2r.evolve3D(*a, **kw)
            elif entry == "evolve3D_resident":
                pc2r.evolve3D_resident(a[0], a[1], a[2], a[3], {0: a[9], 3: a[8], 4: a[10]}, 4, np.ones(5), *a[13:], **kw)
            else:
                pc2r.do_raytracing(a[1], a[2], a[3], True, 10, 4, 0.01, a[9], a[10], a[11], a[12], None, None, -20.0, 0.1, 4.0,
                                   1e-18, **kw)
        return lib, open(log).read()

    lib, text = run(faces, tmp_path / "on.log")
    names = lib.names()
    sets = [c[1] for c in lib.calls if c[0] == "plane_flux"]
    assert [tuple(map(list, s)) for s in sets] == [([0, 5], [2.0, 0.5], [0, 0]), ([], [], [])]      # set once, cleared in the finally
    assert names.index("plane_flux") < next(i for i, n in enumerate(names) if n in ("evolve_begin", "raytrace_device"))
    assert names[-1] == "plane_flux"
    assert text.count("Plane-parallel flux through the -x face: 2.000e+00") == 1 and text.count("through the +z face") == 1
    sources = [c[1] for c in lib.calls if c[0] == "source_data_to_device"]
    assert len(sources) == 1 and sources[0][2] == nsrc and sources[0][0].shape == (3 * nsrc,)
    if entry != "do_raytracing":
        begin = next(c[1] for c in lib.calls if c[0] == "evolve_begin")
        assert begin[13] == nsrc and begin[14] == min(int(1e-4 * 64), (nsrc + 2 - 1) / 3)      # the faces count as sources
    if nsrc == 0:
        return
    # off (no keyword, None, empty): the library never hears of it and the log is the log without the feature
    logs = []
    for k, off in enumerate((False, None, [])):
        lib, text_off = run(off, tmp_path / f"off{k}.log")
        assert "plane_flux" not in lib.names() and "Plane-parallel" not in text_off
        logs.append(text_off)
        if entry != "do_raytracing":
            assert next(c[1] for c in lib.calls if c[0] == "evolve_begin")[14] == min(int(1e-4 * 64), 0 / 3)
    assert logs[0] == logs[1] == logs[2]
    strip = lambda t: "".join(line for line in t.splitlines(True) if "Plane-parallel" not in line and "Convergence Criterion" not in line)
    assert strip(text) == strip(logs[0])


class _Comm:
    """A communicator that is nothing but distributed: the step takes the three-call loop."""


@pytest.mark.parametrize("rank", [0, 1])
def test_only_rank_zero_holds_the_faces(monkeypatch, rank):
    import pyc2ray_amd as pc2r
    from pyc2ray_amd.planeflux import PlaneFlux
    a = _evolve_args(nsrc=2)
    lib = _install(monkeypatch, SB.Recorder())
    with pytest.raises(SB.Stop):
        pc2r.evolve3D_MPI(*a[:8], object(), _Comm(), rank, 2, *a[8:], quiet=True, logfile=None, plane_flux=PlaneFlux("+x", 3.0))
    sets = [tuple(map(list, c[1])) for c in lib.calls if c[0] == "plane_flux"]
    assert sets == ([([1], [3.0], [0]), ([], [], [])] if rank == 0 else [])
    assert lib.names()[-2 if rank == 0 else -1] in ("raytrace_device", "plane_flux")
    assert "raytrace_device" in lib.names()                          # (the three-call loop, on both ranks)


def test_loop_strategy_with_faces():
    from pyc2ray_amd.evolve import _loop_strategy
    from pyc2ray_amd.planeflux import PlaneFlux

    class Lib:
        def get_option(self, which):
            return 1

        def evolve_slab_fold_all(self):
            pass

    class Slab:
        exchange, overlap, device_loop = "slab", False, True

        def slab_enqueue(self):
            pass

        def reduce_begin(self):
            pass

    faces = (PlaneFlux("-x", 1.0),)
    said = []
    assert _loop_strategy(Lib(), Slab(), True) == "slab"
    assert _loop_strategy(Lib(), Slab(), True, (), said.append) == "slab" and said == []
    assert _loop_strategy(Lib(), Slab(), True, faces, said.append) == "all-reduce"
    assert len(said) == 1 and "all-reduce" in said[0] and "plane_flux" in said[0]
    assert _loop_strategy(Lib(), Slab(), False, faces) == "one GPU"

    class AllReduce(Slab):
        exchange = "allreduce"

    class Pipelined(Slab):
        exchange, overlap = "allreduce", True

        def raytrace_and_allreduce(self):
            pass

    for comm, want in ((AllReduce(), "all-reduce"), (Pipelined(), "pipelined"), (_Comm(), "three calls")):
        assert _loop_strategy(Lib(), comm, True, faces) == _loop_strategy(Lib(), comm, True) == want


def test_yaml_keys_and_the_attribute(tmp_path, monkeypatch):
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.c2ray_base as B
    from pyc2ray_amd.planeflux import PlaneFlux
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        plain = pc2r.C2Ray_Test(PLAIN_PARAMS, 8, False)
        assert plain.plane_flux == () and "Plane-parallel" not in open(plain.logfile).read()
        # faces on an object without use_gpu: refused where the file is read, and at the assignment
        with pytest.raises(ValueError, match="Photo: plane_flux: plane_flux needs use_gpu=True"):
            pc2r.C2Ray_Test(PLANE_PARAMS, 8, False)
        with pytest.raises(ValueError, match="C2Ray.plane_flux: plane_flux needs use_gpu=True"):
            plain.plane_flux = PlaneFlux("-x", 1.0)
        plain.plane_flux = None
        assert plain.plane_flux == ()
        # an object with use_gpu (as one constructed with use_gpu=True has it) reading the file's keys
        def with_keys(path):
            sim = pc2r.C2Ray_Test(PLAIN_PARAMS, 8, False)
            sim.gpu = True
            sim._read_paramfile(path)
            sim._plane_flux_init()
            return sim
        sim = with_keys(PLANE_PARAMS)
        assert sim.plane_flux == (PlaneFlux("-x", 2.0e6 / 1e48), PlaneFlux("+z", 1.0e6 / 1e48))
        text = open(sim.logfile).read()
        assert "Plane-parallel flux through the -x face: 2.000e+06 photons/s/cm^2" in text and "through the +z face: 1.000e+06" in text
        sim.plane_flux = PlaneFlux("+y", 1.0)
        assert sim.plane_flux == (PlaneFlux(3, 1.0),)
        for bad in (1.0, "-x", [PlaneFlux(0, 1.0), PlaneFlux("-x", 2.0)]):
            with pytest.raises(ValueError, match="plane_flux"):
                sim.plane_flux = bad
        assert sim.plane_flux == (PlaneFlux(3, 1.0),)                     # (a refused assignment changes nothing)
        sim.plane_flux = []
        assert sim.plane_flux == ()
        # scalars for one face; keys that do not fit together
        body = open(PLAIN_PARAMS).read()
        keys = lambda extra: body.replace("  R_max_cMpc: 15.0\n", "  R_max_cMpc: 15.0\n" + extra)
        with open("p.yml", "w") as f:
            f.write(keys("  plane_flux_face: '+x'\n  plane_flux: 3.0e5\n  plane_flux_spectrum: 0\n"))
        assert with_keys("p.yml").plane_flux == (PlaneFlux(1, 3.0e5 / 1e48),)
        for extra, what in (("  plane_flux_face: '+x'\n", "come together"), ("  plane_flux: 1.0\n", "come together"),
                            ("  plane_flux_face: ['+x', '-x']\n  plane_flux: 1.0\n", "one length"),
                            ("  plane_flux_face: '+w'\n  plane_flux: 1.0\n", "PlaneFlux: face"),
                            ("  plane_flux_face: ['+x', '+x']\n  plane_flux: [1.0, 1.0]\n", "twice"),
                            ("  plane_flux_face: '+x'\n  plane_flux: -1.0\n", "PlaneFlux: flux"),
                            ("  plane_flux_face: '+x'\n  plane_flux: 'many'\n", "Photo: plane_flux must be a number")):
            with open("p.yml", "w") as f:
                f.write(keys(extra))
            with pytest.raises(ValueError, match=what):
                with_keys("p.yml")
    finally:
        os.chdir(cwd)


def test_the_class_hands_the_attribute_to_every_entry(tmp_path, monkeypatch):
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.c2ray_base as B
    from pyc2ray_amd.planeflux import PlaneFlux
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        sim = pc2r.C2Ray_Test(PLAIN_PARAMS, 8, False)
        sim.gpu = True                                     # (as an object constructed with use_gpu=True has it)
        sim.plane_flux = [PlaneFlux("-x", 2.0e6 / 1e48), PlaneFlux("+z", 1.0e6 / 1e48)]
        seen = []

        def spy(name, result):
            def f(*args, **kw):
                seen.append((name, kw.get("plane_flux", "absent")))
                return result
            return f
        N = 8
        monkeypatch.setattr(B, "evolve3D", spy("evolve3D", (np.zeros((N, N, N)), np.zeros((N, N, N)))))
        monkeypatch.setattr(B, "evolve3D_resident", spy("evolve3D_resident", 1))
        monkeypatch.setattr(B, "do_raytracing", spy("do_raytracing", (np.zeros((N, N, N)), None)))
        flux, pos = np.ones(1), np.ones((3, 1), dtype=int)
        sim.device_resident = False
        sim.evolve3D(1.0, flux, pos)
        sim.do_raytracing(flux, pos)
        sim.plane_flux = PlaneFlux("-y", 4.0)
        sim.evolve3D(1.0, np.zeros(0), np.zeros((3, 0), dtype=int))          # (an empty source list reaches the entry as it is)
        want = (PlaneFlux("-x", 2.0e6 / 1e48), PlaneFlux("+z", 1.0e6 / 1e48))
        assert seen == [("evolve3D", want), ("do_raytracing", want), ("evolve3D", (PlaneFlux("-y", 4.0),))]
    finally:
        os.chdir(cwd)
