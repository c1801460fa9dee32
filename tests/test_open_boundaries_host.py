"""CPU: the host side of the open boundaries: the ``periodic=`` keyword's checks, on a stand-in for the
library that the option is set before the first library call of the step and restored after it whatever happens, the YAML key
and the attribute of the simulation class, the option in the C-ABI."""
import os

import numpy as np
import pytest

import open_boundary_standin_backend as SB

HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_test.yml")
OPT = 18
ENTRIES = ["evolve3D", "evolve3D_MPI", "evolve3D_resident", "do_raytracing"]


def _evolve_args(N=4):
    g = np.ones((N, N, N))
    return (1.0, 1.0, np.ones(1), np.ones((3, 1)), True, 10, N, 0.01, g, g, g, np.ones(5), np.ones(5), -20.0, 0.1, 4.0, 1e-4, 1e-18,
            1.0, 1.0, 1.0, 1.0, 1.0)


def _call(pc2r, entry, use_gpu=True, **kw):
    a = _evolve_args()
    kw = dict(quiet=True, logfile=None, **kw)
    if entry == "evolve3D":
        return pc2r.evolve3D(*a[:4], use_gpu, *a[5:], **kw)
    if entry == "evolve3D_MPI":
        return pc2r.evolve3D_MPI(*a[:4], use_gpu, *a[5:8], None, None, 0, 1, *a[8:], **kw)
    if entry == "evolve3D_resident":
        return pc2r.evolve3D_resident(a[0], a[1], a[2], a[3], {0: a[9], 3: a[8], 4: a[10]}, 4, np.ones(5), *a[13:], **kw)
    return pc2r.do_raytracing(a[1], a[2], a[3], use_gpu, 10, 4, 0.01, a[9], a[10], a[11], a[12], None, None, -20.0, 0.1, 4.0, 1e-18, **kw)


def test_periodic_spec():
    from pyc2ray_amd.boundaries import periodic_spec
    assert periodic_spec(True, "t") is True and periodic_spec(False, "t") is False
    assert periodic_spec(np.bool_(False), "t") is False and periodic_spec(True, "t", use_gpu=False) is True
    for bad in (0, 1, None, "no", 0.0, [False], np.int32(0)):
        with pytest.raises(ValueError, match="periodic must be True or False"):
            periodic_spec(bad, "t")
    with pytest.raises(ValueError, match="use_gpu=False.*sub-box"):
        periodic_spec(False, "t", use_gpu=False)


@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_values_are_refused_before_the_library_is_touched(monkeypatch, entry):
    import pyc2ray_amd as pc2r
    SB.install(monkeypatch, SB.Untouchable())
    for bad in (0, 1, None, "open", np.zeros(1)):
        with pytest.raises(ValueError, match=f"{entry}: periodic must be True or False"):
            _call(pc2r, entry, periodic=bad)
    if entry != "evolve3D_resident":                 # (which has no use_gpu=False form)
        with pytest.raises(ValueError, match=f"{entry}: periodic=False needs use_gpu=True.*sub-box"):
            _call(pc2r, entry, use_gpu=False, periodic=False)


@pytest.mark.parametrize("stop", [True, False])
@pytest.mark.parametrize("entry", ENTRIES)
def test_option_is_set_first_and_restored_whatever_happens(monkeypatch, entry, stop):
    """stop: the library fails where the work of the step begins; else the step runs through."""
    import pyc2ray_amd as pc2r
    lib = SB.install(monkeypatch, SB.Recorder(stop=stop))
    if stop:
        with pytest.raises(SB.Stop):
            _call(pc2r, entry, periodic=False)
    else:
        _call(pc2r, entry, periodic=False)
    sets = [(i, c[1]) for i, c in enumerate(lib.calls) if c[0] == "set_option" and c[1][0] == OPT]
    assert [s[1] for s in sets] == [(OPT, 1), (OPT, 0)]
    assert sets[0][0] == 0 and sets[1][0] == len(lib.calls) - 1          # the first and the last thing the library hears
    work = next(i for i, n in enumerate(lib.names()) if n in ("evolve_begin", "raytrace_device"))
    assert sets[0][0] < work < sets[1][0]
    # periodic (no keyword, True): the library never hears of the option
    for kw in ({}, {"periodic": True}):
        lib = SB.install(monkeypatch, SB.Recorder(stop=stop))
        if stop:
            with pytest.raises(SB.Stop):
                _call(pc2r, entry, **kw)
        else:
            _call(pc2r, entry, **kw)
        assert not [c for c in lib.calls if c[0] == "set_option" and c[1][0] == OPT]


def test_restored_after_the_other_opt_ins_states(monkeypatch):
    """With lls= and clumping= as well: each of the three states is set once and put back once."""
    import pyc2ray_amd as pc2r
    from pyc2ray_amd.lls import LLSOpacity
    lib = SB.install(monkeypatch, SB.Recorder(stop=True))
    with pytest.raises(SB.Stop):
        _call(pc2r, "evolve3D", periodic=False, lls=LLSOpacity(1e-6), clumping=2.0)
    assert [c[1] for c in lib.calls if c[0] == "set_option" and c[1][0] == OPT] == [(OPT, 1), (OPT, 0)]
    assert [c[1] for c in lib.calls if c[0] == "lls_opacity"] == [(1e-6, 0.0), (0.0, 0.0)]
    assert [c[1][0] for c in lib.calls if c[0] == "clumping"] == [1, 0]
    assert lib.names()[0] == "set_option" and lib.names()[-3:] == ["set_option", "lls_opacity", "clumping"]


def test_c2ray_class_key_and_attribute(tmp_path):
    import pyc2ray_amd as pc2r
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        plain = pc2r.C2Ray_Test(PLAIN_PARAMS, 8, False)
        assert plain.periodic is True                                              # the key is absent: 1
        assert "boundaries" not in open(plain.logfile).read()
        text = open(PLAIN_PARAMS).read().rstrip("\n")
        with open("p.yml", "w") as f:
            f.write(text + "\n  periodic: 1\n")
        sim = pc2r.C2Ray_Test("p.yml", 8, False)
        assert sim.periodic is True and "boundaries" not in open(sim.logfile).read()
        # 0 on an object without use_gpu: refused where the file is read, not at the first step
        with open("p.yml", "w") as f:
            f.write(text + "\n  periodic: 0\n")
        with pytest.raises(ValueError, match="Raytracing: periodic: 0: periodic=False needs use_gpu=True"):
            pc2r.C2Ray_Test("p.yml", 8, False)
        for bad in ("2", "-1", "0.5", "open", "[0]"):
            with open("p.yml", "w") as f:
                f.write(text + f"\n  periodic: {bad}\n")
            with pytest.raises(ValueError, match="Raytracing: periodic must be 0 or 1"):
                pc2r.C2Ray_Test("p.yml", 8, False)
        # assignable between steps; what evolve3D would refuse is refused at the assignment
        with pytest.raises(ValueError, match="C2Ray.periodic: periodic=False needs use_gpu=True"):
            plain.periodic = False
        assert plain.periodic is True
        plain.gpu = True                                   # (as an object constructed with use_gpu=True has it)
        plain.periodic = False
        assert plain.periodic is False
        plain.periodic = True
        assert plain.periodic is True
        for bad in (0, 1, None, "no"):
            with pytest.raises(ValueError, match="C2Ray.periodic: periodic must be True or False"):
                plain.periodic = bad
        assert plain.periodic is True
    finally:
        os.chdir(cwd)


def test_c2ray_class_passes_the_attribute(monkeypatch, tmp_path):
    """evolve3D (host grids and device-resident), evolve3D_MPI and do_raytracing of the class hand `periodic` on."""
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.c2ray_base as B
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        sim = pc2r.C2Ray_Test(PLAIN_PARAMS, 8, False)
        seen = []

        def spy(name, result):
            def f(*args, **kw):
                seen.append((name, kw.get("periodic", "absent")))
                return result
            return f
        g = np.zeros((8, 8, 8))
        monkeypatch.setattr(B, "evolve3D", spy("evolve3D", (g, g)))
        monkeypatch.setattr(B, "evolve3D_MPI", spy("evolve3D_MPI", (g, g)))
        monkeypatch.setattr(B, "evolve3D_resident", spy("evolve3D_resident", 1))
        monkeypatch.setattr(B, "do_raytracing", spy("do_raytracing", (g, None)))
        flux, pos = np.ones(2), np.ones((3, 2), dtype=int)
        for value in (False, True):
            sim.gpu = True
            sim.periodic = value
            sim.mpi, sim.gpu = False, False
            sim.evolve3D(1.0, flux, pos)
            sim.do_raytracing(flux, pos)
            sim.mpi, sim.comm, sim.nprocs = object(), None, 2
            sim.evolve3D(1.0, flux, pos)
            sim.mpi, sim.gpu, sim.device_resident = False, True, True
            monkeypatch.setattr(B._residency, "reclaim", lambda **kw: None)
            monkeypatch.setattr(B._residency, "register", lambda obj: None)
            sim.evolve3D(1.0, flux, pos)
            sim._device_newer.clear()                       # (nothing ran: there is nothing to fetch from a device)
        assert seen == [(n, v) for v in (False, True) for n in ("evolve3D", "do_raytracing", "evolve3D_MPI", "evolve3D_resident")]
    finally:
        os.chdir(cwd)


def test_capi_option_and_header():
    from pyc2ray_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "asora_hip.h")).read()
    assert "ASORA_OPT_OPEN_BOUNDARIES = 18," in header and "ASORA_OPT_COUNT = 19" in header
    assert "ASORA_VARIANT_OPEN_BOUNDARIES = 64" in header
    assert _capi.OPT_OPEN_BOUNDARIES == OPT
    lib = _capi.load()
    # the option exists without a device: periodic by default, set and read back, and the next number is unknown
    assert lib.asora_get_option(OPT) == 0
    assert lib.asora_set_option(OPT, 1) == 0 and lib.asora_get_option(OPT) == 1
    assert lib.asora_set_option(OPT, 0) == 0 and lib.asora_get_option(OPT) == 0
    assert lib.asora_set_option(OPT + 1, 1) == 3 and lib.asora_get_option(OPT + 1) == -1
