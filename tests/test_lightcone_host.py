"""CPU: the host side of the light cone: the C-ABI symbols and the enums the header pins, the chunking, the
plane order and the orientations of LightCone on a numpy stand-in for the library, what make_lightcone refuses before the library
is touched, and the wiring of the class -- its keys, and the redshift it takes for a state."""
import importlib
import os

import numpy as np
import pytest

import lightcone_reference as R
import lightcone_standin_backend as LB

HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_test.yml")
CONE_PARAMS = os.path.join(HERE, "data", "parameters_lightcone.yml")


@pytest.fixture(scope="module", autouse=True)
def no_leftover_device():
    """As in tests/test_powerspec_host.py: the code-2 check below needs a library without a device."""
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    lib = _capi.load()
    if lib.asora_device_ptr(_capi.GRID_NDENS) and not p.cuda_is_init():
        assert lib.asora_device_close() == 0
    yield


def _module():
    return importlib.import_module("pyc2ray_amd.lightcone")


def _install(monkeypatch, backend, ready=True):
    import pyc2ray_amd.c2ray_base as B
    for mod in (_module(), B):
        monkeypatch.setattr(mod, "load_asora", lambda: backend)
        monkeypatch.setattr(mod, "cuda_is_init", lambda: ready)
    return backend


def _cosmology():
    from pyc2ray_amd.c2ray_base import FlatLambdaCDMLite
    return FlatLambdaCDMLite(70.0, 0.27, 2.726, Ob0=0.044)


def test_capi_symbols_and_header():
    from pyc2ray_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "asora_hip.h")).read()
    assert "enum { ASORA_LC_SLOTS = 4, ASORA_LC_MAX_SLICES = 1024, ASORA_LC_STAGES = 4 };" in header
    assert "int asora_lightcone_advance(int slot, int kind, int src_grid, double t_gamma, int los_axis,\n" in header
    assert "int asora_lightcone_state(int slot, int *has_prev, int *kind, int *src_grid);" in header
    assert "int asora_lightcone_reset(int slot);" in header
    assert "int asora_debug_lightcone_ms(double *ms /* [ASORA_LC_STAGES] */);" in header
    assert (_capi.LC_SLOTS, _capi.LC_MAX_SLICES, _capi.LC_STAGES) == (4, 1024, 4) and _module().MAX_SLICES == 1024
    assert (R.XH, R.XHI, R.DENSITY, R.HI) == (_capi.PS_XH, _capi.PS_XHI, _capi.PS_DENSITY, _capi.PS_HI)
    # the enums the header pins keep their values: a kept field is no grid, no kernel slot or option is new
    for pinned in ("ASORA_GRID_COUNT = 9", "ASORA_PS_KINDS = 4", "ASORA_KERNEL_COUNT = 4", "ASORA_KERNEL_SLOTS = 7", "ASORA_OPT_COUNT = 19",
                   "ASORA_LYA_STAGES = 4", "ASORA_BISPEC_STAGES = 9"):
        assert pinned in header, pinned
    assert [len(_capi.SIGNATURES[name][1]) for name in ("asora_lightcone_advance", "asora_lightcone_state", "asora_lightcone_reset",
                                                        "asora_debug_lightcone_ms")] == [12, 4, 1, 1]
    lib = _capi.load()                    # (opening the library resolves every declared symbol)
    if not lib.asora_device_ptr(_capi.GRID_NDENS):      # no device initialised in this process: refused as every entry is
        planes, w, slices, moments = np.zeros(2, dtype=np.int32), np.ones(2), np.full((2, 4, 4), 9.0), np.full(4, 9.0)
        rc = lib.asora_lightcone_advance(0, 0, -1, 0.0, 2, 2, _capi.iptr(planes), _capi.dptr(w), _capi.dptr(w), 0, _capi.dptr(slices),
                                         _capi.dptr(moments))
        assert rc == 2 and b"lightcone_advance" in lib.asora_last_error()
        assert np.all(slices == 9.0) and np.all(moments == 9.0)
    # the state of a slot is host bookkeeping: readable without a device, and nothing is kept there
    import ctypes as C
    has, kind, src = C.c_int(7), C.c_int(7), C.c_int(7)
    for slot in range(_capi.LC_SLOTS):
        assert lib.asora_lightcone_state(slot, C.byref(has), C.byref(kind), C.byref(src)) == 0
        if not lib.asora_device_ptr(_capi.GRID_NDENS):
            assert (has.value, kind.value, src.value) == (0, 0, -1)
    assert lib.asora_lightcone_state(_capi.LC_SLOTS, C.byref(has), C.byref(kind), C.byref(src)) == 3
    assert lib.asora_lightcone_state(-1, C.byref(has), C.byref(kind), C.byref(src)) == 3
    assert lib.asora_lightcone_state(0, None, C.byref(kind), C.byref(src)) == 3
    assert lib.asora_lightcone_reset(_capi.LC_SLOTS) == 3 and lib.asora_lightcone_reset(-1) == 3
    ms = np.full(4, -1.0)
    assert lib.asora_debug_lightcone_ms(_capi.dptr(ms)) == 0 and np.all(ms >= 0.0)
    assert lib.asora_debug_lightcone_ms(None) == 3


def _states(N, count, seed=5):
    rng = np.random.default_rng(seed)
    return [rng.random((N, N, N)) for _ in range(count)]


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_chunks_planes_and_orientations(monkeypatch, axis):
    """A stand-in limit of 5 slices per call forces the split: no call is larger, the field is refreshed by the last call of a step
    and by no other, a step that crosses nothing makes the one call that refreshes.  The cone equals the plain-Python builder's."""
    M = _module()
    from pyc2ray_amd import _capi
    monkeypatch.setattr(M, "MAX_SLICES", 5)
    N, first_plane = 6, 4
    cosmo = _cosmology()
    dchi = 0.5
    z_all = M.slice_redshifts(cosmo, 9.0, 8.9, dchi)
    assert z_all.size > 4 * N
    # states: the first, one 13 slices on (three calls: 5, 5, 3), one that crosses none, one 2 on, the rest in one go
    mid = lambda m: 0.5 * (z_all[m] + z_all[m + 1])
    z_states = [9.0, mid(12), mid(12) - 1e-7, mid(14), 8.9]
    fields = _states(N, len(z_states))
    lib = LB.Numpy(N, max_slices=5)
    cone = M.LightCone(N, cosmo, 9.0, dchi, kind="xh", los_axis=axis, first_plane=first_plane, slot=2, z_end=8.9)
    steps = []
    for i, (z, g) in enumerate(zip(z_states, fields)):
        lib.grid_to_device(_capi.GRID_XH, g)
        steps.append(cone.advance(lib, None if i == 0 else z_states[i - 1], z))
    calls = [c for c in lib.calls if c[0] == "lightcone_advance"]
    sizes = [len(c[1][5]) for c in calls]
    refresh = [bool(c[1][8]) for c in calls]
    rest = z_all.size - 15
    tail = [5] * (rest // 5) + ([rest % 5] if rest % 5 else [])
    assert sizes == [0, 5, 5, 3, 0, 2] + tail and max(sizes) <= 5
    assert refresh == [True, False, False, True, True, True] + [False] * (len(tail) - 1) + [True]
    assert lib.names().count("lightcone_reset") == 1 and lib.names().index("lightcone_reset") < lib.names().index("lightcone_advance")
    assert all(c[1][:5] == (2, _capi.PS_XH, None, 0.0, axis) for c in calls)
    assert [s.n_slices for s in steps] == [0, 13, 0, 2, rest] and steps[0].stored_only and not steps[2].stored_only
    assert "kept" in steps[0].log_line() and "crossed no slice" in steps[2].log_line() and "13 slices from 0" in steps[1].log_line()
    # consecutive slices are consecutive planes, descending from first_plane, wrapping through 0
    planes = np.concatenate([np.asarray(c[1][5], dtype=np.int64) for c in calls])
    assert np.array_equal(planes, (first_plane - np.arange(z_all.size)) % N) and np.array_equal(planes, cone.planes(0, z_all.size))
    # every slice once, at its redshift; the cube is the reference builder's, bit for bit
    assert cone.n_slices == z_all.size and cone.z.tobytes() == z_all.tobytes()
    cube, emitted_by = R.build_cone(fields, z_states, list(z_all), first_plane=first_plane, axis=axis)
    assert cone.array().tobytes() == cube.tobytes() and cone.array("run").shape == (z_all.size, N, N)
    assert np.bincount(emitted_by, minlength=5).tolist() == [0, 13, 0, 2, rest]
    assert cone.array("distance").tobytes() == np.ascontiguousarray(cube[::-1]).tobytes()
    with pytest.raises(ValueError, match="LightCone.array: order must be 'run' or 'distance'"):
        cone.array("z")
    # the moments give the global signal along the cone
    assert np.allclose(cone.mean, cube.mean(axis=(1, 2)), rtol=1e-13) and np.allclose(cone.variance, cube.var(axis=(1, 2)), rtol=1e-9)
    assert steps[3].mean.tobytes() == cone.mean[13:15].tobytes() and steps[3].first == 13
    # chunk: N slices make a periodic box, every slice in the plane it was taken from, the line of sight along los_axis
    for m0 in (0, 3, N + 1):
        vol = cone.chunk(m0)
        assert vol.shape == (N, N, N) and vol.flags.c_contiguous
        for m in range(m0, m0 + N):
            assert np.take(vol, (first_plane - m) % N, axis=axis).tobytes() == cube[m].tobytes()
    part = cone.chunk(2, 3)
    assert part.shape[axis] == 3 and np.take(part, 0, axis=axis).tobytes() == cube[4].tobytes()
    assert np.take(part, 2, axis=axis).tobytes() == cube[2].tobytes()
    for m0, n in ((-1, 2), (0, 0), (z_all.size - 2, 3), (0.5, 2)):
        with pytest.raises(ValueError, match="LightCone.chunk: "):
            cone.chunk(m0, n)
    # the run goes down in redshift
    with pytest.raises(ValueError, match="LightCone.advance: the run goes from high to low redshift"):
        cone.advance(lib, 8.9, 8.95)


def test_save_scale_and_a_cone_without_slices(monkeypatch, tmp_path):
    M = _module()
    from pyc2ray_amd import _capi
    N = 4
    cosmo = _cosmology()
    z_states = [8.0, 7.99, 7.98]
    triples = [R.fields(N, 10 + i) for i in range(3)]
    scale = lambda z: 2.0 + z
    cones = {}
    for keep in (True, False):
        lib = LB.Numpy(N)
        cone = M.LightCone(N, cosmo, 8.0, 0.4, kind="dtb", los_axis=1, keep=keep)
        for i, (x, n, T) in enumerate(triples):
            for which, g in ((_capi.GRID_XH, x), (_capi.GRID_NDENS, n), (_capi.GRID_TEMP, T)):
                lib.grid_to_device(which, g)
            cone.advance(lib, None if i == 0 else z_states[i - 1], z_states[i], scale=scale, t_gamma=3.0 * (1 + z_states[i]))
        cones[keep] = (cone, lib)
    cone, lib = cones[True]
    formed = [R.form(R.HI, x, n, T, float(np.mean(n)), 3.0 * (1 + z)) for (x, n, T), z in zip(triples, z_states)]
    cube, _ = R.build_cone(formed, z_states, list(cone.z), axis=1, scale=scale)
    assert cone.n_slices > 5 and cone.array().tobytes() == cube.tobytes()
    assert all(c[1][1] == _capi.PS_HI for c in lib.calls if c[0] == "lightcone_advance")
    bare, lib_bare = cones[False]
    assert all(c[2]["slices"] is False for c in lib_bare.calls if c[0] == "lightcone_advance")
    assert bare.moments.tobytes() == cone.moments.tobytes() and bare.z.tobytes() == cone.z.tobytes()
    with pytest.raises(ValueError, match="keeps no slices"):
        bare.array()
    path = str(tmp_path / "cone.npz")
    cone.save(path)
    with np.load(path) as f:
        assert f["slices"].tobytes() == cube.tobytes() and f["z"].tobytes() == cone.z.tobytes() and str(f["kind"]) == "dtb"
        assert (int(f["los_axis"]), int(f["first_plane"]), float(f["dchi"])) == (1, 0, 0.4) and f["mean"].shape == (cone.n_slices,)
    bare.save(path)
    with np.load(path) as f:
        assert "slices" not in f.files and f["variance"].shape == (cone.n_slices,)
    assert "slices of 4 x 4" in repr(cone)


def test_make_lightcone_forms_and_refusals(monkeypatch):
    M = _module()
    from pyc2ray_amd import _capi, _residency
    N = 5
    cosmo = _cosmology()
    lib = _install(monkeypatch, LB.Numpy(N))

    class Holder:
        left = 0

        def _leave_device(self):
            Holder.left += 1
    holder = Holder()
    _residency.register(holder)
    fields = _states(N, 3)
    zs = [7.0, 6.995, 6.99]
    good = dict(fields=fields, redshifts=zs, kind="xhi", los_axis=0, box_len_mpc=2.0, cosmology=cosmo, first_plane=3, slot=1)
    cone = M.make_lightcone(**good)
    assert Holder.left == 3                   # (every upload overwrites a grid someone may keep on the device)
    assert lib.names() == ["grid_to_device", "lightcone_reset", "lightcone_advance"] + ["grid_to_device", "lightcone_advance"] * 2
    assert (cone.kind, cone.los_axis, cone.first_plane, cone.slot, cone.dchi, cone.N) == ("xhi", 0, 3, 1, 0.4, N)
    z_all = M.slice_redshifts(cosmo, 7.0, 6.99, 0.4)
    cube, _ = R.build_cone([1.0 - f for f in fields], zs, list(z_all), first_plane=3, axis=0)
    assert cone.z.tobytes() == z_all.tobytes() and cone.array().tobytes() == cube.tobytes()
    # an iterator of triples, a scale, one t_gamma per state
    triples = [R.fields(N, 20 + i) for i in range(3)]
    cone = M.make_lightcone(iter(triples), zs, kind="dtb", box_len_mpc=2.0, cosmology=cosmo, scale=lambda z: 3.0 * z, t_gamma=[1.0, 2.0, 3.0])
    formed = [R.form(R.HI, x, n, T, float(np.mean(n)), tg) for (x, n, T), tg in zip(triples, (1.0, 2.0, 3.0))]
    cube, _ = R.build_cone(formed, zs, list(z_all), axis=2, scale=lambda z: 3.0 * z)
    assert cone.array().tobytes() == cube.tobytes()
    # every refusal comes before the library is touched
    lib.calls.clear()
    Holder.left = 0
    bad = [(dict(kind="tb"), "kind must be one of"), (dict(los_axis=3), "los_axis must be 0, 1 or 2"), (dict(los_axis=True), "los_axis"),
           (dict(first_plane=-1), "first_plane must be an int in \\[0, N\\)"), (dict(first_plane=N), "first_plane"),
           (dict(first_plane=1.0), "first_plane"), (dict(slot=4), "slot must be an int in \\[0, 4\\)"), (dict(slot=-1), "slot"),
           (dict(box_len_mpc=None), "box_len_mpc must be a finite number > 0"), (dict(box_len_mpc=0.0), "box_len_mpc"),
           (dict(box_len_mpc=float("inf")), "box_len_mpc"), (dict(cosmology=None), "cosmology must have H0, efunc and comoving_distance"),
           (dict(redshifts=[7.0]), "redshifts must be two or more"), (dict(redshifts=[7.0, 7.0, 6.9]), "strictly descending"),
           (dict(redshifts=[6.9, 7.0, 7.1]), "strictly descending"), (dict(redshifts=[7.0, float("nan"), 6.9]), "redshifts"),
           (dict(redshifts="high"), "redshifts must be a one-dimensional sequence"), (dict(scale=2.0), "scale must be None or a function"),
           (dict(t_gamma=-1.0), "t_gamma must be finite and >= 0"), (dict(t_gamma=[1.0, 2.0]), "one number per state"),
           (dict(t_gamma="warm"), "t_gamma must be None, a number or one number per state"), (dict(t_gamma=True), "t_gamma"),
           (dict(fields=fields[:2]), "fields has 2 states, redshifts 3"), (dict(fields=[np.ones((N, N))] * 3), "must be a real \\(N, N, N\\) array"),
           (dict(fields=[(fields[0], fields[1])] * 3), "a triple \\(xh, ndens, temp\\)"),
           (dict(fields=[(fields[0], fields[1], np.ones((4, 4, 4)))] * 3), "must have one shape"),
           (dict(kind="density"), "is formed from triples"), (dict(kind="dtb"), "is formed from triples"),
           (dict(fields=[np.ones((700,) * 3, dtype=np.int8)] * 3), "the mesh must have 1 ... 645 cells a side")]
    for kw, what in bad:
        with pytest.raises(ValueError, match="make_lightcone: .*" + what):
            M.make_lightcone(**{**good, **kw})
        assert lib.calls == [] and Holder.left == 0, kw
    # a later state of another mesh, an iterator that ends early: found when they come
    with pytest.raises(ValueError, match="make_lightcone: fields\\[1\\] has 4 cells a side, the first state 5"):
        M.make_lightcone(**{**good, "fields": [fields[0], np.ones((4, 4, 4)), fields[2]]})
    with pytest.raises(ValueError, match="make_lightcone: fields has 2 states, redshifts 3"):
        M.make_lightcone(**{**good, "fields": iter(fields[:2])})
    # no device
    _install(monkeypatch, LB.Numpy(N), ready=False)
    with pytest.raises(RuntimeError, match="GPU not initialized"):
        M.make_lightcone(**good)
    # the accumulator's own checks
    for kw, what in ((dict(kind="tb"), "kind"), (dict(src_grid=9), "src_grid must be None or a grid selector"),
                     (dict(src_grid=2, kind="xhi"), "src_grid takes a grid as it is"), (dict(z_end=-2.0), "z_end"), (dict(first_plane=N), "first_plane")):
        with pytest.raises(ValueError, match="LightCone: .*" + what):
            M.LightCone(N, cosmo, 7.0, 0.4, **kw)
    for args, what in (((N, cosmo, 7.0, 0.0), "dchi must be a finite number > 0"), ((N, cosmo, -1.5, 0.4), "z_start"), ((N, None, 7.0, 0.4), "cosmology"),
                       ((2.5, cosmo, 7.0, 0.4), "N must be an int")):
        with pytest.raises(ValueError, match="LightCone: .*" + what):
            M.LightCone(*args)
    cone = M.LightCone(N, cosmo, 7.0, 0.4, src_grid=_capi.GRID_XH_AV)
    for kw, what in ((dict(t_gamma=-1.0), "t_gamma must be a finite number >= 0"), (dict(scale=1.0), "scale must be None or a function")):
        with pytest.raises(ValueError, match="LightCone.advance: " + what):
            cone.advance(lib, None, 7.0, **kw)
    # a grid as it is
    lib = LB.Numpy(N)
    for z, g in zip(zs, fields):
        lib.grid_to_device(_capi.GRID_XH_AV, g)
        cone.advance(lib, None if z == zs[0] else prev, z)
        prev = z
    cube, _ = R.build_cone(fields, zs, list(cone.z), axis=2)
    assert cone.array().tobytes() == cube.tobytes() and all(c[1][2] == _capi.GRID_XH_AV for c in lib.calls if c[0] == "lightcone_advance")


def test_yaml_keys_and_the_redshift_of_a_state(tmp_path, monkeypatch):
    """The class on the stand-in: the keys, the refusals of the switch, and two steps whose slices are weighted with the redshift of
    ``time`` -- the state's -- and not with ``zred``, which cosmo_evolve leaves at the half step."""
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.c2ray_base as B
    from pyc2ray_amd import _capi
    M = _module()
    assert B.C2Ray._STEP_ACCUMULATORS == ("lightcone_stats",) and B.C2Ray._step_closers() == B.C2Ray._step_statistics() + ("lightcone_stats",)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 24
        plain = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        assert plain.lightcone_stats is False and plain.lightcone is None and plain.last_lightcone_step is None
        with pytest.raises(ValueError, match="C2Ray.lightcone_stats: lightcone_stats needs use_gpu=True"):
            plain.lightcone_stats = True
        with pytest.raises(ValueError, match="lightcone_stats must be a bool"):
            plain.lightcone_stats = 1
        plain.gpu = True
        assert not plain.cosmological
        with pytest.raises(ValueError, match="C2Ray.lightcone_stats: lightcone_stats needs a cosmological run"):
            plain.lightcone_stats = True
        assert plain.lightcone_stats is False
        body = open(CONE_PARAMS).read()
        assert "  lightcone: 1\n  lightcone_kind: dtb\n  lightcone_los_axis: 1\n  lightcone_first_plane: 5\n" in body
        for old, text, what in (("  lightcone_kind: dtb\n", "  lightcone_kind: tb\n", "kind must be one of"),
                                ("  lightcone_los_axis: 1\n", "  lightcone_los_axis: 4\n", "los_axis must be 0, 1 or 2"),
                                ("  lightcone_first_plane: 5\n", "  lightcone_first_plane: 24\n", "first_plane must be an int in"),
                                ("  lightcone_kind: dtb\n", "  lightcone_spin: cold\n", "spin must be None or 'kinetic'"),
                                ("  lightcone_kind: dtb\n", "  lightcone_z_end: -3\n", "z_end must be a finite number > -1")):
            with open("p.yml", "w") as f:
                f.write(body.replace(old, text).replace("  lightcone: 1\n", "  lightcone: 0\n"))
            with pytest.raises(ValueError, match="Output: lightcone_kind / .*" + what):
                pc2r.C2Ray_Test("p.yml", N, False)
        with open("p.yml", "w") as f:
            f.write(body.replace("  lightcone: 1\n", "  lightcone: 2\n"))
        with pytest.raises(ValueError, match="Output: lightcone must be 0 or 1"):
            pc2r.C2Ray_Test("p.yml", N, False)
        with pytest.raises(ValueError, match="Output: lightcone: 1: lightcone_stats needs use_gpu=True"):
            pc2r.C2Ray_Test(CONE_PARAMS, N, False)
        with open("p.yml", "w") as f:
            f.write(body.replace("  cosmological: 1\n", "  cosmological: 0\n"))
        # an object with use_gpu (as one constructed with use_gpu=True has it) reading its keys
        with open("q.yml", "w") as f:
            f.write(body.replace("  lightcone: 1\n", "  lightcone: 0\n"))
        sim = pc2r.C2Ray_Test("q.yml", N, False)
        sim.gpu = True
        sim._read_paramfile("p.yml")                            # (not cosmological: refused as the assignment is)
        sim.cosmological = False
        with pytest.raises(ValueError, match="Output: lightcone: 1: lightcone_stats needs a cosmological run"):
            sim._statistic_init("lightcone_stats")
        sim.cosmological = True
        sim._read_paramfile(CONE_PARAMS)
        sim._statistic_init("lightcone_stats")
        assert sim.lightcone_stats is True and sim.lightcone is None and sim.last_lightcone_step is None
        assert B.C2Ray.lightcone_stats.defaults(sim) == {"kind": "dtb", "los_axis": 1, "first_plane": 5}
        assert sim.brightness_temperature_scale() == sim.brightness_temperature_scale(sim.zred)
        assert sim.brightness_temperature_scale(8.0) == pytest.approx(sim.brightness_temperature_scale(9.0) * (9.0 / 10.0) ** 0.5, rel=1e-14)
        lib = _install(monkeypatch, LB.Numpy(N))
        seen = []
        advance = M.LightCone.advance
        monkeypatch.setattr(M.LightCone, "advance", lambda self, lib, z_prev, z_now, **kw: (seen.append((z_prev, z_now, kw)), advance(self, lib, z_prev, z_now, **kw))[1])
        monkeypatch.setattr(B, "evolve3D_resident", lambda *a, **kw: None)
        flux, pos = np.ones(1), np.ones((3, 1), dtype=int)
        sim.device_resident = True
        sim.density_init(sim.zred_0)
        z_state, z_half = [], []
        for dt in (3.0e10, 9.0e10, 2.0e10):
            sim.cosmo_evolve(dt)
            sim.evolve3D(dt, flux, pos)
            z_state.append(float(sim.time2zred(sim.time)))
            z_half.append(float(sim.zred))
        assert all(zh > zs for zh, zs in zip(z_half, z_state))                 # (zred stays at the half step)
        assert [s[:2] for s in seen] == [(None, z_state[0]), (z_state[0], z_state[1]), (z_state[1], z_state[2])]
        assert all(s[2]["t_gamma"] == 0.0 and s[2]["scale"] == sim.brightness_temperature_scale for s in seen)
        cone = sim.lightcone
        assert isinstance(cone, M.LightCone) and (cone.kind, cone.los_axis, cone.first_plane, cone.slot, cone.keep) == ("dtb", 1, 5, 0, True)
        assert cone.dchi == pytest.approx(0.014 / 24, rel=1e-12) and cone.z[0] == z_state[0] and cone.z_end is None
        calls = [c for c in lib.calls if c[0] == "lightcone_advance"]
        assert len(calls) == 3 and len(calls[0][1][5]) == 0 and all(c[1][8] for c in calls)
        # the weights of the second step's slices: linear between the two STATES' redshifts, times the prefactor at the slice
        zs = cone.z[:len(calls[1][1][5])]
        assert zs.size >= 10 and np.all(zs <= z_state[0]) and np.all(zs >= z_state[1])
        w_prev, w_now = R.weights(z_state[0], z_state[1], zs, sim.brightness_temperature_scale)
        assert np.asarray(calls[1][1][6]).tobytes() == w_prev.tobytes() and np.asarray(calls[1][1][7]).tobytes() == w_now.tobytes()
        assert np.array_equal(calls[1][1][5], (5 - np.arange(zs.size)) % N) and calls[1][1][4] == 1 and calls[1][1][1] == _capi.PS_HI
        assert cone.n_slices == sum(len(c[1][5]) for c in calls) and sim.last_lightcone_step.n_slices == len(calls[2][1][5])
        log = open(sim.logfile).read()
        assert log.count("Light cone (dtb): ") == 3 and sim.last_lightcone_step.log_line() in log
        assert "Light cone (dtb): the field of the first state is kept, no slice yet" in log
        # the axis of an open cone stays
        with pytest.raises(ValueError, match="C2Ray.los_axis: a light cone is open"):
            sim.los_axis = 0
        # off: a step makes no library call of the feature's and the cone stays for the driver; on again: a new cone
        sim.lightcone_stats = False
        sim.los_axis = 0
        lib.calls.clear()
        sim.cosmo_evolve(1.0e10)
        sim.evolve3D(1.0e10, flux, pos)
        assert lib.names() == ["grid_scale"] and sim.lightcone is cone and len(seen) == 3      # (the density, diluted where it lies)
        sim.lightcone_stats = True
        assert sim.lightcone is None
        sim._read_paramfile("q.yml")
        sim.__dict__["_lightcone_stats_defaults"] = {"kind": "xh", "spin": "kinetic", "z_end": 1.0}
        sim.cosmo_evolve(1.0e10)
        sim.evolve3D(1.0e10, flux, pos)
        z_now = float(sim.time2zred(sim.time))
        assert seen[-1][0] is None and seen[-1][1] == z_now and seen[-1][2]["scale"] is None
        assert seen[-1][2]["t_gamma"] == 2.726 * (1.0 + z_now)
        assert (sim.lightcone.kind, sim.lightcone.los_axis, sim.lightcone.z_end) == ("xh", 0, 1.0) and sim.last_lightcone_step.stored_only
    finally:
        os.chdir(cwd)
        if "sim" in locals():      # (nothing of this object lives on a device: a later step elsewhere must not ask it to fetch)
            sim._device_newer.clear()
            sim.device_resident = False
