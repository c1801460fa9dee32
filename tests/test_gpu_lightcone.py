"""GPU: slices of a light cone (asora_lightcone_advance) against the numpy statement of
tests/lightcone_reference.py -- exactly, as the blend is two rounded products and a sum -- on meshes of 24, 33 and 70 cells along
all three axes; the moments against math.fsum of the device's own slices; the kept field, the slots, the refusals; a run of the class
against make_lightcone on its downloaded states; calls of the most slices the entry takes (tests/untested_trips.py).  Every call is
made twice and compared byte for byte."""
import functools
import math
import os

import numpy as np
import pytest

import lightcone_reference as R
import untested_trips as UT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CONE_PARAMS = os.path.join(HERE, "data", "parameters_lightcone.yml")
EPS = float(np.finfo(np.float64).eps)
# 24, 33 and 70 on all three axes: 70 is above one wave and a multiple of nothing (two tiles of 64 j, the second 6 wide), 33 is odd
CASES = [(N, axis) for N in (24, 33, 70) for axis in (0, 1, 2)]
T_GAMMA = 27.0


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib, _capi
    if p.cuda_is_init():
        p.device_close()


@functools.lru_cache(maxsize=None)
def _state(N, which):
    """(x, n, T, cube) of state `which` of a mesh: the three grids and a cube for a grid taken as it is"""
    x, n, T = R.fields(N, 1000 * which + N)
    cube = np.random.default_rng(7000 * which + N).standard_normal((N, N, N))
    for a in (x, n, T, cube):
        a.flags.writeable = False
    return x, n, T, cube


def _mesh(asora, N):
    p, lib, capi = asora
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)


def _upload(asora, state):
    p, lib, capi = asora
    for which, grid in zip((capi.GRID_XH, capi.GRID_NDENS, capi.GRID_TEMP, capi.GRID_XH_AV), state):
        lib.grid_to_device(which, np.array(grid))


def _formed(asora, kind, t_gamma=0.0):
    """The device's own formed field of the grids as they lie (its mean density differs from numpy's by an ulp)"""
    p, lib, capi = asora
    return lib.power_spectrum(kind, None, 1.0, t_gamma, np.array([1, 2], dtype=np.uint32), field=True)["field"]


def _plane_lists(N, rng):
    """Empty; one plane; a descending run of 7 that wraps through 0; 2 N + 3 slices down from a plane, where planes repeat (and
    runs longer than a tile of 32 are cut); an ascending run; a shuffled list with repeats; runs with short stretches between"""
    down = (3 - np.arange(7)) % N
    cone = (10 - np.arange(2 * N + 3)) % N
    up = np.arange(5, 5 + 9)
    shuffled = rng.integers(0, N, size=11)
    mixed = np.r_[np.arange(2, 8), [N - 1, 0], np.arange(N - 1, N - 6, -1), [4, 4, 5], np.arange(9, 12)]
    return [np.zeros(0, dtype=np.int64), np.array([N - 1]), down, cone, up, shuffled, mixed]


def _weights(n, rng):
    """Ordinary weights, with (1, 0), (0, 1), negative and 1e300-scale ones among them"""
    w_prev, w_now = rng.standard_normal(n), rng.standard_normal(n)
    special = [(1.0, 0.0), (0.0, 1.0), (-2.5, 0.75), (3.0e300, -1.0e300), (0.0, 0.0)]
    for q, (a, b) in zip(rng.permutation(n)[:len(special)], special):
        w_prev[q], w_now[q] = a, b
    return w_prev, w_now


def _advance(lib, slot, kind, src, t_gamma, axis, planes, w_prev, w_now, refresh=False):
    """The call twice without a refresh, then -- if asked -- once more with it: the same bytes every time."""
    got = lib.lightcone_advance(slot, kind, src, t_gamma, axis, planes, w_prev, w_now, False)
    runs = [lib.lightcone_advance(slot, kind, src, t_gamma, axis, planes, w_prev, w_now, False)]
    if refresh:
        runs.append(lib.lightcone_advance(slot, kind, src, t_gamma, axis, planes, w_prev, w_now, True))
    for again in runs:
        assert again["slices"].tobytes() == got["slices"].tobytes() and again["moments"].tobytes() == got["moments"].tobytes()
    bare = lib.lightcone_advance(slot, kind, src, t_gamma, axis, planes, w_prev, w_now, False, slices=False) if not refresh else None
    if bare is not None:
        assert bare["slices"] is None and bare["moments"].tobytes() == got["moments"].tobytes()
    return got


def _check_moments(got, N, what):
    """|sum - fsum of the device's own slice| <= (N^2 + 4) eps sum |out|, the worst case of any order of a double-double sum's
    N^2 inputs and its handful of folds; likewise for the rounded squares.  A sum that overflows is not finite."""
    worst = 0.0
    for t, sl in enumerate(got["slices"]):
        flat = sl.ravel()
        with np.errstate(over="ignore"):
            squares = flat * flat
        for q, v in enumerate((flat, squares)):
            exact, dev = math.fsum(v), float(got["moments"][t, q])
            if not math.isfinite(exact):
                assert not math.isfinite(dev), (what, t, q)
                continue
            bound = (N * N + 4) * EPS * math.fsum(np.abs(v))
            assert abs(dev - exact) <= bound, (what, t, q, dev, exact)
            worst = max(worst, abs(dev - exact) / bound if bound > 0 else 0.0)
    return worst


@pytest.mark.parametrize("N,axis", CASES)
def test_slices_equal_the_statement(asora, N, axis):
    p, lib, capi = asora
    _mesh(asora, N)
    before, after = _state(N, 1), _state(N, 2)
    # two rounds of slots: the kinds that are exact against numpy's own fields, then those fed with the device's formed field
    rounds = [[(0, capi.PS_XH, None, 0.0), (1, capi.PS_XHI, None, 0.0), (2, capi.PS_XH, capi.GRID_XH_AV, 0.0), (3, capi.PS_DENSITY, None, 0.0)],
              [(0, capi.PS_HI, None, 0.0), (1, capi.PS_HI, None, T_GAMMA)]]
    worst = 0.0
    for configs in rounds:
        prev, now = {}, {}
        _upload(asora, before)
        for slot, kind, src, tg in configs:
            lib.lightcone_reset(slot)
            first = lib.lightcone_advance(slot, kind, src, tg, axis, (), (), (), True)
            assert first["slices"].shape == (0, N, N) and first["moments"].shape == (0, 2)
            assert lib.lightcone_state(slot) == dict(has_prev=True, kind=kind, src_grid=src)
            prev[slot] = before[3] if src is not None else (R.form(kind, *before[:3], 1.0) if kind in (capi.PS_XH, capi.PS_XHI) else _formed(asora, kind, tg))
        _upload(asora, after)
        for slot, kind, src, tg in configs:
            now[slot] = after[3] if src is not None else (R.form(kind, *after[:3], 1.0) if kind in (capi.PS_XH, capi.PS_XHI) else _formed(asora, kind, tg))
        rng = np.random.default_rng(N + axis)
        for planes in _plane_lists(N, rng):
            w_prev, w_now = _weights(planes.size, rng)
            for slot, kind, src, tg in configs:
                got = _advance(lib, slot, kind, src, tg, axis, planes, w_prev, w_now)
                ref = R.blend(prev[slot], now[slot], planes, w_prev, w_now, axis)
                assert got["slices"].shape == ref.shape and got["slices"].tobytes() == ref.tobytes(), (N, axis, kind, src, tg, planes)
                worst = max(worst, _check_moments(got, N, (N, axis, kind, planes.size)))
        # weights (1, 0) and (0, 1) return the kept and the present field's planes
        planes = np.arange(N)[::-1]
        ones, zeros = np.ones(N), np.zeros(N)
        for slot, kind, src, tg in configs:
            kept = lib.lightcone_advance(slot, kind, src, tg, axis, planes, ones, zeros, False)["slices"]
            present = lib.lightcone_advance(slot, kind, src, tg, axis, planes, zeros, ones, False)["slices"]
            assert np.array_equal(np.moveaxis(kept[::-1], 0, axis), prev[slot]) and np.array_equal(np.moveaxis(present[::-1], 0, axis), now[slot])
    print(f"N = {N}, axis {axis}: the moments use at most {worst:.2e} of their bound")


def test_refresh_and_independent_slots(asora):
    """refresh = 0 leaves the kept field alone; after refresh = 1 the kept field is the state of THAT call, whatever the grids
    become afterwards.  Two slots of different kinds, interleaved, do not see each other."""
    p, lib, capi = asora
    N, axis = 33, 2
    _mesh(asora, N)
    s1, s2, s3 = _state(N, 1), _state(N, 2), _state(N, 3)
    rng = np.random.default_rng(5)
    planes = (20 - np.arange(12)) % N
    w_prev, w_now = rng.standard_normal(12), rng.standard_normal(12)
    _upload(asora, s1)
    lib.lightcone_advance(0, capi.PS_XH, None, 0.0, axis, (), (), (), True)
    _upload(asora, s2)
    lib.lightcone_advance(1, capi.PS_XHI, None, 0.0, axis, (), (), (), True)        # slot 1 begins a state later
    a = _advance(lib, 0, capi.PS_XH, None, 0.0, axis, planes, w_prev, w_now, refresh=True)      # (twice with refresh = 0, then with 1)
    assert a["slices"].tobytes() == R.blend(s1[0], s2[0], planes, w_prev, w_now, axis).tobytes()
    _upload(asora, s3)                                                              # the grids change behind the refresh
    b = _advance(lib, 0, capi.PS_XH, None, 0.0, axis, planes, w_prev, w_now)
    assert b["slices"].tobytes() == R.blend(s2[0], s3[0], planes, w_prev, w_now, axis).tobytes()
    c = _advance(lib, 1, capi.PS_XHI, None, 0.0, 0, planes, w_prev, w_now, refresh=True)
    assert c["slices"].tobytes() == R.blend(1.0 - s2[0], 1.0 - s3[0], planes, w_prev, w_now, 0).tobytes()
    _upload(asora, s1)
    d = _advance(lib, 1, capi.PS_XHI, None, 0.0, 1, planes, w_prev, w_now)
    assert d["slices"].tobytes() == R.blend(1.0 - s3[0], 1.0 - s1[0], planes, w_prev, w_now, 1).tobytes()
    e = _advance(lib, 0, capi.PS_XH, None, 0.0, axis, planes, w_prev, w_now)         # slot 0 still keeps state 2
    assert e["slices"].tobytes() == R.blend(s2[0], s1[0], planes, w_prev, w_now, axis).tobytes()
    assert lib.lightcone_state(0) == dict(has_prev=True, kind=capi.PS_XH, src_grid=None)
    assert lib.lightcone_state(1) == dict(has_prev=True, kind=capi.PS_XHI, src_grid=None)
    assert lib.lightcone_state(2) == dict(has_prev=False, kind=0, src_grid=None)
    # the memory: one N^3 buffer per slot in use, freed with the mesh; device_close and device_init forget the slots
    count, nbytes = lib.live_buffers(0)
    p.device_close()
    assert lib.live_buffers(0) == (0, 0)
    p.device_init(N, 8)
    assert all(lib.lightcone_state(slot)["has_prev"] is False for slot in range(capi.LC_SLOTS))
    _upload(asora, s1)
    with pytest.raises(RuntimeError, match="lightcone_advance failed \\(code 3\\).*the first call on a slot"):
        lib.lightcone_advance(0, capi.PS_XH, None, 0.0, axis, planes, w_prev, w_now, False)
    lib.lightcone_advance(0, capi.PS_XH, None, 0.0, axis, (), (), (), True)
    _upload(asora, s2)
    f = lib.lightcone_advance(0, capi.PS_XH, None, 0.0, axis, planes, w_prev, w_now, False)
    assert f["slices"].tobytes() == a["slices"].tobytes()
    assert lib.live_buffers(0)[1] < nbytes                                         # (one slot now, two before)


def _raw(lib, capi, N, slot=0, kind=0, src_grid=-1, t_gamma=0.0, los_axis=2, planes=(3, 2, 1), w_prev=(0.5, 0.5, 0.5), w_now=(0.5, 0.5, 0.5),
         refresh=0, n_slices=None, null=()):
    """The C entry with sentinels in every output: (code, are all outputs untouched)"""
    pl, wp, wn = np.array(planes, dtype=np.int32), np.array(w_prev, dtype=np.float64), np.array(w_now, dtype=np.float64)
    n = pl.size if n_slices is None else n_slices
    out = dict(slices=np.full((max(pl.size, 1), N, N), 9.0), moments=np.full(2 * max(pl.size, 1), 9.0))
    ptr = dict(plane=capi.iptr(pl), w_prev=capi.dptr(wp), w_now=capi.dptr(wn), slices=capi.dptr(out["slices"]), moments=capi.dptr(out["moments"]))
    for name in null:
        ptr[name] = None
    rc = lib._lib.asora_lightcone_advance(slot, kind, src_grid, t_gamma, los_axis, n, ptr["plane"], ptr["w_prev"], ptr["w_now"], refresh,
                                          ptr["slices"], ptr["moments"])
    return rc, all(np.all(a == 9.0) for a in out.values())


def test_refusals(asora):
    p, lib, capi = asora
    N = 24
    s1, s2 = _state(N, 1), _state(N, 2)
    _mesh(asora, N)
    lib.grid_to_device(capi.GRID_XH, np.array(s1[0]))
    # a slot without a kept field takes the storing call only
    assert _raw(lib, capi, N) == (3, True) and b"the first call on a slot" in lib._lib.asora_last_error()
    assert _raw(lib, capi, N, planes=(), w_prev=(), w_now=(), refresh=0) == (3, True)
    # grids that hold no data: code 4, and 3 comes before 4
    assert _raw(lib, capi, N, kind=capi.PS_DENSITY, planes=(), w_prev=(), w_now=(), refresh=1) == (4, True)
    assert b"holds no data" in lib._lib.asora_last_error()
    assert _raw(lib, capi, N, kind=capi.PS_HI, planes=(), w_prev=(), w_now=(), refresh=1) == (4, True)
    assert _raw(lib, capi, N, src_grid=capi.GRID_XH_AV, planes=(), w_prev=(), w_now=(), refresh=1) == (4, True)
    assert _raw(lib, capi, N, kind=capi.PS_DENSITY, los_axis=3, planes=(), w_prev=(), w_now=(), refresh=1) == (3, True)
    lib.grid_to_device(capi.GRID_NDENS, np.array(s1[1]))
    assert _raw(lib, capi, N, kind=capi.PS_HI, t_gamma=T_GAMMA, planes=(), w_prev=(), w_now=(), refresh=1) == (4, True)     # (no temperature)
    assert _raw(lib, capi, N, kind=capi.PS_HI, planes=(), w_prev=(), w_now=(), refresh=1)[0] == 0
    lib.lightcone_reset(0)
    assert _raw(lib, capi, N, planes=(), w_prev=(), w_now=(), refresh=1)[0] == 0                   # slot 0 keeps state 1 of 'xh'
    lib.grid_to_device(capi.GRID_XH, np.array(s2[0]))
    good = lib.lightcone_advance(0, capi.PS_XH, None, 0.0, 2, (3, 2, 1), (0.5,) * 3, (0.5,) * 3, False)
    nan, inf = math.nan, math.inf
    bad = [dict(slot=-1), dict(slot=capi.LC_SLOTS), dict(kind=-1), dict(kind=capi.PS_KINDS), dict(src_grid=-2), dict(src_grid=capi.GRID_COUNT),
           dict(src_grid=capi.GRID_XH, kind=capi.PS_XHI), dict(los_axis=-1), dict(los_axis=3), dict(t_gamma=nan), dict(t_gamma=inf), dict(t_gamma=-1.0),
           dict(w_prev=(0.5, nan, 0.5)), dict(w_now=(inf, 0.5, 0.5)), dict(planes=(3, -1, 1)), dict(planes=(3, N, 1)), dict(planes=(2 ** 31 - 1, 0, 0)),
           dict(n_slices=-1), dict(n_slices=capi.LC_MAX_SLICES + 1), dict(refresh=2), dict(null=("plane",)), dict(null=("w_prev",)),
           dict(null=("w_now",)), dict(null=("moments",)),
           dict(kind=capi.PS_XHI), dict(src_grid=capi.GRID_XH), dict(slot=1)]             # (another kind, another source; a slot without a field)
    for kw in bad:
        assert _raw(lib, capi, N, **kw) == (3, True), kw
        assert lib._lib.asora_last_error().startswith(b"lightcone_advance: "), kw
    # ... and each of them left the kept field as it was
    again = lib.lightcone_advance(0, capi.PS_XH, None, 0.0, 2, (3, 2, 1), (0.5,) * 3, (0.5,) * 3, False)
    assert again["slices"].tobytes() == good["slices"].tobytes() == R.blend(s1[0], s2[0], (3, 2, 1), (0.5,) * 3, (0.5,) * 3, 2).tobytes()
    assert lib.lightcone_state(0) == dict(has_prev=True, kind=capi.PS_XH, src_grid=None)
    # slices_out may be NULL; the most slices a call takes
    assert _raw(lib, capi, N, null=("slices",))[0] == 0
    most = capi.LC_MAX_SLICES
    big = lib.lightcone_advance(0, capi.PS_XH, None, 0.0, 2, (5 - np.arange(most)) % N, np.full(most, 0.25), np.full(most, 0.75), False)
    assert big["slices"].shape == (most, N, N)
    assert big["slices"][-1].tobytes() == R.blend(s1[0], s2[0], [(5 - (most - 1)) % N], [0.25], [0.75], 2)[0].tobytes()
    # after a reset the slot takes another kind
    with pytest.raises(RuntimeError, match="lightcone_advance failed \\(code 3\\).*kept field was made with kind 0"):
        lib.lightcone_advance(0, capi.PS_XHI, None, 0.0, 2, (), (), (), True)
    lib.lightcone_reset(0)
    assert lib.lightcone_state(0)["has_prev"] is False
    lib.lightcone_advance(0, capi.PS_XHI, None, 0.0, 2, (), (), (), True)
    assert lib.lightcone_state(0) == dict(has_prev=True, kind=capi.PS_XHI, src_grid=None)
    p.device_close()
    assert _raw(lib, capi, N) == (2, True)


def test_stage_times(asora):
    p, lib, capi = asora
    N = 33
    _mesh(asora, N)
    _upload(asora, _state(N, 1))
    lib.set_option(capi.OPT_TIMING, 1)
    try:
        lib.lightcone_advance(0, capi.PS_HI, None, 0.0, 2, (), (), (), True)
        ms = lib.lightcone_ms()
        assert ms.shape == (capi.LC_STAGES,) and ms[0] > 0.0 and ms[3] > 0.0
        lib.lightcone_advance(0, capi.PS_HI, None, 0.0, 2, np.arange(9), np.ones(9), np.ones(9), False)
        ms = lib.lightcone_ms()
        assert np.all(ms[:3] > 0.0) and np.all(ms >= 0.0)
    finally:
        lib.set_option(capi.OPT_TIMING, 0)


def test_a_mesh_of_five_tiles_along_axis_2(asora):
    """N = 320: five tiles of 64 j, rows longer than a workgroup, 32.8 million cells; one call of 9 slices in one run (and one of 3,
    which takes the per-slice form) of the ionised fraction."""
    p, lib, capi = asora
    N = 320
    _mesh(asora, N)
    rng = np.random.default_rng(320)
    a, b = rng.random((N, N, N)), rng.random((N, N, N))
    lib.grid_to_device(capi.GRID_XH, a)
    lib.lightcone_advance(0, capi.PS_XH, None, 0.0, 2, (), (), (), True)
    lib.grid_to_device(capi.GRID_XH, b)
    for planes in ((4 - np.arange(9)) % N, np.array([N - 1, 0, 1])):
        w_prev, w_now = rng.standard_normal(planes.size), rng.standard_normal(planes.size)
        got = lib.lightcone_advance(0, capi.PS_XH, None, 0.0, 2, planes, w_prev, w_now, False)
        again = lib.lightcone_advance(0, capi.PS_XH, None, 0.0, 2, planes, w_prev, w_now, False)
        assert got["slices"].tobytes() == again["slices"].tobytes() and got["moments"].tobytes() == again["moments"].tobytes()
        assert got["slices"].tobytes() == R.blend(a, b, planes, w_prev, w_now, 2).tobytes()
        _check_moments(got, N, ("N = 320", planes.size))


@pytest.mark.parametrize("case", ["axis_0", "axis_1", "no_run", "runs_of_4", "mixed"])
def test_the_most_slices_a_call_takes(asora, case):
    """ASORA_LC_MAX_SLICES = 1024 slices in one call at N = 70 (tests/untested_trips.py): on the axes 0 and 1 and as a list without a
    run on axis 2, 2.39 trips of lc_emit_kernel's grid-stride loop; on axis 2 in 256 runs of 4, the run table full to its last entry
    with the moments directly behind it; and in 31 runs of 32 with 32 listed slices between.  The ionised fraction and a grid taken
    as it is, byte for byte against the statement; the moments of all 1024 slices, eight workgroups of the fold."""
    p, lib, capi = asora
    N, most = UT.LC_MESH, capi.LC_MAX_SLICES
    assert most == UT.LC_MAX_SLICES and UT.fold_workgroups(most) == 8
    rng = np.random.default_rng(len(case) + 7000)
    if case.startswith("axis"):
        axis, planes = int(case[-1]), rng.integers(0, N, size=most)
        assert UT.emit_trips(most * N * N) > 2.0
    else:
        axis = 2
        planes, n_runs, n_listed, why = UT.plane_lists(N)[case]
        runs, listed = UT.cut_runs(planes)
        assert (len(runs), len(listed)) == (n_runs, n_listed) and n_listed + sum(r.len for r in runs) == most
        if case == "no_run":
            assert UT.emit_trips(len(listed) * N * N) > 2.0 and not np.any(np.abs(np.diff(planes)) == 1)
        if case == "runs_of_4":
            assert len(runs) == UT.LC_RUN_TABLE == most // UT.LC_RUN_MIN and all(r.len == UT.LC_RUN_MIN for r in runs)
    assert planes.size == most
    _mesh(asora, N)
    before, after = _state(N, 1), _state(N, 2)
    configs = [(0, capi.PS_XH, None, before[0], after[0]), (2, capi.PS_XH, capi.GRID_XH_AV, before[3], after[3])]
    _upload(asora, before)
    for slot, kind, src, _, _ in configs:
        lib.lightcone_reset(slot)
        lib.lightcone_advance(slot, kind, src, 0.0, axis, (), (), (), True)
    _upload(asora, after)
    w_prev, w_now = _weights(most, rng)
    for slot, kind, src, prev, now in configs:
        got = _advance(lib, slot, kind, src, 0.0, axis, planes, w_prev, w_now)
        ref = R.blend(prev, now, planes, w_prev, w_now, axis)
        assert got["slices"].shape == ref.shape == (most, N, N) and got["slices"].tobytes() == ref.tobytes(), (case, src)
        assert got["moments"].shape == (most, 2)
        worst = _check_moments(got, N, (case, src))
        print(f"{case}, source grid {src}: the moments of {most} slices use at most {worst:.2e} of their bound")


DTS = (1.0e10, 2.0e11, 1.0e9, 5.0e10)   # the first state is kept; then 34 slices (more than N), none, 8


@pytest.mark.parametrize("resident", [True, False])
def test_class_against_make_lightcone(asora, tmp_path, resident):
    """A cosmological run at N = 24 with ``Output: lightcone: 1``: its cone equals, bit for bit, make_lightcone fed with the states
    downloaded after each step and the redshift of ``time`` of each."""
    p, lib, capi = asora
    import pyc2ray_amd as pc2r
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 24
        with open("src.txt", "w") as f:
            f.write("1\n12 12 12 5e50 1.0\n")
        if p.cuda_is_init():
            p.device_close()
        sim = pc2r.C2Ray_Test(CONE_PARAMS, N, True)
        sim.device_resident = resident
        assert sim.lightcone_stats is True and sim.lightcone is None and sim.cosmological
        sim.density_init(sim.zred_0)
        srcpos, srcflux = sim.read_sources("src.txt", 1)
        states, zs, emitted = [], [], []
        for dt in DTS:
            sim.cosmo_evolve(dt)
            sim.evolve3D(dt, srcflux, srcpos)
            if resident:
                assert sim._device_newer >= {"xh", "phi_ion"}     # the cone fetched nothing but its slices
            emitted.append(sim.last_lightcone_step.n_slices)
            zs.append(float(sim.time2zred(sim.time)))
            states.append((sim.xh.copy(), np.array(sim.ndens, dtype=np.float64), np.array(sim.temp, dtype=np.float64)))
        cone = sim.lightcone
        assert emitted[0] == 0 and emitted[2] == 0 and emitted[1] > N and emitted[3] > 0 and cone.n_slices == sum(emitted)
        assert (cone.kind, cone.los_axis, cone.first_plane) == ("dtb", 1, 5) and cone.z[0] == zs[0] and cone.z[-1] >= zs[-1]
        log = open(sim.logfile).read()
        assert log.count("Light cone (dtb): ") == 4 and log.count("the step crossed no slice") == 1
        mine = cone.array()
        assert mine.shape == (sum(emitted), N, N) and np.all(np.isfinite(mine)) and np.any(mine != 0.0)
        other = pc2r.make_lightcone(states, zs, kind="dtb", los_axis=1, box_len_mpc=sim.boxsize_c / pc2r.Mpc, cosmology=sim.cosmology,
                                    first_plane=5, scale=sim.brightness_temperature_scale)
        assert other.z.tobytes() == cone.z.tobytes() and other.array().tobytes() == mine.tobytes()
        assert other.moments.tobytes() == cone.moments.tobytes()
        assert np.allclose(cone.mean, mine.mean(axis=(1, 2)), rtol=1e-12)
    finally:
        if p.cuda_is_init():
            p.device_close()
        os.chdir(cwd)
