"""CPU: the host side of the bispectrum: the C-ABI symbols, every refusal of bispectrum_spec (before the
library is touched), the order of calls of the module entry, the triangle selections, the default shells and ``aliased``, the
normalisations of Bispectrum from canned sums, and what C2Ray.bispectrum passes (on a stand-in for the library)."""
import importlib
import math
import os

import numpy as np
import pytest

import bispectrum_reference as BR
import bispectrum_standin_backend as BB
import lls_standin_backend as SB
import powerspec_reference as PR

HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_test.yml")


def _module():
    return importlib.import_module("pyc2ray_amd.bispectrum")


def _install(monkeypatch, backend, ready=True):
    import pyc2ray_amd.c2ray_base as B
    for mod in (_module(), B):
        monkeypatch.setattr(mod, "load_asora", lambda: backend)
        monkeypatch.setattr(mod, "cuda_is_init", lambda: ready)
    return backend


def test_capi_symbols_and_header():
    from pyc2ray_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "asora_hip.h")).read()
    assert ("int asora_bispectrum(int kind, double scale, double t_gamma, int n_shells, const unsigned *thresholds /* [n_shells + 1] */,\n"
            "                     int n_tri, const int32_t *tri /* [3 n_tri] shell indices */,\n") in header
    assert "int asora_debug_bispectrum_ms(double *ms /* [ASORA_BISPEC_STAGES] */);" in header
    assert "int asora_debug_bispectrum_plan(int N, int n_shells, int n_tri, int32_t *out /* [ASORA_BISPEC_PLAN_WORDS] */);" in header
    assert "ASORA_BISPEC_MAX_SHELLS = 32, ASORA_BISPEC_MAX_TRIANGLES = 8192" in header
    assert (_capi.BISPEC_MAX_SHELLS, _capi.BISPEC_MAX_TRIANGLES) == (32, 8192)
    assert f"ASORA_BISPEC_STAGES = {_capi.BISPEC_STAGES}" in header and f"ASORA_BISPEC_PLAN_WORDS = {_capi.BISPEC_PLAN_WORDS}" in header
    assert "modulo N" in header.lower() or "MODULO N" in header
    assert len(_capi.SIGNATURES["asora_bispectrum"][1]) == 13
    lib = _capi.load()
    # the plan is a host computation: one pass up to the chunk, the fixed grid, the trips of a workgroup
    from pyc2ray_amd.load_extensions import load_asora
    plan = load_asora().bispectrum_plan(72, 5, 300)
    chunk, groups, cells = plan["chunk"], plan["workgroups"], plan["tile_cells"]
    assert chunk == 4 * plan["wave_chunk"] and plan["passes"] == -(-300 // chunk)
    tiles = -(-72 ** 3 // cells)
    assert (plan["trips_max"], plan["trips_min"]) == (-(-tiles // groups), tiles // groups) and plan["idle_workgroups"] == 0
    small = load_asora().bispectrum_plan(30, 32, 1)
    assert small["passes"] == 1 and small["idle_workgroups"] == groups - (-(-30 ** 3 // cells)) > 0 and small["trips_min"] == 0
    assert lib.asora_debug_bispectrum_plan(72, 5, 300, None) == 3 and lib.asora_debug_bispectrum_ms(None) == 3


def test_normalisations_from_canned_sums():
    Bispectrum = _module().Bispectrum
    N, L = 4, 8.0
    edges = [0.5, 1.5, 2.5, 3.5]
    tri = [(0, 1, 2), (1, 1, 1), (2, 2, 0)]
    got = BB.answer(N, PR.thresholds_of(edges), tri)
    b = Bispectrum(edges, tri, got["sum_ggg"], got["sum_iii"], got["count"], got["sum_k"], got["sum_aa"], got["moments"], N, box_len=L)
    assert b.thresholds.tolist() == [1, 3, 7, 13] and b.L == L
    assert b.n_triangles.tolist() == [6.25, 8.0, 9.0] and b.count_residual == 0.25          # (not rounded silently)
    k = 2 * math.pi / L * np.array([1.0, 2.0, 3.0])
    assert np.allclose(b.k, k) and np.allclose(b.P, 4 * L ** 3)
    assert np.allclose(b.k1, k[[0, 1, 2]]) and np.allclose(b.k2, k[[1, 1, 2]]) and np.allclose(b.k3, k[[2, 1, 0]])
    want_B = L ** 6 / N ** 9 * got["sum_ggg"] / got["sum_iii"]
    assert np.allclose(b.B, want_B) and np.allclose(b.B[1:], -2 * L ** 6)
    P = 4 * L ** 3
    assert np.allclose(b.Q, want_B / (3 * P * P))
    assert np.allclose(b.b_norm, want_B / np.sqrt(b.k1 * b.k2 * b.k3 * P ** 3 / L ** 3))
    assert np.allclose(b.cos_theta, (b.k3 ** 2 - b.k1 ** 2 - b.k2 ** 2) / (2 * b.k1 * b.k2)) and abs(b.cos_theta[1] + 0.5) < 1e-15
    assert b.mean == 512.0 / 64 and b.variance == 2048.0 / 64 - 64.0
    assert b.log_line().startswith("Bispectrum (dtb, 3 shells to |n| = 3.5, 3 triangles, L = 8 units of box_len): mean 8.000000e+00")
    assert "aliased triangles included" in b.log_line() and repr(b) == f"<Bispectrum: {b.log_line()}>"
    # a triangle that cannot close: NaN, not a division by zero
    got = BB.answer(N, PR.thresholds_of(edges), [(1, 1, 1), (1, 2, 2)])
    none = Bispectrum(edges, [(1, 1, 1), (1, 2, 2)], got["sum_ggg"], np.array([8.0, 0.0]), got["count"], got["sum_k"], got["sum_aa"],
                      got["moments"], N)
    assert np.isnan(none.B[1]) and np.isnan(none.Q[1]) and none.B[0] == N ** 6 / N ** 9 * got["sum_ggg"][0] / 8.0 and none.L == 4.0
    for bad in (dict(n_modes=[1, 2]), dict(sum_iii=[1.0, 2.0]), dict(triangles=[(0, 1, 3)]), dict(moments=[1.0])):
        kw = dict(edges=edges, triangles=[(0, 1, 2)], sum_ggg=[1.0], sum_iii=[1.0], n_modes=[1, 2, 3], sum_k=[1.0, 2.0, 3.0],
                  sum_aa=[1.0, 2.0, 3.0], moments=[1.0, 2.0], N=N)
        kw.update(bad)
        with pytest.raises(ValueError, match="Bispectrum: "):
            Bispectrum(**kw)


def test_default_shells_selections_and_aliased():
    M = _module()
    spec = M.bispectrum_spec
    for N in (4, 10, 12, 24, 30, 100, 256):
        s = spec("x", N)
        top = max(1, (N - 1) // 3)
        assert s["edges"].tolist() == (np.arange(0, min(top, 32) + 1) + 0.5).tolist()
        assert s["thresholds"].tolist() == PR.thresholds_of(s["edges"]).tolist()
        assert s["triangles"].tolist() == BR.all_triangles(s["edges"]).tolist()
        b = M.Bispectrum(s["edges"], s["triangles"][:1], [0.0], [1.0], np.ones(s["edges"].size - 1), np.ones(s["edges"].size - 1),
                         np.ones(s["edges"].size - 1), [0.0, 0.0], N)
        assert b.aliased is False
    assert spec("x", 256)["edges"].size == 33 and spec("x", 645, shells=32)["edges"][-1] == 214.5
    # no closed triple of the default shells is aliased: as many close modulo N as close exactly
    N = 10
    s = spec("x", N)
    thr = s["thresholds"]
    _, C = BR.direct_sums(np.zeros((N, N, N)), thr)
    r = np.arange(-(N // 2), N // 2 + 1)
    n = np.array([(x, y, z) for x in r for y in r for z in r if int(thr[0]) <= x * x + y * y + z * z < int(thr[-1])])
    third = -(n[:, None, :] + n[None, :, :])
    n2 = np.sum(third * third, axis=2)
    assert int(C.sum()) == int(np.sum((n2 >= int(thr[0])) & (n2 < int(thr[-1])))) > 0
    e = [0.5, 1.5, 2.5, 3.5]
    assert spec("x", 12, shells=e, triangles="equilateral")["triangles"].tolist() == [[0, 0, 0], [1, 1, 1], [2, 2, 2]]
    assert spec("x", 12, shells=e, triangles="isosceles")["triangles"].tolist() == [[a, a, c] for a in range(3) for c in range(3)]
    # 'all': the lower edge of c below the sum of the upper edges of a and b
    wide = [0.5, 1.0, 4.0, 9.0]
    assert spec("x", 30, shells=wide)["triangles"].tolist() == [[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 2], [0, 2, 2], [1, 1, 1], [1, 1, 2],
                                                                [1, 2, 2], [2, 2, 2]]          # (all but (0, 0, 2): 4 >= 1 + 1)
    assert spec("x", 12, shells=e, triangles=[(2, 0, 1), (2, 0, 1), (1, 1, 1)])["triangles"].tolist() == [[2, 0, 1], [2, 0, 1], [1, 1, 1]]
    assert spec("x", 12, shells=3)["edges"].tolist() == np.linspace(0.5, 3.5, 4).tolist()
    for N, edges, aliased in ((12, [0.5, 3.5], False), (12, [0.5, 4.0], False), (12, [0.5, 4.01], True), (10, [0.5, 3.5], False),
                              (10, [1.0, 4.5], True), (9, [0.5, 2.9], False), (9, [0.5, 3.5], True)):
        b = M.Bispectrum(edges, [(0, 0, 0)], [0.0], [1.0], [1], [1.0], [1.0], [0.0, 0.0], N)
        assert b.aliased is aliased, (N, edges)


def test_bad_arguments_are_refused_before_the_library_is_touched(monkeypatch):
    M = _module()
    bispectrum, spec = M.bispectrum, M.bispectrum_spec
    _install(monkeypatch, SB.Untouchable())
    f = np.zeros((8, 8, 8))
    for kw, what in ((dict(kind="HI"), "kind must be one of"), (dict(kind=3), "kind must be one of"), (dict(kind=None), "kind must be one of"),
                     (dict(shells=0), "shells as an int must be in \\[1, 32\\]"), (dict(shells=33), "shells as an int must be in"),
                     (dict(shells=True), "not a bool"), (dict(shells=[1.0]), "one-dimensional array of 2 ... 257 edges"),
                     (dict(shells=np.arange(1.0, 36.0)), "at most 33 edges, not 35"), (dict(shells=[[1.0, 2.0]]), "one-dimensional"),
                     (dict(shells=2.5), "one-dimensional"), (dict(shells="many"), "shells must be None, an int or an array"),
                     (dict(shells=[1.0, np.nan]), "edges of shells must be finite"), (dict(shells=[0.0, 1.0]), "edges of shells must be > 0"),
                     (dict(shells=[1.0, 1.0]), "strictly ascending"), (dict(shells=[2.0, 1.0]), "strictly ascending"),
                     (dict(triangles="scalene"), "triangles must be one of 'all', 'equilateral', 'isosceles' or a list"),
                     (dict(triangles=[(0, 1)]), "or a list of \\(a, b, c\\)"), (dict(triangles=[]), "or a list of"),
                     (dict(triangles=[(0.0, 1.0, 1.0)]), "or a list of"), (dict(triangles=7), "or a list of"),
                     (dict(triangles=[(0, -1, 0)]), "a triangle names a shell below 0"),
                     (dict(triangles=np.zeros((8193, 3), dtype=int)), "at most 8192 triangles a call, not 8193"),
                     (dict(box_len=0.0), "box_len must be None or a finite number > 0"), (dict(box_len=np.inf), "box_len must be"),
                     (dict(box_len="1"), "box_len must be"), (dict(scale=np.nan), "scale must be a finite number"),
                     (dict(scale=None), "scale must be"), (dict(scale=True), "scale must be"),
                     (dict(t_gamma=-1.0), "t_gamma must be a finite number >= 0"), (dict(t_gamma=np.inf), "t_gamma must be"),
                     (dict(t_gamma="3"), "t_gamma must be")):
        with pytest.raises(ValueError, match=f"bispectrum: .*{what}"):
            bispectrum(None, **kw)
        if "kind" not in kw:
            with pytest.raises(ValueError, match=f"bispectrum: .*{what}"):
                bispectrum(f, **kw)
    with pytest.raises(ValueError, match="bispectrum: a triangle names a shell outside 0 ... 1"):
        bispectrum(f, shells=[1.0, 2.0, 3.0], triangles=[(0, 1, 2)])
    with pytest.raises(ValueError, match="a triangle names a shell outside 0 ... 1"):       # the default shells of N = 8
        bispectrum(f, triangles=[(0, 1, 2)])
    for bad in (np.zeros((8, 8)), np.zeros((8, 8, 4)), np.zeros((4, 4, 4), dtype=complex), [["a"]]):
        with pytest.raises(ValueError, match="field must be a real"):
            bispectrum(bad)
    with pytest.raises(ValueError, match="a host field is analysed as kind 'xh' or 'xhi', not 'density'"):
        bispectrum(f, kind="density")
    with pytest.raises(ValueError, match="1 ... 645 cells a side"):
        spec("x", 646)
    with pytest.raises(ValueError, match="1 ... 645 cells a side"):
        spec("x", 0, shells=[1.0, 2.0])
    with pytest.raises(TypeError):
        bispectrum(f, bins=3)
    _install(monkeypatch, SB.Untouchable(), ready=False)
    with pytest.raises(RuntimeError, match="GPU not initialized"):
        bispectrum(f)


def test_the_two_forms_of_the_module_entry(monkeypatch):
    from pyc2ray_amd import _capi, _residency
    import pyc2ray_amd as pc2r
    M = _module()
    assert pc2r.bispectrum is M.bispectrum and pc2r.Bispectrum is M.Bispectrum
    N = 12
    lib = _install(monkeypatch, BB.Counting(N))
    monkeypatch.setattr(_residency, "reclaim", lambda *a, **kw: lib.calls.append(("reclaim", a, kw)))
    f = np.random.default_rng(0).random((N, N, N))
    b = M.bispectrum(f, shells=[0.5, 1.5, 2.5, 3.5], triangles=[(2, 0, 1), (1, 1, 1)], box_len=16.0)
    assert lib.names() == ["reclaim", "grid_to_device", "bispectrum"]
    _, up, call = lib.calls
    assert up[1][0] == _capi.GRID_XH and np.array_equal(up[1][1], f)
    assert call[1][:3] == (_capi.PS_XH, 1.0, 0.0) and call[1][3].tolist() == [1, 3, 7, 13] and call[1][3].dtype == np.uint32
    assert call[1][4].tolist() == [[2, 0, 1], [1, 1, 1]] and call[1][4].dtype == np.int32 and call[2] == {}
    assert (b.kind, b.N, b.box_len, b.aliased) == ("xh", N, 16.0, False) and b.n_modes.tolist() == [10, 20, 30]
    assert b.sum_iii.tolist() == [6.25, 8.0] and np.array_equal(b.moments, BB.MOMENTS)
    lib.calls.clear()
    b = M.bispectrum(f, kind="xhi", triangles="equilateral")         # the complement; the default shells of N = 12
    assert lib.names() == ["reclaim", "grid_to_device", "bispectrum"] and lib.calls[2][1][0] == _capi.PS_XHI
    assert lib.calls[2][1][3].tolist() == [1, 3, 7, 13] and lib.calls[2][1][4].tolist() == [[0, 0, 0], [1, 1, 1], [2, 2, 2]]
    lib.calls.clear()
    b = M.bispectrum(None, scale=25.0, t_gamma=30.0)                  # the device grids where they lie: no reclaim, no upload
    assert lib.names() == ["bispectrum"] and lib.calls[0][1][:3] == (_capi.PS_HI, 25.0, 30.0)
    assert lib.calls[0][1][4].tolist() == BR.all_triangles(np.arange(0, 4) + 0.5).tolist()
    assert (b.kind, b.N, b.box_len, b.L) == ("dtb", N, None, 12.0)
    assert np.isnan(b.B[b.triangles.sum(axis=1) == 7]).all() and np.isfinite(b.B[b.triangles.sum(axis=1) != 7]).all()
    lib.calls.clear()
    assert M.bispectrum(None, kind="density", shells=2).edges.tolist() == [0.5, 2.0, 3.5] and lib.calls[0][1][0] == _capi.PS_DENSITY


def test_the_class_passes_scale_t_gamma_and_box_len(tmp_path, monkeypatch):
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.c2ray_base as B
    from pyc2ray_amd import _capi
    # no per-step switch: the tuples of step statistics are what they were
    assert B.C2Ray._step_statistics() == B.C2Ray._STEP_STATISTICS + ("redshift_space_stats", "lyman_alpha_stats")
    assert not any("bispectrum" in name for name in B.C2Ray._step_statistics())
    assert "no per-step switch" in B.C2Ray.bispectrum.__doc__ and "sim.bispectrum()" in B.C2Ray.bispectrum.__doc__
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 12
        sim = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        assert not hasattr(sim, "bispectrum_stats") and not hasattr(sim, "last_bispectrum")
        sim.gpu = True
        lib = _install(monkeypatch, BB.Counting(N))
        box, scale = sim.boxsize_c / B.Mpc, sim.brightness_temperature_scale()
        b = sim.bispectrum()
        # not resident: the object's three grids go up, then the one library call
        assert lib.names() == ["grid_to_device"] * 3 + ["bispectrum"]
        assert [c[1][0] for c in lib.calls[:3]] == [_capi.GRID_XH, _capi.GRID_NDENS, _capi.GRID_TEMP]
        assert lib.calls[3][1][:3] == (_capi.PS_HI, scale, 0.0) and lib.calls[3][1][3].tolist() == [1, 3, 7, 13]
        assert (b.kind, b.N, b.box_len) == ("dtb", N, box)
        lib.calls.clear()
        b = sim.bispectrum(spin="kinetic", triangles="isosceles", shells=[1.0, 2.0, 4.0], box_len=5.0, scale=2.0)
        t_gamma = float(sim._ld["Cosmology"]["cmbtemp"]) * (1.0 + float(sim.zred))
        assert lib.calls[-1][1][:3] == (_capi.PS_HI, 2.0, t_gamma) and lib.calls[-1][1][3].tolist() == [1, 4, 16]
        assert lib.calls[-1][1][4].tolist() == [[0, 0, 0], [0, 0, 1], [1, 1, 0], [1, 1, 1]] and b.box_len == 5.0
        # resident: the grids where they lie
        sim.device_resident = True
        sim._device_newer = {"xh"}
        sim._host_newer = set()
        lib.calls.clear()
        sim.bispectrum(kind="xhi")
        assert lib.names() == ["bispectrum"] and lib.calls[0][1][0] == _capi.PS_XHI
        for kw, what in ((dict(field=np.zeros((N, N, N))), "field is not for the class"), (dict(spin="hot"), "spin must be None or 'kinetic'"),
                         (dict(spin="kinetic", t_gamma=3.0), "spin='kinetic' sets t_gamma itself"), (dict(shells=0), "shells as an int"),
                         (dict(triangles="none"), "triangles must be one of")):
            with pytest.raises(ValueError, match=f"C2Ray.bispectrum: .*{what}"):
                sim.bispectrum(**kw)
    finally:
        os.chdir(cwd)
