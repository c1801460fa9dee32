"""CPU: the host side of the halo-catalogue sources: the C-ABI symbols and the enums the header pins, what
HaloCatalogue, SourceModel and halo_sources refuse before the library is touched, the upload bookkeeping of a catalogue on a numpy
stand-in for the library, and the wiring of the class -- its keys, evolve3D(dt) without a list, the list reaching the existing
entries unchanged, last_halo_sources and the log."""
import importlib
import math
import os

import numpy as np
import pytest

import halo_sources_reference as R
import halo_sources_standin_backend as HB

HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN_PARAMS = os.path.join(HERE, "data", "parameters_test.yml")
_ASKING = ("halo_catalogue_state", "halo_catalogue_generation")       # (questions to the library's host bookkeeping)
SOURCES = "Sources:\n  fgamma_hm: 30\n  fgamma_lm: 130.0\n  ts: 3.0\n  m_lm: 1e8\n  m_hm: 1e9\n  suppression: full\n  x_suppress: 0.2\n  f_suppressed: 0.0\n"


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
    return importlib.import_module("pyc2ray_amd.halo_sources")


def _install(monkeypatch, backend, ready=True):
    import pyc2ray_amd.c2ray_base as B
    for mod in (_module(), B):
        monkeypatch.setattr(mod, "load_asora", lambda: backend)
        monkeypatch.setattr(mod, "cuda_is_init", lambda: ready)
    return backend


def _catalogue(N, n=400, seed=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.5 * N, 1.5 * N, size=(n, 3)), 10.0 ** rng.uniform(7.5, 11.0, size=n)


def test_capi_symbols_and_header():
    import ctypes as C
    import pyc2ray_amd as pc2r
    from pyc2ray_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "asora_hip.h")).read()
    assert ("enum { ASORA_HALO_MODEL_NONE = 0, ASORA_HALO_MODEL_FULL = 1, ASORA_HALO_MODEL_PARTIAL = 2, ASORA_HALO_STAGES = 8, "
            "ASORA_HALO_SUMMARY = 5 };") in header
    for name in ("asora_halo_catalogue_to_device", "asora_halo_catalogue_clear", "asora_halo_catalogue_state", "asora_halo_table_to_host",
                 "asora_halo_sources_build", "asora_halo_sources_to_host", "asora_debug_halo_sources_ms"):
        assert f"int {name}(" in header and name in _capi.SIGNATURES, name
    assert (_capi.HALO_MODEL_NONE, _capi.HALO_MODEL_FULL, _capi.HALO_MODEL_PARTIAL, _capi.HALO_STAGES, _capi.HALO_SUMMARY) == (0, 1, 2, 8, 5)
    assert _module().SUPPRESSIONS == R.MODELS == {"none": 0, "full": 1, "partial": 2}
    # the enums the header pins keep their values: the table is no grid, no kernel slot or option is new
    for pinned in ("ASORA_GRID_COUNT = 9", "ASORA_KERNEL_COUNT = 4", "ASORA_KERNEL_SLOTS = 7", "ASORA_OPT_COUNT = 19", "ASORA_LC_STAGES = 4"):
        assert pinned in header, pinned
    assert [len(_capi.SIGNATURES[name][1]) for name in ("asora_halo_catalogue_to_device", "asora_halo_table_to_host", "asora_halo_sources_build",
                                                        "asora_halo_sources_to_host")] == [9, 4, 9, 3]
    for name in ("HaloCatalogue", "SourceModel", "HaloSourceList", "halo_sources", "source_scale"):
        assert getattr(pc2r, name) is getattr(_module(), name)
    lib = _capi.load()                    # (opening the library resolves every declared symbol)
    if not lib.asora_device_ptr(_capi.GRID_NDENS):      # no device initialised in this process: refused as every entry is
        pos, w, counts = np.ones((2, 3)), np.ones(2), (C.c_longlong * 4)(9, 9, 9, 9)
        assert lib.asora_halo_catalogue_to_device(_capi.dptr(pos), _capi.dptr(w), _capi.dptr(w), 2, 1e8, 1e9, 1, 0, counts) == 2
        assert b"halo_catalogue_to_device" in lib.asora_last_error() and list(counts) == [9, 9, 9, 9]
        summary, n = (C.c_ulonglong * 5)(), C.c_longlong(7)
        assert lib.asora_halo_sources_build(_capi.GRID_XH, 1.0, 1.0, 1.0, 0, 0.1, 0.0, summary, C.byref(n)) == 2 and n.value == 7
        assert lib.asora_halo_sources_to_host(None, None, 0) == 2 and lib.asora_halo_table_to_host(None, None, None, 0) == 2
        # what the device holds is host bookkeeping: readable without a device, and nothing is there
        cells, e, gen = C.c_longlong(5), C.c_int(5), C.c_longlong(5)
        assert lib.asora_halo_catalogue_state(C.byref(cells), C.byref(e), C.byref(gen)) == 0 and (cells.value, e.value, gen.value) == (-1, 0, 0)
        assert lib.asora_halo_catalogue_clear() == 0
    assert lib.asora_halo_catalogue_state(None, None, None) == 3
    ms = np.full(_capi.HALO_STAGES, -1.0)
    assert lib.asora_debug_halo_sources_ms(_capi.dptr(ms)) == 0 and np.all(ms >= 0.0)
    assert lib.asora_debug_halo_sources_ms(None) == 3


def test_what_a_catalogue_refuses():
    M = _module()
    pos, mass = _catalogue(8)
    n = mass.size
    for args, kw, what in (
            ((pos[:, :2], mass), {}, "positions must have shape \\(n, 3\\)"),
            ((pos.ravel(), mass), {}, "positions must have shape \\(n, 3\\)"),
            ((pos.astype(complex), mass), {}, "positions must be a real array"),
            ((pos, mass[:-1]), {}, f"masses must have shape \\({n},\\)"),
            ((pos, mass, mass[:5]), {}, f"weights must have shape \\({n},\\)"),
            ((pos, mass, np.array(["a"] * n)), {}, "weights must be a real array"),
            ((pos, mass), dict(m_lm="1e8"), "m_lm must be a number"),
            ((pos, mass), dict(m_hm=float("nan")), "m_hm must be a number"),
            ((pos, mass), dict(m_lm=True), "m_lm must be a number"),
            ((pos, mass), dict(m_lm=2e9, m_hm=1e9), "m_lm must not exceed m_hm"),
            ((pos, mass), dict(wrap=1), "wrap must be a bool"),
            ((pos, mass, -mass), {}, "the weights must be finite and >= 0"),
            ((pos, mass, np.where(np.arange(n) == 7, np.nan, mass)), {}, "the weights must be finite and >= 0"),
            ((pos, np.where(np.arange(n) == 7, np.inf, mass)), {}, "the weights must be finite and >= 0"),
            ((pos, mass, np.full(n, 1e308)), {}, "the sum of the weights is not finite"),
            ((pos, mass), dict(unit=3.0), "unit must be a power of two"),
            ((pos, mass), dict(unit=0.0), "unit must be a power of two"),
            ((pos, mass), dict(unit=-2.0), "unit must be a power of two"),
            ((pos, mass), dict(unit=float("inf")), "unit must be a power of two"),
            ((pos, mass), dict(unit="1"), "unit must be a power of two"),
            ((pos, mass), dict(unit=2.0 ** -1020), "unit must lie between"),
            ((pos, mass), dict(unit=2.0 ** -40), "with unit 2\\^-40 a cell's integer sum could overflow")):
        with pytest.raises(ValueError, match="HaloCatalogue: " + what):
            M.HaloCatalogue(*args, **kw)
    # the rule for the unit, the caller's own, the default weights (a halo below m_lm weighs nothing: a NaN mass is no error)
    cat = M.HaloCatalogue(pos, mass)
    assert cat.unit_exponent == R.unit_exponent(np.where(mass >= 1e8, mass, 0.0)) and cat.unit == 2.0 ** cat.unit_exponent
    assert (cat.n, cat.m_lm, cat.m_hm, cat.wrap, cat.n_cells, cat.below) == (n, 1e8, 1e9, True, None, None)
    assert M.HaloCatalogue(pos, mass, unit=2.0 ** 20).unit_exponent == 20 and M.HaloCatalogue(pos, mass, unit=1).unit_exponent == 0
    holes = np.where(np.arange(n) % 9 == 0, np.nan, mass)
    cat = M.HaloCatalogue(pos, holes, m_lm=1e9, m_hm=1e10, wrap=False)
    assert np.array_equal(cat.weights, np.where(holes >= 1e9, holes, 0.0)) and np.isnan(cat.masses[0])
    # at the edge of the overflow refusal: sum / unit + n / 2 < 2^62
    total = float(np.sum(mass))
    e = math.frexp(total)[1] - 62                      # total / 2^e in [2^61, 2^62)
    assert M.HaloCatalogue(pos, mass, mass, unit=2.0 ** e).unit_exponent == e
    with pytest.raises(ValueError, match="could overflow"):
        M.HaloCatalogue(pos, mass, mass, unit=2.0 ** (e - 1))
    empty = M.HaloCatalogue(np.zeros((0, 3)), np.zeros(0))
    assert (empty.n, empty.unit_exponent) == (0, 0)


def test_what_a_source_model_refuses():
    M = _module()
    good = dict(fgamma_hm=30.0, fgamma_lm=130.0, ts_myr=3.0)
    for kw, what in ((dict(fgamma_hm=-1.0), "fgamma_hm must be a finite number >= 0"), (dict(fgamma_hm="30"), "fgamma_hm must be a finite number"),
                     (dict(fgamma_lm=float("inf")), "fgamma_lm must be a finite number >= 0"), (dict(fgamma_lm=True), "fgamma_lm must be a finite"),
                     (dict(ts_myr=0.0), "ts_myr must be a finite number > 0"), (dict(ts_myr=None), "ts_myr must be a finite number > 0"),
                     (dict(suppression="off"), "suppression must be 'none', 'full' or 'partial'"), (dict(suppression=1), "suppression must be"),
                     (dict(x_suppress=float("nan")), "x_suppress must be a number"), (dict(x_suppress="0.1"), "x_suppress must be a number"),
                     (dict(f_suppressed=1.5), "f_suppressed must be a number in \\[0, 1\\]"), (dict(f_suppressed=-0.1), "f_suppressed must be"),
                     (dict(f_suppressed=float("nan")), "f_suppressed must be a number in")):
        with pytest.raises(ValueError, match="SourceModel: " + what):
            M.SourceModel(**{**good, **kw})
    model = M.SourceModel(30, 0, 3)
    assert (model.fgamma_hm, model.fgamma_lm, model.ts_myr, model.suppression, model.x_suppress, model.f_suppressed) == (30.0, 0.0, 3.0, "none", 0.1, 0.0)
    # the scale is the reference's mass2phot / S_star_ref with the fgamma taken out
    want = 1.98892e33 * 0.044 / (0.27 * 1.222 * 1.67262192369e-24 * 3.0 * 3.15576e13) / 1e48
    assert M.source_scale(3.0, 0.044, 0.27, 1.222) == pytest.approx(want, rel=1e-14) and M.MEAN_MOLECULAR == pytest.approx(1.222, rel=1e-15)


def test_entry_on_the_standin(monkeypatch):
    """halo_sources on the numpy stand-in: what it refuses, the host array uploaded or the device grid read where it lies, the
    scale, and when a catalogue goes up: when first used, after another object's upload, after a new mesh."""
    from pyc2ray_amd import _capi
    from pyc2ray_amd.c2ray_base import FlatLambdaCDMLite
    M = _module()
    N = 8
    pos, mass = _catalogue(N)
    cat, other = M.HaloCatalogue(pos, mass), M.HaloCatalogue(pos[:50], mass[:50], wrap=False)
    model = M.SourceModel(30.0, 130.0, 3.0, suppression="partial", x_suppress=0.3, f_suppressed=0.25)
    cosmo = FlatLambdaCDMLite(70.0, 0.27, 2.726, Ob0=0.044)
    x = np.random.default_rng(4).random((N, N, N))
    lib = _install(monkeypatch, HB.Numpy(N))
    for args, kw, what in (((pos, model), dict(scale=1.0), "catalogue must be a HaloCatalogue, not ndarray"),
                           ((cat, "full"), dict(scale=1.0), "model must be a SourceModel, not str"),
                           ((cat, model), {}, "give either cosmology"), ((cat, model), dict(scale=1.0, cosmology=cosmo), "give either cosmology"),
                           ((cat, model), dict(scale=-1.0), "scale must be a finite number >= 0"), ((cat, model), dict(scale="1"), "scale must be"),
                           ((cat, model), dict(cosmology=FlatLambdaCDMLite(70.0, 0.27)), "cosmology must have Om0 > 0 and Ob0 >= 0"),
                           ((cat, model), dict(cosmology=cosmo, mean_molecular=0.0), "mean_molecular must be a finite number > 0"),
                           ((cat, model), dict(scale=1.0, xh=x, grid=_capi.GRID_XH), "grid selects a device grid and goes with xh=None"),
                           ((cat, model), dict(scale=1.0, xh=x[0]), "xh must be a real \\(N, N, N\\) array"),
                           ((cat, model), dict(scale=1.0, grid=99), "grid must be one of the _capi.GRID_")):
        with pytest.raises(ValueError, match="halo_sources: " + what):
            M.halo_sources(*args, **kw)
    assert lib.calls == [] and cat.n_cells is None           # (refused before the library is touched)
    got = M.halo_sources(cat, model, cosmology=cosmo, xh=x)
    assert [c for c in lib.names() if c not in _ASKING] == ["grid_to_device", "halo_catalogue_to_device", "halo_sources_build"]
    assert lib.calls[0][1][0] == _capi.GRID_XH
    build = [c for c in lib.calls if c[0] == "halo_sources_build"][0][1]
    scale = M.source_scale(3.0, 0.044, 0.27)
    assert build == (_capi.GRID_XH, 30.0, 130.0, cat.unit * scale, _capi.HALO_MODEL_PARTIAL, 0.3, 0.25)
    want_pos, want_flux = R.source_list(pos, mass, cat.weights, x, 1e8, 1e9, True, cat.unit_exponent, 30.0, 130.0, cat.unit * scale, "partial", 0.3, 0.25)
    assert got.src_pos.dtype == np.int32 and np.array_equal(got.src_pos, want_pos) and got.src_flux.tobytes() == want_flux.tobytes()
    assert got.n_active == want_flux.size > 0 and got.n_suppressed > 0 and got.suppression == "partial"
    assert got.mass_hm == got.q_hm * cat.unit and got.mass_lm_active == got.q_lm_active * cat.unit
    assert got.mass_hm + got.mass_lm_active + got.mass_lm_suppressed == pytest.approx(float(np.sum(cat.weights[mass >= 1e8])), rel=1e-12)
    assert got.total_flux == math.fsum(want_flux) and f"{got.n_active:n} active cells" in got.log_line() and "suppression partial" in got.log_line()
    assert (cat.n_cells, cat.outside, cat.nonfinite, cat.below) == (lib.catalogue[0].size, 0, 0, int(np.sum(mass < 1e8))) and cat.on_device(lib)
    # the device grid where it lies: no upload of anything
    lib.calls.clear()
    again = M.halo_sources(cat, model, cosmology=cosmo)
    assert [c for c in lib.names() if c not in _ASKING] == ["halo_sources_build"] and again.src_flux.tobytes() == got.src_flux.tobytes()
    M.halo_sources(cat, model, scale=2.0, grid=_capi.GRID_XH_AV)
    assert lib.calls[-1][1][0] == _capi.GRID_XH_AV and lib.calls[-1][1][3] == cat.unit * 2.0
    # another object's upload, then the first one again; a new mesh
    lib.calls.clear()
    M.halo_sources(other, model, scale=1.0)
    assert other.on_device(lib) and not cat.on_device(lib) and other.outside > 0
    M.halo_sources(cat, model, scale=1.0)
    M.halo_sources(cat, model, scale=1.0)
    assert lib.names().count("halo_catalogue_to_device") == 2 and cat.on_device(lib)
    lib.new_mesh()
    assert not cat.on_device(lib)
    M.halo_sources(cat, model, scale=1.0)
    assert lib.names().count("halo_catalogue_to_device") == 3 and cat.on_device(lib)
    # a catalogue that went up past the class -- the bare entry, or a clear and the bare entry -- is another one: the object uploads again
    lib.halo_catalogue_to_device(pos[:50], mass[:50], mass[:50], 1e8, 1e9, True, 0)
    assert not cat.on_device(lib)
    after_raw = M.halo_sources(cat, model, scale=1.0, grid=_capi.GRID_XH)
    assert cat.on_device(lib) and after_raw.src_flux.tobytes() == M.halo_sources(cat, model, scale=1.0).src_flux.tobytes()
    lib.halo_catalogue_clear()
    lib.halo_catalogue_to_device(pos[:50], mass[:50], mass[:50], 1e8, 1e9, True, 0)
    assert not cat.on_device(lib) and not other.on_device(lib)
    assert M.halo_sources(cat, model, scale=1.0).src_flux.tobytes() == after_raw.src_flux.tobytes()
    # no device
    _install(monkeypatch, HB.Numpy(N), ready=False)
    with pytest.raises(RuntimeError, match="GPU not initialized"):
        M.halo_sources(cat, model, scale=1.0)
    # an empty list keeps its shapes
    nothing = M.HaloSourceList(np.zeros((0, 3), dtype=np.int32), np.zeros(0), [0, 0, 0, 0, 0], 1.0)
    assert nothing.src_pos.shape == (3, 0) and nothing.src_flux.shape == (0,) and nothing.total_flux == 0.0
    with pytest.raises(ValueError, match="one position and one flux per active source"):
        M.HaloSourceList(np.zeros((2, 3)), np.zeros(2), [3, 0, 0, 0, 0], 1.0)


def test_class_plumbing(tmp_path, monkeypatch):
    import pyc2ray_amd as pc2r
    import pyc2ray_amd.c2ray_base as B
    from pyc2ray_amd import _capi
    M = _module()
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N = 8
        pos, mass = _catalogue(N)
        flux1, pos1 = np.ones(1), np.ones((3, 1), dtype=int)
        plain = pc2r.C2Ray_Test(PLAIN_PARAMS, N, False)
        assert plain.halo_catalogue is None and plain.source_model is None and plain.last_halo_sources is None and plain.halo_mass_thresholds == {}
        with pytest.raises(ValueError, match="C2Ray.evolve3D: no sources: pass src_flux and src_pos, or assign halo_catalogue .* and source_model"):
            plain.evolve3D(1.0e10)
        with pytest.raises(ValueError, match="C2Ray.evolve3D: src_flux and src_pos come together or not at all"):
            plain.evolve3D(1.0e10, flux1)
        with pytest.raises(ValueError, match="C2Ray.halo_catalogue: halo_catalogue must be a HaloCatalogue or None, not tuple"):
            plain.halo_catalogue = (pos, mass)
        with pytest.raises(ValueError, match="C2Ray.source_model: source_model must be a SourceModel or None, not dict"):
            plain.source_model = {"fgamma_hm": 30}
        with pytest.raises(ValueError, match="C2Ray.halo_sources: needs halo_catalogue .* and source_model"):
            plain.halo_sources()
        plain.halo_catalogue, plain.source_model = M.HaloCatalogue(pos, mass), M.SourceModel(30.0, 130.0, 3.0)
        with pytest.raises(ValueError, match="C2Ray.halo_sources: halo_sources needs use_gpu=True"):
            plain.evolve3D(1.0e10)
        plain.halo_catalogue = None
        assert plain.halo_catalogue is None
        # the keys of the parameter file
        body = open(PLAIN_PARAMS).read()
        for old, new, what in (("  ts: 3.0\n", "", "Sources: fgamma_hm needs ts"), ("  fgamma_hm: 30\n", "  fgamma_hm: -30\n", "Sources: fgamma_hm must be a finite number >= 0"),
                               ("  suppression: full\n", "  suppression: half\n", "Sources: suppression must be"),
                               ("  x_suppress: 0.2\n", "  x_suppress: high\n", "Sources: x_suppress must be a number"),
                               ("  f_suppressed: 0.0\n", "  f_suppressed: 2\n", "Sources: f_suppressed must be a number in"),
                               ("  m_lm: 1e8\n", "  m_lm: 1e10\n", "HaloCatalogue: m_lm must not exceed m_hm")):
            with open("bad.yml", "w") as f:
                f.write(body + SOURCES.replace(old, new))
            with pytest.raises(ValueError, match=what):
                pc2r.C2Ray_Test("bad.yml", N, False)
        with open("p.yml", "w") as f:
            f.write(body + SOURCES)
        sim = pc2r.C2Ray_Test("p.yml", N, False)
        model = sim.source_model
        assert (model.fgamma_hm, model.fgamma_lm, model.ts_myr, model.suppression, model.x_suppress, model.f_suppressed) == (30.0, 130.0, 3.0, "full", 0.2, 0.0)
        assert sim.halo_mass_thresholds == {"m_lm": 1e8, "m_hm": 1e9} and sim.halo_catalogue is None
        with open("q.yml", "w") as f:
            f.write(body + "Sources:\n  m_lm: 1e9\n  m_hm: 1e10\n")
        other = pc2r.C2Ray_Test("q.yml", N, False)
        assert other.source_model is None
        made = other.new_halo_catalogue(pos, mass)
        assert made is other.halo_catalogue and (made.m_lm, made.m_hm) == (1e9, 1e10) and other.new_halo_catalogue(pos, mass, m_lm=5e8).m_lm == 5e8

        # a step without a list: built from the object's own ionised fraction and handed to the existing entry unchanged
        sim.gpu = True
        lib = _install(monkeypatch, HB.Numpy(N))
        seen = []
        monkeypatch.setattr(B, "evolve3D_resident", lambda *a, **kw: seen.append(("resident", a[2], a[3], a[4])))
        monkeypatch.setattr(B, "evolve3D", lambda *a, **kw: (seen.append(("host", a[2], a[3])), (a[10], np.zeros((N, N, N))))[1])
        sim.density_init(sim.zred_0)
        x0 = np.random.default_rng(8).random((N, N, N))
        sim.xh = np.asfortranarray(x0)
        cat = sim.new_halo_catalogue(pos, mass)
        scale = M.source_scale(3.0, 0.044, 0.27, sim.mean_molecular)
        want = R.source_list(pos, mass, cat.weights, x0, 1e8, 1e9, True, cat.unit_exponent, 30.0, 130.0, cat.unit * scale, "full", 0.2, 0.0)
        sim.device_resident = True
        sim.evolve3D(1.0e10)
        kind, flux, srcpos, uploads = seen[-1]
        assert kind == "resident" and flux is sim.last_halo_sources.src_flux and srcpos is sim.last_halo_sources.src_pos
        assert np.array_equal(srcpos, want[0]) and flux.tobytes() == want[1].tobytes() and _capi.GRID_XH in uploads
        assert sim.last_halo_sources.n_suppressed > 0 and sim._device_newer >= {"xh", "phi_ion"}
        build = [c for c in lib.calls if c[0] == "halo_sources_build"][-1][1]
        assert build == (_capi.GRID_XH, 30.0, 130.0, cat.unit * scale, _capi.HALO_MODEL_FULL, 0.2, 0.0)
        # the second step reads the ionised fraction where it lies: nothing is uploaded or fetched for the list
        lib.calls.clear()
        sim.evolve3D(1.0e10)
        assert [c for c in lib.names() if c not in _ASKING] == ["halo_sources_build"] and sim._device_newer >= {"xh", "phi_ion"}
        assert seen[-1][1].tobytes() == want[1].tobytes()
        # a list of the caller's goes through as ever, and last_halo_sources stays
        last = sim.last_halo_sources
        lib.calls.clear()
        sim.evolve3D(1.0e10, flux1, pos1)
        assert seen[-1][1] is flux1 and seen[-1][2] is pos1 and lib.calls == [] and sim.last_halo_sources is last
        # the host path: the host array goes up for the list
        sim.device_resident = False
        sim.xh = np.asfortranarray(x0)
        sim.evolve3D(1.0e10)
        assert seen[-1][0] == "host" and np.array_equal(seen[-1][2], want[0]) and seen[-1][1].tobytes() == want[1].tobytes()
        assert "grid_to_device" in lib.names() and sim.last_halo_sources is not last
        log = open(sim.logfile).read()
        assert log.count("Halo sources (suppression full): ") == 3 and sim.last_halo_sources.log_line() in log
        # a new snapshot: the next list is built from the new catalogue
        sim.halo_catalogue = M.HaloCatalogue(pos[:100], mass[:100], m_lm=1e8, m_hm=1e9)
        sim.evolve3D(1.0e10)
        assert sim.halo_catalogue.on_device(lib) and not cat.on_device(lib)
        few = R.source_list(pos[:100], mass[:100], sim.halo_catalogue.weights, x0, 1e8, 1e9, True, sim.halo_catalogue.unit_exponent, 30.0, 130.0,
                            sim.halo_catalogue.unit * scale, "full", 0.2, 0.0)
        assert np.array_equal(seen[-1][2], few[0]) and seen[-1][1].tobytes() == few[1].tobytes()
    finally:
        os.chdir(cwd)
        if "sim" in locals():      # (nothing of this object lives on a device: a later step elsewhere must not ask it to fetch)
            sim._device_newer.clear()
            sim.device_resident = False
