"""GPU: every built form of `raytrace_octant_kernel` runs once and meets a reference ("How every built form meets a
reference").  One case per row of RT_FORMS, named by the form's template arguments; tests/form_recipes.py holds the recipe that
makes the library launch that row, tests/test_form_recipes_host.py holds the recipes against the launcher's plan without a device.

A case sets the recipe's options, launches through the ordinary entry of its mode (asora_raytrace_device; the column-density dump
entry for the dump rows; two table sets and per-source table sets for the two-set rows; the f2py-shaped sub-box entry for the six
sub-box rows), puts the options back, and asserts
  * the row: `lib.last_launch_form()` is the recipe's form and row index, that row's launch counter rose by one and no other row's
    did -- a recipe that lands on a neighbouring row fails -- and the geometry tables of the launch have the recipe's shell count
    and largest shell;
  * the numbers: the pattern of non-zero cells equal to the reference's; rates and heating against the oracle at GAMMA_RTOL = 1e-8,
    atol = 0; dumped column densities at 1e-11; on the 257-shell bench the sampled and line values of the oracle-made fixture at
    the same tolerances and its plane sums, block sums and total at the bounds tests/test_gpu_configs.py uses for such digests;
  * rows that leave exact zeros out: values where launch_forms.WELL_LIT allows, the pattern of zeros everywhere, and the count of
    rates left out equal to the oracle's count of (source, cell) pairs rated with exactly +0, which is not 0;
  * paired rows of the per-layout-descriptor family without per-source table sets (SPEC = 0): also against their SPEC = 1 twin
    run on the same sources with both table sets equal, to 1e-11 (only the order of the atomics differs).
The device is initialised once per bench and the references are computed once (form_recipes.reference); the cases are ordered so
that what they share stays in place.
"""
import time

import numpy as np
import pytest

import cases
import form_recipes as FR
import launch_forms as LF
import subbox_forms as SF
from test_gpu_parity import GAMMA_RTOL

pytestmark = pytest.mark.gpu

COLDENS_RTOL = 1e-11
TWIN_RTOL = 1e-11
# the bounds of tests/test_gpu_configs.py (_against_bigconfig_fixture) for plane sums, block sums and the total
SUMS_RTOL, BLOCK_ATOL_OF_MAX, TOTAL_RTOL = 1e-9, 1e-12, 1e-10

_BENCH_ORDER = {b: n for n, b in enumerate(("small", "many_shell", "split", "shells_257"))}
CASES = sorted(FR.RECIPES, key=lambda f: (_BENCH_ORDER[FR.RECIPES[f].bench], FR.RECIPES[f].R, FR.RECIPES[f].ns,
                                          FR.REFERENCE_KIND[FR.RECIPES[f].mode], FR.RECIPES[f].mode))


class _Device:
    """What is on the device: the bench, the medium, the sources."""
    bench = dense = ns = spectra = None
    seconds = {}


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora, load_c2ray
    lib = load_asora()
    dev = _Device()
    yield p, lib, _capi, load_c2ray(), dev
    for k in FR.OPTIONS:
        lib.set_option(getattr(_capi, k), 0)
    if p.cuda_is_init():
        p.device_close()
    print("seconds per bench (device_init, uploads, launches, downloads, comparisons and references):", {k: round(v, 1) for k, v in dev.seconds.items()})


def _table_sets(lib, equal=False):
    """Both table sets of launch_forms.tables() with their heating tables; equal: set 0 twice."""
    sets, dlog = LF.tables()
    use = (sets[0], sets[0]) if equal else sets
    lib.spectra_to_device(*(np.stack([s[q] for s in use]) for q in range(4)))
    return dlog, sets[0][0].shape[0] - 1


def _prepare(asora, rec):
    """The recipe's bench, medium and sources on the device; what is there already stays."""
    p, lib, capi, _, dev = asora
    b = FR.BENCHES[rec.bench]
    if dev.bench != rec.bench:
        if p.cuda_is_init():
            p.device_close()
        lib.set_option(capi.OPT_PLACEMENT_CANDIDATES, 1 if b.N >= 512 else 0)
        try:
            p.device_init(b.N, 8)
        finally:
            lib.set_option(capi.OPT_PLACEMENT_CANDIDATES, 0)
        _table_sets(lib)
        dev.bench, dev.dense, dev.ns, dev.spectra = rec.bench, None, None, None
    dense = rec.mode in ("zeros", "spectra_zeros")
    if dev.dense != dense:
        nd, xh = FR.medium(rec.bench, dense)
        lib.grid_to_device(capi.GRID_NDENS, nd)
        lib.grid_to_device(capi.GRID_XH_AV, xh)
        dev.dense = dense
    spectra = rec.mode.startswith("spectra")
    if (dev.ns, dev.spectra) != (rec.ns, spectra):
        pos0, flux, spec = FR.sources(rec.bench, rec.ns)
        lib.source_data_to_device(pos0, flux, rec.ns)                   # (drops the per-source table sets)
        if spectra:
            lib.source_spectra_to_device(spec)
        dev.ns, dev.spectra = rec.ns, spectra
    sets, dlog = LF.tables()
    return b, dlog, sets[0][0].shape[0] - 1


def _launch(lib, capi, rec, b, dlog, numtau):
    """The recipe's call under its options: ({"phi_ion"[, "phi_heat"]} or {"coldens"}, launches per row during the call)."""
    opts = FR.options(rec)
    before = lib.form_launches()
    out = {}
    try:
        for k, v in opts.items():
            lib.set_option(getattr(capi, k), v)
        if rec.mode.startswith("dump"):
            out["coldens"] = lib.debug_coldens(rec.R, cases.SIG, b.dr, rec.ns - 1, b.N)
        else:
            lib.raytrace_device(rec.R, cases.SIG, b.dr, 0, rec.ns, cases.MINLOGTAU, dlog, numtau)
            out["phi_ion"] = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((b.N,) * 3))
            if opts["OPT_HEATING"]:
                out["phi_heat"] = lib.grid_to_host(capi.GRID_PHI_HEAT, np.empty((b.N,) * 3))
    finally:
        for k in opts:
            lib.set_option(getattr(capi, k), 0)
    return out, (lib.form_launches() - before).astype(np.int64)


def _assert_row(lib, form, launched, tag, geometry=None):
    built = lib.built_forms()
    row = built.index(form)
    got, got_row = lib.last_launch_form()
    assert got is not None, f"{tag}: nothing was launched"
    assert (got, got_row) == (form, row), f"{tag}: the library launched row {got_row} {FR.form_text(got)}, the recipe is for row {row} {FR.form_text(form)}"
    others = {FR.form_text(built[r]): int(n) for r, n in enumerate(launched) if n and r != row}
    assert launched[row] >= 1 and not others, f"{tag}: launches of the row {int(launched[row])}, of other rows {others}"
    if geometry is not None:
        geo = lib.debug_geometry_tables(counts_only=True)[1]
        assert (geo["shells"], geo["max_cells"]) == geometry, f"{tag}: the launch's tables have {geo}, the recipe states {geometry}"


def _against(got, ref, rtol, tag, where=None):
    """Pattern of non-zero cells equal; values at rtol, atol = 0 (where: on those cells only)."""
    w = ref != 0
    assert w.any(), tag
    assert np.array_equal(got != 0, w), f"{tag}: {int(((got != 0) != w).sum())} cells are zero on one side only"
    if where is not None:
        w = w & where
    a, r = got[w], ref[w]
    print(f"{tag}: max rel. difference {np.max(np.abs(a - r) / np.abs(r)):.3e} over {a.size} cells")
    np.testing.assert_allclose(a, r, rtol=rtol, atol=0, err_msg=tag)


def _against_fixture(got, field, pos, rtol, tag):
    g = np.load(FR.fixture_path(field))
    d = FR.digest(got, pos)
    for k in ("vals", "lines"):
        nz = g[k] != 0
        print(f"{tag} {field} {k}: max rel. difference {np.max(np.abs(d[k][nz] - g[k][nz]) / np.abs(g[k][nz])):.3e}")
        np.testing.assert_allclose(d[k], g[k], rtol=rtol, atol=0, err_msg=f"{tag} {field} {k}")
    assert int(d["nonzero"]) == int(g["nonzero"]), f"{tag} {field}"
    assert int((got == 0).sum()) == int(g["zero_inside"]), f"{tag} {field}"
    np.testing.assert_allclose(d["plane_sums"], g["plane_sums"], rtol=SUMS_RTOL, err_msg=f"{tag} {field}")
    np.testing.assert_allclose(d["block_sums"], g["block_sums"], rtol=SUMS_RTOL, atol=BLOCK_ATOL_OF_MAX * float(np.abs(g["block_sums"]).max()),
                               err_msg=f"{tag} {field}")
    np.testing.assert_allclose(float(d["total"]), float(g["total"]), rtol=TOTAL_RTOL, err_msg=f"{tag} {field}")


#: mode -> the fields of the fixture a case of the 257-shell bench is held against, {what the launch returns: field}.  The open rows
#: share the periodic trace: the window of the centred source is the whole box (asserted by the fixture's generator)
FIXTURE_OF = {"tables": {"phi_ion": "phi_ion"}, "heat": {"phi_ion": "phi_ion", "phi_heat": "phi_heat"}, "grey": {"phi_ion": "grey_phi_ion"},
              "dump": {"coldens": "coldens"}, "dump_grey": {"coldens": "coldens"}, "open": {"phi_ion": "phi_ion"},
              "open_heat": {"phi_ion": "phi_ion", "phi_heat": "phi_heat"}}


@pytest.mark.parametrize("form", CASES, ids=FR.form_text)
def test_built_form_launches_its_row_and_meets_its_reference(asora, form):
    p, lib, capi, _, dev = asora
    rec = FR.RECIPES[form]
    tag = f"{FR.form_text(form)} {rec.bench} R={rec.R:g} ns={rec.ns} {rec.mode}"
    t0 = time.perf_counter()
    b, dlog, numtau = _prepare(asora, rec)
    t1 = time.perf_counter()
    out, launched = _launch(lib, capi, rec, b, dlog, numtau)
    t2 = time.perf_counter()
    _assert_row(lib, form, launched, tag, (rec.shells, rec.max_cells))
    assert launched[lib.built_forms().index(form)] == 1, tag
    dump, zeros = rec.mode.startswith("dump"), rec.mode in ("zeros", "spectra_zeros")
    if not dump:
        rated, _ = lib.last_raytrace_counts()
        left_out = lib.last_raytrace_zero_rates()
        if not rec.mode.startswith("open"):
            assert rated == rec.ns * LF.cells_within(b.N, rec.R), tag
        assert (left_out > 0) == zeros, f"{tag}: {left_out} rates left out"
    if rec.bench == "shells_257":
        for key, field in FIXTURE_OF[rec.mode].items():
            _against_fixture(out[key], field, b.pos[0], COLDENS_RTOL if key == "coldens" else GAMMA_RTOL, tag)
    else:
        ref = FR.reference(rec.bench, rec.R, rec.ns, FR.REFERENCE_KIND[rec.mode])
        if dump:
            # the cells the source rates are the cells with a column density (the oracle keeps those of every cell it visits), as
            # tests/test_gpu_parity.py compares a dump
            w = ref["phi_ion"] != 0
            assert np.array_equal(out["coldens"] != 0, w), f"{tag}: {int(((out['coldens'] != 0) != w).sum())} cells have a column density or a rate, not both"
            np.testing.assert_allclose(out["coldens"][w], ref["coldens"][w], rtol=COLDENS_RTOL, atol=0, err_msg=tag)
        elif zeros:
            # the exact zeros cell for cell; the values where the shadows are not deep (launch_forms' docstring); the count
            plain = FR.reference(rec.bench, rec.R, rec.ns, "spectra" if rec.mode == "spectra_zeros" else "tables")["phi_ion"]
            lit = ref["phi_ion"] >= LF.WELL_LIT * plain
            assert (lit & (ref["phi_ion"] != 0)).sum() > 0.9 * (ref["phi_ion"] != 0).sum(), tag      # (most lit cells are compared: 93 ... 99.97 %)
            _against(out["phi_ion"], ref["phi_ion"], GAMMA_RTOL, tag + " phi_ion", where=lit)
            print(f"{tag}: {left_out} exact zeros left out of {rated} rated pairs, the oracle has {ref['zero_pairs']}")
            assert left_out == ref["zero_pairs"], tag
        else:
            _against(out["phi_ion"], ref["phi_ion"], GAMMA_RTOL, tag + " phi_ion")
            if "phi_heat" in out:
                _against(out["phi_heat"], ref["phi_heat"], GAMMA_RTOL, tag + " phi_heat")
    if form[10] and form[8] == 2 and not form[11]:
        # SPEC = 0: the same sources through the SPEC = 1 twin, both table sets equal
        twin = form[:11] + (1,) + form[12:]
        try:
            _table_sets(lib, equal=True)
            lib.source_spectra_to_device(FR.sources(rec.bench, rec.ns)[2])
            out2, launched2 = _launch(lib, capi, rec, b, dlog, numtau)
        finally:
            _table_sets(lib)
            dev.ns = None                                                # (the sources go up again, without table sets)
        _assert_row(lib, twin, launched2, tag + " twin")
        assert np.array_equal(out2["phi_ion"] != 0, out["phi_ion"] != 0), tag
        np.testing.assert_allclose(out2["phi_ion"], out["phi_ion"], rtol=TWIN_RTOL, atol=0, err_msg=tag + " twin")
    t3 = time.perf_counter()
    dev.seconds[rec.bench] = dev.seconds.get(rec.bench, 0.0) + t3 - t0
    print(f"{tag}: wall {t3 - t0:.2f} s (set-up {t1 - t0:.2f}, launch and download {t2 - t1:.2f}, references and comparisons {t3 - t2:.2f})")


@pytest.mark.parametrize("form", list(FR.SUBBOX_RECIPES), ids=FR.form_text)
def test_sub_box_form_launches_its_row_and_meets_the_oracle(asora, form):
    """The six sub-box rows, one row of tests/subbox_forms.py each, compared as tests/test_gpu_subbox_forms.py does: the oracle in
    the library's loss convention, box count exact, loss and rates 1e-8, the dumped source's column densities 1e-11."""
    import test_gpu_subbox_forms as TS
    p, lib, capi, c2ray, dev = asora
    row, heat, opts = FR.SUBBOX_RECIPES[form]
    tag = f"{FR.form_text(form)} {row} heat={heat} {opts}"
    ref = SF.reference(row)
    dev.bench = None                                                    # (the entry brings its own device)
    before = lib.form_launches()
    out = TS._call((p, c2ray, lib, capi), row, heat, **opts)
    launched = (lib.form_launches() - before).astype(np.int64)
    TS._against_oracle(out, ref, heat, tag)
    _assert_row(lib, form, launched, tag)
    report = out[5]
    assert launched[lib.built_forms().index(form)] == report["table_launches"] >= 2, (tag, report)
    assert (report["threads"], report["heat"], report["nsrc"]) == (form[0], form[3], form[8]) and report["table_sources"] == SF.ROWS[row]["ns"] - 1, (tag, report)
