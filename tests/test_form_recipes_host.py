"""CPU: what tests/test_gpu_form_recipes.py rests on (tests/form_recipes.py) -- every row of the table of built forms has exactly one
recipe, the launcher's own plan (asora_debug_launch_plan, no device) puts every recipe on its row, the sources and the media have
the properties the recipes rely on, and the seeded inputs of the sparse fixture are the ones it was made from."""
import os

import numpy as np
import pytest

import cases
import form_recipes as FR
import launch_forms as LF
import subbox_forms as SF

FORMS = list(FR.RECIPES)


@pytest.fixture(scope="module")
def lib():
    from pyc2ray_amd.load_extensions import load_asora
    return load_asora()


def test_every_built_form_has_exactly_one_recipe(lib):
    """The rows of RT_FORMS, as the library reports them, against the keys of the two recipe tables: no row without a recipe (a row
    added to the table later fails here), no recipe without a row, none twice."""
    built = lib.built_forms()
    assert len(built) == len(set(built)) == 152
    assert all(len(f) == 13 for f in built)
    keys = list(FR.RECIPES) + list(FR.SUBBOX_RECIPES)
    assert len(keys) == len(set(keys))
    missing, extra = sorted(set(built) - set(keys)), sorted(set(keys) - set(built))
    assert not missing and not extra, f"rows without a recipe: {[FR.form_text(f) for f in missing]}; recipes without a row: {[FR.form_text(f) for f in extra]}"
    # the sub-box rows are the rows with SUBBOX set, the others follow the table's order
    assert set(FR.SUBBOX_RECIPES) == {f for f in built if f[9]}
    assert list(FR.RECIPES) == [f for f in built if not f[9]]
    assert FR.form_text(built[0]) == lib.form_text(built[0]) == "<64,0,0,0,256,0,0,0,1,0,0,1,0>"
    # by bench: the counts the dispatcher's own functions give for what each mesh can reach
    count = {b: sum(r.bench == b for r in FR.RECIPES.values()) for b in FR.BENCHES}
    assert count == {"small": 79, "many_shell": 28, "shells_257": 15, "split": 24}
    assert {r.mode for r in FR.RECIPES.values()} == set(FR.MODES)


def test_launch_counters_and_last_form_without_a_device(lib):
    """Before any launch of this process: the counters are one per row and zero, the last form is (None, -1); reset is harmless."""
    lib.reset_form_launches()
    n = lib.form_launches()
    assert n.shape == (len(lib.built_forms()),) and n.dtype == np.uint64 and not n.any()
    form, row = lib.last_launch_form()
    assert (form is None and row == -1) or lib.built_forms()[row] == form        # (another module of this process may have launched)


@pytest.mark.parametrize("form", FORMS, ids=FR.form_text)
def test_the_plan_of_a_recipe_is_its_row(lib, form):
    """lib.launch_plan with the recipe's mesh, radius, source count, mode flags, options and stated (shells, max_cells) at 256
    compute units plans the recipe's form, and that form is built.  The stated shell count is the dispatcher's own estimate."""
    from pyc2ray_amd import _capi
    rec = FR.RECIPES[form]
    b = FR.BENCHES[rec.bench]
    opts = FR.options(rec)
    plan_opts = [k for k in FR.OPTIONS if k != "OPT_HEATING"]
    try:
        for k in plan_opts:
            lib.set_option(getattr(_capi, k), opts[k])
        plan = lib.launch_plan(b.N, rec.R, rec.ns, cu_count=FR.CU_COUNT, shells=rec.shells, max_cells=rec.max_cells, **FR.plan_flags(rec))
    finally:
        for k in plan_opts:
            lib.set_option(getattr(_capi, k), 0)
    got = tuple(int(v) for v in plan["form"].values())
    assert got == form, f"{rec}: planned {FR.form_text(got)}, the recipe is for {FR.form_text(form)}"
    assert plan["built"] and lib.built_forms().index(form) >= 0
    assert rec.shells == min(int(np.floor(rec.R)), b.N // 2) and rec.ns <= len(b.pos)
    assert plan["use_lds"] == (not form[1])
    # not marginal: the shells stay in or out of LDS with a fifth more or fewer cells
    for mc in (int(0.8 * rec.max_cells), int(1.25 * rec.max_cells)):
        for k in plan_opts:
            lib.set_option(getattr(_capi, k), opts[k])
        try:
            assert lib.launch_plan(b.N, rec.R, rec.ns, cu_count=FR.CU_COUNT, shells=rec.shells, max_cells=mc, **FR.plan_flags(rec))["use_lds"] == plan["use_lds"]
        finally:
            for k in plan_opts:
                lib.set_option(getattr(_capi, k), 0)
    # the mode is what the row is for
    assert bool(form[2]) == rec.mode.startswith("dump") and bool(form[3]) == (rec.mode in ("heat", "open_heat"))
    assert bool(form[5]) == (rec.mode in ("zeros", "spectra_zeros")) and bool(form[6]) == (rec.mode in ("grey", "dump_grey"))
    assert bool(form[12]) == rec.mode.startswith("open") and form[8] == (2 if rec.pair == 2 else 1)
    if rec.mode.startswith("spectra"):
        assert form[10] and form[11] and form[8] == 2
    if form[10] and form[8] == 2 and not form[11]:
        twin = form[:11] + (1,) + form[12:]
        assert FR.RECIPES[twin]._replace(mode=rec.mode) == rec._replace(mode=rec.mode)
        assert FR.RECIPES[twin].mode == {"tables": "spectra", "zeros": "spectra_zeros"}[rec.mode]


@pytest.mark.parametrize("form", list(FR.SUBBOX_RECIPES), ids=FR.form_text)
def test_the_plan_of_a_sub_box_recipe_is_its_row(lib, form):
    from pyc2ray_amd import _capi
    row, heat, opts = FR.SUBBOX_RECIPES[form]
    r = SF.ROWS[row]
    try:
        for k, v in opts.items():
            lib.set_option(getattr(_capi, k), v)
        plan = lib.subbox_plan(r["N"], r["R"], SF.MAX_SUBBOX, r["ns"], has_dump=True, heat=heat, cu_count=FR.CU_COUNT)
    finally:
        for k in opts:
            lib.set_option(getattr(_capi, k), 0)
    assert plan["table_sources"] == r["ns"] - 1 and plan["fly_sources"] == 1
    assert (plan["threads"], int(heat), 256, plan["nsrc"]) == (form[0], form[3], form[4], form[8])
    assert form[9] and form[7] and not form[1] and not form[2]


@pytest.mark.parametrize("bench", list(FR.BENCHES))
def test_sources_of_a_bench(lib, bench):
    """The corner source first; the second and third overlap by more than half at every radius of the bench and are neighbours in
    the library's sorted list of four, at an even position: they share a workgroup in the paired rows."""
    b = FR.BENCHES[bench]
    pos0, flux, spec = FR.sources(bench, len(b.pos))
    assert pos0.dtype == np.int32 and pos0.min() >= 0 and pos0.max() < b.N and np.all(flux > 0)
    assert b.dr == 2.0 ** round(np.log2(b.dr))                              # lattice points on a sphere of integer radius are inside
    if bench == "shells_257":
        assert b.pos == ((256, 256, 256),) and b.N == 512
        return
    assert b.pos[0] == (0, 0, 0)
    ps, fs, ss = lib.sort_sources(pos0, flux, spec)
    ps = ps.reshape(-1, 3)
    assert [tuple(p) for p in ps] == [b.pos[0], b.pos[3], b.pos[1], b.pos[2]]
    assert ss[2] != ss[3] and ss[0] != ss[1]                                # both workgroups of the paired rows hold two table sets
    radii = sorted({r.R for r in FR.RECIPES.values() if r.bench == bench})
    for R in radii:
        if b.N > 136:                               # large mesh, spheres far from the window's edge: count in the offsets of the second source
            assert R < b.N // 2 - 1
            d = np.array(b.pos[2]) - np.array(b.pos[1])
            (_, di), (_, dj), (_, dk) = FR.window(b.N, R, b.pos[1])
            inside = (di[:, None, None] ** 2 + dj[None, :, None] ** 2 + dk[None, None, :] ** 2) <= R * R
            both = inside & (((di - d[0])[:, None, None] ** 2 + (dj - d[1])[None, :, None] ** 2 + (dk - d[2])[None, None, :] ** 2) <= R * R)
            assert both.sum() > 0.5 * inside.sum(), (bench, R)
        else:
            ra, rb = LF.reach(b.N, R, b.pos[1]), LF.reach(b.N, R, b.pos[2])
            assert (ra & rb).sum() > 0.5 * ra.sum(), (bench, R)
            assert FR.reach_values(ra, R, b.pos[1]).all() and FR.reach_values(ra, R, b.pos[1]).size == ra.sum()      # reach_values restates reach


def test_reach_values_with_open_boundaries():
    N = 24
    g = np.arange(N ** 3, dtype=np.float64).reshape(N, N, N)
    for R in (5.0, 1000.0):
        for pos in ((0, 0, 0), (23, 23, 23), (3, 20, 11)):
            for periodic in (True, False):
                assert np.array_equal(np.sort(FR.reach_values(g, R, pos, periodic)), np.sort(g[LF.reach(N, R, pos, periodic)])), (R, pos, periodic)


@pytest.mark.parametrize("separable", [False, True])
def test_media_keep_nhi_positive_and_the_dense_one_holds_cells_beyond_the_table(separable):
    """On a small mesh with the generator of the benches: nHI > 0, x within [1e-4, 1e-2]; the dense variant differs in one cell of
    3000 and on the plate in front of the corner source, whose cells all lie beyond the last table entry -- at the cell size of
    every bench."""
    N = 40
    sets, dlog = LF.tables()
    last = 10.0 ** (cases.MINLOGTAU + (sets[0][0].shape[0] - 2) * dlog)
    nd, xh = FR.make_medium(N, 7, separable)
    nd2, xh2 = FR.make_medium(N, 7, separable)
    assert np.array_equal(nd, nd2) and np.array_equal(xh, xh2)              # regenerable from the seed
    dn, dx = FR.make_medium(N, 7, separable, dense=True)
    assert np.array_equal(dx, xh)
    for a in (nd, dn):
        nhi = a * (1.0 - xh)
        assert np.isfinite(nhi).all() and nhi.min() > 0.0
    assert xh.min() >= 1e-4 and xh.max() <= 1e-2
    assert len(np.unique(nd)) > N ** 3 // 2                                 # no two cells alike: a wrong cell shows
    changed = dn != nd
    plate = np.arange(-FR.PLATE_HALF_WIDTH, FR.PLATE_HALF_WIDTH + 1) % N
    assert changed[np.ix_([FR.PLATE_PLANE], plate, plate)].all()
    assert 0.3 * (N ** 3 // FR.DENSE_ONE_IN) < changed.sum() - plate.size ** 2 <= N ** 3 // FR.DENSE_ONE_IN
    assert np.array_equal(dn[changed], nd[changed] * FR.DENSE_FACTOR)
    for b in FR.BENCHES.values():
        tau = cases.SIG * (nd * (1.0 - xh)) * b.dr
        assert np.median(tau) < 0.1
        assert (cases.SIG * (dn * (1.0 - xh)) * b.dr)[changed].min() > 1.02 * last
        if b.separable == separable:
            assert tau.max() * b.N < 0.2 * last                             # no path through the box comes near the tables' end


def test_small_references_have_the_pattern_of_the_reach_and_exact_zeros_in_the_dense_medium():
    """The small bench at R = 20, three sources: the oracle's rates are non-zero exactly on the cells a source reaches; in the
    dense medium some of them are exactly +0 (behind the plate), counted per (source, cell) pair, most cells are lit well enough to
    be compared, and the spheres of the second and third source overlap."""
    b = FR.BENCHES["small"]
    ref = FR.reference("small", 20.0, 3, "tables")
    cov = LF.coverage(b.N, 20.0, np.array(b.pos[:3]))
    assert np.array_equal(ref["phi_ion"] != 0, cov > 0) and np.array_equal(ref["phi_heat"] != 0, cov > 0)
    assert (cov >= 2).sum() > 0.5 * LF.cells_within(b.N, 20.0)
    dense = FR.reference("small", 20.0, 3, "dense")
    dark = (dense["phi_ion"] == 0) & (cov > 0)
    assert 0 < dark.sum() <= dense["zero_pairs"] < 0.1 * 3 * LF.cells_within(b.N, 20.0)
    # (the plate sits next to the source and shades a wider cone than launch_forms.medium's: 98.7 % here)
    assert (dense["phi_ion"] >= LF.WELL_LIT * ref["phi_ion"])[dense["phi_ion"] != 0].mean() > 0.95
    opn = FR.reference("small", 20.0, 3, "open")
    lost = (cov > 0) & (LF.coverage(b.N, 20.0, np.array(b.pos[:3]), periodic=False) == 0)
    assert lost.sum() > 100 and not opn["phi_ion"][lost].any() and not opn["phi_heat"][lost].any()
    inside = LF.coverage(b.N, 20.0, np.array(b.pos[1:3]), periodic=False) > 0
    far = inside & (LF.coverage(b.N, 20.0, np.array(b.pos[:1])) == 0)       # where the corner source adds nothing: the periodic rates
    np.testing.assert_allclose(opn["phi_ion"][far], ref["phi_ion"][far], rtol=1e-13, atol=0)


def test_the_fixture_was_made_from_the_seeded_inputs():
    """The separable medium of the 257-shell bench and the tables, regenerated, against the checksums stored in every file of the
    fixture; the stored properties of the 512^3 traces (asserted by the generator) are the ones the GPU test relies on."""
    nd, xh = FR.medium("shells_257")
    sums = FR.input_checksums(nd, xh)
    assert sums[6] > 0.0 and sums[4] >= 1e-4 and sums[5] <= 1e-2
    b = FR.BENCHES["shells_257"]
    idx = FR.sample_indices(b.N)
    assert idx.shape == (FR.NSAMPLE,) and len(np.unique(idx)) == FR.NSAMPLE and idx.max() < b.N ** 3
    size = 0
    for field in FR.FIXTURE_FIELDS:
        path = FR.fixture_path(field)
        size += os.path.getsize(path)
        assert os.path.getsize(path) < 1 << 20, path
        g = np.load(path)
        np.testing.assert_allclose(g["inputs"], sums, rtol=1e-13, atol=0, err_msg=field)
        assert g["vals"].shape == (FR.NSAMPLE,) and g["lines"].shape == (3, b.N) and g["plane_sums"].shape == (b.N,)
        assert g["block_sums"].shape == ((b.N // 16) ** 3,)
        np.testing.assert_allclose(g["plane_sums"].sum(), float(g["total"]), rtol=1e-12)
        np.testing.assert_allclose(g["block_sums"].sum(), float(g["total"]), rtol=1e-12)
        if field != "coldens":
            assert int(g["nonzero"]) == b.N ** 3 and int(g["zero_inside"]) == 0 and g["vals"].min() > 0
    print(f"fixture: {size} bytes in {len(FR.FIXTURE_FIELDS)} files")
