"""CPU: what tests/test_gpu_subbox_forms.py rests on (tests/subbox_forms.py).  The sub-box driver's own plan
(asora_debug_subbox_plan: plan_subbox of csrc/raytrace_plan.hpp, no device needed) puts every row on the form the row names at
256 compute units, and on another one source below the row's threshold; and the conditions on the rows' inputs hold on the oracle
alone: sources that stop early and sources that grow to the end, no marginal stop decision, a photon loss that is not zero."""
import numpy as np
import pytest

import subbox_forms as SF

PLAN_OPTIONS = ("OPT_SUBBOX_TABLES", "OPT_PAIR_SOURCES", "OPT_ALIGNED_ROWS", "OPT_GREY_NOTABLES", "OPT_GLOBAL_ATOMICS")


@pytest.fixture(scope="module")
def lib():
    from pyc2ray_amd.load_extensions import load_asora
    return load_asora()


@pytest.fixture
def plan(lib):
    """plan(row, ns, ...): lib.subbox_plan on the row's mesh under the named options, which go back to 0 afterwards."""
    from pyc2ray_amd import _capi

    def call(row, ns=None, cu_count=256, heat=False, has_dump=True, **opts):
        assert set(opts) <= set(PLAN_OPTIONS)
        for k in PLAN_OPTIONS:
            lib.set_option(getattr(_capi, k), opts.get(k, 0))
        r = SF.ROWS[row]
        out = lib.subbox_plan(r["N"], r["R"], SF.MAX_SUBBOX, r["ns"] if ns is None else ns, has_dump=has_dump, heat=heat, cu_count=cu_count)
        out.pop("S_tab")
        return out

    yield call
    for k in PLAN_OPTIONS:
        lib.set_option(getattr(_capi, k), 0)


def test_the_rows_are_those_of_the_issue():
    rows = [(r["N"], r["box"], r["R"], r["lf"]) for r in SF.ROWS.values()]
    assert rows == [(48, 4, 9.0, 2e-2), (48, 5, 13.0, 2e-2), (56, 5, 18.0, 2e-2), (56, 6, 22.0, 2e-2), (56, 6, 24.5, 2e-2),
                    (64, 7, 27.0, 1e-2), (80, 8, 37.0, 1e-2), (36, 4, 1000.0, 2e-2), (48, 5, 1000.0, 2e-2)]
    forms = [(r["units"], r["threads"], r["nsrc"]) for r in SF.ROWS.values() if "units" in r]
    assert forms == [(1, 256, 1), (1, 256, 1), (1, 512, 2), (2, 256, 2), (2, 512, 2), (6, 256, 2), (12, 256, 2)]
    assert [SF.ROWS[k]["fly_threads"] for k in SF.FLY_ROWS] == [128, 256]
    for name, r in SF.ROWS.items():
        assert r["ns"] >= r["least"], name


@pytest.mark.parametrize("row", list(SF.ROWS))
def test_every_row_lands_on_its_form_and_one_source_fewer_does_not(plan, row):
    r = SF.ROWS[row]
    assert plan(row) == SF.expected_plan(row)
    assert plan(row, ns=r["least"]) == SF.expected_plan(row, ns=r["least"])
    below = plan(row, ns=r["least"] - 1)
    form = lambda p: {k: p[k] for k in ("units", "threads", "nsrc", "fly_threads")}
    assert form(below) != form(SF.expected_plan(row, ns=r["least"] - 1)), below
    # every threshold is a lower bound in the number of compute units: the same rows land on smaller devices
    for cu in (128, 64):
        assert plan(row, cu_count=cu) == SF.expected_plan(row), cu
    # heating has no paired form; the on-the-fly kernel's shape does not depend on it
    assert plan(row, heat=True) == SF.expected_plan(row, heat=True)
    if "units" in r:
        # the resident entry returns no column densities: every source goes through the tables
        assert plan(row, has_dump=False) == dict(SF.expected_plan(row), table_sources=r["ns"], fly_sources=0, fly_threads=0)


def test_what_one_source_fewer_takes(plan):
    """Below 2 x 256 workgroups no tables (the on-the-fly kernel sweeps every source); between the tables' threshold and the pairs'
    one source per workgroup; fewer than 32 sources on the fly take 1024 threads."""
    assert plan("sphere_256_r9", ns=512) == dict(table_sources=0, units=0, threads=0, nsrc=0, aligned=0, fly_sources=512, fly_threads=256)
    assert plan("sphere_512_r18", ns=512)["table_sources"] == 0
    for row in ("halves_256_r22", "sectors_256_r27", "pairs_256_r37"):
        r = SF.ROWS[row]
        assert plan(row, ns=r["least"] - 1) == dict(SF.expected_plan(row, ns=r["least"] - 1), nsrc=1), row
    assert plan("halves_512_r24", ns=256)["table_sources"] == 0          # (tables and pairs start together there)
    for row in SF.FLY_ROWS:
        assert plan(row, ns=31) == dict(SF.expected_plan(row, ns=31), fly_threads=1024)


def test_options_override_the_plan(plan):
    assert plan("sphere_256_r9", OPT_SUBBOX_TABLES=1)["table_sources"] == 0
    assert plan("sphere_256_r9", ns=5, OPT_SUBBOX_TABLES=2) == dict(table_sources=4, units=1, threads=256, nsrc=1, aligned=0, fly_sources=1,
                                                                     fly_threads=1024)
    assert plan("fly_256", OPT_SUBBOX_TABLES=2)["units"] == 2            # the range (24 shells) tabulated on request
    assert plan("sectors_256_r27", OPT_PAIR_SOURCES=1)["nsrc"] == 1
    assert plan("sphere_256_r9", OPT_PAIR_SOURCES=2)["nsrc"] == 2
    assert plan("sphere_256_r9", OPT_PAIR_SOURCES=2, heat=True)["nsrc"] == 1
    assert plan("sectors_256_r27", OPT_ALIGNED_ROWS=2)["aligned"] == 1 and plan("halves_512_r24", OPT_ALIGNED_ROWS=2)["aligned"] == 0
    assert plan("sectors_256_r27", OPT_GREY_NOTABLES=1)["table_sources"] == 0
    assert plan("sectors_256_r27", OPT_GLOBAL_ATOMICS=1)["table_sources"] == 0


@pytest.mark.parametrize("row", list(SF.ROWS))
def test_conditions_on_the_inputs_hold_on_the_oracle(row):
    """At least a tenth of the sources stop before the end of their range and at least a tenth grow to it; the loss is not zero;
    and no stop decision is marginal: loss_fraction x (1 +- 1e-6) gives the same boxes, so a different summation order on the
    device cannot flip a count."""
    c = SF.case(row)
    ref = SF.oracle_call(c, heat=False)
    SF.check_conditions(row, ref)
    assert ref["nbox_per_source"].sum() == ref["nsubbox"]
    for f in (1 - 1e-6, 1 + 1e-6):
        assert np.float32(c["lf"] * f) != np.float32(c["lf"])
        assert np.array_equal(SF.oracle_call(c, lf=c["lf"] * f, heat=False)["nbox_per_source"], ref["nbox_per_source"]), f


@pytest.mark.parametrize("row, kw", [("halves_512_r24", dict(own_flux=True)), ("fly_128", dict(own_flux=True)), ("sphere_256_r9", dict(first=40))])
def test_no_marginal_decision_in_the_further_runs(row, kw):
    """The runs with every source's own flux and on a range of the source list: their own oracle calls, the same two conditions."""
    c = SF.case(row)
    ref = SF.oracle_call(c, heat=False, **kw)
    assert ref["photon_loss"] > 0.0
    for f in (1 - 1e-6, 1 + 1e-6):
        assert np.array_equal(SF.oracle_call(c, lf=c["lf"] * f, heat=False, **kw)["nbox_per_source"], ref["nbox_per_source"]), f
