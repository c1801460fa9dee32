"""GPU: the sub-box sweep (libc2ray.raytracing.do_all_sources, asora_subbox_raytrace_device) in the launch forms it picks BY
ITSELF at ordinary source counts -- all options at 0, hundreds of sources of real flux, sub-boxes grown over several launches while
sources drop out -- against the CPU oracle in the library's loss convention (oracle.STOPPED_CELLS_LOSE_NOTHING), without any
condition, and what it launched (asora_debug_last_subbox_launch) against the row's form.

The rows, their forms and the oracle calls are tests/subbox_forms.py's; tests/test_subbox_forms_host.py checks without a device
that the plan puts each row on its form at 256 compute units and that the conditions on the inputs hold (mixed early stops, no
marginal stop decision).  Tolerances as in test_gpu_subbox.py: box counts exact, photon loss and rates 1e-8, column densities of
the last source 1e-11 on the same cells.  The forms named by the rows are the ones a device of up to 256 compute units takes
(MI355X: 256); the report is asserted against them and against the plan for the device at hand.
"""
import numpy as np
import pytest

import cases
import subbox_forms as SF

pytestmark = pytest.mark.gpu

RATE_RTOL = 1e-8


@pytest.fixture(scope="module")
def libs():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora, load_c2ray
    yield p, load_c2ray(), load_asora(), _capi
    if p.cuda_is_init():
        p.device_close()


def _close(a, b, rtol):
    scale = np.abs(b).max()
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-14 * scale)


def _call(libs, row, heat, first=0, count=None, **options):
    """A fresh device, the f2py-shaped entry on sources [first, first + count) of the row, the named options set for the call
    alone: (phi, phi_heat, coldens, nbox, loss, launch report)."""
    p, c2ray, asora, capi = libs
    c = SF.case(row)
    N = c["N"]
    count = c["ns"] - first if count is None else count
    sl = slice(first, first + count)
    if p.cuda_is_init():
        p.device_close()
    phi = np.zeros((N, N, N), order="F"); hgrid = np.zeros((N, N, N), order="F")
    cd = np.full((N, N, N), 7.0, order="F")          # the input content must not matter (f90:181)
    zeros = np.zeros_like(c["thin"])
    for k, v in options.items():
        asora.set_option(getattr(capi, k), v)
    try:
        nbox, loss = c2ray.raytracing.do_all_sources(c["flux"][sl], np.asfortranarray(c["pos"][:, sl]), SF.MAX_SUBBOX, c["box"], cd, c["sig"],
                                                     c["dr"], c["ndens"], c["xh"], phi, hgrid, c["lf"], c["thin"], c["thick"],
                                                     c["heat_thin"] if heat else zeros, c["heat_thick"] if heat else zeros,
                                                     c["minlogtau"], c["dlogtau"], c["R"])
        report = asora.last_subbox_launch()
    finally:
        for k in options:
            asora.set_option(getattr(capi, k), 0)
    return phi, hgrid, cd, nbox, loss, report


def _against_oracle(out, ref, heat, tag):
    """Every quantity, unconditionally."""
    phi, hgrid, cd, nbox, loss = out[:5]
    print(f"{tag}: nbox {nbox} / oracle {ref['nsubbox']}, loss {loss:.17g} / oracle {ref['photon_loss']:.17g}, "
          f"max |phi - oracle| / max oracle {np.abs(phi - ref['phi_ion']).max() / ref['phi_ion'].max():.3g}"
          + (f", launched {out[5]}" if len(out) > 5 else ""))
    assert nbox == ref["nsubbox"], tag
    np.testing.assert_allclose(loss, ref["photon_loss"], rtol=RATE_RTOL, err_msg=tag)
    _close(phi, ref["phi_ion"], RATE_RTOL)
    if heat:
        _close(hgrid, ref["phi_heat"], RATE_RTOL)
    else:
        assert not hgrid.any(), tag
    if cd is not None:
        assert np.array_equal(cd != 0, ref["coldens"] != 0), tag               # same cells reached by the last source
        np.testing.assert_allclose(cd, ref["coldens"], rtol=1e-11, err_msg=tag)


def _fly_lds(N, global_shells=0):
    """Both shell buffers of the on-the-fly kernel in LDS: 6 W^2 doubles within 56 KB, unless the option sends them to global memory."""
    W = N // 2 + 1
    return int(6 * W * W * 8 <= 56 * 1024 and not global_shells)


def _expected_report(libs, row, ref, heat, ns, has_dump=True, global_shells=0):
    """The report of a one-batch call: the form from the library's plan for THIS device (the row's own at 256 compute units), the
    launches from the oracle's boxes -- one sweep launch per round while any source of the call grows; the tabulated sweep has
    nothing to launch once the box lies beyond the last shell with a cell inside the radius."""
    p, c2ray, asora, capi = libs
    r = SF.ROWS[row]
    plan = asora.subbox_plan(r["N"], r["R"], SF.MAX_SUBBOX, ns, has_dump=has_dump, heat=heat)
    rounds = int(ref["nbox_per_source"].max())
    tables = plan["table_sources"] > 0
    table_rounds = min(rounds, -(-plan["S_tab"] // r["box"]))
    return dict(valid=1, table_sources=plan["table_sources"], units=plan["units"], threads=plan["threads"], nsrc=plan["nsrc"],
                aligned=0, heat=int(heat and tables), table_launches=table_rounds if tables else 0, fly_sources=plan["fly_sources"],
                fly_threads=plan["fly_threads"], fly_lds_shells=_fly_lds(r["N"], global_shells) if plan["fly_sources"] else 0,
                fly_heat=int(heat and plan["fly_sources"] > 0), fly_launches=rounds if plan["fly_sources"] else 0, batches=1)


@pytest.mark.parametrize("heat", [False, True])
@pytest.mark.parametrize("row", SF.TABLE_ROWS)
def test_tabulated_rows_in_the_form_the_library_picks(libs, row, heat):
    """Without heating tables the library pairs the sources where the row says so; with them it runs the HEAT form, one source
    per workgroup.  The last source's cube runs on the side stream beside the tables: its column densities are compared too."""
    r = SF.ROWS[row]
    ref = SF.reference(row)
    SF.check_conditions(row, ref)
    out = _call(libs, row, heat)
    _against_oracle(out, ref, heat, f"{row} heat={heat}")
    report = out[5]
    assert report == _expected_report(libs, row, ref, heat, r["ns"]), report
    form = {k: report[k] for k in ("table_sources", "units", "threads", "nsrc", "fly_sources", "fly_threads")}
    assert form == dict(table_sources=r["ns"] - 1, units=r["units"], threads=r["threads"], nsrc=1 if heat else r["nsrc"],
                        fly_sources=1, fly_threads=1024), form
    assert report["table_launches"] >= 2                       # boxes grown over several launches


@pytest.mark.parametrize("global_shells", [0, 1])
@pytest.mark.parametrize("heat", [False, True])
@pytest.mark.parametrize("row", SF.FLY_ROWS)
def test_on_the_fly_rows_in_the_form_the_library_picks(libs, row, heat, global_shells):
    """R_max_LLS beyond the range: every source on the on-the-fly kernel, 128 threads for the small box and 256 for the larger,
    boxes grown over several launches with the trailing shell through the global buffer while active[] thins out; shells in LDS
    and (ASORA_OPT_SUBBOX_GLOBAL_SHELLS) in global memory, each judged by the oracle."""
    r = SF.ROWS[row]
    ref = SF.reference(row)
    SF.check_conditions(row, ref)
    out = _call(libs, row, heat, OPT_SUBBOX_GLOBAL_SHELLS=global_shells)
    _against_oracle(out, ref, heat, f"{row} heat={heat} global_shells={global_shells}")
    report = out[5]
    assert report == _expected_report(libs, row, ref, heat, r["ns"], global_shells=global_shells), report
    assert report["fly_lds_shells"] == 1 - global_shells and report["fly_launches"] >= 3
    assert report["fly_threads"] == r["fly_threads"] and report["fly_sources"] == r["ns"] and report["table_sources"] == 0


@pytest.mark.parametrize("row", ["halves_512_r24", "fly_128"])
def test_own_flux_in_the_form_the_library_picks(libs, row):
    """ASORA_OPT_C2RAY_OWN_FLUX = 1: every source rated with its own flux, a paired row and the 128-thread row."""
    r = SF.ROWS[row]
    ref = SF.reference(row, own_flux=True)
    assert ref["photon_loss"] > 0
    out = _call(libs, row, False, OPT_C2RAY_OWN_FLUX=1)
    _against_oracle(out, ref, False, f"{row} own flux")
    assert out[5] == _expected_report(libs, row, ref, False, r["ns"]), out[5]


def test_six_sectors_in_several_batches(libs, monkeypatch):
    """A trailing-shell scratch of 2 MB holds a few dozen of the row's sources: the tabulated sources go in three batches at
    least, the dumped source in the last one; same oracle."""
    row = "sectors_256_r27"
    r = SF.ROWS[row]
    ref = SF.reference(row)
    monkeypatch.setenv("ASORA_SUBBOX_TRAIL_BUDGET", "2000000")
    try:
        out = _call(libs, row, False)
    finally:
        monkeypatch.delenv("ASORA_SUBBOX_TRAIL_BUDGET", raising=False)
    _against_oracle(out, ref, False, f"{row} in batches")
    report = out[5]
    assert report["batches"] >= 3, report
    one = _expected_report(libs, row, ref, False, r["ns"])
    for k in ("table_sources", "units", "threads", "nsrc", "aligned", "heat", "fly_sources", "fly_threads", "fly_lds_shells", "fly_heat"):
        assert report[k] == one[k], (k, report)
    # the dumped source sweeps in the last batch only, for as many rounds as that batch lasts; every batch launches the tables
    assert int(ref["nbox_per_source"][-1]) <= report["fly_launches"] <= int(ref["nbox_per_source"].max())
    assert report["table_launches"] >= report["batches"]


@pytest.mark.parametrize("first", [0, 40])
def test_resident_entry_sweeps_every_source_on_the_tables(libs, first):
    """asora_subbox_raytrace_device after grid_to_device and source_data_to_device: no source returns its column densities, so all
    of them go through the tables -- the whole list, and a range that does not start at the first source."""
    p, c2ray, asora, capi = libs
    row = "sphere_256_r9"
    r, c = SF.ROWS[row], SF.case(row)
    N, ns = c["N"], c["ns"]
    count = ns - first
    ref = SF.reference(row) if first == 0 else SF.oracle_call(c, first=first, count=count)
    if p.cuda_is_init():
        p.device_close()
    p.device_init(N, 8)
    try:
        p.photo_table_to_device(c["thin"], c["thick"])
        pos0, flux = cases.flat_sources(c["pos"], c["flux"])
        asora.source_data_to_device(pos0, flux, ns)
        asora.grid_to_device(capi.GRID_NDENS, c["ndens"])
        asora.grid_to_device(capi.GRID_XH_AV, c["xh"])
        nbox, loss = asora.subbox_raytrace_device(SF.MAX_SUBBOX, c["box"], c["lf"], c["R"], c["sig"], c["dr"], c["minlogtau"], c["dlogtau"],
                                                  c["thin"].shape[0], first, count)
        report = asora.last_subbox_launch()
        phi = asora.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
    finally:
        p.device_close()
    _against_oracle((phi, np.zeros(1), None, nbox, loss, report), ref, False, f"{row} resident from {first}")
    assert report == _expected_report(libs, row, ref, False, count, has_dump=False), report
    assert report["table_sources"] == count and report["fly_sources"] == 0
