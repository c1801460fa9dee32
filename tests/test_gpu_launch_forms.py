"""GPU: the launch forms a production run takes -- chosen from the radius and from about 1000 uploaded sources -- against the CPU
oracle, at the radii where they are used (tests/launch_forms.py): NS sources on the device, of which a few carry
flux; the reference is the oracle over those few.  Every case starts from a fresh device_init, so the line-aligned tables are
decided as on a run's first radius, and asserts the form it ran in: a form that is not reached is a failure.

Modes of a case (one parameter each, so that a case's CPU references, shared through launch_forms.reference, are what a test waits
for, not four of them in a row):
  tables   table rates with every rate added (ASORA_OPT_SKIP_ZERO_RATES = 2) against the oracle, the form, the rated pairs; then
           with the exact zeros left out (= 1): the same grid.  Both once more in the dense medium, which has such zeros
           (launch_forms' docstring: why two media, and where the dense one's values are compared)
  heat     tables + heating: PHI_ION and PHI_HEAT against the oracle, one source per workgroup
  spectra  two table sets, the two bright sources that share a workgroup on different ones: the sum of two oracle traces
  open     ASORA_OPT_OPEN_BOUNDARIES against the padded oracle
Tolerances: GAMMA_RTOL of tests/test_gpu_parity.py for every comparison with the oracle, heating included (tests/test_gpu_heating.py).
"""
import time

import numpy as np
import pytest

import cases
import launch_forms as LF
from test_gpu_parity import GAMMA_RTOL

pytestmark = pytest.mark.gpu

OPTIONS = ("OPT_SKIP_ZERO_RATES", "OPT_HEATING", "OPT_OPEN_BOUNDARIES")
PARAMS = [(name, mode) for name, c in LF.CASES.items() for mode in ("tables", "heat") + (("spectra", "open") if c.extra else ())]


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib, _capi
    for name in OPTIONS:
        lib.set_option(getattr(_capi, name), 0)
    if p.cuda_is_init():
        p.device_close()


def _setup(p, lib, capi, name, mode):
    """A fresh device with the case on it: tables, the NS sources, the medium."""
    case, src = LF.CASES[name], LF.build_sources(name)
    nd, xh, dr = LF.medium(name)
    sets, dlog = LF.tables()
    if p.cuda_is_init():
        p.device_close()
    p.device_init(case.N, 8)
    n = sets[0][0].shape[0]
    if mode == "spectra":
        lib.spectra_to_device(np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets]))
    else:
        p.photo_table_to_device(sets[0][0], sets[0][1])
    if mode == "heat":
        lib.heat_table_to_device(sets[0][2], sets[0][3], n)
    lib.source_data_to_device(src.pos0, src.flux, case.NS)
    if mode == "spectra":
        lib.source_spectra_to_device(src.spec)
    lib.grid_to_device(capi.GRID_NDENS, nd)
    lib.grid_to_device(capi.GRID_XH_AV, xh)
    return case, src, dr, dlog, n - 1


def _trace(lib, capi, case, dr, dlog, numtau, opts):
    """asora_raytrace_device of the whole list under `opts`; (phi_ion, phi_heat or None, variant without skip_zero, rated pairs,
    exact zeros left out)."""
    N = case.N
    try:
        for k, v in opts.items():
            lib.set_option(getattr(capi, k), v)
        lib.raytrace_device(case.R, cases.SIG, dr, 0, case.NS, cases.MINLOGTAU, dlog, numtau)
        phi = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
        heat = lib.grid_to_host(capi.GRID_PHI_HEAT, np.empty((N, N, N))) if opts.get("OPT_HEATING") else None
    finally:
        for k in opts:
            lib.set_option(getattr(capi, k), 0)
    v = {k: x for k, x in lib.last_raytrace_variant().items() if k != "skip_zero"}
    return phi, heat, v, lib.last_raytrace_counts()[0], lib.last_raytrace_zero_rates()


def _against_oracle(got, ref, tag):
    w = ref != 0
    rel = np.max(np.abs(got[w] - ref[w]) / ref[w]) if w.any() else 0.0
    print(f"{tag}: max rel. difference {rel:.3e} over {int(w.sum())} cells, {int((~w).sum())} at exactly 0")
    assert w.sum() > 0, tag
    assert np.array_equal(got != 0, w), f"{tag}: {int(((got != 0) != w).sum())} cells are zero on one side only"
    np.testing.assert_allclose(got[w], ref[w], rtol=GAMMA_RTOL, atol=0, err_msg=tag)


@pytest.mark.parametrize("name,mode", PARAMS)
def test_production_form_against_the_oracle(asora, name, mode):
    p, lib, capi = asora
    t0 = time.perf_counter()
    ref = LF.reference(name, "tables" if mode == "heat" else mode)
    t1 = time.perf_counter()
    case, src, dr, dlog, numtau = _setup(p, lib, capi, name, mode)
    N = case.N
    want = LF.expected_variant(case, mode)
    if mode == "spectra":
        # the pair, neighbours in the library's sorted list, on different table sets
        order = LF.sort_order(src.pos0)
        a = int(np.flatnonzero(order == src.pair[0])[0])
        _, fs, ss = lib.sort_sources(src.pos0, src.flux, src.spec)
        assert order[a + 1] == src.pair[1] and ss[a] != ss[a + 1] and fs[a] == src.flux[src.pair[0]] and fs[a + 1] == src.flux[src.pair[1]]
    opts = {"tables": {"OPT_SKIP_ZERO_RATES": 2}, "spectra": {"OPT_SKIP_ZERO_RATES": 2}, "heat": {"OPT_HEATING": 1},
            "open": {"OPT_OPEN_BOUNDARIES": 1}}[mode]
    phi, heat, v, rated, _ = _trace(lib, capi, case, dr, dlog, numtau, opts)
    tag = f"{name} {mode}"
    print(f"{tag}: variant {v}")
    assert v == want, f"{tag}: the library took {v}, the table expects {want}"
    # the host-only window on the launcher's plan (asora_debug_launch_plan), fed this launch's own shell count and largest shell
    # under the options it ran with: the word of the launch that ran, every bit of it, and a form that is built
    ran, geo = lib.last_raytrace_variant(), lib.debug_geometry_tables(counts_only=True)[1]
    try:
        for k, x in opts.items():
            lib.set_option(getattr(capi, k), x)
        plan = lib.launch_plan(N, case.R, case.NS, shells=geo["shells"], max_cells=geo["max_cells"], heat=mode == "heat",
                               table_sets=mode == "spectra")
    finally:
        for k in opts:
            lib.set_option(getattr(capi, k), 0)
    assert lib.variant_fields(plan["variant"]) == ran and plan["built"] and plan["form"]["threads"] == geo["threads"], f"{tag}: {plan}, ran {ran}"
    _against_oracle(phi, ref["phi_ion"], tag + " phi_ion")
    if mode == "heat":
        _against_oracle(heat, ref["phi_heat"], tag + " phi_heat")
    if mode != "open":
        assert rated == case.NS * LF.cells_within(N, case.R), tag
    if mode == "tables":
        # ASORA_OPT_SKIP_ZERO_RATES = 1, the exact zeros left out: the same additions of the same values to every cell, so the same
        # grid -- bit for bit where one bright sphere reaches, to the order of the atomics (the same freedom in both runs) where
        # several do.  In this medium no optical depth lies beyond the tables; then in the dense one, where some do
        several = LF.coverage(N, case.R, LF.bright_positions(name)) >= 2
        for medium in ("lognormal", "dense"):
            if medium == "dense":
                lib.grid_to_device(capi.GRID_NDENS, LF.medium(name, True)[0])
                phi, _, v_a, rated, _ = _trace(lib, capi, case, dr, dlog, numtau, {"OPT_SKIP_ZERO_RATES": 2})
                assert v_a == want and rated == case.NS * LF.cells_within(N, case.R), f"{tag} dense: {v_a}, {rated}"
                # against the oracle: the exact zeros cell for cell, the values where the shadows are not deep
                dense_ref = LF.reference(name, "dense")["phi_ion"]
                dark = dense_ref == 0
                assert np.array_equal(phi == 0, dark), f"{tag} dense: {int(((phi == 0) != dark).sum())} cells are zero on one side only"
                lit = dense_ref >= LF.WELL_LIT * ref["phi_ion"]
                lit &= ~dark
                print(f"{tag} dense: {int((dark & (ref['phi_ion'] != 0)).sum())} cells in full shadow, {int((~lit & ~dark).sum())} in deep penumbra")
                assert lit.sum() > 0.99 * (~dark).sum(), tag
                np.testing.assert_allclose(phi[lit], dense_ref[lit], rtol=GAMMA_RTOL, atol=0, err_msg=tag + " dense")
            phi_b, _, v_b, _, left_out = _trace(lib, capi, case, dr, dlog, numtau, {"OPT_SKIP_ZERO_RATES": 1})
            print(f"{tag} {medium}: {left_out} exact zeros left out of {rated} rated pairs")
            assert v_b == want, f"{tag} {medium}: with the zeros left out the library took {v_b}, the table expects {want}"
            assert (left_out > 0) == (medium == "dense"), f"{tag} {medium}: {left_out} left out"
            assert np.array_equal(phi_b[~several], phi[~several]), f"{tag} {medium}"
            assert np.array_equal(phi_b != 0, phi != 0), f"{tag} {medium}"
            np.testing.assert_allclose(phi_b[several], phi[several], rtol=1e-11, atol=0, err_msg=f"{tag} {medium}")
    if mode == "open":
        # the corner sources lose what they sent through the faces: not the periodic rates
        per = LF.reference(name, "tables")["phi_ion"]
        lost = (per != 0) & (LF.coverage(N, case.R, LF.bright_positions(name), periodic=False) == 0)
        assert lost.sum() > 0 and not phi[lost].any(), tag
        phi_p, _, v_p, _, _ = _trace(lib, capi, case, dr, dlog, numtau, {"OPT_SKIP_ZERO_RATES": 2})
        assert not v_p["open"] and phi_p[lost].all(), tag
    print(f"{tag}: wall {time.perf_counter() - t0:.2f} s, of which the CPU reference (if not shared) {t1 - t0:.2f} s")
