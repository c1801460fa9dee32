"""CPU: the oracle's flag for this library's photon-loss convention (oracle.STOPPED_CELLS_LOSE_NOTHING; c2ray_oracle.c): a cell
that deposits nothing -- beyond R_max_LLS or above the column-density cap -- adds 0 to the loss of its sub-box instead of the value
the reference leaves undefined there.  Where no such cell lies on a box face the flag must change nothing (and the flagged oracle
is still the reference's Fortran); where one does, it must change the box counts -- pinned here on the inputs of two GPU tests
whose comparisons with the oracle rest on it.  What the flag states where it matters has no counterpart in the reference."""
import os

import numpy as np
import pytest

import cases
from oracle import oracle as O
from oracle import ref_fortran as F

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLAG = O.STOPPED_CELLS_LOSE_NOTHING
FIELDS = ("phi_ion", "phi_heat", "coldens")


def _run(call, c, flags):
    n = c["thin"].shape[0] - 1
    return call(c["flux"], c["pos"], c["max_subbox"], c["subboxsize"], c["sig"], c["dr"], c["ndens"], c["xh"], c["loss_fraction"],
                c["thin"][:n], c["thick"][:n], c["minlogtau"], c["dlogtau"], c["R"], heat_thin=c["heat_thin"][:n],
                heat_thick=c["heat_thick"][:n], **flags)


@pytest.mark.parametrize("name", list(cases.SUBBOX_CASES))
def test_flag_changes_nothing_where_every_face_cell_deposits(name):
    """R_max_LLS beyond the range, no cell above the cap: byte-identical results, and still tests/golden/subbox.npz."""
    c = cases.subbox_case(name)
    assert c["R"] >= 1000.0
    plain, flagged = _run(O.do_all_sources, c, {}), _run(O.do_all_sources, c, dict(flags=FLAG))
    assert flagged["coldens"].max() < 2e30                # no cell above the column-density cap
    for k in FIELDS:
        assert np.array_equal(plain[k], flagged[k]), k
    assert plain["nsubbox"] == flagged["nsubbox"] and plain["photon_loss"] == flagged["photon_loss"]
    assert np.array_equal(plain["nbox_per_source"], flagged["nbox_per_source"]) and plain["nbox_per_source"].sum() == plain["nsubbox"]
    g = np.load(os.path.join(G, "subbox.npz"))
    assert flagged["nsubbox"] == int(g[name + "__stats"][0])
    np.testing.assert_allclose(flagged["photon_loss"], g[name + "__stats"][1], rtol=1e-13)
    np.testing.assert_allclose(flagged["phi_ion"], g[name + "__phi"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(flagged["coldens"], g[name + "__cd"], rtol=1e-13, atol=0)


@pytest.mark.skipif(not F.available(), reason="oracle/_ref/libc2ray_ref.so not built here")
@pytest.mark.parametrize("name", list(cases.SUBBOX_CASES))
def test_flagged_oracle_is_the_reference_where_the_flag_changes_nothing(name):
    c = cases.subbox_case(name)
    a = _run(O.do_all_sources, c, dict(flags=FLAG, NumTau=c["thin"].shape[0] - 1))
    b = _run(F.do_all_sources, c, dict(NumTau=c["thin"].shape[0] - 1))
    assert np.array_equal(a["phi_ion"], b["phi_ion"]) and np.array_equal(a["coldens"], b["coldens"])
    assert (a["nsubbox"], a["photon_loss"]) == (b["nsubbox"], b["photon_loss"])


def line_aligned_inputs():
    """The inputs of test_gpu_subbox.py::test_tabulated_sweep_on_line_aligned_tables."""
    N, ns = 64, 41
    rng = np.random.default_rng(77)
    thin, thick, dlog = cases.soft_tables(400)
    nd, xh, dr = cases.grid(N, "lognormal", 78, 0.08)
    pos = 1 + rng.integers(0, N, size=(3, ns))
    pos[:, 0], pos[:, 1] = [1, N, 1], [N, N, N]
    flux = rng.uniform(0.5, 4.0, size=ns)
    return dict(flux=flux, pos=pos, box=7, dr=dr, nd=nd, xh=xh, lf=1e-3, thin=thin, thick=thick, dlog=dlog, R=28.0)


def batches_inputs():
    """The inputs of test_gpu_subbox.py::test_tabulated_sweep_in_several_batches."""
    N = 24
    nd, xh, dr = cases.grid(N, "lognormal", 77, 0.3)
    pos, flux = cases.sources(N, 23, 78, flux=2.0)
    flux = flux * (1.0 + 0.1 * np.arange(23))
    thin, thick, dlog = cases.soft_tables()
    n = thin.shape[0] - 1
    return dict(flux=flux, pos=pos, box=3, dr=dr, nd=nd, xh=xh, lf=2e-2, thin=thin[:n], thick=thick[:n], dlog=dlog, R=7.0)


def _oracle(c, flags, lf=None):
    return O.do_all_sources(c["flux"], c["pos"], 1000, c["box"], cases.SIG, c["dr"], c["nd"], c["xh"], c["lf"] if lf is None else lf,
                            c["thin"], c["thick"], cases.MINLOGTAU, c["dlog"], c["R"], flags=flags)


@pytest.mark.parametrize("inputs, stale, zero", [(line_aligned_inputs, 205, 164), (batches_inputs, 92, 69)])
def test_flag_changes_the_box_counts_with_the_radius_inside_the_range(inputs, stale, zero):
    """R_max_LLS inside the range: the faces of the later boxes hold cells beyond the radius, the stale value keeps sources
    growing that lose nothing under the library's convention.  Counts as measured on this oracle."""
    c = inputs()
    plain, flagged = _oracle(c, 0), _oracle(c, FLAG)
    assert (plain["nsubbox"], flagged["nsubbox"]) == (stale, zero)
    assert flagged["nsubbox"] < plain["nsubbox"]
    assert flagged["photon_loss"] != plain["photon_loss"]
    assert np.all(flagged["nbox_per_source"] <= plain["nbox_per_source"])
    # no stop decision of the flagged run is marginal: the GPU tests on these inputs may assert the count exactly
    for f in (1 - 1e-6, 1 + 1e-6):
        assert _oracle(c, FLAG, lf=c["lf"] * f)["nsubbox"] == zero
