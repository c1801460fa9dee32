"""The open-boundary CPU reference (tests/open_boundary_reference.py) against itself: the cropped result must not depend on what
the padding holds nor on where the box sits in the padded mesh, must equal the periodic trace for an interior source and differ
from it for sources on the faces."""
import numpy as np
import pytest

import cases
import open_boundary_reference as OB
from oracle import oracle as O

N, R, M = 16, 6.0, 24
#: 0-based: two opposite corners, an edge/face mix, the centre, a face
SOURCES = np.array([(0, 0, 0), (15, 15, 15), (0, 7, 15), (8, 8, 8), (3, 15, 0)], dtype=np.int32)


def _case():
    nd, xh, dr = cases.grid(N, "lognormal", 3, 0.08)
    thin, thick, dlog = cases.soft_tables()
    flux = 3.0 * (1.0 + 0.25 * np.arange(len(SOURCES)))
    return dict(ndens=nd, xh=xh, dr=dr, thin=thin, thick=thick, dlog=dlog, flux=flux)


def _open(c, pos, flux, **kw):
    return OB.open_trace(R, cases.SIG, c["dr"], c["ndens"], c["xh"], pos.ravel(), flux, c["thin"], c["thick"], cases.MINLOGTAU,
                         c["dlog"], NumTau=c["thin"].shape[0] - 1, **kw)["phi_ion"]


def _periodic(c, pos, flux):
    return O.asora_do_all_sources(R, cases.SIG, c["dr"], c["ndens"], c["xh"], pos.ravel(), flux, c["thin"], c["thick"],
                                  cases.MINLOGTAU, c["dlog"], NumTau=c["thin"].shape[0] - 1)["phi_ion"]


def test_cropped_trace_is_independent_of_the_padding_and_differs_from_periodic():
    c = _case()
    a = _open(c, SOURCES, c["flux"], M=M, pad=(1e-2, 0.0))
    b = _open(c, SOURCES, c["flux"], M=M, pad=(1e-9, 0.5))
    assert np.array_equal(a, b)                                   # bit for bit: nothing of the padding feeds a cropped cell
    assert np.array_equal(a, _open(c, SOURCES, c["flux"]))        # the smallest padded mesh (22) gives the same
    shifted = _open(c, SOURCES, c["flux"], M=M, offset=1)
    np.testing.assert_allclose(shifted, a, rtol=1e-11, atol=0)    # (another order of summation over the sources' octants)
    per = _periodic(c, SOURCES, c["flux"])
    differ = a != per
    assert 1000 < differ.sum() < N ** 3                           # the wrapped parts of four spheres
    assert np.any((a == 0) & (per != 0)) and not np.any((a != 0) & (per == 0))
    assert np.all(a[differ] < per[differ])                        # open boundaries only ever take rates away


def test_interior_source_is_the_periodic_trace():
    c = _case()
    pos, flux = SOURCES[3:4], c["flux"][3:4]
    assert np.array_equal(_open(c, pos, flux, M=M), _periodic(c, pos, flux))


def test_pair_counts():
    assert OB.rated_pairs(N, R, SOURCES.ravel()) == 1797
    one = OB.rated_pairs(N, R, SOURCES[3:4].ravel())
    assert one == 925 and OB.rated_pairs(N, R, SOURCES.ravel(), periodic=True) == 5 * one
    # with the reference's floating-point distance test: what the oracle rates.  The six lattice points exactly on the sphere fall
    # outside by an ulp at this case's cell size and stay inside where dr is a power of two
    c = _case()
    assert OB.rated_pairs(N, R, SOURCES[3:4].ravel(), dr=c["dr"]) == (_periodic(c, SOURCES[3:4], c["flux"][3:4]) != 0).sum() == 919
    assert OB.rated_pairs(N, R, SOURCES.ravel(), dr=2.0 ** 63) == 1797
    assert (_open(dict(c, dr=2.0 ** 63), SOURCES[3:4], c["flux"][3:4]) != 0).sum() == 925


def test_conditions_are_checked():
    c = _case()
    with pytest.raises(ValueError, match="padded mesh"):
        _open(c, SOURCES, c["flux"], M=N + 5)
    with pytest.raises(ValueError, match="offset"):
        _open(c, SOURCES, c["flux"], M=M, offset=M - N + 1)
    with pytest.raises(ValueError, match="N/2 - 1"):
        OB.open_trace(7.0, cases.SIG, c["dr"], c["ndens"], c["xh"], SOURCES.ravel(), c["flux"], c["thin"], c["thick"],
                      cases.MINLOGTAU, c["dlog"])
