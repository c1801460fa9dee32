"""CPU: the numpy statement of the halo-catalogue sources (tests/halo_sources_reference.py) against a plain Python loop over the
haloes with exact integers, the rule for the unit, the error bound of a cell's sum, and invariance under permutation."""
import importlib
import math
from fractions import Fraction

import numpy as np
import pytest

import halo_sources_reference as R

M = importlib.import_module("pyc2ray_amd.halo_sources")      # (the module, not the function of that name the package exports)


def _catalogue(N, n, seed):
    """Haloes in and around the box, masses across both thresholds, a few on the edges of the statement"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, N, size=(n, 3))
    far = rng.random(n) < 0.25
    pos[far] = rng.uniform(-1.5 * N, 2.5 * N, size=(int(far.sum()), 3))
    mass = 10.0 ** rng.uniform(7.0, 11.0, size=n)
    pos[:6] = [[0.0, 1.0, 2.0], [N, N - 2.0 ** -40, -1e-20], [np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [3e9, 0.0, 0.0], [-3.5, 2 * N + 0.5, 1.5]]
    mass[6:10] = [1e8, 1e9, np.nan, 0.999e8]
    return pos, mass


@pytest.mark.parametrize("wrap", [True, False])
def test_statement_against_a_python_loop(wrap):
    N, n = 4, 200
    pos, mass = _catalogue(N, n, 11)
    weight = np.where(np.isnan(mass), 0.0, mass) * np.random.default_rng(12).uniform(0.5, 2.0, size=n)
    e = R.unit_exponent(weight)
    cell, q_hm, q_lm, counts = R.table(pos, mass, weight, N, 1e8, 1e9, wrap, e)
    loop, loop_counts = R.table_loop(pos, mass, weight, N, 1e8, 1e9, wrap, e)
    assert counts == loop_counts and counts["nonfinite"] == 3 and counts["below"] > 0 and (counts["outside"] > 0) == (not wrap)
    assert counts["outside"] + counts["nonfinite"] + counts["below"] < n and counts["n_cells"] > (N ** 3) // 2
    assert list(cell) == sorted(loop) and np.all(np.diff(cell) > 0)
    assert [int(v) for v in q_hm] == [loop[c][0] for c in cell] and [int(v) for v in q_lm] == [loop[c][1] for c in cell]
    assert np.any(q_hm > 0) and np.any(q_lm > 0)
    # the build: per row in Python, with the roundings the statement names
    x = np.random.default_rng(13).random((N, N, N))
    x.ravel()[cell[0]] = 0.1
    x.ravel()[cell[1]] = np.nextafter(0.1, 1.0)
    x.ravel()[cell[2]] = np.nan
    for model, f in (("none", 0.0), ("full", 0.0), ("partial", 0.25)):
        p, flux, summary = R.build(cell, q_hm, q_lm, x, 2.0, 30.0, 1.25e-9, model, 0.1, f)
        rows, sums = [], [0, 0, 0, 0]
        for c, qh, ql in zip(cell, q_hm, q_lm):
            xc = float(x.ravel()[c])
            sup = model != "none" and xc > 0.1
            s = (0.0 if model == "full" else f) if sup else 1.0
            fl = (2.0 * float(int(qh)) + (30.0 * s) * float(int(ql))) * 1.25e-9
            sums[0] += int(sup and ql > 0)
            sums[1] += int(qh)
            sums[2 + int(sup)] += int(ql)
            if fl > 0.0:
                rows.append((c // (N * N), c // N % N, c % N, fl))
        assert [tuple(int(v) for v in r) for r in p] == [r[:3] for r in rows] and list(flux) == [r[3] for r in rows]
        assert summary == [len(rows)] + sums
    assert not (x.ravel()[cell[0]] > 0.1) and x.ravel()[cell[1]] > 0.1


def test_unit_rule_keeps_the_sums_below_2_to_62():
    """Weights over six decades, a million haloes: the sum of ALL the quantised weights -- no cell's sum can be more -- stays below
    2^62, and the unit is not more than a factor 4 coarser than that needs."""
    rng = np.random.default_rng(21)
    for weights in (10.0 ** rng.uniform(8.0, 14.0, size=1_000_000), np.full(1_000_000, 2.0 ** 40), np.array([2.0 ** 70]), np.array([3.0])):
        e = R.unit_exponent(weights)
        q = np.rint(np.ldexp(weights, -e))
        total = sum(int(v) for v in q)
        assert 2 ** 59 < total < 2 ** 62, (e, total)
    assert R.unit_exponent(np.zeros(5)) == 0 and R.unit_exponent(np.zeros(0)) == 0
    assert R.unit_exponent([1.0]) == -61 and R.unit_exponent([1.5]) == -60 and R.unit_exponent([2.0]) == -60
    for total in (1.0, 1.5, 2.0, 3e19, 2.0 ** -30, 0.0):
        assert M.unit_exponent(total) == R.unit_exponent([total])


def test_error_bound_per_cell():
    """|Q unit - the exact sum of the cell's weights| <= (haloes in the cell) unit / 2, with a coarse unit so that the bound bites"""
    N, n = 4, 200
    pos, mass = _catalogue(N, n, 31)
    mass = np.where(np.isnan(mass), 1e7, mass)
    e = 24                                                          # unit 1.7e7: the masses are 0.6 ... 6000 units
    cell, q_hm, q_lm, counts = R.table(pos, mass, mass, N, 1e8, 1e9, True, e)
    exact, members = {}, {}
    for p, m in zip(pos, mass):
        if not all(math.isfinite(v) and abs(v) < 2.0 ** 31 for v in p) or m < 1e8:
            continue
        c = tuple(math.floor(v) % N for v in p)
        index = (c[0] * N + c[1]) * N + c[2]
        exact[index] = exact.get(index, Fraction(0)) + Fraction(float(m))
        members[index] = members.get(index, 0) + 1
    unit = Fraction(2) ** e
    worst = Fraction(0)
    for c, qh, ql in zip(cell, q_hm, q_lm):
        err = abs((int(qh) + int(ql)) * unit - exact[int(c)])
        assert err <= members[int(c)] * unit / 2
        worst = max(worst, err / (members[int(c)] * unit / 2))
    assert worst > Fraction(1, 4)                                   # (the bound is not slack by much)
    assert set(exact) >= set(int(c) for c in cell)


@pytest.mark.parametrize("wrap", [True, False])
def test_invariance_under_permutation(wrap):
    N, n = 5, 3000
    pos, mass = _catalogue(N, n, 41)
    weight = np.where(np.isnan(mass), 0.0, mass)
    e = R.unit_exponent(weight)
    first = R.table(pos, mass, weight, N, 1e8, 1e9, wrap, e)
    order = np.random.default_rng(42).permutation(n)
    second = R.table(pos[order], mass[order], weight[order], N, 1e8, 1e9, wrap, e)
    assert first[3] == second[3]
    for a, b in zip(first[:3], second[:3]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    x = np.random.default_rng(43).random((N, N, N))
    one = R.build(*first[:3], x, 1.0, 10.0, 3e-12, "partial", 0.5, 0.25)
    two = R.build(*second[:3], x, 1.0, 10.0, 3e-12, "partial", 0.5, 0.25)
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes() and one[2] == two[2]
    assert 0 < one[2][1] < first[3]["n_cells"]
    src_pos, src_flux = R.source_list(pos, mass, weight, x, 1e8, 1e9, wrap, e, 1.0, 10.0, 3e-12, "partial", 0.5, 0.25)
    assert src_pos.shape == (3, one[2][0]) and src_pos.min() >= 1 and src_pos.max() <= N and src_flux.tobytes() == one[1].tobytes()


def test_clustered_generator():
    pos, mass = R.clustered(8, 20000, 5)
    assert pos.shape == (20000, 3) and pos.min() >= 0.0 and pos.max() <= 8.0 and mass.min() >= 1e8 and mass.max() <= 1e13
    per_cell = np.bincount((np.floor(pos).astype(int) % 8 * [64, 8, 1]).sum(axis=1), minlength=512)
    assert per_cell.max() > 20 * max(1, np.median(per_cell))          # (clustered: the fullest cell far above the typical one)
    assert np.mean(mass < 1e9) > 0.85                                 # dn/dM ~ M^-2: nine in ten in the lowest decade
