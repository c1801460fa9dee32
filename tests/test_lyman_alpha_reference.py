"""CPU: the numpy/scipy statement of the Lyman-alpha forest (tests/lyman_alpha_reference.py) against a 40-digit
evaluation of the same sums and against known answers, and its gap finder against a brute-force run counter."""
import math
import os

import mpmath
import numpy as np
import pytest

import lyman_alpha_reference as R
from pyc2ray_amd import _capi, lyman_alpha as LA


def _tau_mp(lo, hi, bt, g, W):
    """The sums of the header in 40 digits from the double lo, hi, bt, g of ONE line."""
    mpmath.mp.dps = 40
    N = lo.size
    mp = mpmath.mpf
    six, half = mp(6), mp("0.5")
    tau = []
    for p in range(N):
        total = mp(0)
        for o in range(-W, W + 1):
            q = (p - o) % N
            l, h, b, s = mp(float(lo[q])), mp(float(hi[q])), mp(float(bt[q])), mp(o) + half
            if float(hi[q]) - float(lo[q]) >= R.FLOOR:
                if s - h > six * b or l - s > six * b:
                    continue
                w = half * (mpmath.erf((s - l) / b) - mpmath.erf((s - h) / b)) / (h - l)
            else:
                t = (s - half * (l + h)) / b
                if abs(t) > six:
                    continue
                w = mp(R.INV_SQRT_PI) / b * mpmath.exp(-(t * t))
            total += w * mp(float(g[q]))
        tau.append(total)
    return tau


@pytest.mark.parametrize("seed", [1, 2])
def test_reference_against_40_digits(seed):
    """Within (2 W + 16) eps S[p] (derived in lyman_alpha_reference.bound); the ratio is printed."""
    N = 16
    x, n, T, v = R.fields(N, seed)
    b_scale = 0.5 / math.sqrt(3.0e4)
    lo, hi, bt, g = R.line_quantities(x, n, T, v, 0.5, b_scale, 1.0)            # lines along axis 2
    W = R.window_of(float(np.max(R.reach_of(lo, hi, bt))), N)
    assert 2 * W + 1 <= N
    tau = R.optical_depth(lo, hi, bt, g, W)
    bnd = R.bound(lo, hi, bt, g, W)
    worst, degenerate = 0.0, 0
    for line in [(0, 0), (3, 5), (5, 11), (11, 4), (15, 15), (7, 5), (2, 11)]:
        sel = line
        exact = _tau_mp(lo[sel], hi[sel], bt[sel], g[sel], W)
        degenerate += int(np.sum(hi[sel] - lo[sel] < R.FLOOR))
        for p in range(N):
            err = abs(mpmath.mpf(float(tau[sel][p])) - exact[p])
            assert err <= mpmath.mpf(float(bnd[sel][p])), (line, p, float(err), float(bnd[sel][p]))
            if bnd[sel][p] > 0:
                worst = max(worst, float(err) * (2 * W + 16) / float(bnd[sel][p]))
    print(f"worst error {worst:.3f} eps S, W = {W}, {degenerate} degenerate cells among the lines")
    assert degenerate >= 1


def test_uniform_neutral_box_at_rest():
    """Every pixel sees the whole of every profile that reaches it: tau = tau_scale n, for resolved and for unresolved profiles."""
    N = 24
    n_val, tau_scale = 0.7, 3.0
    x, n = np.zeros((N, N, N)), np.full((N, N, N), n_val)
    for T, b_scale in ((2.25, 1.0), (1.0, 0.01)):                  # bt = 1.5 cells; T = 1 K and bt = 0.01 << 1
        r = R.forest(x, n, np.full((N, N, N), T), None, 2, 1.0, b_scale, tau_scale, gap_threshold=0.2)
        assert r["clipped"] == 0 and r["degenerate"] == 0 and r["window"] == max(1, math.ceil(6 * b_scale * math.sqrt(T) + 0.5))
        assert np.all(np.abs(r["tau"] - tau_scale * n_val) <= r["bound"]), np.max(np.abs(r["tau"] - tau_scale * n_val) / r["bound"])
        if b_scale == 0.01:
            assert np.all(r["tau"] == tau_scale * n_val)           # (erf(+-50) = +-1 exactly: one term, weight 1)
        # tau = 2.1, F = 0.122: with the threshold at 0.2 every line is one gap; at the default 0.05 (below) none is
        assert r["n_gaps"] == N * N and r["full_lines"] == N * N and r["gaps"][N] == N * N and r["longest"] == N
    r = R.forest(x, n, np.full((N, N, N), 1.0), None, 2, 1.0, 0.01, tau_scale)
    assert r["n_gaps"] == 0 and r["n_dark"] == 0 and r["longest"] == 0 and not r["gaps"].any()


def test_single_neutral_cell_is_an_erf_profile_symmetric_about_its_centre():
    N, q0 = 32, 13
    x = np.ones((N, N, N))
    x[2, 3, q0] = 0.0
    n, T = np.full((N, N, N), 2.0), np.full((N, N, N), 4.0)
    b = 0.6 * 2.0                                                  # bt = b_scale sqrt(T) = 1.2 cells
    r = R.forest(x, n, T, None, 2, 1.0, 0.6, 5.0)
    line = r["tau"][2, 3]
    want = np.array([0.5 * (math.erf((p - q0 + 0.5) / b) - math.erf((p - q0 - 0.5) / b)) * 10.0 for p in range(N)])
    want[np.abs(np.arange(N) - q0) > r["window"]] = 0.0
    assert np.allclose(line, want, rtol=1e-13, atol=1e-300)
    for m in range(1, r["window"] + 1):
        assert abs(line[q0 + m] - line[q0 - m]) <= 4 * R.EPS * line[q0]
    assert np.all(np.delete(r["tau"].reshape(-1, N), 2 * N + 3, axis=0) == 0.0) and line.sum() == pytest.approx(10.0, rel=1e-12)


def test_constant_integer_velocity_shifts_bit_for_bit():
    N = 20
    x, n, T, _ = R.fields(N, 3)
    b_scale = 0.5 / math.sqrt(3.0e4)
    rest = R.forest(x, n, T, None, 1, 1.0, b_scale, 1.0)
    for shift in (3, -2):
        moved = R.forest(x, n, T, np.full((N, N, N), float(shift)), 1, 1.0, b_scale, 1.0, window=rest["window"] + abs(shift))
        assert np.array_equal(moved["tau"], np.roll(rest["tau"], shift, axis=1))
        assert moved["clipped"] == 0


def _runs_brute_force(dark):
    """Walks the periodic line pixel by pixel from behind a bright pixel."""
    N = len(dark)
    if all(dark):
        return [N]
    start = next(p for p in range(N) if not dark[p])
    out, run = [], 0
    for s in range(1, N + 1):
        if dark[(start + s) % N]:
            run += 1
        elif run:
            out.append(run)
            run = 0
    return out


def test_gap_finder_against_brute_force():
    rng = np.random.default_rng(8)
    for N in (1, 2, 7, 64, 65, 130):
        for fill in (0.1, 0.5, 0.9):
            for _ in range(20):
                dark = rng.random(N) < fill
                assert sorted(R.gaps_of_line(dark)) == sorted(_runs_brute_force(dark.tolist()))
    through_the_end = np.array([1, 1, 0, 0, 1, 0, 1, 1, 1], dtype=bool)
    assert sorted(R.gaps_of_line(through_the_end)) == [1, 5]
    assert R.gaps_of_line(np.ones(9, dtype=bool)) == [9] and R.gaps_of_line(np.zeros(9, dtype=bool)) == []
    flux = np.where(np.stack([through_the_end, np.ones(9, bool), np.zeros(9, bool)]), 0.0, 1.0)[None]
    s = R.gap_statistics(flux, 0.05)
    assert (s["n_dark"], s["n_gaps"], s["longest"], s["full_lines"]) == (15, 3, 9, 1)
    assert s["gaps"].tolist() == [0, 1, 0, 0, 0, 1, 0, 0, 0, 1]


def test_constants_are_the_librarys():
    assert (R.FLUX, R.TAU, R.MAX_BINS) == (_capi.LYA_FLUX, _capi.LYA_TAU, _capi.LYA_MAX_BINS) and LA.WHATS == {"flux": R.FLUX, "tau": R.TAU}
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "asora_hip.h")).read()
    assert "(0.5641895835477563 / bt) exp(-(t t))" in header and R.INV_SQRT_PI == 0.5641895835477563 and abs(R.INV_SQRT_PI - 1.0 / math.sqrt(math.pi)) < 2e-16
    assert "width >= 2^-10" in header and R.FLOOR == 2.0 ** -10
    # the default bins of the module are edges the reference's rule takes as they are: F = 1 falls into the last bin
    edges = LA.lyman_alpha_spec("who", 8, b_scale=1.0, tau_scale=1.0)["edges"]
    assert R.pdf_of(np.array([0.0, 1.0]), edges).tolist() == [1] + [0] * (LA.DEFAULT_BINS - 2) + [1]


def test_pdf_rule():
    edges = [0.0, 0.25, 0.25, 0.5, 1.0]
    f = np.array([-0.1, 0.0, 0.2, 0.25, 0.49, 0.5, 0.99, 1.0, np.nan])
    assert R.pdf_of(f, edges).tolist() == [2, 0, 2, 2]             # (the empty bin takes nothing; 1.0 and the NaN are dropped)


@pytest.mark.parametrize("N", [64, 128, 129, 192, 320])
def test_crafted_lines_are_what_they_say(N):
    """The lines by their runs, counted by the brute-force walk; and the vectorised gap statistics against the per-line ones on them."""
    lines = R.crafted_lines(N)
    assert all(l.shape == (N,) and l.dtype == bool for l in lines)
    runs = [sorted(_runs_brute_force(l.tolist())) for l in lines]
    assert runs[0] == [N] and runs[1] == []
    places = len({0, 63, 64, N - 1} & set(range(N)))              # (at N = 64 there is no pixel 64, and N - 1 is 63)
    assert places == (2 if N == 64 else 4) and runs.count([N - 1]) == places and runs.count([1]) == places
    assert [2] in runs or N == 64                                  # [63, 64]
    assert [64] in runs and [N - 2] in runs and [6] in runs        # [0, 63] (and [64, 127]); [1, N - 2]; N - 3 through the wrap to 2
    assert ([111] in runs) == (N >= 192)                           # 40 ... 150: 24 bits of word 0, word 1, 23 bits of word 2
    even, odd = runs[-2], runs[-1]
    assert even == ([1] * (N // 2) if N % 2 == 0 else [1] * (N // 2 - 1) + [2]) and odd == [1] * (N // 2)
    # a run that fills exactly one word (where a line has more than one), and one through the wrap
    assert N == 64 or any(l[:64].all() and not l[64] for l in lines)
    assert any(l[0] and l[N - 1] and not l.all() for l in lines)
    flux = np.where(np.stack(lines), 0.0, 1.0)
    slow, fast = R.gap_statistics(flux, 0.5), R.gap_statistics_fast(flux, 0.5)
    assert fast["gaps"].dtype == np.uint64 and fast["gaps"].tobytes() == slow["gaps"].tobytes()
    assert {k: fast[k] for k in ("n_dark", "n_gaps", "longest", "full_lines")} == {k: slow[k] for k in ("n_dark", "n_gaps", "longest", "full_lines")}
    assert slow["full_lines"] == (2 if N == 64 else 1) and slow["longest"] == N      # (at N = 64 the run [0, 63] is the line)
    assert slow["n_gaps"] == sum(len(r) for r in runs)


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 129])
def test_fast_gap_statistics_against_the_loop(N):
    rng = np.random.default_rng(900 + N)
    for fill in (0.0, 0.03, 0.5, 0.97, 1.0):
        flux = np.where(rng.random((7, 9, N)) < fill, 0.0, 1.0)
        flux[0, 0, 0] = np.nan                                      # (a NaN is bright)
        slow, fast = R.gap_statistics(flux, 0.5), R.gap_statistics_fast(flux, 0.5)
        assert fast["gaps"].tobytes() == slow["gaps"].tobytes(), (N, fill)
        for key in ("n_dark", "n_gaps", "longest", "full_lines"):
            assert fast[key] == slow[key], (N, fill, key)


@pytest.mark.parametrize("N,axis", [(64, 2), (129, 0), (192, 1)])
def test_mask_field_has_the_known_answer(N, axis):
    """What tests/test_gpu_lyman_alpha.py rests on: on the fields of mask_field the statement gives tau == g bit for bit, W = 1,
    nothing clipped or degenerate, and the designed mask back."""
    lines_at = [0, 1, N + 3, N * N - 1]
    x, n, T, dark = R.mask_field(N, axis, lines_at)
    crafted = R.crafted_lines(N)
    for q, at in enumerate(lines_at):
        assert np.array_equal(dark[at], crafted[q]) and np.array_equal(R.pick_lines(x, axis, [at])[0] == 0.0, crafted[q])
    r = R.forest(x, n, T, None, axis, 0.0, 0.37, 5.0, gap_threshold=0.5, lines=np.arange(0, N * N, 7))
    want = np.where(dark[::7], 5.0, 0.0)
    assert r["tau"].tobytes() == want.tobytes() and (r["window"], r["clipped"], r["degenerate"]) == (1, 0, 0)
    assert np.array_equal(r["flux"] < 0.5, dark[::7]) and set(np.unique(r["flux"])) == {math.exp(-5.0), 1.0}
    assert np.all(r["bound"][dark[::7]] > 0.0)


def test_a_non_finite_reach_takes_the_whole_line():
    """One cell at T = +inf: its bt and its reach are infinite, the automatic window is the cap (N - 1) // 2 and the cell counts as
    clipped; its own weight is (erf(0) - erf(0)) / 2 = 0 on every pixel, so tau stays finite everywhere."""
    N = 33
    x, n, T, v = R.fields(N, 133)
    T = T.copy()
    T[4, 5, 6] = np.inf
    b_scale = 0.5 / math.sqrt(3.0e4)
    for axis in (0, 2):
        r = R.forest(x, n, T, v, axis, 0.5, b_scale, 1.0)
        assert r["window"] == 16 == (N - 1) // 2 and r["reach_max"] == math.inf and r["clipped"] >= 1
        assert r["nonfinite"] == 0 and np.all(np.isfinite(r["tau"])) and np.all(np.isfinite(r["bound"]))
        capped = R.forest(x, n, np.where(np.isinf(T), 1.0, T), v, axis, 0.5, b_scale, 1.0, window=16)
        assert r["clipped"] == capped["clipped"] + 1


def test_fsum_of_values_is_math_fsum():
    rng = np.random.default_rng(4)
    f = math.exp(-5.0)
    for values in ([f, 1.0], [f * f, 1.0], [0.1, 0.3, 1.0e16]):
        a = rng.choice(values, size=200_001, p=[0.3, 0.7] if len(values) == 2 else [0.5, 0.3, 0.2])
        assert R.fsum_of_values(a, values) == math.fsum(a)
        assert R.fsum_of_values(a.reshape(3, -1), values) == math.fsum(a)
    with pytest.raises(AssertionError):
        R.fsum_of_values(np.array([0.5, 0.25]), [0.5])
