"""CPU: the in-process world of tests/slab_world.py, proven before any GPU rank is put into it.

A world of P OracleAsora ranks (the C oracle under the calls TorchComm._slab_one / _reduce_one make) against ONE OracleAsora
that owns every plane, same medium and sources.  OracleAsora holds NaN wherever the library would hold stale data, and the
recording asserts that everything it records is finite, so a plane the driver forgot to deliver fails here.  The two differ
only by the order in which the contributions of the sources are summed (per rank first, then over the ranks); the chemistry
amplifies that in ill-conditioned cells, which is why no GPU rank is ever compared with a one-process result.

World-versus-one distances measured (largest relative difference over all iterations: consumed rates, XH_AV):

    small_P2      N=20  P=2 R=4     3 iterations   rates 0          XH_AV 0
    small_P3      N=20  P=3 R=box   3 iterations   rates 2.9e-13    XH_AV 2.8e-13
    small_reduce  N=20  P=2 R=4     3 iterations   rates 0          XH_AV 0
    A_P2_Rbox     N=75  P=2 R=box   3 iterations   rates 1.0e-11    XH_AV 9.2e-12
    A_P3_R11      N=75  P=3 R=11    3 iterations   rates 0          XH_AV 0
    B_200         N=200 P=2 R=9     2 iterations   rates 0          XH_AV 0
    C_75          N=75  P=2 R=11    3 iterations   rates 0          XH_AV 0
    C_168         N=168 P=2 R=9     2 iterations   rates 0          XH_AV 0

(0: with two contributions per cell at most, a + b = b + a.  With a 5 Myr step of strong sources in a hotter medium, where the
pass is ill-conditioned -- see slab_world.make_case --, the same whole-box world measured 1.1e-11 and 7.4e-10.)  The bounds asserted are ten times these; where 0 was measured,
1e-13 for the rates (an order of summation that did matter moves a sum of positive terms by an ulp or a few) and 1e-12 for XH_AV."""
import numpy as np
import pytest

import slab_world as W

#: name -> (make_case arguments, exchange, iterations, bound on the rates, bound on XH_AV)
HOST_WORLDS = {
    "small_P2": (dict(N=20, P=2, ns=6, R=4.0, seed=101), "slab", 3, 1e-13, 1e-12),
    "small_P3": (dict(N=20, P=3, ns=7, R=1000.0, seed=102), "slab", 3, 2.9e-12, 2.8e-12),
    "small_reduce": (dict(N=20, P=2, ns=6, R=4.0, seed=101), "allreduce", 3, 1e-13, 1e-12),
    "A_P2_Rbox": (W.WORLDS["A_P2_Rbox"], "slab", 3, 1.0e-10, 9.2e-11),
    "A_P3_R11": (W.WORLDS["A_P3_R11"], "slab", 3, 1e-13, 1e-12),
    "B_200": (W.WORLDS["B_200"], "slab", 2, 1e-13, 1e-12),
    "C_75": (W.WORLDS["C_75"], "allreduce", 3, 1e-13, 1e-12),
    "C_168": (W.WORLDS["C_168"], "allreduce", 2, 1e-13, 1e-12),
}


@pytest.mark.parametrize("name", list(HOST_WORLDS))
def test_the_cpu_world_against_one_rank_owning_every_plane(name):
    args, exchange, iters, bound_rates, bound_xav = HOST_WORLDS[name]
    c = W.make_case(**args)
    world = W.cpu_world(c, iters, exchange)
    one = W.cpu_world(W.one_rank_of(c), iters, "slab")
    N, P, plan = c["N"], c["P"], c["plan"]
    assert len(world) == len(one) == iters                            # row counts: one history row per rank and iteration
    d_rates = d_xav = 0.0
    for it, (w, o) in enumerate(zip(world, one)):
        assert sorted(w["rows"]) == list(range(P)) and sorted(o["rows"]) == [0]
        if exchange == "slab":
            # every plane delivered: every piece of every send schedule is a message, and the owners' planes tile the grid
            K = plan.common_chunks(W.CHUNKS)
            want = sorted((r, q, a, b, k) for r in range(P) for k, pieces in enumerate(plan.send_schedule(r, K)) for q, a, b in pieces)
            assert sorted(w["msgs"]) == want and (P == 1 or want)
            sent = np.zeros((P, N), dtype=int)
            for r, q, a, b, k in want:
                assert plan.own[q][0] <= a < b <= plan.own[q][1] and q != r
                sent[r, a:b] += 1
            for r in range(P):
                foreign = plan.reach[r].copy()
                foreign[slice(*plan.own[r])] = False
                assert (sent[r][foreign] == 1).all() and (sent[r] <= 1).all()
            rates, xav, xint = (W.gather(c, w, k) for k in ("rates", "xav", "xint"))
            # sums equal: the totals are the sums of the partial sums in rank order, and every rank's row holds them
            assert w["totals"] == tuple(sum(w["sums"][r][q] for r in range(P)) for q in range(3))
            for r in range(P):
                assert tuple(w["rows"][r][:3]) == tuple(float(v) for v in w["totals"])
                assert np.array_equal(w["rows"][r], w["rows"][0])
        else:
            for r in range(1, P):                                     # every rank computed the whole grid on the same sum
                for k in ("rates", "xav", "xint", "rows"):
                    assert np.array_equal(w[k][r], w[k][0]), (k, r)
            assert np.array_equal(w["rates"][0], w["total"])
            rates, xav, xint = w["rates"][0], w["xav"][0], w["xint"][0]
        assert rates.shape == xav.shape == (N, N, N)
        ro, xo = o["rates"][0], o["xav"][0]
        assert np.array_equal(rates != 0, ro != 0) and (ro != 0).any()
        m = ro != 0
        d_rates = max(d_rates, float(np.max(np.abs(rates[m] / ro[m] - 1.0))))
        d_xav = max(d_xav, float(np.max(np.abs(xav / xo - 1.0))))
        # the sums of the world against the one rank's: conv_flag may differ by the cells the conditioning moves across the test
        tot = w["totals"] if exchange == "slab" else w["rows"][0][:3]
        assert tot[1] == pytest.approx(o["rows"][0][1], rel=1e-9) and tot[2] == pytest.approx(o["rows"][0][2], rel=1e-9)
        assert abs(tot[0] - o["rows"][0][0]) <= 1e-4 * N ** 3
    print(f"{name}: world-versus-one distance over {iters} iterations: rates {d_rates:.2e}, XH_AV {d_xav:.2e}")
    assert d_rates <= bound_rates and d_xav <= bound_xav, (d_rates, d_xav)


def test_reached_is_the_zero_pattern_of_the_oracle_trace():
    """slab_world.reached (what the GPU test holds outgoing messages against) is the oracle's own set of rated cells."""
    c = W.make_case(**W.WORLDS["A_P3_R11"])
    world = W.cpu_world(c, 1, "slab")
    assert world[0]["msgs"]
    for (r, q, a, b, k), m in world[0]["msgs"].items():
        reach = W.reached(c, r, a, b)
        assert not m[~reach].any()
    # a whole-share trace: the union over a rank's messages and own planes is exactly `reached`
    from fake_backend import OracleAsora
    lib = OracleAsora(c["thin"], c["thick"])
    W.begin_rank(lib, c, 0, own=(0, c["N"]))
    lib.evolve_slab_trace(0, c["bounds"][1] - c["bounds"][0])
    assert np.array_equal(lib._acc != 0, W.reached(c, 0, 0, c["N"]))


@pytest.mark.parametrize("name", ["A_P2_Rbox", "A_P2_Rbox_uniformT", "A_P3_R11", "C_75"])
def test_the_worlds_are_well_conditioned_for_the_bars_of_the_gpu_test(name):
    """The GPU test holds the pass of a rank to 1e-9 against the C statement of the pass on the rates it read, and what the rank
    sends (all-reduce loop: its out-box) in the second and third iteration to 1e-8 against the CPU rank's, which traced through
    the CPU rank's own XH_AV.  Those bars only mean something where the C statements themselves do not answer an ulp with more.
    Over the three iterations of a world: (1) the response of the C pass to a change of one or two ulp in the rates or in the
    temperatures, in XH_AV and XH_INTERMED; (2) the response of the oracle's trace of the rank's share, on the planes it sends,
    to its own planes of XH_AV being replaced by the most perturbed ones of (1).  Measured:

        A_P2_Rbox           pass 2.1e-11   sent rates 2.2e-11
        A_P2_Rbox_uniformT  pass 9.1e-12   sent rates 3.6e-11
        A_P3_R11            pass 2.0e-13   sent rates 4.4e-12
        C_75                pass 8.2e-14   sent rates 5.7e-12

    (N = 200 and 168, measured once outside the suite: pass 1.6e-13 and 1.7e-13, sent rates 3e-13 at N = 200.)  Asserted: 2e-10 and 2e-10, a fifth of the tighter bar and a
    fiftieth of the other -- a GPU rank legitimately differs from the C pass by more than two ulp of its inputs.
    slab_world.make_case says what the responses are with a shorter step, hotter cells or stronger sources."""
    import cases
    from oracle import oracle as O
    c = W.make_case(**W.WORLDS[name])
    reduce_loop = name.startswith("C")
    world = W.cpu_world(c, 3, "allreduce" if reduce_loop else "slab")
    N = c["N"]

    def trace(r, xav):
        p0, f0, _ = W.share(c, r)
        return O.asora_do_all_sources(c["R"], cases.SIG, c["dr"], c["ndens"], xav, p0, f0, c["thin"], c["thick"], cases.MINLOGTAU,
                                      c["dlog"], NumTau=c["numtau"], flags=O.ASORA_MODE)["phi_ion"]
    d_pass = d_sent = 0.0
    for r in range(c["P"]):
        sl = slice(0, N) if reduce_loop else slice(*c["plan"].own[r])
        n, T, xh, xin = c["ndens"][sl], c["temp"][sl], c["xh"][sl], c["xh"][sl]
        for it, w in enumerate(world):
            rates = w["rates"][r]
            base = O.global_pass(c["dt"], n, T, xh, xin, xin, rates, *W.CHEM)
            assert np.array_equal(base[0], w["xav"][r]) and np.array_equal(base[1], w["xint"][r])
            moved, most = base[0], -1.0
            for eps in (2e-16, -2e-16, 4e-16):
                for TT, rr in ((T * (1.0 + eps), rates), (T, rates * (1.0 + eps))):
                    got = O.global_pass(c["dt"], n, TT, xh, xin, xin, rr, *W.CHEM)
                    d = max(float(np.abs(got[0] / base[0] - 1.0).max()), float(np.abs(got[1] / base[1] - 1.0).max()))
                    if d > most:
                        moved, most = got[0], d
            d_pass = max(d_pass, most)
            if it < 2:
                full = w["xav"][r] if reduce_loop else W.gather(c, w, "xav")
                view = np.array(full)
                view[sl] = moved
                a, b = trace(r, full), trace(r, view)
                sent = a != 0
                if not reduce_loop:
                    sent[sl] = False
                assert sent.any()
                d_sent = max(d_sent, float(np.abs(b[sent] / a[sent] - 1.0).max()))
            xin = w["xav"][r]
    print(f"{name}: response to one or two ulp: pass {d_pass:.2e}, sent rates {d_sent:.2e}")
    assert d_pass < 2e-10 and d_sent < 2e-10, (d_pass, d_sent)
