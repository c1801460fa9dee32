"""TEST INFRASTRUCTURE: an in-process world of P ranks for the sharded device loop (asora_evolve_slab_*).

One process plays every rank in lockstep.  A rank is any object with the `libasora` method set -- tests/fake_backend.OracleAsora
(the C oracle underneath: a CPU world) or the HIP library itself -- and the calls made on it are the ones
pyc2ray_amd.dist.TorchComm._slab_one / _reduce_one make on the gloo transport, every plane through the host.  The plan and the
source shares are the product's own (SlabPlan, TorchComm.shard_sources_by_slab).

``slab_iterations`` / ``reduce_iterations`` RECORD what every live rank did: every message, the own planes of XH_AV,
XH_INTERMED and of the rates the pass consumed, the partial sums, the history row.  Given the record of a world, the same
functions REPLAY one rank of it: only that rank is live, what the others would have sent it (rate messages, XH_AV planes, the
totals of the sums) is taken from the record.  So a single GPU process can play each rank of a world computed on the CPU --
no child processes, no process group."""
import numpy as np

import cases
from pyc2ray_amd import _capi
from pyc2ray_amd.dist import SlabPlan, TorchComm

MYR = 3.15576e13
CHEM = (cases.BH00, cases.ALBPOW, cases.COLH0, cases.TEMPH0, cases.ABU_C)
#: trace chunks per iteration, as TorchComm.slab_chunks of a two-rank job (common_chunks makes it 1 for unsorted shares)
CHUNKS = 2

#: the worlds of tests/test_gpu_slab_world.py (and, at reduced cost, of tests/test_slab_world_host.py): name -> make_case arguments.
#:  A: N = 75 = 32 + 32 + 11 cells per row, 9 lines of 8 and one of 3
WORLDS = {
    "A_P2_Rbox": dict(N=75, P=2, ns=5, R=1000.0, seed=104),
    "A_P2_Rbox_uniformT": dict(N=75, P=2, ns=5, R=1000.0, seed=104, uniform_T=True),
    # first coordinates: rank 0 reaches rank 1's planes upwards and rank 2's through plane 0, rank 1 both neighbours, rank 2
    # rank 1 downwards and rank 0 through plane 0
    "A_P3_R11": dict(N=75, P=3, ns=9, R=11.0, seed=103, first=[3, 21, 29, 31, 46, 53, 61, 71, 74]),
    # second coordinates beyond the first trip of the pass's j loop (jc = 147 on 256 CUs) for half the sources
    "B_200": dict(N=200, P=2, ns=6, R=9.0, seed=105, first=[30, 60, 95, 104, 150, 196], second=[20, 160, 185, 60, 170, 195]),
    "C_75": dict(N=75, P=2, ns=6, R=11.0, seed=106),
    "C_75_uniformT": dict(N=75, P=2, ns=6, R=11.0, seed=106, uniform_T=True),
    "C_168": dict(N=168, P=2, ns=6, R=9.0, seed=107, second=[15, 130, 150, 50, 140, 160]),
}


def make_case(N, P, ns, R, seed, uniform_T=False, first=None, second=None, tables=None, lattice=False, temp_decades=(1.5, 2.5), dt_myr=3000.0,
              flux_scale=0.005):
    """A world: log-normal density, a nearly neutral box, ns sources of unequal flux sharded over P ranks by their first
    coordinate.  first / second: 1-based first / second coordinates of the sources (else random); lattice: non-overlapping sources on the lattice
    of spacing N // 2 (needs 2 floor(R) < N // 2).
    uniform_T: True (100 K everywhere) or the temperature in K.
    The defaults of the temperatures (30 - 300 K), the time step (3000 Myr) and flux_scale (0.005 of the flux of the suite's other
    two-rank cases) are chosen for the CONDITIONING of what the GPU test compares, so that its bars (1e-9 on the pass, 1e-8 on what
    a rank sends in the second and third iteration) mean something.  doric forms x_av = x_eq + (x_0 - x_eq) (1 - exp(-d)) / d: where
    d = delth dt is small and x_eq >> x_av -- weakly irradiated cells of a short step, hot cells whose collisional ionisation lifts
    x_eq -- the C oracle itself answers a change of ONE or two ulp in its rates or temperatures with up to 3e-9 in x_av (N = 75, R
    beyond the box, 5 Myr, flux_scale 1, 1e3 - 1e4 K), 3e-10 (N = 168, R = 9, the same) or 5e-7 (1e3.5 - 1e4.5 K); GPU ranks missed
    the 1e-9 bar in one or two cells of such worlds by that much and ten times that much.  A longer step at the same flux cures the
    pass (5e-11 at 100 Myr) and ionises half the box, and there nHI = n (1 - x_av) cancels: the same two ulp then move what a rank
    sends in the next iteration by 5e-9, and a GPU rank, whose x_av legitimately differs from the CPU rank's, was 4e-8 from it in
    one cell.  A long step (large d everywhere) of weak sources (the box stays neutral) in a cold medium (stronger recombination,
    larger d still) is well-conditioned in both respects: 4e-11 at most at N = 75, 2e-13 at N = 168 and 200.
    tests/test_slab_world_host.py asserts both responses on the N = 75 worlds."""
    rng = np.random.default_rng(seed)
    nd, xh, dr = cases.grid(N, "lognormal", seed, 0.3, xlo=1e-4, xhi=2e-3)
    temp = np.full((N, N, N), 100.0 if uniform_T is True else float(uniform_T)) if uniform_T else 10 ** rng.uniform(*temp_decades, size=(N, N, N))
    if lattice:
        pos = lattice_sources(N, ns, rng)
    else:
        pos = 1 + rng.integers(0, N, size=(3, ns))
        if first is not None:
            pos[0] = np.asarray(first)
        if second is not None:
            pos[1] = np.asarray(second)
    flux = flux_scale * 3e-4 * (N / 16.0) ** 3 / ns * (1.0 + 0.1 * np.arange(ns))
    thin, thick, dlog = tables if tables is not None else cases.soft_tables(600)
    spos, sflux, bounds = TorchComm.shard_sources_by_slab(pos, flux, P)
    plan = SlabPlan(N, P, R, [spos[0, bounds[r]:bounds[r + 1]] - 1 for r in range(P)])
    return dict(N=N, P=P, ns=ns, R=float(R), ndens=nd, xh=xh, temp=temp, dr=dr, dt=dt_myr * MYR, thin=thin, thick=thick, dlog=dlog,
                numtau=thin.shape[0] - 1, pos=spos, flux=sflux, bounds=bounds, plan=plan)


def lattice_sources(N, ns, rng):
    """tests/_thermal_dist_worker.py's _lattice for any N: ns <= 8 sources on the lattice of spacing N // 2, one on the box corner
    (its sphere wraps through plane 0), those at first coordinate 1 + N // 2 straddle plane N // 2."""
    h = N // 2
    pts = np.array([(1 + a * h, 1 + b * h, 1 + c * h) for a in (0, 1) for b in (0, 1) for c in (0, 1)]).T
    pick = np.concatenate([[0], 1 + rng.permutation(7)[:ns - 1]])
    return pts[:, pick]


def share(c, r):
    """(flat 0-based positions, fluxes, count) of rank r's sources, in upload order."""
    lo, hi = c["bounds"][r], c["bounds"][r + 1]
    p0, f0 = cases.flat_sources(c["pos"][:, lo:hi], c["flux"][lo:hi])
    return p0, f0, hi - lo


def reached(c, r, a, b):
    """Cells of the planes [a, b) that a source of rank r rates: inside the periodic window and within R (raytracing.cu:122-123,315)."""
    N, plan = c["N"], c["plan"]
    lo, hi = plan._lo, plan._hi
    p0, _, n = share(c, r)
    out = np.zeros((b - a, N, N), dtype=bool)
    ax = np.arange(N)
    for s in range(n):
        d = [(ax - p0[3 * s + q] + lo) % N - lo for q in range(3)]          # offsets in [-lo, N - 1 - lo]
        ok = [dq <= hi for dq in d]
        d2 = d[0][a:b, None, None] ** 2 + d[1][None, :, None] ** 2 + d[2][None, None, :] ** 2
        out |= (d2 <= c["R"] ** 2) & ok[0][a:b, None, None] & ok[1][None, :, None] & ok[2][None, None, :]
    return out


def begin_rank(lib, c, r, own=None, thermal=False):
    """Upload rank r's share and the medium and begin a step that never converges on its own planes (own: another range)."""
    p0, f0, n = share(c, r)
    lib.source_data_to_device(p0, f0, n)
    for which, a in ((_capi.GRID_NDENS, c["ndens"]), (_capi.GRID_TEMP, c["temp"]), (_capi.GRID_XH, c["xh"])):
        lib.grid_to_device(which, a)
    a, b = c["plan"].own[r] if own is None else own
    begin = lib.evolve_begin_slab_thermal if thermal else lib.evolve_begin_slab
    begin(c["dt"], *CHEM, c["R"], cases.SIG, c["dr"], cases.MINLOGTAU, c["dlog"], c["numtau"], 0, n, -1.0, 0.0, a, b - a)
    return n


def _finite(x):
    x = np.asarray(x)
    assert np.isfinite(x).all(), "a recorded value is not finite: a plane the plan forgot"
    return x


def slab_iterations(live, c, iters, record=None, thermal=False):
    """`iters` iterations of the slab exchange on the ranks `live` = {rank: lib}, each begun with ``begin_rank``.  Every rank of
    the world must be live, or come from `record` (the return value of an earlier call with every rank live).  Returns one
    dict per iteration: msgs[(r, q, a, b, chunk)] (thermal: hmsgs too), xav / xint / rates (thermal: heat, temp_end) [rank] on the
    own planes, sums[rank] = chemistry_finish(), totals, rows[rank] = the history row (thermal: stats[rank] = thermal_stats())."""
    plan, N, P = c["plan"], c["N"], c["P"]
    K = plan.common_chunks(CHUNKS)
    assert record is not None or sorted(live) == list(range(P))
    out = []
    for it in range(iters):
        rec = record[it] if record is not None else None
        cur = dict(msgs={}, hmsgs={}, xav={}, xint={}, rates={}, heat={}, temp_end={}, stats={}, sums={}, rows={})
        for r, lib in live.items():
            n = c["bounds"][r + 1] - c["bounds"][r]
            bounds, sched = plan.chunk_bounds(n, K), plan.send_schedule(r, K)
            for k in range(K):
                lib.evolve_slab_trace(bounds[k], bounds[k + 1] - bounds[k])
                for q, a, b in sched[k]:
                    lib.evolve_slab_fold_out(a, b - a)
                    cur["msgs"][(r, q, a, b, k)] = _finite(lib.evolve_slab_outbox_to_host(a, b - a, N))
                    if thermal:
                        cur["hmsgs"][(r, q, a, b, k)] = _finite(lib.evolve_slab_heat_outbox_to_host(a, b - a, N))
        for q, lib in live.items():                       # chunk order, then rank order; per run the rates, then the heating
            rsched = plan.recv_schedule(q, K)
            for k in range(K):
                for r, a, b in rsched[k]:
                    key = (r, q, a, b, k)
                    src = cur if r in live else rec
                    lib.evolve_slab_add_host(a, src["msgs"][key])
                    if thermal:
                        lib.evolve_slab_add_heat_host(a, src["hmsgs"][key])
        for r, lib in live.items():
            lib.evolve_slab_pass()
            cur["sums"][r] = tuple(_finite(lib.chemistry_finish()))
            a, b = plan.own[r]
            cur["xav"][r] = _finite(lib.planes_to_host(_capi.GRID_XH_AV, a, b - a, N))
            cur["xint"][r] = _finite(lib.planes_to_host(_capi.GRID_XH_INTERMED, a, b - a, N))
        for r, lib in live.items():
            for q, a, b in plan.back_runs(r)[1]:
                a0 = plan.own[q][0]
                lib.planes_to_device(_capi.GRID_XH_AV, a, (cur if q in live else rec)["xav"][q][a - a0:b - a0])
                lib.evolve_slab_nhi(a, b - a)
        if rec is not None:
            cur["totals"] = rec["totals"]
        else:
            cur["totals"] = tuple(sum(cur["sums"][r][q] for r in range(P)) for q in range(3))       # rank order
        for r, lib in live.items():
            lib.evolve_slab_close(cur["totals"])
            niter, done, rows = lib.evolve_poll(1)
            assert niter == it + 1 and not done and len(rows) == 1, (niter, done, len(rows))
            cur["rows"][r] = np.array(rows[0])
            a, b = plan.own[r]
            cur["rates"][r] = _finite(lib.planes_to_host(_capi.GRID_PHI_ION, a, b - a, N))
            if thermal:
                cur["heat"][r] = _finite(lib.planes_to_host(_capi.GRID_PHI_HEAT, a, b - a, N))
                cur["temp_end"][r] = _finite(lib.planes_to_host(_capi.GRID_TEMP_END, a, b - a, N))
                cur["stats"][r] = tuple(lib.thermal_stats())
        out.append(cur)
    return out


def reduce_iterations(live, c, iters, record=None):
    """The same for the all-reduce loop (every live rank begun with own = (0, N)): trace, fold_all, the out-boxes summed over the
    ranks on the host in rank order, the pass on the sum.  Per iteration: box[rank] (its out-box), total (the sum it was given),
    rates / xav / xint [rank] (whole grids), rows[rank]."""
    N, P = c["N"], c["P"]
    assert record is not None or sorted(live) == list(range(P))
    out = []
    for it in range(iters):
        rec = record[it] if record is not None else None
        cur = dict(box={}, rates={}, xav={}, xint={}, rows={}, sums={})
        for r, lib in live.items():
            lib.evolve_slab_trace(0, c["bounds"][r + 1] - c["bounds"][r])
            lib.evolve_slab_fold_all()
            cur["box"][r] = _finite(lib.evolve_slab_outbox_to_host(0, N, N))
        total = np.zeros((N, N, N))
        for r in range(P):
            total += (cur if r in live else rec)["box"][r]
        cur["total"] = total
        for r, lib in live.items():
            lib.evolve_slab_outbox_from_host(0, total)
            lib.evolve_slab_pass()
            cur["sums"][r] = tuple(_finite(lib.chemistry_finish()))
            lib.evolve_slab_close(None)
            niter, done, rows = lib.evolve_poll(1)
            assert niter == it + 1 and not done and len(rows) == 1, (niter, done, len(rows))
            cur["rows"][r] = np.array(rows[0])
            for name, which in (("rates", _capi.GRID_PHI_ION), ("xav", _capi.GRID_XH_AV), ("xint", _capi.GRID_XH_INTERMED)):
                cur[name][r] = _finite(lib.planes_to_host(which, 0, N, N))
        out.append(cur)
    return out


def cpu_world(c, iters=3, exchange="slab"):
    """The world of case `c` on OracleAsora ranks; exchange = "slab" or "allreduce"."""
    from fake_backend import OracleAsora
    live = {r: OracleAsora(c["thin"], c["thick"]) for r in range(c["P"])}
    for r, lib in live.items():
        begin_rank(lib, c, r, own=(0, c["N"]) if exchange == "allreduce" else None)
    return (slab_iterations if exchange == "slab" else reduce_iterations)(live, c, iters)


def one_rank_of(c):
    """The same medium and sources as a world of ONE rank (it owns every plane, nothing travels)."""
    N, R = c["N"], c["R"]
    one = dict(c, P=1, bounds=[0, c["ns"]])
    one["plan"] = SlabPlan(N, 1, R, [c["pos"][0] - 1])
    return one


def gather(c, rec, name):
    """The owners' planes of rec[name] put together into one N^3 grid."""
    return np.concatenate([rec[name][r] for r in range(c["P"])], axis=0)
