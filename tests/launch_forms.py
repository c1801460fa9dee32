"""TEST INFRASTRUCTURE: the production launch forms of `raytrace_octant_kernel` against the CPU oracle ("the
zero-flux-filler check").

The forms a real run takes -- the whole sphere x 128 / 256 / 512 threads, half spheres, six sectors, twelve sector pairs, two
sources per workgroup, line-aligned tables -- are chosen by `pick_launch_shape`, `pair_sources_pays` and the aligned-rows rule of
`plan_shape` (csrc/raytrace_plan.hpp) from the radius and from the NUMBER of uploaded sources, about 1000 of them, which the oracle
cannot trace in seconds.  So a case uploads NS sources of which K are bright and NS - K have flux exactly 0.0: the library culls
nothing on upload, the launch shape is that of NS sources, every rate of a filler is flux / (vol nHI) x (...) = +0 wherever
nHI > 0, and the reference is the oracle over the K bright sources alone.

A fault in a filler's workgroup is invisible (its output is multiplied by 0), so the bright set sits where the forms differ;
`check_properties` states where, and the constructor searches seeded draws until they hold:

  1. two bright sources (the PAIR) are consecutive in the library's position-sorted order and share a workgroup in the paired forms:
     positions (2m, 2m + 1) of the sorted list, or -- line-aligned tables -- equal modulo 8 along i and k and partners in both class
     lists of `source_pairs_by_class`;
  2. a bright source has a filler directly before it (and is the SECOND source of that filler's workgroup);
  3. a bright source has a filler directly after it (and is the FIRST source of that workgroup);
  4. the first and the last source in sorted order are bright, at (0,0,0) and (N-1,N-1,N-1): the periodic wrap, and with an odd NS
     the dummy partner of the last workgroup;
  5. the spheres of the PAIR overlap by more than half: their atomics hit the same addresses;
  6. where the tables are line-aligned, the bright sources cover every residue 0 ... 7 along i and along k.

The medium is the lognormal one of tests/cases.py with x in [1e-4, 1e-2] (nHI > 0 everywhere: a filler's flux x inf would be NaN).
The cell size is a power of two, so the lattice points that sit exactly on a sphere of integer radius are inside for the
reference's floating-point test (tests/open_boundary_reference.py, rated_pairs) and the rated pairs are NS x the lattice points
within R.

A second, "dense" medium serves ASORA_OPT_SKIP_ZERO_RATES.  What that option leaves out are the rates of cells whose optical depth
lies beyond the last table entry (the kernel's test is on the optical depth, not on the flux: a filler's +0 is added like any other
rate), and the lognormal medium has none.  The dense medium has, a hundred million times denser, one cell in 3000 and a plate of
5 x 5 cells in front of the corner source; behind the plate the rates are exactly +0.  Its penumbra holds cells with optical depths
of 1e2 ... 1e4 across which the optical depth grows by 1e-2 or less: there Gamma = pref (T(tau_in) - T(tau_out)) cancels 1e5 ...
1e7-fold, which is outside what the 1e-8 of tests/test_gpu_parity.py is derived for (measured on the MI355X: 1 ... 3 cells in a
million at 1.1e-8 ... 6.4e-8).  So the values of the dense medium are compared where the rate is at least WELL_LIT = 1e-4 of the
same cell's rate in the lognormal medium (the tables fall as tau^-3: an optical depth at most 22 times the lognormal medium's,
below ~100), the pattern of exact zeros everywhere; every other comparison with the oracle runs on the lognormal medium.
"""
import collections
import functools

import numpy as np

import cases
import open_boundary_reference as OB
from oracle import oracle as O

#: one row of the table.  units, threads, paired, aligned: what the library takes for a plain table-rate trace of the whole list on
#: 256 compute units, derived from pick_launch_shape / pair_sources_pays / the aligned-rows rule.  extra: also the two-table-set and
#: the open-boundary mode.
Case = collections.namedtuple("Case", "N NS R units threads paired aligned extra seed")

CU_COUNT = 256                      # the part the table is derived for (MI355X)

# r = min(R, 0.87 N); "merged" kinds need NS x units >= 2 x 256; pairs need 15.5 <= r < 52.5 and
# (NS // 2) x units x (threads / 64) >= 8 x 256; aligned needs 6 or 12 units, N % 8 == 0, r < 52.5 (first radius of a fresh device)
CASES = {
    "n64_1001_R8":     Case(64, 1001, 8.0, 1, 128, False, False, False, 11),       # r < 11.5: whole sphere x 128
    "n64_1001_R13":    Case(64, 1001, 13.0, 1, 256, False, False, False, 12),      # r < 15.5: x 256; no pairs below 15.5
    "n96_1001_R18":    Case(96, 1001, 18.0, 1, 512, True, False, True, 13),        # r < 21.5: x 512, 500 x 1 x 8 waves >= 2048
    "n96_1000_R22.5":  Case(96, 1000, 22.5, 2, 256, True, False, False, 14),       # half spheres
    "n96_1001_R24.5":  Case(96, 1001, 24.5, 2, 512, True, False, False, 15),
    "n128_1001_R30":   Case(128, 1001, 30.0, 6, 256, True, True, True, 16),        # six sectors; lattice points on the sphere
    "n128_1000_R41":   Case(128, 1000, 41.0, 12, 256, True, True, True, 17),       # twelve mirrored sector pairs
    "n128_1001_R56":   Case(128, 1001, 56.0, 12, 512, False, False, False, 18),    # r >= 52.5: round-2 table, 1.2 r^2 > 3500
    # fewer workgroups than 2 x 256 for the merged kinds: the round-2 table.  Twelve units on a mesh of whole lines are line-aligned
    # also with one source per workgroup
    "n64_100_R20":     Case(64, 100, 20.0, 12, 64, False, True, False, 19),        # 1.2 r^2 = 480 > 450, r <= 22.5; 50 x 12 x 1 < 2048
    "n64_64_R25":      Case(64, 64, 25.0, 4, 256, False, False, False, 20),        # r <= 28.5: octant pairs
    "n128_64_R32":     Case(128, 64, 32.0, 12, 256, False, True, False, 21),       # 12 x 128, widened: 64 x 12 <= 4 x 256
    "n64_20_R20":      Case(64, 20, 20.0, 24, 64, False, False, False, 22),        # 20 x 12 < 256: 24 sectors
    "n64_3_R20":       Case(64, 3, 20.0, 96, 256, False, False, False, 23),        # 3 x 48 <= 256: quarter sectors; all three bright
    # radius beyond the box: the periodic window cuts the trace, r = 0.87 N
    "n64_1000_Rbox":   Case(64, 1000, 1000.0, 12, 512, False, False, False, 24),   # r = 55.7
    "n48_1000_Rbox":   Case(48, 1000, 1000.0, 12, 256, True, True, True, 25),      # r = 41.8
    "n33_1001_Rbox":   Case(33, 1001, 1000.0, 6, 256, True, False, False, 26),     # r = 28.7; an odd mesh has no whole lines
}


def expected_shape(N, NS, R, cu_count=CU_COUNT):
    """(units, threads, paired, aligned) of a plain table-rate trace of NS sources: a Python restatement of pick_launch_shape,
    pair_sources_pays and the aligned-rows rule for N <= 512, no forced option, a first radius.  The table above is written out by
    hand; tests/test_launch_forms_host.py holds the two against each other."""
    r = min(R, 0.87 * N)
    est = 1.2 * r * r
    if r <= 12.5: units, threads = 4, 64
    elif r <= 14.5: units, threads = 4, 128
    elif est <= 450.0: units, threads = 8, 64
    elif r <= 22.5: units, threads = 12, 64
    elif r <= 28.5: units, threads = 4, 256
    elif est <= 1500.0: units, threads = 12, 128
    elif est <= 3500.0: units, threads = 12, 256
    else: units, threads = 12, 512
    merged = ((11.5, 1, 128), (15.5, 1, 256), (21.5, 1, 512), (23.5, 2, 256), (25.5, 2, 512), (36.5, 6, 256), (52.5, 12, 256))
    for below, mu, mt in merged:
        if r < below:
            if NS * mu >= 2 * cu_count:
                units, threads = mu, mt
            break
    if NS * 12 <= cu_count * 4 and units == 12 and threads == 128:
        threads = 256
    if NS * 12 < cu_count:
        units = 24
        if est > 900.0: threads = max(threads, 512)
        if est > 2500.0: threads = 1024
    if NS * 48 <= cu_count:
        units = 96
        threads = 1024 if est > 6000.0 else 512 if est > 2500.0 else 256
    paired = 15.5 <= r < 52.5 and NS >= 2 and (NS // 2) * units * (threads // 64) >= 8 * cu_count
    aligned = units in (6, 12) and N % 8 == 0 and r < 52.5
    return units, threads, paired, aligned


def expected_variant(case, mode):
    """What `last_raytrace_variant()` must report (without "skip_zero", which follows the option) in mode "tables", "heat",
    "spectra" or "open"."""
    threads, paired = case.threads, case.paired
    if mode == "heat":
        paired = False                                       # no paired form with heating
    if mode == "open":
        threads = 256 if threads <= 256 else 512             # the workgroup sizes the open forms are built for
        r = min(case.R, 0.87 * case.N)
        paired = 15.5 <= r < 52.5 and (case.NS // 2) * case.units * (threads // 64) >= 8 * CU_COUNT
    return {"paired": paired, "aligned": case.aligned, "buffer_atomics": True, "split_descriptors": False, "global_shells": False,
            "open": mode == "open", "units": case.units, "threads": threads}


# ---- geometry on the host ----------------------------------------------------------------------------------------------------
def cells_within(N, R):
    """Cells one source rates (as _cells_within of tests/test_gpu_parity.py): offsets within R inside the periodic window."""
    m = int(np.floor(R)) if np.isfinite(R) else N
    d = np.arange(-min(m, N // 2), min(m, N // 2 - 1 + N % 2) + 1)
    return int(((d[:, None, None] ** 2 + d[None, :, None] ** 2 + d[None, None, :] ** 2) <= R * R).sum())


def reach(N, R, pos, periodic=True):
    """(N, N, N) bool: the cells the source at 0-based `pos` rates -- within R and inside the window -floor(N/2) ... floor(N/2) - 1
    + N % 2 of every axis; periodic=False: those of them that are reached without leaving the box."""
    off, ok = [], []
    x = np.arange(N)
    for ax in range(3):
        o = (x - int(pos[ax]) + N // 2) % N - N // 2
        off.append(o)
        ok.append(np.ones(N, dtype=bool) if periodic else o == x - int(pos[ax]))
    d2 = off[0][:, None, None] ** 2 + off[1][None, :, None] ** 2 + off[2][None, None, :] ** 2
    return (d2 <= R * R) & ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :]


def coverage(N, R, bright_pos, periodic=True):
    """(N, N, N) int: how many bright spheres hold each cell."""
    n = np.zeros((N, N, N), dtype=np.int32)
    for s in np.asarray(bright_pos).reshape(-1, 3):
        n += reach(N, R, s, periodic)
    return n


def sort_order(pos):
    """The library's order of a source list (grids_api.hip, sort_sources_by_position): lexicographic in (i, j, k), stable."""
    p = np.asarray(pos).reshape(-1, 3)
    return np.lexsort((p[:, 2], p[:, 1], p[:, 0]))          # (the last key is the primary one; lexsort is stable)


def workgroups(sorted_pos, aligned):
    """Who shares a workgroup in a paired launch of the whole sorted list: a list of lists of (first, second), second = -1 for a
    source that sweeps alone.  Packed tables: one list, (2m, 2m + 1).  Line-aligned tables: one list per face kind (raytrace.hip,
    source_pairs_by_class): by the class k & 7 for the x- and y-sectors, i & 7 for the z-sectors; a source waits for the next one
    of its class."""
    p = np.asarray(sorted_pos).reshape(-1, 3)
    n = p.shape[0]
    if not aligned:
        return [[(s, s + 1 if s + 1 < n else -1) for s in range(0, n, 2)]]
    lists = []
    for axis in (2, 0):
        pairs, waiting = [], {}
        for s in range(n):
            c = int(p[s, axis]) & 7
            if c in waiting:
                pairs.append((waiting.pop(c), s))
            else:
                waiting[c] = s
        pairs += [(waiting[c], -1) for c in sorted(waiting)]
        lists.append(pairs)
    return lists


Sources = collections.namedtuple("Sources", "pos0 flux bright pair spec")
Sources.__doc__ = """pos0: flat int32 0-based xyz-interleaved upload list; flux: float64, exactly 0.0 for the fillers; bright: upload
indices of the bright sources, in upload order; pair: upload indices of the PAIR (property 1); spec: table set 0 / 1 per source for
the two-set mode -- the PAIR on different sets, fillers alternating."""


def check_properties(case, pos0, flux, pair, sorted_pos=None, sorted_flux=None):
    """The six properties of the module's docstring on an upload list; `sorted_pos`, `sorted_flux`: the library's own sorted copy
    (lib.sort_sources) in place of the numpy restatement.  Returns the list of violated properties (empty: all hold)."""
    N, K = case.N, int(np.count_nonzero(flux))
    p = np.asarray(pos0).reshape(-1, 3)
    order = sort_order(p)
    if sorted_pos is None:
        sp, sf = p[order], np.asarray(flux)[order]
    else:
        sp, sf = np.asarray(sorted_pos).reshape(-1, 3), np.asarray(sorted_flux)
    n = sp.shape[0]
    b = sf != 0
    where = {int(u): s for s, u in enumerate(order)}        # upload index -> sorted position
    sa, sb = where[pair[0]], where[pair[1]]
    groups = workgroups(sp, case.aligned)
    fillers = n > K
    bad = []
    # 1
    if not (sb == sa + 1 and b[sa] and b[sb] and np.array_equal(sp[sa], p[pair[0]]) and np.array_equal(sp[sb], p[pair[1]])):
        bad.append("1: the pair is not consecutive in sorted order")
    elif case.aligned and not (sp[sa, 0] % 8 == sp[sb, 0] % 8 and sp[sa, 2] % 8 == sp[sb, 2] % 8):
        bad.append("1: the pair does not agree modulo 8 along i and k")
    elif not all((sa, sb) in g for g in groups):
        bad.append("1: the pair does not share a workgroup")
    if fillers:
        # 2, 3: neighbours in the sorted list, and partners in every list of workgroups
        if not any(b[s] and not b[s - 1] for s in range(1, n)):
            bad.append("2: no bright source directly behind a filler")
        if not any(b[s] and not b[s + 1] for s in range(n - 1)):
            bad.append("3: no bright source directly before a filler")
        for g in groups:
            if not any(t >= 0 and b[t] and not b[s] for s, t in g):
                bad.append("2: no bright source second in a filler's workgroup")
            if not any(t >= 0 and b[s] and not b[t] for s, t in g):
                bad.append("3: no bright source first in a workgroup with a filler")
    # 4
    if not (b[0] and b[-1] and not sp[0].any() and np.all(sp[-1] == N - 1)):
        bad.append("4: first / last source in sorted order not bright on the box corners")
    if n % 2 and not case.aligned and groups[0][-1] != (n - 1, -1):
        bad.append("4: the last source of an odd list has a partner")
    # 5
    ra, rb = reach(N, case.R, p[pair[0]]), reach(N, case.R, p[pair[1]])
    if not (ra & rb).sum() > 0.5 * ra.sum():
        bad.append("5: the pair's spheres overlap by less than half")
    # 6
    if case.aligned:
        for axis in (0, 2):
            if set((sp[b, axis] % 8).tolist()) != set(range(8)):
                bad.append(f"6: residues along axis {axis} not all covered")
    return bad


@functools.lru_cache(maxsize=None)
def build_sources(name):
    """The upload list of a case: seeded draws until `check_properties` holds.  K = 8 bright sources, 12 where the tables are
    line-aligned (six of them on the residues the corners and the pair leave open), all three in the three-source case."""
    case = CASES[name]
    N, NS = case.N, case.NS
    K = min(NS, 12 if case.aligned else 8)
    step = 8 if case.aligned else 2                          # the pair: (i, j, k) and (i, j, k + step)
    rng = np.random.default_rng(case.seed)
    for _ in range(4000):
        first, last = np.zeros(3, dtype=np.int64), np.full(3, N - 1)
        if K == 3:
            mid = [np.array([1, 2, 3])]                      # the pair: the corner source and its neighbour, spheres through the wrap
        else:
            a = rng.integers(0, N, 3)
            a[2] = rng.integers(0, N - step)
            mid = [a, a + np.array([0, 0, step])]
            for q in range(K - 4):
                s = rng.integers(0, N, 3)
                if case.aligned and q < 6:                  # residues 1 ... 6 along i and, permuted, along k
                    s[0] = 8 * rng.integers(0, N // 8) + 1 + q
                    s[2] = 8 * rng.integers(0, N // 8) + 1 + (q + 3) % 6
                mid.append(s)
        fill = rng.integers(0, N, (NS - K, 3))
        # upload order: the corners first and last (a filler on a corner then sorts behind / before them), the others anywhere
        slots = np.sort(rng.choice(np.arange(1, NS - 1), K - 2, replace=False))
        pos = np.empty((NS, 3), dtype=np.int64)
        flux = np.zeros(NS)
        rest = np.setdiff1d(np.arange(NS), np.concatenate(([0, NS - 1], slots)))
        pos[rest] = fill
        pos[0], pos[NS - 1] = first, last
        pos[slots] = np.array(mid)
        bright = np.concatenate(([0], slots, [NS - 1]))
        flux[bright] = 3.0 * (1.0 + 0.25 * np.arange(K))
        pair = (0, int(slots[0])) if K == 3 else (int(slots[0]), int(slots[1]))
        pos0 = pos.astype(np.int32).ravel()
        if check_properties(case, pos0, flux, pair):
            continue
        spec = np.zeros(NS, dtype=np.int32)
        spec[rest] = np.arange(rest.size) % 2
        spec[bright] = np.arange(K) % 2
        spec[pair[0]], spec[pair[1]] = 0, 1
        for a in (pos0, flux, bright, spec):
            a.setflags(write=False)
        return Sources(pos0, flux, bright, pair, spec)
    raise RuntimeError(f"launch_forms: no draw of case {name} has the six properties")


# ---- medium, tables, references ----------------------------------------------------------------------------------------------
DENSE_ONE_IN = 3000
DENSE_FACTOR = 1e8
#: a plate of dense cells in front of the corner source at (0,0,0): plane i = 3, j and k = -2 ... 2 through the periodic wrap.  (A
#: single dense cell casts next to no shadow: the interpolation of the column density favours the clear neighbours.)
PLATE_PLANE, PLATE_HALF_WIDTH = 3, 2
#: where the values of the dense medium are compared: rate >= WELL_LIT x the lognormal medium's (the module's docstring)
WELL_LIT = 1e-4


@functools.lru_cache(maxsize=4)
def medium(name, dense=False):
    """(ndens, xh, dr) of a case, read-only; dense: with the dense cells."""
    case = CASES[name]
    N = case.N
    nd, xh, _ = cases.grid(N, "lognormal", 100 + case.seed, 0.05, xlo=1e-4, xhi=1e-2)
    dr = 2.0 ** 63 if N < 128 else 2.0 ** 62                # a mean cell of tau = 0.058 / 0.029
    if dense:
        rng = np.random.default_rng(200 + case.seed)
        where = np.zeros((N, N, N), dtype=bool)
        where.ravel()[rng.integers(0, N ** 3, N ** 3 // DENSE_ONE_IN)] = True
        plate = np.arange(-PLATE_HALF_WIDTH, PLATE_HALF_WIDTH + 1) % N
        where[np.ix_([PLATE_PLANE], plate, plate)] = True
        nd[where] *= DENSE_FACTOR
    nd.setflags(write=False)
    xh.setflags(write=False)
    return nd, xh, dr


@functools.lru_cache(maxsize=None)
def tables():
    """Two table sets, read-only: [(thin, thick, heat_thin, heat_thick)] x 2 and dlogtau.  Set 0: the soft tables with the heating
    tables of tests/cases.py (not proportional to the photo tables); set 1: grey tables, halved."""
    thin, thick, dlog = cases.soft_tables()
    n = thin.shape[0]
    g, _, _ = cases.grey_tables()
    sets = [(thin, thick, 1e-11 * thin * np.linspace(1.0, 2.0, n), 0.7e-11 * thick * np.linspace(2.0, 1.0, n)),
            (0.5 * g, 0.5 * g, 2e-11 * g * np.linspace(1.5, 1.0, n), 2e-11 * g * np.linspace(1.5, 1.0, n))]
    for s in sets:
        for a in s:
            a.setflags(write=False)
    return sets, dlog


def _oracle(case, nd, xh, dr, pos0, flux, tset, heat, R=None):
    sets, dlog = tables()
    thin, thick, hthin, hthick = sets[tset]
    kw = dict(heat_thin=hthin, heat_thick=hthick) if heat else {}
    return O.asora_do_all_sources(case.R if R is None else R, cases.SIG, dr, nd, xh, pos0, flux, thin, thick, cases.MINLOGTAU, dlog,
                                  NumTau=thin.shape[0] - 1, flags=O.ASORA_MODE, **kw)


def _bright(src, which=None):
    idx = src.bright if which is None else src.bright[which]
    return np.ascontiguousarray(src.pos0.reshape(-1, 3)[idx]).ravel(), np.ascontiguousarray(src.flux[idx])


@functools.lru_cache(maxsize=3)
def reference(name, mode):
    """The oracle's trace of the bright sources alone, computed once, read-only.
    "tables": {"phi_ion", "phi_heat"} of one trace with set 0 and its heating tables (the modes with and without heating share it);
    "dense": {"phi_ion"} of the same trace in the dense medium;
    "spectra": {"phi_ion"}, the sum of two traces, each table set on its sources (as tests/step_reference.py composes a step);
    "open": {"phi_ion"} with open boundaries (tests/open_boundary_reference.py)."""
    case, src = CASES[name], build_sources(name)
    nd, xh, dr = medium(name, mode == "dense")
    if mode == "tables":
        r = _oracle(case, nd, xh, dr, *_bright(src), 0, True)
        out = {"phi_ion": r["phi_ion"], "phi_heat": r["phi_heat"]}
    elif mode == "dense":
        out = {"phi_ion": _oracle(case, nd, xh, dr, *_bright(src), 0, False)["phi_ion"]}
    elif mode == "spectra":
        phi = np.zeros((case.N,) * 3)
        for s in (0, 1):
            phi += _oracle(case, nd, xh, dr, *_bright(src, src.spec[src.bright] == s), s, False)["phi_ion"]
        out = {"phi_ion": phi}
    elif mode == "open":
        out = {"phi_ion": _open_reference(case, src, nd, xh, dr)}
    else:
        raise ValueError(mode)
    for a in out.values():
        a.setflags(write=False)
    return out


def _open_reference(case, src, nd, xh, dr):
    """Open boundaries: the periodic oracle on a padded mesh, cropped.  Below R = N/2 - 1 that is open_trace of the bright sources.
    With the radius beyond the box open_trace does not apply (its padded mesh has a wider periodic window than the N-box, so it
    reaches cells the N-box's window cuts off); but a cell's rate only depends on the cells between it and the source, so what each
    source gives the cells of ITS window is the same on both meshes: one padded trace per bright source, cropped and cut to the
    source's window, summed.  M = 2 N: no window -N ... N - 1 around a source of the N-box wraps back into the N-box."""
    sets, dlog = tables()
    thin, thick = sets[0][:2]
    pos0, flux = _bright(src)
    if case.R < case.N / 2 - 1:
        return OB.open_trace(case.R, cases.SIG, dr, nd, xh, pos0, flux, thin, thick, cases.MINLOGTAU, dlog, NumTau=thin.shape[0] - 1)["phi_ion"]
    return open_trace_by_source(case.R, dr, nd, xh, pos0, flux, thin, thick, dlog)


def open_trace_by_source(R, dr, nd, xh, pos0, flux, thin, thick, dlog):
    """The open-boundary trace at any radius: one padded trace per source, cut to the source's window (see _open_reference)."""
    N = nd.shape[0]
    M = 2 * N
    big_nd, big_xh = OB.embed(nd, M, 0, 1e-2), OB.embed(xh, M, 0, 0.0)
    phi = np.zeros((N, N, N))
    for s in range(flux.shape[0]):
        one = O.asora_do_all_sources(R, cases.SIG, dr, big_nd, big_xh, pos0[3 * s:3 * s + 3], flux[s:s + 1], thin, thick,
                                     cases.MINLOGTAU, dlog, NumTau=thin.shape[0] - 1, flags=O.ASORA_MODE)["phi_ion"]
        phi += np.where(reach(N, R, pos0[3 * s:3 * s + 3], periodic=False), OB.crop(one, N, 0), 0.0)
    return phi


def bright_positions(name):
    """(K, 3) 0-based positions of the bright sources, in upload order."""
    return _bright(build_sources(name))[0].reshape(-1, 3)
