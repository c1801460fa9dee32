"""GPU: raytrace launches whose blocks are dealt by the dispatch order of `block_order` (csrc/raytrace_plan.hpp; the kernel's
p.order) against the CPU oracle, by the zero-flux-filler method of tests/launch_forms.py: NS sources on the device of which a few
carry flux, the reference the oracle over those few.  A filler's workgroup adds exact zeros, so the bright sources sit where the
order can go wrong: first and last of a lane's slice of a unit, both members of a pair, alone in an odd leftover, on the box
corners.  Every case starts from a fresh device_init and asserts the form it ran in (asora_last_raytrace_variant).

  (a) N = 64, R = 30, NS = 1003: six sectors x 256 threads, two sources per workgroup, line-aligned tables; 505 pairs by k (class 3
      empty, seven odd leftovers) and 502 by i (one odd leftover), neither a multiple of 8
  (b) the twelve-sector-pair aligned shape of tests/launch_forms.py (N = 128, R = 41, NS = 1000), its sources and reference
  (c) N = 64, R = 30, NS = 125: six sectors, one source per workgroup, line-aligned tables; and the same form with 345 sources
      (ASORA_OPT_PAIR_SOURCES = 1: never two per workgroup), several rounds of resident workgroups
  (d) a sub-range (begin > 0, odd count) through the three-part call (asora_raytrace_begin / _range / _fold) that the sharded loop's
      chunked exchange traces its ranges with (pyc2ray_amd/dist.py, raytrace_and_allreduce)
  (e) a trace, the upload of another list of another count, a trace: the cached order is dropped with the source list
  (f) five sources: a spread launch, which takes the arithmetic map of the kernel's prologue (no order)
Tolerance: GAMMA_RTOL of tests/test_gpu_parity.py, as tests/test_gpu_launch_forms.py; the pattern of exact zeros cell for cell.
The reference of the cases on the N = 64 mesh is the sum of one oracle trace per bright source (the oracle is linear in the
sources to the order of its sum, 1e-13: tests/test_launch_forms_host.py), each traced once and shared."""
import functools

import numpy as np
import pytest

import cases
import launch_forms as LF
from test_block_order_host import positions
from test_gpu_parity import GAMMA_RTOL

pytestmark = pytest.mark.gpu

N, R = 64, 30.0
CASE = LF.Case(N, 0, R, 6, 256, True, True, False, 41)      # what _oracle reads: R
K_COUNTS = [145, 143, 143, 0, 143, 143, 143, 143]           # 505 pairs
I_COUNTS = [126, 126, 126, 126, 126, 126, 126, 121]         # 502 pairs


@pytest.fixture(scope="module")
def asora():
    import pyc2ray_amd as p
    from pyc2ray_amd import _capi
    from pyc2ray_amd.load_extensions import load_asora
    lib = load_asora()
    yield p, lib, _capi
    lib.set_option(_capi.OPT_SKIP_ZERO_RATES, 0)
    lib.set_option(_capi.OPT_PAIR_SOURCES, 0)
    if p.cuda_is_init():
        p.device_close()


@functools.lru_cache(maxsize=None)
def medium():
    nd, xh, _ = cases.grid(N, "lognormal", 141, 0.05, xlo=1e-4, xhi=1e-2)
    nd.setflags(write=False)
    xh.setflags(write=False)
    return nd, xh, 2.0 ** 63


@functools.lru_cache(maxsize=None)
def one_source(pos, flux):
    nd, xh, dr = medium()
    phi = LF._oracle(CASE, nd, xh, dr, np.array(pos, dtype=np.int32), np.array([flux]), 0, False)["phi_ion"]
    phi.setflags(write=False)
    return phi


def reference(pos0, flux):
    p = np.asarray(pos0).reshape(-1, 3)
    phi = np.zeros((N, N, N))
    for s in np.flatnonzero(flux):
        phi += one_source(tuple(int(x) for x in p[s]), float(flux[s]))
    return phi


def with_corners(pos0):
    """The sorted list with a source of classes (0, 0) moved to (0, 0, 0) and one of classes (7, 7) to (N-1, N-1, N-1): the class
    counts stay."""
    p = pos0.reshape(-1, 3).copy()
    for cls, corner in ((0, 0), (7, N - 1)):
        s = np.flatnonzero((p[:, 0] % 8 == cls) & (p[:, 2] % 8 == cls))[0]
        p[s] = corner
    return np.ascontiguousarray(p[LF.sort_order(p)], dtype=np.int32).ravel()


def bright_by_order(order, pos0, units_lanes):
    """Fluxes that light, for each (unit, lane): both sources of the first group of the lane's slice of the unit and the first source
    of its last group; and the two corners."""
    n = pos0.size // 3
    flux = np.zeros(n)
    lit = [0, n - 1]
    for unit, x in units_lanes:
        lane = order[x::8]
        mine = lane[lane[:, 1] == unit]
        assert mine.shape[0] >= 2
        lit += [int(mine[0, 2]), int(mine[-1, 2])] + ([int(mine[0, 3])] if mine[0, 3] >= 0 else [])
    lit = sorted(set(lit))
    flux[lit] = 3.0 * (1.0 + 0.25 * np.arange(len(lit)))
    return flux


def setup(p, lib, capi, pos0, flux, n=N, nd_xh=None):
    nd, xh, _ = medium() if nd_xh is None else nd_xh
    sets, _ = LF.tables()
    if p.cuda_is_init():
        p.device_close()
    p.device_init(n, 8)
    p.photo_table_to_device(sets[0][0], sets[0][1])
    lib.source_data_to_device(pos0, flux, flux.size)
    lib.grid_to_device(capi.GRID_NDENS, nd)
    lib.grid_to_device(capi.GRID_XH_AV, xh)


def trace(lib, capi, radius, dr, count, n=N, pair_sources=0):
    sets, dlog = LF.tables()
    lib.set_option(capi.OPT_SKIP_ZERO_RATES, 2)
    lib.set_option(capi.OPT_PAIR_SOURCES, pair_sources)
    try:
        lib.raytrace_device(radius, cases.SIG, dr, 0, count, cases.MINLOGTAU, dlog, sets[0][0].shape[0] - 1)
        return lib.grid_to_host(capi.GRID_PHI_ION, np.empty((n, n, n)))
    finally:
        lib.set_option(capi.OPT_SKIP_ZERO_RATES, 0)
        lib.set_option(capi.OPT_PAIR_SOURCES, 0)


def against(got, ref, tag):
    w = ref != 0
    rel = np.max(np.abs(got[w] - ref[w]) / ref[w])
    print(f"{tag}: max rel. difference {rel:.3e} over {int(w.sum())} cells")
    assert w.sum() > 0 and np.array_equal(got != 0, w), f"{tag}: {int(((got != 0) != w).sum())} cells are zero on one side only"
    np.testing.assert_allclose(got[w], ref[w], rtol=GAMMA_RTOL, atol=0, err_msg=tag)


def variant(lib):
    v = lib.last_raytrace_variant()
    return v["units"], v["threads"], v["paired"], v["aligned"]


_LIST_A = []


def list_a(lib):
    """The list of case (a), built once: positions, fluxes, its dispatch order."""
    if not _LIST_A:
        pos0 = with_corners(positions(41, N, I_COUNTS, K_COUNTS))
        order = lib.block_order(pos0, 6, 2, True, cu_count=256)
        flux = bright_by_order(order, pos0, ((5, 3), (2, 6)))      # a z-sector unit (pairs by i) and a y-sector unit (pairs by k)
        _LIST_A.append((pos0, flux, order))
    return _LIST_A[0]


def test_a_six_sectors_paired_aligned(asora):
    p, lib, capi = asora
    pos0, flux, order = list_a(lib)
    ns = flux.size
    groups = LF.workgroups(pos0.reshape(-1, 3), True)
    assert ns == 1003 and (len(groups[0]), len(groups[1])) == (505, 502)
    assert sum(b < 0 for _, b in groups[0]) == 7 and sum(b < 0 for _, b in groups[1]) == 1
    lit = np.flatnonzero(flux)
    assert any((a in lit and b in lit) for a, b in groups[0] + groups[1])           # both members of one pair
    assert flux[0] > 0 and flux[-1] > 0 and not pos0[:3].any() and np.all(pos0[-3:] == N - 1)
    setup(p, lib, capi, pos0, flux)
    phi = trace(lib, capi, R, medium()[2], ns)
    assert variant(lib) == (6, 256, True, True)
    assert lib.last_raytrace_counts()[0] == ns * LF.cells_within(N, R)
    against(phi, reference(pos0, flux), "six sectors, paired, aligned")


def test_b_twelve_sector_pairs_aligned(asora):
    p, lib, capi = asora
    name = "n128_1000_R41"
    case, src = LF.CASES[name], LF.build_sources(name)
    nd, xh, dr = LF.medium(name)
    setup(p, lib, capi, src.pos0, src.flux, case.N, (nd, xh, dr))
    phi = trace(lib, capi, case.R, dr, case.NS, case.N)
    assert variant(lib) == (12, 256, True, True)
    assert lib.last_raytrace_counts()[0] == case.NS * LF.cells_within(case.N, case.R)
    against(phi, LF.reference(name, "tables")["phi_ion"], name)


@pytest.mark.parametrize("ns", [125, 345])
def test_c_six_sectors_single_sources(asora, ns):
    p, lib, capi = asora
    counts = {125: ([16, 16, 16, 16, 16, 15, 15, 15], [15, 16, 15, 16, 15, 16, 16, 16]),
              345: ([44, 43, 43, 43, 43, 43, 43, 43], [43, 44, 43, 44, 43, 42, 43, 43])}[ns]
    pos0 = with_corners(positions(43, N, *counts))
    order = lib.block_order(pos0, 6, 1, True, cu_count=256)
    flux = bright_by_order(order, pos0, ((4, 0), (1, 7)))
    assert flux.size == ns
    setup(p, lib, capi, pos0, flux)
    phi = trace(lib, capi, R, medium()[2], ns, pair_sources=1)
    assert variant(lib) == (6, 256, False, True)
    assert lib.last_raytrace_counts()[0] == ns * LF.cells_within(N, R)
    against(phi, reference(pos0, flux), f"six sectors, {ns} single sources")


def test_d_sub_range_of_the_three_part_call(asora):
    p, lib, capi = asora
    pos0, flux, _ = list_a(lib)
    begin, count = 200, 803
    order = lib.block_order(pos0, 6, 2, True, begin=begin, count=count, cu_count=256)
    assert order is not None
    sub = np.zeros_like(flux)
    sub[begin:begin + count] = bright_by_order(order, pos0, ((5, 3), (2, 6)))[begin:begin + count]
    sub[[begin, begin + count - 1]] = (2.0, 5.0)                    # the ends of the range
    assert np.count_nonzero(sub) >= 5
    sets, dlog = LF.tables()
    setup(p, lib, capi, pos0, sub)
    lib.set_option(capi.OPT_SKIP_ZERO_RATES, 2)
    try:
        lib.raytrace_begin(R, cases.SIG, medium()[2], cases.MINLOGTAU, dlog, sets[0][0].shape[0] - 1)
        lib.raytrace_range(begin, count)
        lib.raytrace_fold(0, N)
        lib.synchronize()
    finally:
        lib.set_option(capi.OPT_SKIP_ZERO_RATES, 0)
    phi = lib.grid_to_host(capi.GRID_PHI_ION, np.empty((N, N, N)))
    assert variant(lib) == (6, 256, True, True)
    assert lib.last_raytrace_counts()[0] == count * LF.cells_within(N, R)
    against(phi, reference(pos0, sub), "sub-range")


def test_e_another_list_drops_the_cached_order(asora):
    p, lib, capi = asora
    pos0, flux, _ = list_a(lib)
    setup(p, lib, capi, pos0, flux)
    trace(lib, capi, R, medium()[2], flux.size)
    assert variant(lib) == (6, 256, True, True)
    other = with_corners(positions(47, N, [125] * 7 + [126], [127, 123, 125, 125, 121, 129, 125, 126]))
    order = lib.block_order(other, 6, 2, True, cu_count=256)
    oflux = bright_by_order(order, other, ((4, 1), (0, 5)))
    assert oflux.size == 1001
    lib.source_data_to_device(other, oflux, oflux.size)
    phi = trace(lib, capi, R, medium()[2], oflux.size)
    assert variant(lib) == (6, 256, True, True)
    assert lib.last_raytrace_counts()[0] == 1001 * LF.cells_within(N, R)
    against(phi, reference(other, oflux), "second list")


def test_f_spread_launch_keeps_the_arithmetic_map(asora):
    p, lib, capi = asora
    pos0 = np.array([0, 0, 0, 5, 60, 33, 31, 32, 30, 40, 7, 63, 63, 63, 63], dtype=np.int32)
    flux = np.array([3.0, 0.0, 4.0, 5.0, 6.0])
    assert lib.block_order(pos0, 96, 1, False, cu_count=256) is None
    setup(p, lib, capi, pos0, flux)
    phi = trace(lib, capi, R, medium()[2], 5)
    assert variant(lib) == (96, 256, False, False)
    assert lib.last_raytrace_counts()[0] == 5 * LF.cells_within(N, R)
    against(phi, reference(pos0, flux), "spread")
