"""The sub-box sweep in the launch forms the library picks BY ITSELF on a 256-CU device: the inputs that lead it there, what it
should launch on them, and the CPU oracle's answer in the library's own loss convention.  Shared by test_subbox_forms_host.py
(the plan, and the conditions on the inputs -- both without a device) and test_gpu_subbox_forms.py.

Every row is a fresh log-normal mesh with soft tables (cases.soft_tables(400)), sources of real flux (uniform in 0.5 ... 4; the
first two on the box corners [1, N, 1] and [N, N, N], the rest seeded), max_subbox = 1000 and all options at 0.  A row's `tau`
(optical depth of a mean cell) and `seed` were tuned ON THE ORACLE ALONE until the conditions of check_conditions hold; they are
no measurements of the device.
"""
import numpy as np

import cases
from oracle import oracle as O

MAX_SUBBOX = 1000
#: the library's convention for cells that deposit nothing: they add 0 to the photon loss of their sub-box
LIBRARY_LOSS = O.STOPPED_CELLS_LOSE_NOTHING

#: name -> inputs, the form the library is to pick at 256 CUs (tables: units, threads, nsrc = sources per workgroup without
#: heating tables; on the fly: fly_threads), and `least`: the smallest source count of the call (the dumped source included)
#: at which that form is picked -- one source fewer and it is another one
ROWS = {
    # r < 11.5: the whole sphere in one workgroup of 256 threads, one source each (tables from 2 x 256 workgroups on)
    "sphere_256_r9":   dict(N=48, ns=600, box=4, R=9.0, lf=2e-2, tau=0.3, seed=1, units=1, threads=256, nsrc=1, least=513),
    # 11.5 <= r < 15.5: the same
    "sphere_256_r13":  dict(N=48, ns=600, box=5, R=13.0, lf=2e-2, tau=0.6, seed=2, units=1, threads=256, nsrc=1, least=513),
    # r >= 15.5: 512 threads and two sources per workgroup once (ns - 1) / 2 x 8 waves fill the chip
    "sphere_512_r18":  dict(N=56, ns=560, box=5, R=18.0, lf=2e-2, tau=0.3, seed=3, units=1, threads=512, nsrc=2, least=513),
    "halves_256_r22":  dict(N=56, ns=520, box=6, R=22.0, lf=2e-2, tau=0.3, seed=4, units=2, threads=256, nsrc=2, least=513),
    "halves_512_r24":  dict(N=56, ns=300, box=6, R=24.5, lf=2e-2, tau=0.2, seed=5, units=2, threads=512, nsrc=2, least=257),
    "sectors_256_r27": dict(N=64, ns=200, box=7, R=27.0, lf=1e-2, tau=0.3, seed=6, units=6, threads=256, nsrc=2, least=173),
    "pairs_256_r37":   dict(N=80, ns=100, box=8, R=37.0, lf=1e-2, tau=0.12, seed=7, units=12, threads=256, nsrc=2, least=87),
    # R_max_LLS beyond the range: no tables; 32 sources fill 256 CUs with their 8 octants, pitch W = 19 <= 20: 128 threads
    "fly_128":         dict(N=36, ns=80, box=4, R=1000.0, lf=2e-2, tau=0.36, seed=8, fly_threads=128, least=32),
    # W = 25: 256 threads, boxes grown over several launches
    "fly_256":         dict(N=48, ns=80, box=5, R=1000.0, lf=2e-2, tau=0.3, seed=9, fly_threads=256, least=32),
}
TABLE_ROWS = [k for k, r in ROWS.items() if "units" in r]
FLY_ROWS = [k for k, r in ROWS.items() if "fly_threads" in r]


def expected_plan(row, ns=None, heat=False):
    """What asora_debug_subbox_plan is to say for a call of `ns` sources (the row's own by default) on the row's mesh."""
    r = ROWS[row]
    ns = r["ns"] if ns is None else ns
    if "units" in r:
        return dict(table_sources=ns - 1, units=r["units"], threads=r["threads"], nsrc=1 if heat else r["nsrc"], aligned=0,
                    fly_sources=1, fly_threads=1024)
    return dict(table_sources=0, units=0, threads=0, nsrc=0, aligned=0, fly_sources=ns, fly_threads=r["fly_threads"])


_CASES = {}


def case(row):
    """The inputs of a row (cached; treat as read-only)."""
    if row not in _CASES:
        r = ROWS[row]
        N, ns = r["N"], r["ns"]
        rng = np.random.default_rng(5000 + r["seed"])
        nd, xh, dr = cases.grid(N, "lognormal", 6000 + r["seed"], r["tau"])
        pos = 1 + rng.integers(0, N, size=(3, ns))
        pos[:, 0], pos[:, 1] = [1, N, 1], [N, N, N]
        flux = rng.uniform(0.5, 4.0, size=ns)
        thin, thick, dlog = cases.soft_tables(400)
        _CASES[row] = dict(N=N, ns=ns, ndens=nd, xh=xh, dr=dr, pos=pos, flux=flux, thin=thin, thick=thick, dlogtau=dlog,
                           minlogtau=cases.MINLOGTAU, sig=cases.SIG, heat_thin=1e-11 * thin[::-1].copy(), heat_thick=3e-12 * thick,
                           box=r["box"], R=r["R"], lf=r["lf"])
    return _CASES[row]


def oracle_call(c, lf=None, heat=True, own_flux=False, first=0, count=None):
    """The oracle in the library's loss convention on sources [first, first + count) of a row's inputs."""
    count = c["ns"] - first if count is None else count
    sl = slice(first, first + count)
    return O.do_all_sources(c["flux"][sl], c["pos"][:, sl], MAX_SUBBOX, c["box"], c["sig"], c["dr"], c["ndens"], c["xh"],
                            c["lf"] if lf is None else lf, c["thin"], c["thick"], c["minlogtau"], c["dlogtau"], c["R"],
                            heat_thin=c["heat_thin"] if heat else None, heat_thick=c["heat_thick"] if heat else None,
                            flags=LIBRARY_LOSS | (O.PER_SOURCE_FLUX if own_flux else 0))


_REFS = {}


def reference(row, own_flux=False):
    """One oracle call per row with heating tables (the rates do not depend on them): serves the runs with and without (cached;
    treat as read-only)."""
    key = (row, own_flux)
    if key not in _REFS:
        _REFS[key] = oracle_call(case(row), own_flux=own_flux)
    return _REFS[key]


def box_shares(row, per_source):
    """(share of the sources that stop BEFORE the end of their range, share that grow to it).  The end of a source's range is the
    last box in which a launch still has work: the last box of the traversal range or, with R_max_LLS inside the range, the box
    that holds the last shell with a cell within the radius, floor(R) -- beyond it nothing is rated and, under the library's
    convention, nothing is lost, so nothing is launched.  (A source whose loss through the small cap of that shell's faces is
    still large is booked one further, empty box: it counts as grown to the end.)"""
    r = ROWS[row]
    N = r["N"]
    ext = min(MAX_SUBBOX, N // 2 - 1 + N % 2, N // 2)
    end = -(-min(ext, int(np.floor(r["R"]))) // r["box"])
    per_source = np.asarray(per_source)
    assert per_source.max() <= end + 1
    return float(np.mean(per_source < end)), float(np.mean(per_source >= end))


def check_conditions(row, ref):
    """Conditions on a row's INPUTS, from the oracle alone: sources that stop early and sources that reach the end of their
    range are both at least a tenth (so that `active[]` is mixed in the later launches), and some photons are lost (so that the
    1e-8 comparison of the loss is not 0 against 0)."""
    early, full = box_shares(row, ref["nbox_per_source"])
    assert early >= 0.1 and full >= 0.1, (row, early, full)
    assert ref["photon_loss"] > 0.0, row
    return early, full
