"""Sparse golden vectors for the 257-shell bench of tests/form_recipes.py, from THIS REPOSITORY'S OWN ORACLE (oracle/c2ray_oracle.c).

    make -C oracle
    python tests/golden/make_form_257_shells_golden.py          (a few minutes and about 12 GB on one CPU core)

N = 512, one source at (256, 256, 256), R beyond the box: 257 shells, the only launches that take the 1024-entry LDS tables.  The
oracle visits a cell in about 360 ns, so one whole-box trace takes 50 s: too long for a test, hence this fixture.  Two traces on the
seeded separable medium of form_recipes.make_medium:
  1. set 0 of launch_forms.tables() with its heating tables and the column densities: serves the table, heating and dump rows;
  2. grey opacity: serves the grey rows (its column densities are those of trace 1, asserted here: the grey dump row shares them).
The open rows share trace 1: the window -256 ... 255 of a source at 256 is the whole box and nothing wraps, so the open trace is the
periodic one.  That argument is asserted here on the oracle at a small even mesh (N = 16, source at (8, 8, 8)) against the
padded-mesh reference of tests/launch_forms.py.

Stored per field (form_257_shells_<field>.npz; form_recipes.digest): the values at 30 000 seeded cells and along the three axis
lines through the source, the sums over every i-plane and every 16^3 block, the count of non-zero cells, the total, the count of
cells at exactly +0 (none: every cell is inside the reach and the medium has no optical depth beyond the tables), and the checksums
of the seeded inputs (form_recipes.input_checksums), which tests/test_form_recipes_host.py re-derives.
Data only: the inputs are regenerated from seeds at test time.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, os.path.join(HERE, ".."))

import cases  # noqa: E402
import form_recipes as FR  # noqa: E402
import launch_forms as LF  # noqa: E402
from oracle import oracle as O  # noqa: E402

BENCH = "shells_257"


def open_equals_periodic_for_a_centred_source():
    """N even, the source at N / 2 on every axis, R beyond the box: open boundaries change nothing."""
    N = 16
    nd, xh = FR.make_medium(N, 5, True)
    (thin, thick, _, _), dlog = LF.tables()[0][0], LF.tables()[1]
    pos0, flux = np.array([8, 8, 8], dtype=np.int32), np.array([3.0])
    per = O.asora_do_all_sources(1000.0, cases.SIG, 2.0 ** 63, nd, xh, pos0, flux, thin, thick, cases.MINLOGTAU, dlog,
                                 NumTau=thin.shape[0] - 1, flags=O.ASORA_MODE)["phi_ion"]
    opn = LF.open_trace_by_source(1000.0, 2.0 ** 63, nd, xh, pos0, flux, thin, thick, dlog)
    assert per.min() > 0 and np.array_equal(per, opn)


def main():
    open_equals_periodic_for_a_centred_source()
    b = FR.BENCHES[BENCH]
    N, pos = b.N, b.pos[0]
    t0 = time.time()
    nd, xh = FR.medium(BENCH)
    sums = FR.input_checksums(nd, xh)
    assert sums[6] > 0.0 and 1e-4 <= sums[4] and sums[5] <= 1e-2            # nHI > 0 everywhere; x in [1e-4, 1e-2]
    print(f"medium in {time.time() - t0:.1f} s; checksums {sums[:7]}", flush=True)
    fields = {}
    t0 = time.time()
    one = FR._oracle_one(BENCH, 1000.0, 0, nd, xh, 0, heat=True, coldens=True)
    print(f"tables, heating and column densities: {time.time() - t0:.0f} s, {one['visited']} cells visited", flush=True)
    fields.update(phi_ion=one["phi_ion"], phi_heat=one["phi_heat"], coldens=one["coldens"])
    t0 = time.time()
    grey = FR._oracle_one(BENCH, 1000.0, 0, nd, xh, 0, grey=True, coldens=True)
    print(f"grey opacity: {time.time() - t0:.0f} s", flush=True)
    assert np.array_equal(grey["coldens"], one["coldens"])
    fields["grey_phi_ion"] = grey["phi_ion"]
    for name in FR.FIXTURE_FIELDS:
        a = fields[name]
        out = FR.digest(a, pos)
        zero_inside = int((a == 0).sum())                                  # the reach is the whole box
        if name != "coldens":
            assert zero_inside == 0 and not np.signbit(a).any() and np.isfinite(a).all(), name
        out.update(zero_inside=np.array(zero_inside), inputs=sums)
        np.savez_compressed(FR.fixture_path(name), **out)
        print(f"{name}: nonzero {int(out['nonzero'])}, total {float(out['total']):.6e}, {os.path.getsize(FR.fixture_path(name))} bytes", flush=True)


if __name__ == "__main__":
    main()
