"""CPU: what the new cases of tests/test_gpu_powerspec.py and tests/test_gpu_smoothing.py rest on (tests/fft_meshes.py).  Every claim
of a row -- its plan, its tile, its tails, its LDS request, what it is said to add -- is checked by arithmetic from the two rules the
module restates from csrc/fft_device.hpp; no device and no library is involved."""
import math

import pytest

import fft_meshes as FM


def test_the_rows_are_those_of_the_issue():
    assert FM.MESHES == (121, 139, 140, 169, 243, 256, 271, 272, 273)
    assert [(r.plan, r.T) for r in FM.ROWS.values()] == [((11, 11), 16), ((139,), 16), ((4, 5, 7), 8), ((13, 13), 8), ((3,) * 5, 8), ((4,) * 4, 8),
                                                         ((271,), 8), ((4, 4, 17), 4), ((3, 7, 13), 4)]


def test_the_rules_on_the_old_meshes():
    """the restated rules give what the header's comments say of meshes the suite already has"""
    assert FM.plan(1) == () and FM.plan(2) == (2,) and FM.plan(8) == (4, 2) and FM.plan(64) == (4, 4, 4) and FM.plan(30) == (2, 3, 5)
    assert FM.plan(129) == (3, 43) and FM.plan(136) == (4, 2, 17) and FM.plan(250) == (2, 5, 5, 5) and FM.plan(645) == (3, 5, 43)
    assert [FM.tile(N) for N in (2, 136, 144, 250, 280, 645)] == [16, 16, 8, 8, 4, 4]
    assert 90 * 1024 < FM.lds_bytes(645, 4) == 92880 <= 91 * 1024      # "91 KiB at N = 645"
    assert all(len(FM.plan(N)) <= 12 and math.prod(FM.plan(N)) == N for N in range(1, 646))


@pytest.mark.parametrize("N", FM.MESHES)
def test_every_claim_of_a_row(N):
    row = FM.ROWS[N]
    assert math.prod(row.plan) == N and FM.plan(N) == row.plan
    assert FM.tile(N) == row.T
    NZ = N // 2 + 1
    assert row.tails == (NZ % row.T, N * NZ % row.T, N * N % row.T) == FM.tails(N, row.T)
    if row.lds is not None:
        assert FM.lds_bytes(N, row.T) == row.lds <= FM.LDS_LIMIT
    # the filter pass asks for more than the rule allows for; it has to stay within the 160 KiB of a compute unit
    assert FM.filter_lds_bytes(N, row.T) <= 160 * 1024
    print(f"N {N}: plan {row.plan}, T {row.T}, NZ {NZ}, tails {row.tails}, LDS {FM.lds_bytes(N, row.T)} B (filter pass "
          f"{FM.filter_lds_bytes(N, row.T)} B)")


def test_the_tile_edges_straddle_the_rule():
    for below, above in FM.TILE_EDGES:
        T = FM.tile(below)
        assert above == below + 1 and FM.tile(above) == T // 2
        assert FM.lds_bytes(below, T) <= FM.LDS_LIMIT < FM.lds_bytes(above, T)
    assert FM.LDS_LIMIT - FM.lds_bytes(139, 16) == 336 and FM.LDS_LIMIT - FM.lds_bytes(271, 8) == 16
    assert (FM.lds_bytes(139, 16), FM.lds_bytes(271, 8)) == (73392, 73712)
    # they are THE edges: every mesh below takes the larger tile, every mesh above the smaller one
    assert all(FM.tile(N) == 16 for N in range(1, 140)) and all(FM.tile(N) == 8 for N in range(140, 272))
    assert all(FM.tile(N) == 4 for N in range(272, 646))


def test_what_the_rows_are_there_for():
    R, tails = FM.ROWS, {N: r.tails for N, r in FM.ROWS.items()}
    # two generic stages: the same prime twice at T = 16 and at T = 8; the first of them is followed by a stage, so its twiddles count
    assert FM.generic_stages(121) == [11, 11] and FM.generic_stages(169) == [13, 13] and R[121].T == 16 and R[169].T == 8
    # tails in all three passes at every tile size
    assert all(tails[121]) and all(tails[139]) and all(tails[169]) and all(tails[243]) and all(tails[273])
    assert {R[N].T for N in (121, 139, 169, 243, 273)} == {16, 8, 4}
    assert tails[121] == (13, 5, 1) and tails[169] == (5, 5, 1) and tails[273] == (1, 1, 1) and 273 // 2 + 1 == 137 and 273 % 2 == 1
    # primes; 271 is beyond one trip of a workgroup over a line
    for N in (139, 271):
        assert FM.plan(N) == (N,)
    assert 139 < FM.PS_THREADS < 271
    # the roots beyond index 255 come in by a second trip of the load; a mesh beyond 256 need not read one (273 and the old 280 do not)
    assert [FM.largest_root_read(N) for N in (2, 17, 121, 256, 271, 272, 273, 280)] == [0, 16, 110, 189, 270, 256, 252, 207]
    old = (2, 3, 4, 5, 7, 8, 9, 16, 17, 30, 43, 49, 64, 96, 129, 136, 144, 250, 280)
    assert [N for N in old + FM.MESHES if FM.largest_root_read(N) >= FM.PS_THREADS] == [271, 272]
    # five stages, an odd count; the deepest plans of the old lists have at most four stages
    assert len(R[243].plan) == 5 and len(R[256].plan) == 4
    assert max(len(FM.plan(N)) for N in (2, 3, 4, 5, 7, 8, 9, 16, 17, 30, 43, 49, 64, 96, 129, 136, 144, 250, 280)) == 4
    # the binning's loop over n_z in steps of 64 lanes
    assert [(N // 2 + 1, -(-(N // 2 + 1) // 64), (N // 2 + 1) % 64) for N in (121, 140, 169, 256)] == [(61, 1, 61), (71, 2, 7), (85, 2, 21),
                                                                                                      (129, 3, 1)]
    # uneven trips of the fixed grids of 131 072 work items; the row workgroups the one-workgroup fold takes
    assert FM.PS_SUM_THREADS == 131072
    for N in (121, 169, 273):
        assert N ** 3 % FM.PS_SUM_THREADS != 0
    assert 13.5 < 121 ** 3 / FM.PS_SUM_THREADS < 13.6 and 36.8 < 169 ** 3 / FM.PS_SUM_THREADS < 36.9
    blocks = -(-121 * 121 // 16)
    assert blocks == 916 and -(-blocks // FM.PS_THREADS) == 4 and blocks % FM.PS_THREADS != 0
    # 256 bins of the cross form: four waves' histograms of five values and the thresholds
    assert 4 * 5 * 256 * 8 + 4 * 257 == 41988
