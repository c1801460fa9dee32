"""CPU: what the second-pass cases of tests/test_gpu_lyman_alpha.py, tests/test_gpu_lightcone.py and tests/test_gpu_halo_sources.py
rest on (tests/untested_trips.py).  Every claim -- the words of a line, the tiles the crafted lines straddle, the trips of the emit
kernel, the runs a plane list is cut into, the tiles of the scan -- is checked by arithmetic from the rules the module restates; the
public limits and the forest's tiles are read from the library where it exports them, so a changed constant fails here first.  No
device is involved."""
import os
import re

import numpy as np
import pytest

import lyman_alpha_reference as LR
import untested_trips as UT
from pyc2ray_amd import _capi

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyc2ray_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    from pyc2ray_amd.load_extensions import load_asora
    return load_asora()


def _constant(source, name):
    """the value of ``name = <integer>`` in a unit's constexpr lines"""
    found = re.search(r"\b" + name + r" = (\d+)\b", open(os.path.join(CSRC, source)).read())
    assert found, (source, name)
    return int(found.group(1))


def test_the_constants_are_the_units():
    assert (UT.LC_MAX_SLICES, UT.LYA_MAX_BINS) == (_capi.LC_MAX_SLICES, _capi.LYA_MAX_BINS) == (1024, 1024)
    assert UT.LC_MAX_BLOCKS == _constant("lightcone.hip", "LC_MAX_BLOCKS") and UT.LC_RUN_MIN == _constant("lightcone.hip", "LC_RUN_MIN")
    assert UT.LC_RUN_MAX == _constant("lightcone.hip", "LC_RUN_MAX") and UT.PS_THREADS == _constant("fft_device.hpp", "PS_THREADS")
    assert UT.HS_THREADS == _constant("halo_sources.hip", "HS_THREADS") and _constant("halo_sources.hip", "HS_SCAN_THREADS") * 4 == UT.HS_SCAN_TILE
    assert UT.HS_WAVES == UT.HS_THREADS // 64 == 4
    text = open(os.path.join(CSRC, "halo_sources.hip")).read()
    assert f"(size_t)st.cu_count * {UT.HS_ROW_BLOCKS_PER_CU});" in text and "HS_SCAN_TILE = 4 * HS_SCAN_THREADS" in text
    text = open(os.path.join(CSRC, "lightcone.hip")).read()
    assert "LC_P_MOMENTS = LC_P_RUNS + 2 * (ASORA_LC_MAX_SLICES / LC_RUN_MIN)" in text      # the moments lie directly behind the run table


# ---- Lyman-alpha forest --------------------------------------------------------------------------------------------------------
def test_the_words_of_the_crafted_meshes():
    meshes = UT.LYA_MESHES + (UT.LYA_MESH_OF_8_COLUMNS,)
    assert meshes == (64, 128, 129, 192, 320)
    assert [UT.mask_words(N) for N in meshes] == [1, 2, 3, 3, 5] and [UT.pad_bits(N) for N in meshes] == [0, 0, 63, 0, 0]
    # the meshes the gap counts were checked on before: at most two words, and pad bits in the last
    assert [(UT.mask_words(N), UT.pad_bits(N)) for N in (24, 33, 70)] == [(1, 40), (1, 31), (2, 58)]
    # from three words on a search of the gap walk can step over a whole word: the crafted run 40 ... 150 has word 1 wholly dark
    # and a wholly bright word 1 lies between the bright pixels' neighbours of "all bright but pixel 0"
    for N in (129, 192, 320):
        line = next(l for l in LR.crafted_lines(N) if l.sum() == 111) if N >= 192 else None
        if line is not None:
            assert not line[39] and line[40:151].all() and not line[151] and 40 // 64 == 0 and 150 // 64 == 2
        assert UT.mask_words(N) >= 3


@pytest.mark.parametrize("N", [64, 128, 129, 192, 320])
def test_the_tiles_and_the_placement(lib, N):
    n_lines = len(LR.crafted_lines(N))
    for axis in (0, 1, 2):
        T = UT.lya_tile_lines(N, axis)
        tiles = lib.lyman_alpha_forest_tiles(N, axis)
        assert tiles["lines"] == T and tiles["workgroups"] == len(UT.lya_tile_starts(N, axis, T))
        place = UT.lya_placement(N, axis, T, n_lines)
        at = place["lines_at"]
        assert len(set(at)) == len(at) and at[0] == 0 and at[-1] == N * N - 1 and len(at) >= 2 * n_lines + 2
        # every crafted line lies in the first stretch and in the last; both cross a boundary, and so does the pair in the middle
        assert at[:n_lines] == list(range(n_lines)) and at[-n_lines:] == list(range(N * N - n_lines, N * N))
        assert len(place["boundaries"]) >= 3 and all(b in place["starts"] for b in place["boundaries"])
        ragged = (N % T if axis == 1 else N * N % T)
        assert place["last_width"] == (ragged or T) and N * N - place["last_width"] in at
    if N == 320:
        assert [UT.lya_tile_lines(N, axis) for axis in (0, 1, 2)] == [8, 8, 4]
    else:
        assert [UT.lya_tile_lines(N, axis) for axis in (0, 1)] == [16, 16]


def test_the_tile_rule_on_the_old_meshes(lib):
    for N in (1, 24, 33, 70, 307, 308, 611, 612, 645):
        for axis in (0, 1, 2):
            assert lib.lyman_alpha_forest_tiles(N, axis)["lines"] == UT.lya_tile_lines(N, axis), (N, axis)
    assert [UT.lya_tile_lines(N, 0) for N in (307, 308, 611, 612)] == [16, 8, 8, 4]
    # out of reach of a GPU test: a grid of 612^3 doubles
    assert 612 ** 3 * 8 > 1.8e9


# ---- light cone ----------------------------------------------------------------------------------------------------------------
def test_the_trips_of_the_emit_kernel():
    N = UT.LC_MESH
    assert UT.LC_EMIT_TRIP == 2_097_152
    # the largest calls before: 2 N + 3 slices at N = 70 on the axes 0 and 1; 3 listed slices at N = 320 on axis 2
    assert (2 * 70 + 3) * 70 ** 2 == 700_700 < UT.LC_EMIT_TRIP and 3 * 320 ** 2 == 307_200 < UT.LC_EMIT_TRIP
    assert 2.39 < UT.emit_trips(UT.LC_MAX_SLICES * N * N) < 2.40
    assert UT.fold_workgroups(UT.LC_MAX_SLICES) == 8 and UT.fold_workgroups(2 * 70 + 3) == 2
    assert UT.LC_RUN_TABLE == 256


def test_the_cut_into_runs():
    cut = UT.cut_runs
    assert cut([]) == ([], []) and cut([5]) == ([], [0]) and cut([1, 2, 3]) == ([], [0, 1, 2])
    assert cut([1, 2, 3, 4]) == ([UT.Run(0, 4, 1, 1)], []) and cut([9, 8, 7, 6, 5]) == ([UT.Run(0, 5, 5, -1)], [])
    # a run through the wrap is cut there; a turn ends a run; a run of 33 is one of 32 and a listed slice
    assert cut([3, 2, 1, 0, 69, 68, 67]) == ([UT.Run(0, 4, 0, -1)], [4, 5, 6])
    assert cut([1, 2, 3, 4, 3, 2, 1]) == ([UT.Run(0, 4, 1, 1)], [4, 5, 6])
    assert cut(list(range(33))) == ([UT.Run(0, 32, 0, 1)], [32])
    assert cut(list(range(40))) == ([UT.Run(0, 32, 0, 1), UT.Run(32, 8, 32, 1)], [])
    assert cut([4, 4, 5, 6, 7, 8]) == ([UT.Run(1, 5, 4, 1)], [0])


def test_the_plane_lists():
    N = UT.LC_MESH
    lists = UT.plane_lists(N)
    assert list(lists) == ["no_run", "runs_of_4", "mixed"]
    for name, (planes, n_runs, n_listed, why) in lists.items():
        assert planes.size == UT.LC_MAX_SLICES and planes.min() >= 0 and planes.max() < N
        runs, listed = UT.cut_runs(planes)
        assert (len(runs), len(listed)) == (n_runs, n_listed), name
        assert sorted(listed + [t for r in runs for t in range(r.t0, r.t0 + r.len)]) == list(range(planes.size))
        for r in runs:                                             # what lc_emit_runs_kernel reads: planes k0 ... k0 + len - 1
            assert 0 <= r.k0 and r.k0 + r.len <= N and UT.LC_RUN_MIN <= r.len <= UT.LC_RUN_MAX and r.step in (1, -1)
            want = np.arange(r.k0, r.k0 + r.len)
            assert np.array_equal(planes[r.t0:r.t0 + r.len], want if r.step > 0 else want[::-1])
    steps = np.diff(lists["no_run"][0])
    assert np.all(np.abs(steps) != 1) and 20 <= np.sum(steps == 0) <= 30 and set(np.unique(steps)) == {3 - N, 0, 3}
    assert 2.39 < UT.emit_trips(len(UT.cut_runs(lists["no_run"][0])[1]) * N * N) < 2.40
    runs = UT.cut_runs(lists["runs_of_4"][0])[0]
    assert len(runs) == UT.LC_RUN_TABLE and all(r.len == UT.LC_RUN_MIN for r in runs) and [r.step for r in runs[:4]] == [1, -1, 1, -1]
    runs, listed = UT.cut_runs(lists["mixed"][0])
    assert all(r.len == UT.LC_RUN_MAX for r in runs) and {r.step for r in runs} == {1, -1} and listed[0] == 0 and listed[-1] == 1023


# ---- halo sources --------------------------------------------------------------------------------------------------------------
def test_the_tiles_of_the_scan_and_the_rows():
    N = UT.HS_MESH
    assert UT.HS_CHUNK_SCAN_NEEDS == 1_048_576 and 67 ** 3 == 300_763 < UT.HS_CHUNK_SCAN_NEEDS < N ** 3
    assert 67 * 67 == 4489 > UT.HS_SCAN_TILE                       # (the row scan had its second tile before; the chunk scan had not)
    # a wave's second row: from N = 182 on with 256 compute units
    assert not UT.rows_second_trip(181, 256) and UT.rows_second_trip(182, 256) and UT.rows_second_trip(N, 256)
    assert N % 64 == 0 and N // 64 == 3                            # a row of exactly three trips of 64 cells
    i, j, k = np.meshgrid(*[np.arange(N)] * 3, indexing="ij")
    assert int(np.sum((i + 2 * j + 3 * k) % 5 == 0)) == 1_415_578
