"""TEST INFRASTRUCTURE: the loop trips, tail words and table limits of the Lyman-alpha forest (csrc/lya_forest.hip; DESIGN.md section
4.2k), the light cone (csrc/lightcone.hip; 4.2m) and the halo-catalogue sources (csrc/halo_sources.hip; 4.1e) that the first mesh lists
of their tests did not reach, each with the case that reaches it and what the case is there for.  Shared by
test_untested_trips_host.py (every claim, by arithmetic alone), test_gpu_lyman_alpha.py, test_gpu_lightcone.py and
test_gpu_halo_sources.py.

The module restates constants and three host rules of the units in plain Python; it does not call the library.

* The mask words of a line (lya_tiles): (N + 63) // 64 words of 64 pixels; the last has 64 words - N pad bits, none where 64 | N.
* The tiles of the forest (lya_tiles): along axis 2 T contiguous rows, as many as fit 48 KiB of LDS (128 at the most); along the axes 0
  and 1 T adjacent columns, the largest of 16, 8 whose lines fit 156 KiB, else 4.  Along axis 1 the columns of every i are tiled on their
  own, so a tile also ends where an i ends.
* The cut of a plane list into runs (lc_cut_runs, axis 2): maximal stretches in which consecutive slices take consecutive planes, all
  ascending or all descending, in pieces of at most LC_RUN_MAX; a piece of LC_RUN_MIN or more is a run, every other slice goes on the
  list.
"""
import collections

import numpy as np

# ---- Lyman-alpha forest --------------------------------------------------------------------------------------------------------
LYA_WORD = 64
LYA_LDS_ROWS, LYA_LDS_COLUMNS = 48 * 1024, 156 * 1024
LYA_MAX_WAVES = 16
LYA_MAX_BINS = 1024                 # ASORA_LYA_MAX_BINS: the statistics kernel holds LYA_MAX_BINS + 1 edges in LDS
#: the meshes of the crafted masks: one exact word; two; two and one bit; three (the first mesh on which either search of the gap walk
#: steps over a whole word); and five exact words with tiles of 8 columns and of 4 rows
LYA_MESHES = (64, 128, 129, 192)
LYA_MESH_OF_8_COLUMNS = 320


def mask_words(N):
    return (N + 63) // 64


def pad_bits(N):
    return LYA_WORD * mask_words(N) - N


def lya_tile_lines(N, axis):
    """T of lya_tiles(N, axis)"""
    pitch = N | 1
    line = 4 * pitch * 8 + mask_words(N) * 8
    fixed = LYA_MAX_WAVES * 8 + (N + 1) * 4
    if axis == 2:
        return max(1, min(128, (LYA_LDS_ROWS - fixed) // line))
    for T in (16, 8):
        if T * line + fixed <= LYA_LDS_COLUMNS:
            return T
    return 4


def lya_tile_starts(N, axis, T):
    """The first line of every tile, as indices into the N^2 lines along `axis` (C order of the two other axes), ascending"""
    if axis == 1:
        return [i * N + c for i in range(N) for c in range(0, N, T)]
    return list(range(0, N * N, T))


def lya_placement(N, axis, T, n_lines):
    """Where the crafted lines go: a dict of `lines_at` (position q takes crafted line q mod n_lines), `boundaries` (the tile
    starts b with b - 1 and b both among them) and `last_width` (the lines of the last tile).  Three stretches: from line 0 over whole
    tiles until every crafted line has had a place and a boundary is crossed; the same up to the last line; and the two lines either
    side of a boundary in the middle."""
    starts = lya_tile_starts(N, axis, T)
    rows = N * N
    head_end = next(b for b in starts if b >= n_lines + 1) + 1               # one line into the tile behind
    tail_start = max(b for b in starts if b <= rows - n_lines - 1) - 1       # one line before the tile
    middle = starts[len(starts) // 2]
    assert head_end < middle - 1 and middle + 1 < tail_start, (N, axis, T)
    lines_at = list(range(head_end)) + [middle - 1, middle] + list(range(tail_start, rows))
    chosen = set(lines_at)
    boundaries = [b for b in starts if b > 0 and b - 1 in chosen and b in chosen]
    return dict(lines_at=lines_at, boundaries=boundaries, last_width=rows - starts[-1], starts=starts)


# ---- light cone ----------------------------------------------------------------------------------------------------------------
PS_THREADS = 256
LC_MAX_BLOCKS = 8192
LC_EMIT_TRIP = LC_MAX_BLOCKS * PS_THREADS          # the outputs of one trip of lc_emit_kernel
LC_RUN_MIN, LC_RUN_MAX = 4, 32
LC_MAX_SLICES = 1024                               # ASORA_LC_MAX_SLICES
LC_RUN_TABLE = LC_MAX_SLICES // LC_RUN_MIN         # the int4 the parameter area holds, directly before the moments
LC_MESH = 70

Run = collections.namedtuple("Run", "t0 len k0 step")


def cut_runs(planes):
    """(runs, list) of lc_cut_runs"""
    planes = [int(p) for p in planes]
    n, t, runs, listed = len(planes), 0, [], []
    while t < n:
        length, step = 1, 0
        if t + 1 < n and abs(planes[t + 1] - planes[t]) == 1:
            step = planes[t + 1] - planes[t]
            while t + length < n and length < LC_RUN_MAX and planes[t + length] - planes[t + length - 1] == step:
                length += 1
        if length >= LC_RUN_MIN:
            runs.append(Run(t, length, planes[t] if step > 0 else planes[t + length - 1], step))
        else:
            listed += list(range(t, t + length))
        t += length
    return runs, listed


def emit_trips(outputs):
    """the trips of the grid-stride loop of lc_emit_kernel over `outputs` outputs, as a fraction"""
    return outputs / LC_EMIT_TRIP


def fold_workgroups(n_slices):
    return (2 * n_slices + PS_THREADS - 1) // PS_THREADS


def planes_without_a_run(N, n=LC_MAX_SLICES):
    """Steps of +3 (and of 3 - N through the wrap), every 41st slice repeating the plane before it: no two consecutive slices take
    consecutive planes, so every slice goes on the list"""
    out, p = [], 1
    for t in range(n):
        if t % 41 != 40:
            p = (p + 3) % N
        out.append(p)
    return np.array(out, dtype=np.int64)


def planes_in_runs_of_4(N, n_runs=LC_RUN_TABLE):
    """n_runs runs of exactly LC_RUN_MIN planes, ascending and descending in turn, each begun 7 planes (mod N - 3) behind the one
    before: the jump between two runs is never a step of one"""
    out = []
    for r in range(n_runs):
        base = 7 * r % (N - 3)
        run = list(range(base, base + LC_RUN_MIN))
        out += run if r % 2 == 0 else run[::-1]
    return np.array(out, dtype=np.int64)


def planes_mixed(N, n_runs=31, n_single=32):
    """single, run of LC_RUN_MAX, single, ..., single: the runs ascending and descending in turn, every single slice at least two
    planes from both its neighbours"""
    runs = []
    for r in range(n_runs):
        base = 5 * r % (N - LC_RUN_MAX + 1)
        run = list(range(base, base + LC_RUN_MAX))
        runs.append(run if r % 2 == 0 else run[::-1])
    out = []
    for s in range(n_single):
        before = runs[s - 1][-1] if s > 0 else None
        behind = runs[s][0] if s < n_runs else None
        out.append(next(p for p in range(N - 1, -1, -1) if all(q is None or abs(p - q) >= 2 for q in (before, behind))))
        if s < n_runs:
            out += runs[s]
    return np.array(out, dtype=np.int64)


#: name -> (the plane list, the runs and the listed slices lc_cut_runs is to make of it, what it is there for)
def plane_lists(N=LC_MESH):
    return {
        "no_run": (planes_without_a_run(N), 0, LC_MAX_SLICES,
                   "1024 slices through the list form of lc_emit_kernel: 2.39 trips of its grid-stride loop at N = 70"),
        "runs_of_4": (planes_in_runs_of_4(N), LC_RUN_TABLE, 0,
                      "256 runs: the run table full to the last int4 before the moments"),
        "mixed": (planes_mixed(N), 31, 32,
                  "31 runs of LC_RUN_MAX and 32 listed slices between them: both kernels write one staging buffer"),
    }


# ---- halo sources --------------------------------------------------------------------------------------------------------------
HS_THREADS = 256
HS_WAVES = HS_THREADS // 64
HS_SCAN_TILE = 4096
HS_ROW_BLOCKS_PER_CU = 32
HS_CHUNK_SCAN_NEEDS = HS_SCAN_TILE * HS_THREADS    # occupied cells beyond which the chunk scan takes a second tile
HS_MESH = 192


def rows_second_trip(N, cus):
    """does a wave of halo_rows_kernel take a second row at mesh N on a device of `cus` compute units"""
    return N * N > cus * HS_ROW_BLOCKS_PER_CU * HS_WAVES


def halo_catalogue(N=HS_MESH, n_uniform=300_000, seed=1920):
    """One halo at the centre of every cell with (i + 2 j + 3 k) mod 5 = 0 and n_uniform more anywhere in the box; masses
    10^U(7.5, 12).  (pos, mass)"""
    rng = np.random.default_rng(seed)
    i, j, k = np.meshgrid(*[np.arange(N)] * 3, indexing="ij")
    sel = (i + 2 * j + 3 * k) % 5 == 0
    lattice = np.stack([i[sel], j[sel], k[sel]], axis=1) + 0.5
    pos = np.concatenate([lattice, rng.uniform(0.0, N, size=(n_uniform, 3))])
    mass = 10.0 ** rng.uniform(7.5, 12.0, size=pos.shape[0])
    return pos, mass
