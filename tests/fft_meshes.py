"""TEST INFRASTRUCTURE: the meshes at which the transform units (csrc/fft_device.hpp, power_spectrum.hip, smooth_field.hip; DESIGN.md
sections 4.2h, 4.2i) take a plan, a tile or a pass that the first mesh lists of their tests did not reach, each with what it is there
for.  Shared by test_fft_meshes_host.py (every claim of a row, by arithmetic alone), test_powerspec_reference.py (numpy as the
reference at these meshes), test_gpu_powerspec.py and test_gpu_smoothing.py.

The module restates two rules of fft_device.hpp in plain Python; it does not call the library.

* The plan (ps_plan): the radices 4, 2, 3, 5, 7 in that order, each as often as it divides, then the odd numbers from 11 upward in
  the same way (only primes ever divide what is left).  4, 2, 3, 5 and 7 have butterflies in registers (stage_fixed), any other
  radix goes through stage_generic.  A stage whose radices before it multiply to s uses the twiddle tw[base k] with
  base = idx - idx mod s, idx < N / p: in the LAST stage s = N / p and base is 0 throughout, so a generic stage multiplies by a
  twiddle other than 1 only where another stage follows it.
* The tile (ps_tile): T lines per workgroup, the largest of 16, 8 whose LDS request -- the N roots and two buffers of T lines with
  the odd pitch N | 1, complex doubles -- is at most 72 KiB, else 4.

A row's `tails` are ((N/2 + 1) mod T, N (N/2 + 1) mod T, N^2 mod T): the width of the last tile of the pass along j (per plane), of
the pass along i, and the lines of the last workgroup of the row passes (ps_row_kernel, sm_c2r_kernel).  0: no tail.
"""
import collections

LDS_LIMIT = 72 * 1024
FIXED_RADICES = (4, 2, 3, 5, 7)
PS_THREADS = 256                    # the work items of a workgroup of every transform kernel
PS_SUM_THREADS = 512 * PS_THREADS   # the fixed grid of the mean-density sum and of the second statistics pass


def plan(N):
    """the radices of ps_plan(N), in order"""
    out, n = [], int(N)
    for p in FIXED_RADICES:
        while n > 1 and n % p == 0:
            out.append(p)
            n //= p
    p = 11
    while n > 1:
        while n > 1 and n % p == 0:
            out.append(p)
            n //= p
        p += 2
    return tuple(out)


def lds_bytes(N, T):
    """the dynamic LDS of a transform kernel at T lines per workgroup: roots [N], two buffers [T (N | 1)], 16 bytes each"""
    return (2 * T * (N | 1) + N) * 16


def tile(N):
    """ps_tile(N)"""
    for T in (16, 8):
        if lds_bytes(N, T) <= LDS_LIMIT:
            return T
    return 4


def filter_lds_bytes(N, T):
    """the filter pass's request: behind the transform's, three tables of N doubles and three ints per column of the tile"""
    return lds_bytes(N, T) + 3 * N * 8 + 3 * T * 4


def tails(N, T):
    NZ = N // 2 + 1
    return (NZ % T, N * NZ % T, N * N % T)


def generic_stages(N):
    return [p for p in plan(N) if p not in FIXED_RADICES]


def largest_root_read(N):
    """the largest index of the table of roots tw[0 ... N - 1] that line_fft reads at mesh N: a stage of radix p behind radices of
    product s reads tw[base k], base = idx - idx mod s, idx < N / p, k < p, and a generic stage also tw[m N / p], m < p"""
    s, best = 1, 0
    for p in plan(N):
        L = N // p
        best = max(best, ((L - 1) - (L - 1) % s) * (p - 1))
        if p not in FIXED_RADICES:
            best = max(best, (p - 1) * L)
        s *= p
    return best


#: N -> the plan and the tile the library is to take, the tails, the LDS request where the row states one, and what the row adds
Row = collections.namedtuple("Row", "plan T tails lds why")

ROWS = {
    121: Row((11, 11), 16, (13, 5, 1), None,
             "the generic stage twice, the first with twiddles other than 1; NZ = 61; tails in all three passes at T = 16; 121^3 "
             "cells are 13.5 trips of the fixed grids, 916 row workgroups four trips of the one-workgroup fold"),
    139: Row((139,), 16, (6, 2, 9), 73392,
             "the largest mesh with T = 16: 336 bytes below the limit; prime; tails in all three passes"),
    140: Row((4, 5, 7), 8, (7, 4, 0), 38336,
             "the smallest mesh with T = 8; NZ = 71: a second trip of the binning's n_z loop with 7 lanes"),
    169: Row((13, 13), 8, (5, 5, 1), None,
             "the generic stage twice at T = 8; NZ = 85: two trips of the binning's n_z loop, 21 lanes in the second; tails in all "
             "three passes; 36.8 trips of the mean-density sum"),
    243: Row((3, 3, 3, 3, 3), 8, (2, 6, 1), None,
             "five stages: an odd count, so the result ends in the other LDS buffer; tails in all three passes"),
    256: Row((4, 4, 4, 4), 8, (1, 0, 0), None,
             "the mesh of the published timings; NZ = 129: a third trip of the binning's n_z loop with one lane"),
    271: Row((271,), 8, (0, 0, 1), 73712,
             "the largest mesh with T = 8: 16 bytes below the limit; a prime beyond the 256 work items of a workgroup, so the load of "
             "the roots and the one-work-item-per-output loop of a single line make a second trip"),
    272: Row((4, 4, 17), 4, (1, 0, 0), 39296,
             "the smallest mesh with T = 4; its last stage, of radix 17, reads the root at index 256: beside 271 the one tested mesh "
             "whose plan reads a root that the second trip of the load brought in"),
    273: Row((3, 7, 13), 4, (1, 1, 1), None,
             "T = 4 with tails in all three passes (NZ = 137); odd; uneven trips of the mean-density sum"),
}
MESHES = tuple(ROWS)
#: the pairs that straddle the tile rule
TILE_EDGES = ((139, 140), (271, 272))
#: from here on a GPU case keeps to the `default` and `all` bin sets: numpy's transform and the reference's binning take seconds
FEW_BIN_SETS_FROM = 243
