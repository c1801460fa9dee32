"""TEST INFRASTRUCTURE: one recipe per built form of `raytrace_octant_kernel` ("How every built form meets a
reference").  A recipe makes the real library launch exactly one row of RT_FORMS (csrc/raytrace_plan.hpp; `lib.built_forms()`): the
bench, the radius, the source count, the options and the mode.  tests/test_form_recipes_host.py holds the recipes against the
launcher's own plan without a device; tests/test_gpu_form_recipes.py runs each one, asserts the row that was launched
(`lib.last_launch_form()`, `lib.form_launches()`) and compares the numbers with a reference.

Benches.  Recipes share a mesh, a medium, a short list of sources and references computed once:

  small       N = 64.  R = 20: 21 shells (the 32-entry tables of the paired x 256 row, the 64-entry ones at 64 / 128 threads); R beyond
              the box: 33 shells (64-entry tables at 256 threads paired), and the whole sphere in one workgroup (ASORA_OPT_SECTORS = 6)
              has shells of 23 066 cells, which do not fit LDS
  many_shell  N = 136, R beyond the box: 69 shells, so the 256-entry tables also at 64 and 128 threads; 96 quarter sectors keep the
              shells in LDS (1225 cells), six sectors do not (18 496)
  shells_257  N = 512, one source at (256, 256, 256), R beyond the box: 257 shells, the 1024-entry tables, shells in global memory
  split       N = 520 (the smallest multiple of 8 beyond 512): a buffer descriptor per layout of the rate grid; radii 3, 41, 70 for
              the 32-, 64- and 256-entry tables of the paired rows

The sources of a bench: the first on the corner (0, 0, 0), so that its sphere wraps; the second and third two cells apart (one on
`split`, where R = 3), so that their spheres overlap by more than half; a recipe of ns sources uploads the first ns.  Four sources
sort (the library orders a whole-list call by position) to corner, fourth, second, third: in the paired rows the overlapping two
share a workgroup, and so do the corner source and the fourth.  ASORA_OPT_PAIR_SOURCES = 2 forces two sources per workgroup,
ASORA_OPT_SECTORS and ASORA_OPT_BLOCK_THREADS the decomposition and the workgroup size, so no recipe needs zero-flux fillers, and
ASORA_OPT_ALIGNED_ROWS = 1 keeps the tables packed (line-aligned tables are no template parameter; tests/test_gpu_launch_forms.py
runs them).

Media.  `small` and `many_shell`: the lognormal medium of tests/launch_forms.py.  `shells_257` and `split`: a separable lognormal
n[i,j,k] = n0 exp(a_i + b_j + c_k), x = 1e-4 x 100^(u_i v_j w_k), regenerable from a seed in a second at 1 GiB per grid; nHI > 0
everywhere.  The "dense" variant (modes "zeros", "spectra_zeros") adds what ASORA_OPT_SKIP_ZERO_RATES leaves out: cells a hundred
million times denser, one in 3000 and a plate of 5 x 5 cells in plane i = 1 in front of the corner source (so that even a sphere of
radius 3 holds cells behind it); values are compared where launch_forms.WELL_LIT allows, for the reason documented there.

Modes: "tables" (table rates, every rate added), "zeros" (exact zeros left out, dense medium), "heat", "grey", "dump" / "dump_grey"
(column densities of one source), "spectra" / "spectra_zeros" (two table sets, the overlapping pair on different ones), "open" /
"open_heat".  The tables are launch_forms.tables().

References: the CPU oracle, one trace per source, summed (`reference`); on `shells_257` a whole-box trace takes about 50 s, so
there the reference is the sparse fixture tests/golden/form_257_shells_*.npz, made once by tests/golden/make_form_257_shells_golden.py
from the same oracle (`digest`, `sample_indices`, `axis_lines` are shared with it).

shells / max_cells of a recipe: the shell count and the largest shell of the geometry tables the launch builds, which decide between
LDS and global memory for the shell buffers; the GPU test holds them against the tables of the launch itself.
"""
import collections
import functools
import os

import numpy as np

import cases
import launch_forms as LF
import open_boundary_reference as OB
from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CU_COUNT = 256

Recipe = collections.namedtuple("Recipe", "bench R ns mode sectors threads pair global_atomics shells max_cells")
R = Recipe

#: form (the kernel's 13 template arguments in their order) -> recipe, in the order of RT_FORMS without the sub-box rows
RECIPES = {
    (64,0,0,0,256,0,0,0,1,0,0,1,0): R("many_shell", 1000.0, 1, "tables", 4, 64, 1, 1, 68, 1225),
    (64,0,0,0,256,1,0,0,1,0,0,1,0): R("many_shell", 1000.0, 1, "zeros", 4, 64, 1, 1, 68, 1225),
    (64,0,0,1,256,0,0,0,1,0,0,1,0): R("many_shell", 1000.0, 1, "heat", 4, 64, 1, 1, 68, 1225),
    (64,0,0,0,256,0,1,0,1,0,0,1,0): R("many_shell", 1000.0, 1, "grey", 4, 64, 1, 1, 68, 1225),
    (64,0,0,0,256,0,0,1,1,0,0,1,0): R("many_shell", 1000.0, 1, "tables", 4, 64, 1, 0, 68, 1225),
    (64,0,0,0,256,1,0,1,1,0,0,1,0): R("many_shell", 1000.0, 1, "zeros", 4, 64, 1, 0, 68, 1225),
    (64,0,0,1,256,0,0,1,1,0,0,1,0): R("many_shell", 1000.0, 1, "heat", 4, 64, 1, 0, 68, 1225),
    (64,0,0,0,256,0,1,1,1,0,0,1,0): R("many_shell", 1000.0, 1, "grey", 4, 64, 1, 0, 68, 1225),
    (64,1,0,0,256,0,0,0,1,0,0,1,0): R("many_shell", 1000.0, 1, "tables", 9, 64, 1, 0, 68, 18496),
    (64,1,0,1,256,0,0,0,1,0,0,1,0): R("many_shell", 1000.0, 1, "heat", 9, 64, 1, 0, 68, 18496),
    (64,1,0,0,256,0,1,0,1,0,0,1,0): R("many_shell", 1000.0, 1, "grey", 9, 64, 1, 0, 68, 18496),
    (128,0,0,0,256,0,0,0,1,0,0,1,0): R("many_shell", 1000.0, 1, "tables", 4, 128, 1, 1, 68, 1225),
    (128,0,0,0,256,1,0,0,1,0,0,1,0): R("many_shell", 1000.0, 1, "zeros", 4, 128, 1, 1, 68, 1225),
    (128,0,0,1,256,0,0,0,1,0,0,1,0): R("many_shell", 1000.0, 1, "heat", 4, 128, 1, 1, 68, 1225),
    (128,0,0,0,256,0,1,0,1,0,0,1,0): R("many_shell", 1000.0, 1, "grey", 4, 128, 1, 1, 68, 1225),
    (128,0,0,0,256,0,0,1,1,0,0,1,0): R("many_shell", 1000.0, 1, "tables", 4, 128, 1, 0, 68, 1225),
    (128,0,0,0,256,1,0,1,1,0,0,1,0): R("many_shell", 1000.0, 1, "zeros", 4, 128, 1, 0, 68, 1225),
    (128,0,0,1,256,0,0,1,1,0,0,1,0): R("many_shell", 1000.0, 1, "heat", 4, 128, 1, 0, 68, 1225),
    (128,0,0,0,256,0,1,1,1,0,0,1,0): R("many_shell", 1000.0, 1, "grey", 4, 128, 1, 0, 68, 1225),
    (128,1,0,0,256,0,0,0,1,0,0,1,0): R("many_shell", 1000.0, 1, "tables", 9, 128, 1, 0, 68, 18496),
    (128,1,0,1,256,0,0,0,1,0,0,1,0): R("many_shell", 1000.0, 1, "heat", 9, 128, 1, 0, 68, 18496),
    (128,1,0,0,256,0,1,0,1,0,0,1,0): R("many_shell", 1000.0, 1, "grey", 9, 128, 1, 0, 68, 18496),
    (256,0,0,0,256,0,0,0,1,0,0,1,0): R("small", 20.0, 3, "tables", 3, 256, 1, 1, 20, 344),
    (256,0,0,0,256,1,0,0,1,0,0,1,0): R("small", 20.0, 3, "zeros", 3, 256, 1, 1, 20, 344),
    (256,0,0,1,256,0,0,0,1,0,0,1,0): R("small", 20.0, 3, "heat", 3, 256, 1, 1, 20, 344),
    (256,0,0,0,256,0,1,0,1,0,0,1,0): R("small", 20.0, 3, "grey", 3, 256, 1, 1, 20, 344),
    (256,0,0,0,256,0,0,1,1,0,0,1,0): R("small", 20.0, 3, "tables", 3, 256, 1, 0, 20, 344),
    (256,0,0,0,256,1,0,1,1,0,0,1,0): R("small", 20.0, 3, "zeros", 3, 256, 1, 0, 20, 344),
    (256,0,0,1,256,0,0,1,1,0,0,1,0): R("small", 20.0, 3, "heat", 3, 256, 1, 0, 20, 344),
    (256,0,0,0,256,0,1,1,1,0,0,1,0): R("small", 20.0, 3, "grey", 3, 256, 1, 0, 20, 344),
    (256,1,0,0,256,0,0,0,1,0,0,1,0): R("small", 1000.0, 3, "tables", 6, 256, 1, 0, 32, 23066),
    (256,1,0,1,256,0,0,0,1,0,0,1,0): R("small", 1000.0, 3, "heat", 6, 256, 1, 0, 32, 23066),
    (256,1,0,0,256,0,1,0,1,0,0,1,0): R("small", 1000.0, 3, "grey", 6, 256, 1, 0, 32, 23066),
    (512,0,0,0,256,0,0,0,1,0,0,1,0): R("small", 20.0, 3, "tables", 3, 512, 1, 1, 20, 344),
    (512,0,0,0,256,1,0,0,1,0,0,1,0): R("small", 20.0, 3, "zeros", 3, 512, 1, 1, 20, 344),
    (512,0,0,1,256,0,0,0,1,0,0,1,0): R("small", 20.0, 3, "heat", 3, 512, 1, 1, 20, 344),
    (512,0,0,0,256,0,1,0,1,0,0,1,0): R("small", 20.0, 3, "grey", 3, 512, 1, 1, 20, 344),
    (512,0,0,0,256,0,0,1,1,0,0,1,0): R("small", 20.0, 3, "tables", 3, 512, 1, 0, 20, 344),
    (512,0,0,0,256,1,0,1,1,0,0,1,0): R("small", 20.0, 3, "zeros", 3, 512, 1, 0, 20, 344),
    (512,0,0,1,256,0,0,1,1,0,0,1,0): R("small", 20.0, 3, "heat", 3, 512, 1, 0, 20, 344),
    (512,0,0,0,256,0,1,1,1,0,0,1,0): R("small", 20.0, 3, "grey", 3, 512, 1, 0, 20, 344),
    (512,1,0,0,256,0,0,0,1,0,0,1,0): R("small", 1000.0, 3, "tables", 6, 512, 1, 0, 32, 23066),
    (512,1,0,1,256,0,0,0,1,0,0,1,0): R("small", 1000.0, 3, "heat", 6, 512, 1, 0, 32, 23066),
    (512,1,0,0,256,0,1,0,1,0,0,1,0): R("small", 1000.0, 3, "grey", 6, 512, 1, 0, 32, 23066),
    (1024,0,0,0,256,0,0,0,1,0,0,1,0): R("small", 20.0, 3, "tables", 3, 1024, 1, 1, 20, 344),
    (1024,0,0,0,256,1,0,0,1,0,0,1,0): R("small", 20.0, 3, "zeros", 3, 1024, 1, 1, 20, 344),
    (1024,0,0,1,256,0,0,0,1,0,0,1,0): R("small", 20.0, 3, "heat", 3, 1024, 1, 1, 20, 344),
    (1024,0,0,0,256,0,1,0,1,0,0,1,0): R("small", 20.0, 3, "grey", 3, 1024, 1, 1, 20, 344),
    (1024,0,0,0,256,0,0,1,1,0,0,1,0): R("small", 20.0, 3, "tables", 3, 1024, 1, 0, 20, 344),
    (1024,0,0,0,256,1,0,1,1,0,0,1,0): R("small", 20.0, 3, "zeros", 3, 1024, 1, 0, 20, 344),
    (1024,0,0,1,256,0,0,1,1,0,0,1,0): R("small", 20.0, 3, "heat", 3, 1024, 1, 0, 20, 344),
    (1024,0,0,0,256,0,1,1,1,0,0,1,0): R("small", 20.0, 3, "grey", 3, 1024, 1, 0, 20, 344),
    (1024,1,0,0,256,0,0,0,1,0,0,1,0): R("small", 1000.0, 3, "tables", 6, 1024, 1, 0, 32, 23066),
    (1024,1,0,1,256,0,0,0,1,0,0,1,0): R("small", 1000.0, 3, "heat", 6, 1024, 1, 0, 32, 23066),
    (1024,1,0,0,256,0,1,0,1,0,0,1,0): R("small", 1000.0, 3, "grey", 6, 1024, 1, 0, 32, 23066),
    (64,0,0,0,64,0,0,0,1,0,0,1,0): R("small", 20.0, 3, "tables", 3, 64, 1, 1, 20, 344),
    (64,0,0,0,64,1,0,0,1,0,0,1,0): R("small", 20.0, 3, "zeros", 3, 64, 1, 1, 20, 344),
    (64,0,0,1,64,0,0,0,1,0,0,1,0): R("small", 20.0, 3, "heat", 3, 64, 1, 1, 20, 344),
    (64,0,0,0,64,0,1,0,1,0,0,1,0): R("small", 20.0, 3, "grey", 3, 64, 1, 1, 20, 344),
    (64,0,0,0,64,0,0,1,1,0,0,1,0): R("small", 20.0, 3, "tables", 3, 64, 1, 0, 20, 344),
    (64,0,0,0,64,1,0,1,1,0,0,1,0): R("small", 20.0, 3, "zeros", 3, 64, 1, 0, 20, 344),
    (64,0,0,1,64,0,0,1,1,0,0,1,0): R("small", 20.0, 3, "heat", 3, 64, 1, 0, 20, 344),
    (64,0,0,0,64,0,1,1,1,0,0,1,0): R("small", 20.0, 3, "grey", 3, 64, 1, 0, 20, 344),
    (64,1,0,0,64,0,0,0,1,0,0,1,0): R("small", 1000.0, 3, "tables", 6, 64, 1, 0, 32, 23066),
    (64,1,0,1,64,0,0,0,1,0,0,1,0): R("small", 1000.0, 3, "heat", 6, 64, 1, 0, 32, 23066),
    (64,1,0,0,64,0,1,0,1,0,0,1,0): R("small", 1000.0, 3, "grey", 6, 64, 1, 0, 32, 23066),
    (128,0,0,0,64,0,0,0,1,0,0,1,0): R("small", 20.0, 3, "tables", 3, 128, 1, 1, 20, 344),
    (128,0,0,0,64,1,0,0,1,0,0,1,0): R("small", 20.0, 3, "zeros", 3, 128, 1, 1, 20, 344),
    (128,0,0,1,64,0,0,0,1,0,0,1,0): R("small", 20.0, 3, "heat", 3, 128, 1, 1, 20, 344),
    (128,0,0,0,64,0,1,0,1,0,0,1,0): R("small", 20.0, 3, "grey", 3, 128, 1, 1, 20, 344),
    (128,0,0,0,64,0,0,1,1,0,0,1,0): R("small", 20.0, 3, "tables", 3, 128, 1, 0, 20, 344),
    (128,0,0,0,64,1,0,1,1,0,0,1,0): R("small", 20.0, 3, "zeros", 3, 128, 1, 0, 20, 344),
    (128,0,0,1,64,0,0,1,1,0,0,1,0): R("small", 20.0, 3, "heat", 3, 128, 1, 0, 20, 344),
    (128,0,0,0,64,0,1,1,1,0,0,1,0): R("small", 20.0, 3, "grey", 3, 128, 1, 0, 20, 344),
    (128,1,0,0,64,0,0,0,1,0,0,1,0): R("small", 1000.0, 3, "tables", 6, 128, 1, 0, 32, 23066),
    (128,1,0,1,64,0,0,0,1,0,0,1,0): R("small", 1000.0, 3, "heat", 6, 128, 1, 0, 32, 23066),
    (128,1,0,0,64,0,1,0,1,0,0,1,0): R("small", 1000.0, 3, "grey", 6, 128, 1, 0, 32, 23066),
    (256,1,0,0,1024,0,0,0,1,0,0,1,0): R("shells_257", 1000.0, 1, "tables", 4, 256, 1, 0, 256, 16641),
    (256,1,0,1,1024,0,0,0,1,0,0,1,0): R("shells_257", 1000.0, 1, "heat", 4, 256, 1, 0, 256, 16641),
    (256,1,0,0,1024,0,1,0,1,0,0,1,0): R("shells_257", 1000.0, 1, "grey", 4, 256, 1, 0, 256, 16641),
    (512,1,0,0,1024,0,0,0,1,0,0,1,0): R("shells_257", 1000.0, 1, "tables", 4, 512, 1, 0, 256, 16641),
    (512,1,0,1,1024,0,0,0,1,0,0,1,0): R("shells_257", 1000.0, 1, "heat", 4, 512, 1, 0, 256, 16641),
    (512,1,0,0,1024,0,1,0,1,0,0,1,0): R("shells_257", 1000.0, 1, "grey", 4, 512, 1, 0, 256, 16641),
    (1024,1,0,0,1024,0,0,0,1,0,0,1,0): R("shells_257", 1000.0, 1, "tables", 4, 1024, 1, 0, 256, 16641),
    (1024,1,0,1,1024,0,0,0,1,0,0,1,0): R("shells_257", 1000.0, 1, "heat", 4, 1024, 1, 0, 256, 16641),
    (1024,1,0,0,1024,0,1,0,1,0,0,1,0): R("shells_257", 1000.0, 1, "grey", 4, 1024, 1, 0, 256, 16641),
    (256,0,1,0,256,0,0,0,1,0,0,1,0): R("small", 20.0, 1, "dump", 3, 0, 1, 0, 20, 344),
    (256,0,1,0,256,0,1,0,1,0,0,1,0): R("small", 20.0, 1, "dump_grey", 3, 0, 1, 0, 20, 344),
    (256,1,1,0,256,0,0,0,1,0,0,1,0): R("small", 1000.0, 1, "dump", 6, 0, 1, 0, 32, 23066),
    (256,1,1,0,256,0,1,0,1,0,0,1,0): R("small", 1000.0, 1, "dump_grey", 6, 0, 1, 0, 32, 23066),
    (256,1,1,0,1024,0,0,0,1,0,0,1,0): R("shells_257", 1000.0, 1, "dump", 4, 0, 1, 0, 256, 16641),
    (256,1,1,0,1024,0,1,0,1,0,0,1,0): R("shells_257", 1000.0, 1, "dump_grey", 4, 0, 1, 0, 256, 16641),
    (64,0,0,0,256,0,0,1,2,0,0,1,0): R("many_shell", 1000.0, 4, "tables", 4, 64, 2, 0, 68, 1225),
    (64,0,0,0,256,1,0,1,2,0,0,1,0): R("many_shell", 1000.0, 4, "zeros", 4, 64, 2, 0, 68, 1225),
    (128,0,0,0,256,0,0,1,2,0,0,1,0): R("many_shell", 1000.0, 4, "tables", 4, 128, 2, 0, 68, 1225),
    (128,0,0,0,256,1,0,1,2,0,0,1,0): R("many_shell", 1000.0, 4, "zeros", 4, 128, 2, 0, 68, 1225),
    (256,0,0,0,256,0,0,1,2,0,0,1,0): R("many_shell", 1000.0, 4, "tables", 4, 256, 2, 0, 68, 1225),
    (256,0,0,0,256,1,0,1,2,0,0,1,0): R("many_shell", 1000.0, 4, "zeros", 4, 256, 2, 0, 68, 1225),
    (512,0,0,0,256,0,0,1,2,0,0,1,0): R("small", 20.0, 4, "tables", 3, 512, 2, 0, 20, 344),
    (512,0,0,0,256,1,0,1,2,0,0,1,0): R("small", 20.0, 4, "zeros", 3, 512, 2, 0, 20, 344),
    (64,0,0,0,64,0,0,1,2,0,0,1,0): R("small", 20.0, 4, "tables", 3, 64, 2, 0, 20, 344),
    (64,0,0,0,64,1,0,1,2,0,0,1,0): R("small", 20.0, 4, "zeros", 3, 64, 2, 0, 20, 344),
    (128,0,0,0,64,0,0,1,2,0,0,1,0): R("small", 20.0, 4, "tables", 3, 128, 2, 0, 20, 344),
    (128,0,0,0,64,1,0,1,2,0,0,1,0): R("small", 20.0, 4, "zeros", 3, 128, 2, 0, 20, 344),
    (256,0,0,0,64,0,0,1,2,0,0,1,0): R("small", 1000.0, 4, "tables", 3, 256, 2, 0, 32, 2112),
    (256,0,0,0,64,1,0,1,2,0,0,1,0): R("small", 1000.0, 4, "zeros", 3, 256, 2, 0, 32, 2112),
    (256,0,0,0,32,0,0,1,2,0,0,1,0): R("small", 20.0, 4, "tables", 3, 256, 2, 0, 20, 344),
    (256,0,0,0,32,1,0,1,2,0,0,1,0): R("small", 20.0, 4, "zeros", 3, 256, 2, 0, 20, 344),
    (256,0,0,0,32,0,0,1,2,0,1,0,0): R("split", 3.0, 4, "tables", 3, 256, 2, 0, 3, 13),
    (256,0,0,0,32,0,0,1,2,0,1,1,0): R("split", 3.0, 4, "spectra", 3, 256, 2, 0, 3, 13),
    (256,0,0,0,32,1,0,1,2,0,1,0,0): R("split", 3.0, 4, "zeros", 3, 256, 2, 0, 3, 13),
    (256,0,0,0,32,1,0,1,2,0,1,1,0): R("split", 3.0, 4, "spectra_zeros", 3, 256, 2, 0, 3, 13),
    (256,0,0,0,64,0,0,1,2,0,1,0,0): R("split", 41.0, 4, "tables", 3, 256, 2, 0, 41, 1399),
    (256,0,0,0,64,0,0,1,2,0,1,1,0): R("split", 41.0, 4, "spectra", 3, 256, 2, 0, 41, 1399),
    (256,0,0,0,64,1,0,1,2,0,1,0,0): R("split", 41.0, 4, "zeros", 3, 256, 2, 0, 41, 1399),
    (256,0,0,0,64,1,0,1,2,0,1,1,0): R("split", 41.0, 4, "spectra_zeros", 3, 256, 2, 0, 41, 1399),
    (256,0,0,0,256,0,0,1,2,0,1,0,0): R("split", 70.0, 4, "tables", 3, 256, 2, 0, 70, 4030),
    (256,0,0,0,256,0,0,1,2,0,1,1,0): R("split", 70.0, 4, "spectra", 3, 256, 2, 0, 70, 4030),
    (256,0,0,0,256,1,0,1,2,0,1,0,0): R("split", 70.0, 4, "zeros", 3, 256, 2, 0, 70, 4030),
    (256,0,0,0,256,1,0,1,2,0,1,1,0): R("split", 70.0, 4, "spectra_zeros", 3, 256, 2, 0, 70, 4030),
    (512,0,0,0,256,0,0,1,2,0,1,0,0): R("split", 70.0, 4, "tables", 3, 512, 2, 0, 70, 4030),
    (512,0,0,0,256,0,0,1,2,0,1,1,0): R("split", 70.0, 4, "spectra", 3, 512, 2, 0, 70, 4030),
    (512,0,0,0,256,1,0,1,2,0,1,0,0): R("split", 70.0, 4, "zeros", 3, 512, 2, 0, 70, 4030),
    (512,0,0,0,256,1,0,1,2,0,1,1,0): R("split", 70.0, 4, "spectra_zeros", 3, 512, 2, 0, 70, 4030),
    (256,0,0,0,256,0,0,1,1,0,1,1,0): R("split", 41.0, 3, "tables", 3, 256, 1, 0, 41, 1399),
    (256,0,0,0,256,1,0,1,1,0,1,1,0): R("split", 41.0, 3, "zeros", 3, 256, 1, 0, 41, 1399),
    (256,0,0,1,256,0,0,1,1,0,1,1,0): R("split", 41.0, 3, "heat", 3, 256, 1, 0, 41, 1399),
    (256,0,0,0,256,0,1,1,1,0,1,1,0): R("split", 41.0, 3, "grey", 3, 256, 1, 0, 41, 1399),
    (256,0,0,0,256,0,0,1,2,0,0,1,1): R("small", 20.0, 4, "open", 3, 256, 2, 0, 20, 344),
    (256,0,0,0,256,0,0,1,1,0,0,1,1): R("small", 20.0, 3, "open", 3, 256, 1, 0, 20, 344),
    (256,0,0,1,256,0,0,1,1,0,0,1,1): R("small", 20.0, 3, "open_heat", 3, 256, 1, 0, 20, 344),
    (256,1,0,0,256,0,0,1,1,0,0,1,1): R("small", 1000.0, 3, "open", 6, 256, 1, 0, 32, 23066),
    (256,1,0,1,256,0,0,1,1,0,0,1,1): R("small", 1000.0, 3, "open_heat", 6, 256, 1, 0, 32, 23066),
    (256,1,0,0,1024,0,0,1,1,0,0,1,1): R("shells_257", 1000.0, 1, "open", 4, 256, 1, 0, 256, 16641),
    (256,1,0,1,1024,0,0,1,1,0,0,1,1): R("shells_257", 1000.0, 1, "open_heat", 4, 256, 1, 0, 256, 16641),
    (512,0,0,0,256,0,0,1,1,0,1,1,0): R("split", 41.0, 3, "tables", 3, 512, 1, 0, 41, 1399),
    (512,0,0,0,256,1,0,1,1,0,1,1,0): R("split", 41.0, 3, "zeros", 3, 512, 1, 0, 41, 1399),
    (512,0,0,1,256,0,0,1,1,0,1,1,0): R("split", 41.0, 3, "heat", 3, 512, 1, 0, 41, 1399),
    (512,0,0,0,256,0,1,1,1,0,1,1,0): R("split", 41.0, 3, "grey", 3, 512, 1, 0, 41, 1399),
    (512,0,0,0,256,0,0,1,2,0,0,1,1): R("small", 20.0, 4, "open", 3, 512, 2, 0, 20, 344),
    (512,0,0,0,256,0,0,1,1,0,0,1,1): R("small", 20.0, 3, "open", 3, 512, 1, 0, 20, 344),
    (512,0,0,1,256,0,0,1,1,0,0,1,1): R("small", 20.0, 3, "open_heat", 3, 512, 1, 0, 20, 344),
    (512,1,0,0,256,0,0,1,1,0,0,1,1): R("small", 1000.0, 3, "open", 6, 512, 1, 0, 32, 23066),
    (512,1,0,1,256,0,0,1,1,0,0,1,1): R("small", 1000.0, 3, "open_heat", 6, 512, 1, 0, 32, 23066),
    (512,1,0,0,1024,0,0,1,1,0,0,1,1): R("shells_257", 1000.0, 1, "open", 4, 512, 1, 0, 256, 16641),
    (512,1,0,1,1024,0,0,1,1,0,0,1,1): R("shells_257", 1000.0, 1, "open_heat", 4, 512, 1, 0, 256, 16641),
}

#: the six sub-box forms: form -> (row of tests/subbox_forms.py, heating tables, options of the call).  The call is the f2py-shaped
#: entry, whose last source goes to the on-the-fly kernel of subbox.hip (no row of RT_FORMS); the others sweep on the tables.
SUBBOX_RECIPES = {
    (256,0,0,0,256,0,0,1,1,1,0,1,0): ("sphere_256_r9", False, {}),
    (256,0,0,1,256,0,0,1,1,1,0,1,0): ("sphere_256_r9", True, {}),
    (256,0,0,0,256,0,0,1,2,1,0,1,0): ("halves_256_r22", False, {}),
    (512,0,0,0,256,0,0,1,1,1,0,1,0): ("sphere_512_r18", False, {"OPT_PAIR_SOURCES": 1}),
    (512,0,0,1,256,0,0,1,1,1,0,1,0): ("sphere_512_r18", True, {}),
    (512,0,0,0,256,0,0,1,2,1,0,1,0): ("sphere_512_r18", False, {}),
}


def form_text(form):
    """A form as DESIGN.md and the launcher's messages write it."""
    return "<" + ",".join(str(int(v)) for v in form) + ">"


# ---- what a recipe sets and asks for ------------------------------------------------------------------------------------------
#: the options a recipe may set; a case sets all of them (0 where the recipe says nothing) and puts them back to 0
OPTIONS = ("OPT_SECTORS", "OPT_BLOCK_THREADS", "OPT_PAIR_SOURCES", "OPT_ALIGNED_ROWS", "OPT_GLOBAL_ATOMICS", "OPT_SKIP_ZERO_RATES",
           "OPT_GREY_NOTABLES", "OPT_OPEN_BOUNDARIES", "OPT_HEATING")
MODES = ("tables", "zeros", "heat", "grey", "dump", "dump_grey", "spectra", "spectra_zeros", "open", "open_heat")


def options(rec):
    """{option name: value} of a recipe, every entry of OPTIONS."""
    o = dict.fromkeys(OPTIONS, 0)
    o.update(OPT_SECTORS=rec.sectors, OPT_BLOCK_THREADS=rec.threads, OPT_PAIR_SOURCES=rec.pair, OPT_ALIGNED_ROWS=1,
             OPT_GLOBAL_ATOMICS=rec.global_atomics, OPT_SKIP_ZERO_RATES=1 if rec.mode in ("zeros", "spectra_zeros") else 2,
             OPT_GREY_NOTABLES=int(rec.mode in ("grey", "dump_grey")), OPT_OPEN_BOUNDARIES=int(rec.mode.startswith("open")),
             OPT_HEATING=int(rec.mode in ("heat", "open_heat")))
    return o


def plan_flags(rec):
    """The keywords of lib.launch_plan that describe the call of a recipe."""
    return dict(heat=rec.mode in ("heat", "open_heat"), dump=rec.mode.startswith("dump"), table_sets=rec.mode.startswith("spectra"),
                host_positions=True, radius_stays=True, rate_tables=True)


# ---- benches ------------------------------------------------------------------------------------------------------------------
Bench = collections.namedtuple("Bench", "N dr seed separable pos flux spec")
Bench.__doc__ = """pos: 0-based (i, j, k) of the sources in upload order; flux; spec: table set per source in the two-set modes."""
_FLUX, _SPEC = (3.0, 3.75, 4.5, 5.25), (0, 0, 1, 1)
BENCHES = {
    "small": Bench(64, 2.0 ** 63, 31, False, ((0, 0, 0), (41, 22, 30), (41, 22, 32), (20, 40, 10)), _FLUX, _SPEC),
    "many_shell": Bench(136, 2.0 ** 62, 32, False, ((0, 0, 0), (80, 45, 60), (80, 45, 62), (40, 100, 20)), _FLUX, _SPEC),
    "shells_257": Bench(512, 2.0 ** 60, 33, True, ((256, 256, 256),), _FLUX[:1], _SPEC[:1]),
    "split": Bench(520, 2.0 ** 61, 34, True, ((0, 0, 0), (300, 200, 100), (300, 200, 101), (100, 400, 50)), _FLUX, _SPEC),
}
PLATE_PLANE, PLATE_HALF_WIDTH = 1, 2
DENSE_ONE_IN, DENSE_FACTOR = LF.DENSE_ONE_IN, LF.DENSE_FACTOR


def sources(bench, ns):
    """(pos0 flat int32, flux, spec int32) of the first ns sources of a bench, in upload order."""
    b = BENCHES[bench]
    return (np.array(b.pos[:ns], dtype=np.int32).ravel(), np.array(b.flux[:ns], dtype=np.float64), np.array(b.spec[:ns], dtype=np.int32))


def make_medium(N, seed, separable, dense=False):
    """(ndens, xh) of a bench's mesh; see the module's docstring."""
    if separable:
        rng = np.random.default_rng(seed)
        a, b, c = 0.5 * rng.normal(size=(3, N))
        nd = 1e-3 * np.exp(a[:, None, None] + b[None, :, None] + c[None, None, :] - 0.375)
        u, v, w = rng.uniform(size=(3, N))
        xh = 1e-4 * 100.0 ** (u[:, None, None] * v[None, :, None] * w[None, None, :])
    else:
        nd, xh, _ = cases.grid(N, "lognormal", 100 + seed, 0.05, xlo=1e-4, xhi=1e-2)
    if dense:
        rng = np.random.default_rng(200 + seed)
        where = np.zeros((N, N, N), dtype=bool)
        where.ravel()[rng.integers(0, N ** 3, N ** 3 // DENSE_ONE_IN)] = True
        plate = np.arange(-PLATE_HALF_WIDTH, PLATE_HALF_WIDTH + 1) % N
        where[np.ix_([PLATE_PLANE], plate, plate)] = True
        nd[where] *= DENSE_FACTOR
    return nd, xh


@functools.lru_cache(maxsize=2)
def medium(bench, dense=False):
    b = BENCHES[bench]
    nd, xh = make_medium(b.N, b.seed, b.separable, dense)
    nd.setflags(write=False)
    xh.setflags(write=False)
    return nd, xh


# ---- geometry on the host -----------------------------------------------------------------------------------------------------
def window(N, R, pos, periodic=True):
    """Per axis: the indices of the cells inside the source's window and within floor(R), and their offsets from the source;
    periodic=False: those of them that are reached without leaving the box."""
    m = int(np.floor(R)) if np.isfinite(R) and R < N else N
    d = np.arange(-min(m, N // 2), min(m, N // 2 - 1 + N % 2) + 1)
    out = []
    for ax in range(3):
        x = int(pos[ax]) + d
        keep = np.ones(d.shape, dtype=bool) if periodic else (x >= 0) & (x < N)
        out.append((x[keep] % N, d[keep]))
    return out


def reach_values(grid, R, pos, periodic=True):
    """The values of `grid` on the cells the source at `pos` rates (within R, inside its window), as a flat array."""
    N = grid.shape[0]
    (ix, di), (iy, dj), (iz, dk) = window(N, R, pos, periodic)
    inside = (di[:, None, None] ** 2 + dj[None, :, None] ** 2 + dk[None, None, :] ** 2) <= R * R
    return grid[np.ix_(ix, iy, iz)][inside]


# ---- references ---------------------------------------------------------------------------------------------------------------
def _oracle_one(bench, R, s, nd, xh, tset, grey=False, heat=False, coldens=False):
    b = BENCHES[bench]
    sets, dlog = LF.tables()
    thin, thick, hthin, hthick = sets[tset]
    pos0, flux, _ = sources(bench, len(b.pos))
    kw = dict(heat_thin=hthin, heat_thick=hthick) if heat else {}
    return O.asora_do_all_sources(R, cases.SIG, b.dr, nd, xh, pos0[3 * s:3 * s + 3], flux[s:s + 1], thin, thick, cases.MINLOGTAU, dlog,
                                  NumTau=thin.shape[0] - 1, flags=O.ASORA_MODE | (O.GREY if grey else 0), want_coldens=coldens, **kw)


def _open_one(bench, R, s, nd, xh):
    """One source with open boundaries: the periodic oracle on the mesh of 2 N, cropped and cut to what the source reaches without
    leaving the box (launch_forms.open_trace_by_source, here with heating)."""
    b = BENCHES[bench]
    N, M = b.N, 2 * b.N
    mask = LF.reach(N, R, b.pos[s], periodic=False)
    one = _oracle_one(bench, R, s, OB.embed(nd, M, 0, 1e-2), OB.embed(xh, M, 0, 0.0), 0, heat=True)
    return {k: np.where(mask, OB.crop(one[k], N, 0), 0.0) for k in ("phi_ion", "phi_heat")}


@functools.lru_cache(maxsize=3)
def reference(bench, R, ns, kind):
    """The oracle over the first ns sources of a bench, one trace per source, summed in upload order; read-only.
      "tables"         {"phi_ion", "phi_heat"[, "coldens" of the one source when ns = 1]}: set 0 with its heating tables
      "grey"           {"phi_ion"[, "coldens"]}: grey opacity
      "spectra"        {"phi_ion"}: every source with its own table set
      "dense", "spectra_dense"   {"phi_ion", "zero_pairs"} in the dense medium: zero_pairs = the (source, cell) pairs a source
                       rates with exactly +0 -- what ASORA_OPT_SKIP_ZERO_RATES = 1 leaves out
      "open"           {"phi_ion", "phi_heat"} with open boundaries"""
    b = BENCHES[bench]
    N = b.N
    nd, xh = medium(bench, kind in ("dense", "spectra_dense"))
    out = {"phi_ion": np.zeros((N, N, N))}
    if kind in ("tables", "open"):
        out["phi_heat"] = np.zeros((N, N, N))
    zero_pairs = 0
    for s in range(ns):
        if kind == "open":
            one = _open_one(bench, R, s, nd, xh)
        else:
            one = _oracle_one(bench, R, s, nd, xh, b.spec[s] if kind.startswith("spectra") else 0, grey=kind == "grey",
                              heat=kind == "tables", coldens=ns == 1 and kind in ("tables", "grey"))
        for k in out:
            out[k] += one[k]
        if ns == 1 and kind in ("tables", "grey"):
            out["coldens"] = one["coldens"]
        if kind in ("dense", "spectra_dense"):
            zero_pairs += int((reach_values(one["phi_ion"], R, b.pos[s]) == 0).sum())
    for a in out.values():
        a.setflags(write=False)
    if kind in ("dense", "spectra_dense"):
        out["zero_pairs"] = zero_pairs
    return out


#: mode -> kind of reference (None: the sub-box rows and the fixture have their own)
REFERENCE_KIND = {"tables": "tables", "heat": "tables", "dump": "tables", "zeros": "dense", "grey": "grey", "dump_grey": "grey",
                  "spectra": "spectra", "spectra_zeros": "spectra_dense", "open": "open", "open_heat": "open"}


# ---- the sparse fixture of the 257-shell bench --------------------------------------------------------------------------------
FIXTURE_FIELDS = ("phi_ion", "phi_heat", "coldens", "grey_phi_ion")
NSAMPLE = 30000


def fixture_path(field):
    return os.path.join(GOLDEN, f"form_257_shells_{field}.npz")


def sample_indices(N):
    """Seeded flat C-order cell indices the fixture holds values for."""
    return np.random.default_rng(20261021).choice(N ** 3, size=NSAMPLE, replace=False)


def axis_lines(a, pos):
    """The three lines through the cell `pos`, along i, j and k: (3, N)."""
    i, j, k = (int(x) for x in pos)
    return np.stack([a[:, j, k], a[i, :, k], a[i, j, :]])


def digest(a, pos):
    """What the fixture stores of a field (N a multiple of 16): values at the seeded cells and along the three axis lines through
    the source, the sums over every i-plane and over every 16^3 block (with the plane sums a checksum over all cells), the count of
    non-zero cells and the total."""
    a = np.ascontiguousarray(a)
    N = a.shape[0]
    B = N // 16
    return dict(vals=a.ravel()[sample_indices(N)], lines=axis_lines(a, pos), plane_sums=a.sum(axis=(1, 2)),
                block_sums=a.reshape(B, 16, B, 16, B, 16).sum(axis=(1, 3, 5)).ravel(), nonzero=np.array(int(np.count_nonzero(a))),
                total=np.array(float(a.sum())))


def input_checksums(nd, xh):
    """What pins the seeded inputs of the fixture: sums and extremes of the medium and the sums of the tables."""
    sets, dlog = LF.tables()
    return np.array([nd.sum(), xh.sum(), nd.min(), nd.max(), xh.min(), xh.max(), (nd * (1.0 - xh)).min(), float(dlog)]
                    + [float(t.sum()) for s in sets for t in s])
