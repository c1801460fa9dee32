"""ctypes binding of pyc2ray_amd/lib/libasora_hip.so (the C-ABI declared in include/asora_hip.h).

This is the only place the shared library is opened.  There is no fallback of any kind: when the
library is missing or a call fails, a RuntimeError is raised.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PYC2RAY_AMD_LIBASORA selects another BUILD of the same HIP library (diagnostic variants made by
# `make -C pyc2ray_amd/csrc EXTRA=... OUT=...`, tools/ab_options.sh): never a fallback -- a path that does not exist raises.
LIB_PATH = os.environ.get("PYC2RAY_AMD_LIBASORA") or os.path.join(_HERE, "lib", "libasora_hip.so")

# grid selectors / options / kernels, as in include/asora_hip.h
GRID_NDENS, GRID_XH_AV, GRID_PHI_ION, GRID_TEMP, GRID_XH, GRID_XH_INTERMED, GRID_PHI_HEAT = range(7)
GRID_TEMP_END = 7
GRID_CLUMP = 8
GRID_COUNT = 9
(OPT_FORTRAN_CONSTANTS, OPT_GREY_NOTABLES, OPT_TIMING, OPT_Z_TRANSPOSED, OPT_BLOCK_THREADS, OPT_SECTORS,
 OPT_HEATING, OPT_C2RAY_OWN_FLUX, OPT_NO_UNIFORM_T, OPT_SUBBOX_GLOBAL_SHELLS, OPT_PIPELINED_COPIES,
 OPT_SKIP_ZERO_RATES, OPT_GLOBAL_ATOMICS, OPT_PAIR_SOURCES, OPT_SUBBOX_TABLES, OPT_ALIGNED_ROWS, OPT_GEOMETRY_ON_HOST,
 OPT_PLACEMENT_CANDIDATES, OPT_OPEN_BOUNDARIES) = range(19)
MAX_SPECTRA = 16
KERNEL_RAYTRACE, KERNEL_CHEMISTRY, KERNEL_PREP, KERNEL_FINISH = range(4)
KERNEL_BUBBLE_MASK, KERNEL_BUBBLE_SCAN, KERNEL_BUBBLE_RAYS = 4, 5, 6
VARIANT_PAIRED, VARIANT_ALIGNED, VARIANT_BUFFER_ATOMICS, VARIANT_SPLIT_DESCRIPTORS, VARIANT_SKIP_ZERO, VARIANT_GLOBAL_SHELLS = 1, 2, 4, 8, 16, 32
VARIANT_OPEN_BOUNDARIES = 64
PLAN_HEAT, PLAN_DUMP, PLAN_TABLE_SETS, PLAN_HOST_POSITIONS, PLAN_RADIUS_STAYS, PLAN_RATE_TABLES = 1, 2, 4, 8, 16, 32
PLAN_WORDS = 24
(SBL_VALID, SBL_TABLE_SOURCES, SBL_UNITS, SBL_THREADS, SBL_NSRC, SBL_ALIGNED, SBL_HEAT, SBL_TABLE_LAUNCHES, SBL_FLY_SOURCES,
 SBL_FLY_THREADS, SBL_FLY_LDS_SHELLS, SBL_FLY_HEAT, SBL_FLY_LAUNCHES, SBL_BATCHES) = range(14)
SUBBOX_LAUNCH_WORDS = 16
SUBBOX_PLAN_WORDS = 8
(BUDGET_CELLS, BUDGET_N, BUDGET_X, BUDGET_NX, BUDGET_NX0, BUDGET_DNX, BUDGET_PHOTO, BUDGET_LLS, BUDGET_REC, BUDGET_COL,
 BUDGET_T, BUDGET_NT) = range(12)
BUDGET_COUNT = 12
BUBBLE_ENDED, BUBBLE_CAPPED, BUBBLE_LEFT_BOX = range(3)
BUBBLE_MAX_BINS = 256
(REGION_N_PHASE, REGION_N_REGIONS, REGION_SUM_V2, REGION_V_LARGEST, REGION_LABEL_LARGEST, REGION_EXTENT_I, REGION_EXTENT_J,
 REGION_EXTENT_K, REGION_V_SECOND, REGION_LABEL_SECOND, REGION_UNDERFLOW, REGION_UNDERFLOW_CELLS, REGION_OVERFLOW,
 REGION_OVERFLOW_CELLS) = range(14)
REGION_TALLIES = 14
REGION_MAX_N = 645
REGION_NO_LABEL = 0xFFFFFFFF
(TOPO_CELLS, TOPO_CLOSED_FACES, TOPO_CLOSED_EDGES, TOPO_CLOSED_VERTICES, TOPO_OPEN_FACES, TOPO_OPEN_EDGES, TOPO_OPEN_VERTICES,
 TOPO_COMPONENTS, TOPO_COMPLEMENT_COMPONENTS, TOPO_CAVITIES) = range(10)
TOPO_TALLIES = 10
GRAN_N_PHASE, GRAN_D2_MAX, GRAN_N_UNBOUNDED, GRAN_SUM_D2 = range(4)
GRAN_TALLIES = 4
GRAN_UNBOUNDED = 0xFFFFFFFF
PS_XH, PS_XHI, PS_DENSITY, PS_HI = range(4)
PS_KINDS = 4
PS_STAGES = 5
(SMOOTH_N_FINITE, SMOOTH_N_NONFINITE, SMOOTH_MIN, SMOOTH_MAX, SMOOTH_INPUT_SUM, SMOOTH_INPUT_SUM2, SMOOTH_SUM, SMOOTH_S2, SMOOTH_S3,
 SMOOTH_S4) = range(10)
SMOOTH_STATS = 10
SMOOTH_MAX_BINS = 4096
SMOOTH_STAGES = 8
ANISO_CYLINDRICAL, ANISO_MU = range(2)
ANISO_MODES = 2
ANISO_MAX_BINS = 1024
PSLOS_STAGES = 6
LYA_FLUX, LYA_TAU = range(2)
LYA_MAX_BINS = 1024
LYA_SUM_F, LYA_SUM_F2, LYA_TAU_MIN, LYA_TAU_MAX = range(4)
LYA_STATS = 4
(LYA_NONFINITE, LYA_WINDOW, LYA_CLIPPED, LYA_DEGENERATE, LYA_N_DARK, LYA_N_GAPS, LYA_LONGEST, LYA_FULL_LINES) = range(8)
LYA_COUNTS = 8
LYA_STAGES = 4
BISPEC_MAX_SHELLS = 32
BISPEC_MAX_TRIANGLES = 8192
BISPEC_STAGES = 9
BISPEC_PLAN_WORDS = 8
LC_SLOTS = 4
LC_MAX_SLICES = 1024
LC_STAGES = 4
HALO_MODEL_NONE, HALO_MODEL_FULL, HALO_MODEL_PARTIAL = range(3)
HALO_STAGES = 8
HALO_SUMMARY = 5
(PRIM_LOG2, PRIM_LOOKUP, PRIM_DIV, PRIM_MUL, PRIM_ADD, PRIM_ABSORBER, PRIM_PHOTO, PRIM_HEAT, PRIM_GREY) = range(9)
PRIM_COUNT = 9

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_u64p = C.POINTER(C.c_uint64)

#: every symbol include/asora_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "asora_device_init": (C.c_int, [C.c_int, C.c_int]),
    "asora_device_init_ex": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "asora_device_close": (C.c_int, []),
    "asora_density_to_device": (C.c_int, [_dp, C.c_int]),
    "asora_photo_table_to_device": (C.c_int, [_dp, _dp, C.c_int]),
    "asora_heat_table_to_device": (C.c_int, [_dp, _dp, C.c_int]),
    "asora_source_data_to_device": (C.c_int, [_ip, _dp, C.c_int]),
    "asora_spectra_to_device": (C.c_int, [C.c_int, C.c_int, _dp, _dp, _dp, _dp]),
    "asora_source_spectra_to_device": (C.c_int, [_ip, C.c_int]),
    "asora_num_spectra": (C.c_int, []),
    "asora_debug_sort_sources": (C.c_int, [_ip, _dp, _ip, C.c_int, _ip, _dp, _ip]),
    "asora_do_all_sources": (C.c_int, [C.c_double, _dp, C.c_double, C.c_double, _dp, _dp, _dp, C.c_int, C.c_int,
                                       C.c_double, C.c_double, C.c_int]),
    "c2ray_global_pass": (C.c_int, [C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, C.c_double, C.c_double, C.c_double,
                                    C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "c2ray_do_all_sources": (C.c_int, [_dp, _ip, C.c_int, C.c_int, _dp, C.c_double, C.c_double, _dp, _dp, _dp, _dp,
                                       C.c_float, _dp, _dp, _dp, _dp, C.c_double, C.c_double, C.c_double,
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), _dp]),
    "asora_last_error": (C.c_char_p, []),
    "asora_grid_to_device": (C.c_int, [C.c_int, _dp, C.c_int, C.c_char]),
    "asora_grid_to_host": (C.c_int, [C.c_int, _dp, C.c_int, C.c_char]),
    "asora_grid_copy": (C.c_int, [C.c_int, C.c_int]),
    "asora_grid_scale": (C.c_int, [C.c_int, C.c_double]),
    "asora_device_ptr": (C.c_void_p, [C.c_int]),
    "asora_grid_sum": (C.c_int, [C.c_int, C.POINTER(C.c_double)]),
    "asora_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "asora_host_free": (C.c_int, [C.c_void_p]),
    "asora_raytrace_device": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double,
                                        C.c_double, C.c_int]),
    "asora_raytrace_begin": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int]),
    "asora_raytrace_range": (C.c_int, [C.c_int, C.c_int]),
    "asora_raytrace_begin_planes": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, _ip,
                                              C.c_int]),
    "asora_raytrace_fold": (C.c_int, [C.c_int, C.c_int]),
    "asora_stream": (C.c_void_p, []),
    "asora_subbox_raytrace_device": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_double, C.c_double, C.c_double, C.c_double,
                                               C.c_double, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), _dp]),
    "asora_device_init_auto": (C.c_int, [C.c_int]),
    "asora_chemistry_device": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                         C.POINTER(C.c_int), _dp, _dp]),
    "asora_chemistry_range": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                        C.c_int, C.c_int, C.c_int]),
    "asora_chemistry_finish": (C.c_int, [C.POINTER(C.c_int), _dp, _dp]),
    "asora_reduction_ptr": (C.c_void_p, []),
    "asora_evolve_begin": (C.c_int, [C.c_double] * 11 + [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]),
    "asora_evolve_enqueue": (C.c_int, [C.c_int]),
    "asora_evolve_poll": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), _dp, C.c_int, C.POINTER(C.c_int)]),
    "asora_evolve_begin_slab": (C.c_int, [C.c_double] * 11 + [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int]),
    "asora_evolve_begin_slab_thermal": (C.c_int, [C.c_double] * 11 + [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int]),
    "asora_evolve_slab_trace": (C.c_int, [C.c_int, C.c_int]),
    "asora_evolve_slab_fold_out": (C.c_int, [C.c_int, C.c_int]),
    "asora_evolve_slab_outbox": (C.c_void_p, []),
    "asora_evolve_slab_outbox_to_host": (C.c_int, [C.c_int, C.c_int, _dp]),
    "asora_evolve_slab_outbox_from_host": (C.c_int, [C.c_int, C.c_int, _dp]),
    "asora_evolve_slab_fold_all": (C.c_int, []),
    "asora_debug_placement": (None, [C.POINTER(C.c_int), _dp, _dp]),
    "asora_debug_init_cost": (None, [_dp, _dp]),
    "asora_debug_live_buffers": (C.c_int, [C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_ulonglong)]),
    "asora_evolve_slab_add": (C.c_int, [C.c_int, C.c_int, C.c_void_p]),
    "asora_evolve_slab_add_host": (C.c_int, [C.c_int, C.c_int, _dp]),
    "asora_evolve_slab_heat_outbox": (C.c_void_p, []),
    "asora_evolve_slab_heat_outbox_to_host": (C.c_int, [C.c_int, C.c_int, _dp]),
    "asora_evolve_slab_heat_outbox_from_host": (C.c_int, [C.c_int, C.c_int, _dp]),
    "asora_evolve_slab_add_heat": (C.c_int, [C.c_int, C.c_int, C.c_void_p]),
    "asora_evolve_slab_add_heat_host": (C.c_int, [C.c_int, C.c_int, _dp]),
    "asora_evolve_slab_pass": (C.c_int, []),
    "asora_evolve_slab_nhi": (C.c_int, [C.c_int, C.c_int]),
    "asora_evolve_slab_close": (C.c_int, [_dp]),
    "asora_planes_to_host": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp]),
    "asora_planes_to_device": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp]),
    "asora_thermal_params": (C.c_int, [C.c_int, C.c_double, C.c_double, C.c_int, C.c_uint, C.c_int, C.c_double]),
    "asora_thermal_stats": (C.c_int, [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "asora_clumping": (C.c_int, [C.c_int, C.c_double]),
    "asora_lls_opacity": (C.c_int, [C.c_double, C.c_double]),
    "asora_get_lls_opacity": (C.c_int, [_dp, _dp]),
    "asora_plane_flux": (C.c_int, [C.c_int, _ip, _dp, _ip]),
    "asora_get_plane_flux": (C.c_int, [C.POINTER(C.c_int), _ip, _dp, _ip]),
    "asora_step_budget": (C.c_int, [C.c_double] * 5 + [C.c_int, C.c_int, C.c_int, _dp]),
    "asora_bubble_mfp": (C.c_int, [C.c_int, C.c_double, C.c_int, C.c_int, C.c_ulonglong, C.c_longlong, C.c_double, C.c_int, _dp,
                                   _u64p, _u64p, _dp, _ip, _dp, _dp, _ip]),
    "asora_bubble_mask": (C.c_int, [C.c_int, C.c_double, C.c_int, _u64p, C.POINTER(C.c_uint32)]),
    "asora_region_sizes": (C.c_int, [C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _u64p, _u64p, _u64p,
                                     C.POINTER(C.c_uint32)]),
    "asora_topology": (C.c_int, [C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, _u64p]),
    "asora_granulometry": (C.c_int, [C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, _dp, _u64p, _u64p, _u64p, C.POINTER(C.c_uint32)]),
    "asora_power_spectrum": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_uint32), _u64p, _dp, _dp, _dp, _dp,
                                       _dp, _dp, _dp, _dp]),
    "asora_debug_power_spectrum_ms": (C.c_int, [_dp]),
    "asora_smooth_field": (C.c_int, [C.c_int, C.c_double, C.c_double, _dp, _dp, _dp, _dp, C.c_uint, C.c_int, C.c_int, _dp, C.c_int, _dp, _u64p,
                                     _dp]),
    "asora_debug_smooth_field_ms": (C.c_int, [_dp]),
    "asora_power_spectrum_los": (C.c_int, [C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
                                           C.POINTER(C.c_uint32), C.c_int, _dp, _u64p, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "asora_redshift_space_field": (C.c_int, [C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int, _dp, _dp]),
    "asora_los_velocity_to_device": (C.c_int, [_dp, C.c_int, C.c_char, _dp]),
    "asora_los_velocity_clear": (C.c_int, []),
    "asora_debug_power_spectrum_los_ms": (C.c_int, [_dp]),
    "asora_lyman_alpha_forest": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int, _dp, C.c_int,
                                           C.c_int, _dp, _u64p, _u64p, _u64p, _dp, _dp]),
    "asora_debug_lya_forest_ms": (C.c_int, [_dp]),
    "asora_debug_lya_forest_tiles": (C.c_int, [C.c_int, C.c_int, _ip]),
    "asora_bispectrum": (C.c_int, [C.c_int, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_uint32), C.c_int, _ip, _dp, _dp, _u64p, _dp, _dp,
                                   _dp]),
    "asora_debug_bispectrum_ms": (C.c_int, [_dp]),
    "asora_debug_bispectrum_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, _ip]),
    "asora_lightcone_advance": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _ip, _dp, _dp, C.c_int, _dp, _dp]),
    "asora_lightcone_state": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "asora_lightcone_reset": (C.c_int, [C.c_int]),
    "asora_debug_lightcone_ms": (C.c_int, [_dp]),
    "asora_halo_catalogue_to_device": (C.c_int, [_dp, _dp, _dp, C.c_longlong, C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_longlong)]),
    "asora_halo_catalogue_clear": (C.c_int, []),
    "asora_halo_catalogue_state": (C.c_int, [C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "asora_halo_table_to_host": (C.c_int, [C.POINTER(C.c_int64), _u64p, _u64p, C.c_longlong]),
    "asora_halo_sources_build": (C.c_int, [C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double,
                                           C.POINTER(C.c_ulonglong), C.POINTER(C.c_longlong)]),
    "asora_halo_sources_to_host": (C.c_int, [_ip, _dp, C.c_longlong]),
    "asora_debug_halo_sources_ms": (C.c_int, [_dp]),
    "asora_set_option": (C.c_int, [C.c_int, C.c_int]),
    "asora_get_option": (C.c_int, [C.c_int]),
    "asora_kernel_time_ms": (C.c_int, [C.c_int, _dp, C.POINTER(C.c_long)]),
    "asora_kernel_time_reset": (C.c_int, []),
    "asora_synchronize": (C.c_int, []),
    "asora_last_raytrace_counts": (C.c_int, [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "asora_last_raytrace_counts_ex": (C.c_int, [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "asora_debug_coldens": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_int, _dp, C.c_int]),
    "asora_debug_rate_primitives": (C.c_int, [C.c_int, C.c_size_t, _dp, _dp, _dp, _dp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                              C.c_int, _dp, _dp]),
    "asora_last_raytrace_variant": (C.c_int, []),
    "asora_debug_launch_plan": (C.c_int, [C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip]),
    "asora_debug_last_subbox_launch": (C.c_int, [_ip]),
    "asora_debug_built_forms": (C.c_int, [_ip, C.c_int, C.POINTER(C.c_int)]),
    "asora_debug_form_launches": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int, C.POINTER(C.c_int)]),
    "asora_debug_form_launches_reset": (C.c_int, []),
    "asora_debug_last_launch_form": (C.c_int, [_ip, C.POINTER(C.c_int)]),
    "asora_debug_subbox_plan": (C.c_int, [C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip]),
    "asora_debug_block_order": (C.c_int, [_ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.c_size_t, C.POINTER(C.c_int)]),
    "asora_debug_geometry_bytes": (C.c_size_t, []),
    "asora_debug_geometry_table": (C.c_int, [C.c_int, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int),
                                             C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "asora_build_id": (C.c_char_p, []),
    "asora_build_flags": (C.c_char_p, []),
}

_lib = None


def load():
    """Open libasora_hip.so once.  Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"pyc2ray_amd: HIP library not found at {LIB_PATH}. Build it with "
            "`make -C pyc2ray_amd/csrc` (or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "There is no CPU fallback.")
    # One HIP runtime per process.  torch bundles its own libamdhip64 (same SONAME as /opt/rocm's);
    # if torch were imported AFTER this library had pulled in /opt/rocm's copy, the process would
    # hold two runtimes and a device pointer of one would be unknown to the other (RCCL through
    # torch.distributed on our phi_ion grid).  Importing torch first makes both resolve to one copy.
    # PYC2RAY_AMD_NO_TORCH=1 skips this for torch-free single-GPU use.
    if os.environ.get("PYC2RAY_AMD_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:  # pragma: no cover
            pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the header and the build disagree
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().asora_last_error()
        raise RuntimeError(f"{what} failed (code {rc}): {msg.decode() if msg else 'unknown error'}")


def dptr(a):
    return a.ctypes.data_as(_dp)


def iptr(a):
    return a.ctypes.data_as(_ip)
