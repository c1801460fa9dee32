"""What the analyses of a field share on the host (bubbles, regions, topology, granulometry; powerspec and smoothing in part): one
checker per common argument, each raising the one message of that argument with the entry's name in front, and :func:`analyse`,
the front end of the four analyses of a thresholded field.  A ``*_spec`` function calls the checkers in the order in which it
reports: of two bad arguments the first one checked is the one named.
"""
import math

import numpy as np

from . import _capi, _residency

PHASES = {"ionised": 0, "neutral": 1}
# why a mesh may have REGION_MAX_N cells a side at the most: the two reasons of check_mesh
MESH_LABELS = "8 bytes per cell on the device: 2 GiB there"
MESH_TRANSFORM = "a line of the transform must fit the device's local memory"


def is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def is_real(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def check_threshold(who, threshold):
    if not is_real(threshold) or not math.isfinite(threshold):
        raise ValueError(f"{who}: threshold must be a finite number, not {threshold!r}")


def check_phase(who, phase):
    if phase not in PHASES:
        raise ValueError(f"{who}: phase must be 'ionised' or 'neutral', not {phase!r}")


def check_connectivity(who, connectivity):
    if not is_int(connectivity) or connectivity not in (6, 26):
        raise ValueError(f"{who}: connectivity must be 6 (faces) or 26 (faces, edges and corners), not {connectivity!r}")


def check_flag(who, name, v):
    """A keyword that is a bool and nothing else: ``periodic``, ``labels``, ``distances``, ``return_field``, ..."""
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{who}: {name} must be a bool, not {type(v).__name__}")


def check_dr(who, dr):
    if dr is not None and (not is_real(dr) or not (math.isfinite(dr) and dr > 0)):
        raise ValueError(f"{who}: dr must be None or a finite number > 0, not {dr!r}")


def check_edges(who, edges):
    """Bin edges already made an array: 2 ... BUBBLE_MAX_BINS + 1 of them, finite, > 0 and ascending."""
    if edges.ndim != 1 or not 2 <= edges.size <= _capi.BUBBLE_MAX_BINS + 1:
        raise ValueError(f"{who}: the bin edges must be a 1-D array of 2 ... {_capi.BUBBLE_MAX_BINS + 1} values")
    if not np.all(np.isfinite(edges)) or not edges[0] > 0.0 or not np.all(np.diff(edges) > 0.0):
        raise ValueError(f"{who}: the bin edges must be finite, > 0 and ascending")


def check_scale(who, scale):
    if not is_real(scale) or not math.isfinite(scale):
        raise ValueError(f"{who}: scale must be a finite number, not {scale!r}")


def check_t_gamma(who, t_gamma):
    if not is_real(t_gamma) or not (math.isfinite(t_gamma) and t_gamma >= 0):
        raise ValueError(f"{who}: t_gamma must be a finite number >= 0, not {t_gamma!r}")


def check_mesh(who, N, reason):
    """The mesh limit of the entries that label or transform the grid; `reason` is MESH_LABELS or MESH_TRANSFORM."""
    if not 1 <= N <= _capi.REGION_MAX_N:
        raise ValueError(f"{who}: the mesh must have 1 ... {_capi.REGION_MAX_N} cells a side ({reason}), not {N}")


def host_field(who, name, field):
    """Keyword `name` as a real (N, N, N) array."""
    field = np.asarray(field)
    if field.ndim != 3 or field.shape != (field.shape[0],) * 3 or field.dtype.kind not in "fiu":
        raise ValueError(f"{who}: {name} must be a real (N, N, N) array")
    return field


def grid_selector(who, grid):
    """A ``_capi.GRID_*`` selector of a device grid that holds data (None: the ionised fraction)."""
    grid = _capi.GRID_XH if grid is None else grid
    if not is_int(grid) or not 0 <= grid <= _capi.GRID_CLUMP:
        raise ValueError(f"{who}: grid must be one of the _capi.GRID_* selectors, not {grid!r}")
    return grid


def analyse(who, field, grid, spec, kw, on_device, cuda_is_init, load_asora):
    """The entry `who` of an analysis of a thresholded field: the host array `field` uploaded to the device's ionised-fraction
    grid, or with None the device grid `grid` where it lies.  ``spec(who, N, **kw)`` checks the keywords -- before the library is
    touched, without the mesh size (N = None) where only the device knows it -- and completes them for the mesh;
    ``on_device(lib, grid, spec)`` is the library call.  `cuda_is_init` and `load_asora` are the calling module's own (the
    names under which a test puts a stand-in for the library in that module)."""
    if field is not None:
        if grid is not None:
            raise ValueError(f"{who}: grid selects a device grid and goes with field=None")
        field = host_field(who, "field", field)
        checked = spec(who, field.shape[0], **kw)
    else:
        grid = grid_selector(who, grid)
        spec(who, None, **kw)
    if not cuda_is_init():
        raise RuntimeError("GPU not initialized. Please initialize it by calling device_init(N)")
    lib = load_asora()
    if field is not None:
        _residency.reclaim()              # this call overwrites a device grid a resident C2Ray object may be relying on
        lib.grid_to_device(_capi.GRID_XH, np.asarray(field, dtype=np.float64))
        grid = _capi.GRID_XH
    else:
        if getattr(lib, "_N", None) is None:
            raise RuntimeError(f"{who}: field=None needs a device initialised through device_init (the mesh size)")
        checked = spec(who, int(lib._N), **kw)
    return on_device(lib, grid, checked)
