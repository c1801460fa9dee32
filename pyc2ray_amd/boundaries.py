"""Open (non-periodic) box boundaries of the raytrace: the ``periodic=`` keyword of the entry points.

By default every trace wraps around the box, as the reference's CUDA library built with ``-D PERIODIC`` does.  With
``periodic=False`` a cell whose unwrapped position lies outside the box receives nothing from that source (the reference's
build without ``PERIODIC``; ``periodic_bc`` of C2-Ray proper).  The library holds the choice as option
``ASORA_OPT_OPEN_BOUNDARIES``; the entry points set it for the duration of their work only."""
import contextlib

import numpy as np

from . import _capi

__all__ = ["periodic_spec", "open_boundaries"]


def periodic_spec(periodic, who, use_gpu=True):
    """``periodic=`` of an entry point -> the bool.  Raises ValueError, before any GPU work, for anything but a bool and for
    ``periodic=False`` with ``use_gpu=False``."""
    if not isinstance(periodic, (bool, np.bool_)):
        raise ValueError(f"{who}: periodic must be True or False, not {type(periodic).__name__}")
    periodic = bool(periodic)
    if not periodic and not use_gpu:
        raise ValueError(f"{who}: periodic=False needs use_gpu=True (the use_gpu=False raytracer, the sub-box sweep of the "
                         "reference's Fortran, has no open-boundary mode)")
    return periodic


@contextlib.contextmanager
def open_boundaries(periodic, load):
    """Run the block with open boundaries when `periodic` is False and leave the library periodic afterwards, whatever happens
    (nothing at all when `periodic` is True: the library's own setting stands); `load` returns the library."""
    if periodic:
        yield
        return
    load().set_option(_capi.OPT_OPEN_BOUNDARIES, 1)
    try:
        yield
    finally:
        load().set_option(_capi.OPT_OPEN_BOUNDARIES, 0)
