"""Plane-parallel ionising flux through faces of the box: radiation that enters from outside.

A :class:`PlaneFlux` names the face the radiation ENTERS through and its photon flux.  Each of the N^2 rays of a face is marched
over all N cells along the axis -- never wrapping, whatever ``periodic=`` says, and without the point sources' cut at
``R_max_LLS`` -- and deposits the rates of the point-source trace with the cell size for the path.  ``evolve3D``,
``evolve3D_MPI``, ``evolve3D_resident`` and ``do_raytracing`` take one, or a sequence of them, as ``plane_flux=``.
"""
import contextlib
import math

import numpy as np

from . import _capi
from .utils import printlog

__all__ = ['PlaneFlux', 'FACES']

#: the names of the faces, in the numbering of the C-ABI (include/asora_hip.h, asora_plane_flux); x is the first index of the
#: (N, N, N) C-ordered grids, and "-x" is the plane i = 0, through which the radiation travels towards increasing i
FACES = ("-x", "+x", "-y", "+y", "-z", "+z")


class PlaneFlux:
    """``face``: one of :data:`FACES` (or its number 0 ... 5), the face the radiation enters through; ``flux``: in the units of
    ``src_flux`` per cm^2, i.e. 1e48 photons s^-1 cm^-2, finite and >= 0; ``spectrum``: the table set on the device the face
    shines with (``spectra_to_device``; 0: the one set of ``photo_table_to_device``).  Anything else raises ValueError."""

    def __init__(self, face, flux, spectrum=0):
        if isinstance(face, str):
            if face not in FACES:
                raise ValueError(f"PlaneFlux: face must be one of {', '.join(FACES)}, not {face!r}")
            face = FACES.index(face)
        if isinstance(face, (bool, np.bool_)) or not isinstance(face, (int, np.integer)) or not 0 <= int(face) <= 5:
            raise ValueError(f"PlaneFlux: face must be one of {', '.join(FACES)} or 0 ... 5, not {face!r}")
        if isinstance(flux, (bool, np.bool_)) or not isinstance(flux, (int, float, np.integer, np.floating)):
            raise ValueError(f"PlaneFlux: flux must be a finite number >= 0, not {type(flux).__name__}")
        if not (math.isfinite(float(flux)) and float(flux) >= 0.0):
            raise ValueError(f"PlaneFlux: flux must be finite and >= 0, not {flux!r}")
        if (isinstance(spectrum, (bool, np.bool_)) or not isinstance(spectrum, (int, np.integer))
                or not 0 <= int(spectrum) < _capi.MAX_SPECTRA):
            raise ValueError(f"PlaneFlux: spectrum must be an integer in [0, {_capi.MAX_SPECTRA}), not {spectrum!r}")
        self.face, self.flux, self.spectrum = int(face), float(flux), int(spectrum)

    @property
    def name(self):
        return FACES[self.face]

    def __eq__(self, other):
        return isinstance(other, PlaneFlux) and (self.face, self.flux, self.spectrum) == (other.face, other.flux, other.spectrum)

    def __hash__(self):
        return hash((self.face, self.flux, self.spectrum))

    def __repr__(self):
        return f"PlaneFlux({self.name!r}, {self.flux!r}, spectrum={self.spectrum!r})"


def plane_flux_spec(value, who, use_gpu=True, num_spectra=None):
    """``plane_flux=`` of an entry point -> a tuple of validated :class:`PlaneFlux` (empty: off -- None or an empty sequence).
    Raises ValueError, before any GPU work, for what the library would refuse: anything but PlaneFlux objects, a face given
    twice, faces with ``use_gpu=False`` (the sub-box sweep has none), and -- when `num_spectra`, a callable, is given -- a
    spectrum the device holds no table set for."""
    if value is None:
        return ()
    faces = (value,) if isinstance(value, PlaneFlux) else value
    if isinstance(faces, (str, bytes)) or not hasattr(faces, "__iter__"):
        raise ValueError(f"{who}: plane_flux must be None, a pyc2ray_amd.planeflux.PlaneFlux or a sequence of them, "
                         f"not {type(value).__name__}")
    faces = tuple(faces)
    for f in faces:
        if not isinstance(f, PlaneFlux):
            raise ValueError(f"{who}: plane_flux must hold pyc2ray_amd.planeflux.PlaneFlux objects, not {type(f).__name__}")
    faces = tuple(PlaneFlux(f.face, f.flux, f.spectrum) for f in faces)     # (attributes assigned after construction are checked as well)
    if len({f.face for f in faces}) != len(faces):
        raise ValueError(f"{who}: plane_flux names a face twice (at most one flux per face)")
    if not faces:
        return ()
    if not use_gpu:
        raise ValueError(f"{who}: plane_flux needs use_gpu=True (the use_gpu=False raytracer, the sub-box sweep of the reference's "
                         "Fortran, has no plane-parallel flux)")
    if num_spectra is not None and any(f.spectrum for f in faces):
        held = int(num_spectra())
        for f in faces:
            if f.spectrum >= held:
                raise ValueError(f"{who}: the {f.name} face has spectrum {f.spectrum}, but the device holds {held} table set(s) "
                                 "(spectra_to_device)")
    return faces


def apply_plane_flux(libasora, faces):
    """Set the library's state (an empty tuple: off)."""
    libasora.plane_flux([f.face for f in faces], [f.flux for f in faces], [f.spectrum for f in faces])


def log_plane_flux(faces, logfile, quiet):
    for f in faces:
        printlog(f"Plane-parallel flux through the {f.name} face: {f.flux:.3e} x 1e48 photons/s/cm^2, spectrum {f.spectrum:n}",
                 logfile, quiet)


def source_arrays(src_flux, src_pos, faces):
    """``src_flux``, ``src_pos`` of an entry point; an empty source list -- of any shape, or None -- is accepted when faces are
    given, and becomes arrays of shape (0,) and (3, 0).  Without faces the arguments come back as they are."""
    n = 0 if src_flux is None else int(np.size(src_flux))
    if n == 0 and faces:
        return np.zeros(0, dtype=np.float64), np.zeros((3, 0), dtype=np.int64)
    return src_flux, src_pos


@contextlib.contextmanager
def plane_flux_reset(faces, load):
    """Run the block with the faces set in the library and leave it without any afterwards, whatever happens (nothing at all
    when `faces` is empty); `load` returns the library.  Across ranks the faces belong to rank 0: the other ranks pass ()."""
    if not faces:
        yield
        return
    try:
        apply_plane_flux(load(), faces)
        yield
    finally:
        load().plane_flux((), (), ())
