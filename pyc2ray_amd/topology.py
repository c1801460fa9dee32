"""Topology of the ionised field: Euler characteristic, Minkowski functionals, Betti numbers.

The third morphological description of reionisation next to the sizes of the regions (:mod:`pyc2ray_amd.bubbles`) and their
connectivity (:mod:`pyc2ray_amd.regions`): the genus / Euler characteristic (Gleser et al. 2006; Friedrich et al. 2011), the
Minkowski functionals (Yoshiura et al. 2017) and the Betti numbers (Giri & Mellema 2021; ``tools21cm.topology`` on the CPU).
:func:`topology` runs it on the device (``libasora.topology``): the grid is thresholded into the bit mask of the other two analyses,
the lattice elements of the mask -- cells, faces, edges, vertices -- are counted from whole mask words, and the mask and its
complement are labelled by the union-find of the regions, so an ionised-fraction grid that lives on the device is analysed where it
lies.  ``C2Ray.topology()`` does that for the current state of a run.  Everything is integers: the same call returns the same bits.
"""
import math

import numpy as np

from . import _capi, _residency
from .asora_core import cuda_is_init
from .load_extensions import load_asora

__all__ = ['Topology', 'topology']

_PHASES = {"ionised": 0, "neutral": 1}
_TALLIES = ("cells", "closed_faces", "closed_edges", "closed_vertices", "open_faces", "open_edges", "open_vertices", "components",
            "complement_components", "cavities")


class Topology:
    """The result of :func:`topology`.  Lengths are in cells; with ``dr`` (the size of a cell in the caller's units) the ``*_phys``
    attributes give the volume times dr^3, the surface times dr^2 and the mean breadth times dr (None without).

    The tallies of the library call.  ``cells``: in-phase cells.  ``closed_faces`` / ``_edges`` / ``_vertices``: the faces, edges and
    vertices of the lattice that touch AT LEAST ONE in-phase cell -- the phase as a union of closed cubes, which is what 26 neighbours
    mean.  ``open_faces`` / ``_edges`` / ``_vertices``: those of which ALL incident cells are in phase -- the union of open cubes, 6
    neighbours.  ``components``: the connected regions of the phase under ``connectivity`` (``n_regions`` of ``region_sizes``);
    ``complement_components``: those of the complement under the dual connectivity (6 <-> 26); ``cavities``: in an open box the
    regions of the complement that touch no face of the box, 0 in a periodic one.

    Derived.  ``euler_26`` = V - E + F - C of the closed counts, ``euler_6`` = C - F + E - V of the open ones, ``euler`` the one that
    goes with ``connectivity``.  The Minkowski functionals of the closed complex (Michielsen & De Raedt 2001): ``volume`` = C,
    ``surface`` = 2 F - 6 C, ``mean_breadth`` = (3 C - 2 F + E) / 2 and ``euler_26``; ``minkowski`` is the four of them.

    ``betti``: (b0, b1, b2) = components, tunnels, cavities.  In an OPEN box b0 = ``components``, b2 = ``cavities`` and b1 = b0 + b2 -
    ``euler``: Alexander duality in R^3 -- a cavity of the phase is a bounded component of its complement.  In a PERIODIC box that
    duality does not hold: the box is a 3-torus, whose own cycles a phase can carry without any complement component to show for
    them (a box that is all ionised but for one island has b2 = 3, not 1: the three coordinate 2-tori of the box, while the island's
    own surface bounds the phase and counts for nothing), so ``betti`` is None there and the object gives what is exact: b0 = ``components``, ``euler``,
    ``complement_components`` and ``tunnels_minus_cavities`` = b1 - b2 = b0 - euler - [the whole box is in phase] (the bracket is b3).
    Periodic meshes of N = 1 and 2 follow the formulas through the wrap -- an element then meets the same cell twice -- and mean
    nothing topologically.  An empty phase gives zeros."""

    def __init__(self, tallies, N, threshold=0.5, phase="ionised", connectivity=6, periodic=True, dr=None):
        t = [int(v) for v in tallies]
        if len(t) != len(_TALLIES):
            raise ValueError(f"Topology: {len(_TALLIES)} tallies, not {len(t)}")
        for name, v in zip(_TALLIES, t):
            setattr(self, name, v)
        self.N = int(N)
        self.threshold, self.phase, self.connectivity, self.periodic = float(threshold), phase, int(connectivity), bool(periodic)
        self.dr = None if dr is None else float(dr)

    @property
    def tallies(self):
        return np.array([getattr(self, name) for name in _TALLIES], dtype=np.uint64)

    @property
    def euler_26(self):
        return self.closed_vertices - self.closed_edges + self.closed_faces - self.cells

    @property
    def euler_6(self):
        return self.cells - self.open_faces + self.open_edges - self.open_vertices

    @property
    def euler(self):
        return self.euler_6 if self.connectivity == 6 else self.euler_26

    @property
    def volume(self):
        return self.cells

    @property
    def surface(self):
        return 2 * self.closed_faces - 6 * self.cells

    @property
    def mean_breadth(self):
        return (3 * self.cells - 2 * self.closed_faces + self.closed_edges) / 2

    @property
    def minkowski(self):
        return (self.volume, self.surface, self.mean_breadth, self.euler_26)

    @property
    def full(self):
        """Is the whole box in phase?"""
        return self.cells == self.N ** 3

    @property
    def tunnels_minus_cavities(self):
        return self.components - self.euler - (1 if self.periodic and self.full else 0)

    @property
    def betti(self):
        if self.periodic:
            return None
        return (self.components, self.components + self.cavities - self.euler, self.cavities)

    def _phys(self, v, power):
        return None if self.dr is None else v * self.dr ** power

    volume_phys = property(lambda self: self._phys(self.volume, 3))
    surface_phys = property(lambda self: self._phys(self.surface, 2))
    mean_breadth_phys = property(lambda self: self._phys(self.mean_breadth, 1))

    def log_line(self):
        """The line of the log file (one per step)."""
        unit = "" if self.dr is None else (f" ({self.volume_phys:.4e}, {self.surface_phys:.4e}, {self.mean_breadth_phys:.4e} in units "
                                           f"of dr^3, dr^2, dr)")
        if self.periodic:
            betti = f"tunnels - cavities {self.tunnels_minus_cavities:n}, {self.complement_components:n} components of the complement"
        else:
            betti = f"Betti numbers {self.betti[0]:n}, {self.betti[1]:n}, {self.betti[2]:n}"
        return (f"Topology ({self.phase}, x {'<' if self.phase == 'neutral' else '>='} {self.threshold:g}, {self.connectivity} neighbours, "
                f"{'periodic' if self.periodic else 'open'}): Euler characteristic {self.euler:n}, {self.components:n} components, {betti}; "
                f"volume {self.volume:n}, surface {self.surface:n}, mean breadth {self.mean_breadth:.1f}{unit}")

    def __repr__(self):
        return f"<Topology: {self.log_line()}>"


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _is_real(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def topology_spec(who, N, threshold=0.5, phase="ionised", connectivity=6, periodic=True, dr=None):
    """The keywords of :func:`topology` checked and completed for a mesh of N cells a side, as a dict (N = None: checked only).
    Raises ValueError -- before any device call -- for what the library would refuse."""
    if not _is_real(threshold) or not math.isfinite(threshold):
        raise ValueError(f"{who}: threshold must be a finite number, not {threshold!r}")
    if phase not in _PHASES:
        raise ValueError(f"{who}: phase must be 'ionised' or 'neutral', not {phase!r}")
    if not _is_int(connectivity) or connectivity not in (6, 26):
        raise ValueError(f"{who}: connectivity must be 6 (faces) or 26 (faces, edges and corners), not {connectivity!r}")
    if not isinstance(periodic, (bool, np.bool_)):
        raise ValueError(f"{who}: periodic must be a bool, not {type(periodic).__name__}")
    if dr is not None and (not _is_real(dr) or not (math.isfinite(dr) and dr > 0)):
        raise ValueError(f"{who}: dr must be None or a finite number > 0, not {dr!r}")
    if N is None:                          # (only the checks: the mesh size is the device's, asked for afterwards)
        return None
    if not 1 <= N <= _capi.REGION_MAX_N:
        raise ValueError(f"{who}: the mesh must have 1 ... {_capi.REGION_MAX_N} cells a side (8 bytes per cell on the device: 2 GiB there), not {N}")
    return dict(N=int(N), threshold=float(threshold), phase=phase, connectivity=int(connectivity), periodic=bool(periodic),
                dr=None if dr is None else float(dr))


def topology(field=None, *, threshold=0.5, phase='ionised', connectivity=6, periodic=True, grid=None, dr=None):
    """The topology of the in-phase cells of a grid, a :class:`Topology`.

    ``field``: an (N, N, N) host array (the ionised fraction, as a rule) for the mesh of ``device_init``; it is uploaded to the
    device's ionised-fraction grid, which a C2Ray object that keeps its grids there is told beforehand.  None: the device grid
    ``grid`` (a ``_capi.GRID_*`` selector, default the ionised fraction) is analysed where it lies, nothing is uploaded.
    ``phase``: 'ionised' -- the cells with x >= ``threshold`` -- or 'neutral', those with x < threshold; a NaN is in neither and so in
    the complement of both.  ``connectivity``: 6 (cells joined across faces) or 26 (across faces, edges and corners), for the
    components and for which Euler characteristic is ``euler``; the complement is joined by the other.  ``periodic``: the lattice
    wraps around the box (True) or ends at its faces, beyond which nothing is in phase (False).  ``dr``: the size of a cell, for the
    ``*_phys`` attributes of the result."""
    who = "topology"
    if field is not None:
        if grid is not None:
            raise ValueError(f"{who}: grid selects a device grid and goes with field=None")
        field = np.asarray(field)
        if field.ndim != 3 or field.shape != (field.shape[0],) * 3 or field.dtype.kind not in "fiu":
            raise ValueError(f"{who}: field must be a real (N, N, N) array")
        N = field.shape[0]
    else:
        grid = _capi.GRID_XH if grid is None else grid
        if not _is_int(grid) or not 0 <= grid <= _capi.GRID_CLUMP:
            raise ValueError(f"{who}: grid must be one of the _capi.GRID_* selectors, not {grid!r}")
        N = None
    kw = dict(threshold=threshold, phase=phase, connectivity=connectivity, periodic=periodic, dr=dr)
    spec = topology_spec(who, N, **kw)
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
        spec = topology_spec(who, int(lib._N), **kw)
    return topology_on_device(lib, grid, spec)


def topology_on_device(lib, grid, spec):
    """The library call for a checked `spec` (topology_spec) on device grid `grid`, as a :class:`Topology`."""
    tallies = lib.topology(grid, spec["threshold"], _PHASES[spec["phase"]], spec["periodic"], spec["connectivity"])
    return Topology(tallies, spec["N"], spec["threshold"], spec["phase"], spec["connectivity"], spec["periodic"], spec["dr"])
