"""Topology of the ionised field: Euler characteristic, Minkowski functionals, Betti numbers.

The third morphological description of reionisation next to the sizes of the regions (:mod:`pyc2ray_amd.bubbles`) and their
connectivity (:mod:`pyc2ray_amd.regions`): the genus / Euler characteristic (Gleser et al. 2006; Friedrich et al. 2011), the
Minkowski functionals (Yoshiura et al. 2017) and the Betti numbers (Giri & Mellema 2021; ``tools21cm.topology`` on the CPU).
:func:`topology` runs it on the device (``libasora.topology``): the grid is thresholded into the bit mask of the other two analyses,
the lattice elements of the mask -- cells, faces, edges, vertices -- are counted from whole mask words, and the mask and its
complement are labelled by the union-find of the regions, so an ionised-fraction grid that lives on the device is analysed where it
lies.  ``C2Ray.topology()`` does that for the current state of a run.  Everything is integers: the same call returns the same bits.
"""
import numpy as np

from .asora_core import cuda_is_init
from .load_extensions import load_asora
from ._fieldspec import MESH_LABELS, PHASES, analyse, check_connectivity, check_dr, check_flag, check_mesh, check_phase, check_threshold

__all__ = ['Topology', 'topology']

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


def topology_spec(who, N, threshold=0.5, phase="ionised", connectivity=6, periodic=True, dr=None):
    """The keywords of :func:`topology` checked and completed for a mesh of N cells a side, as a dict (N = None: checked only).
    Raises ValueError -- before any device call -- for what the library would refuse."""
    check_threshold(who, threshold)
    check_phase(who, phase)
    check_connectivity(who, connectivity)
    check_flag(who, "periodic", periodic)
    check_dr(who, dr)
    if N is None:                          # (only the checks: the mesh size is the device's, asked for afterwards)
        return None
    check_mesh(who, N, MESH_LABELS)
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
    kw = dict(threshold=threshold, phase=phase, connectivity=connectivity, periodic=periodic, dr=dr)
    return analyse("topology", field, grid, topology_spec, kw, topology_on_device, cuda_is_init, load_asora)


def topology_on_device(lib, grid, spec):
    """The library call for a checked `spec` (topology_spec) on device grid `grid`, as a :class:`Topology`."""
    tallies = lib.topology(grid, spec["threshold"], PHASES[spec["phase"]], spec["periodic"], spec["connectivity"])
    return Topology(tallies, spec["N"], spec["threshold"], spec["phase"], spec["connectivity"], spec["periodic"], spec["dr"])
