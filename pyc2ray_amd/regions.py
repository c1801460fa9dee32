"""Connected ionised regions: their volumes and percolation.

The friends-of-friends view of the morphology of reionisation (Iliev et al. 2006; Friedrich et al. 2011; Furlanetto & Oh 2016; Giri
et al. 2018; ``tools21cm.fof`` on the CPU), the companion of the mean-free-path sizes of :mod:`pyc2ray_amd.bubbles`: which ionised
cells are connected to which, how many separate regions there are, how the volume is shared among them and whether one of them spans
the box.  :func:`region_sizes` runs it on the device (``libasora.region_sizes``): the grid is thresholded into the same bit mask as
for the mean-free-path method and the mask is labelled there by a lock-free union-find, so an ionised-fraction grid that lives on
the device is analysed where it lies.  ``C2Ray.regions()`` does that for the current state of a run.  Everything is integers: the
same call returns the same bits.
"""
import math

import numpy as np

from .asora_core import cuda_is_init
from .load_extensions import load_asora
from ._fieldspec import (MESH_LABELS, PHASES, analyse, check_connectivity, check_dr, check_edges, check_flag, check_mesh, check_phase,
                         check_threshold, is_int)

__all__ = ['RegionSizes', 'region_sizes']

_TALLIES = ("n_phase", "n_regions", "sum_v2", "v_largest", "label_largest", "extent_i", "extent_j", "extent_k", "v_second",
            "label_second", "underflow", "underflow_cells", "overflow", "overflow_cells")


class RegionSizes:
    """The result of :func:`region_sizes`.  Volumes are in cells; with ``dr`` (the size of a cell in the caller's units) the
    ``*_phys`` attributes give volumes times dr^3 and radii times dr (None without).

    ``edges`` (nb + 1), ``counts`` and ``cells`` (nb, uint64): the regions with edges[b] <= V < edges[b + 1], and the cells they hold;
    ``underflow`` / ``overflow`` (+ ``_cells``): the regions below ``edges[0]`` / at or beyond ``edges[-1]``, in no bin.
    ``n_phase``: in-phase cells; ``n_regions``; ``sum_v2`` = sum V^2; ``v_largest``, ``label_largest`` (the smallest C-order index of
    its cells; ties in V go to the smaller label), ``largest_index`` = that cell as (i, j, k) or None, ``extent`` = how many of the N
    planes along each axis hold a cell of the largest region; ``v_second``, ``label_second``: the same among the others (0 and
    0xFFFFFFFF when there is none).
    ``percolates``: the largest region has a cell in every plane along some axis; ``fraction_largest`` = v_largest / n_phase;
    ``mean_volume`` = n_phase / n_regions; ``weighted_mean_volume`` = sum_v2 / n_phase (the volume of the region a random in-phase
    cell lies in); ``volume_fraction`` = cells / n_phase per bin; ``radius_edges`` = (3 V / 4 pi)^(1/3) of the edges.  An empty phase
    gives zeros, not divisions by zero.  ``labels``: the (N, N, N) uint32 label grid where it was asked for, else None."""

    def __init__(self, edges, counts, cells, tallies, N, threshold=0.5, phase="ionised", connectivity=6, periodic=True, dr=None,
                 labels=None):
        self.edges = np.array(edges, dtype=np.float64)
        self.counts = np.array(counts, dtype=np.uint64)
        self.cells = np.array(cells, dtype=np.uint64)
        if self.edges.ndim != 1 or self.counts.shape != (self.edges.size - 1,) or self.cells.shape != self.counts.shape:
            raise ValueError("RegionSizes: one count and one cell sum per bin, one edge more than bins")
        t = [int(v) for v in tallies]
        if len(t) != len(_TALLIES):
            raise ValueError(f"RegionSizes: {len(_TALLIES)} tallies, not {len(t)}")
        for name, v in zip(_TALLIES, t):
            setattr(self, name, v)
        self.N = int(N)
        self.threshold, self.phase, self.connectivity, self.periodic = float(threshold), phase, int(connectivity), bool(periodic)
        self.dr = None if dr is None else float(dr)
        self.labels = labels

    @property
    def extent(self):
        return (self.extent_i, self.extent_j, self.extent_k)

    @property
    def largest_index(self):
        if not self.v_largest:
            return None
        ij, k = divmod(self.label_largest, self.N)
        return divmod(ij, self.N) + (k,)

    @property
    def percolates(self):
        return self.v_largest > 0 and self.N in self.extent

    @property
    def fraction_largest(self):
        return self.v_largest / self.n_phase if self.n_phase else 0.0

    @property
    def mean_volume(self):
        return self.n_phase / self.n_regions if self.n_regions else 0.0

    @property
    def weighted_mean_volume(self):
        return self.sum_v2 / self.n_phase if self.n_phase else 0.0

    @property
    def volume_fraction(self):
        c = self.cells.astype(np.float64)
        return c / self.n_phase if self.n_phase else np.zeros_like(c)

    @property
    def radius_edges(self):
        return np.cbrt(3.0 * self.edges / (4.0 * math.pi))

    def _phys(self, v, power):
        return None if self.dr is None else v * self.dr ** power

    edges_phys = property(lambda self: self._phys(self.edges, 3))
    radius_edges_phys = property(lambda self: self._phys(self.radius_edges, 1))
    v_largest_phys = property(lambda self: self._phys(self.v_largest, 3))
    v_second_phys = property(lambda self: self._phys(self.v_second, 3))
    mean_volume_phys = property(lambda self: self._phys(self.mean_volume, 3))
    weighted_mean_volume_phys = property(lambda self: self._phys(self.weighted_mean_volume, 3))

    def log_line(self):
        """The line of the log file (one per step)."""
        unit = "" if self.dr is None else f" ({self.v_largest_phys:.4e} in units of dr^3)"
        return (f"Regions ({self.phase}, x {'<' if self.phase == 'neutral' else '>='} {self.threshold:g}, {self.connectivity} neighbours, "
                f"{'periodic' if self.periodic else 'open'}): {self.n_regions:n} regions in {self.n_phase:n} cells, largest {self.v_largest:n} "
                f"cells{unit} = {self.fraction_largest:.4f} of the phase, extent {self.extent_i} x {self.extent_j} x {self.extent_k} of "
                f"{self.N}, {'percolates' if self.percolates else 'does not percolate'}; second {self.v_second:n}, mean volume "
                f"{self.mean_volume:.4f}, weighted mean {self.weighted_mean_volume:.4f}")

    def __repr__(self):
        return f"<RegionSizes: {self.log_line()}>"


def region_spec(who, N, threshold=0.5, phase="ionised", connectivity=6, periodic=True, bins=None, dr=None, labels=False):
    """The keywords of :func:`region_sizes` checked and completed for a mesh of N cells a side: a dict with ``edges`` in place of
    ``bins`` (N = None: checked only).  Raises ValueError -- before any device call -- for what the library would refuse."""
    check_threshold(who, threshold)
    check_phase(who, phase)
    check_connectivity(who, connectivity)
    check_flag(who, "periodic", periodic)
    check_dr(who, dr)
    check_flag(who, "labels", labels)
    edges = None
    if bins is not None:
        if is_int(bins) or isinstance(bins, (bool, np.bool_)):
            raise ValueError(f"{who}: bins must be None (powers of two) or an array of edges: a number of bins has no natural upper "
                             f"edge, not {bins!r}")
        try:
            edges = np.array(bins, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: bins must be None or an array of edges, not {type(bins).__name__}") from None
        check_edges(who, edges)
    if N is None:                          # (only the checks: the mesh size is the device's, asked for afterwards)
        return None
    check_mesh(who, N, MESH_LABELS)
    if edges is None:                      # bin b: 2^b <= V < 2^(b + 1); N^3 < 2^nb, so every possible volume is in a bin
        edges = 2.0 ** np.arange((int(N) ** 3).bit_length() + 1)
    return dict(N=int(N), threshold=float(threshold), phase=phase, connectivity=int(connectivity), periodic=bool(periodic), edges=edges,
                dr=None if dr is None else float(dr), labels=bool(labels))


def region_sizes(field=None, *, threshold=0.5, phase='ionised', connectivity=6, periodic=True, bins=None, grid=None, dr=None,
                 labels=False):
    """The connected regions of a grid and their volumes, a :class:`RegionSizes`.

    ``field``: an (N, N, N) host array (the ionised fraction, as a rule) for the mesh of ``device_init``; it is uploaded to the
    device's ionised-fraction grid, which a C2Ray object that keeps its grids there is told beforehand.  None: the device grid
    ``grid`` (a ``_capi.GRID_*`` selector, default the ionised fraction) is analysed where it lies, nothing is uploaded.
    ``phase``: 'ionised' -- the regions of cells with x >= ``threshold`` -- or 'neutral', those with x < threshold (neutral
    islands).  ``connectivity``: 6 (cells joined across faces) or 26 (across faces, edges and corners).  ``periodic``: regions join
    through the faces of the box (True) or end there (False).  ``bins``: None for powers of two -- bin b holds the regions with
    2^b <= V < 2^(b + 1), floor(log2(N^3)) + 1 bins, every possible volume in one -- or the edges themselves (cells, ascending, > 0; at
    most 256 bins).  ``dr``: the size of a cell, for the ``*_phys`` attributes of the result.  ``labels``: also download the label of
    every cell ((N, N, N) uint32, 4 N^3 bytes across PCIe: tests and visualisation)."""
    kw = dict(threshold=threshold, phase=phase, connectivity=connectivity, periodic=periodic, bins=bins, dr=dr, labels=labels)
    return analyse("region_sizes", field, grid, region_spec, kw, regions_on_device, cuda_is_init, load_asora)


def regions_on_device(lib, grid, spec):
    """The library call for a checked `spec` (region_spec) on device grid `grid`, as a :class:`RegionSizes`."""
    out = lib.region_sizes(grid, spec["threshold"], PHASES[spec["phase"]], spec["periodic"], spec["connectivity"], spec["edges"],
                           **({"labels": True} if spec["labels"] else {}))
    return RegionSizes(spec["edges"], out[0], out[1], out[2], spec["N"], spec["threshold"], spec["phase"], spec["connectivity"],
                       spec["periodic"], spec["dr"], out[3] if spec["labels"] else None)
