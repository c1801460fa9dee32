"""Granulometry of the ionised field: the exact Euclidean distance transform and the size distribution by morphological opening
(DESIGN.md section 4.2g).

The fourth morphological description of reionisation next to the mean-free-path sizes (:mod:`pyc2ray_amd.bubbles`), the connected
regions (:mod:`pyc2ray_amd.regions`) and the topology (:mod:`pyc2ray_amd.topology`): the phase is opened by spheres of growing
radius, and the share of it that an opening of radius R removes is the share in structures smaller than R (Kakiichi et al. 2017;
compared with the other two size measures by Giri et al. 2018).  On the CPU that is ``scipy.ndimage.distance_transform_edt`` and one
``binary_opening`` per radius.  :func:`granulometry` runs it on the device (``libasora.granulometry``): the grid is thresholded into
the bit mask of the other analyses, the exact squared distance to the nearest cell outside the phase is formed by three separable
passes, and every radius costs one more such transform from the eroded set, so an ionised-fraction grid that lives on the device is
analysed where it lies.  ``C2Ray.granulometry()`` does that for the current state of a run.  Everything is integers: the same call
returns the same bits.
"""
import math

import numpy as np

from . import _capi
from .asora_core import cuda_is_init
from .load_extensions import load_asora
from ._fieldspec import MESH_LABELS, PHASES, analyse, check_dr, check_flag, check_mesh, check_phase, check_threshold, is_int

__all__ = ['Granulometry', 'granulometry']

_TALLIES = ("n_phase", "d2_max", "n_unbounded", "sum_d2")
_MAX_R2 = 2.0 ** 31


class Granulometry:
    """The result of :func:`granulometry`.  Lengths are in cells; with ``dr`` (the size of a cell in the caller's units) the
    ``*_phys`` attributes give them times dr (None without).

    From the library call.  ``radii`` R_n (ascending) and ``r2`` = floor(R_n^2): the digital ball of a radius is the set of integer
    offsets with |o|^2 <= r2.  ``eroded[n]``: the cells at which that ball lies wholly in the phase (D2 > r2); ``opened[n]``: the
    cells of the union of those balls, the opening of the phase.  ``n_phase``: the cells in phase; ``d2_max``: the largest finite
    squared distance to a cell outside the phase; ``n_unbounded``: the cells without any such distance -- all of them in a periodic
    box that is entirely in phase, else 0; ``sum_d2``: the sum of the finite squared distances.  ``dist2``: the squared distance of
    every cell, (N, N, N) uint32 (0xFFFFFFFF where unbounded), or None if it was not asked for.

    Derived, all with the implicit R_0 = 0 whose opening is the phase itself.  ``opened_fraction`` = opened / n_phase, the share of
    the phase in structures that admit a ball of radius R_n; ``cumulative`` = 1 - that, the share in smaller ones; ``dF[n]`` =
    opened_fraction[n - 1] - opened_fraction[n], the share between R_(n-1) and R_n; ``mid_radii`` and ``dFdR``, ``RdFdR`` there;
    ``unresolved`` = opened_fraction[-1], the share in structures larger than the last radius; ``mean_radius`` (the dF-weighted mean
    of the mid radii) and ``peak_radius`` (the mid radius of the largest R dF/dR) over the resolved part; ``max_inscribed_r2`` =
    d2_max - 1, the largest r2 whose ball still fits somewhere (None when unbounded or empty), ``max_inscribed_radius`` its root.
    Digital balls are not a granulometry in the strict sense: ``opened`` is not always monotone, so single ``dF`` may be slightly
    negative; nothing is clipped or sorted.  An empty phase gives zeros."""

    def __init__(self, radii, eroded, opened, tallies, N, threshold=0.5, phase="ionised", periodic=True, dr=None, dist2=None):
        self.radii = np.array(radii, dtype=np.float64).ravel()
        self.r2 = np.floor(self.radii * self.radii).astype(np.int64)
        self.eroded = np.array(eroded, dtype=np.uint64).ravel()
        self.opened = np.array(opened, dtype=np.uint64).ravel()
        if not (self.radii.size == self.eroded.size == self.opened.size >= 1):
            raise ValueError(f"Granulometry: radii, eroded and opened must have one common length >= 1, not {self.radii.size}, "
                             f"{self.eroded.size}, {self.opened.size}")
        t = [int(v) for v in tallies]
        if len(t) != len(_TALLIES):
            raise ValueError(f"Granulometry: {len(_TALLIES)} tallies, not {len(t)}")
        for name, v in zip(_TALLIES, t):
            setattr(self, name, v)
        self.N = int(N)
        self.threshold, self.phase, self.periodic = float(threshold), phase, bool(periodic)
        self.dr = None if dr is None else float(dr)
        self.dist2 = dist2

    @property
    def tallies(self):
        return np.array([getattr(self, name) for name in _TALLIES], dtype=np.uint64)

    @property
    def unbounded(self):
        """Is there no cell outside the phase at all (a periodic box entirely in phase)?"""
        return self.n_unbounded > 0

    @property
    def opened_fraction(self):
        if self.n_phase == 0:
            return np.zeros(self.radii.size)
        return self.opened.astype(np.float64) / self.n_phase

    @property
    def cumulative(self):
        if self.n_phase == 0:
            return np.zeros(self.radii.size)
        return 1.0 - self.opened_fraction

    @property
    def dF(self):
        if self.n_phase == 0:
            return np.zeros(self.radii.size)
        return -np.diff(np.concatenate(([1.0], self.opened_fraction)))

    @property
    def mid_radii(self):
        return 0.5 * (self.radii + np.concatenate(([0.0], self.radii[:-1])))

    @property
    def dFdR(self):
        dR = np.diff(np.concatenate(([0.0], self.radii)))
        out = np.zeros(self.radii.size)
        np.divide(self.dF, dR, out=out, where=dR > 0)       # (radii[0] = 0: an interval of no width, and dF = 0 there)
        return out

    @property
    def RdFdR(self):
        return self.mid_radii * self.dFdR

    @property
    def unresolved(self):
        return float(self.opened_fraction[-1])

    @property
    def mean_radius(self):
        w = self.dF
        total = w.sum()
        return float((self.mid_radii * w).sum() / total) if total > 0 else 0.0

    @property
    def peak_radius(self):
        if self.n_phase == 0:
            return 0.0
        return float(self.mid_radii[int(np.argmax(self.RdFdR))])

    @property
    def max_inscribed_r2(self):
        if self.n_phase == 0 or self.unbounded:
            return None
        return self.d2_max - 1

    @property
    def max_inscribed_radius(self):
        v = self.max_inscribed_r2
        return None if v is None else math.sqrt(v)

    def _phys(self, v, power=1):
        return None if self.dr is None or v is None else v * self.dr ** power

    radii_phys = property(lambda self: self._phys(self.radii))
    mid_radii_phys = property(lambda self: self._phys(self.mid_radii))
    dFdR_phys = property(lambda self: self._phys(self.dFdR, -1))
    mean_radius_phys = property(lambda self: self._phys(self.mean_radius))
    peak_radius_phys = property(lambda self: self._phys(self.peak_radius))
    max_inscribed_radius_phys = property(lambda self: self._phys(self.max_inscribed_radius))

    def log_line(self):
        """The line of the log file (one per step)."""
        unit = "" if self.dr is None else f" ({self.mean_radius_phys:.4e}, {self.peak_radius_phys:.4e} in units of dr)"
        if self.n_phase == 0:
            largest = "no cell in phase"
        elif self.unbounded:
            largest = "the whole periodic box in phase"
        else:
            largest = f"largest inscribed ball r2 {self.max_inscribed_r2:n}"
        return (f"Granulometry ({self.phase}, x {'<' if self.phase == 'neutral' else '>='} {self.threshold:g}, "
                f"{'periodic' if self.periodic else 'open'}, {self.radii.size} radii to {self.radii[-1]:g}): {self.n_phase:n} cells, "
                f"{largest}; mean radius {self.mean_radius:.3f}, peak {self.peak_radius:.3f}{unit}, "
                f"{100.0 * self.unresolved:.2f} % above the last radius")

    def __repr__(self):
        return f"<Granulometry: {self.log_line()}>"


def _radii(who, N, radii):
    """None: 1 ... max(1, min(N // 4, 32)) (needs N); an int n: 1 ... n; else an array of finite, >= 0, strictly ascending radii."""
    if radii is None:
        if N is None:
            return None
        return np.arange(1, max(1, min(N // 4, 32)) + 1, dtype=np.float64)
    if isinstance(radii, (bool, np.bool_)):
        raise ValueError(f"{who}: radii must be None, an int or an array of radii, not a bool")
    if is_int(radii):
        if not 1 <= radii <= _capi.BUBBLE_MAX_BINS:
            raise ValueError(f"{who}: radii as an int must be in [1, {_capi.BUBBLE_MAX_BINS}], not {radii}")
        return np.arange(1, int(radii) + 1, dtype=np.float64)
    try:
        r = np.array(radii, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: radii must be None, an int or an array of radii, not {radii!r}") from None
    if r.ndim != 1 or not 1 <= r.size <= _capi.BUBBLE_MAX_BINS:
        raise ValueError(f"{who}: radii must be a one-dimensional array of 1 ... {_capi.BUBBLE_MAX_BINS} radii")
    if not np.all(np.isfinite(r)):
        raise ValueError(f"{who}: radii must be finite")
    if r[0] < 0:
        raise ValueError(f"{who}: radii must be >= 0")
    if np.any(np.diff(r) <= 0):
        raise ValueError(f"{who}: radii must be strictly ascending")
    if not r[-1] * r[-1] < _MAX_R2:
        raise ValueError(f"{who}: radii must have R^2 < 2^31")
    return r


def granulometry_spec(who, N, threshold=0.5, phase="ionised", periodic=True, radii=None, dr=None, distances=False):
    """The keywords of :func:`granulometry` checked and completed for a mesh of N cells a side, as a dict (N = None: checked only).
    Raises ValueError -- before any device call -- for what the library would refuse."""
    check_threshold(who, threshold)
    check_phase(who, phase)
    check_flag(who, "periodic", periodic)
    r = _radii(who, N, radii)
    check_dr(who, dr)
    check_flag(who, "distances", distances)
    if N is None:                          # (only the checks: the mesh size is the device's, asked for afterwards)
        return None
    check_mesh(who, N, MESH_LABELS)
    return dict(N=int(N), threshold=float(threshold), phase=phase, periodic=bool(periodic), radii=r, dr=None if dr is None else float(dr),
                distances=bool(distances))


def granulometry(field=None, *, threshold=0.5, phase='ionised', periodic=True, radii=None, grid=None, dr=None, distances=False):
    """The granulometry of the in-phase cells of a grid, a :class:`Granulometry`.

    ``field``: an (N, N, N) host array (the ionised fraction, as a rule) for the mesh of ``device_init``; it is uploaded to the
    device's ionised-fraction grid, which a C2Ray object that keeps its grids there is told beforehand.  None: the device grid
    ``grid`` (a ``_capi.GRID_*`` selector, default the ionised fraction) is analysed where it lies, nothing is uploaded.
    ``phase``: 'ionised' -- the cells with x >= ``threshold`` -- or 'neutral', those with x < threshold; a NaN is in neither.
    ``periodic``: distances follow the minimum image (True), or the box ends at its faces, beyond which nothing is in phase (False).
    ``radii``: None for 1 ... max(1, min(N // 4, 32)), an int n for 1 ... n, or an array of finite, >= 0, strictly ascending radii
    (at most 256, R^2 < 2^31).  ``dr``: the size of a cell, for the ``*_phys`` attributes of the result.  ``distances``: download the
    squared distance transform as well (``dist2`` of the result)."""
    kw = dict(threshold=threshold, phase=phase, periodic=periodic, radii=radii, dr=dr, distances=distances)
    return analyse("granulometry", field, grid, granulometry_spec, kw, granulometry_on_device, cuda_is_init, load_asora)


def granulometry_on_device(lib, grid, spec):
    """The library call for a checked `spec` (granulometry_spec) on device grid `grid`, as a :class:`Granulometry`."""
    got = lib.granulometry(grid, spec["threshold"], PHASES[spec["phase"]], spec["periodic"], spec["radii"], distances=spec["distances"])
    return Granulometry(spec["radii"], got[0], got[1], got[2], spec["N"], spec["threshold"], spec["phase"], spec["periodic"], spec["dr"],
                        dist2=got[3] if spec["distances"] else None)
