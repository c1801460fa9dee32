"""Size distribution of the ionised regions by the mean-free-path method.

The standard measure of the morphology of reionisation (Mesinger & Furlanetto 2007; ``tools21cm.mfp`` on the CPU): rays start in
random ionised cells, fly in random directions and end at the first neutral cell; the histogram of their lengths, as R dP/dR, is the
bubble size distribution.  :func:`mfp_distribution` runs it on the device (``libasora.bubble_mfp``): the grid is thresholded into a
bit mask there and the rays march through the mask, so an ionised-fraction grid that lives on the device is analysed where it lies.
``C2Ray.bubble_sizes()`` does that for the current state of a run.  Every ray is a pure function of ``(seed, ray index, mask)``:
the same call returns the same bits.
"""
import math

import numpy as np

from . import _capi
from .asora_core import cuda_is_init
from .load_extensions import load_asora
from ._fieldspec import PHASES, analyse, check_dr, check_edges, check_flag, check_phase, check_threshold, is_int, is_real

__all__ = ['BubbleSizes', 'mfp_distribution']


class BubbleSizes:
    """The result of :func:`mfp_distribution`.  Lengths are in cells; with ``dr`` (the size of a cell in the caller's units) the
    ``*_phys`` attributes give them in those units (None without).

    ``edges`` (nb + 1), ``counts`` (nb, uint64): the ENDED rays -- those that met a cell out of phase -- by length;
    ``ended``, ``capped`` (longer than ``l_max``), ``left_box`` (open boundaries: out through a face), ``underflow``, ``overflow``
    (ENDED, but below ``edges[0]`` / at or beyond ``edges[-1]``); ``n_rays`` = ended + capped + left_box; ``n_phase``: in-phase cells of
    the grid (0: no ray could start, every count is 0); ``fraction_capped`` = capped / n_rays.
    ``mean``, ``rms``: of the lengths of the ENDED rays, under- and overflow included.
    ``centres``: geometric bin centres; ``RdPdR`` = counts / (sum(counts) dlnR), dlnR = ln(edges[b + 1] / edges[b]): its sum times
    dlnR over the bins is 1; ``peak_radius``: the centre of the bin where it is largest (0 when every bin is empty)."""

    def __init__(self, edges, counts, tallies, moments, n_rays, threshold=0.5, phase="ionised", seed=0, l_max=None, periodic=True,
                 dr=None):
        self.edges = np.array(edges, dtype=np.float64)
        self.counts = np.array(counts, dtype=np.uint64)
        if self.edges.ndim != 1 or self.counts.shape != (self.edges.size - 1,):
            raise ValueError("BubbleSizes: one count per bin, one edge more than bins")
        t = [int(v) for v in tallies]
        self.ended, self.capped, self.left_box, self.underflow, self.overflow, self.n_phase = t
        self.sum_length, self.sum_length2 = float(moments[0]), float(moments[1])
        self.n_rays = int(n_rays)
        self.threshold, self.phase, self.seed, self.periodic = float(threshold), phase, int(seed), bool(periodic)
        self.l_max = None if l_max is None else float(l_max)
        self.dr = None if dr is None else float(dr)

    @property
    def fraction_capped(self):
        return self.capped / self.n_rays if self.n_rays else 0.0

    @property
    def mean(self):
        return self.sum_length / self.ended if self.ended else 0.0

    @property
    def rms(self):
        return math.sqrt(self.sum_length2 / self.ended) if self.ended else 0.0

    @property
    def centres(self):
        return np.sqrt(self.edges[:-1] * self.edges[1:])

    @property
    def dlnR(self):
        return np.log(self.edges[1:] / self.edges[:-1])

    @property
    def RdPdR(self):
        c = self.counts.astype(np.float64)
        total = c.sum()
        return c / (total * self.dlnR) if total else np.zeros_like(c)

    @property
    def peak_radius(self):
        return float(self.centres[int(np.argmax(self.RdPdR))]) if self.counts.any() else 0.0

    def _phys(self, v):
        return None if self.dr is None else v * self.dr

    edges_phys = property(lambda self: self._phys(self.edges))
    centres_phys = property(lambda self: self._phys(self.centres))
    mean_phys = property(lambda self: self._phys(self.mean))
    rms_phys = property(lambda self: self._phys(self.rms))
    peak_radius_phys = property(lambda self: self._phys(self.peak_radius))

    def log_line(self):
        """The line of the log file (one per step)."""
        unit = "" if self.dr is None else f" ({self.mean_phys:.4e}, {self.peak_radius_phys:.4e} in units of dr)"
        return (f"Bubble sizes ({self.phase}, x {'<' if self.phase == 'neutral' else '>='} {self.threshold:g}): {self.n_rays:n} rays from "
                f"{self.n_phase:n} cells, mean {self.mean:.4f}, rms {self.rms:.4f}, peak of R dP/dR at {self.peak_radius:.4f} cells{unit}; "
                f"capped {self.fraction_capped:.4f}, left the box {self.left_box:n}")

    def __repr__(self):
        return f"<BubbleSizes: {self.log_line()}>"


def bubble_spec(who, N, threshold=0.5, phase="ionised", n_rays=100_000, seed=0, l_max=None, bins=64, periodic=True, dr=None):
    """The keywords of :func:`mfp_distribution` checked and completed for a mesh of N cells a side: a dict with ``edges`` in place
    of ``bins`` and ``l_max`` filled in (N = None: checked only).  Raises ValueError -- before any device call -- for what the
    library would refuse."""
    check_threshold(who, threshold)
    check_phase(who, phase)
    if not is_int(n_rays) or n_rays < 0:
        raise ValueError(f"{who}: n_rays must be an integer >= 0, not {n_rays!r}")
    if not is_int(seed) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"{who}: seed must be an integer in [0, 2^64), not {seed!r}")
    if l_max is not None and (not is_real(l_max) or not (math.isfinite(l_max) and l_max > 0)):
        raise ValueError(f"{who}: l_max must be None or a finite number > 0 (cells), not {l_max!r}")
    check_flag(who, "periodic", periodic)
    check_dr(who, dr)
    edges = None
    if is_int(bins):
        if not 1 <= bins <= _capi.BUBBLE_MAX_BINS:
            raise ValueError(f"{who}: bins must be 1 ... {_capi.BUBBLE_MAX_BINS} or an array of edges, not {bins!r}")
        if l_max is not None and not l_max > 0.5:
            raise ValueError(f"{who}: a number of bins spans [0.5, l_max] and needs l_max > 0.5; pass the edges for l_max = {l_max!r}")
    else:
        try:
            edges = np.array(bins, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: bins must be a number of bins or an array of edges, not {type(bins).__name__}") from None
        check_edges(who, edges)
    if N is None:                          # (only the checks: the mesh size is the device's, asked for afterwards)
        return None
    if l_max is None:
        l_max = float(N)
    if edges is None:
        edges = np.geomspace(0.5, float(l_max), int(bins) + 1)
    return dict(threshold=float(threshold), phase=phase, n_rays=int(n_rays), seed=int(seed), l_max=float(l_max), edges=edges,
                periodic=bool(periodic), dr=None if dr is None else float(dr))


def mfp_distribution(field=None, *, threshold=0.5, phase='ionised', n_rays=100_000, seed=0, l_max=None, bins=64, periodic=True,
                     grid=None, dr=None):
    """The mean-free-path size distribution of the regions of a grid, a :class:`BubbleSizes`.

    ``field``: an (N, N, N) host array (the ionised fraction, as a rule) for the mesh of ``device_init``; it is uploaded to the
    device's ionised-fraction grid, which a C2Ray object that keeps its grids there is told beforehand.  None: the device grid
    ``grid`` (a ``_capi.GRID_*`` selector, default the ionised fraction) is analysed where it lies, nothing is uploaded.
    ``phase``: 'ionised' -- rays start in cells with x >= ``threshold`` and end at the first with x < threshold -- or 'neutral', the
    other way round (neutral islands).  ``n_rays`` rays, numbered from 0, each a function of (``seed``, its number, the mask).
    ``l_max`` (cells, default N): a ray that has not ended by then is counted as capped, in no bin.  ``bins``: a number of bins,
    for ``np.geomspace(0.5, l_max, bins + 1)``, or the edges themselves (cells, ascending, > 0; at most 256 bins).
    ``periodic``: rays wrap around the box (True) or leave it through its faces and are counted as ``left_box`` (False).
    ``dr``: the size of a cell, for the ``*_phys`` attributes of the result."""
    kw = dict(threshold=threshold, phase=phase, n_rays=n_rays, seed=seed, l_max=l_max, bins=bins, periodic=periodic, dr=dr)
    return analyse("mfp_distribution", field, grid, bubble_spec, kw, distribution_on_device, cuda_is_init, load_asora)


def distribution_on_device(lib, grid, spec):
    """The library call for a checked `spec` (bubble_spec) on device grid `grid`, as a :class:`BubbleSizes`."""
    counts, tallies, moments = lib.bubble_mfp(grid, spec["threshold"], PHASES[spec["phase"]], spec["periodic"], spec["seed"],
                                              spec["n_rays"], spec["l_max"], spec["edges"])
    return BubbleSizes(spec["edges"], counts, tallies, moments, spec["n_rays"], spec["threshold"], spec["phase"], spec["seed"],
                       spec["l_max"], spec["periodic"], spec["dr"])
