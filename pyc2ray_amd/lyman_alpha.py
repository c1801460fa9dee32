"""The Lyman-alpha forest of a reionisation state: optical depth and transmitted flux along every line of sight of the box, the
effective optical depth, the flux PDF and the distribution of dark gaps.

Next to the 21-cm signal, the forest in quasar spectra is what constrains the end of reionisation, and the quantities fitted are
the effective optical depth, the PDF of the transmitted flux and the lengths of the dark gaps.  On the CPU that is four N^3
downloads and a loop over N^2 skewers.  :func:`lyman_alpha_forest` runs it on the device (``libasora.lyman_alpha_forest``): every
cell's neutral hydrogen is spread over its displaced extent in velocity space -- the cell edges of the redshift-space mapping -- and
convolved with its thermal Doppler profile, cut at six Doppler widths; F = exp(-tau); the sums, the PDF and the gaps are reduced on
the device in a fixed order: the same call returns the same bits.  Not modelled: the Lorentzian damping wings of neutral islands,
light-cone evolution along the skewer, helium.  ``C2Ray.lyman_alpha_forest()`` does it for the current state of a run with
``C2Ray.los_velocity``, with the two scale factors from the object's cosmology.
"""
import math

import numpy as np

from . import _capi, _residency
from .asora_core import cuda_is_init
from .load_extensions import load_asora
from ._fieldspec import MESH_TRANSFORM, check_flag, check_mesh, host_field, is_int, is_real
from .redshift_space import _check_axis, _check_velocity

__all__ = ['LymanAlphaForest', 'lyman_alpha_forest']

WHATS = {"flux": _capi.LYA_FLUX, "tau": _capi.LYA_TAU}
#: the default number of bins of the flux PDF, equal bins over [0, 1]
DEFAULT_BINS = 20
_GRIDS = (("xh", _capi.GRID_XH), ("ndens", _capi.GRID_NDENS), ("temp", _capi.GRID_TEMP))


class LymanAlphaForest:
    """The result of :func:`lyman_alpha_forest` for a mesh of N cells a side, lines along ``los_axis``.

    From the library call.  ``stats`` and ``counts``: the words of include/asora_hip.h (``_capi.LYA_*``); ``gap_counts`` (uint64, N + 1):
    the number of dark gaps by length in cells, entry 0 always 0; ``pdf`` (uint64) and ``bin_edges``: the cells by transmitted flux,
    edges[i] <= F < edges[i + 1] (None without bins); ``gap_threshold``: a pixel is dark where F is below it; ``velocity``: were the
    cells moved by a velocity; ``tau`` and ``flux``: the (N, N, N) cubes if they were asked for.

    Derived.  ``mean_flux``; ``tau_eff`` = -ln(mean_flux) (inf for a mean of 0); ``flux_variance``; ``tau_min``, ``tau_max``;
    ``gap_lengths_cells``: the lengths that occur, ascending -- ``gap_counts[gap_lengths_cells]`` are their numbers;
    ``longest_gap``, ``n_gaps``, ``dark_fraction`` (dark pixels / N^3), ``full_lines`` (lines that are one gap of length N);
    ``window`` (the W used), ``clipped`` (cells whose reach exceeds W: 0 says the window cut nothing off), ``degenerate`` (cells
    narrower than 2^-10 after the mapping), ``nonfinite`` (pixels whose tau is not finite)."""

    def __init__(self, N, los_axis, stats, counts, gap_counts, pdf=None, bin_edges=None, gap_threshold=0.05, velocity=False, tau=None,
                 flux=None):
        self.N, self.los_axis = int(N), int(los_axis)
        self.stats = np.array(stats, dtype=np.float64).ravel()
        self.counts = np.array(counts, dtype=np.uint64).ravel()
        self.gap_counts = np.array(gap_counts, dtype=np.uint64).ravel()
        if self.stats.size != _capi.LYA_STATS or self.counts.size != _capi.LYA_COUNTS or self.gap_counts.size != self.N + 1:
            raise ValueError(f"LymanAlphaForest: {_capi.LYA_STATS} stats, {_capi.LYA_COUNTS} counts and N + 1 = {self.N + 1} gap counts")
        if (pdf is None) != (bin_edges is None):
            raise ValueError("LymanAlphaForest: pdf and bin_edges go together")
        self.pdf = None if pdf is None else np.array(pdf, dtype=np.uint64).ravel()
        self.bin_edges = None if bin_edges is None else np.array(bin_edges, dtype=np.float64).ravel()
        if self.pdf is not None and self.bin_edges.size != self.pdf.size + 1:
            raise ValueError(f"LymanAlphaForest: {self.pdf.size} bins go with {self.pdf.size + 1} edges, not {self.bin_edges.size}")
        self.gap_threshold, self.velocity, self.tau, self.flux = float(gap_threshold), bool(velocity), tau, flux

    @property
    def _cells(self):
        return float(self.N) ** 3

    @property
    def mean_flux(self):
        return float(self.stats[_capi.LYA_SUM_F]) / self._cells

    @property
    def tau_eff(self):
        m = self.mean_flux
        return -math.log(m) if m > 0.0 else math.inf

    @property
    def flux_variance(self):
        return float(self.stats[_capi.LYA_SUM_F2]) / self._cells - self.mean_flux ** 2

    @property
    def tau_min(self):
        return float(self.stats[_capi.LYA_TAU_MIN])

    @property
    def tau_max(self):
        return float(self.stats[_capi.LYA_TAU_MAX])

    @property
    def gap_lengths_cells(self):
        return np.nonzero(self.gap_counts)[0]

    def gap_lengths(self, dv):
        """(the lengths of the gaps that occur in velocity units, `dv` per cell; how many there are of each)"""
        if not is_real(dv) or not (math.isfinite(dv) and dv > 0):
            raise ValueError(f"LymanAlphaForest.gap_lengths: dv must be a finite number > 0, not {dv!r}")
        cells = self.gap_lengths_cells
        return cells * float(dv), self.gap_counts[cells]

    @property
    def longest_gap(self):
        return int(self.counts[_capi.LYA_LONGEST])

    @property
    def n_gaps(self):
        return int(self.counts[_capi.LYA_N_GAPS])

    @property
    def dark_fraction(self):
        return int(self.counts[_capi.LYA_N_DARK]) / self._cells

    @property
    def full_lines(self):
        return int(self.counts[_capi.LYA_FULL_LINES])

    @property
    def window(self):
        return int(self.counts[_capi.LYA_WINDOW])

    @property
    def clipped(self):
        return int(self.counts[_capi.LYA_CLIPPED])

    @property
    def degenerate(self):
        return int(self.counts[_capi.LYA_DEGENERATE])

    @property
    def nonfinite(self):
        return int(self.counts[_capi.LYA_NONFINITE])

    def log_line(self):
        """The line of the log file (one per step)."""
        space = "with peculiar velocities" if self.velocity else "no velocity"
        line = (f"Lyman-alpha forest (line of sight {self.los_axis}, {space}, W = {self.window}): mean flux {self.mean_flux:.6e}, tau_eff "
                f"{self.tau_eff:.6e}, flux variance {self.flux_variance:.6e}, tau in [{self.tau_min:.4e}, {self.tau_max:.4e}]; "
                f"{self.n_gaps:n} dark gaps (F < {self.gap_threshold:g}), longest {self.longest_gap} cells, dark fraction "
                f"{self.dark_fraction:.6f}, {self.full_lines} lines wholly dark")
        for name in ("clipped", "degenerate", "nonfinite"):
            if getattr(self, name):
                line += f"; {name} {getattr(self, name):n}"
        return line

    def __repr__(self):
        return f"<LymanAlphaForest: {self.log_line()}>"


def _check_positive(who, name, v):
    if not is_real(v) or not (math.isfinite(v) and v > 0):
        raise ValueError(f"{who}: {name} must be a finite number > 0, not {v!r}")


def _pdf_edges(who, bins):
    """The edges of the flux PDF: None for DEFAULT_BINS, an int n for n equal bins over [0, 1] -- the last edge is the next double
    above 1, so that F = 1 is counted; else an array of 2 ... LYA_MAX_BINS + 1 finite, non-decreasing edges, taken as they are."""
    limit = _capi.LYA_MAX_BINS
    if bins is None:
        bins = DEFAULT_BINS
    if isinstance(bins, (bool, np.bool_)):
        raise ValueError(f"{who}: bins must be None, an int or an array of edges, not a bool")
    if is_int(bins):
        if not 1 <= bins <= limit:
            raise ValueError(f"{who}: bins as an int must be in [1, {limit}], not {bins}")
        e = np.linspace(0.0, 1.0, int(bins) + 1)
        e[-1] = np.nextafter(1.0, 2.0)
        return e
    try:
        e = np.array(bins, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: bins must be None, an int or an array of edges, not {bins!r}") from None
    if e.ndim != 1 or not 2 <= e.size <= limit + 1:
        raise ValueError(f"{who}: bins must be a one-dimensional array of 2 ... {limit + 1} edges")
    if not np.all(np.isfinite(e)) or np.any(np.diff(e) < 0):
        raise ValueError(f"{who}: the edges of bins must be finite and non-decreasing")
    return e


def lyman_alpha_spec(who, N, xh=None, ndens=None, temp=None, velocity=None, device_velocity=False, velocity_scale=1.0, b_scale=None,
                     tau_scale=None, los_axis=2, window=None, gap_threshold=0.05, bins=None, into=None, into_what='flux', return_tau=False,
                     return_flux=False):
    """The keywords of :func:`lyman_alpha_forest` checked and completed for a mesh of N cells a side, as a dict (N = None: checked
    only, but for the shapes of the host arrays among themselves).  ``device_velocity``: the velocity is on the device already.
    Raises ValueError -- before any device call -- for what the library would refuse."""
    fields = {}
    for name, a in (("xh", xh), ("ndens", ndens), ("temp", temp)):
        if a is not None:
            a = host_field(who, name, a)
            if N is not None and a.shape[0] != N:
                raise ValueError(f"{who}: {name} must have the shape ({N}, {N}, {N}) of the mesh, not {a.shape}")
            fields[name] = a
    shapes = {a.shape for a in fields.values()}
    if len(shapes) > 1:
        raise ValueError(f"{who}: xh, ndens and temp must have one shape, not {sorted(shapes)}")
    check_flag(who, "device_velocity", device_velocity)
    if velocity is not None and device_velocity:
        raise ValueError(f"{who}: device_velocity goes with a velocity that is on the device already, not with velocity")
    velocity, _ = _check_velocity(who, None, velocity, None, velocity_scale)     # (no window of the mapping's here: W is capped, and clipped says so)
    n_known = N if N is not None else (next(iter(shapes))[0] if shapes else None)
    if velocity is not None and n_known is not None and velocity.shape[0] != n_known:
        raise ValueError(f"{who}: velocity must have the shape ({n_known}, {n_known}, {n_known}) of the mesh, not {velocity.shape}")
    _check_positive(who, "b_scale", b_scale)
    _check_positive(who, "tau_scale", tau_scale)
    _check_axis(who, los_axis)
    if window is not None and (not is_int(window) or window < 1):
        raise ValueError(f"{who}: window must be None (automatic) or an int >= 1, not {window!r}")
    if window is not None and n_known is not None and 2 * window + 1 > n_known:
        raise ValueError(f"{who}: a window of 2 W + 1 = {2 * window + 1} cells is wider than the N = {n_known} cells of a line")
    if not is_real(gap_threshold) or not math.isfinite(gap_threshold):
        raise ValueError(f"{who}: gap_threshold must be a finite number, not {gap_threshold!r}")
    edges = _pdf_edges(who, bins)
    if into is not None and (not is_int(into) or not 0 <= into < _capi.GRID_COUNT):
        raise ValueError(f"{who}: into must be None or a grid selector 0 ... {_capi.GRID_COUNT - 1} (_capi.GRID_*), not {into!r}")
    if not isinstance(into_what, str) or into_what not in WHATS:
        raise ValueError(f"{who}: into_what must be 'flux' or 'tau', not {into_what!r}")
    check_flag(who, "return_tau", return_tau)
    check_flag(who, "return_flux", return_flux)
    if N is None:                          # (only the checks: the mesh size is the device's, asked for afterwards)
        return None
    check_mesh(who, N, MESH_TRANSFORM)
    moved = velocity is not None or bool(device_velocity)
    return dict(N=int(N), fields=fields, velocity=velocity, velocity_scale=float(velocity_scale) if moved else None, b_scale=float(b_scale),
                tau_scale=float(tau_scale), los_axis=int(los_axis), window=0 if window is None else int(window),
                gap_threshold=float(gap_threshold), edges=edges, into=None if into is None else int(into), into_what=into_what,
                return_tau=bool(return_tau), return_flux=bool(return_flux))


def lyman_alpha_forest(xh=None, ndens=None, temp=None, *, velocity=None, velocity_scale=1.0, b_scale, tau_scale, los_axis=2, window=None,
                       gap_threshold=0.05, bins=None, into=None, into_what='flux', return_tau=False, return_flux=False):
    """The Lyman-alpha forest along ``los_axis`` (0, 1 or 2) of the mesh of ``device_init``: a :class:`LymanAlphaForest`.

    ``xh``, ``ndens``, ``temp``: (N, N, N) host arrays -- the ionised fraction, the density and the temperature in K -- uploaded to
    their device grids; None: the device grid where it lies.  ``velocity``: an (N, N, N) array, the velocity along ``los_axis``;
    ``velocity_scale`` converts it to cells (``C2Ray.velocity_scale()`` for proper km/s); None: the gas is at rest.  ``b_scale``:
    the Doppler parameter in cells per sqrt(K) (``C2Ray.lyman_alpha_b_scale()``); ``tau_scale``: the Gunn-Peterson optical depth per
    unit neutral density (``C2Ray.lyman_alpha_tau_scale()``).  ``window``: None for the automatic W, which covers every cell's reach
    (at the cost of one more synchronisation) up to (N - 1) / 2, or W itself; ``clipped`` counts the cells it cuts off.
    ``gap_threshold``: a pixel is dark where F is below it.  ``bins``: the flux PDF's -- None for 20, an int n for n equal bins over
    [0, 1], or an array of finite, non-decreasing edges.  ``into`` (a grid selector, ``_capi.GRID_*``): F (``into_what`` 'flux') or
    tau ('tau') is written into that device grid, where ``power_spectrum_los(kind='xh')``, ``smoothed_field``, ``region_sizes``
    and the other analyses of a grid take it; it may be a grid the call reads.  ``return_tau`` / ``return_flux``: download the
    cubes as well."""
    who = "lyman_alpha_forest"
    kw = dict(xh=xh, ndens=ndens, temp=temp, velocity=velocity, velocity_scale=velocity_scale, b_scale=b_scale, tau_scale=tau_scale,
              los_axis=los_axis, window=window, gap_threshold=gap_threshold, bins=bins, into=into, into_what=into_what,
              return_tau=return_tau, return_flux=return_flux)
    lyman_alpha_spec(who, None, **kw)
    if not cuda_is_init():
        raise RuntimeError("GPU not initialized. Please initialize it by calling device_init(N)")
    lib = load_asora()
    if getattr(lib, "_N", None) is None:
        raise RuntimeError(f"{who}: needs a device initialised through device_init (the mesh size)")
    spec = lyman_alpha_spec(who, int(lib._N), **kw)
    if spec["fields"] or spec["into"] is not None:
        _residency.reclaim()              # this call overwrites a device grid a resident C2Ray object may be relying on
    for name, which in _GRIDS:
        if name in spec["fields"]:
            lib.grid_to_device(which, np.asarray(spec["fields"][name], dtype=np.float64))
    if spec["velocity"] is not None:
        _residency.reclaim()              # (the library has one velocity: a C2Ray object that keeps its own there uploads it again)
        lib.los_velocity_to_device(np.asarray(spec["velocity"], dtype=np.float64))
    return forest_on_device(lib, spec)


def forest_on_device(lib, spec):
    """The library call for a checked `spec` (lyman_alpha_spec) on the device grids, as a :class:`LymanAlphaForest`."""
    got = lib.lyman_alpha_forest(spec["los_axis"], spec["velocity_scale"], spec["b_scale"], spec["tau_scale"], window=spec["window"],
                                 gap_threshold=spec["gap_threshold"], edges=spec["edges"], dst_grid=spec["into"],
                                 dst_what=WHATS[spec["into_what"]], tau=spec["return_tau"], flux=spec["return_flux"])
    return LymanAlphaForest(spec["N"], spec["los_axis"], got["stats"], got["counts"], got["gaps"], pdf=got["pdf"], bin_edges=spec["edges"],
                            gap_threshold=spec["gap_threshold"], velocity=spec["velocity_scale"] is not None, tau=got["tau"],
                            flux=got["flux"])
