"""Smoothed fields: what a telescope of finite resolution sees of a reionisation run, and its one-point statistics (DESIGN.md section
4.2i).

The analyses of the ionised field (:mod:`pyc2ray_amd.bubbles`, :mod:`pyc2ray_amd.regions`, :mod:`pyc2ray_amd.topology`,
:mod:`pyc2ray_amd.granulometry`) and the power spectrum (:mod:`pyc2ray_amd.powerspec`) work at the resolution of the mesh.  Forecasts
smooth the brightness-temperature cube to the instrument's resolution first -- a Gaussian beam across the sky, a top-hat along
frequency, the mean removed (``tools21cm.smooth_coeval``) -- and then take sizes, the PDF, the variance, the skewness and the kurtosis.
:func:`smoothed_field` does that on the device (``libasora.smooth_field``): the field is formed from the device grids inside the
forward transform the power spectrum uses, multiplied by a filter, transformed back by the same hand-written FP64 transform, and
reduced to its statistics by kernels whose sums have a fixed order, so the same call returns the same bits.  The result can be written
into a device grid (``into``), which the mask-based analyses then take by their grid selector without a copy through the host.

What a filter *is* lives here: a :class:`Filter` is a product of per-axis tables over the folded index m = min(n, N - n) and a radial
table over |m|^2; the device only indexes them and multiplies.  ``C2Ray.observed_map()`` builds the telescope's filter from a
baseline, the redshift and the cosmology.
"""
import math

import numpy as np

from . import _capi, _residency
from .asora_core import cuda_is_init
from .load_extensions import load_asora
from ._fieldspec import MESH_TRANSFORM, check_flag, check_mesh, check_scale, check_t_gamma, host_field, is_int, is_real
from .powerspec import _KINDS, _check_kind

__all__ = ['Filter', 'SmoothedField', 'smoothed_field', 'gaussian', 'boxcar', 'spherical_tophat', 'sharp_k', 'telescope']

_FWHM_TO_SIGMA = 1.0 / (2.0 * math.sqrt(2.0 * math.log(2.0)))


class Filter:
    """A filter in Fourier space, W(n) = ((w_i[n_x] w_j[n_y]) w_k[n_z]) w_r[|m|^2]: a product of factors, each a function of the
    folded index m = min(n, N - n) of one axis or of |m| = sqrt(m_x^2 + m_y^2 + m_z^2).  Built by :func:`gaussian`, :func:`boxcar`,
    :func:`spherical_tophat`, :func:`sharp_k`, :func:`telescope`; filters multiply with ``*``.  ``tables(N)`` evaluates it for a mesh:
    ``(w_i, w_j, w_k, w_r)``, arrays of N entries each and of 3 (N // 2)^2 + 1, None where the filter has no factor.  A per-axis
    table is evaluated at m = 0 ... N // 2 and then indexed by the folded index, so w[n] and w[N - n] are the same bits."""

    def __init__(self, factors=(), label="identity"):
        self.factors = tuple(factors)               # (slot 0 ... 3, function(m or |m| as float64 array, N) -> array)
        self.label = label

    def __mul__(self, other):
        if not isinstance(other, Filter):
            return NotImplemented
        labels = [f.label for f in (self, other) if f.factors]
        return Filter(self.factors + other.factors, " * ".join(labels) if labels else "identity")

    def tables(self, N):
        N = int(N)
        if N < 1:
            raise ValueError(f"Filter.tables: N must be >= 1, not {N}")
        half = N // 2
        n = np.arange(N)
        fold = np.minimum(n, N - n)
        out = [None, None, None, None]
        for slot, fn in self.factors:
            arg = np.arange(half + 1, dtype=np.float64) if slot < 3 else np.sqrt(np.arange(3 * half * half + 1, dtype=np.float64))
            w = np.asarray(fn(arg, N), dtype=np.float64)
            if w.shape != arg.shape:
                raise ValueError("Filter.tables: a factor must return one value per index")
            out[slot] = w if out[slot] is None else out[slot] * w
        return tuple(None if w is None else np.ascontiguousarray(w[fold] if slot < 3 else w) for slot, w in enumerate(out))

    def on_mesh(self, N):
        """W of the stored half-space, (N, N, N // 2 + 1), multiplied in the library's order."""
        w_i, w_j, w_k, w_r = self.tables(N)
        one = np.ones(N)
        W = ((one if w_i is None else w_i)[:, None, None] * (one if w_j is None else w_j)[None, :, None]) \
            * (one if w_k is None else w_k)[None, None, :N // 2 + 1]
        if w_r is not None:
            m = np.minimum(np.arange(N), N - np.arange(N)).astype(np.int64)
            mz = np.arange(N // 2 + 1, dtype=np.int64)
            W = W * w_r[m[:, None, None] ** 2 + m[None, :, None] ** 2 + mz[None, None, :] ** 2]
        return W

    def __repr__(self):
        return f"<Filter: {self.label}>"


def _positive(who, name, v):
    if not is_real(v) or not (math.isfinite(v) and v >= 0):
        raise ValueError(f"{who}: {name} must be a finite number >= 0, not {v!r}")
    return float(v)


def _axis(who, axis):
    if not is_int(axis) or axis not in (0, 1, 2):
        raise ValueError(f"{who}: an axis must be 0, 1 or 2, not {axis!r}")
    return int(axis)


def gaussian(fwhm, axes=(0, 1, 2)):
    """A Gaussian of full width at half maximum `fwhm` cells along each of `axes`: exp(-(2 pi m / N)^2 sigma^2 / 2) per axis, sigma
    = fwhm / (2 sqrt(2 ln 2))."""
    fwhm = _positive("gaussian", "fwhm", fwhm)
    axes = (axes,) if is_int(axes) else tuple(axes)
    axes = tuple(_axis("gaussian", a) for a in axes)
    if len(set(axes)) != len(axes):
        raise ValueError(f"gaussian: axes must not repeat, {axes!r}")
    sigma = fwhm * _FWHM_TO_SIGMA
    fn = lambda m, N: np.exp(-0.5 * (2.0 * math.pi * m / N) ** 2 * sigma ** 2)
    return Filter([(a, fn) for a in axes], f"gaussian({fwhm:g}, axes={axes})")


def boxcar(width, axis):
    """A top-hat of `width` cells along `axis`.  For an odd integer width the Dirichlet kernel sin(pi m w / N) / (w sin(pi m / N)),
    which is the periodic moving average over w cells exactly; for any other width sin(x) / x with x = pi m w / N.  1 at m = 0."""
    width = _positive("boxcar", "width", width)
    axis = _axis("boxcar", axis)
    odd = width == int(width) and int(width) % 2 == 1

    def fn(m, N):
        out = np.ones_like(m)
        nz = m > 0
        if odd:
            w = int(width)
            turns = (m[nz].astype(np.int64) * w) % (2 * N)            # sin(pi m w / N) from the integer m w mod 2 N: no angle beyond 2 pi
            out[nz] = np.sin(math.pi * turns / N) / (w * np.sin(math.pi * m[nz] / N))
        else:
            x = math.pi * m[nz] * width / N
            out[nz] = np.where(x > 0, np.sin(x) / np.where(x > 0, x, 1.0), 1.0)
        return out
    return Filter([(axis, fn)], f"boxcar({width:g}, axis={axis})")


def spherical_tophat(R):
    """A sphere of radius `R` cells: 3 (sin x - x cos x) / x^3, x = 2 pi |m| R / N; radial."""
    R = _positive("spherical_tophat", "R", R)

    def fn(k, N):
        x = 2.0 * math.pi * k * R / N
        small = x < 0.1
        xs = np.where(small, 1.0, x)
        x2 = x * x
        series = 1.0 - x2 / 10.0 + x2 * x2 / 280.0 - x2 * x2 * x2 / 15120.0      # (the next term is below 1e-16 for x < 0.1)
        return np.where(small, series, 3.0 * (np.sin(xs) - xs * np.cos(xs)) / xs ** 3)
    return Filter([(3, fn)], f"spherical_tophat({R:g})")


def sharp_k(m_max):
    """1 where |m|^2 <= floor(m_max^2), else 0: a sharp cut in Fourier space (a projection); radial."""
    m_max = _positive("sharp_k", "m_max", m_max)
    cut = math.floor(m_max * m_max)
    fn = lambda k, N: (np.arange(k.size) <= cut).astype(np.float64)            # (the radial table is indexed by |m|^2 itself)
    return Filter([(3, fn)], f"sharp_k({m_max:g})")


def telescope(fwhm_perp, width_los, los_axis=2):
    """An interferometer's resolution: a Gaussian beam of FWHM `fwhm_perp` cells on the two axes across the sky times a top-hat of
    `width_los` cells along the line of sight, `los_axis`."""
    los_axis = _axis("telescope", los_axis)
    return gaussian(fwhm_perp, axes=tuple(a for a in (0, 1, 2) if a != los_axis)) * boxcar(width_los, los_axis)


class SmoothedField:
    """The result of :func:`smoothed_field`.

    From the library call.  ``stats``: the ten raw numbers, indexed by ``_capi.SMOOTH_*``: the finite and the non-finite cells, min,
    max, (sum g, sum g^2) of the field before the filter, sum h, and the central sums S2, S3, S4 = sum (h - mu)^p with mu = sum h /
    N^3.  ``edges`` and ``hist`` (uint64; None without bins): the cells with edges[b] <= h < edges[b + 1]; ``below`` and ``above``:
    the finite cells under the first edge, and at or over the last.  ``field``: h, (N, N, N), if it was asked for.

    Derived, with n = N^3.  ``mean`` = sum h / n; ``variance`` = S2 / n; ``skewness`` = (S3 / n) / (S2 / n)^(3/2); ``kurtosis`` = (S4 /
    n) / (S2 / n)^2 - 3 (the excess); ``min``, ``max``; ``pdf`` = hist / (n_finite x bin width), a density that integrates to the share
    of the cells inside the bins, at ``bin_centres``; ``input_mean``, ``input_variance``; ``n_nonfinite``.  A field without spread
    gives NaN for skewness and kurtosis; nothing is clipped."""

    def __init__(self, stats, N, edges=None, hist=None, kind="dtb", filter=None, subtract_mean=False, field=None):
        self.stats = np.array(stats, dtype=np.float64).ravel()
        if self.stats.size != _capi.SMOOTH_STATS:
            raise ValueError(f"SmoothedField: {_capi.SMOOTH_STATS} stats, not {self.stats.size}")
        self.N = int(N)
        if (edges is None) != (hist is None):
            raise ValueError("SmoothedField: edges and hist come together or not at all")
        self.edges = None if edges is None else np.array(edges, dtype=np.float64).ravel()
        full = None if hist is None else np.array(hist, dtype=np.uint64).ravel()
        if full is not None and (self.edges.size < 2 or full.size != self.edges.size + 1):
            raise ValueError(f"SmoothedField: {self.edges.size} edges go with {max(self.edges.size - 1, 0)} bins and two more counts, "
                             f"not {full.size}")
        self.hist = None if full is None else full[:-2]
        self.below = None if full is None else int(full[-2])
        self.above = None if full is None else int(full[-1])
        self.kind, self.filter, self.subtract_mean, self.field = kind, filter, bool(subtract_mean), field

    @property
    def n(self):
        return float(self.N) ** 3

    @property
    def n_finite(self):
        return int(self.stats[_capi.SMOOTH_N_FINITE])

    @property
    def n_nonfinite(self):
        return int(self.stats[_capi.SMOOTH_N_NONFINITE])

    @property
    def min(self):
        return float(self.stats[_capi.SMOOTH_MIN])

    @property
    def max(self):
        return float(self.stats[_capi.SMOOTH_MAX])

    @property
    def mean(self):
        return float(self.stats[_capi.SMOOTH_SUM]) / self.n

    @property
    def variance(self):
        return float(self.stats[_capi.SMOOTH_S2]) / self.n

    @property
    def skewness(self):
        v = self.variance
        return float(self.stats[_capi.SMOOTH_S3]) / self.n / v ** 1.5 if v > 0 else math.nan

    @property
    def kurtosis(self):
        v = self.variance
        return float(self.stats[_capi.SMOOTH_S4]) / self.n / (v * v) - 3.0 if v > 0 else math.nan

    @property
    def input_mean(self):
        return float(self.stats[_capi.SMOOTH_INPUT_SUM]) / self.n

    @property
    def input_variance(self):
        return float(self.stats[_capi.SMOOTH_INPUT_SUM2]) / self.n - self.input_mean ** 2

    @property
    def bin_centres(self):
        return None if self.edges is None else 0.5 * (self.edges[:-1] + self.edges[1:])

    @property
    def pdf(self):
        if self.hist is None:
            return None
        out = np.full(self.hist.size, np.nan)
        if self.n_finite > 0:
            out = self.hist.astype(np.float64) / (float(self.n_finite) * np.diff(self.edges))
        return out

    def log_line(self):
        """The line of the log file (one per step)."""
        what = "identity" if self.filter is None else getattr(self.filter, "label", str(self.filter))
        head = (f"Smoothed field ({self.kind}, {what}{', mean removed' if self.subtract_mean else ''}): mean {self.mean:.6e}, "
                f"variance {self.variance:.6e}, skewness {self.skewness:.4f}, kurtosis {self.kurtosis:.4f}, min {self.min:.6e}, "
                f"max {self.max:.6e}; input variance {self.input_variance:.6e}")
        if self.n_nonfinite:
            head += f"; {self.n_nonfinite:n} non-finite cells"
        if self.hist is not None:
            head += f"; {self.hist.size} bins hold {int(self.hist.sum()):n} cells"
        return head

    def __repr__(self):
        return f"<SmoothedField: {self.log_line()}>"


def _edges(who, bins):
    """None; an int n in [1, 4096] (edges follow the field's range: two library calls); or 2 ... 4097 finite, strictly ascending edges"""
    if bins is None:
        return None
    if isinstance(bins, (bool, np.bool_)):
        raise ValueError(f"{who}: bins must be None, an int or an array of edges, not a bool")
    if is_int(bins):
        if not 1 <= bins <= _capi.SMOOTH_MAX_BINS:
            raise ValueError(f"{who}: bins as an int must be in [1, {_capi.SMOOTH_MAX_BINS}], not {bins}")
        return int(bins)
    try:
        e = np.array(bins, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: bins must be None, an int or an array of edges, not {bins!r}") from None
    if e.ndim != 1 or not 2 <= e.size <= _capi.SMOOTH_MAX_BINS + 1:
        raise ValueError(f"{who}: bins must be a one-dimensional array of 2 ... {_capi.SMOOTH_MAX_BINS + 1} edges")
    if not np.all(np.isfinite(e)):
        raise ValueError(f"{who}: the edges of bins must be finite")
    if np.any(np.diff(e) <= 0):
        raise ValueError(f"{who}: the edges of bins must be strictly ascending")
    return e


def edges_for_range(who, n, lo, hi):
    """n equal bins that hold every cell of a field with the finite range [lo, hi]: the last edge is the next double above hi (a
    cell AT the last edge counts as above); a field without spread gets [lo - 1/2, lo + 1/2]"""
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f"{who}: bins as an int needs a finite cell to take the range from")
    if not hi > lo:
        lo, hi = lo - 0.5, lo + 0.5
    e = np.linspace(lo, hi, int(n) + 1)
    e[-1] = np.nextafter(hi, math.inf)
    if np.any(np.diff(e) <= 0):
        raise ValueError(f"{who}: the range [{lo!r}, {hi!r}] is too narrow for {n} bins")
    return e


def smoothing_spec(who, N, kind='dtb', filter=None, subtract_mean=False, bins=None, scale=1.0, t_gamma=0.0, into=None,
                   return_field=False):
    """The keywords of :func:`smoothed_field` checked and completed for a mesh of N cells a side, as a dict (N = None: checked
    only).  Raises ValueError -- before any device call -- for what the library would refuse."""
    _check_kind(who, kind)
    if filter is not None and not isinstance(filter, Filter):
        raise ValueError(f"{who}: filter must be None or a Filter (gaussian, boxcar, spherical_tophat, sharp_k, telescope and their "
                         f"products), not {type(filter).__name__}")
    check_flag(who, "subtract_mean", subtract_mean)
    check_flag(who, "return_field", return_field)
    e = _edges(who, bins)
    check_scale(who, scale)
    check_t_gamma(who, t_gamma)
    if into is not None and (not is_int(into) or not 0 <= into < _capi.GRID_COUNT):
        raise ValueError(f"{who}: into must be None or a grid selector 0 ... {_capi.GRID_COUNT - 1} (_capi.GRID_*), not {into!r}")
    if N is None:
        return None
    check_mesh(who, N, MESH_TRANSFORM)
    tables = (None, None, None, None) if filter is None else filter.tables(N)
    for w in tables:
        if w is not None and not np.all(np.isfinite(w)):
            raise ValueError(f"{who}: the filter {filter!r} has a non-finite entry at N = {N}")
    return dict(N=int(N), kind=kind, filter=filter, tables=tables, subtract_mean=bool(subtract_mean), bins=e, scale=float(scale),
                t_gamma=float(t_gamma), into=None if into is None else int(into), return_field=bool(return_field))


def smoothed_field(field=None, *, kind='dtb', filter=None, subtract_mean=False, bins=None, scale=1.0, t_gamma=0.0, into=None,
                   return_field=False):
    """A field multiplied by `filter` in Fourier space, with its one-point statistics: a :class:`SmoothedField`.

    ``field``: an (N, N, N) host array for the mesh of ``device_init``; it is uploaded to the device's ionised-fraction grid, which a
    C2Ray object that keeps its grids there is told beforehand, and analysed as it is (``kind`` 'xh', which the default stands for
    here) or as 1 - field ('xhi').  ``field`` = None: the device grids are analysed where they lie, nothing is uploaded, and ``kind``
    selects what is formed from them as in :func:`pyc2ray_amd.powerspec.power_spectrum`: 'xh', 'xhi', 'density', 'hi' / 'dtb' with
    ``scale`` and ``t_gamma``.
    ``filter``: a :class:`Filter` (None: the identity, a round trip through the transform).  ``subtract_mean``: the mode n = 0 is
    removed, as an interferometer removes it.  ``bins``: None for no histogram; an array of finite, strictly ascending edges (at most
    4097) for the cells with edges[b] <= h < edges[b + 1], one library call; or an int n for n equal bins over the range of the
    result -- which is not known before the call, so TWO library calls are made: one without a histogram for min and max, and the
    same again with the edges from them (both on the device; the second returns the same field).  ``into``: a grid selector
    (``_capi.GRID_*``): the result is written into that device grid, where ``mfp_distribution``, ``region_sizes``, ``topology`` and
    ``granulometry`` take it by the selector; it may be a grid the kind reads.  ``return_field``: download the result as well."""
    who = "smoothed_field"
    if field is not None:
        field = host_field(who, "field", field)
        N = field.shape[0]
        if kind not in ("dtb", "xh", "xhi"):
            raise ValueError(f"{who}: a host field is analysed as kind 'xh' or 'xhi', not {kind!r} (the other kinds go with field=None)")
        kind = "xh" if kind == "dtb" else kind
    else:
        N = None
    kw = dict(kind=kind, filter=filter, subtract_mean=subtract_mean, bins=bins, scale=scale, t_gamma=t_gamma, into=into,
              return_field=return_field)
    spec = smoothing_spec(who, N, **kw)
    if not cuda_is_init():
        raise RuntimeError("GPU not initialized. Please initialize it by calling device_init(N)")
    lib = load_asora()
    if field is not None:
        _residency.reclaim()              # this call overwrites device grids a resident C2Ray object may be relying on
        lib.grid_to_device(_capi.GRID_XH, np.asarray(field, dtype=np.float64))
    else:
        if getattr(lib, "_N", None) is None:
            raise RuntimeError(f"{who}: field=None needs a device initialised through device_init (the mesh size)")
        if into is not None:
            _residency.reclaim()          # (a grid is about to be overwritten)
        spec = smoothing_spec(who, int(lib._N), **kw)
    return smoothing_on_device(lib, spec, who)


def smoothing_on_device(lib, spec, who="smoothed_field"):
    """The library call (two with ``bins`` an int) for a checked `spec` (smoothing_spec) on the device grids, as a
    :class:`SmoothedField`."""
    w_i, w_j, w_k, w_r = spec["tables"]
    call = lambda edges, into, field: lib.smooth_field(_KINDS[spec["kind"]], spec["scale"], spec["t_gamma"], w_i=w_i, w_j=w_j, w_k=w_k,
                                                       w_r=w_r, subtract_mean=spec["subtract_mean"], edges=edges, dst_grid=into,
                                                       field=field)
    edges = spec["bins"]
    if isinstance(edges, int):
        first = call(None, None, False)["stats"]
        edges = edges_for_range(who, edges, float(first[_capi.SMOOTH_MIN]), float(first[_capi.SMOOTH_MAX]))
    got = call(edges, spec["into"], spec["return_field"])
    return SmoothedField(got["stats"], spec["N"], edges=edges, hist=got["hist"], kind=spec["kind"], filter=spec["filter"],
                         subtract_mean=spec["subtract_mean"], field=got["field"])
