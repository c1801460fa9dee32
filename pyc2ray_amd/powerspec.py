"""The 21-cm power spectrum: differential brightness temperature, its spherically averaged power spectrum, cross-spectra and the
correlation coefficient.

The first statistic anyone computes from a reionisation run, next to the morphological descriptions of the ionised field
(:mod:`pyc2ray_amd.bubbles`, :mod:`pyc2ray_amd.regions`, :mod:`pyc2ray_amd.topology`, :mod:`pyc2ray_amd.granulometry`).  On the CPU
that is three N^3 downloads and ``numpy.fft`` per time step (``tools21cm.power_spectrum_1d``, ``cross_power_spectrum_1d``).
:func:`power_spectrum` runs it on the device (``libasora.power_spectrum``): the field -- the ionised or neutral fraction, the density
contrast, the neutral density or the brightness temperature with or without the spin-temperature factor -- is formed from the device
grids inside the first pass of a hand-written FP64 real-to-complex transform, and the modes are binned in shells of |n| by a kernel
whose sums have a fixed order, so grids that live on the device are analysed where they lie and the same call returns the same bits.
``C2Ray.power_spectrum()`` does that for the current state of a run.
"""
import math

import numpy as np

from . import _capi, _residency
from .asora_core import cuda_is_init
from .load_extensions import load_asora
from ._fieldspec import MESH_TRANSFORM, check_flag, check_mesh, check_scale, check_t_gamma, host_field, is_int, is_real

__all__ = ['PowerSpectrum', 'power_spectrum']

_KINDS = {"xh": _capi.PS_XH, "xhi": _capi.PS_XHI, "density": _capi.PS_DENSITY, "hi": _capi.PS_HI, "dtb": _capi.PS_HI}
_MAX_THRESHOLD = 2.0 ** 32 - 1.0


def _nan_divide(a, b):
    out = np.full(np.shape(a), np.nan)
    np.divide(a, b, out=out, where=np.asarray(b) != 0)
    return out


class PowerSpectrum:
    """The result of :func:`power_spectrum`.  Wave numbers are in units of 2 pi / L and powers in units of L^3, with L =
    ``box_len`` the side of the box in the caller's units (None: L = N, lengths in cells).

    From the library call.  ``edges`` (in units of the fundamental mode, ascending) and ``thresholds`` = ceil(edges^2): a mode n
    with folded integer components belongs to bin b if thresholds[b] <= |n|^2 < thresholds[b + 1], so a mode exactly on an edge
    goes to the upper bin.  ``n_modes`` (uint64): the modes of each bin, conjugate partners counted; ``sum_k``: the sum of their
    |n|; ``sum_aa``: the sum of |ahat|^2 of the unnormalised transform of field a; with a second field ``sum_bb`` and ``sum_ab``,
    the sum of Re(ahat conj(bhat)) (else None).  ``moments`` / ``moments_b``: (sum g, sum g^2) over the cells.  ``field`` and
    ``modes``: the formed field a, (N, N, N), and its transform, (N, N, N // 2 + 1) as ``numpy.fft.rfftn`` lays it out, if they
    were asked for.

    Derived.  ``k`` = 2 pi / L times the mean |n| of a bin; ``P`` = L^3 / N^6 sum_aa / n_modes; ``Delta2`` = k^3 P / (2 pi^2);
    ``P_b``, ``P_cross`` and ``r`` = P_cross / sqrt(P P_b) with a second field (else None); ``mean``, ``variance`` (and ``mean_b``,
    ``variance_b``) from the moments; ``parseval_residual``: (the binned power / N^3) / (sum g^2 - (sum g)^2 / N^3) - 1, which is
    rounding when the bins hold every mode but n = 0, and minus the share of the variance they leave out otherwise.  Empty bins
    give NaN; nothing is clipped."""

    def __init__(self, edges, n_modes, sum_k, sum_aa, moments, N, sum_bb=None, sum_ab=None, moments_b=None, box_len=None, kind="dtb",
                 kind_b=None, field=None, modes=None):
        self.edges = np.array(edges, dtype=np.float64).ravel()
        self.n_modes = np.array(n_modes, dtype=np.uint64).ravel()
        self.sum_k = np.array(sum_k, dtype=np.float64).ravel()
        self.sum_aa = np.array(sum_aa, dtype=np.float64).ravel()
        nb = self.edges.size - 1
        if nb < 1 or not (self.n_modes.size == self.sum_k.size == self.sum_aa.size == nb):
            raise ValueError(f"PowerSpectrum: {self.edges.size} edges go with {max(nb, 0)} bins >= 1, not {self.n_modes.size}, "
                             f"{self.sum_k.size}, {self.sum_aa.size}")
        if (sum_bb is None) != (sum_ab is None) or (sum_bb is None) != (moments_b is None):
            raise ValueError("PowerSpectrum: sum_bb, sum_ab and moments_b come together or not at all")
        self.sum_bb = None if sum_bb is None else np.array(sum_bb, dtype=np.float64).ravel()
        self.sum_ab = None if sum_ab is None else np.array(sum_ab, dtype=np.float64).ravel()
        if self.sum_bb is not None and not (self.sum_bb.size == self.sum_ab.size == nb):
            raise ValueError(f"PowerSpectrum: sum_bb and sum_ab must have {nb} bins")
        self.moments = np.array(moments, dtype=np.float64).ravel()
        self.moments_b = None if moments_b is None else np.array(moments_b, dtype=np.float64).ravel()
        for m in (self.moments, self.moments_b):
            if m is not None and m.size != 2:
                raise ValueError(f"PowerSpectrum: 2 moments, not {m.size}")
        self.N = int(N)
        self.box_len = None if box_len is None else float(box_len)
        self.kind, self.kind_b = kind, kind_b
        self.field, self.modes = field, modes

    @property
    def thresholds(self):
        return _edges_to_thresholds(self.edges)

    @property
    def L(self):
        return float(self.N) if self.box_len is None else self.box_len

    @property
    def cross(self):
        return self.sum_bb is not None

    @property
    def k(self):
        return 2.0 * math.pi / self.L * _nan_divide(self.sum_k, self.n_modes.astype(np.float64))

    def _power(self, sums):
        return self.L ** 3 / float(self.N) ** 6 * _nan_divide(sums, self.n_modes.astype(np.float64))

    @property
    def P(self):
        return self._power(self.sum_aa)

    @property
    def Delta2(self):
        return self.k ** 3 * self.P / (2.0 * math.pi ** 2)

    @property
    def P_b(self):
        return self._power(self.sum_bb) if self.cross else None

    @property
    def P_cross(self):
        return self._power(self.sum_ab) if self.cross else None

    @property
    def r(self):
        if not self.cross:
            return None
        with np.errstate(invalid="ignore"):
            return _nan_divide(self.sum_ab, np.sqrt(self.sum_aa * self.sum_bb))

    @staticmethod
    def _mean(m, N):
        return float(m[0]) / float(N) ** 3

    @property
    def mean(self):
        return self._mean(self.moments, self.N)

    @property
    def variance(self):
        return float(self.moments[1]) / float(self.N) ** 3 - self.mean ** 2

    @property
    def mean_b(self):
        return self._mean(self.moments_b, self.N) if self.cross else None

    @property
    def variance_b(self):
        return float(self.moments_b[1]) / float(self.N) ** 3 - self.mean_b ** 2 if self.cross else None

    @property
    def parseval_residual(self):
        n3 = float(self.N) ** 3
        spread = float(self.moments[1]) - float(self.moments[0]) ** 2 / n3
        return float(self.sum_aa.sum()) / n3 / spread - 1.0 if spread != 0 else math.nan

    def log_line(self):
        """The line of the log file (one per step)."""
        what = self.kind if not self.cross else f"{self.kind} x {self.kind_b}"
        unit = "cells" if self.box_len is None else "units of box_len"
        d2 = self.Delta2
        head = (f"Power spectrum ({what}, {self.n_modes.size} bins to |n| = {self.edges[-1]:g}, L = {self.L:g} {unit}): "
                f"{int(self.n_modes.sum()):n} modes, mean {self.mean:.6e}, variance {self.variance:.6e}")
        if np.all(np.isnan(d2)):
            return head + "; no mode in any bin"
        peak = int(np.nanargmax(d2))
        tail = f"; largest Delta2 {d2[peak]:.6e} at k = {self.k[peak]:.4e}"
        if self.cross:
            tail += f", r there {self.r[peak]:.4f}"
        return head + tail

    def __repr__(self):
        return f"<PowerSpectrum: {self.log_line()}>"


def _check_kind(who, kind):
    if not isinstance(kind, str) or kind not in _KINDS:
        raise ValueError(f"{who}: kind must be one of {', '.join(repr(k) for k in _KINDS)}, not {kind!r}")


def _edges_to_thresholds(edges):
    """ceil(edge^2) formed in double, within [1, 2^32 - 1]: the integers the device compares |n|^2 with."""
    e = np.asarray(edges, dtype=np.float64)
    return np.clip(np.ceil(e * e), 1.0, _MAX_THRESHOLD).astype(np.uint32)


def _edges(who, N, bins):
    """None: b + 0.5, b = 0 ... max(1, min(N // 2, 256)) (needs N); an int n: n equal bins over [0.5, max(1, N // 2) + 0.5] (needs N);
    else an array of finite, > 0, strictly ascending edges."""
    if bins is None:
        return None if N is None else np.arange(0, max(1, min(N // 2, _capi.BUBBLE_MAX_BINS)) + 1, dtype=np.float64) + 0.5
    if isinstance(bins, (bool, np.bool_)):
        raise ValueError(f"{who}: bins must be None, an int or an array of edges, not a bool")
    if is_int(bins):
        if not 1 <= bins <= _capi.BUBBLE_MAX_BINS:
            raise ValueError(f"{who}: bins as an int must be in [1, {_capi.BUBBLE_MAX_BINS}], not {bins}")
        return None if N is None else np.linspace(0.5, max(1, N // 2) + 0.5, int(bins) + 1)
    try:
        e = np.array(bins, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: bins must be None, an int or an array of edges, not {bins!r}") from None
    if e.ndim != 1 or not 2 <= e.size <= _capi.BUBBLE_MAX_BINS + 1:
        raise ValueError(f"{who}: bins must be a one-dimensional array of 2 ... {_capi.BUBBLE_MAX_BINS + 1} edges")
    if not np.all(np.isfinite(e)):
        raise ValueError(f"{who}: the edges of bins must be finite")
    if not e[0] > 0:
        raise ValueError(f"{who}: the edges of bins must be > 0 (the mode n = 0 is never binned)")
    if np.any(np.diff(e) <= 0):
        raise ValueError(f"{who}: the edges of bins must be strictly ascending")
    return e


def powerspec_spec(who, N, kind='dtb', kind_b=None, bins=None, box_len=None, scale=1.0, t_gamma=0.0, return_field=False,
                   return_modes=False):
    """The keywords of :func:`power_spectrum` checked and completed for a mesh of N cells a side, as a dict (N = None: checked only).
    Raises ValueError -- before any device call -- for what the library would refuse."""
    _check_kind(who, kind)
    if kind_b is not None and (not isinstance(kind_b, str) or kind_b not in _KINDS):
        raise ValueError(f"{who}: kind_b must be None or one of {', '.join(repr(k) for k in _KINDS)}, not {kind_b!r}")
    e = _edges(who, N, bins)
    if box_len is not None and (not is_real(box_len) or not (math.isfinite(box_len) and box_len > 0)):
        raise ValueError(f"{who}: box_len must be None or a finite number > 0, not {box_len!r}")
    check_scale(who, scale)
    check_t_gamma(who, t_gamma)
    check_flag(who, "return_field", return_field)
    check_flag(who, "return_modes", return_modes)
    if N is None:                          # (only the checks: the mesh size is the device's, asked for afterwards)
        return None
    check_mesh(who, N, MESH_TRANSFORM)
    return dict(N=int(N), kind=kind, kind_b=kind_b, edges=e, thresholds=_edges_to_thresholds(e),
                box_len=None if box_len is None else float(box_len), scale=float(scale), t_gamma=float(t_gamma),
                return_field=bool(return_field), return_modes=bool(return_modes))


def power_spectrum(field=None, field_b=None, *, kind='dtb', kind_b=None, bins=None, box_len=None, scale=1.0, t_gamma=0.0,
                   return_field=False, return_modes=False):
    """The spherically averaged power spectrum of a field, or of two and their cross-spectrum, a :class:`PowerSpectrum`.

    ``field``: an (N, N, N) host array for the mesh of ``device_init``; it is uploaded to the device's ionised-fraction grid, which a
    C2Ray object that keeps its grids there is told beforehand, and analysed as it is (``kind`` 'xh', which the default stands for
    here) or as 1 - field ('xhi').  ``field_b``: a second host array, uploaded to the density grid and analysed as field_b / its mean
    (``kind_b`` 'density', the only one).  ``field`` = None: the device grids are analysed where they lie, nothing is uploaded, and
    ``kind`` / ``kind_b`` select what is formed from them: 'xh' the ionised fraction x, 'xhi' 1 - x, 'density' n / nbar, 'hi' and
    'dtb' ``scale`` (1 - x) n / nbar, times 1 - ``t_gamma`` / T with ``t_gamma`` > 0 (the CMB temperature at the redshift; T the
    temperature grid: the spin temperature coupled to the kinetic one).  The brightness temperature is that with the cosmological
    prefactor as ``scale``, which ``C2Ray.power_spectrum`` supplies.
    ``bins``: None for unit-width bins with the edges b + 0.5, b = 0 ... max(1, min(N // 2, 256)); an int n for n equal bins over
    [0.5, max(1, N // 2) + 0.5]; or an array of finite, > 0, strictly ascending edges (at most 257), all in units of the fundamental
    mode 2 pi / L.  ``box_len``: L in the caller's units (None: N, lengths in cells).  ``return_field`` / ``return_modes``: download
    the formed field a / its transform as well."""
    who = "power_spectrum"
    if field is not None:
        field = host_field(who, "field", field)
        N = field.shape[0]
        if kind not in ("dtb", "xh", "xhi"):
            raise ValueError(f"{who}: a host field is analysed as kind 'xh' or 'xhi', not {kind!r} (the other kinds go with field=None)")
        kind = "xh" if kind == "dtb" else kind
        if field_b is not None:
            field_b = host_field(who, "field_b", field_b)
            if field_b.shape != field.shape:
                raise ValueError(f"{who}: field_b must have the shape of field")
            if kind_b not in (None, "density"):
                raise ValueError(f"{who}: a host field_b is analysed as kind_b 'density', not {kind_b!r}")
            kind_b = "density"
        elif kind_b is not None:
            raise ValueError(f"{who}: kind_b goes with field_b, or with field=None")
    else:
        if field_b is not None:
            raise ValueError(f"{who}: field_b goes with field")
        N = None
    kw = dict(kind=kind, kind_b=kind_b, bins=bins, box_len=box_len, scale=scale, t_gamma=t_gamma, return_field=return_field,
              return_modes=return_modes)
    spec = powerspec_spec(who, N, **kw)
    if not cuda_is_init():
        raise RuntimeError("GPU not initialized. Please initialize it by calling device_init(N)")
    lib = load_asora()
    if field is not None:
        _residency.reclaim()              # this call overwrites device grids a resident C2Ray object may be relying on
        lib.grid_to_device(_capi.GRID_XH, np.asarray(field, dtype=np.float64))
        if field_b is not None:
            lib.grid_to_device(_capi.GRID_NDENS, np.asarray(field_b, dtype=np.float64))
    else:
        if getattr(lib, "_N", None) is None:
            raise RuntimeError(f"{who}: field=None needs a device initialised through device_init (the mesh size)")
        spec = powerspec_spec(who, int(lib._N), **kw)
    return powerspec_on_device(lib, spec)


def powerspec_on_device(lib, spec):
    """The library call for a checked `spec` (powerspec_spec) on the device grids, as a :class:`PowerSpectrum`."""
    got = lib.power_spectrum(_KINDS[spec["kind"]], None if spec["kind_b"] is None else _KINDS[spec["kind_b"]], spec["scale"],
                             spec["t_gamma"], spec["thresholds"], field=spec["return_field"], modes=spec["return_modes"])
    return PowerSpectrum(spec["edges"], got["count"], got["sum_k"], got["sum_aa"], got["moments_a"], spec["N"], sum_bb=got["sum_bb"],
                         sum_ab=got["sum_ab"], moments_b=got["moments_b"], box_len=spec["box_len"], kind=spec["kind"],
                         kind_b=spec["kind_b"], field=got["field"], modes=got["modes"])
