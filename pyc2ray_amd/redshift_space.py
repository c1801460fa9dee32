"""The 21-cm signal in redshift space: the field moved along the line of sight by the peculiar velocity, and its power resolved in
direction -- P(k_perp, k_par), P(k, mu) and the multipoles P_0, P_2, P_4.

What an interferometer measures is neither in real space nor averaged over directions: peculiar velocities move the signal along
the line of sight, and the line of sight is a special axis.  On the CPU that is ``tools21cm.get_distorted_dt``, ``power_spectrum_2d``
and ``power_spectrum_mu`` after three N^3 downloads.  :func:`power_spectrum_los` runs it on the device
(``libasora.power_spectrum_los``): the field of :func:`pyc2ray_amd.powerspec.power_spectrum` is regridded line by line between its
displaced cell edges (the mesh-to-mesh scheme of Mao et al. 2012, number conserving), transformed by the same hand-written FP64
transform, and binned in two dimensions with Legendre-weighted sums, all in a fixed order: the same call returns the same bits.
:func:`redshift_space_field` returns the mapped cube alone, or leaves it in a device grid for the other analyses.
``C2Ray.power_spectrum_los()`` does that for the current state of a run with ``C2Ray.los_velocity``.
"""
import math

import numpy as np

from . import _capi, _residency
from .asora_core import cuda_is_init
from .load_extensions import load_asora
from ._fieldspec import MESH_TRANSFORM, analyse, check_flag, check_mesh, check_scale, check_t_gamma, host_field, is_int, is_real
from .powerspec import _KINDS, _check_kind, _edges, _edges_to_thresholds, _nan_divide

__all__ = ['AnisotropicSpectrum', 'power_spectrum_los', 'redshift_space_field']

BINNINGS = ("cylindrical", "mu", "multipoles")
_MAX_THRESHOLD = 2.0 ** 32 - 1.0
#: the default number of bins per dimension: 32 x 32 is all the library takes
DEFAULT_BINS = 32


class AnisotropicSpectrum:
    """The result of :func:`power_spectrum_los`.  Wave numbers are in units of 2 pi / L and powers in units of L^3, with L =
    ``box_len`` the side of the box in the caller's units (None: L = N, lengths in cells).

    From the library call.  ``binning``: 'cylindrical', 'mu' or 'multipoles'; ``edges_a`` and ``edges_b``: the edges of the first and
    the second index -- k_perp and k_par in units of the fundamental mode, or |n| and mu ('multipoles': mu from 0 to 1 in one bin);
    ``thr_a``, ``thr_b``: what the device compares with, ceil(edge^2) and, for mu, mu^2.  A mode exactly on an edge goes to the upper
    bin; mu = 1 belongs to the last bin of mu if its edge is above 1 (an int ``mu_bins`` and 'multipoles' make it so).  ``n_modes``
    (uint64), ``sum_1``, ``sum_2``, ``sum_aa``, ``sum_l2``, ``sum_l4``: (n_a, n_b) each, as include/asora_hip.h defines them;
    ``moments_real`` and ``moments_rs``: (sum, sum of squares) of the field before and after the mapping; ``los_axis``;
    ``velocity``: was the field mapped (False: real space); ``field`` and ``modes`` if they were asked for.

    Derived, (n_a, n_b) each.  'cylindrical': ``k_perp`` and ``k_par`` = 2 pi / L times the mean n_perp and n_par of a bin, ``k`` =
    their root sum of squares, ``mu`` = k_par / k.  'mu' and 'multipoles': ``k`` = 2 pi / L times the mean |n|, ``mu`` = the mean mu,
    ``k_par`` = k mu, ``k_perp`` = k sqrt(1 - mu^2).  ``P`` = L^3 / N^6 sum_aa / n_modes.  ``P0``, ``P2``, ``P4`` (with 'mu' and
    'multipoles'; (n_a,): the bins of mu added up; None with 'cylindrical'): (2 l + 1) L^3 / N^6 sum of |hhat|^2 L_l(mu) / modes,
    and ``k_multipoles`` the mean k of those modes.  ``mean_real``, ``variance_real``, ``mean_rs``, ``variance_rs``.  Empty bins give
    NaN; nothing is clipped."""

    def __init__(self, binning, edges_a, edges_b, n_modes, sum_1, sum_2, sum_aa, sum_l2, sum_l4, moments_real, moments_rs, N, los_axis=2,
                 velocity=False, box_len=None, kind="dtb", field=None, modes=None):
        if binning not in BINNINGS:
            raise ValueError(f"AnisotropicSpectrum: binning must be one of {BINNINGS}, not {binning!r}")
        self.binning = binning
        self.edges_a = np.array(edges_a, dtype=np.float64).ravel()
        self.edges_b = np.array(edges_b, dtype=np.float64).ravel()
        shape = (self.edges_a.size - 1, self.edges_b.size - 1)
        if shape[0] < 1 or shape[1] < 1:
            raise ValueError("AnisotropicSpectrum: two or more edges per index")
        self.n_modes = np.array(n_modes, dtype=np.uint64)
        arrays = {}
        for name, a in (("sum_1", sum_1), ("sum_2", sum_2), ("sum_aa", sum_aa), ("sum_l2", sum_l2), ("sum_l4", sum_l4)):
            arrays[name] = np.array(a, dtype=np.float64)
        if self.n_modes.shape != shape or any(a.shape != shape for a in arrays.values()):
            raise ValueError(f"AnisotropicSpectrum: {self.edges_a.size} and {self.edges_b.size} edges go with arrays of shape {shape}")
        self.sum_1, self.sum_2, self.sum_aa = arrays["sum_1"], arrays["sum_2"], arrays["sum_aa"]
        self.sum_l2, self.sum_l4 = arrays["sum_l2"], arrays["sum_l4"]
        self.moments_real = np.array(moments_real, dtype=np.float64).ravel()
        self.moments_rs = np.array(moments_rs, dtype=np.float64).ravel()
        if self.moments_real.size != 2 or self.moments_rs.size != 2:
            raise ValueError("AnisotropicSpectrum: 2 moments each")
        self.N, self.los_axis, self.velocity = int(N), int(los_axis), bool(velocity)
        self.box_len = None if box_len is None else float(box_len)
        self.kind, self.field, self.modes = kind, field, modes

    @property
    def L(self):
        return float(self.N) if self.box_len is None else self.box_len

    @property
    def _unit(self):
        return 2.0 * math.pi / self.L

    @property
    def _n(self):
        return self.n_modes.astype(np.float64)

    @property
    def k_perp(self):
        if self.binning == "cylindrical":
            return self._unit * _nan_divide(self.sum_1, self._n)
        with np.errstate(invalid="ignore"):
            return self.k * np.sqrt(np.maximum(1.0 - self.mu ** 2, 0.0))

    @property
    def k_par(self):
        if self.binning == "cylindrical":
            return self._unit * _nan_divide(self.sum_2, self._n)
        return self.k * self.mu

    @property
    def k(self):
        if self.binning == "cylindrical":
            return np.sqrt(self.k_perp ** 2 + self.k_par ** 2)
        return self._unit * _nan_divide(self.sum_1, self._n)

    @property
    def mu(self):
        if self.binning == "cylindrical":
            return _nan_divide(self.k_par, self.k)
        return _nan_divide(self.sum_2, self._n)

    @property
    def P(self):
        return self.L ** 3 / float(self.N) ** 6 * _nan_divide(self.sum_aa, self._n)

    def _multipole(self, ell, sums):
        if self.binning == "cylindrical":
            return None
        return (2 * ell + 1) * self.L ** 3 / float(self.N) ** 6 * _nan_divide(sums.sum(axis=1), self._n.sum(axis=1))

    @property
    def P0(self):
        return self._multipole(0, self.sum_aa)

    @property
    def P2(self):
        return self._multipole(2, self.sum_l2)

    @property
    def P4(self):
        return self._multipole(4, self.sum_l4)

    @property
    def k_multipoles(self):
        if self.binning == "cylindrical":
            return None
        return self._unit * _nan_divide(self.sum_1.sum(axis=1), self._n.sum(axis=1))

    def _mean(self, m):
        return float(m[0]) / float(self.N) ** 3

    def _variance(self, m):
        return float(m[1]) / float(self.N) ** 3 - self._mean(m) ** 2

    @property
    def mean_real(self):
        return self._mean(self.moments_real)

    @property
    def variance_real(self):
        return self._variance(self.moments_real)

    @property
    def mean_rs(self):
        return self._mean(self.moments_rs)

    @property
    def variance_rs(self):
        return self._variance(self.moments_rs)

    def log_line(self):
        """The line of the log file (one per step)."""
        space = "redshift space" if self.velocity else "real space: no velocity"
        unit = "cells" if self.box_len is None else "units of box_len"
        shape = self.n_modes.shape
        head = (f"Redshift-space spectrum ({self.kind}, {self.binning}, {shape[0]} x {shape[1]} bins, line of sight {self.los_axis}, "
                f"{space}, L = {self.L:g} {unit}): {int(self.n_modes.sum()):n} modes, mean {self.mean_rs:.6e}, variance "
                f"{self.variance_rs:.6e} (real space {self.variance_real:.6e})")
        if int(self.n_modes.sum()) == 0:
            return head + "; no mode in any bin"
        if self.binning == "cylindrical":
            p = self.P
            peak = np.unravel_index(int(np.nanargmax(p)), p.shape)
            return head + f"; largest P {p[peak]:.6e} at k_perp = {self.k_perp[peak]:.4e}, k_par = {self.k_par[peak]:.4e}"
        p0, p2 = self.P0, self.P2
        peak = int(np.nanargmax(p0))
        return head + f"; largest P0 {p0[peak]:.6e} at k = {self.k_multipoles[peak]:.4e}, P2 / P0 there {p2[peak] / p0[peak]:.4f}"

    def __repr__(self):
        return f"<AnisotropicSpectrum: {self.log_line()}>"


def _check_axis(who, los_axis):
    if not is_int(los_axis) or los_axis not in (0, 1, 2):
        raise ValueError(f"{who}: los_axis must be 0, 1 or 2, not {los_axis!r}")


def _axis_edges(who, name, N, bins):
    """The edges of k_perp or k_par: None for min(N // 2, 32) + 1 unit-width bins from 0, the first one [0, 0.5) (needs N); an int n
    for n equal bins over [0, max(1, N // 2) + 0.5] (needs N); else an array of finite, >= 0, strictly ascending edges."""
    limit = _capi.ANISO_MAX_BINS
    if bins is None:
        if N is None:
            return None
        top = max(1, min(N // 2, DEFAULT_BINS - 1))
        return np.r_[0.0, np.arange(0, top + 1, dtype=np.float64) + 0.5]
    if isinstance(bins, (bool, np.bool_)):
        raise ValueError(f"{who}: {name} must be None, an int or an array of edges, not a bool")
    if is_int(bins):
        if not 1 <= bins <= limit:
            raise ValueError(f"{who}: {name} as an int must be in [1, {limit}], not {bins}")
        return None if N is None else np.linspace(0.0, max(1, N // 2) + 0.5, int(bins) + 1)
    try:
        e = np.array(bins, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} must be None, an int or an array of edges, not {bins!r}") from None
    if e.ndim != 1 or not 2 <= e.size <= limit + 1:
        raise ValueError(f"{who}: {name} must be a one-dimensional array of 2 ... {limit + 1} edges")
    if not np.all(np.isfinite(e)) or not e[0] >= 0 or np.any(np.diff(e) <= 0):
        raise ValueError(f"{who}: the edges of {name} must be finite, >= 0 and strictly ascending")
    return e


def _mu_thresholds(who, mu_bins):
    """(edges of mu, thresholds on mu^2): None for 5 equal bins; an int n for n equal bins over [0, 1], mu = 1 in the last (its
    threshold is 2); else an array of finite, >= 0, strictly ascending edges of mu, squared as they are -- a last edge of exactly 1
    leaves mu = 1 out."""
    limit = _capi.ANISO_MAX_BINS
    if mu_bins is None:
        mu_bins = 5
    if isinstance(mu_bins, (bool, np.bool_)):
        raise ValueError(f"{who}: mu_bins must be None, an int or an array of edges, not a bool")
    if is_int(mu_bins):
        if not 1 <= mu_bins <= limit:
            raise ValueError(f"{who}: mu_bins as an int must be in [1, {limit}], not {mu_bins}")
        e = np.linspace(0.0, 1.0, int(mu_bins) + 1)
        thr = e * e
        thr[-1] = 2.0
        return e, thr
    try:
        e = np.array(mu_bins, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: mu_bins must be None, an int or an array of edges, not {mu_bins!r}") from None
    if e.ndim != 1 or not 2 <= e.size <= limit + 1:
        raise ValueError(f"{who}: mu_bins must be a one-dimensional array of 2 ... {limit + 1} edges")
    if not np.all(np.isfinite(e)) or not e[0] >= 0 or np.any(np.diff(e) <= 0):
        raise ValueError(f"{who}: the edges of mu_bins must be finite, >= 0 and strictly ascending")
    return e, e * e


def _squared_up(e):
    """ceil(edge^2) within [0, 2^32 - 1], as doubles: an integer m^2 is at or above it exactly when m is at or above the edge"""
    return np.clip(np.ceil(e * e), 0.0, _MAX_THRESHOLD)


def window_of(max_velocity, velocity_scale):
    """W as the library takes it: floor(max|v| |velocity_scale|) + 1"""
    return int(math.floor(float(max_velocity) * abs(float(velocity_scale)))) + 1


def _check_velocity(who, N, velocity, max_velocity, velocity_scale):
    """The velocity of a call: `velocity` a host array (checked, with its max |v|), or `max_velocity` the max |v| of one that is
    on the device already; both None: no velocity.  Returns (the array or None, max |v| or None)."""
    if not is_real(velocity_scale) or not math.isfinite(velocity_scale):
        raise ValueError(f"{who}: velocity_scale must be a finite number, not {velocity_scale!r}")
    if velocity is not None:
        if max_velocity is not None:
            raise ValueError(f"{who}: max_velocity goes with a velocity that is on the device already, not with velocity")
        velocity = host_field(who, "velocity", velocity)
        if N is not None and velocity.shape[0] != N:
            raise ValueError(f"{who}: velocity must have the shape ({N}, {N}, {N}) of the mesh, not {velocity.shape}")
        if not np.all(np.isfinite(velocity)):
            raise ValueError(f"{who}: velocity has a non-finite entry")
        max_velocity = float(np.max(np.abs(velocity))) if velocity.size else 0.0
    elif max_velocity is not None and (not is_real(max_velocity) or not (math.isfinite(max_velocity) and max_velocity >= 0)):
        raise ValueError(f"{who}: max_velocity must be a finite number >= 0, not {max_velocity!r}")
    if max_velocity is not None and N is not None:
        W = window_of(max_velocity, velocity_scale)
        if 2 * W + 1 > N:
            raise ValueError(f"{who}: max|v| |velocity_scale| = {max_velocity * abs(velocity_scale):g} cells needs a window of "
                             f"2 W + 1 = {2 * W + 1} cells, wider than the N = {N} cells of a line")
    return velocity, None if max_velocity is None else float(max_velocity)


def redshift_space_spec(who, N, kind='dtb', velocity=None, max_velocity=None, velocity_scale=1.0, los_axis=2, binning='cylindrical',
                        bins=None, bins_perp=None, bins_par=None, mu_bins=None, box_len=None, scale=1.0, t_gamma=0.0, into=None,
                        return_field=False, return_modes=False):
    """The keywords of :func:`power_spectrum_los` and :func:`redshift_space_field` checked and completed for a mesh of N cells a
    side, as a dict (N = None: checked only).  Raises ValueError -- before any device call -- for what the library would refuse."""
    _check_kind(who, kind)
    _check_axis(who, los_axis)
    if not isinstance(binning, str) or binning not in BINNINGS:
        raise ValueError(f"{who}: binning must be one of {', '.join(repr(b) for b in BINNINGS)}, not {binning!r}")
    velocity, max_velocity = _check_velocity(who, N, velocity, max_velocity, velocity_scale)
    if binning == "cylindrical":
        if bins is not None or mu_bins is not None:
            raise ValueError(f"{who}: binning 'cylindrical' takes bins_perp and bins_par, not bins or mu_bins")
        edges_a, edges_b = _axis_edges(who, "bins_perp", N, bins_perp), _axis_edges(who, "bins_par", N, bins_par)
    else:
        if bins_perp is not None or bins_par is not None:
            raise ValueError(f"{who}: binning {binning!r} takes bins{' and mu_bins' if binning == 'mu' else ''}, not bins_perp or bins_par")
        if binning == "multipoles" and mu_bins is not None:
            raise ValueError(f"{who}: binning 'multipoles' has one bin of mu, from 0 to 1: mu_bins is for binning 'mu'")
        if is_int(bins) and not isinstance(bins, (bool, np.bool_)) and bins > _capi.ANISO_MAX_BINS:
            raise ValueError(f"{who}: bins as an int must be in [1, {_capi.ANISO_MAX_BINS}], not {bins}")
        if bins is None and N is not None:
            edges_a = np.arange(0, max(1, min(N // 2, DEFAULT_BINS)) + 1, dtype=np.float64) + 0.5
        else:
            edges_a = _edges(who, N, bins)
    if box_len is not None and (not is_real(box_len) or not (math.isfinite(box_len) and box_len > 0)):
        raise ValueError(f"{who}: box_len must be None or a finite number > 0, not {box_len!r}")
    check_scale(who, scale)
    check_t_gamma(who, t_gamma)
    if into is not None and (not is_int(into) or not 0 <= into < _capi.GRID_COUNT):
        raise ValueError(f"{who}: into must be None or a grid selector 0 ... {_capi.GRID_COUNT - 1} (_capi.GRID_*), not {into!r}")
    check_flag(who, "return_field", return_field)
    check_flag(who, "return_modes", return_modes)
    if binning == "mu":
        edges_b, thr_b = _mu_thresholds(who, mu_bins)
    elif binning == "multipoles":
        edges_b, thr_b = np.array([0.0, 1.0]), np.array([0.0, 2.0])
    if N is None:                          # (only the checks: the mesh size is the device's, asked for afterwards)
        return None
    check_mesh(who, N, MESH_TRANSFORM)
    if binning == "cylindrical":
        thr_a, thr_b, mode = _squared_up(edges_a).astype(np.uint32), _squared_up(edges_b), _capi.ANISO_CYLINDRICAL
    else:
        thr_a, mode = _edges_to_thresholds(edges_a), _capi.ANISO_MU
    n_a, n_b = thr_a.size - 1, thr_b.size - 1
    if n_a * n_b > _capi.ANISO_MAX_BINS:
        raise ValueError(f"{who}: {n_a} x {n_b} bins are more than the {_capi.ANISO_MAX_BINS} of the library")
    return dict(N=int(N), kind=kind, velocity=velocity, max_velocity=max_velocity,
                velocity_scale=None if max_velocity is None else float(velocity_scale), los_axis=int(los_axis), binning=binning, mode=mode,
                edges_a=edges_a, edges_b=edges_b, thr_a=thr_a, thr_b=np.asarray(thr_b, dtype=np.float64),
                box_len=None if box_len is None else float(box_len), scale=float(scale), t_gamma=float(t_gamma),
                into=None if into is None else int(into), return_field=bool(return_field), return_modes=bool(return_modes))


def _host_kind(who, field, kind):
    if field is not None and kind not in ("dtb", "xh", "xhi"):
        raise ValueError(f"{who}: a host field is analysed as kind 'xh' or 'xhi', not {kind!r} (the other kinds go with field=None)")
    return "xh" if field is not None and kind == "dtb" else kind


def power_spectrum_los(field=None, *, velocity=None, velocity_scale=1.0, los_axis=2, binning='cylindrical', bins=None, bins_perp=None,
                       bins_par=None, mu_bins=None, kind='dtb', box_len=None, scale=1.0, t_gamma=0.0, return_field=False,
                       return_modes=False):
    """The power spectrum of a field in redshift space, resolved in direction: an :class:`AnisotropicSpectrum`.

    ``field``: an (N, N, N) host array for the mesh of ``device_init``, uploaded to the device's ionised-fraction grid and analysed as
    it is (``kind`` 'xh', which the default stands for here) or as 1 - field ('xhi'); None: the device grids are analysed where they
    lie and ``kind`` selects what is formed from them, with ``scale`` and ``t_gamma``, as in
    :func:`pyc2ray_amd.powerspec.power_spectrum`.  ``velocity``: an (N, N, N) array, the velocity along ``los_axis`` (0, 1 or 2);
    ``velocity_scale`` converts it to cells (``C2Ray.velocity_scale()`` for proper km/s); a cell with a positive velocity moves
    towards larger indices.  None: the field stays in real space.  max|velocity| |velocity_scale| may not reach (N - 1) / 2 cells.
    ``binning``: 'cylindrical' for P(k_perp, k_par) with ``bins_perp`` and ``bins_par`` (None: unit-width bins from 0, 32 at the
    most; an int n: n equal bins; or an array of edges >= 0), 'mu' for P(k, mu) with ``bins`` (as in ``power_spectrum``; None: at
    most 32 unit-width bins) and ``mu_bins`` (None: 5; an int n: n equal bins of mu over [0, 1]; or an array of edges of mu, where
    a last edge of exactly 1 leaves mu = 1 out), 'multipoles' for P_0, P_2, P_4 in the bins of ``bins``; all edges of k in units of
    the fundamental mode 2 pi / L, at most 1024 bins in all.  ``box_len``: L in the caller's units (None: N).  ``return_field`` /
    ``return_modes``: download the mapped field / its transform as well."""
    who = "power_spectrum_los"
    kw = dict(kind=_host_kind(who, field, kind), velocity=velocity, velocity_scale=velocity_scale, los_axis=los_axis, binning=binning,
              bins=bins, bins_perp=bins_perp, bins_par=bins_par, mu_bins=mu_bins, box_len=box_len, scale=scale, t_gamma=t_gamma,
              return_field=return_field, return_modes=return_modes)
    return analyse(who, field, None, redshift_space_spec, kw, lambda lib, grid, spec: spectrum_on_device(lib, spec), cuda_is_init,
                   load_asora)


def redshift_space_field(field=None, *, velocity=None, velocity_scale=1.0, los_axis=2, kind='dtb', scale=1.0, t_gamma=0.0, into=None):
    """The field of :func:`power_spectrum_los` moved into redshift space, without the spectrum: the (N, N, N) cube, or with ``into``
    (a grid selector, ``_capi.GRID_*``) None, the result being written into that device grid, where ``smoothed_field``,
    ``mfp_distribution``, ``region_sizes``, ``topology`` and ``granulometry`` take it; it may be a grid the kind reads."""
    who = "redshift_space_field"
    kw = dict(kind=_host_kind(who, field, kind), velocity=velocity, velocity_scale=velocity_scale, los_axis=los_axis, scale=scale,
              t_gamma=t_gamma, into=into)

    def on_device(lib, grid, spec):
        if spec["into"] is not None:
            _residency.reclaim()          # (a grid is about to be overwritten)
        return field_on_device(lib, spec)
    return analyse(who, field, None, redshift_space_spec, kw, on_device, cuda_is_init, load_asora)


def _velocity_scale_on_device(lib, spec):
    """Upload the velocity of a checked `spec` if it brings one; the velocity_scale of the library call (None: no velocity)."""
    if spec["velocity"] is not None:
        _residency.reclaim()              # (the library has one velocity: a C2Ray object that keeps its own there uploads it again)
        lib.los_velocity_to_device(np.asarray(spec["velocity"], dtype=np.float64))
    return spec["velocity_scale"]


def spectrum_on_device(lib, spec):
    """The library call for a checked `spec` (redshift_space_spec) on the device grids, as an :class:`AnisotropicSpectrum`."""
    vscale = _velocity_scale_on_device(lib, spec)
    got = lib.power_spectrum_los(_KINDS[spec["kind"]], spec["scale"], spec["t_gamma"], spec["los_axis"], vscale, spec["mode"],
                                 spec["thr_a"], spec["thr_b"], field=spec["return_field"], modes=spec["return_modes"])
    return AnisotropicSpectrum(spec["binning"], spec["edges_a"], spec["edges_b"], got["count"], got["sum_1"], got["sum_2"], got["sum_aa"],
                               got["sum_l2"], got["sum_l4"], got["moments_real"], got["moments_rs"], spec["N"], los_axis=spec["los_axis"],
                               velocity=vscale is not None, box_len=spec["box_len"], kind=spec["kind"], field=got["field"],
                               modes=got["modes"])


def field_on_device(lib, spec):
    """The library call of :func:`redshift_space_field` for a checked `spec`: the cube, or None with ``into``."""
    vscale = _velocity_scale_on_device(lib, spec)
    got = lib.redshift_space_field(_KINDS[spec["kind"]], spec["scale"], spec["t_gamma"], spec["los_axis"], vscale, dst_grid=spec["into"],
                                   field=spec["into"] is None)
    return got["field"]
