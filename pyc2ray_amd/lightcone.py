"""The light cone of the 21-cm signal, built while a run advances.

What an interferometer records is not a coeval box: along the line of sight every slice is seen at another redshift.  On the CPU
that is ``tools21cm.make_lightcone``, which reads every saved snapshot back and interpolates between neighbours slice by slice.
Here the cone is accumulated step by step on the device (``libasora.lightcone_advance``): the library keeps the formed field of the
previous step, and a step emits the few slices whose redshift it crossed, interpolated linearly in z between the two states --
only those N^2 planes cross to the host.  :class:`LightCone` is the accumulator, :func:`make_lightcone` the offline entry for a
sequence of host states, :func:`slice_redshifts` the redshifts of slices a fixed comoving distance apart.  ``C2Ray`` drives a
LightCone of its own with ``Output: lightcone: 1``.  Slice m of a cone takes plane ``(first_plane - m) mod N`` of the box along the
line of sight: consecutive slices are consecutive planes, the box repeats after N slices, and distance grows with the plane index.
Not modelled: peculiar velocities along the cone (a mapped coeval cube enters through ``src_grid``), angular (non-flat-sky)
cones, interpolation other than linear in z.
"""
import math

import numpy as np

from . import _capi, _residency
from .asora_core import cuda_is_init
from .load_extensions import load_asora
from ._fieldspec import MESH_TRANSFORM, check_mesh, check_t_gamma, host_field, is_int, is_real
from .powerspec import _KINDS, _check_kind
from .redshift_space import _check_axis

__all__ = ['LightCone', 'LightConeStep', 'make_lightcone', 'slice_redshifts']

C_KM_S = 299792.458
#: the most slices of one library call (a step that crosses more is split)
MAX_SLICES = _capi.LC_MAX_SLICES
_GRIDS = (_capi.GRID_XH, _capi.GRID_NDENS, _capi.GRID_TEMP)


# ---- redshifts of the slices -----------------------------------------------------------------------------------------------------
def _hubble_distance_mpc(cosmology):
    h0 = cosmology.H0
    return C_KM_S / float(getattr(h0, "value", h0))


def comoving_interval_mpc(cosmology, z_lo, z_hi):
    """The comoving distance between two redshifts in Mpc, c / H0 times the integral of dz / E(z) between them: integrated over the
    interval itself, so that a spacing of a cell is not the difference of two distances of gigaparsecs."""
    from scipy.integrate import quad
    val, _ = quad(lambda x: 1.0 / float(cosmology.efunc(x)), float(z_lo), float(z_hi), epsabs=0.0, epsrel=1e-13, limit=200)
    return _hubble_distance_mpc(cosmology) * val


def _next_redshift(cosmology, z, dchi_mpc):
    """The redshift a comoving distance `dchi_mpc` nearer than z (None: that is beyond z = 0): brentq on the distance between the
    two, as ``FlatLambdaCDMLite.z_at_age`` inverts the age."""
    from scipy.optimize import brentq
    f = lambda x: comoving_interval_mpc(cosmology, x, z) - dchi_mpc
    # a bracket from the local slope d chi / d z = (c / H0) / E(z), doubled until it holds
    step = 2.0 * dchi_mpc * float(cosmology.efunc(z)) / _hubble_distance_mpc(cosmology)
    lo = z - step
    while lo > -0.5 and f(lo) < 0.0:
        step *= 2.0
        lo = z - step
    lo = max(lo, -0.5)
    if f(lo) < 0.0:
        return None
    return float(brentq(f, lo, z, xtol=1e-15, rtol=1e-15))


def _check_cosmology(who, cosmology):
    if not (hasattr(cosmology, "efunc") and hasattr(cosmology, "H0") and hasattr(cosmology, "comoving_distance")):
        raise ValueError(f"{who}: cosmology must have H0, efunc and comoving_distance (FlatLambdaCDMLite, or astropy's FlatLambdaCDM)")


def _check_positive(who, name, v):
    if not is_real(v) or not (math.isfinite(v) and v > 0):
        raise ValueError(f"{who}: {name} must be a finite number > 0, not {v!r}")


def _check_redshift(who, name, z):
    if not is_real(z) or not (math.isfinite(z) and z > -1.0):
        raise ValueError(f"{who}: {name} must be a finite number > -1, not {z!r}")


def slice_redshifts(cosmology, z_start, z_end, dchi_mpc):
    """The redshifts z_m, m = 0, 1, ..., of slices a comoving distance `dchi_mpc` apart, chi(z_m) = chi(z_start) - m dchi_mpc, down to
    `z_end` (z_m >= z_end): a float64 array, descending.  `cosmology`: ``FlatLambdaCDMLite`` or astropy's ``FlatLambdaCDM``."""
    who = "slice_redshifts"
    _check_cosmology(who, cosmology)
    _check_redshift(who, "z_start", z_start)
    _check_redshift(who, "z_end", z_end)
    _check_positive(who, "dchi_mpc", dchi_mpc)
    if z_end > z_start:
        raise ValueError(f"{who}: z_end = {z_end!r} lies above z_start = {z_start!r}")
    out, z = [], float(z_start)
    while z is not None and z >= z_end:
        out.append(z)
        z = _next_redshift(cosmology, z, float(dchi_mpc))
    return np.array(out, dtype=np.float64)


# ---- the accumulator -------------------------------------------------------------------------------------------------------------
class LightConeStep:
    """What one ``LightCone.advance`` emitted: ``first`` (the index of its first slice), ``z`` and ``mean`` of its slices (arrays,
    empty for a step that crossed none), ``stored_only`` (the first advance, which keeps the field and emits nothing)."""

    def __init__(self, first, z, mean, kind, stored_only=False):
        self.first, self.kind, self.stored_only = int(first), kind, bool(stored_only)
        self.z, self.mean = np.array(z, dtype=np.float64), np.array(mean, dtype=np.float64)

    @property
    def n_slices(self):
        return int(self.z.size)

    def log_line(self):
        """The line of the log file (one per step)."""
        if self.stored_only:
            return f"Light cone ({self.kind}): the field of the first state is kept, no slice yet"
        if not self.n_slices:
            return f"Light cone ({self.kind}): the step crossed no slice"
        return (f"Light cone ({self.kind}): {self.n_slices:n} slices from {self.first:n}, z = {self.z[0]:.5f} ... {self.z[-1]:.5f}, mean "
                f"{float(np.mean(self.mean)):.6e}")

    def __repr__(self):
        return f"<LightConeStep: {self.log_line()}>"


def lightcone_spec(who, N, kind='xh', los_axis=2, first_plane=0, slot=0, src_grid=None, z_end=None, spin=None):
    """The keywords of a :class:`LightCone` checked for a mesh of N cells a side (None: not known yet).  Raises ValueError for what
    the library would refuse."""
    _check_kind(who, kind)
    _check_axis(who, los_axis)
    if not is_int(first_plane) or first_plane < 0 or (N is not None and first_plane >= N):
        raise ValueError(f"{who}: first_plane must be an int in [0, N), not {first_plane!r}")
    if not is_int(slot) or not 0 <= slot < _capi.LC_SLOTS:
        raise ValueError(f"{who}: slot must be an int in [0, {_capi.LC_SLOTS}), not {slot!r}")
    if src_grid is not None and (not is_int(src_grid) or not 0 <= src_grid < _capi.GRID_COUNT):
        raise ValueError(f"{who}: src_grid must be None or a grid selector 0 ... {_capi.GRID_COUNT - 1} (_capi.GRID_*), not {src_grid!r}")
    if src_grid is not None and kind != "xh":
        raise ValueError(f"{who}: src_grid takes a grid as it is: kind 'xh', not {kind!r}")
    if z_end is not None:
        _check_redshift(who, "z_end", z_end)
    if spin not in (None, "kinetic"):
        raise ValueError(f"{who}: spin must be None or 'kinetic', not {spin!r}")
    if N is not None:
        check_mesh(who, N, MESH_TRANSFORM)


class LightCone:
    """A light cone of a mesh of N cells a side, accumulated by :meth:`advance` as a run goes from high to low redshift.

    ``kind``: what a slice shows ('xh', 'xhi', 'density', 'hi', 'dtb': the kinds of ``power_spectrum``; 'dtb' is 'hi' with the
    ``scale`` given to :meth:`advance`); ``src_grid``: a device grid taken as it is instead.  ``los_axis``, ``first_plane``: slice m
    is plane ``(first_plane - m) mod N`` along that axis.  ``dchi``: the comoving distance between slices in Mpc; ``z``: the redshift
    of every slice emitted so far, descending from the `z_start` the cone was made with; ``mean``, ``variance``: of every slice, from
    sums reduced on the device (the global signal along the cone); ``n_slices``: how many there are.  ``slot``: the library's slot.
    ``keep=False`` keeps no slices on the host (the ranks of a multi-rank run but the first): the moments only."""

    def __init__(self, N, cosmology, z_start, dchi, kind='xh', los_axis=2, first_plane=0, slot=0, src_grid=None, z_end=None, keep=True):
        who = "LightCone"
        if not is_int(N):
            raise ValueError(f"{who}: N must be an int, not {N!r}")
        lightcone_spec(who, int(N), kind=kind, los_axis=los_axis, first_plane=first_plane, slot=slot, src_grid=src_grid, z_end=z_end)
        _check_cosmology(who, cosmology)
        _check_redshift(who, "z_start", z_start)
        _check_positive(who, "dchi", dchi)
        self.N, self.cosmology, self.kind, self.los_axis, self.first_plane = int(N), cosmology, kind, int(los_axis), int(first_plane)
        self.dchi, self.slot, self.src_grid, self.keep = float(dchi), int(slot), src_grid, bool(keep)
        self.z_end = None if z_end is None else float(z_end)
        self._z, self._moments, self._chunks = [], [], []
        self._next_z = float(z_start)              # the redshift of slice n_slices (None: the cone has reached z = 0 or z_end)
        self._started = False

    # -- what has been emitted
    @property
    def n_slices(self):
        return len(self._z)

    @property
    def z(self):
        return np.array(self._z, dtype=np.float64)

    @property
    def moments(self):
        """(n_slices, 2): the sum and the sum of squares of every slice."""
        return np.array(self._moments, dtype=np.float64).reshape(-1, 2)

    @property
    def mean(self):
        return self.moments[:, 0] / float(self.N) ** 2

    @property
    def variance(self):
        return self.moments[:, 1] / float(self.N) ** 2 - self.mean ** 2

    def planes(self, m0, n):
        """The box planes of the slices m0 ... m0 + n - 1."""
        return (self.first_plane - (int(m0) + np.arange(int(n), dtype=np.int64))) % self.N

    # -- the run
    def _crossed(self, z_now):
        """The redshifts of the slices not yet emitted with z_m >= z_now (they leave the queue)."""
        zs = []
        while self._next_z is not None and self._next_z >= z_now and (self.z_end is None or self._next_z >= self.z_end):
            zs.append(self._next_z)
            self._next_z = _next_redshift(self.cosmology, self._next_z, self.dchi)
        return zs

    def advance(self, lib, z_prev, z_now, scale=None, t_gamma=0.0):
        """The device grids of `lib` hold the state at redshift `z_now`; the state of the previous call was at `z_prev` > `z_now`.
        Emits every slice not yet emitted with z_m >= z_now, each interpolated linearly in z between the two states, f = (z_prev -
        z_m) / (z_prev - z_now): ``w_now = f s_m`` and ``w_prev = (1 - f) s_m`` with s_m = ``scale(z_m)``, or 1 without `scale`; then
        keeps the present field for the next call.  `t_gamma`: of the kind 'hi' / 'dtb' for the present state.  The first call
        only keeps the field (`z_prev` is not looked at).  A step that crosses more than the library's ``LC_MAX_SLICES`` slices is
        split over several calls, the field being refreshed by the last.  Returns a :class:`LightConeStep`."""
        who = "LightCone.advance"
        _check_redshift(who, "z_now", z_now)
        check_t_gamma(who, t_gamma)
        if scale is not None and not callable(scale):
            raise ValueError(f"{who}: scale must be None or a function of the redshift")
        kind = _KINDS[self.kind]
        if not self._started:
            lib.lightcone_reset(self.slot)           # (whatever the slot kept belongs to another cone)
            lib.lightcone_advance(self.slot, kind, self.src_grid, t_gamma, self.los_axis, (), (), (), True, slices=False)
            self._started = True
            return LightConeStep(self.n_slices, (), (), self.kind, stored_only=True)
        _check_redshift(who, "z_prev", z_prev)
        if not z_now < z_prev:
            raise ValueError(f"{who}: the run goes from high to low redshift: z_now = {z_now!r} must lie below z_prev = {z_prev!r}")
        first = self.n_slices
        zs = np.array(self._crossed(float(z_now)), dtype=np.float64)
        f = (float(z_prev) - zs) / (float(z_prev) - float(z_now))
        s = np.ones_like(zs) if scale is None else np.array([float(scale(z)) for z in zs], dtype=np.float64)
        w_now, w_prev = f * s, (1.0 - f) * s
        planes = self.planes(first, zs.size)
        limit = int(MAX_SLICES)
        starts = list(range(0, zs.size, limit)) or [0]
        for q in starts:
            part = slice(q, q + limit)
            got = lib.lightcone_advance(self.slot, kind, self.src_grid, t_gamma, self.los_axis, planes[part], w_prev[part], w_now[part],
                                        q == starts[-1], slices=self.keep)
            self._moments.extend(np.asarray(got["moments"], dtype=np.float64).reshape(-1, 2))
            if self.keep and zs.size:
                self._chunks.append(got["slices"])
        self._z.extend(zs.tolist())
        return LightConeStep(first, zs, self.mean[first:], self.kind)

    # -- the cube
    def array(self, order='run'):
        """The slices emitted so far as one (n_slices, N, N) array; a slice's two axes are the box axes other than ``los_axis``, in
        ascending order.  ``order='run'``: slice m at index m, the redshift falling; ``'distance'``: flipped, so that the index grows
        with distance and redshift (the orientation of ``tools21cm``)."""
        if order not in ("run", "distance"):
            raise ValueError(f"LightCone.array: order must be 'run' or 'distance', not {order!r}")
        if not self.keep:
            raise ValueError("LightCone.array: this cone keeps no slices (keep=False)")
        cube = np.concatenate(self._chunks, axis=0) if self._chunks else np.zeros((0, self.N, self.N))
        return cube[::-1] if order == "distance" else cube

    def chunk(self, m0, n=None):
        """The slices m0 ... m0 + n - 1 as a volume in box axis order, the line of sight along ``los_axis``.  With n = N (the default)
        an (N, N, N) cube: every slice in the plane of the box it was taken from, so that the cube is periodic where the box is --
        ``lib.grid_to_device`` puts it into a grid for ``power_spectrum_los(kind='xh')`` and the analyses of a grid.  With another n
        the n planes in the order of distance (the nearest, slice m0 + n - 1, first)."""
        n = self.N if n is None else n
        if not is_int(m0) or not is_int(n) or m0 < 0 or n < 1 or m0 + n > self.n_slices:
            raise ValueError(f"LightCone.chunk: the slices {m0!r} ... {m0!r} + {n!r} - 1 are not among the {self.n_slices} emitted")
        part = self.array()[m0:m0 + n]
        if n == self.N:
            vol = np.empty_like(part)
            vol[self.planes(m0, n)] = part
        else:
            vol = part[::-1]
        return np.ascontiguousarray(np.moveaxis(vol, 0, self.los_axis))

    def save(self, path):
        """An ``.npz`` of the cone: ``slices`` (run order; absent with keep=False), ``z``, ``mean``, ``variance``, ``moments``,
        ``kind``, ``los_axis``, ``first_plane``, ``dchi``."""
        data = dict(z=self.z, mean=self.mean, variance=self.variance, moments=self.moments, kind=self.kind, los_axis=self.los_axis,
                    first_plane=self.first_plane, dchi=self.dchi)
        if self.keep:
            data["slices"] = self.array()
        np.savez(path, **data)

    def __repr__(self):
        return (f"<LightCone of {self.kind} along axis {self.los_axis}: {self.n_slices} slices of {self.N} x {self.N}, {self.dchi:.4g} Mpc "
                f"apart>")


# ---- the offline entry ---------------------------------------------------------------------------------------------------------------
def _state_arrays(who, item, index):
    """One item of `fields`: an (N, N, N) array (the ionised fraction), or a triple (xh, ndens, temp) of them."""
    if isinstance(item, (tuple, list)):
        if len(item) != 3:
            raise ValueError(f"{who}: fields[{index}] must be an (N, N, N) array or a triple (xh, ndens, temp)")
        arrays = tuple(host_field(who, f"fields[{index}][{q}]", a) for q, a in enumerate(item))
        if len({a.shape for a in arrays}) != 1:
            raise ValueError(f"{who}: xh, ndens and temp of fields[{index}] must have one shape")
        return arrays
    return (host_field(who, f"fields[{index}]", item),)


def make_lightcone(fields, redshifts, kind='xh', los_axis=2, box_len_mpc=None, cosmology=None, first_plane=0, scale=None, t_gamma=None,
                   slot=0):
    """The light cone of a sequence of states: a :class:`LightCone`.

    ``fields``: a sequence (or an iterator) of host (N, N, N) arrays for the mesh of ``device_init`` -- the ionised fraction, for the
    kinds 'xh' and 'xhi' -- or of triples (xh, ndens, temp) for any kind; ``redshifts``: theirs, descending.  Each state is uploaded
    to the device grids and the cone advanced: the first one is only kept, every later one emits the slices between its
    predecessor's redshift and its own.  ``box_len_mpc``: the comoving side of the box, so that slices lie ``box_len_mpc / N`` apart
    from ``redshifts[0]`` down; ``cosmology``: ``FlatLambdaCDMLite`` or astropy's ``FlatLambdaCDM``.  ``scale``: None, or a function
    of the redshift whose value multiplies a slice (the prefactor of the brightness temperature for 'dtb'); ``t_gamma``: None (0),
    one number, or one per state (the kinds 'hi' and 'dtb': the CMB temperature at the state's redshift for a spin temperature
    coupled to the kinetic one)."""
    who = "make_lightcone"
    lightcone_spec(who, None, kind=kind, los_axis=los_axis, first_plane=first_plane, slot=slot)
    _check_positive(who, "box_len_mpc", box_len_mpc)
    _check_cosmology(who, cosmology)
    try:
        zs = np.array(redshifts, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: redshifts must be a one-dimensional sequence of numbers") from None
    if zs.ndim != 1 or zs.size < 2 or not np.all(np.isfinite(zs)) or np.any(zs <= -1.0) or np.any(np.diff(zs) >= 0.0):
        raise ValueError(f"{who}: redshifts must be two or more finite values > -1, strictly descending")
    if scale is not None and not callable(scale):
        raise ValueError(f"{who}: scale must be None or a function of the redshift")
    if t_gamma is None:
        tg = np.zeros(zs.size)
    else:
        try:
            tg = np.array(t_gamma, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: t_gamma must be None, a number or one number per state") from None
        if isinstance(t_gamma, (bool, np.bool_)) or tg.ndim > 1 or (tg.ndim == 1 and tg.size != zs.size):
            raise ValueError(f"{who}: t_gamma must be None, a number or one number per state")
        tg = np.broadcast_to(tg, zs.shape)
        if not np.all(np.isfinite(tg)) or np.any(tg < 0.0):
            raise ValueError(f"{who}: t_gamma must be finite and >= 0")
    if hasattr(fields, "__len__") and len(fields) != zs.size:
        raise ValueError(f"{who}: fields has {len(fields)} states, redshifts {zs.size}")
    states = iter(fields)                  # (an iterator that ends early is found out when it does)
    cone, lib = None, None
    for index in range(zs.size):
        try:
            item = next(states)
        except StopIteration:
            raise ValueError(f"{who}: fields has {index} states, redshifts {zs.size}") from None
        arrays = _state_arrays(who, item, index)
        N = arrays[0].shape[0]
        if len(arrays) == 1 and kind not in ("xh", "xhi"):
            raise ValueError(f"{who}: kind {kind!r} is formed from triples (xh, ndens, temp); a single array is the ionised fraction")
        if cone is None:
            lightcone_spec(who, N, kind=kind, los_axis=los_axis, first_plane=first_plane, slot=slot)
            if not cuda_is_init():
                raise RuntimeError("GPU not initialized. Please initialize it by calling device_init(N)")
            lib = load_asora()
            cone = LightCone(N, cosmology, float(zs[0]), float(box_len_mpc) / N, kind=kind, los_axis=los_axis, first_plane=first_plane,
                             slot=slot, z_end=float(zs[-1]))
        elif N != cone.N:
            raise ValueError(f"{who}: fields[{index}] has {N} cells a side, the first state {cone.N}")
        _residency.reclaim()              # this call overwrites device grids a resident C2Ray object may be relying on
        for which, a in zip(_GRIDS, arrays):
            lib.grid_to_device(which, np.asarray(a, dtype=np.float64))
        cone.advance(lib, None if index == 0 else float(zs[index - 1]), float(zs[index]), scale=scale, t_gamma=float(tg[index]))
    return cone
