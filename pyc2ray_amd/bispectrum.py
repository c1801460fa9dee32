"""The bispectrum of the 21-cm signal: the FFT triangle estimator on the device.

The signal of reionisation is strongly non-Gaussian, and the bispectrum is the statistic the literature reaches for right after the
power spectrum (Majumdar et al. 2018, Watkinson et al. 2017 and 2019, Hutter et al. 2020, Giri et al. 2019).  On the CPU it is three
N^3 downloads, two ``numpy.fft.irfftn`` per k-shell and a Python loop over the triangles.  :func:`bispectrum` runs it on the device
(``libasora.bispectrum``): one forward transform of the field formed from the device grids -- the one of
:func:`pyc2ray_amd.powerspec.power_spectrum` --, one inverse per shell from the kept spectrum, and a kernel that sums the triple
products of many triangles in one pass over the shell fields.  The same with the spectrum set to 1 counts the closed triples of
modes.  Every sum has a fixed order, so the same call returns the same bits.  ``C2Ray.bispectrum()`` does that for the current
state of a run.
"""
import math

import numpy as np

from . import _capi, _residency
from .asora_core import cuda_is_init
from .load_extensions import load_asora
from ._fieldspec import MESH_TRANSFORM, check_mesh, check_scale, check_t_gamma, host_field, is_int, is_real
from .powerspec import _KINDS, _check_kind, _edges, _edges_to_thresholds, _nan_divide

__all__ = ['Bispectrum', 'bispectrum']

_SELECTIONS = ("all", "equilateral", "isosceles")


class Bispectrum:
    """The result of :func:`bispectrum`.  Wave numbers are in units of 2 pi / L, powers in L^3 and the bispectrum in L^6, with L =
    ``box_len`` the side of the box in the caller's units (None: L = N, lengths in cells).

    From the library call.  ``edges`` of the shells (in units of the fundamental mode) and ``thresholds`` = ceil(edges^2), as in
    :class:`pyc2ray_amd.powerspec.PowerSpectrum`; ``triangles``, (n_tri, 3) shell indices; ``sum_ggg``: per triangle, the sum of
    ghat(n1) ghat(n2) ghat(n3) over the ordered triples of modes, one from each shell, that close modulo N; ``sum_iii``: the number
    of those triples as the transforms give it, a double close to an integer; per shell ``n_modes``, ``sum_k``, ``sum_aa`` and
    ``moments``, the bits of the power spectrum for the same edges.

    Derived.  ``n_triangles``: ``sum_iii`` as floats, not rounded; ``count_residual``: the largest distance of a ``sum_iii`` from an
    integer (0.5 would mean the count is lost).  ``k`` and ``P`` per shell as there; ``k1``, ``k2``, ``k3``: the mean |k| of a
    triangle's shells; ``B`` = L^6 / N^9 sum_ggg / sum_iii, the convention of ``PowerSpectrum.P`` (L^3 / N^6 <|ghat|^2>) carried
    one order up, NaN where no triangle closes; ``Q`` = B / (P1 P2 + P2 P3 + P3 P1); ``b_norm`` = B / sqrt(k1 k2 k3 P1 P2 P3 / L^3),
    the normalised form of Watkinson et al. 2019; ``cos_theta`` = (k3^2 - k1^2 - k2^2) / (2 k1 k2), the cosine of the angle between
    k1 and k2; ``aliased``: True if a shell reaches beyond (N - 1) / 3 -- it holds a mode with a folded component above that
    --, so that triples closing on a multiple of N other than 0 are among those summed; ``mean`` and ``variance`` from the moments."""

    def __init__(self, edges, triangles, sum_ggg, sum_iii, n_modes, sum_k, sum_aa, moments, N, box_len=None, kind="dtb"):
        self.edges = np.array(edges, dtype=np.float64).ravel()
        self.triangles = np.array(triangles, dtype=np.int32).reshape(-1, 3)
        self.sum_ggg = np.array(sum_ggg, dtype=np.float64).ravel()
        self.sum_iii = np.array(sum_iii, dtype=np.float64).ravel()
        self.n_modes = np.array(n_modes, dtype=np.uint64).ravel()
        self.sum_k = np.array(sum_k, dtype=np.float64).ravel()
        self.sum_aa = np.array(sum_aa, dtype=np.float64).ravel()
        self.moments = np.array(moments, dtype=np.float64).ravel()
        ns, nt = self.edges.size - 1, self.triangles.shape[0]
        if ns < 1 or not (self.n_modes.size == self.sum_k.size == self.sum_aa.size == ns):
            raise ValueError(f"Bispectrum: {self.edges.size} edges go with {max(ns, 0)} shells >= 1, not {self.n_modes.size}, "
                             f"{self.sum_k.size}, {self.sum_aa.size}")
        if nt < 1 or not (self.sum_ggg.size == self.sum_iii.size == nt):
            raise ValueError(f"Bispectrum: {nt} triangles >= 1 go with as many sums, not {self.sum_ggg.size}, {self.sum_iii.size}")
        if self.triangles.min() < 0 or self.triangles.max() >= ns:
            raise ValueError(f"Bispectrum: a triangle names a shell outside 0 ... {ns - 1}")
        if self.moments.size != 2:
            raise ValueError(f"Bispectrum: 2 moments, not {self.moments.size}")
        self.N = int(N)
        self.box_len = None if box_len is None else float(box_len)
        self.kind = kind

    @property
    def thresholds(self):
        return _edges_to_thresholds(self.edges)

    @property
    def L(self):
        return float(self.N) if self.box_len is None else self.box_len

    @property
    def n_triangles(self):
        return self.sum_iii.copy()

    @property
    def count_residual(self):
        return float(np.max(np.abs(self.sum_iii - np.rint(self.sum_iii))))

    @property
    def k(self):
        return 2.0 * math.pi / self.L * _nan_divide(self.sum_k, self.n_modes.astype(np.float64))

    @property
    def P(self):
        return self.L ** 3 / float(self.N) ** 6 * _nan_divide(self.sum_aa, self.n_modes.astype(np.float64))

    @property
    def k1(self):
        return self.k[self.triangles[:, 0]]

    @property
    def k2(self):
        return self.k[self.triangles[:, 1]]

    @property
    def k3(self):
        return self.k[self.triangles[:, 2]]

    @property
    def B(self):
        closes = np.rint(self.sum_iii) != 0
        out = np.full(self.sum_ggg.shape, np.nan)
        np.divide(self.sum_ggg, self.sum_iii, out=out, where=closes)
        return self.L ** 6 / float(self.N) ** 9 * out

    def _P3(self):
        P = self.P
        return P[self.triangles[:, 0]], P[self.triangles[:, 1]], P[self.triangles[:, 2]]

    @property
    def Q(self):
        p1, p2, p3 = self._P3()
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.B / (p1 * p2 + p2 * p3 + p3 * p1)

    @property
    def b_norm(self):
        p1, p2, p3 = self._P3()
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.B / np.sqrt(self.k1 * self.k2 * self.k3 * p1 * p2 * p3 / self.L ** 3)

    @property
    def cos_theta(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            return (self.k3 ** 2 - self.k1 ** 2 - self.k2 ** 2) / (2.0 * self.k1 * self.k2)

    @property
    def aliased(self):
        return 3 * math.isqrt(max(int(self.thresholds[-1]) - 1, 0)) > self.N - 1      # (the largest folded component of a shell's modes)

    @property
    def mean(self):
        return float(self.moments[0]) / float(self.N) ** 3

    @property
    def variance(self):
        return float(self.moments[1]) / float(self.N) ** 3 - self.mean ** 2

    def log_line(self):
        """The line of a log file."""
        unit = "cells" if self.box_len is None else "units of box_len"
        B = self.B
        head = (f"Bispectrum ({self.kind}, {self.n_modes.size} shells to |n| = {self.edges[-1]:g}, {self.triangles.shape[0]} triangles, "
                f"L = {self.L:g} {unit}): mean {self.mean:.6e}, variance {self.variance:.6e}, count residual {self.count_residual:.2e}")
        if self.aliased:
            head += ", aliased triangles included"
        if np.all(np.isnan(B)):
            return head + "; no triangle closes"
        peak = int(np.nanargmax(np.abs(B)))
        a, b, c = (int(v) for v in self.triangles[peak])
        return head + f"; largest |B| {B[peak]:.6e} at shells ({a}, {b}, {c}), Q there {self.Q[peak]:.4f}"

    def __repr__(self):
        return f"<Bispectrum: {self.log_line()}>"


def _shell_edges(who, N, shells):
    """None: b + 0.5, b = 0 ... max(1, min((N - 1) // 3, BISPEC_MAX_SHELLS)) (needs N): no aliased triangle exists with these; an int n:
    n equal shells over the same range; else an array of edges, checked as the power spectrum checks its bins."""
    if shells is None or is_int(shells):
        if shells is not None and not 1 <= shells <= _capi.BISPEC_MAX_SHELLS:
            raise ValueError(f"{who}: shells as an int must be in [1, {_capi.BISPEC_MAX_SHELLS}], not {shells}")
        if N is None:
            return None
        top = max(1, (N - 1) // 3)
        if shells is None:
            return np.arange(0, min(top, _capi.BISPEC_MAX_SHELLS) + 1, dtype=np.float64) + 0.5
        return np.linspace(0.5, top + 0.5, int(shells) + 1)
    try:
        e = _edges(who, N, shells)
    except ValueError as err:              # (the power spectrum's checks, under this keyword's name)
        raise ValueError(str(err).replace("bins", "shells")) from None
    if e.size > _capi.BISPEC_MAX_SHELLS + 1:
        raise ValueError(f"{who}: shells must be at most {_capi.BISPEC_MAX_SHELLS + 1} edges, not {e.size}")
    return e


def _triangles(who, triangles, edges):
    """The selection as an (n_tri, 3) int32 array (edges = None: checked only)."""
    if isinstance(triangles, str):
        if triangles not in _SELECTIONS:
            raise ValueError(f"{who}: triangles must be one of {', '.join(repr(s) for s in _SELECTIONS)} or a list of (a, b, c), "
                             f"not {triangles!r}")
        if edges is None:
            return None
        ns = edges.size - 1
        if triangles == "equilateral":
            tri = [(a, a, a) for a in range(ns)]
        elif triangles == "isosceles":
            tri = [(a, a, c) for a in range(ns) for c in range(ns)]
        else:                              # a <= b <= c whose shells can close: the lower edge of c below the upper edges of a and b
            tri = [(a, b, c) for a in range(ns) for b in range(a, ns) for c in range(b, ns) if edges[c] < edges[a + 1] + edges[b + 1]]
        tri = np.array(tri, dtype=np.int32).reshape(-1, 3)
    else:
        try:
            tri = np.array(triangles)
        except (TypeError, ValueError):
            tri = None
        if tri is None or tri.ndim != 2 or tri.shape[1] != 3 or tri.shape[0] < 1 or tri.dtype.kind not in "iu":
            raise ValueError(f"{who}: triangles must be one of {', '.join(repr(s) for s in _SELECTIONS)} or a list of (a, b, c) of "
                             f"shell indices")
        if tri.min() < 0:
            raise ValueError(f"{who}: a triangle names a shell below 0")
        if edges is not None and tri.max() >= edges.size - 1:
            raise ValueError(f"{who}: a triangle names a shell outside 0 ... {edges.size - 2}")
        tri = tri.astype(np.int32)
    if tri.shape[0] > _capi.BISPEC_MAX_TRIANGLES:
        raise ValueError(f"{who}: at most {_capi.BISPEC_MAX_TRIANGLES} triangles a call, not {tri.shape[0]}")
    return tri


def bispectrum_spec(who, N, kind='dtb', shells=None, triangles='all', box_len=None, scale=1.0, t_gamma=0.0):
    """The keywords of :func:`bispectrum` checked and completed for a mesh of N cells a side, as a dict (N = None: checked only).
    Raises ValueError -- before any device call -- for what the library would refuse."""
    _check_kind(who, kind)
    e = _shell_edges(who, N, shells)
    tri = _triangles(who, triangles, e)
    if box_len is not None and (not is_real(box_len) or not (math.isfinite(box_len) and box_len > 0)):
        raise ValueError(f"{who}: box_len must be None or a finite number > 0, not {box_len!r}")
    check_scale(who, scale)
    check_t_gamma(who, t_gamma)
    if N is None:
        return None
    check_mesh(who, N, MESH_TRANSFORM)
    return dict(N=int(N), kind=kind, edges=e, thresholds=_edges_to_thresholds(e), triangles=tri,
                box_len=None if box_len is None else float(box_len), scale=float(scale), t_gamma=float(t_gamma))


def bispectrum(field=None, *, kind='dtb', shells=None, triangles='all', box_len=None, scale=1.0, t_gamma=0.0):
    """The bispectrum of a field for triangles of k-shells, a :class:`Bispectrum`.

    ``field``: an (N, N, N) host array for the mesh of ``device_init``; it is uploaded to the device's ionised-fraction grid, which
    a C2Ray object that keeps its grids there is told beforehand, and analysed as it is (``kind`` 'xh', which the default stands
    for here) or as 1 - field ('xhi').  ``field`` = None: the device grids are analysed where they lie, and ``kind``, ``scale`` and
    ``t_gamma`` select what is formed from them as in :func:`pyc2ray_amd.powerspec.power_spectrum`.
    ``shells``: None for unit-width shells with the edges b + 0.5 up to floor((N - 1) / 3) + 0.5 (32 shells at the most), with which
    no aliased triangle exists; an int n for n equal shells over that range; or an array of at most 33 finite, > 0, strictly
    ascending edges, in units of the fundamental mode 2 pi / L.  A mode exactly on an edge belongs to the upper shell.
    ``triangles``: 'all' for every a <= b <= c whose shells can close (the lower edge of c below the sum of the upper edges of a
    and b), 'equilateral' for (a, a, a), 'isosceles' for (a, a, c), or a list of (a, b, c) shell indices in any order, repeats and
    duplicates allowed; at most 8192.  ``box_len``: L in the caller's units (None: N, lengths in cells).
    Closure of a triangle is modulo N: with a shell that reaches beyond (N - 1) / 3 the sums include aliased triples, and
    ``Bispectrum.aliased`` says so.  The device keeps one N^3 field per shell (134 MB each at 256^3)."""
    who = "bispectrum"
    if field is not None:
        field = host_field(who, "field", field)
        N = field.shape[0]
        if kind not in ("dtb", "xh", "xhi"):
            raise ValueError(f"{who}: a host field is analysed as kind 'xh' or 'xhi', not {kind!r} (the other kinds go with field=None)")
        kind = "xh" if kind == "dtb" else kind
    else:
        N = None
    kw = dict(kind=kind, shells=shells, triangles=triangles, box_len=box_len, scale=scale, t_gamma=t_gamma)
    spec = bispectrum_spec(who, N, **kw)
    if not cuda_is_init():
        raise RuntimeError("GPU not initialized. Please initialize it by calling device_init(N)")
    lib = load_asora()
    if field is not None:
        _residency.reclaim()              # this call overwrites a device grid a resident C2Ray object may be relying on
        lib.grid_to_device(_capi.GRID_XH, np.asarray(field, dtype=np.float64))
    else:
        if getattr(lib, "_N", None) is None:
            raise RuntimeError(f"{who}: field=None needs a device initialised through device_init (the mesh size)")
        spec = bispectrum_spec(who, int(lib._N), **kw)
    return bispectrum_on_device(lib, spec)


def bispectrum_on_device(lib, spec):
    """The library call for a checked `spec` (bispectrum_spec) on the device grids, as a :class:`Bispectrum`."""
    got = lib.bispectrum(_KINDS[spec["kind"]], spec["scale"], spec["t_gamma"], spec["thresholds"], spec["triangles"])
    return Bispectrum(spec["edges"], spec["triangles"], got["sum_ggg"], got["sum_iii"], got["count"], got["sum_k"], got["sum_aa"],
                      got["moments"], spec["N"], box_len=spec["box_len"], kind=spec["kind"])
