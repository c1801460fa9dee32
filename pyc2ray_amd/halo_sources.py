"""Sources from a halo catalogue, with the low-mass haloes suppressed where the gas is ionised.

The C2-Ray source model of the literature (Iliev et al. 2007, 2012; Dixon et al. 2016) has two populations: high-mass
atomically-cooling haloes (HMACHs, ``mass >= m_hm``), which always shine, and low-mass ones (LMACHs, ``m_lm <= mass < m_hm``),
which are switched off or dimmed in cells that are already ionised.  That is the one piece of source physics that needs the
current ionised fraction at every time step.  :class:`HaloCatalogue` is uploaded once and binned on the device into a table of its
occupied cells (``libasora.halo_catalogue_to_device``); :func:`halo_sources` forms the source list of a step from that table and
the device's ionised fraction, so that only the list crosses PCIe; ``C2Ray.halo_sources()`` and ``C2Ray.evolve3D(dt)`` do that
for a run.  The weights are summed as integers in units of a power of two (include/asora_hip.h has the statement, operation by
operation): the table, the list and the summary do not depend on the order of the haloes, and the same call returns the same bits.
"""
import math

import numpy as np

from . import _capi
from .asora_core import cuda_is_init
from .load_extensions import load_asora
from ._fieldspec import analyse, check_flag, host_field, is_real

__all__ = ['HaloCatalogue', 'SourceModel', 'HaloSourceList', 'halo_sources', 'source_scale']

SUPPRESSIONS = {"none": _capi.HALO_MODEL_NONE, "full": _capi.HALO_MODEL_FULL, "partial": _capi.HALO_MODEL_PARTIAL}
# cgs values of the reference's drivers (msun2g of c2ray_base.py, the proton mass of CODATA 2018) and its flux normalisation
MSUN_G = 1.98892e33
M_PROTON = 1.67262192369e-24
MYR_S = 3.15576e13
S_STAR_REF = 1.0e48
MEAN_MOLECULAR = 0.926 + 4.0 * 0.074
_Q_LIMIT = 2.0 ** 62
_MAX_EXPONENT = 1000


def unit_exponent(total):
    """e of the unit 2^e for weights that sum to `total`: ceil(log2(total)) - 61 (0 for a sum of 0), so that the sum of the
    quantised weights stays below 2^62 with one bit to spare for the rounding of `total` and the n/2 of the haloes' own."""
    if not total > 0.0:
        return 0
    m, ex = math.frexp(total)          # total = m 2^ex, 0.5 <= m < 1
    return (ex - 1 if m == 0.5 else ex) - 61


def _real_array(who, name, a, shape_of=None):
    try:
        a = np.asarray(a)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} must be a real array, not {type(a).__name__}") from None
    if a.dtype.kind not in "fiu":
        raise ValueError(f"{who}: {name} must be a real array, not one of dtype {a.dtype}")
    if shape_of is not None and a.shape != shape_of:
        raise ValueError(f"{who}: {name} must have shape {shape_of}, not {a.shape}")
    return np.ascontiguousarray(a, dtype=np.float64)


class HaloCatalogue:
    """A halo catalogue for the mesh of ``device_init``.

    ``positions``: (n, 3) in cell units, cell c covering [c, c + 1), 0-based; ``masses``: (n); ``weights``: (n), what is summed per
    cell (a mass-dependent efficiency is the caller's numpy) -- finite and >= 0.  None: the masses of the haloes with mass >= m_lm and
    0 for the others, which are dropped whatever they weigh: a NaN mass is then no error, and the haloes below ``m_lm`` do not enter
    the sum that sets the automatic ``unit``.  ``m_lm`` <= ``m_hm``: a halo
    is HM with mass >= m_hm, LM with m_lm <= mass < m_hm, else dropped (``below``; a NaN mass too).  ``wrap``: a periodic box --
    positions are taken modulo N -- or, False, haloes outside the box are dropped (``outside``).  Positions that are not finite or
    beyond 2^31 are dropped (``nonfinite``).  ``unit``: the weight that one integer step stands for, a power of two; None:
    2^(ceil(log2(sum of the weights)) - 61).  A cell's sum is then exact to (haloes in the cell) unit / 2.

    Everything is checked here, on the host; the upload happens when the catalogue is first used, and again after a
    ``device_init`` or another catalogue's upload, by whatever way it went up: the library numbers the catalogues it takes, and
    the object remembers the number of its own.  ``n_cells`` (occupied cells), ``outside``, ``nonfinite`` and ``below`` are those
    of the last upload (None before)."""

    def __init__(self, positions, masses, weights=None, *, m_lm=1e8, m_hm=1e9, wrap=True, unit=None):
        who = "HaloCatalogue"
        pos = _real_array(who, "positions", positions)
        if pos.ndim != 2 or pos.shape[1] != 3:
            raise ValueError(f"{who}: positions must have shape (n, 3), not {pos.shape}")
        n = pos.shape[0]
        mass = _real_array(who, "masses", masses, (n,))
        for name, v in (("m_lm", m_lm), ("m_hm", m_hm)):
            if not is_real(v) or math.isnan(v):
                raise ValueError(f"{who}: {name} must be a number, not {v!r}")
        if m_lm > m_hm:
            raise ValueError(f"{who}: m_lm must not exceed m_hm ({m_lm!r} > {m_hm!r})")
        check_flag(who, "wrap", wrap)
        if weights is None:                      # (a halo below m_lm is dropped whatever its weight: a NaN mass weighs nothing)
            with np.errstate(invalid="ignore"):
                w = np.where(mass >= m_lm, mass, 0.0)
        else:
            w = _real_array(who, "weights", weights, (n,))
        if not np.all(np.isfinite(w)) or np.any(w < 0.0):
            raise ValueError(f"{who}: the weights must be finite and >= 0")
        with np.errstate(over="ignore"):
            total = float(np.sum(w))
        if not math.isfinite(total):
            raise ValueError(f"{who}: the sum of the weights is not finite")
        if unit is None:
            e = unit_exponent(total)
        else:
            if not is_real(unit) or not (math.isfinite(unit) and unit > 0.0) or math.frexp(unit)[0] != 0.5:
                raise ValueError(f"{who}: unit must be a power of two, not {unit!r}")
            e = math.frexp(unit)[1] - 1
        if abs(e) > _MAX_EXPONENT:
            raise ValueError(f"{who}: unit must lie between 2^-{_MAX_EXPONENT} and 2^{_MAX_EXPONENT}, not 2^{e}")
        if not math.ldexp(total, -e) + 0.5 * n < _Q_LIMIT:
            raise ValueError(f"{who}: with unit 2^{e} a cell's integer sum could overflow: sum(weights) / unit + n / 2 must stay "
                             f"below 2^62")
        self.positions, self.masses, self.weights = pos, mass, w
        self.m_lm, self.m_hm, self.wrap = float(m_lm), float(m_hm), bool(wrap)
        self.unit_exponent = e
        self.n_cells = self.outside = self.nonfinite = self.below = None
        self._held = None                # (library, generation) of this catalogue's last upload

    @property
    def n(self):
        return self.positions.shape[0]

    @property
    def unit(self):
        return math.ldexp(1.0, self.unit_exponent)

    def on_device(self, lib):
        """Is this catalogue's table the one the device holds?"""
        return self._held is not None and self._held[0] is lib and lib.halo_catalogue_generation() == self._held[1]

    def to_device(self, lib):
        """Uploads and bins the catalogue unless the device holds its table already."""
        if self.on_device(lib):
            return
        self._held = None
        counts = lib.halo_catalogue_to_device(self.positions, self.masses, self.weights, self.m_lm, self.m_hm, self.wrap, self.unit_exponent)
        self.n_cells, self.outside, self.nonfinite, self.below = (counts[k] for k in ("n_cells", "outside", "nonfinite", "below"))
        self._held = (lib, lib.halo_catalogue_generation())

    def __repr__(self):
        return (f"<HaloCatalogue: {self.n:n} haloes, m_lm {self.m_lm:g}, m_hm {self.m_hm:g}, {'periodic' if self.wrap else 'open'}, "
                f"unit 2^{self.unit_exponent}>")


class SourceModel:
    """How halo weights become photon rates.  ``fgamma_hm``, ``fgamma_lm``: the ionising photons per baryon that the HM and the LM
    haloes release over ``ts_myr`` (the keys ``fgamma_hm``, ``fgamma_lm`` and ``ts`` of the reference's parameter files).
    ``suppression``: 'none' -- both populations always shine; 'full' -- the LM haloes of a cell with x > ``x_suppress`` are off;
    'partial' -- they shine with ``f_suppressed`` of their rate.  The comparison is strict and a NaN x does not suppress."""

    def __init__(self, fgamma_hm, fgamma_lm, ts_myr, suppression='none', x_suppress=0.1, f_suppressed=0.0, who="SourceModel"):
        for name, v in (("fgamma_hm", fgamma_hm), ("fgamma_lm", fgamma_lm)):
            if not is_real(v) or not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"{who}: {name} must be a finite number >= 0, not {v!r}")
        if not is_real(ts_myr) or not (math.isfinite(ts_myr) and ts_myr > 0.0):
            raise ValueError(f"{who}: ts_myr must be a finite number > 0, not {ts_myr!r}")
        if suppression not in SUPPRESSIONS:
            raise ValueError(f"{who}: suppression must be 'none', 'full' or 'partial', not {suppression!r}")
        if not is_real(x_suppress) or math.isnan(x_suppress):
            raise ValueError(f"{who}: x_suppress must be a number, not {x_suppress!r}")
        if not is_real(f_suppressed) or not 0.0 <= f_suppressed <= 1.0:
            raise ValueError(f"{who}: f_suppressed must be a number in [0, 1], not {f_suppressed!r}")
        self.fgamma_hm, self.fgamma_lm, self.ts_myr = float(fgamma_hm), float(fgamma_lm), float(ts_myr)
        self.suppression, self.x_suppress, self.f_suppressed = suppression, float(x_suppress), float(f_suppressed)

    def __repr__(self):
        return (f"<SourceModel: fgamma_hm {self.fgamma_hm:g}, fgamma_lm {self.fgamma_lm:g}, ts {self.ts_myr:g} Myr, suppression "
                f"{self.suppression!r}, x_suppress {self.x_suppress:g}, f_suppressed {self.f_suppressed:g}>")


def source_scale(ts_myr, omega_b, omega_m, mean_molecular=MEAN_MOLECULAR):
    """The normalised photon rate of a unit weight (a solar mass) per unit fgamma: M_sun Omega_b / (Omega_m mu m_p t_s) / 1e48 --
    the reference's ``mass2phot / S_star_ref`` (c2ray_cubep3m.py) with the fgamma taken out."""
    return MSUN_G * omega_b / (omega_m * mean_molecular * M_PROTON * (ts_myr * MYR_S)) / S_STAR_REF


class HaloSourceList:
    """The sources of a step.  ``src_pos`` (3, n) 1-based int32 and ``src_flux`` (n) are what ``C2Ray.evolve3D`` and
    ``format_sources`` take, in (x, y, z)-lexicographic order.  ``n_active``; ``n_suppressed``: the cells whose LM haloes were
    suppressed; ``mass_hm``, ``mass_lm_active``, ``mass_lm_suppressed``: the summed weights of the HM haloes, of the LM haloes that
    shine at their full rate and of the suppressed ones -- the integers ``q_hm``, ``q_lm_active``, ``q_lm_suppressed`` times
    ``unit``; ``total_flux``: the sum of ``src_flux``."""

    def __init__(self, pos0, flux, summary, unit, suppression="none"):
        pos0 = np.asarray(pos0, dtype=np.int32).reshape(-1, 3)
        self.src_pos = np.ascontiguousarray(pos0.T + np.int32(1))
        self.src_flux = np.asarray(flux, dtype=np.float64)
        self.n_active, self.n_suppressed, self.q_hm, self.q_lm_active, self.q_lm_suppressed = (int(v) for v in summary)
        if self.src_flux.shape != (self.n_active,) or self.src_pos.shape != (3, self.n_active):
            raise ValueError("HaloSourceList: one position and one flux per active source")
        self.unit, self.suppression = float(unit), suppression

    mass_hm = property(lambda self: self.q_hm * self.unit)
    mass_lm_active = property(lambda self: self.q_lm_active * self.unit)
    mass_lm_suppressed = property(lambda self: self.q_lm_suppressed * self.unit)

    @property
    def total_flux(self):
        return float(math.fsum(self.src_flux))

    def log_line(self):
        """The line of the log file (one per step)."""
        return (f"Halo sources (suppression {self.suppression}): {self.n_active:n} active cells, total flux {self.total_flux:.6e}; "
                f"weight in HM haloes {self.mass_hm:.6e}, in LM haloes {self.mass_lm_active:.6e} shining and "
                f"{self.mass_lm_suppressed:.6e} suppressed in {self.n_suppressed:n} cells")

    def __repr__(self):
        return f"<HaloSourceList: {self.log_line()}>"


def halo_spec(who, N, catalogue=None, model=None, cosmology=None, scale=None, mean_molecular=MEAN_MOLECULAR):
    """The keywords of :func:`halo_sources` checked: a dict with the scale per unit weight (`N` is not needed: the table is made
    for the mesh of the device)."""
    if not isinstance(catalogue, HaloCatalogue):
        raise ValueError(f"{who}: catalogue must be a HaloCatalogue, not {type(catalogue).__name__}")
    if not isinstance(model, SourceModel):
        raise ValueError(f"{who}: model must be a SourceModel, not {type(model).__name__}")
    if (cosmology is None) == (scale is None):
        raise ValueError(f"{who}: give either cosmology (Om0 and Ob0 are read) or scale (the normalised photon rate of a unit weight "
                         f"per unit fgamma)")
    if scale is None:
        om, ob = getattr(cosmology, "Om0", None), getattr(cosmology, "Ob0", None)
        if not is_real(mean_molecular) or not (math.isfinite(mean_molecular) and mean_molecular > 0.0):
            raise ValueError(f"{who}: mean_molecular must be a finite number > 0, not {mean_molecular!r}")
        if om is None or ob is None or not (float(om) > 0.0 and float(ob) >= 0.0):
            raise ValueError(f"{who}: cosmology must have Om0 > 0 and Ob0 >= 0")
        scale = source_scale(model.ts_myr, float(ob), float(om), float(mean_molecular))
    elif not is_real(scale) or not (math.isfinite(scale) and scale >= 0.0):
        raise ValueError(f"{who}: scale must be a finite number >= 0, not {scale!r}")
    return dict(catalogue=catalogue, model=model, scale=float(scale))


def sources_on_device(lib, grid, spec):
    """The library calls for a checked `spec` (halo_spec) on device grid `grid`, as a :class:`HaloSourceList`."""
    cat, model = spec["catalogue"], spec["model"]
    cat.to_device(lib)
    out = lib.halo_sources_build(grid, model.fgamma_hm, model.fgamma_lm, cat.unit * spec["scale"], SUPPRESSIONS[model.suppression],
                                 model.x_suppress, model.f_suppressed)
    return HaloSourceList(out["pos"], out["flux"], out["summary"], cat.unit, model.suppression)


def halo_sources(catalogue, model, *, cosmology=None, scale=None, mean_molecular=MEAN_MOLECULAR, xh=None, grid=None):
    """The source list of a step, a :class:`HaloSourceList`: per occupied cell of `catalogue`
    (fgamma_hm W_hm + fgamma_lm s W_lm) scale with W the summed weights of the cell's HM and LM haloes and s the suppression of
    `model` at the cell's ionised fraction; cells with a flux of 0 leave the list.

    ``cosmology``: an object with ``Om0`` and ``Ob0`` -- the scale is then M_sun Ob0 / (Om0 ``mean_molecular`` m_p ts) / 1e48, the
    reference's normalised photon rate per solar mass and unit fgamma -- or ``scale``: that number itself.  ``xh``: an (N, N, N)
    host array for the mesh of ``device_init``; it is uploaded to the device's ionised-fraction grid, which a C2Ray object that
    keeps its grids there is told beforehand.  None: the device grid ``grid`` (a ``_capi.GRID_*`` selector, default the ionised
    fraction) is read where it lies."""
    kw = dict(catalogue=catalogue, model=model, cosmology=cosmology, scale=scale, mean_molecular=mean_molecular)
    if xh is not None:
        if grid is not None:
            raise ValueError("halo_sources: grid selects a device grid and goes with xh=None")
        xh = host_field("halo_sources", "xh", xh)
    return analyse("halo_sources", xh, grid, halo_spec, kw, sources_on_device, cuda_is_init, load_asora)
