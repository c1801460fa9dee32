"""Thin C2Ray simulation class with the reference's interface (pyc2ray/c2ray_base.py).

Holds the parameters of a run, derives the constants the hot path needs, builds the radiation tables
and forwards ``evolve3D`` / ``do_raytracing`` to the MI355X kernels.  Same YAML layout, attribute names
and method names as the reference, so its driver scripts (e.g. test/paper_tests/test1_Ifront/run_test.py)
work with ``import pyc2ray_amd as pc2r``.

Differences from the reference:
  * ``do_raytracing`` passes the heating tables (the reference's method passes 16 arguments to a
    17-argument function, c2ray_base.py:314-321, and raises TypeError).
  * Cosmology: astropy's ``FlatLambdaCDM`` is used when astropy is installed; otherwise
    ``FlatLambdaCDMLite`` below evaluates the same flat LCDM expressions (matter + Lambda + photons +
    3.04 massless neutrinos).  The lite version could not be compared with astropy in the build
    container (astropy absent), so runs that need cosmological time steps to 1e-6 should have astropy.
  * ``use_mpi`` may be ``pyc2ray_amd.dist.MPI`` (torch.distributed/RCCL) as well as mpi4py's ``MPI``.
  * ``device_resident`` (default True; single GPU): ``ndens``, ``temp``, ``xh`` and ``phi_ion`` stay on the MI355X
    between time steps and cross PCIe only when the host touches them; see :class:`C2Ray`.
  * ``Material: isothermal: false`` (optional key, default true) evolves the temperature from photo-heating and radiative
    cooling (pyc2ray_amd/thermal.py); it needs ``compute_heating_rates: 1`` and ``use_gpu``, and across ranks
    ``use_mpi = pyc2ray_amd.dist.MPI`` (the heating rates are exchanged on the TorchComm's device loops only).
  * ``Material: clumping: C`` (optional key, default 1) and the attribute ``clumping`` (a float, or an (N, N, N) grid assigned
    between steps) set the sub-grid clumping factor of the recombination rate (evolve3D's ``clumping=``).
  * ``Photo: LLS_mfp_pMpc`` / ``LLS_mfp_zref`` / ``LLS_mfp_index`` / ``LLS_per_density`` (optional keys) and the attribute ``lls``
    add the opacity of unresolved Lyman-limit systems to the raytrace (pyc2ray_amd/lls.py; evolve3D's ``lls=``).
  * ``Raytracing: periodic: 0|1`` (optional key, default 1) and the attribute ``periodic`` (a bool, assignable between steps)
    choose between traces that wrap around the box and open boundaries (evolve3D's ``periodic=``; use_gpu only).
  * ``Photo: plane_flux_face`` / ``plane_flux`` / ``plane_flux_spectrum`` (optional keys, scalars or lists of equal length) and the
    attribute ``plane_flux`` add a plane-parallel photon flux that enters through faces of the box (pyc2ray_amd/planeflux.py;
    evolve3D's ``plane_flux=``; use_gpu only).  ``plane_flux`` of the file is in photons s^-1 cm^-2.
  * ``Output: photon_budget: 0|1`` (optional key, default 0) and the attribute ``photon_budget`` (a bool, assignable between steps)
    close every time step with its photon statistics (pyc2ray_amd/budget.py; evolve3D's ``budget=``; use_gpu only): ``last_budget``,
    the cumulative ``total_budget``, and one line in the log.
  * ``bubble_sizes()`` returns the mean-free-path size distribution of the ionised regions of the current state
    (pyc2ray_amd/bubbles.py; on the device-resident path from the ionised fraction where it lies).  ``Output: bubble_sizes: 0|1``
    (optional key, default 0; with ``bubble_rays``, ``bubble_threshold``, ``bubble_seed``) and the attribute ``bubble_stats`` (a bool,
    assignable between steps) do that after every time step (use_gpu only): ``last_bubble_sizes`` and one line in the log.
  * ``regions()`` returns the connected ionised regions of the current state, their volumes and whether the largest spans the box
    (pyc2ray_amd/regions.py; on the device-resident path from the ionised fraction where it lies).  ``Output: region_sizes: 0|1``
    (optional key, default 0; with ``region_threshold``, ``region_connectivity``) and the attribute ``region_stats`` (a bool,
    assignable between steps) do that after every time step (use_gpu only): ``last_regions`` and one line in the log.
  * ``topology()`` returns the Euler characteristic, the Minkowski functionals and the Betti numbers of the ionised cells of the
    current state (pyc2ray_amd/topology.py; on the device-resident path from the ionised fraction where it lies).  ``Output:
    topology: 0|1`` (optional key, default 0; with ``topology_threshold``, ``topology_connectivity``) and the attribute
    ``topology_stats`` (a bool, assignable between steps) do that after every time step (use_gpu only): ``last_topology`` and one
    line in the log.
  * ``granulometry()`` returns the size distribution of the ionised cells of the current state by morphological opening, with the
    exact distance transform behind it (pyc2ray_amd/granulometry.py; on the device-resident path from the ionised fraction where it
    lies).  ``Output: granulometry: 0|1`` (optional key, default 0; with ``granulometry_threshold``, ``granulometry_radii``) and
    the attribute ``granulometry_stats`` (a bool, assignable between steps) do that after every time step (use_gpu only):
    ``last_granulometry`` and one line in the log.
  * ``power_spectrum()`` returns the spherically averaged power spectrum of the 21-cm brightness temperature of the current state
    -- or of the ionised or neutral fraction, the density, and cross-spectra of two of them -- with the prefactor from the object's
    cosmology and redshift (pyc2ray_amd/powerspec.py; on the device-resident path from the grids where they lie).  ``Output:
    power_spectrum: 0|1`` (optional key, default 0; with ``power_spectrum_kind``, ``power_spectrum_bins``) and the attribute
    ``power_spectrum_stats`` (a bool, assignable between steps) do that after every time step (use_gpu only):
    ``last_power_spectrum`` and one line in the log.
  * ``observed_map()`` returns the brightness temperature of the current state smoothed to a radio interferometer's resolution -- a
    Gaussian beam across the sky and a top-hat of the same comoving width along the line of sight, from a maximum baseline, the
    redshift and the cosmology, the mean removed -- with its one-point statistics (variance, skewness, kurtosis, PDF), and
    ``smoothed_field()`` the same for any filter (pyc2ray_amd/smoothing.py; on the device-resident path from the grids where they
    lie).  ``Output: observed_map: 0|1`` (optional key, default 0; with ``observed_baseline_km``, ``observed_los_axis``,
    ``observed_bins``) and the attribute ``observed_stats`` (a bool, assignable between steps) do that after every time step
    (use_gpu only): ``last_observed`` and one line in the log.
  * ``los_velocity`` (an (N, N, N) array in km/s, or None: the proper peculiar velocity along ``los_axis``), ``velocity_scale()``,
    ``power_spectrum_los()`` and ``redshift_space_field()``: the brightness temperature of the current state moved into redshift
    space and its power in (k_perp, k_par), in (k, mu) or as the multipoles P_0, P_2, P_4 (pyc2ray_amd/redshift_space.py; on the
    device-resident path from the grids where they lie; the velocity is uploaded once per assignment).  ``Output: redshift_space:
    0|1`` (optional key, default 0; with ``redshift_space_binning``, ``redshift_space_bins``, ``redshift_space_los_axis``) and the
    attribute ``redshift_space_stats`` (a bool, assignable between steps) do that after every time step (use_gpu only):
    ``last_redshift_space`` and one line in the log.  Without a velocity the spectrum is the real-space one, and the line says so.
  * ``lyman_alpha_forest()`` returns the Lyman-alpha forest of the current state along ``los_axis`` -- optical depth and transmitted
    flux on every line of the box, the effective optical depth, the flux PDF and the dark gaps -- moved by ``los_velocity``, with
    ``lyman_alpha_b_scale()`` and ``lyman_alpha_tau_scale()`` from the object's cosmology and redshift (pyc2ray_amd/lyman_alpha.py;
    on the device-resident path from the grids where they lie).  ``Output: lyman_alpha: 0|1`` (optional key, default 0; with
    ``lyman_alpha_gap_threshold``, ``lyman_alpha_bins``) and the attribute ``lyman_alpha_stats`` (a bool, assignable between steps)
    do that after every time step (use_gpu only): ``last_lyman_alpha`` and one line in the log.
  * ``Output: lightcone: 0|1`` (optional key, default 0; with ``lightcone_kind``, ``lightcone_los_axis``, ``lightcone_first_plane``,
    ``lightcone_spin``, ``lightcone_z_end``) and the attribute ``lightcone_stats`` (a bool, assignable between steps) build the light
    cone of the run while it advances (pyc2ray_amd/lightcone.py; use_gpu and cosmological runs only): every step adds the slices
    whose redshift it crossed, interpolated between the previous state and its own on the device, to ``lightcone``;
    ``last_lightcone_step`` and one line in the log.  ``brightness_temperature_scale(z)`` takes a redshift.
  * Sources from a halo catalogue (pyc2ray_amd/halo_sources.py; use_gpu only): ``halo_catalogue`` (a HaloCatalogue, assigned at
    every new snapshot) and ``source_model`` (a SourceModel; or the optional keys ``Sources: fgamma_hm / fgamma_lm / ts /
    suppression / x_suppress / f_suppressed``, with ``Sources: m_lm / m_hm`` the thresholds of ``new_halo_catalogue``) make
    ``evolve3D(dt)`` without a source list build the list of the step from the catalogue and the object's own ionised fraction --
    on the device-resident path from the grid where it lies: ``halo_sources()``, ``last_halo_sources`` and one line in the log.
"""
import atexit
import math
import re

import numpy as np
import yaml

try:
    from yaml import CSafeLoader as SafeLoader
except ImportError:  # pragma: no cover
    from yaml import SafeLoader

from .asora_core import cuda_is_init, device_close, device_init, photo_table_to_device, spectra_to_device
from . import _capi, _residency
from .evolve import evolve3D, evolve3D_MPI, evolve3D_resident
from .boundaries import periodic_spec
from .bubbles import bubble_spec, mfp_distribution, distribution_on_device
from .regions import region_spec, region_sizes, regions_on_device
from .topology import topology_spec, topology as field_topology, topology_on_device
from .granulometry import granulometry_spec, granulometry as field_granulometry, granulometry_on_device
from .powerspec import powerspec_spec, powerspec_on_device
from .smoothing import smoothing_spec, smoothing_on_device, telescope
from .redshift_space import redshift_space_spec, spectrum_on_device, field_on_device
from .lyman_alpha import lyman_alpha_spec, forest_on_device
from .bispectrum import bispectrum_spec, bispectrum_on_device
from .lightcone import LightCone, lightcone_spec
from .halo_sources import HaloCatalogue, SourceModel, halo_spec, halo_sources as catalogue_sources, sources_on_device
from .budget import StepBudget
from .lls import LLSOpacity, LLSSchedule, lls_spec
from .planeflux import PlaneFlux, plane_flux_spec
from .load_extensions import load_asora
from .radiation import BlackBodySource, make_tau_table
from .raytracing import do_raytracing
from .thermal import ThermalParams
from .utils.logutils import printlog

__all__ = ['C2Ray', 'FlatLambdaCDMLite', 'YEAR', 'Mpc']

# Conversion factors with the values the reference hard-codes (c2ray_base.py:74-80)
pc = 3.086e18
YEAR = 3.15576E+07
ev2fr = 0.241838e15                     # eV to frequency (Hz)
ev2k = 1.0 / 8.617e-05                  # eV to Kelvin
kpc = 1e3 * pc
Mpc = 1e6 * pc
msun2g = 1.98892e33
# cgs constants of the Lyman-alpha forest (CODATA 2018): lyman_alpha_b_scale, lyman_alpha_tau_scale
K_BOLTZMANN = 1.380649e-16
M_PROTON = 1.67262192369e-24
M_ELECTRON = 9.1093837015e-28
E_CHARGE = 4.80320471e-10
C_LIGHT = 2.99792458e10
LYA_F_ALPHA = 0.4164
LYA_LAMBDA_ALPHA = 1215.67e-8


class FlatLambdaCDMLite:
    """Flat LCDM background with the expressions astropy's FlatLambdaCDM(H0, Om0, Tcmb0, Ob0=...) uses
    (massless neutrinos, Neff = 3.04): E(z)^2 = Om0 (1+z)^3 + (Ogamma0 + Onu0)(1+z)^4 + Ode0.
    Only what C2Ray needs: age, lookback_time, scale_factor, and the inverse of age."""

    _G = 6.6743e-11               # CODATA 2018, SI
    _c = 299792458.0
    _sigma_sb = 5.670374419e-8
    _Mpc_m = 3.0856775814913673e22

    def __init__(self, H0, Om0, Tcmb0=0.0, Ob0=None, Neff=3.04):
        self.H0 = float(H0)
        self.Om0 = float(Om0)
        self.Ob0 = Ob0
        self.Tcmb0 = float(Tcmb0)
        self._H0_s = self.H0 * 1e3 / self._Mpc_m                       # s^-1
        rho_crit = 3.0 * self._H0_s ** 2 / (8.0 * np.pi * self._G)      # kg m^-3
        self.Ogamma0 = 4.0 * self._sigma_sb / self._c ** 3 * self.Tcmb0 ** 4 / rho_crit
        self.Onu0 = 0.22710731766 * Neff * self.Ogamma0
        self.Ode0 = 1.0 - self.Om0 - self.Ogamma0 - self.Onu0

    def efunc(self, z):
        zp1 = 1.0 + np.asarray(z, dtype=float)
        return np.sqrt(self.Om0 * zp1 ** 3 + (self.Ogamma0 + self.Onu0) * zp1 ** 4 + self.Ode0)

    def scale_factor(self, z):
        return 1.0 / (1.0 + z)

    def age(self, z):
        """Age of the universe at redshift z, in seconds."""
        from scipy.integrate import quad
        # t = 1/H0 int_0^{a} da' / (a' E(a'))  with a = 1/(1+z)
        a = 1.0 / (1.0 + z)
        f = lambda x: 1.0 / (x * float(self.efunc(1.0 / x - 1.0)))
        val, _ = quad(f, 0.0, a, epsabs=0.0, epsrel=1e-12, limit=200)
        return val / self._H0_s

    def lookback_time(self, z):
        return self.age(0.0) - self.age(z)

    def comoving_distance(self, z):
        """The line-of-sight comoving distance to redshift z, in Mpc: c / H0 int_0^z dz' / E(z')."""
        from scipy.integrate import quad
        val, _ = quad(lambda x: 1.0 / float(self.efunc(x)), 0.0, float(z), epsabs=0.0, epsrel=1e-12, limit=200)
        return self._c / 1e3 / self.H0 * val

    def z_at_age(self, t):
        from scipy.optimize import brentq
        return brentq(lambda z: self.age(z) - t, -0.5, 1e4, xtol=1e-12, rtol=1e-12)


def _make_cosmology(H0, Om0, Tcmb0, Ob0):
    try:
        from astropy.cosmology import FlatLambdaCDM
        return FlatLambdaCDM(H0, Om0, Tcmb0, Ob0=Ob0), True
    except ImportError:
        return FlatLambdaCDMLite(H0, Om0, Tcmb0, Ob0=Ob0), False


class _DeviceGrid:
    """A grid attribute of C2Ray that may live on the device (see C2Ray.device_resident).  The host array is the
    attribute's value as always; what is tracked is which side holds the current data.  Reading the attribute hands
    out the host array, which the caller may then write into, so every read marks the device copy as out of date
    (and first fetches the data if the device holds the newer one); assigning replaces the host array."""

    def __init__(self, name, which):
        self.name, self.which = name, which

    def __set_name__(self, owner, attr):
        self.attr = "_grid_" + attr

    def __get__(self, obj, objtype=None):
        if obj is None:
            return self
        try:
            arr = obj.__dict__[self.attr]
        except KeyError:
            raise AttributeError(self.name) from None
        if self.name in obj._device_newer:                   # results of the last step(s) still only on the device
            lib = load_asora()
            order = 'F' if (arr.flags.f_contiguous and not arr.flags.c_contiguous) else 'C'
            if self.name in ("xh", "phi_ion", "temp"):      # (temp: only a non-isothermal run changes it on the device)
                # into a FRESH array, as the reference binds a fresh array per step (c2ray_base.py:205-226): a caller that keeps
                # `prev = sim.xh` or appends sim.xh to a history must not see it change under its feet
                arr = lib.grid_to_host(self.which, lib.host_empty(arr.shape, order=order))
                obj.__dict__[self.attr] = arr
            else:
                # an input grid changed on the device (the density, diluted by cosmo_evolve): into the caller's OWN array, as the
                # reference scales it in place (c2ray_base.py:248) -- a reference kept to it sees the dilution
                if not (arr.flags.writeable and (arr.flags.c_contiguous or arr.flags.f_contiguous) and arr.dtype == np.float64):
                    arr = lib.host_empty(arr.shape, order=order)
                    obj.__dict__[self.attr] = arr
                lib.grid_to_host(self.which, arr)
                obj.__dict__.setdefault("_grid_fingerprints", {})[self.name] = obj._fingerprint(arr)
            obj._device_newer.discard(self.name)
        obj._host_newer.add(self.name)                       # the caller may modify what it gets
        return arr

    def __set__(self, obj, value):
        obj.__dict__[self.attr] = value
        obj._device_newer.discard(self.name)
        obj._host_newer.add(self.name)


class _StepStatistic:
    """A statistic that C2Ray can take after every time step, declared once: the attribute is its switch, a bool assignable
    between steps.  `key`: its ``Output:`` key (0 | 1; absent: 0), the switch's value at construction.  `last`: the attribute a
    step leaves the result in.  `method`: the method of C2Ray that computes it after the step (None: the step fills it itself).
    `needs_gpu`: why True is refused on an object without use_gpu.  `doc`: the attribute's docstring.  `keys`: the further
    ``Output:`` keys, each with the keyword of `method` whose default it sets.  ``validate(sim, kw)``: raises ValueError at
    construction for what a call with those keywords would refuse.  C2Ray._statistic_init and C2Ray._close_step use all of it."""

    def __init__(self, key, last, method, needs_gpu, doc, keys=(), validate=None):
        self.key, self.last, self.method, self.needs_gpu, self.keys, self.validate = key, last, method, needs_gpu, keys, validate
        self.__doc__ = doc

    def __set_name__(self, owner, attr):
        self.name, self.attr = attr, "_" + attr

    def __get__(self, obj, objtype=None):
        if obj is None:
            return self
        return obj.__dict__.get(self.attr, False)              # (an object that never read its keys: off)

    def __set__(self, obj, value):
        self.set(obj, value, f"C2Ray.{self.name}")

    def set(self, obj, value, who):
        if not isinstance(value, (bool, np.bool_)):
            raise ValueError(f"{who}: {self.name} must be a bool, not {type(value).__name__}")
        if value and not obj.gpu:
            raise ValueError(f"{who}: {self.name} needs use_gpu=True ({self.needs_gpu})")
        obj.__dict__[self.attr] = bool(value)

    def defaults(self, obj):
        """The keywords that the ``Output:`` keys of `obj` set for the method."""
        return obj.__dict__.get(self.attr + "_defaults", {})


class _LightConeStatistic(_StepStatistic):
    """The switch of the light cone: on only where a redshift passes; switching it on begins a new cone -- the first step
    afterwards keeps its field and emits nothing."""

    def set(self, obj, value, who):
        was = obj.__dict__.get(self.attr, False)
        super().set(obj, value, who)
        if value and not getattr(obj, "cosmological", False):
            obj.__dict__[self.attr] = False
            raise ValueError(f"{who}: {self.name} needs a cosmological run (Cosmology: cosmological: 1): no redshift passes without")
        obj.__dict__.setdefault("lightcone", None)
        if value and not was:                                  # (switched off, the cone stays where a driver can take it)
            obj.__dict__["lightcone"] = None
            obj.__dict__["_lightcone_z_prev"] = None


class C2Ray:
    #: Default since round 6 (single GPU, use_gpu=True; set False on an instance for the reference's behaviour: every step uploads
    #: and downloads everything): ndens, temp, xh and phi_ion stay on the device between time steps.  evolve3D then uploads only
    #: the grids that were assigned or READ on the host since the last step (a read hands out the array, which may be written
    #: into), and downloads xh / phi_ion only when they are read; cosmo_evolve dilutes a density that lives on the device ON the
    #: device.  At 256^3 the five 128 MiB transfers of a time step cost as much as the step's outer iterations (33.2 against
    #: 17.4 ms per time step, profiles/r06_time_steps_resident.json).  xh and phi_ion behave as in the reference: every step
    #: binds a FRESH array (c2ray_base.py:205-226), an array kept from an earlier step keeps that step's values.  ndens and temp
    #: are the caller's arrays; writing into one through a reference kept from BEFORE the last step, without touching the
    #: attribute again (``n = sim.ndens`` ... evolve3D ... ``n *= 2``), is caught by a fingerprint of 16 384 samples of the host
    #: array taken at upload time (0.1 ms per grid and step at 256^3; any rescaling or whole-grid update changes it, an edit of a few cells may not: assign or read
    #: the attribute after such an edit, as ``sim.ndens[...] = v`` does by itself): the grid is uploaded again -- or, if the
    #: device copy has meanwhile been diluted by cosmo_evolve, so that the write went into stale values, a RuntimeError says so.
    device_resident = True
    _FINGERPRINT_SAMPLES = 16384

    ndens = _DeviceGrid("ndens", _capi.GRID_NDENS)
    temp = _DeviceGrid("temp", _capi.GRID_TEMP)
    xh = _DeviceGrid("xh", _capi.GRID_XH)
    phi_ion = _DeviceGrid("phi_ion", _capi.GRID_PHI_ION)

    # The statistics of a time step.  A new one is one declaration here, its name in _STEP_STATISTICS and its method.
    photon_budget = _StepStatistic(
        "photon_budget", "last_budget", None, "the use_gpu=False loop takes no photon budget",
        """Is every time step closed with its photon budget (pyc2ray_amd.budget.StepBudget; use_gpu=True only: on an object
        without, True is refused at the assignment)?  A driver may assign a bool between steps.  After a step ``last_budget``
        holds the step's budget and ``total_budget`` the sum since the object was made; rank 0 writes one line to the log.  The
        sums are reduced on the device: no grid crosses PCIe for them, on the device-resident path either.""")
    # bubble_rays: an integer >= 0, default 100000; bubble_threshold: a finite number, default 0.5; bubble_seed: an integer in
    # [0, 2^64), default 0
    bubble_stats = _StepStatistic(
        "bubble_sizes", "last_bubble_sizes", "bubble_sizes", "the rays are marched on the device",
        """Does every time step end with the size distribution of its ionised regions (:meth:`bubble_sizes` with the ``Output:
        bubble_*`` keys; use_gpu=True only: on an object without, True is refused at the assignment)?  A driver may assign a bool
        between steps.  After a step ``last_bubble_sizes`` holds the result and rank 0 writes one line to the log.""",
        keys=(("bubble_rays", "n_rays"), ("bubble_threshold", "threshold"), ("bubble_seed", "seed")),
        validate=lambda sim, kw: bubble_spec("Output: bubble_rays / bubble_threshold / bubble_seed", sim.N, **kw))
    # region_threshold: a finite number, default 0.5; region_connectivity: 6 or 26, default 6  (the keys only are checked at
    # construction, here and below: a mesh beyond the entry's limit is refused by a call)
    region_stats = _StepStatistic(
        "region_sizes", "last_regions", "regions", "the regions are labelled on the device",
        """Does every time step end with the connected regions of its ionised fraction (:meth:`regions` with the ``Output:
        region_*`` keys; use_gpu=True only: on an object without, True is refused at the assignment)?  A driver may assign a bool
        between steps.  After a step ``last_regions`` holds the result and rank 0 writes one line to the log.""",
        keys=(("region_threshold", "threshold"), ("region_connectivity", "connectivity")),
        validate=lambda sim, kw: region_spec("Output: region_threshold / region_connectivity", None, **kw))
    # topology_threshold: a finite number, default 0.5; topology_connectivity: 6 or 26, default 6
    topology_stats = _StepStatistic(
        "topology", "last_topology", "topology", "the elements are counted and the phases labelled on the device",
        """Does every time step end with the topology of its ionised fraction (:meth:`topology` with the ``Output: topology_*``
        keys; use_gpu=True only: on an object without, True is refused at the assignment)?  A driver may assign a bool between
        steps.  After a step ``last_topology`` holds the result and rank 0 writes one line to the log.""",
        keys=(("topology_threshold", "threshold"), ("topology_connectivity", "connectivity")),
        validate=lambda sim, kw: topology_spec("Output: topology_threshold / topology_connectivity", None, **kw))
    # granulometry_threshold: a finite number, default 0.5; granulometry_radii: an int n for the radii 1 ... n, or a list of
    # ascending radii, default 1 ... max(1, min(N // 4, 32))
    granulometry_stats = _StepStatistic(
        "granulometry", "last_granulometry", "granulometry", "the distance transform and the openings run on the device",
        """Does every time step end with the granulometry of its ionised fraction (:meth:`granulometry` with the ``Output:
        granulometry_*`` keys; use_gpu=True only: on an object without, True is refused at the assignment)?  A driver may assign a
        bool between steps.  After a step ``last_granulometry`` holds the result and rank 0 writes one line to the log.""",
        keys=(("granulometry_threshold", "threshold"), ("granulometry_radii", "radii")),
        validate=lambda sim, kw: granulometry_spec("Output: granulometry_threshold / granulometry_radii", None, **kw))
    # power_spectrum_kind: 'xh', 'xhi', 'density', 'hi' or 'dtb', default 'dtb'; power_spectrum_bins: an int n for n equal bins, or
    # a list of ascending edges in units of the fundamental mode, default unit-width bins
    power_spectrum_stats = _StepStatistic(
        "power_spectrum", "last_power_spectrum", "power_spectrum", "the transform and the binning run on the device",
        """Does every time step end with the power spectrum of its state (:meth:`power_spectrum` with the ``Output:
        power_spectrum_*`` keys; use_gpu=True only: on an object without, True is refused at the assignment)?  A driver may assign a
        bool between steps.  After a step ``last_power_spectrum`` holds the result and rank 0 writes one line to the log.""",
        keys=(("power_spectrum_kind", "kind"), ("power_spectrum_bins", "bins")),
        validate=lambda sim, kw: powerspec_spec("Output: power_spectrum_kind / power_spectrum_bins", None, **kw))
    # observed_baseline_km: a number > 0, default 2; observed_los_axis: 0, 1 or 2, default 2; observed_bins: an int n for n equal
    # bins over the map's range, or a list of ascending edges in mK, default no histogram
    observed_stats = _StepStatistic(
        "observed_map", "last_observed", "observed_map", "the transforms and the statistics run on the device",
        """Does every time step end with the observed map of its state (:meth:`observed_map` with the ``Output: observed_*`` keys;
        use_gpu=True only: on an object without, True is refused at the assignment)?  A driver may assign a bool between steps.
        After a step ``last_observed`` holds the result and rank 0 writes one line to the log.""",
        keys=(("observed_baseline_km", "baseline_km"), ("observed_los_axis", "los_axis"), ("observed_bins", "bins")),
        validate=lambda sim, kw: sim._observed_keys_spec(kw))
    # redshift_space_binning: 'cylindrical', 'mu' or 'multipoles', default 'multipoles'; redshift_space_bins: an int n for n equal
    # bins of k (of k_perp and of k_par with 'cylindrical'), or a list of ascending edges in units of the fundamental mode, default
    # unit-width bins; redshift_space_los_axis: 0, 1 or 2, default 2, which is also the object's ``los_axis`` until that is assigned
    redshift_space_stats = _StepStatistic(
        "redshift_space", "last_redshift_space", "power_spectrum_los", "the mapping, the transform and the binning run on the device",
        """Does every time step end with the redshift-space power spectrum of its state (:meth:`power_spectrum_los` with the
        ``Output: redshift_space_*`` keys and ``los_velocity``; use_gpu=True only: on an object without, True is refused at the
        assignment)?  A driver may assign a bool between steps.  After a step ``last_redshift_space`` holds the result and rank 0
        writes one line to the log.""",
        keys=(("redshift_space_binning", "binning"), ("redshift_space_bins", "bins"), ("redshift_space_los_axis", "los_axis")),
        validate=lambda sim, kw: sim._redshift_space_keys_spec(kw))
    #: the order in which __init__ reads their keys and a step writes their lines to the log
    _STEP_STATISTICS = ("photon_budget", "bubble_stats", "region_stats", "topology_stats", "granulometry_stats", "power_spectrum_stats",
                        "observed_stats")
    # lyman_alpha_gap_threshold: a finite number, default 0.05; lyman_alpha_bins: an int n for n equal bins of the transmitted flux
    # over [0, 1], or a list of non-decreasing edges, default 20 bins
    lyman_alpha_stats = _StepStatistic(
        "lyman_alpha", "last_lyman_alpha", "lyman_alpha_forest", "the optical depth, the statistics and the gaps run on the device",
        """Does every time step end with the Lyman-alpha forest of its state (:meth:`lyman_alpha_forest` with the ``Output:
        lyman_alpha_*`` keys and ``los_velocity``; use_gpu=True only: on an object without, True is refused at the assignment)?  A
        driver may assign a bool between steps.  After a step ``last_lyman_alpha`` holds the result and rank 0 writes one line to
        the log.""",
        keys=(("lyman_alpha_gap_threshold", "gap_threshold"), ("lyman_alpha_bins", "bins")),
        validate=lambda sim, kw: lyman_alpha_spec("Output: lyman_alpha_gap_threshold / lyman_alpha_bins", None, b_scale=1.0, tau_scale=1.0, **kw))
    #: the statistics declared since, behind those: read, computed and logged after them
    _STEP_STATISTICS_APPENDED = ("redshift_space_stats",)
    #: ... and those declared since then, behind both (the two tuples above keep the contents their tests pin)
    _STEP_STATISTICS_FURTHER = ("lyman_alpha_stats",)
    # lightcone_kind: 'dtb' (default), 'hi', 'xh', 'xhi' or 'density'; lightcone_los_axis: 0, 1 or 2, default the object's
    # ``los_axis``; lightcone_first_plane: an int in [0, N), default 0; lightcone_spin: None (default) or 'kinetic';
    # lightcone_z_end: the redshift below which no slice is emitted, default none
    lightcone_stats = _LightConeStatistic(
        "lightcone", "last_lightcone_step", "_lightcone_step", "the slices are formed and blended on the device",
        """Does every time step add the slices it crossed to the light cone of the run (pyc2ray_amd.lightcone.LightCone with the
        ``Output: lightcone_*`` keys; use_gpu=True and a cosmological run only: elsewhere True is refused at the assignment)?  A
        driver may assign a bool between steps; switching on begins a new cone, whose first step keeps its field and emits
        nothing.  ``lightcone`` is the cone (it stays after switching off); after a step ``last_lightcone_step`` holds what the
        step emitted and rank 0 writes one line to the log.""",
        keys=(("lightcone_kind", "kind"), ("lightcone_los_axis", "los_axis"), ("lightcone_first_plane", "first_plane"),
              ("lightcone_spin", "spin"), ("lightcone_z_end", "z_end")),
        validate=lambda sim, kw: lightcone_spec("Output: lightcone_kind / lightcone_los_axis / lightcone_first_plane / lightcone_spin / "
                                                "lightcone_z_end", sim.N, **{"kind": "dtb", **kw}))
    #: what closes a step without being a statistic of its state: the light cone, which accumulates over the steps
    _STEP_ACCUMULATORS = ("lightcone_stats",)

    @classmethod
    def _step_statistics(cls):
        """Every declared statistic of a state, in the order in which __init__ reads their keys and a step computes and logs them."""
        return cls._STEP_STATISTICS + cls._STEP_STATISTICS_APPENDED + cls._STEP_STATISTICS_FURTHER

    @classmethod
    def _step_closers(cls):
        """Everything the mechanism of _statistic_init and _close_step serves: the statistics, then the accumulators."""
        return cls._step_statistics() + cls._STEP_ACCUMULATORS

    def __init__(self, paramfile, Nmesh, use_gpu, use_mpi):
        """Basis class of a C2Ray simulation (pyc2ray/c2ray_base.py:82-145).

        paramfile : YAML parameter file (same keys as the reference's parameters.yml files)
        Nmesh     : mesh size
        use_gpu   : True = ASORA path, device-resident; False = the semantics of the reference's CPU raytracer
                    (sub-boxes, photon loss), evaluated on the GPU through the libc2ray-compatible entry points
        use_mpi   : None/False, mpi4py's MPI module, or pyc2ray_amd.dist.MPI
        """
        self._host_newer = set()           # grids whose host array holds newer data than the device
        self._device_newer = set()         # grids whose device copy holds newer data than the host array
        if use_mpi:
            self.mpi = use_mpi
            self.comm = use_mpi.COMM_WORLD
            self.rank = self.comm.Get_rank()
            self.nprocs = self.comm.Get_size()
        else:
            self.mpi = False
            self.rank = 0
            self.nprocs = 1

        self._read_paramfile(paramfile)
        self._thermal_mode_init(use_gpu, use_mpi)
        self._clumping_init()
        self.N = Nmesh
        self.shape = (Nmesh, Nmesh, Nmesh)

        if use_gpu:
            self.gpu = True
            src_batch_size = self._ld["Raytracing"]["source_batch_size"]
            device_init(Nmesh, src_batch_size)
            atexit.register(self._gpu_close)
        else:
            self.gpu = False

        self._param_init()
        self._output_init()
        self._grid_init()
        self._cosmology_init()
        self._redshift_init()
        self._material_init()
        self._sources_init()
        self._radiation_init()
        self._lls_init()
        self._boundaries_init()
        self._plane_flux_init()
        self._halo_sources_init()
        for name in self._step_closers():
            self._statistic_init(name)
        if self.rank == 0:
            if self.gpu:
                q_max = np.ceil(1.73205080757 * min(self.R_max_LLS, 1.73205080757 * self.N / 2))
                self.printlog(f"Using ASORA Raytracing ( q_max = {q_max : n} )")
            else:
                self.printlog(f"Using CPU Raytracing (subboxsize = {self.subboxsize : n}, max_subbox = {self.max_subbox : n})")
            if self.mpi:
                self.printlog(f"Using {self.nprocs:n} MPI Ranks")
            else:
                self.printlog("Running in non-MPI (single-GPU/CPU) mode")
            self.printlog("Starting simulation... \n\n")

    # ---- time evolution -------------------------------------------------------------------------
    def set_timestep(self, z1, z2, num_timesteps):
        """Time step (s) between two redshift slices (c2ray_base.py:147-168)."""
        t1 = self._lookback_s(z1)
        t2 = self._lookback_s(z2)
        return (t1 - t2) / num_timesteps

    def _thermal_mode_init(self, use_gpu, use_mpi):
        """The optional key ``Material: isothermal`` (absent: true, the reference's behaviour).  A non-isothermal run evolves
        the temperature from the photo-heating rates: on one GPU, or across ranks with pyc2ray_amd.dist.MPI, whose communicator
        exchanges the heating rates with the photo-ionisation rates; with any other MPI module it is single-GPU only."""
        self.isothermal = bool(self._ld.get('Material', {}).get('isothermal', True))
        if self.isothermal:
            return
        if not self._ld.get('Photo', {}).get('compute_heating_rates', 0):
            raise ValueError("Material: isothermal: false needs the photo-heating rates (Photo: compute_heating_rates: 1)")
        if not use_gpu:
            raise ValueError("Material: isothermal: false needs use_gpu=True (the use_gpu=False raytracer has no thermal form)")
        from . import dist
        if use_mpi and use_mpi is not dist.MPI:
            raise ValueError("Material: isothermal: false is single-GPU only with this use_mpi (across ranks: "
                             "use_mpi = pyc2ray_amd.dist.MPI)")

    def _thermal_params(self):
        """The ThermalParams of the current step (None when isothermal); Compton exchange with the CMB at self.zred in
        cosmological runs."""
        if self.isothermal:
            return None
        return ThermalParams(self.heat_thin_table, self.heat_thick_table,
                             zred=float(self.zred) if self.cosmological else None,
                             tcmb0=float(self._ld['Cosmology']['cmbtemp']))

    def _clumping_init(self):
        """The optional key ``Material: clumping`` (absent: 1, the reference's behaviour): one sub-grid clumping factor
        C = <n^2>/<n>^2 of the recombination rate for the whole run, until ``clumping`` is assigned."""
        c = self._ld.get('Material', {}).get('clumping', 1.0)
        if isinstance(c, bool) or not isinstance(c, (int, float)) or not (np.isfinite(c) and c > 0):
            raise ValueError(f"Material: clumping must be a finite number > 0, not {c!r}")
        self.__dict__["_clumping"] = float(c)

    @property
    def clumping(self):
        """The clumping factor of the next steps: a float (1: off), or an (N, N, N) float64 grid of factors.  A driver may assign
        either between steps (a redshift-dependent fit, a clumping field of its own).  On the device-resident path a grid stays on
        the device across steps and is uploaded again only when the attribute was assigned or READ since the last step (a read
        hands out the array, which may be written into)."""
        c = self.__dict__.get("_clumping", 1.0)
        if isinstance(c, np.ndarray):
            self._host_newer.add("clumping")
        return c

    @clumping.setter
    def clumping(self, value):
        from .evolve import _clumping_spec
        _clumping_spec(value, self.N)                          # ValueError for what evolve3D would refuse, now
        if not (isinstance(value, np.ndarray) and value.ndim == 3):
            value = 1.0 if value is None else float(value)
        self.__dict__["_clumping"] = value
        self._host_newer.add("clumping")

    def _lls_init(self):
        """The optional ``Photo`` keys of :class:`pyc2ray_amd.lls.LLSSchedule` (none present: no LLS opacity, the reference's
        behaviour): ``lls_schedule``, and from it the opacity at the run's starting redshift."""
        self.lls_schedule = LLSSchedule.from_photo_keys(self._ld.get('Photo', {}), self.sig, self.zred_0)
        self.__dict__["_lls"] = None
        if self.lls_schedule is not None:
            self.__dict__["_lls"] = self.lls_schedule.at(self.zred_0)
            if self.rank == 0:
                self.printlog(f"LLS opacity at z = {self.zred_0:.3f}: n_const = {self._lls.n_const:.3e} cm^-3, "
                              f"per_density = {self._lls.per_density:.3e}")

    @property
    def lls(self):
        """The LLS opacity of the next steps: None (off) or a :class:`pyc2ray_amd.lls.LLSOpacity`.  A driver may assign either
        between steps.  In a cosmological run with the ``Photo: LLS_*`` keys, cosmo_evolve re-evaluates ``lls_schedule`` at the new
        redshift and replaces it; set ``lls_schedule = None`` to keep an assigned value."""
        return self.__dict__.get("_lls")

    @lls.setter
    def lls(self, value):
        lls_spec(value, "C2Ray.lls")                            # ValueError for what evolve3D would refuse, now
        self.__dict__["_lls"] = value

    def _boundaries_init(self):
        """The optional key ``Raytracing: periodic`` (0 | 1; absent: 1, the reference's behaviour): whether the traces wrap around
        the box, until ``periodic`` is assigned."""
        v = self._ld.get('Raytracing', {}).get('periodic', 1)
        if isinstance(v, (bool, np.bool_)):
            v = int(v)
        if not isinstance(v, (int, np.integer)) or v not in (0, 1):
            raise ValueError(f"Raytracing: periodic must be 0 or 1, not {v!r}")
        self.__dict__["_periodic"] = periodic_spec(bool(v), "Raytracing: periodic: 0", self.gpu)     # (0 needs use_gpu: said now)
        if not self.__dict__["_periodic"] and self.rank == 0:
            self.printlog("Open (non-periodic) boundaries for the raytrace")

    @property
    def periodic(self):
        """Do the traces of the next steps wrap around the box (True, the default) or end at its faces (False: open boundaries,
        use_gpu=True only: on an object without, False is refused at the assignment)?  A driver may assign either between steps."""
        return self.__dict__.get("_periodic", True)

    @periodic.setter
    def periodic(self, value):
        self.__dict__["_periodic"] = periodic_spec(value, "C2Ray.periodic", self.gpu)      # ValueError for what evolve3D would refuse, now

    def _plane_flux_init(self):
        """The optional keys ``Photo: plane_flux_face`` (names of :data:`pyc2ray_amd.planeflux.FACES`, or 0 ... 5), ``plane_flux``
        (photons s^-1 cm^-2; divided by 1e48 here, like the source strengths) and ``plane_flux_spectrum`` (default 0): each a
        scalar or a list, of one length.  None present: no faces, until ``plane_flux`` is assigned."""
        photo = self._ld.get('Photo', {})
        self.__dict__["_plane_flux"] = ()
        present = [k for k in ("plane_flux_face", "plane_flux", "plane_flux_spectrum") if k in photo]
        if not present:
            return
        if "plane_flux_face" not in photo or "plane_flux" not in photo:
            raise ValueError("Photo: plane_flux_face and plane_flux come together")
        as_list = lambda v: list(v) if isinstance(v, (list, tuple)) else [v]
        faces, fluxes = as_list(photo["plane_flux_face"]), as_list(photo["plane_flux"])
        spectra = as_list(photo.get("plane_flux_spectrum", [0] * len(faces)))
        if not (len(faces) == len(fluxes) == len(spectra)):
            raise ValueError(f"Photo: plane_flux_face, plane_flux and plane_flux_spectrum must have one length, not "
                             f"{len(faces)}, {len(fluxes)}, {len(spectra)}")
        for x in fluxes:
            if isinstance(x, bool) or not isinstance(x, (int, float)):
                raise ValueError(f"Photo: plane_flux must be a number or a list of numbers, not {x!r}")
        value = [PlaneFlux(f, x / 1e48, s) for f, x, s in zip(faces, fluxes, spectra)]
        self.__dict__["_plane_flux"] = plane_flux_spec(value, "Photo: plane_flux", self.gpu)      # (faces need use_gpu: said now)
        if self.rank == 0:
            for f in self.__dict__["_plane_flux"]:
                self.printlog(f"Plane-parallel flux through the {f.name} face: {f.flux * 1e48:.3e} photons/s/cm^2")

    @property
    def plane_flux(self):
        """The plane-parallel fluxes of the next steps: a tuple of :class:`pyc2ray_amd.planeflux.PlaneFlux` (empty: none).  A
        driver may assign None, one PlaneFlux or a sequence of them between steps (use_gpu=True only)."""
        return self.__dict__.get("_plane_flux", ())

    @plane_flux.setter
    def plane_flux(self, value):
        self.__dict__["_plane_flux"] = plane_flux_spec(value, "C2Ray.plane_flux", self.gpu)    # ValueError for what evolve3D would refuse, now

    # ---- statistics of a time step (the _StepStatistic declarations above) -------------------------
    def _statistic_init(self, name):
        """The ``Output:`` keys of the statistic declared as `name`: its own key (0 | 1; absent: 0) is the switch until that is
        assigned; its further keys, checked now, are the defaults of its method; ``last_*`` starts empty."""
        stat = getattr(type(self), name)
        out = self._ld.get('Output') or {}
        v = out.get(stat.key, 0)
        if isinstance(v, (bool, np.bool_)):
            v = int(v)
        if not isinstance(v, (int, np.integer)) or v not in (0, 1):
            raise ValueError(f"Output: {stat.key} must be 0 or 1, not {v!r}")
        kw = {keyword: out[key] for key, keyword in stat.keys if key in out}
        if stat.validate is not None:
            stat.validate(self, kw)                             # ValueError for what a call would refuse, now
        self.__dict__[stat.attr + "_defaults"] = kw
        setattr(self, stat.last, None)
        if name == "photon_budget":                             # (the one statistic that is also summed over the run)
            self.total_budget = StepBudget()
        stat.set(self, bool(v), f"Output: {stat.key}: 1")

    def _close_step(self, budget):
        """The end of a time step.  The photon budget is filled by the step itself: `budget` (None: off) becomes last_budget, joins
        total_budget and the log.  Every other statistic that is switched on is computed now, by its method, from the state the
        step left: the result becomes its ``last_*`` and joins the log.  Off: no call, and ``last_*`` is left alone."""
        if budget is not None:
            self.last_budget = budget
            self.total_budget = self.__dict__.get("total_budget", StepBudget()) + budget
            if self.rank == 0:
                self.printlog(budget.log_line())
        for name in self._step_closers():
            stat = getattr(type(self), name)
            if stat.method is not None and getattr(self, name):
                result = getattr(self, stat.method)()
                setattr(self, stat.last, result)
                if self.rank == 0:
                    self.printlog(result.log_line())

    def _analyse_xh(self, method, defaults, kw, spec, on_device, entry):
        """The body of `method`, an analysis of the object's own ionised fraction with the keywords `kw` over `defaults`: on the
        device grid where it lies while the last step's ``xh`` is there only, ``on_device(lib, grid, spec(who, N, **kw))``, else
        through the module's ``entry(self.xh, **kw)``, which uploads the host array."""
        for name in ("field", "grid"):
            if name in kw:
                raise ValueError(f"C2Ray.{method}: {name} is not for the class (it analyses its own ionised fraction)")
        kw = {**defaults, "periodic": self.periodic, "dr": self.dr, **kw}
        if self.device_resident and self.gpu and not self.mpi and "xh" in self._device_newer and cuda_is_init():
            return on_device(load_asora(), _capi.GRID_XH, spec(f"C2Ray.{method}", self.N, **kw))
        return entry(self.xh, **kw)

    def bubble_sizes(self, **kw):
        """The mean-free-path size distribution of the ionised regions of the current state, a
        :class:`pyc2ray_amd.bubbles.BubbleSizes`; the keywords of :func:`pyc2ray_amd.bubbles.mfp_distribution` but ``field`` and
        ``grid``, with ``periodic`` = ``self.periodic`` and ``dr`` = ``self.dr`` unless given, and the ``Output: bubble_*`` keys of
        the parameter file for ``n_rays``, ``threshold`` and ``seed``.  While the ionised fraction of the last step lives on the
        device only (``device_resident``), it is analysed there: nothing is downloaded, and ``xh`` stays where it is.  Otherwise --
        with ``use_mpi`` too -- the host array is uploaded and analysed; every rank computes the same result from its own copy."""
        return self._analyse_xh("bubble_sizes", C2Ray.bubble_stats.defaults(self), kw, bubble_spec, distribution_on_device, mfp_distribution)

    def regions(self, **kw):
        """The connected ionised regions of the current state, a :class:`pyc2ray_amd.regions.RegionSizes`; the keywords of
        :func:`pyc2ray_amd.regions.region_sizes` but ``field`` and ``grid``, with ``periodic`` = ``self.periodic`` and ``dr`` =
        ``self.dr`` unless given, and the ``Output: region_*`` keys of the parameter file for ``threshold`` and ``connectivity``.
        While the ionised fraction of the last step lives on the device only (``device_resident``), it is analysed there: nothing
        is downloaded, and ``xh`` stays where it is.  Otherwise -- with ``use_mpi`` too -- the host array is uploaded and analysed;
        every rank computes the same result from its own copy."""
        return self._analyse_xh("regions", C2Ray.region_stats.defaults(self), kw, region_spec, regions_on_device, region_sizes)

    def topology(self, **kw):
        """The topology of the ionised cells of the current state, a :class:`pyc2ray_amd.topology.Topology`; the keywords of
        :func:`pyc2ray_amd.topology.topology` but ``field`` and ``grid``, with ``periodic`` = ``self.periodic`` and ``dr`` =
        ``self.dr`` unless given, and the ``Output: topology_*`` keys of the parameter file for ``threshold`` and ``connectivity``.
        While the ionised fraction of the last step lives on the device only (``device_resident``), it is analysed there: nothing
        is downloaded, and ``xh`` stays where it is.  Otherwise -- with ``use_mpi`` too -- the host array is uploaded and analysed;
        every rank computes the same result from its own copy."""
        return self._analyse_xh("topology", C2Ray.topology_stats.defaults(self), kw, topology_spec, topology_on_device, field_topology)

    def granulometry(self, **kw):
        """The granulometry of the ionised cells of the current state, a :class:`pyc2ray_amd.granulometry.Granulometry`; the keywords
        of :func:`pyc2ray_amd.granulometry.granulometry` but ``field`` and ``grid``, with ``periodic`` = ``self.periodic`` and ``dr``
        = ``self.dr`` unless given, and the ``Output: granulometry_*`` keys of the parameter file for ``threshold`` and ``radii``.
        While the ionised fraction of the last step lives on the device only (``device_resident``), it is analysed there: nothing
        is downloaded, and ``xh`` stays where it is.  Otherwise -- with ``use_mpi`` too -- the host array is uploaded and analysed;
        every rank computes the same result from its own copy."""
        return self._analyse_xh("granulometry", C2Ray.granulometry_stats.defaults(self), kw, granulometry_spec, granulometry_on_device,
                                field_granulometry)

    def brightness_temperature_scale(self, z=None):
        """The prefactor of the 21-cm differential brightness temperature at redshift `z` (None: ``self.zred``) in mK, from the
        object's own cosmology: 27 sqrt((1 + z) / 10  0.15 / (Omega_m h^2)) (Omega_b h^2 / 0.023)."""
        cs = self._ld['Cosmology']
        h2 = float(cs['h']) ** 2
        z = float(self.zred) if z is None else float(z)
        return 27.0 * math.sqrt((1.0 + z) / 10.0 * 0.15 / (float(cs['Omega0']) * h2)) * (float(cs['Omega_B']) * h2 / 0.023)

    def _spin_t_gamma(self, who, kw):
        """``spin`` leaves the keywords `kw` of a transform analysis: 'kinetic' puts ``t_gamma``, the CMB temperature at
        ``self.zred``, in its place."""
        spin = kw.pop("spin", None)
        if spin not in (None, "kinetic"):
            raise ValueError(f"{who}: spin must be None or 'kinetic', not {spin!r}")
        if spin == "kinetic":
            if "t_gamma" in kw:
                raise ValueError(f"{who}: spin='kinetic' sets t_gamma itself")
            kw["t_gamma"] = float(self._ld['Cosmology']['cmbtemp']) * (1.0 + float(self.zred))

    def _state_on_device(self, overwritten=False):
        """The library, with the object's ionised fraction, density and temperature on the device: where they lie while the last
        step's ``xh`` is there only and the host has touched neither of the other two, else -- or if the call to come will have
        `overwritten` a grid -- uploaded from the host arrays."""
        if not cuda_is_init():
            raise RuntimeError("GPU not initialized. Please initialize it by calling device_init(N)")
        lib = load_asora()
        stale = {"ndens", "temp"} & self._host_newer
        resident = self.device_resident and self.gpu and not self.mpi and "xh" in self._device_newer and not stale
        if not resident or overwritten:
            _residency.reclaim()          # (this object's device copies among them: they come down first)
            for which, grid in ((_capi.GRID_XH, self.xh), (_capi.GRID_NDENS, self.ndens), (_capi.GRID_TEMP, self.temp)):
                lib.grid_to_device(which, np.asarray(grid, dtype=np.float64))
        return lib

    def power_spectrum(self, **kw):
        """The spherically averaged power spectrum of the current state, a :class:`pyc2ray_amd.powerspec.PowerSpectrum`; the keywords
        of :func:`pyc2ray_amd.powerspec.power_spectrum` but ``field`` and ``field_b``, and ``spin``.  ``kind`` is 'dtb' unless given
        (or set by ``Output: power_spectrum_kind``): the brightness temperature in mK, with ``scale`` =
        :meth:`brightness_temperature_scale` and ``box_len`` = the comoving side of the box in Mpc unless given.  ``spin``: None
        (default) for a spin temperature far above the CMB's (``t_gamma`` = 0 unless given), 'kinetic' for the spin temperature
        coupled to the object's temperature grid (``t_gamma`` = the CMB temperature at ``self.zred``).
        While the ionised fraction of the last step lives on the device only (``device_resident``) and density and temperature
        there are the host's, the grids are analysed there: nothing is downloaded.  Otherwise -- with ``use_mpi`` too -- the host
        arrays are uploaded and analysed; every rank computes the same result from its own copy."""
        for name in ("field", "field_b"):
            if name in kw:
                raise ValueError(f"C2Ray.power_spectrum: {name} is not for the class (it analyses its own grids)")
        kw = {**C2Ray.power_spectrum_stats.defaults(self), **kw}
        self._spin_t_gamma("C2Ray.power_spectrum", kw)
        kw = {"scale": self.brightness_temperature_scale(), "box_len": self.boxsize_c / Mpc, **kw}
        spec = powerspec_spec("C2Ray.power_spectrum", self.N, **kw)
        return powerspec_on_device(self._state_on_device(), spec)

    def bispectrum(self, **kw):
        """The bispectrum of the current state for triangles of k-shells, a :class:`pyc2ray_amd.bispectrum.Bispectrum`; the keywords
        of :func:`pyc2ray_amd.bispectrum.bispectrum` but ``field``, and ``spin``.  ``kind`` is 'dtb' unless given: the brightness
        temperature in mK, with ``scale`` = :meth:`brightness_temperature_scale` and ``box_len`` = the comoving side of the box in
        Mpc unless given.  ``spin``: as in :meth:`power_spectrum`.  The grids are analysed where they lie under the conditions of
        :meth:`power_spectrum`, else uploaded from the host arrays.
        There is no per-step switch and no ``Output:`` key for it: the device keeps one N^3 field per shell while it runs, and a
        driver that wants it calls ``sim.bispectrum()`` after a step."""
        if "field" in kw:
            raise ValueError("C2Ray.bispectrum: field is not for the class (it analyses its own grids)")
        kw = dict(kw)
        self._spin_t_gamma("C2Ray.bispectrum", kw)
        kw = {"scale": self.brightness_temperature_scale(), "box_len": self.boxsize_c / Mpc, **kw}
        spec = bispectrum_spec("C2Ray.bispectrum", self.N, **kw)
        return bispectrum_on_device(self._state_on_device(), spec)

    @staticmethod
    def _observed_filter_spec(who, baseline_km, los_axis):
        if isinstance(baseline_km, (bool, np.bool_)) or not isinstance(baseline_km, (int, float, np.integer, np.floating)) \
                or not (math.isfinite(baseline_km) and baseline_km > 0):
            raise ValueError(f"{who}: baseline_km must be a finite number > 0, not {baseline_km!r}")
        if isinstance(los_axis, (bool, np.bool_)) or not isinstance(los_axis, (int, np.integer)) or los_axis not in (0, 1, 2):
            raise ValueError(f"{who}: los_axis must be 0, 1 or 2, not {los_axis!r}")
        return float(baseline_km), int(los_axis)

    def _observed_keys_spec(self, kw):
        """What the declaration of ``observed_stats`` checks of the ``Output: observed_*`` keys at construction."""
        self._observed_filter_spec("Output: observed_baseline_km / observed_los_axis", kw.get("baseline_km", 2.0), kw.get("los_axis", 2))
        smoothing_spec("Output: observed_bins", None, bins=kw.get("bins"))

    def comoving_distance(self, z):
        """The line-of-sight comoving distance to redshift z in Mpc, from the object's cosmology."""
        if self._astropy:
            return float(self.cosmology.comoving_distance(z).to('Mpc').value)
        return float(self.cosmology.comoving_distance(z))

    def beam_fwhm_cells(self, baseline_km=2.0, z=None):
        """The resolution of an interferometer with maximum baseline `baseline_km` at redshift `z` (None: ``self.zred``) in cells of
        the mesh: lambda_21 (1 + z) / B radians times the comoving distance to z, over the comoving cell size (the convention of
        ``tools21cm.smooth_coeval``)."""
        z = float(self.zred) if z is None else float(z)
        theta = 0.211 * (1.0 + z) / (float(baseline_km) * 1e3)                  # lambda_21 = 21.1 cm
        return theta * self.comoving_distance(z) / (self.dr_c / Mpc)

    def smoothed_field(self, **kw):
        """The current state multiplied by a filter in Fourier space, with its one-point statistics: a
        :class:`pyc2ray_amd.smoothing.SmoothedField`; the keywords of :func:`pyc2ray_amd.smoothing.smoothed_field` but ``field``, and
        ``spin``.  ``kind`` is 'dtb' unless given: the brightness temperature in mK, with ``scale`` =
        :meth:`brightness_temperature_scale` unless given; ``spin`` as in :meth:`power_spectrum`.
        While the ionised fraction of the last step lives on the device only (``device_resident``) and density and temperature
        there are the host's, the grids are analysed there: nothing is downloaded.  Otherwise -- with ``use_mpi`` too -- the host
        arrays are uploaded and analysed.  ``into`` writes a device grid behind the object's back: the object's own device copies
        come down first, and every grid goes up again at the next step."""
        if "field" in kw:
            raise ValueError("C2Ray.smoothed_field: field is not for the class (it analyses its own grids)")
        self._spin_t_gamma("C2Ray.smoothed_field", kw)
        kw = {"scale": self.brightness_temperature_scale(), **kw}
        spec = smoothing_spec("C2Ray.smoothed_field", self.N, **kw)
        return smoothing_on_device(self._state_on_device(overwritten=spec["into"] is not None), spec, "C2Ray.smoothed_field")

    def observed_map(self, baseline_km=None, los_axis=None, subtract_mean=True, **kw):
        """The brightness temperature of the current state as an interferometer with maximum baseline `baseline_km` (default 2, or
        ``Output: observed_baseline_km``) would see it: smoothed by a Gaussian beam of FWHM :meth:`beam_fwhm_cells` on the two axes
        across the sky and by a top-hat of the same comoving width along `los_axis` (default 2, or ``Output: observed_los_axis``),
        the mean removed unless ``subtract_mean=False``: :meth:`smoothed_field` with that filter, and its other keywords."""
        if "filter" in kw:
            raise ValueError("C2Ray.observed_map: the filter is the telescope's (smoothed_field takes any)")
        d = C2Ray.observed_stats.defaults(self)
        baseline_km = d.get("baseline_km", 2.0) if baseline_km is None else baseline_km
        los_axis = d.get("los_axis", 2) if los_axis is None else los_axis
        baseline_km, los_axis = self._observed_filter_spec("C2Ray.observed_map", baseline_km, los_axis)
        if "bins" in d:
            kw = {"bins": d["bins"], **kw}
        width = self.beam_fwhm_cells(baseline_km)
        return self.smoothed_field(filter=telescope(width, width, los_axis), subtract_mean=subtract_mean, **kw)

    # ---- redshift space (pyc2ray_amd/redshift_space.py) -----------------------------------------------
    @property
    def los_axis(self):
        """The axis of the line of sight, 0, 1 or 2: what ``los_velocity`` is the velocity along.  2, or ``Output:
        redshift_space_los_axis``, until it is assigned."""
        return self.__dict__.get("_los_axis", C2Ray.redshift_space_stats.defaults(self).get("los_axis", 2))

    @los_axis.setter
    def los_axis(self, value):
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or value not in (0, 1, 2):
            raise ValueError(f"C2Ray.los_axis: los_axis must be 0, 1 or 2, not {value!r}")
        if self.lightcone_stats and self.__dict__.get("lightcone") is not None:
            raise ValueError("C2Ray.los_axis: a light cone is open along the present axis (lightcone_stats = False ends it)")
        self.__dict__["_los_axis"] = int(value)

    @property
    def los_velocity(self):
        """The proper peculiar velocity along ``los_axis`` in km/s, an (N, N, N) array, or None (default): what
        :meth:`power_spectrum_los` and :meth:`redshift_space_field` move the signal by.  An assignment is checked at once (shape,
        finite entries) and uploaded to the device once, at the next call that needs it, not per step; assign again after writing
        into the array."""
        return self.__dict__.get("_los_velocity")

    @los_velocity.setter
    def los_velocity(self, value):
        if value is not None:
            value = np.asarray(value)
            if value.shape != (self.N,) * 3 or value.dtype.kind not in "fiu":
                raise ValueError(f"C2Ray.los_velocity: the velocity must be None or a real ({self.N}, {self.N}, {self.N}) array")
            if not np.all(np.isfinite(value)):
                raise ValueError("C2Ray.los_velocity: the velocity has a non-finite entry")
        self.__dict__["_los_velocity"] = value
        self.__dict__["_los_velocity_max"] = None               # (None: not on the device)

    def velocity_scale(self):
        """What converts a proper peculiar velocity in km/s to a displacement in cells of the mesh at ``self.zred``: (1 + z) / (H(z)
        x the comoving cell size in Mpc), H(z) = 100 h E(z) km/s/Mpc from the object's cosmology."""
        z = float(self.zred)
        hubble = 100.0 * float(self._ld['Cosmology']['h']) * float(self.cosmology.efunc(z))
        return (1.0 + z) / (hubble * (self.dr_c / Mpc))

    def _redshift_space_keys_spec(self, kw):
        """What the declaration of ``redshift_space_stats`` checks of the ``Output: redshift_space_*`` keys at construction."""
        redshift_space_spec("Output: redshift_space_binning / redshift_space_bins / redshift_space_los_axis", None,
                            **self._redshift_space_bins({"binning": "multipoles", **kw}))

    @staticmethod
    def _redshift_space_bins(kw):
        """``bins`` of the class is the bins of k: with binning 'cylindrical' those of k_perp and of k_par, unless they are given."""
        if kw.get("binning", "multipoles") == "cylindrical" and "bins" in kw:
            kw = dict(kw)
            b = kw.pop("bins")
            kw = {"bins_perp": b, "bins_par": b, **kw}
        return kw

    def _redshift_space_call(self, who, kw):
        """The keywords `kw` of a redshift-space analysis of the object's state completed and checked, and the library with the
        state and the velocity on the device: (lib, spec)."""
        for name in ("field", "velocity", "max_velocity"):
            if name in kw:
                raise ValueError(f"{who}: {name} is not for the class (it analyses its own grids with its los_velocity)")
        self._spin_t_gamma(who, kw)
        kw = {"scale": self.brightness_temperature_scale(), "los_axis": self.los_axis, "velocity_scale": self.velocity_scale(), **kw}
        v = self.los_velocity
        vmax = None if v is None else (self.__dict__.get("_los_velocity_max") or float(np.max(np.abs(v))))
        spec = redshift_space_spec(who, self.N, max_velocity=vmax, **kw)
        lib = self._state_on_device(overwritten=spec["into"] is not None)
        self._los_velocity_on_device(lib)
        return lib, spec

    def _los_velocity_on_device(self, lib):
        """``los_velocity`` uploaded unless the device holds it since its assignment."""
        v = self.los_velocity
        if v is not None and self.__dict__.get("_los_velocity_max") is None:
            _residency.register(self)                           # (whoever takes the device next says so: _leave_device)
            self.__dict__["_los_velocity_max"] = lib.los_velocity_to_device(np.asarray(v, dtype=np.float64))

    def power_spectrum_los(self, **kw):
        """The power spectrum of the current state in redshift space, resolved in direction: a
        :class:`pyc2ray_amd.redshift_space.AnisotropicSpectrum`; the keywords of
        :func:`pyc2ray_amd.redshift_space.power_spectrum_los` but ``field`` and ``velocity``, and ``spin`` as in
        :meth:`power_spectrum`.  ``kind`` is 'dtb' unless given, with ``scale`` = :meth:`brightness_temperature_scale` and ``box_len``
        = the comoving side of the box in Mpc; ``binning`` is 'multipoles' unless given (or set by ``Output:
        redshift_space_binning``), ``bins`` the bins of k (with 'cylindrical': of k_perp and of k_par), ``los_axis`` =
        ``self.los_axis`` and ``velocity_scale`` = :meth:`velocity_scale`.  The signal is moved by ``los_velocity``; while that is
        None, the spectrum is the real-space one, resolved in direction all the same.  The grids are analysed where they lie, as
        in :meth:`power_spectrum`; the velocity crosses to the device once per assignment."""
        who = "C2Ray.power_spectrum_los"
        defaults = {key: v for key, v in C2Ray.redshift_space_stats.defaults(self).items() if key != "los_axis"}     # (los_axis: the property)
        kw = {"box_len": self.boxsize_c / Mpc, **self._redshift_space_bins({"binning": "multipoles", **defaults, **kw})}
        if "into" in kw:
            raise ValueError(f"{who}: into is for redshift_space_field")
        lib, spec = self._redshift_space_call(who, kw)
        return spectrum_on_device(lib, spec)

    def redshift_space_field(self, **kw):
        """The current state moved into redshift space by ``los_velocity``: the (N, N, N) cube, or with ``into`` (a grid selector)
        None, the cube being left in that device grid for ``pyc2ray_amd.mfp_distribution(grid=...)`` and the other analyses of a
        grid; the keywords of :func:`pyc2ray_amd.redshift_space.redshift_space_field` but ``field`` and ``velocity``, and ``spin``.
        ``into`` writes a device grid behind the object's back: the object's own device copies come down first, and every grid
        and the velocity go up again afterwards."""
        who = "C2Ray.redshift_space_field"
        lib, spec = self._redshift_space_call(who, dict(kw))
        return field_on_device(lib, spec)

    # ---- the Lyman-alpha forest (pyc2ray_amd/lyman_alpha.py) ------------------------------------------
    def lyman_alpha_b_scale(self):
        """The Doppler parameter of hydrogen in cells of the mesh per sqrt(K) at ``self.zred``: sqrt(2 k_B / m_p) = 0.1284... km/s
        per sqrt(K), times :meth:`velocity_scale`."""
        return math.sqrt(2.0 * K_BOLTZMANN / M_PROTON) * 1.0e-5 * self.velocity_scale()

    def lyman_alpha_tau_scale(self):
        """The Gunn-Peterson optical depth per unit proper neutral hydrogen density (cm^-3) at ``self.zred``: I_alpha / H(z), with
        I_alpha = pi e^2 f_alpha lambda_alpha / (m_e c) (f_alpha = 0.4164, lambda_alpha = 1215.67 Angstrom; cgs) and H(z) = 100 h
        E(z) km/s/Mpc from the object's cosmology."""
        z = float(self.zred)
        hubble = 100.0 * float(self._ld['Cosmology']['h']) * float(self.cosmology.efunc(z)) * 1.0e5 / Mpc           # 1/s
        return math.pi * E_CHARGE ** 2 * LYA_F_ALPHA * LYA_LAMBDA_ALPHA / (M_ELECTRON * C_LIGHT) / hubble

    def lyman_alpha_forest(self, **kw):
        """The Lyman-alpha forest of the current state along ``los_axis``: a :class:`pyc2ray_amd.lyman_alpha.LymanAlphaForest`; the
        keywords of :func:`pyc2ray_amd.lyman_alpha.lyman_alpha_forest` but the host arrays and ``velocity``.  ``los_axis`` =
        ``self.los_axis``, ``velocity_scale`` = :meth:`velocity_scale`, ``b_scale`` = :meth:`lyman_alpha_b_scale` and ``tau_scale`` =
        :meth:`lyman_alpha_tau_scale` unless given, and the ``Output: lyman_alpha_*`` keys of the parameter file for
        ``gap_threshold`` and ``bins``.  The gas is moved by ``los_velocity``; while that is None it is at rest.  The grids are
        analysed where they lie, as in :meth:`power_spectrum`; the velocity crosses to the device once per assignment.  ``into``
        writes a device grid behind the object's back: the object's own device copies come down first, and every grid and the
        velocity go up again afterwards."""
        who = "C2Ray.lyman_alpha_forest"
        for name in ("xh", "ndens", "temp", "velocity", "device_velocity"):
            if name in kw:
                raise ValueError(f"{who}: {name} is not for the class (it analyses its own grids with its los_velocity)")
        kw = {"los_axis": self.los_axis, "velocity_scale": self.velocity_scale(), "b_scale": self.lyman_alpha_b_scale(),
              "tau_scale": self.lyman_alpha_tau_scale(), **C2Ray.lyman_alpha_stats.defaults(self), **kw}
        spec = lyman_alpha_spec(who, self.N, device_velocity=self.los_velocity is not None, **kw)
        lib = self._state_on_device(overwritten=spec["into"] is not None)
        self._los_velocity_on_device(lib)
        return forest_on_device(lib, spec)

    # ---- the light cone (pyc2ray_amd/lightcone.py) ------------------------------------------------------
    def _lightcone_step(self):
        """What ``lightcone_stats`` does after a step: the slices between the previous state's redshift and this one's join
        ``self.lightcone``; a :class:`pyc2ray_amd.lightcone.LightConeStep`.  The redshift of the state a step leaves is that of
        ``self.time``: ``zred`` stays at the half step (cosmo_evolve).  The first step after switching on makes the cone -- slices a
        comoving cell apart from that state's redshift down, ``los_axis`` the object's unless ``Output: lightcone_los_axis`` sets it
        -- and keeps the field.  For 'dtb' a slice carries :meth:`brightness_temperature_scale` at its own redshift; with
        ``lightcone_spin: kinetic`` ``t_gamma`` is the CMB temperature at the state's.  The grids are used where they lie, as in
        :meth:`power_spectrum`; across ranks every rank advances its own slot and rank 0 alone keeps slices."""
        d = {"kind": "dtb", "first_plane": 0, "spin": None, "z_end": None, **C2Ray.lightcone_stats.defaults(self)}
        z_now = float(self.time2zred(self.time))
        cone = self.__dict__.get("lightcone")
        if cone is None:
            cone = LightCone(self.N, self.cosmology, z_now, self.boxsize_c / Mpc / self.N, kind=d["kind"], los_axis=d.get("los_axis", self.los_axis),
                             first_plane=d["first_plane"], z_end=d["z_end"], keep=self.rank == 0)
            self.__dict__["lightcone"] = cone
        t_gamma = float(self._ld['Cosmology']['cmbtemp']) * (1.0 + z_now) if d["spin"] == "kinetic" else 0.0
        scale = self.brightness_temperature_scale if cone.kind == "dtb" else None
        step = cone.advance(self._state_on_device(), self.__dict__.get("_lightcone_z_prev"), z_now, scale=scale, t_gamma=t_gamma)
        self.__dict__["_lightcone_z_prev"] = z_now
        return step

    # ---- sources from a halo catalogue (pyc2ray_amd/halo_sources.py) -------------------------------------
    def _halo_sources_init(self):
        """The optional ``Sources:`` keys of the halo source model: with ``fgamma_hm`` there, ``source_model`` is made from
        ``fgamma_hm``, ``fgamma_lm`` (default 0), ``ts`` (Myr), ``suppression``, ``x_suppress`` and ``f_suppressed``, checked now;
        ``m_lm`` and ``m_hm`` are the mass thresholds of :meth:`new_halo_catalogue`."""
        src = self._ld.get('Sources') or {}
        d = self.__dict__
        d["_halo_catalogue"], d["_source_model"], self.last_halo_sources = None, None, None
        self.halo_mass_thresholds = {k: src[k] for k in ("m_lm", "m_hm") if k in src}
        if "fgamma_hm" in src:
            if "ts" not in src:
                raise ValueError("Sources: fgamma_hm needs ts, the time in Myr over which the photons are released")
            extra = {k: src[k] for k in ("suppression", "x_suppress", "f_suppressed") if k in src}
            self.source_model = SourceModel(src["fgamma_hm"], src.get("fgamma_lm", 0.0), src["ts"], who="Sources", **extra)
        HaloCatalogue(np.zeros((0, 3)), np.zeros(0), **self.halo_mass_thresholds)      # ValueError for bad thresholds, now

    @property
    def halo_catalogue(self):
        """The halo catalogue the sources of a step are built from (a :class:`pyc2ray_amd.halo_sources.HaloCatalogue` or None):
        assigned by the driver at every new snapshot; it is uploaded and binned when the next list is built."""
        return self.__dict__.get("_halo_catalogue")

    @halo_catalogue.setter
    def halo_catalogue(self, value):
        if value is not None and not isinstance(value, HaloCatalogue):
            raise ValueError(f"C2Ray.halo_catalogue: halo_catalogue must be a HaloCatalogue or None, not {type(value).__name__}")
        self.__dict__["_halo_catalogue"] = value

    @property
    def source_model(self):
        """How the weights of ``halo_catalogue`` become photon rates (a :class:`pyc2ray_amd.halo_sources.SourceModel` or None)."""
        return self.__dict__.get("_source_model")

    @source_model.setter
    def source_model(self, value):
        if value is not None and not isinstance(value, SourceModel):
            raise ValueError(f"C2Ray.source_model: source_model must be a SourceModel or None, not {type(value).__name__}")
        self.__dict__["_source_model"] = value

    def new_halo_catalogue(self, positions, masses, weights=None, **kw):
        """``halo_catalogue`` <- HaloCatalogue(positions, masses, weights) with the parameter file's ``Sources: m_lm / m_hm``
        unless given; returns it."""
        self.halo_catalogue = HaloCatalogue(positions, masses, weights, **{**self.halo_mass_thresholds, **kw})
        return self.halo_catalogue

    def halo_sources(self):
        """The source list that ``halo_catalogue`` and ``source_model`` give for the current ionised fraction, a
        :class:`pyc2ray_amd.halo_sources.HaloSourceList`, with the scale of the object's cosmology and abundances.  While the
        ionised fraction of the last step lives on the device only (``device_resident``), it is read there: only the list crosses
        PCIe, and ``xh`` stays where it is.  Otherwise -- with ``use_mpi`` too -- the host array is uploaded; every rank builds the
        same list from its own copy."""
        cat, model = self.halo_catalogue, self.source_model
        if cat is None or model is None:
            raise ValueError("C2Ray.halo_sources: needs halo_catalogue (a HaloCatalogue) and source_model (a SourceModel, or the "
                             "Sources: fgamma_hm / fgamma_lm / ts keys of the parameter file)")
        if not self.gpu:
            raise ValueError("C2Ray.halo_sources: halo_sources needs use_gpu=True (the list is built on the device)")
        kw = dict(cosmology=self.cosmology, mean_molecular=self.mean_molecular)
        if self.device_resident and not self.mpi and "xh" in self._device_newer and cuda_is_init():
            return sources_on_device(load_asora(), _capi.GRID_XH, halo_spec("C2Ray.halo_sources", self.N, cat, model, **kw))
        return catalogue_sources(cat, model, xh=self.xh, **kw)

    def _step_sources(self, src_flux, src_pos):
        """The source list of a step: the caller's, or with both left out the one of :meth:`halo_sources`, which becomes
        ``last_halo_sources`` and a line of the log."""
        if src_flux is not None and src_pos is not None:
            return src_flux, src_pos
        if (src_flux is None) != (src_pos is None):
            raise ValueError("C2Ray.evolve3D: src_flux and src_pos come together or not at all")
        if self.halo_catalogue is None or self.source_model is None:
            raise ValueError("C2Ray.evolve3D: no sources: pass src_flux and src_pos, or assign halo_catalogue (a HaloCatalogue) and "
                             "source_model (a SourceModel, or the Sources: keys of the parameter file) for evolve3D(dt)")
        sources = self.halo_sources()
        self.last_halo_sources = sources
        if self.rank == 0:
            self.printlog(sources.log_line())
        return sources.src_flux, sources.src_pos

    def evolve3D(self, dt, src_flux=None, src_pos=None, src_spectrum=None):
        """Evolve the grid over one time step (c2ray_base.py:170-226).  src_spectrum: with ``BlackBodySource: Teff`` a list, the
        index into it of each source's temperature (None: every source the first one); see pyc2ray_amd.evolve3D.  With `src_flux`
        and `src_pos` left out the sources are those of :meth:`halo_sources`."""
        src_flux, src_pos = self._step_sources(src_flux, src_pos)
        if self.device_resident and self.gpu and not self.mpi:
            return self._evolve3D_resident(dt, src_flux, src_pos, src_spectrum)
        budget = {"budget": StepBudget()} if self.photon_budget else {}      # (off: the entry never hears of it)
        head = (dt, self.dr, src_flux, src_pos, self.gpu, self.max_subbox, self.subboxsize, self.loss_fraction)
        tail = (self.temp, self.ndens, self.xh, self.photo_thin_table, self.photo_thick_table, self.minlogtau, self.dlogtau,
                self.R_max_LLS, self.convergence_fraction, self.sig, self.bh00, self.albpow, self.colh0, self.temph0, self.abu_c,
                self.logfile)
        thermal = self._thermal_params()
        if self.mpi and np.size(src_flux) >= self.nprocs:
            result = evolve3D_MPI(*head, self.mpi, self.comm, self.rank, self.nprocs, *tail, thermal=thermal,
                                  clumping=self.__dict__["_clumping"], src_spectrum=src_spectrum, lls=self.lls,
                                  periodic=self.periodic, plane_flux=self.plane_flux, **budget)
        else:
            result = evolve3D(*head, *tail, thermal=thermal, clumping=self.__dict__["_clumping"], src_spectrum=src_spectrum,
                              lls=self.lls, periodic=self.periodic, plane_flux=self.plane_flux, **budget)
        self.xh, self.phi_ion = result[:2]
        if thermal is not None:
            self.temp = result[2]
        self._close_step(budget.get("budget"))

    @classmethod
    def _fingerprint(cls, arr):
        """A strided sample of a host grid (a view of its memory in storage order): what the resident path compares to notice
        in-place changes made through a reference the caller kept."""
        flat = arr.ravel(order='K')
        step = max(1, flat.shape[0] // cls._FINGERPRINT_SAMPLES)
        return flat[::step].copy()

    def _written_behind_the_attribute(self, name):
        """Has the host array of input grid `name` changed since it was last in step with the device, without the attribute having
        been touched?  (``n = sim.ndens`` ... ``n *= 2``.)  True: the caller uploads it again.  If the DEVICE copy has moved on as
        well -- a density diluted on the device -- the two cannot be reconciled (the write went into stale values): that raises."""
        prints = self.__dict__.get("_grid_fingerprints", {})
        if name not in prints or name in self._host_newer:
            return False
        if np.array_equal(self._fingerprint(self.__dict__["_grid_" + name]), prints[name]):
            return False
        if name in self._device_newer:
            raise RuntimeError(f"C2Ray.{name} was written into through a reference kept from before the last time step, while the "
                               f"device held the newer copy (cosmo_evolve dilutes a device-resident density on the device).  Read "
                               f"sim.{name} again before modifying it (`sim.{name} *= f`, `sim.{name}[...] = v` do), or set "
                               f"sim.device_resident = False for the reference's all-through-the-host behaviour.")
        return True

    def _leave_device(self):
        """Someone else is about to overwrite the device grids (pyc2ray_amd/_residency.py): fetch what exists only there, and
        upload everything again at the next step."""
        for name in ("ndens", "temp", "xh", "phi_ion"):
            if name in self._device_newer and ("_grid_" + name) in self.__dict__:
                getattr(self, name)                              # (downloads; marks the host copy as the newer one)
        self._device_newer.clear()
        self._host_newer |= {"ndens", "temp", "xh", "clumping"}
        self.__dict__.pop("_grid_fingerprints", None)
        self.__dict__["_los_velocity_max"] = None               # (the velocity goes up again too)

    def _evolve3D_resident(self, dt, src_flux, src_pos, src_spectrum=None):
        """The same step with the grids left on the device (see `device_resident`)."""
        d = self.__dict__
        _residency.reclaim(except_for=self)                     # (another object's device copies, should there be one)
        _residency.register(self)
        uploads = {}
        prints = d.setdefault("_grid_fingerprints", {})
        for name, which in (("ndens", _capi.GRID_NDENS), ("temp", _capi.GRID_TEMP), ("xh", _capi.GRID_XH)):
            host = d["_grid_" + name]
            # (an input grid the host did not touch through the attribute may still have been written into through a kept reference)
            changed = name in self._host_newer or self._written_behind_the_attribute(name)
            if changed:
                uploads[which] = host
                if name != "xh":
                    prints[name] = self._fingerprint(host)
        clumping = d["_clumping"]
        if isinstance(clumping, np.ndarray) and "clumping" in self._host_newer:
            uploads[_capi.GRID_CLUMP] = clumping                # (else GRID_CLUMP holds it from an earlier step)
        phi_host = d.get("_grid_phi_ion")                       # (a subclass may never have assigned phi_ion)
        if phi_host is None or (phi_host.flags.f_contiguous and not phi_host.flags.c_contiguous):
            d["_grid_phi_ion"] = np.zeros(self.shape)           # the GPU path returns C-ordered rates (evolve.py:200)
        budget = {"budget": StepBudget()} if self.photon_budget else {}      # (off: the entry never hears of it)
        evolve3D_resident(dt, self.dr, src_flux, src_pos, uploads, self.N, self.photo_thin_table, self.minlogtau, self.dlogtau,
                          self.R_max_LLS, self.convergence_fraction, self.sig, self.bh00, self.albpow, self.colh0, self.temph0,
                          self.abu_c, self.logfile, thermal=self._thermal_params(), clumping=clumping, src_spectrum=src_spectrum,
                          lls=self.lls, periodic=self.periodic, plane_flux=self.plane_flux, **budget)
        self._host_newer -= {"ndens", "temp", "xh", "phi_ion", "clumping"}
        self._device_newer |= {"xh", "phi_ion"} if self.isothermal else {"xh", "phi_ion", "temp"}
        self._close_step(budget.get("budget"))

    def cosmo_evolve(self, dt):
        """Advance time and redshift by dt, diluting density and rescaling the cell size when the run is
        cosmological; redshift is set at the half time step (c2ray_base.py:229-257)."""
        t_now = self.time
        t_half = t_now + 0.5 * dt
        t_after = t_now + dt
        z_half = self.time2zred(t_half)
        if self.cosmological:
            dilution_factor = ((1 + z_half) / (1 + self.zred)) ** 3
            if (self.device_resident and self.gpu and not self.mpi and cuda_is_init() and "ndens" not in self._host_newer
                    and "ndens" in self.__dict__.get("_grid_fingerprints", {}) and not self._written_behind_the_attribute("ndens")):
                # the density lives on the device and the host has not touched it since: diluted there (the same IEEE
                # multiplication per cell); the host array is fetched when someone reads sim.ndens
                load_asora().grid_scale(_capi.GRID_NDENS, dilution_factor)
                self._device_newer.add("ndens")
            else:
                self.ndens *= dilution_factor
            if not self.isothermal:
                # adiabatic cooling of the gas with the expansion, T ~ (1+z)^2
                cooling_factor = ((1 + z_half) / (1 + self.zred)) ** 2
                if (self.device_resident and self.gpu and not self.mpi and cuda_is_init() and "temp" not in self._host_newer
                        and "temp" in self.__dict__.get("_grid_fingerprints", {}) and not self._written_behind_the_attribute("temp")):
                    load_asora().grid_scale(_capi.GRID_TEMP, cooling_factor)
                    self._device_newer.add("temp")
                else:
                    self.temp *= cooling_factor
            self.dr = self.dr_c * self._scale_factor(z_half)
        self.zred = z_half
        self.time = t_after
        if self.cosmological and self.__dict__.get("lls_schedule") is not None:
            self.__dict__["_lls"] = self.lls_schedule.at(self.zred)

    def printlog(self, s, quiet=False):
        if self.logfile is None:
            raise RuntimeError("Please set the log file in output_ini")
        printlog(s, self.logfile, quiet)

    def write_output(self, z):
        pass

    # ---- utilities ------------------------------------------------------------------------------
    def time2zred(self, t):
        """Redshift at cosmic age t [s] (c2ray_base.py:281-284)."""
        if self._astropy:
            from astropy import units as u
            from astropy.cosmology import z_at_value
            return z_at_value(self.cosmology.age, t * u.s).value
        return self.cosmology.z_at_age(t)

    def zred2time(self, z, unit='s'):
        """Cosmic age at redshift z (c2ray_base.py:286-297)."""
        if self._astropy:
            return self.cosmology.age(z).to(unit).value
        t = self.cosmology.age(z)
        return {'s': t, 'yr': t / YEAR, 'Myr': t / (1e6 * YEAR), 'Gyr': t / (1e9 * YEAR)}[unit]

    def _lookback_s(self, z):
        if self._astropy:
            return self.cosmology.lookback_time(z).to('s').value
        return self.cosmology.lookback_time(z)

    def _scale_factor(self, z):
        return float(self.cosmology.scale_factor(z))

    def do_raytracing(self, src_flux, src_pos):
        """Photo-ionisation rates of the current state, chemistry untouched (c2ray_base.py:300-323)."""
        gamma = do_raytracing(self.dr, src_flux, src_pos, self.gpu, self.max_subbox, self.subboxsize,
                              self.loss_fraction, self.ndens, self.xh, self.photo_thin_table,
                              self.photo_thick_table, self.heat_thin_table, self.heat_thick_table, self.minlogtau,
                              self.dlogtau, self.R_max_LLS, self.sig, self.logfile, lls=self.lls, periodic=self.periodic,
                              plane_flux=self.plane_flux)
        self.phi_ion = gamma[0]
        if gamma[1] is not None:
            self.phi_heat = gamma[1]
        return gamma

    # ---- initialisation (c2ray_base.py:329-480) ----------------------------------------------------
    def _param_init(self):
        """Constants of the run from the parameter file (c2ray_base.py:329-352)."""
        ld = self._ld
        for key in ('eth0', 'ethe0', 'ethe1', 'bh00', 'fh0', 'xih0', 'albpow'):
            setattr(self, key, ld['CGS'][key])
        for key in ('abu_h', 'abu_he', 'abu_c'):
            setattr(self, key, ld['Abundances'][key])
        for key in ('loss_fraction', 'convergence_fraction', 'max_subbox', 'subboxsize'):
            setattr(self, key, ld['Raytracing'][key])
        self.sig = ld['Photo']['sigma_HI_at_ion_freq']
        self.mean_molecular = self.abu_h + 4.0 * self.abu_he
        # collisional ionisation parameter and ionisation energy in K (c2ray_base.py:346-347)
        self.colh0 = ld['CGS']['colh0_fact'] * self.fh0 * self.xih0 / self.eth0 ** 2
        self.temph0 = self.eth0 * ev2k

    def _cosmology_init(self):
        cs = self._ld['Cosmology']
        self.cosmology, self._astropy = _make_cosmology(100 * cs['h'], cs['Omega0'], cs['cmbtemp'], cs['Omega_B'])
        self.cosmological = cs['cosmological']
        self.zred_0 = cs['zred_0']
        self.age_0 = self.zred2time(self.zred_0)
        if self.cosmological:
            if self.rank == 0:
                self.printlog(f"Cosmology is on, scaling comoving quantities to the initial redshift, which is z0 = {self.zred_0:.3f}...")
            self.dr = self._scale_factor(self.zred_0) * self.dr_c
        else:
            if self.rank == 0:
                self.printlog("Cosmology is off.")

    def _radiation_init(self):
        ph = self._ld['Photo']
        self.minlogtau = ph['minlogtau']
        self.maxlogtau = ph['maxlogtau']
        self.NumTau = ph['NumTau']
        self.SourceType = ph['SourceType']
        self.grey = ph['grey']
        self.compute_heating_rates = ph['compute_heating_rates']
        if self.rank == 0:
            if self.grey:
                self.printlog("Warning: Using grey opacity")
            else:
                self.printlog(f"Using power-law opacity with {self.NumTau:n} table points between tau=10^({self.minlogtau:n}) and tau=10^({self.maxlogtau:n})")
        # NumTau + 1 points: tau = 0 first, then log-spaced (as in C2Ray)
        self.tau, self.dlogtau = make_tau_table(self.minlogtau, self.maxlogtau, self.NumTau)
        ion_freq_HI = ev2fr * self.eth0
        ion_freq_HeII = ev2fr * self.ethe1
        if self.SourceType == 'blackbody':
            freq_min = ion_freq_HI
            freq_max = 10 * ion_freq_HeII
            self.bb_Teff = self._ld['BlackBodySource']['Teff']
            self.cs_pl_idx_h = self._ld['BlackBodySource']['cross_section_pl_index']
            if isinstance(self.bb_Teff, (list, tuple)):
                self._radiation_init_spectra(ion_freq_HI, freq_min, freq_max)
                return
            radsource = BlackBodySource(self.bb_Teff, self.grey, ion_freq_HI, self.cs_pl_idx_h)
            if self.rank == 0:
                self.printlog(f"Using Black-Body sources with effective temperature T = {radsource.temp :.1e} K")
                self.printlog(f"Spectrum Frequency Range: {freq_min:.3e} to {freq_max:.3e} Hz")
                self.printlog("Integrating photoionization rates tables...")
            self.photo_thin_table, self.photo_thick_table = radsource.make_photo_table(self.tau, freq_min, freq_max, 1e48)
            if self.compute_heating_rates:
                self.printlog("Integrating photoheating rates tables...")
                self.heat_thin_table, self.heat_thick_table = radsource.make_heat_table(self.tau, freq_min, freq_max, 1e48)
            else:
                self.printlog("INFO: No heating rates")
                self.heat_thin_table = np.zeros(self.NumTau + 1)
                self.heat_thick_table = np.zeros(self.NumTau + 1)
        else:
            raise NameError("Unknown source type : ", self.SourceType)
        if self.gpu:
            photo_table_to_device(self.photo_thin_table, self.photo_thick_table)
            if self.rank == 0:
                self.printlog("Successfully copied radiation tables to GPU memory.")

    def _radiation_init_spectra(self, ion_freq_HI, freq_min, freq_max):
        """``BlackBodySource: Teff`` is a list: one table set per temperature from the builder of the scalar form, heating tables
        included with compute_heating_rates, uploaded together (spectra_to_device).  ``spectra_*_table`` are (K, NumTau + 1); the
        plain ``photo_*_table`` / ``heat_*_table`` attributes are those of the first temperature.  Which set a source takes:
        ``evolve3D(dt, src_flux, src_pos, src_spectrum)``."""
        teffs = [float(t) for t in self.bb_Teff]
        if not 1 <= len(teffs) <= _capi.MAX_SPECTRA:
            raise ValueError(f"BlackBodySource: Teff lists {len(teffs)} temperatures; 1 to {_capi.MAX_SPECTRA} are possible")
        if self.rank == 0:
            self.printlog("Using Black-Body sources with effective temperatures T = " + ", ".join(f"{t:.1e}" for t in teffs) + " K")
            self.printlog(f"Spectrum Frequency Range: {freq_min:.3e} to {freq_max:.3e} Hz")
            self.printlog("Integrating photoionization rates tables...")
        sources = [BlackBodySource(t, self.grey, ion_freq_HI, self.cs_pl_idx_h) for t in teffs]
        photo = [s.make_photo_table(self.tau, freq_min, freq_max, 1e48) for s in sources]
        self.spectra_photo_thin_table = np.stack([t[0] for t in photo])
        self.spectra_photo_thick_table = np.stack([t[1] for t in photo])
        if self.compute_heating_rates:
            self.printlog("Integrating photoheating rates tables...")
            heat = [s.make_heat_table(self.tau, freq_min, freq_max, 1e48) for s in sources]
            self.spectra_heat_thin_table = np.stack([t[0] for t in heat])
            self.spectra_heat_thick_table = np.stack([t[1] for t in heat])
        else:
            self.printlog("INFO: No heating rates")
            self.spectra_heat_thin_table = self.spectra_heat_thick_table = None
        self.photo_thin_table, self.photo_thick_table = self.spectra_photo_thin_table[0], self.spectra_photo_thick_table[0]
        if self.compute_heating_rates:
            self.heat_thin_table, self.heat_thick_table = self.spectra_heat_thin_table[0], self.spectra_heat_thick_table[0]
        else:
            self.heat_thin_table = np.zeros(self.NumTau + 1)
            self.heat_thick_table = np.zeros(self.NumTau + 1)
        if self.gpu:
            spectra_to_device(self.spectra_photo_thin_table, self.spectra_photo_thick_table, self.spectra_heat_thin_table,
                              self.spectra_heat_thick_table)
            if self.rank == 0:
                self.printlog(f"Successfully copied {len(teffs):n} sets of radiation tables to GPU memory.")

    def _grid_init(self):
        self.boxsize_c = self._ld['Grid']['boxsize'] * Mpc
        self.dr_c = self.boxsize_c / self.N
        if self.rank == 0:
            self.printlog(f"Welcome! Mesh size is N = {self.N:n}.")
            self.printlog(f"Simulation Box size (comoving Mpc): {self.boxsize_c/Mpc:.3e}")
        self.dr = self.dr_c
        # R_max (LLS type 3) in cell units
        self.R_max_LLS = self._ld['Photo']['R_max_cMpc'] * self.N / self._ld['Grid']['boxsize']
        self.printlog(f"Maximum comoving distance for photons from source (type 3 LLS): {self._ld['Photo']['R_max_cMpc'] : .3e} comoving Mpc")
        self.printlog(f"This corresponds to                                             {self.R_max_LLS : .3f} grid cells.")

    # overridden by the concrete simulation classes
    def _output_init(self):
        pass

    def _redshift_init(self):
        pass

    def _material_init(self):
        pass

    def _sources_init(self):
        pass

    def _read_paramfile(self, paramfile):
        """YAML reader that also takes 1e4-style numbers as floats (c2ray_base.py:490-507)."""
        class _Loader(SafeLoader):
            pass
        _Loader.add_implicit_resolver(
            u'tag:yaml.org,2002:float',
            re.compile(u'''^(?:
            [-+]?(?:[0-9][0-9_]*)\\.[0-9_]*(?:[eE][-+]?[0-9]+)?
            |[-+]?(?:[0-9][0-9_]*)(?:[eE][-+]?[0-9]+)
            |\\.[0-9_]+(?:[eE][-+][0-9]+)?
            |[-+]?[0-9][0-9_]*(?::[0-5]?[0-9])+\\.[0-9_]*
            |[-+]?\\.(?:inf|Inf|INF)
            |\\.(?:nan|NaN|NAN))$''', re.X),
            list(u'-+0123456789.'))
        with open(paramfile, 'r') as f:
            self._ld = yaml.load(f, _Loader)

    def _gpu_close(self):
        if cuda_is_init():
            device_close()
