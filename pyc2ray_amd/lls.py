"""Lyman-limit-system (LLS) opacity: unresolved absorbers as a distributed photon sink of the raytrace.

The raytrace's absorber density becomes ``n_abs = ndens * ((1 - xh_av) + per_density) + n_const`` where it was
``ndens * (1 - xh_av)``: column densities accumulate the added opacity, and hydrogen receives the share n_HI / n_abs of the photons
a cell absorbs.  The chemistry keeps ``ndens`` and the rates per atom.  ``evolve3D``, ``evolve3D_MPI``, ``evolve3D_resident`` and
``do_raytracing`` take an :class:`LLSOpacity` as ``lls=``.
"""
import contextlib
import math

from .utils import printlog

__all__ = ['LLSOpacity', 'LLSSchedule']

#: cm per Mpc, the value the simulation class converts box sizes with
MPC_CM = 3.086e24


def _checked(name, value):
    if isinstance(value, bool) or not isinstance(value, (int, float)) and not hasattr(value, "__float__"):
        raise ValueError(f"LLSOpacity: {name} must be a finite number >= 0, not {type(value).__name__}")
    v = float(value)
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError(f"LLSOpacity: {name} must be finite and >= 0, not {v!r}")
    return v


class LLSOpacity:
    """``n_const``: a uniform absorber density in cm^-3 (the reference's "type 1" LLS); ``per_density``: absorbers per atom of the
    local density (the linear "type 2").  Both >= 0 and finite, else ValueError; both 0 is off."""

    def __init__(self, n_const=0.0, per_density=0.0):
        self.n_const = _checked("n_const", n_const)
        self.per_density = _checked("per_density", per_density)

    @classmethod
    def from_mean_free_path(cls, mfp_cm, sig, per_density=0.0):
        """The uniform absorber density of a proper mean free path ``mfp_cm`` [cm] at the cross-section ``sig`` [cm^2]:
        n_const = 1 / (sig * mfp_cm)."""
        for name, v in (("mfp_cm", mfp_cm), ("sig", sig)):
            if isinstance(v, bool) or not (math.isfinite(float(v)) and float(v) > 0.0):
                raise ValueError(f"LLSOpacity.from_mean_free_path: {name} must be finite and > 0, not {v!r}")
        return cls(1.0 / (float(sig) * float(mfp_cm)), per_density)

    @property
    def on(self):
        return self.n_const != 0.0 or self.per_density != 0.0

    def __eq__(self, other):
        return isinstance(other, LLSOpacity) and (self.n_const, self.per_density) == (other.n_const, other.per_density)

    def __hash__(self):
        return hash((self.n_const, self.per_density))

    def __repr__(self):
        return f"LLSOpacity(n_const={self.n_const!r}, per_density={self.per_density!r})"

    def apply(self, libasora):
        libasora.lls_opacity(self.n_const, self.per_density)

    def log(self, logfile, quiet):
        printlog(f"LLS opacity: n_const {self.n_const:.3e} cm^-3, per_density {self.per_density:.3e}", logfile, quiet)


class LLSSchedule:
    """The LLS opacity of a run as a function of redshift, from the optional ``Photo`` keys of a parameter file:

    * ``LLS_mfp_pMpc``    proper mean free path at ``LLS_mfp_zref``, in Mpc (absent: no uniform absorbers)
    * ``LLS_mfp_zref``    its reference redshift (default: `z_start`, the run's starting redshift)
    * ``LLS_mfp_index``   beta of lambda(z) = lambda_ref ((1 + z) / (1 + z_ref))^(-beta) (default 0: the same at every redshift)
    * ``LLS_per_density`` absorbers per atom of the local density (default 0)

    :meth:`from_photo_keys` returns None when none of the keys is present."""

    KEYS = ("LLS_mfp_pMpc", "LLS_mfp_zref", "LLS_mfp_index", "LLS_per_density")

    def __init__(self, sig, mfp_pMpc=None, zref=0.0, index=0.0, per_density=0.0):
        def number(name, v, positive=False):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or (positive and not v > 0):
                raise ValueError(f"Photo: {name} must be a finite number{' > 0' if positive else ''}, not {v!r}")
            return float(v)
        self.sig = number("sigma_HI_at_ion_freq", sig, True)
        self.mfp_pMpc = None if mfp_pMpc is None else number("LLS_mfp_pMpc", mfp_pMpc, True)
        self.zref = number("LLS_mfp_zref", zref)
        if not self.zref > -1.0:
            raise ValueError(f"Photo: LLS_mfp_zref must be > -1, not {zref!r}")
        self.index = number("LLS_mfp_index", index)
        self.per_density = _checked("LLS_per_density", number("LLS_per_density", per_density))

    @classmethod
    def from_photo_keys(cls, photo, sig, z_start):
        if not any(k in photo for k in cls.KEYS):
            return None
        return cls(sig, photo.get("LLS_mfp_pMpc"), photo.get("LLS_mfp_zref", z_start), photo.get("LLS_mfp_index", 0.0),
                   photo.get("LLS_per_density", 0.0))

    def mfp_cm(self, z):
        """Proper mean free path at redshift z in cm (None without ``LLS_mfp_pMpc``)."""
        if self.mfp_pMpc is None:
            return None
        return self.mfp_pMpc * MPC_CM * ((1.0 + z) / (1.0 + self.zref)) ** (-self.index)

    def at(self, z):
        """The :class:`LLSOpacity` at redshift z."""
        mfp = self.mfp_cm(z)
        if mfp is None:
            return LLSOpacity(0.0, self.per_density)
        return LLSOpacity.from_mean_free_path(mfp, self.sig, self.per_density)


def lls_spec(lls, who):
    """``lls=`` of an entry point -> None (off: None, or both values 0) or the :class:`LLSOpacity`.  Raises ValueError, before any
    GPU work, for anything else (the class itself refuses negative and non-finite values)."""
    if lls is None:
        return None
    if not isinstance(lls, LLSOpacity):
        raise ValueError(f"{who}: lls must be None or a pyc2ray_amd.lls.LLSOpacity, not {type(lls).__name__}")
    lls = LLSOpacity(lls.n_const, lls.per_density)              # (attributes assigned after construction are checked as well)
    return lls if lls.on else None


@contextlib.contextmanager
def lls_reset(lls, load):
    """Leave the library without LLS opacity after the block, whatever happens (nothing at all when it is off); `load` returns the
    library."""
    try:
        yield
    finally:
        if lls is not None:
            load().lls_opacity(0.0, 0.0)
