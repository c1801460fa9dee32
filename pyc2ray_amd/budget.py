"""Photon budget and mean ionised fractions of a time step.

C2-Ray closes every time step with its photon statistics: the photons emitted, the photons that ionised, those that
recombinations took back, and the volume- and mass-weighted ionised fraction.  A :class:`StepBudget` passed as ``budget=`` to
``evolve3D``, ``evolve3D_MPI`` or ``evolve3D_resident`` is filled in place with them: twelve sums over the grid, reduced on the
device after the step's loop has ended (``libasora.step_budget``), so no grid crosses PCIe for it.  The return values of the
entry points keep their shapes.
"""
import numpy as np

from . import _capi

__all__ = ['StepBudget', 'SLOTS']

#: names of the twelve sums, in the order of the C-ABI (include/asora_hip.h, ASORA_BUDGET_*)
SLOTS = ("CELLS", "N", "X", "NX", "NX0", "DNX", "PHOTO", "LLS", "REC", "COL", "T", "NT")

#: the extensive quantities, in particles per step; they add up over steps
_COUNTS = ("emitted", "new_ions", "photoionisations", "lls_absorbed", "recombinations", "collisional")
#: the means of the grid; of a sum of steps: those of its last step (``mean_xh_mass_before``: of its first)
_MEANS = ("mean_xh_volume", "mean_xh_mass", "mean_xh_mass_before", "mean_temp", "mean_temp_mass")


class StepBudget:
    """The budget of one time step, or -- as a sum of them, ``a + b`` -- of several.

    ``sums``: the twelve raw sums of :data:`SLOTS` (of a sum of steps: its last step's); ``dt`` [s] (added up), ``dr`` [cm], ``N``;
    ``steps``: how many steps it holds (0: not filled yet; such a budget is the neutral element of ``+``).

    In particles per step, with V = dr^3: ``emitted`` = (sum of src_flux + sum over the faces of flux (N dr)^2) 1e48 dt;
    ``new_ions`` = DNX V; ``photoionisations`` = PHOTO V dt; ``lls_absorbed`` = LLS V dt; ``recombinations`` = REC V dt;
    ``collisional`` = COL V dt; ``absorbed`` = photoionisations + lls_absorbed; ``escaped`` = emitted - absorbed;
    ``residual`` = new_ions - (photoionisations + collisional - recombinations).

    Means: ``mean_xh_volume`` = X / CELLS, ``mean_xh_mass`` = NX / N, ``mean_xh_mass_before`` = NX0 / N, ``mean_temp`` = T / CELLS,
    ``mean_temp_mass`` = NT / N.

    What the residual can and cannot close is derived in DESIGN.md section 4.2c: it is bounded by the inner iteration's exit
    test (1e-3 of the recombinations and collisional ionisations of the neutral gas) on isothermal steps, and reported only on
    thermal ones, whose rates are evaluated at the mean of the step's first and last temperature."""

    def __init__(self):
        self.sums = np.zeros(_capi.BUDGET_COUNT)
        self.dt = self.dr = 0.0
        self.N = self.steps = 0
        for name in _COUNTS + _MEANS:
            setattr(self, name, 0.0)

    def fill(self, sums, dt, dr, N, src_flux=(), faces=()):
        """The budget of ONE step from its twelve sums; `src_flux` in 1e48 photons/s, `faces` the step's PlaneFlux objects."""
        s = np.array(sums, dtype=np.float64).reshape(_capi.BUDGET_COUNT)
        self.sums, self.dt, self.dr, self.N, self.steps = s, float(dt), float(dr), int(N), 1
        V = self.dr ** 3
        area = (self.N * self.dr) ** 2
        self.emitted = (float(np.sum(src_flux)) + sum(f.flux * area for f in faces)) * 1e48 * self.dt
        self.new_ions = s[_capi.BUDGET_DNX] * V
        self.photoionisations = s[_capi.BUDGET_PHOTO] * V * self.dt
        self.lls_absorbed = s[_capi.BUDGET_LLS] * V * self.dt
        self.recombinations = s[_capi.BUDGET_REC] * V * self.dt
        self.collisional = s[_capi.BUDGET_COL] * V * self.dt
        cells, n = s[_capi.BUDGET_CELLS], s[_capi.BUDGET_N]
        self.mean_xh_volume = s[_capi.BUDGET_X] / cells if cells else 0.0
        self.mean_temp = s[_capi.BUDGET_T] / cells if cells else 0.0
        self.mean_xh_mass = s[_capi.BUDGET_NX] / n if n else 0.0
        self.mean_xh_mass_before = s[_capi.BUDGET_NX0] / n if n else 0.0
        self.mean_temp_mass = s[_capi.BUDGET_NT] / n if n else 0.0
        return self

    @property
    def absorbed(self):
        return self.photoionisations + self.lls_absorbed

    @property
    def escaped(self):
        return self.emitted - self.absorbed

    @property
    def residual(self):
        return self.new_ions - (self.photoionisations + self.collisional - self.recombinations)

    def copy(self):
        out = StepBudget()
        out.__dict__.update(self.__dict__)
        out.sums = self.sums.copy()
        return out

    def __add__(self, other):
        """Cumulative totals: the particle counts, dt and `steps` add up; the means, `sums`, dr and N are those of `other`, the
        later step, and ``mean_xh_mass_before`` that of `self`, the earlier one."""
        if not isinstance(other, StepBudget):
            return NotImplemented
        if self.steps == 0:
            return other.copy()
        out = other.copy()
        if other.steps == 0:
            return self.copy()
        for name in _COUNTS:
            setattr(out, name, getattr(self, name) + getattr(other, name))
        out.dt, out.steps = self.dt + other.dt, self.steps + other.steps
        out.mean_xh_mass_before = self.mean_xh_mass_before
        return out

    def log_line(self):
        """The line of the log file (one per step)."""
        return (f"Photon budget: emitted {self.emitted:.4e}, absorbed {self.absorbed:.4e} (LLS {self.lls_absorbed:.3e}), "
                f"escaped {self.escaped:.4e}; new ions {self.new_ions:.4e}, recombinations {self.recombinations:.4e}, "
                f"collisional {self.collisional:.3e}, residual {self.residual:.2e}; "
                f"<x>_vol {self.mean_xh_volume:.6e}, <x>_mass {self.mean_xh_mass:.6e}")

    def __repr__(self):
        return f"<StepBudget of {self.steps} step(s): {self.log_line()}>"


def budget_spec(budget, who, use_gpu=True):
    """``budget=`` of an entry point: None or a :class:`StepBudget`.  Raises ValueError -- before any GPU work -- for anything
    else, and for a budget with ``use_gpu=False`` (the sub-box loop has none)."""
    if budget is None:
        return None
    if not isinstance(budget, StepBudget):
        raise ValueError(f"{who}: budget must be None or a pyc2ray_amd.budget.StepBudget, not {type(budget).__name__}")
    if not use_gpu:
        raise ValueError(f"{who}: budget needs use_gpu=True (the use_gpu=False loop takes no photon budget)")
    return budget
