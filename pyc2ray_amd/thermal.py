"""Non-isothermal chemistry: the parameters of the thermal mode ("Thermal mode").

With a :class:`ThermalParams` handed to ``evolve3D(..., thermal=...)`` the temperature of every cell is integrated over the
time step from photo-heating and radiative cooling, inside the inner iteration of the chemistry where the reference keeps
the placeholders (src/c2ray/chemistry.f90:164,171-176,182-189).  The hot path is the thermal form of the fused chemistry
pass (pyc2ray_amd/csrc/chemistry.hip) and the heating form of the raytrace.  ``evolve3D_MPI(..., thermal=...)`` runs it across
ranks on the two device loops of a ``pyc2ray_amd.dist.TorchComm``, the heating rates exchanged with the photo-ionisation rates.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

__all__ = ['ThermalParams', 'COOL_RECOMBINATION', 'COOL_COLLISIONAL_IONISATION', 'COOL_COLLISIONAL_EXCITATION',
           'COOL_BREMSSTRAHLUNG', 'COOL_COMPTON', 'COOL_ALL', 'COMPTON_C', 'K_B']

#: cooling channels, bits of ``ThermalParams.cooling`` (include/asora_hip.h, asora_thermal_params)
COOL_RECOMBINATION = 1               # case-B recombination, Hui & Gnedin (1997)
COOL_COLLISIONAL_IONISATION = 2      # doric's collisional ionisation rate x the ionisation energy
COOL_COLLISIONAL_EXCITATION = 4      # Cen (1992)
COOL_BREMSSTRAHLUNG = 8              # Cen (1992)
COOL_COMPTON = 16                    # Compton exchange with the CMB (only with a redshift)
COOL_ALL = 31

#: Boltzmann constant (erg/K), the rounded value of radiation/blackbody.py
K_B = 1.381e-16

# Compton coupling 4 sigma_T a_rad k_B / (m_e c), CODATA 2018 in cgs -- the expression chemistry.hip evaluates
_SIGMA_T, _SIGMA_SB, _C, _KB, _ME = 6.6524587321e-25, 5.670374419e-5, 2.99792458e10, 1.380649e-16, 9.1093837015e-28
_A_RAD = 4.0 * _SIGMA_SB / _C
COMPTON_C = 4.0 * _SIGMA_T * _A_RAD * _KB / (_ME * _C)


@dataclass
class ThermalParams:
    """What the thermal mode needs besides the isothermal arguments of evolve3D.

    heat_thin_table, heat_thick_table : photo-heating tables on the tau grid of the photo tables
                                        (radiation.BlackBodySource.make_heat_table)
    relative_denergy : largest relative change of the thermal energy per substep
    t_floor          : lower bound of the temperature (K)
    max_substeps     : substeps per integration; the last one takes the remainder of the step (counted, and logged)
    cooling          : bit mask of the COOL_* channels
    zred             : redshift for Compton exchange with the CMB (None: no Compton)
    tcmb0            : CMB temperature today (K)
    """
    heat_thin_table: np.ndarray
    heat_thick_table: np.ndarray
    relative_denergy: float = 0.1
    t_floor: float = 1.0
    max_substeps: int = 10000
    cooling: int = COOL_ALL
    zred: Optional[float] = None
    tcmb0: float = 2.7255

    @property
    def t_cmb(self):
        """CMB temperature at zred (0 without a redshift)."""
        return 0.0 if self.zred is None else float(self.tcmb0) * (1.0 + float(self.zred))

    def apply(self, libasora):
        """Upload the heating tables and switch the library to the thermal form (photo tables must be on the device).  With
        several table sets on the device (spectra_to_device) the heating tables of every set went up with them and stay as they
        are: heat_thin_table / heat_thick_table are not used then."""
        if getattr(libasora, "num_spectra", lambda: 1)() <= 1:
            thin = np.ascontiguousarray(self.heat_thin_table, dtype=np.float64)
            thick = np.ascontiguousarray(self.heat_thick_table, dtype=np.float64)
            libasora.heat_table_to_device(thin, thick, thin.shape[0])
        libasora.thermal_params(True, self.relative_denergy, self.t_floor, self.max_substeps, int(self.cooling),
                                self.zred is not None, self.t_cmb)
