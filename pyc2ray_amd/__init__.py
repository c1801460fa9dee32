"""pyc2ray_amd -- MI355X-native implementation of pyc2ray's raytracing + chemistry hot path.

The public names are those of the reference package for this path (pyc2ray/__init__.py:1-9):
evolve3D, do_raytracing, cuda_is_init / device_init / device_close / photo_table_to_device,
hydrogenODE, printlog, format_sources, ...  All arithmetic runs in hand-written HIP kernels
(pyc2ray_amd/csrc) behind the C-ABI of include/asora_hip.h; there is no CPU compute path.
"""
from .evolve import *          # noqa: F401,F403  evolve3D, evolve3D_MPI
from .asora_core import *      # noqa: F401,F403
from .raytracing import *      # noqa: F401,F403
from .chemistry import *       # noqa: F401,F403
from .utils import *           # noqa: F401,F403
from .radiation import *       # noqa: F401,F403
from .bubbles import *         # noqa: F401,F403  BubbleSizes, mfp_distribution
from .regions import *         # noqa: F401,F403  RegionSizes, region_sizes
from .powerspec import *       # noqa: F401,F403  PowerSpectrum, power_spectrum
from .smoothing import *       # noqa: F401,F403  SmoothedField, smoothed_field, Filter and the filter builders
from .redshift_space import *  # noqa: F401,F403  AnisotropicSpectrum, power_spectrum_los, redshift_space_field
from .lyman_alpha import *     # noqa: F401,F403  LymanAlphaForest, lyman_alpha_forest
from .lightcone import *       # noqa: F401,F403  LightCone, LightConeStep, make_lightcone, slice_redshifts
from .c2ray_base import *      # noqa: F401,F403
from .c2ray_test import *      # noqa: F401,F403
from . import evolve, raytracing, chemistry, asora_core, utils, dist, bubbles, regions, powerspec, smoothing, redshift_space   # noqa: F401
from . import lyman_alpha, lightcone      # noqa: F401
# (last, so that the package's `topology`, `granulometry`, `bispectrum` and `halo_sources` are the functions, not the modules of
# those names: importlib.import_module finds the modules)
from .topology import *        # noqa: F401,F403,E402  Topology, topology
from .granulometry import *    # noqa: F401,F403,E402  Granulometry, granulometry
from .bispectrum import *      # noqa: F401,F403,E402  Bispectrum, bispectrum
from .halo_sources import *    # noqa: F401,F403,E402  HaloCatalogue, SourceModel, HaloSourceList, halo_sources, source_scale
