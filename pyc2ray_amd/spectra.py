"""Per-source spectra: the ``src_spectrum=`` argument of evolve3D / evolve3D_MPI / evolve3D_resident / do_raytracing
(DESIGN.md section 4.1a).  The device holds K table sets (``spectra_to_device``); source s is rated with set src_spectrum[s]."""
import numpy as np

__all__ = ['source_spectrum_spec']


def source_spectrum_spec(src_spectrum, numsrc, use_gpu, num_spectra, who="evolve3D"):
    """``src_spectrum=`` -> None (every source spectrum 0: None or all zeros, today's path with no extra upload) or an int32
    array of length numsrc.  Raises ValueError -- before any GPU work -- for anything but an integer array of length numsrc
    with values in [0, num_spectra()), and for a non-zero entry with use_gpu=False (the sub-box raytracer rates every source with the
    flux of the last one: it has no spectrum per source).  `num_spectra`: a callable, asked only when an entry is non-zero."""
    if src_spectrum is None:
        return None
    s = np.asarray(src_spectrum)
    if s.ndim != 1 or s.shape[0] != numsrc:
        raise ValueError(f"{who}: src_spectrum must have one entry per source, shape ({numsrc},), not {s.shape}")
    if s.dtype.kind not in "iu":
        raise ValueError(f"{who}: src_spectrum must be an integer array, not {s.dtype}")
    if numsrc and s.min() < 0:
        raise ValueError(f"{who}: src_spectrum holds a negative index ({int(s.min())})")
    if not numsrc or s.max() == 0:
        return None
    if not use_gpu:
        raise ValueError(f"{who}: sources with spectra of their own need use_gpu=True (the use_gpu=False raytracer rates every "
                         "source with the flux of the last one and has one spectrum)")
    K = int(num_spectra())
    if s.max() >= K:
        raise ValueError(f"{who}: src_spectrum holds index {int(s.max())}, but the device holds {K} table set(s) (spectra_to_device)")
    return np.ascontiguousarray(s, dtype=np.int32)
