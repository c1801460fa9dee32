"""Extension loader with the reference's names (pyc2ray/load_extensions.py:9-48).

The reference imports two CPython extension modules, ``pyc2ray.lib.libasora`` (CUDA) and
``pyc2ray.lib.libc2ray`` (f2py Fortran).  Here both are thin objects over ONE ctypes-loaded
shared library, ``pyc2ray_amd/lib/libasora_hip.so``; their methods keep the reference's names,
argument order and in-place conventions, so code written against the reference's extension
modules (pyc2ray/evolve.py:147-210, raytracing_benchmark/run_test.py:66-85) runs unchanged.

Differences, all deliberate:
  * a missing library raises RuntimeError for BOTH loaders (the reference makes ASORA optional and
    prints an "Info" line, load_extensions.py:41-44).  This build has no CPU path to fall back to:
    ``libc2ray.raytracing.do_all_sources`` and ``libc2ray.chemistry.global_pass`` keep the semantics of
    the reference's CPU functions but run on the GPU.
  * errors inside the library come back as RuntimeError carrying the library's message instead of
    an uncaught C++ exception.
  * array arguments are validated (dtype float64 / int32, contiguity, size) instead of being
    trusted (src/asora/python_module.cu:60-63).
"""
import ctypes as C

import numpy as np

from . import _capi, _pinned

__all__ = ["load_c2ray", "load_asora"]


def _flat_f64(a, n, name):
    if not isinstance(a, np.ndarray) or a.dtype != np.float64:
        raise TypeError(f"{name} must be Array of type double")       # python_module.cu:55
    if not (a.flags.c_contiguous or a.flags.f_contiguous):
        raise ValueError(f"{name} must be contiguous")
    if a.size != n:
        raise ValueError(f"{name} has {a.size} elements, expected {n}")
    return a


class _LibAsora:
    """Stand-in for the reference's ``libasora`` module (src/asora/python_module.cu:153-161)."""

    def __init__(self, lib):
        self._lib = lib
        self._N = None

    # ---- the six reference methods --------------------------------------------------------
    def device_init(self, N, num_src_par, device_id=None):
        # PYC2RAY_AMD_OPTIONS="13=2,14=2": library options (asora_set_option; the numbers are those of include/asora_hip.h) applied
        # around every device_init -- before it for the ones device_init itself reads (17: placement candidates), after it as
        # well.  For running an existing script or the test suite with a non-default variant.
        import os

        def apply_env_options():
            for item in filter(None, os.environ.get("PYC2RAY_AMD_OPTIONS", "").split(",")):
                opt, _, val = item.partition("=")
                self.set_option(int(opt), int(val))

        apply_env_options()
        if device_id is None:
            _capi.check(self._lib.asora_device_init(int(N), int(num_src_par)), "device_init")
        else:
            _capi.check(self._lib.asora_device_init_ex(int(N), int(num_src_par), int(device_id)), "device_init")
        self._N = int(N)
        apply_env_options()

    def device_close(self):
        _capi.check(self._lib.asora_device_close(), "device_close")
        self._N = None

    def density_to_device(self, ndens, N):
        a = _flat_f64(ndens, int(N) ** 3, "ndens")
        _capi.check(self._lib.asora_density_to_device(_capi.dptr(a), int(N)), "density_to_device")

    def photo_table_to_device(self, thin_table, thick_table, NumTau):
        t0 = np.ascontiguousarray(thin_table, dtype=np.float64)
        t1 = np.ascontiguousarray(thick_table, dtype=np.float64)
        if t0.size < NumTau or t1.size < NumTau:
            raise ValueError("photo_table_to_device: NumTau exceeds the table length")
        _capi.check(self._lib.asora_photo_table_to_device(_capi.dptr(t0), _capi.dptr(t1), int(NumTau)),
                    "photo_table_to_device")

    def heat_table_to_device(self, heat_thin_table, heat_thick_table, NumTau):
        """Extension: photo-heating tables (the reference's GPU library has none)."""
        t0 = np.ascontiguousarray(heat_thin_table, dtype=np.float64)
        t1 = np.ascontiguousarray(heat_thick_table, dtype=np.float64)
        _capi.check(self._lib.asora_heat_table_to_device(_capi.dptr(t0), _capi.dptr(t1), int(NumTau)),
                    "heat_table_to_device")

    def source_data_to_device(self, pos, flux, NumSrc):
        p = np.ascontiguousarray(pos)
        if p.dtype != np.int32:
            raise TypeError("source positions must be int32 (use format_sources)")
        f = np.ascontiguousarray(flux, dtype=np.float64)
        if p.size < 3 * NumSrc or f.size < NumSrc:
            raise ValueError("source_data_to_device: arrays shorter than NumSrc")
        _capi.check(self._lib.asora_source_data_to_device(_capi.iptr(p), _capi.dptr(f), int(NumSrc)),
                    "source_data_to_device")

    # ---- per-source spectra (extension; include/asora_hip.h) -------------------------------------
    def spectra_to_device(self, photo_thin, photo_thick, heat_thin=None, heat_thick=None):
        """K table sets at once: (K, NumTau) float64 arrays, set k for the sources of spectrum k
        (:meth:`source_spectra_to_device`).  The heating tables come both or not at all."""
        t = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (photo_thin, photo_thick, heat_thin, heat_thick)]
        if t[0] is None or t[1] is None or t[0].ndim != 2:
            raise ValueError("spectra_to_device: the photo tables must be 2-D, (K, NumTau)")
        K, NumTau = t[0].shape
        if not 1 <= K <= _capi.MAX_SPECTRA or NumTau < 1:
            raise ValueError(f"spectra_to_device: {K} spectra of {NumTau} entries; 1 to {_capi.MAX_SPECTRA} spectra of >= 1 entries")
        if (t[2] is None) != (t[3] is None):
            raise ValueError("spectra_to_device: one heating table without the other")
        for a, name in zip(t, ("photo_thin", "photo_thick", "heat_thin", "heat_thick")):
            if a is not None and a.shape != (K, NumTau):
                raise ValueError(f"spectra_to_device: {name} has shape {a.shape}, expected {(K, NumTau)}")
        _capi.check(self._lib.asora_spectra_to_device(K, NumTau, _capi.dptr(t[0]), _capi.dptr(t[1]),
                                                      None if t[2] is None else _capi.dptr(t[2]),
                                                      None if t[3] is None else _capi.dptr(t[3])), "spectra_to_device")

    def source_spectra_to_device(self, spec):
        """The table set of each source of the last source_data_to_device (which resets them all to 0); None: all 0."""
        if spec is None:
            _capi.check(self._lib.asora_source_spectra_to_device(None, 0), "source_spectra_to_device")
            return
        s = np.asarray(spec)
        if s.ndim != 1 or s.dtype.kind not in "iu":
            raise ValueError("source_spectra_to_device: a 1-D integer array, one table set per source")
        s = np.ascontiguousarray(s, dtype=np.int32)
        _capi.check(self._lib.asora_source_spectra_to_device(_capi.iptr(s), int(s.size)), "source_spectra_to_device")

    def num_spectra(self):
        """Table sets on the device (0: none uploaded)."""
        return int(self._lib.asora_num_spectra())

    def sort_sources(self, pos, flux, spec=None):
        """The position-ordered copy of a source list as source_data_to_device forms it (host only, no device needed):
        (pos, flux, spec) reordered, `pos` flat int32 xyz-interleaved as format_sources makes it."""
        p = np.ascontiguousarray(pos, dtype=np.int32).ravel()
        f = np.ascontiguousarray(flux, dtype=np.float64)
        n = int(f.size)
        if p.size != 3 * n:
            raise ValueError("sort_sources: 3 coordinates per source")
        s = None if spec is None else np.ascontiguousarray(spec, dtype=np.int32)
        if s is not None and s.size != n:
            raise ValueError("sort_sources: one table set per source")
        po, fo = np.empty_like(p), np.empty_like(f)
        so = None if s is None else np.empty_like(s)
        _capi.check(self._lib.asora_debug_sort_sources(_capi.iptr(p), _capi.dptr(f), None if s is None else _capi.iptr(s), n,
                                                       _capi.iptr(po), _capi.dptr(fo), None if so is None else _capi.iptr(so)),
                    "sort_sources")
        return po, fo, so

    def do_all_sources(self, R, coldensh_out, sig, dr, ndens, xh_av, phi_ion, NumSrc, m1,
                       minlogtau, dlogtau, NumTau):
        n = int(m1) ** 3
        if not isinstance(coldensh_out, np.ndarray) or coldensh_out.dtype != np.float64:
            raise TypeError("coldensh_out must be Array of type double")   # python_module.cu:53-57
        x = _flat_f64(xh_av, n, "xh_av")
        ph = _flat_f64(phi_ion, n, "phi_ion")
        if not ph.flags.writeable:
            raise ValueError("phi_ion must be writeable (it is filled in place)")
        _capi.check(self._lib.asora_do_all_sources(float(R), None, float(sig), float(dr), None, _capi.dptr(x),
                                                   _capi.dptr(ph), int(NumSrc), int(m1), float(minlogtau),
                                                   float(dlogtau), int(NumTau)), "do_all_sources")
        return None

    # ---- device-resident extension (include/asora_hip.h section B/C) ------------------------
    def grid_to_device(self, which, a):
        N = a.shape[0]
        if a.ndim != 3 or a.shape != (N, N, N):
            raise ValueError("grid must have shape (N,N,N)")
        a = np.asarray(a, dtype=np.float64)
        if a.flags.c_contiguous:
            order = b'C'
        elif a.flags.f_contiguous:
            order = b'F'
        else:
            a, order = np.ascontiguousarray(a), b'C'
        _capi.check(self._lib.asora_grid_to_device(int(which), _capi.dptr(a), int(N), order), "grid_to_device")

    def grid_to_host(self, which, out):
        N = out.shape[0]
        if out.dtype != np.float64 or out.shape != (N, N, N):
            raise ValueError("output grid must be float64 of shape (N,N,N)")
        if out.flags.c_contiguous:
            _capi.check(self._lib.asora_grid_to_host(int(which), _capi.dptr(out), int(N), b'C'), "grid_to_host")
        elif out.flags.f_contiguous:
            _capi.check(self._lib.asora_grid_to_host(int(which), _capi.dptr(out), int(N), b'F'), "grid_to_host")
        else:
            tmp = np.empty((N, N, N))
            _capi.check(self._lib.asora_grid_to_host(int(which), _capi.dptr(tmp), int(N), b'C'), "grid_to_host")
            out[...] = tmp
        return out

    def grid_copy(self, dst, src):
        _capi.check(self._lib.asora_grid_copy(int(dst), int(src)), "grid_copy")

    def grid_scale(self, which, factor):
        """grid *= factor on the device (c2ray_base.py:248 for a device-resident density)."""
        _capi.check(self._lib.asora_grid_scale(int(which), float(factor)), "grid_scale")

    def grid_sum(self, which):
        out = C.c_double(0.0)
        _capi.check(self._lib.asora_grid_sum(int(which), C.byref(out)), "grid_sum")
        return out.value

    def host_empty(self, shape, order='C'):
        """An uninitialised float64 array for a grid download, in page-locked memory when there is some (_pinned.py)."""
        return _pinned.empty(self._lib, shape, order)

    def device_ptr(self, which):
        return self._lib.asora_device_ptr(int(which))

    def raytrace_device(self, R, sig, dr, src_begin, src_count, minlogtau, dlogtau, NumTau):
        _capi.check(self._lib.asora_raytrace_device(float(R), float(sig), float(dr), int(src_begin), int(src_count),
                                                    float(minlogtau), float(dlogtau), int(NumTau)),
                    "raytrace_device")

    def raytrace_begin(self, R, sig, dr, minlogtau, dlogtau, NumTau):
        _capi.check(self._lib.asora_raytrace_begin(float(R), float(sig), float(dr), float(minlogtau), float(dlogtau),
                                                   int(NumTau)), "raytrace_begin")

    def raytrace_begin_planes(self, R, sig, dr, minlogtau, dlogtau, NumTau, runs):
        """runs: [(first plane, number of planes), ...] -- see asora_raytrace_begin_planes."""
        r = np.ascontiguousarray(np.asarray(runs, dtype=np.int32).reshape(-1, 2))
        _capi.check(self._lib.asora_raytrace_begin_planes(float(R), float(sig), float(dr), float(minlogtau),
                                                          float(dlogtau), int(NumTau), _capi.iptr(r), int(r.shape[0])),
                    "raytrace_begin_planes")

    def raytrace_range(self, src_begin, src_count):
        _capi.check(self._lib.asora_raytrace_range(int(src_begin), int(src_count)), "raytrace_range")

    def raytrace_fold(self, i_begin, i_count):
        _capi.check(self._lib.asora_raytrace_fold(int(i_begin), int(i_count)), "raytrace_fold")

    def stream_ptr(self):
        return self._lib.asora_stream()

    def chemistry_device(self, dt, bh00, albpow, colh0, temph0, abu_c):
        conv = C.c_int(0)
        s1 = C.c_double(0.0)
        s0 = C.c_double(0.0)
        _capi.check(self._lib.asora_chemistry_device(float(dt), float(bh00), float(albpow), float(colh0),
                                                     float(temph0), float(abu_c), C.byref(conv), C.byref(s1),
                                                     C.byref(s0)), "chemistry_device")
        return conv.value, s1.value, s0.value

    def device_init_auto(self, N):
        _capi.check(self._lib.asora_device_init_auto(int(N)), "device_init_auto")

    def subbox_raytrace_device(self, max_subbox, subboxsize, loss_fraction, R, sig, dr, minlogtau, dlogtau, NumTau,
                               src_begin, src_count):
        """(sum_nbox, photon_loss): the sub-box raytracer on the device-resident grids and uploaded sources."""
        nbox = C.c_int(0)
        loss = C.c_double(0.0)
        _capi.check(self._lib.asora_subbox_raytrace_device(int(max_subbox), int(subboxsize), float(loss_fraction), float(R),
                                                           float(sig), float(dr), float(minlogtau), float(dlogtau),
                                                           int(NumTau), int(src_begin), int(src_count), C.byref(nbox),
                                                           C.byref(loss)), "subbox_raytrace_device")
        return nbox.value, loss.value

    def chemistry_range(self, dt, bh00, albpow, colh0, temph0, abu_c, i_begin, i_count, first):
        _capi.check(self._lib.asora_chemistry_range(float(dt), float(bh00), float(albpow), float(colh0), float(temph0),
                                                    float(abu_c), int(i_begin), int(i_count), int(bool(first))),
                    "chemistry_range")

    def chemistry_finish(self):
        conv = C.c_int(0)
        s1 = C.c_double(0.0)
        s0 = C.c_double(0.0)
        _capi.check(self._lib.asora_chemistry_finish(C.byref(conv), C.byref(s1), C.byref(s0)), "chemistry_finish")
        return conv.value, s1.value, s0.value

    def reduction_ptr(self):
        """Device address of {sum x, sum 1-x, conv_flag} of the chemistry_range calls so far (three doubles)."""
        return self._lib.asora_reduction_ptr()

    def evolve_begin(self, dt, bh00, albpow, colh0, temph0, abu_c, R, sig, dr, minlogtau, dlogtau, NumTau,
                     src_begin, src_count, conv_criterion, convergence_fraction):
        """Start a time step of the device-resident loop (NDENS, TEMP, XH on the device)."""
        _capi.check(self._lib.asora_evolve_begin(float(dt), float(bh00), float(albpow), float(colh0), float(temph0),
                                                 float(abu_c), float(R), float(sig), float(dr), float(minlogtau),
                                                 float(dlogtau), int(NumTau), int(src_begin), int(src_count),
                                                 float(conv_criterion), float(convergence_fraction)), "evolve_begin")

    def evolve_enqueue(self, iterations):
        _capi.check(self._lib.asora_evolve_enqueue(int(iterations)), "evolve_enqueue")

    def evolve_poll(self, max_rows=32):
        """(niter, converged, rows): rows[q] = (conv_flag, sum_xh1, sum_xh0, rel_change_xh1, rel_change_xh0) of the
        iterations carried out since the last poll."""
        niter, done, got = C.c_int(0), C.c_int(0), C.c_int(0)
        hist = np.zeros((int(max_rows), 5))
        # max_rows = 0: the caller gives the rows up (the library's history ring holds 64 iterations between polls)
        _capi.check(self._lib.asora_evolve_poll(C.byref(niter), C.byref(done), _capi.dptr(hist) if max_rows > 0 else None,
                                                int(max_rows), C.byref(got)), "evolve_poll")
        return niter.value, bool(done.value), hist[:got.value]

    # ---- the device-resident loop with the sources sharded over several GPUs (asora_evolve_slab_*) ----
    def evolve_begin_slab(self, dt, bh00, albpow, colh0, temph0, abu_c, R, sig, dr, minlogtau, dlogtau, NumTau,
                          src_begin, src_count, conv_criterion, convergence_fraction, own_begin, own_count):
        _capi.check(self._lib.asora_evolve_begin_slab(float(dt), float(bh00), float(albpow), float(colh0), float(temph0),
                                                      float(abu_c), float(R), float(sig), float(dr), float(minlogtau),
                                                      float(dlogtau), int(NumTau), int(src_begin), int(src_count),
                                                      float(conv_criterion), float(convergence_fraction), int(own_begin),
                                                      int(own_count)), "evolve_begin_slab")

    def evolve_begin_slab_thermal(self, dt, bh00, albpow, colh0, temph0, abu_c, R, sig, dr, minlogtau, dlogtau, NumTau,
                                  src_begin, src_count, conv_criterion, convergence_fraction, own_begin, own_count):
        """The same step in thermal mode (thermal_params(True, ...) first): the caller exchanges the heating rates as well."""
        _capi.check(self._lib.asora_evolve_begin_slab_thermal(float(dt), float(bh00), float(albpow), float(colh0), float(temph0),
                                                              float(abu_c), float(R), float(sig), float(dr), float(minlogtau),
                                                              float(dlogtau), int(NumTau), int(src_begin), int(src_count),
                                                              float(conv_criterion), float(convergence_fraction), int(own_begin),
                                                              int(own_count)), "evolve_begin_slab_thermal")

    def evolve_slab_trace(self, src_begin, src_count):
        _capi.check(self._lib.asora_evolve_slab_trace(int(src_begin), int(src_count)), "evolve_slab_trace")

    def evolve_slab_fold_out(self, i_begin, i_count):
        _capi.check(self._lib.asora_evolve_slab_fold_out(int(i_begin), int(i_count)), "evolve_slab_fold_out")

    def evolve_slab_outbox_ptr(self):
        return self._lib.asora_evolve_slab_outbox()

    def evolve_slab_outbox_to_host(self, i_begin, i_count, N):
        out = np.empty((int(i_count), N, N))
        _capi.check(self._lib.asora_evolve_slab_outbox_to_host(int(i_begin), int(i_count), _capi.dptr(out)), "evolve_slab_outbox_to_host")
        return out

    def evolve_slab_outbox_from_host(self, i_begin, planes):
        a = np.ascontiguousarray(planes, dtype=np.float64)
        _capi.check(self._lib.asora_evolve_slab_outbox_from_host(int(i_begin), int(a.shape[0]), _capi.dptr(a)), "evolve_slab_outbox_from_host")

    def debug_placement(self):
        """How device_init placed the grids: {candidates tried, probe ms of the allocation kept, of the slowest one}."""
        n, a, b = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        self._lib.asora_debug_placement(C.byref(n), C.byref(a), C.byref(b))
        t, pr = C.c_double(0.0), C.c_double(0.0)
        self._lib.asora_debug_init_cost(C.byref(t), C.byref(pr))
        return {"candidates": n.value, "chosen_probe_ms": a.value, "slowest_probe_ms": b.value,
                "device_init_ms": t.value, "probe_cost_ms": pr.value}

    def live_buffers(self, lifetime):
        """(count, bytes) of the device and pinned buffers the library holds: lifetime 0 = the mesh's (released by device_close),
        1 = the process's (never released).  Host only."""
        n, b = C.c_longlong(0), C.c_ulonglong(0)
        _capi.check(self._lib.asora_debug_live_buffers(int(lifetime), C.byref(n), C.byref(b)), "debug_live_buffers")
        return n.value, b.value

    def evolve_slab_fold_all(self):
        _capi.check(self._lib.asora_evolve_slab_fold_all(), "evolve_slab_fold_all")

    def evolve_slab_add(self, i_begin, i_count, dev_ptr):
        """dev_ptr: device address of i_count*N*N doubles (e.g. torch tensor .data_ptr())."""
        _capi.check(self._lib.asora_evolve_slab_add(int(i_begin), int(i_count), C.c_void_p(int(dev_ptr))), "evolve_slab_add")

    def evolve_slab_add_host(self, i_begin, planes):
        a = np.ascontiguousarray(planes, dtype=np.float64)
        _capi.check(self._lib.asora_evolve_slab_add_host(int(i_begin), int(a.shape[0]), _capi.dptr(a)), "evolve_slab_add_host")

    # the heating rates of a step begun with evolve_begin_slab_thermal: the twins of the out-box and add calls above
    def evolve_slab_heat_outbox_ptr(self):
        return self._lib.asora_evolve_slab_heat_outbox()

    def evolve_slab_heat_outbox_to_host(self, i_begin, i_count, N):
        out = np.empty((int(i_count), N, N))
        _capi.check(self._lib.asora_evolve_slab_heat_outbox_to_host(int(i_begin), int(i_count), _capi.dptr(out)),
                    "evolve_slab_heat_outbox_to_host")
        return out

    def evolve_slab_heat_outbox_from_host(self, i_begin, planes):
        a = np.ascontiguousarray(planes, dtype=np.float64)
        _capi.check(self._lib.asora_evolve_slab_heat_outbox_from_host(int(i_begin), int(a.shape[0]), _capi.dptr(a)),
                    "evolve_slab_heat_outbox_from_host")

    def evolve_slab_add_heat(self, i_begin, i_count, dev_ptr):
        _capi.check(self._lib.asora_evolve_slab_add_heat(int(i_begin), int(i_count), C.c_void_p(int(dev_ptr))), "evolve_slab_add_heat")

    def evolve_slab_add_heat_host(self, i_begin, planes):
        a = np.ascontiguousarray(planes, dtype=np.float64)
        _capi.check(self._lib.asora_evolve_slab_add_heat_host(int(i_begin), int(a.shape[0]), _capi.dptr(a)), "evolve_slab_add_heat_host")

    def evolve_slab_pass(self):
        _capi.check(self._lib.asora_evolve_slab_pass(), "evolve_slab_pass")

    def evolve_slab_nhi(self, i_begin, i_count):
        _capi.check(self._lib.asora_evolve_slab_nhi(int(i_begin), int(i_count)), "evolve_slab_nhi")

    def evolve_slab_close(self, sums=None):
        """sums = None: {sum x, sum 1-x, conv_flag} at reduction_ptr() have been summed over the ranks in place; else the
        three sums over all ranks as (conv_flag, sum x, sum 1-x), the order chemistry_finish() returns them in."""
        if sums is None:
            _capi.check(self._lib.asora_evolve_slab_close(None), "evolve_slab_close")
        else:
            a = np.array([float(sums[1]), float(sums[2]), float(sums[0])])
            _capi.check(self._lib.asora_evolve_slab_close(_capi.dptr(a)), "evolve_slab_close")

    def planes_to_host(self, which, i_begin, i_count, N):
        out = np.empty((int(i_count), N, N))
        _capi.check(self._lib.asora_planes_to_host(int(which), int(i_begin), int(i_count), _capi.dptr(out)),
                    "planes_to_host")
        return out

    def planes_to_device(self, which, i_begin, planes):
        a = np.ascontiguousarray(planes, dtype=np.float64)
        _capi.check(self._lib.asora_planes_to_device(int(which), int(i_begin), int(a.shape[0]), _capi.dptr(a)),
                    "planes_to_device")

    def thermal_params(self, enable, relative_denergy=0.1, t_floor=1.0, max_substeps=10000, cooling_mask=31, compton=False,
                       t_cmb=0.0):
        """Switch asora_chemistry_device and the asora_evolve_* loop to the thermal form (enable) or back (include/asora_hip.h)."""
        _capi.check(self._lib.asora_thermal_params(int(bool(enable)), float(relative_denergy), float(t_floor), int(max_substeps),
                                                   int(cooling_mask), int(bool(compton)), float(t_cmb)), "thermal_params")

    def clumping(self, mode, constant=1.0):
        """Clumping of the recombination rate (include/asora_hip.h, asora_clumping): 0 off, 1 the one factor `constant`, 2 per
        cell from GRID_CLUMP (upload it first)."""
        _capi.check(self._lib.asora_clumping(int(mode), float(constant)), "clumping")

    def lls_opacity(self, n_const, per_density):
        """Lyman-limit-system opacity of the raytrace (include/asora_hip.h, asora_lls_opacity): the absorber density becomes
        ndens ((1 - xh_av) + per_density) + n_const; (0, 0) is off."""
        _capi.check(self._lib.asora_lls_opacity(float(n_const), float(per_density)), "lls_opacity")

    def get_lls_opacity(self):
        a, b = C.c_double(0.0), C.c_double(0.0)
        _capi.check(self._lib.asora_get_lls_opacity(C.byref(a), C.byref(b)), "get_lls_opacity")
        return a.value, b.value

    def plane_flux(self, face, flux, spectrum=None):
        """Plane-parallel flux through faces of the box (include/asora_hip.h, asora_plane_flux): sequences of equal length, face
        0 ... 5 = -x +x -y +y -z +z, flux in 1e48 photons s^-1 cm^-2, spectrum the table set (None: 0); empty sequences: off."""
        f = np.ascontiguousarray(face, dtype=np.int32).ravel()
        x = np.ascontiguousarray(flux, dtype=np.float64).ravel()
        s = np.zeros(f.size, dtype=np.int32) if spectrum is None else np.ascontiguousarray(spectrum, dtype=np.int32).ravel()
        if not (f.size == x.size == s.size):
            raise ValueError("plane_flux: face, flux and spectrum must have the same length")
        _capi.check(self._lib.asora_plane_flux(int(f.size), _capi.iptr(f), _capi.dptr(x), _capi.iptr(s)), "plane_flux")

    def get_plane_flux(self):
        """The setting as a list of (face, flux, spectrum)."""
        n = C.c_int(0)
        f, x, s = np.zeros(6, dtype=np.int32), np.zeros(6), np.zeros(6, dtype=np.int32)
        _capi.check(self._lib.asora_get_plane_flux(C.byref(n), _capi.iptr(f), _capi.dptr(x), _capi.iptr(s)), "get_plane_flux")
        return [(int(f[q]), float(x[q]), int(s[q])) for q in range(n.value)]

    def step_budget(self, chem, use_temp_end=False, planes=None):
        """The twelve sums of the photon budget of the step just run (include/asora_hip.h, asora_step_budget; the slots are
        ``_capi.BUDGET_*``), reduced on the device: an array of 12 float64.  `chem` = (dt, bh00, albpow, colh0, temph0, abu_c) as
        the chemistry calls take it (dt plays no part in the sums); `use_temp_end`: a thermal step, rates at the mean of TEMP and
        TEMP_END; `planes` = (i_begin, i_count), None: every plane."""
        _dt, bh00, albpow, colh0, temph0, abu_c = chem
        i_begin, i_count = (0, self._N) if planes is None else planes
        if i_count is None:
            raise RuntimeError("step_budget: planes=None needs a device initialised through device_init (the mesh size)")
        sums = np.zeros(_capi.BUDGET_COUNT, dtype=np.float64)
        _capi.check(self._lib.asora_step_budget(float(bh00), float(albpow), float(colh0), float(temph0), float(abu_c),
                                                1 if use_temp_end else 0, int(i_begin), int(i_count), _capi.dptr(sums)),
                    "step_budget")
        return sums

    def bubble_mfp(self, which, threshold, phase, periodic, seed, n_rays, l_max, edges, record=False):
        """The mean-free-path size distribution of the in-phase regions of device grid `which` (include/asora_hip.h,
        asora_bubble_mfp): ``(counts, tallies, moments)`` -- uint64 counts of the ``len(edges) - 1`` bins, the uint64 tallies
        (ended, capped, left_box, underflow, overflow, n_phase) and (sum L, sum L^2) over the ended rays, lengths in cells.
        `record`: a fourth value, the per-ray record ``(start (n, 3) int32, direction (n, 3), length (n,), status (n,) int32)``."""
        e = np.ascontiguousarray(edges, dtype=np.float64).ravel()
        n = int(n_rays)
        counts, tallies, moments = np.zeros(max(e.size - 1, 1), dtype=np.uint64), np.zeros(6, dtype=np.uint64), np.zeros(2)
        rec = (np.zeros((max(n, 0), 3), dtype=np.int32), np.zeros((max(n, 0), 3)), np.zeros(max(n, 0)),
               np.zeros(max(n, 0), dtype=np.int32)) if record else None
        u64 = lambda a: a.ctypes.data_as(_capi._u64p)
        _capi.check(self._lib.asora_bubble_mfp(int(which), float(threshold), int(phase), 1 if periodic else 0, int(seed), n, float(l_max),
                                               int(e.size) - 1, _capi.dptr(e), u64(counts), u64(tallies), _capi.dptr(moments),
                                               _capi.iptr(rec[0]) if record else None, _capi.dptr(rec[1]) if record else None,
                                               _capi.dptr(rec[2]) if record else None, _capi.iptr(rec[3]) if record else None),
                    "bubble_mfp")
        return (counts, tallies, moments, rec) if record else (counts, tallies, moments)

    def bubble_mask(self, which, threshold, phase):
        """The products of the threshold pass of bubble_mfp alone: ``(words (N, N, W) uint64, row counts (N, N) uint32)``, bit
        k & 63 of ``words[i, j, k >> 6]`` set where cell (i, j, k) is in phase."""
        if self._N is None:
            raise RuntimeError("bubble_mask needs a device initialised through device_init (the mesh size)")
        N = self._N
        words, rows = np.zeros((N, N, (N + 63) // 64), dtype=np.uint64), np.zeros((N, N), dtype=np.uint32)
        _capi.check(self._lib.asora_bubble_mask(int(which), float(threshold), int(phase), words.ctypes.data_as(_capi._u64p),
                                                rows.ctypes.data_as(C.POINTER(C.c_uint32))), "bubble_mask")
        return words, rows

    def region_sizes(self, which, threshold, phase, periodic, connectivity, edges, labels=False):
        """The connected in-phase regions of device grid `which` (include/asora_hip.h, asora_region_sizes): ``(counts, cells,
        tallies)`` -- per bin of ``edges`` (volumes in cells) the uint64 number of regions and the cells they hold, and the uint64
        tallies indexed by ``_capi.REGION_*``.  `labels`: a fourth value, the label of every cell, (N, N, N) uint32."""
        e = np.ascontiguousarray(edges, dtype=np.float64).ravel()
        nb = max(e.size - 1, 1)
        counts, cells = np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.uint64)
        tallies = np.zeros(_capi.REGION_TALLIES, dtype=np.uint64)
        grid = None
        if labels:
            if self._N is None:
                raise RuntimeError("region_sizes with labels needs a device initialised through device_init (the mesh size)")
            grid = np.zeros((self._N,) * 3, dtype=np.uint32)
        u64 = lambda a: a.ctypes.data_as(_capi._u64p)
        _capi.check(self._lib.asora_region_sizes(int(which), float(threshold), int(phase), 1 if periodic else 0, int(connectivity),
                                                 int(e.size) - 1, _capi.dptr(e), u64(counts), u64(cells), u64(tallies),
                                                 grid.ctypes.data_as(C.POINTER(C.c_uint32)) if labels else None), "region_sizes")
        return (counts, cells, tallies, grid) if labels else (counts, cells, tallies)

    def topology(self, which, threshold, phase, periodic, connectivity):
        """The element and component counts of the in-phase cells of device grid `which` (include/asora_hip.h, asora_topology): the
        uint64 tallies indexed by ``_capi.TOPO_*``."""
        tallies = np.zeros(_capi.TOPO_TALLIES, dtype=np.uint64)
        _capi.check(self._lib.asora_topology(int(which), float(threshold), int(phase), 1 if periodic else 0, int(connectivity),
                                             tallies.ctypes.data_as(_capi._u64p)), "topology")
        return tallies

    def granulometry(self, which, threshold, phase, periodic, radii, distances=False):
        """The erosion and opening counts of the in-phase cells of device grid `which` for the ascending `radii` (include/asora_hip.h,
        asora_granulometry): (eroded, opened, tallies), uint64 arrays, the tallies indexed by ``_capi.GRAN_*``; with `distances`
        also the squared distance transform, an (N, N, N) uint32 array."""
        radii = np.ascontiguousarray(radii, dtype=np.float64)
        if radii.ndim != 1:
            raise ValueError("granulometry: radii must be one-dimensional")
        eroded, opened = np.zeros(radii.size, dtype=np.uint64), np.zeros(radii.size, dtype=np.uint64)
        tallies = np.zeros(_capi.GRAN_TALLIES, dtype=np.uint64)
        grid = None
        if distances:
            if self._N is None:
                raise RuntimeError("granulometry with distances needs a device initialised through device_init (the mesh size)")
            grid = np.zeros((self._N,) * 3, dtype=np.uint32)
        _capi.check(self._lib.asora_granulometry(int(which), float(threshold), int(phase), 1 if periodic else 0, int(radii.size),
                                                 radii.ctypes.data_as(_capi._dp), eroded.ctypes.data_as(_capi._u64p),
                                                 opened.ctypes.data_as(_capi._u64p), tallies.ctypes.data_as(_capi._u64p),
                                                 grid.ctypes.data_as(C.POINTER(C.c_uint32)) if distances else None), "granulometry")
        return (eroded, opened, tallies, grid) if distances else (eroded, opened, tallies)

    def power_spectrum(self, kind_a, kind_b, scale, t_gamma, thresholds, field=False, modes=False):
        """The binned power sums of the field of kind `kind_a` (``_capi.PS_*``) formed from the device grids, and with `kind_b` (None:
        none) those of a second field and of their cross-spectrum (include/asora_hip.h, asora_power_spectrum), for the bins of the
        integer `thresholds` on n^2: a dict of ``count`` (uint64), ``sum_k``, ``sum_aa``, ``moments_a`` = (sum g, sum g^2), with
        `kind_b` also ``sum_bb``, ``sum_ab``, ``moments_b`` (else None); with `field` the formed field a, (N, N, N) float64, under
        ``field``, with `modes` its transform, (N, N, N // 2 + 1) complex128, under ``modes`` (else None)."""
        thr = np.ascontiguousarray(thresholds, dtype=np.uint32)
        if thr.ndim != 1:
            raise ValueError("power_spectrum: thresholds must be one-dimensional")
        nb = max(thr.size - 1, 1)
        cross = kind_b is not None
        out = dict(count=np.zeros(nb, dtype=np.uint64), sum_k=np.zeros(nb), sum_aa=np.zeros(nb), moments_a=np.zeros(2),
                   sum_bb=np.zeros(nb) if cross else None, sum_ab=np.zeros(nb) if cross else None,
                   moments_b=np.zeros(2) if cross else None, field=None, modes=None)
        if field or modes:
            if self._N is None:
                raise RuntimeError("power_spectrum with field or modes needs a device initialised through device_init (the mesh size)")
            if field:
                out["field"] = np.zeros((self._N,) * 3)
            if modes:
                out["modes"] = np.zeros((self._N, self._N, self._N // 2 + 1), dtype=np.complex128)
        ptr = lambda a: None if a is None else a.ctypes.data_as(_capi._dp)
        _capi.check(self._lib.asora_power_spectrum(int(kind_a), int(kind_b) if cross else -1, float(scale), float(t_gamma), int(thr.size) - 1,
                                                   thr.ctypes.data_as(C.POINTER(C.c_uint32)), out["count"].ctypes.data_as(_capi._u64p),
                                                   ptr(out["sum_k"]), ptr(out["sum_aa"]), ptr(out["sum_bb"]), ptr(out["sum_ab"]),
                                                   ptr(out["moments_a"]), ptr(out["moments_b"]), ptr(out["field"]), ptr(out["modes"])),
                    "power_spectrum")
        return out

    def power_spectrum_ms(self):
        """The stage times (ms) of the last power_spectrum call that ran with OPT_TIMING: mean density, the pass along k, along j,
        along i, the binning (include/asora_hip.h, asora_debug_power_spectrum_ms)."""
        ms = np.zeros(_capi.PS_STAGES)
        _capi.check(self._lib.asora_debug_power_spectrum_ms(_capi.dptr(ms)), "debug_power_spectrum_ms")
        return ms

    def smooth_field(self, kind, scale, t_gamma, w_i=None, w_j=None, w_k=None, w_r=None, subtract_mean=False, edges=None, dst_grid=None,
                     field=False):
        """The field of kind `kind` (``_capi.PS_*``) formed from the device grids, multiplied by the filter of the tables `w_i`, `w_j`,
        `w_k` ((N,) each) and `w_r` ((3 (N // 2)^2 + 1,)) -- None: all ones -- in Fourier space and transformed back, with its
        one-point statistics (include/asora_hip.h, asora_smooth_field): a dict of ``stats`` (``_capi.SMOOTH_STATS`` float64, indexed
        by ``_capi.SMOOTH_*``), ``hist`` (with `edges`: uint64, the ``len(edges) - 1`` bins, then the cells below and the cells at or
        above; else None) and ``field`` (with `field`: (N, N, N) float64; else None).  `dst_grid`: the grid the result is written
        into (None: a buffer of the library's own)."""
        tables = []
        for name, w in (("w_i", w_i), ("w_j", w_j), ("w_k", w_k), ("w_r", w_r)):
            if w is not None:
                w = np.ascontiguousarray(w, dtype=np.float64)
                if w.ndim != 1:
                    raise ValueError(f"smooth_field: {name} must be one-dimensional")
                if name != "w_r" and (self._N is None or w.size != self._N):       # (the library reads N entries; w_r carries its length)
                    raise ValueError(f"smooth_field: {name} must have the N = {self._N} entries of the mesh of device_init, not {w.size}")
            tables.append(w)
        e = None
        if edges is not None:
            e = np.ascontiguousarray(edges, dtype=np.float64)
            if e.ndim != 1 or e.size < 2:
                raise ValueError("smooth_field: edges must be one-dimensional, two or more")
        out = dict(stats=np.zeros(_capi.SMOOTH_STATS), hist=None if e is None else np.zeros(e.size + 1, dtype=np.uint64), field=None)
        if field:
            if self._N is None:
                raise RuntimeError("smooth_field with field needs a device initialised through device_init (the mesh size)")
            out["field"] = np.zeros((self._N,) * 3)
        ptr = lambda a: None if a is None else a.ctypes.data_as(_capi._dp)
        _capi.check(self._lib.asora_smooth_field(int(kind), float(scale), float(t_gamma), ptr(tables[0]), ptr(tables[1]), ptr(tables[2]),
                                                 ptr(tables[3]), 0 if tables[3] is None else int(tables[3].size), 1 if subtract_mean else 0,
                                                 0 if e is None else int(e.size) - 1, ptr(e), -1 if dst_grid is None else int(dst_grid),
                                                 ptr(out["stats"]), None if e is None else out["hist"].ctypes.data_as(_capi._u64p),
                                                 ptr(out["field"])), "smooth_field")
        return out

    def smooth_field_ms(self):
        """The stage times (ms) of the last smooth_field call that ran with OPT_TIMING: mean density, forward along k, j, i, back
        along i with the filter, along j, along k with the first statistics, the central moments and the histogram
        (include/asora_hip.h, asora_debug_smooth_field_ms)."""
        ms = np.zeros(_capi.SMOOTH_STAGES)
        _capi.check(self._lib.asora_debug_smooth_field_ms(_capi.dptr(ms)), "debug_smooth_field_ms")
        return ms

    def los_velocity_to_device(self, v):
        """The line-of-sight velocity of power_spectrum_los and redshift_space_field, (N, N, N) float64, into the library's own
        buffer (include/asora_hip.h, asora_los_velocity_to_device); returns max |v|, reduced on the device.  A non-finite entry is
        refused."""
        v = np.asarray(v, dtype=np.float64)
        if self._N is None or v.shape != (self._N,) * 3:
            raise ValueError(f"los_velocity_to_device: the velocity must have the shape ({self._N},) * 3 of the mesh of device_init, "
                             f"not {v.shape}")
        order = b"F" if (v.flags.f_contiguous and not v.flags.c_contiguous) else b"C"
        if order == b"C":
            v = np.ascontiguousarray(v)
        vmax = C.c_double(0.0)
        _capi.check(self._lib.asora_los_velocity_to_device(_capi.dptr(v), int(self._N), order, C.byref(vmax)), "los_velocity_to_device")
        return vmax.value

    def los_velocity_clear(self):
        _capi.check(self._lib.asora_los_velocity_clear(), "los_velocity_clear")

    def power_spectrum_los(self, kind, scale, t_gamma, los_axis, velocity_scale, mode, thr_a, thr_b, field=False, modes=False):
        """The anisotropic power sums of the field of kind `kind` (``_capi.PS_*``) formed from the device grids and, with
        `velocity_scale` not None, moved into redshift space along `los_axis` by the velocity of los_velocity_to_device
        (include/asora_hip.h, asora_power_spectrum_los), in the bins of `mode` (``_capi.ANISO_*``), `thr_a` (integers) and `thr_b`
        (doubles): a dict of ``count`` (uint64), ``sum_1``, ``sum_2``, ``sum_aa``, ``sum_l2``, ``sum_l4``, each (n_a, n_b),
        ``moments_real`` and ``moments_rs`` = (sum, sum of squares) of the field before and after the mapping; with `field` the
        mapped field, (N, N, N), under ``field``, with `modes` its transform, (N, N, N // 2 + 1) complex128, under ``modes``."""
        ta = np.ascontiguousarray(thr_a, dtype=np.uint32)
        tb = np.ascontiguousarray(thr_b, dtype=np.float64)
        if ta.ndim != 1 or tb.ndim != 1 or ta.size < 2 or tb.size < 2:
            raise ValueError("power_spectrum_los: thr_a and thr_b must be one-dimensional, two or more values each")
        shape = (ta.size - 1, tb.size - 1)
        out = dict(count=np.zeros(shape, dtype=np.uint64), moments_real=np.zeros(2), moments_rs=np.zeros(2), field=None, modes=None)
        for name in ("sum_1", "sum_2", "sum_aa", "sum_l2", "sum_l4"):
            out[name] = np.zeros(shape)
        if field or modes:
            if self._N is None:
                raise RuntimeError("power_spectrum_los with field or modes needs a device initialised through device_init (the mesh size)")
            if field:
                out["field"] = np.zeros((self._N,) * 3)
            if modes:
                out["modes"] = np.zeros((self._N, self._N, self._N // 2 + 1), dtype=np.complex128)
        ptr = lambda a: None if a is None else a.ctypes.data_as(_capi._dp)
        use = velocity_scale is not None
        _capi.check(self._lib.asora_power_spectrum_los(int(kind), float(scale), float(t_gamma), int(los_axis), 1 if use else 0,
                                                       float(velocity_scale) if use else 0.0, int(mode), shape[0],
                                                       ta.ctypes.data_as(C.POINTER(C.c_uint32)), shape[1], ptr(tb),
                                                       out["count"].ctypes.data_as(_capi._u64p), ptr(out["sum_1"]), ptr(out["sum_2"]),
                                                       ptr(out["sum_aa"]), ptr(out["sum_l2"]), ptr(out["sum_l4"]), ptr(out["moments_real"]),
                                                       ptr(out["moments_rs"]), ptr(out["field"]), ptr(out["modes"])), "power_spectrum_los")
        return out

    def power_spectrum_los_ms(self):
        """The stage times (ms) of the last power_spectrum_los call that ran with OPT_TIMING: mean density, the mapping, the passes
        along k, j and i, the binning (include/asora_hip.h, asora_debug_power_spectrum_los_ms)."""
        ms = np.zeros(_capi.PSLOS_STAGES)
        _capi.check(self._lib.asora_debug_power_spectrum_los_ms(_capi.dptr(ms)), "debug_power_spectrum_los_ms")
        return ms

    def redshift_space_field(self, kind, scale, t_gamma, los_axis, velocity_scale, dst_grid=None, field=False):
        """The field of kind `kind` moved into redshift space along `los_axis` (`velocity_scale` None: left where it is), kept on
        the device or written into the grid `dst_grid` (include/asora_hip.h, asora_redshift_space_field): a dict of ``moments`` =
        (sum g, sum g^2) of the real-space field and ``field`` (with `field`: (N, N, N) float64; else None)."""
        out = dict(moments=np.zeros(2), field=None)
        if field:
            if self._N is None:
                raise RuntimeError("redshift_space_field with field needs a device initialised through device_init (the mesh size)")
            out["field"] = np.zeros((self._N,) * 3)
        use = velocity_scale is not None
        _capi.check(self._lib.asora_redshift_space_field(int(kind), float(scale), float(t_gamma), int(los_axis), 1 if use else 0,
                                                         float(velocity_scale) if use else 0.0, -1 if dst_grid is None else int(dst_grid),
                                                         _capi.dptr(out["moments"]),
                                                         None if out["field"] is None else _capi.dptr(out["field"])),
                    "redshift_space_field")
        return out

    def lyman_alpha_forest(self, los_axis, velocity_scale, b_scale, tau_scale, window=0, gap_threshold=0.05, edges=None, dst_grid=None,
                           dst_what=_capi.LYA_FLUX, tau=False, flux=False):
        """The Lyman-alpha forest of the device grids along `los_axis`, moved by the velocity of los_velocity_to_device with
        `velocity_scale` not None (include/asora_hip.h, asora_lyman_alpha_forest): a dict of ``stats`` (``_capi.LYA_STATS`` float64,
        indexed by ``_capi.LYA_SUM_F`` ...), ``counts`` (``_capi.LYA_COUNTS`` uint64, indexed by ``_capi.LYA_NONFINITE`` ...), ``gaps``
        (uint64, N + 1: the gaps by length), ``pdf`` (with `edges`: uint64, ``len(edges) - 1`` bins; else None), ``tau`` and ``flux``
        (with `tau`, `flux`: (N, N, N) float64; else None).  `window`: W, or 0 for the automatic one; `dst_grid`: the grid F
        (`dst_what` = ``_capi.LYA_FLUX``) or tau (``_capi.LYA_TAU``) is written into (None: none)."""
        if self._N is None:
            raise RuntimeError("lyman_alpha_forest needs a device initialised through device_init (the mesh size)")
        e = None
        if edges is not None:
            e = np.ascontiguousarray(edges, dtype=np.float64)
            if e.ndim != 1 or e.size < 2:
                raise ValueError("lyman_alpha_forest: edges must be one-dimensional, two or more")
        out = dict(stats=np.zeros(_capi.LYA_STATS), counts=np.zeros(_capi.LYA_COUNTS, dtype=np.uint64),
                   gaps=np.zeros(self._N + 1, dtype=np.uint64), pdf=None if e is None else np.zeros(e.size - 1, dtype=np.uint64),
                   tau=np.zeros((self._N,) * 3) if tau else None, flux=np.zeros((self._N,) * 3) if flux else None)
        ptr = lambda a: None if a is None else a.ctypes.data_as(_capi._dp)
        uptr = lambda a: None if a is None else a.ctypes.data_as(_capi._u64p)
        use = velocity_scale is not None
        _capi.check(self._lib.asora_lyman_alpha_forest(int(los_axis), 1 if use else 0, float(velocity_scale) if use else 0.0, float(b_scale),
                                                       float(tau_scale), int(window), float(gap_threshold), 0 if e is None else int(e.size) - 1,
                                                       ptr(e), -1 if dst_grid is None else int(dst_grid), int(dst_what), ptr(out["stats"]),
                                                       uptr(out["counts"]), uptr(out["pdf"]), uptr(out["gaps"]), ptr(out["tau"]),
                                                       ptr(out["flux"])), "lyman_alpha_forest")
        return out

    def lyman_alpha_forest_ms(self):
        """The stage times (ms) of the last lyman_alpha_forest call that ran with OPT_TIMING: the largest reach with its read-back,
        the optical depth with the gaps, the statistics, the fold (include/asora_hip.h, asora_debug_lya_forest_ms)."""
        ms = np.zeros(_capi.LYA_STAGES)
        _capi.check(self._lib.asora_debug_lya_forest_ms(_capi.dptr(ms)), "debug_lya_forest_ms")
        return ms

    def lyman_alpha_forest_tiles(self, N, los_axis):
        """How lyman_alpha_forest deals the lines along `los_axis` of a mesh of N cells a side to its workgroups: a dict of ``lines``
        (of a tile), ``work_items`` (of a workgroup), ``workgroups`` and ``lds_bytes`` (include/asora_hip.h,
        asora_debug_lya_forest_tiles); needs no device."""
        t = np.zeros(4, dtype=np.int32)
        _capi.check(self._lib.asora_debug_lya_forest_tiles(int(N), int(los_axis), _capi.iptr(t)), "debug_lya_forest_tiles")
        return dict(lines=int(t[0]), work_items=int(t[1]), workgroups=int(t[2]), lds_bytes=int(t[3]))

    def bispectrum(self, kind, scale, t_gamma, thresholds, triangles):
        """The triangle sums of the field of kind `kind` (``_capi.PS_*``) formed from the device grids, for the shells of the integer
        `thresholds` on n^2 and the `triangles`, (n_tri, 3) shell indices (include/asora_hip.h, asora_bispectrum): a dict of
        ``sum_ggg`` and ``sum_iii`` (float64, one per triangle), ``count`` (uint64), ``sum_k``, ``sum_aa`` (one per shell) and
        ``moments`` = (sum g, sum g^2)."""
        thr = np.ascontiguousarray(thresholds, dtype=np.uint32)
        if thr.ndim != 1:
            raise ValueError("bispectrum: thresholds must be one-dimensional")
        tri = np.ascontiguousarray(triangles, dtype=np.int32)
        if tri.ndim != 2 or tri.shape[1] != 3:
            raise ValueError("bispectrum: triangles must have the shape (n_tri, 3)")
        ns, nt = max(thr.size - 1, 1), max(tri.shape[0], 1)
        out = dict(sum_ggg=np.zeros(nt), sum_iii=np.zeros(nt), count=np.zeros(ns, dtype=np.uint64), sum_k=np.zeros(ns), sum_aa=np.zeros(ns),
                   moments=np.zeros(2))
        _capi.check(self._lib.asora_bispectrum(int(kind), float(scale), float(t_gamma), int(thr.size) - 1,
                                               thr.ctypes.data_as(C.POINTER(C.c_uint32)), int(tri.shape[0]), _capi.iptr(tri),
                                               _capi.dptr(out["sum_ggg"]), _capi.dptr(out["sum_iii"]), out["count"].ctypes.data_as(_capi._u64p),
                                               _capi.dptr(out["sum_k"]), _capi.dptr(out["sum_aa"]), _capi.dptr(out["moments"])), "bispectrum")
        return out

    def bispectrum_ms(self):
        """The stage times (ms) of the last bispectrum call that ran with OPT_TIMING: mean density, forward along k, j, i, the
        per-shell binning, the shell fields and the products of the field, the shell fields and the products of the counts (0, 0
        when the kept counts were returned) (include/asora_hip.h, asora_debug_bispectrum_ms)."""
        ms = np.zeros(_capi.BISPEC_STAGES)
        _capi.check(self._lib.asora_debug_bispectrum_ms(_capi.dptr(ms)), "debug_bispectrum_ms")
        return ms

    def bispectrum_plan(self, N, n_shells, n_tri):
        """How bispectrum's product stage deals `n_tri` triangles and the cells of a mesh of N a side: a dict of ``chunk`` (the
        triangles of one pass over the cubes), ``passes``, ``workgroups``, ``trips_max`` and ``trips_min`` (the tiles a workgroup
        takes), ``wave_chunk``, ``tile_cells`` and ``idle_workgroups`` (include/asora_hip.h, asora_debug_bispectrum_plan); needs no
        device."""
        t = np.zeros(_capi.BISPEC_PLAN_WORDS, dtype=np.int32)
        _capi.check(self._lib.asora_debug_bispectrum_plan(int(N), int(n_shells), int(n_tri), _capi.iptr(t)), "debug_bispectrum_plan")
        return dict(zip(("chunk", "passes", "workgroups", "trips_max", "trips_min", "wave_chunk", "tile_cells", "idle_workgroups"),
                        (int(v) for v in t)))

    def lightcone_advance(self, slot, kind, src_grid, t_gamma, los_axis, planes, w_prev, w_now, refresh, slices=True):
        """Slices of a light cone for `slot`: plane ``planes[t]`` along `los_axis` of the slot's kept field times ``w_prev[t]`` plus
        the same plane of the field formed from the device grids now times ``w_now[t]`` -- the field of kind `kind` (``_capi.PS_*``),
        or with `src_grid` (a ``_capi.GRID_*`` selector; None: none) that grid verbatim -- and with `refresh` the present field kept
        for the next call (include/asora_hip.h, asora_lightcone_advance): a dict of ``slices`` ((n, N, N) float64; None with
        ``slices=False``, when only the moments cross to the host) and ``moments`` ((n, 2): the sum and the sum of squares of each
        slice)."""
        if self._N is None:
            raise RuntimeError("lightcone_advance needs a device initialised through device_init (the mesh size)")
        p = np.ascontiguousarray(planes, dtype=np.int32)
        wp, wn = np.ascontiguousarray(w_prev, dtype=np.float64), np.ascontiguousarray(w_now, dtype=np.float64)
        if p.ndim != 1 or wp.shape != p.shape or wn.shape != p.shape:
            raise ValueError("lightcone_advance: planes, w_prev and w_now must be one-dimensional and of one length")
        n = int(p.size)
        out = dict(slices=np.zeros((n, self._N, self._N)) if slices else None, moments=np.zeros((n, 2)))
        some = n > 0
        _capi.check(self._lib.asora_lightcone_advance(int(slot), int(kind), -1 if src_grid is None else int(src_grid), float(t_gamma),
                                                      int(los_axis), n, _capi.iptr(p) if some else None, _capi.dptr(wp) if some else None,
                                                      _capi.dptr(wn) if some else None, 1 if refresh else 0,
                                                      _capi.dptr(out["slices"]) if slices and some else None,
                                                      _capi.dptr(out["moments"]) if some else None), "lightcone_advance")
        return out

    def lightcone_state(self, slot):
        """What `slot` keeps: a dict of ``has_prev`` (bool), ``kind`` and ``src_grid`` (None: none) of its kept field
        (include/asora_hip.h, asora_lightcone_state)."""
        has, kind, src = C.c_int(0), C.c_int(0), C.c_int(-1)
        _capi.check(self._lib.asora_lightcone_state(int(slot), C.byref(has), C.byref(kind), C.byref(src)), "lightcone_state")
        return dict(has_prev=bool(has.value), kind=int(kind.value), src_grid=None if src.value < 0 else int(src.value))

    def lightcone_reset(self, slot):
        _capi.check(self._lib.asora_lightcone_reset(int(slot)), "lightcone_reset")

    def lightcone_ms(self):
        """The stage times (ms) of the last lightcone_advance call that ran with OPT_TIMING: mean density, emit, moments, refresh
        (include/asora_hip.h, asora_debug_lightcone_ms)."""
        ms = np.zeros(_capi.LC_STAGES)
        _capi.check(self._lib.asora_debug_lightcone_ms(_capi.dptr(ms)), "debug_lightcone_ms")
        return ms

    def halo_catalogue_to_device(self, pos, mass, weight, m_lm, m_hm, wrap, unit_exponent):
        """Uploads a halo catalogue -- `pos` (n, 3) in cell units, `mass` and `weight` (n) -- and bins it on the device into the
        table of its occupied cells with the unit 2^`unit_exponent` (include/asora_hip.h, asora_halo_catalogue_to_device): a dict
        of ``n_cells``, ``outside``, ``nonfinite`` and ``below``.  It replaces the catalogue the device held."""
        p = np.ascontiguousarray(pos, dtype=np.float64)
        m, w = np.ascontiguousarray(mass, dtype=np.float64), np.ascontiguousarray(weight, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 3 or m.shape != (p.shape[0],) or w.shape != m.shape:
            raise ValueError("halo_catalogue_to_device: pos must be (n, 3), mass and weight (n)")
        n = int(m.size)
        counts = (C.c_longlong * 4)()
        some = n > 0
        _capi.check(self._lib.asora_halo_catalogue_to_device(_capi.dptr(p) if some else None, _capi.dptr(m) if some else None,
                                                             _capi.dptr(w) if some else None, n, float(m_lm), float(m_hm),
                                                             1 if wrap else 0, int(unit_exponent), counts), "halo_catalogue_to_device")
        return dict(zip(("n_cells", "outside", "nonfinite", "below"), (int(v) for v in counts)))

    def halo_catalogue_clear(self):
        _capi.check(self._lib.asora_halo_catalogue_clear(), "halo_catalogue_clear")

    def halo_catalogue_state(self):
        """(n_cells, unit_exponent) of the catalogue the device holds, or None without one.  Host only."""
        n, e, g = C.c_longlong(0), C.c_int(0), C.c_longlong(0)
        _capi.check(self._lib.asora_halo_catalogue_state(C.byref(n), C.byref(e), C.byref(g)), "halo_catalogue_state")
        return None if n.value < 0 else (int(n.value), int(e.value))

    def halo_catalogue_generation(self):
        """The number of the catalogue the device holds -- every upload in this process takes the next one -- or None without
        one.  Host only."""
        n, e, g = C.c_longlong(0), C.c_int(0), C.c_longlong(0)
        _capi.check(self._lib.asora_halo_catalogue_state(C.byref(n), C.byref(e), C.byref(g)), "halo_catalogue_state")
        return None if n.value < 0 else int(g.value)

    def halo_table_to_host(self):
        """The table of the catalogue on the device: (cell int64, Q_hm uint64, Q_lm uint64), one entry per occupied cell in
        ascending cell index (include/asora_hip.h, asora_halo_table_to_host)."""
        state = self.halo_catalogue_state()
        n = 0 if state is None else state[0]
        cell, q_hm, q_lm = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        _capi.check(self._lib.asora_halo_table_to_host(cell.ctypes.data_as(C.POINTER(C.c_int64)), q_hm.ctypes.data_as(_capi._u64p),
                                                       q_lm.ctypes.data_as(_capi._u64p), n), "halo_table_to_host")
        return cell, q_hm, q_lm

    def halo_sources_build(self, which_grid, g_hm, g_lm, scale, model, x_suppress, f_suppressed):
        """The source list of the catalogue on the device and device grid `which_grid` (include/asora_hip.h,
        asora_halo_sources_build): a dict of ``pos`` ((n_active, 3) int32, 0-based), ``flux`` (n_active) and ``summary`` (five
        Python ints: n_active, n_suppressed, sum Q_hm, sum Q_lm not suppressed, sum Q_lm suppressed)."""
        summary = (C.c_ulonglong * _capi.HALO_SUMMARY)()
        n = C.c_longlong(0)
        _capi.check(self._lib.asora_halo_sources_build(int(which_grid), float(g_hm), float(g_lm), float(scale), int(model), float(x_suppress),
                                                       float(f_suppressed), summary, C.byref(n)), "halo_sources_build")
        pos, flux = np.zeros((n.value, 3), dtype=np.int32), np.zeros(n.value)
        _capi.check(self._lib.asora_halo_sources_to_host(_capi.iptr(pos), _capi.dptr(flux), n.value), "halo_sources_to_host")
        return dict(pos=pos, flux=flux, summary=[int(v) for v in summary])

    def halo_sources_ms(self):
        """The stage times (ms) of the last catalogue call (zeroing and upload, bin, row counts and scan, room, table) and of the last build
        (flux, scan, emit) that ran with OPT_TIMING (include/asora_hip.h, asora_debug_halo_sources_ms)."""
        ms = np.zeros(_capi.HALO_STAGES)
        _capi.check(self._lib.asora_debug_halo_sources_ms(_capi.dptr(ms)), "debug_halo_sources_ms")
        return ms

    def thermal_stats(self):
        """(cells that hit max_substeps, cells clamped to t_floor, most substeps of one integration) since the last
        chemistry_device / evolve_begin."""
        capped, floored, most = C.c_longlong(0), C.c_longlong(0), C.c_int(0)
        _capi.check(self._lib.asora_thermal_stats(C.byref(capped), C.byref(floored), C.byref(most)), "thermal_stats")
        return capped.value, floored.value, most.value

    def set_option(self, option, value):
        _capi.check(self._lib.asora_set_option(int(option), int(value)), "set_option")

    def get_option(self, option):
        return self._lib.asora_get_option(int(option))

    def kernel_time_ms(self, kernel):
        ms = C.c_double(0.0)
        n = C.c_long(0)
        _capi.check(self._lib.asora_kernel_time_ms(int(kernel), C.byref(ms), C.byref(n)), "kernel_time_ms")
        return ms.value, n.value

    def kernel_time_reset(self):
        self._lib.asora_kernel_time_reset()

    def synchronize(self):
        _capi.check(self._lib.asora_synchronize(), "synchronize")

    def last_raytrace_counts(self):
        g = C.c_longlong(0)
        e = C.c_longlong(0)
        _capi.check(self._lib.asora_last_raytrace_counts(C.byref(g), C.byref(e)), "last_raytrace_counts")
        return g.value, e.value

    def last_raytrace_zero_rates(self):
        """Of the rate-receiving pairs of the last raytrace: how many got exactly +0 and were not added (ASORA_OPT_SKIP_ZERO_RATES)."""
        g, e, z = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        _capi.check(self._lib.asora_last_raytrace_counts_ex(C.byref(g), C.byref(e), C.byref(z)), "last_raytrace_counts_ex")
        return z.value

    def last_raytrace_variant(self):
        """{"paired", "aligned", "buffer_atomics", "split_descriptors", "skip_zero", "global_shells", "open": bool, "units", "threads"} of the
        last raytrace launch (asora_last_raytrace_variant)."""
        return self.variant_fields(self._lib.asora_last_raytrace_variant())

    @staticmethod
    def variant_fields(v):
        """The fields of an ASORA_VARIANT_* word (last_raytrace_variant, launch_plan)."""
        return {"paired": bool(v & 1), "aligned": bool(v & 2), "buffer_atomics": bool(v & 4), "split_descriptors": bool(v & 8),
                "skip_zero": bool(v & 16), "global_shells": bool(v & 32), "open": bool(v & _capi.VARIANT_OPEN_BOUNDARIES), "units": (v >> 8) & 255, "threads": v >> 16}

    FORM_FIELDS = ("threads", "global_scratch", "dump", "heat", "tabcap", "skip_zero", "grey", "bufatom", "nsrc", "subbox", "split",
                   "spec", "open")

    def launch_plan(self, N, R, src_count, shape_src_count=0, cu_count=0, shells=-1, max_cells=0, heat=False, dump=False,
                    table_sets=False, host_positions=True, radius_stays=True, rate_tables=True):
        """What a raytrace launch would be under the options as they stand (asora_debug_launch_plan; host only, no device needed):
        {"units", "threads", "aligned"}, and with `shells` >= 0 also "form" (the kernel's template arguments by name), "use_lds",
        "lds_bytes", "variant" (the word of asora_last_raytrace_variant), "built", "zero_form_exists".  A combination the launcher
        refuses raises RuntimeError with its code and message."""
        flags = ((_capi.PLAN_HEAT if heat else 0) | (_capi.PLAN_DUMP if dump else 0) | (_capi.PLAN_TABLE_SETS if table_sets else 0) |
                 (_capi.PLAN_HOST_POSITIONS if host_positions else 0) | (_capi.PLAN_RADIUS_STAYS if radius_stays else 0) |
                 (_capi.PLAN_RATE_TABLES if rate_tables else 0))
        out = np.zeros(_capi.PLAN_WORDS, dtype=np.int32)
        _capi.check(self._lib.asora_debug_launch_plan(int(N), float(R), int(src_count), int(shape_src_count), int(cu_count), flags,
                                                      int(shells), int(max_cells), _capi.iptr(out)), "launch_plan")
        plan = {"units": int(out[0]), "threads": int(out[1]), "aligned": bool(out[2])}
        if out[21]:
            form = {k: int(v) if k in ("threads", "tabcap", "nsrc") else bool(v) for k, v in zip(self.FORM_FIELDS, out[3:16])}
            plan.update(form=form, use_lds=bool(out[16]), lds_bytes=int(out[17]), variant=int(out[18]), built=bool(out[19]),
                        zero_form_exists=bool(out[20]))
        return plan

    def built_forms(self):
        """The forms raytrace_octant_kernel is built in (asora_debug_built_forms; host only, no device needed): a list of 13-tuples
        of ints in the order of FORM_FIELDS, one per row of the launcher's table."""
        rows = C.c_int(0)
        _capi.check(self._lib.asora_debug_built_forms(None, 0, C.byref(rows)), "built_forms")
        out = np.zeros((rows.value, 13), dtype=np.int32)
        _capi.check(self._lib.asora_debug_built_forms(_capi.iptr(out), rows.value, C.byref(rows)), "built_forms")
        return [tuple(int(v) for v in r) for r in out]

    def form_launches(self):
        """Launches of every row of built_forms() this process has made since reset_form_launches (asora_debug_form_launches): a
        uint64 array.  The counters outlive device_close."""
        rows = C.c_int(0)
        _capi.check(self._lib.asora_debug_form_launches(None, 0, C.byref(rows)), "form_launches")
        out = np.zeros(rows.value, dtype=np.uint64)
        _capi.check(self._lib.asora_debug_form_launches(out.ctypes.data_as(C.POINTER(C.c_ulonglong)), rows.value, C.byref(rows)), "form_launches")
        return out

    def reset_form_launches(self):
        _capi.check(self._lib.asora_debug_form_launches_reset(), "reset_form_launches")

    def last_launch_form(self):
        """(form, row) of the last raytrace launch (asora_debug_last_launch_form): the 13-tuple of built_forms() and its row index;
        (None, -1) before the first launch."""
        form, row = np.zeros(13, dtype=np.int32), C.c_int(0)
        _capi.check(self._lib.asora_debug_last_launch_form(_capi.iptr(form), C.byref(row)), "last_launch_form")
        return (tuple(int(v) for v in form) if row.value >= 0 else None), row.value

    @staticmethod
    def form_text(form):
        """A form as DESIGN.md and the launcher's messages write it: <256,0,0,1,...>."""
        return "<" + ",".join(str(int(v)) for v in form) + ">"

    SUBBOX_LAUNCH_FIELDS = ("valid", "table_sources", "units", "threads", "nsrc", "aligned", "heat", "table_launches", "fly_sources",
                            "fly_threads", "fly_lds_shells", "fly_heat", "fly_launches", "batches")

    def last_subbox_launch(self):
        """What the last sub-box call launched (asora_debug_last_subbox_launch), recorded where its launches are made: sources swept on
        tables, their "units", "threads", "nsrc" (sources per workgroup), "aligned" and "heat"; sources swept on the fly, that kernel's
        "fly_threads", "fly_lds_shells" (else global shells) and "fly_heat"; sweep launches of either kind; "batches"."""
        out = np.zeros(_capi.SUBBOX_LAUNCH_WORDS, dtype=np.int32)
        _capi.check(self._lib.asora_debug_last_subbox_launch(_capi.iptr(out)), "last_subbox_launch")
        return {k: int(v) for k, v in zip(self.SUBBOX_LAUNCH_FIELDS, out)}

    def subbox_plan(self, N, R, max_subbox, src_count, has_dump=True, heat=False, cu_count=0):
        """What a sub-box call would launch under the options as they stand, before the built geometry has its say
        (asora_debug_subbox_plan; host only, no device needed): {"table_sources", "units", "threads", "nsrc", "aligned", "fly_sources",
        "fly_threads", "S_tab"}."""
        out = np.zeros(_capi.SUBBOX_PLAN_WORDS, dtype=np.int32)
        _capi.check(self._lib.asora_debug_subbox_plan(int(N), float(R), int(max_subbox), int(src_count), int(bool(has_dump)), int(bool(heat)),
                                                      int(cu_count), _capi.iptr(out)), "subbox_plan")
        keys = ("table_sources", "units", "threads", "nsrc", "aligned", "fly_sources", "fly_threads", "S_tab")
        return {k: int(v) for k, v in zip(keys, out)}

    def block_order(self, pos0, units, nsrc, aligned, begin=0, count=None, cu_count=0):
        """Which workgroup sweeps what in a raytrace launch that is not spread (asora_debug_block_order; host only, no device needed):
        an (blocks, 4) int32 array of {group, unit, first source, second source or -1}, all -1 for a block that does nothing; blocks
        b % 8 == x run on XCD x in the order of b.  None for a launch so small that it is spread."""
        pos0 = np.ascontiguousarray(pos0, dtype=np.int32).ravel()
        count = pos0.size // 3 - begin if count is None else count
        grid = C.c_int(0)
        args = (_capi.iptr(pos0), int(begin), int(count), int(units), int(nsrc), int(bool(aligned)), int(cu_count))
        _capi.check(self._lib.asora_debug_block_order(*args, None, 0, C.byref(grid)), "block_order")
        if grid.value == 0:
            return None
        out = np.zeros((grid.value, 4), dtype=np.int32)
        _capi.check(self._lib.asora_debug_block_order(*args, _capi.iptr(out), grid.value, C.byref(grid)), "block_order")
        return out

    def debug_geometry_bytes(self):
        """Device memory of the current geometry tables (shared parts once)."""
        return int(self._lib.asora_debug_geometry_bytes())

    def debug_geometry_tables(self, counts_only=False):
        """The geometry tables of the last raytrace launch: (list of (entries x 8) uint32 arrays, dict(nsteps, shells, max_cells, threads));
        counts_only: no table is copied, the list and nsteps stay empty."""
        n, ns, nt, sh, mc, th = C.c_size_t(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        _capi.check(self._lib.asora_debug_geometry_table(-1, None, 0, C.byref(n), C.byref(ns), C.byref(nt), C.byref(sh), C.byref(mc),
                                                         C.byref(th)), "debug_geometry_table")
        tables, steps = [], []
        for t in range(0 if counts_only else nt.value):
            _capi.check(self._lib.asora_debug_geometry_table(t, None, 0, C.byref(n), C.byref(ns), C.byref(nt), C.byref(sh), C.byref(mc),
                                                             C.byref(th)), "debug_geometry_table")
            a = np.zeros((n.value, 8), dtype=np.uint32)
            _capi.check(self._lib.asora_debug_geometry_table(t, a.ctypes.data_as(C.POINTER(C.c_uint32)), n.value, C.byref(n), C.byref(ns),
                                                             C.byref(nt), C.byref(sh), C.byref(mc), C.byref(th)), "debug_geometry_table")
            tables.append(a)
            steps.append(ns.value)
        return tables, {"nsteps": steps, "shells": sh.value, "max_cells": mc.value, "threads": th.value}

    def build_id(self):
        """Hash over the library's sources, headers and compiler flags (asora_build_id)."""
        return self._lib.asora_build_id().decode()

    PRIMITIVES = ("log2", "lookup", "div", "mul", "add", "absorber", "photo", "heat", "grey")
    TABLES = ("thick", "thin", "heat_thick", "heat_thin")

    def debug_rate_primitives(self, op, a, b=None, c=None, d=None, which=0, spectrum=0, sig=1.0, minlogtau=-20.0, dlogtau=1.0, NumTau=1):
        """One device function of the rates (csrc/rates_device.hpp) element-wise on float64 arrays (asora_debug_rate_primitives,
        include/asora_hip.h): `op` a name of PRIMITIVES or its number, `which` a name of TABLES or its number.  Returns the
        output array; for "lookup" the pair (value, real table index as formed)."""
        op = self.PRIMITIVES.index(op) if isinstance(op, str) else int(op)
        which = self.TABLES.index(which) if isinstance(which, str) else int(which)
        arrays = [None if x is None else np.ascontiguousarray(x, dtype=np.float64).ravel() for x in (a, b, c, d)]
        n = 0 if arrays[0] is None else arrays[0].size
        for x in arrays[1:]:
            if x is not None and x.size != n:
                raise ValueError("debug_rate_primitives: the inputs must have one length")
        out = np.empty(n)
        out2 = np.empty(n) if op == _capi.PRIM_LOOKUP else None
        _capi.check(self._lib.asora_debug_rate_primitives(op, n, *[None if x is None else _capi.dptr(x) for x in arrays], which, int(spectrum),
                                                          float(sig), float(minlogtau), float(dlogtau), int(NumTau), _capi.dptr(out),
                                                          None if out2 is None else _capi.dptr(out2)), "debug_rate_primitives")
        return (out, out2) if out2 is not None else out

    def debug_coldens(self, R, sig, dr, source_index, N):
        out = np.zeros((N, N, N))
        _capi.check(self._lib.asora_debug_coldens(float(R), float(sig), float(dr), int(source_index),
                                                  _capi.dptr(out), int(N)), "debug_coldens")
        return out


class _Chemistry:
    """Stand-in for ``libc2ray.chemistry`` (f2py wrapper of src/c2ray/chemistry.f90)."""

    def __init__(self, lib):
        self._lib = lib

    def global_pass(self, dt, ndens, temp, xh, xh_av, xh_intermed, phi_ion, bh00, albpow, colh0, temph0, abu_c):
        """conv_flag = global_pass(...); xh_av and xh_intermed are updated IN PLACE, xh is not
        modified (chemistry.f90:13-48,107-108).  The pass is elementwise, so all grids are brought to
        the storage order of xh_av; like f2py's intent(inout), xh_av and xh_intermed must be
        float64 arrays."""
        for name, a in (("xh_av", xh_av), ("xh_intermed", xh_intermed)):
            if not isinstance(a, np.ndarray) or a.dtype != np.float64:
                raise ValueError(f"{name} must be a float64 array (updated in place)")
        shape = np.shape(xh_av)
        if len(shape) != 3:
            raise ValueError("grids must be 3-dimensional")
        order = 'F' if (xh_av.flags.f_contiguous and not xh_av.flags.c_contiguous) else 'C'
        req = lambda a: np.require(np.broadcast_to(np.asarray(a, dtype=np.float64), shape), np.float64, [order])
        nd, tp, x0, ph = req(ndens), req(temp), req(xh), req(phi_ion)
        xa = np.require(xh_av, np.float64, [order, 'W'])
        xi = np.require(xh_intermed, np.float64, [order, 'W'])
        if xi is xh_intermed and np.shares_memory(xa, xi):
            xi = xi.copy(order=order)          # aliased in/out grids (hydrogenODE): keep them apart
        if np.shares_memory(x0, xa) or np.shares_memory(x0, xi):
            x0 = x0.copy(order=order)
        conv = C.c_int(0)
        _capi.check(self._lib.c2ray_global_pass(float(dt), _capi.dptr(nd), _capi.dptr(tp), _capi.dptr(x0),
                                                _capi.dptr(xa), _capi.dptr(xi), _capi.dptr(ph), float(bh00),
                                                float(albpow), float(colh0), float(temph0), float(abu_c),
                                                int(shape[0]), int(shape[1]), int(shape[2]), C.byref(conv)),
                    "global_pass")
        if xa is not xh_av:
            xh_av[...] = xa
        if xi is not xh_intermed:
            xh_intermed[...] = xi
        return conv.value


class _Raytracing:
    """Stand-in for ``libc2ray.raytracing`` (f2py wrapper of src/c2ray/raytracing.f90)."""

    def __init__(self, lib):
        self._lib = lib

    def do_all_sources(self, normflux, srcpos, max_subbox, subboxsize, coldensh_out, sig, dr, ndens, xh_av,
                       phi_ion, phi_heat, loss_fraction, photo_thin_table, photo_thick_table,
                       heat_thin_table, heat_thick_table, minlogtau, dlogtau, r_max_lls):
        """sum_nbox, photon_loss = do_all_sources(...)   (f2py signature of raytracing.f90:52-56)

        The reference's CPU raytracer -- cubic sub-boxes grown until the photon loss through the box faces is
        small, rates within r_max_lls, heating rates, column densities of the last source -- evaluated on the
        GPU (csrc/subbox.hip).  As with f2py's intent(inout), coldensh_out, phi_ion and phi_heat must be
        Fortran-contiguous float64 (N,N,N) arrays and are updated in place; ndens and xh_av are copied to
        Fortran order when needed; srcpos is (3,NumSrc), 1-based."""
        flux = np.ascontiguousarray(normflux, dtype=np.float64)
        pos = np.asfortranarray(srcpos, dtype=np.int32)
        if pos.ndim != 2 or pos.shape[0] != 3 or pos.shape[1] != flux.size:
            raise ValueError("srcpos must have shape (3, NumSrc) matching normflux")
        shape = np.shape(coldensh_out)
        if len(shape) != 3 or shape[0] != shape[1] or shape[0] != shape[2]:
            raise ValueError("grids must have shape (N,N,N)")
        for name, a in (("coldensh_out", coldensh_out), ("phi_ion", phi_ion), ("phi_heat", phi_heat)):
            if not isinstance(a, np.ndarray) or a.dtype != np.float64 or a.shape != shape or not a.flags.f_contiguous:
                raise ValueError(f"{name} must be a Fortran-contiguous float64 array of shape {shape} "
                                 "(updated in place)")
        nd = np.asfortranarray(ndens, dtype=np.float64)
        xa = np.asfortranarray(xh_av, dtype=np.float64)
        if nd.shape != shape or xa.shape != shape:
            raise ValueError("ndens and xh_av must have the shape of the output grids")
        tabs = [np.ascontiguousarray(t, dtype=np.float64) for t in
                (photo_thin_table, photo_thick_table, heat_thin_table, heat_thick_table)]
        numtau = tabs[0].size
        if any(t.size != numtau for t in tabs):
            raise ValueError("the four radiation tables must have the same length")
        nbox = C.c_int(0)
        loss = C.c_double(0.0)
        N = int(shape[0])
        _capi.check(self._lib.c2ray_do_all_sources(
            _capi.dptr(flux), _capi.iptr(pos), int(max_subbox), int(subboxsize), _capi.dptr(coldensh_out),
            float(sig), float(dr), _capi.dptr(nd), _capi.dptr(xa), _capi.dptr(phi_ion), _capi.dptr(phi_heat),
            float(loss_fraction), _capi.dptr(tabs[0]), _capi.dptr(tabs[1]), _capi.dptr(tabs[2]), _capi.dptr(tabs[3]),
            float(minlogtau), float(dlogtau), float(r_max_lls), int(numtau), int(flux.size), N, N, N,
            C.byref(nbox), C.byref(loss)), "do_all_sources")
        return nbox.value, loss.value


class _LibC2Ray:
    """Stand-in for the reference's f2py module ``libc2ray`` (sub-modules chemistry, raytracing)."""

    def __init__(self, lib):
        self.chemistry = _Chemistry(lib)
        self.raytracing = _Raytracing(lib)


_c2ray_lib = None
_asora_lib = None


def load_c2ray():
    """pyc2ray/load_extensions.py:9-29.  Raises RuntimeError when the library is missing."""
    global _c2ray_lib
    if _c2ray_lib is None:
        _c2ray_lib = _LibC2Ray(_capi.load())
    return _c2ray_lib


def load_asora():
    """pyc2ray/load_extensions.py:31-48.  Unlike the reference, a missing library is an error."""
    global _asora_lib
    if _asora_lib is None:
        _asora_lib = _LibAsora(_capi.load())
    return _asora_lib
