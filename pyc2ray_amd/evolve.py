"""One C2-Ray time step: raytrace all sources, solve the chemistry, iterate to convergence.

Same two entry points, argument lists, return values, log lines and convergence logic as the
reference (pyc2ray/evolve.py:38-245 ``evolve3D``, :249-498 ``evolve3D_MPI``).  What differs is where
the data lives: the reference re-uploads xh_av, downloads phi_ion, runs the chemistry on one CPU core
and transposes xh_av back on every iteration (evolve.py:187,200,210,240); here ndens, temp, xh, xh_av,
xh_intermed and phi_ion stay on the MI355X for the whole step, the chemistry is a HIP kernel, and
three scalars (conv_flag, sum x, sum 1-x) cross PCIe per iteration.
"""
import array
import contextlib
import dataclasses
import functools
import os
import time

import numpy as np

from . import _capi, _residency
from .asora_core import cuda_is_init
from .boundaries import open_boundaries, periodic_spec
from .budget import budget_spec
from .lls import lls_reset, lls_spec
from .planeflux import log_plane_flux, plane_flux_reset, plane_flux_spec, source_arrays
from .load_extensions import load_asora, load_c2ray
from .spectra import source_spectrum_spec
from .utils import printlog
from .utils.logutils import printlog_lines
from .utils.sourceutils import format_sources

__all__ = ['evolve3D', 'evolve3D_MPI', 'evolve3D_resident']

#: outer iterations enqueued per host round trip of the single-GPU loop (the device evaluates the convergence test
#: itself; launches enqueued beyond convergence do nothing)
EVOLVE_BATCH = int(os.environ.get("PYC2RAY_AMD_EVOLVE_BATCH", "8"))


def _has_transposed_twins(libasora):
    """The sharded / all-reduce device loops need the [k][j][i] twins of the grids (asora_evolve_begin_slab fails without:
    ASORA_OPT_Z_TRANSPOSED = 0 is a diagnostic setting)."""
    get = getattr(libasora, "get_option", None)
    return True if get is None else get(_capi.OPT_Z_TRANSPOSED) != 0


def _comm_backend(comm):
    """"nccl" / "gloo" of a pyc2ray_amd.dist.TorchComm-shaped communicator (public `backend`; older objects: `_backend()`);
    anything else exchanges through the host like gloo."""
    b = getattr(comm, "backend", None)
    if callable(b):
        b = b()
    if b is None and hasattr(comm, "_backend"):
        b = comm._backend()
    return b if isinstance(b, str) else "gloo"


def _next_batch(history, batch_max, conv_criterion, convergence_fraction):
    """How many iterations of a multi-rank device loop to enqueue before the next poll.  The launches of an iteration are gated
    by the device's `done` flag, its collectives are not: an iteration enqueued beyond convergence still exchanges its planes
    (slab path) or all-reduces the N^3 out-box (all-reduce path).  So the batch follows the distance to the test of
    evolve.py:232: `history` = the rows polled so far (conv_flag, sum1, sum0, rel1, rel0); both criteria decay roughly
    geometrically from iteration to iteration, and the batch is the number of iterations the faster of the two still needs at
    the rate of the last two rows -- at least 1, at most batch_max, and 2 while there is nothing to extrapolate from.  Every
    rank sees the same rows, hence the same batch."""
    import math
    if batch_max <= 1:
        return 1
    if len(history) < 2:
        return min(2, batch_max)

    def remaining(prev, last, target):
        if last < target:
            return 0
        if not (0.0 < last < prev):
            return batch_max
        rate = last / prev
        return max(1, int(math.ceil(math.log(max(target, 1e-300) / last) / math.log(rate))))

    (f0, _, _, r10, r00), (f1, _, _, r11, r01) = history[-2], history[-1]
    by_change = max(remaining(r10, r11, convergence_fraction), remaining(r00, r01, convergence_fraction))
    by_count = remaining(float(f0), float(f1), float(conv_criterion)) if conv_criterion > 0 else batch_max
    return max(1, min(batch_max, by_change, by_count))


def _agree_on_convergence(comm, converged):
    """Rank 0 decides, everyone follows (pyc2ray/evolve.py:484-489).  Every rank derives `converged` from the same
    summed rates, but a collective that sums in a rank-dependent order could leave them one ulp apart; a rank that
    left the loop alone would hang the others in the next collective."""
    flag = array.array('i', [int(bool(converged))])
    comm.Bcast(flag, root=0)
    return bool(flag[0])


@dataclasses.dataclass(frozen=True)
class _Step:
    """The scalars of one time step that the loops need; built once, by :func:`_prologue`."""
    dt: float
    dr: float
    R_max_LLS: float
    sig: float
    minlogtau: float
    dlogtau: float
    NumTau: int                     # evolve.py:124 (the table LENGTH is what the reference passes)
    chem: tuple                     # (dt, bh00, albpow, colh0, temph0, abu_c): the arguments of the chemistry
    convergence_fraction: float
    conv_criterion: float           # evolve.py:127
    N: int
    NumCells: int
    n_local: int                    # sources on this rank's device
    rank: int
    logfile: object
    quiet: bool

    def report(self, conv_flag, rel_change_xh1):
        """The line of evolve.py:227-228 about one outer iteration."""
        return (f"Number of non-converged points: {conv_flag} of {self.NumCells} ({conv_flag / self.NumCells * 100 : .3f} % ), "
                f"Relative change in ionfrac: {rel_change_xh1 : .2e}")


#: `ranks` of a step on one GPU: (use_mpi, comm, rank, nprocs) as evolve3D_MPI takes them
_ONE_RANK = (None, None, 0, 1)


def _is_distributed(ranks):
    use_mpi, comm, _, nprocs = ranks
    return bool(use_mpi) and comm is not None and nprocs > 1


def _contiguous_shard(src_pos, src_flux, ranks, spec=None):
    """The sources that this rank traces (evolve.py:360-371): a contiguous block of NumSrc // nprocs of the list, the last rank to
    the end; all of them when the step is not distributed.  `spec` (their spectra, or None) is cut the same way."""
    _, _, rank, nprocs = ranks
    pos, NumSrc = np.asarray(src_pos), src_flux.shape[0]
    if not _is_distributed(ranks):
        return pos, src_flux, spec
    perrank = NumSrc // nprocs
    i_start = int(rank * perrank)
    i_end = int((rank + 1) * perrank) if rank != nprocs - 1 else NumSrc
    return pos[:, i_start:i_end], src_flux[i_start:i_end], None if spec is None else spec[i_start:i_end]


def _spectra_along(reorder, *args, spec):
    """reorder(*args, src_spectrum=spec) of the communicator's two source re-orderings, which return the re-ordered spectra last
    only when given any: always with that last element, None where there are none."""
    out = tuple(reorder(*args, src_spectrum=spec))
    return out if spec is not None else out + (None,)


def _prologue(libasora, scalars, N, NumTau, src_flux, my_pos, my_flux, uploads, clump, *, ranks=_ONE_RANK,
              calling="Calling evolve3D...", xh_copies=False, say_copied=False, clump_upload=True, tables=None, spec=None,
              lls=None, faces=()):
    """What every form of the step does before its loop: the convergence criterion, this rank's sources (`my_pos`, `my_flux`)
    and the grids of `uploads` ({grid selector: host array}) to the device, the clumping mode, and the header lines of
    evolve.py:156-162 on rank 0.  Returns the :class:`_Step`.  The forms differ in: `calling`, the first header line;
    `xh_copies`, xh_av = xh_intermed = xh made here (the one-GPU device loop makes its own); `say_copied`, the line of the
    reference's one-process GPU branch; `clump_upload=False`, a clumping grid is among `uploads` or on the device already;
    `tables` = (thin, thick), use_gpu=False: that branch has no device_init of its own in the reference, so the library sets itself
    up for the mesh here; `spec`, the spectra of `my_pos` (None: all 0, nothing more is uploaded); `lls`, the LLS opacity of the
    raytrace (None: off), set like the clumping mode: after the uploads, the same on every rank; `faces`, the step's plane-parallel
    fluxes (the library's state is the caller's, plane_flux_reset): each counts as one source in the convergence criterion, so that
    a step with faces alone can still converge by the cell count."""
    NumSrc, n_local, NumCells = src_flux.shape[0], my_flux.shape[0], N * N * N
    logfile, quiet, rank = scalars["logfile"], scalars["quiet"], ranks[2]
    # evolve.py:127 (computed from the TOTAL source count, evolve.py:346)
    conv_criterion = min(int(scalars["convergence_fraction"] * NumCells), (NumSrc + len(faces) - 1) / 3)
    step = _Step(NumTau=NumTau, conv_criterion=conv_criterion, N=N, NumCells=NumCells, n_local=n_local, rank=rank, **scalars)
    if _is_distributed(ranks):
        printlog(f"...rank={rank:n} has {n_local:n} sources.", logfile, quiet)
    if tables is not None:
        libasora.device_init_auto(N)
        libasora.photo_table_to_device(*tables, NumTau)

    # Everything the step needs goes to the device once (evolve.py:136-155 keeps host copies instead)
    srcpos_flat, normflux_flat = format_sources(my_pos, my_flux)
    libasora.source_data_to_device(srcpos_flat, normflux_flat, n_local)
    if spec is not None:
        libasora.source_spectra_to_device(spec)
    for which, grid in uploads.items():
        libasora.grid_to_device(which, grid)
    if xh_copies:
        libasora.grid_copy(_capi.GRID_XH_AV, _capi.GRID_XH)          # xh_av = copy(xh)        evolve.py:136
        libasora.grid_copy(_capi.GRID_XH_INTERMED, _capi.GRID_XH)    # xh_intermed = copy(xh)  evolve.py:137
    if say_copied:
        printlog("Copied source data to device.", logfile, quiet)
    if clump is not None:
        clump.apply(libasora, upload=clump_upload)                     # (every rank uploads the whole grid, as ndens)
    if lls is not None:
        lls.apply(libasora)

    if rank == 0:
        printlog(calling, logfile, quiet)
        printlog(f"dr [Mpc]: {step.dr/3.086e24:.3e}", logfile, quiet)
        printlog(f"dt [years]: {step.dt/3.15576E+07:.3e}", logfile, quiet)
        printlog(f"Running on {NumSrc:n} source(s), total normalized ionizing flux: {src_flux.sum():.2e}", logfile, quiet)
        # the two means of evolve.py:160, summed on the device from the grids just uploaded
        mean_ndens = libasora.grid_sum(_capi.GRID_NDENS) / NumCells
        mean_xh = libasora.grid_sum(_capi.GRID_XH) / NumCells
        printlog(f"Mean density (cgs): {mean_ndens:.3e}, Mean ionized fraction: {mean_xh:.3e}", logfile, quiet)
        if clump is not None:
            clump.log(libasora, NumCells, logfile, quiet)
        if lls is not None:
            lls.log(logfile, quiet)
        log_plane_flux(faces, logfile, quiet)
        printlog(f"Convergence Criterion (Number of points): {conv_criterion : n}", logfile, quiet, end='\n\n')
    return step


def _loop_strategy(libasora, comm, distributed, faces=(), log=None):
    """Which loop runs the outer iterations of a use_gpu=True step: "one GPU", or across ranks "slab", "pipelined", "all-reduce"
    or "three calls" (what an mpi4py communicator gets).  The two device loops across ranks need the [k][j][i] twins of the
    grids (asora_evolve_begin_slab fails without: ASORA_OPT_Z_TRANSPOSED = 0 is a diagnostic setting).  With `faces` (plane-parallel
    fluxes) a communicator set up for the slab exchange runs the all-reduce loop, and `log(line)` is told: rank 0 sweeps the whole
    box, which the slab schedule's per-rank plane reach does not cover."""
    if not distributed:
        return "one GPU"
    overlap = getattr(comm, "overlap", False)
    if hasattr(comm, "slab_enqueue") and getattr(comm, "exchange", "") == "slab" and not overlap and _has_transposed_twins(libasora):
        if not faces:
            return "slab"
        if hasattr(comm, "reduce_begin") and hasattr(libasora, "evolve_slab_fold_all"):
            if log is not None:
                log("plane_flux: a face's sweep spans the whole box; this step takes the all-reduce loop instead of the slab exchange")
            return "all-reduce"
        return "three calls"
    if overlap and hasattr(comm, "raytrace_and_allreduce"):
        return "pipelined"
    if (getattr(comm, "device_loop", False) and hasattr(comm, "reduce_begin") and hasattr(libasora, "evolve_slab_fold_all")
            and _has_transposed_twins(libasora)):
        return "all-reduce"
    return "three calls"


def _device_loop(step, enqueue, poll, batch_max, label=None):
    """A loop of outer iterations that lives on the device (include/asora_hip.h, asora_evolve_*): an iteration is the raytrace
    plus ONE pass over the grids (rates folded, chemistry, nHI for the next trace, accumulators zeroed), and the convergence test of
    evolve.py:216-236 is evaluated on the device, so a batch of iterations is enqueued per host round trip and those beyond
    convergence do nothing.  `enqueue(n)` and `poll(n)` are the library's (one GPU) or the communicator's (across ranks).
    label=None, one GPU: batches of batch_max, the reference's log lines.  Across ranks `label` begins each rank's line, and as the
    collectives of an iteration are not gated by the device's `done` flag the batch shrinks as the test comes within reach
    (:func:`_next_batch`).  Returns the number of outer iterations."""
    history, converged = [], False
    while not converged:
        t0 = time.time()
        batch = batch_max if label is None else _next_batch(history, batch_max, step.conv_criterion, step.convergence_fraction)
        enqueue(batch)
        _, converged, rows = poll(batch)
        history += list(rows)
        per_iteration = (time.time() - t0) / max(len(rows), 1)
        lines = []
        for conv_flag, _s1, _s0, rel_change_xh1, _rel0 in rows:
            if label is None:
                lines += [("Doing Raytracing...", ' '), (f"took {per_iteration : .1f} s.", '\n'), ("Doing Chemistry...", ' '),
                          ("took  0.0 s. (fused with the raytrace on the device: the time above is for both)", '\n')]
            else:
                lines += [(f"{label} (rank={step.rank:n})...", ' '), (f"rank={step.rank:n} took {per_iteration : .1e} s.", '\n')]
            if label is None or step.rank == 0:
                lines.append((step.report(int(conv_flag), rel_change_xh1), '\n'))
        printlog_lines(lines, step.logfile, step.quiet)
    return len(history)


def _one_gpu_loop(libasora, step, thermal=None):
    """One GPU: the whole loop of a time step on the device, EVOLVE_BATCH iterations per host round trip; with `thermal` in the
    library's thermal mode.  NDENS, TEMP, XH and the sources must be on the device."""
    def loop():
        libasora.evolve_begin(*step.chem, step.R_max_LLS, step.sig, step.dr, step.minlogtau, step.dlogtau, step.NumTau, 0,
                              step.n_local, step.conv_criterion, step.convergence_fraction)
        return _device_loop(step, libasora.evolve_enqueue, libasora.evolve_poll, max(1, min(EVOLVE_BATCH, 32)))
    return loop() if thermal is None else _thermal_loop(libasora, thermal, loop, step)


def _thermal_loop(libasora, thermal, loop, step, stats=None):
    """Run `loop()` (a device loop of one step, on one GPU or across ranks) in the library's thermal mode, and leave the library
    isothermal again.  `stats`: where the step's substep statistics come from -- the library's own counters (one GPU), or the
    communicator's, which makes them those of the whole grid on every rank (pyc2ray_amd.dist.TorchComm.thermal_stats)."""
    thermal.apply(libasora)
    try:
        result = loop()
        capped, floored, most = (stats or libasora.thermal_stats)()
    finally:
        libasora.thermal_params(False)
    _evolve.last_thermal_stats = (capped, floored, most)
    if capped and step.rank == 0:
        printlog(f"Warning: the temperature integration of {capped:n} cell(s) hit max_substeps = {thermal.max_substeps:n} "
                 f"(most substeps used: {most:n}); their last substep took the rest of the time step.", step.logfile, step.quiet)
    return result


def _ranks_device_loop(libasora, step, comm, begin, label, thermal=None):
    """The device-resident loop across ranks (pyc2ray_amd.dist.TorchComm), begun by `begin`; with `thermal` in the library's
    thermal mode, the heating rates exchanged with the photo-ionisation rates:
    comm.slab_begin -- sharded: per iteration the trace, the rates to the owners of the planes, ONE fused pass on the own slab,
    xh_av back, and the convergence test on the device behind the in-place all-reduce of its three sums -- identical bits, hence
    the same decision, on every rank; or
    comm.reduce_begin -- trace, fold, all-reduce of the whole rate grid in place, ONE fused pass on the whole grid on every rank,
    test on the device.
    With RCCL a batch of iterations is enqueued per host round trip (launches beyond convergence do nothing); with gloo every
    exchange goes through the host anyway and the batch is one."""
    def loop():
        if thermal is not None:
            begin(step.N, step.R_max_LLS, step.sig, step.dr, step.n_local, step.minlogtau, step.dlogtau, step.NumTau, step.chem,
                  step.conv_criterion, step.convergence_fraction, thermal=True)
        else:
            begin(step.N, step.R_max_LLS, step.sig, step.dr, step.n_local, step.minlogtau, step.dlogtau, step.NumTau, step.chem,
                  step.conv_criterion, step.convergence_fraction)
        batch_max = max(1, min(EVOLVE_BATCH, 32)) if _comm_backend(comm) == "nccl" else 1
        return _device_loop(step, functools.partial(comm.slab_enqueue, libasora), functools.partial(comm.slab_poll, libasora),
                            batch_max, label)
    if thermal is None:
        return loop()
    return _thermal_loop(libasora, thermal, loop, step, functools.partial(comm.thermal_stats, libasora))


def _host_test_loop(step, iteration, comm=None):
    """Outer iterations with the global convergence test of evolve.py:216-236 on the host: `iteration()` traces, sums over the
    ranks, solves the chemistry and returns (conv_flag, sum x, sum 1-x).  With `comm` (a distributed step) the ranks agree on the
    outcome.  Returns the number of outer iterations."""
    prev_sum_xh1_int = prev_sum_xh0_int = 2 * step.NumCells
    niter, converged = 0, False
    while not converged:
        niter += 1
        conv_flag, sum_xh1_int, sum_xh0_int = iteration()
        rel_change_xh1 = np.abs((sum_xh1_int - prev_sum_xh1_int) / sum_xh1_int) if sum_xh1_int > 0.0 else 1.0
        rel_change_xh0 = np.abs((sum_xh0_int - prev_sum_xh0_int) / sum_xh0_int) if sum_xh0_int > 0.0 else 1.0
        if step.rank == 0:
            printlog(step.report(conv_flag, rel_change_xh1), step.logfile, step.quiet)
        converged = (conv_flag < step.conv_criterion) or ((rel_change_xh1 < step.convergence_fraction) and
                                                          (rel_change_xh0 < step.convergence_fraction))
        if comm is not None:
            converged = _agree_on_convergence(comm, converged)            # evolve.py:484-489
        prev_sum_xh1_int, prev_sum_xh0_int = sum_xh1_int, sum_xh0_int
    return niter


def _chemistry(libasora, step):
    """One global pass of the chemistry on the device (evolve.py:207-211), timed in the log of rank 0."""
    tch0 = time.time()
    if step.rank == 0:
        printlog("Doing Chemistry...", step.logfile, step.quiet, ' ')
    sums = libasora.chemistry_device(*step.chem)
    if step.rank == 0:
        printlog(f"took {(time.time()-tch0) : .1f} s.", step.logfile, step.quiet)
    return sums


def _three_call_loop(libasora, step, use_mpi, comm):
    """Across ranks as the reference does it (evolve.py:401-498): raytrace, sum of the rate grids, chemistry, and three scalars
    read back, per iteration.  Every rank runs the chemistry on the identical summed rates (the reference runs it on rank 0 and
    broadcasts two N^3 grids, evolve.py:439-481)."""
    def iteration():
        trt0 = time.time()
        printlog(f"Doing Raytracing (rank={step.rank:n})...", step.logfile, step.quiet, ' ')
        libasora.raytrace_device(step.R_max_LLS, step.sig, step.dr, 0, step.n_local, step.minlogtau, step.dlogtau, step.NumTau)
        libasora.synchronize()
        printlog(f"rank={step.rank:n} took {(time.time()-trt0) : .1e} s.", step.logfile, step.quiet)
        _allreduce_phi(libasora, step.N, use_mpi, comm, step.rank)
        return _chemistry(libasora, step)
    return _host_test_loop(step, iteration, comm)


def _pipelined_loop(libasora, step, comm, src_i0):
    """Raytrace, sum over ranks and chemistry slab by slab (pyc2ray_amd.dist, opt-in); `src_i0`: the first coordinates of the
    rank's sources, which are traced in that order."""
    def iteration():
        trt0 = time.time()
        printlog(f"Doing Raytracing and Chemistry, pipelined (rank={step.rank:n})...", step.logfile, step.quiet, ' ')
        sums = comm.raytrace_and_allreduce(libasora, step.N, step.R_max_LLS, step.sig, step.dr, step.n_local, step.minlogtau,
                                           step.dlogtau, step.NumTau, src_i0=src_i0, chemistry=step.chem)
        printlog(f"rank={step.rank:n} took {(time.time()-trt0) : .1e} s.", step.logfile, step.quiet)
        return sums
    return _host_test_loop(step, iteration, comm)


def _subbox_loop(libasora, step, subbox, ranks):
    """use_gpu=False (evolve.py:168-245, :401-498): per iteration one pass of the CPU library's raytracer -- cubic sub-boxes
    grown until the photon loss is below loss_fraction, photon-loss statistics, Fortran-flavoured constants, every source rated with
    the flux of the last one as the Fortran does -- and one global pass, both evaluated on the GPU."""
    use_mpi, comm, _, _ = ranks
    distributed = _is_distributed(ranks)

    def iteration():
        trt0 = time.time()
        printlog("Doing Raytracing...", step.logfile, step.quiet, ' ')
        nsubbox, photonloss = libasora.subbox_raytrace_device(*subbox, step.R_max_LLS, step.sig, step.dr, step.minlogtau,
                                                              step.dlogtau, step.NumTau, 0, step.n_local)
        printlog(f"took {(time.time()-trt0) : .1f} s.", step.logfile, step.quiet)
        printlog(f"Average number of subboxes: {nsubbox/max(step.n_local, 1):n}, Total photon loss: {photonloss:.3e}",
                 step.logfile, step.quiet)
        if distributed:                                                                 # evolve.py:433-437
            _allreduce_phi(libasora, step.N, use_mpi, comm, step.rank)
        return _chemistry(libasora, step)
    return _host_test_loop(step, iteration, comm if distributed else None)


def _allreduce_phi(libasora, N, use_mpi, comm, rank):
    """Sum the per-rank photo-ionisation rate grids (evolve.py:433-437: Reduce to root + Bcast)."""
    if hasattr(comm, "allreduce_device_grid"):
        # pyc2ray_amd.dist.TorchComm: RCCL all-reduce on the device-resident grid (or gloo via host)
        comm.allreduce_device_grid(libasora, _capi.GRID_PHI_ION, N)
        return
    # mpi4py communicator, host-staged like the reference
    phi = libasora.grid_to_host(_capi.GRID_PHI_ION, np.empty((N, N, N)))
    if rank == 0:
        comm.Reduce(use_mpi.IN_PLACE, [phi, use_mpi.DOUBLE], op=use_mpi.SUM, root=0)
    else:
        comm.Reduce([phi, use_mpi.DOUBLE], None, op=use_mpi.SUM, root=0)
    comm.Bcast([phi, use_mpi.DOUBLE], root=0)
    libasora.grid_to_device(_capi.GRID_PHI_ION, phi)


def _take_budget(libasora, budget, step, src_flux, faces, thermal, planes=None, comm=None):
    """Fill `budget` (a pyc2ray_amd.budget.StepBudget) from the device grids of the step whose loop has just ended: XH still holds
    the step's starting state, XH_INTERMED / XH_AV / PHI_ION its results.  One call of the library over `planes` = (i_begin,
    i_count), None: every plane.  `comm`: the planes are this rank's share of the grid (the slab loop), and the twelve sums are
    added over the ranks on the host -- one small collective that every rank must reach."""
    sums = libasora.step_budget(step.chem, use_temp_end=thermal is not None, planes=planes)
    if comm is not None:
        total = np.zeros_like(sums)
        comm.Allreduce(sums, total)
        sums = total
    budget.fill(sums, step.dt, step.dr, step.N, src_flux, faces)


class _Clumping:
    """A validated ``clumping=`` argument: ``constant`` (a float != 1) or ``grid`` (an (N, N, N)
    float64 array), the sub-grid clumping factor C = <n^2>/<n>^2 of the case-B recombination rate."""

    def __init__(self, constant=None, grid=None):
        self.constant, self.grid = constant, grid

    def apply(self, libasora, upload=True):
        """Set the library's mode; upload=False: GRID_CLUMP already holds the grid."""
        if self.grid is None:
            libasora.clumping(1, self.constant)
            return
        if upload:
            libasora.grid_to_device(_capi.GRID_CLUMP, self.grid)
        libasora.clumping(2)

    def log(self, libasora, NumCells, logfile, quiet):
        if self.grid is None:
            printlog(f"Clumping factor: constant {self.constant:.3e}", logfile, quiet)
        else:
            printlog(f"Clumping factor: grid, mean {libasora.grid_sum(_capi.GRID_CLUMP) / NumCells:.3e}", logfile, quiet)


def _clumping_spec(clumping, N, check_values=True):
    """``clumping=`` of evolve3D / evolve3D_MPI / evolve3D_resident -> None (off: None or 1.0) or a _Clumping.  Raises
    ValueError -- before any GPU work -- for anything but a finite float > 0 or an (N, N, N) grid of such values
    (check_values=False: the grid's shape only, for a grid the caller has already checked)."""
    if clumping is None:
        return None
    if isinstance(clumping, np.ndarray) and clumping.ndim == 3:
        if clumping.shape != (N, N, N):
            raise ValueError(f"clumping: a grid must have the mesh's shape {(N, N, N)}, not {clumping.shape}")
        if clumping.dtype != np.float64:
            raise ValueError(f"clumping: a grid must be float64, not {clumping.dtype}")
        if check_values and not (np.all(np.isfinite(clumping)) and np.all(clumping > 0.0)):
            raise ValueError("clumping: every factor of the grid must be finite and > 0")
        return _Clumping(grid=clumping)
    if isinstance(clumping, np.ndarray) and clumping.ndim == 0:
        clumping = clumping.item()
    if isinstance(clumping, (bool, np.bool_)) or not isinstance(clumping, (int, float, np.integer, np.floating)):
        raise ValueError(f"clumping: None, a float > 0 or an (N, N, N) float64 grid, not {type(clumping).__name__}")
    c = float(clumping)
    if not (np.isfinite(c) and c > 0.0):
        raise ValueError(f"clumping: the factor must be finite and > 0, not {c!r}")
    return None if c == 1.0 else _Clumping(constant=c)


@contextlib.contextmanager
def _clumping_reset(clump):
    """Leave the library unclumped after the block, whatever happens (nothing at all when clumping is off)."""
    try:
        yield
    finally:
        if clump is not None:
            load_asora().clumping(0)


def _scalars(dt, dr, R_max_LLS, convergence_fraction, sig, minlogtau, dlogtau, chem_constants, logfile, quiet):
    """The arguments of an entry form that go into the :class:`_Step` as they are; chem_constants = (bh00, albpow, colh0, temph0,
    abu_c)."""
    return dict(dt=dt, dr=dr, R_max_LLS=R_max_LLS, convergence_fraction=convergence_fraction, sig=sig, minlogtau=minlogtau,
                dlogtau=dlogtau, chem=(dt, *chem_constants), logfile=logfile, quiet=quiet)


def evolve3D_resident(dt, dr, src_flux, src_pos, uploads, N, photo_thin_table, minlogtau, dlogtau, R_max_LLS,
                      convergence_fraction, sig, bh00, albpow, colh0, temph0, abu_c, logfile="pyC2Ray.log", quiet=False,
                      thermal=None, clumping=None, src_spectrum=None, lls=None, periodic=True, plane_flux=None, budget=None):
    """evolve3D for a caller that keeps the grids on the device between time steps (the C2Ray class with
    ``device_resident = True``): same loop, log lines and results as :func:`evolve3D` with ``use_gpu=True``, but only the
    grids in ``uploads`` ({grid selector: host array}, those the caller changed on the host) cross PCIe, and nothing
    comes back: afterwards XH_INTERMED == XH == the new ionised fraction and PHI_ION the rates, on the device
    (``libasora.grid_to_host`` fetches them when someone looks).  Returns the number of outer iterations.
    With ``thermal`` (a :class:`pyc2ray_amd.thermal.ThermalParams`) the temperature is evolved as well: TEMP holds the
    end-of-step temperature afterwards, PHI_HEAT the heating rates.
    ``clumping`` as in :func:`evolve3D`; like the other grids, an (N, N, N) grid crosses PCIe only when ``uploads`` holds it
    (under ``_capi.GRID_CLUMP``, checked then): otherwise GRID_CLUMP must still hold it from an earlier step.
    ``src_spectrum``, ``lls``, ``periodic``, ``plane_flux`` and ``budget`` as in :func:`evolve3D`."""
    budget = budget_spec(budget, "evolve3D_resident")
    periodic = periodic_spec(periodic, "evolve3D_resident")
    lls = lls_spec(lls, "evolve3D_resident")
    faces = plane_flux_spec(plane_flux, "evolve3D_resident", True, lambda: load_asora().num_spectra())
    src_flux, src_pos = source_arrays(src_flux, src_pos, faces)
    spec = source_spectrum_spec(src_spectrum, src_flux.shape[0], True, lambda: load_asora().num_spectra(), "evolve3D_resident")
    clump = _clumping_spec(clumping, N, check_values=_capi.GRID_CLUMP in uploads)
    if clump is not None and clump.grid is not None and _capi.GRID_CLUMP in uploads and uploads[_capi.GRID_CLUMP] is not clumping:
        raise ValueError("evolve3D_resident: uploads[GRID_CLUMP] and clumping must be the same grid")
    if not cuda_is_init():
        raise RuntimeError("GPU not initialized. Please initialize it by calling device_init(N)")
    scalars = _scalars(dt, dr, R_max_LLS, convergence_fraction, sig, minlogtau, dlogtau, (bh00, albpow, colh0, temph0, abu_c),
                       logfile, quiet)
    with _clumping_reset(clump), lls_reset(lls, load_asora), open_boundaries(periodic, load_asora), plane_flux_reset(faces, load_asora):
        return _evolve_resident(scalars, src_flux, src_pos, uploads, N, photo_thin_table, thermal, clump, spec, lls, faces, budget)


def _evolve_resident(scalars, src_flux, src_pos, uploads, N, photo_thin_table, thermal, clump, spec=None, lls=None, faces=(),
                     budget=None):
    libasora = load_asora()
    step = _prologue(libasora, scalars, N, photo_thin_table.shape[0], src_flux, np.asarray(src_pos), src_flux, uploads, clump,
                     say_copied=True, clump_upload=False, spec=spec, lls=lls, faces=faces)
    niter = _one_gpu_loop(libasora, step, thermal)
    printlog("Multiple source convergence reached.", step.logfile, step.quiet)
    if budget is not None:
        _take_budget(libasora, budget, step, src_flux, faces, thermal)
    libasora.grid_copy(_capi.GRID_XH, _capi.GRID_XH_INTERMED)       # the next step starts from the new ionised fraction
    if thermal is not None:
        libasora.grid_copy(_capi.GRID_TEMP, _capi.GRID_TEMP_END)    # ... and from the new temperature
    _evolve.last_niter = niter
    return niter


def _thermal_ranks_refusal(comm):
    """Why a thermal step cannot run across ranks with this communicator, or None when it can.  The heating rates travel with the
    photo-ionisation rates on the two device loops of a pyc2ray_amd.dist.TorchComm only; decided from the communicator alone,
    before any GPU work."""
    if comm is None or not (hasattr(comm, "slab_enqueue") and hasattr(comm, "reduce_begin") and hasattr(comm, "thermal_stats")):
        return "it needs a pyc2ray_amd.dist.TorchComm, which exchanges the heating rates with the photo-ionisation rates"
    if getattr(comm, "overlap", False):
        return "the pipelined loop (overlap=True) is isothermal"
    if getattr(comm, "exchange", "") != "slab" and not getattr(comm, "device_loop", False):
        return "the three-call loop (device_loop=False) is isothermal"
    return None


def _evolve(scalars, src_flux, src_pos, grids, photo_thin_table, ranks=_ONE_RANK, thermal=None, clump=None, spec=None, lls=None,
            faces=(), budget=None):
    """A use_gpu=True step on host arrays, grids = (temp, ndens, xh), on one GPU or across `ranks`; `thermal` on one GPU, or
    across ranks on the "slab" and "all-reduce" device loops; `spec`, the spectrum of each source of the whole list (None: all 0),
    which follows its source through every re-ordering and sharding below."""
    if not cuda_is_init():
        raise RuntimeError("GPU not initialized. Please initialize it by calling device_init(N)")
    _residency.reclaim()              # this step overwrites device grids a resident C2Ray object may be relying on
    use_mpi, comm, rank, nprocs = ranks
    distributed = _is_distributed(ranks)
    libasora = load_asora()
    temp, ndens, xh = grids
    N = temp.shape[0]                   # mesh size
    strategy = _loop_strategy(libasora, comm, distributed, faces,
                              (lambda line: printlog(line, scalars["logfile"], scalars["quiet"])) if rank == 0 else None)
    if thermal is not None and strategy not in ("one GPU", "slab", "all-reduce"):
        raise ValueError(f"evolve3D_MPI: the thermal mode across ranks runs on the slab and all-reduce device loops; this step would "
                         f"take the {strategy} loop (the [k][j][i] twins are off?), where it is single-GPU only")

    # source shard of this rank, evolve.py:360-371
    plan = src_i0 = None
    if strategy == "slab":
        # the same contiguous blocks, of the list ordered by the first coordinate: a rank's rates then live on the
        # planes within R of its slab of sources, and only those planes are exchanged (pyc2ray_amd.dist.SlabPlan)
        from .dist import SlabPlan
        all_pos, all_flux, bounds, all_spec = _spectra_along(comm.shard_sources_by_slab, np.asarray(src_pos), src_flux, nprocs, spec=spec)
        my_pos, my_flux = all_pos[:, bounds[rank]:bounds[rank + 1]], all_flux[bounds[rank]:bounds[rank + 1]]
        my_spec = None if all_spec is None else all_spec[bounds[rank]:bounds[rank + 1]]
        plan = SlabPlan(N, nprocs, scalars["R_max_LLS"], [all_pos[0, bounds[r]:bounds[r + 1]] - 1 for r in range(nprocs)])
    else:
        my_pos, my_flux, my_spec = _contiguous_shard(src_pos, src_flux, ranks, spec)
    if strategy == "pipelined":         # the shard is traced in order of the first coordinate
        my_pos, my_flux, my_spec = _spectra_along(comm.sort_sources_for_overlap, my_pos, my_flux, spec=my_spec)
        src_i0 = np.asarray(my_pos[0]).astype(np.int64) - 1

    step = _prologue(libasora, scalars, N, photo_thin_table.shape[0], src_flux, my_pos, my_flux,
                     {_capi.GRID_NDENS: ndens, _capi.GRID_TEMP: temp, _capi.GRID_XH: xh}, clump, ranks=ranks,
                     calling=f"Calling evolve3D with {nprocs:n} MPI-processors..." if distributed else "Calling evolve3D...",
                     xh_copies=distributed, say_copied=not distributed, spec=my_spec, lls=lls, faces=faces)
    if strategy == "one GPU":
        niter = _one_gpu_loop(libasora, step, thermal)
    elif strategy == "slab":
        niter = _ranks_device_loop(libasora, step, comm, functools.partial(comm.slab_begin, libasora, plan),
                                   "Doing Raytracing and Chemistry, slab-wise", thermal)
    elif strategy == "all-reduce":
        niter = _ranks_device_loop(libasora, step, comm, functools.partial(comm.reduce_begin, libasora),
                                   "Doing Raytracing, all-reduce and Chemistry", thermal)
    elif strategy == "pipelined":
        niter = _pipelined_loop(libasora, step, comm, src_i0)
    else:
        niter = _three_call_loop(libasora, step, use_mpi, comm)

    if rank == 0:
        printlog("Multiple source convergence reached.", step.logfile, step.quiet)
    if budget is not None:
        # the slab loop: a rank's results are complete on the planes whose chemistry it ran, and the ranks add their sums up; on
        # every other loop each rank holds the whole grids and reduces them itself
        if strategy == "slab":
            a, b = plan.own[rank]
            _take_budget(libasora, budget, step, src_flux, faces, thermal, (a, b - a), comm)
        else:
            _take_budget(libasora, budget, step, src_flux, faces, thermal)
    if strategy == "slab":       # every rank returns the whole fields (evolve.py:480-481,497): collect the owners' slabs
        comm.slab_gather(libasora, plan, _capi.GRID_XH_INTERMED, N)
        comm.slab_gather(libasora, plan, _capi.GRID_PHI_ION, N)
        if thermal is not None:      # TEMP_END travels once, here; between iterations no temperature does
            comm.slab_gather(libasora, plan, _capi.GRID_TEMP_END, N)
            comm.slab_gather(libasora, plan, _capi.GRID_PHI_HEAT, N)
    # laid out like `xh`, as np.empty_like would; in page-locked memory (pyc2ray_amd/_pinned.py)
    like_xh = 'F' if (xh.flags.f_contiguous and not xh.flags.c_contiguous) else 'C'
    xh_new = libasora.grid_to_host(_capi.GRID_XH_INTERMED, libasora.host_empty((N, N, N), order=like_xh))
    phi_ion = libasora.grid_to_host(_capi.GRID_PHI_ION, libasora.host_empty((N, N, N)))
    _evolve.last_niter = niter
    if thermal is not None:
        temp_new = libasora.grid_to_host(_capi.GRID_TEMP_END, libasora.host_empty((N, N, N), order=like_xh))
        return xh_new, phi_ion, temp_new
    return xh_new, phi_ion


def _evolve_cpu_semantics(scalars, src_flux, src_pos, grids, tables, subbox, ranks=_ONE_RANK, clump=None, lls=None):
    """The use_gpu=False branch of the reference on host arrays: the loop of :func:`_subbox_loop`, subbox = (max_subbox,
    subboxsize, loss_fraction).  Like the use_gpu=True loop this one keeps the grids on the device for the whole step (the
    reference's host round trips are what ``libc2ray.raytracing.do_all_sources`` / ``libc2ray.chemistry.global_pass`` of this
    package still offer)."""
    _residency.reclaim()              # this step overwrites device grids a resident C2Ray object may be relying on
    libasora = load_asora()
    temp, ndens, xh = grids
    N = temp.shape[0]
    my_pos, my_flux, _ = _contiguous_shard(src_pos, src_flux, ranks)
    step = _prologue(libasora, scalars, N, tables[0].shape[0], src_flux, my_pos, my_flux,
                     {_capi.GRID_NDENS: ndens, _capi.GRID_TEMP: temp, _capi.GRID_XH: xh}, clump,
                     ranks=ranks, xh_copies=True, tables=tables, lls=lls)
    niter = _subbox_loop(libasora, step, subbox, ranks)
    if step.rank == 0:
        printlog("Multiple source convergence reached.", step.logfile, step.quiet)
    # Fortran-ordered results, as the reference's CPU branch returns them (evolve.py:178)
    xh_new = libasora.grid_to_host(_capi.GRID_XH_INTERMED, libasora.host_empty((N, N, N), order='F'))
    phi_ion = libasora.grid_to_host(_capi.GRID_PHI_ION, libasora.host_empty((N, N, N), order='F'))
    _evolve.last_niter = niter
    return xh_new, phi_ion


def evolve3D(dt, dr,
             src_flux, src_pos,
             use_gpu, max_subbox, subboxsize, loss_fraction,
             temp, ndens, xh,
             photo_thin_table, photo_thick_table,
             minlogtau, dlogtau,
             R_max_LLS, convergence_fraction,
             sig, bh00, albpow, colh0, temph0, abu_c,
             logfile="pyC2Ray.log", quiet=False, *, thermal=None, clumping=None, src_spectrum=None, lls=None, periodic=True,
             plane_flux=None, budget=None):
    """Evolve the ionised fraction of the whole grid over one time step.

    Parameters have the reference's meaning (pyc2ray/evolve.py:49-109): dt [s], dr [cm],
    src_flux (numsrc) in units of 1e48 s^-1, src_pos (3,numsrc) 1-based, temp/ndens/xh (N,N,N),
    tables as copied to the GPU beforehand with photo_table_to_device(), R_max_LLS in cells.
    max_subbox, subboxsize and loss_fraction only concern the reference's CPU raytracer and have no
    effect with use_gpu=True.  use_gpu=False selects that raytracer's semantics (cubic sub-boxes grown until
    the photon loss is below loss_fraction, evolve.py:190-194) -- still evaluated on the GPU, through the
    libc2ray-compatible entry points, with host arrays as in the reference.

    Returns (xh_new, phi_ion): end-of-step ionised fraction (laid out like `xh`) and the summed
    photo-ionisation rate (C-ordered with use_gpu=True, Fortran-ordered with use_gpu=False, as in the
    reference, evolve.py:178,200,244-245).

    thermal : None (isothermal, as the reference) or a :class:`pyc2ray_amd.thermal.ThermalParams`: the temperature is
    evolved from photo-heating and radiative cooling as well (use_gpu=True only; the photo tables must be on the device, the
    heating tables are uploaded here).  Returns (xh_new, phi_ion, temp_new) then, temp_new laid out like `xh`.

    clumping : the sub-grid clumping factor C = <n^2>/<n>^2 of the case-B recombination rate: None or
    1.0 (off, the reference's behaviour), a float > 0 for the whole grid, or an (N, N, N) float64 grid (C or Fortran order) of
    factors > 0.  Anything else raises ValueError before any GPU work.  Works with use_gpu=False and with `thermal` (then the
    recombination cooling is clumped as well).

    src_spectrum : which of the table sets on the device (``spectra_to_device``) each source shines with:
    None or all zeros (the reference's one spectrum: nothing more is uploaded), or an integer array of length numsrc with values
    in [0, num_spectra()).  Anything else, or a non-zero entry with use_gpu=False, raises ValueError before any GPU work.  With
    `thermal` the heating tables of every set must have gone up with ``spectra_to_device``.

    lls : None (off) or a :class:`pyc2ray_amd.lls.LLSOpacity`: unresolved Lyman-limit systems as a distributed photon sink of the
    raytrace.  The absorber density of the raytrace becomes ndens ((1 - xh_av) + per_density) + n_const;
    the chemistry is unchanged.  Anything else, a negative or a non-finite value raises ValueError before any GPU work.  Works with
    use_gpu=False, `thermal`, `clumping` and `src_spectrum`.

    periodic : True (default, the reference's ``-D PERIODIC`` build: every trace wraps around the box) or False: open boundaries
     -- a cell whose unwrapped position lies beyond a face of the box receives nothing from that source.
    The reach stays the periodic window's, N/2 cells per axis.  Set in the library for this call only (True leaves the
    library's own option alone).  Anything but a bool, or False with use_gpu=False (the sub-box sweep has no such mode), raises
    ValueError before any GPU work; the library refuses meshes beyond 512.  Works with `thermal`, `clumping`, `src_spectrum` and
    `lls`.

    plane_flux : None or an empty sequence (off), a :class:`pyc2ray_amd.planeflux.PlaneFlux` or a sequence of them, one per face at
    most: a plane-parallel photon flux that enters the box through that face, swept along the axis over
    all N cells -- never wrapping, whatever `periodic` says, and not cut at R_max_LLS.  The flux is in the units of src_flux per
    cm^2 (1e48 photons s^-1 cm^-2).  With faces, src_flux / src_pos may be empty, and each face counts as one source in the
    convergence criterion.  Anything else, a face given twice, or faces with use_gpu=False raises ValueError before any GPU work.
    Works with `thermal`, `clumping`, `src_spectrum`, `lls` and `periodic`.

    budget : None, or a :class:`pyc2ray_amd.budget.StepBudget` that is filled in place with the photon budget and the mean ionised
    fractions of the step: twelve sums reduced on the device once the loop has ended, one call and one
    synchronisation per time step; the return values are what they are without it.  Anything else, or a budget with
    use_gpu=False, raises ValueError before any GPU work.  Works with every keyword above.
    """
    budget = budget_spec(budget, "evolve3D", use_gpu)
    periodic = periodic_spec(periodic, "evolve3D", use_gpu)
    lls = lls_spec(lls, "evolve3D")
    faces = plane_flux_spec(plane_flux, "evolve3D", use_gpu, lambda: load_asora().num_spectra())
    src_flux, src_pos = source_arrays(src_flux, src_pos, faces)
    spec = source_spectrum_spec(src_spectrum, src_flux.shape[0], use_gpu, lambda: load_asora().num_spectra(), "evolve3D")
    clump = _clumping_spec(clumping, np.shape(temp)[0])
    if not use_gpu and thermal is not None:
        raise ValueError("evolve3D: the thermal mode needs use_gpu=True (the use_gpu=False raytracer has no thermal form)")
    scalars = _scalars(dt, dr, R_max_LLS, convergence_fraction, sig, minlogtau, dlogtau, (bh00, albpow, colh0, temph0, abu_c),
                       logfile, quiet)
    with _clumping_reset(clump), lls_reset(lls, load_asora), open_boundaries(periodic, load_asora), plane_flux_reset(faces, load_asora):
        if use_gpu:
            return _evolve(scalars, src_flux, src_pos, (temp, ndens, xh), photo_thin_table, thermal=thermal, clump=clump, spec=spec,
                           lls=lls, faces=faces, budget=budget)
        return _evolve_cpu_semantics(scalars, src_flux, src_pos, (temp, ndens, xh), (photo_thin_table, photo_thick_table),
                                     (max_subbox, subboxsize, loss_fraction), clump=clump, lls=lls)


def evolve3D_MPI(dt, dr,
                 src_flux, src_pos,
                 use_gpu, max_subbox, subboxsize, loss_fraction,
                 use_mpi, comm, rank, nprocs,
                 temp, ndens, xh,
                 photo_thin_table, photo_thick_table,
                 minlogtau, dlogtau,
                 R_max_LLS, convergence_fraction,
                 sig, bh00, albpow, colh0, temph0, abu_c,
                 logfile="pyC2Ray.log", quiet=False, *, thermal=None, clumping=None, src_spectrum=None, lls=None, periodic=True,
                 plane_flux=None, budget=None):
    """Source-sharded variant (pyc2ray/evolve.py:249-498): rank r traces the contiguous block
    [r*(Ns//nprocs), (r+1)*(Ns//nprocs)) of the source list, the last rank to the end
    (evolve.py:362-367); the per-rank rate grids are summed across ranks each iteration.

    `use_mpi`/`comm` may be mpi4py's ``MPI`` module and a communicator, exactly as the reference takes
    them (host-staged Reduce+Bcast), or ``pyc2ray_amd.dist.MPI`` and a ``pyc2ray_amd.dist.TorchComm``
    (one process per GPU under torch.distributed: RCCL all-reduce over xGMI directly on the
    device-resident grid).  All ranks return the same (xh_new, phi_ion).

    ``thermal`` (a :class:`pyc2ray_amd.thermal.ThermalParams`, as in :func:`evolve3D`): with a ``TorchComm`` on one of its two
    device loops -- the slab exchange or the full-grid all-reduce (``exchange``; not ``overlap=True``, not
    ``device_loop=False``) -- the temperature is evolved as well.  The heating rates travel with the photo-ionisation rates
    (slab exchange: the same planes, in the same round; all-reduce: a second grid), temperatures do not travel between
    iterations, and every rank returns identical (xh_new, phi_ion, temp_new); PHI_HEAT on the device holds the summed heating
    rates.  With any other communicator (None, mpi4py) the thermal mode is single-GPU only and a ValueError says so before any GPU
    work; use_gpu=False has no thermal form.
    ``clumping`` as in :func:`evolve3D`; every rank passes (and uploads) the whole grid, as it does ``ndens``.
    ``src_spectrum`` as in :func:`evolve3D`, for the whole source list; a rank's shard of the sources takes its shard of it.
    ``lls`` as in :func:`evolve3D`; every rank passes the same one and sets the same state, on every loop.
    ``periodic`` as in :func:`evolve3D`, the same on every rank and on every loop; the planes the ranks exchange stay those of the
    periodic trace (the wrapped ones then carry zeros).
    ``plane_flux`` as in :func:`evolve3D`, the same on every rank.  The faces belong to rank 0: only its library holds them, and
    its sweep needs nHI of the whole box -- which the all-reduce device loop, the pipelined loop and the three-call loop have on
    every rank.  A ``TorchComm`` set up for the slab exchange runs the all-reduce loop for such a step (one log line says so).
    ``budget`` as in :func:`evolve3D`, on every rank or on none: every rank's is filled with the budget of the whole grid.  On the
    slab loop a rank reduces the planes whose chemistry it ran and the twelve sums are added over the ranks (one small collective
    after the loop); on every other loop each rank holds whole grids and reduces them itself.
    """
    budget = budget_spec(budget, "evolve3D_MPI", use_gpu)
    periodic = periodic_spec(periodic, "evolve3D_MPI", use_gpu)
    lls = lls_spec(lls, "evolve3D_MPI")
    faces = plane_flux_spec(plane_flux, "evolve3D_MPI", use_gpu, lambda: load_asora().num_spectra())
    src_flux, src_pos = source_arrays(src_flux, src_pos, faces)
    spec = source_spectrum_spec(src_spectrum, src_flux.shape[0], use_gpu, lambda: load_asora().num_spectra(), "evolve3D_MPI")
    if thermal is not None:
        if not use_gpu:
            raise ValueError("evolve3D_MPI: the thermal mode needs use_gpu=True (the use_gpu=False raytracer has no thermal form)")
        refusal = _thermal_ranks_refusal(comm)
        if refusal is not None:
            raise ValueError(f"evolve3D_MPI: with this communicator the thermal mode is single-GPU only ({refusal}); use evolve3D "
                             "with use_gpu=True, or a TorchComm on the slab or all-reduce device loop")
    clump = _clumping_spec(clumping, np.shape(temp)[0])
    scalars = _scalars(dt, dr, R_max_LLS, convergence_fraction, sig, minlogtau, dlogtau, (bh00, albpow, colh0, temph0, abu_c),
                       logfile, quiet)
    ranks = (use_mpi, comm, rank, nprocs)
    with _clumping_reset(clump), lls_reset(lls, load_asora), open_boundaries(periodic, load_asora), \
            plane_flux_reset(faces if rank == 0 else (), load_asora):
        if use_gpu:
            return _evolve(scalars, src_flux, src_pos, (temp, ndens, xh), photo_thin_table, ranks, thermal=thermal, clump=clump,
                           spec=spec, lls=lls, faces=faces, budget=budget)
        return _evolve_cpu_semantics(scalars, src_flux, src_pos, (temp, ndens, xh), (photo_thin_table, photo_thick_table),
                                     (max_subbox, subboxsize, loss_fraction), ranks, clump=clump, lls=lls)
