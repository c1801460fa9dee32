/*
 * asora_hip.h -- C-ABI of libasora_hip.so, the MI355X (gfx950) implementation of pyc2ray's
 * raytracing + chemistry hot path.
 *
 * Every entry point is `extern "C"`, takes plain pointers / sizes, and returns 0 on success or
 * a non-zero error code; asora_last_error() then holds a message.  Nothing throws across the
 * boundary (the reference throws std::runtime_error through the CPython C-API uncaught,
 * src/asora/memory.cu:72, src/asora/raytracing.cu:136).
 *
 * Section A is the drop-in boundary: one function per method of the reference's two extension
 * modules, with the reference binding each replaces cited (paths relative to the reference
 * checkout).  Section B is the device-resident extension the fused evolve loop uses (no
 * per-iteration PCIe copies).  Section C holds measurement/diagnostic hooks.
 *
 * Host buffers are owned by the caller and only read/written during the call.  Device memory
 * is process-global library state between asora_device_init and asora_device_close
 * (as in src/asora/memory.cu:20-29).  Not re-entrant, one grid size per process, one GPU per
 * process (asora_device_init_ex selects it).
 *
 * Grid element order: C-order logical [i][j][k], flat index N*N*i + N*j + k
 * (src/asora/raytracing.cu:30).  Sources: int32 0-based, xyz-interleaved
 * [x0,y0,z0,x1,...] (pyc2ray/utils/sourceutils.py:30); flux in units of 1e48 photons/s.
 */
#ifndef ASORA_HIP_H
#define ASORA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------ */
/* A. Drop-in boundary                                                                        */
/* ------------------------------------------------------------------------------------------ */

/* libasora.device_init(N, num_src_par)            src/asora/python_module.cu:73-82 -> memory.cu:34-80.
 * num_src_par is accepted for signature compatibility; this build keeps the per-source
 * column-density scratch in LDS, so no num_src_par*N^3 slab is allocated. */
int asora_device_init(int N, int num_src_par);
/* Same, on an explicit device (one process per GPU under torch.distributed / MPI). */
int asora_device_init_ex(int N, int num_src_par, int device_id);

/* libasora.device_close()                         python_module.cu:87-92 -> memory.cu:119-129 */
int asora_device_close(void);

/* libasora.density_to_device(ndens_flat, N)       python_module.cu:97-109 -> memory.cu:85-88 */
int asora_density_to_device(const double *ndens, int N);

/* libasora.photo_table_to_device(thin, thick, NumTau)   python_module.cu:114-128 -> memory.cu:90-98.
 * NumTau = number of elements of each table. */
int asora_photo_table_to_device(const double *thin_table, const double *thick_table, int NumTau);

/* Heating tables (no counterpart in the reference's GPU library, which lists GPU heating as TODO,
 * pyc2ray/c2ray_base.py:424-426; the Fortran CPU path has them: src/c2ray/photorates.f90:118,124).
 * Same length and tau grid as the photo tables, which must have been uploaded first. */
int asora_heat_table_to_device(const double *heat_thin_table, const double *heat_thick_table, int NumTau);

/* libasora.source_data_to_device(pos, flux, NumSrc)     python_module.cu:133-148 -> memory.cu:99-114 */
int asora_source_data_to_device(const int32_t *pos, const double *flux, int NumSrc);

/* Per-source spectra (no counterpart in the reference, where every source shines with one spectrum).
 * asora_spectra_to_device replaces the rate tables by NumSpec sets, 1 <= NumSpec <= 16: the arrays are [NumSpec][NumTau] in C
 * order, all sets share NumTau and the tau grid of the raytrace calls.  Both heating pointers may be null: no heating tables, as
 * after asora_photo_table_to_device alone.  asora_photo_table_to_device / asora_heat_table_to_device mean NumSpec = 1.
 * asora_source_spectra_to_device gives source s of the last asora_source_data_to_device (which resets every source to set 0) the
 * set spec[s]; null or all zeros: every source set 0.  An index outside [0, NumSpec) fails with code 3 here, or with code 4 in the
 * first raytrace when the tables are replaced by fewer sets afterwards: no index reaches a kernel unchecked.  While any source
 * has a set other than 0, the sub-box calls (asora_subbox_raytrace_device, c2ray_do_all_sources) and grey opacity
 * (ASORA_OPT_GREY_NOTABLES) fail with code 4.
 * asora_debug_sort_sources: host only, no device needed -- the position-ordered copy of a source list exactly as
 * asora_source_data_to_device forms it, with the set of each source carried along (spec / spec_out may be null). */
#define ASORA_MAX_SPECTRA 16
int asora_spectra_to_device(int NumSpec, int NumTau, const double *photo_thin, const double *photo_thick,
                            const double *heat_thin, const double *heat_thick);
int asora_source_spectra_to_device(const int32_t *spec, int NumSrc);
int asora_num_spectra(void);
int asora_debug_sort_sources(const int32_t *pos, const double *flux, const int32_t *spec, int NumSrc, int32_t *pos_out,
                             double *flux_out, int32_t *spec_out);

/* libasora.do_all_sources(R, coldensh_out, sig, dr, ndens, xh_av, phi_ion, NumSrc, m1,
 *                         minlogtau, dlogtau, NumTau)   python_module.cu:21-68 -> raytracing.cu:79-148.
 * coldensh_out and ndens are ignored, as in the reference (raytracing.cu:116: the density must
 * already be on the device).  Uploads xh_av, raytraces, downloads phi_ion (in place). */
int asora_do_all_sources(double R, double *coldensh_out, double sig, double dr, const double *ndens,
                         const double *xh_av, double *phi_ion, int NumSrc, int m1,
                         double minlogtau, double dlogtau, int NumTau);

/* libc2ray.chemistry.global_pass(dt, ndens, temp, xh, xh_av, xh_intermed, phi_ion, bh00, albpow,
 *                                colh0, temph0, abu_c) -> conv_flag
 * f2py wrapper of src/c2ray/chemistry.f90:13-48.  Elementwise: all six grids must share one
 * storage order; xh_av and xh_intermed are updated in place.  Runs on the GPU (uploads the six
 * grids, runs the fused kernel, downloads two); needs no prior asora_device_init. */
int c2ray_global_pass(double dt, const double *ndens, const double *temp, const double *xh,
                      double *xh_av, double *xh_intermed, const double *phi_ion,
                      double bh00, double albpow, double colh0, double temph0, double abu_c,
                      int m1, int m2, int m3, int *conv_flag);

/* libc2ray.raytracing.do_all_sources(normflux, srcpos, max_subbox, subboxsize, coldensh_out, sig, dr, ndens,
 *        xh_av, phi_ion, phi_heat, loss_fraction, photo_thin_table, photo_thick_table, heat_thin_table,
 *        heat_thick_table, minlogtau, dlogtau, R_max_LLS) -> (sum_nbox, photon_loss)
 * f2py wrapper of src/c2ray/raytracing.f90:52-119 (built with -DUSE_SUBBOX, src/c2ray/Makefile:3): the
 * reference's CPU raytracer.  Same semantics, evaluated on the GPU: per source a cube of half-width
 * min(max_subbox, N/2) is traced in sub-boxes of `subboxsize` cells until the photons crossing the box faces
 * fall to loss_fraction of the source's output (do_source, f90:193-221); rates are deposited only within
 * R_max_LLS (cells) and below the column-density cap; Fortran-flavoured constants.
 *   srcpos        (3,NumSrc) column-major, 1-based                       (f90:64)
 *   grids         Fortran order (m1,m2,m3), m1 == m2 == m3               (f90:65-70)
 *   coldensh_out  out: outgoing column density of the cells the LAST source reached, 0 elsewhere (f90:181)
 *   phi_ion       out (zeroed first, f90:95);  phi_heat  in/out (accumulated onto)
 *   xh_av, ndens  in
 *   sum_nbox, photon_loss  out: sub-boxes used by all sources / photons lost through their last boxes
 * Every cell's rate uses the flux of the LAST source, as the reference does (f90:500,503); set
 * ASORA_OPT_C2RAY_OWN_FLUX = 1 for each source's own flux.  Cells on a box face that deposit nothing
 * (beyond R_max_LLS or above the cap) contribute 0 to the loss (the reference adds an undefined value there).
 * Needs no prior asora_device_init: it initialises the library for m1 itself (and again when a later call
 * comes with another m1); a library initialised by asora_device_init for another mesh size makes it fail.
 * Overwrites the device grids NDENS, XH_AV, PHI_ION, PHI_HEAT. */
int c2ray_do_all_sources(const double *normflux, const int32_t *srcpos, int max_subbox, int subboxsize,
                         double *coldensh_out, double sig, double dr, const double *ndens, const double *xh_av,
                         double *phi_ion, double *phi_heat, float loss_fraction,
                         const double *photo_thin_table, const double *photo_thick_table,
                         const double *heat_thin_table, const double *heat_thick_table,
                         double minlogtau, double dlogtau, double R_max_LLS,
                         int NumTau, int NumSrc, int m1, int m2, int m3,
                         int *sum_nbox, double *photon_loss);

/* Message of the last failing call in this thread's process ("" if none). */
const char *asora_last_error(void);

/* ------------------------------------------------------------------------------------------ */
/* B. Device-resident extension (fused evolve loop; pyc2ray/evolve.py:168-240 restated so that  */
/*    only three scalars cross PCIe per iteration)                                              */
/* ------------------------------------------------------------------------------------------ */

/* Grid selectors for asora_grid_to_device / asora_grid_to_host / asora_device_ptr */
enum {
    ASORA_GRID_NDENS = 0,       /* hydrogen density                 (memory.cu n_dev)   */
    ASORA_GRID_XH_AV = 1,       /* time-averaged ionised fraction   (memory.cu x_dev)   */
    ASORA_GRID_PHI_ION = 2,     /* photo-ionisation rate            (memory.cu phi_dev) */
    ASORA_GRID_TEMP = 3,        /* temperature                                          */
    ASORA_GRID_XH = 4,          /* ionised fraction at start of the step                */
    ASORA_GRID_XH_INTERMED = 5, /* end-of-step ionised fraction                         */
    ASORA_GRID_PHI_HEAT = 6,    /* photo-heating rate (only filled when heating is on)  */
    ASORA_GRID_TEMP_END = 7,    /* end-of-step temperature (thermal mode only)          */
    ASORA_GRID_CLUMP = 8,       /* sub-grid clumping factor <n^2>/<n>^2 (asora_clumping mode 2 only) */
    ASORA_GRID_COUNT = 9
};

/* Upload / download one N^3 grid.  order = 'C': buffer is logical [i][j][k] C-contiguous;
 * order = 'F': buffer is Fortran-contiguous (element (i,j,k) at i + N*j + N*N*k) and is
 * transposed on the device. */
int asora_grid_to_device(int which, const double *host, int N, char order);
int asora_grid_to_host(int which, double *host, int N, char order);
/* Device-to-device copy between two grids (e.g. xh -> xh_av at the start of a step). */
int asora_grid_copy(int dst, int src);
/* grid *= factor on the device: the dilution of a device-resident density in a cosmological run
 * (ref: pyc2ray/c2ray_base.py:244-248 scales the host array). */
int asora_grid_scale(int which, double factor);
/* Sum over all cells of a grid, evaluated on the device in a fixed order (the two means of the reference's log line,
 * pyc2ray/evolve.py:160 `ndens.mean()`, `xh.mean()`, without a host pass over N^3 values). */
int asora_grid_sum(int which, double *sum);
/* Page-locked host memory for the grids a caller hands to asora_grid_to_host / asora_grid_to_device: copies into
 * pageable memory that has never been touched run at a fraction of the PCIe rate (page faults inside the copy).
 * The host side keeps a small pool of these behind the arrays evolve3D returns (pyc2ray_amd/_pinned.py). */
int asora_host_alloc(size_t bytes, void **host);
int asora_host_free(void *host);
/* Raw device pointer of a grid (for zero-copy views, e.g. an RCCL all-reduce of phi_ion
 * through torch.distributed).  NULL when not initialised. */
void *asora_device_ptr(int which);

/* Raytrace all uploaded sources from the device-resident ndens/xh_av into the device-resident
 * phi_ion (zeroed first).  Same arithmetic as asora_do_all_sources without the PCIe copies.
 * Sources [src_begin, src_begin+src_count) of the uploaded list are traced. */
int asora_raytrace_device(double R, double sig, double dr, int src_begin, int src_count,
                          double minlogtau, double dlogtau, int NumTau);

/* The same raytrace in three parts, for callers that overlap the multi-GPU sum of the rate grid with the trace
 * (one process per GPU; pyc2ray_amd/dist.py): with the sources uploaded in ascending order of their first
 * coordinate, the planes phi_ion[i][:][:] a chunk of sources can no longer reach are final and can be summed
 * across GPUs (RCCL on asora_device_ptr(ASORA_GRID_PHI_ION), ordered after asora_stream()) while the next chunk
 * is being traced.
 *   asora_raytrace_begin  zeroes the accumulators, forms nHI, fixes the parameters of the call;
 *   asora_raytrace_range  traces sources [src_begin, src_begin + src_count) into the accumulators (asynchronous);
 *   asora_raytrace_fold   completes planes [i_begin, i_begin + i_count) of phi_ion (adds the z-face accumulator,
 *                         which is kept in [k][j][i] order); every plane must be folded exactly once per call.
 * asora_raytrace_device(...) == begin; range(all); fold(0, N). */
int asora_raytrace_begin(double R, double sig, double dr, double minlogtau, double dlogtau, int NumTau);
int asora_raytrace_range(int src_begin, int src_count);
/* asora_raytrace_begin for a rank of a multi-GPU run that only works on SOME planes of the grids: nHI is formed
 * from ndens and xh_av, and both rate accumulators are zeroed, on the `nruns` runs of planes
 * [runs[2q], runs[2q] + runs[2q+1]) only -- the planes this rank's sources reach plus the planes whose rates it
 * collects (pyc2ray_amd/dist.py, SlabPlan).  Everything else of the accumulators must already be zero (it stays
 * zero: nothing is traced into it), which one call of asora_raytrace_begin at the start of a time step ensures. */
int asora_raytrace_begin_planes(double R, double sig, double dr, double minlogtau, double dlogtau, int NumTau,
                                const int *runs, int nruns);
int asora_raytrace_fold(int i_begin, int i_count);
/* The HIP stream (hipStream_t) all of the library's work is ordered on. */
void *asora_stream(void);

/* One chemistry pass on the device-resident grids (ndens, temp, xh, xh_av, xh_intermed,
 * phi_ion): global_pass + the three reductions of pyc2ray/evolve.py:216-217.
 * Outputs: conv_flag (chemistry.f90:99-104), sum(xh_intermed), sum(1-xh_intermed). */
/* The raytracer of libc2ray.raytracing.do_all_sources (cubic sub-boxes, photon loss; see c2ray_do_all_sources in
 * section A) on device-resident inputs: NDENS and XH_AV on the device, tables from asora_photo_table_to_device
 * [+ asora_heat_table_to_device with ASORA_OPT_HEATING], sources [src_begin, src_begin + src_count) of
 * asora_source_data_to_device (0-based positions).  Leaves the rates in ASORA_GRID_PHI_ION (and PHI_HEAT, zeroed
 * first); returns the number of sub-boxes used and the photon loss.  This is what evolve3D(use_gpu=False) iterates. */
int asora_subbox_raytrace_device(int max_subbox, int subboxsize, float loss_fraction, double R_max_LLS, double sig,
                                 double dr, double minlogtau, double dlogtau, int NumTau, int src_begin, int src_count,
                                 int *sum_nbox, double *photon_loss);
/* asora_device_init for callers that have no device_init of their own (the libc2ray-compatible entry points):
 * initialises the library for N if it is not initialised, re-initialises it if it was initialised this way for
 * another N, and fails if asora_device_init was called for another N. */
int asora_device_init_auto(int N);

int asora_chemistry_device(double dt, double bh00, double albpow, double colh0, double temph0,
                           double abu_c, int *conv_flag, double *sum_xh1, double *sum_xh0);

/* The same pass slab by slab (planes [i_begin, i_begin + i_count) of every grid), for callers that start the
 * chemistry of the planes whose rates are already summed across GPUs while the rest is still in flight.
 * `first` != 0 resets the three reductions, later calls add to them in call order; asora_chemistry_finish
 * returns them (and is the only call of the group that waits for the device). */
int asora_chemistry_range(double dt, double bh00, double albpow, double colh0, double temph0, double abu_c,
                          int i_begin, int i_count, int first);
int asora_chemistry_finish(int *conv_flag, double *sum_xh1, double *sum_xh0);
/* Device address of the three reductions {sum(xh_intermed), sum(1 - xh_intermed), conv_flag} (doubles) that
 * asora_chemistry_range accumulates: a multi-GPU caller sums them across ranks in place (one RCCL all-reduce ordered after
 * asora_stream()) and reads them back once, instead of asora_chemistry_finish + a host round trip per rank. */
void *asora_reduction_ptr(void);

/* The whole outer loop of evolve3D (pyc2ray/evolve.py:168-240) on the device.  Per iteration the host of the
 * reference uploads xh_av, downloads phi_ion, reshapes, runs global_pass, forms two sums with numpy and tests
 * convergence (evolve.py:187,200,210,216-236); here an iteration is three launches -- the raytrace, ONE pass over
 * the grids that folds the rate accumulators, solves the chemistry, forms nHI of the new xh_av in both layouts for
 * the next raytrace and zeroes the accumulators, and a one-workgroup kernel that finishes the three reductions and
 * evaluates the convergence test -- so several iterations can be enqueued without the host in between; launches
 * enqueued beyond convergence see the device flag and do nothing, so the iteration count is exactly the reference's.
 *   asora_evolve_begin    NDENS, TEMP, XH must be on the device; xh_av = xh_intermed = xh (evolve.py:136-137) is implied.
 *                         conv_criterion = min(int(convergence_fraction N^3), (NumSrc-1)/3) (evolve.py:127) is the
 *                         caller's to compute (NumSrc is the TOTAL source count, evolve.py:346).
 *   asora_evolve_enqueue  enqueues `iterations` (1..32) outer iterations; asynchronous.
 *   asora_evolve_poll     waits for what was enqueued; returns the iterations carried out so far, whether the test has
 *                         passed, and one row {conv_flag, sum(xh_intermed), sum(1-xh_intermed), rel_change_xh1,
 *                         rel_change_xh0} per iteration not reported yet (at most history_rows rows; history = NULL: the
 *                         rows are given up).  At most 64 iterations may be enqueued between two polls.  The pass does
 *                         not store the folded rates (the accumulators alternate between two pairs instead, so the last
 *                         iteration's survive): the poll folds them into ASORA_GRID_PHI_ION, which is valid from then on.
 * Results: ASORA_GRID_XH_INTERMED (xh_new), ASORA_GRID_XH_AV, and -- after a poll -- ASORA_GRID_PHI_ION. */
int asora_evolve_begin(double dt, double bh00, double albpow, double colh0, double temph0, double abu_c,
                       double R, double sig, double dr, double minlogtau, double dlogtau, int NumTau,
                       int src_begin, int src_count, double conv_criterion, double convergence_fraction);
int asora_evolve_enqueue(int iterations);
int asora_evolve_poll(int *niter, int *converged, double *history, int history_rows, int *rows_written);

/* The same device-resident loop with the sources sharded over several GPUs (pyc2ray/evolve.py:249-498 evolve3D_MPI: sources cut
 * into contiguous blocks :360-371, rate grids summed over the ranks every iteration :433-437, results broadcast :480-497).
 * Here a rank traces its block of sources, owns the chemistry of the planes [own_begin, own_begin + own_count), sends the
 * rates it traced onto other ranks' planes to their owners and receives the new xh_av of the foreign planes its sources
 * reach (pyc2ray_amd/dist.py: SlabPlan, TorchComm).  One iteration, all calls asynchronous on asora_stream():
 *   asora_evolve_slab_trace       traces sources [src_begin, src_begin + src_count) of the step (one call, or one per chunk)
 *   asora_evolve_slab_fold_out    planes owned by ANOTHER rank: the rates traced onto them are summed over the two accumulator
 *                                 layouts into the out-box (asora_evolve_slab_outbox(): an N^3 grid, plane i at i*N*N), from
 *                                 where the caller sends them; the accumulators of the NEXT iteration are zeroed there
 *   asora_evolve_slab_add         rates received for OWN planes (a device buffer of i_count*N*N doubles; _add_host: a host
 *                                 buffer), added in call order
 *   asora_evolve_slab_pass        the fused pass of the one-GPU loop on the own planes (rates folded, chemistry, nHI of the new
 *                                 xh_av in both layouts, next accumulators zeroed); leaves THIS RANK'S {sum x, sum 1-x, conv_flag}
 *                                 at asora_reduction_ptr()
 *   asora_evolve_slab_nhi         planes whose new xh_av has just arrived in ASORA_GRID_XH_AV: nHI for the next trace
 *   asora_evolve_slab_close       host_sums = NULL: the caller has summed the three doubles at asora_reduction_ptr() over the
 *                                 ranks IN PLACE (one all-reduce ordered on asora_stream()); else the three sums over all ranks,
 *                                 from the host.  Evaluates the convergence test of evolve.py:216-236 on them on the device.
 * Every launch is gated by the device's `done` flag, so -- as on one GPU -- several iterations can be enqueued per
 * asora_evolve_poll, and every rank, working from identical sums, stops at the same iteration.  asora_evolve_poll folds the last
 * iteration's rates into ASORA_GRID_PHI_ION (complete on the own planes).  ASORA_GRID_XH_INTERMED / _XH_AV: own planes. */
int asora_evolve_begin_slab(double dt, double bh00, double albpow, double colh0, double temph0, double abu_c,
                            double R, double sig, double dr, double minlogtau, double dlogtau, int NumTau,
                            int src_begin, int src_count, double conv_criterion, double convergence_fraction,
                            int own_begin, int own_count);
/* The same step in thermal mode (asora_thermal_params below).  Fails with code 4 without asora_thermal_params(1, ...), without
 * heating tables on the device, or without the [k][j][i] twins.  Beginning through this entry is how a caller declares that it
 * exchanges the heating rates together with the photo-ionisation rates; every call of the sequence then carries both fields:
 *   asora_evolve_slab_trace       traces with heating, into the iteration's rate pair and heating pair
 *   asora_evolve_slab_fold_out    also sums the heating traced onto the foreign planes into the heating out-box
 *                                 (asora_evolve_slab_heat_outbox(): N^3 doubles, plane i at i*N*N, allocated by the first such
 *                                 step) and zeroes the next iteration's heating accumulators there -- one launch for both fields
 *   asora_evolve_slab_add_heat    heating received for OWN planes (_add_heat_host: from a host buffer), added in call order
 *   asora_evolve_slab_pass        the thermal fused pass on the own planes: writes ASORA_GRID_TEMP_END there and adds to this
 *                                 rank's asora_thermal_stats counters
 *   asora_evolve_slab_fold_all    sums the heating of all planes into the heating out-box as well; the caller all-reduces BOTH
 *                                 out-boxes, and the pass keeps the sums in ASORA_GRID_PHI_ION and ASORA_GRID_PHI_HEAT
 *   asora_evolve_poll             folds the last iteration's heating into ASORA_GRID_PHI_HEAT (complete on the own planes)
 * Temperatures do not travel between iterations: the trace reads nHI only, every rank holds the start-of-step TEMP, and TEMP_END
 * is collected from the owners once, at the end of the step. */
int asora_evolve_begin_slab_thermal(double dt, double bh00, double albpow, double colh0, double temph0, double abu_c,
                                    double R, double sig, double dr, double minlogtau, double dlogtau, int NumTau,
                                    int src_begin, int src_count, double conv_criterion, double convergence_fraction,
                                    int own_begin, int own_count);
int asora_evolve_slab_trace(int src_begin, int src_count);
int asora_evolve_slab_fold_out(int i_begin, int i_count);
/* The full-grid exchange of the reference (pyc2ray/evolve.py:433-437: MPI Allreduce of the rate grid, chemistry on identical data)
 * on the same loop, for a step begun with own_begin = 0, own_count = N on every rank: asora_evolve_slab_fold_all sums the two
 * accumulator layouts of ALL planes into the out-box; the caller all-reduces the out-box over the ranks IN PLACE (ordered on
 * asora_stream()); asora_evolve_slab_pass then takes the rates from the out-box, keeps them in ASORA_GRID_PHI_ION, and its three
 * sums are those of the whole grid already: asora_evolve_slab_close(NULL) without a reduction.  One iteration:
 * trace, fold_all, [all-reduce], pass, close; asora_evolve_poll then has nothing left to fold.  asora_evolve_slab_outbox_from_host: the out-box planes written from the host (for
 * transports that sum on the host). */
int asora_evolve_slab_fold_all(void);
void *asora_evolve_slab_outbox(void);
int asora_evolve_slab_outbox_to_host(int i_begin, int i_count, double *host);
int asora_evolve_slab_outbox_from_host(int i_begin, int i_count, const double *host);
int asora_evolve_slab_add(int i_begin, int i_count, const double *dev_planes);
int asora_evolve_slab_add_host(int i_begin, int i_count, const double *host_planes);
/* the heating rates of a step begun with asora_evolve_begin_slab_thermal: the twins of the five calls above */
void *asora_evolve_slab_heat_outbox(void);
int asora_evolve_slab_heat_outbox_to_host(int i_begin, int i_count, double *host);
int asora_evolve_slab_heat_outbox_from_host(int i_begin, int i_count, const double *host);
int asora_evolve_slab_add_heat(int i_begin, int i_count, const double *dev_planes);
int asora_evolve_slab_add_heat_host(int i_begin, int i_count, const double *host_planes);
int asora_evolve_slab_pass(void);
int asora_evolve_slab_nhi(int i_begin, int i_count);
int asora_evolve_slab_close(const double *host_sums);

/* Runs of i-planes [i_begin, i_begin + i_count) of a grid to / from a host buffer of i_count*N*N doubles (C order).
 * What multi-GPU ranks exchange are such runs: the planes a rank's sources reach, the planes whose chemistry it owns. */
int asora_planes_to_host(int which, int i_begin, int i_count, double *host);
int asora_planes_to_device(int which, int i_begin, int i_count, const double *host);

/* Non-isothermal chemistry ("Thermal mode").  enable != 0 switches asora_chemistry_device and the
 * asora_evolve_* loop to the thermal form: per cell the temperature is integrated over the step from photo-heating
 * (ASORA_GRID_PHI_HEAT, erg/s per HI atom) and radiative cooling inside do_chemistry's inner iteration
 * (src/c2ray/chemistry.f90:164,171-176,182-189); TEMP holds the start-of-step temperature and stays untouched, the
 * end-of-step temperature goes to ASORA_GRID_TEMP_END.  The device loop traces with heating into accumulators of its
 * own and asora_evolve_poll folds the last iteration's heating into PHI_HEAT.
 *   relative_denergy  largest relative change of the thermal energy per substep (> 0)
 *   t_floor           lower bound of the temperature (K, >= 0)
 *   max_substeps      substeps per integration (>= 1); the last one takes the remainder of the step
 *   cooling_mask      bit 0 recombination, 1 collisional ionisation, 2 collisional excitation, 3 bremsstrahlung,
 *                     4 Compton exchange with the CMB (only while `compton` != 0)
 *   t_cmb             CMB temperature at the current redshift (K)
 * Fails with code 4 when no heating tables are on the device (asora_heat_table_to_device) or grey opacity is on.
 * enable = 0 returns to the isothermal form.  Across ranks a thermal step is begun with asora_evolve_begin_slab_thermal;
 * asora_evolve_begin_slab, the isothermal entry, fails while thermal mode is on (its caller exchanges no heating rates).
 * asora_chemistry_range and the pipelined loop built on it stay isothermal. */
int asora_thermal_params(int enable, double relative_denergy, double t_floor, int max_substeps, unsigned cooling_mask,
                         int compton, double t_cmb);
/* Substep statistics of the thermal passes since the last asora_chemistry_device / asora_evolve_begin (summed over the
 * passes of a step): cells whose integration hit max_substeps, cells clamped to t_floor, most substeps of one integration. */
int asora_thermal_stats(long long *cells_max_substeps, long long *cells_floored, int *max_substeps_used);

/* Sub-grid clumping factor C = <n^2>/<n>^2 of the case-B recombination rate: doric's
 * brech0 = C bh00 (T/1e4)^albpow (src/c2ray/chemistry.f90:257), the slot the reference fills with 1.  Nothing else is
 * clumped: collisional and photo-ionisation, the raytrace and c2ray_global_pass are not; in thermal mode the case-B
 * recombination cooling is (the same n_e n_HII process).
 *   mode 0  off (the default, and the reference's behaviour); `constant` is ignored
 *   mode 1  one factor `constant` for the whole grid
 *   mode 2  per cell, from ASORA_GRID_CLUMP (uploaded with asora_grid_to_device in either order; allocated on first
 *           upload, so a run without it allocates nothing); `constant` is ignored
 * Every chemistry entry honours the mode: asora_chemistry_device, asora_chemistry_range, asora_evolve_begin /
 * _enqueue, the asora_evolve_slab_* loop and the thermal passes.  Set it before asora_evolve_begin(_slab): the uniform-
 * temperature pass takes its recombination factor from the probe made there.  Fails with code 3 for a constant that is not
 * finite and > 0 (mode 1) or an unknown mode, with code 4 for mode 2 without ASORA_GRID_CLUMP on the device.  The mode
 * holds until it is set again or the device is re-initialised. */
int asora_clumping(int mode, double constant);

/* Lyman-limit-system (LLS) opacity: unresolved absorbers as a distributed photon sink of the raytrace (DESIGN.md section
 * 4.1b).  The absorber density the raytrace sees becomes
 *   n_abs = ndens ((1 - xh_av) + per_density) + n_const
 * where it was ndens (1 - xh_av):
 *   n_const      a uniform absorber density in cm^-3 (a proper mean free path lambda: n_const = 1 / (sig lambda))
 *   per_density  absorbers per atom of the local density (dimensionless)
 * Column densities accumulate the added opacity, and a cell's rate stays the photon-conserving share per absorber, so
 * hydrogen receives n_HI / n_abs of the photons absorbed in the cell (the heating rate per HI atom likewise).  The
 * chemistry keeps ndens and the rates per atom; R_max_LLS and the column-density cap apply to the total column.
 * Every entry that forms the absorber density honours it: asora_raytrace_device, asora_raytrace_begin / _begin_planes,
 * asora_do_all_sources, asora_debug_coldens, both sub-box entries, asora_evolve_begin / _enqueue and the
 * asora_evolve_slab_* loop (asora_evolve_slab_nhi and the fused pass).  Set it before asora_evolve_begin(_slab) /
 * asora_raytrace_begin: a step in progress forms its next nHI with the values of the moment.  (0, 0) is off, bit for bit
 * the rates without the call.  Fails with code 3 for a value that is negative or not finite, with code 4 while grey opacity
 * (ASORA_OPT_GREY_NOTABLES) is on; a trace begun with both on fails with code 4 as well.  The values hold until they are set
 * again or the device is re-initialised. */
int asora_lls_opacity(double n_const, double per_density);
int asora_get_lls_opacity(double *n_const, double *per_density);

/* Plane-parallel ionising flux through faces of the box: radiation that enters from outside.
 *   face[q]      0 ... 5 = -x +x -y +y -z +z, the face the radiation ENTERS through (-x: the plane i = 0, travelling towards
 *                increasing i; x is the first index of the (N, N, N) C-ordered grids); at most one entry per face
 *   flux[q]      in the units of the source strengths per cm^2: 1e48 photons s^-1 cm^-2; finite and >= 0
 *   spectrum[q]  the table set the face shines with (asora_spectra_to_device), or spectrum = NULL: set 0 for every face
 * count = 0 switches it off.  Each of the N^2 rays of a face is marched over its N cells in travel order, never wrapping
 * (whatever ASORA_OPT_OPEN_BOUNDARIES says) and without a cut at R: cd_out = cd_in + n_abs dr with the absorber density of
 * the point-source trace (asora_lls_opacity included), the rate of photoion_rates with prefact = flux / dr, divided by
 * n_abs and added where cd_in <= the column-density cap.  The sweep runs once per trace, behind the zeroing of the rate
 * accumulators and the forming of nHI and ahead of every point-source launch: asora_raytrace_device, asora_raytrace_begin /
 * _begin_planes (so the three-part call), asora_do_all_sources (which then takes its plain path), asora_evolve_begin /
 * _enqueue (every iteration) and the asora_evolve_slab_* loop (ahead of an iteration's first asora_evolve_slab_trace, which
 * must then be called every iteration, with an empty source range if need be).  A trace or a step with faces and no point
 * source is valid.  With ASORA_OPT_HEATING / the thermal mode the faces deposit heating rates as well.  A trace or step keeps the
 * setting it began with.
 * Fails with code 3 for a count outside 0 ... 6, a face outside 0 ... 5 or given twice, a flux that is negative or not
 * finite, a spectrum index outside 0 ... ASORA_MAX_SPECTRA - 1.  While faces are set, code 4 and nothing launched from: any
 * trace under grey opacity (ASORA_OPT_GREY_NOTABLES), asora_debug_coldens, both sub-box entries (c2ray_do_all_sources,
 * asora_subbox_raytrace_device), asora_evolve_begin_slab(_thermal) with fewer than all planes owned (the slab exchange does not
 * deliver a whole-box sweep; own every plane and use asora_evolve_slab_fold_all), heating without heating tables, a spectrum index the device holds no set for, and a z
 * face without the [k][j][i] twins (ASORA_OPT_Z_TRANSPOSED = 0).  The setting holds until it is set again or the device is
 * re-initialised. */
int asora_plane_flux(int count, const int32_t *face, const double *flux, const int32_t *spectrum);
/* Reads the setting back: *count, and the first *count entries of face / flux / spectrum (room for 6 each; any may be NULL). */
int asora_get_plane_flux(int *count, int32_t *face, double *flux, int32_t *spectrum);

/* Photon budget and mean ionised fractions of a time step: twelve sums over the cells of the planes
 * [i_begin, i_begin + i_count) of the device grids, formed by ONE read-only streaming pass (no grid is written) and returned on
 * the host.  With n = NDENS, x0 = XH, x1 = XH_INTERMED, xav = XH_AV, Gamma = PHI_ION; c the clumping factor of the cell
 * (asora_clumping: 1, the constant, or CLUMP); (a, b) the pair of asora_get_lls_opacity; T = TEMP, or (TEMP + TEMP_END) / 2 with
 * use_temp_end != 0; ne = n (xav + abu_c), nHI = n (1 - xav):
 *   CELLS 1            N   n              X   x1                 NX   n x1
 *   NX0   n x0         DNX n (x1 - x0)    PHOTO Gamma nHI        LLS  Gamma (n b + a)
 *   REC   c bh00 (T/1e4)^albpow ne n xav  COL colh0 sqrt(T) exp(-temph0/T) ne nHI        T  T        NT  n T
 * A thermal step's chemistry uses a time-averaged temperature of its own that is not stored; use_temp_end evaluates REC and COL at
 * the mean of the step's first and last temperature instead.  Call it after the step's loop has ended (after asora_evolve_poll
 * reported convergence, or after the last chemistry pass) and before XH is overwritten with XH_INTERMED.
 * The sums are order-fixed (no floating-point atomics): two calls on the same grids return the same bits.  Ordered on
 * asora_stream(); returns once the twelve doubles are on the host (one synchronisation).  With ASORA_OPT_TIMING the pass counts
 * under ASORA_KERNEL_FINISH.  i_count = 0: twelve zeros.  Fails with code 3 for sums = NULL or a plane range outside the mesh,
 * with code 4 when a grid it reads holds no data: NDENS, XH, XH_INTERMED, XH_AV, PHI_ION, TEMP; TEMP_END with use_temp_end;
 * CLUMP in clumping mode 2. */
enum { ASORA_BUDGET_CELLS = 0, ASORA_BUDGET_N = 1, ASORA_BUDGET_X = 2, ASORA_BUDGET_NX = 3, ASORA_BUDGET_NX0 = 4,
       ASORA_BUDGET_DNX = 5, ASORA_BUDGET_PHOTO = 6, ASORA_BUDGET_LLS = 7, ASORA_BUDGET_REC = 8, ASORA_BUDGET_COL = 9,
       ASORA_BUDGET_T = 10, ASORA_BUDGET_NT = 11, ASORA_BUDGET_COUNT = 12 };
int asora_step_budget(double bh00, double albpow, double colh0, double temph0, double abu_c, int use_temp_end, int i_begin, int i_count, double *sums);

/* Size distribution of the ionised regions by the mean-free-path method (Mesinger & Furlanetto 2007), on
 * the device grid `which_grid` where it lies: n_rays rays start in random in-phase cells, fly in random directions and end at the
 * first cell that is not in phase; their lengths, in cells, are binned.  A cell x is in phase when x >= threshold (phase 0: ionised
 * regions of XH) or x < threshold (phase 1: neutral islands); a NaN is in neither.  No grid is written.  Three stages on
 * asora_stream(): a threshold pass that turns the grid into a bit mask -- bit k & 63 of word (i N + j) W + (k >> 6), W = ceil(N / 64),
 * pad bits 0 -- and one count per row (i, j); an exclusive scan of the counts, whose total is n_phase; the rays.
 * Ray r is a pure function of (seed, r, mask), all hashes in uint64 with wrap-around:
 *   mix(seed, c): z = seed + (c + 1) 0x9E3779B97F4A7C15; z = (z ^ z >> 30) 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) 0x94D049BB133111EB;
 *                 z ^ z >> 31 (splitmix64);  u01(h) = (h >> 11) 2^-53;
 *   start: the u-th in-phase cell in C order, u = mix(seed, 4 r) % n_phase;
 *   direction: mu = 2 u01(mix(seed, 4 r + 1)) - 1, phi = 2 pi u01(mix(seed, 4 r + 2)), s = sqrt(1 - mu mu), d = (s cos phi, s sin phi, mu);
 *   march: exact cell traversal from the cell centre.  Per axis a: step = sign(d_a), tDelta = 1 / |d_a| (infinite for d_a = 0),
 *          m_a = 0 crossings.  Loop: tMax_a = (m_a + 0.5) tDelta_a; the axis of the smallest tMax (ties: the lowest), t = that tMax;
 *          t > l_max: CAPPED, length l_max; else one cell along the axis, ++m_a; periodic != 0: wrap; else outside [0, N): LEFT_BOX,
 *          length t; the new cell not in phase: ENDED, length t.
 * An ENDED ray of length L with edges[b] <= L < edges[b + 1] counts in counts[b]; L < edges[0] is underflow, L >= edges[n_bins]
 * overflow.  tallies = {ENDED rays (under- and overflow included), CAPPED, LEFT_BOX, underflow, overflow, n_phase}; moments =
 * {sum L, sum L^2} over the ENDED rays.  Counts are integers and the two sums are order-fixed: two calls return the same bits.
 * ray_start [n_rays][3], ray_dir [n_rays][3], ray_len [n_rays], ray_status [n_rays] (ASORA_BUBBLE_*): the per-ray record, for
 * tests; all four NULL in production.  n_rays = 0 or n_phase = 0: no ray is marched, every output is zero except n_phase (n_phase
 * is known on the device only, so the ray kernel of a call with n_rays > 0 is enqueued and returns at once when it reads 0).
 * One synchronisation per call; the buffers are allocated by the first call and kept until the device is closed.  With
 * ASORA_OPT_TIMING the stages count under ASORA_KERNEL_BUBBLE_MASK / _SCAN / _RAYS.  Fails with code 2 before device_init, 4 for a
 * grid that holds no data, 3 for: a bad selector, a non-finite threshold, phase not 0 or 1, n_rays < 0, l_max not finite or not > 0,
 * n_bins outside [1, ASORA_BUBBLE_MAX_BINS], edges not finite or not ascending, a null pointer among edges / counts / tallies /
 * moments, some but not all of the four record pointers. */
enum { ASORA_BUBBLE_ENDED = 0, ASORA_BUBBLE_CAPPED = 1, ASORA_BUBBLE_LEFT_BOX = 2 };
enum { ASORA_BUBBLE_MAX_BINS = 256 };
int asora_bubble_mfp(int which_grid, double threshold, int phase, int periodic, unsigned long long seed, long long n_rays, double l_max,
                     int n_bins, const double *edges, unsigned long long *counts, unsigned long long *tallies, double *moments,
                     int32_t *ray_start, double *ray_dir, double *ray_len, int32_t *ray_status);
/* The products of the threshold pass alone, downloaded (tests): mask_words [N^2 W], row_counts [N^2]. */
int asora_bubble_mask(int which_grid, double threshold, int phase, uint64_t *mask_words, uint32_t *row_counts);

/* The connected in-phase regions of device grid `which_grid` (the friends-of-friends view of the ionised bubbles; DESIGN.md section
 * 4.2e): the distribution of their volumes and the numbers that describe percolation.  No grid is written.  The specification,
 * which no implementation detail enters:
 *   in phase  : as for asora_bubble_mfp -- phase 0: x >= threshold, phase 1: x < threshold; a NaN is in neither;
 *   neighbours: connectivity 6: the cells across the faces; 26: across faces, edges and corners.  periodic != 0: the relation wraps
 *               on every axis, else it stops at the faces of the box.  (For N = 1, 2 a cell is its own neighbour, or meets the same
 *               neighbour twice, through the wrap: harmless);
 *   region    : an equivalence class of in-phase cells under the transitive closure of the neighbour relation.  Its label is the
 *               smallest C-order index (i N + j) N + k of its cells, a uint32 (N <= ASORA_REGION_MAX_N = 645, the mesh at which the
 *               labelling's 8 bytes per cell reach 2 GiB: N^3 < 2^32); cells out of phase carry 0xFFFFFFFF.  Its volume V is its number of cells;
 *   histogram : counts[b] = the number of regions with edges[b] <= (double)V < edges[b + 1], cells[b] = the sum of V over them, for
 *               the n_bins bins (1 ... ASORA_BUBBLE_MAX_BINS) of the ascending, finite edges[n_bins + 1]; regions with V < edges[0] or
 *               V >= edges[n_bins] are in no bin and counted, in regions and in cells, as underflow and overflow;
 *   tallies   : uint64 [ASORA_REGION_TALLIES], indexed by the enum below: n_phase (cells in phase), n_regions, sum_v2 = sum V^2
 *               (< 2^63 at 645^3), v_largest and label_largest, extent_i / _j / _k (how many of the N planes along the axis hold a cell
 *               of the largest region), v_second and label_second, underflow and overflow in regions and in cells;
 *   largest   : the greatest V, ties to the smaller label; second: the same rule among the other regions, 0 and 0xFFFFFFFF when
 *               there is none.  No cell in phase: every output is 0, the two labels 0xFFFFFFFF.
 * Every output is an integer formed by order-independent operations: two calls return the same bits.
 * labels [N^3] or NULL: the label of every cell, downloaded (tests, visualisation); NULL in production, where some hundred integers
 * cross to the host.  One synchronisation per call.  The labelling keeps 8 bytes per cell on the device (a uint32 label and a uint32
 * volume: 128 MiB at 256^3, 2.0 GiB at N = 645), allocated by the first call and kept until the device is closed.  With
 * ASORA_OPT_TIMING the threshold pass counts under ASORA_KERNEL_BUBBLE_MASK (it is that launch); the other stages are not timed.
 * Fails with code 2 before device_init, 4 for a grid that holds no data or a mesh with N > ASORA_REGION_MAX_N, 3 for: a bad selector,
 * a non-finite threshold, phase not 0 or 1, connectivity not 6 or 26, n_bins outside [1, ASORA_BUBBLE_MAX_BINS], edges not finite or
 * not ascending, a null pointer among edges / counts / cells / tallies.  A refused call writes nothing. */
enum { ASORA_REGION_MAX_N = 645 };
enum { ASORA_REGION_N_PHASE = 0, ASORA_REGION_N_REGIONS = 1, ASORA_REGION_SUM_V2 = 2, ASORA_REGION_V_LARGEST = 3,
       ASORA_REGION_LABEL_LARGEST = 4, ASORA_REGION_EXTENT_I = 5, ASORA_REGION_EXTENT_J = 6, ASORA_REGION_EXTENT_K = 7,
       ASORA_REGION_V_SECOND = 8, ASORA_REGION_LABEL_SECOND = 9, ASORA_REGION_UNDERFLOW = 10, ASORA_REGION_UNDERFLOW_CELLS = 11,
       ASORA_REGION_OVERFLOW = 12, ASORA_REGION_OVERFLOW_CELLS = 13, ASORA_REGION_TALLIES = 14 };
int asora_region_sizes(int which_grid, double threshold, int phase, int periodic, int connectivity, int n_bins, const double *edges,
                       unsigned long long *counts, unsigned long long *cells, unsigned long long *tallies, uint32_t *labels);

/* The topology of the in-phase cells of device grid `which_grid`: the numbers of lattice elements from which
 * the Euler characteristic and the Minkowski functionals follow, and the numbers of components from which the Betti numbers follow.
 * No grid is written.  The specification, which no implementation detail enters:
 *   in phase   : as for asora_bubble_mfp -- phase 0: x >= threshold, phase 1: x < threshold; a NaN is in neither.  The complement is
 *                every cell that is not in phase, NaN cells included;
 *   element    : an anchor (i, j, k) and a set E of the axes along which the element extends: |E| = 0 a vertex, 1 an edge, 2 a face,
 *                3 a cell.  Its incident cells are (i - a, j - b, k - c), where the offset on an axis in E is 0 and the offset on an
 *                axis not in E takes both 0 and 1: a vertex has 8 incident cells, an edge 4, a face 2, a cell 1;
 *   anchors    : periodic != 0: 0 ... N - 1 on every axis, and indices wrap.  periodic == 0: 0 ... N - 1 on the axes in E and 0 ... N
 *                on the others; cells outside the box are out of phase;
 *   counts     : the closed count of a dimension is the number of its elements with AT LEAST ONE incident cell in phase (the complex
 *                of closed cubes: it goes with 26 neighbours), the open count the number with ALL incident cells in phase (it goes
 *                with 6 neighbours).  Both sets are returned whatever `connectivity` is;
 *   tallies    : uint64 [ASORA_TOPO_TALLIES], indexed by the enum below: CELLS (in-phase cells), CLOSED_FACES, CLOSED_EDGES,
 *                CLOSED_VERTICES, OPEN_FACES, OPEN_EDGES, OPEN_VERTICES, COMPONENTS (the regions of the phase under `connectivity`
 *                and `periodic`: n_regions of asora_region_sizes), COMPLEMENT_COMPONENTS (the regions of the complement under the
 *                DUAL connectivity, 6 <-> 26, and the same `periodic`), CAVITIES (periodic == 0: the complement's regions that hold no
 *                cell on a face of the box; periodic != 0: 0).
 * The Euler characteristics (V - E + F - C of the closed counts, C - F + E - V of the open ones), the Minkowski functionals and the
 * Betti numbers are formed by the caller (pyc2ray_amd/topology.py).  N = 1 and 2 with periodic != 0 follow the formula through the
 * wrap (an element then meets a cell more than once) and mean nothing topologically.
 * Every output is an integer formed by order-independent sums: two calls return the same bits.  One synchronisation per call.
 * Device memory: the labelling's 8 bytes per cell (shared with asora_region_sizes) and a second bit mask (2 MiB at 256^3), allocated
 * by the first call and kept until the device is closed.  With ASORA_OPT_TIMING the threshold pass counts under
 * ASORA_KERNEL_BUBBLE_MASK; the other stages are not timed.
 * Fails with code 2 before device_init, 4 for a grid that holds no data or a mesh with N > ASORA_REGION_MAX_N, 3 for: a bad selector,
 * a non-finite threshold, phase not 0 or 1, connectivity not 6 or 26, tallies = NULL.  A refused call writes nothing. */
enum { ASORA_TOPO_CELLS = 0, ASORA_TOPO_CLOSED_FACES = 1, ASORA_TOPO_CLOSED_EDGES = 2, ASORA_TOPO_CLOSED_VERTICES = 3,
       ASORA_TOPO_OPEN_FACES = 4, ASORA_TOPO_OPEN_EDGES = 5, ASORA_TOPO_OPEN_VERTICES = 6, ASORA_TOPO_COMPONENTS = 7,
       ASORA_TOPO_COMPLEMENT_COMPONENTS = 8, ASORA_TOPO_CAVITIES = 9, ASORA_TOPO_TALLIES = 10 };
int asora_topology(int which_grid, double threshold, int phase, int periodic, int connectivity,
                   unsigned long long *tallies /* [ASORA_TOPO_TALLIES] */);

/* The granulometry of the in-phase cells of device grid `which_grid`: the exact squared Euclidean distance
 * transform of the phase, and from it the numbers of cells that survive an erosion and an opening by digital balls of the given
 * radii (Kakiichi et al. 2017).  No grid is written.  The specification, which no implementation detail enters; all integers:
 *   in phase   : as for asora_bubble_mfp -- phase 0: x >= threshold, phase 1: x < threshold; a NaN is in neither;
 *   metric     : d(c, q)^2 = the sum over the axes of the squared index difference; periodic != 0: of the minimum image,
 *                min(d, N - d) per axis; periodic == 0: the plain difference, and the cells of the exterior (index -1 or N on any
 *                axis) are out of phase;
 *   D2(c)      : a uint32 per cell: the minimum of d(c, q)^2 over the out-of-phase cells q (periodic == 0: those of the exterior
 *                included, so D2(c) <= min(x + 1, N - x)^2 on every axis).  Out-of-phase cells have D2 = 0.  Without any out-of-phase
 *                cell -- a periodic box that is all in phase -- every cell holds ASORA_GRAN_UNBOUNDED = 0xFFFFFFFF.  Every finite
 *                value is < 2^20 (N <= ASORA_REGION_MAX_N);
 *   radii      : radii[n_radii], finite, >= 0, strictly ascending, 1 <= n_radii <= ASORA_BUBBLE_MAX_BINS; r2_n = floor(R_n^2) formed
 *                in double, R_n^2 < 2^31.  The digital ball is B_n = {o in Z^3: |o|^2 <= r2_n};
 *   eroded[n]  : the size of E_n = {c: D2(c) > r2_n}, the centres at which the ball lies wholly in the phase;
 *   opened[n]  : the size of O_n = the union of c + B_n over c in E_n = {x: D2'_n(x) <= r2_n}, D2'_n the squared distance to the
 *                nearest cell of E_n in the same metric -- but the exterior of an open box holds no centre and is no source here.
 *                An empty E_n gives 0; the unbounded case gives E_n = all cells and opened[n] = N^3.  Digital balls are no
 *                granulometry in the strict sense: opened[] is NOT always monotone in n, and is returned as counted;
 *   tallies    : uint64 [ASORA_GRAN_TALLIES], indexed by the enum below: N_PHASE (cells in phase), D2_MAX (the largest finite D2, 0
 *                if there is none), N_UNBOUNDED (the cells that hold ASORA_GRAN_UNBOUNDED: 0 or N^3), SUM_D2 (the sum of the finite D2).
 * dist2 [N^3] or NULL: D2 of every cell in C order, downloaded (tests, distance maps); NULL in production, where 2 n_radii + 4
 * integers cross to the host.  Every output is an integer formed by order-independent operations: two calls return the same bits.
 * One synchronisation per call.  Device memory: the labelling's 8 bytes per cell (shared with asora_region_sizes and asora_topology,
 * used one call after the other), a third uint32 per cell and a second bit mask, allocated by the first call and kept until the
 * device is closed.  With ASORA_OPT_TIMING the threshold pass counts under ASORA_KERNEL_BUBBLE_MASK; the other stages are not timed.
 * Fails with code 2 before device_init, 4 for a grid that holds no data or a mesh with N > ASORA_REGION_MAX_N, 3 for: a bad selector,
 * a non-finite threshold, phase not 0 or 1, n_radii outside [1, ASORA_BUBBLE_MAX_BINS], radii not finite, negative, not strictly
 * ascending or with R^2 >= 2^31, a null pointer among radii / eroded / opened / tallies.  A refused call writes nothing. */
enum { ASORA_GRAN_N_PHASE = 0, ASORA_GRAN_D2_MAX = 1, ASORA_GRAN_N_UNBOUNDED = 2, ASORA_GRAN_SUM_D2 = 3, ASORA_GRAN_TALLIES = 4 };
#define ASORA_GRAN_UNBOUNDED 0xFFFFFFFFu
int asora_granulometry(int which_grid, double threshold, int phase, int periodic, int n_radii, const double *radii,
                       unsigned long long *eroded, unsigned long long *opened, unsigned long long *tallies,
                       unsigned *dist2 /* NULL, or host [N^3] */);

/* The spherically averaged power spectrum of one field formed from the device grids, or of two with their cross-spectrum (DESIGN.md
 * section 4.2h): the 21-cm brightness temperature, the neutral fraction, the density.  No grid is written.  The specification, which
 * no implementation detail enters:
 *   field      : selected by a kind (the enum below) and formed per cell c from ASORA_GRID_XH (x), ASORA_GRID_NDENS (n) and
 *                ASORA_GRID_TEMP (T), in double, in the order of operations written here:
 *                  ASORA_PS_XH      g = x
 *                  ASORA_PS_XHI     g = 1 - x
 *                  ASORA_PS_DENSITY g = n / nbar
 *                  ASORA_PS_HI      g = ((scale (1 - x)) (n / nbar)) s,  s = 1 if t_gamma == 0, s = 1 - t_gamma / T if t_gamma > 0
 *                                   (the spin temperature coupled to the kinetic one);
 *                nbar is the mean of ASORA_GRID_NDENS over all cells, formed on the device by a fixed-order sum (correct to an ulp
 *                or two).  scale and t_gamma apply to ASORA_PS_HI only; the differential brightness temperature is ASORA_PS_HI with
 *                the cosmological prefactor as scale;
 *   call       : kind_a, and kind_b = -1 for the auto-spectrum of a alone, or a second kind for b;
 *   transform  : ghat(n) = sum over the N^3 cells c of g(c) exp(-2 pi i n.c / N): unnormalised, numpy's sign and layout
 *                (np.fft.rfftn).  Only the half-space n_z = 0 ... floor(N/2) is stored and binned;
 *   modes      : every index is folded, m = min(n, N - n) per axis; n2 = m_x^2 + m_y^2 + m_z^2, an integer.  The weight w of a
 *                stored mode is 1 if n_z = 0, or if N is even and n_z = N/2; else 2 (the mode and its conjugate partner).  The mode
 *                n = 0 is never binned;
 *   bins       : n_bins in [1, ASORA_BUBBLE_MAX_BINS] and thresholds[n_bins + 1], unsigned integers, non-decreasing, with
 *                thresholds[0] >= 1.  A mode belongs to bin b if thresholds[b] <= n2 < thresholds[b + 1]; anything outside is
 *                dropped.  (A caller with real edges e_b in units of the fundamental mode passes thresholds[b] = ceil(e_b^2); only
 *                integers are compared here);
 *   per bin    : count (uint64) = sum of w, exact; sum_k = sum of w sqrt(n2); sum_aa = sum of w |ahat|^2; with a second field also
 *                sum_bb = sum of w |bhat|^2 and sum_ab = sum of w Re(ahat conj(bhat)).  With kind_b = -1 sum_bb, sum_ab and
 *                moments_b may be NULL and are not written;
 *   per field  : moments[2] = (sum of g, sum of g^2) over the cells.
 * field_out [N^3] or NULL: the formed real field a in C order; modes_out [N N (floor(N/2) + 1)] complex doubles (re, im interleaved,
 * C order) or NULL: ahat.  Both are for tests and for callers who want the brightness-temperature cube; NULL in production, where
 * 5 n_bins + 4 numbers cross to the host.
 * Every floating-point sum (nbar, the moments, the bin sums) is formed in an order that depends on (N, thresholds) only, and no
 * floating-point atomic enters any of them: two calls return the same bits.  One synchronisation per call.
 * Device memory: one complex buffer of N N (floor(N/2) + 1) entries (138 MB at 256^3, 2.15 GB at 645^3), a second one from the first
 * call with kind_b >= 0, the planes' partial bin sums (40 bytes x ASORA_BUBBLE_MAX_BINS x N) and the table of the N roots of unity;
 * allocated by the first call that needs them and kept until the device is closed.  The stages are not timed under
 * ASORA_OPT_TIMING (no ASORA_KERNEL_* slot is free); asora_debug_power_spectrum_ms reports them.
 * Fails with code 2 before device_init; 3 for: a bad kind, a non-finite scale, a non-finite or negative t_gamma, n_bins outside
 * [1, ASORA_BUBBLE_MAX_BINS], thresholds not non-decreasing or thresholds[0] = 0, a null pointer among thresholds / count / sum_k /
 * sum_aa / moments_a or, with kind_b >= 0, sum_bb / sum_ab / moments_b; 4 for a grid the kinds need that holds no data (ASORA_GRID_TEMP
 * is needed by ASORA_PS_HI with t_gamma > 0) and for a mesh with N > ASORA_REGION_MAX_N; 10 for a failed allocation.  A refused call
 * writes nothing. */
enum { ASORA_PS_XH = 0, ASORA_PS_XHI = 1, ASORA_PS_DENSITY = 2, ASORA_PS_HI = 3, ASORA_PS_KINDS = 4 };
int asora_power_spectrum(int kind_a, int kind_b, double scale, double t_gamma, int n_bins, const unsigned *thresholds,
                         unsigned long long *count, double *sum_k, double *sum_aa, double *sum_bb, double *sum_ab,
                         double *moments_a /* [2] */, double *moments_b /* [2] or NULL */,
                         double *field_out /* NULL, or host [N^3] */, double *modes_out /* NULL, or host [2 N N (N/2 + 1)] */);
/* The durations (ms, HIP events on the library's stream) of the stages of the last asora_power_spectrum call that ran with
 * ASORA_OPT_TIMING = 1: ms[0] the mean density, [1] the pass along k with the forming of the field(s), [2] the pass along j, [3] the
 * pass along i, [4] the binning; zeros if no such call has run.  Code 3 for ms = NULL. */
enum { ASORA_PS_STAGES = 5 };
int asora_debug_power_spectrum_ms(double *ms /* [ASORA_PS_STAGES] */);

/* A field formed from the device grids, multiplied by a filter in Fourier space and transformed back, with the one-point statistics
 * of the result: what a telescope of finite resolution would see of the brightness temperature -- a Gaussian
 * beam across the sky, a top-hat along frequency, the mean removed -- or any other filter that is a product of three per-axis tables
 * and a radial one.  The specification, which no implementation detail enters:
 *   field      : g is formed exactly as asora_power_spectrum forms it: the kinds ASORA_PS_*, the same order of operations, the same
 *                mean density; ghat(n) is its unnormalised transform, as there;
 *   filter     : W(n) = ((w_i[n_x] w_j[n_y]) w_k[n_z]) w_r[m2], multiplied in this order, no product contracted into a fused
 *                multiply-add; m = min(n, N - n) per axis is the folded index and m2 = m_x^2 + m_y^2 + m_z^2, an integer.  w_i, w_j,
 *                w_k: [N] each; w_r: [n_r], n_r = 3 floor(N/2)^2 + 1; a NULL table counts as all ones (n_r is not looked at without w_r).  With
 *                subtract_mean != 0 the mode n = 0 is multiplied by 0 instead.  The library indexes tables and multiplies; what a
 *                filter is, is the caller's business.  w_i and w_j must be symmetric as bits, w[n] = w[N - n], 1 <= n < N: the
 *                output would not be real otherwise.  (w_k is read at n_z = 0 ... floor(N/2) only: the stored half-space);
 *   output     : h(c) = N^-3 sum over n of W(n) ghat(n) exp(+2 pi i n.c / N), a real field in the layout of the grids, kept in a
 *                buffer of the library's own; with dst_grid >= 0 it is written into that grid instead, which is allocated as
 *                asora_grid_to_device would allocate it and marked as holding data.  dst_grid may be a grid the kind reads: the whole
 *                forward transform is stream-ordered before the first write.  field_out [N^3] or NULL: h in C order;
 *   stats      : [ASORA_SMOOTH_STATS]: [0] the number of finite cells of h, [1] of non-finite ones (as doubles; exact, N^3 < 2^53);
 *                [2] min and [3] max over the finite cells (+inf and -inf without one); [4] sum g and [5] sum g^2 of the INPUT field,
 *                the moments asora_power_spectrum returns; [6] sum h; [7], [8], [9] the central sums S_p = sum (h - mu)^p, p = 2, 3,
 *                4, with mu = fl([6] / N^3), (h - mu)^3 formed as ((h - mu)(h - mu))(h - mu) and ^4 as the square of the square.
 *                The sums run over every cell (one non-finite cell makes them non-finite) in double-double, in the fixed order of
 *                the power spectrum's moments;
 *   hist       : n_hist in [0, ASORA_SMOOTH_MAX_BINS] bins with edges[n_hist + 1], finite and strictly ascending.  hist[n_hist + 2]:
 *                hist[b] the finite cells with edges[b] <= h < edges[b + 1], hist[n_hist] those below edges[0], hist[n_hist + 1] those
 *                at or above edges[n_hist].  Integers: any order of counting gives the same bits.  With n_hist = 0 edges and hist may
 *                be NULL and are not touched.
 * (One non-finite cell of g makes every cell of h non-finite: the transform mixes all cells.)
 * No floating-point atomic anywhere: the same call returns the same bits.  One synchronisation per call; 10 + n_hist + 2 numbers
 * cross to the host unless field_out is given.  Device memory beside the power spectrum's complex buffer, which is transformed in
 * place and overwritten on the way back: N^3 doubles for h when a call without dst_grid is made, and the tables.
 * Fails with code 2 before device_init; 3 for: a bad kind, a non-finite scale, a non-finite or negative t_gamma, a table with a
 * non-finite entry, w_i or w_j that is not symmetric as bits, w_r with n_r != 3 floor(N/2)^2 + 1, n_hist
 * outside [0, ASORA_SMOOTH_MAX_BINS], edges that are non-finite or do not strictly ascend, NULL edges or hist with n_hist > 0,
 * dst_grid outside -1 ... ASORA_GRID_COUNT - 1, a NULL stats; 4 for a grid the kind needs that holds no data and for a mesh with
 * N > ASORA_REGION_MAX_N; 10 for a failed allocation.  A refused call writes nothing, on the host or on the device. */
enum { ASORA_SMOOTH_STATS = 10, ASORA_SMOOTH_MAX_BINS = 4096 };
int asora_smooth_field(int kind, double scale, double t_gamma,
                       const double *w_i, const double *w_j, const double *w_k,   /* [N] each, or NULL = all ones */
                       const double *w_r, unsigned n_r,                           /* [n_r] or NULL */
                       int subtract_mean,
                       int n_hist, const double *edges,                           /* [n_hist + 1], or n_hist = 0 and NULL */
                       int dst_grid,                                              /* -1, or a grid selector */
                       double *stats, uint64_t *hist, double *field_out);
/* The durations (ms) of the stages of the last asora_smooth_field call that ran with ASORA_OPT_TIMING = 1: ms[0] the mean density,
 * [1] the forward pass along k with the forming of the field, [2] forward along j, [3] forward along i, [4] back along i with the
 * filter, [5] back along j, [6] back along k to the real field with its first statistics, [7] the central moments and the
 * histogram; zeros if no such call has run.  Code 3 for ms = NULL. */
enum { ASORA_SMOOTH_STAGES = 8 };
int asora_debug_smooth_field_ms(double *ms /* [ASORA_SMOOTH_STAGES] */);      /* stage times of the last call made under ASORA_OPT_TIMING */

/* The field of asora_power_spectrum in redshift space -- every cell moved along one axis, the line of sight, by its peculiar
 * velocity -- and the power of that field resolved in direction: binned in (n_perp, n_par) or in (|n|, mu^2), with Legendre-weighted
 * sums for the multipoles P_0, P_2, P_4.  The mapping is the mesh-to-mesh scheme of Mao et al. 2012
 * (MNRAS 422, 926): a number-conserving regridding of every cell between its displaced edges.  The specification, which no
 * implementation detail enters:
 *   field      : g is formed exactly as asora_power_spectrum forms it: the kinds ASORA_PS_*, the same order of operations, the same
 *                mean density;
 *   velocity   : v, N^3 doubles in a buffer of the library's own (asora_los_velocity_to_device; not a grid), the velocity along the
 *                line of sight in the caller's units; velocity_scale converts it to cells; los_axis is 0, 1 or 2.  With
 *                use_velocity = 0 the field stays g, no velocity is needed and velocity_scale is not looked at;
 *   mapping    : each of the N^2 lines along los_axis is handled alone and is periodic.  On a line with the cells q = 0 ... N - 1
 *                every operation below is one IEEE double operation, in the order written; no product is contracted into a fused
 *                multiply-add:
 *                  u[q] = v[q] velocity_scale;  d[q] = 0.5 (u[q - 1] + u[q]), the displacement of the left edge of cell q;
 *                  relative to q, cell q occupies [a, b], a = d[q], b = 1.0 + d[q + 1];  lo = min(a, b), hi = max(a, b),
 *                  width = hi - lo (an inverted cell, a shell crossing, is spread over its absolute extent);
 *                  the weight of cell q on the output cell p = q + o, o an integer:
 *                    width >= 2^-10 : ov = min(hi, o + 1.0) - max(lo, (double)o);  w = ov / width if ov > 0, else 0;
 *                    width <  2^-10 : (a degenerate cell) w = 1 for o == floor(0.5 (lo + hi)), else 0;
 *                  h[p] = the sum over o = -W ... W, ascending, of w(q, o) g[q], q = (p - o) mod N, started from +0.0, each
 *                  product rounded before it is added.
 *                W is any integer >= ceil(max |d|): terms of weight 0 do not change the bits.  The library takes W = floor(max|v|
 *                |velocity_scale|) + 1 and refuses a call with 2 W + 1 > N, in which the window would wrap onto itself.  The sign
 *                convention is s = x + u: a cell with u > 0 moves towards larger indices;
 *   output     : h, a real field in the layout of the grids.  asora_redshift_space_field keeps it in a buffer of the library's own
 *                (the one asora_smooth_field keeps its result in: either call overwrites the other's), or with dst_grid >= 0
 *                writes it into that grid, which is allocated as asora_grid_to_device would allocate it and marked as holding
 *                data; dst_grid may be a grid the kind reads.  moments [2] or NULL: (sum g, sum g^2) of the real-space field;
 *                field_out [N^3] or NULL: h in C order;
 *   transform  : hhat(n), the unnormalised transform of h as in asora_power_spectrum; modes, folding (m = min(n, N - n) per axis),
 *                the weight w of a stored mode and the exclusion of n = 0 are as there.  With los_axis = a: m_par = m[a], n2_perp
 *                the sum of the other two squares, n2 their total;
 *   bins       : two indices, from thr_a[n_a + 1] (unsigned, non-decreasing) and thr_b[n_b + 1] (doubles, finite, non-decreasing),
 *                n_a, n_b >= 1 and n_a n_b <= ASORA_ANISO_MAX_BINS; a mode outside either range is dropped; the arrays are
 *                [n_a][n_b] in C order.
 *                  ASORA_ANISO_CYLINDRICAL : thr_a[ia] <= n2_perp < thr_a[ia + 1] (thr_a[0] = 0 is allowed);
 *                                            thr_b[ib] <= (double)(m_par m_par) < thr_b[ib + 1];
 *                                            sum_1 = sum of w sqrt(n2_perp), sum_2 = sum of w m_par;
 *                  ASORA_ANISO_MU          : thr_a[ia] <= n2 < thr_a[ia + 1], thr_a[0] >= 1;
 *                                            thr_b[ib] n2 <= m_par^2 < thr_b[ib + 1] n2, each product formed in double with one
 *                                            rounding: thr_b holds edges of mu^2, and a last edge above 1 includes mu = 1;
 *                                            sum_1 = sum of w sqrt(n2), sum_2 = sum of w sqrt(m_par^2 / n2).
 *                (For every finite thr_b the index ib of the rounded comparison is monotone along a row of n_z, as the exact one is:
 *                DESIGN.md section 4.2j; no edge is refused for being close to 1.)  Multipoles are ASORA_ANISO_MU with n_b = 1 and
 *                thr_b = {0, 2};
 *   per bin    : count (uint64) = sum of w, exact; sum_aa = sum of w |hhat|^2; sum_l2 = sum of (w |hhat|^2) L2 and sum_l4 = sum of
 *                (w |hhat|^2) L4 with t = (double)m_par^2 / (double)n2, L2 = 0.5 (3.0 t - 1.0), L4 = 0.125 ((35.0 t - 30.0) t + 3.0),
 *                no product contracted;
 *   moments    : moments_real[2] = (sum g, sum g^2), moments_rs[2] = (sum h, sum h^2) over the cells (the same numbers with
 *                use_velocity = 0).
 * field_out [N^3] or NULL: h; modes_out [N N (floor(N/2) + 1)] complex doubles or NULL: hhat; with use_velocity = 0 both have the
 * bytes asora_power_spectrum returns for the same kind.
 * Every floating-point sum has an order fixed by (N, los_axis, mode, thresholds), and no floating-point atomic enters any of them:
 * the same call returns the same bits.  One synchronisation per call.  Device memory beside the power spectrum's complex buffer:
 * N^3 doubles for the velocity, N^3 for h (shared with asora_smooth_field), the planes' partial bin sums (48 bytes x
 * ASORA_ANISO_MAX_BINS x N); kept until the device is closed (the velocity: or until asora_los_velocity_clear).
 * Fail with code 2 before device_init; 3 for: a bad kind, a non-finite scale, a non-finite or negative t_gamma, los_axis outside
 * 0 ... 2, with use_velocity a non-finite velocity_scale, no velocity on the device or 2 W + 1 > N, a bad mode, n_a or n_b < 1 or
 * n_a n_b > ASORA_ANISO_MAX_BINS, thresholds that are not non-decreasing, a non-finite thr_b, thr_a[0] = 0 in mode ASORA_ANISO_MU, a
 * null pointer among the thresholds and the outputs up to moments_rs, dst_grid outside -1 ... ASORA_GRID_COUNT - 1; 4 for a grid the
 * kind needs that holds no data and for a mesh with N > ASORA_REGION_MAX_N; 10 for a failed allocation.  A refused call writes
 * nothing, on the host or on the device. */
enum { ASORA_ANISO_CYLINDRICAL = 0, ASORA_ANISO_MU = 1, ASORA_ANISO_MODES = 2, ASORA_ANISO_MAX_BINS = 1024 };
int asora_power_spectrum_los(int kind, double scale, double t_gamma, int los_axis, int use_velocity, double velocity_scale, int mode,
                             int n_a, const unsigned *thr_a, int n_b, const double *thr_b,
                             unsigned long long *count, double *sum_1, double *sum_2, double *sum_aa, double *sum_l2, double *sum_l4,
                             double *moments_real /* [2] */, double *moments_rs /* [2] */,
                             double *field_out /* NULL, or host [N^3] */, double *modes_out /* NULL, or host [2 N N (N/2 + 1)] */);
int asora_redshift_space_field(int kind, double scale, double t_gamma, int los_axis, int use_velocity, double velocity_scale,
                               int dst_grid /* -1, or a grid selector */, double *moments /* NULL, or [2] */,
                               double *field_out /* NULL, or host [N^3] */);
/* The line-of-sight velocity of the two calls above: N^3 doubles in the layout `order` ('C' or 'F', as asora_grid_to_device) into a
 * buffer of the library's own, which replaces the one of an earlier call.  max |v| is reduced on the device (a maximum does not
 * depend on the order of its operands), kept with the buffer and returned in *max_abs (may be NULL).  Code 2 before device_init; 3
 * for a wrong N, a null pointer, a bad order, and for a NaN or an infinity among the entries, which the same pass over the buffer
 * finds: the velocity of the last good call then stays in place; 10 for a failed allocation.  asora_los_velocity_clear frees the
 * buffer (nothing to do without one); asora_device_close does too. */
int asora_los_velocity_to_device(const double *v, int N, char order, double *max_abs);
int asora_los_velocity_clear(void);
/* The durations (ms) of the stages of the last asora_power_spectrum_los call that ran with ASORA_OPT_TIMING = 1: ms[0] the mean
 * density, [1] the mapping (0 without use_velocity), [2] the pass along k, [3] along j, [4] along i, [5] the binning; zeros if no such
 * call has run.  Code 3 for ms = NULL. */
enum { ASORA_PSLOS_STAGES = 6 };
int asora_debug_power_spectrum_los_ms(double *ms /* [ASORA_PSLOS_STAGES] */);

/* The Lyman-alpha forest of the state: the optical depth tau and the transmitted flux F = exp(-tau) along each of the N^2 lines of one
 * axis, every cell's neutral hydrogen spread over its displaced extent in velocity space and convolved with its thermal Doppler
 * profile; the one-point statistics of F and tau, and the dark gaps.  The specification, which no
 * implementation detail enters:
 *   inputs     : x = ASORA_GRID_XH, n = ASORA_GRID_NDENS, T = ASORA_GRID_TEMP; v, the line-of-sight velocity buffer of
 *                asora_los_velocity_to_device, with use_velocity = 0: u = 0, no velocity is needed and velocity_scale is not looked
 *                at.  velocity_scale: cells per unit of v; b_scale: the Doppler parameter in cells per sqrt(K); tau_scale: the
 *                Gunn-Peterson optical depth per unit neutral density, I_alpha / H(z), I_alpha = pi e^2 f_alpha lambda_alpha /
 *                (m_e c), f_alpha = 0.4164, lambda_alpha = 1215.67 Angstrom;
 *   per line   : each of the N^2 lines along los_axis is periodic with the cells q = 0 ... N - 1 and is handled alone.  Every
 *                operation below is one IEEE double operation, in the order written; nothing is contracted into a fused
 *                multiply-add; erf and exp are the device library's:
 *                  u[q] = v[q] velocity_scale;  d[q] = 0.5 (u[q - 1] + u[q]);  a = d[q], b = 1.0 + d[q + 1] (the edges of
 *                  asora_redshift_space_field);  lo = b < a ? b : a, hi = b < a ? a : b, width = hi - lo;
 *                  bt[q] = b_scale sqrt(T[q]) where that is > 2^-10, else 2^-10 (so for T = 0 and for the NaN of a negative T);
 *                  g[q] = tau_scale ((1.0 - x[q]) n[q]);
 *   weight     : of cell q on the pixel p = q + o, o an integer, at the pixel centre s = (double)o + 0.5:
 *                  width >= 2^-10 : w = 0 if (s - hi) > 6.0 bt or (lo - s) > 6.0 bt, else
 *                                   w = 0.5 (erf((s - lo) / bt) - erf((s - hi) / bt)) / width;
 *                  width <  2^-10 : (a degenerate cell) c = 0.5 (lo + hi), t = (s - c) / bt;  w = 0 if |t| > 6.0, else
 *                                   w = (0.5641895835477563 / bt) exp(-(t t)).
 *                The cut at six Doppler widths is part of the definition: skipping a term beyond it is exact, and the result does
 *                not depend on W once W covers every cell's reach;
 *   tau, F     : tau[p] = the sum over o = -W ... W, ascending, of w(q, o) g[q], q = (p - o) mod N, started from +0.0, each product
 *                rounded before it is added; a term outside the cut, or with g[q] == 0, is left out (so a non-finite g[q] reaches the
 *                pixels inside its cut only);  F[p] = exp(-tau[p]).  tau is sampled at the pixel centres, not averaged over the
 *                pixels: a cell that is narrower than a pixel after the mapping and colder than the distance to the nearest
 *                centre over six lies between two centres and adds to no pixel;
 *   window     : reach[q] = max((6.0 bt - lo) + 0.5, (hi + 6.0 bt) - 0.5).  window > 0 is W, refused if 2 W + 1 > N.  window = 0:
 *                W = max(1, ceil(max_q reach[q])), then capped at (N - 1) / 2; the maximum is reduced on the device (a maximum does
 *                not depend on the order of its operands) and read back by the host, so the automatic form costs one more
 *                synchronisation than the explicit one (two instead of one);
 *   counts     : counts[ASORA_LYA_*]: NONFINITE, the tau that are not finite; WINDOW, the W used; CLIPPED, the cells with
 *                ceil(reach[q]) > W (exact, never silently zero: 0 says that no term was cut off by the window); DEGENERATE, the
 *                cells with width < 2^-10; and the dark gaps below;
 *   statistics : stats[ASORA_LYA_*]: SUM_F and SUM_F2 over the cells, TAU_MIN and TAU_MAX (over the tau that are not NaN; +inf and
 *                -inf if there is none);  pdf[n_bins] (uint64): F binned by edges[n_bins + 1], finite and non-decreasing, n_bins <=
 *                ASORA_LYA_MAX_BINS, or n_bins = 0 with edges and pdf unused: edges[i] <= F < edges[i + 1], a cell outside every
 *                bin (a NaN too) is dropped;
 *   dark gaps  : exact integers.  On each periodic line a gap is a maximal run of pixels with F < gap_threshold; a run through the
 *                end of the line joins the start; a wholly dark line is one gap of length N and adds to FULL_LINES.  gaps[N + 1]
 *                (uint64): the number of gaps by length, gaps[0] = 0;  N_DARK the dark pixels, N_GAPS, LONGEST;
 *   outputs    : tau_out [N^3] and flux_out [N^3] or NULL, in C order.  dst_grid >= 0 writes F (dst_what = ASORA_LYA_FLUX) or tau
 *                (ASORA_LYA_TAU) into that grid under the rules of asora_redshift_space_field: allocated as asora_grid_to_device
 *                would allocate it, marked as holding data, and it may be one of the three grids the call reads.  dst_grid = -1:
 *                dst_what is not looked at.
 * Every floating-point sum has an order fixed by (N, los_axis) and no floating-point atomic enters: the same call returns the same
 * bits.  Device memory: tau lies in the buffer asora_smooth_field and asora_redshift_space_field keep their result in (each call
 * overwrites the others'), unless dst_grid takes it; N^3 doubles more only for flux_out without a grid for F; 64 bytes per workgroup
 * of the line kernel; kept until the device is closed.
 * Fail with code 2 before device_init; 3 for: los_axis outside 0 ... 2, a b_scale or tau_scale that is not finite and > 0, with
 * use_velocity a non-finite velocity_scale or no velocity on the device, a non-finite gap_threshold, n_bins outside 0 ...
 * ASORA_LYA_MAX_BINS, with n_bins > 0 null edges or pdf and edges that are not finite and non-decreasing, null stats, counts or gaps,
 * dst_grid outside -1 ... ASORA_GRID_COUNT - 1, with dst_grid >= 0 a dst_what that is neither, window < 0, 2 window + 1 > N; 4 for
 * one of the three grids without data and for a mesh with N > ASORA_REGION_MAX_N; 10 for a failed allocation.  A refused call writes
 * nothing, on the host or on the device. */
enum { ASORA_LYA_FLUX = 0, ASORA_LYA_TAU = 1, ASORA_LYA_MAX_BINS = 1024 };
enum { ASORA_LYA_SUM_F = 0, ASORA_LYA_SUM_F2 = 1, ASORA_LYA_TAU_MIN = 2, ASORA_LYA_TAU_MAX = 3, ASORA_LYA_STATS = 4 };
enum { ASORA_LYA_NONFINITE = 0, ASORA_LYA_WINDOW = 1, ASORA_LYA_CLIPPED = 2, ASORA_LYA_DEGENERATE = 3, ASORA_LYA_N_DARK = 4,
       ASORA_LYA_N_GAPS = 5, ASORA_LYA_LONGEST = 6, ASORA_LYA_FULL_LINES = 7, ASORA_LYA_COUNTS = 8 };
int asora_lyman_alpha_forest(int los_axis, int use_velocity, double velocity_scale, double b_scale, double tau_scale,
                             int window /* 0: automatic */, double gap_threshold,
                             int n_bins, const double *edges,                     /* [n_bins + 1], or n_bins = 0 and NULL */
                             int dst_grid /* -1, or a grid selector */, int dst_what /* ASORA_LYA_FLUX or ASORA_LYA_TAU */,
                             double *stats /* [ASORA_LYA_STATS] */, unsigned long long *counts /* [ASORA_LYA_COUNTS] */,
                             unsigned long long *pdf /* [n_bins], or NULL */, unsigned long long *gaps /* [N + 1] */,
                             double *tau_out /* NULL, or host [N^3] */, double *flux_out /* NULL, or host [N^3] */);
/* The durations (ms) of the stages of the last asora_lyman_alpha_forest call that ran with ASORA_OPT_TIMING = 1: ms[0] the staging
 * of the lines for the largest reach with its read-back (0 with an explicit window), [1] the optical depth, the flux and -- in the
 * same launch, on the lines where they lie -- the dark gaps, [2] the statistics, [3] the fold of the workgroups' partial results;
 * zeros if no such call has run.  Code 3 for ms = NULL. */
enum { ASORA_LYA_STAGES = 4 };
int asora_debug_lya_forest_ms(double *ms /* [ASORA_LYA_STAGES] */);
/* How asora_lyman_alpha_forest deals the N^2 lines along los_axis of a mesh of N cells a side to its workgroups (a host computation:
 * callable without a device): tiles[0] the lines of a tile, [1] the work items of a workgroup, [2] the workgroups, [3] the bytes of
 * LDS of one.  Code 3 for tiles = NULL, N outside 1 ... ASORA_REGION_MAX_N or los_axis outside 0 ... 2. */
int asora_debug_lya_forest_tiles(int N, int los_axis, int *tiles /* [4] */);

/* The bispectrum of the field of asora_power_spectrum by the FFT triangle estimator: for triangles of
 * k-shells, the sum of ghat(n1) ghat(n2) ghat(n3) over the closed triples of modes and the number of those triples.  No grid is
 * written.  The specification, which no implementation detail enters:
 *   field      : g and ghat(n) are exactly those of asora_power_spectrum: the kinds ASORA_PS_*, the same order of operations, the
 *                same mean density, the unnormalised transform;
 *   shells     : n_shells in [1, ASORA_BISPEC_MAX_SHELLS] and thresholds[n_shells + 1], unsigned integers, non-decreasing, with
 *                thresholds[0] >= 1.  S_a = { n in the full cube of N^3 modes : thresholds[a] <= n2 < thresholds[a + 1] }, with n2 =
 *                m_x^2 + m_y^2 + m_z^2 of the folded indices m = min(n, N - n), as there.  A shell may be empty;
 *   shell field: d_a(c) = N^-3 sum over n in S_a of ghat(n) exp(+2 pi i n.c / N), a real field: what asora_smooth_field returns for a
 *                w_r that is 1 on the shell and 0 elsewhere and no other table (to rounding: columns outside the shell are not
 *                transformed here).  i_a(c) is the same with ghat = 1;
 *   triangles  : n_tri in [1, ASORA_BISPEC_MAX_TRIANGLES] and tri[3 n_tri], the shell indices (a, b, c) of each, in any order, with
 *                repeats within a triangle and duplicates among them allowed (duplicates return equal bytes);
 *   per triangle: sum_ggg[t] = ((S N^3) N^3) with S = the sum over the N^3 cells of (d_a d_b) d_c, the product formed in this order
 *                and not contracted; sum_iii[t] the same of (i_a i_b) i_c.  Mathematically sum_ggg[t] is the sum of ghat(n1)
 *                ghat(n2) ghat(n3) over the ORDERED triples n1 in S_a, n2 in S_b, n3 in S_c with n1 + n2 + n3 = 0 MODULO N on every
 *                axis, and sum_iii[t] is the number of those triples -- an integer, returned as the double the transforms give
 *                (the caller rounds, and sees how far it was from an integer).  Closure is modulo N: once a shell reaches beyond
 *                (N - 1) / 3 in |n|, aliased triangles (n1 + n2 + n3 = a multiple of N that is not 0) are included;
 *   per shell  : count, sum_k and sum_aa are what asora_power_spectrum returns for kind_a = kind, kind_b = -1 and the same
 *                thresholds as bins, bit for bit; moments[2] = (sum of g, sum of g^2) likewise.
 * Every sum over cells is formed in double-double in an order fixed by (N, thresholds, tri) only; no floating-point atomic enters
 * any of them: the same call returns the same bits.  One synchronisation per call; 2 n_tri + 3 n_shells + 2 numbers cross to the host.
 * sum_iii depends on (N, thresholds, tri) only: the values of the last call are kept (the values, not the cubes) and returned
 * without recomputation when those three repeat, as the bytes they were computed as.
 * Device memory beside the power spectrum's complex buffer, which holds the kept spectrum and is only read on the way back: a
 * second complex buffer of N N (floor(N/2) + 1) entries, n_shells cubes of N^3 doubles (134 MB per shell at 256^3: 2.1 GB for 16,
 * 4.3 GB for 32), and 8 KB of partial sums per triangle; allocated by the first call that needs them, the cubes and partials grown
 * by a later call that needs more, kept until the device is closed.
 * Fails with code 2 before device_init; 3 for: a bad kind, a non-finite scale, a non-finite or negative t_gamma, n_shells outside
 * [1, ASORA_BISPEC_MAX_SHELLS], n_tri outside [1, ASORA_BISPEC_MAX_TRIANGLES], a shell index outside [0, n_shells), thresholds not
 * non-decreasing or thresholds[0] = 0, a null pointer; 4 for a grid the kind needs that holds no data and for a mesh with
 * N > ASORA_REGION_MAX_N; 10 for a failed allocation.  A refused call writes nothing. */
enum { ASORA_BISPEC_MAX_SHELLS = 32, ASORA_BISPEC_MAX_TRIANGLES = 8192 };
int asora_bispectrum(int kind, double scale, double t_gamma, int n_shells, const unsigned *thresholds /* [n_shells + 1] */,
                     int n_tri, const int32_t *tri /* [3 n_tri] shell indices */,
                     double *sum_ggg /* [n_tri] */, double *sum_iii /* [n_tri] */,
                     unsigned long long *count, double *sum_k, double *sum_aa /* [n_shells] each */, double *moments /* [2] */);
/* The durations (ms) of the stages of the last asora_bispectrum call that ran with ASORA_OPT_TIMING = 1: ms[0] the mean density,
 * [1], [2], [3] the forward passes along k, j, i, [4] the per-shell binning, [5] the shell fields of g (three passes back per shell),
 * [6] their triple products with the fold, [7] the shell fields of the indicator, [8] their triple products with the fold.  [7] and
 * [8] are 0 for a call that returned the kept counts.  Zeros if no such call has run.  Code 3 for ms = NULL. */
enum { ASORA_BISPEC_STAGES = 9 };
int asora_debug_bispectrum_ms(double *ms /* [ASORA_BISPEC_STAGES] */);
/* How asora_bispectrum's product stage deals n_tri triangles and the N^3 cells (a host computation: callable without a device):
 * out[0] the triangles of one pass over the cubes (the chunk), [1] the passes, [2] the workgroups (a constant), [3] the most and [4]
 * the fewest tiles a workgroup takes (its trips), [5] the triangles a wave accumulates in registers, [6] the cells of a tile, [7]
 * the workgroups that take no tile.  Code 3 for out = NULL or N, n_shells, n_tri outside what asora_bispectrum takes. */
enum { ASORA_BISPEC_PLAN_WORDS = 8 };
int asora_debug_bispectrum_plan(int N, int n_shells, int n_tri, int32_t *out /* [ASORA_BISPEC_PLAN_WORDS] */);

/* Slices of a light cone, emitted while a run advances: along the line of sight the box is seen at another
 * redshift in every plane, so a slice of the cone is a plane of the box interpolated between two consecutive states of the run.  The
 * library knows nothing of cosmology: per slot it keeps one formed field from the previous call, g_prev, and blends planes of it
 * with planes of the field formed from the present grids, g_now.  No grid is written.  The specification, which no implementation
 * detail enters:
 *   slot       : 0 ... ASORA_LC_SLOTS - 1, each with a kept field of its own; slots do not see each other;
 *   field      : g_now(c), per cell c.  With src_grid = -1 it is the field of asora_power_spectrum for `kind` (ASORA_PS_*) with
 *                scale = 1: the same order of operations, the same mean density, so the bits that asora_power_spectrum(kind, -1,
 *                1.0, t_gamma, ..., field_out) returns.  With src_grid a grid selector (and kind = 0) it is that grid's cell
 *                verbatim: a cube that asora_redshift_space_field, asora_smooth_field or asora_lyman_alpha_forest left in a grid
 *                enters a cone this way;
 *   slice t    : t = 0 ... n_slices - 1, n_slices in [0, ASORA_LC_MAX_SLICES].  p = plane[t] in [0, N) is taken along los_axis (0, 1
 *                or 2); planes may come in any order and may repeat (a cone longer than the box wraps).  With (a, b) the indices on
 *                the two remaining axes, in ascending order of the axes, and cell the cell with p on los_axis and (a, b) on those,
 *                  out[t][a][b] = (w_prev[t] g_prev(cell)) + (w_now[t] g_now(cell)):
 *                two products, each rounded, and one sum, nothing contracted into a fused multiply-add.  The weights (0, 1) and
 *                (1, 0) therefore return a field's plane exactly (but for the sign of a zero);
 *   moments    : moments[2 t] = the sum of out over slice t, moments[2 t + 1] = the sum of out^2 (each square rounded), formed in
 *                double-double in an order that depends on N only, no floating-point atomic: two calls return the same bits.  A
 *                sum whose terms overflow is not finite (an infinity or a NaN);
 *   refresh    : 1: after the slices are emitted (stream order) g_prev <- g_now for all N^3 cells, and the slot remembers kind and
 *                src_grid; 0: g_prev is left alone, so that a caller may split one step over several calls and refresh on the last;
 *   first call : a slot without a kept field (never used, forgotten by asora_lightcone_reset, or after asora_device_close) takes
 *                n_slices = 0 and refresh = 1 only: that call allocates the slot's N^3 doubles and stores the field.
 * slices_out [n_slices N N] or NULL: the slices in C order (NULL: only the moments cross to the host, as on the ranks of a
 * multi-rank run that keep no slices).  One synchronisation per call.  Device memory: N^3 doubles per slot in use (134 MB at
 * 256^3), n_slices N^2 doubles of staging for the largest call so far, 0.6 MB of parameters and partial sums, and for
 * ASORA_PS_DENSITY and ASORA_PS_HI the buffers of asora_power_spectrum, whose mean-density launches are used; kept until the device
 * is closed.
 * Fails with code 2 before device_init; 3 for: a slot, kind, src_grid or los_axis out of range, a kind other than 0 with a
 * src_grid, a non-finite or negative t_gamma, n_slices outside [0, ASORA_LC_MAX_SLICES], a refresh other than 0 or 1, with
 * n_slices > 0 a NULL plane, w_prev, w_now or moments, a plane outside [0, N) or a non-finite weight, a call other than the first
 * call above on a slot without a kept field, a kind or src_grid other than the ones the slot's kept field was made with; 4 for a
 * grid the field needs that holds no data (as asora_power_spectrum needs them; src_grid itself) and for a mesh with
 * N > ASORA_REGION_MAX_N; 10 for a failed allocation.  A refused call writes nothing and leaves g_prev as it was. */
enum { ASORA_LC_SLOTS = 4, ASORA_LC_MAX_SLICES = 1024, ASORA_LC_STAGES = 4 };
int asora_lightcone_advance(int slot, int kind, int src_grid, double t_gamma, int los_axis,
                            int n_slices, const int32_t *plane, const double *w_prev, const double *w_now,
                            int refresh, double *slices_out /* NULL, or host [n_slices N N] */,
                            double *moments /* NULL if n_slices == 0, else [2 n_slices] */);
/* What a slot keeps: *has_prev 1 or 0, and with 1 the *kind and *src_grid its field was made with (else 0 and -1).  A host
 * computation, callable without a device.  Code 3 for a bad slot or a null pointer. */
int asora_lightcone_state(int slot, int *has_prev, int *kind, int *src_grid);
/* Forgets the slot's kept field; its memory stays until asora_device_close.  Code 3 for a bad slot. */
int asora_lightcone_reset(int slot);
/* The durations (ms) of the stages of the last asora_lightcone_advance call that ran with ASORA_OPT_TIMING = 1: ms[0] the mean
 * density, [1] the emitting of the slices, [2] their moments, [3] the refresh; zeros if no such call has run.  Code 3 for ms = NULL. */
int asora_debug_lightcone_ms(double *ms /* [ASORA_LC_STAGES] */);

/* The sources of a time step from a halo catalogue, the low-mass haloes suppressed where the gas is ionised (DESIGN.md section 4.1e;
 * Iliev et al. 2007, 2012; Dixon et al. 2016): a catalogue is uploaded once and binned into a table of its occupied cells; every
 * step forms its source list from that table and a device grid (the ionised fraction).  The library knows nothing of cosmology or
 * of photon budgets: the efficiencies g_hm, g_lm and `scale` are the caller's.  No grid is written.  The specification, which no
 * implementation detail enters:
 *   catalogue  : n haloes.  pos [n][3] in cell units, cell c covering [c, c + 1), 0-based; mass [n]; weight [n] >= 0 and finite.
 *                The weight is what is summed, the mass only classifies;
 *   cell       : a halo with a coordinate p that is not finite or has |p| >= 2^31 is dropped and counted in `nonfinite`.  Else
 *                c_a = (int64)floor(p_a) per axis; wrap = 1: c_a <- c_a mod N with the sign of N (Python's %); wrap = 0: a halo
 *                with a c_a outside [0, N) is dropped and counted in `outside`;
 *   population : of the haloes that have a cell, HM if mass >= m_hm, LM if m_lm <= mass < m_hm, else dropped and counted in `below`
 *                (a NaN mass: both comparisons are false).  A halo is counted in the first of the three it meets, in this order;
 *   fixed point: unit = 2^unit_exponent; q = (uint64)rint(weight / unit), the division exact, the rounding to nearest even.  Per
 *                cell Q_hm = sum of q over its HM haloes, Q_lm over its LM ones: integers, so any order gives the same sums.  A cell's
 *                sum differs from the exact one by at most (haloes in the cell) unit / 2;
 *   table      : the cells with Q_hm + Q_lm > 0 in ascending i N^2 + j N + k, each with (cell, Q_hm, Q_lm);
 *   build      : per table row x = grid[cell] of which_grid; suppressed = model != NONE and x > x_suppress (strict; false for a NaN);
 *                s = 1 unless suppressed, then 0 (FULL) or f_suppressed (PARTIAL);
 *                  flux = (g_hm double(Q_hm) + (g_lm s) double(Q_lm)) scale:
 *                the conversions round to nearest even, then three products, each rounded, their sum, rounded, and the product with
 *                scale, rounded; nothing is contracted into a fused multiply-add.  A row is active when flux > 0;
 *   list       : the active rows in table order -- the (x, y, z)-lexicographic order asora_source_data_to_device sorts into --
 *                pos [n_active][3] int32 (0-based i, j, k) and flux [n_active];
 *   summary    : [0] n_active, [1] n_suppressed = the suppressed rows with Q_lm > 0, [2] sum Q_hm over all rows, [3] sum Q_lm over the
 *                rows that are not suppressed, [4] sum Q_lm over the suppressed ones; exact integers (times unit: weights).
 * The device's table, list and summary equal the numpy statement's (tests/halo_sources_reference.py) bit for bit; a permuted
 * catalogue and a repeated call give the same bits; no floating-point atomic enters.
 * asora_halo_catalogue_to_device replaces the catalogue the device holds: counts_out = n_cells, outside, nonfinite, below.  Device
 * memory while it runs: 40 n bytes of catalogue and 16 N^3 of sums (268 MB at 256^3), released before it returns; kept until the
 * next catalogue, asora_halo_catalogue_clear or asora_device_close: 52 bytes per occupied cell.  Three synchronisations.
 * asora_halo_sources_build: one synchronisation, the summary crosses; asora_halo_sources_to_host: the list of the last build, 20
 * n_active bytes; asora_halo_table_to_host: the table (tests); asora_halo_catalogue_state: *n_cells of the catalogue held, -1
 * without one, its *unit_exponent and its *generation -- every catalogue that goes up in the process takes the next number, from
 * 1, so a caller can tell whether the table on the device is still the one it uploaded; 0 without a catalogue (host bookkeeping,
 * callable without a device).  asora_halo_catalogue_clear releases everything the feature holds on the device.
 * Fail with code 2 before device_init; 3 for: n < 0, a null pointer, a NaN threshold or m_lm > m_hm, a wrap other than 0 or 1, a
 * negative or non-finite weight, a unit_exponent outside [-1000, 1000] or one with which sum weight / unit + n / 2 >= 2^62 (a cell's
 * sum could overflow), no catalogue on the device, a model or which_grid out of range, g_hm, g_lm or scale negative or not finite, a
 * NaN x_suppress, an f_suppressed outside [0, 1], a to_host before a build or with too small a capacity; 4 for a grid without
 * data; 10 for a failed allocation.  A catalogue refused for its arguments leaves the one on the device as it was; a call that
 * fails later leaves the device without one. */
enum { ASORA_HALO_MODEL_NONE = 0, ASORA_HALO_MODEL_FULL = 1, ASORA_HALO_MODEL_PARTIAL = 2, ASORA_HALO_STAGES = 8, ASORA_HALO_SUMMARY = 5 };
int asora_halo_catalogue_to_device(const double *pos /* [n][3] */, const double *mass, const double *weight, long long n,
                                   double m_lm, double m_hm, int wrap, int unit_exponent, long long *counts_out /* [4] */);
int asora_halo_catalogue_clear(void);
int asora_halo_catalogue_state(long long *n_cells, int *unit_exponent, long long *generation);
int asora_halo_table_to_host(int64_t *cell, uint64_t *q_hm, uint64_t *q_lm, long long capacity);
int asora_halo_sources_build(int which_grid, double g_hm, double g_lm, double scale, int model, double x_suppress, double f_suppressed,
                             unsigned long long *summary_out /* [ASORA_HALO_SUMMARY] */, long long *n_active);
int asora_halo_sources_to_host(int32_t *pos /* [capacity][3] */, double *flux, long long capacity);
/* The durations (ms) of the stages of the last catalogue call ([0] zeroing and upload, [1] bin, [2] row counts and scan, [3] the
 * download of n_cells, its synchronisation and the allocations sized by it, [4] table) and of the last build ([5] flux, [6] scan,
 * [7] emit) that ran with ASORA_OPT_TIMING = 1; zeros if none has.  Code 3 for NULL. */
int asora_debug_halo_sources_ms(double *ms /* [ASORA_HALO_STAGES] */);

/* ------------------------------------------------------------------------------------------ */
/* C. Options, measurement and diagnostics                                                     */
/* ------------------------------------------------------------------------------------------ */

/* Behaviour options (asora_set_option).  Defaults follow the CUDA library being replaced. */
enum {
    /* 1: sqrt(2)/sqrt(3), 1e-7, 2e30 as the Fortran's single-precision parameters
     *    (src/c2ray/raytracing.f90:368,608-609, photorates.f90:69) and the thin-cell table
     *    argument tau_in (photorates.f90:121);  0 (default): CUDA literals and tau_out
     *    (src/asora/raytracing.cu:15,435,439, rates.cu:7,37). */
    ASORA_OPT_FORTRAN_CONSTANTS = 0,
    /* 1: analytic grey rates (GREY_NOTABLES builds, rates.cu:48-64); 0 (default): tables. */
    ASORA_OPT_GREY_NOTABLES = 1,
    /* 1: record HIP events around each kernel launch (asora_kernel_time_ms). */
    ASORA_OPT_TIMING = 2,
    /* 0: z-faces read/accumulate through the [k][j][i] transposed copies (default 1). */
    ASORA_OPT_Z_TRANSPOSED = 3,
    /* Workgroup size of the raytrace kernel: 0 (default) = chosen from R and the number of sources;
     * 64, 128, 256, 512 or 1024 force it. */
    ASORA_OPT_BLOCK_THREADS = 4,
    /* Decomposition of a source: 0 (default) = chosen from R; 1 = one workgroup per octant;
     * 2 = one per octant and dominant-axis sector (24 per source, diagonal planes re-derived);
     * 3 = one per pair of mirrored sectors (12 per source; rows are full chords of the sphere);
     * 4 = one per quarter of a sector plus the cells it reads (96 per source: a handful of sources);
     * 5 = one per pair of whole octants mirrored in x (4 per source);
     * 6 = ONE workgroup per source: the whole sphere (nothing evaluated twice, every row a full chord, the least padding;
     *     the shell buffers must fit LDS: small radii);
     * 7 = one per half sphere (x and z mirrored, split by the sign of dj: 2 per source);
     * 8 = one per dominant-axis sector with all signs (3 per source);
     * 9 = one per sector and sign of its dominant offset, both transverse axes mirrored (6 per source). */
    ASORA_OPT_SECTORS = 5,
    /* 1: the raytrace also accumulates the photo-heating rate into ASORA_GRID_PHI_HEAT
     *    (src/c2ray/photorates.f90:118,124; src/c2ray/raytracing.f90:532,537); needs heat tables. */
    ASORA_OPT_HEATING = 6,
    /* c2ray_do_all_sources only.  0 (default): every source's rates use the flux of the LAST source, as the
     *    reference does (src/c2ray/raytracing.f90:500,503 pass normflux(NumSrc));  1: each source its own flux. */
    ASORA_OPT_C2RAY_OWN_FLUX = 7,
    /* 1: never take the uniform-temperature form of the tiled chemistry pass (diagnostics / tests: both forms give
     *    bit-identical results).  0 (default): a temperature grid found uniform when uploaded is not read again. */
    ASORA_OPT_NO_UNIFORM_T = 8,
    /* 1: the sub-box raytracer keeps its shell buffers in global memory even when they would fit LDS (tests). */
    ASORA_OPT_SUBBOX_GLOBAL_SHELLS = 9,
    /* 1 (default): asora_do_all_sources overlaps the upload of xh_av, the trace and the download of phi_ion slab by slab
     *    (when all uploaded sources are traced and R is small against the mesh); 0: upload, trace, download in turn. */
    ASORA_OPT_PIPELINED_COPIES = 10,
    /* A rate that is exactly +0 -- a thick cell whose optical depth lies beyond the last table entry, where both lookups
     * return the same value -- need not be added: the grid is bit-identical without it.  The kernels whose rate atomics go
     * through buffer descriptors (table rates, shells in LDS, N <= 512: the production path) exist in a second form that gives
     * such a lane the out-of-range offset of a lane without a rate, so that its atomic never leaves the wave, and in which a
     * wave with nothing to add skips the rate arithmetic; it costs 5 % where no such cell exists and saves a quarter of the
     * launch where two thirds of the pairs lie beyond the table (the benchmark medium at r_RT = 64: -24 %).
     * 0 (default): the library decides -- it takes that form while its probes (the first launch, every 64th after it, sooner
     *    after an upload; read back without waiting) find more than 15 % of the rated pairs dark.
     * 1: always; kernels without buffer atomics take round 2's variant that tests and branches.
     * 2: never: every rated cell is looked up and added, as the reference does (rates.cu:16-41, raytracing.cu:328). */
    ASORA_OPT_SKIP_ZERO_RATES = 11,
    /* 1: the rate atomics are global_atomic_add_f64 under `if (lane has a rate)` even where the grids are small enough for
     *    the default, buffer_atomic_add_f64 through a descriptor over [phi | phi_t] with out-of-range offsets for lanes
     *    without a rate (N <= 512).  Same arithmetic; for A/B runs and the parity test of the two forms. */
    ASORA_OPT_GLOBAL_ATOMICS = 12,
    /* raytrace: one workgroup sweeps its unit for TWO consecutive sources at once (the source-independent geometry is
     * decoded once per lane-step, two dependency chains per wave).  0 = the library decides from the radius and the
     * number of sources (default), 1 = never, 2 = whenever the variant exists (table rates, no heating, shell buffers
     * in LDS, buffer atomics).  Same rates either way, up to the order in which the atomics add them up.  Since round 4
     * the option also governs the tabulated sub-box sweep (ASORA_OPT_SUBBOX_TABLES): photon loss, trailing shell and
     * activity are kept per source, a source that stopped growing is swept along with its partner. */
    ASORA_OPT_PAIR_SOURCES = 13,
    /* c2ray_do_all_sources / asora_subbox_raytrace_device: sweep the sub-boxes on the tabulated geometry of the ASORA
     * kernel (cells within R_max_LLS only: what is rated or lost) instead of generating the cube's geometry on the fly.
     * 0 = the library decides (radius inside the traversal range, enough sources), 1 = never, 2 = whenever the variant
     * exists (table rates, N <= 512).  The source whose column densities are returned always takes the on-the-fly kernel. */
    ASORA_OPT_SUBBOX_TABLES = 14,
    /* 15: rows of the rate grid cut at 64-byte lines: 0 = the library decides (units of one face, i.e. six sectors or twelve
     * sector pairs per source, mesh a multiple of 8, r_RT < 52.5 cells, and a radius that does not change from call to call: after the first change only
     * once a radius has served 32 CALLS in a row -- decided once per call, never per launch), 1 = never, 2 = whenever possible (r_RT <= 110).  The geometry
     * tables then exist in eight forms, by the source's position modulo 8 along the axis that is contiguous in memory for
     * the unit's face; in each, the cells of one row that fall into one 64-byte line of the rate grid never straddle two
     * waves, so every wave's rate atomics leave as whole-line requests (about 8 % fewer requests; the memory side's
     * request rate is what bounds the trace).  Two sources share a workgroup only when they agree modulo 8.  Results are
     * the same sums in a different order. */
    ASORA_OPT_ALIGNED_ROWS = 15,
    /* 1: the geometry tables of the raytrace are built by the host-side builder (geometry.hip: the statement of what a table
     * holds, and the checker of the device-side builder, geometry_device.hip, which is what runs by default and produces the
     * same tables bit for bit -- tests/test_gpu_geometry.py) */
    ASORA_OPT_GEOMETRY_ON_HOST = 16,
    /* How many allocations of the grid arena asora_device_init may try before it keeps the one on which a kernel with the fused
     * pass's stream mix runs fastest (api.hip choose_arena; set BEFORE device_init): 0 (default) = up to 8, 1 = take the first
     * allocation (memory-tight or shared-GPU runs), n = up to n (at most 32).  Whatever the value, what is held during the probe
     * stays within an eighth of the free device memory, and the probe stops once it holds a placement 7 % faster than another.
     * Same results on any placement. */
    ASORA_OPT_PLACEMENT_CANDIDATES = 17,
    /* 1: open (non-periodic) boundaries for the whole-box raytrace.  A cell whose unwrapped position i0 + di, j0 + dj, k0 + dk
     *    lies outside [0, N) on any axis receives no rate from that source and is not counted -- the reference's CUDA kernel
     *    built without -D PERIODIC (in_box_gpu, src/asora/raytracing.cu:264-267).  0 (default): every trace wraps around the box.
     *    Read when a trace or a step of the device loop begins (asora_raytrace_device, asora_raytrace_begin[_planes],
     *    asora_do_all_sources, asora_evolve_begin[_slab[_thermal]]).  The reach stays the periodic window's, offsets
     *    -N/2 ... N/2 - 1 + N % 2 per axis, as in the reference.  Built for table rates through buffer atomics on meshes of
     *    N <= 512; refused with code 4 before anything is launched: larger meshes, ASORA_OPT_GREY_NOTABLES,
     *    ASORA_OPT_GLOBAL_ATOMICS, asora_debug_coldens and the sub-box sweep (c2ray_do_all_sources,
     *    asora_subbox_raytrace_device: the reference's Fortran has no such mode). */
    ASORA_OPT_OPEN_BOUNDARIES = 18,
    ASORA_OPT_COUNT = 19
};
int asora_set_option(int option, int value);
int asora_get_option(int option);

/* Kernel selectors for asora_kernel_time_ms */
enum { ASORA_KERNEL_RAYTRACE = 0, ASORA_KERNEL_CHEMISTRY = 1, ASORA_KERNEL_PREP = 2,
       ASORA_KERNEL_FINISH = 3, ASORA_KERNEL_COUNT = 4 };
/* Selectors appended later: the stages of asora_bubble_mfp.  ASORA_KERNEL_COUNT stays the count of the first four; every selector
 * below ASORA_KERNEL_SLOTS is valid. */
enum { ASORA_KERNEL_BUBBLE_MASK = 4, ASORA_KERNEL_BUBBLE_SCAN = 5, ASORA_KERNEL_BUBBLE_RAYS = 6, ASORA_KERNEL_SLOTS = 7 };
/* Sum of HIP-event durations (ms) and number of launches of a kernel since the last reset,
 * measured on the library's stream (ASORA_OPT_TIMING must be 1). */
int asora_kernel_time_ms(int kernel, double *total_ms, long *launches);
int asora_kernel_time_reset(void);
/* hipDeviceSynchronize on the library's device. */
int asora_synchronize(void);

/* Work accounting of the last raytrace: (source,cell) pairs that received a rate
 * (|d|<=R inside the periodic window: the Gamma-contributing set of raytracing.cu:315), and
 * (source,cell) column-density evaluations actually performed (incl. octant-boundary planes).
 * Point sources only: the cells a plane-parallel flux (asora_plane_flux) rates are not counted. */
int asora_last_raytrace_counts(long long *gamma_cells, long long *evaluated_cells);
/* The same, and how many of the rate-receiving pairs got a rate of exactly +0 that was therefore not added to the grid
 * (ASORA_OPT_SKIP_ZERO_RATES; they are part of gamma_cells). */
int asora_last_raytrace_counts_ex(long long *gamma_cells, long long *evaluated_cells, long long *zero_rates_left_out);

/* Outgoing column density of ONE source over the cells its trace covers, written into a host
 * N^3 grid (zero elsewhere), C-order.  For parity tests of the column density
 * (the reference keeps it in cdh_dev, src/asora/memory.cu:20, and never downloads it). */
int asora_debug_coldens(double R, double sig, double dr, int source_index, double *coldens_out, int N);

/* The device functions every rate goes through (pyc2ray_amd/csrc/rates_device.hpp), evaluated element-wise on host arrays of
 * length n (tests; no reference counterpart): copy in, one kernel on the library's stream that calls the functions themselves,
 * copy out.  op: ASORA_PRIM_*; inputs a ... d as the table says (the others may be null):
 *   LOG2     a = x                                  out = log2_pos(x), no clamp added
 *   LOOKUP   a = tau; which = 0 thick, 1 thin,      out = the interpolated value of table `which` of table set `spectrum`;
 *            2 heat thick, 3 heat thin              out2 = the real table index as formed (integer part + residual)
 *   DIV      a = x, b = y                           out = div_newton(x, y)
 *   MUL ADD  a, b                                   out = mul_unfused(a, b), add_unfused(a, b)
 *   ABSORBER a = n, b = x, c = a, d = b             out = absorber_density(n, x, a, b)
 *   PHOTO HEAT GREY  a = flux, b = cd_in,           out = rate_value(rate_issue(...)), heat_rate_per_atom(...) of table set
 *            c = cd_out, d = vol_nhi                      `spectrum`, grey_rate_per_atom(...)
 * The parameter block is the one a trace gets (sig, minlogtau, dlogtau, NumTau as given; the table length, the index limit,
 * ASORA_OPT_FORTRAN_CONSTANTS and the tables as they stand on the device).  Code 2 before asora_device_init, 3 for an unknown
 * operation or a null array the operation needs, 4 where LOOKUP / PHOTO / HEAT find no (heating) tables or no such table set. */
enum { ASORA_PRIM_LOG2 = 0, ASORA_PRIM_LOOKUP = 1, ASORA_PRIM_DIV = 2, ASORA_PRIM_MUL = 3, ASORA_PRIM_ADD = 4, ASORA_PRIM_ABSORBER = 5,
       ASORA_PRIM_PHOTO = 6, ASORA_PRIM_HEAT = 7, ASORA_PRIM_GREY = 8, ASORA_PRIM_COUNT = 9 };
int asora_debug_rate_primitives(int op, size_t n, const double *a, const double *b, const double *c, const double *d, int which,
                                int spectrum, double sig, double minlogtau, double dlogtau, int NumTau, double *out, double *out2);

/* Which form of the raytrace kernel the last launch took (measurement and tests; no reference counterpart): a bit set of
 * ASORA_VARIANT_* | workgroups per source << 8 | threads per workgroup << 16.  0 before the first launch. */
enum {
    ASORA_VARIANT_PAIRED = 1,             /* two sources per workgroup */
    ASORA_VARIANT_ALIGNED = 2,            /* line-aligned geometry tables (eight forms by source position) */
    ASORA_VARIANT_BUFFER_ATOMICS = 4,     /* rate atomics through buffer descriptors (else global_atomic_add_f64 under a branch) */
    ASORA_VARIANT_SPLIT_DESCRIPTORS = 8,  /* N > 512: one descriptor per layout of the rate grid */
    ASORA_VARIANT_SKIP_ZERO = 16,         /* the form that leaves exact-zero rates out */
    ASORA_VARIANT_GLOBAL_SHELLS = 32,     /* shell buffers in global memory (they exceed LDS) */
    ASORA_VARIANT_OPEN_BOUNDARIES = 64    /* the open-boundary form (ASORA_OPT_OPEN_BOUNDARIES) */
};
int asora_last_raytrace_variant(void);

/* What a raytrace launch would be, from the launcher's own planning functions (pyc2ray_amd/csrc/raytrace_plan.hpp): host only, no
 * device needed.  The options are read as asora_set_option left them (grey opacity, open boundaries and the [k][j][i] twins among
 * them); cu_count <= 0: the device's, 256 before asora_device_init.  flags: ASORA_PLAN_*.  shells < 0: stage 1 only -- out[0 ... 2]
 * = workgroups per source, threads per workgroup, line-aligned tables.  Else, for geometry tables of `shells` shells whose largest
 * holds max_cells cells: out[3 ... 15] the template arguments of raytrace_octant_kernel in their order, out[16] shells in LDS,
 * out[17] dynamic LDS bytes, out[18] the word asora_last_raytrace_variant would report (with ASORA_OPT_SKIP_ZERO_RATES = 0 the
 * probes of a run decide about the exact zeros: planned as kept), out[19] whether that form is built, out[20] whether a form that
 * drops exact zeros exists, out[21] = 1.  A combination the launcher refuses returns its code and message. */
enum { ASORA_PLAN_HEAT = 1, ASORA_PLAN_DUMP = 2, ASORA_PLAN_TABLE_SETS = 4, ASORA_PLAN_HOST_POSITIONS = 8, ASORA_PLAN_RADIUS_STAYS = 16,
       ASORA_PLAN_RATE_TABLES = 32 /* rate tables with a positive step are loaded */, ASORA_PLAN_WORDS = 24 };
int asora_debug_launch_plan(int N, double R, int src_count, int shape_src_count, int cu_count, int flags, int shells, int max_cells,
                            int32_t *out);

/* Which built kernel forms have run (tests; no reference counterpart).  The raytrace kernel is built in the forms of one table
 * (RT_FORMS, pyc2ray_amd/csrc/raytrace_plan.hpp); a row is the kernel's 13 template arguments in their order: THREADS,
 * GLOBAL_SCRATCH, DUMP, HEAT, TABCAP, SKIP_ZERO, GREY, BUFATOM, NSRC, SUBBOX, SPLIT, SPEC, OPEN.
 *   asora_debug_built_forms: the table, 13 ints per row for up to capacity_rows rows; *rows = the rows of the table.  Host only, no
 *     device needed.
 *   asora_debug_form_launches: per row, how many launches of it this process has made (counted once the launch has been accepted by
 *     the runtime); the counters are the process's, not the device state's: they outlive asora_device_close.  Up to `capacity`
 *     counters are written; *rows = the rows of the table.  asora_debug_form_launches_reset sets them to 0.
 *   asora_debug_last_launch_form: the form and the row of the last raytrace launch, whole-box or sub-box sweep on tables, noted
 *     where asora_last_raytrace_variant's word is; *row = -1 (form all 0) before the first launch. */
int asora_debug_built_forms(int32_t *out, int capacity_rows, int *rows);
int asora_debug_form_launches(unsigned long long *counts, int capacity, int *rows);
int asora_debug_form_launches_reset(void);
int asora_debug_last_launch_form(int32_t form[13], int *row);

/* What the last sub-box call (c2ray_do_all_sources, asora_subbox_raytrace_device) launched, written where its launches are made
 * (tests; no reference counterpart).  out[ASORA_SBL_*], ASORA_SUBBOX_LAUNCH_WORDS ints; all 0 before the first call.  Sources are
 * summed over the batches of the call; units ... heat describe the last launch of their kind (one call launches one form of each
 * kind); launches count the sweep launches, one per sub-box round and batch in which anything was swept. */
enum {
    ASORA_SBL_VALID = 0,             /* 1 once a sub-box call has run */
    ASORA_SBL_TABLE_SOURCES = 1,     /* sources swept on tabulated geometry (raytrace.hip, SUBBOX) */
    ASORA_SBL_UNITS = 2,             /* ... workgroups per source (or per two) */
    ASORA_SBL_THREADS = 3,           /* ... threads per workgroup */
    ASORA_SBL_NSRC = 4,              /* ... sources per workgroup, 1 or 2 */
    ASORA_SBL_ALIGNED = 5,           /* ... on line-aligned tables */
    ASORA_SBL_HEAT = 6,              /* ... the form with heating */
    ASORA_SBL_TABLE_LAUNCHES = 7,    /* launches of the tabulated sweep */
    ASORA_SBL_FLY_SOURCES = 8,       /* sources swept by the on-the-fly kernel (subbox.hip) */
    ASORA_SBL_FLY_THREADS = 9,       /* ... threads per workgroup: 128, 256 or 1024 */
    ASORA_SBL_FLY_LDS_SHELLS = 10,   /* ... 1: both shell buffers in LDS, 0: in global memory */
    ASORA_SBL_FLY_HEAT = 11,         /* ... the form with heating */
    ASORA_SBL_FLY_LAUNCHES = 12,     /* launches of the on-the-fly kernel */
    ASORA_SBL_BATCHES = 13,          /* batches the call's sources were swept in */
    ASORA_SUBBOX_LAUNCH_WORDS = 16
};
int asora_debug_last_subbox_launch(int32_t *out);

/* What a sub-box call would launch when nothing about the built geometry intervenes, from the driver's own planning function
 * (plan_subbox, pyc2ray_amd/csrc/raytrace_plan.hpp): host only, no device needed.  A call on a mesh of N cells with `src_count`
 * sources, the last of which returns its column densities when has_dump (c2ray_do_all_sources: 1, asora_subbox_raytrace_device: 0).
 * ASORA_OPT_SUBBOX_TABLES, _PAIR_SOURCES, _ALIGNED_ROWS, _GREY_NOTABLES and _GLOBAL_ATOMICS are read as asora_set_option left
 * them; cu_count <= 0: the device's, 256 before asora_device_init.  out[0] sources on tables, out[1 ... 4] their units, threads,
 * sources per workgroup and line-aligned tables (before the mesh and the host's positions are asked), out[5] sources on the fly,
 * out[6] that kernel's threads, out[7] the last tabulated shell; ASORA_SUBBOX_PLAN_WORDS ints.  Not planned: the fall-backs that
 * need the built tables (shells of one or two sources exceeding LDS) and batching; asora_debug_last_subbox_launch reports what ran. */
enum { ASORA_SUBBOX_PLAN_WORDS = 8 };
int asora_debug_subbox_plan(int N, double R, int max_subbox, int src_count, int has_dump, int heat, int cu_count, int32_t *out);

/* Which workgroup sweeps what in a raytrace launch that is not spread, from the launcher's own functions (block_order,
 * pyc2ray_amd/csrc/raytrace_plan.hpp): host only, no device needed.  pos0: 0-based xyz-interleaved positions of a source list; the
 * launch is of `count` sources from `begin`, `units` workgroups per source, nsrc = 1 or 2 sources per workgroup, line-aligned tables
 * or not.  Block b sweeps out[4 b ... 4 b + 3] = {group, unit, first source, second source or -1}, all -1 for a block that does
 * nothing; blocks b & 7 = x run on XCD x in the order of b.  *grid = the blocks of the launch; where capacity (in blocks) is less,
 * nothing is written.  cu_count <= 0: the device's, 256 before asora_device_init; a launch so small that it is spread instead
 * (<= 2 cu_count workgroups) has no order: *grid = 0. */
int asora_debug_block_order(const int32_t *pos0, int begin, int count, int units, int nsrc, int aligned, int cu_count, int32_t *out,
                            size_t capacity, int *grid);

/* The geometry tables the last raytrace launch used (tests: device-built against host-built tables).  *ntables = tables of the
 * launch shape (units x 8 when line-aligned); for 0 <= table < *ntables: `words` receives 8 uint32 per entry (the 16-byte
 * cell-A and cell-B records, raytrace.hip) for up to capacity_entries entries, *entries the table's entry count, *nsteps its
 * steps, *shells / *max_cells the launch's shell count and zero slot.  table = -1 only reports the counts. */
/* Device memory the geometry tables of the last launch shape occupy (a part shared between tables counts once). */
size_t asora_debug_geometry_bytes(void);
/* How device_init placed the grids (api.hip choose_arena): allocations tried, probe time of the one kept and of the slowest. */
void asora_debug_placement(int *candidates, double *chosen_probe_ms, double *slowest_probe_ms);
/* Host wall clock (ms) of the last asora_device_init and, inside it, of the placement probe (0 when the first allocation was taken). */
void asora_debug_init_cost(double *device_init_ms, double *placement_probe_ms);
/* What the library holds in device and pinned host memory (pyc2ray_amd/csrc/device_memory.hpp).  Host only, no device needed.
 * lifetime 0: the buffers of the mesh, which asora_device_close and a re-initialising asora_device_init release; 1: the buffers
 * of the process, which are never released.  *buffers = the non-empty ones of that lifetime, *bytes = the sum of the sizes they
 * were allocated with.  Code 3 for another lifetime. */
int asora_debug_live_buffers(int lifetime, long long *buffers, unsigned long long *bytes);
int asora_debug_geometry_table(int table, uint32_t *words, size_t capacity_entries, size_t *entries, int *nsteps, int *ntables,
                               int *shells, int *max_cells, int *threads);

/* Which build this is: a hash over every source and header of the library and the compiler flags (pyc2ray_amd/csrc/Makefile),
 * and those flags.  Measurement hygiene, no reference counterpart: the committed counter summaries under profiles/ name the
 * build they were collected on, and bench.py reports `traffic` only from a summary whose id equals this. */
const char *asora_build_id(void);
const char *asora_build_flags(void);

#ifdef __cplusplus
}
#endif
#endif /* ASORA_HIP_H */
