/*
 * oracle/c2ray_oracle.c  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Plain-C, double-precision, single-threaded restatement of the reference
 * algorithm for the pyc2ray hot path (short-characteristics raytracing +
 * photo-ionisation chemistry).  It exists so that the HIP kernels in
 * pyc2ray_amd/csrc can be checked against an independent CPU statement of
 * the same arithmetic.  Only tests/, __graft_entry__.smoke() and the
 * cpu_baseline leg of bench.py may load it; the product path
 * (pyc2ray_amd/*) never imports, links or calls anything in oracle/.
 *
 * Parity pin: this file is validated (tests/test_oracle_vs_reference.py,
 * tests/golden/*.npz) against the reference's own Fortran sources compiled
 * with flang into oracle/_ref/libc2ray_ref.so (see oracle/Makefile).
 *
 * Each function cites the reference file:line it follows
 * (paths relative to the reference checkout).
 *
 * Build:  gcc -O2 -ffp-contract=off -fPIC -shared  (no -ffast-math, no FMA
 * contraction: the Fortran reference is built for baseline x86-64).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* Behaviour switches.  0 = follow the Fortran CPU path literally. */
#define ORACLE_ASORA_CONSTS     1  /* sqrt(2),sqrt(3) decimal literals, 1e-7 / 2e30 as doubles
                                      (src/asora/raytracing.cu:15,435,439; rates.cu:7) instead of
                                      the Fortran single-precision parameters
                                      (src/c2ray/raytracing.f90:368,608-609; photorates.f90:69) */
#define ORACLE_THIN_TAU_OUT     2  /* thin-cell table argument = tau_out (rates.cu:37)
                                      instead of tau_in (photorates.f90:121) */
#define ORACLE_GREY             4  /* analytic grey rates (GREY_NOTABLES builds) */
#define ORACLE_PER_SOURCE_FLUX  8  /* flux[ns] (raytracing.cu:247) instead of the Fortran's
                                      normflux(NumSrc) for every source (raytracing.f90:500,503) */
#define ORACLE_STOPPED_CELLS_LOSE_NOTHING 16
                                   /* Fortran path only: a cell that deposits nothing (beyond R_max_LLS or above
                                      the column-density cap, raytracing.f90:474-478) adds 0 to the photon loss of
                                      its sub-box instead of the stale phi_out (see fctx.stale_phi_out).  This is
                                      the convention of pyc2ray_amd/csrc/subbox.hip and of the tabulated sweep.
                                      The reference leaves the value undefined, so the flag CANNOT be validated
                                      against oracle/_ref wherever it changes a result: it states this library's
                                      convention, nothing more.  Where no stopped cell lies on a box face it
                                      changes nothing, and there the flagged oracle still equals oracle/_ref. */

static const double PI_F90   = 3.14159265358979323846264338;   /* raytracing.f90:47 */
static const double S_STAR   = 1.0e48;                         /* photorates.f90:7  */
static const double EPS_X    = 1e-14;                          /* chemistry.f90:8   */

static inline int pmod(int a, int n) { int r = a % n; return r < 0 ? r + n : r; }
static inline int imin(int a, int b) { return a < b ? a : b; }
static inline int imax(int a, int b) { return a > b ? a : b; }

/* ------------------------------------------------------------------------- */
/* Column-density scratch as seen by the interpolation: any layout.           */
/* ------------------------------------------------------------------------- */
typedef struct {
    const double *cd;
    int   m[3];       /* mesh size per axis                       */
    long  stride[3];  /* element stride per axis                  */
    int   base;       /* 1: coordinates are 1-based (Fortran), 0: C */
} cd_view;

static inline long cd_index(const cd_view *v, int x, int y, int z)
{
    return (long)pmod(x - v->base, v->m[0]) * v->stride[0]
         + (long)pmod(y - v->base, v->m[1]) * v->stride[1]
         + (long)pmod(z - v->base, v->m[2]) * v->stride[2];
}

/*
 * Short-characteristics interpolation of the incoming column density.
 * Follows cinterp, src/c2ray/raytracing.f90:576-815 (== cinterp_gpu,
 * src/asora/raytracing.cu:345-535).  The three reference branches (z, y, x
 * plane crossing) are one generic branch here: d = crossing axis, (e,f) = the
 * two transverse axes in the reference's own pairing (z:(x,y) y:(x,z) x:(y,z));
 * products/sums that differ only by commutation are bit-identical.
 */
static void short_char_interp(const int pos[3], const int src[3], const cd_view *v,
                              double sig, int flags, double *cdensi, double *path)
{
    int del[3], adel[3], sgn[3], pm[3];
    double dd[3];
    for (int ax = 0; ax < 3; ++ax) {
        del[ax]  = pos[ax] - src[ax];
        adel[ax] = abs(del[ax]);
        sgn[ax]  = del[ax] >= 0 ? 1 : -1;          /* sign(1,idel): sign(0)=+1, f90:643-647 */
        pm[ax]   = pos[ax] - sgn[ax];              /* f90:649-651 */
        dd[ax]   = (double)del[ax];
    }
    int d, e, f;                                    /* branch order z, y, x: f90:662,715,764 */
    if (adel[2] >= adel[1] && adel[2] >= adel[0])      { d = 2; e = 0; f = 1; }
    else if (adel[1] >= adel[0] && adel[1] >= adel[2]) { d = 1; e = 0; f = 2; }
    else                                               { d = 0; e = 1; f = 2; }

    /* crossing point on the upstream face, f90:665-671 */
    double alam = ((double)(pm[d] - src[d]) + sgn[d] * 0.5) / dd[d];
    double ec = alam * dd[e] + (double)src[e];
    double fc = alam * dd[f] + (double)src[f];
    double de = 2.0 * fabs(ec - ((double)pm[e] + 0.5 * sgn[e]));
    double df = 2.0 * fabs(fc - ((double)pm[f] + 0.5 * sgn[f]));

    /* bilinear weights, f90:673-676 */
    double s1 = (1. - de) * (1. - df);
    double s2 = (1. - df) * de;
    double s3 = (1. - de) * df;
    double s4 = de * df;

    /* the four upstream corners, f90:678-689 */
    int q[3];
    q[d] = pm[d];
    q[e] = pm[e];  q[f] = pm[f];   double c1 = v->cd[cd_index(v, q[0], q[1], q[2])];
    q[e] = pos[e]; q[f] = pm[f];   double c2 = v->cd[cd_index(v, q[0], q[1], q[2])];
    q[e] = pm[e];  q[f] = pos[f];  double c3 = v->cd[cd_index(v, q[0], q[1], q[2])];
    q[e] = pos[e]; q[f] = pos[f];  double c4 = v->cd[cd_index(v, q[0], q[1], q[2])];

    /* optical-depth weighting, weightf f90:807-813 */
    double w1 = s1 * (1.0 / fmax(0.6, c1 * sig));
    double w2 = s2 * (1.0 / fmax(0.6, c2 * sig));
    double w3 = s3 * (1.0 / fmax(0.6, c3 * sig));
    double w4 = s4 * (1.0 / fmax(0.6, c4 * sig));

    double cdi = (c1 * w1 + c2 * w2 + c3 * w3 + c4 * w4) / (w1 + w2 + w3 + w4);   /* f90:697 */

    /* cells diagonally adjacent to the source, f90:701-707 */
    if (adel[d] == 1 && (adel[e] == 1 || adel[f] == 1)) {
        double r3 = (flags & ORACLE_ASORA_CONSTS) ? 1.73205080757 : (double)sqrtf(3.0f);  /* f90:608 */
        double r2 = (flags & ORACLE_ASORA_CONSTS) ? 1.41421356237 : (double)sqrtf(2.0f);  /* f90:609 */
        cdi = (adel[e] == 1 && adel[f] == 1) ? r3 * cdi : r2 * cdi;
    }
    *cdensi = cdi;
    *path = sqrt((dd[e] * dd[e] + dd[f] * dd[f]) / (dd[d] * dd[d]) + 1.0);         /* f90:710 */
}

/* ------------------------------------------------------------------------- */
/* Rates                                                                      */
/* ------------------------------------------------------------------------- */
typedef struct {
    const double *thin, *thick, *hthin, *hthick;
    double minlogtau, dlogtau;
    int NumTau;      /* value the caller passes (may equal table_len, see below) */
    int table_len;   /* true number of elements; indices are clamped to table_len-1.
                        The reference reads one past the end when NumTau==len and
                        tau >= 10^maxlogtau (photorates.f90:140-146, rates.cu:78-82);
                        the clamp is this build's defined behaviour there. */
} rate_tables;

/* photo_lookuptable, src/c2ray/photorates.f90:130-147 (rates.cu:70-83) */
static double table_lookup(const double *table, double tau, const rate_tables *t)
{
    double logtau = log10(fmax(1.0e-20, tau));
    double real_i = fmin((double)(float)t->NumTau,
                         fmax(0.0, 1.0 + (logtau - t->minlogtau) / t->dlogtau));
    int i0 = (int)real_i;
    int i1 = imin(t->NumTau, i0 + 1);
    double residual = real_i - (double)i0;
    int last = t->table_len - 1;
    if (i0 > last) i0 = last;
    if (i1 > last) i1 = last;
    return table[i0] + residual * (table[i1] - table[i0]);
}

/* photoion_rates, photorates.f90:62-125 (rates.cu:16-41);
 * photoion_rates_test (grey), photorates.f90:13-57 (rates.cu:48-64). */
static void photo_rates(double normflux, double cd_in, double cd_out, double vfact, double sig,
                        const rate_tables *t, int flags,
                        double *phi_cell, double *phi_out, double *heat_cell)
{
    double limit = (flags & ORACLE_ASORA_CONSTS) ? 1.0e-7 : (double)1.0e-7f;   /* f90:69 */
    double tau_in = cd_in * sig, tau_out = cd_out * sig;
    if (flags & ORACLE_GREY) {
        double prefact = normflux * S_STAR / vfact;
        double phi_in = prefact * exp(-tau_in);
        if (fabs(tau_out - tau_in) > limit) {
            *phi_out = prefact * exp(-tau_out);
            *phi_cell = phi_in - *phi_out;
        } else {
            *phi_cell = prefact * (tau_out - tau_in) * exp(-tau_in);
            *phi_out = phi_in - *phi_cell;
        }
        *heat_cell = 0.0;
        return;
    }
    double prefact = normflux / vfact;
    double phi_in = prefact * table_lookup(t->thick, tau_in, t);
    if (fabs(tau_out - tau_in) > limit) {
        *phi_out = prefact * table_lookup(t->thick, tau_out, t);
        *phi_cell = phi_in - *phi_out;
        *heat_cell = t->hthick
            ? prefact * (table_lookup(t->hthick, tau_in, t) - table_lookup(t->hthick, tau_out, t)) : 0.0;
    } else {
        double targ = (flags & ORACLE_THIN_TAU_OUT) ? tau_out : tau_in;
        *phi_cell = prefact * (tau_out - tau_in) * table_lookup(t->thin, targ, t);
        *phi_out = phi_in - *phi_cell;
        /* (heating at the photo rate's optical depth: the Fortran's tau_in, photorates.f90:124; tau_out where the photo
            rate takes it, as this library's HEAT kernels do in their default constants) */
        *heat_cell = t->hthin ? prefact * (tau_out - tau_in) * table_lookup(t->hthin, targ, t) : 0.0;
    }
}

/* ------------------------------------------------------------------------- */
/* Fortran CPU path: do_all_sources / do_source / evolve2D / evolve0D         */
/* Arrays are Fortran-ordered (m1,m2,m3); srcpos is (3,NumSrc) column-major,  */
/* 1-based.                                                                   */
/* ------------------------------------------------------------------------- */
typedef struct {
    const double *normflux; const int32_t *srcpos; int NumSrc;
    double *coldens; const double *ndens; const double *xh_av;
    double *phi_ion; double *phi_heat;
    double sig, dr, R;
    rate_tables tab; int flags;
    int m[3];
    double loss;          /* photon_loss_src                                  */
    double stale_phi_out; /* the reference leaves phi_ion_out undefined when a
                             cell is beyond R or above max_coldensh
                             (raytracing.f90:408,495-519,543); we carry the last
                             defined value, which is what a reused stack slot
                             does.  Tests only compare photon_loss where no
                             stopped cell lies on a sub-box boundary, or under
                             ORACLE_STOPPED_CELLS_LOSE_NOTHING (0 instead).    */
} fctx;

/* evolve0D, src/c2ray/raytracing.f90:347-567 */
static void f_cell(fctx *c, const int rt[3], const int src[3], int ns,
                   const int last_l[3], const int last_r[3])
{
    int p0 = pmod(rt[0] - 1, c->m[0]), p1 = pmod(rt[1] - 1, c->m[1]), p2 = pmod(rt[2] - 1, c->m[2]);
    long idx = p0 + (long)c->m[0] * (p1 + (long)c->m[1] * p2);
    double xh = c->xh_av[idx];
    double nHI = c->ndens[idx] * (1.0 - xh);
    if (c->coldens[idx] != 0.0) return;                              /* f90:426 */

    double cd_in, path, vol;
    int stop = 0;
    if (rt[0] == src[0] && rt[1] == src[1] && rt[2] == src[2]) {     /* f90:430-439 */
        cd_in = 0.0;
        path = 0.5 * c->dr;
        vol = c->dr * c->dr * c->dr;
    } else {
        cd_view v = { c->coldens, { c->m[0], c->m[1], c->m[2] },
                      { 1, c->m[0], (long)c->m[0] * c->m[1] }, 1 };
        short_char_interp(rt, src, &v, c->sig, c->flags, &cd_in, &path);
        path = path * c->dr;
        double xs = c->dr * (double)(rt[0] - src[0]);
        double ys = c->dr * (double)(rt[1] - src[1]);
        double zs = c->dr * (double)(rt[2] - src[2]);
        double dist2 = xs * xs + ys * ys + zs * zs;
        vol = dist2 * path * (4.0 * PI_F90);                          /* f90:457 */
        if (dist2 / (c->dr * c->dr) > c->R * c->R) stop = 1;          /* f90:474 */
        double maxcd = (c->flags & ORACLE_ASORA_CONSTS) ? 2e30 : (double)2e30f;   /* f90:368 */
        if (cd_in > maxcd) stop = 1;                                  /* f90:478 */
    }
    double cd_out = cd_in + nHI * path;                               /* f90:488 */
    c->coldens[idx] = cd_out;

    double phi = 0.0, heat = 0.0;
    double phi_out = (c->flags & ORACLE_STOPPED_CELLS_LOSE_NOTHING) ? 0.0 : c->stale_phi_out;
    if (!stop) {
        double flux = (c->flags & ORACLE_PER_SOURCE_FLUX) ? c->normflux[ns]
                                                          : c->normflux[c->NumSrc - 1];  /* f90:500,503 */
        photo_rates(flux, cd_in, cd_out, vol, c->sig, &c->tab, c->flags, &phi, &phi_out, &heat);
        c->stale_phi_out = phi_out;
    }
    phi = phi / nHI;                                                  /* f90:531-532 */
    heat = heat / nHI;
    c->phi_ion[idx] += phi;
    if (c->phi_heat) c->phi_heat[idx] += heat;

    /* sub-box photon loss, f90:541-543 */
    int on_edge = 0;
    for (int ax = 0; ax < 3; ++ax)
        if (rt[ax] == last_l[ax] || rt[ax] == last_r[ax]) on_edge = 1;
    if (on_edge) c->loss += phi_out * (c->dr * c->dr * c->dr);
}

/* evolve2D, raytracing.f90:258-340 : one z-plane, four quadrant sweeps */
static void f_plane(fctx *c, int k, const int src[3], int ns, const int last_l[3], const int last_r[3])
{
    int rt[3]; rt[2] = k;
    for (int jdir = 0; jdir < 2; ++jdir) {
        int j0 = jdir == 0 ? src[1] : src[1] - 1;
        int j1 = jdir == 0 ? last_r[1] : last_l[1];
        int js = jdir == 0 ? 1 : -1;
        for (int j = j0; js > 0 ? j <= j1 : j >= j1; j += js) {
            rt[1] = j;
            for (int i = src[0]; i <= last_r[0]; ++i)     { rt[0] = i; f_cell(c, rt, src, ns, last_l, last_r); }
            for (int i = src[0] - 1; i >= last_l[0]; --i) { rt[0] = i; f_cell(c, rt, src, ns, last_l, last_r); }
        }
    }
}

/* do_source, raytracing.f90:127-249 (built with -DUSE_SUBBOX, src/c2ray/Makefile:3) */
static void f_source(fctx *c, int ns, int max_subbox, int subboxsize, float loss_fraction,
                     int *sum_nbox, double *photon_loss)
{
    int src[3], lastpos_l[3], lastpos_r[3], last_l[3], last_r[3];
    int m1 = c->m[0];
    for (int ax = 0; ax < 3; ++ax) {
        src[ax] = c->srcpos[3 * ns + ax];
        lastpos_r[ax] = src[ax] + imin(max_subbox, m1 / 2 - 1 + m1 % 2);   /* f90:174 */
        lastpos_l[ax] = src[ax] - imin(max_subbox, m1 / 2);               /* f90:175 */
        last_r[ax] = last_l[ax] = src[ax];
    }
    memset(c->coldens, 0, sizeof(double) * (size_t)c->m[0] * c->m[1] * c->m[2]);   /* f90:181 */

    int nbox = 0;
    c->loss = c->normflux[ns] * S_STAR;
    while (c->loss > (double)loss_fraction * c->normflux[ns] * S_STAR
           && last_r[2] < lastpos_r[2] && last_l[2] > lastpos_l[2]) {        /* f90:193-195 */
        c->loss = 0.0;
        nbox += 1;
        for (int ax = 0; ax < 3; ++ax) {
            last_r[ax] = imin(src[ax] + subboxsize * nbox, lastpos_r[ax]);
            last_l[ax] = imax(src[ax] - subboxsize * nbox, lastpos_l[ax]);
        }
        for (int k = src[2]; k <= last_r[2]; ++k)     f_plane(c, k, src, ns, last_l, last_r);
        for (int k = src[2] - 1; k >= last_l[2]; --k) f_plane(c, k, src, ns, last_l, last_r);
    }
    *sum_nbox += nbox;
    *photon_loss += c->loss;
}

/* do_all_sources, raytracing.f90:52-119.  nbox_per_source (optional, NumSrc ints): the sub-boxes each source was traced
 * in (tests state conditions on their inputs with it: which sources stop before the range ends). */
void oracle_do_all_sources_boxes(const double *normflux, const int32_t *srcpos, int max_subbox, int subboxsize,
                           double *coldensh_out, double sig, double dr, const double *ndens,
                           const double *xh_av, double *phi_ion, double *phi_heat, float loss_fraction,
                           const double *thin, const double *thick, const double *hthin, const double *hthick,
                           double minlogtau, double dlogtau, double R_max_LLS,
                           int NumTau, int table_len, int NumSrc, int m1, int m2, int m3, int flags,
                           int *sum_nbox, double *photon_loss, int *nbox_per_source)
{
    fctx c;
    memset(&c, 0, sizeof c);
    c.normflux = normflux; c.srcpos = srcpos; c.NumSrc = NumSrc;
    c.coldens = coldensh_out; c.ndens = ndens; c.xh_av = xh_av;
    c.phi_ion = phi_ion; c.phi_heat = phi_heat;
    c.sig = sig; c.dr = dr; c.R = R_max_LLS; c.flags = flags;
    c.tab.thin = thin; c.tab.thick = thick; c.tab.hthin = hthin; c.tab.hthick = hthick;
    c.tab.minlogtau = minlogtau; c.tab.dlogtau = dlogtau; c.tab.NumTau = NumTau; c.tab.table_len = table_len;
    c.m[0] = m1; c.m[1] = m2; c.m[2] = m3;
    size_t n = (size_t)m1 * m2 * m3;
    memset(phi_ion, 0, n * sizeof(double));                            /* f90:95 */
    *sum_nbox = 0; *photon_loss = 0.0;
    for (int ns = 0; ns < NumSrc; ++ns) {
        int before = *sum_nbox;
        f_source(&c, ns, max_subbox, subboxsize, loss_fraction, sum_nbox, photon_loss);
        if (nbox_per_source) nbox_per_source[ns] = *sum_nbox - before;
    }
}

/* (a function of its own above, so that the ABI of oracle_do_all_sources stays) */
void oracle_do_all_sources(const double *normflux, const int32_t *srcpos, int max_subbox, int subboxsize,
                           double *coldensh_out, double sig, double dr, const double *ndens,
                           const double *xh_av, double *phi_ion, double *phi_heat, float loss_fraction,
                           const double *thin, const double *thick, const double *hthin, const double *hthick,
                           double minlogtau, double dlogtau, double R_max_LLS,
                           int NumTau, int table_len, int NumSrc, int m1, int m2, int m3, int flags,
                           int *sum_nbox, double *photon_loss)
{
    oracle_do_all_sources_boxes(normflux, srcpos, max_subbox, subboxsize, coldensh_out, sig, dr, ndens, xh_av, phi_ion,
                                phi_heat, loss_fraction, thin, thick, hthin, hthick, minlogtau, dlogtau, R_max_LLS,
                                NumTau, table_len, NumSrc, m1, m2, m3, flags, sum_nbox, photon_loss, NULL);
}

/* ------------------------------------------------------------------------- */
/* ASORA GPU path restated serially: do_all_sources_gpu + evolve0D_gpu        */
/* src/asora/raytracing.cu:79-339.  Arrays are C-ordered flat                 */
/* (idx = N*N*i + N*j + k, raytracing.cu:30); src_pos is 0-based,             */
/* xyz-interleaved (pyc2ray/utils/sourceutils.py:30).                         */
/* The reference maps a linear thread index to a shell cell                   */
/* (raytracing.cu:39-59,228-238); the set of cells with |di|+|dj|+|dk| = q is */
/* enumerated directly here, order inside a shell being irrelevant            */
/* (same-shell neighbours carry exactly zero weight).                         */
/* coldens_dump (optional, N^3): receives the outgoing column density of the  */
/* LAST source processed (cells it visited), for column-density parity tests. */
/* ------------------------------------------------------------------------- */
static void a_cell(int di, int dj, int dk, const int s0[3], double flux, double R, double sig, double dr,
                   const double *ndens, const double *xh_av, double *phi_ion, double *phi_heat, double *scratch,
                   int N, const rate_tables *tab, int flags, int last_l, int last_r, long *visited)
{
    if (di < last_l || di > last_r || dj < last_l || dj > last_r || dk < last_l || dk > last_r) return; /* cu:241 */
    int i = di + s0[0], j = dj + s0[1], k = dk + s0[2];
    long idx = ((long)N * pmod(i, N) + pmod(j, N)) * N + pmod(k, N);
    double xh = xh_av[idx];
    double nHI = ndens[idx] * (1.0 - xh);                              /* cu:275-276 */
    double cd_in, path, vol, dist2;
    if (di == 0 && dj == 0 && dk == 0) {                                /* cu:285-294 */
        cd_in = 0.0; path = 0.5 * dr; vol = dr * dr * dr; dist2 = 0.0;
    } else {
        int pos[3] = { i, j, k };
        cd_view v = { scratch, { N, N, N }, { (long)N * N, N, 1 }, 0 };
        short_char_interp(pos, s0, &v, sig, flags, &cd_in, &path);
        path *= dr;
        double xs = dr * (i - s0[0]), ys = dr * (j - s0[1]), zs = dr * (k - s0[2]);
        dist2 = xs * xs + ys * ys + zs * zs;
        vol = dist2 * path * 12.566370614359172463991853874177;        /* cu:12,307 */
    }
    double cd_out = cd_in + nHI * path;                                 /* cu:311-312 */
    scratch[idx] = cd_out;
    if (visited) ++*visited;
    double maxcd = (flags & ORACLE_ASORA_CONSTS) ? 2e30 : (double)2e30f;
    if (cd_in <= maxcd && dist2 / (dr * dr) <= R * R) {                 /* cu:315 */
        double phi, phi_out, heat;
        photo_rates(flux, cd_in, cd_out, vol, sig, tab, flags, &phi, &phi_out, &heat);
        phi_ion[idx] += phi / nHI;                                      /* cu:324,328 */
        if (phi_heat) phi_heat[idx] += heat / nHI;                      /* (no heating in the CUDA library) */
    }
}

/* oracle_asora_do_all_sources with heating.  hthin, hthick, phi_heat (optional, all three or none): heating tables and the
 * heating rate per HI atom, accumulated like the photo-ionisation rate (this library's HEAT kernels, raytrace.hip): the same
 * table index and residual, thin cells looked up at the same optical depth as the photo rate (tau_out with
 * ORACLE_THIN_TAU_OUT, tau_in otherwise).  A function of its own, so that the ABI of oracle_asora_do_all_sources stays. */
void oracle_asora_do_all_sources_heat(double R, double sig, double dr, const double *ndens, const double *xh_av,
                                      double *phi_ion, const int32_t *src_pos, const double *src_flux,
                                      int NumSrc, int N, const double *thin, const double *thick,
                                      double minlogtau, double dlogtau, int NumTau, int table_len, int flags,
                                      double *coldens_dump, long *cells_visited,
                                      const double *hthin, const double *hthick, double *phi_heat)
{
    size_t n = (size_t)N * N * N;
    if (!phi_heat) hthin = hthick = NULL;
    rate_tables tab = { thin, thick, hthin, hthick, minlogtau, dlogtau, NumTau, table_len };
    int max_q = (int)ceil(1.73205080757 * fmin(R, 1.73205080757 * N / 2.0));   /* cu:14,101 */
    int last_r = N / 2 - 1 + pmod(N, 2);                                       /* cu:122 */
    int last_l = -(N / 2);                                                     /* cu:123 */
    double *scratch = coldens_dump ? coldens_dump : (double *)calloc(n, sizeof(double));
    if (coldens_dump) memset(coldens_dump, 0, n * sizeof(double));
    memset(phi_ion, 0, n * sizeof(double));                                    /* cu:113 */
    if (phi_heat) memset(phi_heat, 0, n * sizeof(double));
    long visited = 0;
    for (int ns = 0; ns < NumSrc; ++ns) {
        int s0[3] = { src_pos[3 * ns], src_pos[3 * ns + 1], src_pos[3 * ns + 2] };
        double flux = (flags & ORACLE_PER_SOURCE_FLUX) ? src_flux[ns] : src_flux[NumSrc - 1];
        if (coldens_dump && ns == NumSrc - 1) memset(coldens_dump, 0, n * sizeof(double));
        for (int q = 0; q <= max_q; ++q) {                                     /* cu:198 */
            for (int di = -q; di <= q; ++di) {
                int rem = q - abs(di);
                for (int dj = -rem; dj <= rem; ++dj) {
                    int dk = rem - abs(dj);
                    a_cell(di, dj, dk, s0, flux, R, sig, dr, ndens, xh_av, phi_ion, phi_heat, scratch, N, &tab,
                           flags, last_l, last_r, &visited);
                    if (dk != 0)
                        a_cell(di, dj, -dk, s0, flux, R, sig, dr, ndens, xh_av, phi_ion, phi_heat, scratch, N, &tab,
                               flags, last_l, last_r, &visited);
                }
            }
        }
    }
    if (cells_visited) *cells_visited = visited;
    if (!coldens_dump) free(scratch);
}

void oracle_asora_do_all_sources(double R, double sig, double dr, const double *ndens, const double *xh_av,
                                 double *phi_ion, const int32_t *src_pos, const double *src_flux,
                                 int NumSrc, int N, const double *thin, const double *thick,
                                 double minlogtau, double dlogtau, int NumTau, int table_len, int flags,
                                 double *coldens_dump, long *cells_visited)
{
    oracle_asora_do_all_sources_heat(R, sig, dr, ndens, xh_av, phi_ion, src_pos, src_flux, NumSrc, N, thin, thick,
                                     minlogtau, dlogtau, NumTau, table_len, flags, coldens_dump, cells_visited,
                                     NULL, NULL, NULL);
}

/* ------------------------------------------------------------------------- */
/* Chemistry: doric / do_chemistry / evolve0D_global / global_pass            */
/* src/c2ray/chemistry.f90                                                    */
/* ------------------------------------------------------------------------- */

/* doric, chemistry.f90:221-316 */
void oracle_doric(double xh_old, double dt, double temp_p, double rhe, double phi_p,
                  double bh00, double albpow, double colh0, double temph0, double clumping,
                  double *xh, double *xh_av)
{
    double brech0 = clumping * bh00 * pow(temp_p / 1e4, albpow);       /* f90:257 */
    double sqrtt0 = sqrt(temp_p);
    double acolh0 = colh0 * sqrtt0 * exp(-temph0 / temp_p);            /* f90:261-262 */
    double aih0 = phi_p + rhe * acolh0;                                /* f90:279 */
    double delth = aih0 + rhe * brech0;
    double eqxh = aih0 / delth;
    double deltht = delth * dt;
    double ee = exp(-deltht);
    double x = (xh_old - eqxh) * ee + eqxh;                            /* f90:285 */
    if (x < EPS_X) x = EPS_X;
    double avg = (deltht < (double)1.0e-8f) ? 1.0 : (1.0 - ee) / deltht;   /* f90:299-303 */
    double xa = eqxh + (xh_old - eqxh) * avg;                          /* f90:306 */
    if (xa < EPS_X) xa = EPS_X;
    *xh = x; *xh_av = xa;
}

/* do_chemistry, chemistry.f90:117-204.  Returns the iteration count. */
int oracle_do_chemistry(double dt, double ndens_p, double temperature, double xh_p,
                        double *xh_av_p, double *xh_intermed_p, double phi_ion_p,
                        double bh00, double albpow, double colh0, double temph0, double abu_c)
{
    const double min_frac_change = (double)1.0e-3f;                    /* f90:9  */
    const double min_frac_atoms  = (double)1.0e-8f;                    /* f90:10 */
    double t_end = temperature, t_prev;
    int nit = 0;
    for (;;) {
        nit += 1;
        t_prev = t_end;
        double xav_old = *xh_av_p;
        double de = ndens_p * (*xh_av_p + abu_c);                      /* f90:162 */
        oracle_doric(xh_p, dt, t_end, de, phi_ion_p, bh00, albpow, colh0, temph0, 1.0,
                     xh_intermed_p, xh_av_p);
        if ((fabs((*xh_av_p - xav_old) / (1.0 - *xh_av_p)) < min_frac_change
             || (1.0 - *xh_av_p < min_frac_atoms))
            && (fabs((t_end - t_prev) / t_end) < min_frac_change))     /* f90:182-187 */
            break;
        if (nit > 400) break;                                          /* f90:192 */
    }
    return nit;
}

/* global_pass + evolve0D_global, chemistry.f90:13-110.  Elementwise, so the
 * storage order of the grids is irrelevant as long as all share it. */
void oracle_global_pass(double dt, const double *ndens, const double *temp, const double *xh,
                        double *xh_av, double *xh_intermed, const double *phi_ion,
                        double bh00, double albpow, double colh0, double temph0, double abu_c,
                        long ncell, int *conv_flag, long *total_iterations)
{
    const double min_frac_change = (double)1.0e-3f;
    const double min_frac_atoms  = (double)1.0e-8f;
    int conv = 0;
    long its = 0;
    for (long p = 0; p < ncell; ++p) {
        double xav = xh_av[p], xint = xh_intermed[p];
        double xav_old = xav;
        double yh_av = 1.0 - xav;                                       /* f90:93 */
        its += oracle_do_chemistry(dt, ndens[p], temp[p], xh[p], &xav, &xint, phi_ion[p],
                                   bh00, albpow, colh0, temph0, abu_c);
        if (fabs(xav - xav_old) > min_frac_change
            && fabs((xav - xav_old) / yh_av) > min_frac_change
            && yh_av > min_frac_atoms)                                  /* f90:100-104 */
            conv += 1;
        xh_intermed[p] = xint;
        xh_av[p] = xav;
    }
    *conv_flag = conv;
    if (total_iterations) *total_iterations = its;
}

/* ------------------------------------------------------------------------- */
/* Single-cell probes for the golden fixtures                                 */
/* ------------------------------------------------------------------------- */
void oracle_cinterp_probe(const int pos[3], const int src[3], const double *coldens_F, int m1, int m2, int m3,
                          double sig, int flags, double *cdensi, double *path)
{
    cd_view v = { coldens_F, { m1, m2, m3 }, { 1, m1, (long)m1 * m2 }, 1 };
    short_char_interp(pos, src, &v, sig, flags, cdensi, path);
}

void oracle_photo_rates_probe(double normflux, double cd_in, double cd_out, double vfact, double sig,
                              const double *thin, const double *thick, const double *hthin, const double *hthick,
                              double minlogtau, double dlogtau, int NumTau, int table_len, int flags,
                              double *phi_cell, double *phi_out, double *heat_cell)
{
    rate_tables tab = { thin, thick, hthin, hthick, minlogtau, dlogtau, NumTau, table_len };
    photo_rates(normflux, cd_in, cd_out, vfact, sig, &tab, flags, phi_cell, phi_out, heat_cell);
}
