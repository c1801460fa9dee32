// rate_primitives_debug.hip -- asora_debug_rate_primitives: the device functions every rate goes through (rates_device.hpp:
// log2_pos, lookup_issue / lookup_value / lookup_heat, div_newton, mul_unfused / add_unfused / absorber_density, rate_issue /
// rate_value, heat_rate_per_atom, grey_rate_per_atom) evaluated element-wise on arrays, so that tests can hold each of them
// against a high-precision reference (tests/test_gpu_rate_primitives.py).  The kernel calls those functions themselves and
// restates nothing; what it cannot show is the code the compiler generates for them inside the raytrace kernels.
#include "rates_device.hpp"

namespace asora {

struct PrimArgs {
    size_t n;
    const double *a, *b, *c, *d;
    double *out, *out2;
    const double2 *tab;                // the table set of `spectrum`: thick | thin | heat thick | heat thin
    const double2 *ramp;               // LOOKUP: ramp[j] = j over the extent of one table set -- the load address as a value
    int which;                         // LOOKUP: 0 thick, 1 thin, 2 heat thick, 3 heat thin
};

constexpr int PRIM_THREADS = 256;

// One operation (OP: ASORA_PRIM_*) per launch, grid-stride; the log2 table staged in LDS as plane_flux_kernel stages it.  The
// parameter block is read from device memory (uniform loads): with the arrays' pointers next to it, it would not fit a kernel's
// argument segment.
template <int OP>
__global__ void __launch_bounds__(PRIM_THREADS) rate_primitives_kernel(const RtParams *__restrict__ params, const PrimArgs k)
{
    __shared__ double2 logtab[LOG_TABLE_SIZE];
    const RtParams &p = *params;
    for (int t = threadIdx.x; t < LOG_TABLE_SIZE; t += PRIM_THREADS) logtab[t] = p.logtab[t];
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * PRIM_THREADS;
    for (size_t i = (size_t)blockIdx.x * PRIM_THREADS + threadIdx.x; i < k.n; i += stride) {
        if (OP == ASORA_PRIM_LOG2) k.out[i] = log2_pos(k.a[i], logtab);
        if (OP == ASORA_PRIM_LOOKUP) {
            const int off = (k.which & 1) ? table_stride(p.table_len) : 0;
            const double tau = k.a[i];
            Lookup L, I;               // I: the same call on the ramp -- I.t.x - off is the integer index the function formed
            if (k.which & 2) {
                L = lookup_issue<true>(k.tab, tau, p, logtab, off);
                I = lookup_issue<true>(k.ramp, tau, p, logtab, off);
                k.out[i] = lookup_heat(L);
            } else {
                L = lookup_issue(k.tab, tau, p, logtab, off);
                I = lookup_issue(k.ramp, tau, p, logtab, off);
                k.out[i] = lookup_value(L);
            }
            k.out2[i] = (I.t.x - (double)off) + I.residual;
        }
        if (OP == ASORA_PRIM_DIV) k.out[i] = div_newton(k.a[i], k.b[i]);
        if (OP == ASORA_PRIM_MUL) k.out[i] = mul_unfused(k.a[i], k.b[i]);
        if (OP == ASORA_PRIM_ADD) k.out[i] = add_unfused(k.a[i], k.b[i]);
        if (OP == ASORA_PRIM_ABSORBER) k.out[i] = absorber_density(k.a[i], k.b[i], k.c[i], k.d[i]);
        if (OP == ASORA_PRIM_PHOTO) k.out[i] = rate_value(rate_issue(k.a[i], k.b[i], k.c[i], k.d[i], p, logtab, k.tab));
        if (OP == ASORA_PRIM_HEAT) k.out[i] = heat_rate_per_atom(k.a[i], k.b[i], k.c[i], k.d[i], p, logtab, k.tab);
        if (OP == ASORA_PRIM_GREY) k.out[i] = grey_rate_per_atom(k.a[i], k.b[i], k.c[i], k.d[i], p);
    }
}

template <int OP>
static void launch_prim(State &st, const RtParams *p, const PrimArgs &k)
{
    const size_t blocks = std::min<size_t>((k.n + PRIM_THREADS - 1) / PRIM_THREADS, (size_t)4 * (size_t)std::max(st.cu_count, 1));
    hipLaunchKernelGGL(rate_primitives_kernel<OP>, dim3((unsigned)blocks), dim3(PRIM_THREADS), 0, st.stream, p, k);
}

} // namespace asora

using namespace asora;

extern "C" int asora_debug_rate_primitives(int op, size_t n, const double *a, const double *b, const double *c, const double *d,
                                           int which, int spectrum, double sig, double minlogtau, double dlogtau, int NumTau,
                                           double *out, double *out2)
{
    clear_error();
    if (int rc = require_init("debug_rate_primitives")) return rc;
    if (op < 0 || op >= ASORA_PRIM_COUNT) return fail(3, "debug_rate_primitives: unknown operation " + std::to_string(op));
    const int inputs = op == ASORA_PRIM_LOG2 || op == ASORA_PRIM_LOOKUP ? 1 : (op == ASORA_PRIM_DIV || op == ASORA_PRIM_MUL || op == ASORA_PRIM_ADD ? 2 : 4);
    const double *in[4] = {a, b, c, d};
    for (int q = 0; q < inputs; ++q) if (!in[q]) return fail(3, "debug_rate_primitives: null input");
    if (!out || (op == ASORA_PRIM_LOOKUP && !out2)) return fail(3, "debug_rate_primitives: null output");
    State &st = state();
    const bool tables = op == ASORA_PRIM_LOOKUP || op == ASORA_PRIM_PHOTO || op == ASORA_PRIM_HEAT;
    if (tables) {
        if (which < 0 || which > 3) return fail(3, "debug_rate_primitives: which must be 0 ... 3 (thick, thin, heat thick, heat thin)");
        if (NumTau < 1) return fail(3, "debug_rate_primitives: NumTau must be >= 1");
        if (!st.sources.tables) return fail(4, "debug_rate_primitives: radiation tables not on device (photo_table_to_device)");
        if ((op == ASORA_PRIM_HEAT || (op == ASORA_PRIM_LOOKUP && (which & 2))) && !st.sources.loaded.heat_tables)
            return fail(4, "debug_rate_primitives: heating tables not on device (heat_table_to_device)");
        if (spectrum < 0 || spectrum >= st.sources.loaded.num_spec)
            return fail(4, "debug_rate_primitives: table set " + std::to_string(spectrum) + " but the device holds " + std::to_string(st.sources.loaded.num_spec) +
                               " (spectra_to_device)");
    }
    if (n == 0) return 0;
    if (int rc = ensure_logtab(st)) return rc;

    // the parameter block of a trace, as launch_raytrace completes it (this is no trace: the radius history stays as it was)
    State::RadiusHistory history[2] = {st.rt.radius[0], st.rt.radius[1]};
    RtParams p;
    fill_rt_params(p, 0.0, sig, 1.0, minlogtau, dlogtau, NumTau);
    st.rt.radius[0] = history[0]; st.rt.radius[1] = history[1];
    const LutIndex lut = lut_index_constants(p.minlogtau, p.dlogtau);
    p.lut_k1 = lut.k1; p.lut_k0 = lut.k0; p.lut_kc = lut.kc;
    p.logtab = st.logtab_dev;

    Scoped<double> dev[4], d_out, d_out2, d_ramp, d_params;     // device buffers of this call, released however it ends
    PrimArgs k;
    std::memset(&k, 0, sizeof k);
    k.n = n; k.which = which;
    for (int q = 0; q < inputs; ++q) {
        if (int rc = dev[q].allocate(n)) return rc;
        ASORA_HIP_TRY(hipMemcpyAsync(dev[q], in[q], n * sizeof(double), hipMemcpyHostToDevice, st.stream));
    }
    k.a = dev[0]; k.b = dev[1]; k.c = dev[2]; k.d = dev[3];
    if (int rc = d_out.allocate(n)) return rc;
    if (op == ASORA_PRIM_LOOKUP) { if (int rc = d_out2.allocate(n)) return rc; }
    k.out = d_out; k.out2 = d_out2;
    std::vector<double> ramp;
    if (tables) {
        k.tab = p.tables + (size_t)spectrum * p.spec_stride;
        if (op == ASORA_PRIM_LOOKUP) {
            ramp.resize((size_t)4 * table_stride(p.table_len));
            for (size_t j = 0; j < ramp.size(); ++j) ramp[j] = (double)j;
            if (int rc = d_ramp.allocate(ramp.size())) return rc;
            ASORA_HIP_TRY(hipMemcpyAsync(d_ramp, ramp.data(), ramp.size() * sizeof(double), hipMemcpyHostToDevice, st.stream));
            k.ramp = reinterpret_cast<const double2 *>(d_ramp.get());
        }
    }
    if (int rc = d_params.allocate((sizeof(RtParams) + sizeof(double) - 1) / sizeof(double))) return rc;
    ASORA_HIP_TRY(hipMemcpyAsync(d_params, &p, sizeof(RtParams), hipMemcpyHostToDevice, st.stream));
    const RtParams *pd = reinterpret_cast<const RtParams *>(d_params.get());
    switch (op) {
    case ASORA_PRIM_LOG2: launch_prim<ASORA_PRIM_LOG2>(st, pd, k); break;
    case ASORA_PRIM_LOOKUP: launch_prim<ASORA_PRIM_LOOKUP>(st, pd, k); break;
    case ASORA_PRIM_DIV: launch_prim<ASORA_PRIM_DIV>(st, pd, k); break;
    case ASORA_PRIM_MUL: launch_prim<ASORA_PRIM_MUL>(st, pd, k); break;
    case ASORA_PRIM_ADD: launch_prim<ASORA_PRIM_ADD>(st, pd, k); break;
    case ASORA_PRIM_ABSORBER: launch_prim<ASORA_PRIM_ABSORBER>(st, pd, k); break;
    case ASORA_PRIM_PHOTO: launch_prim<ASORA_PRIM_PHOTO>(st, pd, k); break;
    case ASORA_PRIM_HEAT: launch_prim<ASORA_PRIM_HEAT>(st, pd, k); break;
    default: launch_prim<ASORA_PRIM_GREY>(st, pd, k); break;
    }
    ASORA_HIP_TRY(hipGetLastError());
    ASORA_HIP_TRY(hipMemcpyAsync(out, k.out, n * sizeof(double), hipMemcpyDeviceToHost, st.stream));
    if (op == ASORA_PRIM_LOOKUP) ASORA_HIP_TRY(hipMemcpyAsync(out2, k.out2, n * sizeof(double), hipMemcpyDeviceToHost, st.stream));
    ASORA_HIP_TRY(hipStreamSynchronize(st.stream));
    return 0;
}
