// Test-only probe of the device math primitives (csrc/xh_math.h, csrc/xh_abcd_dev.h): every export takes HOST arrays, runs
// one element-wise kernel on the current device and copies the result back, so a test needs ctypes and numpy only.  The
// headers are included as they are; nothing here is loaded by the package.  The probe_host_* entries evaluate the
// primitives that are plain fma / rint / ldexp arithmetic on the CPU and never touch the GPU.
//
// Return value: 0, or the hipError_t of the first failing runtime call (negative for a bad argument).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "xh_abcd_dev.h"
#include "xh_math.h"

using namespace xh_abcd_dev;

namespace {

enum { OP_XH_EXP = 0, OP_LIB_EXP = 1, OP_XH_EXP_NONPOS = 2, OP_XH_SQRT = 3, OP_LIB_SQRT = 4, OP_FRCP = 5 };
enum { OP_QUOT = 0, OP_IEEE_DIV = 1, OP_FDIV = 2 };

__global__ void k_unary(int op, int64_t n, const double *__restrict__ x, double *__restrict__ out) {
    const XhExpConsts K = xh_exp_consts();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = x[i];
        double r;
        switch (op) {
            case OP_XH_EXP: r = xh_exp(v, K); break;
            case OP_LIB_EXP: r = exp(v); break;
            case OP_XH_EXP_NONPOS: r = xh_exp_nonpos(v, K); break;
            case OP_XH_SQRT: r = xh_sqrt(v); break;
            case OP_LIB_SQRT: r = sqrt(v); break;
            default: r = frcp(v); break;
        }
        out[i] = r;
    }
}

__global__ void k_binary(int op, int64_t n, const double *__restrict__ x, const double *__restrict__ d,
                         double *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double a = x[i], b = d[i];
        double r;
        switch (op) {
            case OP_QUOT: r = quot(a, b, 1.0 / b); break;
            case OP_IEEE_DIV: r = a / b; break;
            default: r = fdiv(a, b); break;
        }
        out[i] = r;
    }
}

__global__ void k_split(int64_t n, int snow_on, const double *__restrict__ precip, const double *__restrict__ tmin,
                        double *__restrict__ rain, double *__restrict__ snow, double *__restrict__ frac,
                        int *__restrict__ kind) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double r, s, f;
        int k;
        abcd_split(snow_on != 0, precip[i], tmin[i], r, s, f, k);
        rain[i] = r;
        snow[i] = s;
        frac[i] = f;
        kind[i] = k;
    }
}

// One thread per cell: nmonths of abcd_month from (snowpack, sm, gw) = state0[0 .. 2][cell].  FASTQ = false is the runoff
// kernels' month (abcd_pre + abcd_step); FASTQ = true the calibration kernel's (the exp argument a bare product with 1 / b,
// abcd_step<true>).  Arrays [ncell, nmonths]; pars [ncell, 5] = a, b (x 1000 inside), c, d, m.
template <bool FASTQ>
__global__ void k_march(int64_t ncell, int nmonths, int snow_on, const double *__restrict__ pars,
                        const double *__restrict__ pet, const double *__restrict__ precip, const double *__restrict__ tmin,
                        const double *__restrict__ state0, double *__restrict__ aet, double *__restrict__ q,
                        double *__restrict__ sav, double *__restrict__ decay, double *__restrict__ state1) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    const bool snow = snow_on != 0;
    const AbcdPar P = load_par(pars, (int)c, snow);
    const XhExpConsts K = xh_exp_consts();
    AbcdState s;
    s.snowpack = state0[c];
    s.sm = state0[ncell + c];
    s.gw = state0[2 * ncell + c];
    for (int m = 0; m < nmonths; ++m) {
        const int64_t i = c * (int64_t)nmonths + m;
        double oa, oq;
        if (FASTQ) {
            AbcdPre r;
            r.pet = pet[i];
            abcd_split(snow, precip[i], snow ? tmin[i] : 0.0, r.rain, r.snow, r.frac, r.kind);
            r.decay = xh_exp(-r.pet * P.inv_b, K);
            abcd_step<true>(P, s, snow, m == 0, r, oa, oq);
            decay[i] = r.decay;
        } else {
            const AbcdPre r = abcd_pre(P, K, snow, pet[i], precip[i], snow ? tmin[i] : 0.0);
            abcd_step<false>(P, s, snow, m == 0, r, oa, oq);
            decay[i] = r.decay;
        }
        aet[i] = oa;
        q[i] = oq;
        sav[i] = s.sm;
    }
    state1[c] = s.snowpack;
    state1[ncell + c] = s.sm;
    state1[2 * ncell + c] = s.gw;
}

struct DevBuf {          // device allocations of one call, freed on every way out
    std::vector<void *> p;
    ~DevBuf() {
        for (void *q : p) (void)hipFree(q);
    }
    hipError_t in(const void *h, size_t bytes, void **d) {
        hipError_t e = hipMalloc(d, bytes ? bytes : 8);
        if (e != hipSuccess) return e;
        p.push_back(*d);
        return h ? hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice) : hipSuccess;
    }
};

#define PROBE_HIP(call)                    \
    do {                                   \
        const hipError_t e_ = (call);      \
        if (e_ != hipSuccess) return (int)e_; \
    } while (0)

unsigned grid_for(int64_t n, int block) {
    const int64_t g = (n + block - 1) / block;
    return (unsigned)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

}  // namespace

extern "C" {

int probe_unary(int op, int64_t n, const double *x, double *out) {
    if (op < 0 || op > OP_FRCP || n < 0 || !x || !out) return -1;
    if (n == 0) return 0;
    DevBuf B;
    void *dx, *dout;
    PROBE_HIP(B.in(x, n * sizeof(double), &dx));
    PROBE_HIP(B.in(nullptr, n * sizeof(double), &dout));
    k_unary<<<grid_for(n, 256), 256>>>(op, n, (const double *)dx, (double *)dout);
    PROBE_HIP(hipGetLastError());
    PROBE_HIP(hipMemcpy(out, dout, n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int probe_binary(int op, int64_t n, const double *x, const double *d, double *out) {
    if (op < 0 || op > OP_FDIV || n < 0 || !x || !d || !out) return -1;
    if (n == 0) return 0;
    DevBuf B;
    void *dx, *dd, *dout;
    PROBE_HIP(B.in(x, n * sizeof(double), &dx));
    PROBE_HIP(B.in(d, n * sizeof(double), &dd));
    PROBE_HIP(B.in(nullptr, n * sizeof(double), &dout));
    k_binary<<<grid_for(n, 256), 256>>>(op, n, (const double *)dx, (const double *)dd, (double *)dout);
    PROBE_HIP(hipGetLastError());
    PROBE_HIP(hipMemcpy(out, dout, n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int probe_split(int64_t n, int snow_on, const double *precip, const double *tmin, double *rain, double *snow, double *frac,
                int32_t *kind) {
    if (n < 0 || !precip || !tmin || !rain || !snow || !frac || !kind) return -1;
    if (n == 0) return 0;
    DevBuf B;
    void *dp, *dt, *dr, *ds, *df, *dk;
    PROBE_HIP(B.in(precip, n * sizeof(double), &dp));
    PROBE_HIP(B.in(tmin, n * sizeof(double), &dt));
    PROBE_HIP(B.in(nullptr, n * sizeof(double), &dr));
    PROBE_HIP(B.in(nullptr, n * sizeof(double), &ds));
    PROBE_HIP(B.in(nullptr, n * sizeof(double), &df));
    PROBE_HIP(B.in(nullptr, n * sizeof(int32_t), &dk));
    k_split<<<grid_for(n, 256), 256>>>(n, snow_on, (const double *)dp, (const double *)dt, (double *)dr, (double *)ds,
                                        (double *)df, (int *)dk);
    PROBE_HIP(hipGetLastError());
    PROBE_HIP(hipMemcpy(rain, dr, n * sizeof(double), hipMemcpyDeviceToHost));
    PROBE_HIP(hipMemcpy(snow, ds, n * sizeof(double), hipMemcpyDeviceToHost));
    PROBE_HIP(hipMemcpy(frac, df, n * sizeof(double), hipMemcpyDeviceToHost));
    PROBE_HIP(hipMemcpy(kind, dk, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

// tmin may be NULL (no snow).  state0 / state1 [3, ncell]: snowpack, soil moisture, groundwater before / after.
int probe_march(int64_t ncell, int32_t nmonths, int fastq, const double *pars, const double *pet, const double *precip,
                const double *tmin, const double *state0, double *aet, double *q, double *sav, double *decay,
                double *state1) {
    if (ncell < 0 || nmonths < 1 || !pars || !pet || !precip || !state0 || !aet || !q || !sav || !decay || !state1) return -1;
    if (ncell == 0) return 0;
    const size_t nb = (size_t)ncell * nmonths * sizeof(double), sb = 3 * (size_t)ncell * sizeof(double);
    DevBuf B;
    void *dpar, *dpet, *dpr, *dtn = nullptr, *ds0, *da, *dq, *dsv, *ddc, *ds1;
    PROBE_HIP(B.in(pars, 5 * (size_t)ncell * sizeof(double), &dpar));
    PROBE_HIP(B.in(pet, nb, &dpet));
    PROBE_HIP(B.in(precip, nb, &dpr));
    if (tmin) PROBE_HIP(B.in(tmin, nb, &dtn));
    PROBE_HIP(B.in(state0, sb, &ds0));
    PROBE_HIP(B.in(nullptr, nb, &da));
    PROBE_HIP(B.in(nullptr, nb, &dq));
    PROBE_HIP(B.in(nullptr, nb, &dsv));
    PROBE_HIP(B.in(nullptr, nb, &ddc));
    PROBE_HIP(B.in(nullptr, sb, &ds1));
    const unsigned grid = (unsigned)((ncell + 63) / 64);
    if (fastq)
        k_march<true><<<grid, 64>>>(ncell, nmonths, tmin != nullptr, (const double *)dpar, (const double *)dpet,
                                    (const double *)dpr, (const double *)dtn, (const double *)ds0, (double *)da, (double *)dq,
                                    (double *)dsv, (double *)ddc, (double *)ds1);
    else
        k_march<false><<<grid, 64>>>(ncell, nmonths, tmin != nullptr, (const double *)dpar, (const double *)dpet,
                                     (const double *)dpr, (const double *)dtn, (const double *)ds0, (double *)da, (double *)dq,
                                     (double *)dsv, (double *)ddc, (double *)ds1);
    PROBE_HIP(hipGetLastError());
    PROBE_HIP(hipMemcpy(aet, da, nb, hipMemcpyDeviceToHost));
    PROBE_HIP(hipMemcpy(q, dq, nb, hipMemcpyDeviceToHost));
    PROBE_HIP(hipMemcpy(sav, dsv, nb, hipMemcpyDeviceToHost));
    PROBE_HIP(hipMemcpy(decay, ddc, nb, hipMemcpyDeviceToHost));
    PROBE_HIP(hipMemcpy(state1, ds1, sb, hipMemcpyDeviceToHost));
    return 0;
}

// ---- the same source on the CPU (no GPU call): the primitives that are fma / rint / ldexp arithmetic only
int probe_host_unary(int op, int64_t n, const double *x, double *out) {
    if ((op != OP_XH_EXP && op != OP_XH_EXP_NONPOS) || n < 0 || !x || !out) return -1;
    const XhExpConsts K = xh_exp_consts();
    for (int64_t i = 0; i < n; ++i) out[i] = op == OP_XH_EXP ? xh_exp(x[i], K) : xh_exp_nonpos(x[i], K);
    return 0;
}

int probe_host_binary(int op, int64_t n, const double *x, const double *d, double *out) {
    if (op != OP_QUOT || n < 0 || !x || !d || !out) return -1;
    for (int64_t i = 0; i < n; ++i) out[i] = quot(x[i], d[i], 1.0 / d[i]);
    return 0;
}

}  // extern "C"
