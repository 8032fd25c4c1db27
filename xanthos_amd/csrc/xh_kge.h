// The Kling-Gupta distance ED = 1 - KGE of a series against a record, as every scoring kernel of the library forms it
// (calibrate_abcd.py:196-213), and the 256-lane block sum under it.  Device code only.
//
//   xh_block_sum256   one LDS tree over the 256 lanes of a workgroup, fixed order; every lane gets the total
//   xh_kge_moments    n, the two means and the three centred second moments of one (series, record) pair by one 256-lane
//                     workgroup: 256 strided partial sums per moment, each joined by the tree.  MASKED: over the months whose
//                     observation is finite, n their count; a skipped month adds nothing, so a complete record gives the
//                     unmasked bits
//   xh_kge_finish     r, sd_s / sd_o, mean_s / mean_o and ED from the moments, as numpy forms them: population standard
//                     deviations, np.corrcoef through np.cov clipped to [-1, 1].  A constant series or record gives NaN
//
// One implementation, so two kernels that score the same series against the same record give the same bits.  IEEE
// arithmetic as written: the library is compiled without contraction.
#pragma once
#include <cmath>

#include <hip/hip_runtime.h>

struct XhKgeMoments {
    double n, mx, mo, vxx, voo, vxo;
};

struct XhKge {
    double r, relvar, bias, ed;
};

// sh: 256 doubles of LDS; all 256 lanes of the workgroup call it together
__device__ __forceinline__ double xh_block_sum256(double v, double *sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int stride = 128; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) sh[threadIdx.x] += sh[threadIdx.x + stride];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ XhKge xh_kge_finish(const XhKgeMoments &M) {
    const double n = M.n;
    XhKge k;
    k.relvar = sqrt(M.vxx / n) / sqrt(M.voo / n);                // np.std, population
    k.bias = M.mx / M.mo;
    const double c00 = M.voo / (n - 1.0), c11 = M.vxx / (n - 1.0), c01 = M.vxo / (n - 1.0);   // np.corrcoef via np.cov
    const double r = c01 / sqrt(c11) / sqrt(c00);
    k.r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);                 // corrcoef clips to [-1, 1]; NaN stays NaN
    k.ed = sqrt((k.r - 1.0) * (k.r - 1.0) + (k.relvar - 1.0) * (k.relvar - 1.0) + (k.bias - 1.0) * (k.bias - 1.0));
    return k;
}

struct XhKgeNoHook {
    __device__ __forceinline__ void month(int, double) const {}
    __device__ __forceinline__ void used(double, double) const {}
};

// x[m]: the series (a pointer, or anything with operator[]).  The first pass tells the hook of every month,
// hook.month(m, x[m]), and of every month that enters the sums, hook.used(x[m], obs[m]).
template <bool MASKED, class Series, class Hook = XhKgeNoHook>
__device__ __forceinline__ XhKgeMoments xh_kge_moments(int nmonths, const Series &x, const double *__restrict__ obs, double *sh,
                                                       Hook &&hook = Hook()) {
    XhKgeMoments M;
    double sx = 0.0, so = 0.0, cnt = 0.0;
    for (int m = threadIdx.x; m < nmonths; m += 256) {
        const double o = obs[m], s = x[m];
        hook.month(m, s);
        if (!MASKED || o - o == 0.0) {                           // finite
            sx += s;
            so += o;
            cnt += 1.0;
            hook.used(s, o);
        }
    }
    M.n = MASKED ? xh_block_sum256(cnt, sh) : (double)nmonths;   // (whole numbers: exact)
    M.mx = xh_block_sum256(sx, sh) / M.n;
    M.mo = xh_block_sum256(so, sh) / M.n;
    double vxx = 0.0, voo = 0.0, vxo = 0.0;
    for (int m = threadIdx.x; m < nmonths; m += 256) {
        const double o = obs[m];
        if (!MASKED || o - o == 0.0) {
            const double dx = x[m] - M.mx, d_o = o - M.mo;
            vxx += dx * dx;
            voo += d_o * d_o;
            vxo += dx * d_o;
        }
    }
    M.vxx = xh_block_sum256(vxx, sh);
    M.voo = xh_block_sum256(voo, sh);
    M.vxo = xh_block_sum256(vxo, sh);
    return M;
}
