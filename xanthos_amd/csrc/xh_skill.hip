// Skill of a run's runoff against observed basin runoff, formed in HBM: the Kling-Gupta distance per basin.
//
// The reference scores a parameter set inside its calibration only (calibrate_abcd.py:156-162, the basin series, and
// :196-213, the distance); a set that is run forward afterwards is scored, if at all, from the files.  Here the Q of an
// ensemble member [ncell, nmonths] is scored where it lies, before the writer converts it:
//
//   k_skill_series   series[b, m] = sum over the basin's cells c, ascending, of q[c, m] * area[c] * 1e-6 (km3_per_mth;
//                    without area the plain q[c, m], mm_per_mth), a NaN term adding 0.0 (np.nansum).  Q is month-fastest, so
//                    the lanes of a wave run along 64 consecutive months and every access to a cell's row is one coalesced
//                    512-byte run; the loop over the basin's cells is the sequential sum, eight rows in flight.  One one-wave
//                    workgroup per (64 months, basin).  Each Q row of a listed cell is read exactly once.
//   k_skill_kge      one workgroup per basin over its series and its observations: means, then the centred second
//                    moments, each as 256 strided partial sums joined by one LDS tree (the sums of k_calib_kge, xh_calib.hip),
//                    then ED = sqrt((r - 1)^2 + (sd_s / sd_o - 1)^2 + (mean_s / mean_o - 1)^2) as numpy forms it
//                    (population standard deviations, np.corrcoef through np.cov and clipped to [-1, 1]).
//
// The month split of the first kernel makes the second necessary: the order of the moments' sums must not depend on which
// workgroup ends first.  Every sum has a fixed order and there is no atomic, so two calls give the same bits.  IEEE
// arithmetic as written (no contraction): a constant series or a constant record gives NaN, as numpy does.
#include <cmath>

#include "xh_launch.h"

#pragma clang fp contract(off)

namespace {

constexpr int SKILL_LANES = 64;
constexpr int SKILL_ROWS = 8;        // rows of Q in flight per wave: the loop is bound by the latency of a row, not by its bytes

__global__ void __launch_bounds__(SKILL_LANES) k_skill_series(int64_t ncell, int nmonths, const int64_t *__restrict__ start,
                                                               const int32_t *__restrict__ cells, const double *__restrict__ q,
                                                               const double *__restrict__ area, double *__restrict__ series) {
    const int b = blockIdx.y;
    const int m = blockIdx.x * SKILL_LANES + threadIdx.x;
    if (m >= nmonths) return;
    const int64_t j0 = start[b], j1 = start[b + 1];
    double acc = 0.0;
    int64_t j = j0;
    for (; j + SKILL_ROWS <= j1; j += SKILL_ROWS) {                // SKILL_ROWS rows in flight, added in cell order
        double v[SKILL_ROWS], a[SKILL_ROWS];
#pragma unroll
        for (int u = 0; u < SKILL_ROWS; ++u) {
            const int64_t c = cells[j + u];
            const bool in = c >= 0 && c < ncell;                  // (a cell outside the grid adds nothing and reads nothing)
            v[u] = in ? q[c * nmonths + m] : NAN;
            a[u] = (area && in) ? area[c] : 1.0;
        }
#pragma unroll
        for (int u = 0; u < SKILL_ROWS; ++u) {
            const double t = area ? v[u] * a[u] * 1e-6 : v[u];
            acc += t == t ? t : 0.0;
        }
    }
    for (; j < j1; ++j) {
        const int64_t c = cells[j];
        if (c < 0 || c >= ncell) continue;
        const double v = q[c * nmonths + m];
        const double t = area ? v * area[c] * 1e-6 : v;
        acc += t == t ? t : 0.0;
    }
    series[(int64_t)b * nmonths + m] = acc;
}

__device__ __forceinline__ double skill_block_sum(double v, double *sh) {
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

__global__ void __launch_bounds__(256) k_skill_kge(int nmonths, const double *__restrict__ series, const double *__restrict__ obs_all,
                                                   double *__restrict__ ed) {
    __shared__ double sh[256];
    const int b = blockIdx.x;
    const double *x = series + (int64_t)b * nmonths;
    const double *obs = obs_all + (int64_t)b * nmonths;
    double sx = 0.0, so = 0.0;
    for (int m = threadIdx.x; m < nmonths; m += 256) {
        sx += x[m];
        so += obs[m];
    }
    const double n = (double)nmonths;
    const double mx = skill_block_sum(sx, sh) / n, mo = skill_block_sum(so, sh) / n;
    double vxx = 0.0, voo = 0.0, vxo = 0.0;
    for (int m = threadIdx.x; m < nmonths; m += 256) {
        const double dx = x[m] - mx, d_o = obs[m] - mo;
        vxx += dx * dx;
        voo += d_o * d_o;
        vxo += dx * d_o;
    }
    vxx = skill_block_sum(vxx, sh);
    voo = skill_block_sum(voo, sh);
    vxo = skill_block_sum(vxo, sh);
    if (threadIdx.x == 0) {
        const double relvar = sqrt(vxx / n) / sqrt(voo / n);     // np.std, population
        const double bias = mx / mo;
        const double c00 = voo / (n - 1.0), c11 = vxx / (n - 1.0), c01 = vxo / (n - 1.0);   // np.corrcoef via np.cov
        double r = c01 / sqrt(c11) / sqrt(c00);
        r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);               // corrcoef clips to [-1, 1]; NaN stays NaN
        ed[b] = sqrt((r - 1.0) * (r - 1.0) + (relvar - 1.0) * (relvar - 1.0) + (bias - 1.0) * (bias - 1.0));
    }
}

}  // namespace

extern "C" int xh_basin_kge(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t nbasins, const int64_t *d_start,
                            const int32_t *d_cells, const double *d_q, const double *d_area, const double *d_obs,
                            double *d_series, double *d_ed) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, ncell >= 1 && nmonths >= 2 && nbasins >= 1, "xh_basin_kge: bad size (ncell %lld, nmonths %d, nbasins %d)",
               (long long)ncell, nmonths, nbasins);
    XH_REQUIRE(ctx, nbasins <= 65535, "xh_basin_kge: %d basins exceed the 65535 of one launch", nbasins);
    XH_REQUIRE(ctx, d_start && d_cells && d_q && d_obs && d_ed, "xh_basin_kge: NULL argument");
    if (!d_series) {                                               // the series are the caller's to keep or not
        void *buf = nullptr;
        const int rc = xh_scratch(ctx, 2, sizeof(double) * (size_t)nbasins * (size_t)nmonths, &buf);
        if (rc) return rc;
        d_series = static_cast<double *>(buf);
    }
    return xh_timed(ctx, "basin_kge", ctx->stream, [&] {
        const dim3 grid((unsigned)((nmonths + SKILL_LANES - 1) / SKILL_LANES), (unsigned)nbasins);
        const int rc = xh_launch(ctx, nullptr, ctx->stream, k_skill_series, grid, SKILL_LANES, 0, ncell, (int)nmonths, d_start,
                                 d_cells, d_q, d_area, d_series);
        if (rc) return rc;
        return xh_launch(ctx, nullptr, ctx->stream, k_skill_kge, dim3((unsigned)nbasins), 256, 0, (int)nmonths,
                         (const double *)d_series, d_obs, d_ed);
    });
}
