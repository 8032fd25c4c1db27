// Skill of a run's routed streamflow at stream gauges, formed in HBM on the Avg_ChFlow the run left there.
//
// The reference scores streamflow inside its calibration only (calibrate_abcd.py:196-213); a parameter set that is run
// forward afterwards is scored, if at all, from the 67,420-row avgchflow file.  Here the rows of the gauge cells are
// picked and scored where they lie:
//
//   k_gauge_skill   one workgroup per gauge, 256 lanes along the months of the gauge cell's row of Avg_ChFlow (month-fastest:
//                   every access to the row is coalesced) and of the gauge's record.  V = the months with a finite
//                   observation.  First pass over V: the count, the sums of s and o, of (s - o) and of (s - o)^2 -- and the
//                   row itself, all months, copied out bit for bit when the caller wants the series.  Second pass: the
//                   centred second moments.  Every sum is 256 strided partial sums joined by one LDS tree: the sums of
//                   k_calib_kge_masked (xh_calib.hip), restated here operation for operation, so ED has the bits of the
//                   calibration's per-gauge ED on the same series and record (tests/test_gpu_gauge_skill.py holds it to that).
//
// A skipped month adds nothing; a NaN flow at a month of V reaches every sum it enters and makes columns 1..7 NaN; one outside
// V is never added.  Fixed order, no atomics: two calls give the same bits.  IEEE arithmetic as written (no contraction).
#include <cmath>

#include "xh_launch.h"

#pragma clang fp contract(off)

namespace {

constexpr int GS_THREADS = 256;          // the strides and the tree of k_calib_kge_masked
constexpr int GS_COLS = 8;               // n, ED, r, alpha, beta, NSE, PBIAS, RMSE

__device__ __forceinline__ double gs_block_sum(double v, double *sh) {
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

__global__ void __launch_bounds__(GS_THREADS) k_gauge_skill(int64_t ncell, int nmonths, const int32_t *__restrict__ gauge_cell,
                                                            const double *__restrict__ flow, const double *__restrict__ obs_all,
                                                            double *__restrict__ series, double *__restrict__ metrics) {
    __shared__ double sh[GS_THREADS];
    const int g = blockIdx.x;
    const int64_t cell = gauge_cell[g];
    const bool in = cell >= 0 && cell < ncell;                       // block-uniform; a cell outside the grid reads no flow
    const double *x = flow + (in ? cell : 0) * (int64_t)nmonths;
    const double *obs = obs_all + (int64_t)g * nmonths;
    double *out = series ? series + (int64_t)g * nmonths : nullptr;
    double sx = 0.0, so = 0.0, cnt = 0.0, sd = 0.0, sdd = 0.0;
    for (int m = threadIdx.x; m < nmonths; m += GS_THREADS) {
        const double o = obs[m];
        const double s = in ? x[m] : NAN;
        if (out) out[m] = s;                                         // the row as it lies: a move, the same bits
        if (o - o == 0.0) {                                          // finite
            sx += s;
            so += o;
            cnt += 1.0;
            const double d = s - o;
            sd += d;
            sdd += d * d;
        }
    }
    const double n = gs_block_sum(cnt, sh);                          // (whole numbers: exact)
    const double mx = gs_block_sum(sx, sh) / n, mo = gs_block_sum(so, sh) / n;
    double vxx = 0.0, voo = 0.0, vxo = 0.0;
    for (int m = threadIdx.x; m < nmonths; m += GS_THREADS) {
        const double o = obs[m];
        if (o - o == 0.0) {
            const double dx = (in ? x[m] : NAN) - mx, d_o = o - mo;
            vxx += dx * dx;
            voo += d_o * d_o;
            vxo += dx * d_o;
        }
    }
    vxx = gs_block_sum(vxx, sh);
    voo = gs_block_sum(voo, sh);
    vxo = gs_block_sum(vxo, sh);
    const double sum_o = gs_block_sum(so, sh);
    sd = gs_block_sum(sd, sh);
    sdd = gs_block_sum(sdd, sh);
    if (threadIdx.x == 0) {
        const double relvar = sqrt(vxx / n) / sqrt(voo / n);         // np.std, population
        const double bias = mx / mo;
        const double c00 = voo / (n - 1.0), c11 = vxx / (n - 1.0), c01 = vxo / (n - 1.0);   // np.corrcoef via np.cov
        double r = c01 / sqrt(c11) / sqrt(c00);
        r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);                   // corrcoef clips to [-1, 1]; NaN stays NaN
        const double ed = sqrt((r - 1.0) * (r - 1.0) + (relvar - 1.0) * (relvar - 1.0) + (bias - 1.0) * (bias - 1.0));
        const bool ok = n >= 2.0;                                    // one month has a mean and a bias but no score
        double *row = metrics + (int64_t)g * GS_COLS;
        row[0] = n;
        row[1] = ok ? ed : NAN;
        row[2] = ok ? r : NAN;
        row[3] = ok ? relvar : NAN;
        row[4] = ok ? bias : NAN;
        row[5] = ok ? 1.0 - sdd / voo : NAN;
        row[6] = ok ? 100.0 * sd / sum_o : NAN;
        row[7] = ok ? sqrt(sdd / n) : NAN;
    }
}

}  // namespace

extern "C" int xh_gauge_skill(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t ngauge, const int32_t *d_gauge_cell,
                              const double *d_flow, const double *d_obs, double *d_series, double *d_metrics) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, ncell >= 1 && nmonths >= 2 && ngauge >= 1, "xh_gauge_skill: bad size (ncell %lld, nmonths %d, ngauge %d)",
               (long long)ncell, nmonths, ngauge);
    XH_REQUIRE(ctx, ngauge <= 65535, "xh_gauge_skill: %d gauges exceed the 65535 of one launch", ngauge);
    XH_REQUIRE(ctx, d_gauge_cell && d_flow && d_obs && d_metrics, "xh_gauge_skill: NULL argument");
    return xh_launch(ctx, "gauge_skill", ctx->stream, k_gauge_skill, dim3((unsigned)ngauge), GS_THREADS, 0, ncell, (int)nmonths,
                     d_gauge_cell, d_flow, d_obs, d_series, d_metrics);
}
