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
//                   centred second moments.  Every sum is 256 strided partial sums joined by one LDS tree.  n, the means, the
//                   moments and r, alpha, beta, ED are the masked Kling-Gupta distance of xh_kge.h, the one k_calib_kge_masked
//                   (xh_calib.hip) calls, so ED has the bits of the calibration's per-gauge ED on the same series and record;
//                   the kernel itself adds the copy, the two sums of differences and the eight-column row.
//
// A skipped month adds nothing; a NaN flow at a month of V reaches every sum it enters and makes columns 1..7 NaN; one outside
// V is never added.  Fixed order, no atomics: two calls give the same bits.  IEEE arithmetic as written (no contraction).
#include <cmath>

#include "xh_kge.h"
#include "xh_launch.h"

#pragma clang fp contract(off)

namespace {

constexpr int GS_THREADS = 256;          // the strides and the tree of xh_kge.h
constexpr int GS_COLS = 8;               // n, ED, r, alpha, beta, NSE, PBIAS, RMSE

// the gauge cell's row of Avg_ChFlow; a cell outside the grid reads no flow and gives NaN
struct GaugeRow {
    const double *x;
    bool in;                                                         // block-uniform
    __device__ __forceinline__ double operator[](int m) const { return in ? x[m] : NAN; }
};

// what the kernel adds to the first pass of the distance: the copy-out and the sums the last three columns need
struct GaugeSums {
    double *out;                                                     // the gauge's row of the series output, or NULL
    double so = 0.0, sd = 0.0, sdd = 0.0;
    __device__ __forceinline__ void month(int m, double s) const {
        if (out) out[m] = s;                                         // the row as it lies: a move, the same bits
    }
    __device__ __forceinline__ void used(double s, double o) {
        const double d = s - o;
        so += o;
        sd += d;
        sdd += d * d;
    }
};

__global__ void __launch_bounds__(GS_THREADS) k_gauge_skill(int64_t ncell, int nmonths, const int32_t *__restrict__ gauge_cell,
                                                            const double *__restrict__ flow, const double *__restrict__ obs_all,
                                                            double *__restrict__ series, double *__restrict__ metrics) {
    __shared__ double sh[GS_THREADS];
    const int g = blockIdx.x;
    const int64_t cell = gauge_cell[g];
    const bool in = cell >= 0 && cell < ncell;                       // block-uniform
    const GaugeRow x{flow + (in ? cell : 0) * (int64_t)nmonths, in};
    GaugeSums sums{series ? series + (int64_t)g * nmonths : nullptr};
    const XhKgeMoments M = xh_kge_moments<true>(nmonths, x, obs_all + (int64_t)g * nmonths, sh, sums);
    const double sum_o = xh_block_sum256(sums.so, sh);
    const double sd = xh_block_sum256(sums.sd, sh), sdd = xh_block_sum256(sums.sdd, sh);
    if (threadIdx.x == 0) {
        const XhKge k = xh_kge_finish(M);
        const bool ok = M.n >= 2.0;                                  // one month has a mean and a bias but no score
        double *row = metrics + (int64_t)g * GS_COLS;
        row[0] = M.n;
        row[1] = ok ? k.ed : NAN;
        row[2] = ok ? k.r : NAN;
        row[3] = ok ? k.relvar : NAN;
        row[4] = ok ? k.bias : NAN;
        row[5] = ok ? 1.0 - sdd / M.voo : NAN;
        row[6] = ok ? 100.0 * sd / sum_o : NAN;
        row[7] = ok ? sqrt(sdd / M.n) : NAN;
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
