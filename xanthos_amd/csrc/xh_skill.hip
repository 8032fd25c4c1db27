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
//   k_skill_kge      one workgroup per basin over its series and its observations: the Kling-Gupta distance of xh_kge.h
//                    (means, then centred second moments, each as 256 strided partial sums joined by one LDS tree; then
//                    ED = sqrt((r - 1)^2 + (sd_s / sd_o - 1)^2 + (mean_s / mean_o - 1)^2) as numpy forms it) -- the one
//                    the calibration's objective calls (k_calib_kge, xh_calib.hip), so the bits are the same.
//
// The month split of the first kernel makes the second necessary: the order of the moments' sums must not depend on which
// workgroup ends first.  Every sum has a fixed order and there is no atomic, so two calls give the same bits.  IEEE
// arithmetic as written (no contraction): a constant series or a constant record gives NaN, as numpy does.
#include <cmath>

#include "xh_kge.h"
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

__global__ void __launch_bounds__(256) k_skill_kge(int nmonths, const double *__restrict__ series, const double *__restrict__ obs_all,
                                                   double *__restrict__ ed) {
    __shared__ double sh[256];
    const int b = blockIdx.x;
    const XhKgeMoments M = xh_kge_moments<false>(nmonths, series + (int64_t)b * nmonths, obs_all + (int64_t)b * nmonths, sh);
    if (threadIdx.x == 0) ed[b] = xh_kge_finish(M).ed;
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
