// Bootstrap confidence intervals of the GEV shape and the return levels per row on the device: is the 100-year
// flood of this cell 312 +- 20 or 312 +- 200?  xh_extremes_boot replaces no function of the reference: xanthos has no
// extreme-value statistics.  The obvious route -- xh_extremes on B resampled copies of the array -- costs B launches and B
// arrays; here a replicate is a column of counts over the row's sorted annual series and its sums walk those counts, so
// neither the arrays nor a sort per replicate exist.
//
// The definitions (draws, a replicate's fit, the intervals) and the whole walk over one row stand in xh_exboot_dev.h,
// host-callable; this file gives that walk its team -- one wavefront, lane <-> replicate -- and its memory, and walks the rows.
//
//   k_exboot   one one-wavefront WORKGROUP per row at a time, walking its own rows (a stride of the grid).  A workgroup of
//   several wavefronts on one row would share nothing but zs and the weights (2.4 KB at 50 years) and would pay a workgroup
//   barrier per sort stage; several rows to a workgroup, as k_extremes has them, would multiply the LDS below by four.
//     1  the row: xh_extremes_row as it is (annual series, counted sort, sums, fit), its table to LDS;
//     2  lane <-> i forms the weight rows w_1 .. w_3 [n] once;
//     3  lane <-> replicate, ceil(B / 64) rounds: n draws into the lane's own column of 16-bit counts in LDS (cnt[j 64 + lane]),
//        the 2 n-step walk of the sums, the fit in registers; k* and the levels go to the workgroup's slab in HBM, quantity-
//        major (consecutive lanes, consecutive addresses), (1 + nT) B doubles a workgroup: written once and read once by the
//        same workgroup, 72 KB at B = 1000 and nT = 8, which LDS could not hold next to the counts at 341 years;
//     4  per quantity: the slab's values into LDS, a bitonic sort of the next power of two, lane 0 forms the two bounds.
//   LDS per workgroup: (max(768, n2) + 5 nyear + 16) doubles + 64 ints + 64 nyear 16-bit counts, n2 = the power of two >= B: at
//   50 years 14,928 B (B <= 768), 16,976 B (to 1024) or 25,168 B (2048), at 341 years 63,816 B, 65,864 B or 74,056 B.  Registers and residency:
//   DESIGN 4.22.  No atomics, nothing crosses a workgroup, every loop's trip count is known at launch, a fixed operation
//   order: two calls give the same bytes, whatever the grid and however the rows are cut into calls (row0).
#include "xh_exboot_dev.h"
#include "xh_launch.h"

namespace {

constexpr int EXB_LANES = 64;

struct ExbWave {
    __device__ __forceinline__ int lane() const { return threadIdx.x; }
    __device__ __forceinline__ int lanes() const { return EXB_LANES; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }      // (one wavefront: a fence, not a wait)
};

struct ExbPeriods {
    double T[XH_EX_MAX_T];
};

// doubles of LDS before the ints and the counts
__host__ __device__ inline int exb_lds_doubles(int nyear, int n2) {
    return (n2 > XH_EX_STAGE ? n2 : XH_EX_STAGE) + 5 * nyear + XH_EX_SH + XH_EXTREMES_NPAR;
}

__global__ void __launch_bounds__(EXB_LANES) k_exboot(int64_t nrows, int row_stride, int col0, int nyear, int kind, int min_years,
                                                      int nT, ExbPeriods periods, int B, double p_lo, double p_hi, uint64_t seed,
                                                      int64_t row0, const double *__restrict__ x, double *__restrict__ slab,
                                                      double *__restrict__ ci, double *__restrict__ rep) {
    extern __shared__ double lds[];
    const int n2 = xh_exb_n2(B);
    double *stage = lds;                            // ... and the sort's buffer once the row is done with it
    double *z = lds + (n2 > XH_EX_STAGE ? n2 : XH_EX_STAGE), *zs = z + nyear, *sh = zs + nyear, *tab = sh + XH_EX_SH;
    double *w = tab + XH_EXTREMES_NPAR;
    int *nfit = reinterpret_cast<int *>(w + 3 * nyear);
    uint16_t *cnt = reinterpret_cast<uint16_t *>(nfit + EXB_LANES);
    double *vals = slab + (size_t)blockIdx.x * (size_t)(1 + nT) * (size_t)B;
    const ExbWave team;
    const int ncol = 3 + 2 * nT;
    const int64_t nrep = (int64_t)B * (XH_EXB_NREP + nT);
    for (int64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
        xh_exboot_row(team, x + r * (int64_t)row_stride + col0, nyear, kind, min_years, nT, periods.T, B, p_lo, p_hi, seed, row0 + r,
                      stage, z, zs, sh, tab, w, cnt, nfit, stage, vals, ci + r * ncol, rep ? rep + r * nrep : nullptr);
    }
}

}  // namespace

extern "C" int xh_extremes_boot(xh_ctx *ctx, int64_t nrows, int32_t row_stride, int32_t col0, int32_t nyear, int32_t kind,
                                int32_t min_years, int32_t nT, const double *h_T, int32_t B, double confidence, uint64_t seed,
                                int64_t row0, const double *d_x, double *d_ci, double *d_rep) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, d_x && d_ci && nrows >= 0, "xh_extremes_boot: NULL array or negative nrows");
    XH_REQUIRE(ctx, nyear >= 1 && 12 * (int64_t)nyear <= XH_EX_MAX_COLS,
               "xh_extremes_boot: nyear (%d) must be at least 1 and 12 nyear at most %d columns", nyear, XH_EX_MAX_COLS);
    XH_REQUIRE(ctx, col0 >= 0 && (int64_t)col0 + 12 * (int64_t)nyear <= row_stride,
               "xh_extremes_boot: the window (column %d, %d years = %d columns) does not lie inside a row of %d", col0, nyear,
               12 * nyear, row_stride);
    XH_REQUIRE(ctx, kind == XH_EXTREMES_MAX || kind == XH_EXTREMES_MIN, "xh_extremes_boot: kind (%d) is neither max (0) nor min (1)",
               kind);
    XH_REQUIRE(ctx, min_years >= XH_EX_MIN_YEARS, "xh_extremes_boot: min_years (%d) must be at least %d", min_years, XH_EX_MIN_YEARS);
    XH_REQUIRE(ctx, nT >= 0 && nT <= XH_EX_MAX_T, "xh_extremes_boot: nT (%d) outside 0..%d", nT, XH_EX_MAX_T);
    XH_REQUIRE(ctx, nT == 0 || h_T, "xh_extremes_boot: NULL return periods");
    ExbPeriods periods;
    for (int j = 0; j < XH_EX_MAX_T; ++j) {
        periods.T[j] = j < nT ? h_T[j] : 2.0;
        XH_REQUIRE(ctx, periods.T[j] > 1.0, "xh_extremes_boot: return period %d (%g) must be > 1", j, periods.T[j]);
    }
    XH_REQUIRE(ctx, B >= XH_EXB_MIN_B && B <= XH_EXB_MAX_B, "xh_extremes_boot: B (%d) outside %d..%d", B, XH_EXB_MIN_B, XH_EXB_MAX_B);
    XH_REQUIRE(ctx, confidence > 0.0 && confidence < 1.0, "xh_extremes_boot: confidence (%g) must lie strictly between 0 and 1",
               confidence);
    XH_REQUIRE(ctx, row0 >= 0, "xh_extremes_boot: row0 (%lld) is negative", (long long)row0);
    if (nrows == 0) return XH_OK;
    const int n2 = xh_exb_n2(B);
    const size_t lds = (size_t)exb_lds_doubles(nyear, n2) * sizeof(double) + EXB_LANES * sizeof(int) +
                       (size_t)EXB_LANES * (size_t)nyear * sizeof(uint16_t);
    int64_t blocks = nrows;
    const int64_t cap = (int64_t)ctx->prop.multiProcessorCount * 8;
    if (blocks > cap) blocks = cap;
    void *slab = nullptr;
    const int rc = xh_scratch(ctx, 2, (size_t)blocks * (size_t)(1 + nT) * (size_t)B * sizeof(double), &slab);
    if (rc) return rc;
    if (lds > 64 * 1024)        // beyond what a kernel may take without asking: 74,056 B at the most (341 years, B > 1024)
        XH_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_exboot), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const double p_lo = (1.0 - confidence) / 2.0, p_hi = 1.0 - p_lo;
    return xh_launch(ctx, "extremes_boot", ctx->stream, k_exboot, dim3((unsigned)blocks), dim3(EXB_LANES), lds, nrows,
                     (int)row_stride, (int)col0, (int)nyear, (int)kind, (int)min_years, (int)nT, periods, (int)B, p_lo, p_hi,
                     (uint64_t)seed, (int64_t)row0, d_x, static_cast<double *>(slab), d_ci, d_rep);
}
