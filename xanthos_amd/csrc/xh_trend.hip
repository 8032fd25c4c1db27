// Mann-Kendall trend test and Theil-Sen slope per row on the device: is runoff, soil moisture or streamflow
// changing in this cell, by how much per year, and is the change significant?  xh_trend replaces no function of the
// reference: xanthos has no trend statistic; a user downloads the arrays and loops scipy.stats.theilslopes over the rows,
// which sorts all n (n - 1) / 2 pairwise slopes of every row.
//
// The definitions (pairs, S, the tie-corrected variance without a sort, z and p, the slopes, their median and the two
// confidence ranks, the intercept) and the whole walk over one row stand in xh_trend_dev.h, host-callable; this file gives
// that walk its team -- a workgroup -- and its memory, and walks the rows.
//
//   k_trend   one workgroup of 256 lanes per row at a time (grid-stride over the rows):
//     1  the row's used window x[r, col0 .. col0 + ncol) comes from HBM once, coalesced, into LDS, +-inf as NaN;
//     2  lane <-> element: one walk over the element's season gives its part of n, npairs, S and V; four block sums
//        (xh_block_sum256: whole numbers, exact in a double in any order);
//     3  the order statistics of the up to nseason C(ncol / nseason, 2) slopes by radix select: passes of 8 bits, each
//        recomputing every slope from the row in LDS (one subtraction, one division) and counting it, by an integer LDS
//        add, in the histogram of every wanted rank whose prefix it shares; 64 lanes sum the bins by sixteens and lanes
//        0 .. 3 pick their rank's bin; once every rank is alone in its bin one last pass reads the keys off.  The same
//        routine selects the medians of x and tau (passes over ncol elements);
//     4  lane 0 forms z, p, the medians' means and the intercept and writes the row's 10 doubles.
//   LDS: 8 B per column + 4 KB of histograms + 2 KB of the block sum + 352 B of selection state: 11 KB at 600 columns, 39 KB
//   at the 4096-column limit.  The kernel takes 158 VGPRs, so 3 waves per SIMD = 3 workgroups per CU are resident (33 KB of
//   the CU's 160 KB at 600 columns): registers bound the occupancy, not LDS.  Measured on 67,420 x 600 (profiles/trend):
//   19.2 ms for the seasonal test (14,700 slopes per row), 3.4 ms for the annual one (1,225).
//   No floating-point atomics and a fixed operation order: two calls give the same bits.
#include "xh_kge.h"
#include "xh_launch.h"
#include "xh_trend_dev.h"

namespace {

constexpr int TR_THREADS = 256;

struct TrBlock {
    double *sh;                              // 256 doubles: xh_block_sum256's
    __device__ __forceinline__ int lane() const { return threadIdx.x; }
    __device__ __forceinline__ int lanes() const { return TR_THREADS; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ double sum(double v) const { return xh_block_sum256(v, sh); }
    __device__ __forceinline__ void add(uint32_t *p) const { atomicAdd(p, 1u); }
};

__global__ void __launch_bounds__(TR_THREADS) k_trend(int64_t nrows, int row_stride, int col0, int ncol, int nseason,
                                                     double z_conf, const double *__restrict__ x, double *__restrict__ out) {
    extern __shared__ double lds[];
    double *xs = lds;                                                       // [ncol]
    double *sh = lds + ncol;                                                // [256]
    XhTrSel *st = reinterpret_cast<XhTrSel *>(sh + TR_THREADS);             // 352 B
    uint32_t *hist = reinterpret_cast<uint32_t *>(sh + TR_THREADS + 44);    // [4, 256]
    const TrBlock team = {sh};
    for (int64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
        xh_trend_row(team, x + r * (int64_t)row_stride + col0, ncol, nseason, z_conf, xs, hist, st, out + r * XH_TREND_NCOL);
        __syncthreads();                    // xs is rewritten by the next row
    }
}

}  // namespace

extern "C" int xh_trend(xh_ctx *ctx, int64_t nrows, int32_t row_stride, int32_t col0, int32_t ncol, int32_t nseason,
                        double z_conf, const double *d_x, double *d_out) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, d_x && d_out && nrows >= 0, "xh_trend: NULL array or negative nrows");
    if (nseason < 1 || nseason > 12) return xh_fail(ctx, XH_ERR_LIMIT, "xh_trend: nseason (%d) outside 1..12", nseason);
    XH_REQUIRE(ctx, col0 >= 0 && ncol > 0 && (int64_t)col0 + ncol <= row_stride,
               "xh_trend: the window (column %d, %d columns) does not lie inside a row of %d", col0, ncol, row_stride);
    if (ncol > XH_TR_MAX_COLS) {
        return xh_fail(ctx, XH_ERR_LIMIT, "xh_trend: ncol (%d) exceeds the %d columns a row may take in LDS", ncol, XH_TR_MAX_COLS);
    }
    XH_REQUIRE(ctx, ncol % nseason == 0, "xh_trend: ncol (%d) is no multiple of nseason (%d)", ncol, nseason);
    XH_REQUIRE(ctx, z_conf < 0.0 && z_conf - z_conf == 0.0, "xh_trend: z_conf (%g) must be negative and finite", z_conf);
    if (nrows == 0) return XH_OK;
    static_assert(sizeof(XhTrSel) == 352, "the selection state is 44 doubles of LDS");
    const size_t lds = ((size_t)ncol + TR_THREADS + 44) * sizeof(double) + XH_TR_MAX_RANKS * 256 * sizeof(uint32_t);
    int64_t blocks = (int64_t)ctx->prop.multiProcessorCount * 8;
    if (blocks > nrows) blocks = nrows;
    return xh_launch(ctx, "trend", ctx->stream, k_trend, dim3((unsigned)blocks), dim3(TR_THREADS), lds, nrows, (int)row_stride,
                     (int)col0, (int)ncol, (int)nseason, z_conf, d_x, d_out);
}
