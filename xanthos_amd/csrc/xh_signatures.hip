// Flow duration curves and flow-regime signatures per row on the device: what flow is exceeded 95 % of the time
// in this cell, how variable and how persistent it is, in which month it peaks, how seasonal it is and how much its annual
// totals vary.  xh_signatures replaces no function of the reference: xanthos has no flow signatures; a user downloads the
// arrays and sorts every row in numpy.
//
// The definitions (the S256 sums, the order statistics by numpy's linear rule, the calendar means and the annual totals) and the
// whole walk over one row stand in xh_signatures_dev.h, host-callable; this file gives that walk its team -- one workgroup --
// and its memory, and walks the rows.
//
//   k_signatures   one 256-lane WORKGROUP per row at a time, each walking its own rows (a stride of the grid).  The row comes
//   from HBM once, by consecutive lanes, into LDS padded to the next power of two P with +inf for what is left out; there it
//   gives, in the order of time, the six S256 sums in two passes of three (256 strided partial sums and the tree of
//   xh_block_sum256 each), the annual totals (lane <-> year) and the calendar means (lane <-> month), then the regime's columns
//   on lane 0 while the first lane of the second wavefront walks the annual totals; then a bitonic sort in place --
//   one pass for the phases k = 2 and 4, then per phase one pass per step j >= 4 and one for j = 2 and 1, the passes inside 4
//   consecutive elements in registers; consecutive lanes touch consecutive doubles in every pass -- puts the included values
//   first, and lane <-> probability reads the order statistics.  Lane 0 writes columns 0 .. 7, the first lane of the second
//   wavefront the slope.
//   Barriers: a sort pass with j <= 64 and a tree level with stride <= 32 stay inside one wavefront's elements, so only a
//   wavefront barrier stands after them; at 600 columns 10 of the sort's 45 passes end in a workgroup barrier.
//   Registers: held to 64 VGPRs (8 waves per SIMD = 8 workgroups per CU; 228 B of scratch per lane, in the one-lane chains of log
//   and atan2): the row's work is chains of LDS round trips and barriers, and what hides them is other workgroups -- measured at
//   67,420 x 600: 3.21 ms at 3 workgroups per CU (157 VGPRs, no scratch), 2.51 at 4, 2.44 at 5, 2.39 at 6, 1.93 at 8
//   (profiles/signatures/).
//   LDS per workgroup: (P + 768 + nyear + 32) doubles = 14.6 KB at 600 columns (P = 1024), 40.9 KB at the 4092-column end of the
//   limit (P = 4096).  No atomics, nothing crosses a workgroup, every trip count is known at launch: two calls give the same
//   bytes whatever the grid.
#include "xh_signatures_dev.h"
#include "xh_launch.h"

namespace {

struct SigTeam {
    __device__ __forceinline__ int lane() const { return threadIdx.x; }
    __device__ __forceinline__ int lanes() const { return XH_SIG_LANES; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    // (the LDS operations of one wavefront complete in order; the barrier keeps the compiler from moving them)
    __device__ __forceinline__ void sync_wave() const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
};

struct SigProbs {
    double p[XH_SIG_MAX_P];
};

__global__ void __launch_bounds__(XH_SIG_LANES, 8) k_signatures(int64_t nrows, int row_stride, int col0, int nyear, int cal0, int nP,
                                                            SigProbs probs, const double *__restrict__ x,
                                                            double *__restrict__ table, double *__restrict__ fdc,
                                                            double *__restrict__ regime) {
    extern __shared__ double lds[];
    const int P = xh_sig_pow2(12 * nyear);
    double *buf = lds, *sh = buf + P, *ann = sh + 3 * XH_SIG_LANES, *misc = ann + nyear;
    const SigTeam team;
    for (int64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
        xh_signatures_row(team, x + r * (int64_t)row_stride + col0, nyear, cal0, nP, probs.p, buf, sh, ann, misc,
                          table + r * XH_SIG_NCOL, fdc ? fdc + r * nP : nullptr, regime ? regime + r * 12 : nullptr);
    }
}

}  // namespace

extern "C" int xh_signatures(xh_ctx *ctx, int64_t nrows, int32_t row_stride, int32_t col0, int32_t nyear, int32_t cal0, int32_t nP,
                             const double *h_prob, const double *d_x, double *d_table, double *d_fdc, double *d_regime) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, d_x && d_table && nrows >= 0, "xh_signatures: NULL array (d_x %p, d_table %p) or negative nrows (%lld)",
               (const void *)d_x, (const void *)d_table, (long long)nrows);
    XH_REQUIRE(ctx, nyear >= 1 && 12 * (int64_t)nyear <= XH_SIG_MAX_COLS,
               "xh_signatures: nyear (%d) must be at least 1 and 12 nyear at most %d columns", nyear, XH_SIG_MAX_COLS);
    XH_REQUIRE(ctx, col0 >= 0 && (int64_t)col0 + 12 * (int64_t)nyear <= row_stride,
               "xh_signatures: the window (column %d, %d years = %d columns) does not lie inside a row of %d", col0, nyear,
               12 * nyear, row_stride);
    XH_REQUIRE(ctx, cal0 >= 0 && cal0 <= 11, "xh_signatures: cal0 (%d) outside 0..11", cal0);
    XH_REQUIRE(ctx, nP >= 0 && nP <= XH_SIG_MAX_P, "xh_signatures: nP (%d) outside 0..%d", nP, XH_SIG_MAX_P);
    XH_REQUIRE(ctx, nP == 0 || h_prob, "xh_signatures: NULL probabilities with nP = %d", nP);
    SigProbs probs;
    for (int j = 0; j < XH_SIG_MAX_P; ++j) {
        probs.p[j] = j < nP ? h_prob[j] : 0.5;
        XH_REQUIRE(ctx, probs.p[j] > 0.0 && probs.p[j] < 1.0, "xh_signatures: probability %d (%g) must lie strictly between 0 and 1",
                   j, probs.p[j]);
    }
    if (nrows == 0) return XH_OK;
    const size_t lds = ((size_t)xh_sig_pow2(12 * nyear) + 3 * XH_SIG_LANES + (size_t)nyear + XH_SIG_MISC) * sizeof(double);
    int64_t blocks = nrows;
    const int64_t cap = (int64_t)ctx->prop.multiProcessorCount * 8;
    if (blocks > cap) blocks = cap;
    return xh_launch(ctx, "signatures", ctx->stream, k_signatures, dim3((unsigned)blocks), dim3(XH_SIG_LANES), lds, nrows,
                     (int)row_stride, (int)col0, (int)nyear, (int)cal0, (int)nP, probs, d_x, d_table, d_fdc, d_regime);
}
