// Water balance and Budyko signatures per row on the device: runoff ratio, aridity and evaporative index, the
// closure of the balance, Fu's parameter and the departure from a Budyko curve, the elasticities of runoff to precipitation and
// to PET, and the lag at which runoff answers precipitation.  xh_water_balance replaces no function of the reference: xanthos has
// no signatures of two variables; a user downloads the four arrays and loops over the rows in numpy.
//
// The definitions and the whole walk over one row stand in xh_wbalance_dev.h, host-callable; this file gives that walk its team
// -- one workgroup -- and its memory, and walks the rows.
//
//   k_wbalance   one 256-lane WORKGROUP per row at a time, each walking its own rows (a stride of the grid).  The four rows come
//   from HBM once, by consecutive lanes; P and Q go into LDS, a month that is not included as NaN in both, so that one buffer
//   carries the mask; PET and AET are used where they are loaded (the inclusion and the dry months) and read again, from the
//   cache, for the annual totals (lane <-> year).  Then two or more passes of five S256 sums over the months (the sums of
//   squares and the numerators of the c_k), three passes of five Y256 sums over the years, the e_y of both elasticities sorted
//   by the bitonic network of xh_signatures_dev.h, and at the end three lanes of three wavefronts side by side: the table, phi and
//   eps put aside, the c_k.  The 60 bisection steps of Fu's parameter are one chain per row that no second lane can shorten: the
//   workgroup forms them for 256 of its rows at once, one lane each, after the last of them (4.98 -> 2.63 ms at 67,420 x 600 and 4 workgroups per CU).
//   LDS per workgroup: (24 nyear + 1280 + 4 nyear + 2 P2 + 16 + 512) doubles, P2 the power of two >= nyear: 26.7 KB at 600
//   columns (6 workgroups per CU), 99.0 KB at the 4092-column end of the limit, where the entry asks for it (above 64 KB) and
//   one workgroup fits a CU.
//   Registers: compiled for 6 workgroups per CU, which measured fastest (80 VGPRs, 516 B of scratch per lane, the spills in
//   the bisection's chains): 3.71 ms at 2 (191 VGPRs, no scratch), 2.63 at 4, 2.26 at 6 (profiles/water_balance/).
//   No atomics, nothing crosses a workgroup, every trip count is known at launch: two calls give the same bytes whatever the
//   grid.
#include "xh_wbalance_dev.h"
#include "xh_launch.h"

namespace {

struct WbTeam {
    __device__ __forceinline__ int lane() const { return threadIdx.x; }
    __device__ __forceinline__ int lanes() const { return XH_WB_LANES; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    // (the LDS operations of one wavefront complete in order; the barrier keeps the compiler from moving them)
    __device__ __forceinline__ void sync_wave() const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
};

// workgroups per CU the kernel is compiled and launched for (profiles/water_balance/occupancy_sweep.json)
#ifndef XH_WB_PER_CU
#define XH_WB_PER_CU 6
#endif
constexpr int WB_PER_CU = XH_WB_PER_CU;

size_t wb_lds_doubles(int nyear) {
    return (size_t)24 * nyear + XH_WB_NSUM * XH_WB_LANES + (size_t)4 * nyear + 2 * (size_t)xh_sig_pow2(nyear) + XH_WB_MISC +
           2 * XH_WB_LANES;
}

__global__ void __launch_bounds__(XH_WB_LANES, WB_PER_CU) k_wbalance(int64_t nrows, int row_stride, int col0, int nyear, int max_lag,
                                                                   double omega0, const double *__restrict__ p,
                                                                   const double *__restrict__ pet, const double *__restrict__ q,
                                                                   const double *__restrict__ aet, double *__restrict__ table,
                                                                   double *__restrict__ annual, double *__restrict__ xcorr) {
    extern __shared__ double lds[];
    const int ncol = 12 * nyear, P2 = xh_sig_pow2(nyear);
    double *bp = lds, *bq = bp + ncol, *sh = bq + ncol, *ann = sh + XH_WB_NSUM * XH_WB_LANES, *es = ann + 4 * nyear, *misc = es + 2 * P2;
    double *later = misc + XH_WB_MISC;
    const WbTeam team;
    // this workgroup's rows are blockIdx.x + i gridDim.x, i = 0 .. mine - 1; phi and eps of 256 of them wait in `later`, and
    // then every lane runs the 60 bisection steps of one row: the one chain of a row that no second lane can shorten
    const int64_t mine = nrows > blockIdx.x ? (nrows - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    for (int64_t i = 0; i < mine; ++i) {
        const int64_t r = blockIdx.x + i * gridDim.x, at = r * (int64_t)row_stride + col0;
        const int slot = (int)(i % XH_WB_LANES);
        xh_wbalance_row(team, p + at, pet + at, q + at, aet ? aet + at : nullptr, nyear, max_lag, omega0, bp, bq, sh, ann, es, misc,
                        table + r * XH_WB_NCOL, annual ? annual + r * 4 * (int64_t)nyear : nullptr,
                        xcorr ? xcorr + r * (int64_t)(max_lag + 1) : nullptr, later + 2 * slot);
        if (slot == XH_WB_LANES - 1 || i == mine - 1) {                // (the row's walk ended in a barrier)
            if ((int)threadIdx.x <= slot) {
                const int64_t rl = blockIdx.x + (i - slot + threadIdx.x) * gridDim.x;
                xh_wb_budyko(later[2 * threadIdx.x], later[2 * threadIdx.x + 1], omega0, table + rl * XH_WB_NCOL);
            }
            __syncthreads();
        }
    }
}

}  // namespace

extern "C" int xh_water_balance(xh_ctx *ctx, int64_t nrows, int32_t row_stride, int32_t col0, int32_t nyear, int32_t max_lag,
                                double omega0, const double *d_p, const double *d_pet, const double *d_q, const double *d_aet,
                                double *d_table, double *d_annual, double *d_xcorr) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, d_p && d_pet && d_q && d_table && nrows >= 0,
               "xh_water_balance: NULL array (d_p %p, d_pet %p, d_q %p, d_table %p) or negative nrows (%lld)", (const void *)d_p,
               (const void *)d_pet, (const void *)d_q, (const void *)d_table, (long long)nrows);
    XH_REQUIRE(ctx, nyear >= 1 && 12 * (int64_t)nyear <= XH_WB_MAX_COLS,
               "xh_water_balance: nyear (%d) must be at least 1 and 12 nyear at most %d columns", nyear, XH_WB_MAX_COLS);
    XH_REQUIRE(ctx, col0 >= 0 && (int64_t)col0 + 12 * (int64_t)nyear <= row_stride,
               "xh_water_balance: the window (column %d, %d years = %d columns) does not lie inside a row of %d", col0, nyear,
               12 * nyear, row_stride);
    XH_REQUIRE(ctx, max_lag >= 0 && max_lag <= XH_WB_MAX_LAG, "xh_water_balance: max_lag (%d) outside 0..%d", max_lag, XH_WB_MAX_LAG);
    XH_REQUIRE(ctx, omega0 - omega0 == 0.0 && omega0 > 1.0, "xh_water_balance: omega0 (%g) must be finite and > 1", omega0);
    if (nrows == 0) return XH_OK;
    const size_t lds = wb_lds_doubles(nyear) * sizeof(double);
    int64_t blocks = nrows;
    const int64_t cap = (int64_t)ctx->prop.multiProcessorCount * WB_PER_CU;
    if (blocks > cap) blocks = cap;
    if (lds > 64 * 1024)        // beyond what a kernel may take without asking: 99,040 B at the most (341 years)
        XH_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_wbalance), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return xh_launch(ctx, "water_balance", ctx->stream, k_wbalance, dim3((unsigned)blocks), dim3(XH_WB_LANES), lds, nrows,
                     (int)row_stride, (int)col0, (int)nyear, (int)max_lag, omega0, d_p, d_pet, d_q, d_aet, d_table, d_annual, d_xcorr);
}
