// Flood and low-flow frequency analysis per row on the device: how large is the 10-, 50-, 100-year maximum of
// runoff, streamflow or precipitation in this cell, how low does it fall once in 10 years, and how rare was each year's extreme?
// xh_extremes replaces no function of the reference: xanthos has no extreme-value statistics; a user downloads the arrays and
// loops a maximum-likelihood fit over the rows.
//
// The definitions (annual series, sample L-moments by a counted sort, the GEV by L-moments with its Gumbel limit, return
// levels, each year's return period) and the whole walk over one row stand in xh_extremes_dev.h, host-callable; this file
// gives that walk its team -- one wavefront -- and its memory, and walks the rows.
//
//   k_extremes   one WAVEFRONT per row at a time, EX_WAVES = 4 wavefronts to a workgroup, each walking its own rows (a stride
//   of all the grid's wavefronts) in its own slice of LDS; no workgroup barrier anywhere: the work of a row (12 nyear loads,
//   nyear^2 / 64 comparisons per lane, four sums of nyear terms, one root) is too small for 256 lanes, which would idle on about
//   50 annual values.  Between a write to the slice and another lane's read stands a wavefront barrier (the LDS operations
//   of one wavefront complete in order; the barrier keeps the compiler from moving them).
//     1  the window's months come from HBM once, 768 at a time by consecutive lanes, into the slice's stage; lane <-> year
//        reduces 12 of them to z_y;
//     2  lane <-> year counts its rank over z (every lane reads the same LDS word: a broadcast) and scatters;
//     3  lanes 0 .. 3 sum b_0 .. b_3 in rank order;
//     4  every lane forms l1 .. xi from the four sums (the same instructions on the same numbers);
//     5  lane <-> T the return levels, lane <-> year T_y and a_y, consecutive lanes to consecutive addresses.
//   LDS per wavefront: (768 + 2 nyear + 8) doubles = 6.9 KB at 600 columns (27 KB per workgroup: 5 workgroups fit a CU's
//   160 KB), 11.5 KB at the 4092-column end of the limit (46 KB per workgroup, 3 per CU).  Registers: see DESIGN 4.21.
//   No atomics and a fixed operation order: two calls give the same bits.
#include "xh_extremes_dev.h"
#include "xh_launch.h"

namespace {

constexpr int EX_WAVE = 64;
constexpr int EX_WAVES = 4;

struct ExWave {
    __device__ __forceinline__ int lane() const { return threadIdx.x & (EX_WAVE - 1); }
    __device__ __forceinline__ int lanes() const { return EX_WAVE; }
    __device__ __forceinline__ void sync() const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
};

struct ExPeriods {
    double T[XH_EX_MAX_T];
};

__global__ void __launch_bounds__(EX_WAVE *EX_WAVES) k_extremes(int64_t nrows, int row_stride, int col0, int nyear, int kind,
                                                               int min_years, int nT, ExPeriods periods,
                                                               const double *__restrict__ x, const double *__restrict__ par_in,
                                                               double *__restrict__ table, double *__restrict__ annual,
                                                               double *__restrict__ t_year) {
    extern __shared__ double lds[];
    const int wave = threadIdx.x / EX_WAVE;
    const int per_wave = XH_EX_STAGE + 2 * nyear + XH_EX_SH;
    double *stage = lds + (size_t)wave * per_wave;
    double *z = stage + XH_EX_STAGE, *zs = z + nyear, *sh = zs + nyear;
    const ExWave team;
    const int ncol = XH_EXTREMES_NPAR + nT;
    for (int64_t r = (int64_t)blockIdx.x * EX_WAVES + wave; r < nrows; r += (int64_t)gridDim.x * EX_WAVES) {
        xh_extremes_row(team, x + r * (int64_t)row_stride + col0, nyear, kind, min_years, nT, periods.T,
                        par_in ? par_in + r * XH_EXTREMES_NPAR : nullptr, stage, z, zs, sh, table + r * ncol,
                        annual ? annual + r * nyear : nullptr, t_year ? t_year + r * nyear : nullptr);
    }
}

}  // namespace

extern "C" int xh_extremes(xh_ctx *ctx, int64_t nrows, int32_t row_stride, int32_t col0, int32_t nyear, int32_t kind,
                           int32_t min_years, int32_t nT, const double *h_T, const double *d_x, const double *d_par_in,
                           double *d_table, double *d_annual, double *d_T_year) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, d_x && d_table && nrows >= 0, "xh_extremes: NULL array or negative nrows");
    XH_REQUIRE(ctx, nyear >= 1 && 12 * (int64_t)nyear <= XH_EX_MAX_COLS,
               "xh_extremes: nyear (%d) must be at least 1 and 12 nyear at most %d columns", nyear, XH_EX_MAX_COLS);
    XH_REQUIRE(ctx, col0 >= 0 && (int64_t)col0 + 12 * (int64_t)nyear <= row_stride,
               "xh_extremes: the window (column %d, %d years = %d columns) does not lie inside a row of %d", col0, nyear,
               12 * nyear, row_stride);
    XH_REQUIRE(ctx, kind == XH_EXTREMES_MAX || kind == XH_EXTREMES_MIN, "xh_extremes: kind (%d) is neither max (0) nor min (1)", kind);
    XH_REQUIRE(ctx, min_years >= XH_EX_MIN_YEARS, "xh_extremes: min_years (%d) must be at least %d", min_years, XH_EX_MIN_YEARS);
    XH_REQUIRE(ctx, nT >= 0 && nT <= XH_EX_MAX_T, "xh_extremes: nT (%d) outside 0..%d", nT, XH_EX_MAX_T);
    XH_REQUIRE(ctx, nT == 0 || h_T, "xh_extremes: NULL return periods");
    ExPeriods periods;
    for (int j = 0; j < XH_EX_MAX_T; ++j) {
        periods.T[j] = j < nT ? h_T[j] : 2.0;
        XH_REQUIRE(ctx, periods.T[j] > 1.0, "xh_extremes: return period %d (%g) must be > 1", j, periods.T[j]);
    }
    if (nrows == 0) return XH_OK;
    const size_t lds = (size_t)EX_WAVES * (XH_EX_STAGE + 2 * (size_t)nyear + XH_EX_SH) * sizeof(double);
    int64_t blocks = (nrows + EX_WAVES - 1) / EX_WAVES;
    const int64_t cap = (int64_t)ctx->prop.multiProcessorCount * 16;
    if (blocks > cap) blocks = cap;
    return xh_launch(ctx, "extremes", ctx->stream, k_extremes, dim3((unsigned)blocks), dim3(EX_WAVE * EX_WAVES), lds, nrows,
                     (int)row_stride, (int)col0, (int)nyear, (int)kind, (int)min_years, (int)nT, periods, d_x, d_par_in, d_table,
                     d_annual, d_T_year);
}
