// Standardized drought indices on the device: SRI of runoff (Shukla & Wood 2008), its analogues of soil
// moisture (SSI) and streamflow (SSFI), SPI of precipitation (McKee et al. 1993) and SPEI of the climatic water balance
// precipitation - PET (Vicente-Serrano et al. 2010), at accumulation scales of 1 - 48 months.  xh_std_index / xh_std_index2
// replace no function of the reference: xanthos/drought/drought_stats.py offers a fixed threshold and Sheffield & Wood's
// severity, intensity and duration (xh_drought.hip); a user who wants a standardized index downloads the arrays and runs scipy
// per cell and calendar month.
//
// The definitions (accumulated series, reference sample, Thom's gamma fit, Gringorten's empirical position, the log-logistic
// fit by unbiased probability-weighted moments, ndtri and the clip at +-3.09) stand in xh_sindex_dev.h with the scalar
// functions that implement them; this file is the walk over the cells.
//
//   k_std_index<DIST>   one workgroup of 256 lanes per cell at a time (grid-stride over the cells), one instantiation per
//   distribution (the gamma and the empirical one carry nothing of the log-logistic one: neither its LDS row nor its code):
//     1  the cell's row x[c, :] -- minus y[c, :] when a subtrahend is given, one rounded subtraction -- comes from HBM once,
//        coalesced, into LDS (8 B per month, 32 KB at the 4096-month limit) and serves every scale;
//     2  per scale k, lane <-> month: X[t] = ((x[t-k+1] + x[t-k+2]) + ...) + x[t], left to right, from LDS into a second LDS
//        row (NaN for t < k - 1);
//     3  gamma: lanes 0 .. 11 fit one calendar month each (xh_si_fit_gamma walks the month's reference sample in ascending
//        order: the sums of the definition, in its order) -- or lanes 0 .. 47 copy the cell's rows of a parameter table --
//        into 48 doubles of LDS, which go to the parameter output as they are;
//        log-logistic: all 256 lanes, lane <-> element of the reference period (12 ref_nyear <= 4096 of them, strided), rank
//        their element within its calendar month's sample by counting (xh_si_rank: #{s < x} + #{s = x at an earlier u}; the
//        64 lanes of a wave read 12 neighbouring doubles per step, a conflict-free broadcast) and scatter it into a THIRD LDS
//        row, slot m ref_nyear + rank: the 12 sorted samples.  Then lanes 0 .. 11 form the three sums of their month in the
//        definition's order (xh_si_fit_loglogistic) -- or lanes 0 .. 47 copy a table, and nothing is ranked;
//     4  lane <-> month again: the index of X[t] from the month's parameters (gamma: P(alpha, X / beta) and ndtri, the
//        expensive part; log-logistic: one log, one exp, ndtri) or by counting the month's reference sample in LDS
//        (empirical), written coalesced.
//   LDS: 16 B per month + 384 B; log-logistic 24 B per month + 384 B (98 KB at 4092 months, inside gfx950's 160 KB; the launch
//   raises the kernel's dynamic-LDS limit).  No atomics, a fixed operation order: two calls give the same bits, and a scale's
//   result does not depend on the other scales of the call.  Gamma is bound by the incomplete-gamma iterations (two f64
//   divisions each), log-logistic by the 12 n^2 LDS reads of the ranking and the two divisions per element of the sums, not
//   by HBM (8 or 16 B in once and 8 B out per scale and cell-month).
#include "xh_launch.h"
#include "xh_sindex_dev.h"

namespace {

constexpr int SI_THREADS = 256;
constexpr int SI_MAX_SCALES = 8;
constexpr int SI_MAX_SCALE = 48;
constexpr int SI_MAX_MONTHS = 4096;

struct SiArgs {
    int scale[SI_MAX_SCALES];
    const double *par_in[SI_MAX_SCALES];
    double *par_out[SI_MAX_SCALES];
    double *index[SI_MAX_SCALES];
};

template <int DIST>
__global__ void __launch_bounds__(SI_THREADS) k_std_index(int64_t ncell, int nmonths, int nscale, int ref0, int ref_nyear,
                                                         double max_shape, const double *__restrict__ x,
                                                         const double *__restrict__ y, SiArgs a) {
    extern __shared__ double lds[];
    double *xs = lds;                       // [nmonths] the cell's row
    double *Xs = lds + nmonths;             // [nmonths] its accumulation at the current scale
    // log-logistic: [12, ref_nyear] the sorted reference samples (12 ref_nyear <= nmonths), then the parameters
    double *srt = lds + 2 * (size_t)nmonths;
    double *par = lds + (DIST == XH_SI_LOGLOGISTIC ? 3 : 2) * (size_t)nmonths;  // [12, 4]
    const int tid = threadIdx.x;
    const int ref1 = ref0 + 12 * ref_nyear;
    for (int64_t c = blockIdx.x; c < ncell; c += gridDim.x) {
        const double *row = x + c * (int64_t)nmonths;
        if (y) {
            const double *sub = y + c * (int64_t)nmonths;
            for (int t = tid; t < nmonths; t += SI_THREADS) xs[t] = row[t] - sub[t];
        } else {
            for (int t = tid; t < nmonths; t += SI_THREADS) xs[t] = row[t];
        }
        __syncthreads();
        for (int s = 0; s < nscale; ++s) {
            const int k = a.scale[s];
            for (int t = tid; t < nmonths; t += SI_THREADS) {
                double acc = xh_si_nan();
                if (t >= k - 1) {
                    acc = xs[t - k + 1];
                    for (int j = t - k + 2; j <= t; ++j) acc += xs[j];
                }
                Xs[t] = acc;
            }
            __syncthreads();
            // the reference sample of calendar month m: Xs[u0(m) + 12 i], i in [0, n(m)); u0 the first month of the
            // reference period with u mod 12 = m and u >= k - 1 (ref0 is a multiple of 12)
            auto first = [&](int m) {
                int u = ref0 + m;
                if (u < k - 1) u += 12 * ((k - 1 - u + 11) / 12);
                return u;
            };
            if constexpr (DIST == XH_SI_GAMMA) {
                if (a.par_in[s]) {
                    if (tid < 48) par[tid] = a.par_in[s][c * 48 + tid];
                } else if (tid < 12) {
                    const int u0 = first(tid);
                    const int n = u0 < ref1 ? (ref1 - u0 + 11) / 12 : 0;
                    const XhSiPar p = xh_si_fit_gamma([&](int i) { return Xs[u0 + 12 * i]; }, n, max_shape);
                    par[4 * tid + 0] = p.q0;
                    par[4 * tid + 1] = p.alpha;
                    par[4 * tid + 2] = p.beta;
                    par[4 * tid + 3] = p.n;
                }
                __syncthreads();
                if (a.par_out[s] && tid < 48) a.par_out[s][c * 48 + tid] = par[tid];
                double *out = a.index[s] + c * (int64_t)nmonths;
                for (int t = tid; t < nmonths; t += SI_THREADS) {
                    const int m = t % 12;
                    const XhSiPar p = {par[4 * m], par[4 * m + 1], par[4 * m + 2], par[4 * m + 3]};
                    out[t] = xh_si_eval_gamma(Xs[t], p);
                }
            } else if constexpr (DIST == XH_SI_LOGLOGISTIC) {
                if (a.par_in[s]) {
                    if (tid < 48) par[tid] = a.par_in[s][c * 48 + tid];
                } else {
                    // element e of the reference period is month u = ref0 + e, calendar month e mod 12; it is element
                    // j = (u - u0) / 12 of its sample when u >= u0, and its rank < n <= ref_nyear keeps the scatter inside
                    // the month's slots [m ref_nyear, (m + 1) ref_nyear)
                    for (int e = tid; e < 12 * ref_nyear; e += SI_THREADS) {
                        const int m = e % 12, u = ref0 + e, u0 = first(m);
                        if (u < u0) continue;
                        const int n = (ref1 - u0 + 11) / 12;
                        const int r = xh_si_rank([&](int i) { return Xs[u0 + 12 * i]; }, n, (u - u0) / 12);
                        srt[m * ref_nyear + r] = Xs[u];
                    }
                    __syncthreads();
                    if (tid < 12) {
                        const int u0 = first(tid);
                        const int n = u0 < ref1 ? (ref1 - u0 + 11) / 12 : 0;
                        const double *sm = srt + tid * ref_nyear;
                        const XhSiLogLogistic p = xh_si_fit_loglogistic([&](int i) { return sm[i]; }, n, max_shape);
                        par[4 * tid + 0] = p.alpha;
                        par[4 * tid + 1] = p.beta;
                        par[4 * tid + 2] = p.gamma;
                        par[4 * tid + 3] = p.n;
                    }
                }
                __syncthreads();
                if (a.par_out[s] && tid < 48) a.par_out[s][c * 48 + tid] = par[tid];
                double *out = a.index[s] + c * (int64_t)nmonths;
                for (int t = tid; t < nmonths; t += SI_THREADS) {
                    const int m = t % 12;
                    const XhSiLogLogistic p = {par[4 * m], par[4 * m + 1], par[4 * m + 2], par[4 * m + 3]};
                    out[t] = xh_si_eval_loglogistic(Xs[t], p);
                }
            } else {
                double *out = a.index[s] + c * (int64_t)nmonths;
                for (int t = tid; t < nmonths; t += SI_THREADS) {
                    const int u0 = first(t % 12);
                    const int n = u0 < ref1 ? (ref1 - u0 + 11) / 12 : 0;
                    const int in_ref = (t >= ref0 && t < ref1) ? 1 : 0;
                    out[t] = xh_si_eval_empirical(Xs[t], [&](int i) { return Xs[u0 + 12 * i]; }, n, in_ref);
                }
            }
            __syncthreads();                // Xs, srt and par are rewritten by the next scale, xs by the next cell
        }
    }
}

}  // namespace

extern "C" int xh_std_index2(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t nscale, const int32_t *h_scale,
                             int32_t ref_month0, int32_t ref_nyear, int32_t dist, double max_shape, const double *d_x,
                             const double *d_minus, const double *const *h_d_par_in, double *const *h_d_par_out,
                             double *const *h_d_index) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, d_x && h_scale && h_d_index && ncell >= 0, "xh_std_index: NULL array or negative ncell");
    XH_REQUIRE(ctx, nmonths > 0 && nmonths % 12 == 0, "xh_std_index: nmonths (%d) must be whole years", nmonths);
    if (nmonths > SI_MAX_MONTHS) {
        return xh_fail(ctx, XH_ERR_LIMIT, "xh_std_index: nmonths (%d) exceeds the %d months a cell's row may take in LDS", nmonths, SI_MAX_MONTHS);
    }
    if (nscale < 1 || nscale > SI_MAX_SCALES) {
        return xh_fail(ctx, XH_ERR_LIMIT, "xh_std_index: nscale (%d) outside 1..%d", nscale, SI_MAX_SCALES);
    }
    XH_REQUIRE(ctx, dist == XH_SI_GAMMA || dist == XH_SI_EMPIRICAL || dist == XH_SI_LOGLOGISTIC,
               "xh_std_index: dist (%d) is none of gamma (0), empirical (1), log-logistic (2)", dist);
    XH_REQUIRE(ctx, !(h_d_par_in && dist == XH_SI_EMPIRICAL), "xh_std_index: a parameter table (par_in) has no meaning with the "
               "empirical distribution");
    XH_REQUIRE(ctx, max_shape > 0.0, "xh_std_index: max_shape (%g) must be positive", max_shape);
    XH_REQUIRE(ctx, ref_month0 >= 0 && ref_month0 % 12 == 0 && ref_nyear >= 1 &&
               (int64_t)ref_month0 + 12 * (int64_t)ref_nyear <= nmonths,
               "xh_std_index: reference period (month %d, %d years) is not whole years inside the %d months", ref_month0,
               ref_nyear, nmonths);
    SiArgs a = {};
    for (int s = 0; s < nscale; ++s) {
        if (h_scale[s] < 1 || h_scale[s] > SI_MAX_SCALE) {
            return xh_fail(ctx, XH_ERR_LIMIT, "xh_std_index: scale %d (%d months) outside 1..%d", s, h_scale[s], SI_MAX_SCALE);
        }
        XH_REQUIRE(ctx, h_d_index[s], "xh_std_index: index array of scale %d is NULL", s);
        XH_REQUIRE(ctx, !h_d_par_in || h_d_par_in[s], "xh_std_index: par_in of scale %d is NULL", s);
        a.scale[s] = h_scale[s];
        a.par_in[s] = h_d_par_in ? h_d_par_in[s] : nullptr;
        a.par_out[s] = (h_d_par_out && dist != XH_SI_EMPIRICAL) ? h_d_par_out[s] : nullptr;
        a.index[s] = h_d_index[s];
    }
    if (ncell == 0) return XH_OK;
    // the sorted samples of the log-logistic fit are a third row: 12 ref_nyear <= nmonths doubles
    const size_t lds = ((dist == XH_SI_LOGLOGISTIC ? 3 : 2) * (size_t)nmonths + 48) * sizeof(double);
    int64_t blocks = (int64_t)ctx->prop.multiProcessorCount * 8;
    if (blocks > ncell) blocks = ncell;
    auto *kernel = dist == XH_SI_GAMMA ? k_std_index<XH_SI_GAMMA>
                   : dist == XH_SI_EMPIRICAL ? k_std_index<XH_SI_EMPIRICAL> : k_std_index<XH_SI_LOGLOGISTIC>;
    if (dist == XH_SI_LOGLOGISTIC && lds > 64 * 1024) {
        // beyond the 64 KB a kernel may take without asking (the two-row instantiations pass it by 320 B at most, which the
        // runtime has always granted; 98 KB it is asked for.  A device without that much LDS fails the launch, which is
        // checked like every launch: nothing runs.)
        XH_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    return xh_launch(ctx, "std_index", ctx->stream, kernel, dim3((unsigned)blocks), dim3(SI_THREADS), lds, ncell,
                     (int)nmonths, (int)nscale, (int)ref_month0, (int)ref_nyear, max_shape, d_x, d_minus, a);
}

extern "C" int xh_std_index(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t nscale, const int32_t *h_scale,
                            int32_t ref_month0, int32_t ref_nyear, int32_t dist, double max_shape, const double *d_x,
                            const double *const *h_d_par_in, double *const *h_d_par_out, double *const *h_d_index) {
    return xh_std_index2(ctx, ncell, nmonths, nscale, h_scale, ref_month0, ref_nyear, dist, max_shape, d_x, nullptr, h_d_par_in,
                         h_d_par_out, h_d_index);
}
