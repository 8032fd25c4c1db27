// Host entries over the log-logistic part of csrc/xh_sindex_dev.h for tests/test_spei_host.py (ctypes): the fit of one sample
// (ranked by counting and scattered, as the kernel does), the distribution function element by element, and sp_std_index, the
// walk of k_std_index<log-logistic> (xh_sindex.hip) over a whole array on the host -- subtract, accumulate, rank and scatter,
// fit or take the parameters, evaluate -- with the same functions in the same order.
#include <cstdint>
#include <vector>

#include "xh_sindex_dev.h"

extern "C" {

// s: the sample in any order; sorted_out (n doubles, may be NULL) receives the scatter
void sp_fit(int32_t n, const double *s, double max_shape, double *out4, double *sorted_out) {
    std::vector<double> srt(n > 0 ? n : 1);
    for (int j = 0; j < n; ++j) srt[xh_si_rank([&](int i) { return s[i]; }, n, j)] = s[j];
    const XhSiLogLogistic p = xh_si_fit_loglogistic([&](int i) { return srt[i]; }, n, max_shape);
    out4[0] = p.alpha, out4[1] = p.beta, out4[2] = p.gamma, out4[3] = p.n;
    if (sorted_out)
        for (int j = 0; j < n; ++j) sorted_out[j] = srt[j];
}

void sp_cdf(int64_t nx, const double *X, const double *par4, double *H, double *index) {
    const XhSiLogLogistic p = {par4[0], par4[1], par4[2], par4[3]};
    for (int64_t i = 0; i < nx; ++i) {
        H[i] = xh_si_cdf_loglogistic(X[i], p);
        index[i] = xh_si_eval_loglogistic(X[i], p);
    }
}

// minus, par_in, par_out: [ncell, nmonths] / [ncell, 12, 4] or NULL
void sp_std_index(int64_t ncell, int32_t nmonths, int32_t k, int32_t ref0, int32_t ref_nyear, double max_shape, const double *x,
                  const double *minus, const double *par_in, double *par_out, double *index) {
    const int ref1 = ref0 + 12 * ref_nyear;
    std::vector<double> xs(nmonths), Xs(nmonths), srt(12 * (size_t)ref_nyear);
    for (int64_t c = 0; c < ncell; ++c) {
        for (int t = 0; t < nmonths; ++t) xs[t] = minus ? x[c * nmonths + t] - minus[c * nmonths + t] : x[c * nmonths + t];
        for (int t = 0; t < nmonths; ++t) {
            double acc = xh_si_nan();
            if (t >= k - 1) {
                acc = xs[t - k + 1];
                for (int j = t - k + 2; j <= t; ++j) acc += xs[j];
            }
            Xs[t] = acc;
        }
        double par[48];
        for (int m = 0; m < 12; ++m) {
            int u0 = ref0 + m;
            if (u0 < k - 1) u0 += 12 * ((k - 1 - u0 + 11) / 12);
            const int n = u0 < ref1 ? (ref1 - u0 + 11) / 12 : 0;
            if (par_in) {
                for (int j = 0; j < 4; ++j) par[4 * m + j] = par_in[c * 48 + 4 * m + j];
            } else {
                double *sm = srt.data() + (size_t)m * ref_nyear;
                for (int j = 0; j < n; ++j) sm[xh_si_rank([&](int i) { return Xs[u0 + 12 * i]; }, n, j)] = Xs[u0 + 12 * j];
                const XhSiLogLogistic p = xh_si_fit_loglogistic([&](int i) { return sm[i]; }, n, max_shape);
                par[4 * m] = p.alpha, par[4 * m + 1] = p.beta, par[4 * m + 2] = p.gamma, par[4 * m + 3] = p.n;
            }
            if (par_out)
                for (int j = 0; j < 4; ++j) par_out[c * 48 + 4 * m + j] = par[4 * m + j];
        }
        for (int t = 0; t < nmonths; ++t) {
            const int m = t % 12;
            const XhSiLogLogistic p = {par[4 * m], par[4 * m + 1], par[4 * m + 2], par[4 * m + 3]};
            index[c * nmonths + t] = xh_si_eval_loglogistic(Xs[t], p);
        }
    }
}

}  // extern "C"
