// Host entries over csrc/xh_sindex_dev.h for tests/test_sindex_host.py (ctypes): the scalar functions element by element, and
// si_std_index, the walk of k_std_index (xh_sindex.hip) over a whole array on the host -- accumulate, fit or take the
// parameters, evaluate -- with the same functions in the same order.
#include <cstdint>

#include "xh_sindex_dev.h"

extern "C" {

void si_gammap(int64_t n, const double *a, const double *x, double *out, int32_t *iters) {
    for (int64_t i = 0; i < n; ++i) {
        int it = 0;
        out[i] = xh_si_gammap(a[i], x[i], &it);
        iters[i] = it;
    }
}

void si_ndtri(int64_t n, const double *p, double *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = xh_si_ndtri(p[i]);
}

int32_t si_maxit(void) { return XH_SI_MAXIT; }

void si_fit_gamma(int32_t n, const double *s, double max_shape, double *out4) {
    const XhSiPar p = xh_si_fit_gamma([&](int i) { return s[i]; }, n, max_shape);
    out4[0] = p.q0;
    out4[1] = p.alpha;
    out4[2] = p.beta;
    out4[3] = p.n;
}

void si_eval_empirical(int64_t nx, const double *X, const int32_t *in_ref, int32_t n, const double *s, double *out) {
    for (int64_t i = 0; i < nx; ++i) out[i] = xh_si_eval_empirical(X[i], [&](int j) { return s[j]; }, n, in_ref[i]);
}

// dist: 0 gamma, 1 empirical; par_in / par_out [ncell, 12, 4] or NULL; X_out [ncell, nmonths] or NULL
void si_std_index(int64_t ncell, int32_t nmonths, int32_t k, int32_t ref0, int32_t ref_nyear, int32_t dist, double max_shape,
                  const double *x, const double *par_in, double *par_out, double *X_out, double *index) {
    const int ref1 = ref0 + 12 * ref_nyear;
    double *Xs = new double[nmonths];
    for (int64_t c = 0; c < ncell; ++c) {
        const double *xs = x + c * nmonths;
        for (int t = 0; t < nmonths; ++t) {
            double acc = xh_si_nan();
            if (t >= k - 1) {
                acc = xs[t - k + 1];
                for (int j = t - k + 2; j <= t; ++j) acc += xs[j];
            }
            Xs[t] = acc;
            if (X_out) X_out[c * nmonths + t] = acc;
        }
        double par[48];
        int u0s[12], ns[12];
        for (int m = 0; m < 12; ++m) {
            int u0 = ref0 + m;
            if (u0 < k - 1) u0 += 12 * ((k - 1 - u0 + 11) / 12);
            u0s[m] = u0;
            ns[m] = u0 < ref1 ? (ref1 - u0 + 11) / 12 : 0;
            if (dist != XH_SI_GAMMA) continue;
            if (par_in) {
                for (int j = 0; j < 4; ++j) par[4 * m + j] = par_in[c * 48 + 4 * m + j];
            } else {
                const XhSiPar p = xh_si_fit_gamma([&](int i) { return Xs[u0 + 12 * i]; }, ns[m], max_shape);
                par[4 * m] = p.q0, par[4 * m + 1] = p.alpha, par[4 * m + 2] = p.beta, par[4 * m + 3] = p.n;
            }
            if (par_out)
                for (int j = 0; j < 4; ++j) par_out[c * 48 + 4 * m + j] = par[4 * m + j];
        }
        for (int t = 0; t < nmonths; ++t) {
            const int m = t % 12;
            if (dist == XH_SI_GAMMA) {
                const XhSiPar p = {par[4 * m], par[4 * m + 1], par[4 * m + 2], par[4 * m + 3]};
                index[c * nmonths + t] = xh_si_eval_gamma(Xs[t], p);
            } else {
                const int u0 = u0s[m];
                const int in_ref = (t >= ref0 && t < ref1) ? 1 : 0;
                index[c * nmonths + t] = xh_si_eval_empirical(Xs[t], [&](int i) { return Xs[u0 + 12 * i]; }, ns[m], in_ref);
            }
        }
    }
    delete[] Xs;
}

}  // extern "C"
