// Host entries over csrc/xh_extremes_dev.h for tests/test_extremes_host.py (ctypes): ep_extremes is the walk of k_extremes
// (xh_extremes.hip) over the rows on the host -- the same function, xh_extremes_row, with a team of one lane instead of a
// wavefront -- and the others are the definition's pieces, element by element.
#include <cstdint>
#include <vector>

#include "xh_extremes_dev.h"

extern "C" {

// x: [nrows, row_stride]; par_in: NULL or [nrows, 8]; table: [nrows, 8 + nT]; annual, t_year: NULL or [nrows, nyear].  The
// arguments xh_extremes refuses are refused here (return 1, nothing written).
int ep_extremes(int64_t nrows, int32_t row_stride, int32_t col0, int32_t nyear, int32_t kind, int32_t min_years, int32_t nT,
                const double *T, const double *x, const double *par_in, double *table, double *annual, double *t_year) {
    if (!x || !table || nrows < 0 || nyear < 1 || 12 * (int64_t)nyear > XH_EX_MAX_COLS || col0 < 0 ||
        (int64_t)col0 + 12 * (int64_t)nyear > row_stride || (kind != XH_EXTREMES_MAX && kind != XH_EXTREMES_MIN) ||
        min_years < XH_EX_MIN_YEARS || nT < 0 || nT > XH_EX_MAX_T || (nT > 0 && !T))
        return 1;
    for (int j = 0; j < nT; ++j)
        if (!(T[j] > 1.0)) return 1;
    std::vector<double> stage(XH_EX_STAGE), z(nyear), zs(nyear), sh(XH_EX_SH);
    const XhExSerial team;
    const int ncol = XH_EXTREMES_NPAR + nT;
    for (int64_t r = 0; r < nrows; ++r)
        xh_extremes_row(team, x + r * (int64_t)row_stride + col0, nyear, kind, min_years, nT, T,
                        par_in ? par_in + r * XH_EXTREMES_NPAR : nullptr, stage.data(), z.data(), zs.data(), sh.data(),
                        table + r * ncol, annual ? annual + r * nyear : nullptr, t_year ? t_year + r * nyear : nullptr);
    return 0;
}

void ep_k_of_t3(int64_t n, const double *t3, double *k) {
    for (int64_t i = 0; i < n; ++i) k[i] = xh_ex_k_of_t3(t3[i]);
}

void ep_parameters(int64_t n, const double *l1, const double *l2, const double *k, double *alpha, double *xi) {
    for (int64_t i = 0; i < n; ++i) xh_ex_parameters(l1[i], l2[i], k[i], alpha + i, xi + i);
}

void ep_quantile(int64_t n, const double *T, const double *k, const double *alpha, const double *xi, double *q) {
    for (int64_t i = 0; i < n; ++i) q[i] = xh_ex_quantile(T[i], k[i], alpha[i], xi[i]);
}

void ep_cdf(int64_t n, const double *z, const double *k, const double *alpha, const double *xi, double *F) {
    for (int64_t i = 0; i < n; ++i) F[i] = xh_ex_cdf(z[i], k[i], alpha[i], xi[i]);
}

void ep_return_period(int64_t n, const double *z, const double *k, const double *alpha, const double *xi, double *T) {
    for (int64_t i = 0; i < n; ++i) T[i] = xh_ex_return_period(z[i], k[i], alpha[i], xi[i]);
}

}  // extern "C"
