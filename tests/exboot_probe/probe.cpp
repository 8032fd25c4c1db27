// Host entries over csrc/xh_exboot_dev.h for tests/test_exboot_host.py (ctypes): ep_exboot is the walk of k_exboot
// (xh_exboot.hip) over the rows on the host -- the same function, xh_exboot_row, with a team of one lane instead of a
// wavefront --, ep_draws the indices of one replicate and ep_percentile the header's selection and lerp.
#include <cstdint>
#include <vector>

#include "xh_exboot_dev.h"

extern "C" {

// x: [nrows, row_stride]; ci: [nrows, 3 + 2 nT]; rep: NULL or [nrows, B, 5 + nT].  The arguments xh_extremes_boot refuses are
// refused here (return 1, nothing written).
int ep_exboot(int64_t nrows, int32_t row_stride, int32_t col0, int32_t nyear, int32_t kind, int32_t min_years, int32_t nT,
              const double *T, int32_t B, double confidence, uint64_t seed, int64_t row0, const double *x, double *ci, double *rep) {
    if (!x || !ci || nrows < 0 || nyear < 1 || 12 * (int64_t)nyear > XH_EX_MAX_COLS || col0 < 0 ||
        (int64_t)col0 + 12 * (int64_t)nyear > row_stride || (kind != XH_EXTREMES_MAX && kind != XH_EXTREMES_MIN) ||
        min_years < XH_EX_MIN_YEARS || nT < 0 || nT > XH_EX_MAX_T || (nT > 0 && !T) || B < XH_EXB_MIN_B || B > XH_EXB_MAX_B ||
        !(confidence > 0.0 && confidence < 1.0) || row0 < 0)
        return 1;
    for (int j = 0; j < nT; ++j)
        if (!(T[j] > 1.0)) return 1;
    const int n2 = xh_exb_n2(B);
    std::vector<double> stage(XH_EX_STAGE), z(nyear), zs(nyear), sh(XH_EX_SH), tab(XH_EXTREMES_NPAR), w(3 * (size_t)nyear), sortbuf(n2);
    std::vector<double> vals((size_t)(1 + nT) * B);
    std::vector<uint16_t> cnt(nyear);
    int nfit[1];
    const XhExSerial team;
    const double p_lo = (1.0 - confidence) / 2.0, p_hi = 1.0 - p_lo;
    const int64_t nrep = (int64_t)B * (XH_EXB_NREP + nT);
    for (int64_t r = 0; r < nrows; ++r)
        xh_exboot_row(team, x + r * (int64_t)row_stride + col0, nyear, kind, min_years, nT, T, B, p_lo, p_hi, seed, row0 + r,
                      stage.data(), z.data(), zs.data(), sh.data(), tab.data(), w.data(), cnt.data(), nfit, sortbuf.data(),
                      vals.data(), ci + r * (3 + 2 * nT), rep ? rep + r * nrep : nullptr);
    return 0;
}

// j_i, i = 0 .. n - 1, of replicate b of row `row`
void ep_draws(uint64_t seed, int64_t row, int32_t b, int32_t n, int32_t *j) {
    const uint64_t h_rep = xh_exb_rep_key(xh_exb_row_key(seed, row), b);
    for (int i = 0; i < n; ++i) j[i] = xh_exb_index(xh_exb_word(h_rep, i >> 1), i, n);
}

// the `linear` quantile p of the nb values v (no NaN): the header's sort of the next power of two and its lerp
double ep_percentile(int32_t nb, const double *v, double p) {
    const int n2 = xh_exb_n2(nb);
    std::vector<double> buf(n2, xh_ex_inf());
    for (int i = 0; i < nb; ++i) buf[i] = v[i];
    xh_exb_sort(XhExSerial(), buf.data(), n2);
    return xh_exb_percentile(buf.data(), nb, p);
}

}  // extern "C"
