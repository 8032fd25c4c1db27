// Host entries over csrc/xh_signatures_dev.h for tests/test_signatures_host.py (ctypes): sp_signatures is the walk of
// k_signatures (xh_signatures.hip) over the rows on the host -- the same function, xh_signatures_row, with a team of one lane
// instead of a workgroup -- and sp_quantile is the order statistic alone.
#include <cstdint>
#include <vector>

#include "xh_signatures_dev.h"

extern "C" {

// x: [nrows, row_stride]; table: [nrows, 18]; fdc: NULL or [nrows, nP]; regime: NULL or [nrows, 12].  The arguments
// xh_signatures refuses are refused here (return 1, nothing written).
int sp_signatures(int64_t nrows, int32_t row_stride, int32_t col0, int32_t nyear, int32_t cal0, int32_t nP, const double *prob,
                  const double *x, double *table, double *fdc, double *regime) {
    if (!x || !table || nrows < 0 || nyear < 1 || 12 * (int64_t)nyear > XH_SIG_MAX_COLS || col0 < 0 ||
        (int64_t)col0 + 12 * (int64_t)nyear > row_stride || cal0 < 0 || cal0 > 11 || nP < 0 || nP > XH_SIG_MAX_P ||
        (nP > 0 && !prob))
        return 1;
    for (int j = 0; j < nP; ++j)
        if (!(prob[j] > 0.0 && prob[j] < 1.0)) return 1;
    const int P = xh_sig_pow2(12 * nyear);
    std::vector<double> buf(P), sh(3 * XH_SIG_LANES), ann(nyear), misc(XH_SIG_MISC);
    const XhSigSerial team;
    for (int64_t r = 0; r < nrows; ++r)
        xh_signatures_row(team, x + r * (int64_t)row_stride + col0, nyear, cal0, nP, prob, buf.data(), sh.data(), ann.data(),
                          misc.data(), table + r * XH_SIG_NCOL, fdc ? fdc + r * nP : nullptr, regime ? regime + r * 12 : nullptr);
    return 0;
}

// q[i] = the linear quantile p[i] of sorted[0 .. n)
void sp_quantile(int32_t n, const double *sorted, int64_t np, const double *p, double *q) {
    for (int64_t i = 0; i < np; ++i) q[i] = xh_sig_quantile(sorted, n, p[i]);
}

}  // extern "C"
