// Host entries over csrc/xh_wbalance_dev.h for tests/test_wbalance_host.py (ctypes): wp_water_balance is the walk of k_wbalance
// (xh_wbalance.hip) over the rows on the host -- the same function, xh_wbalance_row, with a team of one lane instead of a
// workgroup -- and wp_omega / wp_fu are Fu's parameter and Fu's curve alone.
#include <cstdint>
#include <vector>

#include "xh_wbalance_dev.h"

extern "C" {

// p, pet, q, aet (or NULL): [nrows, row_stride]; table: [nrows, 21]; annual: NULL or [nrows, 4, nyear]; xcorr: NULL or
// [nrows, max_lag + 1].  The arguments xh_water_balance refuses are refused here (return 1, nothing written).
int wp_water_balance(int64_t nrows, int32_t row_stride, int32_t col0, int32_t nyear, int32_t max_lag, double omega0, const double *p,
                     const double *pet, const double *q, const double *aet, double *table, double *annual, double *xcorr) {
    if (!p || !pet || !q || !table || nrows < 0 || nyear < 1 || 12 * (int64_t)nyear > XH_WB_MAX_COLS || col0 < 0 ||
        (int64_t)col0 + 12 * (int64_t)nyear > row_stride || max_lag < 0 || max_lag > XH_WB_MAX_LAG ||
        !(omega0 - omega0 == 0.0 && omega0 > 1.0))
        return 1;
    const int P2 = xh_sig_pow2(nyear);
    std::vector<double> bp(12 * nyear), bq(12 * nyear), sh(XH_WB_NSUM * XH_WB_LANES), ann(4 * nyear), es(2 * P2), misc(XH_WB_MISC);
    const XhSigSerial team;
    for (int64_t r = 0; r < nrows; ++r) {
        const int64_t at = r * (int64_t)row_stride + col0;
        xh_wbalance_row(team, p + at, pet + at, q + at, aet ? aet + at : nullptr, nyear, max_lag, omega0, bp.data(), bq.data(),
                        sh.data(), ann.data(), es.data(), misc.data(), table + r * XH_WB_NCOL,
                        annual ? annual + r * 4 * (int64_t)nyear : nullptr, xcorr ? xcorr + r * (int64_t)(max_lag + 1) : nullptr, nullptr);
    }
    return 0;
}

void wp_omega(int64_t n, const double *phi, const double *eps, double *omega) {
    for (int64_t i = 0; i < n; ++i) omega[i] = xh_wb_omega(phi[i], eps[i]);
}

void wp_fu(int64_t n, const double *phi, double omega, double *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = xh_wb_fu(phi[i], omega);
}

}  // extern "C"
