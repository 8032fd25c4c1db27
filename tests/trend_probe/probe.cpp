// Host entry over csrc/xh_trend_dev.h for tests/test_trend_host.py (ctypes): tp_trend is the walk of k_trend (xh_trend.hip)
// over the rows on the host -- the same function, xh_trend_row, with a team of one lane instead of a workgroup.
#include <cstdint>
#include <vector>

#include "xh_trend_dev.h"

extern "C" {

// x: [nrows, row_stride]; out: [nrows, 10].  The arguments xh_trend refuses are refused here (return 1, nothing written).
int tp_trend(int64_t nrows, int32_t row_stride, int32_t col0, int32_t ncol, int32_t nseason, double z_conf, const double *x,
             double *out) {
    if (!x || !out || nrows < 0 || nseason < 1 || nseason > 12 || col0 < 0 || ncol < 1 || ncol > XH_TR_MAX_COLS ||
        (int64_t)col0 + ncol > row_stride || ncol % nseason != 0 || !(z_conf < 0.0) || !xh_tr_finite(z_conf))
        return 1;
    std::vector<double> xs(ncol);
    std::vector<uint32_t> hist(XH_TR_MAX_RANKS * 256);
    XhTrSel st;
    const XhTrSerial team;
    for (int64_t r = 0; r < nrows; ++r)
        xh_trend_row(team, x + r * (int64_t)row_stride + col0, ncol, nseason, z_conf, xs.data(), hist.data(), &st,
                     out + r * XH_TREND_NCOL);
    return 0;
}

}  // extern "C"
