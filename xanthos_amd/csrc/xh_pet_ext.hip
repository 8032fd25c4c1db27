// Hargreaves-Samani and Thornthwaite PET on gfx950 (fp64).
//
// Replaces xanthos/pet/hargreaves_samani.py:execute (:95-119) with its per-element pet() (:34-64), and
// xanthos/pet/thornthwaite.py:execute (:51-130) with calc_daylight_hours (:18-48).
//
// Launches:
//   k_hs_lat        per cell: phi = lat * pi / 180 (hargreaves_samani.py:50), cos(phi) and tan(phi) (scratch)
//   k_hs_pet        one lane per (cell, month) element in C order, as k_hargreaves_pet (xh_gwam.hip): lane i takes element
//                   base + i; cos / tan of the 12 mid-month declinations come from a small table, the days of each month
//                   of the run from another
//   k_trn_daylight  one thread per (cell, month of a common or a leap year): the mean of arccos(clip(-tan(phi) tan(dec_d)))
//                   x 24 / pi over the month's days, summed in day order -> [ncell, 24] (12 common months, 12 leap)
//   k_trn_pet       one thread per (cell, year) group of 12 contiguous months.  A block of 256 groups moves its 3,072
//                   contiguous elements through LDS (rows padded to 13 doubles), so that every global access is
//                   coalesced; each thread then forms the heat index I, the exponent a and the 12 PET values of its year.
//
// Thornthwaite's month-order quirk (thornthwaite.py:113): np.repeat(L, nyears, axis=1) instead of a tile gives global
// month m of a common year the daylight of month-of-year m // nyears; leap years are then overwritten with the correctly
// tiled leap table (:119-122).  XH_DAYLIGHT_REFERENCE reproduces that, XH_DAYLIGHT_MONTHLY gives every month its own.
#include <cmath>
#include <cstdint>
#include <vector>

#include "xh_launch.h"

namespace {

constexpr double PI = 3.141592653589793;

// ---------------------------------------------------------------------------------------------- Hargreaves-Samani
struct HsMonth {
    double cos_dec, tan_dec;
};

__global__ void __launch_bounds__(256) k_hs_lat(int64_t ncell, const double *__restrict__ lat, double *__restrict__ trig) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    const double phi = lat[c] * PI / 180.0;                      // hargreaves_samani.py:50
    trig[c] = cos(phi);
    trig[ncell + c] = tan(phi);
}

__global__ void __launch_bounds__(256) k_hs_pet(int64_t n, int nmonths, int64_t ncell, const double *__restrict__ tas,
                                                const double *__restrict__ tmax, const double *__restrict__ tmin,
                                                const double *__restrict__ trig, const HsMonth *__restrict__ tab,
                                                const double *__restrict__ ndays, double *__restrict__ pet) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t c;
        int m;
        if (n <= 0xffffffffll) {                      // 32-bit quotient (the 0.5-degree grid has 40 M elements at 600 months)
            const uint32_t u = (uint32_t)i;
            c = u / (uint32_t)nmonths;
            m = (int)(u - (uint32_t)c * (uint32_t)nmonths);
        } else {
            c = i / nmonths;
            m = (int)(i - c * nmonths);
        }
        const double t = tas[i];
        if (t < 0.0) {                                           // :36-37 (NaN is not < 0 and goes on to give NaN)
            pet[i] = 0.0;
            continue;
        }
        const double tx = tmax[i], tm = tmin[i];
        const HsMonth d = tab[m % 12];                           // :42-48: j[mth % 12]
        const double cphi = trig[c], tphi = trig[ncell + c];
        const double tn = -d.tan_dec * tphi;                     // :52
        const double acs = (tn < -1.0 || tn > 1.0) ? 0.0 : acos(tn);                  // :54-57
        const double ra = 118.0 / PI * acs + cphi * d.cos_dec * sin(acs);            // :60, as written
        const double p = 0.408 * 0.0023 * ra * (t + 17.8) * sqrt(fabs(tx - tm));    // :63
        pet[i] = p * ndays[m];                                   // :115: mm/day -> mm/month
    }
}

// ---------------------------------------------------------------------------------------------- Thornthwaite
__constant__ int c_month_days[2][12] = {{31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31},
                                        {31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31}};

// dl[c * 24 + k]: k < 12 month k of a common year, k >= 12 month k - 12 of a leap year (thornthwaite.py:18-48)
__global__ void __launch_bounds__(256) k_trn_daylight(int64_t ncell, const double *__restrict__ lat,
                                                      const double *__restrict__ tan_dec, double *__restrict__ dl) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncell * 24) return;
    const int64_t c = i / 24;
    const int k = (int)(i - c * 24);
    const int leap = k >= 12, mo = k - 12 * leap;
    int d0 = 0;
    for (int j = 0; j < mo; ++j) d0 += c_month_days[leap][j];
    const int nd = c_month_days[leap][mo];
    const double mt = -tan(lat[c]);                              // :35: -tan(lat) * tan(dec)
    double s = 0.0;
    for (int d = d0; d < d0 + nd; ++d) {
        double x = mt * tan_dec[d];
        x = x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x);               // np.clip: NaN stays NaN
        s += acos(x) * (24.0 / PI);                              // :36, :39
    }
    dl[i] = s / (double)nd;                                      // :40-42
}

constexpr int TG = 256;            // (cell, year) groups per block = threads per block
constexpr int TLD = 13;            // padded LDS row of one group (doubles)

__global__ void __launch_bounds__(TG) k_trn_pet(int64_t ngroups, int nyears, int start_year, int monthly,
                                                const double *__restrict__ tas, const double *__restrict__ dl,
                                                double *__restrict__ pet) {
    __shared__ double T[TG * TLD];
    const int tid = threadIdx.x;
    const int64_t g0 = (int64_t)blockIdx.x * TG;
    const int ng = (int)(ngroups - g0 < TG ? ngroups - g0 : TG);
    const int nel = ng * 12;
    const double *__restrict__ src = tas + g0 * 12;
    for (int e = tid; e < nel; e += TG) T[e + e / 12] = src[e];
    __syncthreads();
    if (tid < ng) {
        const int64_t g = g0 + tid;
        const int64_t c = g / nyears;
        const int y = (int)(g - c * nyears);
        double *row = T + tid * TLD;
        double t[12];
        double I = 0.0;
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const double v = row[k];
            t[k] = (v != v || v < 0.0) ? 0.0 : v;                // :85: NaN and negatives -> 0
            I += pow(t[k] / 5.0, 1.514);                         // :91, :94
        }
        const double a = (.000000675 * pow(I, 3.0)) - (.0000771 * (I * I)) + (.0179 * I) + .492;     // :97
        const int yr = start_year + y;
        const int leap = (yr % 4 == 0 && yr % 100 != 0) || yr % 400 == 0;        // calendar.isleap (:116)
        const double *__restrict__ L = dl + c * 24;
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            double pu = I != 0.0 ? 10.0 * t[k] / I : 0.0;        // :107
            pu = 16.0 * pow(pu, a);                              // :108
            const int col = leap ? 12 + k : (monthly ? k : (12 * y + k) / nyears);  // :113-122
            const double n = (double)c_month_days[leap][k];
            row[k] = pu * (L[col] / 12.0) * (n / 30.0);          // :131
        }
    }
    __syncthreads();
    double *__restrict__ dst = pet + g0 * 12;
    for (int e = tid; e < nel; e += TG) dst[e] = T[e + e / 12];
}

}  // namespace

extern "C" int xh_hs_pet(xh_ctx *ctx, int64_t ncell, int32_t nmonths, const double *d_tas, const double *d_tmax,
                         const double *d_tmin, const double *d_lat_deg, const double *h_ndays, double *d_pet) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, ncell >= 0 && nmonths > 0, "xh_hs_pet: bad size");
    XH_REQUIRE(ctx, d_tas && d_tmax && d_tmin && d_lat_deg && h_ndays && d_pet, "xh_hs_pet: NULL argument");
    if (ncell == 0) return XH_OK;
    // the mid-month declinations on the host (libm), as the reference takes them of numpy scalars (:40-48)
    static const int j[12] = {15, 45, 75, 105, 135, 165, 195, 225, 255, 285, 315, 345};
    std::vector<HsMonth> tab(12);
    for (int m = 0; m < 12; ++m) {
        const double delta = 0.4102 * std::sin(2 * (PI / 365) * (j[m] - 80));
        tab[m] = HsMonth{std::cos(delta), std::tan(delta)};
    }
    void *at[3];
    const int rc = xh_stage(ctx, 2, {{tab.data(), sizeof(HsMonth) * 12}, {h_ndays, sizeof(double) * nmonths}},
                            sizeof(double) * 2 * ncell, at);
    if (rc) return rc;
    const HsMonth *d_tab = static_cast<const HsMonth *>(at[0]);
    const double *d_nd = static_cast<const double *>(at[1]);
    double *d_trig = static_cast<double *>(at[2]);
    const int64_t n = ncell * (int64_t)nmonths;
    return xh_timed(ctx, "hs_pet", ctx->stream, [&] {
        const int rc = xh_launch(ctx, nullptr, ctx->stream, k_hs_lat, xh_grid(ctx, ncell, 256), 256, 0, ncell, d_lat_deg, d_trig);
        if (rc) return rc;
        return xh_launch(ctx, nullptr, ctx->stream, k_hs_pet, xh_grid(ctx, n, 256, 32), 256, 0, n, (int)nmonths, ncell, d_tas,
                         d_tmax, d_tmin, d_trig, d_tab, d_nd, d_pet);
    });
}

extern "C" int xh_thornthwaite_pet(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t start_year, int32_t daylight_mode,
                                   const double *d_tas, const double *d_lat_rad, double *d_pet, double *d_daylight) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, ncell >= 0 && nmonths >= 0 && nmonths % 12 == 0,
               "xh_thornthwaite_pet: nmonths (%d) must be whole years", nmonths);
    XH_REQUIRE(ctx, daylight_mode == XH_DAYLIGHT_REFERENCE || daylight_mode == XH_DAYLIGHT_MONTHLY,
               "xh_thornthwaite_pet: bad daylight mode %d", daylight_mode);
    XH_REQUIRE(ctx, d_lat_rad && (nmonths == 0 || (d_tas && d_pet)), "xh_thornthwaite_pet: NULL argument");
    if (ncell == 0) return XH_OK;
    // tan of the solar declination of days 1..366 (thornthwaite.py:29-32) on the host (libm)
    std::vector<double> tdec(366);
    for (int d = 0; d < 366; ++d) tdec[d] = std::tan(0.409 * std::sin(((2 * PI / 365.0) * (d + 1) - 1.39)));
    void *at[2];
    int rc = xh_stage(ctx, 2, {{tdec.data(), sizeof(double) * 366}}, d_daylight ? 0 : sizeof(double) * 24 * ncell, at);
    if (rc) return rc;
    double *d_dl = d_daylight ? d_daylight : static_cast<double *>(at[1]);
    rc = xh_launch(ctx, "trn_daylight", ctx->stream, k_trn_daylight, xh_grid(ctx, ncell * 24, 256), 256, 0, ncell, d_lat_rad,
                   static_cast<const double *>(at[0]), d_dl);
    if (rc || nmonths == 0) return rc;
    const int nyears = nmonths / 12;
    const int64_t ngroups = ncell * (int64_t)nyears;
    return xh_launch(ctx, "trn_pet", ctx->stream, k_trn_pet, xh_grid(ctx, ngroups, TG), TG, 0, ngroups, nyears, (int)start_year,
                     (int)(daylight_mode == XH_DAYLIGHT_MONTHLY), d_tas, d_dl, d_pet);
}
