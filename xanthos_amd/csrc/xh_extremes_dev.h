// Frequency analysis of annual extremes of one row (xh_extremes.hip): annual maxima or minima of a monthly
// series, Hosking's sample L-moments (Hosking 1990), the generalized extreme value distribution fitted by them (Hosking &
// Wallis 1997; for minima the same fit of the negated series, the three-parameter Weibull distribution of low-flow analysis),
// return levels, and every year's return period under the fit.  Callable on the host and on the device, so that the same text
// runs in the kernel and in a probe on a machine without a GPU (tests/extremes_probe).  It mirrors no function of the
// reference: xanthos has no extreme-value statistics.
//
// DEFINITIONS (the contract; include/xanthos_hip.h restates them at xh_extremes).  No operation is contracted.
//   Input: one row x[0 .. 12 nyear), the window of a monthly series; year y is columns 12 y .. 12 y + 11.
//   1 Annual series.  a_y = the largest (kind = XH_EXTREMES_MAX) or smallest (XH_EXTREMES_MIN) of the year's 12 months, found
//     by comparisons from the first month on (v > a, v < a replaces a: of equal months the first stays).  A NaN or +-inf
//     month makes the year missing (a_y = NaN).  n = the number of years not missing.  z_y = a_y for max, -a_y for min.
//   2 Sample L-moments of the n values z.  Sorted ascending by counting (rank = #{smaller} + #{equal at an earlier year}, a
//     missing year after every number: xh_si_rank's rule), z_(0) <= ... <= z_(n-1).  The unbiased probability-weighted moments
//     b_r = (sum_i w_r(i) z_(i)) / (double)n, r = 0 .. 3 (defined for n > r), the sum from 0.0 over ascending rank i of the
//     rounded products, w_0(i) = 1, w_r(i) = (w_{r-1}(i) (double)(i - r + 1)) / (double)(n - r).
//     l1 = b0;  l2 = 2 b1 - b0;  l3 = (6 b2 - 6 b1) + b0;  l4 = ((20 b3 - 30 b2) + 12 b1) - b0;  t3 = l3 / l2;  t4 = l4 / l2.
//   3 GEV, Hosking's sign of the shape k (scipy.stats.genextreme's c).  k is the root of f(k) = (3 + t3) / 2,
//     f(k) = (1 - 3^-k) / (1 - 2^-k) = expm1(-k ln 3) / expm1(-k ln 2), f(0) = ln 3 / ln 2:  XH_EX_NEWTON = 10 Newton steps
//     k <- k - (f - (3 + t3) / 2) / (f dlog), always all of them, from Hosking's k0 = 7.8590 c + (2.9554 c) c, c = 2 / (3 + t3)
//     - ln 2 / ln 3.  (A sweep of 200,000 t3 in [-0.95, 0.99] is at its fixed point after 6 steps, [-0.999, -0.95] after 10;
//     "until |dk| is small" never ends at t3 = 0.17, where the last bits of k alternate.)  dlog = d log f / dk = ln 2 (B + 1) / B
//     - ln 3 (A + 1) / A with A = expm1(-k ln 3), B = expm1(-k ln 2); the two terms cancel like 1 / k, so below |k| < 2^-7 =
//     XH_EX_K_DLOG its series -(ln 3 - ln 2) / 2 + (ln^2 3 - ln^2 2) k / 12 - (ln^4 3 - ln^4 2) k^3 / 720 (next term 5e-5 k^5)
//     stands in; the derivative decides the speed of the steps only, not where they end.
//     G = tgamma(1 + k) (the mathematics library's);  alpha = (l2 d) / G, d = k / -expm1(-k ln 2), 1 / ln 2 at k = 0;
//     xi = l1 - alpha g, g = (1 - G) / k.  g cancels as k -> 0 (the Gumbel limit g = Euler's gamma, reached at t3 = 0.1699):
//     THE SWITCH-OVER is |k| < XH_EX_K_SERIES = 0.25, below which g = -(c_1 + c_2 k + ... + c_30 k^29) by Horner, c_j the Taylor
//     coefficients of Gamma(1 + x) (truncation 0.25^30 / 0.75 = 1e-18); at |k| >= 0.25 the quotient magnifies tgamma's rounding
//     4 times at most.  At k = 0 these are the Gumbel formulas alpha = l2 / ln 2, xi = l1 - gamma alpha.
//     NO FIT when n < min_years, when the series is constant (z_(0) = z_(n-1): its 2 b1 - b0 is rounding noise, 0 only for
//     a series of zeros), when l2 is not > 0, or when k <= -1, where the distribution has no mean.  k <= -1 is t3 >= 1, and
//     it is decided on t3, whose bits every build shares: no fit when t3 is not <= XH_EX_T3_MAX = 1 - 2^-20.  (A series
//     whose only non-zero year is its largest has t3 = 1 up to the rounding of its sums, which must not decide; and within
//     5e-7 of k = -1 Gamma(1 + k) magnifies the rounding of k a million times.)  A k that then still is not > -1 or not
//     finite gives no fit either.  The table row then holds n, l1 (n >= 1) and l2 (n >= 2) as computed, the rest is NaN.
//   4 Return level of period T > 1:  y = -log1p(-1 / T);  q = xi - alpha (expm1(k log y) / k), xi - alpha log y at k = 0.
//     Reported: q for max (exceeded once in T years on average), -q for min (undershot once in T years); l1 and xi are
//     reported negated back for min as well; l2, t3, t4, k, alpha are those of z.
//   5 Return period of year y:  s = (z_y - xi) / alpha;  u = -log F = exp(log1p(-k s) / k), exp(-s) at k = 0; outside the
//     support (-k s <= -1) u = 0 for k > 0 (above the upper bound: F = 1) and +inf for k < 0 (below the lower bound: F = 0);
//     T_y = -1 / expm1(-u): 1 at F = 0, +inf at F = 1.  NaN for a missing year or a row without a fit.
//   Output per row: the table XH_EXTREMES_NPAR + nT doubles n, l1, l2, t3, t4, k, alpha, xi, x_T...; the annual series a_y
//     [nyear]; T_y [nyear].  With a parameter row handed in (8 doubles n .. xi as reported), steps 2 and 3 are skipped: the 8
//     columns are copied, and steps 4 and 5 use them on this row's annual series (NaN parameters: no fit).
//
// HOW.  A `Team` does one row: lanes() workers, this one lane(), and sync() between a write to the team's memory and another
//   lane's read.  The kernel's team is one 64-lane wavefront with its slice of LDS; XhExSerial below is one host thread.
//   The months pass through `stage` 64 years at a time (team-strided loads: coalesced), lane <-> year forms a_y; lane <-> year
//   counts the year's rank over the series and scatters z_y to its sorted place; the lanes 0 .. 3 walk the sorted series for
//   b_0 .. b_3; then EVERY lane forms the same parameters from the four sums (the same instructions on the same numbers:
//   no lane waits for another), lane <-> T forms the return levels and lane <-> year T_y.
//   Team memory: stage [XH_EX_STAGE], z [nyear], zs [nyear], sh [XH_EX_SH] doubles.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XH_EX_HD __host__ __device__ __forceinline__
#else
#define XH_EX_HD inline
#endif
#include <cmath>
#include <cstdint>

#define XH_EXTREMES_NPAR 8
#define XH_EXTREMES_MAX 0
#define XH_EXTREMES_MIN 1
#define XH_EX_MAX_T 8
#define XH_EX_MAX_COLS 4096
#define XH_EX_MIN_YEARS 5
#define XH_EX_NEWTON 10
#define XH_EX_K_SERIES 0.25
#define XH_EX_K_DLOG 0.0078125
#define XH_EX_T3_MAX 0.99999904632568359375
#define XH_EX_CHUNK_YEARS 64
#define XH_EX_STAGE (12 * XH_EX_CHUNK_YEARS)
#define XH_EX_SH 8

#define XH_EX_LN2 0.6931471805599453094
#define XH_EX_LN3 1.0986122886681096914
#define XH_EX_EULER 0.57721566490153286061

XH_EX_HD double xh_ex_nan() { return __builtin_nan(""); }
XH_EX_HD double xh_ex_inf() { return __builtin_inf(); }
XH_EX_HD bool xh_ex_finite(double v) { return v - v == 0.0; }

struct XhExSerial {
    int lane() const { return 0; }
    int lanes() const { return 1; }
    void sync() const {}
};

// a_y of the 12 months at m
XH_EX_HD double xh_ex_annual(const double *m, int kind) {
    double a = m[0];
    bool ok = xh_ex_finite(a);
    for (int j = 1; j < 12; ++j) {
        const double v = m[j];
        ok = ok && xh_ex_finite(v);
        if (kind == XH_EXTREMES_MAX ? (v > a) : (v < a)) a = v;
    }
    return ok ? a : xh_ex_nan();
}

// rank of year j of z[0 .. nyear) (NaN = missing, after every number and after the missing years before it)
XH_EX_HD int xh_ex_rank(const double *z, int nyear, int j) {
    const double x = z[j];
    const bool xnan = x != x;
    int r = 0;
    for (int i = 0; i < nyear; ++i) {
        const double v = z[i];
        const bool less = xnan ? (v == v) : (v < x);
        const bool same = xnan ? (v != v) : (v == x);
        r += (less || (same && i < j)) ? 1 : 0;
    }
    return r;
}

// b_r of the sorted zs[0 .. n), n > r
XH_EX_HD double xh_ex_pwm(const double *zs, int n, int r) {
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        double w = 1.0;
        for (int j = 1; j <= r; ++j) w = (w * (double)(i - j + 1)) / (double)(n - j);
        sum += w * zs[i];
    }
    return sum / (double)n;
}

XH_EX_HD double xh_ex_k_of_t3(double t3) {
    const double target = (3.0 + t3) / 2.0;
    const double c = 2.0 / (3.0 + t3) - XH_EX_LN2 / XH_EX_LN3;
    double k = 7.8590 * c + (2.9554 * c) * c;
    const double l2 = XH_EX_LN2, l3 = XH_EX_LN3;
    for (int it = 0; it < XH_EX_NEWTON; ++it) {
        const double A = expm1(-k * l3), B = expm1(-k * l2);
        const double f = k == 0.0 ? l3 / l2 : A / B;
        const double series = (-(l3 - l2) / 2.0 + ((l3 * l3 - l2 * l2) / 12.0) * k) -
                              (((l3 * l3) * (l3 * l3) - (l2 * l2) * (l2 * l2)) / 720.0) * ((k * k) * k);
        const double direct = (l2 * (B + 1.0)) / B - (l3 * (A + 1.0)) / A;
        const double dlog = fabs(k) < XH_EX_K_DLOG ? series : direct;
        k = k - (f - target) / (f * dlog);
    }
    return k;
}

// (1 - Gamma(1 + k)) / k, gam = tgamma(1 + k)
XH_EX_HD double xh_ex_gamma1_over_k(double k, double gam) {
    if (!(fabs(k) < XH_EX_K_SERIES)) return (1.0 - gam) / k;
    // Gamma(1 + x) = 1 + sum_j c_j x^j, j = 1 .. 30 (40-digit values, rounded once)
    const double c[30] = {
        -0.57721566490153286061, 0.9890559953279725554,  -0.90747907608088628902, 0.98172808683440018734, -0.9819950689031452021,
        0.99314911462127619315,  -0.99600176044243153397, 0.99810569378312892198, -0.99902526762195486779, 0.99951565607277744107,
        -0.99975659750860128703, 0.99987827131513327573, -0.99993906420644431684, 0.9999695177634821045,  -0.99998475269937704874,
        0.99999237447907321586,  -0.99999618658947331203, 0.99999809308113089205, -0.99999904646891115772, 0.99999952321060573958,
        -0.99999976159734438057, 0.99999988079601916842, -0.99999994039712498375, 0.99999997019826758236, -0.99999998509903547505,
        0.99999999254948496246,  -0.99999999627473155544, 0.99999999813736213559, -0.99999999906867985371, 0.99999999953433952215};
    double p = c[29];
    for (int j = 28; j >= 0; --j) p = p * k + c[j];
    return -p;
}

// alpha, xi from l1, l2 (of z) and k
XH_EX_HD void xh_ex_parameters(double l1, double l2, double k, double *alpha, double *xi) {
    const double gam = tgamma(1.0 + k);
    const double d = k == 0.0 ? 1.0 / XH_EX_LN2 : k / -expm1(-k * XH_EX_LN2);
    *alpha = (l2 * d) / gam;
    *xi = l1 - *alpha * xh_ex_gamma1_over_k(k, gam);
}

// the value of z exceeded once in T years on average
XH_EX_HD double xh_ex_quantile(double T, double k, double alpha, double xi) {
    const double ly = log(-log1p(-1.0 / T));
    return k == 0.0 ? xi - alpha * ly : xi - alpha * (expm1(k * ly) / k);
}

// T = 1 / (1 - F(z))
XH_EX_HD double xh_ex_return_period(double z, double k, double alpha, double xi) {
    const double s = (z - xi) / alpha;
    if (s != s || k != k) return xh_ex_nan();
    const double t = -k * s;
    double u;
    if (k == 0.0) u = exp(-s);
    else if (t <= -1.0) u = k > 0.0 ? 0.0 : xh_ex_inf();
    else u = exp(log1p(t) / k);
    return -1.0 / expm1(-u);
}

// F(z) itself (the probe's; T_y does not pass through it)
XH_EX_HD double xh_ex_cdf(double z, double k, double alpha, double xi) {
    const double s = (z - xi) / alpha;
    if (s != s || k != k) return xh_ex_nan();
    const double t = -k * s;
    if (k == 0.0) return exp(-exp(-s));
    if (t <= -1.0) return k > 0.0 ? 1.0 : 0.0;
    return exp(-exp(log1p(t) / k));
}

// One row.  src: the 12 nyear months of the window; T: nT return periods; par_in: NULL or the row's 8 parameters; stage, z, zs,
// sh: the team's memory (see HOW); table: the row's 8 + nT doubles; annual, t_year: the row's nyear doubles each, or NULL.
template <class Team>
XH_EX_HD void xh_extremes_row(const Team &team, const double *src, int nyear, int kind, int min_years, int nT, const double *T,
                              const double *par_in, double *stage, double *z, double *zs, double *sh, double *table,
                              double *annual, double *t_year) {
    const double nan = xh_ex_nan();
    const bool neg = kind == XH_EXTREMES_MIN;
    for (int y0 = 0; y0 < nyear; y0 += XH_EX_CHUNK_YEARS) {
        const int cy = nyear - y0 < XH_EX_CHUNK_YEARS ? nyear - y0 : XH_EX_CHUNK_YEARS;
        for (int t = team.lane(); t < 12 * cy; t += team.lanes()) stage[t] = src[12 * y0 + t];
        team.sync();
        for (int y = team.lane(); y < cy; y += team.lanes()) {
            const double ay = xh_ex_annual(stage + 12 * y, kind);
            z[y0 + y] = neg ? -ay : ay;         // (a_y is -z_y again, bit for bit)
        }
        team.sync();                            // (stage is rewritten by the next 64 years)
    }
    double par[XH_EXTREMES_NPAR];               // n, l1, l2, t3, t4, k, alpha, xi of z
    if (par_in) {
        for (int i = 0; i < XH_EXTREMES_NPAR; ++i) par[i] = par_in[i];
        if (neg) par[1] = -par[1], par[7] = -par[7];
    } else {
        for (int y = team.lane(); y < nyear; y += team.lanes()) zs[xh_ex_rank(z, nyear, y)] = z[y];
        int n = 0;
        for (int y = 0; y < nyear; ++y) n += (z[y] == z[y]) ? 1 : 0;
        team.sync();
        for (int r = team.lane(); r < 4; r += team.lanes()) sh[r] = n > r ? xh_ex_pwm(zs, n, r) : nan;
        team.sync();
        const double b0 = sh[0], b1 = sh[1], b2 = sh[2], b3 = sh[3];
        const double l1 = b0, l2 = 2.0 * b1 - b0;
        const double l3 = (6.0 * b2 - 6.0 * b1) + b0, l4 = ((20.0 * b3 - 30.0 * b2) + 12.0 * b1) - b0;
        par[0] = (double)n, par[1] = l1, par[2] = l2;
        par[3] = par[4] = par[5] = par[6] = par[7] = nan;
        if (n >= min_years && zs[0] < zs[n - 1] && l2 > 0.0) {
            const double t3 = l3 / l2, k = t3 <= XH_EX_T3_MAX ? xh_ex_k_of_t3(t3) : nan;
            if (k > -1.0 && xh_ex_finite(k)) {
                par[3] = t3, par[4] = l4 / l2, par[5] = k;
                xh_ex_parameters(l1, l2, k, &par[6], &par[7]);
            }
        }
    }
    const double k = par[5], alpha = par[6], xi = par[7];
    if (team.lane() == 0) {
        for (int i = 0; i < XH_EXTREMES_NPAR; ++i) table[i] = (neg && (i == 1 || i == 7)) ? -par[i] : par[i];
    }
    for (int j = team.lane(); j < nT; j += team.lanes()) {
        const double q = xh_ex_quantile(T[j], k, alpha, xi);
        table[XH_EXTREMES_NPAR + j] = neg ? -q : q;
    }
    for (int y = team.lane(); y < nyear; y += team.lanes()) {
        const double zy = z[y];
        if (annual) annual[y] = neg ? -zy : zy;
        if (t_year) t_year[y] = xh_ex_return_period(zy, k, alpha, xi);
    }
    team.sync();                                // (z, zs and sh are rewritten by the team's next row)
}
