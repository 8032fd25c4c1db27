// Flow duration curve and flow-regime signatures of one row (xh_signatures.hip): what flow is exceeded 95 % of the
// time, how variable and how persistent the series is, in which month it peaks and how seasonal it is, and how much its annual
// totals vary.  Callable on the host and on the device, so that the same text runs in the kernel and in a probe on a machine
// without a GPU (tests/signatures_probe).  It mirrors no function of the reference: xanthos has no flow signatures.
//
// DEFINITIONS (the contract; include/xanthos_hip.h restates them at xh_signatures).  No operation is contracted.
//   Input: one row x[0 .. 12 nyear), the window of a monthly series; column t has calendar month (cal0 + t) mod 12, 0 = January;
//   year y of the window is columns 12 y .. 12 y + 11.  Every element enters as x + 0.0 (-0.0 counts as +0.0); a NaN or +-inf
//   element is left out of everything.  n = the number of elements left in.
//   S256(f): lane l of 256 adds f(t) from 0.0 over the included t = l, l + 256, ... in ascending order; the 256 partial sums are
//     joined by the tree of xh_block_sum256 (csrc/xh_kge.h: sh[l] += sh[l + stride], stride = 128, 64, ..., 1).  A "pair" is
//     (t, t + 1) with both elements included.  "Sequential": from 0.0 in ascending index order.
//   Order statistics: the n included values sorted ascending a[0 .. n); Q(p) is numpy's `linear` quantile, h = (n - 1) p,
//     lo = floor(h), hi = min(lo + 1, n - 1), g = h - lo, d = a[hi] - a[lo], Q = g < 0.5 ? a[lo] + d g : a[hi] - d (1 - g).
//   Calendar means: xbar_m = (the sequential sum of the included elements of calendar month m) / c_m, c_m their count.
//     R = sequential sum over m = 0 .. 11 of xbar_m;  C, S = sequential sums over m of xbar_m COS[m], xbar_m SIN[m], COS and SIN
//     the correctly rounded doubles of cos and sin of pi (2 m + 1) / 12 (the middle of month m on the circle of the year).
//   Annual totals: A_y = the sequential sum of the 12 months of year y, for the years whose 12 months are all included.
//   The table, XH_SIG_NCOL = 18 doubles:
//      0 n            1 n_zero = #{x == 0}     2 mean = S256(x) / n     3 std = sqrt(S256((x - mean)^2) / (n - 1)), NaN for n < 2
//      4 cv = std / mean     5 median = Q(0.5)
//      6 lag1 = S256 over pairs((x_t - mean)(x_{t+1} - mean)) / S256((x - mean)^2), NaN for n < 2
//      7 flashiness = S256 over pairs(|x_{t+1} - x_t|) / S256(x)      (Richards-Baker)
//      8 fdc_slope = (log Q(0.67) - log Q(0.34)) / 0.33, NaN when Q(0.34) is not > 0
//      9 regime_total = R     10 peak_month, 11 low_month = 1 + the first m of the largest, the smallest xbar_m
//     12 seasonality = (sequential sum over m of |xbar_m - R / 12.0|) / R      (Walsh & Lawler 1981)
//     13 centroid = atan2(S, C) XH_SIG_MONTHS_PER_RADIAN, plus 12.0 if negative: months from 1 January, 0.5 = mid-January
//     14 concentration = sqrt(C C + S S) / R      (Markham 1970)
//     15 n_years = the complete years     16 annual_mean = (sequential sum of A_y) / n_years
//     17 annual_cv = sqrt((sequential sum of (A_y - annual_mean)^2) / (n_years - 1)) / annual_mean, NaN for n_years < 2
//     Columns 9 - 14 are NaN when any c_m = 0.  With n = 0 only n, n_zero and n_years are numbers; the rest is NaN.
//   fdc[j] = Q(prob[j]), NaN for n = 0;  regime[m] = xbar_m, NaN where c_m = 0.
//
// HOW.  A `Team` does one row: lanes() workers, this one lane(), and sync() between a write to the team's memory and another
//   lane's read; sync_wave() is a sync() that holds only among the lanes 64 w .. 64 w + 63 of a 256-lane team, for the steps that
//   stay inside them.  The kernel's team is one 256-lane workgroup with its LDS; XhSigSerial below is one host thread, which walks the
//   256 partial sums of S256 one after another.  Every loop over lanes is written `for (l = lane(); l < L; l += lanes())`, so
//   that a team of any size forms the same numbers.
//   The row lies in buf[0 .. P), P the power of two >= 12 nyear, the elements left out and the padding as +inf (no included
//   element is +inf).  In the order of time it gives the S256 sums, the annual totals (lane <-> year) and the calendar means
//   (lane <-> month, then lane 0 their columns; one more lane, of another wavefront, walks the annual totals meanwhile); then a
//   bitonic sort in place puts the n included values first, ascending, and lane <-> probability reads the order statistics.
//   Lane 0 writes columns 0 .. 7, the first lane of the second wavefront the slope with its two logarithms.
//   Team memory: buf [P], sh [3 x 256], ann [nyear], misc [XH_SIG_MISC] doubles.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XH_SIG_HD __host__ __device__ __forceinline__
#else
#define XH_SIG_HD inline
#endif
#include <cmath>
#include <cstdint>

#define XH_SIG_NCOL 18
#define XH_SIG_MAX_P 16
#define XH_SIG_MAX_COLS 4096
#define XH_SIG_LANES 256
#define XH_SIG_MISC 32
// 6 / pi, correctly rounded
#define XH_SIG_MONTHS_PER_RADIAN 1.909859317102744

// misc: xbar_m [12], c_m [12], then Q(0.5), Q(0.67), Q(0.34)
#define XH_SIG_M_Q 24

XH_SIG_HD double xh_sig_nan() { return __builtin_nan(""); }
XH_SIG_HD double xh_sig_inf() { return __builtin_inf(); }
XH_SIG_HD bool xh_sig_finite(double v) { return v - v == 0.0; }

struct XhSigSerial {
    int lane() const { return 0; }
    int lanes() const { return 1; }
    void sync() const {}
    void sync_wave() const {}
};

// cos and sin of pi (2 m + 1) / 12, 50-digit values rounded once
XH_SIG_HD double xh_sig_cos(int m) {
    const double c[12] = {0.9659258262890683,  0.7071067811865476,  0.25881904510252074,  -0.25881904510252074,
                          -0.7071067811865476, -0.9659258262890683, -0.9659258262890683,  -0.7071067811865476,
                          -0.25881904510252074, 0.25881904510252074, 0.7071067811865476,  0.9659258262890683};
    return c[m];
}
XH_SIG_HD double xh_sig_sin(int m) {
    const double s[12] = {0.25881904510252074,  0.7071067811865476,  0.9659258262890683,  0.9659258262890683,
                          0.7071067811865476,   0.25881904510252074, -0.25881904510252074, -0.7071067811865476,
                          -0.9659258262890683,  -0.9659258262890683, -0.7071067811865476, -0.25881904510252074};
    return s[m];
}

// the power of two >= ncol, at least 4
XH_SIG_HD int xh_sig_pow2(int ncol) {
    int P = 4;
    while (P < ncol) P <<= 1;
    return P;
}

// buf[0 .. P) = the ncol elements at src as the walk wants them: x + 0.0, and +inf for what is left out and for the padding
template <class Team>
XH_SIG_HD void xh_sig_load(const Team &team, const double *src, int ncol, double *buf, int P) {
    for (int t = team.lane(); t < P; t += team.lanes()) {
        double v = xh_sig_inf();
        if (t < ncol) {
            const double x = src[t] + 0.0;
            if (xh_sig_finite(x)) v = x;
        }
        buf[t] = v;
    }
    team.sync();
}

// Three S256 sums at once: add(t, s) adds the terms of t to the partial sums s[0 .. 3), or nothing; out[0 .. 3) are the totals,
// the same in every lane.  sh: 3 x 256 doubles.  The tree is xh_block_sum256's (sh[l] += sh[l + stride], stride = 128 .. 1);
// from stride 32 on it reads and writes within the team's first 64 lanes, where sync_wave() is enough.
template <class Team, class Add>
XH_SIG_HD void xh_sig_sum256x3(const Team &team, double *sh, int count, Add add, double *out) {
    for (int l = team.lane(); l < XH_SIG_LANES; l += team.lanes()) {
        double s[3] = {0.0, 0.0, 0.0};
        for (int t = l; t < count; t += XH_SIG_LANES) add(t, s);
        for (int v = 0; v < 3; ++v) sh[v * XH_SIG_LANES + l] = s[v];
    }
    team.sync();
    for (int stride = XH_SIG_LANES / 2; stride > 0; stride >>= 1) {
        for (int l = team.lane(); l < stride; l += team.lanes())
            for (int v = 0; v < 3; ++v) sh[v * XH_SIG_LANES + l] += sh[v * XH_SIG_LANES + l + stride];
        if (stride > 64 || stride == 1) team.sync();
        else team.sync_wave();
    }
    for (int v = 0; v < 3; ++v) out[v] = sh[v * XH_SIG_LANES];
    team.sync();
}

// One step (k, j) of the bitonic sort of buf[0 .. P): this lane's share of the P / 2 compare-exchanges.  Pair q is the elements
// i (q with a 0 bit put in at j) and i + j: every element is touched by one lane only.
template <class Team>
XH_SIG_HD void xh_sig_sort_step(const Team &team, double *buf, int P, int k, int j) {
    for (int q = team.lane(); q < P / 2; q += team.lanes()) {
        const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), o = i | j;
        const double a = buf[i], b = buf[o];
        if ((i & k) == 0 ? (a > b) : (a < b)) buf[i] = b, buf[o] = a;
    }
}

XH_SIG_HD void xh_sig_cx(double &a, double &b, bool up) {
    if (up ? (a > b) : (a < b)) {
        const double t = a;
        a = b, b = t;
    }
}

// The steps that stay inside 4 consecutive elements, on those 4 in registers: the steps j = 2 and j = 1 of phase k >= 8, or
// (head) the whole phases k = 2 and k = 4.  P >= 4.  Group g = 32 (q / 64) + q mod 32 of the pairs' numbering q, on the lanes with
// q mod 64 < 32: the lanes that take the pairs of the elements 128 b .. 128 b + 127 in xh_sig_sort_step take their groups here.
template <class Team>
XH_SIG_HD void xh_sig_sort_four(const Team &team, double *buf, int P, int k, bool head) {
    for (int q = team.lane(); q < (P / 2 > 32 ? P / 2 : 32); q += team.lanes()) {
        const int g = ((q >> 6) << 5) | (q & 31);
        if ((q & 63) >= 32 || g >= P / 4) continue;
        double *e = buf + 4 * g;
        double e0 = e[0], e1 = e[1], e2 = e[2], e3 = e[3];
        if (head) xh_sig_cx(e0, e1, true), xh_sig_cx(e2, e3, false);
        const bool up = ((4 * g) & k) == 0;
        xh_sig_cx(e0, e2, up), xh_sig_cx(e1, e3, up);
        xh_sig_cx(e0, e1, up), xh_sig_cx(e2, e3, up);
        e[0] = e0, e[1] = e1, e[2] = e2, e[3] = e3;
    }
}

// bitonic sort of buf[0 .. P) ascending, P a power of two >= 4; no NaN in buf.  One pass over the row for the phases k = 2 and 4,
// then per phase k = 8 .. P one pass per step j = k / 2 .. 4 and one for the steps j = 2 and 1.  A pass with j <= 64 keeps the
// pairs q = 64 b .. 64 b + 63 inside the elements 128 b .. 128 b + 127 (i / 128 = q / 64), and the lanes 64 w .. 64 w + 63 of a
// 256-lane team take the same blocks b = w, w + 4, ... in every pass: between two such passes sync_wave() is enough.
template <class Team>
XH_SIG_HD void xh_sig_sort(const Team &team, double *buf, int P) {
    xh_sig_sort_four(team, buf, P, 4, true);
    if (P == 4) team.sync();                                          // (no pass follows; else j = 4 of phase 8)
    else team.sync_wave();
    for (int k = 8; k <= P; k <<= 1) {
        for (int j = k >> 1; j >= 4; j >>= 1) {
            xh_sig_sort_step(team, buf, P, k, j);
            if (j > 64) team.sync();                                  // (this pass crossed the blocks of 128)
            else team.sync_wave();
        }
        xh_sig_sort_four(team, buf, P, k, false);
        if (k > 64 || k == P) team.sync();                            // (the pass that follows is j = k of phase 2 k, or none)
        else team.sync_wave();
    }
}

// numpy's `linear` quantile p of sorted[0 .. n), n >= 1
XH_SIG_HD double xh_sig_quantile(const double *sorted, int n, double p) {
    const double h = (double)(n - 1) * p, fl = floor(h), g = h - fl;
    const int lo = (int)fl, hi = lo + 1 < n ? lo + 1 : n - 1;
    const double a = sorted[lo], b = sorted[hi], d = b - a;
    return g < 0.5 ? a + d * g : b - d * (1.0 - g);
}

// xbar_m and c_m of calendar month m from the row in the order of time.  (A partial sum that started at +0.0 never is -0.0,
// so adding 0.0 for an element left out leaves its bits: no branch in the chain.)
XH_SIG_HD void xh_sig_month(const double *buf, int ncol, int cal0, int m, double *mean, double *count) {
    double s = 0.0;
    int c = 0;
    for (int t = (m - cal0 + 12) % 12; t < ncol; t += 12) {
        const double v = buf[t];
        const bool keep = v != xh_sig_inf();
        s += keep ? v : 0.0;
        c += keep ? 1 : 0;
    }
    *count = (double)c;
    *mean = c > 0 ? s / (double)c : xh_sig_nan();
}

// columns 9 .. 14 of the table from xbar_m = misc[0 .. 12) and c_m = misc[12 .. 24)
XH_SIG_HD void xh_sig_regime_columns(const double *misc, double *table) {
    bool every = true;
    for (int m = 0; m < 12; ++m) every = every && misc[12 + m] > 0.0;
    for (int i = 9; i <= 14; ++i) table[i] = xh_sig_nan();
    if (!every) return;
    double R = 0.0, C = 0.0, S = 0.0, top = misc[0], bottom = misc[0];
    int peak = 0, low = 0;
    for (int m = 0; m < 12; ++m) {
        const double xm = misc[m];
        R += xm, C += xm * xh_sig_cos(m), S += xm * xh_sig_sin(m);
        if (xm > top) top = xm, peak = m;
        if (xm < bottom) bottom = xm, low = m;
    }
    const double even = R / 12.0;
    double dev = 0.0;
    for (int m = 0; m < 12; ++m) dev += fabs(misc[m] - even);
    double centroid = atan2(S, C) * XH_SIG_MONTHS_PER_RADIAN;
    if (centroid < 0.0) centroid += 12.0;
    table[9] = R, table[10] = (double)(1 + peak), table[11] = (double)(1 + low), table[12] = dev / R;
    table[13] = centroid, table[14] = sqrt(C * C + S * S) / R;
}

// columns 15 .. 17 of the table, n_years, annual_mean and annual_cv, from ann[0 .. nyear) (NaN: an incomplete year); a row
// without a complete year has 0 / 0 = NaN for its mean
XH_SIG_HD void xh_sig_annual_columns(const double *ann, int nyear, double *table) {
    double s = 0.0;
    int ny = 0;
    for (int y = 0; y < nyear; ++y) {
        const double a = ann[y];
        const bool keep = a == a;
        s += keep ? a : 0.0;
        ny += keep ? 1 : 0;
    }
    const double mean = s / (double)ny;
    double ss = 0.0;
    for (int y = 0; y < nyear; ++y) {
        const double a = ann[y];
        ss += a == a ? (a - mean) * (a - mean) : 0.0;
    }
    table[15] = (double)ny;
    table[16] = mean;
    table[17] = ny >= 2 ? sqrt(ss / (double)(ny - 1)) / mean : xh_sig_nan();
}

// One row.  src: the 12 nyear months of the window; prob: nP probabilities; buf, sh, ann, misc: the team's memory (see HOW);
// table: the row's 18 doubles; fdc: the row's nP doubles, or NULL; regime: the row's 12 doubles, or NULL.
template <class Team>
XH_SIG_HD void xh_signatures_row(const Team &team, const double *src, int nyear, int cal0, int nP, const double *prob, double *buf,
                                 double *sh, double *ann, double *misc, double *table, double *fdc, double *regime) {
    const double nan = xh_sig_nan(), inf = xh_sig_inf();
    const int ncol = 12 * nyear, P = xh_sig_pow2(ncol);
    xh_sig_load(team, src, ncol, buf, P);
    // in the order of time: the S256 sums, three at a time
    double first[3], second[3];
    xh_sig_sum256x3(team, sh, ncol, [=](int t, double *s) {
        const double v = buf[t];
        if (v != inf) s[0] += 1.0, s[2] += v;
        if (v == 0.0) s[1] += 1.0;
    }, first);
    const double cnt = first[0], n_zero = first[1], sx = first[2];
    const int n = (int)cnt;
    const double mean = sx / cnt;
    xh_sig_sum256x3(team, sh, ncol, [=](int t, double *s) {
        const double v = buf[t], w = buf[t + 1];                  // (12 nyear is no power of two: buf[12 nyear] is padding)
        if (v != inf) {
            s[0] += (v - mean) * (v - mean);
            if (t + 1 < ncol && w != inf) s[1] += (v - mean) * (w - mean), s[2] += fabs(w - v);
        }
    }, second);
    const double sxx = second[0], sprod = second[1], sabs = second[2];
    // the annual totals, lane <-> year
    for (int y = team.lane(); y < nyear; y += team.lanes()) {
        double a = 0.0;
        bool ok = true;
        for (int j = 0; j < 12; ++j) {
            const double v = buf[12 * y + j];
            ok = ok && v != inf;
            a += v;
        }
        ann[y] = ok ? a : nan;
    }
    team.sync();
    // the calendar means, lane <-> month, then their columns on lane 0, while the first lane of the second wavefront walks the
    // annual totals: the two long chains of one lane each run side by side
    for (int w = team.lane(); w <= 64; w += team.lanes()) {
        if (w < 12) {
            xh_sig_month(buf, ncol, cal0, w, &misc[w], &misc[12 + w]);
            if (regime) regime[w] = misc[w];
        } else if (w == 64) {
            xh_sig_annual_columns(ann, nyear, table);
        }
    }
    team.sync_wave();                           // (lanes 0 .. 11 -> lane 0)
    if (team.lane() == 0) xh_sig_regime_columns(misc, table);
    team.sync();
    // the order statistics
    xh_sig_sort(team, buf, P);
    for (int j = team.lane(); j < nP + 3; j += team.lanes()) {
        const double p = j < nP ? prob[j] : (j == nP ? 0.5 : (j == nP + 1 ? 0.67 : 0.34));
        const double q = n > 0 ? xh_sig_quantile(buf, n, p) : nan;
        if (j >= nP) misc[XH_SIG_M_Q + (j - nP)] = q;
        else if (fdc) fdc[j] = q;
    }
    team.sync();
    // columns 0 .. 7 on lane 0, the slope and its two logarithms on the first lane of the second wavefront
    for (int w = team.lane(); w <= 64; w += team.lanes()) {
        if (w == 0) {
            const double sd = n >= 2 ? sqrt(sxx / (double)(n - 1)) : nan;
            table[0] = cnt, table[1] = n_zero;
            table[2] = n > 0 ? mean : nan, table[3] = sd, table[4] = sd / mean, table[5] = misc[XH_SIG_M_Q];
            table[6] = n >= 2 ? sprod / sxx : nan;
            table[7] = n > 0 ? sabs / sx : nan;
        } else if (w == 64) {
            const double q67 = misc[XH_SIG_M_Q + 1], q34 = misc[XH_SIG_M_Q + 2];
            table[8] = q34 > 0.0 ? (log(q67) - log(q34)) / 0.33 : nan;
        }
    }
    team.sync();                                // (buf, ann and misc are rewritten by the team's next row)
}
