// Water balance and Budyko signatures of one row of four monthly series (xh_wbalance.hip): where the row sits in
// Budyko space, how much of its precipitation runs off, whether the balance closes, how strongly runoff answers a change of
// precipitation or of PET, and after how many months it answers.  Callable on the host and on the device, so that the same text
// runs in the kernel and in a probe on a machine without a GPU (tests/wbalance_probe).  It mirrors no function of the
// reference: xanthos has no signatures of two variables.
//
// DEFINITIONS (the contract; include/xanthos_hip.h restates them at xh_water_balance).  No operation is contracted.
//   Input: the rows P, PET, Q and (or none) AET over the window [0 .. 12 nyear); year y is columns 12 y .. 12 y + 11.  Every
//   element enters as x + 0.0.  Month t is INCLUDED when every array given is finite at t; a year is COMPLETE when its 12 months
//   are included.
//   A^v_y, v in {P, PET, AET, Q}: the sequential sum (from 0.0, ascending) of the 12 months of a complete year.
//   Y256(f): lane l of 256 adds f(y) from 0.0 over the complete years y = l, l + 256, ... in ascending order; the 256 partial
//     sums are joined by the tree of xh_block_sum256 (csrc/xh_kge.h: sh[l] += sh[l + stride], stride = 128, 64, ..., 1).
//   S256(f): the same over the included months t.
//   n_years = the complete years; vbar = Y256(A^v) / n_years; dv_y = A^v_y - vbar.
//   The table, XH_WB_NCOL = 21 doubles:
//      0 n_years     1 n_months = the included months     2 p_mean = pbar   3 pet_mean = petbar   4 aet_mean = aetbar (NaN
//      without AET)   5 q_mean = qbar     6 runoff_ratio = qbar / pbar     7 aridity = phi = petbar / pbar
//      8 evaporative = aetbar / pbar     9 residual = (pbar - aetbar) - qbar     10 closure = residual / pbar
//     11 omega = Fu's parameter: the omega > 1 with fu(phi, omega) = eps, eps = (pbar - qbar) / pbar (below)
//     12 budyko_dev = eps - fu(phi, omega0)
//     13 elast_p = the median (numpy's `linear` rule at 0.5 on the values sorted ascending, xh_sig_quantile) of
//        e_y = (dQ_y / dP_y) (pbar / qbar) over the complete years with dP_y != 0; 14 elast_pet the same with dPET_y and petbar.
//        NaN when qbar is not > 0 or no year qualifies.      (Sankarasubramanian et al. 2001)
//     15 elast_p_ls = b1, 16 elast_pet_ls = b2: with x1 = dP_y / pbar, x2 = dPET_y / petbar, z = dQ_y / qbar and the Y256 sums
//        s11 = x1 x1, s12 = x1 x2, s22 = x2 x2, s1z = x1 z, s2z = x2 z:  det = s11 s22 - s12 s12,
//        b1 = (s1z s22 - s2z s12) / det, b2 = (s2z s11 - s1z s12) / det; NaN unless n_years >= 3 and det > 0.
//     17 r_pq = Y256(dP dQ) / sqrt(Y256(dP dP) Y256(dQ dQ)), NaN unless the product is > 0
//     18 dry_fraction = #{included t: P_t < PET_t} / n_months
//     19 lag_peak = the first k in 0 .. max_lag with the largest c_k, 20 r_peak = that c_k; NaN when no c_k is a number, with
//        mP = S256(P) / n_months, mQ = S256(Q) / n_months and
//        c_k = S256 over the t with t and t + k both included ((P_t - mP) (Q_{t+k} - mQ)) / sqrt(S256((P - mP)^2) S256((Q - mQ)^2))
//   xcorr[k] = c_k, k = 0 .. max_lag.   annual[v, y] = A^v_y, NaN for a year that is not complete, the AET plane NaN without AET.
//   Fu's curve: lo = min(1, phi), m = max(1, phi), r = lo / m, g(omega) = log1p(exp(omega log r)) / omega, and
//     fu(phi, omega) = lo - m expm1(g(omega)); NaN when phi is NaN.  omega solves m expm1(g(omega)) = lo - eps by exactly
//     XH_WB_BISECT = 60 bisection steps on s = log(omega - 1) over [log 2^-20, log 2^7], always all of them, and is
//     1 + exp(the last interval's midpoint); NaN unless 0 < eps < lo and the target lies strictly between the function's values
//     at the two ends.
//   With n_years = 0 every mean is 0 / 0: only columns 0, 1, 18, 19 and 20 may be numbers.  A ratio whose denominator is 0 follows
//   IEEE.  Every column but omega and budyko_dev is comparisons, + - x / and sqrt in this order: the same bits in every build.
//
// HOW.  The `Team` of xh_signatures_dev.h does one row: lanes(), lane(), sync(), sync_wave().  P and Q lie in bp, bq [12 nyear],
//   a month that is not included as NaN in both: one pass over the four rows loads them, decides the inclusion and forms the four
//   month sums of the first kind; PET and AET are used where they are loaded, there and in the annual totals (lane <-> year).
//   The S256 and Y256 sums go five at a time through sh; the e_y of both elasticities are padded with +inf to the power of
//   two P2 >= nyear and sorted by xh_sig_sort.  At the end lane 0 writes the table, the first lane of the second wavefront
//   runs the bisection -- or hands phi and eps on for later (`later`) --, that of the third forms the c_k.
//   Team memory: bp, bq [12 nyear], sh [5 x 256], ann [4 nyear], es [2 P2], misc [XH_WB_MISC] doubles (and the kernel's 2 x 256
//   for `later`).
#pragma once
#include "xh_signatures_dev.h"

#define XH_WB_NCOL 21
#define XH_WB_MAX_COLS 4096
#define XH_WB_MAX_LAG 12
#define XH_WB_LANES 256
#define XH_WB_NSUM 5
#define XH_WB_MISC 16
#define XH_WB_BISECT 60
// log 2^-20 and log 2^7, correctly rounded
#define XH_WB_S_LO -13.862943611198906
#define XH_WB_S_HI 4.852030263919617

// misc: the numerators of c_0 .. c_12, then S256((P - mP)^2), S256((Q - mQ)^2)
#define XH_WB_M_DEN 13

// xh_sig_sum256x3 for N <= XH_WB_NSUM sums at once: add(i, s) adds the terms of item i to the partial sums s[0 .. N), or nothing;
// out[0 .. N) are the totals, the same in every lane.  sh: N x 256 doubles.
template <int N, class Team, class Add>
XH_SIG_HD void xh_wb_sum256(const Team &team, double *sh, int count, Add add, double *out) {
    for (int l = team.lane(); l < XH_WB_LANES; l += team.lanes()) {
        double s[N];
        for (int v = 0; v < N; ++v) s[v] = 0.0;
        for (int i = l; i < count; i += XH_WB_LANES) add(i, s);
        for (int v = 0; v < N; ++v) sh[v * XH_WB_LANES + l] = s[v];
    }
    team.sync();
    for (int stride = XH_WB_LANES / 2; stride > 0; stride >>= 1) {
        for (int l = team.lane(); l < stride; l += team.lanes())
            for (int v = 0; v < N; ++v) sh[v * XH_WB_LANES + l] += sh[v * XH_WB_LANES + l + stride];
        if (stride > 64 || stride == 1) team.sync();
        else team.sync_wave();
    }
    for (int v = 0; v < N; ++v) out[v] = sh[v * XH_WB_LANES];
    team.sync();
}

// m expm1(g(omega)) of Fu's curve, lr = log r: what the curve lies below min(1, phi) by
XH_SIG_HD double xh_wb_excess(double m, double lr, double omega) { return m * expm1(log1p(exp(omega * lr)) / omega); }

// fu(phi, omega)
XH_SIG_HD double xh_wb_fu(double phi, double omega) {
    if (!(phi == phi)) return xh_sig_nan();
    const double lo = phi < 1.0 ? phi : 1.0, m = phi > 1.0 ? phi : 1.0;
    return lo - xh_wb_excess(m, log(lo / m), omega);
}

// Fu's parameter of (phi, eps): 60 bisection steps whatever the data
XH_SIG_HD double xh_wb_omega(double phi, double eps) {
    const double lo = phi < 1.0 ? phi : 1.0, m = phi > 1.0 ? phi : 1.0;
    const double lr = log(lo / m), target = lo - eps;
    double a = XH_WB_S_LO, b = XH_WB_S_HI;
    bool ok = phi == phi && eps > 0.0 && eps < lo;
    ok = ok && target < xh_wb_excess(m, lr, 1.0 + exp(a)) && target > xh_wb_excess(m, lr, 1.0 + exp(b));
    for (int i = 0; i < XH_WB_BISECT; ++i) {
        const double mid = 0.5 * (a + b);
        if (xh_wb_excess(m, lr, 1.0 + exp(mid)) > target) a = mid;      // (the excess falls as omega grows)
        else b = mid;
    }
    return ok ? 1.0 + exp(0.5 * (a + b)) : xh_sig_nan();
}

// columns 11 and 12 of the table, omega and budyko_dev, from phi and eps: pure functions of the two, so a team may put them off
// and form those of many rows side by side, one lane each (k_wbalance does)
XH_SIG_HD void xh_wb_budyko(double phi, double eps, double omega0, double *table) {
    table[11] = xh_wb_omega(phi, eps);
    table[12] = eps - xh_wb_fu(phi, omega0);
}

// es[0 .. P2) = e(y) for the years y < nyear (+inf from e: the year does not qualify) and +inf for the padding
template <class Team, class E>
XH_SIG_HD void xh_wb_fill(const Team &team, double *es, int nyear, int P2, E e) {
    for (int y = team.lane(); y < P2; y += team.lanes()) es[y] = y < nyear ? e(y) : xh_sig_inf();
}

// the median of the n qualifying values, which the sort has put first: numpy's `linear` rule at 0.5; NaN for none
XH_SIG_HD double xh_wb_median(const double *sorted, int n) { return n > 0 ? xh_sig_quantile(sorted, n, 0.5) : xh_sig_nan(); }

// One row.  p, pet, q, aet (or NULL): the 12 nyear months of the window; bp, bq, sh, ann, es, misc: the team's memory (see HOW);
// table: the row's 21 doubles; annual: the row's [4, nyear] doubles, or NULL; xcorr: the row's max_lag + 1 doubles, or NULL;
// later: NULL, or two doubles that receive phi and eps INSTEAD of columns 11 and 12 being written, for xh_wb_budyko afterwards.
template <class Team>
XH_SIG_HD void xh_wbalance_row(const Team &team, const double *p, const double *pet, const double *q, const double *aet, int nyear,
                               int max_lag, double omega0, double *bp, double *bq, double *sh, double *ann, double *es,
                               double *misc, double *table, double *annual, double *xcorr, double *later) {
    const double nan = xh_sig_nan(), inf = xh_sig_inf();
    const int ncol = 12 * nyear, P2 = xh_sig_pow2(nyear);
    // the four rows once: the inclusion, P and Q into the team's memory, and n_months, the dry months, S256(P), S256(Q)
    double mo[4];
    xh_wb_sum256<4>(team, sh, ncol, [=](int t, double *s) {
        const double a = p[t] + 0.0, b = pet[t] + 0.0, c = q[t] + 0.0, d = aet ? aet[t] + 0.0 : 0.0;
        const bool in = xh_sig_finite(a) && xh_sig_finite(b) && xh_sig_finite(c) && xh_sig_finite(d);
        bp[t] = in ? a : nan, bq[t] = in ? c : nan;
        if (in) {
            s[0] += 1.0, s[2] += a, s[3] += c;
            if (a < b) s[1] += 1.0;
        }
    }, mo);
    const double n_months = mo[0], mP = mo[2] / n_months, mQ = mo[3] / n_months;
    // the two sums of squares and the numerators of the c_k, five sums at a time
    for (int k0 = -2; k0 <= max_lag; k0 += XH_WB_NSUM) {
        double out[XH_WB_NSUM];
        xh_wb_sum256<XH_WB_NSUM>(team, sh, ncol, [=](int t, double *s) {
            const double v = bp[t];
            if (!(v == v)) return;
            for (int j = 0; j < XH_WB_NSUM; ++j) {
                const int k = k0 + j;
                if (k == -2) s[j] += (v - mP) * (v - mP);
                else if (k == -1) s[j] += (bq[t] - mQ) * (bq[t] - mQ);
                else if (k <= max_lag && t + k < ncol) {
                    const double w = bq[t + k];
                    if (w == w) s[j] += (v - mP) * (w - mQ);
                }
            }
        }, out);
        if (team.lane() == 0)
            for (int j = 0; j < XH_WB_NSUM; ++j) {
                const int k = k0 + j;
                if (k < 0) misc[XH_WB_M_DEN + 2 + k] = out[j];
                else if (k <= max_lag) misc[k] = out[j];
            }
    }
    // the annual totals, lane <-> year; PET and AET from where they lie
    for (int y = team.lane(); y < nyear; y += team.lanes()) {
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        bool ok = true;
        for (int j = 0; j < 12; ++j) {
            const int t = 12 * y + j;
            const double v = bp[t];
            ok = ok && v == v;
            a[0] += v, a[1] += pet[t] + 0.0, a[2] += aet ? aet[t] + 0.0 : 0.0, a[3] += bq[t];
        }
        for (int v = 0; v < 4; ++v) {
            const double tot = ok && (v != 2 || aet) ? a[v] : nan;
            ann[v * nyear + y] = tot;
            if (annual) annual[v * nyear + y] = tot;
        }
    }
    team.sync();
    // the means over the complete years
    double first[XH_WB_NSUM];
    xh_wb_sum256<XH_WB_NSUM>(team, sh, nyear, [=](int y, double *s) {
        if (!(ann[y] == ann[y])) return;
        s[0] += 1.0, s[1] += ann[y], s[2] += ann[nyear + y], s[4] += ann[3 * nyear + y];
        if (aet) s[3] += ann[2 * nyear + y];
    }, first);
    const double n_years = first[0], pbar = first[1] / n_years, petbar = first[2] / n_years, qbar = first[4] / n_years;
    const double aetbar = aet ? first[3] / n_years : nan;
    // the sums of the least squares, then those of the correlation and the qualifying years
    double ls[XH_WB_NSUM], co[XH_WB_NSUM];
    xh_wb_sum256<XH_WB_NSUM>(team, sh, nyear, [=](int y, double *s) {
        if (!(ann[y] == ann[y])) return;
        const double x1 = (ann[y] - pbar) / pbar, x2 = (ann[nyear + y] - petbar) / petbar, z = (ann[3 * nyear + y] - qbar) / qbar;
        s[0] += x1 * x1, s[1] += x1 * x2, s[2] += x2 * x2, s[3] += x1 * z, s[4] += x2 * z;
    }, ls);
    xh_wb_sum256<XH_WB_NSUM>(team, sh, nyear, [=](int y, double *s) {
        if (!(ann[y] == ann[y])) return;
        const double dP = ann[y] - pbar, dE = ann[nyear + y] - petbar, dQ = ann[3 * nyear + y] - qbar;
        s[0] += dP * dQ, s[1] += dP * dP, s[2] += dQ * dQ;
        if (dP != 0.0) s[3] += 1.0;
        if (dE != 0.0) s[4] += 1.0;
    }, co);
    // the e_y of both elasticities, padded with +inf, sorted
    xh_wb_fill(team, es, nyear, P2, [=](int y) {
        const double dP = ann[y] - pbar;
        return ann[y] == ann[y] && dP != 0.0 ? ((ann[3 * nyear + y] - qbar) / dP) * (pbar / qbar) : inf;
    });
    xh_wb_fill(team, es + P2, nyear, P2, [=](int y) {
        const double dE = ann[nyear + y] - petbar;
        return ann[y] == ann[y] && dE != 0.0 ? ((ann[3 * nyear + y] - qbar) / dE) * (petbar / qbar) : inf;
    });
    team.sync();
    xh_sig_sort(team, es, P2);
    xh_sig_sort(team, es + P2, P2);
    // lane 0 the table, the first lane of the second wavefront Fu's curve, that of the third the cross-correlation
    for (int w = team.lane(); w <= 128; w += team.lanes()) {
        if (w == 0) {
            const int ny = (int)n_years, nP = (int)co[3], nE = (int)co[4];
            const double residual = (pbar - aetbar) - qbar;
            const double det = ls[0] * ls[2] - ls[1] * ls[1], pp = co[1] * co[2];
            const bool fit = ny >= 3 && det > 0.0;
            table[0] = n_years, table[1] = n_months, table[2] = pbar, table[3] = petbar, table[4] = aetbar, table[5] = qbar;
            table[6] = qbar / pbar, table[7] = petbar / pbar, table[8] = aetbar / pbar, table[9] = residual;
            table[10] = residual / pbar;
            table[13] = qbar > 0.0 ? xh_wb_median(es, nP) : nan;
            table[14] = qbar > 0.0 ? xh_wb_median(es + P2, nE) : nan;
            table[15] = fit ? (ls[3] * ls[2] - ls[4] * ls[1]) / det : nan;
            table[16] = fit ? (ls[4] * ls[0] - ls[3] * ls[1]) / det : nan;
            table[17] = pp > 0.0 ? co[0] / sqrt(pp) : nan;
            table[18] = mo[1] / n_months;
        } else if (w == 64) {
            const double phi = petbar / pbar, eps = (pbar - qbar) / pbar;
            if (later) later[0] = phi, later[1] = eps;
            else xh_wb_budyko(phi, eps, omega0, table);
        } else if (w == 128) {
            const double den = sqrt(misc[XH_WB_M_DEN] * misc[XH_WB_M_DEN + 1]);
            double best = nan, at = nan;
            for (int k = 0; k <= max_lag; ++k) {
                const double c = misc[k] / den;
                if (xcorr) xcorr[k] = c;
                if (c == c && !(c <= best)) best = c, at = (double)k;
            }
            table[19] = at, table[20] = best;
        }
    }
    team.sync();                                // (bp, bq, ann, es and misc are rewritten by the team's next row)
}
