// The Mann-Kendall trend test (Mann 1945, Kendall 1975; seasonal form of Hirsch & Slack 1984) and the Theil-Sen slope with its
// rank-based confidence interval (Sen 1968) of one row (xh_trend.hip), callable on the host and on the device so
// that the same text runs in the kernel and in a probe on a machine without a GPU (tests/trend_probe).  It mirrors no
// function of the reference: xanthos has no trend statistic.
//
// DEFINITIONS (the contract; include/xanthos_hip.h restates them at xh_trend)
//   Input: one row x[0 .. ncol).  Column t belongs to season m = t mod nseason; its time is tau = (double)t / (double)nseason
//     years, one correctly rounded division.  A NaN element is left out of everything; +-inf is treated as NaN.
//   A pair is (i, j), i < j, of the same season, both elements finite; npairs their number, n the number of finite elements.
//   S = sum over the pairs of (x_j > x_i) - (x_j < x_i), by comparisons.
//   V = sum_m n_m (n_m - 1)(2 n_m + 5) - sum over the finite elements of (e - 1)(2 e + 5), n_m the finite count of season m,
//     e the number of finite elements of the element's season equal to it (==, itself included): integers, exact; the second
//     sum is the tie correction sum over tie groups of g (g - 1)(2 g + 5), without a sort.  var_s = (double)V / 18.0.
//   z = (S - 1) / sqrt(var_s) for S > 0, (S + 1) / sqrt(var_s) for S < 0, 0 for S = 0 or var_s = 0;
//   p = erfc(|z| 0.70710678118654752).
//   The slope of a pair is (x_j - x_i) / (double)((j - i) / nseason): one rounded subtraction, one correctly rounded division
//     by a whole number of years; -0.0 counts as +0.0.  s_(0) <= ... <= s_(N-1) the sorted slopes, N = npairs:
//     slope = s_((N-1)/2) for odd N, (s_(N/2-1) + s_(N/2)) / 2.0 for even N (numpy's median);
//     sigma = sqrt(var_s);  Ru = min((int)rint((N - z_conf sigma) / 2.0), N - 1);  Rl = max((int)rint((N + z_conf sigma) / 2.0)
//     - 1, 0), rint to even;  slope_lo = s_(Rl), slope_hi = s_(Ru);  z_conf, the caller's, is the normal quantile of
//     (1 - confidence) / 2, a negative number.  For nseason = 1 without NaN this is scipy.stats.theilslopes(x, arange(n)).
//   intercept = median(finite x) - slope median(tau of the finite elements), medians by numpy's rule.
//   Output, XH_TREND_NCOL = 10 doubles: n, s, var_s, z, p, slope, intercept, slope_lo, slope_hi, npairs.  With n < 4 or
//     npairs = 0 only n and npairs are filled, the other eight are NaN.
//
// HOW.  A `Team` does the work of one row: lanes() workers, this one lane(), with sync(), sum(v) (a whole-number sum over the
// lanes, exact in a double, returned to every lane) and add(p) (one more in a shared 32-bit counter; integer adds, so their
// order does not matter).  The kernel's team is a 256-lane workgroup with the row, the histograms and the selection state in
// LDS; XhTrSerial below is one host thread.
//   Counts: element t walks its season once: c finite elements, e equal ones, and over the later ones the pairs and
//     (x_u > x_t) - (x_u < x_t).  sum (c - 1)(2 c + 5) over the finite elements is sum_m n_m (n_m - 1)(2 n_m + 5).
//   Order statistics: the slopes are never stored.  xh_tr_select finds up to 4 ranks of a VIRTUAL array -- anything that gives
//     element k, NaN meaning "no element" -- by an MSB-first radix select on an order-preserving 64-bit key: 8 passes of 8 bits,
//     per pass and rank a 256-bin histogram of the elements whose higher digits equal the rank's prefix, then the bin that
//     holds the rank.  Pass 0 is one histogram for all ranks.  Every pass recomputes the elements.  Exact: ties and all.
//     Once every wanted rank is alone in its bin (untied data: well before the 8th pass) one more pass reads the keys of those
//     elements off, and the selection ends early; tied ranks take all 8 passes.  The result is the same bits.
//   XhTrSlopes lays the N' = nseason C(ny, 2) index pairs of ny = ncol / nseason years out as a rectangle, so that element k
//     costs no square root: k = (d - 1) ncol + t pairs column t with the column d years later AROUND THE CIRCLE of ny years,
//     u = t + d nseason (mod ncol), d = 1 .. (ny - 1) / 2; each unordered pair with circular distance d < ny / 2 occurs once.
//     For even ny the distance ny / 2 occurs once from the first half: ncol / 2 more elements, k continuing the same formula.
//     The division k / ncol is a multiplication by ceil(2^40 / ncol) (exact for k < 2^23, ncol <= 4096: k e < 2^40 with
//     e <= ncol the excess of the multiplier).  The pair's distance in years is |u - t| / nseason = d or ny - d.
//   The row and tau use the same selection: the median of x, and of {tau_t : x_t finite}.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XH_TR_HD __host__ __device__ __forceinline__
#else
#define XH_TR_HD inline
#endif
#include <cmath>
#include <cstdint>

#define XH_TREND_NCOL 10
#define XH_TR_MAX_COLS 4096
#define XH_TR_MAX_RANKS 4

XH_TR_HD double xh_tr_nan() { return __builtin_nan(""); }
XH_TR_HD bool xh_tr_finite(double v) { return v - v == 0.0; }

// order-preserving: a < b <=> key(a) < key(b) for non-NaN doubles (-0.0 sorts before +0.0)
XH_TR_HD uint64_t xh_tr_key(double v) {
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
XH_TR_HD double xh_tr_unkey(uint64_t k) {
    const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    __builtin_memcpy(&v, &b, 8);
    return v;
}

// the selection's shared state (LDS in the kernel): per rank the digits found so far and the rank among what shares them
struct XhTrSel {
    uint64_t prefix[XH_TR_MAX_RANKS];
    uint32_t rem[XH_TR_MAX_RANKS];
    uint32_t part[XH_TR_MAX_RANKS * 16];     // sums of 16 bins
    uint32_t cnt[XH_TR_MAX_RANKS];           // elements in the bin that holds the rank
    uint64_t full[XH_TR_MAX_RANKS];          // the whole key, once the rank is alone in its bin
};

struct XhTrSerial {
    int lane() const { return 0; }
    int lanes() const { return 1; }
    void sync() const {}
    double sum(double v) const { return v; }
    void add(uint32_t *p) const { ++*p; }
};

// out[r] = element rank[r] (0-based, ascending) of the non-NaN elements of arr(0 .. nvirt); every rank < their count.
// hist: NR x 256 counters; st: the state; every lane of the team calls it and gets the results.
template <int NR, class Team, class Arr>
XH_TR_HD void xh_tr_select(const Team &team, const Arr &arr, int nvirt, const uint32_t *rank, double *out, uint32_t *hist,
                           XhTrSel *st) {
    static_assert(NR >= 1 && NR <= XH_TR_MAX_RANKS, "ranks per selection");
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        const int nh = pass ? NR : 1;
        for (int b = team.lane(); b < nh * 256; b += team.lanes()) hist[b] = 0;
        team.sync();
        uint64_t prefix[NR];
        for (int r = 0; r < NR; ++r) prefix[r] = pass ? st->prefix[r] : 0;
        for (int k = team.lane(); k < nvirt; k += team.lanes()) {
            const double v = arr(k);
            if (!(v == v)) continue;
            const uint64_t key = xh_tr_key(v);
            const uint32_t digit = (uint32_t)(key >> shift) & 255u;
            if (pass == 0) {
                team.add(hist + digit);
            } else {
                const uint64_t hi = key >> (shift + 8);
                for (int r = 0; r < NR; ++r)
                    if (hi == prefix[r]) team.add(hist + 256 * r + digit);
            }
        }
        team.sync();
        // the bin that holds each rank, in two levels: 16 sums of 16 bins per histogram by 16 lanes, then one lane per rank
        // walks the 16 sums and the 16 bins of the one it lands in (loads that do not wait for the comparisons)
        for (int i = team.lane(); i < nh * 16; i += team.lanes()) {
            const uint32_t *h = hist + 16 * i;
            uint32_t sum = 0;
            for (int b = 0; b < 16; ++b) sum += h[b];
            st->part[i] = sum;
        }
        team.sync();
        for (int r = team.lane(); r < NR; r += team.lanes()) {
            const int h0 = pass ? r : 0;
            uint32_t rem = pass ? st->rem[r] : rank[r];
            uint32_t cum = 0, base = 0;
            int chunk = 0, bin = 0;
            for (int c = 0; c < 15; ++c) {
                cum += st->part[16 * h0 + c];
                if (cum <= rem) chunk = c + 1, base = cum;
            }
            rem -= base;
            const uint32_t *h = hist + 256 * h0 + 16 * chunk;
            cum = base = 0;
            for (int b = 0; b < 15; ++b) {
                cum += h[b];
                if (cum <= rem) bin = b + 1, base = cum;
            }
            st->prefix[r] = ((pass ? st->prefix[r] : 0) << 8) | (uint64_t)(16 * chunk + bin);
            st->rem[r] = rem - base;
            st->cnt[r] = h[bin];
        }
        team.sync();
        // every rank alone in its bin: the remaining digits are those of that one element, which one more pass reads off
        // instead of the 7 - pass passes that would count them out (the same bits either way)
        bool alone = pass < 6;
        for (int r = 0; r < NR; ++r) alone = alone && st->cnt[r] == 1u;
        if (alone) {
            for (int r = 0; r < NR; ++r) prefix[r] = st->prefix[r];
            for (int k = team.lane(); k < nvirt; k += team.lanes()) {
                const double v = arr(k);
                if (!(v == v)) continue;
                const uint64_t key = xh_tr_key(v);
                for (int r = 0; r < NR; ++r)
                    if ((key >> shift) == prefix[r]) st->full[r] = key;
            }
            team.sync();
            for (int r = 0; r < NR; ++r) out[r] = xh_tr_unkey(st->full[r]);
            return;
        }
    }
    for (int r = 0; r < NR; ++r) out[r] = xh_tr_unkey(st->prefix[r]);
}

// the row itself: NaN where not finite (the row in `xs` is sanitized already)
struct XhTrRow {
    const double *xs;
    XH_TR_HD double operator()(int k) const { return xs[k]; }
};

// tau of the finite elements
struct XhTrTau {
    const double *xs;
    double nseason;
    XH_TR_HD double operator()(int k) const { return xs[k] == xs[k] ? (double)k / nseason : xh_tr_nan(); }
};

// the pairwise slopes (see HOW above); NaN where an element of the pair is
struct XhTrSlopes {
    const double *xs;
    int ncol, nseason, ny;
    uint64_t magic;
    XH_TR_HD XhTrSlopes(const double *xs_, int ncol_, int nseason_)
        : xs(xs_), ncol(ncol_), nseason(nseason_), ny(ncol_ / nseason_), magic(((uint64_t)1 << 40) / (uint64_t)ncol_ + 1) {}
    XH_TR_HD int size() const { return nseason * (ny * (ny - 1) / 2); }
    XH_TR_HD double operator()(int k) const {
        const int d1 = (int)(((uint64_t)k * magic) >> 40);      // k / ncol
        const int t = k - d1 * ncol, d = d1 + 1;
        int u = t + d * nseason, years = d;
        if (u >= ncol) u -= ncol, years = ny - d;
        const double a = xs[t < u ? t : u], b = xs[t < u ? u : t];
        const double s = (b - a) / (double)years;                // NaN when either is
        return s == 0.0 ? 0.0 : s;                               // -0.0 counts as +0.0
    }
};

// One row.  src: the ncol used elements of the row; xs: ncol doubles of the team's (LDS); hist: 4 x 256 counters; st: the
// selection's state; out: the row's XH_TREND_NCOL doubles, written by lane 0.  ncol a positive multiple of nseason.
template <class Team>
XH_TR_HD void xh_trend_row(const Team &team, const double *src, int ncol, int nseason, double z_conf, double *xs,
                           uint32_t *hist, XhTrSel *st, double *out) {
    for (int t = team.lane(); t < ncol; t += team.lanes()) {
        const double v = src[t];
        xs[t] = xh_tr_finite(v) ? v : xh_tr_nan();
    }
    team.sync();
    // whole numbers below 2^53 (V < 3 ncol^3 = 2^38): exact as doubles, whatever the order of the lanes' sums
    int64_t cnt = 0, pairs = 0, s_sum = 0, v_sum = 0;
    for (int t = team.lane(); t < ncol; t += team.lanes()) {
        const double v = xs[t];
        if (!(v == v)) continue;
        int64_t c = 0, e = 0;
        for (int u = t % nseason; u < ncol; u += nseason) {
            const double w = xs[u];
            if (!(w == w)) continue;
            ++c;
            e += (w == v) ? 1 : 0;
            if (u > t) {
                ++pairs;
                s_sum += (int64_t)(w > v) - (int64_t)(w < v);
            }
        }
        ++cnt;
        v_sum += (c - 1) * (2 * c + 5) - (e - 1) * (2 * e + 5);
    }
    const double n = team.sum((double)cnt), npairs = team.sum((double)pairs);
    const double S = team.sum((double)s_sum), V = team.sum((double)v_sum);
    if (n < 4.0 || npairs == 0.0) {
        if (team.lane() == 0) {
            for (int i = 0; i < XH_TREND_NCOL; ++i) out[i] = xh_tr_nan();
            out[0] = n;
            out[9] = npairs;
        }
        return;
    }
    const double var_s = V / 18.0, sigma = sqrt(var_s);
    const uint32_t N = (uint32_t)npairs;
    int64_t ru = (int64_t)rint((npairs - z_conf * sigma) / 2.0), rl = (int64_t)rint((npairs + z_conf * sigma) / 2.0) - 1;
    if (ru > (int64_t)N - 1) ru = (int64_t)N - 1;
    if (rl < 0) rl = 0;
    const uint32_t ranks[4] = {(N - 1) / 2, N / 2, (uint32_t)rl, (uint32_t)ru};
    double sl[4], mx[2], mt[2];
    const XhTrSlopes slopes(xs, ncol, nseason);
    xh_tr_select<4>(team, slopes, slopes.size(), ranks, sl, hist, st);
    const uint32_t nn = (uint32_t)n;
    const uint32_t mid[2] = {(nn - 1) / 2, nn / 2};
    xh_tr_select<2>(team, XhTrRow{xs}, ncol, mid, mx, hist, st);
    xh_tr_select<2>(team, XhTrTau{xs, (double)nseason}, ncol, mid, mt, hist, st);
    if (team.lane() == 0) {
        double z = 0.0;
        if (var_s != 0.0 && S > 0.0) z = (S - 1.0) / sigma;
        if (var_s != 0.0 && S < 0.0) z = (S + 1.0) / sigma;
        const double slope = (N & 1u) ? sl[0] : (sl[0] + sl[1]) / 2.0;
        const double med_x = (nn & 1u) ? mx[0] : (mx[0] + mx[1]) / 2.0;
        const double med_t = (nn & 1u) ? mt[0] : (mt[0] + mt[1]) / 2.0;
        out[0] = n;
        out[1] = S;
        out[2] = var_s;
        out[3] = z;
        out[4] = erfc(fabs(z) * 0.70710678118654752);
        out[5] = slope;
        out[6] = med_x - slope * med_t;
        out[7] = sl[2];
        out[8] = sl[3];
        out[9] = npairs;
    }
}
