// Bootstrap confidence intervals of the GEV shape and the return levels of one row (xh_exboot.hip): the annual
// series of xh_extremes_dev.h resampled with replacement B times, every replicate refitted by the same L-moment rules, and
// percentiles of the refitted values (the non-parametric percentile bootstrap; Efron & Tibshirani 1993, ch. 13).  Callable on
// the host and on the device, so that the same text runs in the kernel and in a probe on a machine without a GPU
// (tests/exboot_probe).  It mirrors no function of the reference: xanthos has no extreme-value statistics.
//
// DEFINITIONS (the contract; include/xanthos_hip.h restates them at xh_extremes_boot).  No operation is contracted.
//   1 The row.  The annual series, the counted sort zs[0 .. n), the L-moments and the fit are xh_extremes_row's (steps 1 - 3 of
//     xh_extremes_dev.h), by calling it.  A row without a fit gets nb = 0 and NaN everywhere else; no replicate is drawn.
//   2 Draws, all arithmetic mod 2^64; splitmix64 is the library's (x + 0x9E3779B97F4A7C15, two xor-shift-multiplies by
//     0xBF58476D1CE4E5B9 and 0x94D049BB133111EB, z ^ z >> 31):
//       h_row = splitmix64(seed ^ ((uint64)(row0 + r) * 0xD1342543DE82EF95));   h_rep = splitmix64(h_row ^ (uint64)(b + 1));
//       word(m) = splitmix64(h_rep ^ (uint64)(m + 1));
//     draw i of replicate b takes u32 = the low 32 bits of word(i >> 1) for even i, the high 32 bits for odd i, and
//       j_i = (u32 * (uint64)n) >> 32,  i = 0 .. n - 1,  an index into zs[0 .. n).
//     (u32 n >> 32 is not exactly uniform: a cell's probability is off by at most n / 2^32 of itself -- 8e-8 at 341 years.)
//     The draws depend on (seed, row0 + r, b, i) alone: not on B, the grid or how the rows are cut into calls.
//   3 A replicate's fit.  Its sample is the multiset {zs[j_i]} sorted ascending; b_0 .. b_3, l1 .. l4, t3, t4 are step 2 of
//     xh_extremes_dev.h on it (the same w_r(i), sums from 0.0 in rank order).  Equal values are interchangeable, so walking the
//     counts c_j = #{i : j_i = j} over ascending j gives the bits a sort would.  The same rules decide the fit (a sample that
//     is not constant, l2 > 0, t3 <= XH_EX_T3_MAX, k > -1 and finite) and the same functions form it (xh_ex_k_of_t3,
//     xh_ex_parameters, xh_ex_quantile).  nb = the number of replicates with a fit.
//   4 Intervals.  p_lo = (1 - confidence) / 2, p_hi = 1 - p_lo.  For k and for each return level the nb replicate values sorted
//     ascending, numpy's `linear` quantile: h = (nb - 1) p, lo = floor(h), hi = min(lo + 1, nb - 1), g = h - lo, d = a[hi] -
//     a[lo], g < 0.5 ? a[lo] + d g : a[hi] - d (1 - g).  Reported in the variable's own sign with lo <= hi: for min the level
//     bounds are -Q(p_hi) and -Q(p_lo); k's interval is that of z's k.  nb < ceil(B / 2): every bound NaN, nb still reported.
//   5 Output per row: ci [3 + 2 nT] = nb, k_lo, k_hi, x_T1_lo, x_T1_hi, ...; optionally rep [B, 5 + nT] = l1*, l2*, t3*, t4*, k*,
//     q*_T... of every replicate in z's sign (k* and the levels NaN for a replicate without a fit, the sums as computed; all
//     NaN for a row without a fit).
//
// HOW.  A `Team` as in xh_extremes_dev.h; lane <-> replicate.  Team memory: the row's (stage [XH_EX_STAGE], z, zs [nyear],
//   sh [XH_EX_SH]), tab [XH_EXTREMES_NPAR], w [3 nyear] (the weight rows w_1 .. w_3, formed once per row by the definition's
//   own expression: no division is left in a replicate), cnt [lanes nyear] 16-bit counts (a count can reach n <= 341; lane l's
//   count of j at cnt[j lanes + l]: consecutive lanes, consecutive addresses), nfit [lanes] ints, sortbuf [XH_EXB_N2(B)]
//   doubles, which may be the stage's memory (the row is done with it), and vals [(1 + nT) B] doubles, quantity-major, which
//   need not be fast memory (the kernel: a slab of its workgroup's in HBM).  A replicate's sums walk its counts in 2 n steps,
//   each either a term of the sums or a move to the next j: a trip count known beforehand whatever was drawn.  The order
//   statistics are exact: a bitonic sort of the quantity's values, a replicate without a fit as +inf after every number.
#pragma once
#include "xh_extremes_dev.h"

#define XH_EXB_MAX_B 2048
#define XH_EXB_MIN_B 2
#define XH_EXB_NREP 5

XH_EX_HD uint64_t xh_exb_splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

XH_EX_HD uint64_t xh_exb_row_key(uint64_t seed, int64_t row) {
    return xh_exb_splitmix64(seed ^ ((uint64_t)row * 0xD1342543DE82EF95ull));
}

XH_EX_HD uint64_t xh_exb_rep_key(uint64_t h_row, int b) { return xh_exb_splitmix64(h_row ^ (uint64_t)(b + 1)); }

XH_EX_HD uint64_t xh_exb_word(uint64_t h_rep, int m) { return xh_exb_splitmix64(h_rep ^ (uint64_t)(m + 1)); }

// j_i from the word of draw i
XH_EX_HD int xh_exb_index(uint64_t word, int i, int n) {
    const uint32_t u = (i & 1) ? (uint32_t)(word >> 32) : (uint32_t)word;
    return (int)(((uint64_t)u * (uint64_t)n) >> 32);
}

// the smallest power of two >= B
XH_EX_HD int xh_exb_n2(int B) {
    int n2 = 2;
    while (n2 < B) n2 <<= 1;
    return n2;
}

// w_r(i) of n values, r = 1 .. 3: xh_ex_pwm's expression
XH_EX_HD double xh_exb_weight(int i, int n, int r) {
    double w = 1.0;
    for (int j = 1; j <= r; ++j) w = (w * (double)(i - j + 1)) / (double)(n - j);
    return w;
}

// The counts of replicate h_rep over zs[0 .. n): cnt[j stride], j = 0 .. n - 1.
XH_EX_HD void xh_exb_count(uint64_t h_rep, int n, uint16_t *cnt, int stride) {
    for (int j = 0; j < n; ++j) cnt[j * stride] = 0;
    for (int m = 0; 2 * m < n; ++m) {
        const uint64_t word = xh_exb_word(h_rep, m);
        const int j0 = xh_exb_index(word, 2 * m, n);
        cnt[j0 * stride] = (uint16_t)(cnt[j0 * stride] + 1);
        if (2 * m + 1 < n) {
            const int j1 = xh_exb_index(word, 2 * m + 1, n);
            cnt[j1 * stride] = (uint16_t)(cnt[j1 * stride] + 1);
        }
    }
}

// One replicate from its counts (n >= 4 values; w = w_1, w_2, w_3 [n] each): lm = l1, l2, t3, t4 as computed, fit = k, alpha, xi
// (NaN without a fit).  Returns whether it has a fit.
XH_EX_HD bool xh_exb_fit(int n, const double *zs, const double *w, const uint16_t *cnt, int stride, double *lm, double *fit) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, first = 0.0, last = 0.0, zj = 0.0;
    int i = 0, j = -1, left = 0;
    for (int step = 0; step < 2 * n; ++step) {      // n terms and at most n moves
        if (left > 0) {
            if (i == 0) first = zj;
            last = zj;
            s0 += zj;
            s1 += w[i] * zj;
            s2 += w[n + i] * zj;
            s3 += w[2 * n + i] * zj;
            ++i, --left;
        } else if (j + 1 < n) {
            ++j;
            left = cnt[j * stride];
            zj = zs[j];
        }
    }
    const double b0 = s0 / (double)n, b1 = s1 / (double)n, b2 = s2 / (double)n, b3 = s3 / (double)n;
    const double l1 = b0, l2 = 2.0 * b1 - b0;
    const double l3 = (6.0 * b2 - 6.0 * b1) + b0, l4 = ((20.0 * b3 - 30.0 * b2) + 12.0 * b1) - b0;
    const double t3 = l3 / l2;
    lm[0] = l1, lm[1] = l2, lm[2] = t3, lm[3] = l4 / l2;
    fit[0] = fit[1] = fit[2] = xh_ex_nan();
    if (first < last && l2 > 0.0) {
        const double k = t3 <= XH_EX_T3_MAX ? xh_ex_k_of_t3(t3) : xh_ex_nan();
        if (k > -1.0 && xh_ex_finite(k)) {
            fit[0] = k;
            xh_ex_parameters(l1, l2, k, &fit[1], &fit[2]);
            return true;
        }
    }
    return false;
}

// One stage (k, j) of the bitonic sort of buf[0 .. n2), n2 a power of two, no NaN in it; a sync follows every stage.
template <class Team>
XH_EX_HD void xh_exb_sort_stage(const Team &team, double *buf, int n2, int k, int j) {
    for (int t = team.lane(); t < n2 / 2; t += team.lanes()) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const double a = buf[i], b = buf[p];
        const bool up = (i & k) == 0;
        if ((a > b) == up && a != b) buf[i] = b, buf[p] = a;
    }
}

template <class Team>
XH_EX_HD void xh_exb_sort(const Team &team, double *buf, int n2) {
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            xh_exb_sort_stage(team, buf, n2, k, j);
            team.sync();
        }
}

// numpy's `linear` quantile p of sorted[0 .. nb), nb >= 1
XH_EX_HD double xh_exb_percentile(const double *sorted, int nb, double p) {
    const double h = (double)(nb - 1) * p, fl = floor(h), g = h - fl;
    const int lo = (int)fl, hi = lo + 1 < nb ? lo + 1 : nb - 1;
    const double a = sorted[lo], b = sorted[hi], d = b - a;
    return g < 0.5 ? a + d * g : b - d * (1.0 - g);
}

// One row.  src, nyear, kind, min_years, nT, T: as xh_extremes_row; row = row0 + r; stage .. vals: the team's memory (see HOW);
// ci: the row's 3 + 2 nT doubles; rep: the row's B (5 + nT) doubles, or NULL.
template <class Team>
XH_EX_HD void xh_exboot_row(const Team &team, const double *src, int nyear, int kind, int min_years, int nT, const double *T, int B,
                            double p_lo, double p_hi, uint64_t seed, int64_t row, double *stage, double *z, double *zs, double *sh,
                            double *tab, double *w, uint16_t *cnt, int *nfit, double *sortbuf, double *vals, double *ci,
                            double *rep) {
    const double nan = xh_ex_nan();
    const bool neg = kind == XH_EXTREMES_MIN;
    const int L = team.lanes(), me = team.lane(), nrep = XH_EXB_NREP + nT;
    xh_extremes_row(team, src, nyear, kind, min_years, 0, T, nullptr, stage, z, zs, sh, tab, nullptr, nullptr);
    const int n = (int)tab[0];
    if (!(tab[5] == tab[5])) {                      // no fit: nothing is drawn
        for (int c = me; c < 3 + 2 * nT; c += L) ci[c] = c == 0 ? 0.0 : nan;
        if (rep)
            for (int c = me; c < B * nrep; c += L) rep[c] = nan;
        team.sync();                                // (tab is rewritten by the team's next row)
        return;
    }
    for (int i = me; i < n; i += L)
        for (int r = 1; r <= 3; ++r) w[(r - 1) * n + i] = xh_exb_weight(i, n, r);
    team.sync();
    const uint64_t h_row = xh_exb_row_key(seed, row);
    int mine = 0;
    for (int b0 = 0; b0 < B; b0 += L) {
        const int b = b0 + me;
        if (b < B) {
            double lm[4], fit[3];
            xh_exb_count(xh_exb_rep_key(h_row, b), n, cnt + me, L);
            mine += xh_exb_fit(n, zs, w, cnt + me, L, lm, fit) ? 1 : 0;
            vals[b] = fit[0];
            if (rep) {
                for (int c = 0; c < 4; ++c) rep[b * nrep + c] = lm[c];
                rep[b * nrep + 4] = fit[0];
            }
            for (int t = 0; t < nT; ++t) {
                const double q = xh_ex_quantile(T[t], fit[0], fit[1], fit[2]);
                vals[(1 + t) * B + b] = q;
                if (rep) rep[b * nrep + XH_EXB_NREP + t] = q;
            }
        }
    }
    nfit[me] = mine;
    team.sync();
    int nb = 0;
    for (int l = 0; l < L; ++l) nb += nfit[l];
    if (me == 0) ci[0] = (double)nb;
    const bool enough = 2 * nb >= B;                // nb >= ceil(B / 2)
    const int n2 = xh_exb_n2(B);
    for (int q = 0; q <= nT; ++q) {
        for (int i = me; i < n2; i += L) {
            const double v = i < B ? vals[q * B + i] : nan;
            sortbuf[i] = v == v ? v : xh_ex_inf();
        }
        team.sync();
        xh_exb_sort(team, sortbuf, n2);
        if (me == 0) {
            const double lo = enough ? xh_exb_percentile(sortbuf, nb, p_lo) : nan;
            const double hi = enough ? xh_exb_percentile(sortbuf, nb, p_hi) : nan;
            const bool flip = neg && q > 0;
            ci[1 + 2 * q] = flip ? -hi : lo;
            ci[2 + 2 * q] = flip ? -lo : hi;
        }
        team.sync();                                // (sortbuf is rewritten by the next quantity, nfit by the next row)
    }
}
