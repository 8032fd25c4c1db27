// Stand-alone check of the count walk, the weights and the selection of csrc/xh_exboot_dev.h against std::sort of the explicit
// resample; built with AddressSanitizer + UndefinedBehaviorSanitizer (host code only) and started as a child process by
// tests/test_exboot_host.py.
//
//   usage: boot_check [cases] [seed]
//
// Every case is one row of 12 nyear months (nyear 1 .. 8, 63, 64, 65, 128, 129, 255, 256, 257, 341 first, then random up to
// 341; the count is 16 bits wide at every year count: there is no layout switch) with ties, +-0.0 and missing years, and a
// number of replicates B from 2, 3, 64, 65, 130, 768, 769, 1000, 2048 (both sides of n2 = 768, where the sort's buffer outgrows
// the stage).  All memory is held in vectors of exactly the sizes the kernel gives its workgroup (z, zs nyear, sh 8, tab 8, w
// 3 nyear, cnt lanes x nyear, nfit lanes, vals (1 + nT) B, and ONE vector of max(768, n2) doubles that is the stage and then the
// sort's buffer, as in the kernel): an index outside any of them is an ASan report.
//   team of 1: xh_exboot_row as it is.  Teams of 3 and 64 (the kernel's width): the pieces, the lanes one after another
//   between two syncs, every lane with its own column of counts at the team's stride.
// Checked, bit for bit: every replicate's l1, l2, t3, t4 against xh_ex_pwm on std::sort of the sample zs[j_i];  the counts
// against a histogram of the draws;  every stage-wise sort against std::sort;  nb and the bounds against the `linear`
// quantile formed from std::sort of the replicates' values.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "xh_exboot_dev.h"

static bool same(double a, double b) { return (a != a && b != b) || std::memcmp(&a, &b, sizeof a) == 0; }

struct Lanes {
    int me, count;
    int lane() const { return me; }
    int lanes() const { return count; }
    void sync() const {}
};

static double linear(std::vector<double> v, double p) {
    std::sort(v.begin(), v.end());
    const int nb = (int)v.size();
    const double h = (double)(nb - 1) * p, fl = std::floor(h), g = h - fl;
    const int lo = (int)fl, hi = std::min(lo + 1, nb - 1);
    const double d = v[hi] - v[lo];
    return g < 0.5 ? v[lo] + d * g : v[hi] - d * (1.0 - g);
}

int main(int argc, char **argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 60;
    const unsigned seed = argc > 2 ? (unsigned)std::strtoul(argv[2], nullptr, 10) : 20263u;
    std::mt19937_64 rng(seed);
    const int fixed[17] = {1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 128, 129, 255, 256, 257, 341};
    const int reps[9] = {2, 3, 64, 65, 130, 768, 769, 1000, 2048};
    const int team_sizes[3] = {1, 3, 64};
    const double T[3] = {2.0, 10.0, 100.0};
    const int nT = 3, nrep = XH_EXB_NREP + nT;
    const double p_lo = 0.05, p_hi = 1.0 - p_lo;
    int failed = 0, fitted = 0;
    for (int c = 0; c < cases; ++c) {
        const int nyear = c < 17 ? fixed[c] : 1 + (int)(rng() % 341);
        const int kind = c % 2, B = reps[c % 9], n2 = xh_exb_n2(B);
        const int distinct = 2 + (int)(rng() % (c % 3 == 0 ? 4 : 1000));
        const uint64_t bseed = rng();
        const int64_t row = (int64_t)(rng() % 100000);
        std::vector<double> x(12 * (size_t)nyear);
        for (double &v : x) {
            v = (double)(rng() % (uint64_t)distinct) * 0.37 - 20.0;
            if (c % 5 == 1 && rng() % 6 == 0) v = (rng() & 1) ? 0.0 : -0.0;
        }
        if (c % 7 == 4)
            for (int j = 0; j < 12; ++j) x[12 * (rng() % (uint64_t)nyear) + j] = std::nan("");
        for (int L : team_sizes) {
            std::vector<double> stage(n2 > XH_EX_STAGE ? n2 : XH_EX_STAGE, -777.0), z(nyear, -777.0), zs(nyear, -777.0), sh(XH_EX_SH, -777.0);
            std::vector<double> tab(XH_EXTREMES_NPAR, -777.0), w(3 * (size_t)nyear, -777.0);
            std::vector<double> &sortbuf = stage;           // the kernel's alias: the row is done with the stage
            std::vector<double> vals((size_t)(1 + nT) * B, -777.0), ci(3 + 2 * nT, -777.0), rep((size_t)B * nrep, -777.0);
            std::vector<uint16_t> cnt((size_t)L * nyear, 777);
            std::vector<int> nfit(L, -777);
            bool ok = true;
            if (L == 1) {
                xh_exboot_row(XhExSerial(), x.data(), nyear, kind, 5, nT, T, B, p_lo, p_hi, bseed, row, stage.data(), z.data(),
                              zs.data(), sh.data(), tab.data(), w.data(), cnt.data(), nfit.data(), sortbuf.data(), vals.data(),
                              ci.data(), rep.data());
            } else {
                // the row serially (series_check walks it with teams), then the pieces lane after lane
                xh_extremes_row(XhExSerial(), x.data(), nyear, kind, 5, 0, T, nullptr, stage.data(), z.data(), zs.data(), sh.data(),
                                tab.data(), nullptr, nullptr);
                if (tab[5] == tab[5]) {
                    const int n = (int)tab[0];
                    for (int me = 0; me < L; ++me)
                        for (int i = me; i < n; i += L)
                            for (int r = 1; r <= 3; ++r) w[(size_t)(r - 1) * n + i] = xh_exb_weight(i, n, r);
                    const uint64_t h_row = xh_exb_row_key(bseed, row);
                    for (int me = 0; me < L; ++me) {
                        int mine = 0;
                        for (int b = me; b < B; b += L) {
                            double lm[4], fit[3];
                            xh_exb_count(xh_exb_rep_key(h_row, b), n, cnt.data() + me, L);
                            std::vector<int> hist(n, 0);
                            const uint64_t h_rep = xh_exb_rep_key(h_row, b);
                            for (int i = 0; i < n; ++i) hist[xh_exb_index(xh_exb_word(h_rep, i >> 1), i, n)] += 1;
                            for (int j = 0; j < n; ++j) ok = ok && cnt[(size_t)j * L + me] == hist[j];
                            mine += xh_exb_fit(n, zs.data(), w.data(), cnt.data() + me, L, lm, fit) ? 1 : 0;
                            for (int q = 0; q < 4; ++q) rep[(size_t)b * nrep + q] = lm[q];
                            rep[(size_t)b * nrep + 4] = vals[b] = fit[0];
                            for (int t = 0; t < nT; ++t)
                                rep[(size_t)b * nrep + XH_EXB_NREP + t] = vals[(size_t)(1 + t) * B + b] = xh_ex_quantile(T[t], fit[0], fit[1], fit[2]);
                        }
                        nfit[me] = mine;
                    }
                    int nb = 0;
                    for (int l = 0; l < L; ++l) nb += nfit[l];
                    ci[0] = (double)nb;
                    for (int q = 0; q <= nT; ++q) {
                        std::vector<double> want(n2, INFINITY);
                        for (int i = 0; i < B; ++i) {
                            const double v = vals[(size_t)q * B + i];
                            sortbuf[i] = want[i] = v == v ? v : INFINITY;
                        }
                        for (int i = B; i < n2; ++i) sortbuf[i] = INFINITY;
                        for (int k = 2; k <= n2; k <<= 1)
                            for (int j = k >> 1; j > 0; j >>= 1)
                                for (int me = 0; me < L; ++me) xh_exb_sort_stage(Lanes{me, L}, sortbuf.data(), n2, k, j);
                        std::sort(want.begin(), want.end());
                        for (int i = 0; i < n2; ++i) ok = ok && (sortbuf[i] == want[i]);
                        const bool enough = 2 * nb >= B, flip = kind == XH_EXTREMES_MIN && q > 0;
                        const double lo = enough ? xh_exb_percentile(sortbuf.data(), nb, p_lo) : std::nan("");
                        const double hi = enough ? xh_exb_percentile(sortbuf.data(), nb, p_hi) : std::nan("");
                        ci[1 + 2 * q] = flip ? -hi : lo, ci[2 + 2 * q] = flip ? -lo : hi;
                    }
                } else {
                    ci[0] = 0.0;
                    for (int q = 1; q < 3 + 2 * nT; ++q) ci[q] = std::nan("");
                    for (double &v : rep) v = std::nan("");
                }
            }
            // the reference: the explicit resample, sorted
            const bool fit = tab[5] == tab[5];
            const int n = (int)tab[0];
            std::vector<std::vector<double>> got(1 + nT);
            for (int b = 0; b < B && fit; ++b) {
                const uint64_t h_rep = xh_exb_rep_key(xh_exb_row_key(bseed, row), b);
                std::vector<double> s(n);
                for (int i = 0; i < n; ++i) s[i] = zs[xh_exb_index(xh_exb_word(h_rep, i >> 1), i, n)];
                std::sort(s.begin(), s.end());
                const double b0 = xh_ex_pwm(s.data(), n, 0), b1 = xh_ex_pwm(s.data(), n, 1), b2 = xh_ex_pwm(s.data(), n, 2),
                             b3 = xh_ex_pwm(s.data(), n, 3);
                const double l2 = 2.0 * b1 - b0, l3 = (6.0 * b2 - 6.0 * b1) + b0, l4 = ((20.0 * b3 - 30.0 * b2) + 12.0 * b1) - b0;
                const double *r = rep.data() + (size_t)b * nrep;
                ok = ok && same(r[0], b0) && same(r[1], l2) && same(r[2], l3 / l2) && same(r[3], l4 / l2);
                const bool has = s[0] < s[n - 1] && l2 > 0.0 && l3 / l2 <= XH_EX_T3_MAX;
                ok = ok && (r[4] == r[4]) == has;
                for (int q = 0; q <= nT && has; ++q) got[q].push_back(r[4 + q]);
            }
            const int nb = (int)got[0].size();
            ok = ok && ci[0] == (double)nb;
            for (int q = 0; q <= nT; ++q) {
                const bool enough = fit && 2 * nb >= B, flip = kind == XH_EXTREMES_MIN && q > 0;
                const double lo = enough ? linear(got[q], p_lo) : std::nan(""), hi = enough ? linear(got[q], p_hi) : std::nan("");
                ok = ok && same(ci[1 + 2 * q], flip ? -hi : lo) && same(ci[2 + 2 * q], flip ? -lo : hi);
            }
            if (!fit)
                for (double v : rep) ok = ok && v != v;
            fitted += fit ? 1 : 0;
            if (!ok) {
                ++failed;
                std::printf("case %d (%d years, kind %d, B %d, team of %d): FAILED\n", c, nyear, kind, B, L);
            }
        }
    }
    std::printf("boot_check: %d cases, %d with a fit, %d failed\n", cases, fitted / 3, failed);
    return failed ? 1 : 0;
}
