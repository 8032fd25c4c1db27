// Stand-alone check of xh_si_rank (csrc/xh_sindex_dev.h), the rank-by-counting that k_std_index<log-logistic> sorts its
// reference samples with, against std::sort; built with AddressSanitizer + UndefinedBehaviorSanitizer (host code only) and
// started as a child process by tests/test_spei_host.py.
//
//   usage: rank_check [cases] [seed]
//
// Every case: a sample of n in [0, 341] values with many ties (a few distinct values, zeros, +-0.0, infinities) and sometimes
// NaNs, laid out as the kernel's LDS row is (stride 12 from an offset).  The ranks must be a permutation of 0 .. n - 1 -- the
// scatter then writes every slot exactly once and none outside --, the scattered row must equal std::sort of the sample
// (NaNs last) value for value, equal values must keep their order (the definition's tie rule), and the fit from it must be
// what the fit from the std::sort-ed sample is, bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "xh_sindex_dev.h"

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main(int argc, char **argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 2000;
    const unsigned seed = argc > 2 ? (unsigned)std::strtoul(argv[2], nullptr, 10) : 20251u;
    std::mt19937_64 rng(seed);
    int failed = 0;
    for (int c = 0; c < cases; ++c) {
        const int n = c < 8 ? c : (c % 5 == 0 ? 341 : (int)(rng() % 342));
        const int offset = (int)(rng() % 48), stride = 12;
        const int distinct = 1 + (int)(rng() % (c % 3 == 0 ? 4 : 1000));
        const bool with_nan = c % 7 == 3;
        // exactly the row the kernel reads: nothing before `offset`, nothing after the last element (ASan sees an overrun)
        std::vector<double> row(n > 0 ? offset + stride * (size_t)(n - 1) + 1 : 0, -777.0);
        std::vector<double> pool(distinct);
        for (double &v : pool) v = std::ldexp((double)((int64_t)(rng() % 2001) - 1000), -3);
        if (distinct > 2) pool[0] = 0.0, pool[1] = -0.0;
        if (distinct > 5 && c % 11 == 0) pool[2] = INFINITY, pool[3] = -INFINITY;
        for (int i = 0; i < n; ++i) {
            double v = pool[rng() % distinct];
            if (with_nan && rng() % 16 == 0) v = std::nan("");
            row[offset + stride * (size_t)i] = v;
        }
        auto sample = [&](int i) { return row[offset + stride * (size_t)i]; };
        std::vector<double> srt(n, -777.0);
        std::vector<int> hits(n, 0), rank(n, -1);
        bool ok = true;
        for (int j = 0; j < n; ++j) {
            const int r = xh_si_rank(sample, n, j);
            if (r < 0 || r >= n) {
                ok = false;
                continue;
            }
            rank[j] = r;
            ++hits[r];
            srt[r] = sample(j);
        }
        for (int r = 0; r < n; ++r) ok = ok && hits[r] == 1;
        // std::sort with the NaNs last
        std::vector<double> ref(n);
        for (int i = 0; i < n; ++i) ref[i] = sample(i);
        std::sort(ref.begin(), ref.end(), [](double a, double b) { return (a == a) && (!(b == b) || a < b); });
        for (int i = 0; i < n && ok; ++i) ok = (srt[i] != srt[i] && ref[i] != ref[i]) || srt[i] == ref[i];
        // equal values keep their order
        for (int j = 1; j < n && ok; ++j)
            for (int i = 0; i < j; ++i)
                if (sample(i) == sample(j) && rank[i] >= rank[j]) ok = false;
        if (ok) {
            // the sums do not see the order among equal values -- except that of +0.0 and -0.0, which std::sort may leave
            // either way: compare the fits where the two rows agree in sign bits too
            bool same_rows = true;
            for (int i = 0; i < n; ++i) same_rows = same_rows && (same_bits(srt[i], ref[i]) || (srt[i] != srt[i] && ref[i] != ref[i]));
            const XhSiLogLogistic a = xh_si_fit_loglogistic([&](int i) { return srt[i]; }, n, 1000.0);
            const XhSiLogLogistic b = xh_si_fit_loglogistic([&](int i) { return ref[i]; }, n, 1000.0);
            if (same_rows && !(same_bits(a.alpha, b.alpha) && same_bits(a.beta, b.beta) && same_bits(a.gamma, b.gamma) && same_bits(a.n, b.n))) ok = false;
            if ((with_nan && n > 0 && srt[n - 1] != srt[n - 1] && a.alpha == a.alpha) || (n < 4 && a.n == a.n)) ok = false;
        }
        if (!ok) {
            ++failed;
            std::printf("case %d (n = %d, %d distinct values%s): FAILED\n", c, n, distinct, with_nan ? ", NaNs" : "");
        }
    }
    std::printf("rank_check: %d cases, %d failed\n", cases, failed);
    return failed ? 1 : 0;
}
