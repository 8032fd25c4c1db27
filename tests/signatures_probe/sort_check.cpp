// Stand-alone check of the load, the bitonic sort and the order statistics of csrc/xh_signatures_dev.h against std::sort; built
// with AddressSanitizer + UndefinedBehaviorSanitizer (host code only) and started as a child process by
// tests/test_signatures_host.py.
//
//   usage: sort_check [cases] [seed]
//
// Every case is one series of 1 .. 4096 elements (1 .. 17, 255 .. 257, 511 .. 513, 1023 .. 1025, 2047 .. 2049, 4095, 4096 first,
// then random) with ties (a few distinct values), +-0.0, NaN and +-inf elements, already ascending or descending now and then,
// held in a vector of exactly that length, and the team's buffer in a vector of exactly the power of two the kernel gives it:
// an index outside either is an ASan report.  Walked with teams of 1, 3 and 256 lanes (the lanes one after another between
// two syncs, which is what a team's memory must allow: every step of the sort touches each element from one lane only).
// Checked, bit for bit:
//   the first n elements of the buffer against std::sort of the included values (x + 0.0), the rest +inf;
//   the order statistics at 0.01 .. 0.99, 0.34, 0.5, 0.67 against the rule written out on the std::sort result, and within
//   [a[lo], a[hi]].
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "xh_signatures_dev.h"

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// lane `me` of `count`, run one after another by the caller
struct Lanes {
    int me, count;
    int lane() const { return me; }
    int lanes() const { return count; }
    void sync() const {}
    void sync_wave() const {}
};

// the sort with a team of L lanes taken one after another: one step (k, j) at a time, every lane's share of it
static void sort_by_lanes(double *buf, int P, int L) {
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1)
            for (int me = 0; me < L; ++me) {
                const Lanes team = {me, L};
                xh_sig_sort_step(team, buf, P, k, j);
            }
}

int main(int argc, char **argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 300;
    const unsigned seed = argc > 2 ? (unsigned)std::strtoul(argv[2], nullptr, 10) : 20263u;
    std::mt19937_64 rng(seed);
    std::vector<int> fixed;
    for (int n = 1; n <= 17; ++n) fixed.push_back(n);
    for (int c : {256, 512, 1024, 2048})
        for (int d = -1; d <= 1; ++d) fixed.push_back(c + d);
    fixed.push_back(4095), fixed.push_back(4096);
    std::vector<double> probs;
    for (int i = 1; i <= 99; ++i) probs.push_back((100.0 - i) / 100.0);
    probs.push_back(0.34), probs.push_back(0.5), probs.push_back(0.67);
    int failed = 0;
    for (int c = 0; c < cases; ++c) {
        const int len = c < (int)fixed.size() ? fixed[c] : 1 + (int)(rng() % 4096);
        const int distinct = 1 + (int)(rng() % (c % 3 == 0 ? 4 : 100000));
        std::vector<double> x((size_t)len);
        for (double &v : x) {
            v = (double)(rng() % (uint64_t)distinct) * 0.37 - (c % 2 ? 20.0 : 0.0);
            if (c % 5 == 1 && rng() % 6 == 0) v = 0.0;
            if (c % 5 == 1 && rng() % 6 == 0) v = -0.0;
            if (c % 4 == 2 && rng() % 20 == 0) v = std::nan("");
            if (c % 8 == 3 && rng() % 30 == 0) v = (rng() & 1) ? INFINITY : -INFINITY;
        }
        if (c % 11 == 5) std::sort(x.begin(), x.end(), [](double a, double b) { return a < b; });   // (no NaN in these cases)
        if (c % 11 == 7) std::sort(x.begin(), x.end(), [](double a, double b) { return a > b; });
        if (c % 13 == 6) std::fill(x.begin(), x.end(), std::nan(""));
        // the reference
        std::vector<double> a;
        for (double v : x)
            if (std::isfinite(v)) a.push_back(v + 0.0);
        std::sort(a.begin(), a.end());
        const int n = (int)a.size();
        const int P = xh_sig_pow2(len);
        for (int L : {1, 3, 256}) {
            std::vector<double> buf((size_t)P, -777.0);
            bool ok = true;
            if (L == 1) {
                const XhSigSerial team;
                xh_sig_load(team, x.data(), len, buf.data(), P);
                xh_sig_sort(team, buf.data(), P);
            } else {
                for (int me = 0; me < L; ++me) {
                    const Lanes team = {me, L};
                    xh_sig_load(team, x.data(), len, buf.data(), P);
                }
                sort_by_lanes(buf.data(), P, L);
            }
            for (int i = 0; i < P; ++i) ok = ok && same_bits(buf[i], i < n ? a[i] : (double)INFINITY);
            for (double p : probs) {
                if (n == 0) break;
                const double h = (double)(n - 1) * p, fl = std::floor(h), g = h - fl;
                const int lo = (int)fl, hi = std::min(lo + 1, n - 1);
                const double d = a[hi] - a[lo];
                const double want = g < 0.5 ? a[lo] + d * g : a[hi] - d * (1.0 - g);
                const double got = xh_sig_quantile(buf.data(), n, p);
                ok = ok && same_bits(got, want) && got >= a[lo] && got <= a[hi];
            }
            if (!ok) {
                ++failed;
                std::printf("case %d (%d elements, %d included, %d distinct values, team of %d): FAILED\n", c, len, n, distinct, L);
            }
        }
    }
    std::printf("sort_check: %d cases, %d failed\n", cases, failed);
    return failed ? 1 : 0;
}
