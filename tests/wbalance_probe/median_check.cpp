// Stand-alone check of the padded sort and the median of csrc/xh_wbalance_dev.h (xh_wb_fill, xh_sig_sort, xh_wb_median) against
// std::sort; built with AddressSanitizer + UndefinedBehaviorSanitizer (host code only) and started as a child process by
// tests/test_wbalance_host.py.
//
//   usage: median_check [seed]
//
// For every count n = 0 .. 341 of qualifying years, three year counts nyear >= max(n, 1) (n itself, a random one, 341): the e_y in
// a vector of exactly nyear doubles, +inf (does not qualify) at nyear - n random places, with ties, +-0.0 and negative values,
// and the team's buffer in a vector of exactly the power of two the kernel gives it: an index outside either is an ASan
// report.  Walked with teams of 1, 3 and 256 lanes (the lanes one after another between two syncs).  Checked, as values (-0.0
// and +0.0 have no order among themselves):
//   the first n elements of the buffer against std::sort of the qualifying values, the rest +inf;
//   the median against the `linear` rule at 0.5 written out on the std::sort result, NaN for n = 0, and for an odd n the middle
//   value itself.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "xh_wbalance_dev.h"

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// lane `me` of `count`, run one after another by the caller
struct Lanes {
    int me, count;
    int lane() const { return me; }
    int lanes() const { return count; }
    void sync() const {}
    void sync_wave() const {}
};

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 10) : 20264u;
    std::mt19937_64 rng(seed);
    int cases = 0, failed = 0;
    for (int n = 0; n <= 341; ++n) {
        const int least = n > 1 ? n : 1;
        for (int nyear : {least, least + (int)(rng() % (uint64_t)(341 - least + 1)), 341}) {
            const int distinct = 1 + (int)(rng() % (cases % 3 == 0 ? 4 : 100000));
            std::vector<double> e((size_t)nyear, (double)INFINITY);
            std::vector<int> place((size_t)nyear);
            for (int y = 0; y < nyear; ++y) place[y] = y;
            std::shuffle(place.begin(), place.end(), rng);
            for (int i = 0; i < n; ++i) {
                double v = (double)(rng() % (uint64_t)distinct) * 0.37 - (cases % 2 ? 20.0 : 0.0);
                if (cases % 5 == 1 && rng() % 6 == 0) v = 0.0;
                if (cases % 5 == 1 && rng() % 6 == 0) v = -0.0;
                e[place[i]] = v;
            }
            std::vector<double> a;
            for (double v : e)
                if (v != (double)INFINITY) a.push_back(v);
            std::sort(a.begin(), a.end());
            const int P2 = xh_sig_pow2(nyear);
            const double *src = e.data();
            for (int L : {1, 3, 256}) {
                std::vector<double> es((size_t)P2, -777.0);
                if (L == 1) {
                    const XhSigSerial team;
                    xh_wb_fill(team, es.data(), nyear, P2, [=](int y) { return src[y]; });
                    xh_sig_sort(team, es.data(), P2);
                } else {
                    for (int me = 0; me < L; ++me) {
                        const Lanes team = {me, L};
                        xh_wb_fill(team, es.data(), nyear, P2, [=](int y) { return src[y]; });
                    }
                    for (int k = 2; k <= P2; k <<= 1)
                        for (int j = k >> 1; j > 0; j >>= 1)
                            for (int me = 0; me < L; ++me) {
                                const Lanes team = {me, L};
                                xh_sig_sort_step(team, es.data(), P2, k, j);
                            }
                }
                bool ok = true;
                for (int i = 0; i < P2; ++i) ok = ok && (i < n ? es[i] == a[i] : same_bits(es[i], (double)INFINITY));
                const double got = xh_wb_median(es.data(), n);
                if (n == 0) {
                    ok = ok && got != got;
                } else {
                    const double h = (double)(n - 1) * 0.5, fl = std::floor(h), g = h - fl;
                    const int lo = (int)fl, hi = std::min(lo + 1, n - 1);
                    const double d = a[hi] - a[lo];
                    const double want = g < 0.5 ? a[lo] + d * g : a[hi] - d * (1.0 - g);
                    ok = ok && (got == want) && got >= a[lo] && got <= a[hi];
                    if (n % 2 == 1) ok = ok && got == a[n / 2];
                }
                if (!ok) {
                    ++failed;
                    std::printf("count %d of %d years (%d distinct values, team of %d): FAILED\n", n, nyear, distinct, L);
                }
            }
            ++cases;
        }
    }
    std::printf("median_check: %d cases, %d failed\n", cases, failed);
    return failed ? 1 : 0;
}
