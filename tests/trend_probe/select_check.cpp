// Stand-alone check of the radix select of csrc/xh_trend_dev.h (xh_tr_select) and of the virtual slope array it runs on
// (XhTrSlopes) against std::sort; built with AddressSanitizer + UndefinedBehaviorSanitizer (host code only) and started as a
// child process by tests/test_trend_host.py.
//
//   usage: select_check [cases] [seed]
//
// Part 1, the selection: virtual arrays of N present elements (N = 1, 2, 255, 256, 257 first, then random up to 3000) among
// absent ones (NaN), with many ties (a few distinct values), +-0.0, infinities, denormals and values that differ in the last
// bit only; ranks 0, N - 1, the two middle ones and random ones, 1 to 4 per call.  Every selected value must be the element of
// that rank of std::sort, bit for bit (a key order puts -0.0 before +0.0, and so does the comparison used here).
// Part 2, the slopes: rows of nseason x ny columns (every ny from 1 to 12, then random; nseason 1 .. 12) with NaNs, held in a
// vector of exactly ncol doubles (an index outside the row is an ASan report): the multiset of the non-NaN elements of
// XhTrSlopes must be that of the slopes of all pairs (i, j), i < j, same season, both finite, formed by two loops.
// Part 3, whole rows through xh_trend_row with buffers of exactly the documented sizes: slope, slope_lo and slope_hi must be
// the order statistics of the sorted slopes of part 2 at the ranks of the definition.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "xh_trend_dev.h"

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static bool key_less(double a, double b) { return xh_tr_key(a) < xh_tr_key(b); }

static std::vector<double> pair_slopes(const std::vector<double> &x, int nseason) {
    std::vector<double> s;
    const int ncol = (int)x.size();
    for (int i = 0; i < ncol; ++i)
        for (int j = i + nseason; j < ncol; j += nseason) {
            if (!(xh_tr_finite(x[i]) && xh_tr_finite(x[j]))) continue;
            double v = (x[j] - x[i]) / (double)((j - i) / nseason);
            if (v == 0.0) v = 0.0;
            s.push_back(v);
        }
    std::sort(s.begin(), s.end(), key_less);
    return s;
}

int main(int argc, char **argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 600;
    const unsigned seed = argc > 2 ? (unsigned)std::strtoul(argv[2], nullptr, 10) : 20261u;
    std::mt19937_64 rng(seed);
    const XhTrSerial team;
    int failed = 0;
    const int fixed_n[5] = {1, 2, 255, 256, 257};

    for (int c = 0; c < cases; ++c) {
        const int N = c < 5 ? fixed_n[c] : 1 + (int)(rng() % 3000);
        const int distinct = 1 + (int)(rng() % (c % 3 == 0 ? 4 : 2000));
        std::vector<double> pool(distinct);
        for (double &v : pool) v = std::ldexp((double)((int64_t)(rng() % 200001) - 100000), (int)(rng() % 40) - 30);
        if (distinct > 2) pool[0] = 0.0, pool[1] = -0.0;
        if (distinct > 8 && c % 5 == 0) {
            pool[2] = INFINITY, pool[3] = -INFINITY, pool[4] = 4.9e-324, pool[5] = -4.9e-324;
            pool[6] = std::nextafter(pool[7], INFINITY);
        }
        std::vector<double> arr;                 // exactly nvirt doubles
        while ((int)arr.size() < N || rng() % 4 == 0) {
            if ((int)arr.size() - N > 500) break;
            arr.push_back(0.0);
        }
        const int nvirt = (int)arr.size();
        std::vector<int> slot(nvirt);
        for (int i = 0; i < nvirt; ++i) slot[i] = i;
        std::shuffle(slot.begin(), slot.end(), rng);
        std::vector<double> ref;
        for (int i = 0; i < nvirt; ++i) {
            if (i < N) {
                arr[slot[i]] = pool[rng() % distinct];
                ref.push_back(arr[slot[i]]);
            } else {
                arr[slot[i]] = std::nan("");
            }
        }
        std::sort(ref.begin(), ref.end(), key_less);
        uint32_t ranks[4] = {0, (uint32_t)N - 1, (uint32_t)(N - 1) / 2, (uint32_t)N / 2};
        if (c % 4 == 1)
            for (uint32_t &r : ranks) r = (uint32_t)(rng() % (uint64_t)N);
        std::vector<uint32_t> hist(XH_TR_MAX_RANKS * 256, 0xdeadbeefu);
        XhTrSel st;
        double out[4] = {-777.0, -777.0, -777.0, -777.0};
        const double *a = arr.data();
        auto elem = [a](int k) { return a[k]; };
        const int nr = 1 + c % 4;
        if (nr == 1) xh_tr_select<1>(team, elem, nvirt, ranks, out, hist.data(), &st);
        if (nr == 2) xh_tr_select<2>(team, elem, nvirt, ranks, out, hist.data(), &st);
        if (nr == 3) xh_tr_select<3>(team, elem, nvirt, ranks, out, hist.data(), &st);
        if (nr == 4) xh_tr_select<4>(team, elem, nvirt, ranks, out, hist.data(), &st);
        bool ok = true;
        for (int r = 0; r < nr; ++r) ok = ok && same_bits(out[r], ref[ranks[r]]);
        if (!ok) {
            ++failed;
            std::printf("select case %d (N = %d of %d, %d distinct values, %d ranks): FAILED\n", c, N, nvirt, distinct, nr);
        }
    }

    for (int c = 0; c < cases; ++c) {
        const int nseason = c < 144 ? 1 + c % 12 : 1 + (int)(rng() % 12);
        const int ny = c < 144 ? 1 + c / 12 : 1 + (int)(rng() % 40);
        const int ncol = nseason * ny;
        std::vector<double> x(ncol);
        const int distinct = 1 + (int)(rng() % (c % 3 == 0 ? 3 : 500));
        for (double &v : x) {
            v = (double)(rng() % (uint64_t)distinct) * 0.37 - 20.0;
            if (c % 2 == 1 && rng() % 8 == 0) v = std::nan("");
            if (c % 7 == 2 && rng() % 16 == 0) v = 0.0;
            if (c % 7 == 2 && rng() % 16 == 0) v = -0.0;
        }
        const std::vector<double> ref = pair_slopes(x, nseason);
        const XhTrSlopes slopes(x.data(), ncol, nseason);
        std::vector<double> got;
        for (int k = 0; k < slopes.size(); ++k) {
            const double v = slopes(k);
            if (v == v) got.push_back(v);
        }
        std::sort(got.begin(), got.end(), key_less);
        bool ok = slopes.size() == nseason * (ny * (ny - 1) / 2) && got.size() == ref.size();
        for (size_t i = 0; ok && i < ref.size(); ++i) ok = same_bits(got[i], ref[i]);
        // the whole row, with buffers of exactly the sizes the kernel gives it
        std::vector<double> xs(ncol), out(XH_TREND_NCOL, -777.0);
        std::vector<uint32_t> hist(XH_TR_MAX_RANKS * 256);
        XhTrSel st;
        const double z_conf = -1.959963984540054;
        xh_trend_row(team, x.data(), ncol, nseason, z_conf, xs.data(), hist.data(), &st, out.data());
        const int N = (int)ref.size();
        ok = ok && out[9] == (double)N;
        if (ok && out[0] >= 4.0 && N > 0) {
            const double sigma = std::sqrt(out[2]);
            const int ru = std::min((int)std::rint((N - z_conf * sigma) / 2.0), N - 1);
            const int rl = std::max((int)std::rint((N + z_conf * sigma) / 2.0) - 1, 0);
            const double med = (N & 1) ? ref[(N - 1) / 2] : (ref[N / 2 - 1] + ref[N / 2]) / 2.0;
            ok = same_bits(out[5], med) && same_bits(out[7], ref[rl]) && same_bits(out[8], ref[ru]);
        } else if (ok) {
            for (int i = 1; i < 9; ++i) ok = ok && out[i] != out[i];
        }
        if (!ok) {
            ++failed;
            std::printf("slope case %d (nseason = %d, %d years, %d distinct values): FAILED\n", c, nseason, ny, distinct);
        }
    }
    std::printf("select_check: %d cases of each kind, %d failed\n", cases, failed);
    return failed ? 1 : 0;
}
