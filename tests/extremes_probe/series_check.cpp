// Stand-alone check of the annual reduction, the counted sort and the four sums of csrc/xh_extremes_dev.h against std::sort and
// plain loops; built with AddressSanitizer + UndefinedBehaviorSanitizer (host code only) and started as a child process by
// tests/test_extremes_host.py.
//
//   usage: series_check [cases] [seed]
//
// Every case is one row of 12 nyear months (nyear 1 .. 8, 63, 64, 65, 128, 129, 341 first, then random up to 341) with ties (a
// few distinct values), +-0.0, NaN and +-inf months and whole missing years, held in a vector of exactly 12 nyear doubles, and
// the team's memory in vectors of exactly the sizes the kernel gives a wavefront (stage 768, z and zs nyear, sh 8): an index
// outside any of them is an ASan report.  Walked with teams of 1, 3 and 64 lanes (the lanes one after another between two
// syncs, which is what a team's memory must allow).  Checked, bit for bit:
//   the annual series against a loop over the 12 months;  n;  the sorted series against std::stable_sort of z;
//   l1 and l2 against the sums formed from that sorted series by plain loops in the definition's order.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "xh_extremes_dev.h"

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static bool same(double a, double b) { return (a != a && b != b) || same_bits(a, b); }

// a team of L lanes run one after another: xh_extremes_row is called once per lane with the team's memory kept between the
// calls, and the whole round is repeated: a row has five phases between its syncs (stage, z, sorted z, sums, outputs), each
// writing only what its own lane owns from what the phase before completed, so round p completes phase p for every lane and
// the sixth round repeats finished work.
struct Lanes {
    int me, count;
    int lane() const { return me; }
    int lanes() const { return count; }
    void sync() const {}
};

int main(int argc, char **argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 400;
    const unsigned seed = argc > 2 ? (unsigned)std::strtoul(argv[2], nullptr, 10) : 20262u;
    std::mt19937_64 rng(seed);
    const int fixed[14] = {1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 128, 129, 341};
    const int team_sizes[3] = {1, 3, 64};
    int failed = 0;
    for (int c = 0; c < cases; ++c) {
        const int nyear = c < 14 ? fixed[c] : 1 + (int)(rng() % 341);
        const int kind = c % 2;
        const int distinct = 1 + (int)(rng() % (c % 3 == 0 ? 4 : 1000));
        std::vector<double> x(12 * (size_t)nyear);
        for (double &v : x) {
            v = (double)(rng() % (uint64_t)distinct) * 0.37 - 20.0;
            if (c % 5 == 1 && rng() % 6 == 0) v = 0.0;
            if (c % 5 == 1 && rng() % 6 == 0) v = -0.0;
            if (c % 4 == 2 && rng() % 40 == 0) v = std::nan("");
            if (c % 8 == 3 && rng() % 60 == 0) v = (rng() & 1) ? INFINITY : -INFINITY;
        }
        if (c % 7 == 4)
            for (int j = 0; j < 12; ++j) x[12 * (rng() % (uint64_t)nyear) + j] = std::nan("");
        // the reference
        std::vector<double> a(nyear), z;
        for (int y = 0; y < nyear; ++y) {
            double m = x[12 * y];
            bool ok = std::isfinite(m);
            for (int j = 1; j < 12; ++j) {
                const double v = x[12 * y + j];
                ok = ok && std::isfinite(v);
                if (kind == XH_EXTREMES_MAX ? v > m : v < m) m = v;
            }
            a[y] = ok ? m : std::nan("");
            if (ok) z.push_back(kind == XH_EXTREMES_MIN ? -m : m);
        }
        std::stable_sort(z.begin(), z.end());
        const int n = (int)z.size();
        double b[2] = {0.0, 0.0};
        for (int i = 0; i < n; ++i) {
            b[0] += z[i];
            if (n > 1) b[1] += (((double)i) / (double)(n - 1)) * z[i];
        }
        const double l1 = n > 0 ? b[0] / n : std::nan(""), l2 = n > 1 ? 2.0 * (b[1] / n) - b[0] / n : std::nan("");
        const double T[3] = {2.0, 10.0, 100.0};
        for (int L : team_sizes) {
            std::vector<double> stage(XH_EX_STAGE, -777.0), zy(nyear, -777.0), zs(nyear, -777.0), sh(XH_EX_SH, -777.0);
            std::vector<double> table(XH_EXTREMES_NPAR + 3, -777.0), annual(nyear, -777.0), ty(nyear, -777.0);
            bool ok = true;
            if (L == 1) {
                const XhExSerial team;
                xh_extremes_row(team, x.data(), nyear, kind, 5, 3, T, nullptr, stage.data(), zy.data(), zs.data(), sh.data(),
                                table.data(), annual.data(), ty.data());
            } else if (nyear <= XH_EX_CHUNK_YEARS) {
                // (beyond one stage the chunks of a sequential team would overwrite each other: the phases are walked by hand)
                for (int round = 0; round < 6; ++round)
                    for (int me = 0; me < L; ++me) {
                        const Lanes team = {me, L};
                        xh_extremes_row(team, x.data(), nyear, kind, 5, 3, T, nullptr, stage.data(), zy.data(), zs.data(),
                                        sh.data(), table.data(), annual.data(), ty.data());
                    }
            } else {
                continue;
            }
            for (int y = 0; y < nyear; ++y) ok = ok && same(annual[y], a[y]);
            ok = ok && table[0] == (double)n;
            for (int i = 0; i < n; ++i) ok = ok && same_bits(zs[i], z[i]);
            ok = ok && same(kind == XH_EXTREMES_MIN ? -table[1] : table[1], l1) && same(table[2], l2);
            for (int y = 0; y < nyear; ++y) ok = ok && (ty[y] != ty[y] || ty[y] >= 1.0);
            if (!ok) {
                ++failed;
                std::printf("case %d (%d years, kind %d, %d distinct values, team of %d): FAILED\n", c, nyear, kind, distinct, L);
            }
        }
    }
    std::printf("series_check: %d cases, %d failed\n", cases, failed);
    return failed ? 1 : 0;
}
