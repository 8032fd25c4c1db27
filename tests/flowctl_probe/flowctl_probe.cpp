// Test-only host program: the flow-control rule of the dataflow routing kernels (csrc/xh_mrtm_flowctl.h) as it is, built for
// the host alone with -fsanitize=address,undefined (Makefile); tests/test_flowctl_host.py builds and runs it.
//     flowctl_probe expr            the header's expressions against the ones check() spelled out until profiles/check_path
//     flowctl_probe chains <n> <seed>   n seeded chains of 2-5 units run by a model of check() that looks by the header's rule
// Prints one summary line and exits 0, or says what went wrong and exits 1.
//
// The model.  Unit u imports ONE stream from unit u - 1 and exports one to unit u + 1 (the ends have one side only).  A unit
// is at iteration n, a multiple of CH, in front of its check; a check is what the kernel does, in its order:
//     publish ready = clamp(n - RING - lmax)           (everything stored so far)
//     make sure done(consumer) >= fc_need_done(n)      -- look only if fc_look(), poll while the value is short
//     publish done = clamp(n - glmax)
//     make sure ready(producer) >= fc_need_ready(n)    -- look only if fc_look(), poll while the value is short
//     run CH iterations
// A counter keeps every value ever published; a look or a poll returns ANY of them between the one this unit read last and the
// newest (a load may be served stale; it never goes backwards for one reader), a poll the newest with probability 1/2.  Which
// unit moves next is drawn by the units' random integer service times.  Before a unit runs its CH iterations the model
// checks, against the NEWEST published values (what is really in memory), what the protocol is there for:
//     its loads reach sub-step n + CH + GROUP - 1 - lag: below the producer's newest `ready`;
//     its stores reach sub-step n + CH - 1 - RING - lmax, each overwriting the sub-step one ring before: below the consumer's
//     newest `done`.
// A chain must finish: when every unfinished unit polls in vain against the newest values the model reports a deadlock.
// Rings of 2-16 check intervals: so short that a producer and its consumer can block each other whatever they look at
// (no multiple of CH may lie in the open interval (rs - CH + lmax_p - glmax_c, CH + GROUP + RING + lmax_p - lag_c): with
// n_p - n_c there, the producer waits for ring space and the consumer for data); the model draws the ring again in that case,
// as the launch code sizes its rings well beyond it (8 CH + 4 lmax at the least).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "xh_mrtm_flowctl.h"

namespace {

constexpr int CH = 256, GROUP = 16, RING = 8;

int clampi(int v, int total) { return v < 0 ? 0 : (v > total ? total : v); }

int check_expressions() {
    long long cases = 0;
    const int lmaxs[] = {0, 2, 48}, rss[] = {512, 4096}, lags[] = {0, 16, 48};
    for (int total : {300, 511, 512, 5000, 8192, 175312})      // short (fewer than two check intervals) and long
        for (int n = 0; n <= 8192; n += 256)
            for (int lmax : lmaxs)
                for (int rs : rss)
                    for (int lag_g : lags) {
                        // check() until profiles/check_path, the ring: `need = n + CH - lmax - rs; if (need > 0) wait(min(need, total))`
                        const int need_d = n + CH - lmax - rs;
                        const unsigned old_done = need_d > 0 ? (unsigned)(need_d < total ? need_d : total) : 0u;
                        // the data: `need = min(total, n + CH + GROUP - lag_g); wait(has_g && need > 0, max(need, 0))`
                        const int need_r = (total < n + CH + GROUP - lag_g) ? total : n + CH + GROUP - lag_g;
                        const unsigned old_ready = need_r > 0 ? (unsigned)need_r : 0u;
                        const unsigned d = fc_need_done(n, CH, lmax, rs, total), r = fc_need_ready(n, CH, GROUP, lag_g, total);
                        if (d != old_done || r != old_ready) {
                            printf("expressions differ: n %d lmax %d rs %d lag %d total %d: done %u (was %u), ready %u (was %u)\n", n, lmax, rs,
                                   lag_g, total, d, old_done, r, old_ready);
                            return 1;
                        }
                        // a wait polled exactly when the lane had the stream, needed something and had seen less (wave_wait_ge)
                        for (unsigned seen : {0u, 1u, d ? d - 1u : 0u, d, d + 1u, r ? r - 1u : 0u, r, r + 1u, 0xffffffffu})
                            for (bool has : {false, true}) {
                                const bool old_d = has && need_d > 0 && !(seen >= old_done), old_r = has && need_r > 0 && !(seen >= old_ready);
                                if (fc_look(has, d, seen) != old_d || fc_look(has, r, seen) != old_r) {
                                    printf("look rule differs: n %d lmax %d rs %d lag %d total %d seen %u has %d\n", n, lmax, rs, lag_g, total, seen, (int)has);
                                    return 1;
                                }
                                ++cases;
                            }
                    }
    static_assert(fc_need_done(0, 256, 0, 2048, 1000) == 0u && fc_need_done(4096, 256, 48, 2048, 100000) == 2256u, "constexpr");
    static_assert(fc_need_ready(0, 256, 16, 48, 100) == 100u && !fc_look(false, 5u, 0u) && fc_look(true, 5u, 4u), "constexpr");
    printf("expr ok: %lld cases\n", cases);
    return 0;
}

struct Counter {
    std::vector<unsigned> hist;      // every value published, oldest first (non-decreasing)
    Counter() : hist(1, 0u) {}
    void publish(unsigned v) { hist.push_back(v); }
    unsigned newest() const { return hist.back(); }
};

struct Reader {      // one unit's view of one counter
    size_t idx = 0;          // index of the publication it read last
    unsigned seen = 0;       // the kernel's seen_done / seen_ready
    long long looks = 0, covered = 0, polls = 0;
};

struct Unit {
    int lmax = 0, glmax = 0, lag = 0, service = 1;
    int n = 0, N = 0, phase = 0;      // phase 0: in front of a check; 1: polling `done`; 2: polling `ready`; 3: finished
    bool has_x = false, has_g = false;
    Reader rd_done, rd_ready;
};

struct Chain {
    std::mt19937_64 rng;
    int total = 0;
    std::vector<Unit> u;
    std::vector<int> rs;               // ring of the stream u -> u + 1
    std::vector<Counter> ready, done;  // ready[u]: published by producer u; done[u]: published by consumer u
    const char *err = nullptr;

    unsigned read(const Counter &c, Reader &r, bool poll) {
        const size_t newest = c.hist.size() - 1;
        size_t i = r.idx + (size_t)(rng() % (newest - r.idx + 1));      // anything between what it read last and the newest
        if (poll && (rng() & 1)) i = newest;
        r.idx = i;
        const unsigned v = c.hist[i];
        r.seen = r.seen > v ? r.seen : v;
        return v;
    }

    // one move of unit k; returns whether anything changed
    bool move(int k) {
        Unit &a = u[k];
        if (a.phase == 3) return false;
        if (a.n >= a.N) {      // the end of the run: everything is published
            if (a.has_x) ready[k].publish((unsigned)total);
            if (a.has_g) done[k].publish((unsigned)total);
            a.phase = 3;
            return true;
        }
        const unsigned need_d = a.has_x ? fc_need_done(a.n, CH, a.lmax, rs[k], total) : 0u;
        const unsigned need_r = a.has_g ? fc_need_ready(a.n, CH, GROUP, a.lag, total) : 0u;
        if (a.phase == 0) {
            if (a.has_x) ready[k].publish((unsigned)clampi(a.n - RING - a.lmax, total));
            // both looks ride under the one wait at the start of the check
            if (a.has_x) {
                if (fc_look(true, need_d, a.rd_done.seen)) { ++a.rd_done.looks; read(done[k + 1], a.rd_done, false); }
                else ++a.rd_done.covered;
            }
            if (a.has_g) {
                if (fc_look(true, need_r, a.rd_ready.seen)) { ++a.rd_ready.looks; read(ready[k - 1], a.rd_ready, false); }
                else ++a.rd_ready.covered;
            }
            a.phase = 1;
        }
        if (a.phase == 1) {
            if (a.has_x && fc_look(true, need_d, a.rd_done.seen)) {
                ++a.rd_done.polls;
                read(done[k + 1], a.rd_done, true);
                if (fc_look(true, need_d, a.rd_done.seen)) return false;      // still short: it polls again when it moves next
            }
            if (a.has_g) done[k].publish((unsigned)clampi(a.n - a.glmax, total));
            a.phase = 2;
        }
        if (a.has_g && fc_look(true, need_r, a.rd_ready.seen)) {
            ++a.rd_ready.polls;
            read(ready[k - 1], a.rd_ready, true);
            if (fc_look(true, need_r, a.rd_ready.seen)) return true;          // (its `done` went out: that is a change)
        }
        // the next CH iterations (the last run ends at N), against what is really in memory
        const int n_end = a.n + CH < a.N ? a.n + CH : a.N;
        if (a.has_g) {
            const int top = clampi(n_end + GROUP - a.lag, total);             // one past the last sub-step it loads
            if ((unsigned)top > ready[k - 1].newest()) { err = "a consumer passed what its producer published"; return true; }
        }
        if (a.has_x) {
            const int top = clampi(n_end - RING - a.lmax, total);             // one past the last sub-step it stores
            if (top - rs[k] > (int)done[k + 1].newest()) { err = "a producer overwrote what its consumer had not marked done"; return true; }
        }
        a.n = n_end;
        a.phase = 0;
        return true;
    }

    bool blocked_for_good(int k) {      // polls in vain even against the newest values
        const Unit &a = u[k];
        if (a.phase == 1) return a.has_x && done[k + 1].newest() < fc_need_done(a.n, CH, a.lmax, rs[k], total);
        if (a.phase == 2) return a.has_g && ready[k - 1].newest() < fc_need_ready(a.n, CH, GROUP, a.lag, total);
        return false;
    }
};

bool pair_can_block(int rs, int lmax_p, int glmax_c, int lag_c) {
    const int lo = rs - CH + lmax_p - glmax_c, hi = CH + GROUP + RING + lmax_p - lag_c;      // open interval of n_p - n_c
    for (int d = -64 * CH; d <= 64 * CH; d += CH)
        if (d > lo && d < hi) return true;
    return false;
}

int run_chains(int n_chains, unsigned long long seed) {
    long long looks = 0, covered = 0, polls = 0, checks_total = 0, redrawn = 0;
    for (int c = 0; c < n_chains; ++c) {
        Chain ch;
        ch.rng.seed(seed * 1000003ull + (unsigned long long)c);
        auto rnd = [&](int lo, int hi) { return lo + (int)(ch.rng() % (unsigned long long)(hi - lo + 1)); };
        const int nu = rnd(2, 5);
        ch.total = (c % 7 == 0) ? rnd(1, 2 * CH - 1) : rnd(2 * CH, 40 * CH);      // also fewer sub-steps than two check intervals
        ch.u.resize(nu);
        ch.rs.assign(nu, 0);
        ch.ready.assign(nu, Counter());
        ch.done.assign(nu, Counter());
        for (int k = 0; k < nu; ++k) {
            Unit &a = ch.u[k];
            a.has_x = k + 1 < nu;
            a.has_g = k > 0;
            a.lmax = 2 * rnd(0, 24);
            a.glmax = a.has_g ? 2 * rnd(0, 24) : 0;
            a.lag = a.has_g ? rnd(0, a.glmax) : 0;
            a.service = rnd(1, 9);
            a.N = (ch.total + a.lmax + 1 + GROUP - 1) & ~(GROUP - 1);
        }
        for (int k = 0; k + 1 < nu; ++k) {
            ch.rs[k] = CH * rnd(2, 16);
            while (pair_can_block(ch.rs[k], ch.u[k].lmax, ch.u[k + 1].glmax, ch.u[k + 1].lag)) {
                ch.rs[k] += CH;
                ++redrawn;
            }
        }
        // a unit with a long service time moves rarely: time is drawn, not kept
        long long steps = 0;
        for (;;) {
            bool all_done = true, any_free = false;
            for (int k = 0; k < nu; ++k) {
                if (ch.u[k].phase != 3) all_done = false;
                if (ch.u[k].phase != 3 && !ch.blocked_for_good(k)) any_free = true;
            }
            if (all_done) break;
            if (!any_free) {
                printf("chain %d (seed %llu): deadlock: every unfinished unit polls in vain\n", c, seed);
                return 1;
            }
            int k = rnd(0, nu - 1);
            if (rnd(1, ch.u[k].service) != 1) continue;
            ch.move(k);
            if (ch.err) {
                printf("chain %d (seed %llu), unit %d at n = %d: %s\n", c, seed, k, ch.u[k].n, ch.err);
                return 1;
            }
            if (++steps > 50000000ll) {
                printf("chain %d (seed %llu): did not finish\n", c, seed);
                return 1;
            }
        }
        for (int k = 0; k < nu; ++k) {
            const Unit &a = ch.u[k];
            if (a.n != a.N) { printf("chain %d: unit %d ended at %d, not %d\n", c, k, a.n, a.N); return 1; }
            looks += a.rd_done.looks + a.rd_ready.looks;
            covered += a.rd_done.covered + a.rd_ready.covered;
            polls += a.rd_done.polls + a.rd_ready.polls;
            checks_total += (a.N + CH - 1) / CH;
        }
        for (int k = 0; k + 1 < nu; ++k)
            if (ch.ready[k].newest() != (unsigned)ch.total || ch.done[k + 1].newest() != (unsigned)ch.total) {
                printf("chain %d: stream %d ended at ready %u done %u, not %d\n", c, k, ch.ready[k].newest(), ch.done[k + 1].newest(), ch.total);
                return 1;
            }
    }
    if (looks == 0 || covered == 0 || polls == 0) {
        printf("vacuous: looks %lld covered %lld polls %lld\n", looks, covered, polls);
        return 1;
    }
    printf("chains ok: %d chains, %lld checks, counters looked at %lld times, covered by the known value %lld times, polls %lld, rings enlarged %lld times\n",
           n_chains, checks_total, looks, covered, polls, redrawn);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "expr")) return check_expressions();
    if (argc >= 4 && !strcmp(argv[1], "chains")) return run_chains(atoi(argv[2]), strtoull(argv[3], nullptr, 10));
    fprintf(stderr, "usage: flowctl_probe expr | chains <n> <seed>\n");
    return 2;
}
