// Month records of the two time-skewed dataflow routing kernels (xh_mrtm_wave_unit.h reads them with scalar loads) and the
// host function that fills them (xh_mrtm_wave_launch.hip).  Plain C++, no HIP: tests/rec_probe builds the filler for the host
// alone, under the sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>

struct MonthRec {                             // one iteration of the schedule (spin-up months, then every month)
    int m, nt, g, write;                      // month index, sub-steps, first global sub-step, 1 = simulation pass
    double secs;
    long long q_off;                          // byte offset of month m inside a cell's row of the runoff source
};
static_assert(sizeof(MonthRec) == 32, "MonthRec is read with one s_load_dwordx8");

// What the month bookkeeping of iteration `it` needs -- the lanes' next crossing, the outputs of iteration it - 1, the lateral
// inflow of iteration it + 1, the fetch of iteration it + 2 -- gathered in one record that is loaded a whole month before it
// is used (round 3 profile: three dependent loads of month records, each waited for, cost every unit ~30 cycles per sub-step).
// Each kernel loads the fields it uses: the bit-exact one divides as the reference does (secs_next1, nt_prev), the
// reassociated one multiplies by what the host has divided once (erl_scale_next1, inv_nt_prev).
struct FinRec {
    int m_prev_w, nt_prev;                    // month index (bit 30: write flag) and sub-steps of iteration it - 1
    int m_next2;                              // month index of iteration it + 2 (its runoff is loaded now)
    int g_next1;                              // first global sub-step of iteration it + 1
    double secs_next1;                        // seconds of iteration it + 1
    long long q_off_next2;                    // byte offset of month m_next2 inside a cell's row of the runoff source
    double erl_scale_next1;                   // 1000 dt / secs_next1: mm of runoff x km2 -> m3 per sub-step (mrtm.py:45, times dt)
    double inv_nt_prev;                       // 1 / nt_prev (mrtm.py:80)
    int nt_cur;                               // sub-steps of iteration it: how far the lanes' next crossing lies behind this one
    int pad_[3];
};
constexpr int FIN_WRITE = 1 << 30;
static_assert(sizeof(FinRec) == 64, "FinRec is one 64-byte line");

// The schedule (nit iterations: month index m, sub-steps nt, first sub-step g [nit + 1 values, g[nit] = total], write flag,
// seconds) as records: h [nit + 3] (the last three zero: the month bookkeeping looks two ahead), hf [nit + 2].  Both arrays
// arrive zeroed.  q_off(m): where month m lies in a cell's row of the runoff source.
template <class QOff>
inline void wave_fill_records(int nit, int total, double dt, const int *m, const int *nt, const int *g, const unsigned char *wr,
                              const double *secs, QOff q_off, MonthRec *h, FinRec *hf) {
    for (int it = 0; it < nit; ++it) {
        h[it].m = m[it];
        h[it].nt = nt[it];
        h[it].g = g[it];
        h[it].write = wr[it];
        h[it].secs = secs[it];
        h[it].q_off = q_off(m[it]);
    }
    h[nit].g = total;
    for (int it = 0; it <= nit; ++it) {
        if (it >= 1) {
            hf[it].m_prev_w = h[it - 1].m | (h[it - 1].write ? FIN_WRITE : 0);
            hf[it].nt_prev = h[it - 1].nt;
        }
        hf[it].nt_prev = std::max(hf[it].nt_prev, 1);
        hf[it].secs_next1 = it + 1 < nit ? h[it + 1].secs : 1.0;
        hf[it].m_next2 = it + 2 < nit ? h[it + 2].m : 0;
        hf[it].q_off_next2 = q_off(hf[it].m_next2);
        hf[it].g_next1 = it + 1 <= nit ? h[it + 1].g : total;
        hf[it].erl_scale_next1 = 1000.0 * dt / hf[it].secs_next1;
        hf[it].inv_nt_prev = 1.0 / (double)hf[it].nt_prev;
        hf[it].nt_cur = it < nit ? h[it].nt : 0;
    }
    hf[nit + 1].nt_prev = 1;
    hf[nit + 1].secs_next1 = 1.0;
    hf[nit + 1].erl_scale_next1 = 1000.0 * dt;
    hf[nit + 1].inv_nt_prev = 1.0;
}
