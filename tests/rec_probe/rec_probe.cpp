// Test-only host program: the filler of the routing kernels' month records (csrc/xh_mrtm_rec.h, wave_fill_records) as it
// is, built for the host alone with -fsanitize=address,undefined (Makefile).  Reads a schedule from the command line, fills the
// records into buffers of exactly the size the launch code allocates (the sanitizer sees any write beside them) and prints
// every record, the doubles as hexadecimal floats, for tests/test_month_records.py.
//     rec_probe <dt> <write from iteration> <days of iteration 0> <days of iteration 1> ...
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "xh_mrtm_rec.h"

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const double dt = atof(argv[1]);
    const int wr_from = atoi(argv[2]);
    const int nit = argc - 3;
    std::vector<int> m(nit), nt(nit), g(nit + 1);
    std::vector<unsigned char> wr(nit);
    std::vector<double> secs(nit);
    int total = 0;
    for (int it = 0; it < nit; ++it) {
        const int days = atoi(argv[3 + it]);
        m[it] = it >= wr_from ? it - wr_from : it;      // spin-up months, then the series from month 0
        secs[it] = days * 86400.0;
        nt[it] = (int)(days * 86400.0 / dt);
        g[it] = total;
        wr[it] = it >= wr_from;
        total += nt[it];
    }
    g[nit] = total;
    // heap buffers of the exact sizes (xh_mrtm_wave_launch.hip: nit + 3 and nit + 2 records), zeroed
    MonthRec *h = static_cast<MonthRec *>(calloc((size_t)nit + 3, sizeof(MonthRec)));
    FinRec *hf = static_cast<FinRec *>(calloc((size_t)nit + 2, sizeof(FinRec)));
    if (!h || !hf) return 3;
    wave_fill_records(nit, total, dt, m.data(), nt.data(), g.data(), wr.data(), secs.data(), [](int mm) { return (long long)mm * 8; }, h, hf);
    for (int it = 0; it < nit + 3; ++it)
        printf("rec %d m %d nt %d g %d write %d secs %a q_off %lld\n", it, h[it].m, h[it].nt, h[it].g, h[it].write, h[it].secs, h[it].q_off);
    for (int it = 0; it < nit + 2; ++it)
        printf("fin %d m_prev %d write_prev %d nt_prev %d m_next2 %d g_next1 %d secs_next1 %a q_off_next2 %lld erl_scale_next1 %a inv_nt_prev %a nt_cur %d\n",
               it, hf[it].m_prev_w & (FIN_WRITE - 1), (hf[it].m_prev_w & FIN_WRITE) != 0, hf[it].nt_prev, hf[it].m_next2, hf[it].g_next1,
               hf[it].secs_next1, hf[it].q_off_next2, hf[it].erl_scale_next1, hf[it].inv_nt_prev, hf[it].nt_cur);
    free(h);
    free(hf);
    return 0;
}
