// Flow control of the time-skewed dataflow routing kernels (check() of xh_mrtm_wave_unit.h): what a unit needs of its two
// stream counters for the next CH iterations, and whether it has to LOOK at a counter at all.  Plain functions of integers,
// no HIP types: the kernels include it, and so does a host program (tests/flowctl_probe).
//
// The protocol.  A producer stores sub-steps into a ring of `rs` entries per stream and publishes, at every check, how many
// are certainly in memory (`ready`, per stream).  A consumer publishes, at every check, how many it has consumed (`done`, per
// unit).  Both counters only grow.  At the check of iteration n (a multiple of CH) a unit makes sure that the next CH
// iterations can run without another look:
//   a consumer loads up to sub-step n + CH + GROUP - 1 - lag_g of an import (two blocks ahead), so it needs
//       ready >= min(total, n + CH + GROUP - lag_g);
//   a producer stores up to sub-step n + CH - 1 - RING - lmax, which overwrites sub-step (that) - rs, so it needs
//       done >= n + CH - lmax - rs   (nothing while that is <= 0; never more than total).
// The last value a unit read of a counter (`seen`) is a lower bound of the counter for ever after, so a unit whose `seen`
// already covers its need learns nothing from a fresh value that it has to know before the next check: it does not ask.
// A unit asks exactly when it has the stream kind and need > seen; what it reads may be short, and then it polls.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XH_FC_FN __host__ __device__ inline constexpr
#else
#define XH_FC_FN inline constexpr
#endif

// sub-steps of the consumer's progress (`done`) a producer needs before it runs iterations n .. n + ch - 1; 0: none
XH_FC_FN unsigned fc_need_done(int n, int ch, int lmax, int rs, int total) {
    const int need = n + ch - lmax - rs;
    return need <= 0 ? 0u : (unsigned)(need < total ? need : total);
}

// sub-steps of the producer's publication (`ready`) a consumer needs before it runs iterations n .. n + ch - 1; 0: none
XH_FC_FN unsigned fc_need_ready(int n, int ch, int group, int lag_g, int total) {
    const int need = n + ch + group - lag_g;
    const int m = need < total ? need : total;
    return m <= 0 ? 0u : (unsigned)m;
}

// whether a lane has to look at a counter: it has the stream kind, and what it last saw does not cover what it needs
XH_FC_FN bool fc_look(bool has_stream, unsigned need, unsigned seen) { return has_stream && need > seen; }
