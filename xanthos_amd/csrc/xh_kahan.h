// pandas' compensated add (groupby.pyx group_sum / group_mean, pandas 2.x), the one definition of the device code:
//     NaN skipped;  y = v - c;  t = s + y;  c = (t - s) - y;  c reset to 0 when it is NaN (an infinite value went in);  s = t
// The reset keeps a lone +/-inf infinite; +inf and -inf together give NaN.  Used by xh_agg.hip (the writer's yearly
// sums and means), xh_diag.hip (groupby('id').sum()) and xh_hydro.hip (resample / groupby sums and means).
//
// The update depends on the absence of fp contraction and reassociation.  The Makefile builds with -ffp-contract=off;
// every file that includes this header also says `#pragma clang fp contract(off)`, so it stays so if a file is ever
// compiled on its own.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void kahan_add(double &s, double &comp, double v) {
#pragma clang fp contract(off)
    if (v != v) return;
    const double y = v - comp;
    const double t = s + y;
    comp = t - s - y;
    if (comp != comp) comp = 0.0;
    s = t;
}
