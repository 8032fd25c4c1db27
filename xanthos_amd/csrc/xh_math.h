// exp() for the kernels that evaluate it in a loop (ABCD march, calibration march, Penman-Monteith).
//
// The device library's f64 exp is a 13-fma sequence, but the compiler issues its Horner steps as v_fmac_f64 (dst += a*b
// with the coefficient pre-loaded in dst), which destroys the coefficient register: every call re-materialises its ten
// 64-bit coefficients with 19 v_mov_b32 -- 45 % of the call's instructions, ~14 % of an ABCD month.  xh_exp is the SAME
// sequence (same constants, read off the library's code; same order of operations; same overflow / underflow selects),
// so its results are bit-identical to exp(), but the coefficients are passed in as values the compiler cannot see
// through (xh_exp_consts pins them in vector registers once per thread): the Horner steps become three-operand
// v_fma_f64 and nothing is re-materialised inside the loop.
//
// xh_exp, xh_exp_nonpos (and quot() of xh_abcd_dev.h) are plain fma / rint / ldexp arithmetic and callable on the host
// too, so that the algorithm can be tested on any machine (tests/math_probe); xh_sqrt, frcp and fdiv start from the
// hardware's v_rsq_f64 / v_rcp_f64 estimates and exist on the device only.
#pragma once
#include <hip/hip_runtime.h>

__host__ __device__ __forceinline__ double xh_from_bits(unsigned long long bits) { return __builtin_bit_cast(double, bits); }

struct XhExpConsts {
    double c[10];      // c2 .. c11 of the library's polynomial for exp(r) - 1 - r, |r| <= ln2 / 2
};

__host__ __device__ __forceinline__ XhExpConsts xh_exp_consts() {
    const unsigned long long bits[10] = {0x3fe000000000000bull, 0x3fc5555555555511ull, 0x3fa55555555502a1ull,
                                         0x3f81111111122322ull, 0x3f56c16c1852b7b0ull, 0x3f2a01a014761f6eull,
                                         0x3efa01997c89e6b0ull, 0x3ec71dee623fde64ull, 0x3e928af3fca7ab0cull,
                                         0x3e5ade156a5dcb37ull};
    XhExpConsts k;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        k.c[i] = xh_from_bits(bits[i]);
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(k.c[i]));      // opaque from here on: kept in registers, never rebuilt from literals
#endif                                        // (a vector-register constraint: the host compiler takes the plain values)
    }
    return k;
}

__host__ __device__ __forceinline__ double xh_exp(double x, const XhExpConsts &K) {
    const double log2e = xh_from_bits(0x3ff71547652b82feull);
    const double neg_ln2_hi = xh_from_bits(0xbfe62e42fefa39efull);
    const double neg_ln2_lo = xh_from_bits(0xbc7abc9e3b39803full);
    const double k = __builtin_rint(x * log2e);
    double r = __builtin_fma(neg_ln2_hi, k, x);
    r = __builtin_fma(neg_ln2_lo, k, r);
    double p = __builtin_fma(K.c[9], r, K.c[8]);
#pragma unroll
    for (int i = 7; i >= 0; --i) p = __builtin_fma(r, p, K.c[i]);
    p = __builtin_fma(r, p, 1.0);
    p = __builtin_fma(r, p, 1.0);
    double e = __builtin_ldexp(p, (int)k);
    e = (1024.0 < x) ? __builtin_inf() : e;       // as the library: guards the integer conversion, NaN falls through
    e = (-1075.0 > x) ? 0.0 : e;
    return e;
}

// exp(x) for x <= 0 where 1e-11 relative is enough (Penman-Monteith's pow(rh / 100, vpd / beta), :323: its result is one
// of three addends of a class's ET, and PET is held to 1e-9): the same reduction, the polynomial two terms shorter
// (degree 9: the dropped terms are < r^10 / 10! = 7e-12 for |r| <= ln2 / 2), no overflow select.
__host__ __device__ __forceinline__ double xh_exp_nonpos(double x, const XhExpConsts &K) {
    const double log2e = xh_from_bits(0x3ff71547652b82feull);
    const double neg_ln2_hi = xh_from_bits(0xbfe62e42fefa39efull);
    const double neg_ln2_lo = xh_from_bits(0xbc7abc9e3b39803full);
    const double k = __builtin_rint(x * log2e);
    double r = __builtin_fma(neg_ln2_hi, k, x);
    r = __builtin_fma(neg_ln2_lo, k, r);
    double p = __builtin_fma(K.c[7], r, K.c[6]);
#pragma unroll
    for (int i = 5; i >= 0; --i) p = __builtin_fma(r, p, K.c[i]);
    p = __builtin_fma(r, p, 1.0);
    p = __builtin_fma(r, p, 1.0);
    const double e = __builtin_ldexp(p, (int)k);
    return (-1075.0 > x) ? 0.0 : e;               // also x = -inf (rh = 0)
}

// sqrt for arguments that are zero or of ordinary magnitude (the ABCD month update's rpt^2 - w b / a; Penman-Monteith's
// temperature ratio).  The library's f64 sqrt is v_rsq_f64 + the Goldschmidt / Newton steps below, wrapped in a
// rescaling for arguments below 2^-767 and a class test (22 instructions); its argument here, rpt^2 - w b / a, is zero
// or of ordinary magnitude, so the same steps run bare (10 instructions + the zero / infinity select): identical
// results, correctly rounded, 9 instructions fewer on the march's dependent chain.  Negative -> NaN like sqrt.
// (Equal to IEEE sqrt in bits on [2^-700, 2^1023], tests/test_gpu_math.py::test_xh_sqrt_is_ieee.  The last correction, g3,
// changes the result only where the root lies within ~2^-43 of a step ABOVE a rounding boundary -- g2 errs low -- which
// random arguments never are; the test constructs such arguments, and without g3 it fails at them.)
__device__ __forceinline__ double xh_sqrt(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    const double g0 = x * y, h0 = 0.5 * y;
    const double r0 = __builtin_fma(-h0, g0, 0.5);
    const double g1 = __builtin_fma(g0, r0, g0), h1 = __builtin_fma(h0, r0, h0);
    const double d0 = __builtin_fma(-g1, g1, x);
    const double g2 = __builtin_fma(d0, h1, g1);
    const double d1 = __builtin_fma(-g2, g2, x);
    const double g3 = __builtin_fma(d1, h1, g2);
    return (x == 0.0 || x == __builtin_inf()) ? x : g3;
}

// a / b as a * (1 / b), the reciprocal from v_rcp_f64 refined by one Newton step (see frcp), for the magnitudes that occur in
// Penman-Monteith (xh_pm.hip; no scaling for operands near the exponent limits; b == 0 gives NaN, not an infinity -- every
// denominator there is guarded or strictly positive) in 6 instructions instead of the ~13 of the correctly rounded sequence.
// Accuracy, measured on MI355X against the exact quotient over |a|, |b| in [1e-6, 1e12], both signs
// (tests/test_gpu_math.py::test_frcp_fdiv_error, which asserts these bounds): frcp within 12 ulp of 1 / b (worst 11.11), fdiv
// within 19 ulp of a / b (worst 18.31), i.e. up to 2.5e-15 relative.  (v_rcp_f64 delivers ~24.5 bits and one step squares the
// error; until the measurement this comment said "a few ulp, ~1e-15 relative", which was too optimistic by a factor of 2 - 4.)
// The kernel is bound by its divisions (~145 per cell-month as written in the reference, ~50 after the regroupings described
// in xh_pm.hip): 4.9 ms -> 3.7 ms -> 3.1 ms per 67,420 x 600 launch.  Round 4: ONE Newton step (two until then): PET 8.6e-12
// against numpy on the bench world (7.9e-12 with two steps; exp / log dominate; tolerance 1e-6) and every PM test and fuzz
// case unchanged in outcome, for 3.2 % of the kernel's time (1.95 -> 1.89 ms).
__device__ __forceinline__ double frcp(double b) {
    double r = __builtin_amdgcn_rcp(b);
    r = __builtin_fma(r, __builtin_fma(-b, r, 1.0), r);
#ifdef XH_PM_RCP2      // the second step (round 1 - 3)
    r = __builtin_fma(r, __builtin_fma(-b, r, 1.0), r);
#endif
    return r;
}
__device__ __forceinline__ double fdiv(double a, double b) { return a * frcp(b); }
