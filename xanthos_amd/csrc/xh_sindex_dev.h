// Scalar mathematics of the standardized drought indices (SRI / SSI / SSFI; xh_sindex.hip), callable on the host
// and on the device so that every function can be tested on a machine without a GPU (tests/sindex_probe).  It mirrors no
// function of the reference: xanthos has no standardized index.
//
// DEFINITIONS (the contract; include/xanthos_hip.h restates them at xh_std_index)
//   Sample of one (cell, calendar month, scale): s[0 .. n), the accumulated values X[c, u] of the reference period's months
//   u with u mod 12 = m and u >= k - 1, in ascending u.
//   gamma fit (Thom's closed-form approximation of the maximum-likelihood estimate, as NCAR climate_indices):
//     any s NaN or negative -> NaN row;  n0 = #{s == 0}, q0 = n0 / n;  P = the positive s, np = |P|, np < 4 -> NaN row;
//     mu = (sum of P from 0.0, ascending) / np;  ml = (sum of log(P) from 0.0, ascending) / np;  A = log(mu) - ml, not A > 0 ->
//     NaN row;  alpha = (1 + sqrt(1 + 4 A / 3)) / (4 A), alpha > max_shape -> NaN row;  beta = mu / alpha.
//     The row is (q0, alpha, beta, n); a NaN row is four NaNs.
//   gamma evaluation: X NaN or negative, or a NaN row -> NaN;  X == 0 -> H = q0;  else H = q0 + (1 - q0) P(alpha, X / beta);
//     index = min(max(ndtri(H), -3.09), 3.09).
//   empirical (Gringorten): X NaN, any s NaN or n < 4 -> NaN;  in = 1 when X's own month lies in the reference period;
//     L = #{s < X}, E = #{s == X}, N = n + 1 - in, rank = L + (E + 2 - in) / 2, p = (rank - 0.44) / (N + 0.12);
//     index = clip(ndtri(p), +-3.09).
//
// P(a, x), the regularized lower incomplete gamma function: the series  P = F sum_{j >= 0} x^j / (a (a + 1) ... (a + j))  for
// x < a + 1 and  P = 1 - F cf  with the modified Lentz evaluation of Legendre's continued fraction otherwise, F = x^a e^-x /
// Gamma(a).  F is where a plain a log x - x - lgamma(a) would lose digits (three terms of size ~ a log a, eps each): for
// a >= 12  F = sqrt(a / 2 pi) exp(a (log1p(u) - u) - c(a)),  u = (x - a) / a,  c = the Stirling correction, whose exponent is
// of the size of log F itself; for a < 12 the terms are small, and lgamma(a) comes from the same Stirling form at a + N >= 12
// through Gamma(a) = Gamma(a + N) / (a (a + 1) ... (a + N - 1)).
// LOOP BOUND.  Both loops stop after XH_SI_MAXIT = 512 iterations; a call that has not converged there returns NaN (it never
// spins).  Series: for x < a + 1 term j over term 0 is prod_{i <= j} x / (a + i) <= exp(-j (j - 1) / (2 (a + j))), below
// 2^-53 once j (j - 1) >= 73.5 (a + j), i.e. j >= 37.3 + sqrt(37.3^2 + 73.5 a): 312 for a = 1000 (max_shape's default and
// the design limit).  Continued fraction: for x >= a + 1 its convergents approach like the same Gaussian of width sqrt(a);
// the worst count met over a in [0.01, 1000], x / a in [1e-3, 10] and x next to a + 1 is held to the bound by
// tests/test_sindex_host.py (see DESIGN 4.18 for the counts measured).  A shape above 1000 can only come from a caller's
// max_shape or parameter table; such entries may run into the bound and are NaN then.
//
// ndtri, the inverse of the standard normal distribution function: Wichura's algorithm AS 241, routine PPND16 (Applied
// Statistics 37, 1988): |p - 1/2| <= 0.425 a rational function of 0.180625 - (p - 1/2)^2 (central region); otherwise of
// r = sqrt(-log(min(p, 1 - p))) - 1.6 for r <= 5 and of r - 5 beyond (the two tail regions).  About 1e-16 relative.
//
// SPI / SPEI AND THE LOG-LOGISTIC DISTRIBUTION.  The definitions above hold unchanged (X at scale k, the sample
// R(c, m) in ascending u, n = |R|, the clip).
//   Input with a subtrahend: with a second array y the input element is x[c, t] - y[c, t], one rounded subtraction (a NaN
//     propagates), formed when the row enters LDS: SPEI is the index of the climatic water balance D = P - PET.
//   log-logistic fit (three parameters, unbiased probability-weighted moments; Vicente-Serrano et al. 2010, Begueria et al.
//     2014 "ub-pwm"): an element of R NaN, or n < 4 -> NaN row.  Sort R ascending, s_1 <= ... <= s_n (the order among equal
//     values does not matter).  Every sum runs from 0.0 over ascending i, no contraction; every coefficient is the quotient of
//     two exactly converted integers, multiplied into s_i:
//       w0 = (sum s_i) / n;   w1 = (sum s_i ((n - i) / (n - 1))) / n;   w2 = (sum s_i (((n - i)(n - i - 1)) / ((n - 1)(n - 2)))) / n
//       beta = (2 w1 - w0) / (6 w1 - w0 - 6 w2);   g = (pi / beta) / sin(pi / beta)   [= Gamma(1 + 1/beta) Gamma(1 - 1/beta)]
//       alpha = (w0 - 2 w1) beta / g;   gamma = w0 - alpha g.
//     Usable when all three are finite and 1 < |beta| <= max_shape; otherwise four NaNs (a constant sample, s_1 = s_n: 0 / 0
//     in exact arithmetic, tested for as such because the rounded sums leave noise over noise; |beta| beyond max_shape: a sample without measurable skew, alpha and gamma differences of huge numbers).  The sign is general:
//     beta = 1 / (L-skewness), so a negatively skewed sample gives beta < 0 and alpha < 0, and the same formulas describe the
//     mirrored distribution with the UPPER bound gamma.  The row is (alpha, beta, gamma, n).
//   log-logistic evaluation: X NaN or a NaN row -> NaN;  z = (X - gamma) / alpha;  z <= 0 (outside the support): H = 0 for
//     alpha > 0, H = 1 for alpha < 0;  else H = 1 / (1 + exp(-beta log z));  index = clip(ndtri(H), +-3.09): H = 0 gives
//     exactly -3.09, H = 1 exactly +3.09.
//   WHERE THE ERROR IS.  (1) the denominator 6 w1 - w0 - 6 w2 is a difference of three numbers of the size of the
//     sample's mean that leaves a number of the size of its L-skewness times its L-scale: beta, and through it
//     alpha and gamma, lose log2(|mean| |beta| / L-scale) bits -- the row shifted by 1e6 in the golden inputs is the worst
//     case there.  (2) exp(beta log z) at large |beta|: the rounding of log z (and of z itself) is multiplied by |beta|, so H
//     carries a relative error of ~ |beta log z| eps.  Both are shared by every float64 implementation of the definition;
//     the 40-digit golden has neither.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XH_SI_HD __host__ __device__ __forceinline__
#else
#define XH_SI_HD inline
#endif
#include <cmath>

#define XH_SI_MAXIT 512
#define XH_SI_CLIP 3.09
#define XH_SI_GAMMA 0
#define XH_SI_EMPIRICAL 1

struct XhSiPar {
    double q0, alpha, beta, n;
};

XH_SI_HD double xh_si_nan() { return __builtin_nan(""); }

// log(1 + u) - u without the cancellation at small u (the alternating series below |u| < 1/4: 27 terms reach 2^-56)
XH_SI_HD double xh_si_log1pmx(double u) {
    if (!(fabs(u) < 0.25)) return log1p(u) - u;
    const double mu = -u;
    double pw = u * u, s = 0.0;              // pw = (-u)^j
    for (int j = 2; j < 30; ++j) {
        s += pw / (double)j;
        pw *= mu;
    }
    return -s;
}

// Stirling's correction: lgamma(z) = (z - 1/2) log z - z + log(2 pi) / 2 + c(z); six terms, below 6e-17 beyond them at z >= 12
XH_SI_HD double xh_si_stirling(double z) {
    const double w = 1.0 / (z * z);
    return (1.0 / 12.0 - (1.0 / 360.0 - (1.0 / 1260.0 - (1.0 / 1680.0 - (1.0 / 1188.0 - (691.0 / 360360.0) * w) * w) * w) * w) * w) / z;
}

// F = x^a e^-x / Gamma(a) for a > 0, x > 0
XH_SI_HD double xh_si_prefactor(double a, double x) {
    const double two_pi = 6.283185307179586476925;
    if (a >= 12.0) {
        const double u = (x - a) / a;
        // (towards u = -1 the rounding of u is large against 1 + u: log(x / a) there, where the exponent is below -0.19 a)
        const double l = u > -0.5 ? xh_si_log1pmx(u) : log(x / a) - u;
        return sqrt(a / two_pi) * exp(a * l - xh_si_stirling(a));
    }
    double z = a, prod = 1.0;
    for (int i = 0; i < 12; ++i) {
        if (z >= 12.0) break;
        prod *= z;
        z += 1.0;
    }
    const double lg = (z - 0.5) * log(z) - z + 0.5 * log(two_pi) + xh_si_stirling(z) - log(prod);
    return exp(a * log(x) - x - lg);
}

// P(a, x); *iters (may be NULL) receives the iterations the loop took.  a <= 0, x < 0 or a NaN -> NaN; x == 0 -> 0.
XH_SI_HD double xh_si_gammap(double a, double x, int *iters) {
    if (iters) *iters = 0;
    if (!(a > 0.0) || !(x >= 0.0) || a == __builtin_inf()) return xh_si_nan();
    if (x == 0.0) return 0.0;
    if (x == __builtin_inf()) return 1.0;
    const double eps = 1.1102230246251565e-16;             // 2^-53
    const double f = xh_si_prefactor(a, x);
    if (x < a + 1.0) {
        double ap = a, del = 1.0 / a, sum = del;
        for (int j = 1; j <= XH_SI_MAXIT; ++j) {
            ap += 1.0;
            del *= x / ap;
            sum += del;
            if (del <= sum * eps) {
                if (iters) *iters = j;
                const double p = f * sum;
                return p > 1.0 ? 1.0 : p;
            }
        }
        if (iters) *iters = XH_SI_MAXIT + 1;
        return xh_si_nan();
    }
    if (f == 0.0) return 1.0;                               // the fraction is finite: Q underflows
    const double tiny = 1e-300;
    double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
    for (int j = 1; j <= XH_SI_MAXIT; ++j) {
        const double an = -(double)j * ((double)j - a);
        b += 2.0;
        d = an * d + b;
        d = fabs(d) < tiny ? tiny : d;
        c = b + an / c;
        c = fabs(c) < tiny ? tiny : c;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) <= 2.0 * eps) {
            if (iters) *iters = j;
            const double q = f * h;
            return q > 1.0 ? 0.0 : 1.0 - q;
        }
    }
    if (iters) *iters = XH_SI_MAXIT + 1;
    return xh_si_nan();
}

// AS 241 PPND16.  p <= 0 -> -inf, p >= 1 -> +inf, NaN -> NaN.
XH_SI_HD double xh_si_ndtri(double p) {
    if (p != p) return p;
    if (p <= 0.0) return -__builtin_inf();
    if (p >= 1.0) return __builtin_inf();
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                                4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                             1.3314166789178437745e+2) * r + 3.3871328727963666080e+0);
        const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                                2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                             4.2313330701600911252e+1) * r + 1.0);
        return q * num / den;
    }
    double r = q < 0.0 ? p : 1.0 - p;
    r = sqrt(-log(r));
    double val;
    if (r <= 5.0) {
        r -= 1.6;
        const double num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                                1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
                             4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
        const double den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                                1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
                             2.05319162663775882187e+0) * r + 1.0);
        val = num / den;
    } else {
        r -= 5.0;
        const double num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
                                2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
                             5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
        const double den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
                                7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
                             5.99832206555887937690e-1) * r + 1.0);
        val = num / den;
    }
    return q < 0.0 ? -val : val;
}

XH_SI_HD double xh_si_clip(double z) {
    z = z < -XH_SI_CLIP ? -XH_SI_CLIP : z;                  // (a NaN passes both selects)
    return z > XH_SI_CLIP ? XH_SI_CLIP : z;
}

// The gamma fit of one sample: s(i), i in [0, n), is the sample in ascending month order.
template <typename S>
XH_SI_HD XhSiPar xh_si_fit_gamma(S s, int n, double max_shape) {
    const double nan = xh_si_nan();
    const XhSiPar bad = {nan, nan, nan, nan};
    int n0 = 0, np = 0;
    bool unusable = false;
    double sum = 0.0, sumlog = 0.0;
    for (int i = 0; i < n; ++i) {
        const double v = s(i);
        unusable |= !(v >= 0.0);                            // NaN or negative
        if (v > 0.0) {
            sum += v;
            sumlog += log(v);
            ++np;
        } else if (v == 0.0) {
            ++n0;
        }
    }
    if (unusable || np < 4) return bad;
    const double mu = sum / (double)np, ml = sumlog / (double)np;
    const double A = log(mu) - ml;
    if (!(A > 0.0)) return bad;
    const double alpha = (1.0 + sqrt(1.0 + 4.0 * A / 3.0)) / (4.0 * A);
    if (!(alpha <= max_shape)) return bad;
    const XhSiPar par = {(double)n0 / (double)n, alpha, mu / alpha, (double)n};
    return par;
}

XH_SI_HD double xh_si_eval_gamma(double X, const XhSiPar &par) {
    if (!(X >= 0.0) || par.q0 != par.q0 || par.alpha != par.alpha || par.beta != par.beta) return xh_si_nan();
    const double H = X == 0.0 ? par.q0 : par.q0 + (1.0 - par.q0) * xh_si_gammap(par.alpha, X / par.beta, nullptr);
    return xh_si_clip(xh_si_ndtri(H));
}

// The empirical index of X against the sample s(i), i in [0, n); in_ref: 1 when X is itself an element of the sample.
template <typename S>
XH_SI_HD double xh_si_eval_empirical(double X, S s, int n, int in_ref) {
    int L = 0, E = 0;
    bool has_nan = false;
    for (int i = 0; i < n; ++i) {
        const double v = s(i);
        has_nan |= (v != v);
        L += v < X ? 1 : 0;
        E += v == X ? 1 : 0;
    }
    if (X != X || has_nan || n < 4) return xh_si_nan();
    const double N = (double)(n + 1 - in_ref);
    const double rank = (double)L + (double)(E + 2 - in_ref) / 2.0;
    return xh_si_clip(xh_si_ndtri((rank - 0.44) / (N + 0.12)));
}

// ---- log-logistic (SPEI)
#define XH_SI_LOGLOGISTIC 2

struct XhSiLogLogistic {
    double alpha, beta, gamma, n;
};

// Rank by counting: the position of element j of the sample s(i), i in [0, n), in ascending order -- #{s < s_j} + #{s = s_j
// at an earlier i}.  A NaN counts as larger than every number and equal to another NaN, so the ranks of a sample are always a
// permutation of 0 .. n - 1 (a scatter by rank writes every slot once), with the NaNs last.
template <typename S>
XH_SI_HD int xh_si_rank(S s, int n, int j) {
    const double x = s(j);
    const bool xnan = x != x;
    int r = 0;
    for (int i = 0; i < n; ++i) {
        const double v = s(i);
        const bool less = xnan ? (v == v) : (v < x);
        const bool same = xnan ? (v != v) : (v == x);
        r += (less || (same && i < j)) ? 1 : 0;
    }
    return r;
}

// The log-logistic fit of one sample: s(i), i in [0, n), is the sample SORTED ascending (NaNs, if any, last).
template <typename S>
XH_SI_HD XhSiLogLogistic xh_si_fit_loglogistic(S s, int n, double max_shape) {
    const double nan = xh_si_nan();
    const XhSiLogLogistic bad = {nan, nan, nan, nan};
    if (n < 4 || s(0) == s(n - 1)) return bad;              // (a constant sample: in exact arithmetic 0 / 0)
    const double d1 = (double)(n - 1), d2 = (double)((n - 1) * (n - 2));
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = 1; i <= n; ++i) {                          // (i as in the definition: s_1 the smallest)
        const double v = s(i - 1);
        s0 += v;
        s1 += v * ((double)(n - i) / d1);
        s2 += v * ((double)((n - i) * (n - i - 1)) / d2);
    }
    if (s0 != s0) return bad;                               // an element NaN (an infinite one fails the test below)
    const double w0 = s0 / (double)n, w1 = s1 / (double)n, w2 = s2 / (double)n;
    const double pi = 3.141592653589793238463;
    const double beta = (2.0 * w1 - w0) / (6.0 * w1 - w0 - 6.0 * w2);
    const double pb = pi / beta;
    const double g = pb / sin(pb);
    const double alpha = (w0 - 2.0 * w1) * beta / g;
    const double gamma = w0 - alpha * g;
    const double inf = __builtin_inf();
    const bool finite = fabs(alpha) < inf && fabs(beta) < inf && fabs(gamma) < inf;      // (false for a NaN)
    if (!finite || !(fabs(beta) > 1.0) || !(fabs(beta) <= max_shape)) return bad;
    const XhSiLogLogistic par = {alpha, beta, gamma, (double)n};
    return par;
}

// H(X) of the fitted distribution; NaN for a NaN X or a NaN row.
XH_SI_HD double xh_si_cdf_loglogistic(double X, const XhSiLogLogistic &par) {
    if (X != X || par.alpha != par.alpha || par.beta != par.beta || par.gamma != par.gamma) return xh_si_nan();
    const double z = (X - par.gamma) / par.alpha;
    if (z != z) return xh_si_nan();                         // (inf - inf, 0 / 0: a table that no fit writes)
    if (z <= 0.0) return par.alpha > 0.0 ? 0.0 : 1.0;       // outside the support
    return 1.0 / (1.0 + exp(-par.beta * log(z)));
}

XH_SI_HD double xh_si_eval_loglogistic(double X, const XhSiLogLogistic &par) {
    return xh_si_clip(xh_si_ndtri(xh_si_cdf_loglogistic(X, par)));
}
