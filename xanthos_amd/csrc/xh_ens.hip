// Across-member statistics of an ensemble of runs, formed in HBM.
//
// Replaces nothing of the reference: there the members of a scenario sweep are whole runs of Xanthos.execute(args) and
// their mean / spread / quantiles are formed afterwards on the host, from S x [ncell, ncols] arrays per variable.  Here the
// S arrays of one variable as written (xanthos_amd/ensemble.py keeps them in HBM) go through one kernel:
//
//   k_ens_reg<SMAX>   S <= 16: the S values of an element live in registers (SMAX = 2, 4, 8, 16 doubles: 28 / 32 / 46 / 88
//                     VGPRs in all, no scratch: 8 waves per SIMD up to SMAX = 8, 5 at 16); sorted by an odd-even
//                     transposition network whose indices are compile-time constants, the tail padded with +inf.
//   k_ens_lds         16 < S <= 64: one-wave workgroups, the values of lane l at lds[j * 64 + l] (a column per lane, so a
//                     wave's access to member j is 512 consecutive bytes: no bank conflicts, and no barrier is ever needed
//                     because a lane touches only its own column).  S x 512 B per wave: 18 waves per CU at S = 17, 5 at
//                     S = 64 of the 160 KB -- 64 doubles in registers would be 128 VGPRs of values alone (<= 2 waves per
//                     SIMD with the temporaries, 8 per CU, and a 2016-exchange network); sorted by insertion.
//
// Either way thread <-> element with consecutive lanes on consecutive elements, so every access to a member array or an
// output is a coalesced 512-byte row of a wave, and each member array is read from HBM exactly ONCE per call whatever the
// number of statistics: the value is added to the running sum, compared for min / max and kept (registers / LDS) for the
// second pass of the standard deviation and for the sort of the quantiles.  Plain vector loads and stores, no atomics.
//
// The definitions are numpy's over axis 0 of the stacked array, operation for operation (the tests hold the kernel to
// numpy itself, bit for bit; finite or NaN inputs):
//   mean      sum in member order from 0.0, / S
//   std       ddof = 1: that mean, sum in member order of (x - mean)^2, / (S - 1), sqrt; NaN for S = 1 (0 / 0)
//   min, max  m = (m < x || m != m) ? m : x in member order (NaN propagates)
//   quantile  ascending sort, h = (S - 1) q, lo = floor(h), hi = min(lo + 1, S - 1), g = h - lo, d = a[hi] - a[lo],
//             g < 0.5 ? a[lo] + d g : a[hi] - d (1 - g)  (numpy's _lerp); NaN when any member is NaN
// (h, lo, hi and g depend on S and q only: the host computes them in double as numpy does.)
// The lerp and the squared deviations depend on the absence of fp contraction (-ffp-contract=off; the pragma keeps it so).
#include <cmath>

#include "xh_launch.h"

#pragma clang fp contract(off)

namespace {

constexpr int ENS_MAX_MEMBERS = 64;       // compiled limit of S (the LDS form: 32 KB per one-wave workgroup)
constexpr int ENS_REG_MEMBERS = 16;       // up to here the values of an element are held in registers
constexpr int ENS_MAX_QUANTILES = 16;
constexpr int ENS_LDS_LANES = 64;

struct EnsOut {      // kernel argument: where each requested statistic goes (NULL: not requested) and the quantiles' indices
    double *mean, *std, *mn, *mx;
    double *q[ENS_MAX_QUANTILES];
    double g[ENS_MAX_QUANTILES];
    int lo[ENS_MAX_QUANTILES], hi[ENS_MAX_QUANTILES];
    int nq;
};

__device__ __forceinline__ double np_min(double m, double x) { return (m < x || m != m) ? m : x; }
__device__ __forceinline__ double np_max(double m, double x) { return (m > x || m != m) ? m : x; }

// numpy's _lerp(a, b, t) of the 'linear' method
__device__ __forceinline__ double np_lerp(double a, double b, double g) {
    const double d = b - a;
    return g < 0.5 ? a + d * g : b - d * (1.0 - g);
}

template <int SMAX>
__global__ void __launch_bounds__(256) k_ens_reg(int64_t n, int S, const double *const *__restrict__ members, EnsOut o) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double v[SMAX];
#pragma unroll
        for (int j = 0; j < SMAX; ++j) v[j] = j < S ? members[j][i] : INFINITY;
        double sum = 0.0, mn = v[0], mx = v[0];
        bool nan = false;
#pragma unroll
        for (int j = 0; j < SMAX; ++j) {
            if (j < S) {
                sum += v[j];
                nan |= v[j] != v[j];
                if (j > 0) {
                    mn = np_min(mn, v[j]);
                    mx = np_max(mx, v[j]);
                }
            }
        }
        const double mean = sum / (double)S;
        if (o.mean) o.mean[i] = mean;
        if (o.mn) o.mn[i] = mn;
        if (o.mx) o.mx[i] = mx;
        if (o.std) {
            double ss = 0.0;
#pragma unroll
            for (int j = 0; j < SMAX; ++j) {
                if (j < S) {
                    const double d = v[j] - mean;
                    ss += d * d;
                }
            }
            o.std[i] = sqrt(ss / (double)(S - 1));
        }
        if (o.nq > 0) {
            // odd-even transposition sort: SMAX rounds over fixed pairs (the +inf pads stay behind the values)
#pragma unroll
            for (int r = 0; r < SMAX; ++r) {
#pragma unroll
                for (int j = r & 1; j + 1 < SMAX; j += 2) {
                    const double a = v[j], b = v[j + 1];
                    const bool swap = b < a;
                    v[j] = swap ? b : a;
                    v[j + 1] = swap ? a : b;
                }
            }
            for (int k = 0; k < o.nq; ++k) {
                const int lo = o.lo[k], hi = o.hi[k];
                double a = v[0], b = v[0];
#pragma unroll
                for (int j = 1; j < SMAX; ++j) {
                    if (j == lo) a = v[j];
                    if (j == hi) b = v[j];
                }
                o.q[k][i] = nan ? NAN : np_lerp(a, b, o.g[k]);
            }
        }
    }
}

__global__ void __launch_bounds__(ENS_LDS_LANES) k_ens_lds(int64_t n, int S, const double *const *__restrict__ members,
                                                            EnsOut o) {
    extern __shared__ double ens_lds[];                 // [S][64]
    double *col = ens_lds + threadIdx.x;                // this lane's values: col[j * 64]
    for (int64_t i = (int64_t)blockIdx.x * ENS_LDS_LANES + threadIdx.x; i < n; i += (int64_t)gridDim.x * ENS_LDS_LANES) {
        double sum = 0.0, mn = 0.0, mx = 0.0;
        bool nan = false;
#pragma unroll 8
        for (int j = 0; j < S; ++j) {
            const double x = members[j][i];
            col[j * ENS_LDS_LANES] = x;
            sum += x;
            nan |= x != x;
            mn = j ? np_min(mn, x) : x;
            mx = j ? np_max(mx, x) : x;
        }
        const double mean = sum / (double)S;
        if (o.mean) o.mean[i] = mean;
        if (o.mn) o.mn[i] = mn;
        if (o.mx) o.mx[i] = mx;
        if (o.std) {
            double ss = 0.0;
#pragma unroll 8
            for (int j = 0; j < S; ++j) {
                const double d = col[j * ENS_LDS_LANES] - mean;
                ss += d * d;
            }
            o.std[i] = sqrt(ss / (double)(S - 1));
        }
        if (o.nq > 0) {
            if (!nan) {                                 // (a NaN member makes every quantile NaN: nothing to sort)
                for (int j = 1; j < S; ++j) {
                    const double x = col[j * ENS_LDS_LANES];
                    int k = j - 1;
                    while (k >= 0) {
                        const double y = col[k * ENS_LDS_LANES];
                        if (!(y > x)) break;
                        col[(k + 1) * ENS_LDS_LANES] = y;
                        --k;
                    }
                    col[(k + 1) * ENS_LDS_LANES] = x;
                }
            }
            for (int k = 0; k < o.nq; ++k)
                o.q[k][i] = nan ? NAN : np_lerp(col[o.lo[k] * ENS_LDS_LANES], col[o.hi[k] * ENS_LDS_LANES], o.g[k]);
        }
    }
}

}  // namespace

extern "C" int xh_ens_stats(xh_ctx *ctx, int64_t n, int32_t nmembers, const double *const *h_d_members, uint32_t stat_mask,
                            int32_t nq, const double *h_q, double *const *h_d_out) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, n >= 0 && nmembers >= 1 && nq >= 0, "xh_ens_stats: bad size (n %lld, members %d, quantiles %d)", (long long)n,
               nmembers, nq);
    if (nmembers > ENS_MAX_MEMBERS)
        return xh_fail(ctx, XH_ERR_LIMIT, "xh_ens_stats: %d members exceed the compiled limit of %d", nmembers, ENS_MAX_MEMBERS);
    if (nq > ENS_MAX_QUANTILES)
        return xh_fail(ctx, XH_ERR_LIMIT, "xh_ens_stats: %d quantiles exceed the compiled limit of %d", nq, ENS_MAX_QUANTILES);
    const uint32_t all = XH_ENS_MEAN | XH_ENS_STD | XH_ENS_MIN | XH_ENS_MAX;
    XH_REQUIRE(ctx, (stat_mask & ~all) == 0 && (stat_mask != 0 || nq > 0), "xh_ens_stats: no statistic, or an unknown bit in 0x%x",
               stat_mask);
    XH_REQUIRE(ctx, h_d_members && h_d_out && (h_q || nq == 0), "xh_ens_stats: NULL argument");
    for (int j = 0; j < nmembers; ++j) XH_REQUIRE(ctx, h_d_members[j] || n == 0, "xh_ens_stats: member %d is NULL", j);
    EnsOut o{};
    int nout = 0;
    double **slots[4] = {&o.mean, &o.std, &o.mn, &o.mx};
    for (int b = 0; b < 4; ++b)
        if (stat_mask & (1u << b)) *slots[b] = h_d_out[nout++];
    o.nq = nq;
    for (int k = 0; k < nq; ++k) {
        const double q = h_q[k];
        XH_REQUIRE(ctx, q >= 0.0 && q <= 1.0, "xh_ens_stats: quantile %d (%g) outside [0, 1]", k, q);
        const double h = (double)(nmembers - 1) * q;
        const double fl = floor(h);
        o.lo[k] = (int)fl;
        o.hi[k] = o.lo[k] + 1 < nmembers ? o.lo[k] + 1 : nmembers - 1;
        o.g[k] = h - fl;
        o.q[k] = h_d_out[nout++];
    }
    for (int k = 0; k < nout; ++k) XH_REQUIRE(ctx, h_d_out[k] || n == 0, "xh_ens_stats: output %d is NULL", k);
    if (n == 0) return XH_OK;
    void *at[2];
    const int rc = xh_stage(ctx, 2, {{h_d_members, sizeof(double *) * (size_t)nmembers}}, 0, at);
    if (rc) return rc;
    const double *const *d_members = static_cast<const double *const *>(at[0]);
    const int S = nmembers;
    if (S <= ENS_REG_MEMBERS) {
        const unsigned grid = xh_grid(ctx, n, 256, 16);
        if (S <= 2) return xh_launch(ctx, "ens_stats", ctx->stream, k_ens_reg<2>, grid, 256, 0, n, S, d_members, o);
        if (S <= 4) return xh_launch(ctx, "ens_stats", ctx->stream, k_ens_reg<4>, grid, 256, 0, n, S, d_members, o);
        if (S <= 8) return xh_launch(ctx, "ens_stats", ctx->stream, k_ens_reg<8>, grid, 256, 0, n, S, d_members, o);
        return xh_launch(ctx, "ens_stats", ctx->stream, k_ens_reg<16>, grid, 256, 0, n, S, d_members, o);
    }
    const size_t lds = sizeof(double) * ENS_LDS_LANES * (size_t)S;
    const int per_cu = (int)((size_t)160 * 1024 / lds);            // one-wave workgroups that fit a CU's LDS
    return xh_launch(ctx, "ens_stats", ctx->stream, k_ens_lds, xh_grid(ctx, n, ENS_LDS_LANES, 4 * per_cu), ENS_LDS_LANES, lds, n,
                     S, d_members, o);
}
