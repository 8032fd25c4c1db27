// Hydropower post-processors on the device: the array math of xanthos/hydropower/potential.py and actual.py on the
// routed channel flow Avg_ChFlow [ncell, nmonths] the pipeline leaves in HBM.
//
//   k_hpot_qmax    constrain_q (potential.py:75-86): per cell, np.percentile(q[c, :], q_ex * 100) over all months with
//                  numpy's "linear" method.  One wave per cell: the row is staged in LDS as order-preserving 64-bit keys
//                  and an 8-bit radix select finds order statistic k_prev; order statistic k_next is the same value when
//                  more than k_next samples are <= it, else the smallest larger sample.  numpy's _lerp, both branches.
//                  A NaN anywhere in the row gives NaN, as np.percentile does.
//   k_hpot_energy  potential.py:30-46 for one cell per thread: np.clip(q, 0, q_max), the energy
//                  ef * 9810 * q * 730.5 * 1e-12 * elevD evaluated left to right, summed per calendar year with pandas'
//                  compensated group sum (resample("A").sum(): Kahan in month order, NaN skipped, an empty year 0), times
//                  0.0036.  The monthly energy is never stored: E [ncell, nyears].
//   k_hpot_region  groupby(key, axis=1).sum() (:50, :61): one thread per (group, year) walks the group's cells in cell
//                  order (CSR from the host) with the same compensated sum.
//   k_hact_inflow  actual.py:56-62: the dam cells' rows of Avg_ChFlow times CATCH / assumed area times 2.6298, written
//                  transposed to [nmonths, ndams] (the march reads one row per month, coalesced), then per dam the
//                  environmental flow (:109-117): monthly means by pandas' compensated group mean, the mean of all
//                  months by numpy's pairwise sum / n (Series.mean).  A dam whose inflow holds a NaN is flagged.
//   k_hact_sim     get_power (:124-145) with one lane per dam marching the months; Python's min / max as written (the
//                  first argument unless the second is strictly smaller / larger).  power [nmonths, ndams] and the
//                  per-dam annual means (resample("A").mean(), compensated, [nyears, ndams]).  A month in which no
//                  rule-curve row is <= s / cap (the reference's IndexError) is flagged with the first such month.
//
// Every compensated loop below depends on the absence of fp contraction (the Makefile builds with -ffp-contract=off;
// the pragma keeps it so if the file is ever compiled on its own).
#include <cmath>
#include <cstdint>

#include "xh_launch.h"
#include "xh_kahan.h"

#pragma clang fp contract(off)

namespace {

constexpr int QMAX_THREADS = 64;                 // one wave per cell
constexpr int QMAX_MAX_MONTHS = 8192;            // 64 KiB of keys in LDS

__device__ __forceinline__ uint64_t order_key(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double key_value(uint64_t k) {
    const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// pandas' compensated add (xh_kahan.h) with the count of the values that went in (group_mean divides by it)
struct Kahan {
    double s, c;
    int n;
    __device__ void reset() { s = 0.0; c = 0.0; n = 0; }
    __device__ void add(double v) {
        if (v != v) return;
        ++n;
        kahan_add(s, c, v);
    }
};

__global__ void __launch_bounds__(QMAX_THREADS) k_hpot_qmax(int64_t ncell, int nmonths, int k_prev, int k_next,
                                                            double gamma, const double *__restrict__ q,
                                                            double *__restrict__ qmax) {
    extern __shared__ uint64_t keys[];
    __shared__ unsigned hist[256];
    __shared__ uint64_t s_prefix, s_next;
    __shared__ int s_k, s_nan, s_le;
    const int lane = threadIdx.x;
    for (int64_t c = blockIdx.x; c < ncell; c += gridDim.x) {
        const double *row = q + c * (int64_t)nmonths;
        if (lane == 0) {
            s_nan = 0;
            s_prefix = 0;
            s_k = k_prev;
            s_le = 0;
            s_next = ~0ull;
        }
        __syncthreads();
        int nan = 0;
        for (int i = lane; i < nmonths; i += QMAX_THREADS) {
            const double v = row[i];
            nan |= (v != v);
            keys[i] = order_key(v);
        }
        if (nan) s_nan = 1;
        __syncthreads();
        if (s_nan) {                                   // np.percentile: a NaN in the sample gives NaN
            if (lane == 0) qmax[c] = NAN;
            __syncthreads();
            continue;
        }
        uint64_t mask = 0;
        for (int shift = 56; shift >= 0; shift -= 8) {
            for (int b = lane; b < 256; b += QMAX_THREADS) hist[b] = 0;
            __syncthreads();
            const uint64_t prefix = s_prefix;
            for (int i = lane; i < nmonths; i += QMAX_THREADS) {
                const uint64_t k = keys[i];
                if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
            }
            __syncthreads();
            // lane l owns bins 4l .. 4l+3: an inclusive scan over the wave finds the bin that holds rank s_k
            unsigned h4[4], own = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                h4[j] = hist[4 * lane + j];
                own += h4[j];
            }
            unsigned incl = own;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned o = __shfl_up(incl, d, 64);
                if (lane >= d) incl += o;
            }
            const int k = s_k;
            const unsigned long long hit = __ballot(incl > (unsigned)k);
            const int first = __ffsll((long long)hit) - 1;
            if (lane == first) {
                unsigned before = incl - own;
                int bin = 0;
                for (int j = 0; j < 4; ++j) {
                    if (before + h4[j] > (unsigned)k) {
                        bin = 4 * lane + j;
                        break;
                    }
                    before += h4[j];
                }
                s_k = k - (int)before;
                s_prefix = prefix | ((uint64_t)bin << shift);
            }
            mask |= (uint64_t)255 << shift;
            __syncthreads();
        }
        const uint64_t ka = s_prefix;
        int le = 0;
        uint64_t next = ~0ull;
        for (int i = lane; i < nmonths; i += QMAX_THREADS) {
            const uint64_t k = keys[i];
            le += k <= ka ? 1 : 0;
            next = (k > ka && k < next) ? k : next;
        }
        atomicAdd(&s_le, le);
        atomicMin((unsigned long long *)&s_next, (unsigned long long)next);
        __syncthreads();
        if (lane == 0) {
            const double a = key_value(ka);
            const double b = (k_next == k_prev || s_le > k_next) ? a : key_value(s_next);
            const double d = b - a;                                   // numpy _lerp
            double r = a + d * gamma;
            r = gamma >= 0.5 ? b - d * (1.0 - gamma) : r;
            qmax[c] = r;
        }
        __syncthreads();
    }
}

// np.clip(x, lo, hi) for floats: _NPY_MIN(_NPY_MAX(x, lo), hi) with NaN in x propagated
__device__ __forceinline__ double np_clip(double x, double lo, double hi) {
    const double m = (x != x) ? x : (x > lo ? x : lo);
    return (m != m) ? m : (m < hi ? m : hi);
}

// thread <-> cell; year_of_month[t] = index of month t's calendar year (0 .. nyears-1, non-decreasing)
__global__ void __launch_bounds__(256) k_hpot_energy(int64_t ncell, int nmonths, int nyears,
                                                     const int *__restrict__ year_of_month, double c_ef_sww, double c_hours,
                                                     double c_twh, double c_ej, const double *__restrict__ q,
                                                     const double *__restrict__ qmax, const double *__restrict__ elev,
                                                     double *__restrict__ E) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    const double *row = q + c * (int64_t)nmonths;
    const double hi = qmax[c], el = elev[c];
    double *out = E + c * (int64_t)nyears;
    Kahan k;
    k.reset();
    int y = 0;
    for (int t = 0; t < nmonths; ++t) {
        const int yt = year_of_month[t];
        if (yt != y) {
            out[y] = k.s * c_ej;
            k.reset();
            y = yt;
        }
        const double qc = np_clip(row[t], 0.0, hi);
        const double e = (((c_ef_sww * qc) * c_hours) * c_twh) * el;      // potential.py:33-36, left to right
        k.add(e);
    }
    out[y] = k.s * c_ej;
}

// thread <-> (group, year): R [ngroups, nyears]
__global__ void __launch_bounds__(256) k_hpot_region(int ngroups, int nyears, const int64_t *__restrict__ indptr,
                                                     const int64_t *__restrict__ cells, const double *__restrict__ E,
                                                     double *__restrict__ R) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)ngroups * nyears) return;
    const int g = (int)(i / nyears), y = (int)(i - (int64_t)g * nyears);
    Kahan k;
    k.reset();
    int64_t j = indptr[g];
    const int64_t end = indptr[g + 1];
    // the adds are one dependent chain in cell order; the loads are not: 16 in flight at a time (one group may hold
    // half the grid, and a load per add would make its thread wait a memory latency per cell)
    for (; j + 16 <= end; j += 16) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = E[cells[j + u] * (int64_t)nyears + y];
#pragma unroll
        for (int u = 0; u < 16; ++u) k.add(v[u]);
    }
    for (; j < end; ++j) k.add(E[cells[j] * (int64_t)nyears + y]);
    R[i] = k.s;
}

// thread <-> (month, dam): inflow [nmonths, ndams]
__global__ void __launch_bounds__(256) k_hact_gather(int64_t ncell, int nmonths, int ndams, const int64_t *__restrict__ dam_cell,
                                                     const double *__restrict__ catch_area,
                                                     const double *__restrict__ assumed_area, double cumecs_to_mm3,
                                                     const double *__restrict__ q, double *__restrict__ inflow) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)nmonths * ndams) return;
    const int t = (int)(i / ndams), d = (int)(i - (int64_t)t * ndams);
    const double v = q[dam_cell[d] * (int64_t)nmonths + t];
    inflow[i] = ((v * catch_area[d]) / assumed_area[d]) * cumecs_to_mm3;     // actual.py:60-62
}

// numpy's pairwise sum (loops_utils.h.src pairwise_sum) of x[0], x[stride], ... x[(n-1) stride], n <= 128 leaf
__device__ double pairwise_leaf(const double *x, int64_t stride, int n) {
    if (n < 8) {
        double r = -0.0;
        for (int i = 0; i < n; ++i) r += x[i * stride];
        return r;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = x[j * stride];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += x[(i + j) * stride];
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += x[i * stride];
    return res;
}

// the recursion of pairwise_sum (halves rounded down to a multiple of 8) with an explicit stack, left to right
__device__ double pairwise_sum(const double *x, int64_t stride, int n) {
    struct Frame {
        int off, n, state;
        double left;
    };
    Frame st[24];
    int sp = 0;
    st[0] = {0, n, 0, 0.0};
    double ret = 0.0;
    while (sp >= 0) {
        Frame &f = st[sp];
        if (f.n <= 128) {
            ret = pairwise_leaf(x + (int64_t)f.off * stride, stride, f.n);
            --sp;
            continue;
        }
        int n2 = f.n / 2;
        n2 -= n2 % 8;
        if (f.state == 0) {
            f.state = 1;
            st[sp + 1] = {f.off, n2, 0, 0.0};
            ++sp;
        } else if (f.state == 1) {
            f.left = ret;
            f.state = 2;
            st[sp + 1] = {f.off + n2, f.n - n2, 0, 0.0};
            ++sp;
        } else {
            ret = f.left + ret;
            --sp;
        }
    }
    return 0.0 + ret;                                  // np.add.reduce starts from the identity
}

// thread <-> dam: env [ndams, 12] (calendar months 1..12 -> 0..11), bad[d] = 1 when the inflow holds a NaN
__global__ void __launch_bounds__(256) k_hact_env(int nmonths, int ndams, int month0, const double *__restrict__ inflow,
                                                  double *__restrict__ env, int *__restrict__ bad) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= ndams) return;
    Kahan k[12];
    for (int m = 0; m < 12; ++m) k[m].reset();
    int nan = 0;
    int m = month0;
    for (int t = 0; t < nmonths; ++t) {
        const double v = inflow[(int64_t)t * ndams + d];
        nan |= (v != v);
        k[m].add(v);
        m = m == 11 ? 0 : m + 1;
    }
    const double maf = pairwise_sum(inflow + d, ndams, nmonths) / (double)nmonths;   // Series.mean (no NaN: n = count)
    for (int j = 0; j < 12; ++j) {
        const double mmf = k[j].s / (double)k[j].n;                                    // groupby(month).mean()
        const double lo = 0.4 * maf, hi = 0.8 * maf;
        const double p = (mmf < lo ? 0.6 : 0.0) + ((mmf >= lo && mmf <= hi) ? 0.45 : 0.0) +
                         ((mmf > hi) ? 0.3 * ((mmf < 1.0) ? 0.0 : 1.0) : 0.0);
        env[(int64_t)d * 12 + j] = p * mmf;
    }
    bad[d] = nan;
}

__device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }

// thread <-> dam.  rc [5, 12, ndams] (NaN already replaced by 1.1); par [5, ndams]: cap, cap_live, q_max, eff, head
__global__ void __launch_bounds__(256) k_hact_sim(int nmonths, int ndams, int nyears, int month0,
                                                  const int *__restrict__ year_of_month, double sww, double secs_in_month,
                                                  const double *__restrict__ inflow, const double *__restrict__ env,
                                                  const double *__restrict__ rc, const double *__restrict__ par,
                                                  double *__restrict__ power, double *__restrict__ annual,
                                                  int *__restrict__ bad_month) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= ndams) return;
    const double cap = par[d], cap_live = par[ndams + d], q_max = par[2 * ndams + d], eff = par[3 * ndams + d],
                 head = par[4 * ndams + d];
    const double breaks[5] = {0.0, 0.25, 0.5, 0.75, 1.0};          // np.linspace(0, 1, 5)
    double e12[12];
    for (int j = 0; j < 12; ++j) e12[j] = env[(int64_t)d * 12 + j];
    double s = cap;
    int m = month0, y = 0, first_bad = -1;
    Kahan k;
    k.reset();
    for (int t = 0; t < nmonths; ++t) {
        const double in = inflow[(int64_t)t * ndams + d];
        const double s_state = s / cap;
        const double active = s + in - (cap - cap_live);
        int last = -1;
#pragma unroll
        for (int i = 0; i < 5; ++i) last = rc[((int64_t)i * 12 + m) * ndams + d] <= s_state ? i : last;
        if (last < 0 && first_bad < 0) first_bad = t;
        const double release = breaks[last < 0 ? 0 : last] * q_max;
        const double r = py_min(py_min(py_max(release, e12[m]), active), q_max);
        const double s1 = py_max(py_min(s + in - r, cap), 0.0);
        const double h = ((0.0 + (s + s1)) / 2.0 / cap) * head;        // np.mean([s, s']): add.reduce from 0.0, / 2
        const double p = py_max(eff * sww * h * (r / secs_in_month), 0.0);
        power[(int64_t)t * ndams + d] = p;
        const int yt = year_of_month[t];
        if (yt != y) {
            annual[(int64_t)y * ndams + d] = k.s / (double)k.n;
            k.reset();
            y = yt;
        }
        k.add(p);
        s = s1;
        m = m == 11 ? 0 : m + 1;
    }
    annual[(int64_t)y * ndams + d] = k.s / (double)k.n;
    (void)nyears;
    bad_month[d] = first_bad;
}

}  // namespace

extern "C" int xh_hpot_qmax(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t k_prev, int32_t k_next, double gamma,
                            const double *d_q, double *d_qmax) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, d_q && d_qmax && ncell >= 0 && nmonths > 0, "xh_hpot_qmax: bad argument");
    XH_REQUIRE(ctx, nmonths <= QMAX_MAX_MONTHS,
               "xh_hpot_qmax: %d months per cell, at most %d fit the kernel's LDS staging", nmonths, QMAX_MAX_MONTHS);
    XH_REQUIRE(ctx, k_prev >= 0 && k_prev < nmonths && k_next >= k_prev && k_next < nmonths && gamma >= 0.0 && gamma <= 1.0,
               "xh_hpot_qmax: order statistics %d, %d / weight %g invalid for %d samples", k_prev, k_next, gamma, nmonths);
    if (ncell == 0) return XH_OK;
    return xh_launch(ctx, "hpot_qmax", ctx->stream, k_hpot_qmax, xh_grid(ctx, ncell, 1, 32), QMAX_THREADS,
                     (size_t)nmonths * sizeof(uint64_t), ncell, (int)nmonths, (int)k_prev, (int)k_next, gamma, d_q, d_qmax);
}

extern "C" int xh_hpot_energy(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t nyears, const int32_t *d_year_of_month,
                              double c_ef_sww, double c_hours, double c_twh, double c_ej, const double *d_q,
                              const double *d_qmax, const double *d_elev, double *d_E) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, d_year_of_month && d_q && d_qmax && d_elev && d_E && ncell >= 0 && nmonths > 0 && nyears > 0,
               "xh_hpot_energy: bad argument");
    if (ncell == 0) return XH_OK;
    return xh_launch(ctx, "hpot_energy", ctx->stream, k_hpot_energy, xh_grid(ctx, ncell, 256), 256, 0, ncell, (int)nmonths,
                     (int)nyears, d_year_of_month, c_ef_sww, c_hours, c_twh, c_ej, d_q, d_qmax, d_elev, d_E);
}

extern "C" int xh_hpot_region(xh_ctx *ctx, int32_t ngroups, int32_t nyears, const int64_t *d_indptr, const int64_t *d_cells,
                              const double *d_E, double *d_R) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, d_indptr && d_cells && d_E && d_R && ngroups >= 0 && nyears > 0, "xh_hpot_region: bad argument");
    if (ngroups == 0) return XH_OK;
    return xh_launch(ctx, "hpot_region", ctx->stream, k_hpot_region, xh_grid(ctx, (int64_t)ngroups * nyears, 256), 256, 0,
                     (int)ngroups, (int)nyears, d_indptr, d_cells, d_E, d_R);
}

extern "C" int xh_hact_inflow(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t ndams, int32_t month0,
                              const int64_t *d_dam_cell, const double *d_catch, const double *d_assumed, double cumecs_to_mm3,
                              const double *d_q, double *d_inflow, double *d_env, int32_t *d_bad) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, d_dam_cell && d_catch && d_assumed && d_q && d_inflow && d_env && d_bad && ncell > 0 && nmonths > 0 &&
                        ndams >= 0 && month0 >= 0 && month0 < 12,
               "xh_hact_inflow: bad argument");
    XH_REQUIRE(ctx, nmonths >= 12, "xh_hact_inflow: %d months do not cover every calendar month", nmonths);
    if (ndams == 0) return XH_OK;
    return xh_timed(ctx, "hact_inflow", ctx->stream, [&] {
        const int rc = xh_launch(ctx, nullptr, ctx->stream, k_hact_gather, xh_grid(ctx, (int64_t)nmonths * ndams, 256), 256, 0,
                                 ncell, (int)nmonths, (int)ndams, d_dam_cell, d_catch, d_assumed, cumecs_to_mm3, d_q, d_inflow);
        if (rc) return rc;
        return xh_launch(ctx, nullptr, ctx->stream, k_hact_env, xh_grid(ctx, ndams, 256), 256, 0, (int)nmonths, (int)ndams,
                         (int)month0, d_inflow, d_env, d_bad);
    });
}

extern "C" int xh_hact_sim(xh_ctx *ctx, int32_t nmonths, int32_t ndams, int32_t nyears, int32_t month0,
                           const int32_t *d_year_of_month, double sww, double secs_in_month, const double *d_inflow,
                           const double *d_env, const double *d_rc, const double *d_par, double *d_power, double *d_annual,
                           int32_t *d_bad_month) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, d_year_of_month && d_inflow && d_env && d_rc && d_par && d_power && d_annual && d_bad_month &&
                        nmonths > 0 && ndams >= 0 && nyears > 0 && month0 >= 0 && month0 < 12,
               "xh_hact_sim: bad argument");
    if (ndams == 0) return XH_OK;
    return xh_launch(ctx, "hact_sim", ctx->stream, k_hact_sim, xh_grid(ctx, ndams, 256), 256, 0, (int)nmonths, (int)ndams,
                     (int)nyears, (int)month0, d_year_of_month, sww, secs_in_month, d_inflow, d_env, d_rc, d_par, d_power,
                     d_annual, d_bad_month);
}
