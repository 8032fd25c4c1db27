// Diagnostics post-processor on the device: the reductions over cells of xanthos/diagnostics/diagnostics.py (DESIGN
// section 4.11).  The time-series plots (diagnostics/time_series.py:Aggregation_Map) reuse xh_agg_spatial.
//
//   k_diag_cell_total  diagnostics.py:58, q = np.sum(Q, axis=1) / nyear * area / 1e6, and np.mean(VIC, axis=1) (:62):
//                      per cell the total of its contiguous row in numpy's order for any row length, then the scaling
//                      in the reference's order.  numpy's reduction hands its inner loop blocks of at most 8192 values
//                      (the default ufunc buffer size) and adds their totals one after the other from 0.0; each block is
//                      summed by pairwise_sum (numpy/_core/src/umath/loops_utils.h.src).  One wave per cell: the row is
//                      staged in LDS with coalesced loads (rows are ncols x 8 bytes apart, so one lane per cell would
//                      touch 64 lines per wave instruction; rows over 60 KiB are read in place), then each lane runs one of
//                      the eight accumulators of one leaf of numpy's recursion, one lane per leaf folds its eight
//                      accumulators and its tail, and lane 0 combines the leaves in the recursion's order.  The shape of
//                      the recursion depends on ncols alone: the host writes it once as a leaf table and a postfix program.
//   k_diag_group_sum   diagnostics.py:112, runoff_df.groupby('id').sum(): per (group, column) pandas' compensated sum
//                      (groupby.pyx group_sum) over the group's cells in ascending cell order, NaN skipped, the
//                      compensation reset to 0 when it turns NaN (an infinite value), so +/-inf sums stay infinite.
//
// The compensated loop depends on the absence of fp contraction (the Makefile builds with -ffp-contract=off; the pragma
// keeps it so if the file is ever compiled on its own).
#include <cstdint>
#include <vector>

#include "xh_launch.h"
#include "xh_kahan.h"

#pragma clang fp contract(off)

namespace {

constexpr int TOTAL_THREADS = 64;                // one wave per cell
constexpr int PW_BLOCK = 128;                    // numpy's PW_BLOCKSIZE
constexpr int NP_BUFSIZE = 8192;                 // numpy's default ufunc buffer size: the longest inner-loop call
constexpr int PROGRAM_STACK = 16;                // a block of 8192 values is 7 levels deep, plus the running total
constexpr size_t STAGE_MAX_BYTES = 60 * 1024;    // rows longer than this are read from global memory in place

// numpy's recursion for n values at offset off: leaves of n <= 128 values in order, and the postfix program that adds
// them back up (token >= 0: push leaf; -1: pop b, pop a, push a + b)
void pairwise_plan(int off, int n, std::vector<int> &leaves, std::vector<int> &prog) {
    if (n <= PW_BLOCK) {
        prog.push_back((int)(leaves.size() / 2));
        leaves.push_back(off);
        leaves.push_back(n);
        return;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    pairwise_plan(off, n2, leaves, prog);
    pairwise_plan(off + n2, n - n2, leaves, prog);
    prog.push_back(-1);
}

// block <-> cell (grid-stride); d_leaves [2 * nleaves] (offset, length), d_prog [nprog]
template <bool STAGE>
__global__ void __launch_bounds__(TOTAL_THREADS) k_diag_cell_total(int64_t ncell, int ncols, int nleaves,
                                                                   const int *__restrict__ leaves, int nprog,
                                                                   const int *__restrict__ prog,
                                                                   const double *__restrict__ in, double div1,
                                                                   const double *__restrict__ scale, double div2,
                                                                   double *__restrict__ out, int64_t out_stride) {
    extern __shared__ double sh[];
    double *part = sh + (STAGE ? ncols : 0);     // [8 * nleaves] accumulators
    double *lsum = part + 8 * nleaves;           // [nleaves] leaf totals
    const int lane = threadIdx.x;
    for (int64_t c = blockIdx.x; c < ncell; c += gridDim.x) {
        const double *row = in + c * (int64_t)ncols;
        const double *src = row;
        if (STAGE) {
            int i = lane;
            for (; i + 3 * TOTAL_THREADS < ncols; i += 4 * TOTAL_THREADS) {      // four loads in flight per lane
                const double a = row[i], b = row[i + TOTAL_THREADS], d = row[i + 2 * TOTAL_THREADS],
                             e = row[i + 3 * TOTAL_THREADS];
                sh[i] = a;
                sh[i + TOTAL_THREADS] = b;
                sh[i + 2 * TOTAL_THREADS] = d;
                sh[i + 3 * TOTAL_THREADS] = e;
            }
            for (; i < ncols; i += TOTAL_THREADS) sh[i] = row[i];
            __syncthreads();
            src = sh;
        }
        // the eight accumulators of every leaf of >= 8 values: r[j] = a[j] + a[8 + j] + ... up to n - n % 8
        for (int p = lane; p < 8 * nleaves; p += TOTAL_THREADS) {
            const int lf = p >> 3, j = p & 7;
            const int off = leaves[2 * lf], n = leaves[2 * lf + 1];
            if (n < 8) continue;
            const double *a = src + off;
            double r = a[j];
            for (int i = 8; i < n - (n % 8); i += 8) r += a[i + j];
            part[p] = r;
        }
        __syncthreads();
        for (int lf = lane; lf < nleaves; lf += TOTAL_THREADS) {
            const int off = leaves[2 * lf], n = leaves[2 * lf + 1];
            const double *a = src + off;
            double res;
            int i;
            if (n < 8) {
                res = 0.0;
                i = 0;
            } else {
                const double *r = part + 8 * lf;
                res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
                i = n - (n % 8);
            }
            for (; i < n; ++i) res += a[i];
            lsum[lf] = res;
        }
        __syncthreads();
        if (lane == 0) {
            double stack[PROGRAM_STACK];
            int top = 0;
            for (int k = 0; k < nprog; ++k) {
                const int t = prog[k];
                if (t >= 0) {
                    stack[top++] = lsum[t];
                } else {
                    const double b = stack[--top];
                    stack[top - 1] = stack[top - 1] + b;
                }
            }
            double v = (0.0 + stack[0]) / div1;            // np.add.reduce starts from the identity 0.0
            if (scale) v = v * scale[c];
            out[c * out_stride] = v / div2;
        }
        __syncthreads();                                   // the next cell overwrites the LDS
    }
}

// thread <-> (group, column); the group's cells in ascending order (CSR from the host)
__global__ void __launch_bounds__(256) k_diag_group_sum(int ngroups, int k, const int *__restrict__ ptr,
                                                        const int *__restrict__ cells, const double *__restrict__ vals,
                                                        double *__restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)ngroups * k) return;
    const int g = (int)(i / k), col = (int)(i - (int64_t)g * k);
    double s = 0.0, comp = 0.0;
    int j = ptr[g];
    const int end = ptr[g + 1];
    // one dependent chain of adds in cell order; the loads run 16 ahead (a group may hold a large part of the grid)
    for (; j + 16 <= end; j += 16) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = vals[(int64_t)cells[j + u] * k + col];
#pragma unroll
        for (int u = 0; u < 16; ++u) kahan_add(s, comp, v[u]);
    }
    for (; j < end; ++j) kahan_add(s, comp, vals[(int64_t)cells[j] * k + col]);
    sums[i] = s;
}

}  // namespace

extern "C" int xh_diag_cell_total(xh_ctx *ctx, int64_t ncell, int32_t ncols, const double *d_in, double div1,
                                  const double *d_scale, double div2, double *d_out, int64_t out_stride) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, d_in && d_out && ncell >= 0 && ncols >= 1 && out_stride >= 1, "xh_diag_cell_total: bad argument");
    if (ncell == 0) return XH_OK;
    std::vector<int> leaves, prog;
    for (int off = 0; off < ncols; off += NP_BUFSIZE) {            // ((0 + block 0) + block 1) + ...
        pairwise_plan(off, ncols - off < NP_BUFSIZE ? ncols - off : NP_BUFSIZE, leaves, prog);
        if (off > 0) prog.push_back(-1);
    }
    const int nleaves = (int)(leaves.size() / 2);
    const size_t work = (size_t)9 * nleaves * sizeof(double);
    XH_REQUIRE(ctx, work <= STAGE_MAX_BYTES, "xh_diag_cell_total: %d values per cell need %d leaves, more than the LDS holds",
               ncols, nleaves);
    const bool stage = work + (size_t)ncols * sizeof(double) <= STAGE_MAX_BYTES;
    void *at[3];
    const int rc = xh_stage(ctx, 2, {{leaves.data(), leaves.size() * sizeof(int)}, {prog.data(), prog.size() * sizeof(int)}},
                            0, at);
    if (rc) return rc;
    const size_t lds = work + (stage ? (size_t)ncols * sizeof(double) : 0);
    return xh_launch(ctx, "diag_cell_total", ctx->stream, stage ? k_diag_cell_total<true> : k_diag_cell_total<false>,
                     xh_grid(ctx, ncell, 1, 32), TOTAL_THREADS, lds, ncell, (int)ncols, nleaves, static_cast<const int *>(at[0]),
                     (int)prog.size(), static_cast<const int *>(at[1]), d_in, div1, d_scale, div2, d_out, out_stride);
}

extern "C" int xh_diag_group_sum(xh_ctx *ctx, int64_t ncell, int32_t k, int32_t ngroups, const int32_t *h_group,
                                 const double *d_vals, double *d_sums, int64_t *d_counts) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, h_group && d_vals && d_sums && d_counts && ncell >= 0 && k >= 1 && ngroups >= 1,
               "xh_diag_group_sum: bad argument");
    XH_REQUIRE(ctx, ncell < ((int64_t)1 << 31), "xh_diag_group_sum: too many cells");
    std::vector<int> ptr(ngroups + 1, 0), cells;
    for (int64_t c = 0; c < ncell; ++c) {
        const int g = h_group[c];
        XH_REQUIRE(ctx, g >= -1 && g < ngroups, "xh_diag_group_sum: group %d of cell %lld out of range", g, (long long)c);
        if (g >= 0) ptr[g + 1]++;
    }
    std::vector<int64_t> counts(ngroups);
    for (int g = 0; g < ngroups; ++g) {
        counts[g] = ptr[g + 1];
        ptr[g + 1] += ptr[g];
    }
    cells.resize(ptr[ngroups]);
    {
        std::vector<int> fill(ptr.begin(), ptr.end() - 1);
        for (int64_t c = 0; c < ncell; ++c)
            if (h_group[c] >= 0) cells[fill[h_group[c]]++] = (int)c;
    }
    void *at[4];
    const int rc = xh_stage(ctx, 2,
                            {{ptr.data(), ptr.size() * sizeof(int)},
                             {cells.data(), cells.size() * sizeof(int)},
                             {counts.data(), counts.size() * sizeof(int64_t), d_counts}},
                            0, at);
    if (rc) return rc;
    return xh_launch(ctx, "diag_group_sum", ctx->stream, k_diag_group_sum, xh_grid(ctx, (int64_t)ngroups * k, 256), 256, 0,
                     (int)ngroups, (int)k, static_cast<const int *>(at[0]), static_cast<const int *>(at[1]), d_vals, d_sums);
}
