// Csv text on the device: the lines of data_writer/out_writer.py's csv branch (out_writer.py:187-194; the reference's
// df.to_csv(..., index_label='id')) formatted from an array in HBM, so that text and not doubles crosses PCIe.
//
// A line is str(first_id + r) + ',' + ','.join(fields) + '\n'; a field is repr(float) (xh_dtoa.h), NaN the empty field.
//
//   k_csv_rowlen  a wave per row, lanes over the columns in strips of 64: the length of every field (the digits are made
//                 and dropped), a wave sum, the row's length to off[r + 1]
//   k_csv_scan    one workgroup: off[] becomes the running sum, int64 -- a chunk of text stays below 4 GB, a file may not
//   k_csv_emit    a wave per row: the digits again (keeping them, 16 B per value, gains 5 % of the kernels' 1.4 ms per
//                 67,420 x 600 array and costs a buffer twice the array's size), a wave scan of the strip's field
//                 lengths, each lane writes its field into the row's image in LDS; the image leaves as aligned 16-byte
//                 stores, only the head and the tail of the row's span, which share their 16 bytes with the neighbouring
//                 rows, go byte by byte.  The image is placed in LDS at the row's offset modulo 16, so LDS and global
//                 blocks line up; it holds 8 KB, a longer row is flushed whenever the next strip might not fit and
//                 carries on.
//
// Two other layouts can be compiled in for an A/B (make expcsv; profiles/csv_writer has the figures): XH_CSV_TABLE_LDS copies
// the table into LDS per workgroup, XH_CSV_KEEP_DIGITS has k_csv_rowlen store each value's digits (16 B) for k_csv_emit to
// read back instead of making them again (one array at a time: not under xh_csv_write_many).
//
// No atomics; every byte is written once, by the wave of its row; two runs give the same bytes.  The power-of-ten table
// (10 KB, computed at first use, one upload per context) is read through L1 / L2: the index follows each value's binary
// exponent, real outputs span a few dozen entries.
#include <vector>

#include "xh_csv.h"
#include "xh_dtoa.h"

namespace {

constexpr int CSV_LB = 8192;                               // bytes of a row's image in LDS
constexpr int CSV_STRIP = 64 * (XH_DTOA_MAX_LEN + 1);      // the most a strip of 64 fields adds

#ifdef XH_CSV_TABLE_LDS
#define CSV_TABLE(pow10)                                                                   \
    __shared__ uint64_t lds_pow10[XH_DTOA_TABLE_WORDS];                                    \
    for (int i = threadIdx.x; i < XH_DTOA_TABLE_WORDS; i += blockDim.x) lds_pow10[i] = pow10[i]; \
    __syncthreads();                                                                       \
    const uint64_t *table = lds_pow10
#else
#define CSV_TABLE(pow10) const uint64_t *table = pow10
#endif

#ifdef XH_CSV_KEEP_DIGITS
struct CsvKept {
    uint64_t digits;
    int16_t ndig, e10;
    int8_t kind, neg;
    int16_t pad;
};
static_assert(sizeof(CsvKept) == 16, "one 16-byte record per value");
__device__ CsvKept *g_kept;      // [nrows * ncols] of the array measured last (xh_csv_measure)
__device__ __forceinline__ void keep_put(int64_t i, const xh_repr &r) {
    g_kept[i] = CsvKept{r.digits, (int16_t)r.ndig, (int16_t)r.e10, (int8_t)r.kind, (int8_t)r.neg, 0};
}
__device__ __forceinline__ xh_repr keep_get(int64_t i) {
    const CsvKept k = g_kept[i];
    xh_repr r;
    r.digits = k.digits;
    r.ndig = k.ndig;
    r.e10 = k.e10;
    r.kind = k.kind;
    r.neg = k.neg != 0;
    return r;
}
#endif

__global__ void __launch_bounds__(256) k_csv_rowlen(const uint64_t *__restrict__ pow10, const double *__restrict__ arr,
                                                    int64_t nrows, int64_t ncols, int64_t first_id, int64_t *__restrict__ off) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    CSV_TABLE(pow10);
    if (blockIdx.x == 0 && threadIdx.x == 0) off[0] = 0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < nrows; r += (int64_t)gridDim.x * 4) {
        const double *row = arr + r * ncols;
        int sum = 0;
        for (int64_t c = lane; c < ncols; c += 64) {
            const xh_repr rep = xh_dtoa_repr(row[c], table);
#ifdef XH_CSV_KEEP_DIGITS
            keep_put(r * ncols + c, rep);
#endif
            sum += xh_dtoa_len(rep);
        }
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
        if (lane == 0) off[r + 1] = (int64_t)xh_dtoa_id_len((uint64_t)(first_id + r)) + sum + ncols + 1;
    }
}

// in place: off[i] <- off[0] + ... + off[i], i <= n; thread t owns a run of consecutive entries
__global__ void __launch_bounds__(1024) k_csv_scan(int64_t *__restrict__ off, int64_t n) {
    __shared__ int64_t part[1024];
    const int t = threadIdx.x;
    const int64_t per = (n + 1 + 1023) / 1024;
    const int64_t lo = t * per, hi = lo + per < n + 1 ? lo + per : n + 1;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += off[i];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int64_t add = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int64_t run = part[t] - sum;
    for (int64_t i = lo; i < hi; ++i) {
        run += off[i];
        off[i] = run;
    }
}

__global__ void __launch_bounds__(64) k_csv_emit(const uint64_t *__restrict__ pow10, const double *__restrict__ arr, int64_t r0,
                                                 int64_t r1, int64_t ncols, int64_t first_id, const int64_t *__restrict__ off,
                                                 int64_t origin, char *__restrict__ text) {
    __shared__ __attribute__((aligned(16))) char buf[CSV_LB];
    const int lane = threadIdx.x;
    CSV_TABLE(pow10);
    for (int64_t r = r0 + blockIdx.x; r < r1; r += gridDim.x) {
        const int64_t row_begin = off[r] - origin, row_end = off[r + 1] - origin;
        int64_t gbase = row_begin & ~(int64_t)15;      // where buf[0] lies in the text: a multiple of 16
        int lo = (int)(row_begin - gbase);             // the image's first byte (non-zero only before the first flush)
        int pos = lo;                                  // its end
        // the image's bytes lo .. end to the text; all of them (last), or the whole 16-byte blocks, the rest moving to the front
        auto flush = [&](bool last) {
            __syncthreads();
            int end = last ? pos : (pos & ~15);
            if (gbase + end > row_end) end = (int)(row_end - gbase);      // never beyond the row's own span
            int a = (lo + 15) & ~15;
            if (a > end) a = end;                      // head lo .. a: shares its block with the row before
            int b = end & ~15;
            if (b < a) b = a;                          // body a .. b in whole blocks, tail b .. end
            char *g = text + gbase;
            if (lane < a - lo) g[lo + lane] = buf[lo + lane];
            for (int i = a + lane * 16; i < b; i += 64 * 16)
                *reinterpret_cast<uint4 *>(g + i) = *reinterpret_cast<const uint4 *>(buf + i);
            if (lane < end - b) g[b + lane] = buf[b + lane];
            if (!last) {
                const int rem = pos - end;
                char keep = 0;
                if (lane < rem) keep = buf[end + lane];
                __syncthreads();
                if (lane < rem) buf[lane] = keep;
                gbase += end;
                lo = 0;
                pos = rem;
            }
            __syncthreads();
        };
        const uint64_t id = (uint64_t)(first_id + r);
        if (lane == 0) buf[pos + xh_dtoa_id_put(id, buf + pos)] = ',';
        pos += xh_dtoa_id_len(id) + 1;
        const double *row = arr + r * ncols;
        for (int64_t c0 = 0; c0 < ncols; c0 += 64) {
            if (pos + CSV_STRIP > CSV_LB) flush(false);
            const int64_t c = c0 + lane;
            xh_repr rep;
            int len = 0;                               // the field and the ',' or '\n' behind it
            if (c < ncols) {
#ifdef XH_CSV_KEEP_DIGITS
                (void)row, (void)table;
                rep = keep_get(r * ncols + c);
#else
                rep = xh_dtoa_repr(row[c], table);
#endif
                len = xh_dtoa_len(rep) + 1;
            }
            int incl = len;
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d, 64);
                if (lane >= d) incl += up;
            }
            if (c < ncols) {
                char *p = buf + pos + (incl - len);
                p[xh_dtoa_put(rep, p)] = c == ncols - 1 ? '\n' : ',';
            }
            pos += __shfl(incl, 63, 64);
        }
        flush(true);
    }
}

}  // namespace

int xh_csv_table(xh_ctx *ctx) {
    if (ctx->csv_pow10) return XH_OK;
    void *d = nullptr;
    XH_HIP(ctx, hipMalloc(&d, XH_DTOA_TABLE_WORDS * sizeof(uint64_t)));
    const hipError_t e = hipMemcpy(d, xh_dtoa_host_table(), XH_DTOA_TABLE_WORDS * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return xh_fail(ctx, XH_ERR_HIP, "upload of the power-of-ten table: %s", hipGetErrorString(e));
    }
    ctx->csv_pow10 = d;
    return XH_OK;
}

int xh_csv_measure(xh_ctx *ctx, const double *d_arr, int64_t nrows, int64_t ncols, int64_t first_id, int64_t *d_off) {
    const int rc = xh_csv_table(ctx);
    if (rc) return rc;
#ifdef XH_CSV_KEEP_DIGITS      // (the A/B build only: one buffer, grown and never returned)
    static void *kept = nullptr;
    static size_t kept_bytes = 0;
    const size_t need = (size_t)(nrows * ncols) * 16;
    if (need > kept_bytes) {
        XH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (kept) XH_HIP(ctx, hipFree(kept));
        XH_HIP(ctx, hipMalloc(&kept, need));
        kept_bytes = need;
        XH_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(g_kept), &kept, sizeof(kept)));
    }
#endif
    return xh_timed(ctx, "csv_measure", ctx->stream, [&] {
        const int r = xh_launch(ctx, nullptr, ctx->stream, k_csv_rowlen, xh_grid(ctx, nrows > 0 ? nrows : 1, 4, 8), 256, 0,
                                static_cast<const uint64_t *>(ctx->csv_pow10), d_arr, nrows, ncols, first_id, d_off);
        if (r) return r;
        return xh_launch(ctx, nullptr, ctx->stream, k_csv_scan, 1, 1024, 0, d_off, nrows);
    });
}

hipError_t xh_csv_emit_on(hipStream_t stream, int cus, const uint64_t *d_pow10, const double *d_arr, int64_t r0, int64_t r1,
                          int64_t ncols, int64_t first_id, const int64_t *d_off, int64_t origin, char *d_text) {
    if (r1 <= r0) return hipSuccess;
    const int64_t cap = (int64_t)cus * 16;
    const unsigned grid = (unsigned)(r1 - r0 < cap ? r1 - r0 : cap);
    hipLaunchKernelGGL(k_csv_emit, grid, 64, 0, stream, d_pow10, d_arr, r0, r1, ncols, first_id, d_off, origin, d_text);
    return hipGetLastError();
}

extern "C" int xh_csv_format(xh_ctx *ctx, const double *d_arr, int64_t nrows, int64_t ncols, int64_t first_id, char *d_text,
                             size_t cap, int64_t *d_row_offsets) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, nrows >= 0 && ncols > 0 && ncols <= XH_CSV_MAX_COLS && first_id >= 0 && d_row_offsets && (d_arr || nrows == 0),
               "xh_csv_format: bad argument");
    XH_REQUIRE(ctx, (d_text || cap == 0) && xh_aligned16(d_text), "xh_csv_format: the text buffer must be 16-byte aligned");
    int rc = xh_csv_measure(ctx, d_arr, nrows, ncols, first_id, d_row_offsets);
    if (rc) return rc;
    int64_t total = 0;
    XH_HIP(ctx, hipMemcpyAsync(&total, d_row_offsets + nrows, sizeof(total), hipMemcpyDeviceToHost, ctx->stream));
    rc = xh_settle(ctx);
    if (rc) return rc;
    if ((uint64_t)total > cap)
        return xh_fail(ctx, XH_ERR_LIMIT, "xh_csv_format: the text takes %lld bytes, the buffer holds %zu", (long long)total, cap);
    return xh_timed(ctx, "csv_emit", ctx->stream, [&] {
        const hipError_t e = xh_csv_emit_on(ctx->stream, ctx->prop.multiProcessorCount, static_cast<const uint64_t *>(ctx->csv_pow10),
                                            d_arr, 0, nrows, ncols, first_id, d_row_offsets, 0, d_text);
        if (e != hipSuccess) return xh_fail(ctx, XH_ERR_HIP, "k_csv_emit: %s", hipGetErrorString(e));
        xh_note_work(ctx, ctx->stream);
        return (int)XH_OK;
    });
}
