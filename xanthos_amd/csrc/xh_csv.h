// The csv formatter's kernels as the file writer (xh_io.hip) drives them (internal; not part of the C-ABI).
#pragma once
#include "xh_launch.h"

constexpr int64_t XH_CSV_MAX_COLS = (int64_t)1 << 24;      // a row's length stays below 2^31

// The digit generator's power-of-ten table in HBM (ctx->csv_pow10), computed and uploaded on the context's first call.
int xh_csv_table(xh_ctx *ctx);
// d_off[0 .. nrows] = where each line of the text of d_arr [nrows, ncols] starts, and the length of the whole; on the
// context's stream, span "csv_measure".
int xh_csv_measure(xh_ctx *ctx, const double *d_arr, int64_t nrows, int64_t ncols, int64_t first_id, int64_t *d_off);
// The lines of rows r0 .. r1 - 1 to d_text (16-byte aligned) + d_off[r] - origin, on `stream`.  Touches nothing of a
// context: the writer threads of xh_csv_write call it side by side.
hipError_t xh_csv_emit_on(hipStream_t stream, int cus, const uint64_t *d_pow10, const double *d_arr, int64_t r0, int64_t r1,
                          int64_t ncols, int64_t first_id, const int64_t *d_off, int64_t origin, char *d_text);
