// Host side of the stage entry points: kernel launches, grid sizes and host-table uploads (internal; not part of the C-ABI).
//
// Every entry point that enqueues work on a stream of the context says so through xh_note_work: xh_fault_check uses the
// count to tell a caller that work enqueued after a faulted routing call read its invalid outputs, and
// xh_comm_gather_rows_side to see whether a fed call's "runoff is final" event is still the thing to wait for.  xh_launch
// notes every kernel it launches, so an entry point built on it cannot forget.
#pragma once
#include <initializer_list>

#include "xh_common.h"

// Work was enqueued on `stream` (the context's stream or a side stream): bumps ctx->work_seq and, on the context's own
// stream, makes a fed call's "runoff is final" event stale.  The one writer of work_seq (xh_ctx.hip).
void xh_note_work(xh_ctx *ctx, hipStream_t stream);

// Workgroups for n items of `threads` each; at most per_cu workgroups per CU when per_cu > 0 (grid-stride kernels).
static inline unsigned xh_grid(const xh_ctx *ctx, int64_t n, int threads, int per_cu = 0) {
    int64_t blocks = (n + threads - 1) / threads;
    const int64_t cap = (int64_t)ctx->prop.multiProcessorCount * per_cu;
    if (per_cu > 0 && blocks > cap) blocks = cap;
    return (unsigned)blocks;
}

// Span `name` on `stream` around `launches` (a callable returning XH_OK or an error code), for the spans that time more
// than one kernel: the kernels inside go through xh_launch untimed.
template <typename F>
int xh_timed(xh_ctx *ctx, const char *name, hipStream_t stream, F &&launches) {
    xh_span sp = xh_span_begin_on(ctx, name, stream);
    const int rc = launches();
    xh_span_end(sp);
    return rc;
}

// Kernel `k` on `stream` under span `name` (nullptr: untimed), its launch error checked, the work noted.  (A span notes
// work too; the readers of work_seq only ask whether it moved.)
template <typename... P, typename... A>
int xh_launch(xh_ctx *ctx, const char *name, hipStream_t stream, void (*k)(P...), dim3 grid, dim3 block, size_t lds,
              A... args) {
    if (name) return xh_timed(ctx, name, stream, [&] { return xh_launch(ctx, nullptr, stream, k, grid, block, lds, args...); });
    hipLaunchKernelGGL(k, grid, block, lds, stream, args...);
    XH_HIP(ctx, hipGetLastError());
    xh_note_work(ctx, stream);
    return XH_OK;
}

// One host array of an upload: `bytes` bytes at `src`, placed in the scratch slot, or copied to `dst` (a device array of
// the caller's) when that is given.
struct xh_host_array {
    const void *src;
    size_t bytes;
    void *dst = nullptr;
};

// NULL or 16-byte aligned (kernels that move rows as double2)
static inline bool xh_aligned16(const void *p) { return p == nullptr || ((uintptr_t)p & 15) == 0; }

// The host tables of one call in scratch slot `slot` (one xh_scratch call): the arrays one after another, each on a 256-byte
// boundary, then `tail_bytes` of uninitialised device memory.  at[i] receives the device address of array i, at[n] that of
// the tail.  Copies on the context's stream, then one synchronisation: the host arrays may go away on return.  (Not noted
// as work: the copies read nothing a routing call produces.)
int xh_stage(xh_ctx *ctx, int slot, std::initializer_list<xh_host_array> arrays, size_t tail_bytes, void **at);
