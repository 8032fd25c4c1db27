// File <-> HBM movers of the loader / writer either side of the hot path.
//
// The reference loads every forcing array with np.load and keeps it on the host (data_load.py:186-195, :342-350); at the
// full grid that is 8 x 324 MB which then has to cross PCIe.  Measured on the MI355X box (tools/io_experiment.py, 4 x 324 MB
// from the page cache): read() into a host array + copy 8 GB/s; threads pread()-ing into page-locked slots + asynchronous
// copies 5-8 GB/s (the page-cache copy is the bottleneck, whatever the number of threads); a copy straight out of a
// read-only MAPPING of the file 34 GB/s (the runtime pins the page-cache pages and the DMA engines read them in place).
// So xh_upload_file maps the byte range and hands the mapping to hipMemcpy -- no host copy of the data at all.
// The other direction is the opposite: a copy into a shared mapping of a fresh file runs at 2.8 GB/s (a page fault per
// 4 KB), device -> pageable array -> write() at 6 GB/s, and xh_download_file(s) -- one thread per file, device -> page-locked
// slot i + 1 under the write() of slot i -- at 15 GB/s.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <cstring>
#include <thread>
#include <utility>
#include <vector>

#include "xh_csv.h"

namespace {

constexpr size_t IO_CHUNK = 8u << 20;
constexpr int IO_SLOTS = 2;            // per writer thread
constexpr int IO_MAX_FILES = 16;

int io_ring(xh_ctx *ctx, int writers) {
    const size_t need = (size_t)writers * IO_SLOTS * IO_CHUNK;
    if (ctx->io_ring_bytes >= need) return XH_OK;
    if (ctx->io_ring) XH_HIP(ctx, hipHostFree(ctx->io_ring));
    ctx->io_ring = nullptr;
    ctx->io_ring_bytes = 0;
    XH_HIP(ctx, hipHostMalloc(&ctx->io_ring, need, hipHostMallocDefault));
    ctx->io_ring_bytes = need;
    return XH_OK;
}

struct IoJob {
    const char *dev;
    const char *path;
    uint64_t offset;
    size_t bytes;
};

// One writer: the chunks of one device array, in order, into one file.  The copy of chunk i + 1 into the other slot is in
// flight while chunk i is written.
void io_writer(int device, int fd, IoJob job, char *slots, std::atomic<int> *err) {
    hipStream_t st = nullptr;
    hipEvent_t ev[IO_SLOTS] = {};
    size_t pend_off[IO_SLOTS] = {}, pend_len[IO_SLOTS] = {};
    bool used[IO_SLOTS] = {};
    auto fail = [&](int code) {
        int z = 0;
        err->compare_exchange_strong(z, code);
    };
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
        fail(-1);
        return;
    }
    for (int s = 0; s < IO_SLOTS; ++s)
        if (hipEventCreateWithFlags(&ev[s], hipEventDisableTiming) != hipSuccess) fail(-1);
    auto drain = [&](int s) {      // the slot's chunk is written out once its copy has landed
        if (!used[s]) return;
        if (hipEventSynchronize(ev[s]) != hipSuccess) fail(-1);
        size_t done = 0;
        while (done < pend_len[s] && err->load() == 0) {
            const ssize_t w = pwrite(fd, slots + (size_t)s * IO_CHUNK + done, pend_len[s] - done,
                                     (off_t)(job.offset + pend_off[s] + done));
            if (w < 0 && errno == EINTR) continue;
            if (w <= 0) {
                fail(errno ? errno : EIO);
                break;
            }
            done += (size_t)w;
        }
        used[s] = false;
    };
    int s = 0;
    for (size_t off = 0; off < job.bytes && err->load() == 0; off += IO_CHUNK) {
        const size_t len = job.bytes - off < IO_CHUNK ? job.bytes - off : IO_CHUNK;
        drain(s);
        if (hipMemcpyAsync(slots + (size_t)s * IO_CHUNK, job.dev + off, len, hipMemcpyDeviceToHost, st) != hipSuccess) fail(-1);
        if (hipEventRecord(ev[s], st) != hipSuccess) fail(-1);
        used[s] = true;
        pend_off[s] = off;
        pend_len[s] = len;
        s = (s + 1) % IO_SLOTS;
    }
    for (int k = 0; k < IO_SLOTS; ++k) drain((s + k) % IO_SLOTS);
    if (hipStreamSynchronize(st) != hipSuccess) fail(-1);
    for (int k = 0; k < IO_SLOTS; ++k)
        if (ev[k]) (void)hipEventDestroy(ev[k]);
    (void)hipStreamDestroy(st);
}

// One writer thread per job (file): buffered writes to one file are serialised by the file system (one inode lock), so
// a second writer on the same file only adds contention; different files do run side by side.
int io_download(xh_ctx *ctx, const IoJob *jobs, int njobs) {
    if (!ctx || njobs < 0 || (njobs && !jobs)) return XH_ERR_ARG;
    for (int j = 0; j < njobs; ++j)
        if (!jobs[j].path || (jobs[j].bytes && !jobs[j].dev)) return XH_ERR_ARG;
    if (njobs > IO_MAX_FILES) return xh_fail(ctx, XH_ERR_LIMIT, "at most %d files per call", IO_MAX_FILES);
    const int rc = xh_settle(ctx);      // earlier work may still write the sources; a routing call that must be re-run is re-run here
    if (rc != XH_OK && rc != XH_ERR_DEVICE) return rc;
    xh_note_work(ctx, ctx->stream);
    if (njobs == 0) return rc;
    int fds[IO_MAX_FILES];
    auto close_all = [&](int upto) {
        int bad = 0;
        for (int j = 0; j < upto; ++j)
            if (close(fds[j]) != 0) bad = errno ? errno : EIO;
        return bad;
    };
    for (int j = 0; j < njobs; ++j) {
        fds[j] = open(jobs[j].path, O_WRONLY | O_CREAT, 0644);
        if (fds[j] < 0) {
            const int e = errno;
            close_all(j);
            return xh_fail(ctx, XH_ERR_ARG, "%s: %s", jobs[j].path, strerror(e));
        }
    }
    const int rr = io_ring(ctx, njobs);
    if (rr != XH_OK) {
        close_all(njobs);
        return rr;
    }
    std::atomic<int> err{0};
    std::thread pool[IO_MAX_FILES];
    for (int t = 0; t < njobs; ++t)
        pool[t] = std::thread(io_writer, ctx->device, fds[t], jobs[t], (char *)ctx->io_ring + (size_t)t * IO_SLOTS * IO_CHUNK, &err);
    for (int t = 0; t < njobs; ++t) pool[t].join();
    const int cerr = close_all(njobs);
    if (cerr && err.load() == 0) err.store(cerr);
    if (err.load() > 0) return xh_fail(ctx, XH_ERR_ARG, "%s: %s", jobs[0].path, strerror(err.load()));
    if (err.load() < 0) return xh_fail(ctx, XH_ERR_HIP, "%s: a copy of the file transfer failed", jobs[0].path);
    return rc;
}

// ---- csv: the same slots and file code, the text formatted on the device (xh_csv.hip) chunk by chunk
struct CsvJob {
    const double *arr;
    int64_t nrows, ncols, first_id;
    const char *path;
    uint64_t offset;
    int64_t *d_off;                       // [nrows + 1] row offsets in HBM
    char *d_slots;                        // IO_SLOTS text slots of IO_CHUNK bytes in HBM
    std::vector<int64_t> off;             // the row offsets on the host
    std::vector<std::pair<hipEvent_t, hipEvent_t>> spans;      // around the format kernels, for the context's timer
};

// One writer: chunks of whole rows, at most `chunk` bytes of text each (one row when a row alone is longer).  Chunk k + 1 is
// formatted into its HBM slot while chunk k crosses PCIe into its page-locked slot and chunk k - 1 is in pwrite().
void csv_writer(int device, int cus, const uint64_t *d_pow10, bool timing, int fd, CsvJob *job, int64_t chunk, char *slots,
                std::atomic<int> *err) {
    hipStream_t sf = nullptr, sc = nullptr;          // format kernels / copies
    hipEvent_t formatted[IO_SLOTS] = {}, copied[IO_SLOTS] = {};
    int64_t pend_off[IO_SLOTS] = {}, pend_len[IO_SLOTS] = {};
    bool used[IO_SLOTS] = {};
    auto fail = [&](int code) {
        int z = 0;
        err->compare_exchange_strong(z, code);
    };
    auto hip = [&](hipError_t e) {
        if (e != hipSuccess) fail(-1);
        return e == hipSuccess;
    };
    if (!hip(hipSetDevice(device)) || !hip(hipStreamCreateWithFlags(&sf, hipStreamNonBlocking)) ||
        !hip(hipStreamCreateWithFlags(&sc, hipStreamNonBlocking))) {
        if (sf) (void)hipStreamDestroy(sf);
        return;
    }
    for (int s = 0; s < IO_SLOTS; ++s) {
        hip(hipEventCreateWithFlags(&formatted[s], hipEventDisableTiming));
        hip(hipEventCreateWithFlags(&copied[s], hipEventDisableTiming));
    }
    auto landed = [&](int s) {       // the slot's copy has ended: its HBM slot is free again
        if (used[s]) hip(hipEventSynchronize(copied[s]));
    };
    auto drain = [&](int s) {        // ... and its text is written out
        if (!used[s]) return;
        size_t done = 0;
        while (done < (size_t)pend_len[s] && err->load() == 0) {
            const ssize_t w = pwrite(fd, slots + (size_t)s * IO_CHUNK + done, (size_t)pend_len[s] - done,
                                     (off_t)(job->offset + (uint64_t)pend_off[s] + done));
            if (w < 0 && errno == EINTR) continue;
            if (w <= 0) {
                fail(errno ? errno : EIO);
                break;
            }
            done += (size_t)w;
        }
        used[s] = false;
    };
    const std::vector<int64_t> &off = job->off;
    int s = 0;
    for (int64_t r0 = 0; r0 < job->nrows && err->load() == 0; s = (s + 1) % IO_SLOTS) {
        int64_t r1 = r0 + 1;
        while (r1 < job->nrows && off[r1 + 1] - off[r0] <= chunk) ++r1;
        const int64_t len = off[r1] - off[r0];
        char *d_slot = job->d_slots + (size_t)s * IO_CHUNK;
        landed(s);
        hipEvent_t a = nullptr, b = nullptr;
        if (timing && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess) hip(hipEventRecord(a, sf));
        hip(xh_csv_emit_on(sf, cus, d_pow10, job->arr, r0, r1, job->ncols, job->first_id, job->d_off, off[r0], d_slot));
        if (a && b) {
            hip(hipEventRecord(b, sf));
            job->spans.emplace_back(a, b);
        } else if (a) {
            (void)hipEventDestroy(a);
        }
        hip(hipEventRecord(formatted[s], sf));
        drain(s);
        hip(hipStreamWaitEvent(sc, formatted[s], 0));
        hip(hipMemcpyAsync(slots + (size_t)s * IO_CHUNK, d_slot, (size_t)len, hipMemcpyDeviceToHost, sc));
        hip(hipEventRecord(copied[s], sc));
        used[s] = true;
        pend_off[s] = off[r0];
        pend_len[s] = len;
        r0 = r1;
    }
    for (int k = 0; k < IO_SLOTS; ++k) {
        landed((s + k) % IO_SLOTS);
        drain((s + k) % IO_SLOTS);
    }
    hip(hipStreamSynchronize(sf));
    hip(hipStreamSynchronize(sc));
    for (int k = 0; k < IO_SLOTS; ++k) {
        if (formatted[k]) (void)hipEventDestroy(formatted[k]);
        if (copied[k]) (void)hipEventDestroy(copied[k]);
    }
    (void)hipStreamDestroy(sf);
    (void)hipStreamDestroy(sc);
}

int csv_download(xh_ctx *ctx, CsvJob *jobs, int njobs, size_t chunk_bytes, uint64_t *bytes_written) {
    if (!ctx || njobs < 0 || (njobs && !jobs)) return XH_ERR_ARG;
    if (njobs > IO_MAX_FILES) return xh_fail(ctx, XH_ERR_LIMIT, "at most %d files per call", IO_MAX_FILES);
    for (int j = 0; j < njobs; ++j) {
        const CsvJob &q = jobs[j];
        XH_REQUIRE(ctx, q.path && q.nrows >= 0 && q.ncols > 0 && q.ncols <= XH_CSV_MAX_COLS && q.first_id >= 0 &&
                            (q.arr || q.nrows == 0), "xh_csv_write: bad argument");
        if (bytes_written) bytes_written[j] = 0;
    }
    const int64_t chunk = (int64_t)(chunk_bytes == 0 || chunk_bytes > IO_CHUNK ? IO_CHUNK : chunk_bytes);
    int rc = xh_settle(ctx);            // earlier work may still write the sources
    if (rc != XH_OK && rc != XH_ERR_DEVICE) return rc;
    const int rc_settle = rc;
    if (njobs == 0) return rc_settle;
    int fds[IO_MAX_FILES];
    auto close_all = [&](int upto) {
        int bad = 0;
        for (int j = 0; j < upto; ++j)
            if (close(fds[j]) != 0) bad = errno ? errno : EIO;
        return bad;
    };
    for (int j = 0; j < njobs; ++j) {
        fds[j] = open(jobs[j].path, O_WRONLY | O_CREAT, 0644);
        if (fds[j] < 0) {
            const int e = errno;
            close_all(j);
            return xh_fail(ctx, XH_ERR_ARG, "%s: %s", jobs[j].path, strerror(e));
        }
    }
    auto bail = [&](int code) {
        close_all(njobs);
        return code;
    };
    // HBM: per file its row offsets and its text slots
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    size_t need = 0;
    for (int j = 0; j < njobs; ++j) need += pad((size_t)(jobs[j].nrows + 1) * sizeof(int64_t)) + (size_t)IO_SLOTS * IO_CHUNK;
    if (ctx->csv_dev_bytes < need) {
        if (ctx->csv_dev && hipFree(ctx->csv_dev) != hipSuccess) return bail(xh_fail(ctx, XH_ERR_HIP, "hipFree of the csv slots failed"));
        ctx->csv_dev = nullptr;
        ctx->csv_dev_bytes = 0;
        if (hipMalloc(&ctx->csv_dev, need) != hipSuccess) {
            ctx->csv_dev = nullptr;
            return bail(xh_fail(ctx, XH_ERR_HIP, "no %zu bytes of device memory for the csv slots", need));
        }
        ctx->csv_dev_bytes = need;
    }
    if ((rc = io_ring(ctx, njobs)) != XH_OK) return bail(rc);
    char *at = static_cast<char *>(ctx->csv_dev);
    for (int j = 0; j < njobs; ++j) {
        CsvJob &q = jobs[j];
        q.d_off = reinterpret_cast<int64_t *>(at);
        at += pad((size_t)(q.nrows + 1) * sizeof(int64_t));
        q.d_slots = at;
        at += (size_t)IO_SLOTS * IO_CHUNK;
        if ((rc = xh_csv_measure(ctx, q.arr, q.nrows, q.ncols, q.first_id, q.d_off)) != XH_OK) return bail(rc);
        q.off.resize((size_t)q.nrows + 1);
        if (hipMemcpyAsync(q.off.data(), q.d_off, q.off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            return bail(xh_fail(ctx, XH_ERR_HIP, "download of the row offsets failed"));
    }
    if ((rc = xh_settle(ctx)) != XH_OK) return bail(rc);
    for (int j = 0; j < njobs; ++j)
        for (int64_t r = 0; r < jobs[j].nrows; ++r)
            if (jobs[j].off[r + 1] - jobs[j].off[r] > (int64_t)IO_CHUNK)
                return bail(xh_fail(ctx, XH_ERR_LIMIT, "%s: line %lld is longer than a transfer slot (%zu bytes)", jobs[j].path,
                                    (long long)r, IO_CHUNK));
    std::atomic<int> err{0};
    std::thread pool[IO_MAX_FILES];
    for (int t = 0; t < njobs; ++t)
        pool[t] = std::thread(csv_writer, ctx->device, ctx->prop.multiProcessorCount, static_cast<const uint64_t *>(ctx->csv_pow10),
                              ctx->timing, fds[t], &jobs[t], chunk, (char *)ctx->io_ring + (size_t)t * IO_SLOTS * IO_CHUNK, &err);
    for (int t = 0; t < njobs; ++t) pool[t].join();
    xh_note_work(ctx, ctx->stream);
    for (int j = 0; j < njobs; ++j) {      // the writers' kernel times join the context's timer
        xh_timer_slot &slot = ctx->timers["csv_emit"];
        for (auto &p : jobs[j].spans) slot.pending.push_back(p);
        jobs[j].spans.clear();
        if (bytes_written) bytes_written[j] = (uint64_t)jobs[j].off[jobs[j].nrows];
    }
    const int cerr = close_all(njobs);
    if (cerr && err.load() == 0) err.store(cerr);
    if (err.load() > 0) return xh_fail(ctx, XH_ERR_ARG, "%s: %s", jobs[0].path, strerror(err.load()));
    if (err.load() < 0) return xh_fail(ctx, XH_ERR_HIP, "%s: a kernel or a copy of the csv transfer failed", jobs[0].path);
    return rc_settle;
}

}  // namespace

extern "C" {

int xh_csv_write(xh_ctx *ctx, const double *d_arr, int64_t nrows, int64_t ncols, int64_t first_id, const char *path,
                 uint64_t offset, size_t chunk_bytes, uint64_t *bytes_written) {
    CsvJob job{d_arr, nrows, ncols, first_id, path, offset, nullptr, nullptr, {}, {}};
    return csv_download(ctx, &job, 1, chunk_bytes, bytes_written);
}

int xh_csv_write_many(xh_ctx *ctx, int n, const double *const *d_arrs, const int64_t *nrows, const int64_t *ncols,
                      const int64_t *first_ids, const char *const *paths, const uint64_t *offsets, size_t chunk_bytes,
                      uint64_t *bytes_written) {
    if (n < 0 || n > IO_MAX_FILES || (n && (!d_arrs || !nrows || !ncols || !first_ids || !paths || !offsets))) return XH_ERR_ARG;
    std::vector<CsvJob> jobs;
    for (int j = 0; j < n; ++j) jobs.push_back(CsvJob{d_arrs[j], nrows[j], ncols[j], first_ids[j], paths[j], offsets[j], nullptr, nullptr, {}, {}});
    return csv_download(ctx, jobs.data(), n, chunk_bytes, bytes_written);
}

int xh_upload_file(xh_ctx *ctx, void *d_dst, const char *path, uint64_t offset, size_t bytes, int threads) {
    (void)threads;                                   // kept in the signature: the mapped copy needs no host threads
    if (!ctx || !path || (bytes && !d_dst)) return XH_ERR_ARG;
    const int rc = xh_settle(ctx);                   // earlier work may still read the destination; re-routes happen here
    if (rc != XH_OK && rc != XH_ERR_DEVICE) return rc;
    xh_note_work(ctx, ctx->stream);
    if (bytes == 0) return rc;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return xh_fail(ctx, XH_ERR_ARG, "%s: %s", path, strerror(errno));
    struct stat sb;
    if (fstat(fd, &sb) != 0 || (uint64_t)sb.st_size < offset + bytes) {
        close(fd);
        return xh_fail(ctx, XH_ERR_ARG, "%s: shorter than offset %llu + %zu bytes", path, (unsigned long long)offset, bytes);
    }
    const uint64_t page = (uint64_t)sysconf(_SC_PAGESIZE);
    const uint64_t start = offset - offset % page;
    const size_t span = (size_t)(offset - start) + bytes;
    void *map = mmap(nullptr, span, PROT_READ, MAP_SHARED, fd, (off_t)start);   // shared, like numpy.memmap(mode="r")
    close(fd);                                       // the mapping keeps the file
    if (map == MAP_FAILED) return xh_fail(ctx, XH_ERR_ARG, "%s: mmap: %s", path, strerror(errno));
    (void)madvise(map, span, MADV_SEQUENTIAL);
    hipError_t e = hipMemcpyAsync(d_dst, (const char *)map + (offset - start), bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // the mapping goes away below
    munmap(map, span);
    if (e != hipSuccess) return xh_fail(ctx, XH_ERR_HIP, "%s: copy from the mapped file: %s", path, hipGetErrorString(e));
    return rc;
}

int xh_download_file(xh_ctx *ctx, const void *d_src, const char *path, uint64_t offset, size_t bytes, int threads) {
    (void)threads;                                   // one writer per file
    const IoJob job{(const char *)d_src, path, offset, bytes};
    return io_download(ctx, &job, 1);
}

int xh_download_files(xh_ctx *ctx, int n, const void *const *d_srcs, const char *const *paths, const uint64_t *offsets,
                      const size_t *bytes) {
    if (n < 0 || n > IO_MAX_FILES || (n && (!d_srcs || !paths || !offsets || !bytes))) return XH_ERR_ARG;
    IoJob jobs[IO_MAX_FILES];
    for (int j = 0; j < n; ++j) jobs[j] = IoJob{(const char *)d_srcs[j], paths[j], offsets[j], bytes[j]};
    return io_download(ctx, jobs, n);
}

}  // extern "C"
