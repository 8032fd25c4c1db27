/*
 * xanthos_hip.h -- C-ABI of libxanthos_hip.so: the MI355X (gfx950) implementation of the Xanthos monthly
 * PET -> runoff -> routing hot path.
 *
 * The reference (JGCRI/xanthos v2.4.1) is pure Python/numpy and has no FFI of its own; its "plugin API" for this
 * path is a set of module-level Python functions that xanthos/components.py calls.  Each entry point below states
 * the reference function (file:line under /root/reference) whose work it replaces.  The Python stubs that bind
 * these symbols with ctypes are in xanthos_amd/_hip.py; INTEGRATION.md shows the lines a Xanthos maintainer would
 * add to pet/penman_monteith.py, runoff/abcd.py and routing/mrtm.py.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, fp64 only.  All 2-D arrays are [ncell, nmonths], C order (month
 *     fastest) -- exactly the reference's in-memory layout, so uploads/downloads are plain copies.
 *   - Pointers named d_* are DEVICE pointers (from xh_malloc, or any HIP allocation on the context's device);
 *     pointers named h_* are HOST pointers (small index/table arrays read during the call).
 *   - Every function returns XH_OK (0) or an error code; xh_last_error(ctx) gives the message.
 *   - Kernels are enqueued on the context's own HIP stream and the call returns without waiting; xh_sync,
 *     xh_memcpy_d2h and xh_timing_get wait for the stream.  Calls on one context must not be concurrent
 *     (one context per host thread); different contexts are independent.
 *   - A call never falls back to the CPU: if the device or the code object is unusable it fails.
 */
#ifndef XANTHOS_HIP_H
#define XANTHOS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XH_OK 0
#define XH_ERR_ARG 1     /* bad argument (NULL, size, unsupported value)          */
#define XH_ERR_HIP 2     /* a HIP runtime call or kernel failed                   */
#define XH_ERR_LIMIT 3   /* problem exceeds a compiled-in limit (e.g. land classes) */
#define XH_ERR_DEVICE 4  /* routing kernel reported a device-side fault (spin timeout) */

#define XH_MAX_LCS 32    /* max land-cover classes in xh_pm_pet */

typedef struct xh_ctx xh_ctx;
typedef struct xh_route_plan xh_route_plan;

/* ------------------------------------------------------------------ context, memory, timing */
int xh_abi_version(void);                                  /* bumps when a signature changes */
int xh_device_count(int *n);
int xh_ctx_create(int device, xh_ctx **out);
void xh_ctx_destroy(xh_ctx *ctx);
const char *xh_last_error(const xh_ctx *ctx);              /* ctx may be NULL: last error of a failed xh_ctx_create */
int xh_device_name(xh_ctx *ctx, char *buf, size_t len);

int xh_malloc(xh_ctx *ctx, size_t bytes, void **d_ptr);
int xh_free(xh_ctx *ctx, void *d_ptr);
int xh_mem_info(xh_ctx *ctx, size_t *free_bytes, size_t *total_bytes);         /* hipMemGetInfo of the context's device */
int xh_memcpy_h2d(xh_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int xh_memcpy_d2h(xh_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);   /* waits for the stream */
int xh_memcpy_d2d(xh_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);
/* Page-locked host memory and transfers that do not wait: a loader / writer that keeps its arrays in xh_host_alloc
 * memory moves them at PCIe rate and overlaps them with kernels; the buffers must stay untouched until xh_sync. */
int xh_host_alloc(xh_ctx *ctx, size_t bytes, void **h_ptr);
int xh_host_free(xh_ctx *ctx, void *h_ptr);
int xh_memcpy_h2d_async(xh_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int xh_memcpy_d2h_async(xh_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
/* File <-> HBM without a host copy of the data: `bytes` of `path` from byte `offset` (the body of a .npy: the loader of
 * data_load.py:186-195, :342-350 keeps np.load's memory map instead of a 324 MB host array) are mapped read-only and
 * copied out of the mapping (34 GB/s from the page cache on the MI355X box against 8 GB/s for read() + copy; `threads`
 * is ignored).  xh_download_file is the writer's side (data_writer/out_writer.py np.save: the caller writes the header,
 * this call the body; the file is created when missing, never truncated): device -> page-locked slots -> write(), the
 * copy of one chunk under the write of the one before (15 GB/s against 6 GB/s for a download + np.save).  Both wait for
 * earlier work of the context and return when the transfer is complete.  XH_ERR_ARG: file missing / too short / write
 * error (xh_last_error has errno's text). */
int xh_upload_file(xh_ctx *ctx, void *d_dst, const char *path, uint64_t offset, size_t bytes, int threads);
int xh_download_file(xh_ctx *ctx, const void *d_src, const char *path, uint64_t offset, size_t bytes, int threads);
/* Several device arrays to several files at once (n <= 16), one writer thread per file: the output variables of one run. */
int xh_download_files(xh_ctx *ctx, int n, const void *const *d_srcs, const char *const *paths, const uint64_t *offsets,
                      const size_t *bytes);
/* Csv text from HBM: the csv branch of data_writer/out_writer.py (out_writer.py:187-194, the reference's
 * df.to_csv(..., index_label='id')) without the doubles crossing PCIe.  d_arr is [nrows, ncols] row-major; a line is
 * str(first_id + r) + ',' + ','.join(fields) + '\n', a field Python's repr(float) -- the shortest digits that read back as
 * the same double, fixed notation for decimal exponents -4 .. 15, d[.ddd]e+XX otherwise -- and NaN the empty field, byte
 * for byte what the host loop writes.  first_id >= 0.
 * xh_csv_format replaces the formatting loop alone: the text into d_text (16-byte aligned, `cap` bytes; XH_ERR_LIMIT and
 * nothing written when the text is longer), the offset of every line and the total length into d_row_offsets[nrows + 1].
 * It waits for the lengths; the text is enqueued on the context's stream. */
int xh_csv_format(xh_ctx *ctx, const double *d_arr, int64_t nrows, int64_t ncols, int64_t first_id, char *d_text, size_t cap,
                  int64_t *d_row_offsets);
/* xh_csv_write replaces the loop and its fh.write (out_writer.py:189-194): the text goes to `path` from byte `offset` on
 * (the caller has written the header line; the file is created when missing, never truncated, as with xh_download_file),
 * in chunks of whole lines of at most chunk_bytes of text (0: the transfer slot's size, which also is the most; a longer
 * line goes alone) -- chunk k + 1 is formatted while chunk k crosses PCIe into the page-locked slots of
 * xh_download_file and chunk k - 1 is in write().  *bytes_written (may be NULL) receives the length of the text.  Waits
 * for earlier work of the context, returns when the file is complete.  XH_ERR_ARG on file errors (xh_last_error has
 * errno's text), XH_ERR_LIMIT for a line longer than a transfer slot. */
int xh_csv_write(xh_ctx *ctx, const double *d_arr, int64_t nrows, int64_t ncols, int64_t first_id, const char *path,
                 uint64_t offset, size_t chunk_bytes, uint64_t *bytes_written);
/* Several arrays to several files at once (n <= 16), one writer thread per file as in xh_download_files: the variables of
 * one OutWriter.write() (out_writer.py:81-125 calls write_data, :187-194, once per variable). */
int xh_csv_write_many(xh_ctx *ctx, int n, const double *const *d_arrs, const int64_t *nrows, const int64_t *ncols,
                      const int64_t *first_ids, const char *const *paths, const uint64_t *offsets, size_t chunk_bytes,
                      uint64_t *bytes_written);
/* The body of a NetCDF-classic 'f4' variable from HBM: the reference's save_netcdf (out_writer.py:196-223) assigns the
 * float64 array to an 'f4' variable, which scipy writes as numpy's a.astype('>f4').tobytes().  d_dst receives n IEEE
 * binary32 values, most significant byte first, each d_src[i] rounded to nearest even: overflow gives +/-inf, binary32
 * subnormals are kept, zero keeps its sign, the NaN 0x7ff8000000000000 becomes 0x7fc00000.  d_src 8-byte, d_dst 16-byte
 * aligned (XH_ERR_ARG otherwise); enqueued on the context's stream, timer "pack_f32_be".  The caller writes the header
 * and sends the 4 n bytes out with xh_download_files.  (MATLAB's column-major body is xh_transpose.) */
int xh_pack_f32_be(xh_ctx *ctx, const double *d_src, int64_t n, void *d_dst);
/* The body of a gridded 'f4' variable [time, lat, lon] from HBM (data_writer/gridded.py, GriddedOutput = 1).  The reference
 * has no gridded output: this replaces the host-side scatter a user writes behind it -- download the [ncell, ncols] array,
 * fancy-index it into a [ncols, nslots] cube of fill values, narrow and swap.  d_src is the array as written, [ncell, ncols]
 * row-major; d_cell_of_slot [nslots], nslots = ngridrow * ngridcol in row-major grid order, holds the 0-based cell lying
 * in each slot or -1 for none (trusted: the host validates it, GridMap); d_dst receives [ncols, nslots] IEEE binary32
 * values, most significant byte first: with c = cell_of_slot[s], dst[t * nslots + s] is fill_bits when c < 0 or
 * src[c * ncols + t] is NaN, otherwise the value narrowed exactly as by xh_pack_f32_be (nearest even, overflow to +/-inf,
 * binary32 subnormals and the sign of zero kept).  Nothing is uploaded; enqueued on the context's stream, timer
 * "grid_pack"; offsets are 64-bit.  XH_ERR_ARG: a NULL array, ncell < 1, nslots < 1, ncols < 0, d_src not 8-byte or d_dst
 * not 16-byte aligned.  ncols == 0 is XH_OK and launches nothing. */
int xh_grid_pack_f32_be(xh_ctx *ctx, const double *d_src, int64_t ncell, int64_t ncols, const int32_t *d_cell_of_slot,
                        int64_t nslots, uint32_t fill_bits, void *d_dst);
/* The reader's side of the same: forcing as it is stored -> native doubles, in HBM (the loader of data_load.py:342-390
 * byte-swaps NetCDF variables and widens single precision on the host; here the stored bytes cross PCIe and are widened
 * behind it).  d_dst receives numpy's a.astype(np.float64) of the n stored values at d_src: every non-NaN value exactly
 * (binary32 subnormals widened, not flushed; the sign of zero and both infinities kept), NaN stays NaN, the quiet NaN
 * 0x7fc00000 becomes 0x7ff8000000000000 (other payloads are only promised to stay NaN); XH_SRC_F64_BE is a byte swap and
 * keeps every bit pattern.  n >= 0; the pointers may be NULL only when n == 0; d_src aligned to its element, d_dst to 8
 * bytes.  XH_SRC_F64_BE may run in place (d_src == d_dst exactly); every other overlap of the two ranges, an unknown kind
 * or a misaligned pointer is XH_ERR_ARG (xh_last_error says which) and nothing is launched.  Enqueued on the context's
 * stream, timer "widen". */
#define XH_SRC_F32_LE 1             /* native float32 (a .npy saved as '<f4')        */
#define XH_SRC_F32_BE 2             /* NetCDF-classic `float`, numpy '>f4'            */
#define XH_SRC_F64_BE 3             /* NetCDF-classic `double`, numpy '>f8': a swap   */
int xh_widen(xh_ctx *ctx, const void *d_src, int kind, int64_t n, double *d_dst);
int xh_memset(xh_ctx *ctx, void *d_ptr, int value, size_t bytes);
int xh_sync(xh_ctx *ctx);
/* Gather / scatter whole rows of a [nrows_total, ncols] device array by row index (shard packing, samples). */
int xh_gather_rows(xh_ctx *ctx, const double *d_src, const int64_t *d_rows, int64_t nrows, int64_t ncols,
                   double *d_dst);
int xh_scatter_rows(xh_ctx *ctx, const double *d_src, const int64_t *d_rows, int64_t nrows, int64_t ncols,
                    double *d_dst);
/* [rows, cols] -> [cols, rows] */
int xh_transpose(xh_ctx *ctx, const double *d_src, int64_t rows, int64_t cols, double *d_dst);

/* HIP-event timing of the kernels each entry point launches, accumulated per kernel name on the context's stream.
 * Names: "pm_pet", "abcd_spinup", "abcd_basin_mean", "abcd_sim", "mrtm_route", "calib_abcd", "calib_kge", "calib_de",
 * "agg_time", "agg_spatial", "drought_thresh", "drought_stats", "hargreaves_pet", "gwam_spinup", "gwam_sim",
 * "hs_pet", "trn_daylight", "trn_pet", "diag_cell_total", "diag_group_sum", "ens_stats", "pack_f32_be", "widen", "grid_pack".  xh_timing_get waits for the stream, then
 * returns total milliseconds and launch count. */
int xh_timing_reset(xh_ctx *ctx);
/* a caller-named span on the context's stream, read back with xh_timing_get like the library's own timers (one open
 * at a time): e.g. what a step still spends in the write-out gather after the routing kernel has ended                */
int xh_mark_begin(xh_ctx *ctx, const char *name);
int xh_mark_end(xh_ctx *ctx);
int xh_timing_enable(xh_ctx *ctx, int on);
int xh_timing_get(xh_ctx *ctx, const char *name, double *total_ms, int64_t *launches);

/* ------------------------------------------------------------------ Penman-Monteith PET
 * Replaces pet/penman_monteith.py:run_pmpet (:394-477) with SetData (:17-99), et_veg (:223-334),
 * et_water (:337-361) and et_snow (:364-377) fused into one kernel over (cell, month).
 * Host tables are the DataLoader fields of data_load.py:94-117.                                         */
typedef struct xh_pm_tables {
    int32_t nlcs;                       /* number of land-cover classes (>= 7: rows 0 and 6 are hard-wired, :361,:377) */
    const double *cL, *beta, *rslimit, *Tminopen, *Tminclose, *VPDclose, *VPDopen, *RBLmin, *RBLmax, *rc,
        *emiss;                         /* host, [nlcs] each (gcam_ET_para.csv columns 0-2, 5-12)      */
    const double *alpha, *lai, *laimin, *laimax; /* host, [nlcs*12] each, row = class, col = month of year */
} xh_pm_tables;

int xh_pm_pet(xh_ctx *ctx, const xh_pm_tables *h_tab,
              int64_t ncell, int32_t nmonths,       /* nmonths = 12 * number of years                    */
              int32_t start_year,
              int32_t n_lc_years, const int32_t *h_lc_years, /* years of the land-cover slices (pm_lc_years) */
              int32_t water_idx, int32_t snow_idx,
              const double *d_tas, const double *d_tmin, const double *d_rhs, const double *d_wind,
              const double *d_rsds, const double *d_rlds,
              const double *d_tairprev,             /* [ncell,nmonths] or NULL: NULL = tas of the previous CELL,
                                                       zeros for cell 0 (data_load.py:128-129)            */
              const double *d_lct,                  /* [ncell, nlcs, n_lc_years]                          */
              const double *d_elev,                 /* [ncell]                                            */
              double *d_pet);                       /* out [ncell, nmonths]                               */

/* ------------------------------------------------------------------ ABCD runoff
 * Replaces runoff/abcd.py:abcd_execute / abcd_parallel / _run_basins (:314-422) and the ABCD class
 * (:41-311): spin-up, per-basin December means (set_vals :246-282), simulation.
 *   h_basin_index[ncell] : dense 0-based group id used for the spin-up means (cells of one basin share it)
 *   h_par_index[ncell]   : row of d_pars used by each cell (basin row for abcd_execute; cell row for ABCD(pars))
 *   d_pars[npar_rows,5]  : a, b (x1000 applied inside, abcd.py:48), c, d, m
 *   d_tmin may be NULL   : no snow component (abcd.py:44,51,144-146)
 * Outputs may individually be NULL.  spinup < 25 is rejected like the reference's IndexError (:258-266).  */
int xh_abcd(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t spinup, int32_t n_groups,
            const int32_t *h_basin_index, const int32_t *h_par_index, int64_t npar_rows, const double *d_pars,
            const double *d_pet, const double *d_precip, const double *d_tmin,
            double *d_aet, double *d_q, double *d_sav,
            double *d_sm0, double *d_gw0);          /* optional out [n_groups]: post-spin-up initial state */

/* ------------------------------------------------------------------ Hargreaves PET
 * Replaces pet/hargreaves.py:calculate_pet (:17-73) over every month at once, with the input preparation of
 * components.py:144-187 (nan_to_num of T and D) and data_load.py:83-84 (negative DTR -> 0) applied on the device to the
 * forcing as uploaded.  h_solar_dec / h_dr: utils/general.py:calc_sinusoidal_factor (:53-90) per month; h_ndays: days of
 * each month (general.py set_month_arrays).  d_lat_rad: radians(coords[:, 2]) (data_load.py:71-72).
 * Asynchronous (one stream synchronisation for the small month table).                                             */
int xh_hargreaves_pet(xh_ctx *ctx, int64_t ncell, int32_t nmonths,
                      const double *d_temp, const double *d_dtr,  /* [ncell, nmonths]                                 */
                      const double *d_lat_rad,                    /* [ncell]                                          */
                      const double *h_solar_dec, const double *h_dr, const double *h_ndays,   /* host, [nmonths]  */
                      double *d_pet);                             /* out [ncell, nmonths]                             */

/* ------------------------------------------------------------------ Hargreaves-Samani PET
 * Replaces pet/hargreaves_samani.py:execute (:95-119), one scalar pet() call per cell and month (:34-64), over every
 * month at once.  Inputs as the loader keeps them (data_load.py:86-90: NaN stays): t < 0 gives 0, a NaN t, tmax or tmin
 * gives NaN.  The day of year is j[m % 12] (15, 45, ..., 345); arccos of -tan(dec) tan(phi) inside [-1, 1], 0 outside;
 * ra = 118 / pi * acs + cos(phi) cos(dec) sin(acs) exactly as written (:60).  d_lat_deg: coords[:, 2] in degrees;
 * h_ndays: days of each month of the run (:18-28, leap years included).  Asynchronous after one stream synchronisation
 * for the small month tables.                                                                                        */
int xh_hs_pet(xh_ctx *ctx, int64_t ncell, int32_t nmonths,
              const double *d_tas, const double *d_tmax, const double *d_tmin,   /* [ncell, nmonths]                */
              const double *d_lat_deg,                                           /* [ncell]                         */
              const double *h_ndays,                                             /* host, [nmonths]                 */
              double *d_pet);                                                    /* out [ncell, nmonths]            */

/* ------------------------------------------------------------------ Thornthwaite PET
 * Replaces pet/thornthwaite.py:execute (:51-130) and calc_daylight_hours (:18-48).  NaN and negative temperatures count
 * as 0 (:85; the loader's nan_to_num, data_load.py:137-138, is xh_nan_to_num on the upload).  I = sum over each year of
 * (T / 5)^1.514, a = 6.75e-7 I^3 - 7.71e-5 I^2 + 0.0179 I + 0.492 (the code's constants, not the docstring's), PET =
 * 16 (10 T / I)^a (0 where I == 0) x L / 12 x N / 30.  daylight_mode XH_DAYLIGHT_REFERENCE: the daylight L of a common
 * year's month m is that of month-of-year m // nyears, as np.repeat spreads it (:113); leap years get the leap table in
 * month order (:116-122).  XH_DAYLIGHT_MONTHLY: every month its own month's daylight.  nmonths: whole years from
 * start_year; 0 with d_tas / d_pet NULL computes only the daylight table.  d_daylight (optional out [ncell, 24]): mean
 * daylight hours of the 12 months of a common year, then of a leap year.                                             */
#define XH_DAYLIGHT_REFERENCE 0
#define XH_DAYLIGHT_MONTHLY 1
int xh_thornthwaite_pet(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t start_year, int32_t daylight_mode,
                        const double *d_tas,                      /* [ncell, nmonths]                                  */
                        const double *d_lat_rad,                  /* [ncell]: radians(coords[:, 2])                    */
                        double *d_pet,                            /* out [ncell, nmonths]                              */
                        double *d_daylight);                      /* optional out [ncell, 24]                          */

/* ------------------------------------------------------------------ GWAM runoff
 * Replaces runoff/gwam.py:runoffgen (:18-88) driven month by month as components.py:298-384 / configurations.py:54-121
 * drive it: a spin-up pass over months [0, spinup) from d_sm0 whose final soil moisture starts the simulation over
 * [0, nmonths).  precip_col_spinup / precip_col_sim: the column of d_precip every month of that pass reads (the
 * reference's self.P, components.py:230 and :334: runoff_spinup - 1 and nmonths - 1); -1 = month m reads column m.
 * indexing: the soil-moisture marker of water bodies (999, gwam.py:18).  nmonths must be even and the [ncell, nmonths]
 * arrays 16-byte aligned.  d_aet, d_q, d_sav, d_sm_end (out [ncell]: soil moisture after the last month) may be NULL. */
int xh_gwam(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t spinup, int32_t precip_col_spinup,
            int32_t precip_col_sim, double indexing,
            const double *d_pet, const double *d_precip,  /* [ncell, nmonths]                                        */
            const double *d_sm_max, const double *d_sm0,  /* [ncell]: max soil moisture, initial soil moisture       */
            double *d_aet, double *d_q, double *d_sav,    /* out [ncell, nmonths]                                    */
            double *d_sm_end);

/* ------------------------------------------------------------------ MRTM routing
 * xh_route_plan_create replaces the per-call topology work of routing/mrtm.py:upstream_genmatrix (:194-230):
 * it takes UM = UP - I as CSR (row i = sorted columns j with +1 for "j flows into i" and -1 on the diagonal),
 * finds the independent river networks and lays them out for the LDS-resident kernel.  Row order of the
 * entries is preserved so sums are accumulated exactly as scipy's csr mat-vec does.                       */
int xh_route_plan_create(xh_ctx *ctx, int64_t ncell, const int64_t *h_indptr, const int32_t *h_indices,
                         const int8_t *h_sign, xh_route_plan **out);
void xh_route_plan_destroy(xh_route_plan *plan);
/* info[0]=networks, [1]=largest network (cells), [2]=workgroup-per-network units, [3]=cells routed by the global
 * fallback, [4]=largest such unit (cells), [5]=padded slots, [6]=1 if every cell has one downstream cell,
 * [7]=dataflow units, [8]=stream edges between them, [9]=pipeline depth, [10]=cells routed by the dataflow kernel,
 * [11]=most imported streams of one unit, [12]=deepest lane lag of the time-skewed layout in sub-steps (-1: layout
 * not available), [13]=kernel that routed the tree networks in the last xh_route_series call on this plan (0 none,
 * 1 lock-step units with monthly streams -- months shorter than the lane lags, or rows beyond the time-skewed kernels'
 * 32-bit offsets --, 2 time-skewed units of the bit-exact kernel k_mrtm_wave, 4 the reassociated kernel k_mrtm_rsum: the
 * default), [14]=calls of this plan re-run with one workgroup per
 * network after a device fault, [15]=calls cross-checked by XH_ROUTE_VALIDATE */
int xh_route_plan_info(const xh_route_plan *plan, int64_t info[16]);

/* (Rounds 3-5 had a second, PLAIN form of the bit-exact kernel's units here -- selected by XH_ROUTE_TYPED or learnt call by
 * call, with xh_route_plan_typed_info.  Retired in round 6: the bit-exact kernels are the checker and the XH_ROUTE_EXACT
 * option now, every unit of theirs in pair form; what knows which cells can fire is the PREPARED plan of the default form,
 * below.) */
/* Optional, with the HOST copies of the arrays the calls will pass on the device: makes the PREPARED plan of the default
 * (reassociated) routing form -- xh_route_plan_rsum_info below says what is in it -- from WHICH cells can fire at these
 * velocities, lengths and dt.  The package's own callers do it for the user (the pipeline on its planning thread beside the
 * forcing upload; routing.mrtm.route_series / streamrouting from the L, ChV and dt they hold).  May be called again: the same
 * data is a no-op, other data replaces the prepared plan.  Results never depend on it (the kernel guards what the plan
 * assumes; a trip routes the call again on the plan of pairs).  Partitions are kept per box under $XH_CACHE_DIR or
 * ~/.cache/xanthos_amd (XH_ROUTE_LEARN_CACHE=0: not).  A no-op in a process whose default form is the bit-exact one. */
int xh_route_plan_prepare(xh_ctx *ctx, xh_route_plan *plan, const double *h_flow_dist, const double *h_velocity, double dt);

/* Diagnostics: with XH_FLOW_STATS=1 in the environment the dataflow kernel records, per unit, {shader cycles inside the
 * sub-step loops, shader cycles total, 100 MHz ticks total, shape bits + placement, cycles waiting for data, cycles waiting for ring space}
 * -- the last two in bits 0-35 of their words, above them the flow-control checks that looked at the stream counter (36-49) and
 * those at which the value already known covered the need (50-63); this call waits for the
 * stream and copies up to max_words 64-bit words (6 per unit) of the last xh_route_series launch. */
int xh_route_plan_stats(xh_route_plan *plan, int64_t max_words, uint64_t *h_words, int64_t *n_words);

/* Host-side topology (integer work, no device needed).
 * xh_mrtm_downstream replaces routing/mrtm.py:downstream + make_flowdirgrid (:85-120, :233-258): D8 decode, the
 * longitude wrap quirk ((col+1) mod ncol for off-grid columns), off-grid rows -> self, ocean/self targets -> -1.
 *   h_ilon / h_ilat [ncell]: 1-based column / row of each cell (coords[:,3], coords[:,4]); h_id [ncell]: 1-based
 *   cell ids (coords[:,0]); h_flowdir [ncell]: D8 codes (-9999 = none).  h_dsid out [ncell], 1-based or -1.
 * xh_mrtm_upstream replaces routing/mrtm.py:upstream (:123-191): for each cell its 8 in-grid neighbours (no
 * date-line wrap), those draining into it first, then the count.  h_upid out [ncell, 9].
 * xh_mrtm_um_csr replaces upstream_genmatrix (:194-230): UM = UP - I as CSR with ascending columns;
 *   h_indptr [ncell+1], h_indices / h_sign sized ncell + sum(upid[:,8]).                                      */
int xh_mrtm_downstream(int64_t ncell, int32_t nrow, int32_t ncol, const int64_t *h_id, const int32_t *h_ilon,
                       const int32_t *h_ilat, const double *h_flowdir, int64_t *h_dsid);
int xh_mrtm_upstream(int64_t ncell, int32_t nrow, int32_t ncol, const int64_t *h_id, const int32_t *h_ilon,
                     const int32_t *h_ilat, const int64_t *h_dsid, int64_t *h_upid);
int xh_mrtm_um_csr(int64_t ncell, const int64_t *h_upid, int64_t *h_indptr, int32_t *h_indices, int8_t *h_sign);

/* xh_route_series replaces routing/mrtm.py:streamrouting (:16-82) and the month loops of
 * components.py:calculate_routing (:273-294): spin-up over months [0, spinup_months) then all nmonths,
 * nt = int(nday*86400/dt) explicit-Euler sub-steps per month, all inside one persistent kernel.
 *   h_ndays[nmonths]; d_runoff [ncell, nmonths] (mm/month); d_flow_dist, d_velocity, d_area [ncell]
 *   d_S0 [ncell] or NULL (zeros); outputs d_chstorage / d_avgchflow [ncell, nmonths] (either may be NULL),
 *   d_S_end / d_F_end [ncell] optional.  streamrouting() itself is the nmonths = 1, spinup = 0 case.
 * flags: XH_ROUTE_ATOMIC routes with global fp64 atomic scatter-adds (non bit-reproducible variant).
 * The dataflow kernels (tree networks) keep every unit resident and let units wait for each other, each wait bounded
 * by a 5 s timeout (two orders of magnitude above the kernel's run time at the full grid).  On a device shared with
 * another routing call the units may not all fit: the timeout then raises a sticky device fault, and the next
 * synchronising call (xh_sync, xh_memcpy_d2h) re-routes every call enqueued since the last synchronisation with one
 * workgroup per network (no waits between workgroups) before it returns -- XH_OK if nothing else was enqueued behind
 * the routing, XH_ERR_DEVICE (routing outputs valid, later results not) otherwise.  xh_route_plan_info[14] counts such
 * re-runs.  After such a fault the plan's next 8 calls (16, 32 ... 256 when faults repeat) skip the dataflow kernels, so
 * a device that stays shared does not cost a timeout per call; a fault-free dataflow call resets the back-off.
 * Bit-exactness of the dataflow kernels rests on a hardware assumption stated at xh_mrtm_wave.hip ("MEMORY-ORDERING
 * ASSUMPTION": write-through stream stores retire in order under s_waitcnt vmcnt); XH_ROUTE_VALIDATE checks a call
 * against the kernel that does not need it.                                                                        */
#define XH_ROUTE_DEFAULT 0
#define XH_ROUTE_FORCE_FALLBACK 1   /* route every network with the global-memory kernels (testing)        */
#define XH_ROUTE_ATOMIC 2           /* with the fallback: scatter-add outflow with global_atomic_add_f64   */
#define XH_ROUTE_NO_DATAFLOW 4      /* one workgroup per network even for tree-shaped networks (testing)   */
#define XH_ROUTE_NO_SKEW 8          /* dataflow units in lock-step with monthly streams, not time-skewed   */
#define XH_ROUTE_TEST_FAULT 16      /* testing: the dataflow kernel raises its fault word as a timed-out wait would */
#define XH_ROUTE_VALIDATE 32        /* cross-check: after a dataflow kernel routed the call, route it again with one
                                       workgroup per network (barriers only, no streams between units) and compare every
                                       output bit; synchronous; XH_ERR_DEVICE on a difference.  Also switched on for every
                                       call by XH_ROUTE_VALIDATE=1 in the environment.  xh_route_plan_info[15] counts the
                                       validated calls.                                                            */
/* (64 was XH_ROUTE_TYPED until round 5: ignored now) */
#define XH_ROUTE_REASSOC 128        /* tree networks by the REASSOCIATED form of the time-skewed kernel (k_mrtm_rsum): the row sum
                                       of mrtm.py:50-51 travels as running sums along chains of lanes (two LDS reads per
                                       sub-step for every unit instead of up to six) and the update of mrtm.py:54-69 is fused.
                                       Equal to the reference to rounding -- <= 1e-9 relative on every routed value at the
                                       full grid, identical NaN masks; the gate is 1e-6 -- NOT bit for bit.  THE DEFAULT since
                                       round 5 for calls that carry neither this flag nor XH_ROUTE_EXACT; XH_ROUTE_REASSOC=0 /
                                       1 in the environment moves that default.  xh_route_plan_info[13] = 4 when it routed
                                       the call (months shorter than its lane lags, networks that are not trees: the
                                       bit-exact kernels).  XH_ROUTE_VALIDATE then compares within 1e-9.               */
#define XH_ROUTE_EXACT 256          /* the bit-exact kernels for this call (every row sum in scipy's stored order) whatever
                                       the default says                                                                  */
/* The reassociated plan the last call ran on: info[8] = {its units; the leaves it folded into their downstream cells' lanes;
 * 1 if a guard trip has switched the prepared plan off; folded leaves of the prepared plan; cells in pair form of the plan
 * the last call ran on, -1 if ALL its lanes pass pairs of sums; the same for the prepared plan (-1: pairs, or none prepared);
 * calls routed again on the plan of pairs after a guard trip, so far; pair units of the plan the last call ran on}.
 * The PREPARED plan is the one xh_route_plan_prepare makes from the call's velocities, lengths and dt (reassociated form
 * only; XH_FLOW_FOLD=0 / XH_RSUM_SINGLE=0 switch its two parts off):
 *  - leaves that cannot fire (velocity * dt / length < 1) of river networks small enough to have no streams are carried by
 *    their parents' lanes, which frees enough lanes for every unit to have a SIMD of its own;
 *  - the lanes pass ONE running sum (of the adjusted flows) instead of the pair {sum F, sum F2}: only a cell that may fire
 *    AND has an upstream neighbour that may needs both -- the cells that can fire by construction with such a neighbour and
 *    a halo of XH_RSUM_HALO (8) cells downstream of them, where the reference's corner S1 >= 0 > S2 (mrtm.py:54, :66-69)
 *    sends negative flows -- and those few sit in pair units of their own.
 * Both rest on which cells can fire; the kernel guards the assumptions (folded leaves' storage, lateral inflow and initial
 * storage >= 0, the outflow of the halos' exit cells >= 0) and a trip routes the call again on the plan of pairs.          */
int xh_route_plan_rsum_info(const xh_route_plan *plan, int64_t info[8]);
/* Single units of the plan the last call ran on that ran the step WITHOUT the clamp of mrtm.py:54-63 ("linear units": none of
 * their cells may fire; guarded by the smallest storage each lane has seen).  0 with XH_RSUM_LINEAR=0 and on a plan of pairs. */
int64_t xh_route_plan_linear_units(const xh_route_plan *plan);
int xh_route_series(xh_ctx *ctx, xh_route_plan *plan, int32_t nmonths, int32_t spinup_months,
                    const int32_t *h_ndays, double dt,
                    const double *d_flow_dist, const double *d_velocity, const double *d_area,
                    const double *d_runoff, const double *d_S0,
                    double *d_chstorage, double *d_avgchflow, double *d_S_end, double *d_F_end, int32_t flags);

/* ------------------------------------------------------------------ the whole path as one pipelined call
 * xh_run_fused replaces the stage-after-stage hand-over of components.py:simulation (:344-370: calculate_pet ->
 * calculate_runoff -> calculate_routing): Penman-Monteith, ABCD (spin-up, basin means, simulation) and MRTM are enqueued
 * together -- PM runs in blocks of `block_months` months and the ABCD march follows one block behind on a second stream
 * (PET still in cache, the march on the issue slots PM leaves empty, its state carried from block to block); routing
 * follows when the last block of runoff exists.  Results are bit-identical to xh_pm_pet + xh_abcd +
 * xh_route_series with the same arguments (same kernels, same arithmetic).  Arguments mean what they mean there.
 * d_pet and d_q must be given (they are the stages' hand-over and outputs of the model); d_aet, d_sav, d_chstorage,
 * d_avgchflow may be NULL; plan = NULL stops after the runoff.  block_months = 0 picks the default (96); it must be a
 * multiple of 48.  Asynchronous; on return the context's stream is ordered after every output.                    */
typedef struct xh_fused_args {
    int64_t ncell;
    int32_t nmonths, start_year;
    const xh_pm_tables *pm;
    int32_t n_lc_years;
    const int32_t *h_lc_years;
    int32_t water_idx, snow_idx;
    const double *d_tas, *d_tmin, *d_rhs, *d_wind, *d_rsds, *d_rlds, *d_tairprev, *d_lct, *d_elev;
    int32_t abcd_spinup, n_groups;
    const int32_t *h_basin_index, *h_par_index;
    int64_t npar_rows;
    const double *d_pars, *d_precip, *d_abcd_tmin;
    xh_route_plan *plan;
    int32_t routing_spinup;
    const int32_t *h_ndays;
    double dt;
    const double *d_flow_dist, *d_velocity, *d_area, *d_S0;
    int32_t route_flags;
    double *d_pet, *d_aet, *d_q, *d_sav, *d_chstorage, *d_avgchflow;
    int32_t block_months;
    int32_t mode;       /* 0: PM blocks with the ABCD march one block behind, then routing (above).  1 (needs plan): the first
                         * max(spin-ups) months of PM and ABCD, then the ROUTING KERNEL, and the remaining months of PM and ABCD
                         * beside it on a second stream, fed to the running kernel through a months-ready word; falls back to
                         * the stage-by-stage order when the plan is not routed by the time-skewed dataflow kernel. Same results. */
} xh_fused_args;
int xh_run_fused(xh_ctx *ctx, const xh_fused_args *args);

/* ------------------------------------------------------------------ calibration objective
 * Replaces calibrate/calibrate_abcd.py:basin_runoff + objective_kge (:134-213) for set_calibrate = 0, batched
 * over a population: every member runs ABCD on the basin's cells, the simulated runoff is summed over cells per
 * month (nansum; x area x 1e-6 if d_area != NULL) and scored against h_obs with ED = 1 - KGE.
 *   d_pet_t / d_precip_t / d_tmin_t : [nmonths, ncell_b] (cell fastest; use xh_transpose), d_tmin_t may be NULL
 *   h_pars [nmembers, npar] with npar = 5 (a,b,c,d,m) or 4 (no snow)
 *   h_ed [nmembers] out; h_series [nmembers, nmonths] optional out                                          */
int xh_calib_objective(xh_ctx *ctx, int64_t ncell_b, int32_t nmonths, int32_t spinup, int32_t nmembers,
                       int32_t npar, const double *h_pars, const double *d_pet_t, const double *d_precip_t,
                       const double *d_tmin_t, const double *d_area, const double *h_obs, double *h_ed,
                       double *h_series);

/* ------------------------------------------------------------------ output aggregation
 * xh_agg_time replaces data_writer/out_writer.py:agg_to_year (:237-248) and the mm -> km3 scaling of write()
 * (:111-112): out[c, g] = f(in[c, g*group .. (g+1)*group)) x (d_scale ? d_scale[c] : 1), with f = NaN-skipping sum
 * (mode 0; an all-NaN block gives 0, as pandas does) or NaN-skipping mean (mode 1; all-NaN gives NaN), both in
 * pandas' compensated order (groupby.pyx group_sum / group_mean, columns ascending), bit for bit.
 * group = 12 aggregates months to years; group = 1, mode 0 is a plain per-cell scaling (NaN kept).  Mode 2 is
 * np.sum over the block in numpy's own order (eight accumulators, NaN propagates): the yearly totals of
 * accessible/accessible.py:41-42, bit for bit.
 * xh_agg_spatial: out[k, t] = plain NaN-skipping sum (ascending cells, from 0.0) over the cells with h_group[c] == k
 * (h_group is 0-based, -1 = cell not aggregated); groups without cells give NaN.  The order of the plain loops of
 * time_series.py:Aggregation_Map and accessible.py:50-53; out_writer.py:agg_spatial (pandas' groupby('id').sum(),
 * compensated) uses xh_diag_group_sum.                                                                       */
int xh_agg_time(xh_ctx *ctx, int64_t ncell, int32_t ncols, int32_t group, int32_t mode, const double *d_scale,
                const double *d_in, double *d_out);
int xh_agg_spatial(xh_ctx *ctx, int64_t ncell, int32_t ncols, int32_t n_groups, const int32_t *h_group,
                   const double *d_in, double *d_out);
/* Loader transform on the device: np.nan_to_num in place, as data_load.py applies to the PM forcings
 * and the ABCD tmin (:120-125, :194-195): NaN -> 0, +inf / -inf -> +/- largest finite double.                */
int xh_nan_to_num(xh_ctx *ctx, double *d_arr, int64_t n);

/* ------------------------------------------------------------------ drought statistics
 * xh_drought_thresholds replaces drought/drought_stats.py:getthresh (:150-171) as called by calculate_thresholds
 * (:69-83): for every cell and each of the nper periods of the year, the quantile over the nyear samples
 * d_hydro[c, month0 + y*nper + p] (y < nyear), by numpy's "linear" method.  The caller passes what depends only on
 * (nyear, q): the ranks k_prev / k_next of the two order statistics and the weight gamma = (nyear-1) q - k_prev
 * (xanthos_amd/drought/drought_stats.py computes them the way numpy does).  A NaN sample gives a NaN threshold.
 *   d_hydro [ncell, nmonths]; d_thresh out [nper, ncell] (the layout of the reference's thresholds file).
 * xh_drought_stats replaces droughtstats (:85-148): severity / intensity / duration [ncell, nmonths] (any may be
 * NULL) from d_hydro [ncell, nmonths] and d_thresh [nthresh, ncell]; month t uses threshold row t mod nthresh.   */
int xh_drought_thresholds(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t month0, int32_t nyear, int32_t nper,
                          int32_t k_prev, int32_t k_next, double gamma, const double *d_hydro, double *d_thresh);
int xh_drought_stats(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t nthresh, const double *d_hydro,
                     const double *d_thresh, double *d_severity, double *d_intensity, double *d_duration);

/* ------------------------------------------------------------------ hydropower potential
 * xh_hpot_qmax replaces hydropower/potential.py:constrain_q (:75-86) row by row: q_max[c] = np.percentile(d_q[c, :],
 * q_ex * 100) over all nmonths (<= 8192) samples, numpy's "linear" method; the caller passes k_prev / k_next / gamma
 * exactly as for xh_drought_thresholds.  A NaN in the row gives NaN.
 * xh_hpot_energy replaces :30-46: per cell and calendar year, the compensated sum (pandas resample("A").sum(), NaN
 * skipped) of (((c_ef_sww * clip(q, 0, q_max)) * c_hours) * c_twh) * elev[c], times c_ej.  d_year_of_month [nmonths]
 * int32: the year index 0 .. nyears-1 of each month.  d_E out [ncell, nyears].
 * xh_hpot_region replaces groupby(key, axis=1).sum() (:50, :61): d_R[g, y] = compensated sum of d_E[cells[j], y] over
 * j in [indptr[g], indptr[g+1]), in that order.  d_indptr [ngroups + 1], d_cells int64.                              */
int xh_hpot_qmax(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t k_prev, int32_t k_next, double gamma,
                 const double *d_q, double *d_qmax);
int xh_hpot_energy(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t nyears, const int32_t *d_year_of_month,
                   double c_ef_sww, double c_hours, double c_twh, double c_ej, const double *d_q, const double *d_qmax,
                   const double *d_elev, double *d_E);
int xh_hpot_region(xh_ctx *ctx, int32_t ngroups, int32_t nyears, const int64_t *d_indptr, const int64_t *d_cells,
                   const double *d_E, double *d_R);

/* ------------------------------------------------------------------ hydropower actual
 * xh_hact_inflow replaces hydropower/actual.py:56-62 and env_flow_constraint (:109-117): d_inflow out [nmonths, ndams] =
 * d_q[dam_cell[d], t] * catch[d] / assumed[d] * cumecs_to_mm3; d_env out [ndams, 12] by calendar month (month0 = start
 * month - 1), from the compensated monthly means and numpy's pairwise mean of all months; d_bad out [ndams] int32: 1
 * where the dam's inflow holds a NaN.  nmonths >= 12.
 * xh_hact_sim replaces get_power (:124-145) for every dam: d_rc [5, 12, ndams] rule curves (NaN already 1.1), d_par
 * [5, ndams] = cap, cap_live, q_max, efficiency, head (fall-backs applied); d_power out [nmonths, ndams] (MW), d_annual
 * out [nyears, ndams] compensated annual means (resample("A").mean()), d_bad_month out [ndams] int32: the first month
 * with no rule-curve row <= s / cap (the reference's IndexError), else -1.                                           */
int xh_hact_inflow(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t ndams, int32_t month0, const int64_t *d_dam_cell,
                   const double *d_catch, const double *d_assumed, double cumecs_to_mm3, const double *d_q, double *d_inflow,
                   double *d_env, int32_t *d_bad);
int xh_hact_sim(xh_ctx *ctx, int32_t nmonths, int32_t ndams, int32_t nyears, int32_t month0, const int32_t *d_year_of_month,
                double sww, double secs_in_month, const double *d_inflow, const double *d_env, const double *d_rc,
                const double *d_par, double *d_power, double *d_annual, int32_t *d_bad_month);

/* ------------------------------------------------------------------ diagnostics
 * xh_diag_cell_total replaces diagnostics/diagnostics.py:58 (q = np.sum(Q, axis=1) / nyear * area / 1e6) and :62
 * (np.mean(VIC, axis=1)): d_out[c * out_stride] = (((0.0 + pairwise(d_in[c, :])) / div1) * d_scale[c]) / div2, with
 * pairwise = np.sum's order over the contiguous row of ncols >= 1 values (blocks of 8192 added in turn, each by numpy's
 * pairwise_sum; NaN propagates; up to about 50,000 values, whose leaf table fills the LDS) and the multiplication
 * skipped when d_scale is NULL.
 * xh_diag_group_sum replaces :111-112 (runoff_df.groupby('id').sum()): d_sums[g, j] = pandas' compensated sum of
 * d_vals[c, j] over the cells with h_group[c] == g in ascending order, NaN skipped (0-based groups, -1 = no group;
 * d_vals [ncell, k], d_sums [ngroups, k]; a group without cells gives 0); d_counts [ngroups] out: cells per group.
 * The time-series plots (time_series.py:Aggregation_Map) use xh_agg_spatial.                                         */
int xh_diag_cell_total(xh_ctx *ctx, int64_t ncell, int32_t ncols, const double *d_in, double div1, const double *d_scale,
                       double div2, double *d_out, int64_t out_stride);
int xh_diag_group_sum(xh_ctx *ctx, int64_t ncell, int32_t k, int32_t ngroups, const int32_t *h_group, const double *d_vals,
                      double *d_sums, int64_t *d_counts);

/* ------------------------------------------------------------------ ensemble statistics
 * xh_ens_stats replaces no function of the reference: there an ensemble is a Python loop of whole runs and the
 * across-run mean / spread / quantiles are a host-side reduction over the files.  n elements (rows x columns of one
 * variable as written); h_d_members: host array of nmembers DEVICE pointers, [n] each; stat_mask: XH_ENS_* bits; h_q
 * [nq] quantiles in [0, 1]; h_d_out: host array of DEVICE pointers, [n] each, one per requested statistic in the order
 * mean, std, min, max (those whose bit is set), then the nq quantiles.  Every member array is read once per call.
 * Definitions (numpy's over axis 0 of the stacked array, bit for bit, for finite or NaN values): mean = sum in member
 * order from 0.0, / S; std = sample standard deviation (ddof = 1: sum in member order of (x - mean)^2, / (S - 1), sqrt;
 * NaN for S = 1); min / max NaN-propagating; quantile q: ascending sort, h = (S - 1) q, lo = floor(h), hi = min(lo + 1,
 * S - 1), g = h - lo, d = a[hi] - a[lo], g < 0.5 ? a[lo] + d g : a[hi] - d (1 - g); NaN if any member is NaN.
 * XH_ERR_LIMIT: more than 64 members or 16 quantiles.  Asynchronous on the context's stream (after one upload of the
 * pointer table, which waits for the stream).                                                                      */
#define XH_ENS_MEAN 1u
#define XH_ENS_STD 2u
#define XH_ENS_MIN 4u
#define XH_ENS_MAX 8u
int xh_ens_stats(xh_ctx *ctx, int64_t n, int32_t nmembers, const double *const *h_d_members, uint32_t stat_mask,
                 int32_t nq, const double *h_q, double *const *h_d_out);

/* ------------------------------------------------------------------ member skill
 * xh_basin_kge: the Kling-Gupta distance of a run's runoff against observed basin runoff, per basin, on the Q of the run
 * in HBM ([ncell, nmonths], mm per month, before any conversion of the writer).  The reference forms the same number inside
 * its calibration only: the basin series of calibrate_abcd.py:156-162 -- np.nansum over the basin's cells of rsim * area *
 * 1e-6 (km3_per_mth) or of rsim (mm_per_mth) -- and the distance of :196-213, ED = sqrt((r - 1)^2 + (sd_s / sd_o - 1)^2 +
 * (mean_s / mean_o - 1)^2) with population standard deviations and np.corrcoef's r; KGE = 1 - ED.
 * d_start [nbasins + 1] / d_cells: the cells of basin b, ascending, are d_cells[d_start[b] .. d_start[b + 1]); d_area
 * [ncell] in km2, NULL for mm_per_mth; d_obs [nbasins, nmonths]; d_series [nbasins, nmonths] optional out (NULL: kept in
 * the context's scratch); d_ed [nbasins] out.  The series is summed in cell order, a NaN term adding nothing; the moments
 * run over the months in a fixed tree; no atomics: two calls give the same bits.  A constant series or record gives NaN,
 * as numpy does.  XH_ERR_ARG: a NULL array other than d_area / d_series, nbasins <= 0 or > 65535, nmonths < 2, ncell < 1.
 * Asynchronous on the context's stream; nothing is uploaded (the tables are the caller's, made once, in HBM).       */
int xh_basin_kge(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t nbasins, const int64_t *d_start,
                 const int32_t *d_cells, const double *d_q, const double *d_area, const double *d_obs, double *d_series,
                 double *d_ed);

/* ------------------------------------------------------------------ skill at stream gauges
 * xh_gauge_skill: the routed streamflow of a run scored at stream gauges, on the Avg_ChFlow the run left in HBM.  The
 * reference scores streamflow inside its calibration only (calibrate_abcd.py:196-213); a forward run's flow is compared
 * with a measured discharge, if at all, from the files.  d_gauge_cell [ngauge]: 0-based grid cell of each gauge (two gauges
 * may share a cell); d_flow [ncell, nmonths] m3/s; d_obs [ngauge, nmonths] m3/s, NaN (or an infinity) = no observation;
 * d_series [ngauge, nmonths] optional out (NULL: not written): d_flow[cell_g, :], the same bits; d_metrics [ngauge, 8] out.
 * Per gauge, with V the months whose observation is finite, n = |V|, s = flow[cell_g, V], o = obs[g, V]:
 *   col 0  n (as a double)
 *   col 1  ED = sqrt((r - 1)^2 + (alpha - 1)^2 + (beta - 1)^2); KGE = 1 - ED is the caller's to form
 *   col 2  r: np.corrcoef through np.cov with n - 1, clipped to [-1, 1]
 *   col 3  alpha = std(s) / std(o), population standard deviations
 *   col 4  beta = mean(s) / mean(o)
 *   col 5  NSE = 1 - sum (s - o)^2 / sum (o - mean(o))^2
 *   col 6  PBIAS = 100 sum (s - o) / sum o
 *   col 7  RMSE = sqrt(sum (s - o)^2 / n)
 * Columns 1-4 are formed as the gauge form of the streamflow objective forms them (xh_calib_gauge_objective_multi): every
 * sum over V is 256 strided partial sums joined by one tree in shared memory, a skipped month adds nothing, no contraction --
 * so ED has the bits of that objective's per-gauge ED on the same series and record, and of the outlet form's for a
 * complete record.  The sums of columns 5-7 have the same order.  A NaN flow at a month of V makes columns 1-7 NaN, one at a
 * month outside V changes nothing; n < 2 gives NaN in columns 1-7; a record or a series of zero variance gives the NaN or
 * infinity numpy gives.  A gauge cell outside [0, ncell) reads no flow: columns 1-7 and its row of d_series are NaN (col 0
 * still counts the record).  One workgroup per gauge, fixed summation order, no atomics: two calls give the same bits.
 * XH_ERR_ARG: a NULL array other than d_series, ngauge < 1 or > 65535, nmonths < 2, ncell < 1.  Asynchronous on the
 * context's stream; nothing is uploaded (the tables are the caller's, made once, in HBM).                            */
int xh_gauge_skill(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t ngauge, const int32_t *d_gauge_cell,
                   const double *d_flow, const double *d_obs, double *d_series, double *d_metrics);

/* ------------------------------------------------------------------ standardized drought indices
 * xh_std_index replaces NO function of the reference: xanthos/drought/drought_stats.py knows a fixed threshold and Sheffield
 * & Wood's severity / intensity / duration only (xh_drought_*).  It forms the standardized runoff index SRI (Shukla & Wood
 * 2008) -- or, on soil moisture or routed flow, SSI / SSFI -- of d_x [ncell, nmonths] (month 0 a January, nmonths whole
 * years, <= 4096) in the SPI construction of McKee et al. (1993) at nscale (1..8) accumulation scales h_scale[s] (1..48
 * months) in one pass over d_x: h_d_index[s] [ncell, nmonths] out, one array per scale.
 *   Accumulated series  X[c, t] = ((x[c, t-k+1] + x[c, t-k+2]) + ...) + x[c, t], left to right, no contraction; NaN for
 *     t < k - 1; a NaN term makes X NaN.
 *   Reference sample    the period of ref_nyear whole years from month ref_month0 (a multiple of 12); for calendar month
 *     m = t mod 12: R(c, m) = {X[c, u] : u in the period, u mod 12 = m, u >= k - 1} in ascending u, n = |R|.
 *   dist = 0, gamma (Thom's closed-form approximation of the maximum-likelihood fit, as NCAR climate_indices): an element of
 *     R NaN or negative -> NaN parameters; n0 = #{s == 0}, q0 = n0 / n; P the positive elements, np = |P| < 4 -> NaN; mu =
 *     (sum of P from 0.0, ascending) / np; ml = (sum of log P from 0.0, ascending) / np; A = log(mu) - ml, not A > 0 -> NaN;
 *     alpha = (1 + sqrt(1 + 4 A / 3)) / (4 A), alpha > max_shape -> NaN; beta = mu / alpha.  X NaN or negative or NaN
 *     parameters -> index NaN; X == 0 -> H = q0; else H = q0 + (1 - q0) P(alpha, X / beta), P the regularized lower incomplete
 *     gamma function; index = min(max(ndtri(H), -3.09), 3.09).  The parameters are [ncell, 12, 4] tables of (q0, alpha, beta,
 *     n), an unusable entry four NaNs: h_d_par_out (NULL, or one per scale) receives the fit; h_d_par_in (NULL, or one per
 *     scale) is used INSTEAD of fitting (a future run indexed against a historic run's fit).
 *   dist = 1, empirical (Gringorten; Farahmand & AghaKouchak 2015): X NaN, an element of R NaN or n < 4 -> NaN; in = 1 when
 *     t lies in the reference period; L = #{s < X}, E = #{s == X}, N = n + 1 - in, rank = L + (E + 2 - in) / 2, p = (rank -
 *     0.44) / (N + 0.12); index = clip(ndtri(p), +-3.09).  h_d_par_out is ignored.
 * P(a, x) (series / continued fraction, at most 512 iterations, NaN when not converged: none for a <= 1000) and ndtri
 * (Wichura's AS 241) are csrc/xh_sindex_dev.h.  Fixed operation order, no atomics: two calls give the same bits.
 * XH_ERR_ARG: a NULL array (other than the two parameter lists), nmonths not a positive multiple of 12, a reference period
 * that is not whole years inside the series, dist not 0 / 1 / 2 (2: log-logistic, below), h_d_par_in with dist = 1, max_shape <= 0 (or NaN).
 * XH_ERR_LIMIT: nmonths > 4096, nscale outside 1..8, a scale outside 1..48.  Nothing is launched then.  Asynchronous on the
 * context's stream, timer "std_index"; nothing is uploaded.                                                          */
#define XH_STD_INDEX_GAMMA 0
#define XH_STD_INDEX_EMPIRICAL 1
int xh_std_index(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t nscale, const int32_t *h_scale, int32_t ref_month0,
                 int32_t ref_nyear, int32_t dist, double max_shape, const double *d_x, const double *const *h_d_par_in,
                 double *const *h_d_par_out, double *const *h_d_index);

/* ------------------------------------------------------------------ SPI, SPEI and the log-logistic distribution
 * xh_std_index2 replaces NO function of the reference either (xanthos has no standardized index): it is xh_std_index with an
 * optional subtrahend, and both entries take a third distribution.  xh_std_index IS xh_std_index2 with d_minus = NULL.
 *   d_minus (NULL: none) [ncell, nmonths]: the input element is d_x[c, t] - d_minus[c, t], one rounded subtraction (a NaN
 *     propagates), formed when the row enters LDS; no [ncell, nmonths] scratch array is made.  SPI is the index of
 *     precipitation, SPEI that of the climatic water balance D = precipitation - PET (Vicente-Serrano et al. 2010).
 *   dist = 2, log-logistic (three parameters, fitted by unbiased probability-weighted moments, Begueria et al. 2014): an
 *     element of R NaN or n < 4 -> NaN parameters.  Sort R ascending, s_1 <= ... <= s_n (the order among equal values does not
 *     matter).  Every sum from 0.0 over ascending i, no contraction, every coefficient the quotient of two exactly converted
 *     integers, multiplied into s_i:  w0 = (sum s_i) / n;  w1 = (sum s_i ((n - i) / (n - 1))) / n;  w2 = (sum s_i (((n - i)
 *     (n - i - 1)) / ((n - 1)(n - 2)))) / n;  beta = (2 w1 - w0) / (6 w1 - w0 - 6 w2);  g = (pi / beta) / sin(pi / beta)
 *     (Gamma(1 + 1/beta) Gamma(1 - 1/beta) in closed form);  alpha = (w0 - 2 w1) beta / g;  gamma = w0 - alpha g.  Usable when
 *     all three are finite and 1 < |beta| <= max_shape; four NaNs otherwise, and for a constant sample (s_1 = s_n: 0 / 0).  A negatively skewed sample gives beta < 0 and
 *     alpha < 0: the mirrored distribution with the upper bound gamma.  X NaN or NaN parameters -> index NaN;  z = (X -
 *     gamma) / alpha;  z <= 0: H = 0 for alpha > 0, H = 1 for alpha < 0;  else H = 1 / (1 + exp(-beta log z));  index =
 *     clip(ndtri(H), +-3.09), so H = 0 gives exactly -3.09 and H = 1 exactly +3.09.  The parameter tables are [ncell, 12, 4] =
 *     (alpha, beta, gamma, n); h_d_par_out / h_d_par_in as with gamma, bit for bit.
 * Errors as xh_std_index, with dist outside 0..2 an XH_ERR_ARG; h_d_par_in stays refused with dist = 1.  LDS: 24 B per month
 * + 384 B with dist = 2 (98 KB at 4092 months), 16 B per month + 384 B otherwise.  Timer "std_index".                 */
#define XH_STD_INDEX_LOGLOGISTIC 2
int xh_std_index2(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t nscale, const int32_t *h_scale, int32_t ref_month0,
                  int32_t ref_nyear, int32_t dist, double max_shape, const double *d_x, const double *d_minus,
                  const double *const *h_d_par_in, double *const *h_d_par_out, double *const *h_d_index);

/* ------------------------------------------------------------------ trend per row: Mann-Kendall and Theil-Sen
 * xh_trend replaces NO function of the reference: xanthos has no trend statistic.  Per row r of d_x (nrows rows of row_stride
 * doubles) it takes the window x[0 .. ncol) = d_x[r, col0 .. col0 + ncol) and writes d_out[r, 0 .. 10):
 *   n, s, var_s, z, p, slope, intercept, slope_lo, slope_hi, npairs.
 *   Column t belongs to season m = t mod nseason; its time is tau = (double)t / (double)nseason years from the window's start
 *     (one correctly rounded division).  nseason = 1 is the plain Mann-Kendall test (Mann 1945, Kendall 1975) on an annual
 *     series, nseason = 12 on a monthly one the seasonal Kendall test (Hirsch & Slack 1984).  A NaN element is left out of
 *     everything; +-inf is treated as NaN.
 *   A pair is (i, j), i < j, of the same season, both finite; npairs their number, n the number of finite elements.
 *   s = sum over the pairs of (x_j > x_i) - (x_j < x_i), by comparisons.
 *   V = sum_m n_m (n_m - 1)(2 n_m + 5) - sum over the finite elements of (e - 1)(2 e + 5), n_m the finite count of season m, e
 *     the number of finite elements of the element's season equal to it (==, itself included): integers, exact; the second
 *     sum is the tie correction sum over tie groups g (g - 1)(2 g + 5), without a sort.  var_s = (double)V / 18.0.
 *   z = (s - 1) / sqrt(var_s) for s > 0, (s + 1) / sqrt(var_s) for s < 0, 0 for s = 0 or var_s = 0;
 *     p = erfc(|z| 0.70710678118654752), two-sided.
 *   The slope of a pair is (x_j - x_i) / (double)((j - i) / nseason): one rounded subtraction, one correctly rounded division
 *     by a whole number of years, no contraction; -0.0 counts as +0.0.  With s_(0) <= ... <= s_(N-1) the sorted slopes, N =
 *     npairs: slope = s_((N-1)/2) for odd N, (s_(N/2-1) + s_(N/2)) / 2.0 for even N (numpy's median; Sen 1968);  sigma =
 *     sqrt(var_s);  Ru = min((int)rint((N - z_conf sigma) / 2.0), N - 1);  Rl = max((int)rint((N + z_conf sigma) / 2.0) - 1, 0),
 *     rint to even;  slope_lo = s_(Rl), slope_hi = s_(Ru).  z_conf is the normal quantile of (1 - confidence) / 2, a negative
 *     number.  For nseason = 1 without NaN these four are scipy.stats.theilslopes(x, arange(n), confidence), bit for bit.
 *   intercept = median(finite x) - slope median(tau of the finite elements), medians by numpy's rule (theilslopes' default
 *     method 'separate').
 *   With n < 4 or npairs = 0 only n and npairs are filled; the other eight columns are NaN.  A constant row gives s = 0,
 *     var_s = 0, z = 0, p = 1 and zero slopes.
 * The order statistics are exact: the slopes (up to nseason C(ncol / nseason, 2) per row) are not stored but recomputed from
 * the row in LDS by every pass of an MSB-first radix select on an order-preserving 64-bit key (csrc/xh_trend_dev.h, which
 * a host build runs too).  One workgroup per row; integer LDS adds only, a fixed floating-point order: two calls give the
 * same bits.  LDS: 8 B per column + 6.2 KB.
 * XH_ERR_ARG: a NULL array, col0 < 0, col0 + ncol > row_stride, ncol not a positive multiple of nseason, z_conf not negative
 * and finite.  XH_ERR_LIMIT: ncol > 4096, nseason outside 1..12.  Nothing is launched then.  Asynchronous on the context's
 * stream, timer "trend"; nothing is uploaded.                                                                          */
#define XH_TREND_NCOL 10
int xh_trend(xh_ctx *ctx, int64_t nrows, int32_t row_stride, int32_t col0, int32_t ncol, int32_t nseason, double z_conf,
             const double *d_x, double *d_out);

/* ------------------------------------------------------------------ annual extremes: GEV by L-moments
 * xh_extremes replaces NO function of the reference: xanthos has no extreme-value statistics.  Per row r of d_x (nrows rows of
 * row_stride doubles) it takes the window x[0 .. 12 nyear) = d_x[r, col0 .. col0 + 12 nyear) of a monthly series, year y being
 * columns 12 y .. 12 y + 11, and writes d_table[r, 0 .. 8 + nT) = n, l1, l2, t3, t4, k, alpha, xi, x_T..., d_annual[r, 0 .. nyear)
 * and d_T_year[r, 0 .. nyear) (either may be NULL).  No operation is contracted.
 *   1 a_y = the largest (kind = XH_EXTREMES_MAX) or smallest (XH_EXTREMES_MIN) of the year's 12 months, by comparisons from the
 *     first month on (of equal months the first stays); a NaN or +-inf month makes the year missing (a_y = NaN).  n = the years
 *     not missing.  z_y = a_y for max, -a_y for min: the low-flow fit is the GEV of the negated minima, the three-parameter
 *     Weibull distribution.
 *   2 Sample L-moments (Hosking 1990) of the n values z, sorted ascending by counting (ties by position, as the log-logistic
 *     fit ranks): b_r = (sum_i w_r(i) z_(i)) / (double)n, r = 0 .. 3, from 0.0 over ascending rank i, w_0 = 1, w_r(i) =
 *     (w_{r-1}(i) (double)(i - r + 1)) / (double)(n - r);  l1 = b0;  l2 = 2 b1 - b0;  l3 = (6 b2 - 6 b1) + b0;  l4 = ((20 b3 -
 *     30 b2) + 12 b1) - b0;  t3 = l3 / l2;  t4 = l4 / l2.
 *   3 GEV by L-moments (Hosking & Wallis 1997), Hosking's sign of the shape (scipy.stats.genextreme's c): k solves
 *     expm1(-k ln 3) / expm1(-k ln 2) = (3 + t3) / 2 by 10 Newton steps, always all of them, from k0 = 7.8590 c + (2.9554 c) c,
 *     c = 2 / (3 + t3) - ln 2 / ln 3;  G = tgamma(1 + k);  alpha = (l2 d) / G with d = k / -expm1(-k ln 2) (1 / ln 2 at k = 0);
 *     xi = l1 - alpha g with g = (1 - G) / k for |k| >= 0.25 and the Taylor series of Gamma(1 + k) (30 terms) below, which at
 *     k = 0 is the Gumbel limit alpha = l2 / ln 2, xi = l1 - 0.5772... alpha.  No fit when n < min_years, when the series is
 *     constant (z_(0) = z_(n-1)), when l2 is not > 0, or when k <= -1, decided as t3 > 1 - 2^-20 on the shared bits of t3
 *     (or a k that is not > -1 or not finite): the row then holds n, l1 and l2 as far as defined, the rest NaN.
 *   4 x_T, T > 1:  y = -log1p(-1 / T);  q = xi - alpha (expm1(k log y) / k), xi - alpha log y at k = 0;  x_T = q for max (exceeded
 *     once in T years on average), -q for min (undershot once in T years).  l1 and xi are reported negated back for min;
 *     l2, t3, t4, k, alpha are those of z.
 *   5 T_y:  s = (z_y - xi) / alpha;  u = -log F = exp(log1p(-k s) / k), exp(-s) at k = 0, outside the support (-k s <= -1) 0 for
 *     k > 0 and +inf for k < 0;  T_y = -1 / expm1(-u): 1 at F = 0, +inf at F = 1; NaN for a missing year or a row without a fit.
 *   d_par_in (NULL: none) [nrows, 8] = n .. xi as reported by another call (a historic run): steps 2 and 3 are skipped, the 8
 *     columns are copied bit for bit, and steps 4 and 5 use them on this call's annual series.
 * csrc/xh_extremes_dev.h holds this definition for device and host.  One wavefront per row, four to a workgroup, no workgroup
 * barrier; no atomics, a fixed order: two calls give the same bits.  LDS per workgroup: 4 (776 + 2 nyear) doubles.
 * XH_ERR_ARG: a NULL d_x or d_table (or h_T with nT > 0), col0 < 0, col0 + 12 nyear > row_stride, nyear < 1, 12 nyear > 4096,
 * nT outside 0..8, a T not > 1, kind neither 0 nor 1, min_years < 5.  Nothing is launched then.  Asynchronous on the context's
 * stream, timer "extremes"; h_T is read before the call returns; nothing is uploaded.                                   */
#define XH_EXTREMES_NPAR 8
#define XH_EXTREMES_MAX 0
#define XH_EXTREMES_MIN 1
int xh_extremes(xh_ctx *ctx, int64_t nrows, int32_t row_stride, int32_t col0, int32_t nyear, int32_t kind, int32_t min_years,
                int32_t nT, const double *h_T, const double *d_x, const double *d_par_in, double *d_table, double *d_annual,
                double *d_T_year);

/* ------------------------------------------------------------------ bootstrap intervals of the return levels
 * xh_extremes_boot replaces NO function of the reference.  Per row r of d_x (the window as in xh_extremes) it writes
 * d_ci[r, 0 .. 3 + 2 nT) = nb, k_lo, k_hi, x_T1_lo, x_T1_hi, ... and, when d_rep is not NULL, d_rep[r, b, 0 .. 5 + nT) = l1*, l2*,
 * t3*, t4*, k*, q*_T... of replicate b = 0 .. B - 1 in z's sign (a test and diagnosis output).  No operation is contracted.
 *   1 The row: the annual series, the counted sort zs[0 .. n), the L-moments and the fit of xh_extremes, steps 1 - 3.  A row
 *     without a fit gets nb = 0 and NaN everywhere else, and no replicate is drawn for it.
 *   2 Draws, mod 2^64, splitmix64(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) 0xBF58476D1CE4E5B9; z = (z ^ z >> 27)
 *     0x94D049BB133111EB; z ^ z >> 31.  h_row = splitmix64(seed ^ ((uint64)(row0 + r) * 0xD1342543DE82EF95));  h_rep =
 *     splitmix64(h_row ^ (uint64)(b + 1));  word(m) = splitmix64(h_rep ^ (uint64)(m + 1));  draw i of replicate b takes u32 = the
 *     low 32 bits of word(i >> 1) for even i, the high 32 bits for odd i;  j_i = (u32 * (uint64)n) >> 32, i = 0 .. n - 1, an
 *     index into zs (its bias: a cell's probability is off by at most n / 2^32 of itself).  The draws depend on (seed,
 *     row0 + r, b, i) alone: rows [a, b) of a call equal the call on that slice with row0 = a, and the replicates b < B1 of a
 *     call with B2 > B1 are those of the call with B1.
 *   3 A replicate's sample is the multiset {zs[j_i]} sorted ascending; its b_0 .. b_3, l1 .. l4, t3, t4 are step 2 of xh_extremes
 *     on it (formed by walking the counts c_j = #{i : j_i = j} over ascending j: equal values are interchangeable, the bits
 *     are a sort's), its fit follows the same rules (not constant, l2 > 0, t3 <= 1 - 2^-20, k > -1 and finite) through the
 *     same functions.  nb = the replicates with a fit.
 *   4 p_lo = (1 - confidence) / 2, p_hi = 1 - p_lo.  For k and each return level, the nb values sorted ascending, numpy's
 *     `linear` quantile: h = (nb - 1) p, lo = floor(h), hi = min(lo + 1, nb - 1), g = h - lo, d = a[hi] - a[lo], g < 0.5 ?
 *     a[lo] + d g : a[hi] - d (1 - g).  Reported in the variable's own sign with lo <= hi: for min the level bounds are
 *     -Q(p_hi) and -Q(p_lo); k's interval is that of z's k.  nb < ceil(B / 2): every bound NaN, nb still reported.
 * csrc/xh_exboot_dev.h holds this definition for device and host.  One one-wavefront workgroup per row at a time, lane <->
 * replicate; no atomics, nothing crosses a workgroup, every trip count known at launch, a fixed order: two calls give the
 * same bytes whatever the grid.  Scratch slot 2 holds (1 + nT) B doubles per workgroup.
 * XH_ERR_ARG: what xh_extremes refuses, B outside 2..2048, confidence not strictly between 0 and 1, row0 < 0; each message
 * names its value.  Nothing is launched then.  Asynchronous on the context's stream, timer "extremes_boot"; h_T is read
 * before the call returns; nothing is uploaded.                                                                        */
#define XH_EXB_MAX_B 2048
int xh_extremes_boot(xh_ctx *ctx, int64_t nrows, int32_t row_stride, int32_t col0, int32_t nyear, int32_t kind, int32_t min_years,
                     int32_t nT, const double *h_T, int32_t B, double confidence, uint64_t seed, int64_t row0, const double *d_x,
                     double *d_ci, double *d_rep);

/* ------------------------------------------------------------------ flow duration curve and regime signatures
 * xh_signatures replaces NO function of the reference: xanthos has no flow signatures.  Per row r of d_x (nrows rows of
 * row_stride doubles) the window is x[0 .. 12 nyear) = d_x[r, col0 ..); column t has calendar month (cal0 + t) mod 12, 0 =
 * January; year y is columns 12 y .. 12 y + 11.  Every element enters as x + 0.0 (-0.0 counts as +0.0); a NaN or +-inf element is
 * left out of everything.  No operation is contracted.
 *   S256(f): lane l of 256 adds f(t) from 0.0 over the included t = l, l + 256, ... in ascending order; the 256 partial sums are
 *     joined by the tree of xh_block_sum256 (csrc/xh_kge.h).  A "pair" is (t, t + 1) with both elements included.  "Sequential":
 *     from 0.0 in ascending index order.
 *   Q(p): the n included values sorted ascending a[0 .. n), numpy's `linear` quantile: h = (n - 1) p, lo = floor(h), hi =
 *     min(lo + 1, n - 1), g = h - lo, d = a[hi] - a[lo], g < 0.5 ? a[lo] + d g : a[hi] - d (1 - g).
 *   xbar_m = (the sequential sum over ascending t of the included elements of calendar month m) / c_m, c_m their count;
 *     R = the sequential sum over m = 0 .. 11 of xbar_m;  C, S = the sequential sums over m of xbar_m COS[m], xbar_m SIN[m], COS
 *     and SIN the correctly rounded doubles of cos and sin of pi (2 m + 1) / 12.  A_y = the sequential sum of the 12 months of
 *     year y, for the years whose 12 months are all included.
 *   d_table[r, 0 .. 18):
 *      0 n   1 n_zero = #{x == 0}   2 mean = S256(x) / n   3 std = sqrt(S256((x - mean)^2) / (n - 1)), NaN for n < 2
 *      4 cv = std / mean   5 median = Q(0.5)
 *      6 lag1 = S256 over pairs((x_t - mean)(x_{t+1} - mean)) / S256((x - mean)^2), NaN for n < 2
 *      7 flashiness = S256 over pairs(|x_{t+1} - x_t|) / S256(x)   (Richards-Baker)
 *      8 fdc_slope = (log Q(0.67) - log Q(0.34)) / 0.33, NaN when Q(0.34) is not > 0
 *      9 regime_total = R   10 peak_month, 11 low_month = 1 + the first m of the largest, the smallest xbar_m
 *     12 seasonality = (sequential sum over m of |xbar_m - R / 12.0|) / R   (Walsh & Lawler 1981)
 *     13 centroid = atan2(S, C) (6 / pi), plus 12.0 if negative: months from 1 January, 0.5 = mid-January
 *     14 concentration = sqrt(C C + S S) / R   (Markham 1970)
 *     15 n_years = the complete years   16 annual_mean = (sequential sum of A_y) / n_years
 *     17 annual_cv = sqrt((sequential sum of (A_y - annual_mean)^2) / (n_years - 1)) / annual_mean, NaN for n_years < 2
 *     Columns 9 - 14 are NaN when any c_m = 0.  With n = 0 only n, n_zero and n_years are numbers, the rest is NaN.
 *   d_fdc (NULL: none) [nrows, nP]: Q(h_prob[j]), NaN for n = 0.   d_regime (NULL: none) [nrows, 12]: xbar_m, NaN where c_m = 0.
 * csrc/xh_signatures_dev.h holds this definition for device and host.  One 256-lane workgroup per row at a time, the row in
 * LDS padded to a power of two P, a bitonic sort in place; no atomics, nothing crosses a workgroup, every trip count known at
 * launch, a fixed order: two calls give the same bytes whatever the grid.  LDS per workgroup: (P + 800 + nyear) doubles.
 * XH_ERR_ARG: a NULL d_x or d_table (or h_prob with nP > 0), col0 < 0, col0 + 12 nyear > row_stride, nyear < 1, 12 nyear > 4096,
 * cal0 outside 0..11, nP outside 0..16, a probability not strictly between 0 and 1; each message names its value.  Nothing is
 * launched then.  Asynchronous on the context's stream, timer "signatures"; h_prob is read before the call returns; nothing is
 * uploaded.                                                                                                             */
#define XH_SIG_NCOL 18
#define XH_SIG_MAX_P 16
int xh_signatures(xh_ctx *ctx, int64_t nrows, int32_t row_stride, int32_t col0, int32_t nyear, int32_t cal0, int32_t nP,
                  const double *h_prob, const double *d_x, double *d_table, double *d_fdc, double *d_regime);

/* ------------------------------------------------------------------ water balance and Budyko signatures
 * xh_water_balance replaces NO function of the reference: xanthos has no signatures of two variables.  Per row r of d_p, d_pet,
 * d_q and d_aet (NULL: none; nrows rows of row_stride doubles each) the window is columns col0 .. col0 + 12 nyear; year y is
 * columns 12 y .. 12 y + 11 of it.  Every element enters as x + 0.0.  Month t is INCLUDED when every array given is finite at t;
 * a year is COMPLETE when its 12 months are included.  No operation is contracted.
 *   A^v_y, v in {P, PET, AET, Q}: the sequential sum (from 0.0, ascending) of the 12 months of a complete year.
 *   Y256(f): lane l of 256 adds f(y) from 0.0 over the complete years y = l, l + 256, ... in ascending order; the 256 partial
 *     sums are joined by the tree of xh_block_sum256 (csrc/xh_kge.h).  S256(f): the same over the included months.
 *   n_years = the complete years; vbar = Y256(A^v) / n_years; dv_y = A^v_y - vbar.
 *   d_table[r, 0 .. 21):
 *      0 n_years   1 n_months = the included months   2 p_mean = pbar   3 pet_mean = petbar   4 aet_mean = aetbar (NaN without
 *      d_aet)   5 q_mean = qbar   6 runoff_ratio = qbar / pbar   7 aridity = phi = petbar / pbar   8 evaporative = aetbar / pbar
 *      9 residual = (pbar - aetbar) - qbar, the implied storage change per year   10 closure = residual / pbar
 *     11 omega = Fu's parameter: the omega > 1 with fu(phi, omega) = eps, eps = (pbar - qbar) / pbar
 *     12 budyko_dev = eps - fu(phi, omega0)
 *     13 elast_p = the median (the values sorted ascending, numpy's `linear` rule at 0.5 as xh_signatures writes it) of
 *        e_y = (dQ_y / dP_y) (pbar / qbar) over the complete years with dP_y != 0; 14 elast_pet the same with dPET_y and petbar;
 *        NaN when qbar is not > 0 or no year qualifies      (Sankarasubramanian et al. 2001)
 *     15 elast_p_ls = b1, 16 elast_pet_ls = b2: with x1 = dP_y / pbar, x2 = dPET_y / petbar, z = dQ_y / qbar and the Y256 sums
 *        s11 = x1 x1, s12 = x1 x2, s22 = x2 x2, s1z = x1 z, s2z = x2 z: det = s11 s22 - s12 s12,
 *        b1 = (s1z s22 - s2z s12) / det, b2 = (s2z s11 - s1z s12) / det; NaN unless n_years >= 3 and det > 0
 *     17 r_pq = Y256(dP dQ) / sqrt(Y256(dP dP) Y256(dQ dQ)), NaN unless the product is > 0
 *     18 dry_fraction = #{included t: P_t < PET_t} / n_months
 *     19 lag_peak = the first k in 0 .. max_lag with the largest c_k, 20 r_peak = that c_k; NaN when no c_k is a number, with
 *        mP = S256(P) / n_months, mQ = S256(Q) / n_months and c_k = S256 over the t with t and t + k both included
 *        ((P_t - mP) (Q_{t+k} - mQ)) / sqrt(S256((P - mP)^2) S256((Q - mQ)^2))
 *   d_xcorr (NULL: none) [nrows, max_lag + 1]: c_k.   d_annual (NULL: none) [nrows, 4, nyear]: A^v_y, NaN for a year that is not
 *   complete, the AET plane NaN without d_aet.
 *   Fu's curve in a form that neither overflows nor cancels: lo = min(1, phi), m = max(1, phi), r = lo / m,
 *     g(omega) = log1p(exp(omega log r)) / omega, fu(phi, omega) = lo - m expm1(g(omega)); NaN when phi is NaN.  omega solves
 *     m expm1(g(omega)) = lo - eps by exactly 60 bisection steps on s = log(omega - 1) over [log 2^-20, log 2^7], always all of
 *     them, and is 1 + exp(the last interval's midpoint); NaN unless 0 < eps < lo and the target lies strictly between the
 *     function's values at the two ends.
 *   With n_years = 0 only columns 0, 1, 18, 19 and 20 may be numbers.  A ratio whose denominator is 0 follows IEEE.  Every column
 *   but omega and budyko_dev is comparisons, + - x / and sqrt in this order: the same bits from the host and the device build.
 * csrc/xh_wbalance_dev.h holds this definition for device and host.  One 256-lane workgroup per row at a time, P and Q in LDS;
 * no atomics, nothing crosses a workgroup, every trip count known at launch, a fixed order: two calls give the same bytes
 * whatever the grid.  LDS per workgroup: (28 nyear + 2 P2 + 1808) doubles, P2 the power of two >= nyear.
 * XH_ERR_ARG: a NULL d_p, d_pet, d_q or d_table, col0 < 0, col0 + 12 nyear > row_stride, nyear < 1, 12 nyear > 4096, max_lag
 * outside 0..12, omega0 not finite or not > 1; each message names its value.  Nothing is launched then.  Asynchronous on the
 * context's stream, timer "water_balance"; nothing is uploaded.                                                         */
#define XH_WB_NCOL 21
#define XH_WB_MAX_LAG 12
int xh_water_balance(xh_ctx *ctx, int64_t nrows, int32_t row_stride, int32_t col0, int32_t nyear, int32_t max_lag, double omega0,
                     const double *d_p, const double *d_pet, const double *d_q, const double *d_aet, double *d_table,
                     double *d_annual, double *d_xcorr);

/* The same objective for SEVERAL basins in one launch, each basin with its own population: one basin alone is only
 * months x ~1.7 us of dependent chain, far too little to fill the chip.  h_ncell [nbasins]; h_pars [nbasins, nmembers,
 * npar]; h_pet_t / h_precip_t / h_tmin_t / h_area: host arrays of nbasins DEVICE pointers ([nmonths, ncell_b] each;
 * h_tmin_t NULL for npar = 4, h_area NULL for mm_per_mth); h_obs [nbasins, nmonths]; h_ed [nbasins, nmembers] out;
 * h_series [nbasins, nmembers, nmonths] optional out.                                                        */
int xh_calib_objective_multi(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, int32_t nmonths, int32_t spinup,
                             int32_t nmembers, int32_t npar, const double *h_pars, const double *const *h_pet_t,
                             const double *const *h_precip_t, const double *const *h_tmin_t,
                             const double *const *h_area, const double *h_obs, double *h_ed, double *h_series);

/* ------------------------------------------------------------------ streamflow objective (set_calibrate = 1)
 * ABCD on the basin's cells (spin-up and initial state as above), the runoff scattered onto the basin's upstream
 * closure through UM (foreign cells of the closure carry zero runoff and their own initial storage), MRTM over the
 * closure (routing_spinup months, then all nmonths with the carried storage; dt seconds per sub-step, the day counts
 * of h_ndays), the basin's outlet series = sum of Avg_ChFlow over its outlets in ascending cell order [m3/s], scored
 * against h_obs with ED = 1 - KGE.  Host tables of every basin's closure, rows concatenated basin after basin:
 *   h_closure_ptr [nbasins + 1]  first row of each basin's closure; rows in ascending cell order
 *   h_row_ptr [ncl + 1], h_cols [nnz], h_sign [nnz]   the closure's rows of UM, columns closure-local, stored order
 *   h_basin_col [ncl]    column of the basin's forcing ([nmonths, ncell_b]) of a closure row, -1 outside the basin
 *   h_outlet_rank [ncl]  rank of the row among its basin's outlets (0, 1, ... ascending), -1 for other rows
 *   h_tauinv, h_area, h_s0 [ncl]   ChV / L, cell area (km2), initial channel storage (m3)
 * A closure holds at most 3072 cells.                                                                          */
typedef struct {
    int32_t routing_spinup;
    double dt;
    const int32_t *h_ndays;
    const int64_t *h_closure_ptr;
    const int64_t *h_row_ptr;
    const int32_t *h_cols;
    const int8_t *h_sign;
    const int32_t *h_basin_col;
    const int32_t *h_outlet_rank;
    const double *h_tauinv;
    const double *h_area;
    const double *h_s0;
} xh_calib_flow_desc;

/* As xh_calib_objective_multi (no h_area: the routing tables carry the areas); h_series [nbasins, nmembers, nmonths]
 * optional out = the outlet series.                                                                            */
int xh_calib_flow_objective_multi(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, int32_t nmonths, int32_t spinup,
                                  int32_t nmembers, int32_t npar, const double *h_pars, const double *const *h_pet_t,
                                  const double *const *h_precip_t, const double *const *h_tmin_t,
                                  const xh_calib_flow_desc *flow, const double *h_obs, double *h_ed, double *h_series);

/* ------------------------------------------------------------------ streamflow objective at stream gauges
 * The same objective scored at gauges on cells inside the network instead of at the basin's outlets; records may have
 * gaps.  A gauge is (id, cell, weight) and belongs to the basin of its cell.  Runoff of basin B, spin-up and initial
 * state are those of the outlet form (the basin-mean December state over ALL of B's cells); rsim = 0 outside B.  B is
 * routed ONCE per member on the union of its gauges' upstream closures through UM (a subset of the outlet closure;
 * basin cells outside the union take no part in the routing pass, closure cells outside B carry zero runoff from their
 * own initial storage): routing_spinup months, then all nmonths, dt seconds per sub-step.  The series of gauge g is
 * Avg_ChFlow[cell_g] [m3/s] for every month, nothing summed: the bits of routing the world.
 * ED_g = 1 - KGE of series_g against obs_g over the months V_g whose observation is finite (n = |V_g| >= 2; population
 * std, corrcoef via cov with n - 1, clipped to [-1, 1]); a complete record gives the bits of the outlet form's score.
 * ED_B = (sum w_g ED_g) / (sum w_g), the basin's gauges taken in ascending (cell, gauge id) order and summed left to
 * right; one gauge of weight 1 gives ED_B == ED_g.
 * Tables as xh_calib_flow_desc without outlet ranks, the closure being the union closure, plus
 *   h_gauge_ptr [nbasins + 1]  first gauge of each basin (every basin has at least one); ngauge = h_gauge_ptr[nbasins]
 *   h_gauge_row [ngauge]       closure-local row of the gauge's cell (a basin cell), ascending within a basin
 *   h_gauge_weight [ngauge]    w_g > 0, finite
 * h_basin_col addresses the basin's forcing ([nmonths, ncell_b], all of B's cells) as in the outlet form; only the
 * basin cells present in the closure run ABCD in the routing pass.  A union closure holds at most 3072 cells.     */
typedef struct {
    int32_t routing_spinup;
    double dt;
    const int32_t *h_ndays;
    const int64_t *h_closure_ptr;
    const int64_t *h_row_ptr;
    const int32_t *h_cols;
    const int8_t *h_sign;
    const int32_t *h_basin_col;
    const double *h_tauinv;
    const double *h_area;
    const double *h_s0;
    const int64_t *h_gauge_ptr;
    const int32_t *h_gauge_row;
    const double *h_gauge_weight;
} xh_calib_gauge_desc;

/* As xh_calib_flow_objective_multi with h_obs [ngauge, nmonths] (NaN = missing) and h_ed [nbasins, nmembers] = ED_B.
 * Optional outs: h_ed_gauge [ngauge, nmembers] = ED_g, h_series [ngauge, nmembers, nmonths] = the gauge series.  */
int xh_calib_gauge_objective_multi(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, int32_t nmonths, int32_t spinup,
                                   int32_t nmembers, int32_t npar, const double *h_pars, const double *const *h_pet_t,
                                   const double *const *h_precip_t, const double *const *h_tmin_t,
                                   const xh_calib_gauge_desc *gauge, const double *h_obs, double *h_ed,
                                   double *h_ed_gauge, double *h_series);

/* ------------------------------------------------------------------ streamflow objective with a velocity scale
 * One more calibration parameter per basin, the dimensionless velocity scale v > 0, in either form above.  Steps of the
 * contract other than the routing are unchanged; the routing (mrtm.py:42 on a scaled channel velocity) uses
 *   ChV_i' = v ChV_i for the closure's cells of basin B,  ChV_i' = ChV_i for its cells outside B (those belong to
 *   another basin's calibration),  tau^-1 = (v ChV_i) / L_i: the product first, then the IEEE quotient.
 * A member's row of parameters is [a, b, c, d, (m), v]: h_pars [nbasins, nmembers, npar + 1], npar = 4 or 5 still
 * counting the ABCD genes.  v = 1.0 returns the bits of the form without the scale, and a member's result depends on its
 * own row only.  Beside the desc of the form:
 *   h_velocity, h_length [ncl]   ChV (m/s) and L (m) of every closure row; h_tauinv must equal h_velocity / h_length   */
typedef struct {
    const double *h_velocity;
    const double *h_length;
} xh_calib_velocity_desc;

/* As xh_calib_flow_objective_multi (calibrate_abcd.py:134-213 with mrtm.py:42 on the scaled ChV), h_pars rows
 * [npar + 1].                                                                                                    */
int xh_calib_flow_velocity_objective_multi(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, int32_t nmonths,
                                           int32_t spinup, int32_t nmembers, int32_t npar, const double *h_pars,
                                           const double *const *h_pet_t, const double *const *h_precip_t,
                                           const double *const *h_tmin_t, const xh_calib_flow_desc *flow,
                                           const xh_calib_velocity_desc *velocity, const double *h_obs, double *h_ed,
                                           double *h_series);
/* As xh_calib_gauge_objective_multi (the same lines, scored at gauges), h_pars rows [npar + 1].                 */
int xh_calib_gauge_velocity_objective_multi(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, int32_t nmonths,
                                            int32_t spinup, int32_t nmembers, int32_t npar, const double *h_pars,
                                            const double *const *h_pet_t, const double *const *h_precip_t,
                                            const double *const *h_tmin_t, const xh_calib_gauge_desc *gauge,
                                            const xh_calib_velocity_desc *velocity, const double *h_obs, double *h_ed,
                                            double *h_ed_gauge, double *h_series);

/* ------------------------------------------------------------------ differential evolution on the device
 * Replaces the scipy.optimize.differential_evolution call of calibrate/calibrate_abcd.py:calibrate_basin (:103-112,
 * SciPy defaults: best1bin, Latin-hypercube start, dither (0.5, 1), recombination 0.7, tol 0.01, polish off) AND the
 * serial loop over basins of calibrate_all (:256-262): all basins of the session search at once in lock-step
 * generations; populations, trial vectors, energies and convergence flags stay in HBM and a generation is five
 * kernel launches with no host work.  Selection is generation-synchronous (SciPy's updating='deferred').
 * Random numbers are counter-based on (seed, h_basin_key[b], generation, member): a basin's search does not depend
 * on the other basins of the session or on the device, so basin-sharded multi-GPU runs reproduce one-GPU runs.
 *   xh_calib_de_create : basins as for xh_calib_objective_multi (device forcing [nmonths, ncell_b] per basin, which
 *                        must outlive the session); h_basin_key [nbasins] or NULL (= 0..nbasins-1); h_lo / h_hi
 *                        [npar] parameter bounds (:62-64); nmembers = popsize x npar in SciPy's terms
 *   xh_calib_de_init   : Latin-hypercube population and its energies
 *   xh_calib_de_step   : ngen generations; a basin stops when std(E) <= atol + tol |mean(E)| (SciPy's test);
 *                        *h_n_active = basins still searching after the last generation
 *   xh_calib_de_result : h_x [nbasins, npar] best parameters, h_fun [nbasins] = ED = 1 - KGE, h_nfev, h_nit,
 *                        h_active (each may be NULL)
 *   xh_calib_de_state  : which = 0 population + energies, 1 last trial vectors + their energies (unit cube),
 *                        2 last trial vectors scaled to parameter space; [nbasins, nmembers, npar] / [nbasins, nmembers]
 *   xh_calib_de_set_state : overwrite population and energies and re-activate every basin (tests, restarts)   */
typedef struct xh_calib_de xh_calib_de;
int xh_calib_de_create(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, const uint64_t *h_basin_key,
                       int32_t nmonths, int32_t spinup, int32_t nmembers, int32_t npar,
                       const double *const *h_pet_t, const double *const *h_precip_t, const double *const *h_tmin_t,
                       const double *const *h_area, const double *h_obs, const double *h_lo, const double *h_hi,
                       uint64_t seed, xh_calib_de **out);
/* The same search on the streamflow objective (xh_calib_flow_objective_multi's tables; no h_area).               */
int xh_calib_de_create_flow(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, const uint64_t *h_basin_key,
                            int32_t nmonths, int32_t spinup, int32_t nmembers, int32_t npar,
                            const double *const *h_pet_t, const double *const *h_precip_t,
                            const double *const *h_tmin_t, const xh_calib_flow_desc *flow, const double *h_obs,
                            const double *h_lo, const double *h_hi, uint64_t seed, xh_calib_de **out);
/* The same search on the gauge form of the streamflow objective (the contract of xh_calib_gauge_objective_multi:
 * union closures routed once per member, masked ED per gauge, weighted mean per basin); h_obs [ngauge, nmonths],
 * NaN = missing.  The energies of the search are ED_B.                                                          */
int xh_calib_de_create_gauge(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, const uint64_t *h_basin_key,
                             int32_t nmonths, int32_t spinup, int32_t nmembers, int32_t npar,
                             const double *const *h_pet_t, const double *const *h_precip_t,
                             const double *const *h_tmin_t, const xh_calib_gauge_desc *gauge, const double *h_obs,
                             const double *h_lo, const double *h_hi, uint64_t seed, xh_calib_de **out);
/* The same searches (calibrate_abcd.py:103-112) on the velocity forms of the streamflow objective: npar = 4 or 5 ABCD
 * genes, the search has npar + 1 genes with v last; h_lo / h_hi [npar + 1], results and states [.., npar + 1].     */
int xh_calib_de_create_flow_velocity(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, const uint64_t *h_basin_key,
                                     int32_t nmonths, int32_t spinup, int32_t nmembers, int32_t npar,
                                     const double *const *h_pet_t, const double *const *h_precip_t,
                                     const double *const *h_tmin_t, const xh_calib_flow_desc *flow,
                                     const xh_calib_velocity_desc *velocity, const double *h_obs, const double *h_lo,
                                     const double *h_hi, uint64_t seed, xh_calib_de **out);
int xh_calib_de_create_gauge_velocity(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, const uint64_t *h_basin_key,
                                      int32_t nmonths, int32_t spinup, int32_t nmembers, int32_t npar,
                                      const double *const *h_pet_t, const double *const *h_precip_t,
                                      const double *const *h_tmin_t, const xh_calib_gauge_desc *gauge,
                                      const xh_calib_velocity_desc *velocity, const double *h_obs, const double *h_lo,
                                      const double *h_hi, uint64_t seed, xh_calib_de **out);
void xh_calib_de_destroy(xh_calib_de *de);
int xh_calib_de_init(xh_calib_de *de);
int xh_calib_de_step(xh_calib_de *de, int32_t ngen, double tol, double atol, double mut_lo, double mut_hi,
                     double recombination, int32_t *h_n_active);
int xh_calib_de_result(xh_calib_de *de, double *h_x, double *h_fun, int64_t *h_nfev, int32_t *h_nit,
                       int32_t *h_active);
int xh_calib_de_state(xh_calib_de *de, int32_t which, double *h_vectors, double *h_energy);
int xh_calib_de_set_state(xh_calib_de *de, const double *h_pop, const double *h_energy, int32_t generation);

/* ------------------------------------------------------------------ multi-GPU write-out (RCCL over xGMI)
 * The reference has no distributed path; BASELINE's north star shards the 235 basins over the GPUs of a node with a
 * single RCCL gather at write-out.  One process per GPU; the launcher (torchrun, mpirun, anything) starts the ranks
 * and carries the 128-byte id from rank 0 to the others.  RCCL is bound at run time (dlopen of librccl.so.1).
 *   xh_comm_unique_id   : ncclGetUniqueId (rank 0); len >= 128
 *   xh_comm_create      : ncclCommInitRank on the context's device (collective over all ranks)
 *   xh_comm_gather_rows : every rank contributes nvar device arrays [h_counts[rank], ncols] (h_d_local: host array of
 *                         nvar device pointers -- the pipeline's own output buffers, nothing is staged or padded on the
 *                         senders); grouped ncclSend / ncclRecv of the exact sizes on the context's stream.  On the root
 *                         d_perm [sum h_counts] (device) holds, rank-major, the destination row of every gathered row and
 *                         h_d_out the nvar device arrays [total rows, ncols] that receive them in grid order.
 *                         Asynchronous like every call: xh_sync to wait.                                       */
typedef struct xh_comm xh_comm;
int xh_comm_unique_id(char *id, size_t len);
int xh_comm_create(xh_ctx *ctx, int32_t nranks, int32_t rank, const char *id, size_t len, xh_comm **out);
void xh_comm_destroy(xh_comm *comm);
/*   xh_comm_info        : info[4] = {ranks, this rank, ncclSend calls, ncclRecv calls issued through this communicator so far}.
 *                         XH_COMM_SELF_LOOP=1 in the environment when a communicator is created (testing on a one-GPU box, with
 *                         the REAL librccl): the root also sends its OWN rows to itself -- ncclSend and ncclRecv to the own
 *                         rank inside the group, which RCCL allows -- so they take the whole data path of a remote rank's rows
 *                         (send kernel, receive into the staging area, row scatter to grid order) instead of the local short cut. */
int xh_comm_info(const xh_comm *comm, int64_t info[4]);
int xh_comm_gather_rows(xh_ctx *ctx, xh_comm *comm, int32_t root, int32_t nvar, const double *const *h_d_local,
                        int64_t ncols, const int64_t *h_counts, const int64_t *d_perm, double *const *h_d_out);
/*   xh_comm_gather_rows_side : the same gather on the context's gather stream (a hardware queue of its own), ordered behind
 *                         the kernels that produced the arrays -- everything enqueued on the context so far, or, right after
 *                         an xh_run_fused in mode 1, the side stream that completed PET / AET / Q / Sav while the routing
 *                         kernel already runs -- and beside whatever the context does next: the write-out of the four
 *                         arrays the routing does not touch travels over xGMI while the routing kernel runs.  Give this
 *                         stream a communicator of its own.
 *   xh_comm_join        : orders the context's stream behind the side gather (xh_sync and every other synchronising
 *                         call do so too).                                                                            */
int xh_comm_gather_rows_side(xh_ctx *ctx, xh_comm *comm, int32_t root, int32_t nvar, const double *const *h_d_local,
                             int64_t ncols, const int64_t *h_counts, const int64_t *d_perm, double *const *h_d_out);
int xh_comm_join(xh_ctx *ctx);

/* ------------------------------------------------------------------ bench support (not on the hot path)
 * Fills the eight forcing arrays of the synthetic benchmark world on the device (same distributions as
 * xanthos_amd/synth.py:make_forcing); d_lat [ncell] degrees; nan_frac = share of cells whose precipitation is NaN.
 * d_cell_ids [ncell] or NULL: GLOBAL cell index of each row (the random streams are keyed on it, so a rank can generate
 * just its shard of a world; -1 = no cell: a row of zeros).  With only d_tas non-NULL, only temperature is generated
 * (the tairprev rows of a shard: the previous GLOBAL cell's temperature, data_load.py:128-129).             */
int xh_synth_forcing(xh_ctx *ctx, uint64_t seed, double nan_frac, int64_t ncell, int32_t nmonths, const double *d_lat,
                     const int64_t *d_cell_ids, double *d_tas, double *d_tmin, double *d_rhs, double *d_wind, double *d_rsds,
                     double *d_rlds, double *d_precip, double *d_abcd_tmin);

#ifdef __cplusplus
}
#endif
#endif /* XANTHOS_HIP_H */
