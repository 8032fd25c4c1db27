// The body of a gridded NetCDF-classic 'f4' variable [time, lat, lon] from HBM (data_writer/gridded.py, GriddedOutput = 1).
//
// The writer's arrays are the reference's per-cell tables: [ncell, ncols], time fastest, rows in the order of
// coordinates.csv.  A map wants [ncols, nslots] with nslots = ngridrow * ngridcol, longitude fastest, and a fill value
// where no cell lies.  The reference has no such output; on the host it is a download of the array, a fancy-indexed
// scatter of ncell * ncols values into a cube of nslots * ncols and a narrowing pass.  k_grid_pack forms the cube's bytes
// in HBM: dst[t, s] = fill when cell_of_slot[s] < 0 or the value is NaN, otherwise numpy's astype('>f4') of
// src[cell_of_slot[s], t], narrowed exactly as k_pack_f32_be does (xh_pack.hip: v_cvt_f32_f64 under the kernel's float
// mode, nearest even, overflow to +/-inf, binary32 subnormals kept, the sign of zero kept; one v_perm_b32 swaps the bytes).
//
// A gather-transpose: the source runs along time, the destination along the slots.  One workgroup takes a tile of
// TILE slots x TILE time steps through LDS.
//   read : one wave per slot, its 64 lanes on 64 consecutive months of that cell's row -- a 512-byte run of 8-byte loads
//          (a row of an array with an odd ncols is only 8-byte aligned, so nothing wider is asked for, as in
//          k_pack_f32_be<false>).  The narrowed, swapped word goes to tile[slot][month]: consecutive lanes on consecutive
//          banks.
//   write: one wave per month, its 64 lanes on 64 consecutive slots -- a 256-byte run of 4-byte stores.  The lanes read
//          tile[lane][month], a column: with rows of TILE + 1 words the 32 lanes of a ds_read_b32 group fall on 32
//          different banks (k_transpose's padding, for 4-byte words).
// The 64 table entries of the tile are read once, by the first wave.  When all are negative (74 % of the slots of a
// global 0.5-degree land grid are ocean, and mostly in whole tiles) the workgroup stores the fill value and reads nothing
// else.  Bytes moved at the least: 8 ncell ncols read + 4 nslots ncols written, and the table once per time tile.
#include "xh_launch.h"

namespace {

constexpr int TILE = 64;

__global__ void __launch_bounds__(256) k_grid_pack(const double *__restrict__ src, int64_t ncols,
                                                   const int32_t *__restrict__ cell_of_slot, int64_t nslots,
                                                   uint32_t fill_be, uint32_t *__restrict__ dst) {
    __shared__ uint32_t tile[TILE][TILE + 1];
    __shared__ int32_t cells[TILE];
    const int64_t s0 = (int64_t)blockIdx.x * TILE, t0 = (int64_t)blockIdx.y * TILE;
    const int tx = threadIdx.x & (TILE - 1), ty = threadIdx.x >> 6;      // 64 x 4: a wave per row of the tile

    int32_t c = -1;
    if (ty == 0) {
        if (s0 + tx < nslots) c = cell_of_slot[s0 + tx];
        cells[tx] = c;
    }
    const bool land = __syncthreads_or(c >= 0);                          // (also: cells[] is visible)

    constexpr int PER = TILE / 4;                                        // rows of the tile per wave
    if (!land) {                                                         // ocean: nothing is read but the table
        if (s0 + tx < nslots)
#pragma unroll
            for (int k = 0; k < PER; ++k)
                if (t0 + ty + 4 * k < ncols) dst[(t0 + ty + 4 * k) * nslots + s0 + tx] = fill_be;
        return;
    }
    // Every load of the wave's 16 rows is issued before the first is waited for: a lane without a value of its own (a
    // slot without a cell in a tile that has some, a month behind the last) reads a value that exists -- its clamped month
    // of cell 0, a line the cache holds -- and drops it.
    const bool t_in = t0 + tx < ncols;
    const int64_t t = t_in ? t0 + tx : ncols - 1;
    double v[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int32_t cj = cells[ty + 4 * k];
        v[k] = src[(int64_t)(cj >= 0 ? cj : 0) * ncols + t];
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const bool has = cells[ty + 4 * k] >= 0 && t_in && v[k] == v[k];
        tile[ty + 4 * k][tx] = has ? __builtin_bswap32(__float_as_uint((float)v[k])) : fill_be;
    }
    __syncthreads();
    uint32_t w[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) w[k] = tile[tx][ty + 4 * k];
    if (s0 + tx >= nslots) return;
#pragma unroll
    for (int k = 0; k < PER; ++k)
        if (t0 + ty + 4 * k < ncols) dst[(t0 + ty + 4 * k) * nslots + s0 + tx] = w[k];
}

}  // namespace

extern "C" int xh_grid_pack_f32_be(xh_ctx *ctx, const double *d_src, int64_t ncell, int64_t ncols,
                                   const int32_t *d_cell_of_slot, int64_t nslots, uint32_t fill_bits, void *d_dst) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, d_src && d_cell_of_slot && d_dst && ncell >= 1 && nslots >= 1 && ncols >= 0,
               "xh_grid_pack_f32_be: bad argument");
    XH_REQUIRE(ctx, ((uintptr_t)d_src & 7) == 0 && ((uintptr_t)d_dst & 15) == 0,
               "xh_grid_pack_f32_be: the source must be 8-byte and the destination 16-byte aligned");
    if (ncols == 0) return XH_OK;
    const int64_t slot_tiles = (nslots + TILE - 1) / TILE, time_tiles = (ncols + TILE - 1) / TILE;
    XH_REQUIRE(ctx, slot_tiles <= 0x7fffffff && time_tiles <= 65535, "xh_grid_pack_f32_be: too many slots or time steps");
    return xh_launch(ctx, "grid_pack", ctx->stream, k_grid_pack, dim3((unsigned)slot_tiles, (unsigned)time_tiles), 256, 0,
                     d_src, ncols, d_cell_of_slot, nslots, __builtin_bswap32(fill_bits), static_cast<uint32_t *>(d_dst));
}
