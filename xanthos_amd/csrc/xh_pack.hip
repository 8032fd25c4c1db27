// The body of a NetCDF-classic variable from HBM (data_writer/out_writer.py, OutputFormat 0).
//
// The reference's save_netcdf (out_writer.py:196-223) assigns the [nrows, ncols] float64 array to an 'f4' variable of
// scipy's netcdf_file, which writes it as numpy's a.astype('>f4').tobytes(): every value narrowed to IEEE binary32, round
// to nearest even (overflow to +/-inf, binary32 subnormals kept, the sign of zero kept, NaN stays NaN), most significant
// byte first, row-major.  k_pack_f32_be forms those bytes in HBM, so that half of the array's bytes cross PCIe
// (xh_download_files) and no host core converts 40 M values.
//
// The narrowing is v_cvt_f32_f64 under the kernel's float mode: both rounding modes are nearest even, and subnormal
// binary32 results are kept (the kernel descriptor has float_denorm_mode_32 = 3; hipcc flushes only when a translation
// unit is built with -fgpu-flush-denormals-to-zero, which the Makefile does not do) -- tests/test_gpu_outfmt.py has 1e-40,
// 1e-45 and 7e-46 among its values.  The byte swap is one v_perm_b32 per value.
//
// Bandwidth-bound, 12 bytes per value: a lane takes 4 consecutive doubles (two 16-byte loads; when the source is only
// 8-byte aligned -- a row slice of an array with an odd number of columns -- a variant that reads them as four doubles and
// leaves the width of the loads to the compiler) and issues one 16-byte store.
#include "xh_launch.h"

namespace {

__device__ __forceinline__ uint32_t f32_be(double v) { return __builtin_bswap32(__float_as_uint((float)v)); }

template <bool ALIGNED16>
__global__ void __launch_bounds__(256) k_pack_f32_be(const double *__restrict__ src, int64_t n, uint32_t *__restrict__ dst) {
    const int64_t nquads = n >> 2;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    uint4 *__restrict__ out = reinterpret_cast<uint4 *>(dst);
    for (int64_t q = first; q < nquads; q += stride) {
        double v0, v1, v2, v3;
        if (ALIGNED16) {
            const double2 a = reinterpret_cast<const double2 *>(src)[2 * q], b = reinterpret_cast<const double2 *>(src)[2 * q + 1];
            v0 = a.x, v1 = a.y, v2 = b.x, v3 = b.y;
        } else {
            v0 = src[4 * q], v1 = src[4 * q + 1], v2 = src[4 * q + 2], v3 = src[4 * q + 3];
        }
        out[q] = make_uint4(f32_be(v0), f32_be(v1), f32_be(v2), f32_be(v3));
    }
    const int64_t tail = 4 * nquads + first;          // the n % 4 values behind the last whole quad
    if (first < 4 && tail < n) dst[tail] = f32_be(src[tail]);
}

}  // namespace

extern "C" int xh_pack_f32_be(xh_ctx *ctx, const double *d_src, int64_t n, void *d_dst) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, n >= 0 && ((d_src && d_dst) || n == 0), "xh_pack_f32_be: bad argument");
    XH_REQUIRE(ctx, ((uintptr_t)d_src & 7) == 0 && xh_aligned16(d_dst),
               "xh_pack_f32_be: the source must be 8-byte and the destination 16-byte aligned");
    if (n == 0) return XH_OK;
    const unsigned blocks = xh_grid(ctx, n >> 2, 256, 16);
    return xh_launch(ctx, "pack_f32_be", ctx->stream, xh_aligned16(d_src) ? k_pack_f32_be<true> : k_pack_f32_be<false>,
                     blocks ? blocks : 1u, 256, 0, d_src, n, static_cast<uint32_t *>(d_dst));
}
