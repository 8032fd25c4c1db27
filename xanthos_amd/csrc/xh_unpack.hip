// Forcing as it is stored -> native doubles in HBM: the reader-side counterpart of xh_pack.hip.
//
// The forcing files people hand to the model are rarely float64: NetCDF-classic `float` variables are big-endian binary32
// (numpy '>f4'), NetCDF `double` is big-endian binary64 ('>f8'), and a .npy saved as float32 halves the disk.  The loader
// used to byte-swap and widen them on the host (data_load.py), after which 8 bytes per value crossed PCIe; now the stored
// bytes cross (pipeline.py set_forcing) and k_widen_f32 / k_swap_f64 make numpy's a.astype(np.float64) of them in HBM.
//
// binary32 -> binary64 is exact, so there is one right answer per input: v_cvt_f64_f32 under the kernel's float mode, which
// keeps binary32 subnormals as inputs (the kernel descriptor has float_denorm_mode_32 = 3; hipcc flushes only when a
// translation unit is built with -fgpu-flush-denormals-to-zero, which the Makefile does not do), the sign of zero and both
// infinities; the quiet NaN 0x7fc00000 becomes 0x7ff8000000000000 and every other NaN stays a NaN (nothing downstream
// reads payloads: xh_nan_to_num or the kernels' own isnan follow).  '>f8' is a byte swap and keeps every bit pattern.
//
// Bandwidth-bound, 12 bytes per binary32 value: a lane takes 4 consecutive values (one 16-byte load, two 16-byte stores;
// two and two for '>f8').  When the source is only element-aligned or the destination only 8-byte aligned -- a row slice of
// an array with an odd number of columns -- a variant that moves them one by one and leaves the widths to the compiler.
#include "xh_launch.h"

namespace {

template <bool BE>
__device__ __forceinline__ double widen32(uint32_t bits) {
    return (double)__uint_as_float(BE ? __builtin_bswap32(bits) : bits);
}

template <bool BE, bool ALIGNED16>
__global__ void __launch_bounds__(256) k_widen_f32(const uint32_t *__restrict__ src, int64_t n, double *__restrict__ dst) {
    const int64_t nquads = n >> 2;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = first; q < nquads; q += stride) {
        if (ALIGNED16) {
            const uint4 v = reinterpret_cast<const uint4 *>(src)[q];
            double2 *__restrict__ out = reinterpret_cast<double2 *>(dst);
            out[2 * q] = make_double2(widen32<BE>(v.x), widen32<BE>(v.y));
            out[2 * q + 1] = make_double2(widen32<BE>(v.z), widen32<BE>(v.w));
        } else {
            const uint32_t v0 = src[4 * q], v1 = src[4 * q + 1], v2 = src[4 * q + 2], v3 = src[4 * q + 3];
            dst[4 * q] = widen32<BE>(v0), dst[4 * q + 1] = widen32<BE>(v1);
            dst[4 * q + 2] = widen32<BE>(v2), dst[4 * q + 3] = widen32<BE>(v3);
        }
    }
    const int64_t tail = 4 * nquads + first;          // the n % 4 values behind the last whole quad
    if (first < 4 && tail < n) dst[tail] = widen32<BE>(src[tail]);
}

// (no __restrict__: the swap may run in place, every lane then reads its four values before it writes them)
template <bool ALIGNED16>
__global__ void __launch_bounds__(256) k_swap_f64(const uint64_t *src, int64_t n, uint64_t *dst) {
    const int64_t nquads = n >> 2;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = first; q < nquads; q += stride) {
        uint64_t v0, v1, v2, v3;
        if (ALIGNED16) {
            const ulong2 a = reinterpret_cast<const ulong2 *>(src)[2 * q], b = reinterpret_cast<const ulong2 *>(src)[2 * q + 1];
            v0 = a.x, v1 = a.y, v2 = b.x, v3 = b.y;
        } else {
            v0 = src[4 * q], v1 = src[4 * q + 1], v2 = src[4 * q + 2], v3 = src[4 * q + 3];
        }
        v0 = __builtin_bswap64(v0), v1 = __builtin_bswap64(v1), v2 = __builtin_bswap64(v2), v3 = __builtin_bswap64(v3);
        if (ALIGNED16) {
            reinterpret_cast<ulong2 *>(dst)[2 * q] = make_ulong2(v0, v1);
            reinterpret_cast<ulong2 *>(dst)[2 * q + 1] = make_ulong2(v2, v3);
        } else {
            dst[4 * q] = v0, dst[4 * q + 1] = v1, dst[4 * q + 2] = v2, dst[4 * q + 3] = v3;
        }
    }
    const int64_t tail = 4 * nquads + first;
    if (first < 4 && tail < n) dst[tail] = __builtin_bswap64(src[tail]);
}

}  // namespace

extern "C" int xh_widen(xh_ctx *ctx, const void *d_src, int kind, int64_t n, double *d_dst) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, kind == XH_SRC_F32_LE || kind == XH_SRC_F32_BE || kind == XH_SRC_F64_BE,
               "xh_widen: unknown kind %d (1 float32, 2 big-endian float32, 3 big-endian float64)", kind);
    XH_REQUIRE(ctx, n >= 0 && ((d_src && d_dst) || n == 0), "xh_widen: bad argument");
    const size_t width = kind == XH_SRC_F64_BE ? 8 : 4;
    XH_REQUIRE(ctx, ((uintptr_t)d_src & (width - 1)) == 0 && ((uintptr_t)d_dst & 7) == 0,
               "xh_widen: the source must be %d-byte and the destination 8-byte aligned", (int)width);
    if (n == 0) return XH_OK;
    const uintptr_t s = (uintptr_t)d_src, d = (uintptr_t)d_dst;
    const bool in_place = kind == XH_SRC_F64_BE && s == d;
    XH_REQUIRE(ctx, in_place || s + (uint64_t)n * width <= d || d + (uint64_t)n * 8 <= s,
               "xh_widen: the source and the destination overlap (only big-endian float64 may be swapped in place, with "
               "d_src == d_dst)");
    const bool aligned = xh_aligned16(d_src) && xh_aligned16(d_dst);
    unsigned blocks = xh_grid(ctx, n >> 2, 256, 16);
    if (!blocks) blocks = 1u;
    if (kind == XH_SRC_F64_BE)
        return xh_launch(ctx, "widen", ctx->stream, aligned ? k_swap_f64<true> : k_swap_f64<false>, blocks, 256, 0,
                         static_cast<const uint64_t *>(d_src), n, reinterpret_cast<uint64_t *>(d_dst));
    const uint32_t *src = static_cast<const uint32_t *>(d_src);
    if (kind == XH_SRC_F32_BE)
        return xh_launch(ctx, "widen", ctx->stream, aligned ? k_widen_f32<true, true> : k_widen_f32<true, false>, blocks, 256,
                         0, src, n, d_dst);
    return xh_launch(ctx, "widen", ctx->stream, aligned ? k_widen_f32<false, true> : k_widen_f32<false, false>, blocks, 256, 0,
                     src, n, d_dst);
}
