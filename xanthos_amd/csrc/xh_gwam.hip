// Hargreaves PET and the GWAM water balance on gfx950 (fp64).
//
// Replaces xanthos/pet/hargreaves.py:calculate_pet (:17-73) with the input preparation of components.py:144-187
// (prep_arrays / prep_pet: nan_to_num of T and D) and data_load.py:83-84 (negative DTR -> 0), and
// xanthos/runoff/gwam.py:runoffgen (:18-88) driven month by month as components.py:298-384 drives it.
//
// Launches:
//   k_hg_lat          per cell: sin / cos / tan of the latitude (scratch), so the element kernel takes no trig of it
//   k_hargreaves_pet  one lane per (cell, month) element in C order: lane i takes element base + i (coalesced); the
//                     per-month sin / cos / tan of the declination, dr and the days of the month come from a small table
//   k_gwam_spinup     one thread per cell marches months [0, spinup) from sm0 and keeps only the final soil moisture
//   k_gwam_tile       the k_abcd_tile data movement (xh_abcd.hip): one wave owns CPW cells and moves whole
//                     aligned 128-byte lines; 16-month tiles sit in LDS as [cell][17]; each row is shifted by
//                     s(c) = (c x nmonths) mod 16 months so that every global access is a full line.  Slot 0 holds PET and
//                     takes AET, slot 1 holds precipitation (monthly mode) and takes Q, slot 2 takes the soil moisture.
//
// The reference's GWAM driver reads ONE precipitation column for every month of a pass (components.py:230 passes
// self.P, which only the PET step loop sets, :334): column runoff_spinup - 1 in the spin-up pass, nmonths - 1 in the
// simulation.  A precipitation column >= 0 reproduces that (one value per cell, read once per pass); -1 reads month m's
// precipitation in month m (the intended model, opt-in).
#include <cmath>
#include <cstdint>
#include <vector>

#include "xh_launch.h"

namespace {

// ---------------------------------------------------------------------------------------------- Hargreaves
struct HgMonth {
    double sin_dec, cos_dec, tan_dec, dr, ndays;
};

__global__ void __launch_bounds__(256) k_hg_lat(int64_t ncell, const double *__restrict__ lat, double *__restrict__ trig) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    const double x = lat[c];
    trig[c] = sin(x);
    trig[ncell + c] = cos(x);
    trig[2 * ncell + c] = tan(x);
}

__device__ __forceinline__ double nan_to_num(double v) {       // np.nan_to_num: NaN -> 0, +-inf -> +-DBL_MAX
    if (v != v) return 0.0;
    if (v == INFINITY) return 1.7976931348623157e308;
    if (v == -INFINITY) return -1.7976931348623157e308;
    return v;
}

__global__ void __launch_bounds__(256) k_hargreaves_pet(int64_t n, int nmonths, int64_t ncell, const double *__restrict__ temp,
                                                        const double *__restrict__ dtr, const double *__restrict__ trig,
                                                        const HgMonth *__restrict__ tab, double *__restrict__ pet) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t c;
        int m;
        if (n <= 0xffffffffll) {                      // 32-bit quotient (the 0.5-degree grid has 40 M elements at 600 months)
            const uint32_t u = (uint32_t)i;
            c = u / (uint32_t)nmonths;
            m = (int)(u - (uint32_t)c * (uint32_t)nmonths);
        } else {
            c = i / nmonths;
            m = (int)(i - c * nmonths);
        }
        const HgMonth t = tab[m];
        const double sx = trig[c], cx = trig[ncell + c], tx = trig[2 * ncell + c];
        const double T = nan_to_num(temp[i]);                    // components.py:156-157, :178-179
        double D = nan_to_num(dtr[i]);
        D = D < 0.0 ? 0.0 : D;                                   // data_load.py:83-84, hargreaves.py:33
        const double arg = -tx * t.tan_dec;                      // hargreaves.py:52: -tan(X) * tan(Y)
        // hargreaves.py:55-73: arccos inside [-1, 1], pi below, 0 above; NaN matches no branch and stays 0
        const double ws = (arg <= 1.0 && arg >= -1.0) ? acos(arg) : (arg < -1.0 ? 3.141592653589793 : 0.0);
        const double ra = 15.392 * t.dr * (ws * sx * t.sin_dec + cx * t.cos_dec * sin(ws));     // :46
        const double evap = t.ndays * 0.0023 * ra * (T + 17.8) * sqrt(D);                         // :36
        pet[i] = evap < 0.0 ? 0.0 : evap;                        // np.maximum(evap, 0): NaN stays NaN
    }
}

// ---------------------------------------------------------------------------------------------- GWAM
// gwam.py:runoffgen (:18-88) for one cell and month.  Branches as the reference's index sets, NaN included: water bodies
// (Sm == indexing), then -- for Sm != 0 and Sm != indexing -- B >= Sm and B < Sm; a NaN B or Sm, and Sm == 0, match none
// and leave the three outputs 0.  np.minimum / np.maximum are spelled with their NaN behaviour (the first argument wins
// ties and NaN; a NaN second argument is returned).
__device__ __forceinline__ void gwam_month(double pet, double p, double sm, double chstor, double indexing, double k1,
                                           double &aet, double &q, double &sav) {
    aet = q = sav = 0.0;
    if (sm == indexing) {                                        // :54, :61-65
        const double d = p - pet;
        q = d > 0.0 ? d : 0.0;                                   // max(0, P - PET), NaN -> 0
        aet = p <= pet ? p : pet;                                // min(P, PET), NaN -> PET
        return;
    }
    if (sm == 0.0) return;                                       // :53 c0
    const double B = chstor + p - pet;                           // :43
    if (B >= sm) {                                               // :68-71
        q = B - sm;
        sav = sm;
        aet = pet;
    } else if (B < sm) {                                         // :73-86
        const double tmp3 = chstor + p;
        const double x = chstor / sm;
        const double tmp5 = (5.0 * chstor / sm - 2.0 * (x * x)) / 3.0;
        const double tmp6 = 1.0 <= tmp5 ? 1.0 : tmp5;
        const double tmp7 = pet * (0.1 >= tmp6 ? 0.1 : tmp6);
        double a = (tmp3 <= tmp7 || tmp3 != tmp3) ? tmp3 : tmp7;
        const double tmp8 = chstor * (1.0 - exp(-x)) / k1 + (p - a);
        double s = (sm <= tmp8 || sm != sm) ? sm : tmp8;
        if (s <= 0.0) {                                          // :83-85
            s = 0.0;
            a = p + chstor;
        }
        const double r = chstor + p - a - s;
        q = 0.0 >= r ? 0.0 : r;                                  // np.maximum(0, r): NaN stays NaN
        aet = a;
        sav = s;
    }
}

// spin-up: months [0, nsteps) from sm0, final soil moisture to sm_out (components.py:344-357 with runoff_num_steps = spinup)
__global__ void __launch_bounds__(64) k_gwam_spinup(int64_t ncell, int nmonths, int nsteps, int pcol, double indexing, double k1,
                                                    const double *__restrict__ pet, const double *__restrict__ precip,
                                                    const double *__restrict__ smax, const double *__restrict__ sm0,
                                                    double *__restrict__ sm_out) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    const int64_t row = c * (int64_t)nmonths;
    const double sm = smax[c];
    const double p1 = pcol >= 0 ? precip[row + pcol] : 0.0;
    double st = sm0[c];
    for (int m = 0; m < nsteps; ++m) {
        double a, q, s;
        gwam_month(pet[row + m], pcol >= 0 ? p1 : precip[row + m], sm, st, indexing, k1, a, q, s);
        st = s;
    }
    sm_out[c] = st;
}

constexpr int TMS = 16;            // months per LDS tile = one 128-byte line per row and array
constexpr int TLD = TMS + 1;       // padded row length (doubles)
constexpr int CPW = 32;            // cells per wave (two waves per SIMD)

template <bool MONTHLY>
__global__ void __launch_bounds__(64) k_gwam_tile(int64_t ncell, int nmonths, int pcol, double indexing, double k1,
                                                  const double *__restrict__ pet, const double *__restrict__ precip,
                                                  const double *__restrict__ smax, const double *__restrict__ sm0,
                                                  double *__restrict__ aet, double *__restrict__ q, double *__restrict__ sav,
                                                  double *__restrict__ sm_end) {
    constexpr int NP = CPW / 8;                          // copy passes per tile (8 rows each)
    constexpr int NIN = MONTHLY ? 2 : 1;                 // arrays read: PET (+ precipitation)
    __shared__ double T[3][CPW * TLD];
    const int lane = threadIdx.x;
    const int64_t cell0 = (int64_t)blockIdx.x * CPW;
    const double *__restrict__ src[2] = {pet, precip};
    double *__restrict__ dst[3] = {aet, q, sav};

    // ---- copy role: lane (r, k) = (lane / 8, lane % 8) moves 16-byte chunk k of row r (+ 8 rows per pass)
    const int ck = lane & 7, cr = lane >> 3;
    int64_t crow[NP];                                    // element offset of the row, or -1
    int cshift[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int64_t c = cell0 + p * 8 + cr;
        crow[p] = c < ncell ? c * (int64_t)nmonths : -1;
        cshift[p] = c < ncell ? (int)((c * (int64_t)nmonths) & (TMS - 1)) : 0;
    }
    const int ntiles = (nmonths + (TMS - 2) + TMS - 1) / TMS;
    double2 R[NIN][NP];
    auto load_tile = [&](int t) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int m = t * TMS - cshift[p] + 2 * ck;   // first of the chunk's two months
            const bool ok = crow[p] >= 0 && m >= 0 && m < nmonths;
#pragma unroll
            for (int a = 0; a < NIN; ++a)
                R[a][p] = ok ? *reinterpret_cast<const double2 *>(src[a] + crow[p] + m) : make_double2(0.0, 0.0);
        }
    };

    // ---- compute role: lanes < CPW march their cell
    const int64_t c = cell0 + lane;
    const bool mine = lane < CPW && c < ncell;
    const int64_t cc = mine ? c : (ncell - 1);
    const int shift = (int)((cc * (int64_t)nmonths) & (TMS - 1));
    const double sm = smax[cc];
    const double p1 = MONTHLY ? 0.0 : precip[cc * (int64_t)nmonths + pcol];
    double st = sm0[cc];
    const int lrow = (lane < CPW ? lane : 0) * TLD;

    load_tile(0);
    for (int t = 0; t < ntiles; ++t) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int o = (p * 8 + cr) * TLD + 2 * ck;
#pragma unroll
            for (int a = 0; a < NIN; ++a) {
                T[a][o] = R[a][p].x;
                T[a][o + 1] = R[a][p].y;
            }
        }
        if (t + 1 < ntiles) load_tile(t + 1);            // in flight while this tile is computed
        __syncthreads();
        if (mine) {
            const int mbase = t * TMS - shift;
#pragma unroll
            for (int j = 0; j < TMS; ++j) {
                const int m = mbase + j;
                if (m >= 0 && m < nmonths) {
                    double a, qq, s;
                    gwam_month(T[0][lrow + j], MONTHLY ? T[1][lrow + j] : p1, sm, st, indexing, k1, a, qq, s);
                    st = s;
                    T[0][lrow + j] = a;
                    T[1][lrow + j] = qq;
                    T[2][lrow + j] = s;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int m = t * TMS - cshift[p] + 2 * ck;
            if (crow[p] >= 0 && m >= 0 && m < nmonths) {
                const int o = (p * 8 + cr) * TLD + 2 * ck;
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    if (dst[a]) *reinterpret_cast<double2 *>(dst[a] + crow[p] + m) = make_double2(T[a][o], T[a][o + 1]);
            }
        }
        __syncthreads();
    }
    if (mine && sm_end) sm_end[c] = st;
}

}  // namespace

extern "C" int xh_hargreaves_pet(xh_ctx *ctx, int64_t ncell, int32_t nmonths, const double *d_temp, const double *d_dtr,
                                 const double *d_lat_rad, const double *h_solar_dec, const double *h_dr,
                                 const double *h_ndays, double *d_pet) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, ncell >= 0 && nmonths > 0, "xh_hargreaves_pet: bad size");
    XH_REQUIRE(ctx, d_temp && d_dtr && d_lat_rad && h_solar_dec && h_dr && h_ndays && d_pet, "xh_hargreaves_pet: NULL argument");
    if (ncell == 0) return XH_OK;
    // the per-month factors of the declination on the host (libm), as the reference takes them of a numpy scalar
    std::vector<HgMonth> tab(nmonths);
    for (int m = 0; m < nmonths; ++m)
        tab[m] = HgMonth{std::sin(h_solar_dec[m]), std::cos(h_solar_dec[m]), std::tan(h_solar_dec[m]), h_dr[m], h_ndays[m]};
    void *at[2];
    const int rc = xh_stage(ctx, 2, {{tab.data(), sizeof(HgMonth) * nmonths}}, sizeof(double) * 3 * ncell, at);
    if (rc) return rc;
    const HgMonth *d_tab = static_cast<const HgMonth *>(at[0]);
    double *d_trig = static_cast<double *>(at[1]);
    const int64_t n = ncell * (int64_t)nmonths;
    return xh_timed(ctx, "hargreaves_pet", ctx->stream, [&] {
        const int rc = xh_launch(ctx, nullptr, ctx->stream, k_hg_lat, xh_grid(ctx, ncell, 256), 256, 0, ncell, d_lat_rad, d_trig);
        if (rc) return rc;
        return xh_launch(ctx, nullptr, ctx->stream, k_hargreaves_pet, xh_grid(ctx, n, 256, 32), 256, 0, n, (int)nmonths, ncell,
                         d_temp, d_dtr, d_trig, d_tab, d_pet);
    });
}

extern "C" int xh_gwam(xh_ctx *ctx, int64_t ncell, int32_t nmonths, int32_t spinup, int32_t precip_col_spinup,
                       int32_t precip_col_sim, double indexing, const double *d_pet, const double *d_precip,
                       const double *d_sm_max, const double *d_sm0, double *d_aet, double *d_q, double *d_sav,
                       double *d_sm_end) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, ncell >= 0 && nmonths > 0 && nmonths % 2 == 0, "xh_gwam: nmonths (%d) must be positive and even", nmonths);
    XH_REQUIRE(ctx, spinup >= 0 && spinup <= nmonths, "xh_gwam: spin-up (%d) outside [0, nmonths = %d]", spinup, nmonths);
    XH_REQUIRE(ctx, precip_col_spinup >= -1 && precip_col_spinup < nmonths && precip_col_sim >= -1 && precip_col_sim < nmonths,
               "xh_gwam: precipitation column outside [-1, nmonths)");
    XH_REQUIRE(ctx, d_pet && d_precip && d_sm_max && d_sm0, "xh_gwam: NULL argument");
    XH_REQUIRE(ctx,
               xh_aligned16(d_pet) && xh_aligned16(d_precip) && xh_aligned16(d_aet) && xh_aligned16(d_q) && xh_aligned16(d_sav),
               "xh_gwam: [ncell, nmonths] arrays must be 16-byte aligned");
    if (ncell == 0) return XH_OK;
    const double k1 = 1.0 - std::exp(-1.0);              // gwam.py:80: 1 - exp(-alpha), alpha = 1
    const double *sm_start = d_sm0;
    if (spinup > 0) {
        void *buf = nullptr;
        int rc = xh_scratch(ctx, 2, sizeof(double) * ncell, &buf);
        if (rc) return rc;
        double *d_state = static_cast<double *>(buf);
        rc = xh_launch(ctx, "gwam_spinup", ctx->stream, k_gwam_spinup, xh_grid(ctx, ncell, 64), 64, 0, ncell, (int)nmonths,
                       (int)spinup, (int)precip_col_spinup, indexing, k1, d_pet, d_precip, d_sm_max, d_sm0, d_state);
        if (rc) return rc;
        sm_start = d_state;
    }
    return xh_launch(ctx, "gwam_sim", ctx->stream, precip_col_sim < 0 ? k_gwam_tile<true> : k_gwam_tile<false>,
                     xh_grid(ctx, ncell, CPW), 64, 0, ncell, (int)nmonths, (int)precip_col_sim, indexing, k1, d_pet, d_precip,
                     d_sm_max, sm_start, d_aet, d_q, d_sav, d_sm_end);
}
