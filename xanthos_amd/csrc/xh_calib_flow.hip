// Streamflow calibration objective on gfx950 (set_calibrate = 1).
//
// The objective of a parameter vector p for basin B: ABCD on B's cells as the runoff objective runs it,
// the runoff scattered onto B's upstream closure through UM (cells of the closure outside B carry zero runoff), MRTM
// over the closure -- routing_spinup months, then all months with the carried storage -- and the sum of Avg_ChFlow
// over B's outlets, scored with ED = 1 - KGE.  Only the closure can reach the outlets, so every (basin, member) routes
// its own closure and never the world, and every such routing is independent of every other: a population of every
// basin fills the chip, where the one-world routing kernel is latency-bound.
//
//   spin-up      xh_calib_spinup_enqueue (xh_calib.hip, the runoff objective's kernels unchanged): sm0, gw0 per
//                (basin, member)
//   k_calib_flow one workgroup per (closure, block of members); lanes <-> (member, closure cell), CPL cells per lane.
//                Each month: the ABCD step of the lane's basin cells (state in registers, nothing stored), then the
//                month's 8 nday routing sub-steps with F double-buffered in LDS.  A sub-step gathers UM F from one
//                buffer, computes the trial storage and writes the NEXT sub-step's F = S tau^-1 into the other buffer
//                before its one barrier; a cell that fires (dSdt dt < -S, mrtm.py:54) raises a flag, and only when the
//                flag is up after the barrier does the workgroup take the reference's second pass (fired cells'
//                F = dSdt + F + S / dt, S = 0, a second gather for the others, mrtm.py:56-69) and rewrite the next F.
//                A cell none of whose terms changed gathers the same bits twice, so the flag's reach (the workgroup
//                instead of the reference's world) does not change a bit.  At the month's end the outlets' Avg_ChFlow
//                go to LDS and one lane per member sums them in ascending cell order into series[basin][member][month].
//                The launch classes (closure sizes) run concurrently: class 0 on the context's stream, the others on
//                streams of their own, forked after the spin-up and joined before the KGE.
//   k_calib_kge  (xh_calib.hip) ED per (basin, member)
//
// Gauge form (xh_calib_gauge_desc): the basin is scored at stream gauges on cells inside the network instead of at its
// outlets.  The closure is the UNION of the gauges' upstream closures (a subset of the outlet closure), routed once per
// member by the same kernel -- same launch classes, LDS double buffer, one-barrier sub-step and flag protocol; ABCD runs
// on the basin cells the closure holds.  There is no outlet stage: the lane that owns a gauge cell writes its
// Avg_ChFlow = favg / nt straight to series[gauge][member][month] in the simulation pass, so the outlet sums' LDS
// share and the two barriers per month around it go.  k_calib_kge_masked then scores every (gauge, member) over the
// months with a finite observation and k_calib_gauge_combine forms the basin's weighted mean (xh_calib.hip).
//
// Velocity form (xh_calib_velocity_desc, either form above): a member's row of parameters carries one more gene behind
// the ABCD genes, the velocity scale v > 0 of its basin.  The instantiations with VEL route the basin's own cells with
// tau^-1 = (v ChV) / L -- the product first, then the IEEE quotient, as mrtm.py:42 forms it on a scaled ChV -- and the
// closure's foreign cells with the table's ChV / L: those belong to another basin's calibration.  v is read once per
// (basin, member) and tau stays in the lane's registers, so nothing else of the sub-step changes.  (1.0 ChV) / L has the
// bits of ChV / L: v = 1 returns the series of the instantiations without VEL, which are compiled as before.
//
// Everything is fp64 in the reference's operation order (-ffp-contract=off), summation orders are fixed, outputs are
// written once: results are bit-identical run to run.
#include <algorithm>
#include <cmath>
#include <vector>

#include "xh_abcd_dev.h"
#include "xh_calib.h"
#include "xh_launch.h"

namespace {

using namespace xh_abcd_dev;

constexpr int MAX_CLOSURE = 3072;            // cells of one closure (the largest class: 1024 threads x 3 cells)
constexpr size_t LDS_LIMIT = 160 * 1024;     // per workgroup on gfx950

struct FlowBasin {
    int nc, cell0, nout, tpm, mpw, klass;    // closure cells, first row, outlets, threads per member, members per group
    int64_t e0;                              // first entry of the closure's rows
    int nnz, g1;                             // gauge form: nout = the basin's gauges, g1 = one past its last gauge
};

// launch classes: threads per workgroup x cells per lane
struct Klass {
    int bt, cpl, lo, hi;                     // closures of (lo, hi] cells
};
constexpr Klass KLASSES[] = {{64, 1, 0, 64}, {256, 1, 64, 256}, {256, 2, 256, 512}, {256, 4, 512, 1024},
                             {1024, 3, 1024, MAX_CLOSURE}};
constexpr int NKLASS = 5;

// UM F of one row from LDS: 0 + sum of +-F[col] in stored order (scipy's csr_matvec; the entry holds col or ~col)
__device__ __forceinline__ double gather(const int *__restrict__ ent, int e_lo, int e_hi, const double *__restrict__ F) {
    double g = 0.0;
    for (int e = e_lo; e < e_hi; ++e) {
        const int v = ent[e];
        g = v >= 0 ? g + F[v] : g - F[~v];
    }
    return g;
}

// GAUGE: g_orank holds, per closure row, the first gauge on that cell (index into the problem's gauges, which are sorted
// by cell within a basin) or -1, g_grow the closure-local row of every gauge, and series is [gauge][member][month].
// VEL: pars rows are [npar ABCD genes, v]; g_chv, g_len [closure row] = ChV and L (else unused, NULL).
template <int BT, int CPL, bool GAUGE, bool VEL>
__global__ void __launch_bounds__(BT) k_calib_flow(const xh_calib_basin *__restrict__ basins,
                                                   const FlowBasin *__restrict__ fbs, const int2 *__restrict__ work,
                                                   const int *__restrict__ active, int nmonths, int rspin, double dt,
                                                   const int *__restrict__ ndays, const int *__restrict__ nts,
                                                   int nmembers, int npar, const double *__restrict__ pars,
                                                   const double *__restrict__ sm0, const double *__restrict__ gw0,
                                                   const int64_t *__restrict__ row_ptr, const int *__restrict__ g_ent,
                                                   const double *__restrict__ g_tau, const double *__restrict__ g_area,
                                                   const double *__restrict__ g_s0, const int *__restrict__ g_bcol,
                                                   const int *__restrict__ g_orank, const int *__restrict__ g_grow,
                                                   double *__restrict__ series, const double *__restrict__ g_chv,
                                                   const double *__restrict__ g_len) {
    extern __shared__ double lds[];
    const int2 wk = work[blockIdx.x];
    const int b = wk.x;
    if (active && !active[b]) return;                                // workgroup-uniform
    const FlowBasin FB = fbs[b];
    const xh_calib_basin B = basins[b];
    const int nc = FB.nc, tpm = FB.tpm, mpw = FB.mpw, nout = FB.nout;
    const int t = threadIdx.x;
    const int mloc = t / tpm, lane = t - mloc * tpm;
    const int mem = wk.y + mloc;
    const bool mem_ok = mem < nmembers;
    const int row = b * nmembers + min(mem, nmembers - 1);

    double *Fbuf = lds;                                              // [2][mpw][nc]
    double *outv = lds + 2 * mpw * nc;                               // [mpw][nout] (outlet form only)
    int *ent = reinterpret_cast<int *>(outv + (GAUGE ? 0 : mpw * nout));   // [nnz]
    int *flag = ent + FB.nnz;                                        // [3]
    for (int e = t; e < FB.nnz; e += BT) ent[e] = g_ent[FB.e0 + e];
    if (t < 3) flag[t] = 0;

    const bool snow_on = B.tn != nullptr;
    const int pstride = VEL ? npar + 1 : npar;
    const AbcdPar P = calib_par(pars, pstride, npar, row);
    const double vscale = VEL ? pars[(int64_t)row * pstride + npar] : 1.0;
    const XhExpConsts K = xh_exp_consts();
    const double sm_init = sm0[row], gw_init = gw0[row];
    const double dtinv = 1.0 / dt;

    bool own[CPL];
    int ci[CPL], e_lo[CPL], e_hi[CPL], bcol[CPL], gfirst[CPL];
    double S[CPL], F[CPL], tau[CPL], erl[CPL], favg[CPL];
    AbcdState st[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int i = lane + k * tpm;
        own[k] = i < nc;
        ci[k] = own[k] ? i : 0;
        const int c = FB.cell0 + ci[k];
        e_lo[k] = own[k] ? (int)(row_ptr[c] - FB.e0) : 0;
        e_hi[k] = own[k] ? (int)(row_ptr[c + 1] - FB.e0) : 0;
        bcol[k] = own[k] ? g_bcol[c] : -1;
        gfirst[k] = (GAUGE && own[k]) ? g_orank[c] : -1;
        tau[k] = own[k] ? g_tau[c] : 0.0;
        if constexpr (VEL)
            if (bcol[k] >= 0) tau[k] = (vscale * g_chv[c]) / g_len[c];           // mrtm.py:42 on the basin's scaled ChV
        S[k] = own[k] ? g_s0[c] : 0.0;
        F[k] = S[k] * tau[k];
        erl[k] = favg[k] = 0.0;
    }
    // F of this member in buffer p: Fbuf + (p mpw + mloc) nc
    const int fstride = mpw * nc;
    double *Fmine = Fbuf + mloc * nc;
    int par = 0;
#pragma unroll
    for (int k = 0; k < CPL; ++k)
        if (own[k]) Fmine[ci[k]] = F[k];
    __syncthreads();

    unsigned gs = 0;                                                 // sub-steps so far: the flag slot is gs % 3
    for (int pass = 0; pass < 2; ++pass) {
        const int nmon = pass ? nmonths : rspin;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {                              // every pass starts ABCD from the month-0 state
            st[k].snowpack = 0.0;
            st[k].sm = sm_init;
            st[k].gw = gw_init;
        }
        for (int m = 0; m < nmon; ++m) {
            const int nday = ndays[m], nt = nts[m];
            const double secs = (double)((int64_t)nday * 86400);     // nday * 24 * 3600 (mrtm.py:38)
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                double q = 0.0;                                      // rsim = 0 outside the basin
                if (bcol[k] >= 0) {
                    const int64_t o = (int64_t)m * B.ncell + bcol[k];
                    const AbcdPre pre = abcd_pre(P, K, snow_on, B.pet[o], B.pr[o], snow_on ? B.tn[o] : 0.0);
                    double aet;
                    abcd_step(P, st[k], snow_on, m == 0, pre, aet, q);
                }
                erl[k] = own[k] ? ((q * g_area[FB.cell0 + ci[k]]) * 1000.0) / secs : 0.0;   // (q area) (1e6 / 1e3) / s
                favg[k] = 0.0;
            }
            for (int s = 0; s < nt; ++s, ++gs) {
                double *Fc = Fmine + par * fstride;
                double *Fn = Fmine + (par ^ 1) * fstride;
                bool fire[CPL];
                double dsdt[CPL], Sn[CPL];
                bool any = false;
#pragma unroll
                for (int k = 0; k < CPL; ++k) {
                    fire[k] = false;
                    dsdt[k] = 0.0;
                    Sn[k] = S[k];
                    if (own[k]) {
                        dsdt[k] = gather(ent, e_lo[k], e_hi[k], Fc) + erl[k];     // UM.dot(F) + erlateral (:52)
                        const double d = dsdt[k] * dt;
                        fire[k] = d < -S[k];                                      // :54
                        Sn[k] = S[k] + d;                                         // :76
                        any = any || fire[k];
                        Fn[ci[k]] = Sn[k] * tau[k];                               // next sub-step's F (:50), if none fires
                    }
                }
                if (any) flag[gs % 3] = 1;
                if (t == 0) flag[(gs + 1) % 3] = 0;                  // read two sub-steps ago, written next sub-step
                __syncthreads();
                if (flag[gs % 3]) {                                  // workgroup-uniform
#pragma unroll
                    for (int k = 0; k < CPL; ++k)
                        if (fire[k]) {
                            F[k] = (dsdt[k] + F[k]) + S[k] * dtinv;                // :60
                            Fc[ci[k]] = F[k];
                            Sn[k] = 0.0;                                          // :63
                        }
                    __syncthreads();
#pragma unroll
                    for (int k = 0; k < CPL; ++k)
                        if (own[k] && !fire[k]) {
                            const double d2 = gather(ent, e_lo[k], e_hi[k], Fc) + erl[k];   // :66-67
                            Sn[k] = S[k] + d2 * dt;                               // :69
                        }
#pragma unroll
                    for (int k = 0; k < CPL; ++k)
                        if (own[k]) Fn[ci[k]] = Sn[k] * tau[k];
                    __syncthreads();
                }
#pragma unroll
                for (int k = 0; k < CPL; ++k) {
                    favg[k] += F[k];                                 // :78
                    S[k] = Sn[k];
                    F[k] = S[k] * tau[k];
                }
                par ^= 1;
            }
            if constexpr (GAUGE) {
                if (pass == 1 && mem_ok) {
#pragma unroll
                    for (int k = 0; k < CPL; ++k)
                        if (gfirst[k] >= 0) {                        // every gauge on this cell: Avg_ChFlow (:80), nothing summed
                            const double v = favg[k] / (double)nt;
                            for (int g = gfirst[k]; g < FB.g1 && g_grow[g] == ci[k]; ++g)
                                series[((int64_t)g * nmembers + mem) * nmonths + m] = v;
                        }
                }
            } else {
#pragma unroll
                for (int k = 0; k < CPL; ++k)
                    if (own[k]) {
                        const int r = g_orank[FB.cell0 + ci[k]];
                        if (r >= 0) outv[mloc * nout + r] = favg[k] / (double)nt;       // Avg_ChFlow (:80)
                    }
                __syncthreads();
                if (pass == 1 && lane == 0 && mem_ok) {
                    double sum = 0.0;
                    for (int r = 0; r < nout; ++r) sum += outv[mloc * nout + r];
                    series[((int64_t)b * nmembers + mem) * nmonths + m] = sum;
                }
                __syncthreads();                                     // outv is rewritten next month
            }
        }
    }
}

}  // namespace

struct xh_calib_flow {
    int nbasins = 0, nmonths = 0, nmembers = 0, rspin = 0;
    double dt = 0.0;
    void *d_buf = nullptr;
    FlowBasin *d_fb = nullptr;
    int64_t *d_row_ptr = nullptr;
    int *d_ent = nullptr, *d_bcol = nullptr, *d_orank = nullptr, *d_ndays = nullptr, *d_nt = nullptr;
    double *d_tau = nullptr, *d_area = nullptr, *d_s0 = nullptr;
    double *d_chv = nullptr, *d_len = nullptr;   // velocity form: ChV and L of every closure row (else NULL)
    // gauge form: d_orank holds the first gauge of each closure row; per gauge its closure-local row, basin and weight,
    // per basin its first gauge
    int ngauge = 0;                          // 0 = the outlet form
    int *d_grow = nullptr, *d_gbasin = nullptr, *d_gptr = nullptr;
    double *d_gw = nullptr;
    int2 *d_work = nullptr;
    int work0[NKLASS] = {0}, nwork[NKLASS] = {0};
    size_t lds[NKLASS] = {0};
    // classes 1..4 run on streams of their own beside class 0 on the context's stream: every class is a chain of all
    // the sub-steps, and one after another the classes would take (classes in use) x chain
    hipStream_t side[NKLASS] = {nullptr};
    hipEvent_t fork = nullptr, join[NKLASS] = {nullptr};
};

namespace {

template <int BT, int CPL, bool GAUGE, bool VEL>
int launch_form(xh_ctx *ctx, const xh_calib_problem &P, const xh_calib_flow &f, int kl, const double *d_pars,
                const int *d_active) {
    return xh_launch(ctx, nullptr, kl ? f.side[kl] : ctx->stream, k_calib_flow<BT, CPL, GAUGE, VEL>, dim3((unsigned)f.nwork[kl]), dim3(BT), f.lds[kl],
                     P.d_basins, f.d_fb, f.d_work + f.work0[kl], d_active, f.nmonths, f.rspin, f.dt, f.d_ndays, f.d_nt,
                     P.nmembers, P.npar, d_pars, P.d_sm0, P.d_gw0, f.d_row_ptr, f.d_ent, f.d_tau, f.d_area, f.d_s0,
                     f.d_bcol, f.d_orank, f.d_grow, P.d_series, f.d_chv, f.d_len);
}

template <int BT, int CPL>
int launch_klass(xh_ctx *ctx, const xh_calib_problem &P, const xh_calib_flow &f, int kl, const double *d_pars,
                 const int *d_active) {
    if (f.d_chv)
        return f.ngauge ? launch_form<BT, CPL, true, true>(ctx, P, f, kl, d_pars, d_active)
                        : launch_form<BT, CPL, false, true>(ctx, P, f, kl, d_pars, d_active);
    return f.ngauge ? launch_form<BT, CPL, true, false>(ctx, P, f, kl, d_pars, d_active)
                    : launch_form<BT, CPL, false, false>(ctx, P, f, kl, d_pars, d_active);
}

}  // namespace

void xh_calib_flow_destroy(xh_calib_flow *f) {
    if (!f) return;
    for (int kl = 0; kl < NKLASS; ++kl) {
        if (f->side[kl]) {
            (void)hipStreamSynchronize(f->side[kl]);
            (void)hipStreamDestroy(f->side[kl]);
        }
        if (f->join[kl]) (void)hipEventDestroy(f->join[kl]);
    }
    if (f->fork) (void)hipEventDestroy(f->fork);
    if (f->d_buf) (void)hipFree(f->d_buf);
    delete f;
}

namespace {

// the gauge part of an xh_calib_gauge_desc (NULL = the outlet form, whose desc carries h_outlet_rank)
struct GaugePart {
    const int64_t *ptr;
    const int32_t *row;
    const double *weight;
};

int flow_create(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, int32_t nmonths, int32_t nmembers,
                const xh_calib_flow_desc *d, const GaugePart *gp, const xh_calib_velocity_desc *vd, xh_calib_flow **out) {
    XH_REQUIRE(ctx, d && out && h_ncell, "xh_calib_flow: NULL argument");
    *out = nullptr;
    XH_REQUIRE(ctx, d->h_ndays && d->h_closure_ptr && d->h_row_ptr && d->h_cols && d->h_sign && d->h_basin_col &&
                        (gp || d->h_outlet_rank) && d->h_tauinv && d->h_area && d->h_s0,
               "xh_calib_flow: NULL table");
    XH_REQUIRE(ctx, !gp || (gp->ptr && gp->row && gp->weight), "xh_calib_flow: NULL gauge table");
    XH_REQUIRE(ctx, !vd || (vd->h_velocity && vd->h_length), "xh_calib_flow: NULL velocity table");
    const int64_t ngauge = gp ? gp->ptr[nbasins] : 0;
    XH_REQUIRE(ctx, !gp || (gp->ptr[0] == 0 && ngauge > 0 && ngauge < ((int64_t)1 << 24)), "xh_calib_flow: bad gauge_ptr");
    XH_REQUIRE(ctx, d->routing_spinup >= 0 && d->routing_spinup <= nmonths,
               "xh_calib_flow: routing_spinup = %d must lie in [0, nmonths = %d]", d->routing_spinup, nmonths);
    XH_REQUIRE(ctx, d->dt > 0.0, "xh_calib_flow: dt must be positive");
    const int64_t *cp = d->h_closure_ptr;
    XH_REQUIRE(ctx, cp[0] == 0, "xh_calib_flow: closure_ptr[0] must be 0");
    const int64_t ncl = cp[nbasins];
    const int64_t nnz = d->h_row_ptr[ncl];
    XH_REQUIRE(ctx, ncl > 0 && ncl < ((int64_t)1 << 30) && d->h_row_ptr[0] == 0 && nnz >= 0 && nnz < ((int64_t)1 << 30),
               "xh_calib_flow: bad table sizes");
    std::vector<int> nt(nmonths);
    for (int m = 0; m < nmonths; ++m) {
        XH_REQUIRE(ctx, d->h_ndays[m] > 0 && d->h_ndays[m] <= 31, "xh_calib_flow: month %d has %d days", m, d->h_ndays[m]);
        nt[m] = (int)((double)((int64_t)d->h_ndays[m] * 86400) / d->dt);      // int(nday * 24 * 3600 / dt) (mrtm.py:35)
        XH_REQUIRE(ctx, nt[m] >= 1, "xh_calib_flow: dt = %g leaves month %d without a sub-step", d->dt, m);
    }
    std::vector<FlowBasin> fb(nbasins);
    std::vector<int> ent(nnz > 0 ? nnz : 1);
    std::vector<int> gfirst(gp ? ncl : 0, -1), gbasin(ngauge), gptr(gp ? nbasins + 1 : 0);
    std::vector<std::vector<int2>> work(NKLASS);
    std::vector<size_t> lds(NKLASS, 0);
    for (int b = 0; b < nbasins; ++b) {
        const int64_t c0 = cp[b], c1 = cp[b + 1];
        XH_REQUIRE(ctx, c1 > c0, "xh_calib_flow: basin %d has an empty closure", b);
        const int64_t nc = c1 - c0;
        XH_REQUIRE(ctx, nc <= MAX_CLOSURE, "xh_calib_flow: the closure of basin %d has %lld cells, more than %d", b,
                   (long long)nc, MAX_CLOSURE);
        FlowBasin &B = fb[b];
        B.nc = (int)nc;
        B.cell0 = (int)c0;
        B.e0 = d->h_row_ptr[c0];
        B.nnz = (int)(d->h_row_ptr[c1] - B.e0);
        B.g1 = 0;
        int nout = 0, nbc = 0;
        for (int64_t c = c0; c < c1; ++c) {
            XH_REQUIRE(ctx, d->h_row_ptr[c + 1] >= d->h_row_ptr[c], "xh_calib_flow: row_ptr decreases");
            for (int64_t e = d->h_row_ptr[c]; e < d->h_row_ptr[c + 1]; ++e) {
                const int col = d->h_cols[e];
                XH_REQUIRE(ctx, col >= 0 && col < nc && (d->h_sign[e] == 1 || d->h_sign[e] == -1),
                           "xh_calib_flow: basin %d: bad entry %lld", b, (long long)e);
                ent[e] = d->h_sign[e] > 0 ? col : ~col;
            }
            // (velocity form: the kernel divides by L and the scaled cells' tau^-1 must be what h_tauinv says at v = 1)
            XH_REQUIRE(ctx, !vd || (vd->h_length[c] > 0.0 && std::isfinite(vd->h_length[c]) && vd->h_velocity[c] >= 0.0 &&
                                    std::isfinite(vd->h_velocity[c]) && vd->h_velocity[c] / vd->h_length[c] == d->h_tauinv[c]),
                       "xh_calib_flow: basin %d: row %lld: tauinv must be velocity / length, both finite, length positive", b,
                       (long long)(c - c0));
            const int bc = d->h_basin_col[c];
            XH_REQUIRE(ctx, bc >= -1 && bc < h_ncell[b], "xh_calib_flow: basin %d: bad basin column %d", b, bc);
            nbc += bc >= 0;
            if (gp) continue;
            const int r = d->h_outlet_rank[c];
            XH_REQUIRE(ctx, r == -1 || r == nout, "xh_calib_flow: basin %d: outlet ranks must count up in row order", b);
            nout += r >= 0;
        }
        if (gp) {                                                    // the basin's gauges, sorted by closure row
            const int64_t g0 = gp->ptr[b], g1 = gp->ptr[b + 1];
            XH_REQUIRE(ctx, g1 > g0 && g1 <= ngauge, "xh_calib_flow: basin %d has no gauge", b);
            for (int64_t g = g0; g < g1; ++g) {
                const int r = gp->row[g];
                XH_REQUIRE(ctx, r >= 0 && r < nc && (g == g0 || r >= gp->row[g - 1]),
                           "xh_calib_flow: basin %d: gauge rows must lie in the closure and ascend", b);
                XH_REQUIRE(ctx, d->h_basin_col[c0 + r] >= 0, "xh_calib_flow: gauge %lld is not on a cell of basin %d",
                           (long long)g, b);
                XH_REQUIRE(ctx, gp->weight[g] > 0.0 && std::isfinite(gp->weight[g]),
                           "xh_calib_flow: gauge %lld: the weight must be positive and finite", (long long)g);
                if (gfirst[c0 + r] < 0) gfirst[c0 + r] = (int)g;
                gbasin[g] = b;
            }
            gptr[b] = (int)g0;
            gptr[b + 1] = (int)g1;
            nout = (int)(g1 - g0);
            B.g1 = (int)g1;
        } else {
            // (the outlet form only: every basin cell is in the outlet closure; a union of gauge closures may leave some out)
            XH_REQUIRE(ctx, nbc == h_ncell[b], "xh_calib_flow: basin %d: %d closure rows carry forcing, the basin has %lld cells",
                       b, nbc, (long long)h_ncell[b]);
            XH_REQUIRE(ctx, nout > 0, "xh_calib_flow: basin %d has no outlet", b);
        }
        B.nout = nout;
        int kl = 0;
        while (nc > KLASSES[kl].hi) ++kl;
        const Klass &K = KLASSES[kl];
        int tpm = K.bt;
        if (K.cpl == 1) {                                            // smallest power of two that holds the closure
            tpm = 1;
            while (tpm < nc) tpm <<= 1;
        }
        B.tpm = tpm;
        B.mpw = K.bt / tpm;
        B.klass = kl;
        const size_t bytes = sizeof(double) * (2 * (size_t)B.mpw * nc + (gp ? 0 : (size_t)B.mpw * nout)) + sizeof(int) * (B.nnz + 4);
        XH_REQUIRE(ctx, bytes <= LDS_LIMIT, "xh_calib_flow: basin %d needs %zu bytes of LDS, more than %zu", b, bytes,
                   LDS_LIMIT);
        lds[kl] = std::max(lds[kl], bytes);
        for (int m0 = 0; m0 < nmembers; m0 += B.mpw) work[kl].push_back(make_int2(b, m0));
    }
    xh_calib_flow *f = new xh_calib_flow();
    f->nbasins = nbasins;
    f->nmonths = nmonths;
    f->nmembers = nmembers;
    f->rspin = d->routing_spinup;
    f->dt = d->dt;
    f->ngauge = (int)ngauge;
    std::vector<int2> all;
    for (int kl = NKLASS - 1; kl >= 0; --kl) {                       // (the largest closures first: the longest chains)
        std::stable_sort(work[kl].begin(), work[kl].end(),
                         [&](const int2 &x, const int2 &y) { return fb[x.x].nc > fb[y.x].nc; });
        f->work0[kl] = (int)all.size();
        f->nwork[kl] = (int)work[kl].size();
        f->lds[kl] = lds[kl];
        all.insert(all.end(), work[kl].begin(), work[kl].end());
    }
    auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
    const size_t o_fb = 0, o_rp = al(o_fb + sizeof(FlowBasin) * nbasins), o_ent = al(o_rp + 8 * (size_t)(ncl + 1)),
                 o_bcol = al(o_ent + 4 * ent.size()), o_or = al(o_bcol + 4 * (size_t)ncl),
                 o_nd = al(o_or + 4 * (size_t)ncl), o_nt = al(o_nd + 4 * (size_t)nmonths),
                 o_tau = al(o_nt + 4 * (size_t)nmonths), o_area = al(o_tau + 8 * (size_t)ncl),
                 o_s0 = al(o_area + 8 * (size_t)ncl), o_work = al(o_s0 + 8 * (size_t)ncl),
                 o_grow = al(o_work + sizeof(int2) * std::max<size_t>(all.size(), 1)), o_gb = al(o_grow + 4 * (size_t)ngauge),
                 o_gp = al(o_gb + 4 * (size_t)ngauge), o_gw = al(o_gp + 4 * gptr.size()),
                 o_chv = al(o_gw + 8 * (size_t)ngauge), o_len = al(o_chv + (vd ? 8 * (size_t)ncl : 0)),
                 total = al(o_len + (vd ? 8 * (size_t)ncl : 0));
    hipError_t e = hipMalloc(&f->d_buf, total);
    if (e != hipSuccess) {
        xh_calib_flow_destroy(f);
        return xh_fail(ctx, XH_ERR_HIP, "xh_calib_flow: hipMalloc(%zu) failed: %s", total, hipGetErrorString(e));
    }
    char *base = static_cast<char *>(f->d_buf);
    f->d_fb = reinterpret_cast<FlowBasin *>(base + o_fb);
    f->d_row_ptr = reinterpret_cast<int64_t *>(base + o_rp);
    f->d_ent = reinterpret_cast<int *>(base + o_ent);
    f->d_bcol = reinterpret_cast<int *>(base + o_bcol);
    f->d_orank = reinterpret_cast<int *>(base + o_or);
    f->d_ndays = reinterpret_cast<int *>(base + o_nd);
    f->d_nt = reinterpret_cast<int *>(base + o_nt);
    f->d_tau = reinterpret_cast<double *>(base + o_tau);
    f->d_area = reinterpret_cast<double *>(base + o_area);
    f->d_s0 = reinterpret_cast<double *>(base + o_s0);
    f->d_work = reinterpret_cast<int2 *>(base + o_work);
    f->d_grow = reinterpret_cast<int *>(base + o_grow);
    f->d_gbasin = reinterpret_cast<int *>(base + o_gb);
    f->d_gptr = reinterpret_cast<int *>(base + o_gp);
    f->d_gw = reinterpret_cast<double *>(base + o_gw);
    if (vd) {
        f->d_chv = reinterpret_cast<double *>(base + o_chv);
        f->d_len = reinterpret_cast<double *>(base + o_len);
    }
    const struct {
        void *dst;
        const void *src;
        size_t n;
    } up[] = {{f->d_fb, fb.data(), sizeof(FlowBasin) * nbasins}, {f->d_row_ptr, d->h_row_ptr, 8 * (size_t)(ncl + 1)},
              {f->d_ent, ent.data(), 4 * ent.size()},            {f->d_bcol, d->h_basin_col, 4 * (size_t)ncl},
              {f->d_orank, gp ? gfirst.data() : d->h_outlet_rank, 4 * (size_t)ncl},   {f->d_ndays, d->h_ndays, 4 * (size_t)nmonths},
              {f->d_nt, nt.data(), 4 * (size_t)nmonths},         {f->d_tau, d->h_tauinv, 8 * (size_t)ncl},
              {f->d_area, d->h_area, 8 * (size_t)ncl},           {f->d_s0, d->h_s0, 8 * (size_t)ncl},
              {f->d_work, all.data(), sizeof(int2) * all.size()},
              {f->d_grow, gp ? gp->row : nullptr, 4 * (size_t)ngauge},   {f->d_gbasin, gbasin.data(), 4 * (size_t)ngauge},
              {f->d_gptr, gptr.data(), 4 * gptr.size()},         {f->d_gw, gp ? gp->weight : nullptr, 8 * (size_t)ngauge},
              {f->d_chv, vd ? vd->h_velocity : nullptr, vd ? 8 * (size_t)ncl : 0},
              {f->d_len, vd ? vd->h_length : nullptr, vd ? 8 * (size_t)ncl : 0}};
    for (const auto &u : up) {
        if (!u.n) continue;
        e = hipMemcpyAsync(u.dst, u.src, u.n, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            xh_calib_flow_destroy(f);
            return xh_fail(ctx, XH_ERR_HIP, "xh_calib_flow: upload failed: %s", hipGetErrorString(e));
        }
    }
    e = hipStreamSynchronize(ctx->stream);                           // the host tables are locals
    if (e != hipSuccess) {
        xh_calib_flow_destroy(f);
        return xh_fail(ctx, XH_ERR_HIP, "xh_calib_flow: upload failed: %s", hipGetErrorString(e));
    }
    e = hipEventCreateWithFlags(&f->fork, hipEventDisableTiming);
    for (int kl = 1; kl < NKLASS && e == hipSuccess; ++kl) {
        if (!f->nwork[kl]) continue;
        e = hipStreamCreateWithFlags(&f->side[kl], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&f->join[kl], hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        xh_calib_flow_destroy(f);
        return xh_fail(ctx, XH_ERR_HIP, "xh_calib_flow: stream / event creation failed: %s", hipGetErrorString(e));
    }
    *out = f;
    return XH_OK;
}

}  // namespace

int xh_calib_flow_create(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, int32_t nmonths, int32_t nmembers,
                         const xh_calib_flow_desc *d, xh_calib_flow **out, const xh_calib_velocity_desc *vel) {
    return flow_create(ctx, nbasins, h_ncell, nmonths, nmembers, d, nullptr, vel, out);
}

int xh_calib_gauge_create(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, int32_t nmonths, int32_t nmembers,
                          const xh_calib_gauge_desc *g, xh_calib_flow **out, const xh_calib_velocity_desc *vel) {
    XH_REQUIRE(ctx, g && out, "xh_calib_gauge: NULL argument");
    const xh_calib_flow_desc d = {g->routing_spinup, g->dt,        g->h_ndays, g->h_closure_ptr, g->h_row_ptr, g->h_cols,
                                  g->h_sign,         g->h_basin_col, nullptr,    g->h_tauinv,      g->h_area,    g->h_s0};
    const GaugePart gp = {g->h_gauge_ptr, g->h_gauge_row, g->h_gauge_weight};
    return flow_create(ctx, nbasins, h_ncell, nmonths, nmembers, &d, &gp, vel, out);
}

int xh_calib_flow_enqueue(xh_ctx *ctx, const xh_calib_problem &P, const double *d_pars, const int *d_active, double *d_ed) {
    const xh_calib_flow &f = *P.flow;
    hipStream_t st = ctx->stream;
    int rc = xh_timed(ctx, "calib_abcd", st, [&] { return xh_calib_spinup_enqueue(ctx, P, d_pars, d_active); });
    if (rc) return rc;
    rc = xh_timed(ctx, "calib_flow", st, [&] {
        // fork: the side streams start after the spin-up; join: the context's stream waits for every class
        XH_HIP(ctx, hipEventRecord(f.fork, st));
        for (int kl = 1; kl < NKLASS; ++kl)
            if (f.nwork[kl]) XH_HIP(ctx, hipStreamWaitEvent(f.side[kl], f.fork, 0));
        int r = XH_OK;
        if (!r && f.nwork[4]) r = launch_klass<1024, 3>(ctx, P, f, 4, d_pars, d_active);
        if (!r && f.nwork[3]) r = launch_klass<256, 4>(ctx, P, f, 3, d_pars, d_active);
        if (!r && f.nwork[2]) r = launch_klass<256, 2>(ctx, P, f, 2, d_pars, d_active);
        if (!r && f.nwork[1]) r = launch_klass<256, 1>(ctx, P, f, 1, d_pars, d_active);
        if (!r && f.nwork[0]) r = launch_klass<64, 1>(ctx, P, f, 0, d_pars, d_active);
        for (int kl = 1; kl < NKLASS; ++kl)
            if (f.nwork[kl]) {
                XH_HIP(ctx, hipEventRecord(f.join[kl], f.side[kl]));
                XH_HIP(ctx, hipStreamWaitEvent(st, f.join[kl], 0));
            }
        return r;
    });
    if (rc) return rc;
    if (f.ngauge)
        return xh_timed(ctx, "calib_kge", st, [&] {
            return xh_calib_gauge_score_enqueue(ctx, P, d_active, f.ngauge, f.d_gbasin, f.d_gptr, f.d_gw, P.d_series, d_ed);
        });
    return xh_timed(ctx, "calib_kge", st, [&] { return xh_calib_kge_enqueue(ctx, P, d_active, P.d_series, d_ed); });
}

// one evaluation of either form: `flow` (outlets) or `gauge`
static int objective_multi(xh_ctx *ctx, const char *who, int32_t nbasins, const int64_t *h_ncell, int32_t nmonths,
                           int32_t spinup, int32_t nmembers, int32_t npar, const double *h_pars,
                           const double *const *h_pet_t, const double *const *h_precip_t, const double *const *h_tmin_t,
                           const xh_calib_flow_desc *flow, const xh_calib_gauge_desc *gauge,
                           const xh_calib_velocity_desc *vel, const double *h_obs, double *h_ed, double *h_ed_gauge,
                           double *h_series) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, h_pars && h_obs && h_ed && (flow || gauge), "%s: NULL argument", who);
    XH_REQUIRE(ctx, !gauge || (gauge->h_gauge_ptr && nbasins > 0), "%s: NULL gauge table", who);
    const int64_t ng64 = gauge ? gauge->h_gauge_ptr[nbasins] : 0;
    XH_REQUIRE(ctx, !gauge || (ng64 > 0 && ng64 < ((int64_t)1 << 24)), "%s: bad gauge_ptr", who);
    const int32_t ngauge = (int32_t)ng64;
    std::vector<xh_calib_basin> basins;
    std::vector<int> chunk_basin;
    size_t bytes = 0;
    int ml = 0;
    int rc = xh_calib_problem_plan(ctx, nbasins, h_ncell, nmonths, spinup, nmembers, npar, h_pet_t, h_precip_t, h_tmin_t,
                                   nullptr, basins, chunk_basin, &bytes, &ml, ngauge);
    if (rc) return rc;
    xh_calib_flow *f = nullptr;
    rc = gauge ? xh_calib_gauge_create(ctx, nbasins, h_ncell, nmonths, nmembers, gauge, &f, vel)
               : xh_calib_flow_create(ctx, nbasins, h_ncell, nmonths, nmembers, flow, &f, vel);
    if (rc) return rc;
    const size_t nbm = (size_t)nbasins * nmembers, nsm = (size_t)(gauge ? ngauge : nbasins) * nmembers;
    const size_t pstride = (size_t)npar + (vel ? 1 : 0);             // h_pars rows: the ABCD genes, then v
    const size_t io_bytes = ((nbm * pstride + nbm) * sizeof(double) + 255) & ~size_t(255);
    void *buf = nullptr;
    rc = xh_scratch(ctx, 1, io_bytes + bytes, &buf);
    xh_calib_problem P;
    if (!rc) {
        double *d_pars = static_cast<double *>(buf);
        double *d_ed = d_pars + nbm * pstride;
        const hipError_t e = hipMemcpyAsync(d_pars, h_pars, sizeof(double) * nbm * pstride, hipMemcpyHostToDevice, ctx->stream);
        rc = e == hipSuccess ? XH_OK : xh_fail(ctx, XH_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
        if (!rc)
            rc = xh_calib_problem_place(ctx, P, nmonths, spinup, nmembers, npar, basins, chunk_basin, h_obs,
                                        static_cast<char *>(buf) + io_bytes, ml, ngauge);
        P.flow = f;
        P.pstride = (int)pstride;
        if (!rc) rc = xh_calib_enqueue(ctx, P, d_pars, nullptr, d_ed);
        if (!rc) {
            hipError_t e2 = hipMemcpyAsync(h_ed, d_ed, sizeof(double) * nbm, hipMemcpyDeviceToHost, ctx->stream);
            if (e2 == hipSuccess && h_ed_gauge && gauge)
                e2 = hipMemcpyAsync(h_ed_gauge, P.d_ed_gauge, sizeof(double) * nsm, hipMemcpyDeviceToHost, ctx->stream);
            if (e2 == hipSuccess && h_series)
                e2 = hipMemcpyAsync(h_series, P.d_series, sizeof(double) * nsm * nmonths, hipMemcpyDeviceToHost,
                                    ctx->stream);
            if (e2 == hipSuccess) e2 = hipStreamSynchronize(ctx->stream);
            if (e2 != hipSuccess) rc = xh_fail(ctx, XH_ERR_HIP, "%s: %s", who, hipGetErrorString(e2));
        }
    }
    (void)hipStreamSynchronize(ctx->stream);                         // nothing of the call may still run on f
    xh_calib_flow_destroy(f);
    return rc;
}

extern "C" int xh_calib_flow_objective_multi(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, int32_t nmonths,
                                             int32_t spinup, int32_t nmembers, int32_t npar, const double *h_pars,
                                             const double *const *h_pet_t, const double *const *h_precip_t,
                                             const double *const *h_tmin_t, const xh_calib_flow_desc *flow,
                                             const double *h_obs, double *h_ed, double *h_series) {
    return objective_multi(ctx, "xh_calib_flow_objective_multi", nbasins, h_ncell, nmonths, spinup, nmembers, npar, h_pars,
                           h_pet_t, h_precip_t, h_tmin_t, flow, nullptr, nullptr, h_obs, h_ed, nullptr, h_series);
}

extern "C" int xh_calib_gauge_objective_multi(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, int32_t nmonths,
                                              int32_t spinup, int32_t nmembers, int32_t npar, const double *h_pars,
                                              const double *const *h_pet_t, const double *const *h_precip_t,
                                              const double *const *h_tmin_t, const xh_calib_gauge_desc *gauge,
                                              const double *h_obs, double *h_ed, double *h_ed_gauge, double *h_series) {
    return objective_multi(ctx, "xh_calib_gauge_objective_multi", nbasins, h_ncell, nmonths, spinup, nmembers, npar, h_pars,
                           h_pet_t, h_precip_t, h_tmin_t, nullptr, gauge, nullptr, h_obs, h_ed, h_ed_gauge, h_series);
}

extern "C" int xh_calib_flow_velocity_objective_multi(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, int32_t nmonths,
                                                      int32_t spinup, int32_t nmembers, int32_t npar, const double *h_pars,
                                                      const double *const *h_pet_t, const double *const *h_precip_t,
                                                      const double *const *h_tmin_t, const xh_calib_flow_desc *flow,
                                                      const xh_calib_velocity_desc *velocity, const double *h_obs,
                                                      double *h_ed, double *h_series) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, flow && velocity, "xh_calib_flow_velocity_objective_multi: NULL tables");
    return objective_multi(ctx, "xh_calib_flow_velocity_objective_multi", nbasins, h_ncell, nmonths, spinup, nmembers, npar,
                           h_pars, h_pet_t, h_precip_t, h_tmin_t, flow, nullptr, velocity, h_obs, h_ed, nullptr, h_series);
}

extern "C" int xh_calib_gauge_velocity_objective_multi(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, int32_t nmonths,
                                                       int32_t spinup, int32_t nmembers, int32_t npar, const double *h_pars,
                                                       const double *const *h_pet_t, const double *const *h_precip_t,
                                                       const double *const *h_tmin_t, const xh_calib_gauge_desc *gauge,
                                                       const xh_calib_velocity_desc *velocity, const double *h_obs,
                                                       double *h_ed, double *h_ed_gauge, double *h_series) {
    if (!ctx) return XH_ERR_ARG;
    XH_REQUIRE(ctx, gauge && velocity, "xh_calib_gauge_velocity_objective_multi: NULL tables");
    return objective_multi(ctx, "xh_calib_gauge_velocity_objective_multi", nbasins, h_ncell, nmonths, spinup, nmembers, npar,
                           h_pars, h_pet_t, h_precip_t, h_tmin_t, nullptr, gauge, velocity, h_obs, h_ed, h_ed_gauge, h_series);
}
