// Internal interface between the calibration objective (xh_calib.hip) and the device-side differential evolution
// (xh_calib_de.hip).  Not part of the C-ABI.
#pragma once
#include <vector>

#include "xh_common.h"

struct xh_calib_basin {
    int ncell, chunk0, nchunks, pad;
    const double *pet, *pr, *tn, *area;      // [month, cell] forcing of this basin; area may be NULL (mm_per_mth)
    // member-lane layout only: the member-independent rain / snow split of every (month, cell), made once per problem
    double *rain, *snow, *frac;
    int *kind;
};

// A set of basins laid out for the objective kernels: tables and work arrays in ONE device allocation.
struct xh_calib_problem {
    int nbasins = 0, nmonths = 0, spinup = 0, nmembers = 0, npar = 0;
    // length of a member's row of d_pars: npar (the ABCD genes: 4, or 5 with snow) unless the streamflow objective
    // calibrates the velocity scale, whose gene follows them (npar + 1); xh_calib_problem_place sets npar
    int pstride = 0;
    size_t nchunks = 0;
    // 0: lanes <-> cells, 4 members per thread (any population).  1: lanes <-> members, 16 cells per wave, forcing as
    // scalar loads, no cross-lane sums (populations that fill waves of 64 members: 100 instead of 145 wave-instructions
    // per member-cell-month).  Chosen by xh_calib_problem_plan; the work arrays below are laid out accordingly.
    int member_lanes = 0;
    mutable bool split_done = false;          // member-lane layout: rain / snow split computed (set by the first enqueue)
    xh_calib_basin *d_basins = nullptr;
    int *d_chunk_basin = nullptr;
    int ngauge = 0;                           // gauge form of the streamflow objective: gauges of all basins (else 0)
    double *d_obs = nullptr;                  // [nbasins, nmonths]; gauge form: [ngauge, nmonths], NaN = missing
    double *d_sm0 = nullptr, *d_gw0 = nullptr;   // [nbasins, nmembers]
    double *d_dec = nullptr;                  // [nchunks, nmembers, 6]
    int *d_cnt = nullptr;                     // [nchunks, nmembers, 6]
    double *d_part = nullptr;                 // [nchunks, nmembers, nmonths]
    double *d_series = nullptr;               // [nbasins, nmembers, nmonths]; gauge form: [ngauge, nmembers, nmonths]
    double *d_ed_gauge = nullptr;             // gauge form: [ngauge, nmembers] ED of every gauge
    double *d_series_m = nullptr;             // member-lane layout: [nbasins, nmonths, nmembers]
    // streamflow objective (set_calibrate = 1; xh_calib_flow.hip): closures, routing tables and launch lists of the
    // basins, owned by whoever made the problem; NULL = the runoff objective
    struct xh_calib_flow *flow = nullptr;
};

// Validates the arguments, fills the host tables and returns the bytes xh_calib_problem_place needs.  ngauge > 0: the
// gauge form, whose observations and series are per gauge (h_obs [ngauge, nmonths]).
int xh_calib_problem_plan(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, int32_t nmonths, int32_t spinup,
                          int32_t nmembers, int32_t npar, const double *const *h_pet_t,
                          const double *const *h_precip_t, const double *const *h_tmin_t,
                          const double *const *h_area, std::vector<xh_calib_basin> &basins,
                          std::vector<int> &chunk_basin, size_t *bytes, int *member_lanes, int32_t ngauge = 0);
// Carves the problem out of `buf` (device, 256-byte aligned, at least `bytes` long) and uploads tables and obs.
int xh_calib_problem_place(xh_ctx *ctx, xh_calib_problem &P, int32_t nmonths, int32_t spinup, int32_t nmembers,
                           int32_t npar, std::vector<xh_calib_basin> &basins, const std::vector<int> &chunk_basin,
                           const double *h_obs, void *buf, int member_lanes, int32_t ngauge = 0);
// member-lane layout: d_series in the [nbasins, nmembers, nmonths] order of the C-ABI (a transpose of d_series_m)
int xh_calib_series_out(xh_ctx *ctx, const xh_calib_problem &P);
// Enqueues one evaluation of every basin's population on the context's stream: d_pars [nbasins, nmembers, npar] ->
// d_ed [nbasins, nmembers] (ED = 1 - KGE).  d_active [nbasins] (may be NULL): basins with 0 are skipped and their
// d_ed entries left untouched.  No host synchronisation.
int xh_calib_enqueue(xh_ctx *ctx, const xh_calib_problem &P, const double *d_pars, const int *d_active, double *d_ed);

// The pieces of xh_calib_enqueue the streamflow objective shares: the spin-up march + basin-mean initial state
// (P.d_sm0, P.d_gw0) in the problem's layout, and ED of series [nbasins, nmembers, nmonths] against P.d_obs.
int xh_calib_spinup_enqueue(xh_ctx *ctx, const xh_calib_problem &P, const double *d_pars, const int *d_active);
int xh_calib_kge_enqueue(xh_ctx *ctx, const xh_calib_problem &P, const int *d_active, const double *d_series, double *d_ed);

// Streamflow objective (xh_calib_flow.hip).  create: validates and uploads the closure tables of `desc` for a problem of
// nbasins basins (h_ncell basin cells each) and nmembers members; enqueue: spin-up, the fused ABCD + routing march and
// ED into d_ed (d_active as for xh_calib_enqueue).  velocity != NULL (either form): the velocity form, whose members' rows
// of d_pars are [npar ABCD genes, v]; the owner of the problem sets P.pstride = npar + 1.
int xh_calib_flow_create(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, int32_t nmonths, int32_t nmembers,
                         const xh_calib_flow_desc *desc, xh_calib_flow **out,
                         const xh_calib_velocity_desc *velocity = nullptr);
void xh_calib_flow_destroy(xh_calib_flow *f);
int xh_calib_flow_enqueue(xh_ctx *ctx, const xh_calib_problem &P, const double *d_pars, const int *d_active, double *d_ed);

// Gauge form of the streamflow objective: the tables of an xh_calib_gauge_desc (union closures, gauges); enqueue is
// xh_calib_flow_enqueue.  score: masked ED of every (gauge, member) into P.d_ed_gauge, then the basin's weighted mean in
// gauge order into d_ed.
int xh_calib_gauge_create(xh_ctx *ctx, int32_t nbasins, const int64_t *h_ncell, int32_t nmonths, int32_t nmembers,
                          const xh_calib_gauge_desc *desc, xh_calib_flow **out,
                          const xh_calib_velocity_desc *velocity = nullptr);
int xh_calib_gauge_score_enqueue(xh_ctx *ctx, const xh_calib_problem &P, const int *d_active, int ngauge,
                                 const int *d_gauge_basin, const int *d_gauge_ptr, const double *d_weight,
                                 const double *d_series, double *d_ed);
