// The routing plan (xh_route_plan) as the two halves of the routing code see it: xh_mrtm.hip (kernels for general graphs, plan
// create / prepare / info, route_choose + route_series_impl: which kernel routes a call) and xh_mrtm_check.hip (the call layer:
// first-call and periodic cross-checks, XH_ROUTE_VALIDATE, the record of unconfirmed calls and their re-runs after a device
// fault).
//
// A call's route is decided in ONE place, route_choose (plan state, flags, dt, fed or not): the form whose partition the tree
// networks try first, whether the dataflow kernels may run at all, which cells the global kernels take, whether a fed call
// is turned down.  route_series_impl walks that choice with its fall-backs and returns what ran (xh_route_outcome, xh_common.h)
// without writing into the plan; the call layer keeps it as the plan's `last` call for the caller's own calls and their
// re-runs (never for a cross-check's second routing) and in the call's record, and decides from it -- not from a prediction --
// whether the first-call cross-check is due.  Its marker names the device, build and runtime, the topology and the form;
// the prepared form's also its prep_key, so a partition prepared for other data is checked again.
#pragma once
#include <string>
#include <vector>

#include "xh_common.h"
#include "xh_mrtm_flow.h"

constexpr int XH_ROUTE_N_CLASS = 8;      // workgroup shapes of the workgroup-per-network kernel (xh_mrtm.hip: CLASSES)

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    bool pooled = false;        // p points into an UploadPool's allocation (freed with the pool, not on its own)
};

// Cells routed by the global-memory kernels and their rows (CSR in `cells` order)
struct FbCsr {
    int64_t n = 0;
    bool single_ds = true;      // every cell feeds at most one row and has one -1 on its diagonal: XH_ROUTE_ATOMIC can route it
    DevBuf cells, ptr, col, sgn, ds;      // [n] cell ids, [n + 1] row offsets, each term's cell and sign, [n] downstream cell or -1
};

// One form of the tree networks' partition (xh_route_form)
struct RouteForm {
    FlowPlan *fp = nullptr;
    bool first_checked = false;      // the first-call cross-check passed on this partition, or its marker says it did
    const char *suffix = "";         // of the marker's name
};

struct xh_route_plan {
    xh_ctx *ctx = nullptr;
    int64_t ncell = 0, n_networks = 0, largest_network = 0, n_units = 0, largest_unit = 0, total_slots = 0;
    // LDS units, grouped by class
    std::vector<int> class_units[XH_ROUTE_N_CLASS];       // slot0 of the units of each class (every network)
    DevBuf d_class_units[XH_ROUTE_N_CLASS];
    std::vector<int> rest_units[XH_ROUTE_N_CLASS];        // only the units of networks the dataflow kernel does not route
    DevBuf d_rest_units[XH_ROUTE_N_CLASS];
    // The tree-shaped networks as single-wave dataflow units, one partition per form:
    //   XH_FORM_EXACT    the bit-exact kernels' (made with the plan);
    //   XH_FORM_PAIRS    the reassociated kernel's with every unit in pair form (XH_ROUTE_REASSOC; xh_flow_rsum.cpp, k_mrtm_rsum):
    //                    needs nothing of a call's data, made with the plan when the environment asks for the form, else on the
    //                    first call that does (rsum_failed: the planner turned the grid down, not tried again);
    //   XH_FORM_PREPARED the same with FOLDED LEAVES and SINGLE SUMS: which cells can fire depends on velocity, flow distance and
    //                    dt, so xh_route_plan_prepare makes it from the host copies (marker "_rs" single sums, "_rf" folded leaves
    //                    only); the kernel guards the assumption, and a trip routes the call again on the pairs and bans this one.
    RouteForm form[XH_N_FORMS] = {{nullptr, false, ""}, {nullptr, false, "_r"}, {nullptr, false, "_rf"}};
    bool rsum_failed = false;
    double fold_dt = 0.0;
    bool fold_disabled = false;
    bool fold_tried = false;      // prepare() has asked the planner (it may have had nothing to fold)
    uint64_t prep_key = 0;        // ... for these sets of cells that can fire / leaves that cannot, and this dt
    xh_route_outcome last;        // the caller's last call (xh_route_plan_info[13], rsum_info, stats)
    std::vector<int64_t> h_indptr;
    std::vector<int32_t> h_indices;
    std::vector<int8_t> h_sign;
    std::vector<int> h_comp;
    int h_ncomp = 0;
    int guard_trips = 0;                         // calls routed again on the plan of pairs after a guard of the prepared plan tripped
    int64_t reroutes = 0;                        // calls re-run with one workgroup per network after a device fault
    // After a fault the dataflow kernels are skipped for the next `skip_calls` calls of this plan (the device is shared:
    // every further attempt would first sit out a bounded wait), doubling with every fault in a row up to 256 calls; a
    // dataflow call confirmed fault-free resets the streak (xh_route_confirm).
    int fault_streak = 0, skip_calls = 0;
    int64_t validated = 0;                       // calls cross-checked against the workgroup-per-network kernel (XH_ROUTE_VALIDATE)
    // The dataflow kernels' streams rest on an ordering assumption outside the HIP memory model (xh_mrtm_wave.hip, check()).
    // So that no product run is unverified on a new box, the FIRST dataflow call of a plan on each partition is cross-checked
    // like XH_ROUTE_VALIDATE unless a marker file says this library build already passed on this device with this topology and
    // partition (route_first_check_*; XH_ROUTE_VALIDATE_FIRST=0 switches it off) ...
    // ... and every XH_ROUTE_VALIDATE_EVERY-th dataflow call of a long-lived plan is cross-checked again (default 1,000; 0 =
    // never): one clean pass says little about call 10^4 of a server that routes scenarios all day (~0.25 s each time)
    int64_t dataflow_calls = 0;
    bool validate_due = false;
    uint64_t topo_hash = 0;
    int64_t n_rest_units = 0;
    // the global kernels' cells: the whole graph (XH_ROUTE_FORCE_FALLBACK), those no workgroup unit routes, and those neither
    // a workgroup unit nor the dataflow kernels route (the rest beside them)
    FbCsr fb_all, fb, fb_rest;
    DevBuf d_cell_of_slot, d_ent, d_cnt;
    hipStream_t streams[XH_ROUTE_N_CLASS] = {};
    hipEvent_t ev_fork = nullptr, ev_join[XH_ROUTE_N_CLASS + 1] = {};
    hipStream_t fb_stream = nullptr;
    void *d_pool = nullptr;     // the allocation behind the tables uploaded at create (UploadPool)
};

// The route of one call (route_choose).  The flags that bypass a path are read there and nowhere else.
struct RouteChoice {
    int form = XH_FORM_EXACT;    // the partition the tree networks try first (PAIRS before it exists: made by route_series_impl)
    bool dataflow = false;       // the dataflow kernels may route the tree networks (route_series_impl clears it if they cannot)
    bool skew = false;           // ... the time-skewed ones (else the lock-step kernel)
    bool whole_graph = false;    // the global kernels route every cell (XH_ROUTE_FORCE_FALLBACK)
    bool atomic = false;         // ... with fp64 atomic scatter-adds
    bool checkable = false;      // a call the cross-checks are for: the dataflow kernels may run, no atomics, no test fault
    bool refuse_fed = false;     // a fed call: not every cell can be routed by the time-skewed kernel that waits for its runoff
    const FbCsr &fallback(const xh_route_plan *p) const { return whole_graph ? p->fb_all : dataflow ? p->fb_rest : p->fb; }
};

// xh_mrtm.hip
RouteChoice route_choose(const xh_route_plan *plan, int flags, double dt, bool fed);
int route_series_impl(xh_ctx *ctx, xh_route_plan *plan, int32_t nmonths, int32_t spinup_months, const int32_t *h_ndays, double dt,
                      const double *d_flow_dist, const double *d_velocity, const double *d_area, const double *d_runoff,
                      const double *d_S0, double *d_chstorage, double *d_avgchflow, double *d_S_end, double *d_F_end,
                      int32_t flags, xh_route_outcome *out, const FlowFeed *feed = nullptr);
