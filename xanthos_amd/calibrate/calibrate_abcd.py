"""ABCD calibration on MI355X -- mirror of xanthos/calibrate/calibrate_abcd.py.

The reference wraps ``scipy.optimize.differential_evolution`` around ``objective_kge`` (:103-112, :176-213), which
runs ABCD on one basin for ONE parameter vector per call.  Here the objective is evaluated for a whole population
per call by ``xh_calib_objective`` (csrc/xh_calib.hip: members x cells on the GPU, forcing transposed once per basin
and kept in HBM), and the differential evolution itself runs on the device too (csrc/xh_calib_de.hip): ``best1bin``
with SciPy's defaults (popsize 15 x n_parameters members, Latin-hypercube start, dithered mutation in (0.5, 1),
recombination 0.7, tol 0.01, maxiter 1000, the two sampled members distinct from the candidate), generation-synchronous
like SciPy's ``updating='deferred'``, for ALL requested basins at once instead of the reference's serial basin loop
(:256-262).  With several ranks (``launch.current_group()``) the basins are dealt to the ranks largest-first and the
``[n_basins, n_par + 1]`` results gathered on rank 0.  SciPy's driver is unseeded, so the reference's search
trajectory is not reproducible; the objective is the parity target (tests/golden/kge.npz) and the generation step is
checked against a numpy restatement of SciPy's (oracle/de.py).

``set_calibrate = 1`` calibrates against observed streamflow (``m3_per_sec``) with the objective of DESIGN 4.4: the
basin's runoff scattered onto its upstream closure through UM, routed by MRTM (routing spin-up, then all months) and
summed over the basin's outlets.  The reference's branch cannot run (a flat ``np.put`` of the runoff, :170-171, and the
whole ``[ncell, nmonths]`` Avg_ChFlow handed to ``np.corrcoef``, :173, :196-213); this is its evident intent.  Each
basin routes its own closure on the device (flow_tables.py, csrc/xh_calib_flow.hip); ``router_func`` is accepted for
signature compatibility and not called.

With ``gauges`` (gauge_tables.Gauges: stream gauges on cells inside the network, records with gaps) the same objective is
scored at the gauges instead of the outlets: each basin is routed once per member on the union of its gauges' upstream
closures, every gauge is scored over its finite months, and the basin's energy is the weighted mean of its gauges' ED
(gauge_tables.py).  ``calibrate_all`` then also writes ``gauge_kge.csv``.

With velocity bounds (``velocity_bounds = (lo, hi)``; ``[Calibrate] calibrate_velocity = 1``) the streamflow objective, in
either form, has one more parameter per basin: the dimensionless velocity scale v, last in the vector [a, b, c, d, (m), v].
The basin's own cells are routed with tau^-1 = (v ChV) / L, the closure's foreign cells with their own ChV / L (DESIGN
4.4).  The reference's two files per basin keep their names and shapes (the ABCD columns only); v goes to
``velocity_scale_basin_N.npy`` and ``calibrate_all`` writes ``velocity_scale.csv`` for a forward run (velocity_scale.py).
"""
import logging
import os
import time

import numpy as np

from .. import _hip
from .flow_tables import FlowTables, check_forcing
from .gauge_tables import GaugeTables
from .velocity_scale import DEFAULT_BOUNDS, check_bounds, combined_scales, write_velocity_scale

LB = 1e-4
UB = 1 - LB


class BasinObjective:
    """ED = 1 - KGE of the basin runoff for batches of parameter vectors (basin_runoff + objective_kge, :134-213)."""

    def __init__(self, pet, precip, tmin, n_months, runoff_spinup, obs_unit, bsn_areas, bsn_robs, device=0,
                 set_calibrate=0):
        if set_calibrate == 1:
            if obs_unit != 'm3_per_sec':
                raise ValueError('obs_unit must be m3_per_sec for set_calibrate = 1')
        elif obs_unit not in ('km3_per_mth', 'mm_per_mth'):
            raise ValueError('obs_unit must be km3_per_mth or mm_per_mth for set_calibrate = 0')
        if runoff_spinup < 25:
            raise IndexError('Spin-up steps must produce at least 25 months of spin-up; got {}'.format(runoff_spinup))
        self.ctx = _hip.get_context(device)
        self.ncell = int(np.asarray(pet).shape[0])
        self.n_months, self.spinup = int(n_months), int(runoff_spinup)
        self.nosnow = tmin is None
        self.npar = 4 if self.nosnow else 5
        tr = lambda a: self.ctx.upload(np.ascontiguousarray(np.asarray(a, dtype=np.float64)[:, :n_months].T))
        self.d_pet, self.d_precip = tr(pet), tr(precip)
        # the loader's np.nan_to_num of TempMinFile (data_load.py:194-195); precipitation keeps its NaNs (:186)
        self.d_tmin = None if self.nosnow else self.ctx.nan_to_num(tr(tmin))
        self.d_area = self.ctx.upload(bsn_areas) if obs_unit == 'km3_per_mth' else None   # (m3_per_sec: in the routing tables)
        # (gauge form: the records live in the gauge tables)
        self.obs = None if bsn_robs is None else np.ascontiguousarray(np.asarray(bsn_robs, dtype=np.float64)[:n_months])
        self.obs_unit = obs_unit
        self.nfev = 0

    def __call__(self, pars, want_series=False):
        if self.obs_unit == 'm3_per_sec':
            raise TypeError('the streamflow objective needs the routing tables: evaluate through BasinSet')
        pars = np.atleast_2d(np.asarray(pars, dtype=np.float64))[:, :self.npar]
        self.nfev += pars.shape[0]
        return self.ctx.calib_objective(self.ncell, self.n_months, self.spinup, pars, self.d_pet, self.d_precip,
                                        self.d_tmin, self.d_area, self.obs, want_series=want_series)

    def close(self):
        for b in (self.d_pet, self.d_precip, self.d_tmin, self.d_area):
            if b is not None:
                b.free()


class BasinSet:
    """Several basins prepared for the device: forcing transposed to [month, cell] in HBM, observations, bounds."""

    def __init__(self, cals, n_months, runoff_spinup, obs_unit, device=0, flow=None):
        self.cals = cals
        # set_calibrate = 1: the closure tables of these basins in this order (``flow``, or those of the Calibrates)
        self.flow = None
        if obs_unit == 'm3_per_sec':
            self.flow = flow if flow is not None else type(cals[0].flow).join([c.flow for c in cals])
            if self.flow.basins != [c.basin_num for c in cals]:
                raise ValueError('the flow tables hold basins {}, not {}'.format(self.flow.basins,
                                                                                  [c.basin_num for c in cals]))
        self.objs = [c.objective() for c in cals]
        self.ctx = self.objs[0].ctx
        self.nosnow, self.npar = self.objs[0].nosnow, self.objs[0].npar
        self.n_months, self.spinup = int(n_months), int(runoff_spinup)
        self.gauge_form = getattr(self.flow, 'gauge_form', False)
        # gauge form: one record per gauge [ngauge, nmonths], NaN = missing
        self.obs = self.flow.obs if self.gauge_form else np.stack([o.obs for o in self.objs])
        self.bounds = cals[0].bounds
        # the velocity form: rows of parameters are [npar ABCD genes, v]
        self.velocity = cals[0].velocity_bounds is not None
        if any((c.velocity_bounds is not None) != self.velocity or c.bounds != self.bounds for c in cals):
            raise ValueError('the basins of a set share their bounds')
        self.nx = self.npar + (1 if self.velocity else 0)

    def args(self):
        o = self.objs
        return ([x.ncell for x in o], [x.d_pet for x in o], [x.d_precip for x in o],
                None if self.nosnow else [x.d_tmin for x in o],
                None if o[0].d_area is None else [x.d_area for x in o])

    def evaluate(self, pars, want_series=False, want_gauges=False):
        """ED for parameter sets pars [nbasins, nmembers, npar] in ONE launch (and the modelled series).  Gauge form: the
        series is [ngauge, nmembers, nmonths], and ``want_gauges`` adds ED of every gauge [ngauge, nmembers].  With
        velocity bounds pars is [nbasins, nmembers, npar + 1], the velocity scale last."""
        nc, pet, pr, tn, ar = self.args()
        pars = np.asarray(pars)
        if pars.ndim != 3 or pars.shape[2] < self.nx:
            raise ValueError('pars must be [nbasins, nmembers, {}]'.format(self.nx))
        pars = pars[:, :, :self.nx]
        if self.gauge_form:
            return self.ctx.calib_gauge_objective_multi(nc, self.n_months, self.spinup, pars, pet, pr, tn, self.flow,
                                                        want_series=want_series, want_gauges=want_gauges,
                                                        velocity=self.velocity)
        if want_gauges:
            raise ValueError('want_gauges needs gauge tables')
        if self.flow is not None:
            return self.ctx.calib_flow_objective_multi(nc, self.n_months, self.spinup, pars, pet, pr, tn, self.flow,
                                                       self.obs, want_series=want_series, velocity=self.velocity)
        return self.ctx.calib_objective_multi(nc, self.n_months, self.spinup, pars, pet, pr, tn, ar, self.obs,
                                              want_series=want_series)

    def solver(self, nmembers, seed=0):
        nc, pet, pr, tn, ar = self.args()
        return _hip.CalibDE(self.ctx, nc, self.n_months, self.spinup, nmembers, self.bounds, pet, pr, tn, ar, self.obs,
                            seed=seed, keys=[c.basin_num for c in self.cals], flow=self.flow, velocity=self.velocity)

    def close(self):
        for o in self.objs:
            o.close()


def differential_evolution_device(bset, popsize=15, maxiter=1000, tol=0.01, atol=0.0, mutation=(0.5, 1.0),
                                  recombination=0.7, seed=None, nmembers=None, check_every=4):
    """DE/best/1/bin for every basin of ``bset`` at once, entirely on the device (csrc/xh_calib_de.hip).

    SciPy's defaults as the reference uses them (calibrate_abcd.py:103-112): ``popsize x n_parameters`` members,
    Latin-hypercube start, dither (0.5, 1), recombination 0.7, tol 0.01, maxiter 1000, no polish; selection is
    generation-synchronous (SciPy's ``updating='deferred'``).  The host only enqueues generations, ``check_every`` at
    a time, and reads back how many basins are still searching.  Returns (x [nb, d], fun [nb], nfev [nb], nit [nb]).
    """
    d = len(bset.bounds)
    n = int(nmembers) if nmembers else max(5, popsize * d)
    if seed is None:
        seed = int.from_bytes(os.urandom(8), 'little')       # unseeded like the reference; pass a seed to reproduce
    de = bset.solver(n, seed=seed)
    try:
        de.init()
        done, left = 0, len(bset.cals)
        while done < maxiter and left > 0:
            k = min(check_every, maxiter - done)
            left = de.step(k, tol=tol, atol=atol, mutation=mutation, recombination=recombination)
            done += k
        x, fun, nfev, nit, _ = de.result()
    finally:
        de.close()
    return x, fun, nfev, nit


class Calibrate:
    """Calibrate the ABCD runoff module for one basin; constructor as calibrate_abcd.Calibrate (:20-88)."""

    def __init__(self, basin_num, basin_ids, basin_areas, precip, pet, obs, tmin, n_months, runoff_spinup,
                 set_calibrate, obs_unit, out_dir, router_func=None, device=0, seed=None, um=None, flow_dist=None,
                 velocity=None, chs_prev=None, ndays=None, routing_spinup=0, dt=10800, flow=None, gauges=None,
                 velocity_bounds=None):
        """set_calibrate = 1 also needs the routing inputs: ``um`` (routing.mrtm.upstream_genmatrix), ``flow_dist``,
        ``velocity``, ``chs_prev`` (None = zeros), ``ndays`` [nmonths] and ``routing_spinup`` -- or ``flow``, this
        basin's FlowTables.  ``router_func`` is kept for the reference's signature and not called.
        ``gauges`` (gauge_tables.Gauges; or ``flow`` = this basin's GaugeTables): score the basin at its stream gauges
        instead of its outlets; ``obs`` may then be None.
        ``velocity_bounds`` = (lo, hi), 0 < lo < hi (set_calibrate = 1 only): also calibrate the basin's velocity scale;
        the bounds list gains it as its last entry."""
        if velocity_bounds is not None:
            if set_calibrate != 1:
                raise ValueError('velocity_bounds need set_calibrate = 1: the velocity scale acts on the routing')
            velocity_bounds = check_bounds(velocity_bounds, 'velocity_bounds')
        self.velocity_bounds = velocity_bounds
        if gauges is not None and set_calibrate != 1:
            raise ValueError('gauges need set_calibrate = 1')
        if set_calibrate not in (0, 1):
            raise ValueError('set_calibrate must be 0 or 1')
        self.flow = None
        if set_calibrate == 1:
            if flow is None:
                if um is None or flow_dist is None or velocity is None or ndays is None:
                    raise ValueError('set_calibrate = 1 needs um, flow_dist, velocity and ndays (or flow)')
                check_forcing([basin_num], basin_ids, pet, precip, n_months)
                if gauges is not None:
                    flow = GaugeTables(um, basin_ids, [basin_num], gauges, flow_dist, velocity, basin_areas, chs_prev,
                                       ndays, n_months, routing_spinup, dt=dt)
                else:
                    flow = FlowTables(um, basin_ids, [basin_num], flow_dist, velocity, basin_areas, chs_prev, ndays,
                                      n_months, routing_spinup, dt=dt)
            self.flow = flow
        self.basin_num, self.n_months, self.runoff_spinup = basin_num, n_months, runoff_spinup
        self.set_calibrate, self.obs_unit, self.out_dir, self.seed = set_calibrate, obs_unit, out_dir, seed
        self.nosnow = tmin is None
        self.bounds = [(LB, UB), (LB, 8 - LB), (LB, UB), (LB, UB), (LB, UB)]          # :62-64
        if self.nosnow:
            self.bounds.pop()
        self.all_pars = np.zeros((1, len(self.bounds)))                               # the ABCD columns only
        self.velocity_scale = np.ones(1)
        if velocity_bounds is not None:
            self.bounds.append(velocity_bounds)
        self.kge_vals = np.zeros(1)
        self.basin_idx = np.where(np.asarray(basin_ids) == basin_num)
        self.bsn_areas = np.asarray(basin_areas)[self.basin_idx]
        self.bsn_PET = np.asarray(pet)[self.basin_idx]
        self.bsn_P = np.asarray(precip)[self.basin_idx]
        self.bsn_TMIN = None if self.nosnow else np.asarray(tmin)[self.basin_idx]
        if getattr(self.flow, 'gauge_form', False):
            self.bsn_Robs = None                                                      # the records are in the gauge tables
        else:
            obs = np.asarray(obs)
            self.bsn_Robs = obs[np.where(obs[:, 0] == basin_num)][:n_months, 1]       # :88
        self.device = device
        self.nfev = 0

    def objective(self):
        return BasinObjective(self.bsn_PET, self.bsn_P, self.bsn_TMIN, self.n_months, self.runoff_spinup,
                              self.obs_unit, self.bsn_areas, self.bsn_Robs, device=self.device,
                              set_calibrate=self.set_calibrate)

    def calibrate_basin(self, popsize=15, polish=False):
        """Optimise (a, b, c, d[, m]) for maximum KGE and save the results (:90-131)."""
        if polish:
            raise NotImplementedError('polish=True (L-BFGS-B after the search) is not offered; the reference default is False')
        st = time.time()
        bset = BasinSet([self], self.n_months, self.runoff_spinup, self.obs_unit)
        try:
            x, ed, nfev, nit = differential_evolution_device(bset, popsize=popsize, seed=self.seed)
        finally:
            bset.close()
        self._store(x[0], ed[0], int(nfev[0]))
        logging.debug('\t\tFinished calibration for basin {0} which contains {1} grid cells.'.format(
            self.basin_num, self.basin_idx[0].shape[0]))
        logging.debug('\t\tPopulation size:  {}'.format(popsize))
        logging.debug('\t\tParameter values ({}):  {}'.format(
            ','.join(list(self.par_names()) + ['v'] * (self.velocity_bounds is not None)), x[0]))
        logging.debug('\t\tKGE:  {}'.format(1 - ed[0]))
        logging.debug('\t\tNumber of function evaluations:  {} in {} generations'.format(int(nfev[0]), int(nit[0])))
        logging.debug('\t\tCalibration time (seconds):  {}'.format(time.time() - st))

    def par_names(self):
        return 'abcd' + 'm' * (not self.nosnow)

    def _store(self, x, ed, nfev, save=True):
        """x = the best vector: the ABCD parameters, then the velocity scale if it was calibrated."""
        nabcd = self.all_pars.shape[1]
        self.all_pars[0, :] = x[:nabcd]
        if self.velocity_bounds is not None:
            self.velocity_scale[0] = x[nabcd]
        self.kge_vals[0] = 1 - ed
        self.nfev = nfev
        if save and self.out_dir is not None:
            os.makedirs(self.out_dir, exist_ok=True)
            np.save('{}/kge_result_basin_{}.npy'.format(self.out_dir, self.basin_num), self.kge_vals)
            np.save('{}/{}_parameters_basin_{}.npy'.format(self.out_dir, self.par_names(), self.basin_num), self.all_pars)
            if self.velocity_bounds is not None:
                np.save('{}/velocity_scale_basin_{}.npy'.format(self.out_dir, self.basin_num), self.velocity_scale)


def objective_kge(pars, pet, precip, tmin, n_months, runoff_spinup, obs_unit, bsn_areas, bsn_robs, device=0):
    """Single evaluation of the reference's objective_kge (:176-213) for set_calibrate = 0."""
    obj = BasinObjective(pet, precip, tmin, n_months, runoff_spinup, obs_unit, bsn_areas, bsn_robs, device=device)
    try:
        return float(obj(np.asarray(pars)[None, :])[0])
    finally:
        obj.close()


def expand_str_range(str_ranges):
    """['0-2', '6'] -> [0, 1, 2, 6] (:235-253)."""
    out = []
    for r in str_ranges:
        if '-' in r:
            a, b = r.split('-')
            out.extend(range(int(a), int(b) + 1))
        else:
            out.append(int(r))
    return out


def settings_velocity_bounds(settings, velocity_bounds=None):
    """The velocity bounds of a run: the keyword if given, else ``settings.velocity_scale_bounds`` (default 0.25, 4) when
    ``settings.calibrate_velocity`` is on, else None."""
    if velocity_bounds is not None:
        return check_bounds(velocity_bounds, 'velocity_bounds')
    if getattr(settings, 'calibrate_velocity', 0):
        return check_bounds(getattr(settings, 'velocity_scale_bounds', None) or DEFAULT_BOUNDS)
    return None


def process_basin(basin_num, settings, data, pet, router_function=None, um=None, ndays=None, dt=10800,
                  velocity_bounds=None):
    flow = None
    if settings.set_calibrate == 1:
        flow = flow_tables(settings, data, pet, [basin_num], um, ndays, dt)
    cal = Calibrate(basin_num=basin_num, set_calibrate=settings.set_calibrate, obs_unit=settings.obs_unit,
                    basin_ids=data.basin_ids, basin_areas=data.area, precip=data.precip, pet=pet,
                    obs=getattr(data, 'cal_obs', None), tmin=data.tmin, n_months=settings.nmonths,
                    runoff_spinup=settings.runoff_spinup, router_func=router_function, out_dir=settings.calib_out_dir,
                    device=getattr(settings, 'device', 0), flow=flow,
                    velocity_bounds=settings_velocity_bounds(settings, velocity_bounds))
    cal.calibrate_basin()
    return cal


def flow_tables(settings, data, pet, basins, um, ndays, dt=10800):
    """set_calibrate = 1: check the forcing of ``basins`` and build their closure tables from the run's routing inputs
    (``um`` = the topology routing uses, ``ndays`` [nmonths] the days of each month)."""
    if um is None or ndays is None:
        raise ValueError('set_calibrate = 1 needs the routing topology (um) and the day counts (ndays)')
    check_forcing(basins, data.basin_ids, pet, data.precip, settings.nmonths)
    gauges = getattr(data, 'gauges', None)
    if gauges is not None:      # scored at stream gauges: union closures of each basin's gauges
        return GaugeTables(um, data.basin_ids, basins, gauges, data.flow_dist, data.str_velocity, data.area,
                           getattr(data, 'chs_prev', None), ndays, settings.nmonths,
                           getattr(settings, 'routing_spinup', 0), dt=dt)
    return FlowTables(um, data.basin_ids, basins, data.flow_dist, data.str_velocity, data.area,
                      getattr(data, 'chs_prev', None), ndays, settings.nmonths, getattr(settings, 'routing_spinup', 0),
                      dt=dt)


def assign_basins(sizes, n_ranks):
    """Largest-first onto the least-loaded rank (LPT) by ``sizes`` (cells x months). Returns rank of each basin."""
    sizes = np.asarray(sizes, dtype=np.int64)
    load = np.zeros(n_ranks, dtype=np.int64)
    owner = np.empty(len(sizes), dtype=np.int64)
    for b in np.argsort(-sizes, kind='stable'):
        r = int(np.argmin(load))
        owner[b] = r
        load[r] += sizes[b]
    return owner


def gather_results(local, owner, group, root=0):
    """Gather per-basin result rows to ``root``: local [n_local, w] in the rank's basin order -> [n_basins, w].

    ONE collective of ``n_basins x (n_par + 3)`` doubles in all through the job's process group (``group``:
    ``launch.SocketGroup`` or anything with ``rank`` and ``gather``): every rank sends its own rows, the root puts them
    where ``owner`` says."""
    owner = np.asarray(owner)
    got = group.gather(np.ascontiguousarray(local, dtype=np.float64), root=root)
    if group.rank != root:
        return None
    table = np.zeros((len(owner), local.shape[1]))
    for r, rows in enumerate(got):
        table[np.nonzero(owner == r)[0]] = rows
    return table


def _make_calibrate(b, settings, data, pet, flow=None, velocity_bounds=None):
    return Calibrate(basin_num=b, set_calibrate=settings.set_calibrate, obs_unit=settings.obs_unit,
                     basin_ids=data.basin_ids, basin_areas=data.area, precip=data.precip, pet=pet,
                     obs=getattr(data, 'cal_obs', None), tmin=data.tmin, n_months=settings.nmonths,
                     runoff_spinup=settings.runoff_spinup, out_dir=settings.calib_out_dir, device=getattr(settings, 'device', 0),
                     flow=None if flow is None else flow.subset([b]), velocity_bounds=velocity_bounds)


def _calibrate_local(mine, settings, data, pet, seed, popsize, nmembers, flow=None, velocity_bounds=None):
    """This rank's share: rows [len(mine), npar + 3] = (parameters, ED, nfev, nit) and {basin: Calibrate}.
    ``flow`` (set_calibrate = 1): the closure tables of at least these basins.  With ``velocity_bounds`` the parameters
    end in the velocity scale and a row is one column longer."""
    npar = (5 if data.tmin is not None else 4) + (1 if velocity_bounds is not None else 0)
    if not mine:
        return np.zeros((0, npar + 3)), {}
    cals = [_make_calibrate(b, settings, data, pet, flow, velocity_bounds) for b in mine]
    bset = BasinSet(cals, settings.nmonths, settings.runoff_spinup, settings.obs_unit,
                    flow=None if flow is None else flow.subset(mine))
    try:
        x, ed, nfev, nit = differential_evolution_device(bset, popsize=popsize, seed=seed, nmembers=nmembers)
    finally:
        bset.close()
    return np.column_stack([x, ed, nfev, nit]), dict(zip(mine, cals))


def calibrate_all(settings, data, pet, router_function=None, seed=None, popsize=15, nmembers=None, group=None, um=None,
                  ndays=None, dt=10800, velocity_bounds=None):
    """Calibrate every requested basin (:256-262).

    All basins search in lock-step on the device (differential_evolution_device).  ``group`` = the job's process group
    (``launch.current_group()``; None = one rank): the basins are dealt to the ranks by size (every rank needs the same
    ``seed``), each rank calibrates its share on its own GPU, and rank 0 receives all results in one collective.  Writes the
    reference's two files per basin (:130-131; on rank 0) and returns {basin: (parameters, kge)} (rank 0; {} elsewhere).
    set_calibrate = 1 also needs ``um`` (the routing topology), ``ndays`` [nmonths] and ``dt``; ``data`` then carries
    flow_dist, str_velocity and chs_prev, and the basins are dealt by closure cells x (nmonths + routing_spinup).
    With ``data.gauges`` (gauge_tables.Gauges) the basins are scored at their stream gauges (union closures; dealt by
    union-closure cells x (nmonths + routing_spinup)) and rank 0 also writes ``gauge_kge.csv`` to ``calib_out_dir``: per
    gauge its id, basin, cell (1-based), months used and KGE at the basin's best parameters.
    ``velocity_bounds`` = (lo, hi) (or ``settings.calibrate_velocity`` with ``settings.velocity_scale_bounds``;
    set_calibrate = 1 only): the basins' velocity scales are calibrated too.  The returned parameters then end in v, each
    basin also gets ``velocity_scale_basin_N.npy``, and rank 0 writes ``velocity_scale.csv`` to ``calib_out_dir``: one row
    for every basin of the grid, the calibrated basins with v times the scale the run had loaded (``data.velocity_scale``,
    else 1) and every other basin with its loaded scale, so that the file is the next run's ``[[mrtm]] velocity_scale``.
    """
    if settings.set_calibrate not in (0, 1):
        raise ValueError('set_calibrate must be 0 or 1')
    basins = expand_str_range(settings.cal_basins)
    basin_ids = np.asarray(data.basin_ids)
    sizes = np.array([(basin_ids == b).sum() for b in basins])
    basins = [b for b, n in zip(basins, sizes) if n > 0]
    sizes = sizes[sizes > 0]
    if not basins:
        return {}
    rank, n_ranks = (group.rank, group.size) if group is not None else (0, 1)
    if n_ranks > 1 and seed is None:
        raise ValueError('a multi-rank calibration needs the same explicit seed on every rank')
    st = time.time()
    vb = settings_velocity_bounds(settings, velocity_bounds)
    if vb is not None and settings.set_calibrate != 1:
        raise ValueError('velocity bounds need set_calibrate = 1: the velocity scale acts on the routing')
    nabcd = 5 if data.tmin is not None else 4
    npar = nabcd + (1 if vb is not None else 0)                  # the search's parameters: v last
    if settings.set_calibrate == 1:
        flow = flow_tables(settings, data, pet, basins, um, ndays, dt)
        owner = assign_basins(flow.weights, n_ranks)
        mine = [b for b, r in zip(basins, owner) if r == rank]
        local, cals = _calibrate_local(mine, settings, data, pet, seed, popsize, nmembers, flow=flow, velocity_bounds=vb)
    else:
        flow = None
        owner = assign_basins(sizes * settings.nmonths, n_ranks)
        mine = [b for b, r in zip(basins, owner) if r == rank]
        local, cals = _calibrate_local(mine, settings, data, pet, seed, popsize, nmembers)
    table = gather_results(local, owner, group) if n_ranks > 1 else local
    if rank != 0:
        return {}
    logging.info('\tCalibrated {} basins on {} GPU(s) in {:.1f} s ({} objective evaluations)'.format(
        len(basins), n_ranks, time.time() - st, int(table[:, npar + 1].sum())))
    results = {}
    for b, row in zip(basins, table):
        c = cals[b] if b in cals else _make_calibrate(b, settings, data, pet, flow, vb)
        c._store(row[:npar], row[npar], int(row[npar + 1]))
        results[b] = (row[:npar].copy(), 1 - row[npar])
    if getattr(flow, 'gauge_form', False) and settings.calib_out_dir is not None:
        write_gauge_kge(os.path.join(settings.calib_out_dir, 'gauge_kge.csv'), flow,
                        gauge_kge(basins, table[:, :npar], settings, data, pet, flow, velocity_bounds=vb))
    if vb is not None and settings.calib_out_dir is not None:
        n_basins = int(getattr(settings, 'n_basins', 0) or basin_ids.max())
        write_velocity_scale(os.path.join(settings.calib_out_dir, 'velocity_scale.csv'),
                             combined_scales(getattr(data, 'velocity_scale', None), basins, table[:, nabcd], n_basins))
    return results


def gauge_kge(basins, best, settings, data, pet, flow, velocity_bounds=None):
    """KGE of every gauge of ``flow`` (GaugeTables of ``basins``) at its basin's parameters ``best`` [nbasins, npar]
    (with ``velocity_bounds``: [nbasins, npar + 1], the velocity scale included): one evaluation of one member per basin."""
    cals = [_make_calibrate(b, settings, data, pet, flow, velocity_bounds) for b in basins]
    bset = BasinSet(cals, settings.nmonths, settings.runoff_spinup, settings.obs_unit, flow=flow.subset(basins))
    try:
        _, edg = bset.evaluate(np.asarray(best)[:, None, :], want_gauges=True)
    finally:
        bset.close()
    return 1 - edg[:, 0]


def write_gauge_kge(path, flow, kge):
    """gauge_kge.csv: gauge_id, basin, cell_id (1-based, as the coordinates' first column), months_used, kge."""
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'w') as fh:
        fh.write('gauge_id,basin,cell_id,months_used,kge\n')
        for gid, b, c, n, k in zip(flow.gauge_id, flow.gauge_basin, flow.gauge_cell, flow.months_used, kge):
            fh.write('{},{},{},{},{!r}\n'.format(int(gid), int(b), int(c) + 1, int(n), float(k)))
