"""Components: the harness of the PET -> runoff -> routing path (mirror of xanthos/components.py:29-497).

Same selectors (``pet_module = pm``, ``runoff_module = abcd``, ``routing_module = mrtm``), same methods
(``calculate_pet``, ``calculate_runoff``, ``calculate_routing``, ``simulation``, ``calibrate``) and same result
attributes (``PET, AET, Q, Sav, ChStorage, Avg_ChFlow`` as host float64 ``[ncell, nmonths]``, components.py:95-100).
``import_core`` binds the module globals ``pet_mod / runoff_mod / routing_mod`` to this package's plugins, which call
the HIP kernels through the C-ABI.  ``simulation`` keeps the arrays in HBM between the three stages (one upload of
the forcing, one download of the six outputs); the per-stage ``calculate_*`` methods remain for callers that drive
the stages one by one (the calibration routing callback, components.py:486-497).
"""
import logging
import time
from types import SimpleNamespace

import numpy as np

from . import _hip, dist, launch
from .calibrate import calibrate_abcd as calib_mod
from .data_load import DataLoader
from .ini_reader import ValidationException, check_modules
from .pipeline import DevicePipeline
from .utils import set_month_arrays

HGM_PET = ('hargreaves', 'hs', 'thornthwaite')      # PET modules that run device resident with any runoff module

# DevicePipeline forcing name -> DataLoader attribute, per PET / runoff module
_FORCING_DATA = {'pm': {'tas': 'tair_load', 'tmin': 'TMIN_load', 'rhs': 'rhs_load', 'wind': 'wind_load',
                        'rsds': 'rsds_load', 'rlds': 'rlds_load'},
                 'hargreaves': {'temp': 'temp', 'dtr': 'dtr'}, 'hs': {'tas': 'hs_tas', 'tmax': 'hs_tmax', 'tmin': 'hs_tmin'},
                 'thornthwaite': {'tas': 'tair'}, 'abcd': {'precip': 'precip', 'abcd_tmin': 'tmin'},
                 'gwam': {'precip': 'precip'}, 'none': {}}

# DevicePipeline forcing name -> (setting that names its file or array, setting of its NetCDF variable, the loader's
# nan_to_num), per module: how the loader fills the attributes above (data_load.py), for a caller that loads one member's
# forcing without a second DataLoader (ensemble.py)
_FORCING_SETTINGS = {'pm': {k: ('pm_' + k, None, True) for k in ('tas', 'tmin', 'rhs', 'wind', 'rsds', 'rlds')},
                     'hargreaves': {'temp': ('TemperatureFile', 'TempVarName', False),
                                    'dtr': ('DailyTemperatureRangeFile', 'DTRVarName', False)},
                     'hs': {k: ('hs_' + k, None, False) for k in ('tas', 'tmax', 'tmin')},
                     'thornthwaite': {'tas': ('trn_tas', None, True)},
                     'abcd': {'precip': ('PrecipitationFile', 'PrecipVarName', False),
                              'abcd_tmin': ('TempMinFile', 'TempMinVarName', True)},
                     'gwam': {'precip': ('PrecipitationFile', 'PrecipVarName', False)}, 'none': {}}

pet_mod = runoff_mod = routing_mod = None

_TOPOLOGIES = {}      # (digest of coords + flow directions, grid shape) -> (dsid, upid, UM with its cached device plan)

# result attribute -> name of the array in the device pipeline
_RESULTS = {'PET': 'pet', 'AET': 'aet', 'Q': 'q', 'Sav': 'sav', 'ChStorage': 'chs', 'Avg_ChFlow': 'avg'}


def runs_device_resident(s, run_pet=True, run_runoff=True):
    """Whether ``Components.simulation`` keeps this configuration in HBM from the forcing to the six outputs: Hargreaves,
    Hargreaves-Samani or Thornthwaite PET with any runoff module, or PM -> ABCD.  Anything else (a PET file, PM without
    ABCD) runs stage by stage on host arrays."""
    return bool(run_pet) and (s.pet_module in HGM_PET or (s.pet_module == 'pm' and s.runoff_module == 'abcd' and bool(run_runoff)))


def _result(attr):
    """Host float64 [ncell, nmonths] result attribute (components.py:95-100).  After a device-resident simulation the
    array is fetched from HBM the first time it is read: a run that writes two of the six variables moves two across PCIe."""
    def get(self):
        if attr not in self._host:
            pipe = self.pipe
            key = _RESULTS[attr]
            if pipe is not None and (key in ('pet', 'aet', 'q', 'sav') or pipe.plan is not None):
                t = time.time()
                self._host[attr] = pipe.out[key].download()
                self.timings['download'] = self.timings.get('download', 0.0) + time.time() - t
            else:
                self._host[attr] = np.zeros((self.s.ncell, self.s.nmonths))
        return self._host[attr]

    def put(self, value):
        self._host[attr] = value
    return property(get, put)


class Components:
    PET, AET, Q, Sav = _result('PET'), _result('AET'), _result('Q'), _result('Sav')
    ChStorage, Avg_ChFlow = _result('ChStorage'), _result('Avg_ChFlow')

    def __init__(self, config, gauges=None):
        """``gauges``: the checked gauge set of [Evaluate] when the caller has loaded it already (the ensemble driver)."""
        self.s = config
        self.import_core()
        self.timings = {}                  # seconds per phase of run_model(): load, topology, plan, upload, kernels, download, ...
        t0 = time.time()
        self.data = DataLoader(config)
        self.timings['load'] = time.time() - t0
        self.yr_imth_dys = set_month_arrays(self.s.nmonths, self.s.StartYear, self.s.EndYear)
        self.routing_timestep_hours = 3 * 3600          # seconds, despite the name (components.py:91)
        self._host = {}                    # result arrays already on the host (the rest: zeros, or still in HBM)
        self.pipe = None                   # DevicePipeline of the last device-resident simulation
        self.um = self.dsid = self.upid = None
        self.instream_flow = None
        self._writer = None                # OutWriter of output_simulation(): q / ac come from it
        self._q = self._ac = None
        # several ranks (one process per GPU, started by launch.spawn / any launcher that sets RANK, WORLD_SIZE, ...): the
        # basins are sharded over them and rank 0 ends up with the gathered outputs, writes the files and runs the
        # post-processors; the other ranks have nothing to write
        self.group = launch.current_group()
        self.is_root = self.group is None or self.group.rank == 0
        self.gather = None
        # GriddedOutput = 1: the one map of cells to grid slots that every writer of this run takes (validated here, before
        # anything is computed)
        self.grid = None
        if getattr(config, 'GriddedOutput', 0) and self.is_root:
            from .data_writer.gridded import GridMap
            self.grid = GridMap(self.data.coords, config.ngridrow, config.ngridcol)
        # [Evaluate]: the stream gauges the routed flow is scored at (loaded and checked here, before anything is computed),
        # and what evaluate() leaves: gauge_skill {column: ndarray [ngauge]} and gauge_flow [ngauge, nmonths]
        self.gauges = gauges
        self.gauge_skill = self.gauge_flow = None
        if gauges is None and getattr(config, 'evaluate', None) and self.is_root:
            from .evaluate import load_gauge_set
            self.gauges = load_gauge_set(config)

    @property
    def q(self):
        """Runoff as written (aggregated / converted), or Q when 'q' is not an output variable (components.py:461-466)."""
        if self._q is None and self._writer is not None:
            self._q = self._writer.get('q') if 'q' in self._writer.output_names else self.Q
        return self._q

    @property
    def ac(self):
        """Channel flow as written, or Avg_ChFlow (components.py:467-472)."""
        if self._ac is None and self._writer is not None:
            self._ac = self._writer.get('avgchflow') if 'avgchflow' in self._writer.output_names else self.Avg_ChFlow
        return self._ac

    def import_core(self):
        """Bind the selected plugins (components.py:114-142)."""
        global pet_mod, runoff_mod, routing_mod
        if self.s.pet_module == 'pm':
            from .pet import penman_monteith as pet_mod
        elif self.s.pet_module == 'hargreaves':
            from .pet import hargreaves as pet_mod
        elif self.s.pet_module == 'hs':
            from .pet import hargreaves_samani as pet_mod
        elif self.s.pet_module == 'thornthwaite':
            from .pet import thornthwaite as pet_mod
        elif self.s.pet_module != 'none':
            raise ValidationException("pet_module '{}' is not part of the MI355X hot path".format(self.s.pet_module))
        if self.s.runoff_module == 'abcd':
            from .runoff import abcd as runoff_mod
        elif self.s.runoff_module == 'gwam':
            from .runoff import gwam as runoff_mod
        elif self.s.runoff_module != 'none':
            raise ValidationException("runoff_module '{}' is not part of the MI355X hot path".format(self.s.runoff_module))
        if self.s.routing_module == 'mrtm':
            from .routing import mrtm as routing_mod
        check_modules(self.s)

    # ------------------------------------------------------------------ stage by stage (host arrays)
    def calculate_pet(self):
        """Monthly PET (components.py:189-210)."""
        if self.s.pet_module == 'pm':
            return pet_mod.run_pmpet(self.data, self.s.ncell, self.s.pm_nlcs, self.s.StartYear, self.s.EndYear,
                                     self.s.pm_water_idx, self.s.pm_snow_idx, self.s.pm_lc_years, device=self.s.device)
        if self.s.pet_module == 'hargreaves':
            return pet_mod.run_hargreaves(self.data.temp, self.data.dtr, self.data.lat_radians, self.s.StartYear,
                                          self.s.EndYear, device=self.s.device)
        if self.s.pet_module == 'hs':
            return pet_mod.execute(self.s, self.data)
        if self.s.pet_module == 'thornthwaite':
            return pet_mod.execute(self.data.tair, self.data.lat_radians, self.s.StartYear, self.s.EndYear,
                                   daylight=self.s.trn_daylight, device=self.s.device)
        if self.s.pet_module == 'none':
            return self.data.pet_out

    def calculate_runoff(self, step_num=None, pet=None):
        """ABCD over all months (components.py:212-247)."""
        if self.s.runoff_module == 'abcd':
            rg = runoff_mod.abcd_execute(n_basins=self.s.n_basins, basin_ids=self.data.basin_ids, pet=pet,
                                         precip=self.data.precip, tmin=self.data.tmin, calib_file=self.s.calib_file,
                                         n_months=self.s.nmonths, spinup_steps=self.s.runoff_spinup, jobs=self.s.ro_jobs)
            self.PET, self.AET, self.Q, self.Sav = rg
        elif self.s.runoff_module == 'gwam':
            self._check_gwam_spinup()
            rg = runoff_mod.gwam_execute(pet, self.data.precip, self.data.soil_moisture, self.data.sm_prev,
                                         self.s.runoff_spinup, self.s.nmonths, precipitation=self.s.gwam_precipitation,
                                         device=self.s.device)
            self.PET, self.AET, self.Q, self.Sav = rg
        elif getattr(self.s, 'alt_runoff', None) is not None:
            self.Q = np.load(self.s.alt_runoff)

    def topology(self):
        """dsid -> upid -> UM, built once per Components (the reference rebuilds it on every call, :268-270) -- and once
        per process for one grid: the UM of the last two distinct (coords, flow directions) is kept with its device
        routing plan, so a second run_model() on the same grid (a scenario sweep) does not partition the networks again."""
        if self.um is None:
            import hashlib
            h = hashlib.blake2b(digest_size=16)
            for a in (self.data.coords, self.data.flow_dir):
                h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
            key = (h.hexdigest(), int(self.s.ngridrow), int(self.s.ngridcol))
            hit = _TOPOLOGIES.get(key)
            if hit is None:
                dsid = routing_mod.downstream(self.data.coords, self.data.flow_dir, self.s)
                upid = routing_mod.upstream(self.data.coords, dsid, self.s)
                hit = (dsid, upid, routing_mod.upstream_genmatrix(upid))
                while len(_TOPOLOGIES) >= 2:
                    _TOPOLOGIES.pop(next(iter(_TOPOLOGIES)))
                _TOPOLOGIES[key] = hit
            self.dsid, self.upid, self.um = hit
        return self.um

    def route_flags(self):
        """[[mrtm]] routing_form -> flag of xh_route_series (0: the library default)."""
        return {'reassociated': _hip.XH_ROUTE_REASSOC, 'exact': _hip.XH_ROUTE_EXACT}.get(getattr(self.s, 'routing_form', 'default'), 0)

    def calculate_routing(self, runoff):
        """Spin-up + simulation of MRTM over all months (components.py:249-296). Returns Avg_ChFlow."""
        if self.s.routing_module == 'mrtm':
            um = self.topology()
            chs, avg, fend = routing_mod.route_series(um, self.data.flow_dist, self.data.str_velocity, self.data.area,
                                                      runoff, self.yr_imth_dys[:, 2], self.s.routing_spinup,
                                                      S0=self.data.chs_prev, dt=self.routing_timestep_hours,
                                                      device=self.s.device, flags=self.route_flags())
            self.ChStorage, self.Avg_ChFlow, self.instream_flow = chs, avg, fend
            return self.Avg_ChFlow

    # ------------------------------------------------------------------ whole simulation, device resident
    def simulation(self, run_pet=True, run_runoff=True, run_routing=True, pet_num_steps=0, runoff_num_steps=0,
                   routing_num_steps=0, notify='simulation'):
        """Run the configured stages (components.py:298-384).  Hargreaves, Hargreaves-Samani or Thornthwaite PET (-> GWAM /
        ABCD / no runoff) and PM -> ABCD run device resident: one upload of the forcing, the outputs left in HBM.  GWAM's
        spin-up pass and its simulation are one xh_gwam call; the spin-up pass's routing is skipped -- it changes nothing
        (streamrouting does not mutate its inputs and calculate_routing starts again from data.chs_prev).  Anything else
        runs stage by stage on host arrays.
        On several ranks (PM -> ABCD only) ``dist.make_shards`` deals connected components of (same basin) U (flow edge)
        onto the ranks -- the reference's only parallel seam is the basin chunking of abcd.py:369-389; every rank reads
        only its rows of the forcing, runs the pipeline, and the six outputs travel to rank 0 in one RCCL gather (PET /
        AET / Q / Sav beside the routing, ChStorage / Avg_ChFlow behind it), where they sit in HBM in grid order exactly
        as a one-rank run leaves them."""
        if self.s.calibrate:
            self.calibrate()
            return
        logging.info('---{} in progress...'.format(notify))
        t0 = time.time()
        s, group = self.s, self.group
        if not runs_device_resident(s, run_pet, run_runoff):
            pet_out = self.calculate_pet()
            if run_runoff:
                self.calculate_runoff(pet=pet_out)
            if run_routing and s.routing_module == 'mrtm':
                self.calculate_routing(self.Q)
            return
        runoff = s.runoff_module if run_runoff else 'none'
        sharded = group is not None and group.size > 1
        self.check_resident(runoff, sharded)
        ctx = _hip.get_context(s.device)
        t = time.time()
        um = self.topology() if (run_routing and s.routing_module == 'mrtm') else None
        self.timings['topology'] = time.time() - t
        t = time.time()
        shards = cells = None
        if sharded:
            shards = dist.make_shards(SimpleNamespace(basin_ids=np.asarray(self.data.basin_ids)), um, group.size)
            cells = shards[group.rank].cells
        pipe = DevicePipeline(ctx, **self._pipeline_args(runoff, um, cells))
        ctx.sync()
        self.timings['plan'] = time.time() - t          # static uploads; the routing partition runs on a host thread meanwhile
        t = time.time()
        pipe.set_forcing(*self._forcing(runoff, cells))
        ctx.sync()
        self.timings['upload'] = time.time() - t
        t = time.time()
        gather = None
        if sharded:
            gather = dist.OutputGather(ctx, pipe, shards, group, s.ncell,
                                       names=('pet', 'aet', 'q', 'sav') + (('chs', 'avg') if um is not None else ()))
        pipe.plan                                       # waits for the partition if it is still being made
        self.timings['plan_wait'] = time.time() - t
        t = time.time()
        ctx.timing_reset()
        # one rank runs the stages strictly in order; a sharded run leaves XH_FUSED its say
        pipe.run(fed=False, fused=None if sharded else False, after_runoff=gather.run_side if sharded else None)
        if sharded:
            gather.run_tail()
        ctx.sync()
        if sharded:
            group.barrier()
        self.timings['kernels'] = time.time() - t
        where = ' and the gather ({}), {} of {} cells on this rank'.format(gather.kind, pipe.ncell, s.ncell) if sharded else ''
        logging.info('\tPET + runoff + routing kernels{}: {:.3f} seconds'.format(where, time.time() - t))
        # one line per stage: kernel time (HIP events on the library's stream) and achieved HBM GB/s against the
        # algorithmic bytes of the stage
        for name, nbytes in pipe.stage_traffic():
            ms, n = ctx.timing(name)
            if n:
                logging.info('\t{:14s} {:8.3f} ms, {:7.1f} GB/s of {} MB algorithmic traffic'.format(
                    name, ms / n, nbytes / (ms / n) / 1e6, nbytes // 1000000))
                self.timings['kernel_' + name] = ms / n / 1e3
        self._host = {}                    # the six results stay in HBM until they are read (or written)
        self.pipe = pipe
        if sharded:
            self.gather, self.shard_pipe = gather, pipe
            # what the result properties and the writer look at: on the root the gathered arrays, in HBM, in grid order
            self.pipe = SimpleNamespace(out=gather.out, plan=pipe.plan, ncell=s.ncell, nmonths=s.nmonths) if self.is_root else None
        self.timings['download'] = 0.0
        logging.info('---{0} has finished successfully: {1} seconds ---'.format(notify, time.time() - t0))

    def check_resident(self, runoff, sharded=False):
        """What a device-resident run of Hargreaves / Hargreaves-Samani / Thornthwaite PET checks before it touches the
        device: one GPU, and spin-ups inside the series."""
        s = self.s
        if s.pet_module in HGM_PET:
            if sharded:
                raise ValidationException('{}: {} PET and {} runoff run on one GPU; sharding them over several GPUs is not '
                                          'implemented.'.format(s.mod_cfg, s.pet_module, s.runoff_module))
            if runoff == 'gwam':
                self._check_gwam_spinup()
            elif runoff == 'abcd':
                from .runoff import abcd as abcd_mod
                abcd_mod._check_spinup(s.runoff_spinup, s.nmonths)

    def member_view(self, settings, pipe):
        """A Components of the same grid and static data whose results are ``pipe.out`` (anything with ``out``, ``plan``,
        ``ncell``, ``nmonths``) and whose settings are ``settings``: what the post-processors and the writer of one
        ensemble member run on.  Nothing is loaded or copied."""
        import copy
        c = copy.copy(self)
        c.s, c.pipe = settings, pipe
        c.timings, c._host = {}, {}
        c._writer = c._q = c._ac = None
        c.gauge_skill = c.gauge_flow = None
        c.__dict__.pop('drought_index', None)          # (the result of drought_index() stands in the method's place)
        c.__dict__.pop('trend', None)                  # (... and that of trend())
        c.__dict__.pop('extremes', None)               # (... and that of extremes())
        c.__dict__.pop('signatures', None)             # (... and that of signatures())
        c.__dict__.pop('water_balance', None)          # (... and that of water_balance())
        return c

    def _pipeline_args(self, runoff, um, cells=None):
        """DevicePipeline's keyword arguments for this configuration; ``cells``: one rank's rows of the grid."""
        s, d = self.s, self.data

        def sel(a):
            return a if cells is None or a is None else np.asarray(a)[cells]
        kw = dict(ncell=s.ncell if cells is None else len(cells), nmonths=s.nmonths, start_year=s.StartYear,
                  pet_module=s.pet_module, runoff_module=runoff)
        if s.pet_module == 'pm':
            kw.update(pm_tables=pet_mod.tables_from(d, s.pm_nlcs), lct=sel(d.lct_load), elev=sel(d.elev),
                      lc_years=s.pm_lc_years, water_idx=s.pm_water_idx, snow_idx=s.pm_snow_idx)
        else:
            kw.update(lat_radians=sel(d.lat_radians), lat_degrees=sel(d.latitude),
                      daylight=getattr(s, 'trn_daylight', 'reference'))
        if runoff == 'abcd':
            kw.update(basin_ids=sel(d.basin_ids), abcd_spinup=s.runoff_spinup, use_snow=d.tmin is not None,
                      abcd_pars=s.calib_file if isinstance(s.calib_file, np.ndarray) else np.load(s.calib_file))
        elif runoff == 'gwam':
            kw.update(sm_max=sel(d.soil_moisture), sm0=sel(d.sm_prev), gwam_spinup=s.runoff_spinup,
                      precipitation=s.gwam_precipitation)
        if um is not None:
            kw.update(um=um if cells is None else dist.sub_matrix(um, cells), flow_dist=sel(d.flow_dist),
                      velocity=sel(d.str_velocity), area=sel(d.area), routing_spinup=getattr(s, 'routing_spinup', 0),
                      chs_prev=sel(getattr(d, 'chs_prev', None)), route_flags=self.route_flags(), plan_async=True)
        return kw

    def _forcing(self, runoff, cells=None):
        """(host forcing, tairprev) for DevicePipeline.set_forcing; ``cells``: one rank's rows (of a memory map: only these
        rows are read)."""
        s, d = self.s, self.data

        def rows(a):
            return a if cells is None or a is None else np.ascontiguousarray(a[cells], dtype=np.float64)
        host = {name: rows(getattr(d, attr, None))
                for module in (s.pet_module, runoff) for name, attr in _FORCING_DATA[module].items()}
        tairprev = None
        if s.pet_module == 'pm' and cells is None:
            tairprev = d._tairprev if hasattr(d, '_tairprev') else d.tairprev_load
        elif s.pet_module == 'pm':
            # the previous CELL's temperature (data_load.py:128-129) of a shard's rows is not the row above: taken from the grid
            prev = cells - 1
            tairprev = np.ascontiguousarray(d.tair_load[np.maximum(prev, 0)], dtype=np.float64)
            tairprev[prev < 0] = 0.0
        return host, tairprev

    def _check_gwam_spinup(self):
        n = self.s.runoff_spinup
        if n < 1 or n > self.s.nmonths:
            # the reference dies here: an IndexError in its PET step loop beyond the last month (components.py:330-340),
            # an AttributeError with no step at all (:337-340 take the whole-series branch, which Hargreaves lacks)
            raise ValidationException('[[gwam]] runoff_spinup = {} must lie in [1, nmonths = {}].'.format(n, self.s.nmonths))

    def calibrate(self):
        """Calibrate the ABCD parameters per basin (components.py:486-497)."""
        pet_out = self.calculate_pet()
        multi = self.group is not None and self.group.size > 1
        # (several ranks: the basins are dealt over them; the search needs the same explicit seed on every rank)
        flow = {}
        if self.s.set_calibrate == 1:       # streamflow: each basin is routed on its own closure of the run's topology
            flow = dict(um=self.topology(), ndays=self.yr_imth_dys[:, 2], dt=self.routing_timestep_hours)
        calib_mod.calibrate_all(settings=self.s, data=self.data, pet=pet_out, router_function=self.calculate_routing,
                                group=self.group if multi else None, seed=20240807 if multi else None, **flow)

    def drought(self):
        """Drought statistics of runoff or soil moisture (components.py:391-399)."""
        if self.s.CalculateDroughtStats and self.is_root:
            from .drought.drought_stats import DroughtStats
            logging.info('---Start Drought Statistics:')
            t0 = time.time()
            DroughtStats(self.s, self.Q, self.Sav)
            logging.info('---Drought Statistics has finished successfully: %s seconds ------' % (time.time() - t0))

    def drought_index(self, keep_on_device=False, write_files=True):
        """Standardized drought indices of [DroughtIndex] (not in the reference): SRI / SSI / SSFI of the run's runoff, soil
        moisture or routed flow, SPI of its precipitation or SPEI of precipitation minus PET (subtracted inside the kernel),
        from the arrays in HBM.  Leaves the result as the ATTRIBUTE ``drought_index`` of this
        object, {scale: ndarray [ncell, nmonths]} (or DeviceArrays with ``keep_on_device``), in place of this method, and
        the fitted tables as ``drought_index_parameters`` ({scale: [ncell, 12, 4]} or None)."""
        if getattr(self.s, 'CalculateDroughtIndex', 0) and self.is_root:
            from .drought.standardized import StandardizedIndex
            logging.info('---Start Drought Index:')
            t0 = time.time()
            var = self.s.drought_index['var']
            minus = None
            if var in ('precip', 'balance'):
                rows = self._precipitation(var)
                if var == 'balance':
                    minus = self.pipe.out[_RESULTS['PET']] if self.pipe is not None and 'PET' not in self._host else self.PET
            elif var == 'q':
                rows = self._runoff()
            elif var == 'avgchflow':
                rows = self._routed_flow()
            else:
                rows = self.pipe.out[_RESULTS['Sav']] if self.pipe is not None and 'Sav' not in self._host else self.Sav
            res = StandardizedIndex(self.s, rows, keep_on_device=keep_on_device, write_files=write_files, grid=self.grid,
                                    minus=minus)
            self.drought_index, self.drought_index_parameters = res.index, res.parameters
            logging.info('---Drought Index has finished successfully: %s seconds ------' % (time.time() - t0))

    def trend(self):
        """Trend tables of [Trend] (not in the reference): the Mann-Kendall test and the Theil-Sen slope per cell of the
        run's runoff, PET, AET, soil moisture, routed flow or precipitation, from the arrays in HBM.  Leaves the result as
        the ATTRIBUTE ``trend`` of this object, {(var, series): ndarray [ncell, 10]}, in place of this method."""
        if getattr(self.s, 'CalculateTrend', 0) and self.is_root:
            from .trend import Trend
            logging.info('---Start Trend:')
            t0 = time.time()

            def result(attr):
                if self.pipe is not None and attr not in self._host:
                    return self.pipe.out[_RESULTS[attr]]
                return getattr(self, attr)
            rows_of = {'q': self._runoff, 'avgchflow': self._routed_flow, 'precip': lambda: self._precipitation('precip', 'Trend'),
                       'pet': lambda: result('PET'), 'aet': lambda: result('AET'), 'soilmoisture': lambda: result('Sav')}
            tables = {}
            for var in self.s.trend['vars']:
                for series, table in Trend(self.s, var, rows_of[var]()).tables.items():
                    tables[(var, series)] = table
            self.trend = tables
            logging.info('---Trend has finished successfully: %s seconds ------' % (time.time() - t0))

    def extremes(self):
        """Extremes of [Extremes] (not in the reference): annual maxima or minima per cell of the run's runoff, PET, AET, soil
        moisture, routed flow or precipitation, the GEV fitted to them by L-moments, return levels and every year's return
        period, from the arrays in HBM.  Leaves the result as the ATTRIBUTE ``extremes`` of this object, {(var, kind):
        {'table': [ncell, 8 + nT], 'annual': [ncell, nyear], 'return_period': [ncell, nyear]}}, in place of this method; with
        ``bootstrap`` in the section (the settings' ``extremes_bootstrap``, which Extremes reads) every entry also holds 'ci':
        [ncell, 3 + 2 nT], the bootstrap intervals of the shape and the return levels."""
        if getattr(self.s, 'CalculateExtremes', 0) and self.is_root:
            from .extremes import Extremes
            logging.info('---Start Extremes:')
            t0 = time.time()

            def result(attr):
                if self.pipe is not None and attr not in self._host:
                    return self.pipe.out[_RESULTS[attr]]
                return getattr(self, attr)
            rows_of = {'q': self._runoff, 'avgchflow': self._routed_flow, 'precip': lambda: self._precipitation('precip', 'Extremes'),
                       'pet': lambda: result('PET'), 'aet': lambda: result('AET'), 'soilmoisture': lambda: result('Sav')}
            results = {}
            for var in self.s.extremes['vars']:
                for kind, res in Extremes(self.s, var, rows_of[var]()).results.items():
                    results[(var, kind)] = res
            self.extremes = results
            logging.info('---Extremes has finished successfully: %s seconds ------' % (time.time() - t0))

    def signatures(self):
        """Signatures of [Signatures] (not in the reference): the flow duration curve, the variability, persistence and
        seasonality signatures and the annual totals' variation per cell of the run's runoff, PET, AET, soil moisture, routed
        flow or precipitation, from the arrays in HBM.  Leaves the result as the ATTRIBUTE ``signatures`` of this object,
        {var: {'table': [ncell, 18], 'fdc': [ncell, nP], 'regime': [ncell, 12]}}, in place of this method."""
        if getattr(self.s, 'CalculateSignatures', 0) and self.is_root:
            from .signatures import Signatures
            logging.info('---Start Signatures:')
            t0 = time.time()

            def result(attr):
                if self.pipe is not None and attr not in self._host:
                    return self.pipe.out[_RESULTS[attr]]
                return getattr(self, attr)
            rows_of = {'q': self._runoff, 'avgchflow': self._routed_flow, 'precip': lambda: self._precipitation('precip', 'Signatures'),
                       'pet': lambda: result('PET'), 'aet': lambda: result('AET'), 'soilmoisture': lambda: result('Sav')}
            results = {}
            for var in self.s.signatures['vars']:
                results[var] = Signatures(self.s, var, rows_of[var]()).results
            self.signatures = results
            logging.info('---Signatures has finished successfully: %s seconds ------' % (time.time() - t0))

    def water_balance(self):
        """Water balance of [WaterBalance] (not in the reference): the runoff ratio, the aridity and evaporative index, the
        closure of the balance, Fu's parameter and the departure from a Budyko curve, the elasticities of runoff to
        precipitation and to PET and the lag of runoff behind precipitation, per cell and per basin, from the run's
        precipitation, PET, AET and runoff in HBM.  Leaves the result as the ATTRIBUTE ``water_balance`` of this object,
        {level: {'table': [n, 21], 'annual': [n, 4, nyear], 'xcorr': [n, max_lag + 1]}}, in place of this method."""
        if getattr(self.s, 'CalculateWaterBalance', 0) and self.is_root:
            from .waterbalance import WaterBalance
            logging.info('---Start Water Balance:')
            t0 = time.time()

            def result(attr):
                if self.pipe is not None and attr not in self._host:
                    return self.pipe.out[_RESULTS[attr]]
                return getattr(self, attr)
            precip = self._precipitation('precip', 'WaterBalance')
            aet = result('AET') if self.s.runoff_module in ('abcd', 'gwam') else None     # (handed in when the run makes it)
            results = {}
            for level in self.s.water_balance['levels']:
                results[level] = WaterBalance(self.s, level, precip, result('PET'), self._runoff(), aet, area=self.data.area,
                                              basin_ids=self.data.basin_ids).results
            self.water_balance = results
            logging.info('---Water Balance has finished successfully: %s seconds ------' % (time.time() - t0))

    def _precipitation(self, var, section='DroughtIndex'):
        """The run's precipitation [ncell, nmonths] for SPI / SPEI: the forcing array in HBM after a device-resident
        simulation, the loader's host array after a run that went stage by stage.  On a sharded run every rank's pipeline
        holds its own rows of the forcing only, and nothing gathers them: refused rather than indexed in part."""
        if self.pipe is None:
            return self.data.precip
        forcing = getattr(self.pipe, 'forcing', None)
        rows = forcing.get('precip') if forcing is not None else None
        if rows is None or tuple(rows.shape) != (self.s.ncell, self.s.nmonths):
            raise ValidationException("[{}] {} = {} needs the run's whole precipitation array on one GPU: in a run "
                                      "sharded over several GPUs every rank holds its own cells' rows only.".format(
                                          section, {'DroughtIndex': 'index_var', 'Extremes': 'extreme_vars', 'Signatures': 'signature_vars', 'WaterBalance': 'levels'}.get(section, 'trend_vars'), var))
        return rows

    def accessible_water(self):
        """Accessible water per basin (components.py:401-409)."""
        if self.s.CalculateAccessibleWater and self.is_root:
            from .accessible.accessible import AccessibleWater
            logging.info('---Start Accessible Water:')
            t0 = time.time()
            AccessibleWater(self.s, self.data, self.Q)
            logging.info('---Accessible Water has finished successfully: %s seconds ------' % (time.time() - t0))

    def _routed_flow(self):
        """Avg_ChFlow for a post-processor: the DeviceArray in HBM after a device-resident simulation (on a sharded run the
        root's gathered array, in grid order), without the download the host property would make."""
        if self.pipe is not None and 'Avg_ChFlow' not in self._host and self.pipe.plan is not None:
            return self.pipe.out[_RESULTS['Avg_ChFlow']]
        return self.Avg_ChFlow

    def hydropower_potential(self):
        """Hydropower potential per GCAM region (components.py:411-419)."""
        if self.s.CalculateHydropowerPotential and self.is_root:
            from .hydropower.potential import HydropowerPotential
            logging.info('---Start Hydropower Potential:')
            t0 = time.time()
            HydropowerPotential(self.s, self._routed_flow())
            logging.info('---Hydropower Potential has finished successfully: %s seconds ------' % (time.time() - t0))

    def hydropower_actual(self):
        """Actual hydropower per GCAM region (components.py:421-429)."""
        if self.s.CalculateHydropowerActual and self.is_root:
            from .hydropower.actual import HydropowerActual
            logging.info('---Start Hydropower Actual:')
            t0 = time.time()
            HydropowerActual(self.s, self._routed_flow())
            logging.info('---Hydropower Actual has finished successfully: %s seconds ------' % (time.time() - t0))

    def evaluate(self):
        """Skill of the routed flow at the stream gauges of [Evaluate] (not in the reference): gauge_skill.csv and
        gauge_flow.csv, and the attributes gauge_skill / gauge_flow."""
        if self.gauges is not None and self.is_root:
            from .evaluate import GaugeSkill
            logging.info('---Start Gauge Skill:')
            t0 = time.time()
            res = GaugeSkill(self.s, self.gauges, self._routed_flow())
            self.gauge_skill, self.gauge_flow = res.skill, res.flow
            logging.info('---Gauge Skill has finished successfully: %s seconds ------' % (time.time() - t0))

    def _runoff(self):
        """Q for a post-processor: the DeviceArray in HBM after a device-resident simulation (on a sharded run the root's
        gathered array), without the download the host property would make."""
        if self.pipe is not None and 'Q' not in self._host:
            return self.pipe.out[_RESULTS['Q']]
        return self.Q

    def _diag_maps(self):
        """The loader's maps as the reference's diagnostics and plots see them.  In a GWAM run its loader sets the basin and
        country ids of every cell without maximum soil moisture, country or basin to -9999, in place
        (data_load.py:241-271); those cells then fall out of both post-processors.  The maps of this package's loader
        stay as read (the writer's aggregation uses them): the change is made on copies, for these two only."""
        d = self.data
        if self.s.runoff_module != 'gwam' or d.country_ids is None:
            return d
        invalid = (np.asarray(d.soil_moisture) == 0) | (d.country_ids == 0) | (d.basin_ids == 0)
        view = SimpleNamespace(**vars(d))
        view.country_ids, view.basin_ids = d.country_ids.copy(), d.basin_ids.copy()
        view.country_ids[invalid] = -9999
        view.basin_ids[invalid] = -9999
        return view

    def diagnostics(self):
        """Runoff diagnostics against the comparison data (components.py:431-439)."""
        if self.s.PerformDiagnostics and self.is_root:
            from .diagnostics.diagnostics import Diagnostics
            logging.info('---Start Diagnostics:')
            t0 = time.time()
            Diagnostics(self.s, self._runoff(), self._diag_maps())
            logging.info('---Diagnostics has finished successfully: %s seconds ------' % (time.time() - t0))

    def plots(self):
        """Time-series plots of the written q and ac (components.py:476-484), read from the writer without a download."""
        if self.s.CreateTimeSeriesPlot and self.is_root:
            from .diagnostics.time_series import TimeSeriesPlot
            logging.info('---Creating Time Series Plots:')
            t0 = time.time()
            w = self._writer
            q = w.get('q', host=False) if w is not None and 'q' in w.output_names else self._runoff()
            ac = w.get('avgchflow', host=False) if w is not None and 'avgchflow' in w.output_names else self._routed_flow()
            TimeSeriesPlot(self.s, q, ac, self._diag_maps())
            logging.info('---Plots has finished successfully: %s seconds ------' % (time.time() - t0))

    def output_simulation(self, keep_device=False, write_files=True):
        """Aggregate / convert on the device and write the selected variables (components.py:441-474).  ``keep_device`` /
        ``write_files = False`` (the ensemble driver): the arrays as written stay in HBM too / are formed without files."""
        from .data_writer.out_writer import OutWriter
        if not self.is_root:               # (a sharded run: rank 0 holds the gathered outputs and writes)
            return
        names = {'pet': 'PET', 'aet': 'AET', 'q': 'Q', 'soilmoisture': 'Sav', 'avgchflow': 'Avg_ChFlow'}
        # arrays still in HBM go to the writer as they are (it aggregates / converts / saves from there)
        all_outputs = {k: (self.pipe.out[_RESULTS[a]] if self.pipe is not None and a not in self._host
                           and (a != 'Avg_ChFlow' or self.pipe.plan is not None) else getattr(self, a))
                       for k, a in names.items() if k in self.s.output_vars or k in ('q', 'avgchflow')}
        writer = OutWriter(self.s, self.data.area, all_outputs, grid=self.grid)
        writer.keep_device, writer.write_files = keep_device, write_files
        writer.write()
        self._writer, self._q, self._ac = writer, None, None
        if not write_files:
            return
        q_written = writer.get('q', host=False) if 'q' in writer.output_names else all_outputs['q']
        # always from the written runoff, or from self.Q when 'q' is not among the output variables (:461-472)
        writer.write_aggregates(self.data, q_written, self.s.AggregateRunoffBasin, self.s.AggregateRunoffCountry,
                                self.s.AggregateRunoffGCAMRegion)
