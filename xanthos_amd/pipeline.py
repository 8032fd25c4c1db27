"""Device-resident PET -> runoff -> routing pipeline.

One object owns the static grid data and the six output arrays in HBM and enqueues the stages back to back on the
context's stream; nothing crosses PCIe between stages.  ``components.Components`` (the reference-shaped harness),
``bench.py`` and the multi-GPU sharding all drive this class; the per-stage plugin functions in ``pet/``, ``runoff/``
and ``routing/`` are the host-array entry points around the same C-ABI calls.
"""
import os
import threading

import numpy as np

from ._hip import NARROW_KINDS
from .data_load import stored_kind
from .pet import hargreaves as hg_mod, hargreaves_samani as hs_mod, penman_monteith as pm_mod, thornthwaite as trn_mod
from .routing import mrtm as mrtm_mod
from .runoff import gwam as gwam_mod
from .utils import set_month_arrays

FEED_DEFAULT = '1'      # measured on MI355X: 26.4 -> 25.35 ms per full-grid step (profiles/round4/feed_first_block.txt)
# forcing of each PET / runoff module, in upload order
MODULE_FORCING = {'pm': ('tas', 'tmin', 'rhs', 'wind', 'rsds', 'rlds'), 'hargreaves': ('temp', 'dtr'),
                  'hs': ('tas', 'tmax', 'tmin'), 'thornthwaite': ('tas',), 'abcd': ('precip', 'abcd_tmin'),
                  'gwam': ('precip',), 'none': ()}
# the names that lose their NaNs on the device right after the upload, as the loader's nan_to_num (data_load.py:120-125,
# :137-138, :194-195); Hargreaves' and Hargreaves-Samani's forcing goes up as it is (the kernels clean it or keep NaN as
# the reference does) and precipitation keeps NaN
NAN_TO_NUM = {'pm': MODULE_FORCING['pm'], 'thornthwaite': ('tas',), 'abcd': ('abcd_tmin',)}
FORCING = MODULE_FORCING['pm'] + MODULE_FORCING['abcd']
OUTPUTS = ('pet', 'aet', 'q', 'sav', 'chs', 'avg')


def file_range_of(arr, stored=False):
    """(path, byte offset) of the first element of a C-contiguous float64 np.memmap in its file, or None.  The position
    is taken from the addresses (the array's data pointer against the start of its mapping), not from ``arr.offset``,
    which a slice of a memory map inherits unchanged from its parent.  ``stored``: the maps that cross PCIe as they are
    stored count as well (float32, big-endian float32 and float64: _hip.NARROW_KINDS)."""
    import mmap
    if not isinstance(arr, np.memmap):
        return None
    wanted = arr.dtype == np.float64 and arr.dtype.isnative
    if not ((wanted or (stored and arr.dtype in NARROW_KINDS)) and arr.flags.c_contiguous
            and getattr(arr, 'filename', None) is not None and getattr(arr, '_mmap', None) is not None):
        return None
    base = np.frombuffer(arr._mmap, dtype=np.uint8)
    delta = arr.ctypes.data - base.ctypes.data
    if delta < 0 or delta + arr.nbytes > base.size:
        return None
    map_start = arr.offset - arr.offset % mmap.ALLOCATIONGRANULARITY        # where numpy placed the mapping in the file
    return str(arr.filename), map_start + delta


class DevicePipeline:
    """PET -> runoff (-> MRTM) for one set of cells (the whole grid, or one rank's shard) on one GPU.  PET: Penman-Monteith
    (``pm``), Hargreaves, Hargreaves-Samani (``hs``) or Thornthwaite; runoff: ABCD, GWAM or none (AET / Q / Sav stay zero,
    as the reference's arrays); routing when ``um`` is given.  Only the selected modules' arguments are needed."""

    def __init__(self, ctx, *, ncell, nmonths, start_year, pet_module='pm', runoff_module='abcd',
                 pm_tables=None, lct=None, elev=None, lc_years=(), water_idx=0, snow_idx=6,
                 lat_radians=None, lat_degrees=None, daylight='reference',
                 sm_max=None, sm0=None, gwam_spinup=0, precipitation='reference',
                 basin_ids=None, abcd_pars=None, abcd_spinup=0, use_snow=True,
                 um=None, flow_dist=None, velocity=None, area=None, routing_spinup=0, chs_prev=None, route_flags=0,
                 plan_async=False):
        if pet_module not in ('pm', 'hargreaves', 'hs', 'thornthwaite') or runoff_module not in ('abcd', 'gwam', 'none'):
            raise ValueError("unknown pet_module '{}' or runoff_module '{}'".format(pet_module, runoff_module))
        self.ctx = ctx
        self.ncell, self.nmonths, self.start_year = int(ncell), int(nmonths), int(start_year)
        self.end_year = self.start_year + self.nmonths // 12 - 1
        self.pet_module, self.runoff_module = pet_module, runoff_module
        self.abcd_spinup, self.gwam_spinup, self.routing_spinup = int(abcd_spinup), int(gwam_spinup), int(routing_spinup)
        self.use_snow, self.precipitation, self.route_flags = use_snow, precipitation, route_flags
        self.ndays = set_month_arrays(self.nmonths, self.start_year, self.end_year)[:, 2]      # routing's days per month
        self.forcing_names = MODULE_FORCING[pet_module] + MODULE_FORCING[runoff_module]
        self._nan_to_num = NAN_TO_NUM.get(pet_module, ()) + NAN_TO_NUM.get(runoff_module, ())
        self.forcing = {}
        # what set_forcing sent last, by forcing name: (kind, bytes host -> device), kind 'f64' for doubles sent as they are,
        # 'f32' / 'f32be' / 'f64be' for values sent as stored and widened in HBM (xh_widen)
        self.forcing_upload = {}
        self._stored_scratch = {}          # uploading context -> its scratch DeviceArray for single-precision bytes
        self.d_tairprev = None
        self._setup_pet(pm_tables, lct, elev, lc_years, water_idx, snow_idx, lat_radians, lat_degrees, daylight)
        if runoff_module == 'abcd':
            self._setup_abcd(basin_ids, abcd_pars)
        elif runoff_module == 'gwam':
            self.d_sm_max, self.d_sm0 = ctx.upload(sm_max), ctx.upload(sm0)
        self.out = {k: ctx.empty((self.ncell, self.nmonths)) for k in OUTPUTS}
        if runoff_module == 'none':
            for k in ('aet', 'q', 'sav'):
                self.out[k].zero()
        self.um = um
        self.d_flow_dist = self.d_velocity = self.d_area = self.d_S0 = None
        self._plan, self._plan_thread, self._plan_error = None, None, None
        if um is not None:
            self._setup_routing(flow_dist, velocity, area, chs_prev, plan_async)

    def _setup_pet(self, pm_tables, lct, elev, lc_years, water_idx, snow_idx, lat_radians, lat_degrees, daylight):
        up = self.ctx.upload
        if self.pet_module == 'pm':
            self.pm_tables, self.lc_years, self.water_idx, self.snow_idx = pm_tables, sorted(lc_years), water_idx, snow_idx
            self.nlcs = len(pm_tables['cL'])                    # land-cover classes the PM kernel reads
            self.d_lct = up(lct)
            self.d_elev = up(np.asarray(elev, dtype=np.float64).reshape(-1))
        elif self.pet_module == 'hs':                                 # latitude in degrees (hargreaves_samani.py:105)
            if lat_degrees is None:
                raise ValueError('Hargreaves-Samani PET needs lat_degrees')
            self.hs_ndays = hs_mod.days_per_month(self.start_year, self.end_year)
            self.d_lat = up(np.asarray(lat_degrees, dtype=np.float64).reshape(-1))
        else:
            if self.pet_module == 'hargreaves':
                self.solar_dec, self.dr, self.ndays_f = hg_mod.month_factors(self.start_year, self.end_year)
            else:
                trn_mod.daylight_mode(daylight)                      # (a bad name fails here, not at run time)
                self.daylight = daylight
            self.d_lat = up(np.asarray(lat_radians, dtype=np.float64).reshape(-1))

    def _setup_abcd(self, basin_ids, abcd_pars):
        basin_ids = np.asarray(basin_ids)
        uniq, inv = np.unique(basin_ids, return_inverse=True)
        self.basin_index = inv.astype(np.int32)
        self.n_groups = len(uniq)
        self.par_index = (basin_ids - 1).astype(np.int32)          # row of abcd_pars = basin id - 1 (abcd.py:332)
        self.npar_rows = int(np.asarray(abcd_pars).shape[0])
        self.d_pars = self.ctx.upload(np.asarray(abcd_pars, dtype=np.float64))

    def _setup_routing(self, flow_dist, velocity, area, chs_prev, plan_async):
        up, um, ctx = self.ctx.upload, self.um, self.ctx
        self.d_flow_dist, self.d_velocity, self.d_area = up(flow_dist), up(velocity), up(area)
        # initial channel storage (future mode, data_load.py:427-438); None = zeros
        self.d_S0 = up(chs_prev) if chs_prev is not None and np.any(np.asarray(chs_prev) != 0) else None
        # The routing plan (partition of the networks, 50-70 ms of host time at the full grid) touches neither the
        # context's stream nor the arrays above; it is made on a host thread, and `plan` waits for it: with plan_async
        # while the caller uploads the forcing (run_model()), otherwise at once.

        def make():
            try:
                self._plan = um.plan(ctx)
                self._plan.prepare(flow_dist, velocity, 10800.0)      # the prepared plan (folded leaves, single sums) ahead of the first call
            except BaseException as exc:      # re-raised by `plan`
                self._plan_error = exc
        self._plan_thread = threading.Thread(target=make, name='xh-route-plan')
        self._plan_thread.start()
        if not plan_async:
            self.plan

    @property
    def plan(self):
        """The device routing plan (None without routing)."""
        if self._plan_thread is not None:
            self._plan_thread.join()
            self._plan_thread = None
            if self._plan_error is not None:
                raise self._plan_error
        return self._plan

    # ---- forcing
    def alloc_forcing(self):
        for k in self.forcing_names:
            if k not in self.forcing:
                self.forcing[k] = self.ctx.empty((self.ncell, self.nmonths))
        return self.forcing

    def set_forcing(self, host, tairprev=None, ctx=None, into=None):
        """host: dict of [ncell, nmonths] arrays keyed by the modules' forcing names (MODULE_FORCING; a missing or None
        entry is left as it is, e.g. abcd_tmin when use_snow is False).  A read-only memory map of a .npy
        (np.load(mmap_mode='r'), what DataLoader keeps) is copied straight out of the mapping (no host copy: the runtime
        pins the page-cache pages); tairprev=None leaves PM's previous-cell temperature to the PM kernel (it reads the row
        above of ``tas``, data_load.py:127-128).
        ``ctx`` / ``into``: another context of the same device and another set of forcing arrays (allocated by that
        context): the ensemble driver uploads the next member on a second stream while this pipeline runs.
        A C-contiguous float32, big-endian float32 or big-endian float64 array of the right shape (what DataLoader keeps of
        a single-precision .npy or a NetCDF variable) crosses PCIe as it is stored and becomes doubles in HBM (xh_widen):
        exactly ``src.astype(np.float64)``.  ``forcing_upload`` records what was sent."""
        own = ctx is None and into is None
        ctx = self.ctx if ctx is None else ctx
        forcing = self.forcing if into is None else into
        from_file = os.environ.get('XH_UPLOAD_FROM_FILE', '0') == '1'
        for k in self.forcing_names:
            src = host.get(k)
            if src is None:
                continue
            stored = stored_kind(src)
            if stored is not None and src.shape == (self.ncell, self.nmonths):
                if k not in forcing:
                    forcing[k] = ctx.empty((self.ncell, self.nmonths))
                self._upload_stored(ctx, src, stored, forcing[k], file_range_of(src, stored=True) if from_file else None)
                self.forcing_upload[k] = (stored[1], src.nbytes)
                if k in self._nan_to_num:
                    ctx.nan_to_num(forcing[k])
                continue
            # XH_UPLOAD_FROM_FILE=1: through xh_upload_file (maps the file range itself: 34 GB/s with its own map /
            # unmap per array); default: xh_memcpy_h2d out of numpy's mapping, which stays alive in the loader (51 GB/s)
            where = file_range_of(src) if from_file else None
            arr = src if where is not None else np.asarray(src, dtype=np.float64)
            if arr.shape != (self.ncell, self.nmonths):
                raise ValueError('forcing {} has shape {}, expected {}'.format(k, arr.shape, (self.ncell, self.nmonths)))
            if k not in forcing:
                forcing[k] = ctx.empty((self.ncell, self.nmonths))
            if where is not None:
                ctx.upload_file(forcing[k], where[0], where[1], src.nbytes)
            else:
                forcing[k].upload(arr)
            self.forcing_upload[k] = ('f64', forcing[k].nbytes)
            if k in self._nan_to_num:
                ctx.nan_to_num(forcing[k])
        if tairprev is not None:
            if not own:
                raise ValueError('tairprev belongs to the pipeline: set it without ctx / into')
            self.d_tairprev = self.ctx.nan_to_num(self.ctx.upload(tairprev))

    def _upload_stored(self, ctx, src, stored, dst, where):
        """``src`` (float32 / big-endian float32 / big-endian float64, as stored) -> the doubles of ``dst``: its bytes through
        the movers (``where``: its file range, through xh_upload_file; otherwise out of the array or its mapping), then
        xh_widen.  Single precision lands in the context's scratch first -- one per uploading context, kept until close():
        the movers are enqueued on the context's stream and wait for it, so the next array's bytes arrive behind this
        array's widen; big-endian float64 lands in ``dst`` and is swapped in place."""
        kind, _ = stored
        if src.dtype.itemsize == 8:
            raw = dst
        else:
            raw = self._stored_scratch.get(ctx)
            if raw is None or raw.ptr is None or raw.nbytes != src.nbytes:
                if raw is not None:
                    raw.free()
                raw = self._stored_scratch[ctx] = ctx.empty((src.nbytes,), dtype=np.uint8)
        if where is not None:
            ctx.upload_file(raw, where[0], where[1], src.nbytes)
        else:
            raw.upload(src.view(raw.dtype))                   # the bytes as they are stored, whatever they mean
        ctx.widen(raw, kind, src.size, dst)

    def close(self):
        """Release the scratch of the stored-forcing uploads (the arrays of the pipeline go with their contexts)."""
        for a in self._stored_scratch.values():
            a.free()
        self._stored_scratch = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- stages (asynchronous; call ctx.sync() or download to wait)
    def run_pet(self):
        f, pet = self.forcing, self.out['pet']
        if self.pet_module == 'pm':
            pm_mod.run_pmpet_device(self.ctx, self.pm_tables, self.ncell, self.start_year, self.end_year, self.water_idx,
                                    self.snow_idx, self.lc_years, f['tas'], f['tmin'], f['rhs'], f['wind'], f['rsds'],
                                    f['rlds'], self.d_tairprev, self.d_lct, self.d_elev, pet)
        elif self.pet_module == 'hargreaves':
            hg_mod.hargreaves_device(self.ctx, self.ncell, self.nmonths, f['temp'], f['dtr'], self.d_lat, self.solar_dec,
                                     self.dr, self.ndays_f, pet)
        elif self.pet_module == 'hs':
            hs_mod.hs_device(self.ctx, self.ncell, self.nmonths, f['tas'], f['tmax'], f['tmin'], self.d_lat, self.hs_ndays,
                             pet)
        else:
            trn_mod.thornthwaite_device(self.ctx, self.ncell, self.nmonths, self.start_year, f['tas'], self.d_lat,
                                        daylight=self.daylight, d_pet=pet)

    def run_runoff(self):
        f, o = self.forcing, self.out
        if self.runoff_module == 'abcd':
            self.ctx.abcd(self.ncell, self.nmonths, self.abcd_spinup, self.n_groups, self.basin_index, self.par_index,
                          self.npar_rows, self.d_pars, o['pet'], f['precip'], f['abcd_tmin'] if self.use_snow else None,
                          o['aet'], o['q'], o['sav'])
        elif self.runoff_module == 'gwam':
            gwam_mod.gwam_device(self.ctx, self.ncell, self.nmonths, self.gwam_spinup, o['pet'], f['precip'], self.d_sm_max,
                                 self.d_sm0, precipitation=self.precipitation, out={k: o[k] for k in ('aet', 'q', 'sav')})

    def run_mrtm(self, runoff=None):
        self.ctx.route_series(self.plan, self.nmonths, self.routing_spinup, self.ndays, 10800.0, self.d_flow_dist,
                              self.d_velocity, self.d_area, self.out['q'] if runoff is None else runoff, self.d_S0,
                              self.out['chs'], self.out['avg'], flags=self.route_flags)

    def run_fused(self, with_routing=True, block_months=0, mode=0):
        """PM -> ABCD (-> MRTM) as one pipelined call (xh_run_fused): the stages overlap on the device.  mode 1 ("fed"):
        the routing kernel starts once the first max(spin-ups) months of runoff exist and the rest of PM and ABCD runs beside it."""
        f = self.forcing
        route = with_routing and self.plan is not None
        self.ctx.run_fused(tables=self.pm_tables, ncell=self.ncell, nmonths=self.nmonths, start_year=self.start_year,
                           lc_years=self.lc_years, water_idx=self.water_idx, snow_idx=self.snow_idx, tas=f['tas'],
                           tmin=f['tmin'], rhs=f['rhs'], wind=f['wind'], rsds=f['rsds'], rlds=f['rlds'],
                           tairprev=self.d_tairprev, lct=self.d_lct, elev=self.d_elev, abcd_spinup=self.abcd_spinup,
                           n_groups=self.n_groups, basin_index=self.basin_index, par_index=self.par_index,
                           npar_rows=self.npar_rows, pars=self.d_pars, precip=f['precip'],
                           abcd_tmin=f['abcd_tmin'] if self.use_snow else None, pet=self.out['pet'], aet=self.out['aet'],
                           q=self.out['q'], sav=self.out['sav'], plan=self.plan if route else None,
                           routing_spinup=self.routing_spinup, ndays=self.ndays, dt=10800.0,
                           flow_dist=self.d_flow_dist, velocity=self.d_velocity, area=self.d_area, S0=self.d_S0,
                           chs=self.out['chs'] if route else None, avg=self.out['avg'] if route else None,
                           route_flags=self.route_flags, block_months=block_months, mode=mode)

    def run(self, stages=None, fused=None, fed=None, after_runoff=None):
        """Enqueue ``stages`` (default: the configured ones) on the context's stream, one after the other.  PM + ABCD has
        two more orders.  With all three stages the default is the FED order (xh_run_fused mode 1): the first
        max(spin-ups) months of PM and ABCD, then the routing kernel, and the remaining months of PM and ABCD beside it on
        a second stream -- identical results, the 2.8 ms of PM + ABCD mostly hidden under the routing.  ``fed=False`` (or
        XH_FEED=0) runs the stages strictly one after the other; ``fused=True`` (or XH_FUSED=1) is round 2's block pipeline
        of PM and ABCD with the routing behind it (slower on MI355X at the full grid).
        ``after_runoff``: called once PET / AET / Q / Sav have been enqueued and before anything waits for the routing --
        the place for a side gather of the four arrays (dist.OutputGather.run_side)."""
        if stages is None:
            stages = (self.pet_module, self.runoff_module) + (('mrtm',) if self.um is not None else ())
        if self.pet_module == 'pm' and self.runoff_module == 'abcd' and 'pm' in stages and 'abcd' in stages:
            if fused is None:
                fused = os.environ.get('XH_FUSED') == '1'
            if fed is None:
                fed = os.environ.get('XH_FEED', FEED_DEFAULT) == '1'
            if fused or (fed and 'mrtm' in stages and self.plan is not None):
                block = int(os.environ.get('XH_FUSED_BLOCK', '0')) if fused else 0
                self.run_fused(with_routing='mrtm' in stages, block_months=block, mode=0 if fused else 1)
                if after_runoff:      # the routing kernel is in the queue; a side gather waits for the runoff's side stream only
                    after_runoff()
                return
        if self.pet_module in stages:
            self.run_pet()
        if self.runoff_module in stages:
            self.run_runoff()
        if after_runoff:
            after_runoff()
        if 'mrtm' in stages:
            self.run_mrtm()

    def stage_traffic(self):
        """[(timer name, algorithmic bytes)] of the configured stages: what each kernel must move through HBM at the least
        (PM 6 reads + 1 write + land cover, ABCD 3 + 3, MRTM 1 + 2)."""
        n, cm = self.ncell, self.ncell * self.nmonths
        if self.pet_module == 'pm':
            stages = [('pm_pet', cm * 56 + n * (self.nmonths // 12) * self.nlcs * 8)]
        elif self.pet_module == 'hargreaves':
            stages = [('hargreaves_pet', cm * 24)]
        elif self.pet_module == 'hs':
            stages = [('hs_pet', cm * 32)]
        else:
            stages = [('trn_daylight', n * 24 * 8), ('trn_pet', cm * 16)]
        if self.runoff_module == 'abcd':
            stages += [('abcd_spinup', n * self.abcd_spinup * 24), ('abcd_sim', cm * 48)]
        elif self.runoff_module == 'gwam':
            stages += [('gwam_spinup', n * self.gwam_spinup * 16),
                       ('gwam_sim', cm * (40 if self.precipitation == 'monthly' else 32))]
        if self.um is not None:
            stages.append(('mrtm_route', cm * 24 + n * self.routing_spinup * 8))
        return stages

    def download(self, names=OUTPUTS):
        return {k: self.out[k].download() for k in names}

    def download_pinned(self, names=OUTPUTS):
        """All outputs into page-locked host arrays with asynchronous copies and ONE synchronisation (run_model()'s
        result arrays: numpy views of memory the context keeps until it is closed).  XH_PAGEABLE_OUTPUTS=1 falls back to
        plain numpy arrays filled by synchronous copies."""
        if os.environ.get('XH_PAGEABLE_OUTPUTS') == '1':
            return self.download(names)
        host = {k: self.ctx.pinned((self.ncell, self.nmonths)) for k in names}
        self.ctx.sync()                      # settles a routing fault (re-route) before anything is copied
        for k in names:
            self.ctx.d2h_async(host[k], self.out[k])
        self.ctx.sync()
        return host

    def rows(self, darr, cells):
        """Download selected rows of a [ncell, nmonths] device array."""
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        d_idx = self.ctx.upload(cells, dtype=np.int64)
        d_tmp = self.ctx.empty((len(cells), self.nmonths))
        self.ctx.gather_rows(darr, d_idx, len(cells), self.nmonths, d_tmp)
        host = d_tmp.download()
        d_idx.free()
        d_tmp.free()
        return host


def topology_from_world(world):
    """dsid -> upid -> UM for a synth world / DataLoader-like object (coords, flow_dir, nrow, ncol)."""
    from types import SimpleNamespace
    st = SimpleNamespace(ngridrow=world.nrow, ngridcol=world.ncol)
    ds = mrtm_mod.downstream(world.coords, world.flow_dir, st)
    return mrtm_mod.upstream_genmatrix(mrtm_mod.upstream(world.coords, ds, st))


def pipeline_from_world(ctx, world, nmonths, start_year, abcd_spinup, routing_spinup, um=None, **kw):
    tables = pm_mod.tables_from(world, world.nlcs)
    if um is None:
        um = topology_from_world(world)
    return DevicePipeline(ctx, ncell=world.ncell, nmonths=nmonths, start_year=start_year, basin_ids=world.basin_ids,
                          abcd_pars=world.abcd_pars, pm_tables=tables, lct=world.lct, elev=world.elev,
                          lc_years=world.lc_years, um=um, flow_dist=world.flow_dist, velocity=world.velocity,
                          area=world.area, abcd_spinup=abcd_spinup, routing_spinup=routing_spinup, **kw)
