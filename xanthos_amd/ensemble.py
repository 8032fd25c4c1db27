"""An ensemble of forcing scenarios and ABCD parameter sets through one grid in one device-resident pass.

The reference's way to run S forcing sets is a Python loop of ``Xanthos.execute(args)``: every run reads the static inputs
again, and the across-run statistics are formed afterwards on the host.  ``run_ensemble`` keeps one ``Components``, one
``DevicePipeline``, one topology and one routing plan; the members stream through two buffer sets -- member k + 1's forcing
is read and uploaded on a second context while member k's kernels run on the main one and member k - 1's post-processors
and write-out proceed on a third -- and the mean / spread / quantiles over the members are formed in HBM by
``xh_ens_stats`` on the arrays as written (after OutputInYear and OutputUnit).

Member ``name`` is written to ``<OutputFolder>/<name>/`` with exactly the files
``Xanthos(ini).execute({**overrides, 'OutputFolder': ...})`` writes (the log stays in ``<OutputFolder>``); the statistics
go to ``<OutputFolder>/ensemble/<var>_<unit>_<ProjectName>_<stat>.<ext>`` through ``OutWriter.write_data``
(with ``GriddedOutput = 1`` the members' maps and ``..._<stat>_grid.nc`` next to them, from the run's one ``GridMap``).

Only the settings that name the forcing arrays of the configured PET / runoff modules may vary per member
(``ConfigReader.forcing_settings``), and with ABCD the parameter table: ``abcd_pars``, an ndarray or .npy of the shape of the
run's calib_file array -- the member then equals the single run with ``calib_file`` set to it.  When no member overrides a
forcing setting the ensemble is *resident*: the forcing is uploaded once, PET is computed once, and a member is one ABCD and
one routing pass.  With ``observed`` every member's Q is scored in HBM against observed basin runoff (``xh_basin_kge``, the
reference's KGE): ``EnsembleResult.kge`` and ``<OutputFolder>/ensemble/member_kge.csv``.  With stream gauges ([Evaluate],
or ``gauges`` / ``gauge_observed``) every member's Avg_ChFlow is scored at the gauge cells in HBM (``xh_gauge_skill``,
DESIGN.md 4.17): ``EnsembleResult.gauge_kge`` / ``gauge_skill`` / ``gauge_flow``, ``ensemble/member_gauge_kge.csv`` and
``member_gauge_skill.csv``, and with ``statistics`` the across-member statistics of the gauge hydrographs.
There is no host fallback: without a device the call raises ``HipUnavailable``.
"""
import copy
import csv
import logging
import os
import threading
import time
from types import SimpleNamespace

import numpy as np

from . import _hip, launch, nc_header
from .components import _FORCING_DATA, _FORCING_SETTINGS, Components, runs_device_resident
from .configurations import ConfigRunner
from .data_load import load_file
from .evaluate import gauge_skill as gskill
from .ini_reader import ValidationException, parse_statistic
from .pipeline import OUTPUTS, DevicePipeline

MAX_MEMBERS_WITH_STATISTICS = 64        # xh_ens_stats' compiled limit
STATISTICS_DIR = 'ensemble'
PARS_KEY = 'abcd_pars'                  # a member's own [rows, 5] table of a, b, c, d, m (the shape of the run's calib_file array)
KGE_TABLE = 'member_kge.csv'
GAUGE_KGE_TABLE, GAUGE_SKILL_TABLE = 'member_gauge_kge.csv', 'member_gauge_skill.csv'
GAUGE_STAT_FILE = 'gauge_flow_{}.csv'
OBS_UNITS = ('km3_per_mth', 'mm_per_mth')
# output variable -> result attribute (Components.output_simulation)
_WRITTEN = ('pet', 'aet', 'q', 'soilmoisture', 'avgchflow')


def refuse(member, key, why):
    """The ValidationException of an ensemble refusal: names the member (None: the ensemble itself) and the key."""
    who = 'the ensemble' if member is None else "member '{}'".format(member)
    return ValidationException('[Ensemble] {}, {}: {}'.format(who, key, why))


class EnsemblePlan(SimpleNamespace):
    """What validate() made of a request: names, overrides (one dict per member), statistics [(label, q or None)],
    statistics_vars, member_outputs, ncols (columns of an array as written), bytes_needed, resident (no member overrides a
    forcing setting: one upload, one PET), skill (None, or load_observed()'s basins / observations / cell lists), gauge_skill
    (None, or evaluate.load_gauge_set()'s ids / cells / basins / records)."""


def read_members(config, path):
    """The members table of [Ensemble]: a header row with ``name`` and setting names, one row per member; every cell is
    resolved as the same key's value in the ini would be, an empty cell keeps the ini's value."""
    if not os.path.isfile(path):
        raise refuse(None, 'members', 'the members table {} does not exist'.format(path))
    with open(path, newline='') as fh:
        rows = [[c.strip() for c in r] for r in csv.reader(fh) if any(c.strip() for c in r)]
    if not rows or 'name' not in rows[0]:
        raise refuse(None, 'members', "{} needs a header row with a 'name' column".format(path))
    header, known = rows[0], config.forcing_settings()
    pars_dir = getattr(config, 'ro_model_dir', None)      # abcd_pars resolves as calib_file does: against the runoff model directory

    def resolve(k, v):
        if k in known:
            return config.resolve_forcing_setting(k, v)
        if k == PARS_KEY and pars_dir is not None:
            return os.path.join(pars_dir, v)
        return v                                          # (kept as written: validate() refuses it with the member's name)
    members = []
    for r in rows[1:]:
        cells = dict(zip(header, r + [''] * (len(header) - len(r))))
        name = cells.pop('name')
        members.append((name, {k: resolve(k, v) for k, v in cells.items() if v != ''}))
    return members


def _normalise(members):
    out = []
    for m in members:
        if isinstance(m, dict):
            if 'name' not in m:
                raise refuse(None, 'name', "a member given as a dict needs a 'name' key")
            out.append((m['name'], {k: v for k, v in m.items() if k != 'name'}))
        else:
            name, overrides = m
            out.append((name, dict(overrides or {})))
    return out


def _header_of(value, key=None):
    """(shape, dtype as stored) of a forcing override without reading it: an ndarray, the header of a .npy, or the header of
    a NetCDF-classic file whose variable ``key`` is one block of values (nc_header); (None, None) when only the loader can
    tell (MATLAB, text, any other NetCDF)."""
    if isinstance(value, np.ndarray):
        return value.shape, value.dtype
    if isinstance(value, str) and value.endswith('.npy'):
        mm = np.load(value, mmap_mode='r')
        return mm.shape, mm.dtype
    if isinstance(value, str) and value.endswith('.nc'):
        where = nc_header.variable_range(value, key)
        if where is not None:
            return where[1], where[0]
    return None, None


def _through_scratch(dtype):
    """Whether an array stored as ``dtype`` passes through the uploading context's scratch (single precision, sent as stored)."""
    return dtype is not None and dtype in _hip.NARROW_KINDS and dtype.itemsize == 4


def written_vars(config):
    return [v for v in config.output_vars if v in _WRITTEN and (v != 'avgchflow' or config.routing_module == 'mrtm')]


def _table_header(value):
    """(shape, dtype) of a parameter table: an ndarray, or a .npy by its header."""
    if isinstance(value, np.ndarray):
        return value.shape, value.dtype
    mm = np.load(value, mmap_mode='r')
    return mm.shape, mm.dtype


def _check_pars(s, runs_runoff, name, value):
    """The refusals of one member's ``abcd_pars``.  The values are not range-checked: the contract is the single run with
    that table as calib_file."""
    if s.runoff_module != 'abcd' or not runs_runoff:
        raise refuse(name, PARS_KEY, 'the table of a, b, c, d, m belongs to runoff_module = abcd; the configuration {} runs '
                     '{}'.format(s.mod_cfg, 'runoff_module = ' + s.runoff_module if runs_runoff else 'without runoff'))
    if not isinstance(value, (str, np.ndarray)):
        raise refuse(name, PARS_KEY, 'a path or an ndarray is expected, not {}'.format(type(value).__name__))
    if isinstance(value, str) and not os.path.isfile(value):
        raise refuse(name, PARS_KEY, 'file {} does not exist'.format(value))
    try:
        shape, dtype = _table_header(value)
    except Exception as exc:
        raise refuse(name, PARS_KEY, '{} is not a .npy array ({})'.format(value, exc))
    try:
        expected = tuple(_table_header(s.calib_file)[0])
    except Exception:                  # (the run's own table cannot be read: the run itself says so)
        expected = None
    if expected is not None and tuple(shape) != expected:
        raise refuse(name, PARS_KEY, "the table has shape {}, expected the shape of the run's calib_file, {}".format(
            tuple(shape), expected))
    if not np.can_cast(dtype, np.float64, 'same_kind'):
        raise refuse(name, PARS_KEY, 'values of type {} do not cast to float64'.format(dtype))


def load_observed(s, observed, obs_unit, runs_runoff=True):
    """[Ensemble] observed / obs_unit -> what the skill of a member is formed against: the basins with a record
    (ascending), their first nmonths observations [basins, nmonths] and their cells as xh_basin_kge takes them (``start``
    into ``cells``, ascending per basin).  ``observed``: a file in the format of [Calibrate] observed -- rows [basin id, *,
    *, value], months in order -- or such an ndarray [rows, 4]."""
    if obs_unit not in OBS_UNITS:
        raise refuse(None, 'obs_unit', "{} is not one of {}".format(
            'it is required with observed' if obs_unit is None else "'{}'".format(obs_unit), ' / '.join(OBS_UNITS)))
    if not runs_runoff or s.runoff_module not in ('abcd', 'gwam'):
        raise refuse(None, 'observed', 'the skill is formed on the runoff Q, which the configuration {} does not compute'
                     .format(s.mod_cfg))
    if isinstance(observed, str):
        if not os.path.isfile(observed):
            raise refuse(None, 'observed', 'file {} does not exist'.format(observed))
        table = np.asarray(load_file(observed, 0))
    else:
        table = np.asarray(observed)
    if table.ndim != 2 or table.shape[1] < 4:
        raise refuse(None, 'observed', 'rows of [basin id, *, *, value] are expected, not an array of shape {}'.format(table.shape))
    table = np.asarray(table[:, [0, 3]], dtype=np.float64)         # (data_load.py:243)
    if not np.isfinite(table[:, 0]).all():
        raise refuse(None, 'observed', 'a basin id is NaN or infinite')
    basin_of = np.asarray(load_file(s.BasinIDs, 1)).reshape(-1).astype(int)
    basins = sorted({int(b) for b in table[:, 0]})
    obs, start, cells = np.empty((len(basins), s.nmonths)), [0], []
    for j, b in enumerate(basins):
        mine = np.flatnonzero(basin_of == b)
        if mine.size == 0:
            raise refuse(None, 'observed', 'basin {} has a record but no cells on the grid'.format(b))
        record = table[table[:, 0] == b, 1]
        if record.size < s.nmonths:
            raise refuse(None, 'observed', 'basin {} has {} months of observations, the run has nmonths = {}'.format(
                b, record.size, s.nmonths))
        obs[j] = record[:s.nmonths]
        cells.append(mine)
        start.append(start[-1] + mine.size)
    return SimpleNamespace(basins=basins, obs=obs, unit=obs_unit, start=np.asarray(start, dtype=np.int64),
                           cells=np.concatenate(cells).astype(np.int32))


def validate(config, members, statistics=(), statistics_vars=None, member_outputs=1, gpus=None, observed=None, obs_unit=None,
             gauges=None, gauge_observed=None, gauge_missing=None):
    """Every refusal of an ensemble request, before any GPU work; returns the EnsemblePlan."""
    s = config
    if getattr(s, 'calibrate', 0):
        raise refuse(None, 'Calibrate', '[Ensemble] and Calibrate = 1 ([Calibrate]) exclude each other')
    if getattr(s, 'CalculateTrend', 0):
        raise refuse(None, 'CalculateTrend', 'the trend tables of [Trend] belong to one run; per-member trends are not '
                     'implemented: run the ensemble with CalculateTrend = 0')
    if getattr(s, 'CalculateExtremes', 0):
        raise refuse(None, 'CalculateExtremes', 'the extremes of [Extremes] belong to one run; per-member extremes are not '
                     'implemented: run the ensemble with CalculateExtremes = 0')
    if getattr(s, 'CalculateSignatures', 0):
        raise refuse(None, 'CalculateSignatures', 'the signatures of [Signatures] belong to one run; per-member signatures are '
                     'not implemented: run the ensemble with CalculateSignatures = 0')
    if getattr(s, 'CalculateWaterBalance', 0):
        raise refuse(None, 'CalculateWaterBalance', 'the water balance of [WaterBalance] belongs to one run; per-member water '
                     'balances are not implemented: run the ensemble with CalculateWaterBalance = 0')
    env_gpus = int(os.environ.get('XH_GPUS') or 1)
    if (gpus and int(gpus) > 1) or env_gpus > 1 or launch.env_world()[2] > 1:
        raise refuse(None, 'gpus', 'members dealt over several GPUs are not implemented; run the ensemble on one GPU')
    runner = ConfigRunner(s)
    if not runs_device_resident(s, runner.run_pet, runner.run_runoff):
        raise refuse(None, 'pet_module / runoff_module', "the configuration {} runs stage by stage on host arrays, not device "
                     'resident (device resident: hargreaves / hs / thornthwaite PET, or pm with abcd)'.format(s.mod_cfg))
    members = _normalise(members)
    if not members:
        raise refuse(None, 'members', 'no members')
    allowed = s.forcing_settings()
    # setting that names a forcing file -> setting that names its NetCDF variable (None: the file format has no names)
    varkeys = {setting: varkey for m in (s.pet_module, s.runoff_module) for setting, varkey, _ in _FORCING_SETTINGS[m].values()}
    single = False                     # some member sends single-precision values: they pass through a scratch array in HBM
    for setting, varkey in varkeys.items():      # (the run's own arrays, which the members share where they override nothing)
        value = getattr(s, setting, None)
        if isinstance(value, np.ndarray) or (isinstance(value, str) and os.path.isfile(value)):
            single |= _through_scratch(_header_of(value, getattr(s, varkey, None) if varkey else None)[1])
    seen = set()
    for name, overrides in members:
        if not isinstance(name, str) or not name.strip():
            raise refuse(name, 'name', 'a member needs a non-empty name')
        if name != name.strip() or name in ('.', '..', STATISTICS_DIR) or os.path.basename(name) != name or \
                any(ch in name for ch in '/\\\0') or (os.altsep and os.altsep in name):
            raise refuse(name, 'name', "not a plain directory name ('{}' is kept for the statistics)".format(STATISTICS_DIR))
        if name in seen:
            raise refuse(name, 'name', 'duplicate member name')
        seen.add(name)
        for key, value in overrides.items():
            if key == PARS_KEY:
                _check_pars(s, runner.run_runoff, name, value)
                continue
            if key not in allowed:
                hint = " (a member's own ABCD parameter table goes in as {})".format(PARS_KEY) if key == 'calib_file' else ''
                raise refuse(name, key, 'may not vary per member: only the forcing arrays of pet_module = {} / runoff_module = {} '
                             'may ({}){}'.format(s.pet_module, s.runoff_module, ', '.join(sorted(allowed)), hint))
            if getattr(s, key, None) is None:
                raise refuse(name, key, 'the configuration runs without it (no {} in the ini): a member cannot switch it on'.format(key))
            if not isinstance(value, (str, np.ndarray)):
                raise refuse(name, key, 'a path or an ndarray is expected, not {}'.format(type(value).__name__))
            if isinstance(value, str) and not os.path.isfile(value):
                raise refuse(name, key, 'file {} does not exist'.format(value))
            varkey = varkeys.get(key)
            shape, stored = _header_of(value, getattr(s, varkey, None) if varkey else None)
            if shape is not None and tuple(shape) != (s.ncell, s.nmonths):
                raise refuse(name, key, 'the forcing array has shape {}, expected [ncell, nmonths] = {}'.format(
                    tuple(shape), (s.ncell, s.nmonths)))
            single |= _through_scratch(stored)
    stats, labels = [], set()
    for text in (statistics or ()):
        try:
            label, q = parse_statistic(text)
        except ValidationException as exc:
            raise refuse(None, 'statistics', str(exc))
        if label not in labels:
            labels.add(label)
            stats.append((label, q))
    outputs = written_vars(s)
    if statistics_vars is None:
        statistics_vars = list(outputs)
    statistics_vars = list(statistics_vars) if stats else []
    # index<k>: the standardized drought index of [DroughtIndex] at one of its scales (monthly, like the variable it indexes)
    index_names = ['index{}'.format(k) for k in s.drought_index['scales']] if getattr(s, 'CalculateDroughtIndex', 0) else []
    for v in statistics_vars:
        if v not in outputs and v not in index_names:
            raise refuse(None, 'statistics_vars', "'{}' is not among the variables the run writes ({})".format(
                v, ', '.join(list(outputs) + index_names)))
    member_outputs = int(member_outputs)
    if member_outputs not in (0, 1):
        raise refuse(None, 'member_outputs', 'must be 0 or 1')
    skill = None if observed is None else load_observed(s, observed, obs_unit, runner.run_runoff)
    # stream gauges: the arguments, or the ini's [Evaluate]; loaded and checked once for all members
    gauge_skill = None
    if gauges is not None or gauge_observed is not None or getattr(s, 'evaluate', None):
        gauge_skill = gskill.load_gauge_set(s, gauges, gauge_observed, gauge_missing)
    if not member_outputs and not (stats and statistics_vars) and skill is None and gauge_skill is None:
        # (with observed or gauges: the tables of the members' skill)
        raise refuse(None, 'member_outputs', 'member_outputs = 0 without statistics writes nothing')
    if stats and len(members) > MAX_MEMBERS_WITH_STATISTICS:
        raise refuse(None, 'statistics', '{} members exceed the {} the statistics kernel takes'.format(
            len(members), MAX_MEMBERS_WITH_STATISTICS))
    ncols = s.nmonths // 12 if s.OutputInYear else s.nmonths
    nforcing = sum(len(_FORCING_DATA[m]) for m in (s.pet_module, s.runoff_module))
    # resident: no member overrides a forcing setting -- the run's forcing goes up once and PET is computed once
    resident = not any(key in allowed for _, overrides in members for key in overrides)
    # the member stack of every statistics variable, one variable's statistics, and the two buffer sets (resident: one
    # forcing set, and the two output sets share the one PET array)
    arrays = nforcing + 2 * len(OUTPUTS) - 1 if resident else 2 * (nforcing + len(OUTPUTS))
    need = 8 * s.ncell * (ncols * (len(members) * len(statistics_vars) + len(stats)) + s.nmonths * arrays)
    if single:                         # the uploading context's scratch of one array as stored (pipeline._upload_stored)
        need += 4 * s.ncell * s.nmonths
    if gauge_skill is not None:        # cells, records, the members' hydrographs and metrics, the hydrographs' statistics
        ng = gauge_skill.ids.size
        need += 4 * ng + 8 * ng * (s.nmonths + len(members) * (s.nmonths + gskill.NCOLS) + len(stats) * s.nmonths)
    return EnsemblePlan(names=[n for n, _ in members], overrides=[o for _, o in members], statistics=stats,
                        statistics_vars=statistics_vars, member_outputs=member_outputs, ncols=ncols, bytes_needed=need,
                        resident=resident, skill=skill, gauge_skill=gauge_skill)


def index_scale(var):
    """The scale k of a statistics variable 'index<k>' (a standardized drought index), or None."""
    t = str(var)
    return int(t[5:]) if t.startswith('index') and t[5:].isdigit() else None


def check_fits(plan, free_bytes):
    """The member stack (and the gauge hydrographs of all members) against the free HBM."""
    gauges = getattr(plan, 'gauge_skill', None) is not None
    if (plan.statistics or gauges) and plan.bytes_needed > free_bytes:
        key = 'statistics' if plan.statistics else 'gauges'
        raise refuse(None, key, 'the stack of {} members x {} variables and the buffer sets need {} bytes of HBM, {} '
                     'bytes are free'.format(len(plan.names), len(plan.statistics_vars), plan.bytes_needed, free_bytes))


class _Aborted(Exception):
    pass


def run_schedule(n, upload, compute, write, overlap=True, nsets=2, write_reads_forcing=False):
    """Members 0 .. n - 1 through ``upload(k, i)``, ``compute(k, i)``, ``write(k, i)`` (i: buffer set).  ``overlap``:
    uploads on one host thread, write-outs on another, computes on the caller's, over ``nsets`` buffer sets -- member k's
    compute starts only when its upload has completed, its write-out when its compute has; a set's forcing is
    uploaded anew only when the compute that read it has ended, its outputs are computed anew only when their write-out
    has.  ``write_reads_forcing``: the write-out reads its set's forcing too (SPI / SPEI index the precipitation), so that
    forcing is uploaded anew only when the write-out has ended as well.  Otherwise strictly one after the other on set 0.
    The first exception of any stage ends the run and is raised."""
    if not overlap:
        for k in range(n):
            upload(k, 0)
            compute(k, 0)
            write(k, 0)
        return
    uploaded, computed, written = ([threading.Event() for _ in range(n)] for _ in range(3))
    abort, errors = threading.Event(), []

    def wait(event):
        while not event.wait(0.05):
            if abort.is_set():
                raise _Aborted()
        if abort.is_set():
            raise _Aborted()

    def guarded(body):
        def run():
            try:
                body()
            except _Aborted:
                pass
            except BaseException as exc:          # handed to the caller's thread
                errors.append(exc)
                abort.set()
        return run

    def uploads():
        for k in range(n):
            if k >= nsets:
                wait(computed[k - nsets])
                if write_reads_forcing:
                    wait(written[k - nsets])
            upload(k, k % nsets)
            uploaded[k].set()

    def computes():
        for k in range(n):
            wait(uploaded[k])
            if k >= nsets:
                wait(written[k - nsets])
            compute(k, k % nsets)
            computed[k].set()

    def writes():
        for k in range(n):
            wait(computed[k])
            write(k, k % nsets)
            written[k].set()

    threads = [threading.Thread(target=guarded(uploads), name='xh-ens-upload'),
               threading.Thread(target=guarded(writes), name='xh-ens-write')]
    for t in threads:
        t.start()
    guarded(computes)()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]


class _Lazy(dict):
    """stat -> host array; an array still in HBM is fetched (and released there) the first time it is read."""

    def __getitem__(self, key):
        v = dict.__getitem__(self, key)
        if isinstance(v, _hip.DeviceArray):
            host = v.download()
            v.free()
            dict.__setitem__(self, key, host)
            v = host
        return v

    def get(self, key, default=None):
        return self[key] if key in self else default

    def items(self):
        return [(k, self[k]) for k in self]

    def values(self):
        return [self[k] for k in self]


class EnsembleResult:
    """names, member_dirs, statistics[var][stat] (host arrays, fetched from HBM on first read), timings (seconds per
    member: 'upload', 'kernels', 'post', 'write'; 'statistics' and 'total' for the run), forcing_upload (per member, what
    DevicePipeline.set_forcing sent: {forcing name: (kind, bytes host -> device)}; a resident ensemble uploads once, the
    other members' entries are empty), kge [members, basins] and kge_basins (ascending basin ids) with ``observed``: each
    member's Kling-Gupta efficiency against the observed basin runoff, also in ensemble/member_kge.csv; None without."""

    def __init__(self, names, member_dirs, statistics, timings, forcing_upload=None, kge=None, kge_basins=None, gauges=None):
        self.names, self.member_dirs, self.statistics, self.timings = names, member_dirs, statistics, timings
        self.forcing_upload = forcing_upload
        self.kge, self.kge_basins = kge, kge_basins
        # with stream gauges: gauge_ids (the order of the gauges file), gauge_kge [members, gauges], gauge_skill {column:
        # [members, gauges]} (evaluate.COLUMNS), gauge_flow [members, gauges, nmonths] and, with statistics,
        # gauge_flow_statistics {stat: [gauges, nmonths]}; None without
        g = gauges or {}
        self.gauge_ids, self.gauge_skill, self.gauge_flow = g.get('ids'), g.get('skill'), g.get('flow')
        self.gauge_kge = None if self.gauge_skill is None else self.gauge_skill['kge']
        self.gauge_flow_statistics = g.get('statistics')


def run(config, members=None, statistics=None, statistics_vars=None, member_outputs=None, overlap=True, observed=None,
        obs_unit=None, gauges=None, gauge_observed=None, gauge_missing=None):
    """The driver behind run_ensemble / Xanthos.execute_ensemble; ``config``: a staged ConfigReader."""
    s = config
    ens = getattr(s, 'ensemble', None) or {}
    if members is None:
        if not ens:
            raise refuse(None, 'members', 'neither a members argument nor an [Ensemble] section')
        members = read_members(s, ens['members'])
    statistics = ens.get('statistics', ()) if statistics is None else statistics
    statistics_vars = ens.get('statistics_vars') if statistics_vars is None else statistics_vars
    member_outputs = ens.get('member_outputs', 1) if member_outputs is None else member_outputs
    observed = ens.get('observed') if observed is None else observed
    obs_unit = ens.get('obs_unit') if obs_unit is None else obs_unit
    plan = validate(s, members, statistics, statistics_vars, member_outputs, observed=observed, obs_unit=obs_unit,
                    gauges=gauges, gauge_observed=gauge_observed, gauge_missing=gauge_missing)
    ctx = _hip.get_context(s.device)                      # HipUnavailable without a device: there is no host fallback
    check_fits(plan, ctx.mem_info()[0])
    return _Driver(s, plan, ctx, overlap).run()


class _Driver:
    def __init__(self, s, plan, ctx, overlap):
        self.s, self.plan, self.ctx, self.overlap = s, plan, ctx, bool(overlap)
        n = len(plan.names)
        self.timings = {k: [0.0] * n for k in ('upload', 'kernels', 'post', 'write')}
        self.forcing_upload = [{} for _ in range(n)]
        self.member_dirs = [os.path.join(s.OutputFolder, name) for name in plan.names]
        self.settings = []
        for k in range(n):
            cfg = copy.copy(s)
            for key, value in plan.overrides[k].items():      # (a member's table is its run's calib_file)
                setattr(cfg, 'calib_file' if key == PARS_KEY else key, value)
            cfg.OutputFolder = self.member_dirs[k]
            self.settings.append(cfg)
        self.stack = {v: [] for v in plan.statistics_vars}
        self.up = self.wr = None
        self.member_pars = [None] * n                     # DeviceArray of a member's own parameter table
        self.run_pars = self.skill = self.kge = None
        self.gauges = self.gauge_result = None            # the device tables of xh_gauge_skill; what member_gauge_skill() made

    # ---- set-up: everything static, once
    def setup(self):
        s, ctx = self.s, self.ctx
        runner = ConfigRunner(s)
        self.c = c = Components(s, gauges=self.plan.gauge_skill)
        self.runoff = s.runoff_module if runner.run_runoff else 'none'
        c.check_resident(self.runoff)
        um = c.topology() if (runner.run_routing and s.routing_module == 'mrtm') else None
        self.pipe = pipe = DevicePipeline(ctx, **c._pipeline_args(self.runoff, um))
        pipe.plan                                         # the one routing plan of all members (waits for the partition)
        shape = (pipe.ncell, pipe.nmonths)
        if self.runoff == 'abcd':                         # the tables of all members, a few KB each
            self.run_pars = pipe.d_pars
            for k, overrides in enumerate(self.plan.overrides):
                table = overrides.get(PARS_KEY)
                if table is not None:
                    table = table if isinstance(table, np.ndarray) else np.load(table)
                    self.member_pars[k] = ctx.upload(np.asarray(table, dtype=np.float64))
        if c.grid is not None:                            # GriddedOutput = 1: the table of the maps, up before any writer asks
            c.grid.device_table(ctx)
        resident = self.plan.resident
        if not self.overlap:
            self.up = self.wr = ctx
            self.sets = [(pipe.forcing, pipe.out)]
            self.setup_skill()
            return
        # two buffer sets: the forcing belongs to the uploading context, the outputs to the writing one (a DeviceArray's
        # copies run on the context that made it, and a context serves one host thread); the kernels only take pointers
        self.up, self.wr = _hip.Context(ctx.device), _hip.Context(ctx.device)
        for a in pipe.out.values():
            a.free()
        self.sets = []
        forcing = {}                                      # resident: both sets read the one forcing ...
        for _ in range(2):
            out = {k: self.wr.empty(shape) for k in OUTPUTS if not (resident and self.sets and k == 'pet')}
            if resident and self.sets:                    # ... and refer to the one PET (owned by the first set's entry)
                out['pet'] = self.sets[0][1]['pet']
            if self.runoff == 'none':
                for k in ('aet', 'q', 'sav'):
                    out[k].zero()
            self.sets.append((forcing if resident else {}, out))
        self.wr.sync()
        pipe.forcing, pipe.out = self.sets[0]
        self.setup_skill()

    def setup_skill(self):
        """The tables of xh_basin_kge, once per ensemble, on the writing context: the skill is formed in the write stage."""
        gs = self.plan.gauge_skill
        if gs is not None:             # xh_gauge_skill: cells and records once, every member's hydrographs and metrics
            wr, n, ng = self.wr, len(self.plan.names), gs.ids.size
            self.gauges = SimpleNamespace(
                ngauge=ng, cells=wr.upload(gs.cells, dtype=np.int32), obs=wr.upload(gs.obs),
                series=wr.empty((n, ng, self.pipe.nmonths)), metrics=wr.empty((n, ng, gskill.NCOLS)))
            wr.sync()
        sk = self.plan.skill
        if sk is None:
            return
        wr, n, nb = self.wr, len(self.plan.names), len(sk.basins)
        self.skill = SimpleNamespace(
            nbasins=nb, start=wr.upload(sk.start, dtype=np.int64), cells=wr.upload(sk.cells, dtype=np.int32),
            obs=wr.upload(sk.obs), area=wr.upload(self.c.data.area) if sk.unit == 'km3_per_mth' else None,
            series=wr.empty((nb, self.pipe.nmonths)), ed=wr.empty((n, nb)))
        wr.sync()

    def member_forcing(self, k):
        """Host forcing of member k by DevicePipeline name: the member's own arrays / memory maps where it overrides a
        setting (loaded as DataLoader loads them), the run's otherwise."""
        s, cfg, data = self.s, self.settings[k], self.c.data
        loader = copy.copy(data)
        loader.s = cfg
        host = {}
        for module in (s.pet_module, self.runoff):
            for name, attr in _FORCING_DATA[module].items():
                setting, varkey, clean = _FORCING_SETTINGS[module][name]
                if setting in self.plan.overrides[k]:
                    try:
                        host[name] = loader.load_to_array(getattr(cfg, setting), setting, nan_to_num=clean,
                                                          key=getattr(cfg, varkey, None) if varkey else None)
                    except ValidationException as exc:
                        raise refuse(self.plan.names[k], setting, str(exc))
                else:
                    host[name] = getattr(data, attr, None)
        return host

    # ---- the three stages of a member
    def upload(self, k, i):
        if self.plan.resident and k > 0:                  # the forcing is up: nothing crosses PCIe for this member
            return
        t = time.time()
        self.pipe.set_forcing(self.member_forcing(k), ctx=self.up, into=self.sets[i][0])
        self.up.sync()
        self.timings['upload'][k] = time.time() - t
        self.forcing_upload[k] = dict(self.pipe.forcing_upload)

    def compute(self, k, i):
        t = time.time()
        pipe = self.pipe
        pipe.forcing, pipe.out = self.sets[i]
        if self.run_pars is not None:                     # the member's own table, or the run's
            pipe.d_pars = self.member_pars[k] if self.member_pars[k] is not None else self.run_pars
        if self.plan.resident:                            # PET does not depend on the parameters: once, before the first member
            if k == 0:
                pipe.run_pet()
            pipe.run(stages=(self.runoff,) + (('mrtm',) if pipe.um is not None else ()), fed=False, fused=False)
        else:
            pipe.run(fed=False, fused=False)              # the stages strictly in order, as Components.simulation
        self.ctx.sync()
        self.timings['kernels'][k] = time.time() - t

    def write(self, k, i):
        if self.wr is not self.ctx:
            with _hip.thread_context(self.wr):
                self._write(k, i)
        else:
            self._write(k, i)

    def _write(self, k, i):
        plan, pipe, cfg = self.plan, self.pipe, self.settings[k]
        view = SimpleNamespace(out=self.sets[i][1], plan=pipe.plan, ncell=pipe.ncell, nmonths=pipe.nmonths,
                               forcing=self.sets[i][0])        # (the member's own forcing: SPI / SPEI index it)
        c = self.c.member_view(cfg, view)
        logging.info("---ensemble member '{}' ({} of {})".format(plan.names[k], k + 1, len(plan.names)))
        t = time.time()
        sk = self.skill
        if sk is not None:                                # ED of this member's Q, mm per month, into row k (asynchronous)
            self.wr.basin_kge(pipe.ncell, pipe.nmonths, sk.nbasins, sk.start, sk.cells, self.sets[i][1]['q'], sk.area, sk.obs,
                              sk.ed.ptr + 8 * k * sk.nbasins, series=sk.series)
        gd = self.gauges
        if gd is not None:                                # this member's Avg_ChFlow at the gauges, into slice k (asynchronous)
            series = gd.series.ptr + 8 * k * gd.ngauge * pipe.nmonths
            metrics = gd.metrics.ptr + 8 * k * gd.ngauge * gskill.NCOLS
            self.wr.gauge_skill(pipe.ncell, pipe.nmonths, gd.ngauge, gd.cells, self.sets[i][1]['avg'], gd.obs, metrics, series=series)
        if plan.member_outputs:                           # the phases of ConfigRunner.run() after the simulation, in its order
            os.makedirs(cfg.OutputFolder, exist_ok=True)
            c.accessible_water()
            c.drought()
            self._drought_index(c)
            c.hydropower_potential()
            c.hydropower_actual()
            if gd is not None:                            # Components.evaluate()'s two files, from slice k
                gs = plan.gauge_skill
                raw, flow = np.empty((gd.ngauge, gskill.NCOLS)), np.empty((gd.ngauge, pipe.nmonths))
                self.wr.d2h_async(raw, metrics)
                self.wr.d2h_async(flow, series)
                self.wr.sync()
                gskill.write_skill(os.path.join(cfg.OutputFolder, gskill.SKILL_FILE), gs, gskill.skill_table(raw))
                gskill.write_flow(os.path.join(cfg.OutputFolder, gskill.FLOW_FILE), gs, flow, gskill.month_labels(cfg))
            c.diagnostics()
        elif any(index_scale(v) is not None for v in plan.statistics_vars):
            self._drought_index(c)                        # member_outputs = 0: no files, the arrays for the statistics
        self.timings['post'][k] = time.time() - t
        t = time.time()
        if not (plan.member_outputs or plan.statistics_vars):      # (member_outputs = 0 with observed or gauges alone: only the skill)
            self.wr.sync()
            self.timings['write'][k] = time.time() - t
            return
        c.output_simulation(keep_device=bool(plan.statistics_vars), write_files=bool(plan.member_outputs))
        if plan.member_outputs and cfg.CreateTimeSeriesPlot:
            c.plots()
        w = c._writer
        for var in plan.statistics_vars:                  # the array as written joins the member stack in HBM
            if index_scale(var) is not None:              # (the member's index array: _drought_index put it there)
                continue
            arr, owned = w.get_device(var)
            if not owned:                                 # the run's own array: the next member of this set overwrites it
                arr = w.ctx.d2d(w.ctx.empty(arr.shape), arr)
            self.stack[var].append(arr)
        for a in w.device_outputs.values():
            a.free()
        w.device_outputs = {}
        w.ctx.sync()
        if (sk is not None or gd is not None) and w.ctx is not self.wr:
            self.wr.sync()
        self.timings['write'][k] = time.time() - t

    def _drought_index(self, c):
        """Components.drought_index() of one member: its files with member_outputs = 1, and the arrays of the scales named
        in statistics_vars onto the member stack (they are the member's own: nothing overwrites them)."""
        if not getattr(c.s, 'CalculateDroughtIndex', 0):
            return
        wanted = {index_scale(v): v for v in self.plan.statistics_vars if index_scale(v) is not None}
        c.drought_index(keep_on_device=True, write_files=bool(self.plan.member_outputs))      # (no download: files leave from HBM)
        for k, arr in c.drought_index.items():
            if k in wanted:
                self.stack[wanted[k]].append(arr)
            else:
                arr.free()

    # ---- the across-member statistics
    def statistics(self):
        from .data_writer.out_writer import OutWriter
        plan, s, ctx = self.plan, self.s, self.ctx
        result = {}
        if not plan.statistics_vars:
            return result
        cfg = copy.copy(s)
        cfg.OutputFolder = os.path.join(s.OutputFolder, STATISTICS_DIR)
        w = OutWriter(cfg, self.c.data.area, {}, grid=self.c.grid)
        plain = [label for label in _hip.ENS_STAT_BITS if any(label == l for l, _ in plan.statistics)]      # the library's order
        quant = [(label, q) for label, q in plan.statistics if q is not None]
        for var in plan.statistics_vars:
            members = self.stack[var]
            shape = members[0].shape
            outs = [ctx.empty(shape) for _ in range(len(plain) + len(quant))]
            ctx.ens_stats(members[0].size, members, plain, [q for _, q in quant], outs)
            ctx.sync()
            for a in members:
                a.free()
            self.stack[var] = []
            result[var] = _Lazy()
            for label, arr in zip(plain + [label for label, _ in quant], outs):
                if index_scale(var) is not None:
                    from .drought.standardized import output_stem
                    w.write_data('{}_{}'.format(output_stem(cfg, s.drought_index['var'], index_scale(var)), label),
                                 'drought_index', arr, w.time_steps)
                    dict.__setitem__(result[var], label, arr)
                    continue
                filename = os.path.join(cfg.OutputFolder, '{}_{}_{}_{}'.format(var, w.unit_of(var), s.ProjectName, label))
                w.write_data(filename, var, arr, w.time_steps)      # npy and csv are written from HBM
                dict.__setitem__(result[var], label, arr)
        return result

    def member_skill(self):
        """KGE = 1 - ED [members, basins] from HBM, and the table ensemble/member_kge.csv (written on the host)."""
        sk, plan = self.skill, self.plan
        if sk is None:
            return
        self.kge = 1.0 - sk.ed.download()
        folder = os.path.join(self.s.OutputFolder, STATISTICS_DIR)
        os.makedirs(folder, exist_ok=True)
        with open(os.path.join(folder, KGE_TABLE), 'w') as fh:
            fh.write('name,' + ','.join(str(b) for b in plan.skill.basins) + '\n')
            for name, row in zip(plan.names, self.kge):
                fh.write(name + ',' + ','.join(repr(float(v)) for v in row) + '\n')

    def member_gauge_skill(self):
        """The members' skill at the stream gauges from HBM -- {column: [members, gauges]}, the hydrographs [members,
        gauges, nmonths] --, the tables ensemble/member_gauge_kge.csv (one column per gauge, the format of member_kge.csv)
        and member_gauge_skill.csv (long form), and with statistics the across-member statistics of the hydrographs
        (xh_ens_stats on the members' slices in HBM) as ensemble/gauge_flow_<stat>.csv."""
        gd, plan, gs = self.gauges, self.plan, self.plan.gauge_skill
        if gd is None:
            return
        wr = self.wr
        skill = gskill.skill_table(gd.metrics.download())
        flow = gd.series.download()
        folder = os.path.join(self.s.OutputFolder, STATISTICS_DIR)
        os.makedirs(folder, exist_ok=True)
        with open(os.path.join(folder, GAUGE_KGE_TABLE), 'w') as fh:
            fh.write('name,' + ','.join(str(int(g)) for g in gs.ids) + '\n')
            for name, row in zip(plan.names, skill['kge']):
                fh.write(name + ',' + ','.join(repr(float(v)) for v in row) + '\n')
        with open(os.path.join(folder, GAUGE_SKILL_TABLE), 'w') as fh:
            fh.write('name,gauge_id,' + ','.join(gskill.COLUMNS) + '\n')
            for k, name in enumerate(plan.names):
                member = {col: v[k] for col, v in skill.items()}
                for g in range(gd.ngauge):
                    fh.write(','.join([name, str(int(gs.ids[g]))] + gskill.skill_fields(member, g)) + '\n')
        stats = None
        if plan.statistics:
            plain = [label for label in _hip.ENS_STAT_BITS if any(label == l for l, _ in plan.statistics)]      # the library's order
            quant = [(label, q) for label, q in plan.statistics if q is not None]
            n = gd.ngauge * self.pipe.nmonths
            outs = [wr.empty((gd.ngauge, self.pipe.nmonths)) for _ in range(len(plain) + len(quant))]
            try:
                wr.ens_stats(n, [gd.series.ptr + 8 * k * n for k in range(len(plan.names))], plain, [q for _, q in quant], outs)
                stats = {label: arr.download() for label, arr in zip(plain + [label for label, _ in quant], outs)}
            finally:
                for a in outs:
                    a.free()
            labels = gskill.month_labels(self.s)
            for label, arr in stats.items():
                gskill.write_flow(os.path.join(folder, GAUGE_STAT_FILE.format(label)), gs, arr, labels)
        self.gauge_result = {'ids': [int(g) for g in gs.ids], 'skill': skill, 'flow': flow, 'statistics': stats}

    def run(self):
        plan = self.plan
        t0 = time.time()
        logging.info('---ensemble of {} members in progress ({})...'.format(
            len(plan.names), 'overlapped' if self.overlap else 'one after the other'))
        try:
            self.setup()
            di = self.c.s.drought_index if getattr(self.c.s, 'CalculateDroughtIndex', 0) else None
            run_schedule(len(plan.names), self.upload, self.compute, self.write, overlap=self.overlap,
                         write_reads_forcing=di is not None and di['var'] in ('precip', 'balance'))
            self.member_skill()
            t = time.time()
            self.member_gauge_skill()
            stats = self.statistics()
            self.timings['statistics'] = time.time() - t
        finally:
            for owned in self.stack.values():
                for a in owned:
                    a.free()
            for a in self.member_pars + [v for tables in (self.skill, self.gauges) for v in vars(tables or SimpleNamespace()).values()
                                         if isinstance(v, _hip.DeviceArray)]:
                if a is not None:
                    a.free()
            if getattr(self, 'pipe', None) is not None:
                self.pipe.close()
            for extra in (self.up, self.wr):
                if extra is not None and extra is not self.ctx:
                    extra.close()
        self.timings['total'] = time.time() - t0
        n = max(len(plan.names), 1)
        logging.info('ensemble phases (s per member): ' + ', '.join(
            '{} {:.3f}'.format(k, sum(self.timings[k]) / n) for k in ('upload', 'kernels', 'post', 'write')) +
            '; statistics {:.3f} s, total {:.3f} s'.format(self.timings['statistics'], self.timings['total']))
        return EnsembleResult(list(plan.names), list(self.member_dirs) if plan.member_outputs else [], stats, self.timings,
                              self.forcing_upload, kge=self.kge, kge_basins=list(plan.skill.basins) if plan.skill else None,
                              gauges=self.gauge_result)
