"""Skill of a forward run's routed streamflow at stream gauges ([Evaluate]).

The reference scores streamflow inside its calibration only; a parameter set that is run forward afterwards is compared
with measured discharge, if at all, by hand from the ``avgchflow`` file.  With ``[Evaluate] gauges`` / ``gauge_observed``
(the file formats of the ``[Calibrate]`` keys of the same names: rows gauge_id,cell_id[,weight] and rows [gauge_id, *, *,
value], NaN or ``gauge_missing`` = no observation; the weight is read and ignored) the rows of the gauge cells are picked
out of Avg_ChFlow and scored where they lie, in HBM (``xh_gauge_skill``): per gauge the months used, KGE and its three
components, NSE, PBIAS and RMSE over the months with a finite observation.  Only ``[ngauge, 8]`` metrics and the
``[ngauge, nmonths]`` hydrographs cross PCIe.

``GaugeSkill(settings, gauge_set, flow)`` is the post-processor of a single run (``Components.evaluate``): it writes
``gauge_skill.csv`` and ``gauge_flow.csv`` into ``settings.OutputFolder``.  The ensemble driver (ensemble.py) uses the
tables, the column names and the two writers for every member.
"""
import logging
import os
from types import SimpleNamespace

import numpy as np

from .. import _hip
from ..calibrate.gauge_tables import check_gauges, check_records
from ..data_load import load_file, load_gauges
from ..ini_reader import ValidationException

NCOLS = 8                                        # columns of xh_gauge_skill's metrics
COLUMNS = ('months_used', 'kge', 'r', 'alpha', 'beta', 'nse', 'pbias', 'rmse')      # ... as the tables name them
SKILL_FILE, FLOW_FILE = 'gauge_skill.csv', 'gauge_flow.csv'
MAX_GAUGES = 65535                               # one launch of xh_gauge_skill


def refuse(key, why):
    return ValidationException('[Evaluate] {}: {}'.format(key, why))


def check_routes(s):
    """[Evaluate] scores Avg_ChFlow: the run has to route."""
    if getattr(s, 'routing_module', 'none') != 'mrtm':
        raise refuse('gauges', "the gauges are scored on the routed channel flow (Avg_ChFlow) and need routing_module = mrtm, "
                     "not '{}'".format(getattr(s, 'routing_module', 'none')))


def load_gauge_set(s, gauges=None, gauge_observed=None, gauge_missing=None):
    """The gauges of a forward run, loaded and checked before any GPU work: ``gauges`` / ``gauge_observed`` /
    ``gauge_missing`` (default: the ini's [Evaluate] keys).  Returns ids [ng] int64, cells [ng] int32 (0-based), basins
    [ng] (the basin of each gauge's cell), obs [ng, nmonths] (NaN = no observation) and months_used [ng], in the order of
    the gauges file."""
    ev = getattr(s, 'evaluate', None) or {}
    if gauges is None and gauge_observed is None:
        gauges, gauge_observed = ev.get('gauges'), ev.get('gauge_observed')
        gauge_missing = ev.get('gauge_missing') if gauge_missing is None else gauge_missing
    if (gauges is None) != (gauge_observed is None):
        raise refuse('gauges' if gauges is None else 'gauge_observed',
                     'gauges and gauge_observed go together: the stations and their records')
    check_routes(s)
    for key, path in (('gauges', gauges), ('gauge_observed', gauge_observed)):
        if not isinstance(path, str) or not os.path.isfile(path):
            raise refuse(key, 'file {} does not exist'.format(path))
    try:
        g = load_gauges(gauges, gauge_observed, s.nmonths, None if gauge_missing is None else float(gauge_missing))
    except ValidationException as exc:
        raise refuse('gauge_observed' if 'gauge_observed' in str(exc) else 'gauges', str(exc))
    if g.ids.size < 1 or g.ids.size > MAX_GAUGES:
        raise refuse('gauges', '{} gauges; one run scores between 1 and {}'.format(g.ids.size, MAX_GAUGES))
    try:
        check_gauges(g, s.ncell)
    except ValidationException as exc:
        raise refuse('gauges', str(exc))
    try:
        check_records(g.ids, g.obs)
    except ValidationException as exc:
        raise refuse('gauge_observed', str(exc))
    basin_of = np.asarray(load_file(s.BasinIDs, 1)).reshape(-1).astype(np.int64)
    return SimpleNamespace(ids=g.ids, cells=g.cells.astype(np.int32), basins=basin_of[g.cells],
                           obs=np.ascontiguousarray(g.obs[:, :s.nmonths], dtype=np.float64),
                           months_used=np.isfinite(g.obs[:, :s.nmonths]).sum(1))


def month_labels(s):
    """The column names the writer gives the months of avgchflow."""
    return ['{}{:02}'.format(y, m) for y in range(s.StartYear, s.EndYear + 1) for m in range(1, 13)]


def skill_table(raw):
    """xh_gauge_skill's metrics [..., 8] -> {column: ndarray [...]}: months_used as integers, kge = 1 - ED, the rest as
    they are."""
    raw = np.asarray(raw)
    out = {'months_used': raw[..., 0].astype(np.int64), 'kge': 1.0 - raw[..., 1]}
    for j, name in enumerate(COLUMNS[2:], start=2):
        out[name] = raw[..., j].copy()
    return out


def skill_fields(skill, g):
    """The fields of gauge ``g`` in a skill table from months_used on, as the csv files hold them."""
    return [str(int(skill['months_used'][g]))] + [repr(float(skill[name][g])) for name in COLUMNS[1:]]


def write_skill(path, gs, skill):
    """gauge_skill.csv: one row per gauge in the order of the gauges file; cell_id 1-based, floats as repr."""
    with open(path, 'w') as fh:
        fh.write('gauge_id,basin,cell_id,' + ','.join(COLUMNS) + '\n')
        for g in range(gs.ids.size):
            fh.write(','.join([str(int(gs.ids[g])), str(int(gs.basins[g])), str(int(gs.cells[g]) + 1)] +
                              skill_fields(skill, g)) + '\n')


def write_flow(path, gs, flow, labels):
    """gauge_flow.csv: the simulated series of every gauge [ngauge, nmonths], floats as repr."""
    with open(path, 'w') as fh:
        fh.write('gauge_id,' + ','.join(labels[:flow.shape[1]]) + '\n')
        for gid, row in zip(gs.ids, flow):
            fh.write(str(int(gid)) + ',' + ','.join(repr(float(v)) for v in row) + '\n')


class GaugeSkill:
    """Score ``flow`` (Avg_ChFlow [ncell, nmonths] in m3/s, a DeviceArray or a host array) at the gauges of ``gauge_set``
    (``load_gauge_set``): one upload of the gauge cells and records, one xh_gauge_skill call, the downloads of [ngauge, 8]
    and [ngauge, nmonths], the two files.  ``skill``: {column: ndarray [ngauge]}; ``flow``: [ngauge, nmonths]."""

    def __init__(self, settings, gauge_set, flow):
        gs = gauge_set
        ctx = _hip.get_context(getattr(settings, 'device', 0))
        mine = not isinstance(flow, _hip.DeviceArray)
        src = ctx.upload(np.ascontiguousarray(flow, dtype=np.float64)) if mine else flow
        ncell, nmonths = src.shape
        ng = gs.ids.size
        if gs.obs.shape != (ng, nmonths):
            raise ValueError('the gauge records are {}, the flow has {} months'.format(gs.obs.shape, nmonths))
        bufs = [ctx.upload(gs.cells, dtype=np.int32), ctx.upload(gs.obs), ctx.empty((ng, nmonths)), ctx.empty((ng, NCOLS))]
        try:
            d_cells, d_obs, d_series, d_metrics = bufs
            ctx.gauge_skill(ncell, nmonths, ng, d_cells, src, d_obs, d_metrics, series=d_series)
            self.skill = skill_table(d_metrics.download())
            self.flow = d_series.download()
        finally:
            for b in bufs + ([src] if mine else []):
                b.free()
        os.makedirs(settings.OutputFolder, exist_ok=True)
        write_skill(os.path.join(settings.OutputFolder, SKILL_FILE), gs, self.skill)
        write_flow(os.path.join(settings.OutputFolder, FLOW_FILE), gs, self.flow, month_labels(settings))
        logging.info('\t{} gauges scored ({} and {})'.format(ng, SKILL_FILE, FLOW_FILE))
