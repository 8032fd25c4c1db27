"""Diagnostics (mirror of xanthos/diagnostics/diagnostics.py:20-131) on the GPU.

``Diagnostics(settings, Q, ref)`` keeps the reference's call surface.  ``Q`` is the run's own runoff ``[ncell, nmonths]``
in mm/month, a host array or a DeviceArray (``Components.diagnostics`` hands over the one the pipeline holds in HBM).
The reductions over cells are HIP kernels (csrc/xh_diag.hip): each cell's total in numpy's pairwise order, scaled to
km3/yr as the reference scales it, the mean of the VIC columns in the same order, and pandas' compensated per-group sums.
The host builds the small per-scale tables with pandas, adds the global row and writes the csv files, as the reference
does.  Its quirks are kept: country names are matched to ids from 0, basin and region names from
1; a WBM row with id 0 lands on the last cell; names without ids come out as rows of 0.  Where it crashes, this module
refuses with a ValidationException that names the input.
"""
import logging
import os

import numpy as np
import pandas as pd

from .. import _hip
from ..hydropower.potential import device_rows
from ..ini_reader import ValidationException

REF_DATA_NAME = 'VIC_1971-2000'
COLUMNS = ['xanthos', REF_DATA_NAME, 'WBM', 'WBMc', 'UNH_1986-1995']
FILE = 'Diagnostics_Runoff_{}_Scale_km3peryr.csv'
SCALES = (('Basin', 1, 'basin', 1), ('Country', 2, 'country', 0), ('Region', 3, 'region', 1))


def scatter_table(table, ncell, name):
    """A two-column (cell id, value) table scattered by id - 1 into zeros, row by row as diagnostics.py:68-72 does: a
    later row wins, id 0 lands on the last cell (Python's index -1)."""
    t = np.asarray(table, dtype=float)
    if t.ndim != 2 or t.shape[1] < 2:
        raise ValidationException('{} must be a table of (cell id, value) rows, not shape {}'.format(name, t.shape))
    out = np.zeros(ncell, dtype=float)
    if t.shape[0] == 0:
        return out
    if not np.isfinite(t[:, 0]).all():
        raise ValidationException('{} holds a cell id that is not a number'.format(name))
    idx = t[:, 0].astype(np.int64) - 1                       # int() truncates toward zero, as astype does
    bad = (idx < -ncell) | (idx >= ncell)
    if bad.any():
        raise ValidationException('{}: cell id {} is outside the {} cells'.format(name, int(t[np.argmax(bad), 0]), ncell))
    idx = idx % ncell
    last = len(idx) - 1 - np.unique(idx[::-1], return_index=True)[1]        # the last row of each cell
    out[idx[last]] = t[last, 1]
    return out


def cell_columns(ctx, Q, area, nyear, vic, wbm, wbmc, unh):
    """The five per-cell columns of diagnostics.py:58-72 as a DeviceArray [ncell, 5]: xanthos, VIC mean, WBM, WBMc, UNH.
    Column 0 is np.sum(Q, axis=1) / nyear * area / 1e6 and column 1 np.mean(VIC, axis=1), both reduced on the device."""
    src, mine = device_rows(ctx, Q)
    ncell, nmonths = src.shape
    area = np.ascontiguousarray(area, dtype=np.float64).reshape(-1)
    vic = np.asarray(vic, dtype=np.float64)
    unh = np.asarray(unh, dtype=np.float64)
    if area.shape != (ncell,):
        raise ValidationException('the grid areas hold {} cells, the runoff {}'.format(area.shape[0], ncell))
    if vic.ndim != 2 or vic.shape[0] != ncell or vic.shape[1] < 1:
        raise ValidationException('VICDataFile must hold {} rows of one or more columns (np.mean(VIC, axis=1)), not shape '
                                  '{}'.format(ncell, vic.shape))
    if unh.shape != (ncell,):
        raise ValidationException('UNHDataFile must hold one value per cell ({}), not shape {}'.format(ncell, unh.shape))
    host = np.zeros((ncell, len(COLUMNS)))
    host[:, 2] = scatter_table(wbm, ncell, 'WBMDataFile')
    host[:, 3] = scatter_table(wbmc, ncell, 'WBMCDataFile')
    host[:, 4] = unh
    vals = ctx.upload(host)
    d_area, d_vic = ctx.upload(area), ctx.upload(np.ascontiguousarray(vic))
    k = len(COLUMNS)
    ctx.diag_cell_total(ncell, nmonths, src, float(nyear), d_area, 1e6, vals, k)
    ctx.diag_cell_total(ncell, vic.shape[1], d_vic, float(vic.shape[1]), None, 1.0, vals.ptr + 8, k)
    for b in (d_area, d_vic, src if mine else None):
        if b is not None:
            b.free()
    return vals


def group_sums(ctx, vals, id_map):
    """runoff_df.groupby('id', as_index=False).sum() of the [ncell, k] DeviceArray (diagnostics.py:111-112): the sorted
    ids that have cells, and the [ngroups, k] compensated sums."""
    ncell, k = vals.shape
    ids = np.asarray(id_map).reshape(-1).astype(np.int64)
    if ids.shape != (ncell,):
        raise ValidationException('the id map holds {} cells, the runoff {}'.format(ids.shape[0], ncell))
    uniq, inv = np.unique(ids, return_inverse=True)
    d_sums, d_counts = ctx.empty((len(uniq), k)), ctx.empty((len(uniq),), dtype=np.int64)
    ctx.diag_group_sum(ncell, k, len(uniq), inv, vals, d_sums, d_counts)
    sums, counts = d_sums.download(), d_counts.download()
    d_sums.free()
    d_counts.free()
    return uniq, sums, counts


def scale_table(uniq, sums, name_map, name_map_offset=0):
    """diagnostics.py:101-128 from the grouped sums: names left-merged with the groups, a Global row of column sums on top
    (every column after ``name``: the intent of ``agg_df.loc[-1, 1:]``, which pandas >= 2 refuses), ids shifted by one."""
    agg_df = pd.DataFrame(sums, columns=COLUMNS)
    agg_df.insert(0, 'id', uniq)
    names_df = pd.DataFrame({'name': name_map})
    names_df.index += name_map_offset
    agg_df = names_df.merge(agg_df, 'left', left_index=True, right_on='id')
    agg_df.set_index('id', inplace=True)
    agg_df.loc[-1, 'name'] = 'Global'
    agg_df.loc[-1, agg_df.columns[1:]] = agg_df.sum(numeric_only=True)
    agg_df.index = agg_df.index + 1
    return agg_df.sort_index()


class Diagnostics:
    """Average annual runoff (km3/yr) per basin, country and region next to VIC, WBM, WBMc and UNH (diagnostics.py:20)."""

    def __init__(self, settings, xanthos_q, ref):
        self.tables = {}
        if not settings.PerformDiagnostics:
            return
        self.REF_DATA_NAME = REF_DATA_NAME
        self.output_folder = settings.OutputFolder
        ctx = _hip.get_context(getattr(settings, 'device', 0))
        nyear = int(settings.EndYear - settings.StartYear + 1)
        vals = cell_columns(ctx, xanthos_q, ref.area, nyear, ref.vic, ref.wbmd, ref.wbmc, ref.unh)
        try:
            for scale, code, attr, offset in SCALES:
                if settings.DiagnosticScale in (0, code):
                    ids, names = getattr(ref, attr + '_ids'), getattr(ref, attr + '_names')
                    self.tables[scale] = self.write_diagnostics(ctx, scale, vals, ids, names, offset)
        finally:
            vals.free()

    def write_diagnostics(self, ctx, scale, vals, id_map, name_map, name_map_offset=0):
        """Group, name, total and write one scale (diagnostics.py:96-131); returns the table as written."""
        uniq, sums, _ = group_sums(ctx, vals, id_map)
        agg_df = scale_table(uniq, sums, name_map, name_map_offset)
        os.makedirs(self.output_folder, exist_ok=True)
        output_name = os.path.join(self.output_folder, FILE.format(scale))
        agg_df.to_csv(output_name, na_rep=0, index=False)
        logging.info('Diagnostics written to {}'.format(output_name))
        return agg_df
