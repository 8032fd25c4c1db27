"""Water balance and Budyko signatures per grid cell and per basin on the GPU (no counterpart in the reference): where each cell
or basin sits in Budyko space (aridity and evaporative index, Fu's parameter, the departure from a Budyko curve), how much of
its precipitation runs off, whether the balance closes, how strongly runoff answers a 1 % change of precipitation or of PET
(Sankarasubramanian et al. 2001, as the median of the annual ratios and by bivariate least squares), and after how many months
it answers.

``balance_rows(ctx, precip, pet, q, aet=None, ...)`` runs ``xh_water_balance`` (csrc/xh_wbalance.hip; the definition stands in
csrc/xh_wbalance_dev.h, include/xanthos_hip.h and DESIGN 4.24) on ``[nrows, ncols]`` arrays, host or DeviceArray, and returns the
table ``[nrows, 21]`` of ``COLUMNS``, the annual totals ``[nrows, 4, nyear]`` of P, PET, AET and Q and the cross-correlation
``[nrows, max_lag + 1]``, all in HBM.  ``WaterBalance(settings, level, ...)`` does what ``[WaterBalance]`` asks at one level --
``cell``: the run's rows as they are, in mm; ``basin``: every variable x cell area x 1e-6 (``xh_agg_time``) summed per basin
(``xh_agg_spatial``, NaN cell-months skipped), km3 per month, formed in HBM -- and writes
``water_balance_<level>_<OutputNameStr>.npy`` and ``.csv`` (ids from 1, the text formatted in HBM),
``water_balance_<level>_xcorr_<OutputNameStr>.npy`` and, with ``annual = 1``, ``water_balance_<level>_annual_<OutputNameStr>.npy``,
whatever the OutputFormat.
"""
import logging
import os

import numpy as np

from .. import _hip

COLUMNS = ('n_years', 'n_months', 'p_mean', 'pet_mean', 'aet_mean', 'q_mean', 'runoff_ratio', 'aridity', 'evaporative', 'residual',
           'closure', 'omega', 'budyko_dev', 'elast_p', 'elast_pet', 'elast_p_ls', 'elast_pet_ls', 'r_pq', 'dry_fraction', 'lag_peak',
           'r_peak')
LEVELS = ('cell', 'basin')
MAX_COLS = 4096          # months of one row's window in xh_water_balance
MAX_LAG = 12
OMEGA0 = 2.6             # Fu's parameter of the curve budyko_dev is measured from


def csv_columns(level):
    """The csv header's names: the four means carry their unit, mm per year at cell level, km3 per year at basin level."""
    unit = '_km3' if level == 'basin' else '_mm'
    return tuple(c + unit if c.endswith('_mean') else c for c in COLUMNS)


def balance_rows(ctx, precip, pet, q, aet=None, start=0, nyear=None, max_lag=6, omega0=OMEGA0):
    """(table, annual, xcorr) of the monthly window ``[:, start : start + 12 nyear]`` of the rows of ``precip``, ``pet``, ``q``
    and ``aet`` (or None), host arrays or DeviceArrays [nrows, ncols] of one shape (``nyear`` None: the whole years to the end
    of the row): DeviceArrays [nrows, 21] = ``COLUMNS``, [nrows, 4, nyear] the annual totals of P, PET, AET and Q and
    [nrows, max_lag + 1] the correlation of P with Q ``k`` months later.  A month at which any array given is NaN or +-inf is
    left out of all of them, so the rows need not be a run's grid: observed basin series with gaps are host arrays this takes
    as they are.  Asynchronous for DeviceArrays; the caller frees the three."""
    given = [precip, pet, q] + ([aet] if aet is not None else [])
    mine, src, out = [], [], []
    try:
        for a in given:
            if isinstance(a, _hip.DeviceArray):
                src.append(a)
            else:
                src.append(ctx.upload(np.ascontiguousarray(a, dtype=np.float64)))
                mine.append(src[-1])
        shape = tuple(src[0].shape)
        if len(shape) != 2 or any(tuple(a.shape) != shape for a in src):
            raise ValueError('the rows are {}, not four arrays [nrows, ncols] of one shape'.format([tuple(a.shape) for a in src]))
        nrows, stride = shape
        nyear = (stride - int(start)) // 12 if nyear is None else int(nyear)
        out = [ctx.empty((nrows, len(COLUMNS))), ctx.empty((nrows, 4, max(nyear, 0))), ctx.empty((nrows, max(int(max_lag), 0) + 1))]
        ctx.water_balance(nrows, stride, start, nyear, max_lag, omega0, src[0], src[1], src[2], src[3] if aet is not None else None,
                          out[0], out[1], out[2])
    except Exception:
        for a in out:
            a.free()
        out = None
        raise
    finally:
        if mine:
            ctx.sync()                               # the call is asynchronous: its inputs go only when it is done
            for a in mine:
                a.free()
    return tuple(out)


def basin_rows(ctx, rows, area, basin_ids, n_basins):
    """[n_basins, nmonths] km3 per month in HBM: ``rows`` [ncell, nmonths] (mm; host array or DeviceArray) x area (km2) x 1e-6
    per cell (xh_agg_time: group 1, mode 0), summed over the cells of every basin, NaN cell-months skipped (xh_agg_spatial); a
    basin without cells is NaN.  The caller frees it."""
    src = rows if isinstance(rows, _hip.DeviceArray) else ctx.upload(np.ascontiguousarray(rows, dtype=np.float64))
    ncell, nmonths = src.shape
    d_scale = ctx.upload(np.asarray(area, dtype=np.float64).reshape(-1) * 1e-6)
    d_km3 = ctx.empty((ncell, nmonths))
    d_out = ctx.empty((n_basins, nmonths))
    try:
        ctx.agg_time(ncell, nmonths, 1, 0, d_scale, src, d_km3)
        ids = np.asarray(basin_ids).reshape(-1).astype(np.int64)
        group = np.where((ids > 0) & (ids <= n_basins), ids - 1, -1).astype(np.int32)
        ctx.agg_spatial(ncell, nmonths, n_basins, group, d_km3, d_out)
        ctx.sync()
    except Exception:
        d_out.free()
        raise
    finally:
        for a in (d_scale, d_km3) + (() if src is rows else (src,)):      # a caller's array stays resident
            a.free()
    return d_out


def output_stem(settings, level, what=None):
    name = 'water_balance_{}_{}'.format(level, settings.OutputNameStr) if what is None else \
        'water_balance_{}_{}_{}'.format(level, what, settings.OutputNameStr)
    return os.path.join(settings.OutputFolder, name)


class WaterBalance:
    """The water balance of one level of ``[WaterBalance]``: ``results`` = {'table': ndarray [n, 21], 'annual': [n, 4, nyear],
    'xcorr': [n, max_lag + 1]}, n the cells or the basins.  ``precip``, ``pet``, ``q`` and ``aet`` (or None) are the run's
    [ncell, nmonths] arrays, host or DeviceArray; the basin level needs ``area`` (km2 per cell) and ``basin_ids`` (from 1)."""

    def __init__(self, settings, level, precip, pet, q, aet=None, area=None, basin_ids=None, write_files=True):
        cfg = settings.water_balance
        self.ctx = ctx = _hip.get_context(getattr(settings, 'device', 0))
        month0 = 12 * (cfg['start_year'] - settings.StartYear) + cfg['year_start_month'] - 1
        nyear = cfg['end_year'] - cfg['start_year'] + 1
        rows, formed = [precip, pet, q, aet], []
        table = annual = xcorr = None
        try:
            if level == 'basin':
                n_basins = int(np.max(np.asarray(basin_ids)))
                for i, a in enumerate(rows):
                    if a is not None:
                        rows[i] = basin_rows(ctx, a, area, basin_ids, n_basins)
                        formed.append(rows[i])
            table, annual, xcorr = balance_rows(ctx, rows[0], rows[1], rows[2], rows[3], month0, nyear, cfg['max_lag'], cfg['omega0'])
            logging.info('\twater balance per {}, {} - {}'.format(level, cfg['start_year'], cfg['end_year']))
            if write_files:
                os.makedirs(settings.OutputFolder, exist_ok=True)
                stem = output_stem(settings, level)
                ctx.save_npy(stem + '.npy', table)
                with open(stem + '.csv', 'w') as fh:
                    fh.write('id,' + ','.join(csv_columns(level)) + '\n')
                    offset = fh.tell()
                ctx.csv_write(stem + '.csv', table, 1, offset)
                ctx.save_npy(output_stem(settings, level, 'xcorr') + '.npy', xcorr)
                if cfg['annual']:
                    ctx.save_npy(output_stem(settings, level, 'annual') + '.npy', annual)
            self.results = {'table': table.download(), 'annual': annual.download(), 'xcorr': xcorr.download()}
        finally:
            for a in formed + [a for a in (table, annual, xcorr) if a is not None]:
                a.free()
