"""Trend per grid cell on the GPU (no counterpart in the reference): the Mann-Kendall test (Mann 1945, Kendall 1975; on a
monthly series the seasonal Kendall test of Hirsch & Slack 1984) and the Theil-Sen slope with its rank-based confidence
interval (Sen 1968) of a run's runoff, PET, AET, soil moisture, routed flow or precipitation: is it changing in this cell, by
how much per year, and is the change significant?

``trend_rows(ctx, rows, nseason, ...)`` runs ``xh_trend`` (csrc/xh_trend.hip; the definition stands in csrc/xh_trend_dev.h,
include/xanthos_hip.h and DESIGN 4.20) on a ``[nrows, ncols]`` array, host or DeviceArray, and returns the ``[nrows, 10]``
table ``COLUMNS`` in HBM.  ``Trend(settings, var, rows)`` does what ``[Trend]`` asks of one variable: ``annual`` aggregates
the months of each year in HBM (``xh_agg_time``: np.sum's order, a NaN month makes the year NaN -- or pandas' mean) and tests
the yearly series, ``seasonal`` tests the monthly series with its 12 calendar months as seasons; each table is written as
``trend_<var>_<series>_<OutputNameStr>.npy`` and ``.csv`` (ids from 1, the text formatted in HBM), whatever the OutputFormat:
a NetCDF body would narrow the p-values to binary32 under a time axis.
"""
import logging
import os
from statistics import NormalDist

import numpy as np

from .. import _hip

COLUMNS = ('n', 's', 'var_s', 'z', 'p', 'slope', 'intercept', 'slope_lo', 'slope_hi', 'npairs')
VARS = ('q', 'pet', 'aet', 'soilmoisture', 'avgchflow', 'precip')
SERIES = ('annual', 'seasonal')
ANNUAL_DEFAULT = {'q': 'sum', 'pet': 'sum', 'aet': 'sum', 'precip': 'sum', 'soilmoisture': 'mean', 'avgchflow': 'mean'}
MAX_COLS = 4096                                  # columns of one row in xh_trend's LDS
MIN_YEARS = 4


def z_of(confidence):
    """The normal quantile of (1 - confidence) / 2: xh_trend's z_conf, a negative number."""
    confidence = float(confidence)
    if not 0.5 < confidence < 1.0:
        raise ValueError('confidence = {} must lie in (0.5, 1)'.format(confidence))
    return NormalDist().inv_cdf((1.0 - confidence) / 2.0)


def trend_rows(ctx, rows, nseason=1, start=0, ncol=None, confidence=0.95):
    """The trend table of ``rows[:, start : start + ncol]`` (host array or DeviceArray [nrows, ncols]; ``ncol`` None: to the
    end of the row): a DeviceArray [nrows, 10] of ``COLUMNS``.  Column t of the window belongs to season ``t mod nseason``
    and stands ``t / nseason`` years after the window's start.  Asynchronous for a DeviceArray; the caller frees the table."""
    mine = not isinstance(rows, _hip.DeviceArray)
    src = ctx.upload(np.ascontiguousarray(rows, dtype=np.float64)) if mine else rows
    if len(src.shape) != 2:
        raise ValueError('the rows are {}, not [nrows, ncols]'.format(tuple(src.shape)))
    nrows, stride = src.shape
    ncol = stride - int(start) if ncol is None else int(ncol)
    out = ctx.empty((nrows, len(COLUMNS)))
    try:
        ctx.trend(nrows, stride, start, ncol, nseason, z_of(confidence), src, out)
    except Exception:
        out.free()
        raise
    finally:
        if mine:
            ctx.sync()                               # the call is asynchronous: its input goes only when it is done
            src.free()
    return out


def output_stem(settings, var, series):
    return os.path.join(settings.OutputFolder, 'trend_{}_{}_{}'.format(var, series, settings.OutputNameStr))


class Trend:
    """The tables of one variable of ``[Trend]``: ``tables`` = {series: ndarray [ncell, 10]}."""

    def __init__(self, settings, var, rows, write_files=True):
        cfg = settings.trend
        self.ctx = ctx = _hip.get_context(getattr(settings, 'device', 0))
        mine = not isinstance(rows, _hip.DeviceArray)
        src = ctx.upload(np.ascontiguousarray(rows, dtype=np.float64)) if mine else rows
        ncell, nmonths = src.shape
        year0 = cfg['start_year'] - settings.StartYear
        nyears = cfg['end_year'] - cfg['start_year'] + 1
        self.tables = {}
        if write_files:
            os.makedirs(settings.OutputFolder, exist_ok=True)
        for series in cfg['series']:
            if series == 'annual':
                yearly = ctx.empty((ncell, nmonths // 12))
                ctx.agg_time(ncell, nmonths, 12, 2 if cfg['annual'][var] == 'sum' else 1, None, src, yearly)
                table = trend_rows(ctx, yearly, 1, year0, nyears, cfg['confidence'])
            else:
                yearly = None
                table = trend_rows(ctx, src, 12, 12 * year0, 12 * nyears, cfg['confidence'])
            logging.info('\ttrend of {} ({}), {} - {}'.format(var, series, cfg['start_year'], cfg['end_year']))
            if write_files:
                stem = output_stem(settings, var, series)
                ctx.save_npy(stem + '.npy', table)
                with open(stem + '.csv', 'w') as fh:
                    fh.write('id,' + ','.join(COLUMNS) + '\n')
                    offset = fh.tell()
                ctx.csv_write(stem + '.csv', table, 1, offset)
            self.tables[series] = table.download()
            table.free()
            if yearly is not None:
                yearly.free()
        if mine:
            src.free()
