"""Time-series plots (mirror of xanthos/diagnostics/time_series.py:21-153) with the aggregation on the GPU.

``TimeSeriesPlot(settings, q, ac, ref)`` keeps the reference's call surface.  ``q`` and ``ac`` are the runoff and channel
flow as the writer wrote them (unit conversion applied, annual when OutputInYear = 1), host arrays or DeviceArrays.
``Aggregation_Map`` sums the cells of every basin / country / region per time step with ``xh_agg_spatial``, whose order
(ascending cells from 0.0, NaN skipped) is the reference's double loop.  The global row and the rendering stay on the
host; matplotlib is imported only here, only when plots are on, and draws on its Agg canvas (no pyplot, no
backend switch in the caller's process).  Quirks kept:
the table has ``max(id)`` rows, ids of 0 or less are left out, an id without cells gives a row of 0, and the names are
``['Global'] + names`` by position.  A MapID beyond the table, or a row without a name, is refused before anything is
drawn (the reference's bare ``except`` turns it into a second crash).
"""
import datetime
import logging
import os

import numpy as np

from .. import _hip
from ..hydropower.potential import device_rows
from ..ini_reader import ValidationException

SCALES = {1: ('Basin',), 2: ('Country',), 3: ('GCAMRegion',)}
ALL_SCALES = ('Basin', 'Country', 'GCAMRegion')
_REF_ATTR = {'Basin': 'basin', 'Country': 'country', 'GCAMRegion': 'region'}


def Aggregation_Map(Map, runoff, ctx=None):
    """[max(Map), ncols] sums of the cells with Map == k + 1 (time_series.py:142-153), on the device."""
    ctx = ctx or _hip.get_context(0)
    ids = np.asarray(Map).reshape(-1).astype(np.int64)
    src, mine = device_rows(ctx, runoff)
    ncell, ncols = src.shape
    try:
        if ids.shape != (ncell,):
            raise ValidationException('the id map holds {} cells, the data {}'.format(ids.shape[0], ncell))
        nb = int(ids.max()) if ncell else 0
        if nb < 1:
            raise ValidationException('the id map has no id above 0: the time-series table would have no rows')
        group = np.where(ids > 0, ids - 1, -1).astype(np.int32)
        d_out = ctx.empty((nb, ncols))
        ctx.agg_spatial(ncell, ncols, nb, group, src, d_out)
        table = d_out.download()
        d_out.free()
    finally:
        if mine:
            src.free()
    table[np.bincount(group[group >= 0], minlength=nb) == 0] = 0.0        # ids without cells: 0, not the kernel's NaN
    return table


def with_global(table):
    """The table with the reference's global row on top: np.sum(table, axis=0), row after row (time_series.py:94-95)."""
    return np.insert(table, 0, np.sum(table, axis=0), axis=0)


def plot_rows(map_id, nrows, nnames, scalestr):
    """Row indices the reference plots for MapID (time_series.py:97-124): every row for 999, one row for another
    integer, the listed rows for a list.  Refuses a row outside the table or without a name."""
    rows = list(map_id) if isinstance(map_id, (list, tuple)) else (list(range(nrows)) if map_id == 999 else [map_id])
    for i in rows:
        if not -nrows <= i < nrows:
            raise ValidationException('[TimeSeriesPlot] MapID {} is beyond the {} table of {} rows (row 0 is Global)'
                                      .format(i, scalestr, nrows))
        if not -nnames <= i < nnames:
            raise ValidationException('[TimeSeriesPlot] MapID {}: the {} table has {} rows but only {} names (with Global)'
                                      .format(i, scalestr, nrows, nnames))
    return rows


def time_axis(settings):
    """x values and limits of the plots (time_series.py:34-45)."""
    if settings.OutputInYear == 1:
        return 'year', {'data': np.array([datetime.datetime(i, 1, 1) for i in range(settings.StartYear, settings.EndYear + 1)]),
                        'xmin': datetime.datetime(settings.StartYear - 1, 1, 1),
                        'xmax': datetime.datetime(settings.EndYear + 1, 1, 1)}
    return 'month', {'data': np.array([datetime.datetime(i, j, 1) for i in range(settings.StartYear, settings.EndYear + 1)
                                       for j in range(1, 13)]),
                     'xmin': datetime.datetime(settings.StartYear - 1, 12, 1),
                     'xmax': datetime.datetime(settings.EndYear + 1, 1, 1)}


def Plot_TS(data, outputname, qstr, TimeUnit, LengthUnit, X):
    """One series to ``<outputname>_<qstr>.png`` at 300 dpi: yearly major ticks, monthly minor ticks for monthly data."""
    import matplotlib.dates as mdates
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure

    fig = Figure()
    FigureCanvasAgg(fig)
    ax = fig.add_subplot()
    ax.plot(X['data'], data)
    ax.xaxis.set_major_locator(mdates.YearLocator())
    ax.xaxis.set_major_formatter(mdates.DateFormatter('%Y'))
    if TimeUnit == 'month':
        ax.xaxis.set_minor_locator(mdates.MonthLocator())
    ax.set_xlim(X['xmin'], X['xmax'])
    ax.grid(True)
    ax.set_xlabel('Time (' + TimeUnit + ')', fontsize=12)
    ax.set_ylabel(qstr + ' ($' + LengthUnit + '$/' + TimeUnit + ')', fontsize=12)
    fig.autofmt_xdate()
    fig.savefig('{0}_{1}.png'.format(outputname, qstr), dpi=300)


def TimeSeriesPlot(settings, q, ac, ref):
    """Plots of the written runoff and channel flow per basin, country and/or region (time_series.py:21-69)."""
    if not settings.CreateTimeSeriesPlot:
        return {}
    ctx = _hip.get_context(getattr(settings, 'device', 0))
    time_unit, x = time_axis(settings)
    length_unit = 'km^3' if settings.OutputUnit == 1 else 'mm'
    d_q, q_mine = device_rows(ctx, q)
    d_ac, ac_mine = device_rows(ctx, ac)
    tables = {}
    try:
        for name, arr in (('q', d_q), ('ac', d_ac)):
            if arr.shape[1] != len(x['data']):
                raise ValidationException('the {} to plot has {} time steps, the time axis {} ({}ly)'.format(
                    name, arr.shape[1], len(x['data']), time_unit))
        for scalestr in SCALES.get(settings.TimeSeriesScale, ALL_SCALES):
            tables[scalestr] = scale_plots(settings, ctx, d_q, d_ac, ref, scalestr, time_unit, length_unit, x)
    finally:
        for arr, mine in ((d_q, q_mine), (d_ac, ac_mine)):
            if mine:
                arr.free()
    return tables


def scale_plots(settings, ctx, q, ac, ref, scalestr, time_unit, length_unit, x):
    """CreateData_TimeSeriesScale (time_series.py:72-139): both tables with their global rows, then the plots of the
    rows MapID selects.  Returns (q table, ac table, names)."""
    attr = _REF_ATTR[scalestr]
    id_map, names = getattr(ref, attr + '_ids'), getattr(ref, attr + '_names')
    qt = with_global(Aggregation_Map(id_map, q, ctx))
    act = with_global(Aggregation_Map(id_map, ac, ctx))
    Names = np.insert(np.asarray(names), 0, 'Global')
    rows = plot_rows(settings.TimeSeriesMapID, qt.shape[0], len(Names), scalestr)
    folder = os.path.join(settings.OutputFolder, 'TimeSeriesPlot', scalestr)
    os.makedirs(folder, exist_ok=True)
    for i in rows:
        outputname = os.path.join(folder, '{0}{1}_{2}'.format(scalestr, i, Names[i]))
        Plot_TS(qt[i, :], outputname, 'runoff', time_unit, length_unit, x)
        Plot_TS(act[i, :], outputname, 'streamflow', 'sec', 'm^3', x)
    logging.info('Scale: {}, created plots for {} rows'.format(scalestr, len(rows)))
    return qt, act, Names
