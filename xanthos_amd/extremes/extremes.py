"""Flood and low-flow return levels per grid cell on the GPU (no counterpart in the reference): the annual maxima or minima of
a run's runoff, PET, AET, soil moisture, routed flow or precipitation, the generalized extreme value distribution fitted to
them by Hosking's L-moments (Hosking 1990; Hosking & Wallis 1997; for minima the fit of the negated series, the
three-parameter Weibull distribution of low-flow analysis), the return levels of the periods asked for, and how rare each
year's extreme is under the fit -- or under the fit of another, historic run.

``extremes_rows(ctx, rows, kind, ...)`` runs ``xh_extremes`` (csrc/xh_extremes.hip; the definition stands in
csrc/xh_extremes_dev.h, include/xanthos_hip.h and DESIGN 4.21) on a ``[nrows, ncols]`` array, host or DeviceArray, and
returns the table ``[nrows, 8 + nT]`` of ``COLUMNS`` and the return levels, the annual series and every year's return period
``[nrows, nyear]``, all in HBM.  ``Extremes(settings, var, rows)`` does what ``[Extremes]`` asks of one variable and writes, per
kind, ``extremes_<var>_<kind>_<OutputNameStr>.npy`` and ``.csv`` (ids from 1, the text formatted in HBM),
``extremes_<var>_<kind>_annual_<OutputNameStr>.npy`` and ``extremes_<var>_<kind>_return_period_<OutputNameStr>.npy``,
whatever the OutputFormat: a NetCDF body would narrow them to binary32 under a time axis.

``bootstrap_rows(ctx, rows, kind, ...)`` runs ``xh_extremes_boot`` (csrc/xh_exboot.hip; csrc/xh_exboot_dev.h and DESIGN 4.22 hold
the definition): the percentile-bootstrap confidence intervals of the shape and the return levels, ``[nrows, 3 + 2 nT]`` of
``CI_COLUMNS`` and a lower and an upper bound per return period.  With ``bootstrap`` in ``[Extremes]``, ``Extremes`` adds
``results[kind]['ci']`` and writes ``extremes_<var>_<kind>_ci_<OutputNameStr>.npy`` and ``.csv``.
"""
import logging
import os

import numpy as np

from .. import _hip

COLUMNS = ('n', 'l1', 'l2', 't3', 't4', 'k', 'alpha', 'xi')
VARS = ('q', 'pet', 'aet', 'soilmoisture', 'avgchflow', 'precip')
KINDS = ('max', 'min')
RETURN_PERIODS = (2.0, 5.0, 10.0, 20.0, 50.0, 100.0)
MAX_PERIODS = 8
MAX_COLS = 4096                                  # months of one row's window in xh_extremes
MIN_YEARS = 5                                    # the least min_years
MIN_YEARS_DEFAULT = 10
CI_COLUMNS = ('nb', 'k_lo', 'k_hi')             # ... and x_T<T>_lo, x_T<T>_hi per return period
BOOTSTRAP_MIN, BOOTSTRAP_MAX = 100, 2048         # replicates [Extremes] accepts; xh_extremes_boot itself takes 2 .. 2048
CONFIDENCE_DEFAULT = 0.90


def period_name(T):
    """The csv column of return period T: x_T10, x_T2.5."""
    return 'x_T{:g}'.format(float(T))


def extremes_rows(ctx, rows, kind, start=0, nyear=None, return_periods=RETURN_PERIODS, min_years=MIN_YEARS_DEFAULT,
                  parameters=None):
    """(table, annual, T_year) of the monthly window ``rows[:, start : start + 12 nyear]`` (host array or DeviceArray [nrows,
    ncols]; ``nyear`` None: the whole years to the end of the row): DeviceArrays [nrows, 8 + nT] = ``COLUMNS`` and the return
    levels, [nrows, nyear] the annual ``kind`` ('max' or 'min') and [nrows, nyear] each year's return period.  ``parameters``
    (host array or DeviceArray [nrows, >= 8]): the table of another call, whose first 8 columns stand in for the fit.
    Asynchronous for DeviceArrays; the caller frees the three."""
    if kind not in KINDS:
        raise ValueError("kind = {!r} must be 'max' or 'min'".format(kind))
    mine = not isinstance(rows, _hip.DeviceArray)
    src = ctx.upload(np.ascontiguousarray(rows, dtype=np.float64)) if mine else rows
    made = [src] if mine else []
    out = []
    try:
        if len(src.shape) != 2:
            raise ValueError('the rows are {}, not [nrows, ncols]'.format(tuple(src.shape)))
        nrows, stride = src.shape
        nyear = (stride - int(start)) // 12 if nyear is None else int(nyear)
        T = np.asarray(return_periods, dtype=np.float64).ravel()
        par = None
        if parameters is not None:
            host = parameters.download() if isinstance(parameters, _hip.DeviceArray) else np.asarray(parameters, dtype=np.float64)
            if host.ndim != 2 or host.shape[0] != nrows or host.shape[1] < len(COLUMNS):
                raise ValueError('the parameters are {}, not [{}, >= {}]'.format(host.shape, nrows, len(COLUMNS)))
            par = ctx.upload(np.ascontiguousarray(host[:, :len(COLUMNS)]))
            made.append(par)
        out = [ctx.empty((nrows, len(COLUMNS) + T.size)), ctx.empty((nrows, max(nyear, 0))), ctx.empty((nrows, max(nyear, 0)))]
        ctx.extremes(nrows, stride, start, nyear, kind, min_years, T, src, out[0], out[1], out[2], par)
    except Exception:
        for a in out:
            a.free()
        out = None
        raise
    finally:
        if made:
            ctx.sync()                               # the call is asynchronous: its inputs go only when it is done
            for a in made:
                a.free()
    return tuple(out)


def bootstrap_rows(ctx, rows, kind, start=0, nyear=None, return_periods=RETURN_PERIODS, min_years=MIN_YEARS_DEFAULT, B=1000,
                   confidence=CONFIDENCE_DEFAULT, seed=1, row0=0, replicates=False):
    """The bootstrap intervals of the window of ``extremes_rows`` (host array or DeviceArray [nrows, ncols]): the DeviceArray
    [nrows, 3 + 2 nT] = ``CI_COLUMNS`` and x_T_lo, x_T_hi per return period, from ``B`` replicates per row drawn from ``seed``
    and the row's number ``row0 + r`` (rows a .. b of an array give, with ``row0 = a``, what they give inside the whole
    array).  ``replicates``: also the DeviceArray [nrows, B, 5 + nT] of every replicate's l1, l2, t3, t4, k and levels, returned
    as a pair (ci, rep).  Asynchronous for DeviceArrays; the caller frees what is returned."""
    if kind not in KINDS:
        raise ValueError("kind = {!r} must be 'max' or 'min'".format(kind))
    mine = not isinstance(rows, _hip.DeviceArray)
    src = ctx.upload(np.ascontiguousarray(rows, dtype=np.float64)) if mine else rows
    out = []
    try:
        if len(src.shape) != 2:
            raise ValueError('the rows are {}, not [nrows, ncols]'.format(tuple(src.shape)))
        nrows, stride = src.shape
        nyear = (stride - int(start)) // 12 if nyear is None else int(nyear)
        T = np.asarray(return_periods, dtype=np.float64).ravel()
        out = [ctx.empty((nrows, len(CI_COLUMNS) + 2 * T.size))]
        if replicates:
            out.append(ctx.empty((nrows, max(int(B), 0), 5 + T.size)))
        ctx.extremes_boot(nrows, stride, start, nyear, kind, min_years, T, B, confidence, seed, src, out[0],
                          out[1] if replicates else None, row0)
    except Exception:
        for a in out:
            a.free()
        raise
    finally:
        if mine:
            ctx.sync()                               # the call is asynchronous: its input goes only when it is done
            src.free()
    return tuple(out) if replicates else out[0]


def output_stem(settings, var, kind, what=None):
    name = 'extremes_{}_{}_{}'.format(var, kind, settings.OutputNameStr) if what is None else \
        'extremes_{}_{}_{}_{}'.format(var, kind, what, settings.OutputNameStr)
    return os.path.join(settings.OutputFolder, name)


def parameter_file(stem, var, kind):
    """The table of ``var`` and ``kind`` of the run whose ``<OutputFolder>/<OutputNameStr>`` is ``stem``."""
    folder, name = os.path.split(stem)
    return os.path.join(folder, 'extremes_{}_{}_{}.npy'.format(var, kind, name))


class Extremes:
    """The extremes of one variable of ``[Extremes]``: ``results`` = {kind: {'table': ndarray [ncell, 8 + nT], 'annual':
    [ncell, nyear], 'return_period': [ncell, nyear]}}, and with ``bootstrap`` in the section 'ci': [ncell, 3 + 2 nT]."""

    def __init__(self, settings, var, rows, write_files=True):
        cfg = settings.extremes
        boot = getattr(settings, 'extremes_bootstrap', None)
        self.ctx = ctx = _hip.get_context(getattr(settings, 'device', 0))
        mine = not isinstance(rows, _hip.DeviceArray)
        src = ctx.upload(np.ascontiguousarray(rows, dtype=np.float64)) if mine else rows
        month0 = 12 * (cfg['start_year'] - settings.StartYear) + cfg['year_start_month'] - 1
        nyear = cfg['end_year'] - cfg['start_year'] + 1
        self.results = {}
        if write_files:
            os.makedirs(settings.OutputFolder, exist_ok=True)
        try:
            for kind in cfg['kinds']:
                par = None
                if cfg['parameters'] is not None:
                    par = np.load(cfg['parameters'][(var, kind)])
                table, annual, t_year = extremes_rows(ctx, src, kind, month0, nyear, cfg['return_periods'], cfg['min_years'], par)
                logging.info('\textremes of {} ({}), {} - {}'.format(var, kind, cfg['start_year'], cfg['end_year']))
                if write_files:
                    stem = output_stem(settings, var, kind)
                    ctx.save_npy(stem + '.npy', table)
                    with open(stem + '.csv', 'w') as fh:
                        fh.write('id,' + ','.join(COLUMNS + tuple(period_name(T) for T in cfg['return_periods'])) + '\n')
                        offset = fh.tell()
                    ctx.csv_write(stem + '.csv', table, 1, offset)
                    ctx.save_npy(output_stem(settings, var, kind, 'annual') + '.npy', annual)
                    ctx.save_npy(output_stem(settings, var, kind, 'return_period') + '.npy', t_year)
                self.results[kind] = {'table': table.download(), 'annual': annual.download(), 'return_period': t_year.download()}
                for a in (table, annual, t_year):
                    a.free()
                if boot is not None:
                    ci = bootstrap_rows(ctx, src, kind, month0, nyear, cfg['return_periods'], cfg['min_years'], boot['B'],
                                        boot['confidence'], boot['seed'])
                    try:
                        if write_files:
                            stem = output_stem(settings, var, kind, 'ci')
                            ctx.save_npy(stem + '.npy', ci)
                            with open(stem + '.csv', 'w') as fh:
                                names = [period_name(T) + end for T in cfg['return_periods'] for end in ('_lo', '_hi')]
                                fh.write('id,' + ','.join(list(CI_COLUMNS) + names) + '\n')
                                offset = fh.tell()
                            ctx.csv_write(stem + '.csv', ci, 1, offset)
                        self.results[kind]['ci'] = ci.download()
                    finally:
                        ci.free()
        finally:
            if mine:
                src.free()
