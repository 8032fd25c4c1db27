"""Flow duration curves and flow-regime signatures per grid cell on the GPU (no counterpart in the reference): what value of a
run's runoff, PET, AET, soil moisture, routed flow or precipitation is exceeded 95 % of the time, how variable (cv) and how
persistent (lag-1 autocorrelation, Richards-Baker flashiness) the monthly series is, the slope of the duration curve, in which
month the regime peaks and how seasonal it is (Walsh & Lawler 1981; Markham 1970), and how much the annual totals vary.

``signature_rows(ctx, rows, ...)`` runs ``xh_signatures`` (csrc/xh_signatures.hip; the definition stands in
csrc/xh_signatures_dev.h, include/xanthos_hip.h and DESIGN 4.23) on a ``[nrows, ncols]`` array, host or DeviceArray, and returns
the table ``[nrows, 18]`` of ``COLUMNS``, the duration curve ``[nrows, nP]`` and the calendar months' means ``[nrows, 12]``, all
in HBM.  ``Signatures(settings, var, rows)`` does what ``[Signatures]`` asks of one variable and writes
``signatures_<var>_<OutputNameStr>.npy`` and ``.csv`` (ids from 1, the text formatted in HBM),
``signatures_<var>_fdc_<OutputNameStr>.npy`` and ``.csv`` and ``signatures_<var>_regime_<OutputNameStr>.npy``, whatever the
OutputFormat: a NetCDF body would narrow them to binary32 under a time axis.
"""
import logging
import os

import numpy as np

from .. import _hip

COLUMNS = ('n', 'n_zero', 'mean', 'std', 'cv', 'median', 'lag1', 'flashiness', 'fdc_slope', 'regime_total', 'peak_month',
           'low_month', 'seasonality', 'centroid', 'concentration', 'n_years', 'annual_mean', 'annual_cv')
VARS = ('q', 'pet', 'aet', 'soilmoisture', 'avgchflow', 'precip')
EXCEEDANCE = (1, 5, 10, 20, 50, 80, 90, 95, 99)  # percent of the time the value is exceeded
MAX_EXCEEDANCE = 16
MAX_COLS = 4096                                  # months of one row's window in xh_signatures


def probabilities(exceedance=EXCEEDANCE):
    """The non-exceedance probabilities xh_signatures takes for the exceedance percents: (100 - p) / 100."""
    return np.array([(100.0 - float(p)) / 100.0 for p in exceedance], dtype=np.float64)


def exceedance_name(p):
    """The csv column of exceedance percent p: Q95, Q0.5."""
    return 'Q{:g}'.format(float(p))


def signature_rows(ctx, rows, start=0, nyear=None, cal0=0, exceedance=EXCEEDANCE):
    """(table, fdc, regime) of the monthly window ``rows[:, start : start + 12 nyear]`` (host array or DeviceArray [nrows, ncols];
    ``nyear`` None: the whole years to the end of the row), whose first column is calendar month ``cal0`` (0 = January):
    DeviceArrays [nrows, 18] = ``COLUMNS``, [nrows, nP] the values exceeded ``exceedance`` percent of the time (numpy's linear
    quantile at (100 - p) / 100) and [nrows, 12] the calendar months' means.  NaN and +-inf months are left out, so the rows
    need not be a run's grid: ``Components.gauge_flow`` or an observed gauge record with NaN gaps are host arrays this takes as
    they are, which sets a gauge's simulated and observed duration curve side by side.  Asynchronous for DeviceArrays; the
    caller frees the three."""
    mine = not isinstance(rows, _hip.DeviceArray)
    src = ctx.upload(np.ascontiguousarray(rows, dtype=np.float64)) if mine else rows
    out = []
    try:
        if len(src.shape) != 2:
            raise ValueError('the rows are {}, not [nrows, ncols]'.format(tuple(src.shape)))
        nrows, stride = src.shape
        nyear = (stride - int(start)) // 12 if nyear is None else int(nyear)
        p = probabilities(np.asarray(exceedance, dtype=np.float64).ravel())
        out = [ctx.empty((nrows, len(COLUMNS))), ctx.empty((nrows, p.size)), ctx.empty((nrows, 12))]
        ctx.signatures(nrows, stride, start, nyear, cal0, p, src, out[0], out[1], out[2])
    except Exception:
        for a in out:
            a.free()
        out = None
        raise
    finally:
        if mine:
            ctx.sync()                               # the call is asynchronous: its input goes only when it is done
            src.free()
    return tuple(out)


def output_stem(settings, var, what=None):
    name = 'signatures_{}_{}'.format(var, settings.OutputNameStr) if what is None else \
        'signatures_{}_{}_{}'.format(var, what, settings.OutputNameStr)
    return os.path.join(settings.OutputFolder, name)


class Signatures:
    """The signatures of one variable of ``[Signatures]``: ``results`` = {'table': ndarray [ncell, 18], 'fdc': [ncell, nP],
    'regime': [ncell, 12]}."""

    def __init__(self, settings, var, rows, write_files=True):
        cfg = settings.signatures
        self.ctx = ctx = _hip.get_context(getattr(settings, 'device', 0))
        month0 = 12 * (cfg['start_year'] - settings.StartYear) + cfg['year_start_month'] - 1
        nyear = cfg['end_year'] - cfg['start_year'] + 1
        table, fdc, regime = signature_rows(ctx, rows, month0, nyear, cfg['year_start_month'] - 1, cfg['exceedance'])
        try:
            logging.info('\tsignatures of {}, {} - {}'.format(var, cfg['start_year'], cfg['end_year']))
            if write_files:
                os.makedirs(settings.OutputFolder, exist_ok=True)
                for arr, what, names in ((table, None, COLUMNS), (fdc, 'fdc', tuple(exceedance_name(p) for p in cfg['exceedance']))):
                    stem = output_stem(settings, var, what)
                    ctx.save_npy(stem + '.npy', arr)
                    with open(stem + '.csv', 'w') as fh:
                        fh.write('id,' + ','.join(names) + '\n')
                        offset = fh.tell()
                    ctx.csv_write(stem + '.csv', arr, 1, offset)
                ctx.save_npy(output_stem(settings, var, 'regime') + '.npy', regime)
            self.results = {'table': table.download(), 'fdc': fdc.download(), 'regime': regime.download()}
        finally:
            for a in (table, fdc, regime):
                a.free()
