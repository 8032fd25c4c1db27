"""Standardized drought indices on the GPU (no counterpart in the reference, whose drought module is drought_stats.py): the
standardized runoff index SRI (Shukla & Wood 2008) of a run's runoff, its analogues SSI of soil moisture and SSFI of
routed streamflow, and the two indices of what drives the run -- SPI of its precipitation and SPEI of the climatic water
balance precipitation - PET (Vicente-Serrano et al. 2010), whose subtraction happens inside the kernel --, in the SPI
construction of McKee et al. (1993) at the accumulation scales of ``[DroughtIndex] scales``.

``StandardizedIndex(settings, rows)`` takes the ``[ncell, nmonths]`` array ``Components`` already holds (a DeviceArray after
a device-resident simulation, or a host array), forms every scale in one ``xh_std_index`` call (csrc/xh_sindex.hip; the
definitions stand in csrc/xh_sindex_dev.h and DESIGN 4.18) and writes each index through ``OutWriter.write_data`` -- ids from
1, the run's monthly column labels, so every OutputFormat and GriddedOutput work -- as
``drought_index_<var>_<k>m_<OutputNameStr>``.  With the gamma distribution and no ``parameters`` the fit of each scale is
written beside it as ``drought_index_<var>_<k>m_parameters_<OutputNameStr>.npy`` ([ncell, 12, 4]: q0, alpha, beta, n per
calendar month), with the log-logistic distribution as ``..._llparameters_...`` ([ncell, 12, 4]: alpha, beta,
gamma, n -- other columns, hence another name); with ``parameters`` those tables of an earlier run are used and nothing is
fitted (a future run indexed against the historic fit).  ``index`` is {k: ndarray} (or {k: DeviceArray} with ``keep_on_device``).
"""
import logging
import os

import numpy as np

from .. import _hip

INDEX_NAMES = {'q': 'SRI', 'soilmoisture': 'SSI', 'avgchflow': 'SSFI', 'precip': 'SPI', 'balance': 'SPEI'}
FITTED = ('gamma', 'loglogistic')          # the distributions with a parameter table


def output_stem(settings, var, k):
    return os.path.join(settings.OutputFolder, 'drought_index_{}_{}m_{}'.format(var, k, settings.OutputNameStr))


def parameter_file(settings, var, k):
    return os.path.join(settings.OutputFolder, 'drought_index_{}_{}m_parameters_{}.npy'.format(var, k, settings.OutputNameStr))


def ll_parameter_file(settings, var, k):
    """The table of a log-logistic fit: (alpha, beta, gamma, n), never to be read as a gamma table's (q0, alpha, beta, n)."""
    return os.path.join(settings.OutputFolder, 'drought_index_{}_{}m_llparameters_{}.npy'.format(var, k, settings.OutputNameStr))


def reference_window(settings):
    """(ref_month0, ref_nyear) of [DroughtIndex] reference_start_year / reference_end_year."""
    di = settings.drought_index
    return (di['reference_start_year'] - settings.StartYear) * 12, di['reference_end_year'] - di['reference_start_year'] + 1


def std_index_rows(ctx, rows, scales, ref_month0, ref_nyear, distribution='gamma', max_shape=1000.0, par_in=None,
                   want_parameters=False, minus=None):
    """The index of ``rows`` [ncell, nmonths] (host array or DeviceArray) -- of ``rows - minus`` with a subtrahend of the same
    shape, host or device -- at ``scales``: ({k: DeviceArray [ncell, nmonths]}, {k: DeviceArray [ncell, 12, 4]} or None).
    ``par_in``: {k: host table} used instead of fitting.  Asynchronous; the caller frees the arrays."""
    def on_device(a):
        return (a, False) if isinstance(a, _hip.DeviceArray) else (ctx.upload(np.ascontiguousarray(a, dtype=np.float64)), True)
    src, mine = on_device(rows)
    sub, sub_mine = on_device(minus) if minus is not None else (None, False)
    if sub is not None and tuple(sub.shape) != tuple(src.shape):
        raise ValueError('the subtrahend is {}, the rows are {}'.format(tuple(sub.shape), tuple(src.shape)))
    ncell, nmonths = src.shape
    index = [ctx.empty((ncell, nmonths)) for _ in scales]
    d_in = [ctx.upload(np.ascontiguousarray(par_in[k], dtype=np.float64)) for k in scales] if par_in is not None else None
    d_out = [ctx.empty((ncell, 12, 4)) for _ in scales] if want_parameters else None
    ctx.std_index(ncell, nmonths, scales, ref_month0, ref_nyear, distribution, max_shape, src, index, par_in=d_in, par_out=d_out,
                  minus=sub)
    if mine or sub_mine or d_in:
        ctx.sync()                                   # the call is asynchronous: its inputs go only when it is done
        for a in ([src] if mine else []) + ([sub] if sub_mine else []) + (d_in or []):
            a.free()
    return dict(zip(scales, index)), (dict(zip(scales, d_out)) if want_parameters else None)


class StandardizedIndex:
    def __init__(self, settings, rows, keep_on_device=False, write_files=True, grid=None, minus=None):
        from ..data_writer.out_writer import OutWriter
        di = settings.drought_index
        var, scales, dist = di['var'], list(di['scales']), di['distribution']
        self.ctx = _hip.get_context(getattr(settings, 'device', 0))
        ref0, nyr = reference_window(settings)
        par_in = None
        if di['parameters'] is not None:
            par_in = {k: np.load(di['parameters'][k]) for k in scales}
        fit = dist in FITTED and par_in is None
        table_file = ll_parameter_file if dist == 'loglogistic' else parameter_file
        logging.info('\t{} ({}) at {} months, {} distribution, reference {} - {}{}'.format(
            INDEX_NAMES[var], var, ', '.join(str(k) for k in scales), dist, di['reference_start_year'],
            di['reference_end_year'], '' if par_in is None else ', parameters of an earlier run'))
        index, pars = std_index_rows(self.ctx, rows, scales, ref0, nyr, dist, di['max_shape'], par_in, want_parameters=fit,
                                     minus=minus)
        self.parameters = None
        if write_files:
            os.makedirs(settings.OutputFolder, exist_ok=True)
            writer = OutWriter(settings, np.zeros(0), {}, grid=grid)
            for k in scales:
                writer.write_data(output_stem(settings, var, k), 'drought_index', index[k], writer.time_steps, first_id=1)
        if fit:
            self.parameters = {k: pars[k].download() for k in scales}
            for k in scales:
                if write_files:
                    np.save(table_file(settings, var, k), self.parameters[k])
                pars[k].free()
        if keep_on_device:
            self.index = index
        else:
            self.index = {k: index[k].download() for k in scales}
            for a in index.values():
                a.free()
