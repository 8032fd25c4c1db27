"""Hydropower potential (mirror of xanthos/hydropower/potential.py:19-86) on the GPU.

``HydropowerPotential(settings, q_grids)`` and ``constrain_q(q, ex)`` keep the reference's call surface.  ``q_grids`` is
Avg_ChFlow ``[ncell, nmonths]`` in m3/s, a host array or a DeviceArray (``Components.hydropower_potential`` hands over the
one the pipeline holds in HBM).  The per-cell percentile, the clip, the monthly energy, its calendar-year sums and the
region sums are HIP kernels (csrc/xh_hydro.hip); the host builds the two small ``[regions, years]`` tables and writes
them with pandas, as the reference does.  The reference's behaviour is kept as written: a NaN in any
month of a cell makes the whole cell NaN, so it contributes 0 in every year; region 0 stays in the technical file; the
exploitable file drops the smallest key of regID * inGrandELEC, whatever it is.
"""
import os
from types import SimpleNamespace

import numpy as np
import pandas as pd

from .. import _hip
from ..drought.drought_stats import quantile_plan

SWW = 9810                      # specific weight of water N/m^3 (potential.py:21)
AV_HOURS_IN_MONTH = 730.5       # hours in a month (average)
WATTHR_TO_TWH = 10 ** -12       # watt-hours to TWh
TWH_TO_EXAJOULE = 0.0036        # TWh to EJ

TECHPOT_FILE = 'tech_hydro_pot_by_gcam_region_EJperyr_{}.csv'
EXPL_FILE = 'tech_expliot_hyd_pot_by_gcam_region_EJperyr_{}.csv'      # (sic: the reference's file name)


def device_rows(ctx, arr):
    """[ncell, nmonths] DeviceArray from a host array or a DeviceArray (no copy in the second case); True if uploaded."""
    if isinstance(arr, _hip.DeviceArray):
        return arr, False
    return ctx.upload(np.ascontiguousarray(arr, dtype=np.float64)), True


def year_plan(start_date, nmonths):
    """Calendar years of ``pd.period_range(start_date, periods=nmonths, freq="M")``: (year index of each month int32,
    the annual PeriodIndex ``resample("A")`` labels its rows with)."""
    months = pd.period_range(start_date, periods=nmonths, freq='M')
    years = np.asarray(months.year)
    uniq, idx = np.unique(years, return_inverse=True)
    return idx.astype(np.int32), pd.PeriodIndex([pd.Period(int(y), freq='Y') for y in uniq])


def qmax_device(ctx, src, ex):
    """q_max per cell (DeviceArray [ncell]): np.percentile(row, ex * 100) over all months (potential.py:84)."""
    ncell, nmonths = src.shape
    k_prev, k_next, gamma = quantile_plan(nmonths, (ex * 100) / 100.0)   # np.percentile divides ex * 100 by 100 again
    out = ctx.empty((ncell,))
    ctx.hpot_qmax(ncell, nmonths, k_prev, k_next, gamma, src, out)
    return out


def constrain_q(q, ex, device=0):
    """np.clip(q, 0, np.percentile(q, ex * 100)) of one series ``[nmonths]`` or of every row of ``[ncell, nmonths]``
    (potential.py:75-86); the percentile on the device."""
    ctx = _hip.get_context(device)
    q = np.asarray(q, dtype=np.float64)
    rows = q.reshape(1, -1) if q.ndim == 1 else q
    src, mine = device_rows(ctx, rows)
    d_qmax = qmax_device(ctx, src, ex)
    qmax = d_qmax.download()
    d_qmax.free()
    if mine:
        src.free()
    return np.clip(rows, 0, qmax[:, None]).reshape(q.shape)


def _csr(keys):
    """Dense group index of each cell (sorted unique keys, as groupby sorts them) and a stable CSR of the groups' cells."""
    uniq, inv = np.unique(keys, return_inverse=True)
    order = np.argsort(inv, kind='stable').astype(np.int64)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=len(uniq)))]).astype(np.int64)
    return uniq, indptr, order


def potential_rows(ctx, q_grids, elev, keys, ex, ef, start_date):
    """Device part of HydropowerPotential.  ``keys``: list of group keys per cell (one array each).  Returns q_max [ncell],
    the annual energies E [ncell, nyears] (EJ) and, per key, (sorted unique keys, sums [ngroups, nyears])."""
    src, mine = device_rows(ctx, q_grids)
    ncell, nmonths = src.shape
    elev = np.ascontiguousarray(elev, dtype=np.float64)
    if elev.shape != (ncell,):
        raise ValueError('gridData has {} rows, Avg_ChFlow {} cells'.format(elev.shape[0], ncell))
    year_idx, years = year_plan(start_date, nmonths)
    nyears = len(years)
    d_qmax = qmax_device(ctx, src, ex)
    d_year, d_elev = ctx.upload(year_idx, dtype=np.int32), ctx.upload(elev)
    d_E = ctx.empty((ncell, nyears))
    # the constants as the reference's expressions make them: (ef * sww) first, then q, hours, TWh (potential.py:33)
    ctx.hpot_energy(ncell, nmonths, nyears, d_year, ef * SWW, AV_HOURS_IN_MONTH, WATTHR_TO_TWH, TWH_TO_EXAJOULE, src, d_qmax,
                    d_elev, d_E)
    groups = []
    for k in keys:
        uniq, indptr, cells = _csr(np.asarray(k))
        d_ptr, d_cells = ctx.upload(indptr, dtype=np.int64), ctx.upload(cells, dtype=np.int64)
        d_R = ctx.empty((len(uniq), nyears))
        ctx.hpot_region(len(uniq), nyears, d_ptr, d_cells, d_E, d_R)
        groups.append((uniq, d_R.download()))
        for b in (d_ptr, d_cells, d_R):
            b.free()
    res = SimpleNamespace(q_max=d_qmax.download(), E=d_E.download(), years=years, groups=groups)
    for b in (d_qmax, d_year, d_elev, d_E):
        b.free()
    if mine:
        src.free()
    return res


def region_tables(res, reg_name='regID'):
    """The reference's techpot / techpot_expl_ DataFrames (rows: years, columns: group keys) from ``potential_rows``."""
    (reg, r_sum), (expl, e_sum) = res.groups
    techpot = pd.DataFrame(r_sum.T, index=res.years, columns=pd.Index(reg, name=reg_name))
    techpot_expl = pd.DataFrame(e_sum.T, index=res.years, columns=pd.Index(expl))
    return techpot, techpot_expl.drop(techpot_expl.columns[0], axis=1)           # the smallest key goes (potential.py:62)


def write_tables(techpot, techpot_expl_, folder, project):
    """The two csv files as potential.py:51-71 writes them."""
    outdf_hyd = techpot.T
    outdf_hyd.reset_index(inplace=True)
    outdf_hyd.rename(columns={'regID': 'region'}, inplace=True)
    pd.DataFrame.to_csv(outdf_hyd, os.path.join(folder, TECHPOT_FILE.format(project)), index=False)
    outdf_expl = techpot_expl_.T
    outdf_expl.reset_index(inplace=True)
    outdf_expl.rename(columns={'index': 'region'}, inplace=True)
    pd.DataFrame.to_csv(outdf_expl, os.path.join(folder, EXPL_FILE.format(project)), index=False)


def HydropowerPotential(settings, q_grids):
    """Technical and exploitable hydropower potential per GCAM region in EJ/yr (potential.py:19-72): writes the two csv
    files into ``settings.OutputFolder`` and returns the results (q_max, E, techpot, techpot_expl)."""
    ctx = _hip.get_context(getattr(settings, 'device', 0))
    hyd_grid_data = pd.read_csv(settings.GridData)
    reg = hyd_grid_data['regID']
    res = potential_rows(ctx, q_grids, hyd_grid_data['elevD'].values, [reg.values, (reg * hyd_grid_data['inGrandELEC']).values],
                         settings.q_ex, settings.ef, settings.hpot_start_date)
    res.techpot, res.techpot_expl = region_tables(res)
    os.makedirs(settings.OutputFolder, exist_ok=True)
    write_tables(res.techpot, res.techpot_expl, settings.OutputFolder, settings.ProjectName)
    return res
