"""Actual hydropower (mirror of xanthos/hydropower/actual.py:20-217) on the GPU.

``HydropowerActual(settings, q_grids)`` keeps the reference's class surface: ``power_all_dams`` ``[nmonths, ndams]`` (MW,
downloaded on first read), ``grid_ids``, ``dr_ar_assumed``, ``env_flow`` and ``hydro_gcam_regions_EJ``.  The dam inputs
are read and prepared on the host exactly as the reference prepares them (nearest longitude and latitude by ``idxmin``,
the drainage area of the unique land-cell latitudes and longitudes, the CAPLIVE / HEAD fall-backs, NaN rule curves ->
1.1).  The inflow, the environmental flow and the monthly march of every dam run on the device (csrc/xh_hydro.hip); the
country and region tables are built on the host with the reference's pandas calls.  Where the reference crashes -- a NaN
in a dam's inflow, a month with no rule-curve row at or below s / cap, zero or several gridData rows for a dam, a country
table that does not match the dams' countries -- this module raises ValueError naming the dam or the table.
"""
import os

import numpy as np
import pandas as pd

from .. import _hip
from .potential import device_rows, year_plan

HYDRO_FILE = 'actual_hydro_by_gcam_region_EJperyr_{}.csv'


def _dam_name(res_data, d):
    return 'dam {} (LONG_DD {!r}, LAT_DD {!r})'.format(d, float(res_data.iloc[d, 0]), float(res_data.iloc[d, 1]))


def find_grid_ids(loc_refs, res_data, chunk=64):
    """get_grid_id (actual.py:93-97) for every dam: the nearest longitude and, separately, the nearest latitude, each
    by ``idxmin`` (the first row in gridData order on a tie), then the ID of the one row holding both."""
    lon_all = loc_refs['long'].values.astype(np.float64)
    lat_all = loc_refs['lati'].values.astype(np.float64)
    dam = res_data.iloc[:, 0:2]
    dlon, dlat = dam['LONG_DD'].values.astype(np.float64), dam['LAT_DD'].values.astype(np.float64)
    lon = np.empty(len(dlon))
    lat = np.empty(len(dlat))
    for a in range(0, len(dlon), chunk):
        b = min(a + chunk, len(dlon))
        lon[a:b] = lon_all[np.argmin(np.abs(lon_all[None, :] - dlon[a:b, None]), axis=1)]
        lat[a:b] = lat_all[np.argmin(np.abs(lat_all[None, :] - dlat[a:b, None]), axis=1)]
    rows = {}
    for i, key in enumerate(zip(lon_all.tolist(), lat_all.tolist())):
        rows.setdefault(key, []).append(i)
    ids = loc_refs['ID'].values
    out = np.empty(len(dlon), dtype=np.int64)
    for d, key in enumerate(zip(lon.tolist(), lat.tolist())):
        hit = rows.get(key, [])
        if len(hit) != 1:
            raise ValueError('{}: {} gridData rows have the nearest longitude {!r} and the nearest latitude {!r}; the '
                             'reference needs exactly one'.format(_dam_name(res_data, d), len(hit), key[0], key[1]))
        out[d] = int(ids[hit[0]])
    return out


def find_drain_areas(loc_refs, grid_ids, drainage_area):
    """get_drain_area (actual.py:99-103): the drainage grid indexed by the position of the dam cell's latitude among the
    unique land-cell latitudes (descending) and of its longitude among the unique longitudes (ascending)."""
    x = np.array(loc_refs)[grid_ids - 1, 1:3]
    lonseq = np.unique(loc_refs['long'])
    latseq = np.unique(loc_refs['lati'])[::-1]
    col = np.searchsorted(lonseq, x[:, 0])
    row = len(latseq) - 1 - np.searchsorted(latseq[::-1], x[:, 1])
    return drainage_area[row, col]


class HydropowerActual:
    """Country and GCAM-region hydropower production from the routed channel flow (see the reference class)."""

    secs_in_month = 2629800  # number of seconds in an average month
    cumecs_to_Mm3permonth = 2.6298  # m3/s to Mm3/month
    sww = 9810  # specific weight of water (N/m^3)
    hours_in_year = 8766  # number of hours in a year
    mwh_to_exajoule = 3.6 * (10 ** -9)  # megawatts to exajoules

    def __init__(self, settings, q_grids):
        """Load inputs, run the simulation on the device, build the region table and write it."""
        self.settings = settings
        self.ctx = _hip.get_context(getattr(settings, 'device', 0))
        self.res_data = pd.read_csv(settings.HydroDamData)
        self.grid_data = pd.read_csv(settings.GridData)
        self.drainage_area = np.loadtxt(settings.DrainArea)
        self.missing_cap = pd.read_csv(settings.MissingCap)
        self.rule_curves = np.load(settings.rule_curves)
        self.filename_hydro = os.path.join(settings.OutputFolder, HYDRO_FILE.format(settings.ProjectName))
        self.start_date = settings.hact_start_date
        self.loc_refs = self.grid_data[['ID', 'long', 'lati']]
        self.grid_ids = find_grid_ids(self.loc_refs, self.res_data)
        self.dr_ar_assumed = find_drain_areas(self.loc_refs, self.grid_ids, self.drainage_area)
        self.dr_ar_actual = np.array(self.res_data['CATCH'], dtype=np.float64)
        self._power = None
        self.hydro_gcam_regions_EJ = None
        self.hydro_sim(q_grids)
        self.to_region()
        self.write_output()

    def dam_parameters(self):
        """[5, ndams]: CAP, CAPLIVE (CAP where NaN), q_max = FLOW_M3S * 2.6298, EFF, HEAD (ECAP / (EFF * sww * (q_max /
        secs)) where NaN) -- sim_vars (actual.py:147-170) for every dam."""
        r = self.res_data
        cap = np.asarray(r['CAP'], dtype=np.float64)
        cap_live = np.asarray(r['CAPLIVE'], dtype=np.float64).copy()
        cap_live[np.isnan(cap_live)] = cap[np.isnan(cap_live)]
        q_max = np.asarray(r['FLOW_M3S'], dtype=np.float64) * self.cumecs_to_Mm3permonth
        eff = np.asarray(r['EFF'], dtype=np.float64)
        head = np.asarray(r['HEAD'], dtype=np.float64).copy()
        ecap = np.asarray(r['ECAP'], dtype=np.float64)
        fb = np.isnan(head)
        head[fb] = ecap[fb] / (eff[fb] * self.sww * (q_max[fb] / self.secs_in_month))
        return np.stack([cap, cap_live, q_max, eff, head])

    def hydro_sim(self, q_grids):
        """Inflow, environmental flow and the monthly march of every dam (actual.py:56-62, :109-189) on the device."""
        ctx = self.ctx
        src, mine = device_rows(ctx, q_grids)
        ncell, nmonths = src.shape
        ndams = len(self.res_data)
        cells = self.grid_ids - 1
        if ((cells < 0) | (cells >= ncell)).any():
            d = int(np.nonzero((cells < 0) | (cells >= ncell))[0][0])
            raise ValueError('{}: grid ID {} outside the {} cells of Avg_ChFlow'.format(_dam_name(self.res_data, d),
                                                                                       int(self.grid_ids[d]), ncell))
        rc = np.array(self.rule_curves, dtype=np.float64)
        if rc.shape != (5, 12, ndams):
            raise ValueError('rule curves have shape {}, expected (5, 12, {})'.format(rc.shape, ndams))
        rc[np.isnan(rc)] = 1.1                                                      # actual.py:136
        month0 = pd.Period(self.start_date, freq='M').month - 1
        year_idx, self.years = year_plan(self.start_date, nmonths)
        nyears = len(self.years)
        if nmonths < 12:
            raise ValueError('{} months of inflow: the environmental flow of every calendar month needs at least 12'.format(
                nmonths))
        bufs = [ctx.upload(cells, dtype=np.int64), ctx.upload(self.dr_ar_actual),
                ctx.upload(np.asarray(self.dr_ar_assumed, dtype=np.float64))]
        d_in, d_env, d_bad = ctx.empty((nmonths, ndams)), ctx.empty((ndams, 12)), ctx.empty((ndams,), dtype=np.int32)
        ctx.hact_inflow(ncell, nmonths, ndams, month0, bufs[0], bufs[1], bufs[2], self.cumecs_to_Mm3permonth, src, d_in,
                        d_env, d_bad)
        bad = d_bad.download()
        if mine:
            src.free()
        if bad.any():
            for b in bufs + [d_in, d_env, d_bad]:
                b.free()
            d = int(np.nonzero(bad)[0][0])
            raise ValueError('{}: its inflow (Avg_ChFlow of grid ID {}) holds NaN; the reference stops with an IndexError '
                             'there'.format(_dam_name(self.res_data, d), int(self.grid_ids[d])))
        d_year, d_rc, d_par = (ctx.upload(year_idx, dtype=np.int32), ctx.upload(rc),
                               ctx.upload(np.ascontiguousarray(self.dam_parameters())))
        d_power, d_annual = ctx.empty((nmonths, ndams)), ctx.empty((nyears, ndams))
        d_badm = ctx.empty((ndams,), dtype=np.int32)
        ctx.hact_sim(nmonths, ndams, nyears, month0, d_year, self.sww, self.secs_in_month, d_in, d_env, d_rc, d_par,
                     d_power, d_annual, d_badm)
        badm = d_badm.download()
        self.env_flow = d_env.download()
        self.annual_power = d_annual.download()                                    # [nyears, ndams], MW
        for b in bufs + [d_in, d_env, d_bad, d_year, d_rc, d_par, d_annual, d_badm]:
            b.free()
        if (badm >= 0).any():
            d_power.free()
            d = int(np.nonzero(badm >= 0)[0][0])
            raise ValueError('{}: in month {} of the run no rule-curve row is at or below the storage fraction s / cap; the '
                             'reference stops with an IndexError there'.format(_dam_name(self.res_data, d), int(badm[d])))
        self._d_power = d_power

    @property
    def power_all_dams(self):
        """[nmonths, ndams] power in MW (fetched from the device on first read)."""
        if self._power is None:
            self._power = self._d_power.download()
            self._d_power.free()
            self._d_power = None
        return self._power

    def to_region(self):
        """actual.py:198-206 on the device's annual means: EJ per dam and year, summed per country, scaled by the country
        factor, summed per GCAM region."""
        ncountry = len(pd.unique(self.res_data['COUNTRY'].dropna()))
        for col in ('factor', 'GCAM_ID'):
            if len(self.missing_cap[col]) != ncountry:
                raise ValueError('simulated_cap_by_country.csv has {} {} values for the {} countries of the dams; the '
                                 'reference matches them by position'.format(len(self.missing_cap[col]), col, ncountry))
        energy_all_dams = pd.DataFrame(self.annual_power, index=self.years) * (self.hours_in_year * self.mwh_to_exajoule)
        energy_all_countries = energy_all_dams.T.groupby(self.res_data['COUNTRY']).sum().T
        energy_all_countries_total = energy_all_countries.multiply(list(self.missing_cap['factor']))
        self.hydro_gcam_regions_EJ = energy_all_countries_total.T.groupby(list(self.missing_cap['GCAM_ID'])).sum().T

    def write_output(self):
        """actual.py:208-217."""
        odf = self.hydro_gcam_regions_EJ.T
        odf.reset_index(inplace=True)
        odf.rename(columns={'index': 'region'}, inplace=True)
        os.makedirs(os.path.dirname(self.filename_hydro), exist_ok=True)
        pd.DataFrame.to_csv(odf, self.filename_hydro, index=False)
