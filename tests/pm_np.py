"""Penman-Monteith in extended precision: oracle/pm.py restated on np.longdouble (test infrastructure only).

Same formulas in the same order as oracle/pm.py (and through it xanthos/pet/penman_monteith.py); the inputs are the doubles
the kernel gets, widened; the constants are the doubles the reference writes (a Python float next to a long-double array is
widened from its double value, never re-read from its decimal text).  On x86-64 np.longdouble has a 64-bit mantissa, so
against the 1e-9 bar of the device comparison this is the truth: where the double reference itself loses digits (esx - vap
near saturation, exp(-lai / 2) differences at tiny lai) it is the reference that is off, not this.

Besides PET it records which way every decision went, per (class, cell, month), and how far the two decisions that are taken
on COMPUTED values -- vpd against VPDopen / VPDclose, gsum against 1e-4 -- are from their thresholds, relative to the
threshold.  Those two are the only places where a correct kernel may legitimately land on the other side of a
discontinuity; every other decision is either taken on an input (RH steps, tmin, T < -1, lai, month: exact on both sides) or
continuous where it switches (the caps and clamps).

The vegetated, water and snow formulas do not depend on which class the indices name, so one evaluation serves every
(water_idx, snow_idx): Truth.pet(water_idx, snow_idx) only selects.
"""
import numpy as np

from oracle.months import pm_days_in_month, pm_land_cover_index

LD = np.longdouble

LAMBDA1 = 2.46e6
CP = 1006
SIGMA = 4.9e-3
SIGMA2 = 5.67e-8
GAMMA = 0.67

VEG_BRANCHES = ('mtmin_open', 'mtmin_closed', 'mtmin_linear', 'vpd_low', 'vpd_high', 'vpd_mid', 'rh_clip',
                'fwet_0', 'fwet_8', 'fwet_10', 'fwet_12', 'fwet_16', 'gsum_lt_1e-4', 'lai_lt_1e-4', 'lai_le_1e-5',
                'lai_fwet_0', 'rs_1e5_seen', 'rs_gt_rslimit', 'rhc_gt_rslimit', 'rtot_gt_80', 'ra_gt_rtot', 'rhrc_gt_rtot', 'fc_gt_1',
                'fc_denom_0', 'fc_0', 'eet_lt_0')
WATER_BRANCHES = ('water_cold', 'water_warm', 'month_le_5', 'month_gt_5', 'rn_w_lt_0', 'ax_lt_0')
SNOW_BRANCHES = ('rn_s_lt_0',)
CELL_BRANCHES = ('totpct_0', 'leap_february', 'land_cover_switch')
ALL_BRANCHES = VEG_BRANCHES + WATER_BRANCHES + SNOW_BRANCHES + CELL_BRANCHES


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def _lc(v):
    return _ld(v)[:, None, None]


def _tab(t):
    return _ld(t)[:, None, :]


def _radiation(tair, rsds, rlds, alpha, emiss, dz):
    rnl = SIGMA * np.power(tair + 273, LD(4.0)) * emiss * dz - rlds * 86400 * dz
    rn = ((1 - alpha) * rsds) * 86400 * dz - rnl
    return rnl, rn


def _year(data, year, st, nlcs, land_cover_years, prev_slice):
    """One calendar year: (veg [L,C,12], water [C,12], snow [C,12], lct [L,C,1], totpct [C,1], branches, margins)."""
    ed = st + 12
    tair, tmin, rhs, wind, rsds, rlds, tairprev = (_ld(getattr(data, k)[:, st:ed]) for k in (
        'tair_load', 'TMIN_load', 'rhs_load', 'wind_load', 'rsds_load', 'rlds_load', 'tairprev_load'))
    elev = _ld(data.elev).reshape(-1, 1)
    shape = (nlcs,) + tair.shape
    B = {}
    full = lambda b: np.broadcast_to(b, shape)

    lc_i = pm_land_cover_index(year, land_cover_years)
    lct = _ld(data.lct_load[:, :, lc_i]).T[:, :, None]
    totpct = np.sum(lct, axis=0)
    B['totpct_0'] = np.broadcast_to(totpct == 0, tair.shape)
    totpct = np.where(totpct == 0, LD(0.01), totpct)

    dz_i = pm_days_in_month(year)
    dz = dz_i.astype(LD)
    B['leap_february'] = np.broadcast_to(dz_i == 29, tair.shape)
    B['land_cover_switch'] = np.full(tair.shape, prev_slice is not None and prev_slice != lc_i)
    alpha = _tab(data.alpha)

    esx = 6.10588 * np.exp(17.32491 * tair / (tair + 238.102))
    vap = esx * (rhs / 100)
    sx = 238.1 * 17.325 * esx / np.power(tair + 238.1, 2)
    rsnx = (1 - alpha) * rsds * 86400 * dz
    wind2 = wind * np.power(LD(2) / 10, LD(0.11))

    # ---------------- vegetated surfaces
    p = 101325 * np.power(1 - 0.0065 * elev / 288.15, LD(5.2558))
    rcorr = p / (101300 * np.power((273.15 + tair) / 293.15, LD(1.75)))
    gcu = 0.00001 * rcorr

    topen, tclose = _lc(data.Tminopen), _lc(data.Tminclose)
    B['mtmin_open'] = full((tmin >= topen) & ~(tmin <= tclose))
    B['mtmin_closed'] = full(tmin <= tclose)
    mid = (tmin < topen) & (tmin > tclose)
    B['mtmin_linear'] = full(mid)
    mtmin = np.zeros(shape, dtype=LD)
    mtmin = np.where(tmin >= topen, LD(1.0), mtmin)
    mtmin = np.where(tmin <= tclose, LD(0.1), mtmin)
    mtmin = np.where(mid, (tmin - tclose) / (topen - tclose), mtmin)

    vopen, vclose = _lc(data.VPDopen), _lc(data.VPDclose)
    vpd = esx - vap
    vmid = (vpd > vopen) & (vpd < vclose)
    B['vpd_low'] = full((vpd <= vopen) & ~(vpd >= vclose))
    B['vpd_high'] = full(vpd >= vclose)
    B['vpd_mid'] = full(vmid)
    margin_vpd = np.minimum(np.abs(vpd - vopen) / np.abs(vopen), np.abs(vpd - vclose) / np.abs(vclose))
    mvpd = np.broadcast_to(vpd, shape)
    mvpd = np.where(vpd <= vopen, LD(1.0), mvpd)
    mvpd = np.where(vpd >= vclose, LD(0.1), mvpd)
    mvpd = np.where(vmid, (vclose - vpd) / (vclose - vopen), mvpd)

    gs1 = _lc(data.cL) * mtmin * mvpd * rcorr

    B['rh_clip'] = full(rhs > 99.9999)
    rh = np.where(rhs > 99.9999, LD(99.9), rhs)

    rblmax, rblmin = _lc(data.RBLmax), _lc(data.RBLmin)
    rtotc = np.zeros(shape, dtype=LD)
    rtotc = np.where(vpd <= vopen, rblmax, rtotc)
    rtotc = np.where(vpd >= vclose, rblmin, rtotc)
    rtotc = np.where(vmid, rblmax - (rblmax - rblmin) * (vclose - vpd) / (vclose - vopen), rtotc)

    g = 1.6198 * (tair - tairprev)
    g[:, 0] = 0

    _, rn = _radiation(tair, rsds, rlds, alpha, _lc(data.emiss), dz)
    a = rn / (86400 * dz)

    lai, laimin, laimax = _tab(data.lai), _tab(data.laimin), _tab(data.laimax)
    fc_denom = np.exp(-0.5 * laimin) - np.exp(-0.5 * laimax)
    B['fc_denom_0'] = full(fc_denom == 0.0)
    fc_denom = np.where(fc_denom == 0.0, LD(1), fc_denom)
    fc = (np.exp(-0.5 * laimin) - np.exp(-0.5 * lai)) / fc_denom
    B['fc_gt_1'] = full(fc > 1)
    fc = np.where(fc > 1, LD(1), fc)
    B['fc_0'] = full(fc == 0)

    ac = fc * a
    asoil = (1 - fc) * a - g

    rtot = rtotc * rcorr
    B['rtot_gt_80'] = full(rtot > 80)
    rtot = np.where(rtot > 80, LD(80), rtot)
    rho = p / ((tair + 273.15) * 287.058)
    rr = rho * CP / (4.0 * SIGMA2 * np.power(tair + 273.15, 3))
    rcx = _lc(data.rc)
    ra = rcx * rr / (rcx + rr)
    B['ra_gt_rtot'] = full(ra > rtot)
    ra = np.where(ra > rtot, rtot, ra)

    r100 = rh / 100
    B['fwet_0'] = full(rh < 70)
    B['fwet_8'] = full((rh >= 70) & (rh < 80))
    B['fwet_10'] = full((rh >= 80) & (rh < 90))
    B['fwet_12'] = full((rh >= 90) & (rh < 95))
    B['fwet_16'] = full(rh >= 95)
    fwet = np.where(rh < 70, LD(0), rh)
    fwet = np.where(rh >= 70, np.power(r100, 8), fwet)
    fwet = np.where(rh >= 80, np.power(r100, 10), fwet)
    fwet = np.where(rh >= 90, np.power(r100, 12), fwet)
    fwet = np.where(rh >= 95, np.power(r100, 16), fwet)

    gsum = gs1 + 1 / rcx + gcu
    B['gsum_lt_1e-4'] = full(gsum < 0.0001)
    margin_gsum = np.abs(gsum - 0.0001) / 0.0001
    B['lai_lt_1e-4'] = full(lai < 0.0001)
    B['lai_le_1e-5'] = full(~(lai > 0.00001))
    cc = np.where(gsum < 0.0001, LD(10000),
                  np.where(fwet == 1, LD(0.00001), np.where(lai < 0.0001, LD(0.00001), LD(0))))
    with np.errstate(divide='ignore', invalid='ignore'):
        cc = np.where(cc == 0, 1 / rcx * (gs1 + gcu) * lai * (1 - fwet) / gsum, cc)
        rs = np.where(cc == 0, LD(100000), 1 / cc)
    rslimit = _lc(data.rslimit)
    B['rs_gt_rslimit'] = full(rs > rslimit)
    # rs = 1e5 from 1e-5 < lai < 1e-4 alone, below the cap, in a class with a canopy share: the only place where that test shows
    B['rs_1e5_seen'] = full((lai < 0.0001) & (lai > 0.00001) & ~(gsum < 0.0001) & ~(rs > rslimit) & (fc > 0) & (fwet < 1))
    rs = np.where(rs > rslimit, rslimit, rs)

    B['lai_fwet_0'] = full(lai * fwet == 0)
    lai_fwet = np.where(lai * fwet == 0, LD(1), lai * fwet)
    rhc = np.where(lai > 0.00001, rcx / lai_fwet, rslimit)
    B['rhc_gt_rslimit'] = full(rhc > rslimit)
    rhc = np.where(rhc > rslimit, rslimit, rhc)
    rvc = rhc
    rhrc = rhc * rr / (rhc + rr)
    B['rhrc_gt_rtot'] = full(rhrc > rtot)
    rhrc = np.where(rhrc > rtot, rtot, rhrc)

    apres = dz * 86400 * (sx * ac + rho * CP * vpd * fc / rhrc) * fwet / (
        (sx + p * 0.01 * CP * rvc / (LAMBDA1 * 0.622 * rhrc)) * LAMBDA1)
    ewet_c = np.where(rh >= 70, apres, LD(0.0))

    rasoil = rtot * rr / (rtot + rr)
    soil_num = 86400 * dz * (sx * asoil + rho * CP * (1 - fc) * vpd / rasoil)
    soil_den = (sx + GAMMA * rtot / rasoil) * LAMBDA1
    ewet_soil = soil_num * fwet / soil_den
    esoilpot = soil_num * (1 - fwet) / soil_den
    with np.errstate(divide='ignore'):
        esoil = ewet_soil + esoilpot * np.power(r100, vpd / _lc(data.beta))

    trans = dz * 86400 * (sx * ac + rho * CP * vpd * fc / ra) * (1 - fwet) / (
        (sx + GAMMA * (1 + rs / ra)) * LAMBDA1)
    trans = np.where(fc == 0, LD(0), trans)

    eet = trans + ewet_c + esoil
    B['eet_lt_0'] = full(eet < 0.0)
    veg = np.where(eet < 0.0, LD(0.0), eet)

    # ---------------- open water: albedo row 0, emissivity 0.98
    a0 = _ld(data.alpha)[0]
    rnl_w, rn_w = _radiation(tair, rsds, rlds, a0, 0.98, dz)
    B['rn_w_lt_0'] = rn_w < 0
    rn_w = np.where(rn_w < 0, LD(0.0), rn_w)
    mth = np.arange(12)
    B['month_le_5'] = np.broadcast_to(mth <= 5, tair.shape)
    B['month_gt_5'] = np.broadcast_to(mth > 5, tair.shape)
    qt = 0.5 * rsnx[0] - np.where(mth <= 5, 0.8, 1.3) * rnl_w
    ax = (rn_w - qt) / (86400 * dz)
    B['ax_lt_0'] = ax < 0
    ax = np.where(ax < 0, LD(0), ax)
    ewetx = rn_w / (86400 * dz) * dz * 0.6 / 2845
    ewety = dz * 86400 * (sx * ax + GAMMA * 6.43 * (0.5 + 0.54 * wind2) * (esx - vap)) / ((sx + GAMMA) * LAMBDA1)
    B['water_cold'] = tair < -1
    B['water_warm'] = ~(tair < -1)
    wat = np.where(tair < -1, ewetx, ewety)
    wat = np.where(wat < 0.0, LD(0.0), wat)

    # ---------------- snow / ice: albedo row 6, emissivity 0.85
    a6 = _ld(data.alpha)[6]
    _, rn_s = _radiation(tair, rsds, rlds, a6, 0.85, dz)
    B['rn_s_lt_0'] = rn_s < 0
    rn_s = np.where(rn_s < 0, LD(0.0), rn_s)
    snw = rn_s / (86400 * dz) * dz * 0.6 / 2845
    snw = np.where(snw < 0.0, LD(0.0), snw)

    margins = {'vpd': np.broadcast_to(margin_vpd, shape), 'gsum': np.broadcast_to(margin_gsum, shape)}
    return veg, wat, snw, lct, totpct, B, margins


class Truth:
    """Result of run(): per-class ET of every (cell, month), the land cover in force, the branch record and the margins."""

    def __init__(self, nlcs, veg, wat, snw, lct, totpct, branches, margins):
        self.nlcs, self.veg, self.wat, self.snw, self.lct, self.totpct = nlcs, veg, wat, snw, lct, totpct
        self.branches, self.margins = branches, margins
        self.active = lct > 0                                   # [L, C, nm]: the class the cell holds that month

    def pet(self, water_idx, snow_idx):
        """[ncell, nmonths] long double: the reference's assignment order, water first and snow last (:460-464)."""
        arr = self.veg.copy()
        arr[water_idx] = self.wat
        arr[snow_idx] = self.snw
        return np.sum(arr * self.lct, axis=0) / self.totpct

    def kinds(self, water_idx, snow_idx):
        """[L] of 'veg' / 'water' / 'snow' as the reference ends up treating each class."""
        k = np.array(['veg'] * self.nlcs, dtype=object)
        k[water_idx] = 'water'
        k[snow_idx] = 'snow'
        return k

    def taken(self, name, water_idx, snow_idx):
        """[L, C, nm] (class branches) or [C, nm] (cell branches): where branch ``name`` was taken by the class that the
        cell actually holds and that is of the kind the branch belongs to."""
        b = self.branches[name]
        if name in CELL_BRANCHES:
            return b
        kind = 'veg' if name in VEG_BRANCHES else ('water' if name in WATER_BRANCHES else 'snow')
        sel = (self.kinds(water_idx, snow_idx) == kind)[:, None, None]
        return np.broadcast_to(b, self.active.shape) & self.active & sel

    def counts(self, water_idx, snow_idx):
        return {name: int(self.taken(name, water_idx, snow_idx).sum()) for name in ALL_BRANCHES}

    def near_threshold(self, water_idx, snow_idx, rel=1e-9):
        """[C, nm]: a vegetated class the cell holds is within ``rel`` (relative) of a computed threshold."""
        veg = (self.kinds(water_idx, snow_idx) == 'veg')[:, None, None]
        near = (self.margins['vpd'] < rel) | (self.margins['gsum'] < rel)
        return np.any(near & self.active & veg, axis=0)


def run(data, nlcs, start_yr, end_yr, land_cover_years):
    """Evaluate every class of every (cell, month) of the run once; see Truth."""
    parts, prev = [], None
    for k, year in enumerate(range(start_yr, end_yr + 1)):
        parts.append(_year(data, year, 12 * k, nlcs, land_cover_years, prev))
        prev = pm_land_cover_index(year, land_cover_years)
    cat = lambda i, ax: np.concatenate([np.broadcast_to(p[i], p[i].shape[:-1] + (12,)) for p in parts], axis=ax)
    veg, wat, snw, lct, totpct = cat(0, 2), cat(1, 1), cat(2, 1), cat(3, 2), cat(4, 1)
    branches = {n: np.concatenate([p[5][n] for p in parts], axis=-1) for n in parts[0][5]}
    margins = {n: np.concatenate([p[6][n] for p in parts], axis=-1) for n in parts[0][6]}
    return Truth(nlcs, veg, wat, snw, lct, totpct, branches, margins)
