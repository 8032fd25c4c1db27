"""Deterministic synthetic 0.5-degree world and climate forcing.

The reference's input data (Zenodo archive; xanthos/install_supplement.py:19) is not available, so benchmarks
and tests run on a synthetic world with the same shapes and value ranges as the `pm_abcd_mrtm` example:
67,420 land cells on a 360 x 720 grid, 235 basins, 8 land classes.

Every random draw is a counter-based SplitMix64 hash of (seed, stream, index), so a world or a forcing block
can be regenerated identically anywhere, in any order and in pieces (per rank, per cell range) without
depending on a numpy Generator version.
"""
import heapq
from types import SimpleNamespace

import numpy as np

MASTER_SEED = 20240807
_U64 = np.uint64
_GOLD = _U64(0x9E3779B97F4A7C15)


def splitmix64(x):
    """SplitMix64 finaliser on a uint64 array (wrapping arithmetic)."""
    with np.errstate(over='ignore'):
        z = (np.asarray(x, dtype=_U64) + _GOLD)
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
        return z ^ (z >> _U64(31))


def uniform(seed, stream, idx):
    """U[0,1) doubles for integer indices ``idx`` on random stream ``stream``."""
    with np.errstate(over='ignore'):
        key = splitmix64(_U64(seed) * _U64(0xD1342543DE82EF95) + _U64(stream) * _U64(0xA0761D6478BD642F))
        h = splitmix64(np.asarray(idx, dtype=_U64) ^ key)
    return (h >> _U64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def normal(seed, stream, idx):
    """Standard normal (Box-Muller on two hashed uniforms)."""
    u1 = uniform(seed, 2 * stream, idx)
    u2 = uniform(seed, 2 * stream + 1, idx)
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)


# D8 code for a step (drow, dcol); "row + 1" is 'up' in the reference's decode (mrtm.py:236-240)
_D8 = {(0, 1): 1, (-1, 1): 2, (-1, 0): 4, (-1, -1): 8, (0, -1): 16, (1, -1): 32, (1, 0): 64, (1, 1): 128}


def make_world(nrow=360, ncol=720, ncell=67420, n_basins=235, nlcs=8, lc_years=(1970, 1990, 2005),
               seed=MASTER_SEED, row_margin=None, outlet_frac=0.03):
    """Grow ``n_basins`` tree-structured basins (Eden growth from outlet seeds) until ``ncell`` land cells exist.

    Returns a namespace with the arrays the reference's DataLoader would hold (data_load.py:35-224):
    coords [ncell,5] (id, lon, lat, ilon, ilat; 1-based indices), basin_ids [ncell] (1..n_basins),
    flow_dir [ncell] D8 codes (0 at outlets), area km2, flow_dist m, velocity m/s, elev [ncell,1],
    lct [ncell, nlcs, len(lc_years)], Penman-Monteith tables, ABCD parameters [n_basins,5].
    """
    if row_margin is None:
        row_margin = nrow // 12
    r_lo, r_hi = row_margin, nrow - row_margin
    usable = (r_hi - r_lo) * ncol
    if ncell > usable:
        raise ValueError('ncell does not fit the grid')

    # ---- basin seeds and growth weights (log-normal => heavy-tailed basin sizes)
    sidx = np.arange(n_basins)
    seed_r = r_lo + (uniform(seed, 1, sidx) * (r_hi - r_lo)).astype(int)
    seed_c = (uniform(seed, 2, sidx) * ncol).astype(int)
    weight = np.exp(0.45 * normal(seed, 3, sidx))

    owner = np.zeros((nrow, ncol), dtype=np.int32)          # basin id, 0 = ocean
    code = np.zeros((nrow, ncol), dtype=np.int32)           # D8 code towards the parent
    order = []                                              # growth order of (row, col)
    heap = []
    for b in range(n_basins):
        heapq.heappush(heap, (0.0, int(seed_r[b]), int(seed_c[b]), b + 1, 0))
    steps = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
    # pre-hashed exponential waiting times per (cell, direction)
    wait = -np.log(1.0 - uniform(seed, 4, np.arange(nrow * ncol * 8))).reshape(nrow, ncol, 8)
    while heap and len(order) < ncell:
        t, r, c, b, d8 = heapq.heappop(heap)
        if owner[r, c]:
            continue
        owner[r, c] = b
        code[r, c] = d8
        order.append((r, c))
        wb = weight[b - 1]
        for k, (dr, dc) in enumerate(steps):
            rr, cc = r + dr, c + dc
            if r_lo <= rr < r_hi and 0 <= cc < ncol and not owner[rr, cc]:
                # the child at (rr,cc) drains back to (r,c): step (-dr,-dc)
                heapq.heappush(heap, (t + wait[r, c, k] / wb, rr, cc, b, _D8[(-dr, -dc)]))
    if len(order) != ncell:
        raise RuntimeError('world growth stalled')

    # ---- flatten in column-major grid order like the reference's coordinate table (id increases with lon, then lat)
    rows = np.array([rc[0] for rc in order])
    cols = np.array([rc[1] for rc in order])
    perm = np.lexsort((rows, cols))
    rows, cols = rows[perm], cols[perm]
    ids = np.arange(1, ncell + 1)
    lat = -90.0 + (rows + 0.5) * (180.0 / nrow)
    lon = -180.0 + (cols + 0.5) * (360.0 / ncol)
    coords = np.stack([ids, lon, lat, cols + 1, rows + 1], axis=1).astype(float)
    basin_ids = owner[rows, cols].astype(int)
    flow_dir = code[rows, cols].astype(float)

    cidx = np.arange(ncell)
    # a few percent of cells are extra sea outlets => many small river networks inside each basin
    flow_dir[uniform(seed, 5, cidx) < outlet_frac] = 0.0

    w = SimpleNamespace()
    w.nrow, w.ncol, w.ncell, w.n_basins, w.nlcs = nrow, ncol, ncell, n_basins, nlcs
    w.lc_years = list(lc_years)
    w.coords, w.basin_ids, w.flow_dir = coords, basin_ids, flow_dir
    w.area = 3091.0 * np.cos(np.radians(lat))                                  # km2 (data_load.py:48 gives km2)
    w.flow_dist = 25e3 + 50e3 * uniform(seed, 6, cidx)
    w.flow_dist[uniform(seed, 7, cidx) < 0.01] = 1000.0                        # clamped short reaches (data_load.py:204)
    w.velocity = 0.1 + 2.4 * uniform(seed, 8, cidx)
    w.velocity[uniform(seed, 9, cidx) < 0.005] = 0.0                           # data_load.py:207
    w.elev = (3000.0 * uniform(seed, 10, cidx))[:, None]
    w.latitude = lat

    nly = len(lc_years)
    e = -np.log(1.0 - uniform(seed, 11, np.arange(ncell * nlcs * nly))).reshape(ncell, nlcs, nly)
    lct = 100.0 * e / e.sum(axis=1, keepdims=True)
    lct[uniform(seed, 12, cidx) < 0.01] = 0.0                                  # cells with no land cover at all
    w.lct = lct

    li = np.arange(nlcs)
    ti = np.arange(nlcs * 12)
    u = lambda s, i=li: uniform(seed, s, i)
    w.cL = 0.0013 + 0.0052 * u(20)
    w.beta = 100.0 + 400.0 * u(21)
    w.rslimit = 500.0 + 1500.0 * u(22)
    w.ae = 0.34 + 0.1 * u(23)
    w.be = -0.14 - 0.11 * u(24)
    w.Tminopen = 8.0 + 4.0 * u(25)
    w.Tminclose = -8.0 + 2.0 * u(26)
    w.VPDclose = 25.0 + 18.0 * u(27)
    w.VPDopen = 6.5 + 3.5 * u(28)
    w.RBLmin = 20.0 + 45.0 * u(29)
    w.RBLmax = w.RBLmin + 25.0 + 10.0 * u(30)
    w.rc = 20.0 + 100.0 * u(31)
    w.emiss = 0.94 + 0.05 * u(32)
    w.alpha = (0.05 + 0.35 * u(33, ti)).reshape(nlcs, 12)
    w.lai = (6.0 * u(34, ti)).reshape(nlcs, 12)
    w.lai[min(3, nlcs - 1)] = 0.0                                               # a bare class: lai = laimin = laimax = 0
    w.laimin = np.repeat(w.lai.min(axis=1, keepdims=True), 12, axis=1)
    w.laimax = np.repeat(w.lai.max(axis=1, keepdims=True), 12, axis=1)

    bi = np.arange(n_basins)
    w.abcd_pars = np.stack([0.9 + 0.099 * uniform(seed, 40, bi), 0.1 + 1.9 * uniform(seed, 41, bi),
                            0.01 + 0.89 * uniform(seed, 42, bi), 0.01 + 0.89 * uniform(seed, 43, bi),
                            0.1 + 0.8 * uniform(seed, 44, bi)], axis=1)
    w.seed = seed
    return w


FORCING_NAMES = ('tas', 'tmin', 'rhs', 'wind', 'rsds', 'rlds', 'precip', 'abcd_tmin')


def make_forcing(world, nmonths, seed=None, cells=None, chunk=None, nan_precip=True):
    """Monthly climate forcing [ncell(or len(cells)), nmonths] float64 (SURVEY.md section 8(d) distributions).

    ``cells``: optional array of 0-based global cell indices to generate (rank shards, samples) -- values are
    identical to the same rows of the full array.
    """
    seed = world.seed + 1 if seed is None else seed
    if chunk is None:
        chunk = max(1, 32768 // nmonths)      # keep temporaries small enough to stay in the malloc heap
    sel = np.arange(world.ncell) if cells is None else np.asarray(cells)
    n = len(sel)
    out = {k: np.empty((n, nmonths)) for k in FORCING_NAMES}
    mth = np.arange(nmonths)
    season = np.sin(2.0 * np.pi * ((mth % 12) - 3.5) / 12.0)
    for s in range(0, n, chunk):
        c = sel[s:s + chunk]
        idx = (c[:, None].astype(np.int64) * 4096 + mth[None, :]).astype(np.uint64)   # < 4096 months supported
        coslat = np.cos(np.radians(world.latitude[c]))[:, None]
        hemi = np.sign(world.latitude[c])[:, None]
        tas = -10.0 + 35.0 * coslat ** 2 + 10.0 * hemi * season[None, :] + 2.0 * normal(seed, 1, idx)
        tmin = tas - (2.0 + 8.0 * uniform(seed, 4, idx))
        rhs = np.clip(65.0 + 20.0 * normal(seed, 3, idx), 5.0, 100.0)
        out['tas'][s:s + chunk] = tas
        out['tmin'][s:s + chunk] = tmin
        out['rhs'][s:s + chunk] = rhs
        out['wind'][s:s + chunk] = 0.5 + 7.5 * uniform(seed, 10, idx)
        out['rsds'][s:s + chunk] = 30.0 + 300.0 * uniform(seed, 11, idx)
        out['rlds'][s:s + chunk] = 150.0 + 280.0 * uniform(seed, 12, idx)
        pr = -40.0 * (np.log(1.0 - uniform(seed, 13, idx)) + np.log(1.0 - uniform(seed, 14, idx)))
        if nan_precip:
            pr[uniform(seed, 15, c) < 0.001] = np.nan                                # missing-data cells (kept NaN)
        out['precip'][s:s + chunk] = pr
        out['abcd_tmin'][s:s + chunk] = tmin
    return out


def data_bag(world, forcing):
    """Attribute bag with the field names run_pmpet reads from the reference DataLoader (data_load.py:92-135)."""
    d = SimpleNamespace()
    for k in ('cL', 'beta', 'rslimit', 'ae', 'be', 'Tminopen', 'Tminclose', 'VPDclose', 'VPDopen', 'RBLmin',
              'RBLmax', 'rc', 'emiss', 'alpha', 'lai', 'laimax', 'laimin', 'elev'):
        setattr(d, k, getattr(world, k))
    d.tair_load = forcing['tas']
    d.TMIN_load = forcing['tmin']
    d.rhs_load = forcing['rhs']
    d.wind_load = forcing['wind']
    d.rsds_load = forcing['rsds']
    d.rlds_load = forcing['rlds']
    d.tairprev_load = np.zeros_like(d.tair_load)
    d.tairprev_load[1:, :] = d.tair_load[:-1, :]             # the reference's cell-shift (data_load.py:128-129)
    d.lct_load = world.lct
    return d


def write_example(root, world, forcing, start_year, end_year, project='pm_abcd_mrtm_synth', runoff_spinup=36,
                  routing_spinup=None, output_vars=('q', 'avgchflow'), obs=None, post=False, aggregates=False,
                  hist_flag=True, ch_storage=None, output_format=1, output_in_year=0, set_calibrate=0,
                  calibration_basins='1-2', gauges=None, gauge_obs=None, gauge_missing=None, calibrate_velocity=0,
                  velocity_scale_bounds=None, velocity_scale=None, gridded=False, drought_index=None):
    """Write ``world`` + ``forcing`` as a Xanthos-style input tree under ``root`` and return the .ini path.

    Layout and file names follow the reference's example (ini_reader.py:254-279, 353-381, 399-416, 425-437):
    input/reference/{Grid_Areas_ID.csv, coordinates.csv, basin.csv}, input/pet/penman_monteith/*.npy + gcam_*.csv,
    input/runoff/abcd/{pars.npy, pr.npy, tmin.npy}, input/routing/mrtm/{velocity.npy, flow_dist.npy, flow_dir.npy}.
    ``post=True`` also switches on the drought-threshold and accessible-water post-processors (basin names, reservoir
    capacity and base-flow index tables under input/reference and input/accessible; ini_reader.py:460-486).
    ``aggregates=True`` writes GCAM-region and country maps with their name tables (7 regions / 10 countries, the last
    name of each without cells; countries numbered from 0) and switches the three runoff aggregations on.
    ``hist_flag=False`` + ``ch_storage`` (array [ncell]): future mode starting from a saved channel storage file
    (ini_reader.py HistFlag / ChStorageFile, data_load.py:427-438).
    ``obs`` (rows [basin, 0, 0, value]) switches calibration on: ``set_calibrate = 0`` against runoff in km3_per_mth,
    ``set_calibrate = 1`` against the basins' outlet streamflow in m3_per_sec (the values then made by the caller, e.g.
    from known parameters), for ``calibration_basins``.
    ``gauges`` (rows [gauge_id, cell_id (1-based)[, weight]]) + ``gauge_obs`` (rows [gauge_id, 0, 0, value], NaN =
    missing; ``gauge_missing``: a sentinel written to the ini) switch on ``set_calibrate = 1`` at stream gauges; ``obs``
    is then optional.
    ``calibrate_velocity`` = 1 (with ``set_calibrate = 1`` or gauges) and ``velocity_scale_bounds`` = (lo, hi) go to
    [Calibrate] as given; ``velocity_scale`` (rows [basin_id, scale], or a dict) is written as routing/mrtm/
    velocity_scale.csv and named in [[mrtm]].
    ``gridded=True`` adds ``GriddedOutput = 1`` to [Project]: every per-cell output also as a CF NetCDF map.
    ``drought_index`` (a dict of ``enable_drought_index``'s arguments, {} for its defaults) appends
    ``CalculateDroughtIndex = 1`` and a [DroughtIndex] section.
    """
    import os
    inp = os.path.join(root, 'input')
    dirs = {k: os.path.join(inp, *v) for k, v in dict(ref=('reference',), pet=('pet', 'penman_monteith'),
                                                      ro=('runoff', 'abcd'), rt=('routing', 'mrtm')).items()}
    for d in dirs.values():
        os.makedirs(d, exist_ok=True)
    np.savetxt(os.path.join(dirs['ref'], 'Grid_Areas_ID.csv'), world.area * 100.0, delimiter=',', fmt='%.17g')   # ha
    np.savetxt(os.path.join(dirs['ref'], 'coordinates.csv'), world.coords, delimiter=',', fmt='%.17g')
    np.savetxt(os.path.join(dirs['ref'], 'basin.csv'), np.concatenate([[0], world.basin_ids]), fmt='%d')   # 1 header row
    et = np.stack([world.cL, world.beta, world.rslimit, world.ae, world.be, world.Tminopen, world.Tminclose,
                   world.VPDclose, world.VPDopen, world.RBLmin, world.RBLmax, world.rc, world.emiss], axis=1)
    np.savetxt(os.path.join(dirs['pet'], 'gcam_ET_para.csv'), et, delimiter=',', fmt='%.17g')
    for name, arr in (('gcam_albedo', world.alpha), ('gcam_lai', world.lai), ('gcam_laimin', world.laimin),
                      ('gcam_laimax', world.laimax)):
        np.savetxt(os.path.join(dirs['pet'], name + '.csv'), arr, delimiter=',', fmt='%.17g')
    np.save(os.path.join(dirs['pet'], 'elev.npy'), world.elev)
    np.save(os.path.join(dirs['pet'], 'lct.npy'), world.lct)
    for key in ('tas', 'tmin', 'rhs', 'wind', 'rsds', 'rlds'):
        np.save(os.path.join(dirs['pet'], key + '.npy'), forcing[key])
    np.save(os.path.join(dirs['ro'], 'pars.npy'), world.abcd_pars)
    np.save(os.path.join(dirs['ro'], 'pr.npy'), forcing['precip'])
    np.save(os.path.join(dirs['ro'], 'tmin.npy'), forcing['abcd_tmin'])
    np.save(os.path.join(dirs['rt'], 'velocity.npy'), world.velocity)
    np.save(os.path.join(dirs['rt'], 'flow_dist.npy'), world.flow_dist)
    np.save(os.path.join(dirs['rt'], 'flow_dir.npy'), world.flow_dir)
    nmonths = (end_year - start_year + 1) * 12
    ini = os.path.join(root, project + '.ini')
    calib = ''
    if gauges is not None:
        lines = 'set_calibrate = 1\n'
        if obs is not None:
            np.savetxt(os.path.join(inp, 'obs.csv'), obs, delimiter=',', fmt='%.17g')
            lines += 'observed = {}\n'.format(os.path.join(inp, 'obs.csv'))
        np.savetxt(os.path.join(inp, 'gauges.csv'), np.atleast_2d(gauges), delimiter=',', fmt='%.17g')
        np.savetxt(os.path.join(inp, 'gauge_obs.csv'), gauge_obs, delimiter=',', fmt='%.17g')
        lines += 'gauges = {}\ngauge_observed = {}\n'.format(os.path.join(inp, 'gauges.csv'),
                                                           os.path.join(inp, 'gauge_obs.csv'))
        if gauge_missing is not None:
            lines += 'gauge_missing = {!r}\n'.format(float(gauge_missing))
        calib = '\n[Calibrate]\n{}obs_unit = m3_per_sec\ncalib_out_dir = {}\ncalibration_basins = {}\n'.format(
            lines, os.path.join(root, 'calib_out'), calibration_basins)
    elif obs is not None:
        obs_file = os.path.join(inp, 'obs.csv')
        np.savetxt(obs_file, obs, delimiter=',', fmt='%.17g')
        calib = ('\n[Calibrate]\nset_calibrate = {}\nobserved = {}\nobs_unit = {}\ncalib_out_dir = {}\n'
                 'calibration_basins = {}\n').format(int(set_calibrate), obs_file,
                                                     'm3_per_sec' if set_calibrate else 'km3_per_mth',
                                                     os.path.join(root, 'calib_out'), calibration_basins)
    if calib and calibrate_velocity:
        calib += 'calibrate_velocity = {}\n'.format(int(calibrate_velocity))
    if calib and velocity_scale_bounds is not None:
        calib += 'velocity_scale_bounds = {!r}, {!r}\n'.format(*[float(x) for x in velocity_scale_bounds])
    vs_line = ''
    if velocity_scale is not None:
        rows = sorted(velocity_scale.items()) if isinstance(velocity_scale, dict) else np.atleast_2d(velocity_scale)
        with open(os.path.join(dirs['rt'], 'velocity_scale.csv'), 'w') as fh:
            fh.write('basin_id,scale\n' + ''.join('{},{!r}\n'.format(int(b), float(v)) for b, v in rows))
        vs_line = 'velocity_scale = velocity_scale.csv\n'
    post_project = post_sections = ''
    if post:
        acc = os.path.join(inp, 'accessible')
        os.makedirs(acc, exist_ok=True)
        nb = world.n_basins
        with open(os.path.join(dirs['ref'], 'BasinNames235.txt'), 'w') as fh:
            fh.write('\n'.join('Basin {:03d}'.format(k) for k in range(1, nb + 1)) + '\n')
        cap = uniform(splitmix64(np.arange(nb, dtype=np.uint64) + np.uint64(77001)), 0.0, 5.0)
        bfi = uniform(splitmix64(np.arange(nb, dtype=np.uint64) + np.uint64(77002)), 0.2, 0.9)
        np.savetxt(os.path.join(acc, 'total_reservoir_storage.csv'), cap, fmt='%.17g')
        with open(os.path.join(acc, 'bfi_per_basin.csv'), 'w') as fh:
            fh.write('basin_id,bfi_avg\n' + ''.join('{},{!r}\n'.format(k + 1, float(bfi[k])) for k in range(nb)))
        post_project = 'AccWatDir = accessible\nCalculateDroughtStats = 1\nCalculateAccessibleWater = 1\n'
        post_sections = ('\n[Drought]\ndrought_var = q\nthreshold_nper = 12\nthreshold_start_year = {y0}\n'
                         'threshold_end_year = {y1}\n\n[AccessibleWater]\nResCapacityFile = total_reservoir_storage.csv\n'
                         'BfiFile = bfi_per_basin.csv\nHistEndYear = {y1}\nGCAM_StartYear = {y0}\nGCAM_EndYear = {y1}\n'
                         'GCAM_YearStep = 1\nMovingMeanWindow = 3\nEnv_FlowPercent = 0.1\n').format(y0=start_year, y1=end_year)
    if aggregates:
        names = os.path.join(dirs['ref'], 'BasinNames235.txt')
        if not os.path.isfile(names):
            with open(names, 'w') as fh:
                fh.write('\n'.join('Basin {:03d}'.format(k) for k in range(1, world.n_basins + 1)) + '\n')
        np.savetxt(os.path.join(dirs['ref'], 'region32_grids.csv'), np.concatenate([[0], world.basin_ids % 6 + 1]), fmt='%d')
        with open(os.path.join(dirs['ref'], 'Rgn32Names.csv'), 'w') as fh:
            fh.write('region,region_id\n' + '\n'.join('Region {},{}'.format(k, k) for k in range(1, 8)))
        np.savetxt(os.path.join(dirs['ref'], 'country.csv'), np.concatenate([[0], world.basin_ids % 9]), fmt='%d')
        with open(os.path.join(dirs['ref'], 'country-names.csv'), 'w') as fh:
            fh.write(''.join('{},Country {}\n'.format(k, k) for k in range(10)))
        post_project += 'AggregateRunoffBasin = 1\nAggregateRunoffCountry = 1\nAggregateRunoffGCAMRegion = 1\n'
    chs_lines = ''
    if not hist_flag:
        np.save(os.path.join(dirs['rt'], 'ch_storage.npy'), np.asarray(ch_storage, dtype=float))
        chs_lines = 'ChStorageFile = {}\nChStorageVarName = chs\n'.format(os.path.join(dirs['rt'], 'ch_storage.npy'))
    with open(ini, 'w') as fh:
        fh.write('''[Project]
# synthetic pm_abcd_mrtm example written by xanthos_amd.synth.write_example
ProjectName = {project}
RootDir = {root}
InputFolder = input
OutputFolder = output
RefDir = reference
pet_dir = pet
RunoffDir = runoff
RoutingDir = routing
HistFlag = {hist}
n_basins = {nb}
ncell = {ncell}
ngridrow = {nrow}
ngridcol = {ncol}
StartYear = {y0}
EndYear = {y1}
output_vars = {ov}
OutputFormat = {ofmt}
OutputUnit = 0
OutputInYear = {oyear}{grid}
Calibrate = {cal}
{post_project}
[PET]
pet_module = pm
[[penman-monteith]]
pet_dir = penman_monteith
pm_tas = tas.npy
pm_tmin = tmin.npy
pm_rhs = rhs.npy
pm_rlds = rlds.npy
pm_rsds = rsds.npy
pm_wind = wind.npy
pm_lct = lct.npy
pm_nlcs = {nlcs}
pm_water_idx = 0
pm_snow_idx = 6
pm_lc_years = {lcy}

[Runoff]
runoff_module = abcd
[[abcd]]
runoff_dir = abcd
calib_file = pars.npy
runoff_spinup = {rsp}
jobs = -1
PrecipitationFile = {pr}
TempMinFile = {tn}
{chs}
[Routing]
routing_module = mrtm
[[mrtm]]
routing_dir = mrtm
routing_spinup = {rtsp}
channel_velocity = velocity.npy
flow_distance = flow_dist.npy
flow_direction = flow_dir.npy
{vs}{calib}{post_sections}'''.format(vs=vs_line, grid='\nGriddedOutput = 1' if gridded else '', ofmt=int(output_format), oyear=int(output_in_year), chs=chs_lines, hist='True' if hist_flag else 'False', post_project=post_project, post_sections=post_sections, project=project, root=root, nb=world.n_basins, ncell=world.ncell, nrow=world.nrow, ncol=world.ncol,
                  y0=start_year, y1=end_year, ov=', '.join(output_vars), cal=int(obs is not None or gauges is not None), nlcs=world.nlcs,
                  lcy=', '.join(str(y) for y in world.lc_years), rsp=runoff_spinup,
                  rtsp=nmonths if routing_spinup is None else routing_spinup,
                  pr=os.path.join(dirs['ro'], 'pr.npy'), tn=os.path.join(dirs['ro'], 'tmin.npy'), calib=calib))
    if drought_index is not None:
        enable_drought_index(ini, **drought_index)
    return ini


def write_ensemble_example(root, world, forcings, start_year, end_year, names=None, statistics=(), statistics_vars=None,
                           member_outputs=1, section=True, output_unit=0, **kw):
    """``write_example`` of ``forcings[0]`` plus one forcing set per member under input/ensemble/<name>/ and the
    members table input/ensemble/members.csv (PM's files relative to the PET directory, as the ini names them; ABCD's
    two as full paths, as the ini does).  ``section``: an [Ensemble] section naming the table, ``statistics``,
    ``statistics_vars`` and ``member_outputs`` is appended to the ini; ``output_unit``: OutputUnit of the ini.
    Returns (ini path, [(name, {setting: full path})]) -- the second is what ``run_ensemble(ini, members=...)`` takes."""
    import os
    ini = write_example(root, world, forcings[0], start_year, end_year, **kw)
    names = ['m{:02d}'.format(k) for k in range(len(forcings))] if names is None else list(names)
    ens = os.path.join(root, 'input', 'ensemble')
    pet_dir = os.path.join(root, 'input', 'pet', 'penman_monteith')
    pm = {'pm_tas': 'tas', 'pm_tmin': 'tmin', 'pm_rhs': 'rhs', 'pm_wind': 'wind', 'pm_rsds': 'rsds', 'pm_rlds': 'rlds'}
    ro = {'PrecipitationFile': 'precip', 'TempMinFile': 'abcd_tmin'}
    members, rows = [], ['name,' + ','.join(list(pm) + list(ro))]
    for name, f in zip(names, forcings):
        d = os.path.join(ens, name)
        os.makedirs(d, exist_ok=True)
        paths = {}
        for setting, key in list(pm.items()) + list(ro.items()):
            paths[setting] = os.path.join(d, key + '.npy')
            np.save(paths[setting], f[key])
        members.append((name, paths))
        rows.append(','.join([name] + [os.path.relpath(paths[k], pet_dir) for k in pm] + [paths[k] for k in ro]))
    table = os.path.join(ens, 'members.csv')
    with open(table, 'w') as fh:
        fh.write('\n'.join(rows) + '\n')
    text = open(ini).read()
    if output_unit:
        text = text.replace('OutputUnit = 0', 'OutputUnit = {}'.format(int(output_unit)))
    if section:
        text += '\n[Ensemble]\nmembers = {}\n'.format(table)
        if statistics:
            text += 'statistics = {}\n'.format(', '.join(statistics))
        if statistics_vars:
            text += 'statistics_vars = {}\n'.format(', '.join(statistics_vars))
        text += 'member_outputs = {}\n'.format(int(member_outputs))
    with open(ini, 'w') as fh:
        fh.write(text)
    return ini, members


def hgm_forcing(world, forcing):
    """Hargreaves inputs from a ``make_forcing`` set: temperature = tas, daily temperature range = tas - tmin."""
    return {'temp': forcing['tas'], 'dtr': forcing['tas'] - forcing['tmin'], 'precip': forcing['precip'],
            'abcd_tmin': forcing['abcd_tmin']}


def hgm_soil(world, seed=7):
    """GWAM soil inputs for ``world``: maximum soil moisture [ncell] (mm, zeros at every 37th cell: no soil) and the two
    water-body tables, rows of (1-based cell id, 999)."""
    n = world.ncell
    sm = 50.0 + 450.0 * uniform(splitmix64(np.uint64(seed)), 1, np.arange(n, dtype=np.uint64))
    sm[::37] = 0.0
    cells = np.arange(1, n + 1)
    lakes = np.stack([cells[5::41], np.full(len(cells[5::41]), 999)], axis=1)
    addit = np.stack([cells[9::53], np.full(len(cells[9::53]), 999)], axis=1)
    return sm, lakes, addit


def write_hgm_example(root, world, forcing, start_year, end_year, project='hargreaves_gwam_mrtm_synth', runoff='gwam',
                      runoff_spinup=12, routing_spinup=12, output_vars=('q', 'avgchflow'), hist_flag=True, sav=None,
                      ch_storage=None, precipitation=None, soil=None, routing=True, pet='hargreaves', daylight=None,
                      obs=None, drought_index=None):
    """Write a hargreaves_gwam_mrtm (``runoff='abcd'``: hargreaves_abcd_mrtm) input tree under ``root``; returns the .ini.

    Keys and layout follow the reference's test configuration (xanthos/test/configs/hargreaves_gwam_mrtm.ini; ini_reader.py
    :216-243, :311-350): input/pet/hargreaves/{tas.npy, dtr.npy}, input/runoff/gwam/{soil_moisture.csv, lakes.csv,
    addit.csv, pr.npy}, the reference grid tables under input/reference (with the region / country maps the reference's
    loader always reads) and the routing inputs under input/routing/mrtm.  ``forcing``: ``hgm_forcing`` keys.
    ``hist_flag=False``: future mode from ``sav`` and ``ch_storage`` [ncell, k] (SavFile, ChStorageFile: last column read).
    ``precipitation``: the [[gwam]] precipitation key (None: not written, the reference's behaviour).
    ``pet``: 'hs' or 'thornthwaite' write that PET module instead (``write_pet_ext_example``), ``daylight`` its
    [[thornthwaite]] daylight key.  ``obs``: observed runoff rows (basin, -, -, value) -> Calibrate = 1 on basins 1-2."""
    import os
    inp = os.path.join(root, 'input')
    pet_dirname = {'hargreaves': 'hargreaves', 'hs': 'hargreaves_samani', 'thornthwaite': 'thornthwaite'}[pet]
    dirs = {k: os.path.join(inp, *v) for k, v in dict(ref=('reference',), pet=('pet', pet_dirname),
                                                      ro=('runoff', runoff), rt=('routing', 'mrtm')).items()}
    for d in dirs.values():
        os.makedirs(d, exist_ok=True)
    np.savetxt(os.path.join(dirs['ref'], 'Grid_Areas_ID.csv'), world.area * 100.0, delimiter=',', fmt='%.17g')   # ha
    np.savetxt(os.path.join(dirs['ref'], 'coordinates.csv'), world.coords, delimiter=',', fmt='%.17g')
    np.savetxt(os.path.join(dirs['ref'], 'basin.csv'), np.concatenate([[0], world.basin_ids]), fmt='%d')   # 1 header row
    with open(os.path.join(dirs['ref'], 'BasinNames235.txt'), 'w') as fh:
        fh.write('\n'.join('Basin{:03d}'.format(k) for k in range(1, world.n_basins + 1)) + '\n')
    np.savetxt(os.path.join(dirs['ref'], 'region32_grids.csv'), np.concatenate([[0], world.basin_ids % 6 + 1]), fmt='%d')
    with open(os.path.join(dirs['ref'], 'Rgn32Names.csv'), 'w') as fh:
        fh.write('region,region_id\n' + '\n'.join('Region{},{}'.format(k, k) for k in range(1, 8)))
    np.savetxt(os.path.join(dirs['ref'], 'country.csv'), np.concatenate([[0], world.basin_ids % 9 + 1]), fmt='%d')
    with open(os.path.join(dirs['ref'], 'country-names.csv'), 'w') as fh:
        fh.write(''.join('{},Country{}\n'.format(k, k) for k in range(10)))
    pet_files = {'hargreaves': (('tas', 'temp'), ('dtr', 'dtr')), 'hs': (('tas', 'tas'), ('tmin', 'tmin'), ('tmax', 'tmax')),
                 'thornthwaite': (('tas', 'tas'),)}[pet]
    for fn, key in pet_files:
        np.save(os.path.join(dirs['pet'], fn + '.npy'), forcing[key])
    pet_sec = {'hargreaves': '[[hargreaves]]\npet_dir = hargreaves\nTemperatureFile = tas.npy\n'
                             'DailyTemperatureRangeFile = dtr.npy\n',
               'hs': '[[hargreaves-samani]]\npet_dir = hargreaves_samani\nhs_tas = tas.npy\nhs_tmin = tmin.npy\n'
                     'hs_tmax = tmax.npy\n',
               'thornthwaite': '[[thornthwaite]]\npet_dir = thornthwaite\ntrn_tas = tas.npy\n'}[pet]
    if daylight is not None:
        pet_sec += 'daylight = {}\n'.format(daylight)
    calib = ''
    if obs is not None:
        obs_file = os.path.join(inp, 'obs.csv')
        np.savetxt(obs_file, obs, delimiter=',', fmt='%.17g')
        calib = ('\n[Calibrate]\nset_calibrate = 0\nobserved = {}\nobs_unit = km3_per_mth\ncalib_out_dir = {}\n'
                 'calibration_basins = 1-2\n').format(obs_file, os.path.join(root, 'calib_out'))
    np.save(os.path.join(dirs['ro'], 'pr.npy'), forcing['precip'])
    if routing:
        np.save(os.path.join(dirs['rt'], 'velocity.npy'), world.velocity)
        np.save(os.path.join(dirs['rt'], 'flow_dist.npy'), world.flow_dist)
        np.save(os.path.join(dirs['rt'], 'flow_dir.npy'), world.flow_dir)
    future = ''
    if runoff == 'gwam':
        sm, lakes, addit = hgm_soil(world) if soil is None else soil
        np.savetxt(os.path.join(dirs['ro'], 'soil_moisture.csv'), sm, fmt='%.17g', header='max_soil_moisture', comments='')
        np.savetxt(os.path.join(dirs['ro'], 'lakes.csv'), lakes, delimiter=',', fmt='%d')
        np.savetxt(os.path.join(dirs['ro'], 'addit.csv'), addit, delimiter=',', fmt='%d')
        runoff_sec = ('[[gwam]]\nrunoff_dir = gwam\nrunoff_spinup = {}\nPrecipitationFile = pr.npy\n'
                      'max_soil_moisture = soil_moisture.csv\nlakes_msm = lakes.csv\naddit_water_msm = addit.csv\n'
                      ).format(runoff_spinup)
        if precipitation is not None:
            runoff_sec += 'precipitation = {}\n'.format(precipitation)
        if not hist_flag:
            np.save(os.path.join(dirs['ro'], 'sav.npy'), np.asarray(sav, dtype=float))
            np.save(os.path.join(dirs['rt'], 'ch_storage.npy'), np.asarray(ch_storage, dtype=float))
            future = ('ChStorageFile = {}\nChStorageVarName = chs\nSavFile = {}\nSavVarName = sav\n').format(
                os.path.join(dirs['rt'], 'ch_storage.npy'), os.path.join(dirs['ro'], 'sav.npy'))
    else:
        np.save(os.path.join(dirs['ro'], 'pars.npy'), world.abcd_pars)
        np.save(os.path.join(dirs['ro'], 'tmin.npy'), forcing['abcd_tmin'])
        runoff_sec = ('[[abcd]]\nrunoff_dir = abcd\ncalib_file = pars.npy\nrunoff_spinup = {}\njobs = -1\n'
                      'PrecipitationFile = {}\nTempMinFile = {}\n').format(
            runoff_spinup, os.path.join(dirs['ro'], 'pr.npy'), os.path.join(dirs['ro'], 'tmin.npy'))
    routing_sec = ''
    if routing:
        routing_sec = ('[Routing]\nrouting_module = mrtm\n[[mrtm]]\nrouting_dir = mrtm\nrouting_spinup = {}\n'
                       'channel_velocity = velocity.npy\nflow_distance = flow_dist.npy\nflow_direction = flow_dir.npy\n'
                       ).format(routing_spinup)
    ini = os.path.join(root, project + '.ini')
    with open(ini, 'w') as fh:
        fh.write('''[Project]
# synthetic {pet}_{runoff}_mrtm example written by xanthos_amd.synth.write_hgm_example
ProjectName = {project}
RootDir = {root}
InputFolder = input
OutputFolder = output
RefDir = reference
pet_dir = pet
RunoffDir = runoff
RoutingDir = routing
HistFlag = {hist}
n_basins = {nb}
ncell = {ncell}
ngridrow = {nrow}
ngridcol = {ncol}
StartYear = {y0}
EndYear = {y1}
output_vars = {ov}
OutputFormat = 1
OutputUnit = 0
OutputInYear = 0
AggregateRunoffBasin = 0
AggregateRunoffCountry = 0
AggregateRunoffGCAMRegion = 0
PerformDiagnostics = 0
CreateTimeSeriesPlot = 0
CalculateDroughtStats = 0
CalculateAccessibleWater = 0
CalculateHydropowerPotential = 0
CalculateHydropowerActual = 0
Calibrate = {cal}

[PET]
pet_module = {pet}
{pet_sec}
[Runoff]
runoff_module = {runoff}
{runoff_sec}{future}
{routing_sec}{calib}'''.format(pet=pet, pet_sec=pet_sec, cal=int(obs is not None), calib=calib, runoff=runoff, project=project, root=root, hist='True' if hist_flag else 'False',
                        nb=world.n_basins, ncell=world.ncell, nrow=world.nrow, ncol=world.ncol, y0=start_year,
                        y1=end_year, ov=', '.join(output_vars), runoff_sec=runoff_sec, future=future,
                        routing_sec=routing_sec))
    if drought_index is not None:          # (as in write_example)
        enable_drought_index(ini, **drought_index)
    return ini


def pet_ext_forcing(world, forcing):
    """Hargreaves-Samani / Thornthwaite inputs from a ``make_forcing`` set: tas, tmin, tmax = 2 tas - tmin."""
    return {'tas': forcing['tas'], 'tmin': forcing['tmin'], 'tmax': 2.0 * forcing['tas'] - forcing['tmin'],
            'precip': forcing['precip'], 'abcd_tmin': forcing['abcd_tmin']}


def write_pet_ext_example(root, world, forcing, start_year, end_year, pet='hs', runoff_spinup=25, **kw):
    """Write an hs_abcd_mrtm (``pet='hs'``) or thornthwaite_abcd_mrtm input tree under ``root``; returns the .ini.
    ``forcing``: ``pet_ext_forcing`` keys; the other keywords as ``write_hgm_example``'s (``daylight``, ``obs``, ...)."""
    if pet not in ('hs', 'thornthwaite'):
        raise ValueError("pet must be 'hs' or 'thornthwaite', not '{}'".format(pet))
    kw.setdefault('project', '{}_abcd_mrtm_synth'.format(pet))
    return write_hgm_example(root, world, forcing, start_year, end_year, runoff='abcd', runoff_spinup=runoff_spinup,
                             pet=pet, **kw)


def write_hydro_inputs(root, world, ndams=40, seed=11, nan_rule_frac=0.1, ties=True, dir_name='hydropower'):
    """Write a hydropower input tree matched to ``world`` under ``root``/input/``dir_name`` (the reference's HydActDir,
    ini_reader.py:495-504) and return its path.

    gridData.csv (ID, long, lati from world.coords, elevD, regID 0..32, inGrandELEC); resData_1593.csv with LONG_DD / LAT_DD
    first (the reference reads them with iloc[:, 0:2]), some CAPLIVE / HEAD NaN (the fall-backs); a few dams exactly on a
    cell border (idxmin ties: the first value in gridData order wins); simulated_cap_by_country.csv (factor, GCAM_ID by
    the position of the sorted countries); rule_curves_1593.npy [5, 12, ndams] with NaN entries (-> 1.1) and a first row
    of 0 (a release option for every storage); DRT_half_SourceArea_globe_float.txt, 360 x 720.  Dams sit on distinct
    cells; the routed flow of those cells must be finite (``make_forcing(..., nan_precip=False)``) for every dam to run.
    """
    import os
    import pandas as pd
    rng = np.random.default_rng(seed)
    hyd = os.path.join(root, 'input', dir_name)
    os.makedirs(hyd, exist_ok=True)
    n = world.ncell
    lon, lat = world.coords[:, 1], world.coords[:, 2]
    grid = pd.DataFrame({'ID': np.arange(1, n + 1), 'long': lon, 'lati': lat,
                         'elevD': np.round(rng.uniform(0.0, 400.0, n), 3), 'regID': rng.integers(0, 33, n),
                         'inGrandELEC': (rng.random(n) < 0.6).astype(int)})
    grid.loc[rng.random(n) < 0.05, 'elevD'] = 0.0
    grid.to_csv(os.path.join(hyd, 'gridData.csv'), index=False)
    cells = rng.choice(n, size=min(ndams, n), replace=False)
    nd = len(cells)
    dlon = lon[cells] + rng.uniform(-0.2, 0.2, nd)
    dlat = lat[cells] + rng.uniform(-0.2, 0.2, nd)
    if ties:
        # half a cell east / north of the cell centre: two longitudes (latitudes) are equally near; keep such a dam only
        # where the pair the reference's idxmin picks is a land cell
        pairs = set(zip(lon.tolist(), lat.tolist()))
        for d in range(0, nd, 5):
            tl, tt = lon[cells[d]] + 0.25, lat[cells[d]] + (0.25 if d % 10 == 0 else 0.0)
            pl = lon[np.argmin(np.abs(lon - tl))]
            pt = lat[np.argmin(np.abs(lat - tt))]
            if (pl, pt) in pairs:
                dlon[d], dlat[d] = tl, tt
    countries = np.array(['C{:02d}'.format(k) for k in range(7)])
    cap = rng.uniform(50.0, 3000.0, nd)
    res = pd.DataFrame({'LONG_DD': dlon, 'LAT_DD': dlat, 'DAM_NAME': ['Dam {}'.format(k) for k in range(nd)],
                        'COUNTRY': countries[np.arange(nd) % len(countries)], 'CAP': cap,
                        'CAPLIVE': cap * rng.uniform(0.3, 1.0, nd), 'ECAP': rng.uniform(20.0, 2000.0, nd),
                        'FLOW_M3S': rng.uniform(20.0, 600.0, nd), 'EFF': rng.uniform(0.8, 0.95, nd),
                        'HEAD': rng.uniform(10.0, 200.0, nd), 'CATCH': rng.uniform(500.0, 20000.0, nd)})
    res.loc[rng.random(nd) < 0.2, 'CAPLIVE'] = np.nan
    res.loc[rng.random(nd) < 0.2, 'HEAD'] = np.nan
    res.to_csv(os.path.join(hyd, 'resData_1593.csv'), index=False)
    nc = len(np.unique(res['COUNTRY']))
    pd.DataFrame({'country': np.unique(res['COUNTRY']), 'factor': rng.uniform(1.0, 2.5, nc),
                  'GCAM_ID': rng.integers(1, 4, nc)}).to_csv(os.path.join(hyd, 'simulated_cap_by_country.csv'), index=False)
    rc = np.sort(rng.uniform(0.0, 1.05, (5, 12, nd)), axis=0)
    rc[0] = 0.0
    rc[1:][rng.random((4, 12, nd)) < nan_rule_frac] = np.nan
    np.save(os.path.join(hyd, 'rule_curves_1593.npy'), rc)
    ii, jj = np.mgrid[0:360, 0:720]
    np.savetxt(os.path.join(hyd, 'DRT_half_SourceArea_globe_float.txt'), 750.0 * (1 + (3 * ii + jj) % 23), fmt='%.1f')
    return hyd


def enable_hydro(ini, hpot_start_date='1/1971', hact_start_date='1/1971', q_ex=0.9, ef=0.85, dir_name='hydropower',
                 potential=True, actual=True):
    """Switch the hydropower post-processors on in an .ini written by ``write_example`` / ``write_hgm_example``."""
    text = open(ini).read()
    proj = 'HydActDir = {}\nCalculateHydropowerPotential = {}\nCalculateHydropowerActual = {}\n'.format(
        dir_name, int(potential), int(actual))
    text = text.replace('\n[PET]', '\n' + proj + '\n[PET]', 1)
    text += ('\n[HydropowerPotential]\nhpot_start_date = {}\nq_ex = {!r}\nef = {!r}\n'
             '\n[HydropowerActual]\nhact_start_date = {}\n').format(hpot_start_date, q_ex, ef, hact_start_date)
    open(ini, 'w').write(text)
    return ini


def enable_evaluate(ini, gauges, gauge_obs, gauge_missing=None):
    """Switch the scoring at stream gauges on in an .ini written by ``write_example`` / ``write_hgm_example``: ``gauges``
    (rows [gauge_id, cell_id (1-based)[, weight]]) and ``gauge_obs`` (rows [gauge_id, 0, 0, value], NaN = missing) are
    written next to the ini's input tree as eval_gauges.csv / eval_gauge_obs.csv and named in an [Evaluate] section;
    ``gauge_missing``: a sentinel written to the section."""
    import os
    text = open(ini).read()
    inp = os.path.join(os.path.dirname(os.path.abspath(ini)), 'input')
    os.makedirs(inp, exist_ok=True)
    paths = os.path.join(inp, 'eval_gauges.csv'), os.path.join(inp, 'eval_gauge_obs.csv')
    np.savetxt(paths[0], np.atleast_2d(gauges), delimiter=',', fmt='%.17g')
    np.savetxt(paths[1], gauge_obs, delimiter=',', fmt='%.17g')
    text += '\n[Evaluate]\ngauges = {}\ngauge_observed = {}\n'.format(*paths)
    if gauge_missing is not None:
        text += 'gauge_missing = {!r}\n'.format(float(gauge_missing))
    open(ini, 'w').write(text)
    return ini


def enable_drought_index(ini, index_var='q', scales=(1, 3, 12), **keys):
    """Switch the standardized drought indices on in an .ini written by one of the example writers: ``CalculateDroughtIndex
    = 1`` in [Project] and a [DroughtIndex] section with ``index_var``, ``scales`` and whatever else is given
    (``distribution``, ``reference_start_year``, ``reference_end_year``, ``parameters``, ``max_shape``) as written."""
    text = open(ini).read()
    text = text.replace('\n[PET]', '\nCalculateDroughtIndex = 1\n\n[PET]', 1)
    text += '\n[DroughtIndex]\nindex_var = {}\nscales = {}\n'.format(index_var, ', '.join(str(k) for k in scales))
    text += ''.join('{} = {}\n'.format(k, v) for k, v in keys.items())
    open(ini, 'w').write(text)
    return ini


def enable_trend(ini, trend_vars=('q',), series=('annual', 'seasonal'), **keys):
    """Switch the trend tables on in an .ini written by one of the example writers: ``CalculateTrend = 1`` in [Project] and a
    [Trend] section with ``trend_vars``, ``series`` and whatever else is given (``annual``, ``start_year``, ``end_year``,
    ``confidence``) as written."""
    text = open(ini).read()
    text = text.replace('\n[PET]', '\nCalculateTrend = 1\n\n[PET]', 1)
    text += '\n[Trend]\ntrend_vars = {}\nseries = {}\n'.format(', '.join(trend_vars), ', '.join(series))
    text += ''.join('{} = {}\n'.format(k, v) for k, v in keys.items())
    open(ini, 'w').write(text)
    return ini


def enable_extremes(ini, extreme_vars=('q',), kinds=('max', 'min'), **keys):
    """Switch the extremes on in an .ini written by one of the example writers: ``CalculateExtremes = 1`` in [Project] and an
    [Extremes] section with ``extreme_vars``, ``kinds`` and whatever else is given (``return_periods`` -- a sequence is joined
    by commas --, ``start_year``, ``end_year``, ``year_start_month``, ``min_years``, ``parameters``) as written."""
    text = open(ini).read()
    text = text.replace('\n[PET]', '\nCalculateExtremes = 1\n\n[PET]', 1)
    text += '\n[Extremes]\nextreme_vars = {}\nkinds = {}\n'.format(', '.join(extreme_vars), ', '.join(kinds))
    for k, v in keys.items():
        text += '{} = {}\n'.format(k, ', '.join(str(w) for w in v) if isinstance(v, (list, tuple)) else v)
    open(ini, 'w').write(text)
    return ini


def with_signatures(ini, signature_vars=('q',), **keys):
    """Switch the flow signatures on in an .ini written by one of the example writers: ``CalculateSignatures = 1`` in [Project]
    and a [Signatures] section with ``signature_vars`` and whatever else is given (``exceedance`` -- a sequence is joined by
    commas --, ``start_year``, ``end_year``, ``year_start_month``) as written."""
    text = open(ini).read()
    text = text.replace('\n[PET]', '\nCalculateSignatures = 1\n\n[PET]', 1)
    text += '\n[Signatures]\nsignature_vars = {}\n'.format(', '.join(signature_vars))
    for k, v in keys.items():
        text += '{} = {}\n'.format(k, ', '.join(str(w) for w in v) if isinstance(v, (list, tuple)) else v)
    open(ini, 'w').write(text)
    return ini


def with_water_balance(ini, levels=('cell',), **keys):
    """Switch the water balance on in an .ini written by one of the example writers: ``CalculateWaterBalance = 1`` in [Project]
    and a [WaterBalance] section with ``levels`` and whatever else is given (``start_year``, ``end_year``, ``year_start_month``,
    ``max_lag``, ``omega0``, ``annual``) as written."""
    text = open(ini).read()
    text = text.replace('\n[PET]', '\nCalculateWaterBalance = 1\n\n[PET]', 1)
    text += '\n[WaterBalance]\nlevels = {}\n'.format(', '.join(levels))
    for k, v in keys.items():
        text += '{} = {}\n'.format(k, ', '.join(str(w) for w in v) if isinstance(v, (list, tuple)) else v)
    open(ini, 'w').write(text)
    return ini


def write_diag_inputs(root, world, seed=17, nvic=30, dir_name='diagnostics'):
    """Write the four comparison tables of the diagnostics (the reference's DiagDir, ini_reader.py:439-445) matched to
    ``world`` under ``root``/input/``dir_name`` and return its path.

    vic.csv [ncell, nvic] (km3/yr, a few NaN cells), unh.csv [ncell], and the two-column (cell id, value) tables wbm.csv and
    wbmc.csv: most cells once, some missing, a few ids repeated (the later row wins) and one row with id 0 (the reference
    puts it on the last cell)."""
    import os
    rng = np.random.default_rng(seed)
    d = os.path.join(root, 'input', dir_name)
    os.makedirs(d, exist_ok=True)
    n = world.ncell
    vic = rng.lognormal(-3.0, 1.5, (n, nvic))
    vic[rng.random(n) < 0.03] = np.nan
    np.savetxt(os.path.join(d, 'vic.csv'), vic, delimiter=',', fmt='%.17g')
    unh = rng.lognormal(-3.0, 1.5, n)
    unh[rng.random(n) < 0.03] = np.nan
    np.savetxt(os.path.join(d, 'unh.csv'), unh, fmt='%.17g')
    for k, name in enumerate(('wbm.csv', 'wbmc.csv')):
        ids = np.flatnonzero(rng.random(n) < 0.9) + 1
        ids = np.concatenate([ids, rng.choice(ids, max(1, n // 50)), [0]])
        vals = rng.lognormal(-3.0 + k, 1.5, len(ids))
        np.savetxt(os.path.join(d, name), np.stack([ids, vals], axis=1), delimiter=',', fmt='%.17g')
    return d


def enable_diagnostics(ini, diag_scale=0, plot_scale=0, map_id=999, dir_name='diagnostics', diagnostics=True, plots=True):
    """Switch the diagnostics and / or the time-series plots on in an .ini written by ``write_example`` /
    ``write_hgm_example`` (DiagDir, [Diagnostics] for ``write_diag_inputs``' files, [TimeSeriesPlot]).  ``map_id``: an
    integer or a list.  The basin, country and region maps must be in the reference directory (``write_hgm_example``, or
    ``write_example(..., aggregates=True)``)."""
    import re
    text = open(ini).read()
    text = re.sub(r'\n(PerformDiagnostics|CreateTimeSeriesPlot) *=[^\n]*', '', text)
    proj = 'DiagDir = {}\nPerformDiagnostics = {}\nCreateTimeSeriesPlot = {}\n'.format(dir_name, int(diagnostics), int(plots))
    text = text.replace('\n[PET]', '\n' + proj + '\n[PET]', 1)
    if diagnostics:
        text += ('\n[Diagnostics]\nVICDataFile = vic.csv\nUNHDataFile = unh.csv\nWBMDataFile = wbm.csv\n'
                 'WBMCDataFile = wbmc.csv\nScale = {}\n').format(diag_scale)
    if plots:
        ids = ', '.join(str(int(i)) for i in map_id) if isinstance(map_id, (list, tuple)) else str(int(map_id))
        text += '\n[TimeSeriesPlot]\nScale = {}\nMapID = {}\n'.format(plot_scale, ids)
    open(ini, 'w').write(text)
    return ini
