"""The member skill of the ensemble in numpy: the reference's basin series (calibrate_abcd.py:156-162) and the Kling-Gupta
distance of oracle.calib.kge_distance (:196-213); what xh_basin_kge is held to."""
import numpy as np

from oracle.calib import kge_distance


def basin_series(q, area, cells, unit='km3_per_mth'):
    """q [ncell, nmonths] in mm per month -> the basin's series [nmonths]: np.nansum over its cells of q * area * 1e-6
    (km3_per_mth) or of q (mm_per_mth)."""
    rows = np.asarray(q)[np.asarray(cells)]
    if unit == 'km3_per_mth':
        return np.nansum(rows * np.asarray(area)[np.asarray(cells)][:, None] * 1e-6, 0)
    if unit == 'mm_per_mth':
        return np.nansum(rows, 0)
    raise ValueError(unit)


def distance(series, obs):
    """ED of one series against one record; NaN where numpy gives NaN (a constant series or record)."""
    with np.errstate(all='ignore'):
        return float(kge_distance(np.asarray(series, dtype=float), np.asarray(obs, dtype=float)))


def skill(q, area, basin_cells, obs, unit='km3_per_mth'):
    """(series [nbasins, nmonths], ED [nbasins]) of q against obs [nbasins, nmonths]; basin_cells: one ascending index
    array per basin."""
    series = np.stack([basin_series(q, area, cells, unit) for cells in basin_cells])
    return series, np.array([distance(s, o) for s, o in zip(series, obs)])


def cells_of(basin_ids, basins):
    """The ascending cell indices of each basin id of ``basins`` on the grid's basin map."""
    basin_ids = np.asarray(basin_ids)
    return [np.flatnonzero(basin_ids == b) for b in basins]
