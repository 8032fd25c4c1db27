"""Host tables of the gauge form of the streamflow calibration objective (set_calibrate = 1 with ``gauges``).

A gauge is (gauge_id, cell, weight) with a record of monthly discharge [m3/s] that may have gaps (NaN).  It belongs to
the basin of its cell.  Basin B is scored at its gauges instead of at its outlets:

* the series of gauge g is Avg_ChFlow[cell_g], nothing summed;
* only the union of the gauges' upstream closures through UM can reach them, so B is routed once per member on that
  union -- a subset of the outlet closure of flow_tables.FlowTables, in ascending cell order.  Basin cells outside the
  union take no part in the routing pass (they do in the runoff spin-up, whose basin mean runs over all of B's cells);
  closure cells outside B carry zero runoff from their own initial storage;
* ED_g = 1 - KGE over the months with a finite observation, ED_B = (sum w_g ED_g) / (sum w_g) with the gauges in
  ascending (cell, gauge_id) order.

The tables are those of FlowTables without outlet ranks, plus per basin its gauges in that order: gauge_ptr [nb + 1],
gauge_row [ng] (closure-local row), gauge_weight [ng], and gauge_id, gauge_cell (0-based grid index), obs [ng, nmonths].

Pure numpy; nothing here touches the device.
"""
import logging

import numpy as np

from ..ini_reader import ValidationException
from .flow_tables import MAX_CLOSURE, outlets_and_closure, um_arrays


class Gauges:
    """Stream gauges as the loader delivers them: ids [n], cells [n] (0-based grid index), weights [n] (default 1) and
    obs [n, nmonths] in m3/s, NaN = missing."""

    def __init__(self, ids, cells, weights=None, obs=None):
        self.ids = np.asarray(ids).astype(np.int64).reshape(-1)
        self.cells = np.asarray(cells).astype(np.int64).reshape(-1)
        self.weights = (np.ones(self.ids.size) if weights is None else np.asarray(weights, dtype=np.float64)).reshape(-1)
        self.obs = None if obs is None else np.atleast_2d(np.asarray(obs, dtype=np.float64))
        if not (self.ids.size == self.cells.size == self.weights.size) or \
                (self.obs is not None and self.obs.shape[0] != self.ids.size):
            raise ValueError('gauge ids, cells, weights and records must have one entry per gauge')


def check_gauges(g, ncell):
    """Refuse a gauge cell outside the grid, a duplicate gauge id, a weight that is not positive and finite."""
    bad = (g.cells < 0) | (g.cells >= ncell)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValidationException('gauge {}: cell_id {} lies outside the grid of {} cells'.format(
            int(g.ids[i]), int(g.cells[i]) + 1, ncell))
    u, cnt = np.unique(g.ids, return_counts=True)
    if (cnt > 1).any():
        raise ValidationException('duplicate gauge id {}'.format(int(u[np.argmax(cnt > 1)])))
    bad = ~(np.isfinite(g.weights) & (g.weights > 0))
    if bad.any():
        i = int(np.argmax(bad))
        raise ValidationException('gauge {}: the weight must be positive and finite, not {}'.format(
            int(g.ids[i]), g.weights[i]))


def check_records(ids, obs):
    """Refuse a record the score cannot use -- fewer than 2 finite observations, or finite observations of zero variance
    or zero mean (KGE divides by both) -- and warn about one with fewer than 12 finite months."""
    for gid, row in zip(ids, obs):
        v = row[np.isfinite(row)]
        if v.size < 2:
            raise ValidationException('gauge {} has {} finite observation(s); the score needs at least 2'.format(
                int(gid), v.size))
        if np.std(v) == 0:
            raise ValidationException('gauge {}: its finite observations have zero variance; KGE is undefined'.format(
                int(gid)))
        if np.mean(v) == 0:
            raise ValidationException('gauge {}: its finite observations have zero mean; KGE is undefined'.format(
                int(gid)))
        if v.size < 12:
            logging.warning('gauge {} has only {} finite months'.format(int(gid), v.size))


class GaugeTables:
    """Union-closure tables and gauges of the basins ``basins`` (1-based basin numbers), basin after basin.

    Arrays (as the C-ABI's xh_calib_gauge_desc takes them): closure_ptr [nb + 1]; row_ptr [ncl + 1], cols [nnz] (closure
    local), sign [nnz]; basin_col [ncl] (column of the basin's own cell list -- all of the basin's cells -- or -1 outside
    the basin); tauinv, area, s0 [ncl]; velocity, length [ncl] (ChV and L, tauinv == velocity / length in bits: what the
    velocity form scales); ndays [nmonths]; gauge_ptr [nb + 1], gauge_row [ng], gauge_weight [ng]; plus
    gauge_id, gauge_cell, obs [ng, nmonths], per basin the closure as global cell indices and the dealing weight
    union-closure cells x (nmonths + routing_spinup)."""

    gauge_form = True
    _ROW_ARRAYS = ('basin_col', 'tauinv', 'velocity', 'length', 'area', 's0')
    _GAUGE_ARRAYS = ('gauge_id', 'gauge_cell', 'gauge_weight', 'gauge_row', 'obs')

    def __init__(self, um, basin_ids, basins, gauges, flow_dist, velocity, area, chs_prev, ndays, nmonths,
                 routing_spinup, dt=10800, max_closure=MAX_CLOSURE):
        indptr, indices, sign = um_arrays(um)
        basin_ids = np.asarray(basin_ids)
        flow_dist, velocity, area = (np.asarray(a, dtype=np.float64) for a in (flow_dist, velocity, area))
        ncell = indptr.size - 1
        s0 = np.zeros(ncell) if chs_prev is None else np.asarray(chs_prev, dtype=np.float64)
        self.basins = [int(b) for b in basins]
        self.nmonths, self.routing_spinup, self.dt = int(nmonths), int(routing_spinup), float(dt)
        if not 0 <= self.routing_spinup <= self.nmonths:
            raise ValidationException('routing_spinup = {} must lie in [0, nmonths = {}] for set_calibrate = 1'.format(
                self.routing_spinup, self.nmonths))
        self.ndays = np.ascontiguousarray(np.asarray(ndays)[:self.nmonths], dtype=np.int32)
        check_gauges(gauges, ncell)
        if gauges.obs is None or gauges.obs.shape[1] < self.nmonths:
            raise ValidationException('the gauge records must hold {} months'.format(self.nmonths))
        g_basin = basin_ids[gauges.cells]
        out = ~np.isin(g_basin, self.basins)
        if out.any():
            logging.info('\t{} gauge(s) in basins that are not calibrated are ignored: {}'.format(
                int(out.sum()), ', '.join(str(int(i)) for i in gauges.ids[out])))
        self.closures, self.basin_cells = [], []
        cptr, rptr, cols, sgn, bcol, gptr = [0], [0], [], [], [], [0]
        gid, gcell, gw, grow, gobs = [], [], [], [], []
        for b in self.basins:
            cells = np.nonzero(basin_ids == b)[0]
            if cells.size == 0:
                raise ValidationException('basin {} has no cells'.format(b))
            sel = np.nonzero(g_basin == b)[0]
            if sel.size == 0:
                raise ValidationException('set_calibrate = 1 with gauges: basin {} has no gauge; leave it out of '
                                          'calibration_basins.'.format(b))
            sel = sel[np.lexsort((gauges.ids[sel], gauges.cells[sel]))]       # ascending (cell, gauge_id)
            check_records(gauges.ids[sel], gauges.obs[sel, :self.nmonths])
            _, clo = outlets_and_closure(indptr, indices, sign, np.unique(gauges.cells[sel]))
            if clo.size > max_closure:
                raise ValidationException(
                    'set_calibrate = 1: the union of the upstream closures of the gauges of basin {} has {} cells; the '
                    'streamflow objective routes at most {} cells per basin.'.format(b, clo.size, max_closure))
            self.closures.append(clo)
            self.basin_cells.append(cells)
            loc = np.full(ncell, -1, dtype=np.int64)
            loc[clo] = np.arange(clo.size)
            for i, j in zip(indptr[clo], indptr[clo + 1]):
                cols.append(loc[indices[i:j]])
                sgn.append(sign[i:j])
                rptr.append(rptr[-1] + (j - i))
            assert all((c >= 0).all() for c in cols[-clo.size:])
            col_of = np.full(ncell, -1, dtype=np.int64)
            col_of[cells] = np.arange(cells.size)
            bcol.append(col_of[clo].astype(np.int32))
            cptr.append(cptr[-1] + clo.size)
            gid.append(gauges.ids[sel])
            gcell.append(gauges.cells[sel])
            gw.append(gauges.weights[sel])
            grow.append(loc[gauges.cells[sel]])
            gobs.append(gauges.obs[sel, :self.nmonths])
            gptr.append(gptr[-1] + sel.size)
        cat = np.concatenate
        allc = cat(self.closures)
        self.closure_ptr = np.asarray(cptr, dtype=np.int64)
        self.row_ptr = np.asarray(rptr, dtype=np.int64)
        self.cols = np.ascontiguousarray(cat(cols), dtype=np.int32)
        self.sign = np.ascontiguousarray(cat(sgn), dtype=np.int8)
        self.basin_col = np.ascontiguousarray(cat(bcol), dtype=np.int32)
        self.tauinv = np.ascontiguousarray(velocity[allc] / flow_dist[allc])           # ChV / L (mrtm.py:37)
        self.velocity = np.ascontiguousarray(velocity[allc])
        self.length = np.ascontiguousarray(flow_dist[allc])
        self.area = np.ascontiguousarray(area[allc])
        self.s0 = np.ascontiguousarray(s0[allc])
        self.gauge_ptr = np.asarray(gptr, dtype=np.int64)
        self.gauge_id = np.ascontiguousarray(cat(gid), dtype=np.int64)
        self.gauge_cell = np.ascontiguousarray(cat(gcell), dtype=np.int64)
        self.gauge_weight = np.ascontiguousarray(cat(gw), dtype=np.float64)
        self.gauge_row = np.ascontiguousarray(cat(grow), dtype=np.int32)
        self.obs = np.ascontiguousarray(cat(gobs), dtype=np.float64)
        self.weights = np.array([c.size for c in self.closures], dtype=np.int64) * (self.nmonths + self.routing_spinup)

    @property
    def foreign(self):
        """[ncl] bool: closure rows outside their basin, which a velocity scale of the basin leaves alone."""
        return self.basin_col < 0

    @property
    def gauge_basin(self):
        """Basin number of every gauge."""
        return np.repeat(np.asarray(self.basins, dtype=np.int64), np.diff(self.gauge_ptr))

    @property
    def months_used(self):
        """Finite observations of every gauge."""
        return np.isfinite(self.obs).sum(1)

    def part(self, i):
        """The tables of the i-th basin alone."""
        t = GaugeTables.__new__(GaugeTables)
        t.nmonths, t.routing_spinup, t.dt, t.ndays = self.nmonths, self.routing_spinup, self.dt, self.ndays
        t.basins, t.closures, t.basin_cells = [self.basins[i]], [self.closures[i]], [self.basin_cells[i]]
        c0, c1 = self.closure_ptr[i], self.closure_ptr[i + 1]
        e0, e1 = self.row_ptr[c0], self.row_ptr[c1]
        g0, g1 = self.gauge_ptr[i], self.gauge_ptr[i + 1]
        t.closure_ptr = np.array([0, c1 - c0], dtype=np.int64)
        t.row_ptr = np.ascontiguousarray(self.row_ptr[c0:c1 + 1] - e0)
        t.cols, t.sign = self.cols[e0:e1].copy(), self.sign[e0:e1].copy()
        for name in self._ROW_ARRAYS:
            setattr(t, name, np.ascontiguousarray(getattr(self, name)[c0:c1]))
        t.gauge_ptr = np.array([0, g1 - g0], dtype=np.int64)
        for name in self._GAUGE_ARRAYS:
            setattr(t, name, np.ascontiguousarray(getattr(self, name)[g0:g1]))
        t.weights = self.weights[i:i + 1].copy()
        return t

    @staticmethod
    def join(parts):
        """One table of the basins of several tables, in order (same months, spin-up, dt and day counts)."""
        p0 = parts[0]
        t = GaugeTables.__new__(GaugeTables)
        t.nmonths, t.routing_spinup, t.dt, t.ndays = p0.nmonths, p0.routing_spinup, p0.dt, p0.ndays
        for name in ('basins', 'closures', 'basin_cells'):
            setattr(t, name, [x for p in parts for x in getattr(p, name)])
        t.closure_ptr = np.concatenate([[0], np.cumsum([c.size for c in t.closures])]).astype(np.int64)
        off = np.cumsum([0] + [p.row_ptr[-1] for p in parts[:-1]])
        t.row_ptr = np.concatenate([[0]] + [p.row_ptr[1:] + o for p, o in zip(parts, off)]).astype(np.int64)
        t.gauge_ptr = np.concatenate([[0], np.cumsum([p.gauge_ptr[-1] for p in parts])]).astype(np.int64)
        for name in ('cols', 'sign', 'weights') + GaugeTables._ROW_ARRAYS + GaugeTables._GAUGE_ARRAYS:
            setattr(t, name, np.ascontiguousarray(np.concatenate([getattr(p, name) for p in parts])))
        return t

    def subset(self, basins):
        """The tables of some of the basins (in the order given)."""
        return GaugeTables.join([self.part(self.basins.index(int(b))) for b in basins])
