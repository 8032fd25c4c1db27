"""Host tables of the streamflow calibration objective (set_calibrate = 1).

For a basin B the objective routes B's runoff through UM (the connection matrix routing uses, upstream_genmatrix) and
sums Avg_ChFlow over B's outlets.  Only B's upstream closure can reach those outlets, so each basin is routed on its own
closure with the tables built here:

* outlets(B): the cells i of B whose outflow reaches no cell of B through UM (UM[j, i] = +1 for no j of B, j != i) --
  cells that drain to the ocean, into a sink or into another basin;
* closure(B): B and every cell upstream of a cell of B through UM, in ascending cell order;
* the closure's rows of UM in the stored column order (the summation order of UM.dot), columns re-indexed to the
  closure (the mapping is increasing, so the order is kept), tau^-1 = ChV / L, area and initial storage of every closure
  cell, the forcing column of each basin cell and the outlet ranks.

Pure numpy; nothing here touches the device.
"""
import numpy as np

from ..ini_reader import ValidationException

MAX_CLOSURE = 3072          # cells of one closure the kernel takes (csrc/xh_calib_flow.hip MAX_CLOSURE)


def um_arrays(um):
    """(indptr, indices, sign) of UM: a routing.mrtm.UpstreamMatrix or a scipy sparse matrix (stored order kept)."""
    if not callable(getattr(um, 'sign', None)):          # routing.mrtm.UpstreamMatrix
        return np.asarray(um.indptr, dtype=np.int64), np.asarray(um.indices, dtype=np.int64), np.asarray(um.sign, np.int8)
    m = um.tocsr()
    return np.asarray(m.indptr, dtype=np.int64), np.asarray(m.indices, dtype=np.int64), np.asarray(m.data).astype(np.int8)


def _rows(indptr, n):
    return np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))


def outlets_and_closure(indptr, indices, sign, cells):
    """(outlets, closure) of the basin with the cells ``cells`` (ascending global indices): both ascending arrays."""
    n = indptr.size - 1
    cells = np.asarray(cells, dtype=np.int64)
    in_b = np.zeros(n, dtype=bool)
    in_b[cells] = True
    rows = _rows(indptr, n)
    edge = (sign > 0) & (rows != indices)              # row <- column: the column cell flows into the row cell
    drains_into_b = np.zeros(n, dtype=bool)
    drains_into_b[indices[edge & in_b[rows]]] = True
    outlets = cells[~drains_into_b[cells]]
    in_c = in_b.copy()
    frontier = cells
    while frontier.size:
        lo, hi = indptr[frontier], indptr[frontier + 1]
        cnt = hi - lo
        take = np.repeat(lo - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(cnt.sum())
        e = take[sign[take] > 0]
        up = np.unique(indices[e])
        up = up[~in_c[up]]
        in_c[up] = True
        frontier = up
    return outlets, np.nonzero(in_c)[0]


class FlowTables:
    """Closure tables of the basins ``basins`` (1-based basin numbers), concatenated basin after basin.

    Arrays (as the C-ABI's xh_calib_flow_desc takes them): closure_ptr [nb + 1]; row_ptr [ncl + 1], cols [nnz] (closure
    local), sign [nnz]; basin_col [ncl] (column of the basin's own cell list, -1 outside the basin); outlet_rank [ncl];
    tauinv, area, s0 [ncl]; velocity, length [ncl] (ChV and L, tauinv == velocity / length in bits: what the velocity
    form scales, xh_calib_velocity_desc); ndays [nmonths]; plus per basin the closure and outlets as global cell indices and the
    dealing weight closure cells x (nmonths + routing_spinup)."""

    def __init__(self, um, basin_ids, basins, flow_dist, velocity, area, chs_prev, ndays, nmonths, routing_spinup,
                 dt=10800, max_closure=MAX_CLOSURE):
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
        self.closures, self.outlets, self.basin_cells = [], [], []
        cptr, rptr, cols, sgn, bcol, orank = [0], [0], [], [], [], []
        for b in self.basins:
            cells = np.nonzero(basin_ids == b)[0]
            if cells.size == 0:
                raise ValidationException('basin {} has no cells'.format(b))
            out, clo = outlets_and_closure(indptr, indices, sign, cells)
            if clo.size > max_closure:
                raise ValidationException(
                    'set_calibrate = 1: the upstream closure of basin {} has {} cells; the streamflow objective routes at '
                    'most {} cells per basin.'.format(b, clo.size, max_closure))
            self.closures.append(clo)
            self.outlets.append(out)
            self.basin_cells.append(cells)
            loc = np.full(ncell, -1, dtype=np.int64)
            loc[clo] = np.arange(clo.size)
            lo, hi = indptr[clo], indptr[clo + 1]
            for i, j in zip(lo, hi):
                cols.append(loc[indices[i:j]])
                sgn.append(sign[i:j])
                rptr.append(rptr[-1] + (j - i))
            assert all((c >= 0).all() for c in cols[-clo.size:])
            bc = np.full(clo.size, -1, dtype=np.int32)
            bc[loc[cells]] = np.arange(cells.size)
            bcol.append(bc)
            orr = np.full(clo.size, -1, dtype=np.int32)
            orr[loc[out]] = np.arange(out.size)
            orank.append(orr)
            cptr.append(cptr[-1] + clo.size)
        cat = np.concatenate
        allc = cat(self.closures)
        self.closure_ptr = np.asarray(cptr, dtype=np.int64)
        self.row_ptr = np.asarray(rptr, dtype=np.int64)
        self.cols = np.ascontiguousarray(cat(cols), dtype=np.int32)
        self.sign = np.ascontiguousarray(cat(sgn), dtype=np.int8)
        self.basin_col = np.ascontiguousarray(cat(bcol), dtype=np.int32)
        self.outlet_rank = np.ascontiguousarray(cat(orank), dtype=np.int32)
        self.tauinv = np.ascontiguousarray(velocity[allc] / flow_dist[allc])           # ChV / L (mrtm.py:37)
        self.velocity = np.ascontiguousarray(velocity[allc])
        self.length = np.ascontiguousarray(flow_dist[allc])
        self.area = np.ascontiguousarray(area[allc])
        self.s0 = np.ascontiguousarray(s0[allc])
        self.weights = np.array([c.size for c in self.closures], dtype=np.int64) * (self.nmonths + self.routing_spinup)

    @property
    def foreign(self):
        """[ncl] bool: closure rows outside their basin, which a velocity scale of the basin leaves alone."""
        return self.basin_col < 0

    def part(self, i):
        """The tables of the i-th basin alone."""
        t = FlowTables.__new__(FlowTables)
        t.nmonths, t.routing_spinup, t.dt, t.ndays = self.nmonths, self.routing_spinup, self.dt, self.ndays
        t.basins, t.closures, t.outlets = [self.basins[i]], [self.closures[i]], [self.outlets[i]]
        t.basin_cells = [self.basin_cells[i]]
        c0, c1 = self.closure_ptr[i], self.closure_ptr[i + 1]
        e0, e1 = self.row_ptr[c0], self.row_ptr[c1]
        t.closure_ptr = np.array([0, c1 - c0], dtype=np.int64)
        t.row_ptr = np.ascontiguousarray(self.row_ptr[c0:c1 + 1] - e0)
        t.cols, t.sign = self.cols[e0:e1].copy(), self.sign[e0:e1].copy()
        for name in ('basin_col', 'outlet_rank', 'tauinv', 'velocity', 'length', 'area', 's0'):
            setattr(t, name, np.ascontiguousarray(getattr(self, name)[c0:c1]))
        t.weights = self.weights[i:i + 1].copy()
        return t

    @staticmethod
    def join(parts):
        """One table of the basins of several tables, in order (same months, spin-up, dt and day counts)."""
        p0 = parts[0]
        t = FlowTables.__new__(FlowTables)
        t.nmonths, t.routing_spinup, t.dt, t.ndays = p0.nmonths, p0.routing_spinup, p0.dt, p0.ndays
        for name in ('basins', 'closures', 'outlets', 'basin_cells'):
            setattr(t, name, [x for p in parts for x in getattr(p, name)])
        t.closure_ptr = np.concatenate([[0], np.cumsum([c.size for c in t.closures])]).astype(np.int64)
        off = np.cumsum([0] + [p.row_ptr[-1] for p in parts[:-1]])
        t.row_ptr = np.concatenate([[0]] + [p.row_ptr[1:] + o for p, o in zip(parts, off)]).astype(np.int64)
        for name in ('cols', 'sign', 'basin_col', 'outlet_rank', 'tauinv', 'velocity', 'length', 'area', 's0', 'weights'):
            setattr(t, name, np.ascontiguousarray(np.concatenate([getattr(p, name) for p in parts])))
        return t

    def subset(self, basins):
        """The tables of some of the basins (in the order given)."""
        return FlowTables.join([self.part(self.basins.index(int(b))) for b in basins])


def check_forcing(basins, basin_ids, pet, precip, nmonths):
    """ValidationException listing every basin with a cell of NaN precipitation or PET in months [0, nmonths), with its
    first such cell (0-based grid index): its runoff would be NaN, routing would carry it to the outlet and every
    member's ED would be NaN."""
    basin_ids = np.asarray(basin_ids)
    bad = []
    for b in basins:
        cells = np.nonzero(basin_ids == b)[0]
        nan = np.isnan(np.asarray(precip)[cells, :nmonths]).any(1) | np.isnan(np.asarray(pet)[cells, :nmonths]).any(1)
        if nan.any():
            bad.append('basin {} (cell {})'.format(b, int(cells[np.argmax(nan)])))
    if bad:
        raise ValidationException('set_calibrate = 1: NaN precipitation or PET in ' + ', '.join(bad) +
                                  '; the routed outlet flow would be NaN for every parameter vector. Leave these basins '
                                  'out through calibration_basins.')
