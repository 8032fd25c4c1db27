"""Generate outfmt.npz in this directory: NetCDF and MATLAB files written by the REAL reference (JGCRI/xanthos v2.4.1).

Run in the build container only (needs the reference checkout, scipy and pandas):

    python tests/golden/make_golden_outfmt.py

The reference's ``OutWriter`` (xanthos/data_writer/out_writer.py) is imported unmodified by file path.

* MATLAB (OutputFormat 2): ``OutWriter.write()`` as it is; ``write_aggregates`` for the basin table.
* NetCDF (OutputFormat 0): ``OutWriter.write()`` raises here (``save_netcdf`` indexes the DataFrame it is handed with
  ``data[:, :]``, a KeyError / InvalidIndexError under pandas >= 1), so the files come from the writer's own steps in the
  order of ``write()`` -- ``agg_to_year``, the mm -> km3 ``multiply`` -- followed by its ``save_netcdf(filename, df.values,
  var)``, the call its docstring describes ("Write numpy array as a NetCDF").

The fixture holds the inputs and every produced file as a uint8 array:

  area, basin_ids, basin_names, in_<var>          67 cells x 24 months from 2000; var in q, avgchflow, soilmoisture
  <case>_<var>_written                            the array as written (DataFrame.values), case m0 = (OutputInYear 0,
                                                  OutputUnit 0), y1 = (1, 1)
  <case>_<var>_nc, <case>_<var>_mat               the files
  <case>_<var>_file                               their common name without the extension
  basin_values, basin_mat, basin_file             the basin table of case m0's written runoff and its .mat

The first rows of every input carry, two per row in the first month of either year and NaN elsewhere, the values that
decide a float64 -> big-endian float32 conversion (SPECIAL below, and their negatives); those rows have area 1e6 km2, so
that the yearly sum / mean and the km3 conversion of case y1 hand the same values to the file.
"""
import importlib.util
import os
import sys
import tempfile
import warnings
from types import SimpleNamespace

import numpy as np

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

NCELL, NMONTHS, START = 67, 24, 2000
VARS = ('q', 'avgchflow', 'soilmoisture')
CASES = {'m0': (0, 0), 'y1': (1, 1)}
PROJECT = 'golden'
# NaN; the sign of zero; binary32 subnormals (1e-45 rounds to the smallest one, 7e-46 lies just below half of it ... and
# rounds to zero); overflow (1e39, and the double just above the midpoint between the largest binary32 and 2**128) and the
# largest value that does not; ties to even in the last binary32 place
SPECIAL = (np.nan, 0.0, 1e-40, 1e-45, 7e-46, 1e39, 3.4028235677973366e38, 3.4028234e38, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24)


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs():
    rng = np.random.default_rng(20260)
    values = [v for s in SPECIAL for v in (s, -s)]
    nrows = (len(values) + 1) // 2
    area = rng.uniform(500.0, 3100.0, NCELL)
    area[:nrows] = 1e6
    out = {}
    for k, var in enumerate(VARS):
        a = rng.gamma(2.0, 40.0, (NCELL, NMONTHS)) * 10.0 ** rng.integers(-3, 4, (NCELL, 1))
        a[rng.random(a.shape) < 0.02] = np.nan
        a[-1] = np.nan                                          # a cell without data
        a[:nrows] = np.nan
        a[:nrows, 0] = values[0::2]
        a[:nrows, 12] = (values[1::2] + [0.0])[:nrows]
        a[:nrows] = np.roll(a[:nrows], k, axis=0)               # not the same file three times
        out[var] = a
    basin_ids = rng.integers(1, 3, NCELL)                       # basins 1 and 2 have cells, basin 3 only a name
    return area, basin_ids, np.array(['Amazon', 'Baltic Sea', 'No cells']), out


def settings(folder, fmt, in_year, unit):
    return SimpleNamespace(
        output_vars=list(VARS), ProjectName=PROJECT, OutputNameStr=PROJECT, OutputFolder=folder, OutputFormat=fmt,
        OutputUnit=unit, OutputInYear=in_year, StartYear=START, EndYear=START + NMONTHS // 12 - 1,
        OutputUnitStr='{}per{}'.format(('mm', 'km3')[unit], ('month', 'year')[in_year]))


def read(path):
    with open(path, 'rb') as fh:
        return np.frombuffer(fh.read(), dtype=np.uint8)


def main():
    warnings.simplefilter('ignore', FutureWarning)              # DataFrame.groupby(axis=1) of agg_to_year
    ow = _load('ref_out_writer', 'xanthos/data_writer/out_writer.py')
    area, basin_ids, basin_names, arrays = inputs()
    fix = {'area': area, 'basin_ids': basin_ids, 'basin_names': basin_names}
    fix.update({'in_' + v: a for v, a in arrays.items()})
    with tempfile.TemporaryDirectory() as tmp:
        for case, (in_year, unit) in CASES.items():
            # MATLAB: the reference's write()
            s = settings(os.path.join(tmp, case + '_mat'), ow.FORMAT_MAT, in_year, unit)
            os.makedirs(s.OutputFolder)
            w = ow.OutWriter(s, area, {v: a.copy() for v, a in arrays.items()})
            w.write()
            for var in VARS:
                name = '{}_{}_{}'.format(var, 'm3persec' if var == 'avgchflow' else s.OutputUnitStr, PROJECT)
                fix['{}_{}_file'.format(case, var)] = np.array(name)
                fix['{}_{}_mat'.format(case, var)] = read(os.path.join(s.OutputFolder, name + '.mat'))
                fix['{}_{}_written'.format(case, var)] = np.array(w.get(var).values, dtype=np.float64)
            if case == 'm0':
                ref = SimpleNamespace(basin_ids=basin_ids, basin_names=basin_names)
                table = w.agg_spatial(w.get('q').copy(), ref.basin_ids, ref.basin_names, inc_name_idx=True)
                fix['basin_values'] = np.array(table.drop(columns='name').values, dtype=np.float64)
                w.write_aggregates(ref, w.get('q'), True, False, False)
                name = 'Basin_runoff_{}_{}'.format(s.OutputUnitStr, PROJECT)
                fix['basin_file'] = np.array(name)
                fix['basin_mat'] = read(os.path.join(s.OutputFolder, name + '.mat'))
            # NetCDF: write()'s steps (:102-125), then save_netcdf on the values
            s = settings(os.path.join(tmp, case + '_nc'), ow.FORMAT_NETCDF, in_year, unit)
            os.makedirs(s.OutputFolder)
            w = ow.OutWriter(s, area, {v: a.copy() for v, a in arrays.items()})
            for i, var in enumerate(w.output_names):
                flow = var == 'avgchflow'
                if w.output_in_year:
                    w.outputs[i] = w.agg_to_year(w.outputs[i], 'mean' if flow else 'sum')
                if w.out_unit == ow.UNIT_KM3_MTH and not flow:
                    w.outputs[i] = w.outputs[i].multiply(w.conversion_mm_km3, axis=0)
                name = '{}_{}_{}'.format(var, 'm3persec' if flow else w.out_unit_str, PROJECT)
                assert name == str(fix['{}_{}_file'.format(case, var)])
                values = np.array(w.outputs[i].values, dtype=np.float64)
                assert values.tobytes() == fix['{}_{}_written'.format(case, var)].tobytes()
                w.save_netcdf(os.path.join(s.OutputFolder, name), values, var)
                fix['{}_{}_nc'.format(case, var)] = read(os.path.join(s.OutputFolder, name + '.nc'))
    out = os.path.join(HERE, 'outfmt.npz')
    np.savez_compressed(out, **fix)
    print('wrote', out, os.path.getsize(out), 'bytes,', len(fix), 'arrays')


if __name__ == '__main__':
    main()
