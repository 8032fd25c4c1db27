"""GPU (-m gpu): OutputFormat 0 (NetCDF) and 2 (MATLAB) written from HBM.

xh_pack_f32_be against numpy's astype('>f4') byte for byte; OutWriter in both formats on the inputs of
tests/golden/outfmt.npz against the files the reference wrote (tests/golden/make_golden_outfmt.py), from host arrays and
from DeviceArrays, read back through the loader; run_model() and run_ensemble() in the formats against their own npy run.
tests/test_outfmt_host.py pins the numpy restatement and the headers without a GPU."""
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VARS = ('q', 'avgchflow', 'soilmoisture')
CASES = {'m0': (0, 0), 'y1': (1, 1)}                 # (OutputInYear, OutputUnit)
SPECIAL = (np.nan, 0.0, 1e-40, 1e-45, 7e-46, 1e39, 3.4028235677973366e38, 3.4028234e38, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24)
NC, CSV, MAT, NPY = 0, 1, 2, 4
EXT = {NC: '.nc', MAT: '.mat', NPY: '.npy'}


@pytest.fixture(scope='module')
def fix(golden):
    return golden('outfmt')


def be_f32(a):
    with np.errstate(over='ignore'):
        return np.ascontiguousarray(a, dtype=np.float64).astype('>f4').tobytes()


def read(path):
    with open(path, 'rb') as fh:
        return fh.read()


# ---- the kernel alone
@pytest.mark.parametrize('shape', [(1, 1), (5, 3), (67, 24), (1000, 36)])
def test_pack_f32_be_equals_numpy(shape):
    """(1, 1): the tail alone; (5, 3): three quads and a tail of three; (1000, 36): more workgroups than one round of the
    grid-stride loop of a single one.  The special values and their negatives lead, random values of every binary32
    exponent (and beyond, on both sides) follow."""
    from xanthos_amd import _hip
    ctx = _hip.get_context(0)
    rng = np.random.default_rng(shape[0])
    n = shape[0] * shape[1]
    a = rng.standard_normal(n) * 10.0 ** rng.integers(-50, 42, n)
    special = np.array([v for s in SPECIAL for v in (s, -s)])
    k = min(n, special.size)
    a[:k] = special[(shape[0] % special.size + np.arange(k)) % special.size]      # (a different one leads at every shape)
    a = a.reshape(shape)
    src, dst = ctx.upload(a), ctx.empty((n,), dtype=np.uint32)
    try:
        ctx.pack_f32_be(src, n, dst)
        assert dst.download().tobytes() == be_f32(a)
        if n > 1:         # a row slice: the source 8-byte but not 16-byte aligned, a quad fewer or a tail of another length
            dst.zero()
            ctx.pack_f32_be(src.ptr + 8, n - 1, dst)
            got = dst.download().tobytes()
            assert got[:4 * (n - 1)] == be_f32(a.ravel()[1:]) and got[4 * (n - 1):] == b'\x00' * 4
        with pytest.raises(_hip.HipError, match='aligned'):
            ctx.pack_f32_be(src, n, dst.ptr + 4)
    finally:
        src.free()
        dst.free()


# ---- the writer on the golden inputs
def settings(folder, fmt, case, **extra):
    in_year, unit = CASES[case]
    return SimpleNamespace(output_vars=list(VARS), ProjectName='golden', OutputFolder=str(folder), OutputFormat=fmt,
                           OutputUnit=unit, OutputInYear=in_year, StartYear=2000, EndYear=2001, device=0, **extra)


@pytest.mark.parametrize('device', [False, True], ids=['host', 'hbm'])
@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('fmt', [NC, MAT], ids=['nc', 'mat'])
def test_writer_equals_the_reference_files(fix, tmp_path, fmt, case, device):
    from xanthos_amd import _hip, data_load
    from xanthos_amd.data_writer.out_writer import OutWriter
    ctx = _hip.get_context(0)
    inputs = {v: (ctx.upload(fix['in_' + v]) if device else fix['in_' + v].copy()) for v in VARS}
    w = OutWriter(settings(tmp_path, fmt, case), fix['area'], inputs)
    w.write()
    assert w._bodies_from_device is None and sorted(os.listdir(str(tmp_path))) == sorted(
        str(fix['{}_{}_file'.format(case, v)]) + EXT[fmt] for v in VARS)
    for var in VARS:
        written = fix['{}_{}_written'.format(case, var)]
        path = os.path.join(str(tmp_path), str(fix['{}_{}_file'.format(case, var)]) + EXT[fmt])
        got, ref = read(path), fix['{}_{}_{}'.format(case, var, EXT[fmt][1:])].tobytes()
        skip = 0 if fmt == NC else 116                           # the text with the time of writing
        assert len(got) == len(ref) and got[skip:] == ref[skip:], (var, path)
        back = data_load.load_file(path, key='data' if fmt == NC else var)
        if fmt == NC:
            assert back.dtype.itemsize == 4 and back.shape == written.shape and back.astype('>f4').tobytes() == be_f32(written)
        else:
            assert back.dtype == np.float64 and back.shape == written.shape and back.tobytes() == written.tobytes()
        assert w.get(var).tobytes() == written.tobytes()          # the array as written, for the caller
    if device:
        for a in inputs.values():
            a.free()


def test_writer_tables_with_names_and_refusals(fix, tmp_path):
    """write_aggregates under MATLAB: the cell array the reference wrote; a table without names and a single array
    outside write() (the ensemble statistics' route) go out at once; NetCDF refuses a name column."""
    from scipy import io as spio
    from xanthos_amd.data_writer.out_writer import OutWriter
    from xanthos_amd.ini_reader import ValidationException
    w = OutWriter(settings(tmp_path, MAT, 'm0', AggregateRunoffBasin=1), fix['area'], {'q': fix['in_q'].copy()})
    w.write()
    ref_data = SimpleNamespace(basin_ids=fix['basin_ids'], basin_names=[str(n) for n in fix['basin_names']])
    out = w.write_aggregates(ref_data, w.get('q'), True, False, False)
    assert out['Basin_runoff'].tobytes() == fix['basin_values'].tobytes()
    got = spio.loadmat(os.path.join(str(tmp_path), str(fix['basin_file']) + '.mat'))['Basin_runoff']
    ref = spio.loadmat(io.BytesIO(fix['basin_mat'].tobytes()))['Basin_runoff']
    assert got.shape == ref.shape and all(g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes()
                                          for g, r in zip(got.ravel(), ref.ravel()))
    for fmt in (NC, MAT):
        w = OutWriter(settings(tmp_path, fmt, 'm0'), fix['area'], {})
        dev = w.ctx.upload(fix['in_q'])
        w.write_data(os.path.join(str(tmp_path), 'q_stat'), 'q', dev, w.time_steps)
        dev.free()
        body = read(os.path.join(str(tmp_path), 'q_stat' + EXT[fmt]))
        assert body.endswith(be_f32(fix['in_q']) if fmt == NC else fix['in_q'].tobytes(order='F'))
    with pytest.raises(ValidationException, match='name'):
        w = OutWriter(settings(tmp_path, NC, 'm0'), fix['area'], {})
        w.write_data(os.path.join(str(tmp_path), 'table'), 'Basin_runoff', fix['basin_values'], w.time_steps, names=['a', 'b', 'c'])


# ---- whole runs
def run_outputs(folder, fmt):
    """{file name without extension: the array it holds (NetCDF: its values as big-endian bytes)} of the files of format ``fmt``."""
    from scipy import io as spio
    from xanthos_amd import data_load
    out = {}
    for name in sorted(os.listdir(folder)):
        stem, ext = os.path.splitext(name)
        if ext != EXT[fmt]:
            continue
        path = os.path.join(folder, name)
        if fmt == NPY:
            out[stem] = np.load(path)
        elif fmt == MAT:
            out[stem] = spio.loadmat(path)[stem.split('_')[0]]
        else:
            values = data_load.load_file(path, key='data')
            assert values.dtype.itemsize == 4 and os.path.getsize(path) > values.size * 4
            out[stem] = values.astype('>f4').tobytes()
    return out


def same_as_npy(got, ref, fmt, tag):
    assert sorted(got) == sorted(ref) and ref, (tag, sorted(got), sorted(ref))
    for stem, a in ref.items():
        if fmt == NC:
            assert got[stem] == be_f32(a), (tag, stem)
        else:
            assert got[stem].dtype == np.float64 and got[stem].shape == a.shape and got[stem].tobytes() == a.tobytes(), (tag, stem)


def test_run_model_in_every_array_format(tmp_path):
    """An ini with OutputFormat 0 or 2 runs through run_model() and holds what the npy run holds."""
    from xanthos_amd import run_model, synth
    w = synth.make_world(nrow=36, ncol=72, ncell=900, n_basins=7, seed=33)
    f = synth.make_forcing(w, 36)
    files = {}
    for fmt in (NPY, NC, MAT):
        root = str(tmp_path / 'fmt{}'.format(fmt))
        ini = synth.write_example(root, w, f, 1971, 1973, runoff_spinup=25, routing_spinup=6, output_format=fmt,
                                  output_vars=('q', 'avgchflow', 'soilmoisture'))
        run_model(ini)
        files[fmt] = run_outputs(os.path.join(root, 'output', 'pm_abcd_mrtm_synth'), fmt)
    assert len(files[NPY]) == 3 and files[NPY]['q_mmpermonth_pm_abcd_mrtm_synth'].shape == (900, 36)
    same_as_npy(files[NC], files[NPY], NC, 'NetCDF')
    same_as_npy(files[MAT], files[NPY], MAT, 'MATLAB')


def test_run_ensemble_in_netcdf(tmp_path):
    """Two members, statistics = mean, OutputFormat 0: the member files and ensemble/ hold what the npy run holds."""
    from xanthos_amd import run_ensemble, synth
    w = synth.make_world(nrow=36, ncol=72, ncell=900, n_basins=7, seed=31)
    forcings = [synth.make_forcing(w, 36, seed=100 + 7 * k) for k in range(2)]
    files = {}
    for fmt in (NPY, NC):
        root = str(tmp_path / 'fmt{}'.format(fmt))
        ini, _ = synth.write_ensemble_example(root, w, forcings, 1971, 1973, runoff_spinup=25, routing_spinup=6,
                                              statistics=('mean',), output_format=fmt)
        res = run_ensemble(ini)
        out = os.path.join(root, 'output', 'pm_abcd_mrtm_synth')
        assert sorted(os.listdir(out)) == ['ensemble', 'logfile.log', 'm00', 'm01'] and len(res.names) == 2
        files[fmt] = {d: run_outputs(os.path.join(out, d), fmt) for d in ('m00', 'm01', 'ensemble')}
    assert sorted(files[NPY]['ensemble']) == ['avgchflow_m3persec_pm_abcd_mrtm_synth_mean', 'q_mmpermonth_pm_abcd_mrtm_synth_mean']
    for d in files[NPY]:
        same_as_npy(files[NC][d], files[NPY][d], NC, d)
