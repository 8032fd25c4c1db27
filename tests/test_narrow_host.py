"""CPU-only checks of the stored-forcing path: the NetCDF-classic header reader against scipy's files and the project's own
writer, the loader's memory maps of .nc variables, the rule by which load_to_array keeps an array as stored, the C-ABI
entry, and the ensemble's refusal of a mis-shaped .nc member before any GPU work."""
import os

import numpy as np
import pytest
import scipy.io as sio

from xanthos_amd import _hip, ensemble, nc_header, synth
from xanthos_amd.data_load import DataLoader, load_file, stored_kind
from xanthos_amd.ini_reader import ConfigReader, ValidationException

NM = 36


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.dtype('u{}'.format(a.dtype.itemsize)).newbyteorder(a.dtype.byteorder))


def mapped(path, key):
    where = nc_header.variable_range(path, key)
    assert where is not None, key
    dtype, shape, offset = where
    return np.memmap(path, dtype=dtype, mode='r', offset=offset, shape=shape)


def same_as_scipy(path, key):
    """The map at the returned range against scipy's own view of the variable, bit for bit."""
    grp = sio.netcdf_file(path, 'r', mmap=False)
    ref = grp.variables[key][:].copy()
    grp.close()
    got = mapped(path, key)
    assert got.dtype == ref.dtype and got.dtype.byteorder == '>' and got.shape == ref.shape, key
    assert np.array_equal(bits(got), bits(ref)), key
    return got


def write_nc(path, variables, version=1, attrs=(), record=None):
    """variables: [(name, type, dims, values, {attribute: value})]; record: (name, values [nrec, x]) over an unlimited dim."""
    f = sio.netcdf_file(path, 'w', version=version)
    for k, v in attrs:
        setattr(f, k, v)
    made = {}
    if record is not None:
        f.createDimension('time', None)
    for name, typ, values, vattrs in variables:
        dims = []
        for axis, n in enumerate(values.shape):
            d = 'd{}'.format(n)
            if d not in made:
                f.createDimension(d, n)
                made[d] = n
            dims.append(d)
        var = f.createVariable(name, typ, tuple(dims))
        var[:] = values
        for k, v in vattrs.items():
            setattr(var, k, v)
    if record is not None:
        name, values = record
        d = 'd{}'.format(values.shape[1])
        if d not in made:
            f.createDimension(d, values.shape[1])
        var = f.createVariable(name, 'f4', ('time', d))
        for k in range(values.shape[0]):
            var[k] = values[k]
    f.close()


def awkward(shape, seed):
    """Values with NaN, infinities, signed zeros and single-precision subnormals among them."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape) * 10.0 ** rng.integers(-30, 30, shape)
    flat = a.reshape(-1)
    flat[:6] = [np.nan, np.inf, -np.inf, -0.0, 1e-40, -1e-45]
    return a


# ------------------------------------------------------------------ nc_header
def test_one_f4_variable(tmp_path):
    p = str(tmp_path / 'one.nc')
    write_nc(p, [('pr', 'f4', awkward((11, 7), 1).astype('f4'), {})])
    got = same_as_scipy(p, 'pr')
    assert got.dtype == np.dtype('>f4') and got.shape == (11, 7)


@pytest.mark.parametrize('version', [1, 2])
def test_mixed_variables_and_odd_attributes(tmp_path, version):
    """Three variables of f4 / f8 / i2 with global and per-variable attributes of lengths 1, 2, 3 and 5 (the 4-byte padding of
    names and values), in both header versions (version 2: 64-bit offsets)."""
    p = str(tmp_path / 'mixed.nc')
    write_nc(p, [('a', 'f4', awkward((5, 3), 2).astype('f4'), {'u': 'x', 'long_name_': 'abcde'}),
                 ('count', 'i2', np.arange(7, dtype='i2'), {'k': np.int16(3)}),
                 ('bb', 'f8', awkward((3, 5), 3), {'units': 'mm', 'scale': np.array([1.5, 2.5, 3.5])})],
             version=version, attrs=(('history', 'abc'), ('t', 'ab'), ('n', np.int32(7)), ('odd', np.array([1, 2, 3], dtype='i2'))))
    assert open(p, 'rb').read(4) == b'CDF' + bytes([version])
    same_as_scipy(p, 'a')
    assert same_as_scipy(p, 'bb').dtype == np.dtype('>f8')
    assert nc_header.variable_range(p, 'count') is None            # i2: another type
    assert nc_header.variable_range(p, 'missing') is None and nc_header.variable_range(p, None) is None


def test_record_variable_other_formats_and_truncated_header(tmp_path):
    p = str(tmp_path / 'rec.nc')
    write_nc(p, [('fixed', 'f4', awkward((4, 5), 4).astype('f4'), {})], record=('series', np.arange(15.0).reshape(3, 5)))
    assert nc_header.variable_range(p, 'series') is None           # a record variable: its records interleave
    same_as_scipy(p, 'fixed')                                      # ... the fixed-size variable beside it is one block
    raw = open(p, 'rb').read()
    where = nc_header.variable_range(p, 'fixed')
    for cut in (0, 3, 4, 8, 30, where[2] - 4, where[2] + 7):       # inside the magic, the lists, the last begin, the data
        q = str(tmp_path / 'cut{}.nc'.format(cut))
        with open(q, 'wb') as fh:
            fh.write(raw[:cut])
        assert nc_header.variable_range(q, 'fixed') is None, cut
    for magic in (b'CDF\x05', b'\x89HDF\r\n\x1a\n', b'NUMPY'):
        q = str(tmp_path / 'other.nc')
        with open(q, 'wb') as fh:
            fh.write(magic + raw[len(magic):])
        assert nc_header.variable_range(q, 'fixed') is None, magic
    assert nc_header.variable_range(str(tmp_path / 'absent.nc'), 'fixed') is None


def test_file_of_the_projects_own_writer(tmp_path):
    """data_writer/formats.nc_header + the body as the device writes it (astype('>f4')): the reader is its mirror."""
    from xanthos_amd.data_writer.formats import nc_header as write_header
    a = awkward((13, 5), 5)
    p = str(tmp_path / 'own.nc')
    with open(p, 'wb') as fh:
        fh.write(write_header(13, 5, False, 'mmpermonth', 'q') + a.astype('>f4').tobytes())
    got = same_as_scipy(p, 'data')
    assert np.array_equal(bits(got), bits(a.astype('>f4')))
    assert nc_header.variable_range(p, 'data')[2] == len(write_header(13, 5, False, 'mmpermonth', 'q'))


# ------------------------------------------------------------------ load_file
def test_load_file_maps_a_netcdf_variable(tmp_path):
    p = str(tmp_path / 'f.nc')
    a4, a8 = awkward((9, 4), 6).astype('f4'), awkward((9, 4), 7)
    write_nc(p, [('a4', 'f4', a4, {}), ('a8', 'f8', a8, {}), ('n', 'i2', np.arange(4, dtype='i2'), {})],
             record=('rec', np.ones((2, 4))))
    for key, ref in (('a4', a4), ('a8', a8)):
        eager = load_file(p, key=key, mmap=False)
        assert type(eager) is np.ndarray and eager.dtype == ref.dtype and eager.dtype.isnative and eager.flags.writeable
        assert np.array_equal(bits(eager), bits(ref))             # what it returned before: native order, a host copy
        assert np.array_equal(bits(load_file(p, key=key)), bits(ref))
        lazy = load_file(p, key=key, mmap=True)
        assert isinstance(lazy, np.memmap) and lazy.dtype.byteorder == '>' and not lazy.flags.writeable
        assert np.array_equal(bits(lazy.astype(ref.dtype)), bits(eager))
        assert stored_kind(lazy) == _hip.NARROW_KINDS[np.dtype('>f' + str(ref.dtype.itemsize))]
    for key in ('n', 'rec'):                                       # no range: today's path, today's values
        assert np.array_equal(load_file(p, key=key, mmap=True), load_file(p, key=key, mmap=False))
        assert not isinstance(load_file(p, key=key, mmap=True), np.memmap)
    with pytest.raises(KeyError):
        load_file(p, key='missing', mmap=True)


def test_stored_kind():
    a = np.zeros((4, 3), dtype=np.float32)
    assert stored_kind(a) == (_hip.XH_SRC_F32_LE, 'f32') and stored_kind(a.astype('>f4')) == (_hip.XH_SRC_F32_BE, 'f32be')
    assert stored_kind(a.astype('>f8')) == (_hip.XH_SRC_F64_BE, 'f64be')
    for other in (a.astype(np.float64), a.astype(np.float16), a.astype('i4'), a[:, :2], a.T, a[0], a.tolist(), None):
        assert stored_kind(other) is None


# ------------------------------------------------------------------ load_to_array
@pytest.fixture(scope='module')
def trees(tmp_path_factory):
    """pm + abcd + mrtm with float32 .npy forcing, and hargreaves + abcd + mrtm with its four forcing files as NetCDF
    `float` variables; every value representable in single precision."""
    root = str(tmp_path_factory.mktemp('narrow_host'))
    w = synth.make_world(nrow=12, ncol=24, ncell=60, n_basins=3, seed=3)
    f = {k: v.astype(np.float32) for k, v in synth.make_forcing(w, NM, seed=50).items()}
    pm_ini = synth.write_example(os.path.join(root, 'pm'), w, f, 1971, 1973, runoff_spinup=25, routing_spinup=6)
    h = synth.hgm_forcing(w, f)
    hg_root = os.path.join(root, 'hg')
    hg_ini = synth.write_hgm_example(hg_root, w, h, 1971, 1973, runoff='abcd', runoff_spinup=25, routing_spinup=6)
    hg_ini = nc_forced(hg_ini, hg_root, h, 'f4')
    return w, f, h, pm_ini, hg_ini


NC_FILES = {'temp': ('TemperatureFile', 'TempVarName', 'tas'), 'dtr': ('DailyTemperatureRangeFile', 'DTRVarName', 'dtr'),
            'precip': ('PrecipitationFile', 'PrecipVarName', 'pr'), 'abcd_tmin': ('TempMinFile', 'TempMinVarName', 'tmin')}


def nc_forced(ini, root, forcing, typ):
    """A copy of a write_hgm_example(runoff='abcd') ini whose four forcing files are NetCDF variables of type ``typ``."""
    import re
    text = open(ini).read()
    for key, (setting, varname, var) in NC_FILES.items():
        path = os.path.join(root, 'input', var + '_' + typ + '.nc')
        write_nc(path, [(var, typ, np.asarray(forcing[key]).astype(typ), {'units': 'x'})], attrs=(('title', 'abc'),))
        text = re.sub(r'(?m)^{} = .*$'.format(setting), '{} = {}\n{} = {}'.format(setting, path, varname, var), text)
    out = ini.replace('.ini', '_nc_{}.ini'.format(typ))
    with open(out, 'w') as fh:
        fh.write(text)
    return out


def off_the_device_path(s, how):
    if how == 'calibrate':
        s.calibrate = 1
        s.cal_observed = s.cal_gauges = None
    elif how == 'stage_by_stage':
        s.runoff_module = 'none'                                   # PM without ABCD runs stage by stage on host arrays
    elif how == 'device_transforms':
        s.device_transforms = False
    elif how == 'mmap_inputs':
        s.mmap_inputs = False
    return s


HOW = ('calibrate', 'stage_by_stage', 'device_transforms', 'mmap_inputs')


def test_load_to_array_keeps_f4_npy_as_stored(trees):
    w, f, h, pm_ini, hg_ini = trees
    d = DataLoader(ConfigReader(pm_ini))
    for attr, key in (('tair_load', 'tas'), ('rlds_load', 'rlds'), ('precip', 'precip'), ('tmin', 'abcd_tmin')):
        a = getattr(d, attr)
        assert isinstance(a, np.memmap) and a.dtype == np.float32 and not a.flags.writeable, attr
        assert np.array_equal(bits(a), bits(f[key])), attr
    assert np.array_equal(d.tairprev_load[1:], np.nan_to_num(f['tas'][:-1].astype(np.float64)))      # built in double precision
    for how in HOW:
        d = DataLoader(off_the_device_path(ConfigReader(pm_ini), how))
        for attr, key, clean in (('tair_load', 'tas', True), ('rlds_load', 'rlds', True)) + (
                () if how == 'stage_by_stage' else (('precip', 'precip', False), ('tmin', 'abcd_tmin', True))):
            a, ref = getattr(d, attr), f[key].astype(np.float64)
            if how == 'device_transforms' and clean:
                ref = np.nan_to_num(ref)
            assert a.dtype == np.float64 and a.dtype.isnative and np.array_equal(bits(a), bits(ref)), (how, attr)


def test_load_to_array_keeps_f4_nc_as_stored(trees):
    w, f, h, pm_ini, hg_ini = trees
    d = DataLoader(ConfigReader(hg_ini))
    for attr, key in (('temp', 'temp'), ('dtr', 'dtr'), ('precip', 'precip'), ('tmin', 'abcd_tmin')):
        a = getattr(d, attr)
        assert isinstance(a, np.memmap) and a.dtype == np.dtype('>f4') and a.shape == (w.ncell, NM), attr
        assert np.array_equal(bits(a.astype('<f4')), bits(h[key])), attr
    for how in ('calibrate', 'device_transforms', 'mmap_inputs'):
        d = DataLoader(off_the_device_path(ConfigReader(hg_ini), how))
        for attr, key in (('temp', 'temp'), ('dtr', 'dtr'), ('precip', 'precip'), ('tmin', 'abcd_tmin')):
            a, ref = getattr(d, attr), h[key].astype(np.float64)
            if how == 'device_transforms' and attr == 'tmin':
                ref = np.nan_to_num(ref)
            assert a.dtype == np.float64 and a.dtype.isnative and np.array_equal(bits(a), bits(ref)), (how, attr)
    # the shape check and its message are unchanged
    s = ConfigReader(hg_ini)
    s.nmonths = NM + 12
    with pytest.raises(ValidationException, match=r'Inconsistent TemperatureFile data grid size. Expecting size: \(60, 48\). '
                                                  r'Received size: \(60, 36\)'):
        DataLoader(s)


def test_load_to_array_keeps_an_in_memory_float32_array(trees):
    w, f, h, pm_ini, hg_ini = trees
    s = ConfigReader(pm_ini)
    s.update({'PrecipitationFile': f['precip'], 'pm_tas': np.asfortranarray(f['tas'])})      # (the second: not C-contiguous)
    d = DataLoader(s)
    assert d.precip is f['precip']
    assert d.tair_load.dtype == np.float64 and np.array_equal(bits(d.tair_load), bits(f['tas'].astype(np.float64)))
    for how in HOW[:1] + HOW[2:]:
        s = off_the_device_path(ConfigReader(pm_ini), how)
        s.update({'PrecipitationFile': f['precip']})
        d = DataLoader(s)
        assert d.precip.dtype == np.float64 and np.array_equal(bits(d.precip), bits(f['precip'].astype(np.float64))), how


# ------------------------------------------------------------------ pipeline plumbing, C-ABI, ensemble
def test_file_range_of_stored_maps(trees, tmp_path):
    from xanthos_amd.pipeline import file_range_of
    w, f, h, pm_ini, hg_ini = trees
    d = DataLoader(ConfigReader(hg_ini))
    for a in (d.precip, d.precip[7:]):
        assert file_range_of(a) is None                            # float64 maps only, unless asked
        path, off = file_range_of(a, stored=True)
        raw = open(path, 'rb').read()[off:off + a.nbytes]
        assert np.array_equal(bits(np.frombuffer(raw, dtype='>f4').reshape(a.shape)), bits(a))
    np.save(str(tmp_path / 'f4.npy'), f['tas'])
    mm = np.load(str(tmp_path / 'f4.npy'), mmap_mode='r')
    assert file_range_of(mm, stored=True) == (str(tmp_path / 'f4.npy'), mm.offset)
    assert file_range_of(f['tas'], stored=True) is None and file_range_of(mm.astype('f2'), stored=True) is None


def test_library_exports_xh_widen():
    assert _hip.SIGNATURES['xh_widen'][1] == [_hip._P, _hip._P, _hip.c_int, _hip.c_int64, _hip._P]
    assert hasattr(_hip.lib(), 'xh_widen') and _hip.lib().xh_abi_version() == 7
    assert (_hip.XH_SRC_F32_LE, _hip.XH_SRC_F32_BE, _hip.XH_SRC_F64_BE) == (1, 2, 3)
    assert callable(_hip.Context.widen)
    if _hip.device_count() == 0:                                   # argument errors need no device, but a context does
        with pytest.raises(_hip.HipUnavailable):
            _hip.Context(0)


def test_ensemble_refuses_a_misshaped_nc_member_before_any_context(trees, tmp_path, monkeypatch):
    w, f, h, pm_ini, hg_ini = trees
    monkeypatch.setattr(_hip, 'get_context', lambda *a, **k: pytest.fail('a context was made'))
    monkeypatch.setattr(_hip, 'Context', lambda *a, **k: pytest.fail('a context was made'))
    s = ConfigReader(hg_ini)
    good, bad = str(tmp_path / 'good.nc'), str(tmp_path / 'bad.nc')
    write_nc(good, [('pr', 'f4', h['precip'], {})])
    write_nc(bad, [('pr', 'f4', h['precip'][:, :24], {})])
    plan = ensemble.validate(s, [('ok', {'PrecipitationFile': good})], member_outputs=1)
    base = 8 * w.ncell * 2 * NM * (4 + 6)
    assert plan.bytes_needed == base + 4 * w.ncell * NM             # the scratch of single-precision uploads is counted
    with pytest.raises(ValidationException) as exc:
        ensemble.run(s, members=[('ok', {'PrecipitationFile': good}), ('short', {'PrecipitationFile': bad})], member_outputs=1)
    msg = str(exc.value)
    assert "'short'" in msg and 'PrecipitationFile' in msg and '(60, 24)' in msg and '(60, 36)' in msg, msg
    # a float64 ensemble needs what it needed before
    s64 = ConfigReader(pm_ini)
    arr = {k: np.zeros((w.ncell, NM)) for k in ('PrecipitationFile',)}
    for key in ('pm_tas', 'pm_tmin', 'pm_rhs', 'pm_wind', 'pm_rsds', 'pm_rlds', 'PrecipitationFile', 'TempMinFile'):
        setattr(s64, key, np.zeros((w.ncell, NM)))
    assert ensemble.validate(s64, [('m', arr)]).bytes_needed == 8 * w.ncell * 2 * NM * (8 + 6)
