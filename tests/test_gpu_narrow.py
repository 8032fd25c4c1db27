"""GPU tests (-m gpu) of forcing sent as it is stored: xh_widen against numpy's astype(np.float64) bit for bit (every binary32
exponent, the subnormal edges, zeros, infinities, NaNs, random patterns; tails, several sweeps of the grid, unaligned slices,
guards), its argument checks, DevicePipeline.set_forcing from float32 / NetCDF maps against the same call on doubles, and
whole runs and ensembles whose single-precision and NetCDF forcing must write the files of their float64 twins."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.io as sio

pytestmark = pytest.mark.gpu

KINDS = {'f32': 1, 'f32be': 2, 'f64be': 3}
SENTINEL = -1234.5
BIG = 67420 * 70            # more quads than one sweep of the grid-stride loop has lanes (16 x 256 CUs x 256)


@pytest.fixture(scope='module')
def ctx():
    from xanthos_amd import _hip
    return _hip.get_context(0)


def patterns32():
    """Every binary32 exponent x both signs x the mantissas at the edges (all subnormal edges, +-0, +-inf, quiet and
    signalling NaNs), then 100,000 random bit patterns."""
    exp = np.arange(256, dtype=np.uint32)[:, None, None] << np.uint32(23)
    sign = np.array([0, 1], dtype=np.uint32)[None, :, None] << np.uint32(31)
    mant = np.array([0, 1, 2, 0x3fffff, 0x400000, 0x400001, 0x7ffffe, 0x7fffff], dtype=np.uint32)[None, None, :]
    edges = (exp | sign | mant).reshape(-1)
    rnd = np.random.default_rng(20240807).integers(0, 1 << 32, 100000, dtype=np.uint32)
    return np.concatenate([edges, rnd])


def patterns64():
    """The same values widened, then 100,000 random 64-bit patterns."""
    with np.errstate(invalid='ignore'):                            # (signalling NaNs among them)
        wide = patterns32().view(np.float32).astype(np.float64).view(np.uint64)
    rnd = np.random.default_rng(20240808).integers(0, 1 << 64, 100000, dtype=np.uint64)
    return np.concatenate([wide, rnd])


def stored(kind, n):
    """(bytes as stored [uint8], expected doubles as uint64 bits, NaN mask or None) of ``n`` values of ``kind``."""
    if kind == 'f64be':
        want = np.resize(patterns64(), n)
        return want.astype('>u8').view(np.uint8), want, None
    bits32 = np.resize(patterns32(), n)
    with np.errstate(invalid='ignore'):
        want = bits32.view(np.float32).astype(np.float64)
    raw = bits32.astype('>u4' if kind == 'f32be' else '<u4').view(np.uint8)
    return raw, want.view(np.uint64), np.isnan(want)


def check(got, want, nan, tag):
    got = got.view(np.uint64)
    if nan is None:                                                # a swap: raw bits, no NaN caveat
        assert np.array_equal(got, want), tag
        return
    assert np.array_equal(np.isnan(got.view(np.float64)), nan), ('NaN for NaN', tag)
    assert np.array_equal(got[~nan], want[~nan]), (tag, int((got[~nan] != want[~nan]).sum()))


def run_widen(ctx, kind, n, src_off=0, dst_off=0):
    """xh_widen of n values whose source starts ``src_off`` elements and whose destination ``dst_off`` doubles behind a
    16-byte boundary, between two guard doubles; returns the n doubles."""
    raw, want, nan = stored(kind, n)
    width = 8 if kind == 'f64be' else 4
    d_src = ctx.upload(np.concatenate([np.zeros(src_off * width, np.uint8), raw, np.zeros(16, np.uint8)]), dtype=np.uint8)
    lead = 2 + dst_off                                             # doubles in front: index lead - 1 is the guard
    d_dst = ctx.upload(np.full(lead + n + 1, SENTINEL))
    ctx.widen(d_src.ptr + src_off * width if n else None, KINDS[kind], n, d_dst.ptr + 8 * lead if n else None)
    out = d_dst.download()
    d_src.free()
    d_dst.free()
    assert (out[:lead] == SENTINEL).all() and out[lead + n] == SENTINEL, ('guards', kind, n, src_off, dst_off)
    check(out[lead:lead + n], want, nan, (kind, n, src_off, dst_off))
    return out[lead:lead + n]


# ------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('kind', sorted(KINDS))
def test_kernel_bits(ctx, kind):
    """All 104,096 binary32 patterns (and for '>f8' 100,000 random 64-bit ones more) against numpy, bit for bit."""
    n = patterns64().size if kind == 'f64be' else patterns32().size
    assert n == (204096 if kind == 'f64be' else 104096)
    got = run_widen(ctx, kind, n)
    if kind != 'f64be':
        p = patterns32()
        at = int(np.flatnonzero(p == 0x7fc00000)[0])
        assert got.view(np.uint64)[at] == 0x7ff8000000000000       # the default quiet NaN
        sub = ((p & 0x7f800000) == 0) & ((p & 0x7fffff) != 0)
        assert sub.sum() >= 12 and (got[sub] != 0).all()           # subnormals are widened, not flushed
        zero = (p & 0x7fffffff) == 0
        assert np.array_equal(np.signbit(got[zero]), (p[zero] >> 31).astype(bool))


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_shapes_tails_and_unaligned_slices(ctx, kind):
    for n in (0, 1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025):
        ref = run_widen(ctx, kind, n)
        for src_off, dst_off in ((1, 0), (0, 1), (1, 1)):          # the instantiation for element-aligned slices
            got = run_widen(ctx, kind, n, src_off, dst_off)
            assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (kind, n, src_off, dst_off)


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_more_than_one_sweep_of_the_grid(ctx, kind):
    assert (BIG >> 2) > 16 * ctx.cu_count() * 256                  # lanes of the capped grid
    ref = run_widen(ctx, kind, BIG)
    got = run_widen(ctx, kind, BIG, 1, 1)
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))


def test_arguments(ctx):
    from xanthos_amd import _hip
    n = 1024
    d_src = ctx.upload(stored('f32', 2 * n + 8)[0], dtype=np.uint8)
    before = np.full(n + 8, SENTINEL)
    d_dst = ctx.upload(before)

    def refused(word, src, kind, count, dst):
        with pytest.raises(_hip.HipError, match='error {}'.format(_hip.XH_ERR_ARG)) as exc:
            ctx.widen(src, kind, count, dst)
        assert word in str(exc.value), str(exc.value)
        assert np.array_equal(d_dst.download(), before), word      # nothing was launched
    for kind in (0, 4, -1):
        refused('unknown kind', d_src, kind, n, d_dst)
    refused('bad argument', d_src, 1, -1, d_dst)
    refused('bad argument', None, 1, n, d_dst)
    refused('bad argument', d_src, 1, n, None)
    refused('aligned', d_src.ptr + 2, 1, n, d_dst)                  # a float32 source on an odd half-word
    refused('aligned', d_src.ptr + 4, 3, n, d_dst)                  # a float64 source on a word
    refused('aligned', d_src, 2, n, d_dst.ptr + 4)
    # overlaps: single precision inside its own destination (front, back), '>f8' one double apart
    refused('overlap', d_dst, 1, n, d_dst)
    refused('overlap', d_dst.ptr + 4 * n, 2, n, d_dst)
    refused('overlap', d_dst.ptr + 8 * n - 4, 1, n, d_dst)
    refused('overlap', d_dst.ptr + 8, 3, n, d_dst)
    refused('overlap', d_dst, 3, n, d_dst.ptr + 8)
    ctx.widen(None, 1, 0, None)                                    # n == 0: NULL is fine, nothing to do
    ctx.widen(d_dst.ptr + 8 * n, 1, 2, d_dst)                       # touching ranges do not overlap
    assert np.array_equal(d_dst.download()[2:], before[2:])
    # '>f8' in place
    raw, want, _ = stored('f64be', n + 3)
    d_io = ctx.upload(raw, dtype=np.uint8)
    ctx.widen(d_io, 3, n + 3, d_io)
    assert np.array_equal(d_io.download().view(np.uint64), want)
    for a in (d_src, d_dst, d_io):
        a.free()


# ------------------------------------------------------------------ set_forcing
WORLD = dict(nrow=36, ncol=72, ncell=900, n_basins=7)
NM = 36
NAMES = ('tas', 'tmin', 'rhs', 'wind', 'rsds', 'rlds', 'precip', 'abcd_tmin')


def holed_forcing(w, seed=61):
    """make_forcing with NaN holes in every array (the six PM arrays and abcd_tmin lose them on the device)."""
    from xanthos_amd import synth
    f = synth.make_forcing(w, NM, seed=seed)
    for i, k in enumerate(NAMES):
        f[k] = np.array(f[k], dtype=np.float64)
        f[k].reshape(-1)[11 + 7 * i::997] = np.nan
    return f


def write_nc(path, var, values, typ):
    g = sio.netcdf_file(path, 'w')
    g.title = 'abc'
    g.createDimension('index', values.shape[0])
    g.createDimension('month', values.shape[1])
    v = g.createVariable(var, typ, ('index', 'month'))
    v[:] = values
    v.units = 'x'
    g.close()


def sources(root, f):
    """form -> {forcing name: array as DataLoader would keep it}."""
    from xanthos_amd.data_load import load_file
    out = {'f32': {}, 'f32be': {}, 'f64be': {}, 'memory': {}}
    for k in NAMES:
        np.save(os.path.join(root, k + '_f4.npy'), f[k].astype(np.float32))
        out['f32'][k] = load_file(os.path.join(root, k + '_f4.npy'), mmap=True)
        for form, typ in (('f32be', 'f4'), ('f64be', 'f8')):
            path = os.path.join(root, '{}_{}.nc'.format(k, typ))
            write_nc(path, k, f[k], typ)
            out[form][k] = load_file(path, key=k, mmap=True)
            assert isinstance(out[form][k], np.memmap) and out[form][k].dtype == np.dtype('>' + typ)
        out['memory'][k] = f[k].astype(np.float32)
    return out


def check_set_forcing(root, expect_file_uploads=None):
    """Every form of source through set_forcing against set_forcing of src.astype(np.float64), bit for bit; also the body
    of the XH_UPLOAD_FROM_FILE=1 child (``expect_file_uploads``: xh_upload_file calls to expect per mapped form)."""
    from xanthos_amd import _hip, synth
    from xanthos_amd.pipeline import pipeline_from_world
    ctx = _hip.get_context(0)
    w = synth.make_world(seed=33, **WORLD)
    f = holed_forcing(w)
    pipe = pipeline_from_world(ctx, w, NM, 1971, 25, 6)
    calls = []
    real = _hip.lib().xh_upload_file
    _hip.lib().xh_upload_file = lambda *a: calls.append(a[4]) or real(*a)
    try:
        for form, host in sources(root, f).items():
            pipe.set_forcing({k: np.asarray(host[k]).astype(np.float64) for k in NAMES})
            assert all(pipe.forcing_upload[k] == ('f64', 8 * w.ncell * NM) for k in NAMES)
            ref = {k: pipe.forcing[k].download() for k in NAMES}
            for k in NAMES:
                pipe.forcing[k].zero()
            del calls[:]
            pipe.set_forcing(host)
            kind = 'f32' if form == 'memory' else form
            for k in NAMES:
                got = pipe.forcing[k].download()
                assert np.array_equal(got.view(np.uint64), ref[k].view(np.uint64)), (form, k)
                assert np.isnan(got).any() == (k == 'precip'), (form, k)       # the names that get nan_to_num got it
                assert pipe.forcing_upload[k] == (kind, host[k].dtype.itemsize * w.ncell * NM), (form, k)
            if expect_file_uploads is not None:
                n = 0 if form == 'memory' else expect_file_uploads
                assert calls == [host[k].nbytes for k in NAMES][:n], (form, calls)
    finally:
        _hip.lib().xh_upload_file = real
    with pytest.raises(ValueError, match='forcing tas has shape'):      # the shape check of a narrow source is the usual one
        pipe.set_forcing({'tas': np.zeros((w.ncell, NM + 1), dtype=np.float32)})
    pipe.close()


def test_set_forcing_from_stored_arrays(tmp_path, monkeypatch):
    monkeypatch.delenv('XH_UPLOAD_FROM_FILE', raising=False)
    check_set_forcing(str(tmp_path), expect_file_uploads=0)


def test_set_forcing_from_file_ranges_in_a_child_process(tmp_path):
    """XH_UPLOAD_FROM_FILE=1: the stored bytes of the mapped forms go through xh_upload_file, same bits."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ('import sys; sys.path[:0] = [{!r}, {!r}]; import test_gpu_narrow as t; '
            't.check_set_forcing({!r}, expect_file_uploads=len(t.NAMES)); print("child ok")').format(
        os.path.dirname(here), here, str(tmp_path))
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, XH_UPLOAD_FROM_FILE='1'), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and 'child ok' in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ------------------------------------------------------------------ whole runs
def files_of(folder):
    out = {}
    for base, _, names in os.walk(folder):
        for n in names:
            if n != 'logfile.log':
                out[os.path.relpath(os.path.join(base, n), folder)] = os.path.join(base, n)
    return out


def same_files(a, b, tag=''):
    fa, fb = files_of(a), files_of(b)
    assert sorted(fa) == sorted(fb) and fa, (tag, sorted(fa), sorted(fb))
    for rel in fa:
        assert filecmp.cmp(fa[rel], fb[rel], shallow=False), (tag, rel)


def rounded_forcing(w, seed=100):
    """(values rounded to single precision as float64, the same as float32)."""
    from xanthos_amd import synth
    f32 = {k: np.asarray(v).astype(np.float32) for k, v in synth.make_forcing(w, NM, seed=seed).items()}
    return {k: v.astype(np.float64) for k, v in f32.items()}, f32


OUTPUT_VARS = ('pet', 'aet', 'q', 'soilmoisture', 'avgchflow')


def test_float32_npy_run_writes_the_float64_runs_files(tmp_path):
    from xanthos_amd import Xanthos, synth
    w = synth.make_world(seed=33, **WORLD)
    f64, f32 = rounded_forcing(w)
    runs = {}
    for tag, f in (('f64', f64), ('f32', f32)):
        root = str(tmp_path / tag)
        ini = synth.write_example(root, w, f, 1971, 1973, runoff_spinup=25, routing_spinup=6, output_vars=OUTPUT_VARS)
        c = Xanthos(ini).execute()
        assert {k: v[0] for k, v in c.pipe.forcing_upload.items()} == {k: tag for k in NAMES}
        assert all(v[1] == (4 if tag == 'f32' else 8) * w.ncell * NM for v in c.pipe.forcing_upload.values())
        runs[tag] = os.path.join(root, 'output')
    assert len(files_of(runs['f64'])) >= len(OUTPUT_VARS)
    same_files(runs['f32'], runs['f64'], 'pm + abcd + mrtm')


def test_netcdf_float_run_writes_the_float64_runs_files(tmp_path):
    import re
    from xanthos_amd import Xanthos, synth
    w = synth.make_world(seed=33, **WORLD)
    f64, f32 = rounded_forcing(w)
    h = synth.hgm_forcing(w, f64)
    h['dtr'] = h['dtr'].astype(np.float32).astype(np.float64)      # (a difference of two singles need not be one)
    root = str(tmp_path / 'f64')
    ini = synth.write_hgm_example(root, w, h, 1971, 1973, runoff='abcd', runoff_spinup=25, routing_spinup=6,
                                  output_vars=OUTPUT_VARS)
    c = Xanthos(ini).execute()
    assert {v[0] for v in c.pipe.forcing_upload.values()} == {'f64'} and len(c.pipe.forcing_upload) == 4
    nc_root = str(tmp_path / 'nc')
    nc_ini = synth.write_hgm_example(nc_root, w, h, 1971, 1973, runoff='abcd', runoff_spinup=25, routing_spinup=6,
                                     output_vars=OUTPUT_VARS)
    text = open(nc_ini).read()
    for key, setting, varname, var in (('temp', 'TemperatureFile', 'TempVarName', 'tas'),
                                       ('dtr', 'DailyTemperatureRangeFile', 'DTRVarName', 'dtr'),
                                       ('precip', 'PrecipitationFile', 'PrecipVarName', 'pr'),
                                       ('abcd_tmin', 'TempMinFile', 'TempMinVarName', 'tmin')):
        path = os.path.join(nc_root, 'input', var + '.nc')
        write_nc(path, var, h[key], 'f4')
        text, n = re.subn(r'(?m)^{} = .*$'.format(setting), '{} = {}\n{} = {}'.format(setting, path, varname, var), text)
        assert n == 1, setting
    with open(nc_ini, 'w') as fh:
        fh.write(text)
    c = Xanthos(nc_ini).execute()
    assert c.pipe.forcing_upload == {k: ('f32be', 4 * w.ncell * NM) for k in ('temp', 'dtr', 'precip', 'abcd_tmin')}
    same_files(os.path.join(nc_root, 'output'), os.path.join(root, 'output'), 'hargreaves + abcd + mrtm')


def test_ensemble_of_a_float32_and_a_float64_member(tmp_path):
    from xanthos_amd import Xanthos, run_ensemble, synth
    w = synth.make_world(seed=33, **WORLD)
    f64, f32 = rounded_forcing(w, seed=107)
    root = str(tmp_path)
    ini, members = synth.write_ensemble_example(root, w, [f64, f64], 1971, 1973, names=('single', 'double'), runoff_spinup=25,
                                                routing_spinup=6, section=False, output_format=4)
    keys = {'pm_tas': 'tas', 'pm_tmin': 'tmin', 'pm_rhs': 'rhs', 'pm_wind': 'wind', 'pm_rsds': 'rsds', 'pm_rlds': 'rlds',
            'PrecipitationFile': 'precip', 'TempMinFile': 'abcd_tmin'}
    for setting, path in members[0][1].items():
        np.save(path, f32[keys[setting]])                          # member 'single': the same values, stored as float32
    out = os.path.join(root, 'output', 'pm_abcd_mrtm_synth')
    res = run_ensemble(ini, members=members, statistics=['mean'], overlap=True)
    assert {v[0] for v in res.forcing_upload[0].values()} == {'f32'} and {v[0] for v in res.forcing_upload[1].values()} == {'f64'}
    assert sum(v[1] for v in res.forcing_upload[1].values()) == 2 * sum(v[1] for v in res.forcing_upload[0].values())
    same_files(os.path.join(out, 'single'), os.path.join(out, 'double'), 'float32 member against float64 member')
    for name, overrides in members:
        ref = os.path.join(root, 'alone', name)
        Xanthos(ini).execute(dict(overrides, OutputFolder=ref))
        same_files(os.path.join(out, name), ref, name)
    kept = out + '_overlapped'
    os.rename(out, kept)
    serial = run_ensemble(ini, members=members, statistics=['mean'], overlap=False)
    assert serial.forcing_upload == res.forcing_upload
    same_files(kept, out, 'overlap')
