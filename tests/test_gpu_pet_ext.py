"""GPU tests of Hargreaves-Samani and Thornthwaite PET (csrc/xh_pet_ext.hip) against the reference's golden vectors, the
reference's own Thornthwaite test, whole model runs and numpy restatements of hargreaves_samani.py / thornthwaite.py."""
import calendar
import io
import os
import zipfile

import numpy as np
import pytest

from xanthos_amd import synth

pytestmark = pytest.mark.gpu

MONTHDAYS = [31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]
LEAP_MONTHDAYS = [31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]


def hs_np(tas, tmax, tmin, lat_deg, y0, y1):
    """hargreaves_samani.py:34-64, :95-119 restated over whole arrays, operation order kept."""
    nm = tas.shape[1]
    j = np.array([15, 45, 75, 105, 135, 165, 195, 225, 255, 285, 315, 345])
    delta = 0.4102 * np.sin(2 * (np.pi / 365) * (j[np.arange(nm) % 12] - 80))[None, :]
    phi = (np.asarray(lat_deg)[:, None] * np.pi / 180)
    with np.errstate(all='ignore'):
        tn = -np.tan(delta) * np.tan(phi)
        acs = np.where((tn < -1.) | (tn > 1.), 0.0, np.arccos(tn))
        ra = 118 / np.pi * acs + np.cos(phi) * np.cos(delta) * np.sin(acs)
        pet = 0.408 * 0.0023 * ra * (tas + 17.8) * np.sqrt(np.abs(tmax - tmin))
    pet = np.where(tas < 0, 0.0, pet)
    days = [calendar.monthrange(y, m)[1] for y in range(y0, y1 + 1) for m in range(1, 13)]
    return pet * np.array(days)


def daylight_np(mth_days, lat):
    d = np.arange(sum(mth_days)) + 1
    dec = 0.409 * np.sin(((2 * np.pi / 365.0) * d - 1.39))
    x = np.clip(-np.tan(lat[:, None]) * np.tan(dec[None, :]), -1, 1)
    hours = np.arccos(x) * (24.0 / np.pi)
    idx = np.concatenate([[0], np.cumsum(mth_days)[:-1]])
    return np.add.reduceat(hours, idx, axis=1) / mth_days


def trn_np(tas, lat, y0, y1, monthly=False):
    """thornthwaite.py:51-130 restated; monthly=True tiles the daylight instead of the reference's np.repeat."""
    t = np.array(tas, dtype=float)
    t[np.isnan(t) | (t < 0)] = 0
    ny = y1 - y0 + 1
    with np.errstate(all='ignore'):
        I = np.add.reduceat(np.power(t / 5.0, 1.514), np.arange(0, t.shape[1], 12), axis=1)
        a = (.000000675 * I ** 3) - (.0000771 * I ** 2) + (.0179 * I) + .492
        I, a = np.repeat(I, 12, axis=1), np.repeat(a, 12, axis=1)
        pu = 16 * np.power(np.divide(10 * t, I, out=np.zeros_like(I), where=(I != 0)), a)
    L = daylight_np(MONTHDAYS, lat)
    L = np.tile(L, ny) if monthly else np.repeat(L, ny, axis=1)
    leap = [calendar.isleap(y) for y in range(y0, y1 + 1)]
    if any(leap):
        L[:, np.repeat(leap, 12)] = np.tile(daylight_np(LEAP_MONTHDAYS, lat), sum(leap))
    N = np.array([LEAP_MONTHDAYS if ly else MONTHDAYS for ly in leap]).flatten()
    with np.errstate(all='ignore'):
        return pu * (L / 12) * (N / 30.0)


def _close(name, x, ref, rtol, atol=0.0, zeros=True):
    assert np.array_equal(np.isnan(x), np.isnan(ref)), name + ': NaN masks differ'
    if zeros:
        assert np.array_equal(x == 0, ref == 0), name + ': zero masks differ'
    inf = np.isinf(ref)
    assert np.array_equal(x[inf], ref[inf]) and not np.isinf(x[~inf]).any(), name + ': infinities differ'
    m = np.isfinite(ref)
    err = np.abs(x[m] - ref[m])
    bad = err > np.maximum(rtol * np.abs(ref[m]), atol)
    assert not bad.any(), '{}: {} values off, worst {:.3e}'.format(name, int(bad.sum()), float(err.max()))


# ---------------------------------------------------------------------------------------------- kernels vs the reference
def test_hs_kernel_matches_reference(golden):
    from types import SimpleNamespace as NS
    from xanthos_amd.pet import hargreaves_samani as hs
    g = golden('hs')
    y0, y1 = int(g['start_year']), int(g['end_year'])
    pet = hs.run_hs(g['tas'], g['tmax'], g['tmin'], g['lat'], y0, y1)
    _close('PET', pet, g['pet'], 1e-10, 1e-9)
    # the reference's call surface: execute(config, data)
    nc = g['lat'].size
    data = NS(coords=np.stack([np.arange(nc), np.zeros(nc), g['lat']], axis=1), hs_tas=g['tas'], hs_tmax=g['tmax'],
              hs_tmin=g['tmin'])
    pet2 = hs.execute(NS(ncell=nc, nmonths=pet.shape[1], StartYear=y0, EndYear=y1), data)
    assert np.array_equal(pet2, pet, equal_nan=True)
    _close('restatement', hs_np(g['tas'], g['tmax'], g['tmin'], g['lat'], y0, y1), g['pet'], 1e-10, 1e-9)


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_thornthwaite_kernel_matches_reference(golden, tag):
    from xanthos_amd.pet import thornthwaite as trn
    g = golden('thornthwaite')
    y0, y1 = int(g[tag + '_start_year']), int(g[tag + '_end_year'])
    tas = g[tag + '_tas']
    pet = trn.execute(tas, g['lat'], y0, y1)
    _close('PET', pet, g[tag + '_pet'], 1e-10, 1e-9)
    assert np.array_equal(tas, g[tag + '_tas'], equal_nan=True)      # the caller's array is left as it was
    _close('restatement', trn_np(np.nan_to_num(tas), g['lat'], y0, y1), g[tag + '_pet'], 1e-10, 1e-9)


def test_daylight_matches_reference(golden):
    from xanthos_amd.pet import thornthwaite as trn
    g = golden('thornthwaite')
    _close('common', trn.calc_daylight_hours(MONTHDAYS, g['lat']), g['dl_common'], 1e-10, 1e-9)
    _close('leap', trn.calc_daylight_hours(LEAP_MONTHDAYS, g['lat']), g['dl_leap'], 1e-10, 1e-9)
    with pytest.raises(ValueError):
        trn.calc_daylight_hours([30] * 12, g['lat'])


# ---------------------------------------------------------------------------------------------- the reference's own test
def test_reference_thornthwaite_assertions():
    """xanthos/test/test_thornthwaite.py through the device path."""
    from xanthos_amd.pet import thornthwaite as trn
    equator = trn.calc_daylight_hours(MONTHDAYS, np.array([0]))
    north_pole = trn.calc_daylight_hours(MONTHDAYS, np.array([np.pi / 2]))
    south_pole = trn.calc_daylight_hours(MONTHDAYS, np.array([-np.pi / 2]))
    assert np.all(equator == 12)
    assert np.any(north_pole[0] == 0.0)
    assert np.any(north_pole[0] == 24.0)
    assert np.all(24 - north_pole == south_pole)

    lat_radians = np.array([0.698132])
    tas1 = np.array([[2, 5, 6, 8, 10, 12, 15, 12, 10, 8, 6, 5]])
    tas2 = np.array([[-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1]])
    pet1_correct = np.array([[9.7, 22.9, 33.7, 47.6, 66.0, 78.8, 98.5, 74.4, 54.8, 40.9, 27.1, 22.3]])
    assert np.all(np.round(trn.execute(tas1, lat_radians, 1999, 1999), 1) == pet1_correct)
    assert np.all(trn.execute(tas2, lat_radians, 1999, 1999) == 0)


def test_daylight_monthly_mode(golden):
    """daylight = monthly: the true month order; it differs from the reference's in the common years of a multi-year run
    and agrees in the leap year and in a one-year run."""
    from xanthos_amd.pet import thornthwaite as trn
    g = golden('thornthwaite')
    tas, lat = np.nan_to_num(g['b_tas']), g['lat']                   # 1975-1977: 1976 is a leap year
    pet = trn.execute(tas, lat, 1975, 1977, daylight='monthly')
    _close('monthly', pet, trn_np(tas, lat, 1975, 1977, monthly=True), 1e-10, 1e-9)
    ref = g['b_pet']
    _close('leap year', pet[:, 12:24], ref[:, 12:24], 1e-10, 1e-9)
    busy = np.abs(lat) < 1.2                                         # (daylight changes with the month)
    assert not np.allclose(pet[busy][:, :12], ref[busy][:, :12], equal_nan=True)
    assert not np.allclose(pet[busy][:, 24:], ref[busy][:, 24:], equal_nan=True)
    one = tas[:, :12]
    assert np.array_equal(trn.execute(one, lat, 1975, 1975, daylight='monthly'), trn.execute(one, lat, 1975, 1975),
                          equal_nan=True)
    with pytest.raises(ValueError):
        trn.execute(one, lat, 1975, 1975, daylight='tiled')


# ---------------------------------------------------------------------------------------------- whole model runs
def _tree(golden, tmp_path, tag, extra=None):
    g = golden('pet_ext')
    root = str(tmp_path / tag)
    with zipfile.ZipFile(io.BytesIO(g[tag + '_tree_zip'].tobytes())) as z:
        z.extractall(root)
    ini = os.path.join(root, str(g[tag + '_ini_name']))
    text = open(ini).read().replace(str(g[tag + '_old_root']), root)
    if extra:
        text = text.replace(*extra)
    open(ini, 'w').write(text)
    return g, ini


@pytest.mark.parametrize('tag', ['hs', 'trn'])
def test_model_matches_reference_run(golden, tmp_path, tag):
    from xanthos_amd.model import Xanthos
    g, ini = _tree(golden, tmp_path, tag)
    c = Xanthos(ini).execute()
    assert c.pipe is not None                                        # the device-resident pipeline ran it
    for name in ('PET', 'AET', 'Q', 'Sav'):
        _close(name, getattr(c, name), g[tag + '_' + name], 1e-10, 1e-12, zeros=False)
    for name in ('ChStorage', 'Avg_ChFlow'):
        _close(name, getattr(c, name), g[tag + '_' + name], 1e-9, 1e-9, zeros=False)
    out = os.path.join(os.path.dirname(ini), 'output')
    assert any(f.endswith('.csv') for _, _, fs in os.walk(out) for f in fs)


def test_model_daylight_monthly(golden, tmp_path):
    from xanthos_amd.model import Xanthos
    g, ini = _tree(golden, tmp_path, 'trn', ('trn_tas = tas.npy', 'trn_tas = tas.npy\ndaylight = monthly'))
    c = Xanthos(ini).execute()
    tas = np.nan_to_num(np.load(os.path.join(os.path.dirname(ini), 'input', 'pet', 'thornthwaite', 'tas.npy')))
    _close('PET', c.PET, trn_np(tas, c.data.lat_radians, 1975, 1977, monthly=True), 1e-10, 1e-9)
    assert not np.allclose(c.PET, g['trn_PET'])


def test_calibration_with_thornthwaite(tmp_path):
    """Calibrate = 1 with Thornthwaite PET: the ABCD calibration runs on the device PET and writes its results."""
    from xanthos_amd.model import Xanthos
    w = synth.make_world(nrow=36, ncol=72, ncell=300, n_basins=3, seed=21)
    nm = 36
    f = synth.pet_ext_forcing(w, synth.make_forcing(w, nm, nan_precip=False))
    rng = np.random.default_rng(5)
    obs = np.concatenate([np.stack([np.full(nm, b), np.zeros(nm), np.zeros(nm), rng.uniform(0.1, 2.0, nm)], axis=1)
                          for b in (1, 2)])
    ini = synth.write_pet_ext_example(str(tmp_path), w, f, 1975, 1977, pet='thornthwaite', runoff_spinup=25,
                                      routing_spinup=6, output_vars=('q',), obs=obs)
    Xanthos(ini).execute()
    for b in (1, 2):
        kge = np.load(str(tmp_path / 'calib_out' / 'kge_result_basin_{}.npy'.format(b)))
        assert np.isfinite(kge).all()
        assert np.load(str(tmp_path / 'calib_out' / 'abcdm_parameters_basin_{}.npy'.format(b))).shape == (1, 5)


@pytest.mark.parametrize('pet', ['hargreaves', 'hs', 'thornthwaite'])
def test_pipeline_pet_only_matches_plugin(pet):
    """The device-resident pipeline with runoff_module='none' and no routing: PET bit for bit that of the plugin's host
    entry (the same kernel; NaN holes in every forcing go through the pipeline's own NaN rules), AET / Q / Sav zero."""
    from xanthos_amd import _hip
    from xanthos_amd.pet import hargreaves, hargreaves_samani as hs, thornthwaite as trn
    from xanthos_amd.pipeline import DevicePipeline
    w = synth.make_world(nrow=36, ncol=72, ncell=300, n_basins=3, seed=21)
    y0, y1, nm = 1975, 1977, 36
    base = synth.make_forcing(w, nm, nan_precip=False)
    f = synth.hgm_forcing(w, base) if pet == 'hargreaves' else synth.pet_ext_forcing(w, base)
    f = {k: np.array(v, dtype=np.float64) for k, v in f.items() if k not in ('precip', 'abcd_tmin')}
    for i, v in enumerate(f.values()):
        v[i::37, 5 + i] = np.nan
    lat_deg = np.asarray(w.latitude, dtype=np.float64)
    pipe = DevicePipeline(_hip.get_context(0), ncell=w.ncell, nmonths=nm, start_year=y0, pet_module=pet,
                          runoff_module='none', lat_radians=np.radians(lat_deg), lat_degrees=lat_deg)
    pipe.set_forcing(f)
    pipe.run()
    got = pipe.download(('pet', 'aet', 'q', 'sav'))
    if pet == 'hargreaves':
        want = hargreaves.run_hargreaves(f['temp'], f['dtr'], np.radians(lat_deg), y0, y1)
    elif pet == 'hs':
        want = hs.run_hs(f['tas'], f['tmax'], f['tmin'], lat_deg, y0, y1)
    else:
        want = trn.execute(f['tas'], np.radians(lat_deg), y0, y1)
    assert np.array_equal(got['pet'], want, equal_nan=True)
    assert np.isfinite(want).any()
    for k in ('aet', 'q', 'sav'):
        assert np.array_equal(got[k], np.zeros((w.ncell, nm))), k


# ---------------------------------------------------------------------------------------------- full size
def test_fullsize_hs():
    from xanthos_amd.pet import hargreaves_samani as hs
    ncell, nm = 67420, 600
    rng = np.random.default_rng(67)
    tas = rng.uniform(-20, 35, (ncell, nm))
    tmin = tas - rng.uniform(0, 15, (ncell, nm))
    tmax = tas + rng.uniform(0, 15, (ncell, nm))
    tas[rng.random(tas.shape) < 0.001] = np.nan
    lat = rng.uniform(-90, 90, ncell)
    pet = hs.run_hs(tas, tmax, tmin, lat, 1901, 1950)
    _close('PET', pet, hs_np(tas, tmax, tmin, lat, 1901, 1950), 1e-10, 1e-9)


@pytest.mark.parametrize('daylight', ['reference', 'monthly'])
def test_fullsize_thornthwaite(daylight):
    from xanthos_amd import _hip
    from xanthos_amd.pet import thornthwaite as trn
    ncell, nm = 67420, 600
    rng = np.random.default_rng(68)
    tas = rng.uniform(-15, 35, (ncell, nm))
    tas[rng.random(tas.shape) < 0.001] = np.nan
    lat = np.radians(rng.uniform(-90, 90, ncell))
    ctx = _hip.get_context(0)
    d_tas, d_lat = ctx.upload(tas), ctx.upload(lat)
    ctx.nan_to_num(d_tas)
    d_pet = trn.thornthwaite_device(ctx, ncell, nm, 1901, d_tas, d_lat, daylight=daylight)
    pet = d_pet.download()
    for b in (d_tas, d_lat, d_pet):
        b.free()
    _close('PET', pet, trn_np(np.nan_to_num(tas), lat, 1901, 1950, monthly=daylight == 'monthly'), 1e-10, 1e-9)
