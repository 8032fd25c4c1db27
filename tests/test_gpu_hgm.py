"""GPU tests of Hargreaves PET and GWAM runoff (csrc/xh_gwam.hip) against the reference's golden vectors and a numpy
restatement of gwam.py:runoffgen."""
import io
import os
import zipfile

import numpy as np
import pytest

from xanthos_amd import synth

pytestmark = pytest.mark.gpu


def gwam_month_np(pet, p, sm, ch, indexing=999.0):
    """gwam.py:runoffgen (:18-88) restated with boolean masks: the branches, their NaN behaviour and the operation order."""
    aet, q, sav = np.zeros_like(pet), np.zeros_like(pet), np.zeros_like(pet)
    with np.errstate(all='ignore'):
        B = ch + p - pet
        lake = sm == indexing
        soil = (sm != 0) & ~lake
        full = soil & (B >= sm)
        part = soil & (B < sm)
        d = p - pet
        q[lake] = np.where(d[lake] > 0, d[lake], 0.0)
        a = np.minimum(p[lake], pet[lake])
        aet[lake] = np.where(np.isnan(a), pet[lake], a)
        q[full], sav[full], aet[full] = B[full] - sm[full], sm[full], pet[full]
        c, pp, e, s = ch[part], p[part], pet[part], sm[part]
        x = c / s
        t5 = (5. * c / s - 2. * (x * x)) / 3.
        a = np.minimum(c + pp, e * np.maximum(0.1, np.minimum(1.0, t5)))
        sv = np.minimum(s, c * (1 - np.exp(-x)) / (1 - np.exp(-1.0)) + (pp - a))
        low = sv <= 0
        sv[low] = 0.0
        a[low] = pp[low] + c[low]
        aet[part], sav[part], q[part] = a, sv, np.maximum(0.0, c + pp - a - sv)
    return aet, q, sav


def gwam_series_np(pet, precip, sm, sm0, spinup, monthly):
    st = sm0.copy()
    nm = pet.shape[1]
    out = [np.zeros_like(pet) for _ in range(3)]
    for steps in (spinup, nm):
        for m in range(steps):
            a, q, s = gwam_month_np(pet[:, m], precip[:, m] if monthly else precip[:, steps - 1], sm, st)
            if steps == nm:
                out[0][:, m], out[1][:, m], out[2][:, m] = a, q, s
            st = s
    return out


def _close(name, x, ref, rtol, atol=0.0):
    assert np.array_equal(np.isnan(x), np.isnan(ref)), name + ': NaN masks differ'
    m = ~np.isnan(ref)
    err = np.abs(x[m] - ref[m])
    bad = err > np.maximum(rtol * np.abs(ref[m]), atol)
    assert not bad.any(), '{}: {} values off, worst {:.3e}'.format(name, int(bad.sum()), float(err.max()))


def test_hargreaves_kernel_matches_reference(golden):
    from xanthos_amd.pet import hargreaves
    g = golden('hargreaves')
    pet = hargreaves.run_hargreaves(g['temp'], g['dtr'], g['lat'], int(g['start_year']), int(g['end_year']))
    _close('PET', pet, g['pet'], 1e-10, 1e-9)
    assert np.array_equal(pet == 0, g['pet'] == 0)
    one = hargreaves.calculate_pet(np.nan_to_num(g['temp'][:, 5]), np.nan_to_num(g['dtr'][:, 5]), g['lat'],
                                   g['solar_dec'][5], g['dr'][5], g['yr_imth_ndays'][5, 2])
    _close('PET month 5', one, g['pet'][:, 5], 1e-10, 1e-9)


@pytest.mark.parametrize('mode', ['reference', 'monthly'])
def test_gwam_kernel_matches_reference(golden, mode):
    from xanthos_amd.runoff import gwam
    g = golden('gwam')
    _, aet, q, sav = gwam.gwam_execute(g['pet'], g['precip'], g['sm'], g['sm0'], int(g['spinup']), precipitation=mode)
    pre = '' if mode == 'reference' else 'monthly_'
    for name, x in (('aet', aet), ('q', q), ('sav', sav)):
        ref = g[pre + name]
        # 1e-12 relative; values that are differences of nearly equal terms (Sav = soil term + P - AET, close to 0) are
        # held to 1e-12 mm absolute: exp(-x) of the device and of numpy may differ by an ulp
        _close(name, x, ref, 1e-12, 1e-12)
        assert np.array_equal(x == 0, ref == 0), name + ': zero masks differ'


def test_runoffgen_one_month(golden):
    from xanthos_amd.runoff import gwam
    g = golden('gwam')
    pet, p, sm = g['pet'][:, 0], g['precip'][:, 3], g['sm']
    res = gwam.runoffgen(pet, p, None, sm, g['sm0'])
    ref = gwam_month_np(pet, p, sm, g['sm0'])
    assert np.array_equal(res[0], pet, equal_nan=True)
    for x, r in zip(res[1:], ref):
        _close('runoffgen', x, r, 1e-12, 1e-12)


def _tree(golden, tmp_path, tag, extra=None):
    g = golden('hgm')
    root = str(tmp_path / tag)
    with zipfile.ZipFile(io.BytesIO(g[tag + '_tree_zip'].tobytes())) as z:
        z.extractall(root)
    ini = os.path.join(root, str(g[tag + '_ini_name']))
    text = open(ini).read().replace(str(g[tag + '_old_root']), root)
    if extra:
        text = text.replace(*extra)
    open(ini, 'w').write(text)
    return g, ini


@pytest.mark.parametrize('tag,form', [('hist', 'default'), ('future', 'default'), ('abcd', 'default'), ('hist', 'exact')])
def test_model_matches_reference_run(golden, tmp_path, tag, form):
    from xanthos_amd.model import Xanthos
    extra = ('routing_spinup', 'routing_form = exact\nrouting_spinup') if form == 'exact' else None
    g, ini = _tree(golden, tmp_path, tag, extra)
    c = Xanthos(ini).execute()
    for name in ('PET', 'AET', 'Q', 'Sav'):
        _close(name, getattr(c, name), g[tag + '_' + name], 1e-10, 1e-12)
    for name in ('ChStorage', 'Avg_ChFlow'):
        _close(name, getattr(c, name), g[tag + '_' + name], 1e-9, 1e-9)
    out = os.path.join(os.path.dirname(ini), 'output')
    assert any(f.endswith('.csv') for _, _, fs in os.walk(out) for f in fs)


def test_model_monthly_precipitation(golden, tmp_path):
    from xanthos_amd.model import Xanthos
    g, ini = _tree(golden, tmp_path, 'hist', ('PrecipitationFile', 'precipitation = monthly\nPrecipitationFile'))
    c = Xanthos(ini).execute()
    d = c.data
    want = gwam_series_np(np.asarray(c.PET), np.asarray(d.precip), d.soil_moisture, d.sm_prev, c.s.runoff_spinup, True)
    _close('PET', c.PET, g['hist_PET'], 1e-10, 1e-12)
    for name, ref in zip(('AET', 'Q', 'Sav'), want):
        _close(name, getattr(c, name), ref, 1e-12, 1e-12)
    assert not np.allclose(c.Q, g['hist_Q'])          # the opt-in mode is a different model run


def test_reference_test_distributions(tmp_path):
    """xanthos/test/test_hargreaves_gwam_mrtm.py: T ~ U(-5, 30), DTR ~ U(1, 10), P ~ N(50, 10) for 12 months in memory."""
    from xanthos_amd.model import Xanthos
    w = synth.make_world(nrow=360, ncol=720, ncell=400, n_basins=5, seed=12)
    f = synth.hgm_forcing(w, synth.make_forcing(w, 12, nan_precip=False))
    ini = synth.write_hgm_example(str(tmp_path), w, f, 1971, 1971, output_vars=('q',))
    rng = np.random.default_rng(0)
    args = {'TemperatureFile': rng.uniform(-5, 30, (w.ncell, 12)),
            'DailyTemperatureRangeFile': rng.uniform(1, 10, (w.ncell, 12)),
            'PrecipitationFile': rng.normal(50, 10, (w.ncell, 12))}
    res = Xanthos(ini).execute(args)
    assert res.Q.shape == (w.ncell, 12)
    assert not np.any(np.isnan(res.Q))
    assert not np.any(res.Q < 0)


def test_fullsize_gwam_on_device_pet():
    """67,420 cells x 600 months: Hargreaves on the device, GWAM fed that PET in HBM, against the restatement."""
    from xanthos_amd import _hip
    from xanthos_amd.pet import hargreaves
    from xanthos_amd.runoff import gwam
    ncell, nm, spinup = 67420, 600, 120
    rng = np.random.default_rng(600)
    ctx = _hip.get_context(0)
    temp = rng.uniform(-20, 35, (ncell, nm))
    dtr = rng.uniform(0, 15, (ncell, nm))
    precip = rng.gamma(1.5, 40.0, (ncell, nm))
    lat = np.radians(rng.uniform(-60, 85, ncell))
    sm = rng.uniform(10, 500, ncell)
    sm[::50] = 999.0
    sm[3::97] = 0.0
    sm0 = 0.5 * sm
    dec, dr, nd = hargreaves.month_factors(1901, 1950)
    bufs = {k: ctx.upload(v) for k, v in (('t', temp), ('d', dtr), ('p', precip), ('lat', lat), ('sm', sm), ('sm0', sm0))}
    d_pet = hargreaves.hargreaves_device(ctx, ncell, nm, bufs['t'], bufs['d'], bufs['lat'], dec, dr, nd)
    for mode in ('reference', 'monthly'):
        out = gwam.gwam_device(ctx, ncell, nm, spinup, d_pet, bufs['p'], bufs['sm'], bufs['sm0'], precipitation=mode)
        pet = d_pet.download()
        want = gwam_series_np(pet, precip, sm, sm0, spinup, mode == 'monthly')
        for name, ref in zip(('aet', 'q', 'sav'), want):
            _close(name, out[name].download(), ref, 1e-10, 1e-10)
        for v in out.values():
            v.free()
    d_pet.free()
    for v in bufs.values():
        v.free()
