"""CPU tests of the Hargreaves-Samani / Thornthwaite host side: the [[hargreaves-samani]] and [[thornthwaite]] reader
surface, the refused configurations, the exported C-ABI symbols and the loader's NaN handling."""
import os

import numpy as np
import pytest

from xanthos_amd import _hip, synth
from xanthos_amd.ini_reader import ConfigReader, ValidationException


def _world():
    return synth.make_world(nrow=24, ncol=48, ncell=80, n_basins=3, seed=4)


def _ini(tmp_path, pet, nm=36, forcing=None, **kw):
    w = _world()
    f = forcing if forcing is not None else synth.pet_ext_forcing(w, synth.make_forcing(w, nm))
    return synth.write_pet_ext_example(str(tmp_path), w, f, 1975, 1974 + nm // 12, pet=pet, **kw)


def _variant(ini, old, new):
    text = open(ini).read()
    assert old in text, old
    with open(ini, 'w') as fh:
        fh.write(text.replace(old, new))
    return ini


def test_reader_accepts_hs(tmp_path):
    c = ConfigReader(_ini(tmp_path, 'hs'))
    assert (c.pet_module, c.runoff_module, c.routing_module) == ('hs', 'abcd', 'mrtm')
    assert c.mod_cfg == 'hs_abcd_mrtm'
    d = os.path.join(str(tmp_path), 'input', 'pet', 'hargreaves_samani')
    assert c.pet_dir == d
    assert (c.hs_tas, c.hs_tmin, c.hs_tmax) == tuple(os.path.join(d, k + '.npy') for k in ('tas', 'tmin', 'tmax'))


def test_reader_accepts_thornthwaite(tmp_path):
    c = ConfigReader(_ini(tmp_path / 'a', 'thornthwaite'))
    assert (c.pet_module, c.mod_cfg) == ('thornthwaite', 'thornthwaite_abcd_mrtm')
    assert c.trn_tas == os.path.join(str(tmp_path / 'a'), 'input', 'pet', 'thornthwaite', 'tas.npy')
    assert c.trn_daylight == 'reference'
    m = ConfigReader(_ini(tmp_path / 'b', 'thornthwaite', daylight='Monthly'))
    assert m.trn_daylight == 'monthly'


@pytest.mark.parametrize('pet,old,new', [
    ('hs', '[[hargreaves-samani]]', '[[hs]]'),                    # missing subsection
    ('hs', 'hs_tmax = tmax.npy\n', ''),                           # missing keys
    ('hs', 'hs_tas = tas.npy\n', ''),
    ('hs', 'pet_dir = hargreaves_samani\n', ''),
    ('thornthwaite', '[[thornthwaite]]', '[[trn]]'),
    ('thornthwaite', 'trn_tas = tas.npy\n', ''),
    ('thornthwaite', 'trn_tas = tas.npy\n', 'trn_tas = tas.npy\ndaylight = tiled\n'),   # bad daylight value
])
def test_refused_configurations(tmp_path, pet, old, new):
    ini = _variant(_ini(tmp_path, pet), old, new)
    with pytest.raises(ValidationException):
        ConfigReader(ini)


@pytest.mark.parametrize('pet', ['hs', 'thornthwaite'])
def test_gwam_still_needs_hargreaves(tmp_path, pet):
    from types import SimpleNamespace as NS
    from xanthos_amd.ini_reader import check_modules
    with pytest.raises(ValidationException):
        check_modules(NS(pet_module=pet, runoff_module='gwam', calibrate=0))
    check_modules(NS(pet_module=pet, runoff_module='abcd', calibrate=1))
    w = _world()
    f = synth.pet_ext_forcing(w, synth.make_forcing(w, 24))
    f.update(temp=f['tas'], dtr=f['tas'] - f['tmin'])
    ini = synth.write_hgm_example(str(tmp_path), w, f, 1971, 1972, pet=pet)     # pet + gwam
    with pytest.raises(ValidationException):
        ConfigReader(ini)


def test_runner_lists_every_reference_pet_module():
    from xanthos_amd.configurations import ConfigRunner
    assert sorted(ConfigRunner.PET_COMPONENTS) == ['hargreaves', 'hs', 'pm', 'thornthwaite']
    assert ConfigReader.PET_OTHER == ()


def test_cabi_symbols_exported():
    lib = _hip.lib()
    for name in ('xh_hs_pet', 'xh_thornthwaite_pet'):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    assert lib.xh_abi_version() == _hip.ABI_VERSION == 7


def test_multi_gpu_refused(tmp_path):
    from xanthos_amd.model import run_model
    with pytest.raises(ValidationException):
        run_model(_ini(tmp_path, 'thornthwaite'), gpus=2)


def _holes(nm=36):
    w = _world()
    f = synth.pet_ext_forcing(w, synth.make_forcing(w, nm))
    for k in ('tas', 'tmin', 'tmax'):
        f[k] = f[k].copy()
    f['tas'][1, 2], f['tas'][2, 3], f['tmax'][3, 4], f['tmin'][4, 5] = np.nan, np.inf, np.nan, np.nan
    return f


def test_loader_keeps_nan_for_hs(tmp_path):
    from xanthos_amd.data_load import DataLoader
    f = _holes()
    c = ConfigReader(_ini(tmp_path, 'hs', forcing=f))
    d = DataLoader(c)
    for k in ('tas', 'tmin', 'tmax'):
        assert np.array_equal(np.asarray(getattr(d, 'hs_' + k)), f[k], equal_nan=True)
    assert np.array_equal(d.latitude, d.coords[:, 2])


@pytest.mark.parametrize('device_transforms', [True, False])
def test_loader_thornthwaite_nan_to_num(tmp_path, device_transforms):
    """data_load.py:137-138: nan_to_num of trn_tas -- on the host only with device_transforms = False; otherwise the
    pipeline applies it on the device right after the upload."""
    from xanthos_amd.data_load import DataLoader
    f = _holes()
    c = ConfigReader(_ini(tmp_path, 'thornthwaite', forcing=f))
    c.update({'device_transforms': device_transforms})
    d = DataLoader(c)
    want = f['tas'] if device_transforms else np.nan_to_num(f['tas'])
    assert np.array_equal(np.asarray(d.tair), want, equal_nan=True)
    assert np.array_equal(d.lat_radians, np.radians(d.coords[:, 2]))


def test_hs_days_per_month():
    from xanthos_amd.pet import hargreaves_samani as hs
    nd = hs.days_per_month(1899, 1901)
    assert len(nd) == 36 and nd[1] == 28 and nd[13] == 28 and nd[25] == 28      # 1900 is not a leap year
    assert hs.days_per_month(2000, 2000)[1] == 29


def test_daylight_mode_names():
    from xanthos_amd.pet import thornthwaite as trn
    assert trn.daylight_mode('reference') == _hip.XH_DAYLIGHT_REFERENCE
    assert trn.daylight_mode('monthly') == _hip.XH_DAYLIGHT_MONTHLY
    with pytest.raises(ValueError):
        trn.daylight_mode('tiled')
