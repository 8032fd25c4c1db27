"""CPU tests of the Hargreaves / GWAM host side: the .ini surface of the reference's test configuration, the refused
combinations, the loader's soil moisture and the month factors against the reference's golden vectors."""
import os

import numpy as np
import pytest

from xanthos_amd import synth
from xanthos_amd.ini_reader import ConfigReader, ValidationException
from xanthos_amd.utils import calc_sinusoidal_factor, set_month_arrays

# the reference's own test configuration (xanthos/test/configs/hargreaves_gwam_mrtm.ini), keys and values as shipped
REF_TEST_INI = '''[Project]
ProjectName                 = test_hargreaves_gwam_mrtm
RootDir                     = {root}
InputFolder                 = input
OutputFolder                = output
RefDir                      = reference
pet_dir                     = pet
RoutingDir                  = routing
RunoffDir                   = runoff
DiagDir                     = diagnostics
AccWatDir                   = accessible_water
HydActDir                   = hydropower_actual
HistFlag                    = True
n_basins                    = 235
StartYear                   = 1971
EndYear                     = 1971
output_vars                 =
OutputFormat                = 1
OutputUnit                  = 1
OutputInYear                = 1
AggregateRunoffBasin        = 0
AggregateRunoffCountry      = 0
AggregateRunoffGCAMRegion   = 0
PerformDiagnostics          = 0
CreateTimeSeriesPlot        = 0
CalculateDroughtStats       = 0
CalculateAccessibleWater    = 0
CalculateHydropowerPotential = 0
CalculateHydropowerActual   = 0
Calibrate                   = 0

[PET]
pet_module                  = hargreaves

[[hargreaves]]
pet_dir                     = penman_monteith
TemperatureFile             = none
DailyTemperatureRangeFile   = none

[Runoff]
runoff_module               = gwam

[[gwam]]
runoff_dir                  = gwam
runoff_spinup               = 12
PrecipitationFile           = none
max_soil_moisture           = soil_moisture.csv
lakes_msm                   = Lakes_wo_casp.csv
addit_water_msm             = Addit_water421.csv

[Routing]
routing_module              = mrtm

[[mrtm]]
routing_dir                 = mrtm
routing_spinup              = 12
channel_velocity            = velocity_half_degree.npy
flow_distance               = DRT_half_FDISTANCE_globe.txt
flow_direction              = DRT_half_FDR_globe_bystr50.txt
'''


@pytest.fixture
def ref_ini(tmp_path):
    p = tmp_path / 'hargreaves_gwam_mrtm.ini'
    p.write_text(REF_TEST_INI.format(root=str(tmp_path)))
    return str(p), p.read_text()


def _variant(tmp_path, text, old, new):
    assert old in text, old
    p = tmp_path / 'variant.ini'
    p.write_text(text.replace(old, new))
    return str(p)


def test_reader_accepts_reference_test_config(ref_ini, tmp_path):
    ini, _ = ref_ini
    c = ConfigReader(ini)
    assert (c.pet_module, c.runoff_module, c.routing_module) == ('hargreaves', 'gwam', 'mrtm')
    assert c.mod_cfg == 'hargreaves_gwam_mrtm' and c.nmonths == 12 and c.runoff_spinup == 12
    pet_dir = os.path.join(str(tmp_path), 'input', 'pet', 'penman_monteith')
    assert c.TemperatureFile == os.path.join(pet_dir, 'none') and c.TempVarName is None
    assert c.DailyTemperatureRangeFile == os.path.join(pet_dir, 'none') and c.DTRVarName is None
    gw = os.path.join(str(tmp_path), 'input', 'runoff', 'gwam')
    assert c.max_soil_moisture == os.path.join(gw, 'soil_moisture.csv')
    assert c.lakes_msm == os.path.join(gw, 'Lakes_wo_casp.csv')
    assert c.addit_water_msm == os.path.join(gw, 'Addit_water421.csv')
    assert c.PrecipitationFile == os.path.join(gw, 'none') and c.PrecipVarName is None
    assert c.gwam_precipitation == 'reference'
    assert c.ChStorageFile is None and c.SavFile is None


def test_reader_gwam_options_and_future_keys(ref_ini, tmp_path):
    ini, text = ref_ini
    m = ConfigReader(_variant(tmp_path, text, 'runoff_spinup               = 12',
                              'runoff_spinup = 12\nprecipitation = Monthly'))
    assert m.gwam_precipitation == 'monthly'
    with pytest.raises(ValidationException):
        ConfigReader(_variant(tmp_path, text, 'runoff_spinup               = 12', 'runoff_spinup = 12\nprecipitation = daily'))
    fut = text.replace('HistFlag                    = True', 'HistFlag = False')
    with pytest.raises(ValidationException):               # future mode without the four keys (ini_reader.py:330-338)
        ConfigReader(_variant(tmp_path, fut, 'runoff_spinup               = 12', 'runoff_spinup = 12\nSavFile = s.npy'))
    c = ConfigReader(_variant(tmp_path, fut, 'runoff_spinup               = 12',
                              'runoff_spinup = 12\nChStorageFile = /x/c.npy\nChStorageVarName = c\nSavFile = /x/s.npy\n'
                              'SavVarName = s'))
    assert (c.ChStorageFile, c.ChStorageVarName, c.SavFile, c.SavVarName) == ('/x/c.npy', 'c', '/x/s.npy', 's')


@pytest.mark.parametrize('old,new', [
    ('[PET]\npet_module                  = hargreaves', '[PET]\npet_module = none\npet_file = pet.npy'),   # none + gwam
    ('Calibrate                   = 0', 'Calibrate = 1'),                                # no calibration of GWAM
    ('pet_module                  = hargreaves', 'pet_module = hs'),                     # still refused
    ('pet_module                  = hargreaves', 'pet_module = thornthwaite'),
    ('[[gwam]]', '[[gwam_typo]]'),                                                        # missing subsection
    ('[[hargreaves]]', '[[nothing]]'),
    ('max_soil_moisture           = soil_moisture.csv\n', ''),                            # missing required keys
    ('DailyTemperatureRangeFile   = none\n', ''),
    ('runoff_spinup               = 12\n', ''),
])
def test_refused_configurations(ref_ini, tmp_path, old, new):
    ini, text = ref_ini
    with pytest.raises(ValidationException):
        ConfigReader(_variant(tmp_path, text, old, new))


def test_pm_gwam_refused():
    """pm + gwam: the reference's GWAM driver reads data.temp, which only Hargreaves loads (components.py:144-160)."""
    from types import SimpleNamespace as NS
    from xanthos_amd.ini_reader import check_modules
    with pytest.raises(ValidationException):
        check_modules(NS(pet_module='pm', runoff_module='gwam', calibrate=0))
    check_modules(NS(pet_module='hargreaves', runoff_module='gwam', calibrate=0))
    check_modules(NS(pet_module='hargreaves', runoff_module='abcd', calibrate=1))


def test_hargreaves_abcd_is_accepted(tmp_path):
    w = synth.make_world(nrow=24, ncol=48, ncell=80, n_basins=3, seed=4)
    f = synth.hgm_forcing(w, synth.make_forcing(w, 36))
    c = ConfigReader(synth.write_hgm_example(str(tmp_path), w, f, 1971, 1973, runoff='abcd', runoff_spinup=25))
    assert c.mod_cfg == 'hargreaves_abcd_mrtm' and c.runoff_spinup == 25


def test_multi_gpu_refused(tmp_path):
    from xanthos_amd.model import run_model
    w = synth.make_world(nrow=24, ncol=48, ncell=80, n_basins=3, seed=4)
    ini = synth.write_hgm_example(str(tmp_path), w, synth.hgm_forcing(w, synth.make_forcing(w, 24)), 1971, 1972)
    with pytest.raises(ValidationException):
        run_model(ini, gpus=2)


def test_month_factors_match_reference(golden):
    g = golden('hargreaves')
    tab = set_month_arrays(72, int(g['start_year']), int(g['end_year']))
    assert np.array_equal(tab, g['yr_imth_ndays'])
    dec, dr = calc_sinusoidal_factor(tab)
    assert np.array_equal(dec, g['solar_dec']) and np.array_equal(dr, g['dr'])


def _hgm_tree(golden, tmp_path, tag):
    import io
    import zipfile
    g = golden('hgm')
    root = str(tmp_path / tag)
    with zipfile.ZipFile(io.BytesIO(g[tag + '_tree_zip'].tobytes())) as z:
        z.extractall(root)
    ini = os.path.join(root, str(g[tag + '_ini_name']))
    text = open(ini).read().replace(str(g[tag + '_old_root']), root)
    open(ini, 'w').write(text)
    return g, ini


@pytest.mark.parametrize('tag', ['hist', 'future'])
def test_loader_soil_moisture(golden, tmp_path, tag):
    """Sm composite (max_soil_moisture with the water bodies of both tables) and sm0 (0.5 Sm, or SavFile's last column)."""
    from xanthos_amd.data_load import DataLoader
    g, ini = _hgm_tree(golden, tmp_path, tag)
    c = ConfigReader(ini)
    d = DataLoader(c)
    root = os.path.dirname(ini)
    gw = os.path.join(root, 'input', 'runoff', 'gwam')
    raw = np.genfromtxt(os.path.join(gw, 'soil_moisture.csv'), delimiter=',', skip_header=1)
    want = raw.copy()
    for f in ('lakes.csv', 'addit.csv'):
        t = np.genfromtxt(os.path.join(gw, f), delimiter=',').astype(int)
        want[t[:, 0] - 1] = t[:, 1]
    assert np.array_equal(d.soil_moisture, want) and (want == 999).sum() > 0 and (want == 0).sum() > 0
    if tag == 'hist':
        assert np.array_equal(d.sm_prev, 0.5 * want)
    else:
        assert np.array_equal(d.sm_prev, np.load(os.path.join(gw, 'sav.npy'))[:, -1])
    assert np.array_equal(d.lat_radians, np.radians(d.coords[:, 2]))
    assert d.temp.shape == d.dtr.shape == d.precip.shape == (c.ncell, c.nmonths)


def test_gwam_spinup_out_of_range_is_refused(golden, tmp_path):
    from xanthos_amd.components import Components
    g, ini = _hgm_tree(golden, tmp_path, 'hist')
    c = ConfigReader(ini)
    for n in (0, c.nmonths + 1):
        c.update({'runoff_spinup': n})
        with pytest.raises(ValidationException):
            Components(c).simulation()
