"""Configuration reader for the pm / abcd / mrtm path -- same .ini surface as xanthos/data_reader/ini_reader.py.

The reference parses the file with ``configobj`` (not installed here) and flattens it into an attribute bag
(ini_reader.py:24-607).  This module has its own small parser for the same syntax (``[Section]``, nested
``[[subsection]]``, ``key = value``, ``#`` comments, comma lists, optional quotes) and builds the same attributes for
the sections the hot path reads: ``[Project]``, ``[PET][[penman-monteith]]`` / ``[[hargreaves]]`` /
``[[hargreaves-samani]]`` / ``[[thornthwaite]]``,
``[Runoff][[abcd]]`` / ``[[gwam]]``, ``[Routing][[mrtm]]``, ``[Calibrate]``, ``[Ensemble]`` and the post-processors' sections.  Selector strings are lower-cased and validated exactly like the
reference (:214, :309, :397); selectors that belong to other reference modules are rejected with a clear message
because only the MI355X hot path is implemented here.  ``update()`` keeps the in-memory override hook (:598-607).
"""
import os
import logging


class ValidationException(Exception):
    """Invalid Xanthos configuration (ini_reader.py:17)."""


def parse_ini(path):
    """Nested dict of the file's sections; values are str or list of str (comma separated)."""
    root = {}
    stack = [root]
    with open(path, 'r') as fh:
        for raw in fh:
            line = _strip_comment(raw).strip()
            if not line:
                continue
            if line.startswith('['):
                depth = len(line) - len(line.lstrip('['))
                name = line.strip('[]').strip()
                if depth < 1 or depth > len(stack):
                    raise ValidationException('bad section nesting: ' + raw.strip())
                del stack[depth:]
                sec = {}
                stack[-1][name] = sec
                stack.append(sec)
            elif '=' in line:
                key, val = line.split('=', 1)
                stack[-1][key.strip()] = _value(val.strip())
            else:
                raise ValidationException('cannot parse line: ' + raw.strip())
    return root


def _strip_comment(line):
    out, quote = [], None
    for ch in line:
        if quote:
            if ch == quote:
                quote = None
        elif ch in '"\'':
            quote = ch
        elif ch == '#':
            break
        out.append(ch)
    return ''.join(out)


def _value(text):
    parts = [p.strip().strip('"\'') for p in text.split(',')]
    if len(parts) > 1:
        return [p for p in parts if p != '']
    return parts[0] if parts else ''


def check_modules(s):
    """Module combinations the reference accepts in its reader but cannot run (components.py:144-187, :229-232), and the
    GWAM features this package leaves out: each a ValidationException here instead of a crash later."""
    pet, runoff = s.pet_module, s.runoff_module
    if runoff == 'gwam' and pet == 'none':
        raise ValidationException("runoff_module = gwam needs pet_module = hargreaves: the reference's GWAM driver takes its "
                                  "precipitation from the Hargreaves step loop (components.py:230, :334), so with a PET file "
                                  "it has none.")
    if runoff == 'gwam' and pet != 'hargreaves':
        raise ValidationException("runoff_module = gwam runs with pet_module = hargreaves only, not '{}': the reference's "
                                  "GWAM driver reads the temperature only Hargreaves loads (components.py:144-160).".format(pet))
    if runoff == 'gwam' and getattr(s, 'calibrate', 0):
        raise ValidationException('Calibrate = 1 calibrates the ABCD parameters; there is no calibration of GWAM.')
    check_calibration(s)


def check_calibration(s):
    """[Calibrate] against the modules: set_calibrate = 1 routes the basin's runoff, so it needs MRTM."""
    if getattr(s, 'calibrate', 0) and getattr(s, 'set_calibrate', 0) == 1 and getattr(s, 'routing_module', None) != 'mrtm':
        raise ValidationException("[Calibrate] set_calibrate = 1 calibrates against routed streamflow and needs "
                                  "routing_module = mrtm, not '{}'.".format(getattr(s, 'routing_module', None)))


# The settings that name forcing arrays, per PET / runoff module, and the attribute of the directory their ini value is
# joined to (None: taken as written).  These are the settings an ensemble member may vary ([Ensemble], ensemble.py); a
# cell of the members table is resolved by resolve_forcing_setting exactly as configure_pet / configure_runoff resolve
# the same key of the ini.
FORCING_SETTINGS = {
    'pm': {k: 'pet_dir' for k in ('pm_tas', 'pm_tmin', 'pm_rhs', 'pm_wind', 'pm_rsds', 'pm_rlds')},
    'hargreaves': {'TemperatureFile': 'pet_dir', 'DailyTemperatureRangeFile': 'pet_dir'},
    'hs': {'hs_tas': 'pet_dir', 'hs_tmax': 'pet_dir', 'hs_tmin': 'pet_dir'},
    'thornthwaite': {'trn_tas': 'pet_dir'},
    'abcd': {'PrecipitationFile': None, 'TempMinFile': None},
    'gwam': {'PrecipitationFile': 'ro_model_dir'},
    'none': {},
}
ENSEMBLE_STATISTICS = ('mean', 'std', 'min', 'max')


def parse_statistic(text):
    """'mean' / 'std' / 'min' / 'max' -> (name, None); 'qNN' (NN an integer 0-100) -> ('qNN', NN / 100)."""
    t = str(text).strip().lower()
    if t in ENSEMBLE_STATISTICS:
        return t, None
    if t[:1] == 'q' and t[1:].isdigit() and 0 <= int(t[1:]) <= 100:
        return 'q{}'.format(int(t[1:])), int(t[1:]) / 100.0
    raise ValidationException("[Ensemble] statistics: '{}' is not one of mean, std, min, max or qNN with NN an integer "
                              "from 0 to 100.".format(text))


def _subsection(cfg, name, section):
    m = cfg.get(name)
    if not isinstance(m, dict):
        raise ValidationException('[{0}] selects {1} but has no [[{1}]] subsection.'.format(section, name))
    return m


def _key(m, key, name):
    if key not in m:
        raise ValidationException('{} is required in the [[{}]] section of the config file.'.format(key, name))
    return m[key]


class ConfigReader:
    """Attribute bag of settings for one run (ini_reader.py:24)."""

    PET_OTHER = ()
    RUNOFF_OTHER = ()

    def __init__(self, ini):
        c = parse_ini(ini) if not isinstance(ini, dict) else ini
        try:
            p = c['Project']
        except KeyError:
            raise ValidationException('no [Project] section in ' + str(ini))

        self.root = p['RootDir']
        self.ProjectName = p['ProjectName']
        self.OutputNameStr = p['ProjectName']
        self.InputFolder = os.path.join(self.root, p['InputFolder'])
        self.OutDir = os.path.join(self.root, p['OutputFolder'])
        self.OutputFolder = os.path.join(self.OutDir, self.ProjectName)

        self.Reference = os.path.join(self.InputFolder, p['RefDir']) if 'RefDir' in p else None
        self.PET = os.path.join(self.InputFolder, p['pet_dir']) if 'pet_dir' in p else self.InputFolder
        self.RunoffDir = os.path.join(self.InputFolder, p['RunoffDir']) if 'RunoffDir' in p else self.InputFolder
        self.RoutingDir = os.path.join(self.InputFolder, p['RoutingDir']) if 'RoutingDir' in p else self.InputFolder

        # project-level settings (ini_reader.py:117-142); the grid is hard-wired in the reference (:117-119) --
        # here ncell / ngridrow / ngridcol may be overridden for reduced test grids
        self.ncell = int(p.get('ncell', 67420))
        self.ngridrow = int(p.get('ngridrow', 360))
        self.ngridcol = int(p.get('ngridcol', 720))
        self.n_basins = int(p['n_basins'])
        # spelled 'True' / 'False' in the reference's examples; its own code compares the raw string in three different ways
        # (ini_reader.py:330 == 'False', :582 .lower() in [...], data_load.py:431 == "True"), so a config with 'false' or
        # 'F' would silently run a mix of both modes there.  Normalised once here: historic iff it reads as true.
        raw_hist = str(p.get('HistFlag', 'True')).strip()
        if raw_hist.lower() not in ('true', 't', 'yes', 'y', '1', 'false', 'f', 'no', 'n', '0'):
            raise ValidationException("HistFlag must be True or False, not '{}'".format(raw_hist))
        self.historic = raw_hist.lower() in ('true', 't', 'yes', 'y', '1')
        self.HistFlag = 'True' if self.historic else 'False'
        self.StartYear = int(p['StartYear'])
        self.EndYear = int(p['EndYear'])
        ov = p.get('output_vars', '')
        self.output_vars = ov if isinstance(ov, list) else [ov]
        for key in ('OutputFormat', 'OutputUnit', 'OutputInYear', 'AggregateRunoffBasin', 'AggregateRunoffCountry',
                    'AggregateRunoffGCAMRegion', 'PerformDiagnostics', 'CreateTimeSeriesPlot', 'CalculateDroughtStats',
                    'CalculateAccessibleWater', 'CalculateHydropowerPotential', 'CalculateHydropowerActual'):
            setattr(self, key, int(p.get(key, 0)))
        # every per-cell output also as a CF NetCDF map <same stem>_grid.nc (data_writer/gridded.py); not in the reference
        raw_grid = str(p.get('GriddedOutput', 0)).strip()
        if raw_grid not in ('0', '1'):
            raise ValidationException("GriddedOutput must be 0 or 1, not '{}'".format(raw_grid))
        self.GriddedOutput = int(raw_grid)
        self.calibrate = int(p.get('Calibrate', 0))
        self.nmonths = (self.EndYear - self.StartYear + 1) * 12
        self.device = int(p.get('device', 0))

        self.configure_pet(c.get('PET'))
        self.configure_runoff(c.get('Runoff'))
        self.configure_routing(c.get('Routing'))
        self.mod_cfg = '{0}_{1}_{2}'.format(self.pet_module, self.runoff_module, self.routing_module)
        if self.mod_cfg == 'none_none_none':
            raise ValidationException('No PET, Runoff, or Routing model selected.')
        self.configure_reference_data()
        # post-processors next to the hot path (ini_reader.py:85-98, 178-184)
        if c.get('Drought') and self.CalculateDroughtStats:
            self.configure_drought_stats(c['Drought'])
        if c.get('AccessibleWater') and self.CalculateAccessibleWater:
            if 'AccWatDir' not in p:
                raise ValidationException('CalculateAccessibleWater = 1 needs AccWatDir in [Project].')
            self.AccWatDir = os.path.join(self.InputFolder, p['AccWatDir'])
            self.configure_acc_water(c['AccessibleWater'])
        if self.PerformDiagnostics:
            self.configure_diagnostics(c, p)
        if self.CreateTimeSeriesPlot:
            self.configure_timeseries_plot(c)
        if self.CalculateHydropowerPotential or self.CalculateHydropowerActual:
            self.configure_hydropower(c, p)
        check_modules(self)
        if self.calibrate:
            if 'Calibrate' not in c:
                raise ValidationException('Calibrate = 1 but no [Calibrate] section.')
            self.configure_calibration(c['Calibrate'])
            check_calibration(self)
        self.ensemble = None
        if isinstance(c.get('Ensemble'), dict):
            self.configure_ensemble(c['Ensemble'])
        self.evaluate = None
        if isinstance(c.get('Evaluate'), dict):
            self.configure_evaluate(c['Evaluate'])
        # [DroughtIndex] (not in the reference): standardized drought indices of the run's runoff, soil moisture or routed flow
        raw_di = str(p.get('CalculateDroughtIndex', 0)).strip()
        if raw_di not in ('0', '1'):
            raise ValidationException("CalculateDroughtIndex must be 0 or 1, not '{}'".format(raw_di))
        self.CalculateDroughtIndex = int(raw_di)
        self.drought_index = None
        if self.CalculateDroughtIndex:
            if not isinstance(c.get('DroughtIndex'), dict):
                raise ValidationException('CalculateDroughtIndex = 1 but the config file has no [DroughtIndex] section.')
            self.configure_drought_index(c['DroughtIndex'])
        # [Trend] (not in the reference): Mann-Kendall test and Theil-Sen slope per cell of the run's results
        raw_tr = str(p.get('CalculateTrend', 0)).strip()
        if raw_tr not in ('0', '1'):
            raise ValidationException("CalculateTrend must be 0 or 1, not '{}'".format(raw_tr))
        self.CalculateTrend = int(raw_tr)
        self.trend = None
        if self.CalculateTrend:
            if not isinstance(c.get('Trend'), dict):
                raise ValidationException('CalculateTrend = 1 but the config file has no [Trend] section.')
            self.configure_trend(c['Trend'])
        # [Extremes] (not in the reference): annual maxima / minima per cell, the GEV by L-moments, return levels and periods
        raw_ex = str(p.get('CalculateExtremes', 0)).strip()
        if raw_ex not in ('0', '1'):
            raise ValidationException("CalculateExtremes must be 0 or 1, not '{}'".format(raw_ex))
        self.CalculateExtremes = int(raw_ex)
        self.extremes = None
        self.extremes_bootstrap = None
        if self.CalculateExtremes:
            if not isinstance(c.get('Extremes'), dict):
                raise ValidationException('CalculateExtremes = 1 but the config file has no [Extremes] section.')
            self.configure_extremes(c['Extremes'])
        # [Signatures] (not in the reference): the flow duration curve and the flow-regime signatures per cell
        raw_sg = str(p.get('CalculateSignatures', 0)).strip()
        if raw_sg not in ('0', '1'):
            raise ValidationException("CalculateSignatures must be 0 or 1, not '{}'".format(raw_sg))
        self.CalculateSignatures = int(raw_sg)
        self.signatures = None
        if self.CalculateSignatures:
            if not isinstance(c.get('Signatures'), dict):
                raise ValidationException('CalculateSignatures = 1 but the config file has no [Signatures] section.')
            self.configure_signatures(c['Signatures'])
        # [WaterBalance] (not in the reference): water balance and Budyko signatures per cell and per basin
        raw_wb = str(p.get('CalculateWaterBalance', 0)).strip()
        if raw_wb not in ('0', '1'):
            raise ValidationException("CalculateWaterBalance must be 0 or 1, not '{}'".format(raw_wb))
        self.CalculateWaterBalance = int(raw_wb)
        self.water_balance = None
        if self.CalculateWaterBalance:
            if not isinstance(c.get('WaterBalance'), dict):
                raise ValidationException('CalculateWaterBalance = 1 but the config file has no [WaterBalance] section.')
            self.configure_water_balance(c['WaterBalance'])

    # ------------------------------------------------------------------ modules
    def configure_pet(self, cfg):
        """[PET] / [[penman-monteith]] (ini_reader.py:198-300)."""
        if not cfg:
            self.pet_module = 'none'
            return
        self.pet_module = cfg['pet_module'].lower()
        if self.pet_module == 'pm':
            m = cfg['penman-monteith']
            self.pet_dir = os.path.join(self.PET, m['pet_dir'])
            for key in ('pm_tas', 'pm_tmin', 'pm_rhs', 'pm_rlds', 'pm_rsds', 'pm_wind', 'pm_lct'):
                setattr(self, key, os.path.join(self.pet_dir, m[key]))
            self.pm_nlcs = int(m['pm_nlcs'])
            self.pm_water_idx = int(m['pm_water_idx'])
            self.pm_snow_idx = int(m['pm_snow_idx'])
            years = m['pm_lc_years']
            self.pm_lc_years = [int(i) for i in (years if isinstance(years, list) else [years])]
            self.pm_params = os.path.join(self.pet_dir, 'gcam_ET_para.csv')
            self.pm_alpha = os.path.join(self.pet_dir, 'gcam_albedo.csv')
            self.pm_lai = os.path.join(self.pet_dir, 'gcam_lai.csv')
            self.pm_laimin = os.path.join(self.pet_dir, 'gcam_laimin.csv')
            self.pm_laimax = os.path.join(self.pet_dir, 'gcam_laimax.csv')
            self.pm_elev = os.path.join(self.pet_dir, 'elev.npy')
        elif self.pet_module == 'hargreaves':
            m = _subsection(cfg, 'hargreaves', 'PET')
            self.pet_dir = os.path.join(self.PET, _key(m, 'pet_dir', 'hargreaves'))
            # climate data (ini_reader.py:216-243): file names relative to pet_dir, optional NetCDF variable names
            self.TemperatureFile = os.path.join(self.pet_dir, _key(m, 'TemperatureFile', 'hargreaves'))
            self.TempVarName = m.get('TempVarName')
            self.DailyTemperatureRangeFile = os.path.join(self.pet_dir, _key(m, 'DailyTemperatureRangeFile', 'hargreaves'))
            self.DTRVarName = m.get('DTRVarName')
        elif self.pet_module == 'hs':
            m = _subsection(cfg, 'hargreaves-samani', 'PET')
            self.pet_dir = os.path.join(self.PET, _key(m, 'pet_dir', 'hargreaves-samani'))
            # climate data (ini_reader.py:245-252): file names relative to pet_dir
            for key in ('hs_tas', 'hs_tmin', 'hs_tmax'):
                setattr(self, key, os.path.join(self.pet_dir, _key(m, key, 'hargreaves-samani')))
        elif self.pet_module == 'thornthwaite':
            m = _subsection(cfg, 'thornthwaite', 'PET')
            self.pet_dir = os.path.join(self.PET, _key(m, 'pet_dir', 'thornthwaite'))
            self.trn_tas = os.path.join(self.pet_dir, _key(m, 'trn_tas', 'thornthwaite'))      # (ini_reader.py:281-287)
            # (not a key of the reference) which month's daylight each month gets.  `reference` (default): the order the
            # reference's np.repeat gives common years (thornthwaite.py:113); `monthly`: every month its own month's.
            self.trn_daylight = str(m.get('daylight', 'reference')).strip().lower()
            if self.trn_daylight not in ('reference', 'monthly'):
                raise ValidationException("[[thornthwaite]] daylight must be 'reference' or 'monthly', not '{}'".format(
                    self.trn_daylight))
        elif self.pet_module == 'none':
            try:
                self.pet_file = cfg['pet_file']
            except KeyError:
                raise ValidationException('USAGE: Must provide a pet_file variable in the PET config section that '
                                          'contains the full path to an input PET file if not using an existing module.')
        elif self.pet_module in self.PET_OTHER:
            raise ValidationException("PET module '{0}' belongs to the reference's CPU modules; this package implements "
                                      "the MI355X hot path only (pet_module = pm).".format(self.pet_module))
        else:
            raise ValidationException("ERROR: PET module '{0}' not found. Please check "
                                      "spelling and try again.".format(self.pet_module))

    def configure_runoff(self, cfg):
        """[Runoff] / [[abcd]] (ini_reader.py:302-388)."""
        if not cfg:
            self.runoff_module = 'none'
            return
        self.runoff_module = cfg['runoff_module'].lower()
        if self.runoff_module == 'abcd':
            m = cfg['abcd']
            self.ro_model_dir = os.path.join(self.RunoffDir, m['runoff_dir'])
            self.calib_file = os.path.join(self.ro_model_dir, m['calib_file'])
            self.runoff_spinup = int(m['runoff_spinup'])
            self.ro_jobs = int(m.get('jobs', -1))
            try:
                self.PrecipitationFile = m['PrecipitationFile']
            except KeyError:
                raise ValidationException('File path not provided for the PrecipitationFile variable in the ABCD '
                                          'runoff section of the config file.')
            self.PrecipVarName = m.get('PrecipVarName')
            self.TempMinFile = m.get('TempMinFile')
            self.TempMinVarName = m.get('TempMinVarName')
            # Future mode (HistFlag = False): channel storage at the end of the historical run.  The reference reads these
            # two keys only in its gwam section (ini_reader.py:322-338), so with abcd its loader silently starts from
            # zeros (data_load.py:427-438); here they are honoured in the abcd section as well.
            self.ChStorageFile = self.ChStorageVarName = None
            if not self.historic:
                self.ChStorageFile = m.get('ChStorageFile')
                self.ChStorageVarName = m.get('ChStorageVarName')
                if not self.ChStorageFile:
                    # the reference accepts this configuration and starts from empty channels (its abcd section never
                    # reads the key; load_chs_data, data_load.py:427-438, falls back to zeros): so does this package,
                    # loudly -- XH_STRICT_FUTURE=1 turns the warning into the error it almost always deserves
                    msg = ('HistFlag = False (future mode) without ChStorageFile (and ChStorageVarName for NetCDF) in the '
                           'runoff section: routing starts from EMPTY channels, as in the reference, instead of the '
                           'channel storage the historical run ended with.')
                    if os.environ.get('XH_STRICT_FUTURE') == '1':
                        raise ValidationException(msg)
                    logging.warning(msg)
        elif self.runoff_module == 'gwam':
            self.configure_gwam(_subsection(cfg, 'gwam', 'Runoff'))
        elif self.runoff_module == 'none':
            pass
        elif self.runoff_module in self.RUNOFF_OTHER:
            raise ValidationException("Runoff module '{0}' belongs to the reference's CPU modules; this package "
                                      "implements the MI355X hot path only (runoff_module = abcd).".format(self.runoff_module))
        else:
            raise ValidationException("ERROR: Runoff module '{0}' not found. Please check "
                                      "spelling and try again.".format(self.runoff_module))

    def configure_gwam(self, m):
        """[[gwam]] (ini_reader.py:311-350)."""
        self.ro_model_dir = os.path.join(self.RunoffDir, _key(m, 'runoff_dir', 'gwam'))
        try:
            self.runoff_spinup = int(_key(m, 'runoff_spinup', 'gwam'))
        except ValueError:
            raise ValidationException('runoff_spinup in [[gwam]] must be an integer')
        # built-in files: maximum soil moisture and the two water-body tables
        for key in ('max_soil_moisture', 'lakes_msm', 'addit_water_msm'):
            setattr(self, key, os.path.join(self.ro_model_dir, _key(m, key, 'gwam')))
        # future mode: channel storage and soil moisture at the end of the historical run, all four keys required
        self.ChStorageFile = self.ChStorageVarName = self.SavFile = self.SavVarName = None
        if not self.historic:
            missing = [k for k in ('ChStorageFile', 'ChStorageVarName', 'SavFile', 'SavVarName') if k not in m]
            if missing:
                raise ValidationException('Error: ChStorageFile, ChStorageVarName, SavFile and SavVarName are required '
                                          'in [[gwam]] for Future Mode (missing: {}).'.format(', '.join(missing)))
            self.ChStorageFile, self.ChStorageVarName = m['ChStorageFile'], m['ChStorageVarName']
            self.SavFile, self.SavVarName = m['SavFile'], m['SavVarName']
        self.PrecipitationFile = os.path.join(self.ro_model_dir, _key(m, 'PrecipitationFile', 'gwam'))
        self.PrecipVarName = m.get('PrecipVarName')
        # (not a key of the reference) which precipitation GWAM reads.  `reference` (default): what the reference's driver
        # hands it -- ONE column for every month of a pass, runoff_spinup - 1 in the spin-up and nmonths - 1 in the
        # simulation (components.py:230, :334).  `monthly`: month m's precipitation in month m.
        self.gwam_precipitation = str(m.get('precipitation', 'reference')).strip().lower()
        if self.gwam_precipitation not in ('reference', 'monthly'):
            raise ValidationException("[[gwam]] precipitation must be 'reference' or 'monthly', not '{}'".format(
                self.gwam_precipitation))

    def configure_routing(self, cfg):
        """[Routing] / [[mrtm]] (ini_reader.py:390-423)."""
        if not cfg:
            self.routing_module = 'none'
            return
        self.routing_module = cfg['routing_module'].lower()
        if self.routing_module == 'mrtm':
            m = cfg['mrtm']
            self.rt_model_dir = os.path.join(self.RoutingDir, m['routing_dir'])
            self.strm_veloc = os.path.join(self.rt_model_dir, m['channel_velocity'])
            self.flow_distance = os.path.join(self.rt_model_dir, m['flow_distance'])
            self.flow_direction = os.path.join(self.rt_model_dir, m['flow_direction'])
            self.routing_spinup = int(m['routing_spinup']) if 'routing_spinup' in m else self.nmonths
            alt = m.get('alt_runoff')
            self.alt_runoff = None if alt in (None, 'none') else os.path.join(self.rt_model_dir, alt)
            # (not a key of the reference) which form of the routing kernel: `reassociated` -- row sums as running sums along
            # chains of lanes, equal to the reference to rounding (<= 1e-9 relative; NOT bit for bit), twice as fast --, `exact`
            # -- every sum in scipy's stored order, ChStorage / Avg_ChFlow bit-identical to the reference --, or `default`: the
            # library's, which is `reassociated` since round 5 (XH_ROUTE_REASSOC=0 in the environment makes it `exact`)
            # (not a key of the reference) per-basin scales of the channel velocity, as a calibration with
            # calibrate_velocity = 1 writes them: csv basin_id,scale relative to the routing directory; the loader
            # multiplies the velocity of every cell by its basin's scale (basins not listed: 1)
            vs = m.get('velocity_scale')
            self.velocity_scale_file = None if vs in (None, 'none') else os.path.join(self.rt_model_dir, vs)
            self.routing_form = str(m.get('routing_form', 'default')).strip().lower()
            if self.routing_form not in ('default', 'reassociated', 'exact'):
                raise ValidationException("routing_form must be 'reassociated', 'exact' or 'default', not '{}'".format(
                    self.routing_form))
        elif self.routing_module == 'none':
            pass
        else:
            raise ValidationException("ERROR: Routing module '{0}' not found. Please check "
                                      "spelling and try again.".format(self.routing_module))

    def configure_reference_data(self):
        """Reference grid files (ini_reader.py:425-437); only the ones the hot path reads."""
        if self.Reference:
            self.Area = os.path.join(self.Reference, 'Grid_Areas_ID.csv')
            self.Coord = os.path.join(self.Reference, 'coordinates.csv')
            self.BasinIDs = os.path.join(self.Reference, 'basin.csv')
            self.BasinNames = os.path.join(self.Reference, 'BasinNames235.txt')
            self.GCAMRegionIDs = os.path.join(self.Reference, 'region32_grids.csv')
            self.GCAMRegionNames = os.path.join(self.Reference, 'Rgn32Names.csv')
            self.CountryIDs = os.path.join(self.Reference, 'country.csv')
            self.CountryNames = os.path.join(self.Reference, 'country-names.csv')

    def configure_drought_stats(self, cfg):
        """[Drought] (ini_reader.py:460-471)."""
        self.drought_var = cfg['drought_var']
        self.drought_thresholds = cfg.get('drought_thresholds')            # optional: thresholds file of an earlier run
        if self.drought_thresholds is None:
            self.threshold_nper = int(cfg['threshold_nper'])
            self.threshold_start_year = int(cfg['threshold_start_year'])
            self.threshold_end_year = int(cfg['threshold_end_year'])
            if self.StartYear > self.threshold_start_year or self.EndYear < self.threshold_end_year:
                raise ValidationException('Drought threshold year range is outside the output year range.')

    def configure_acc_water(self, cfg):
        """[AccessibleWater] (ini_reader.py:473-486)."""
        self.ResCapacityFile = os.path.join(self.AccWatDir, cfg['ResCapacityFile'])
        self.BfiFile = os.path.join(self.AccWatDir, cfg['BfiFile'])
        self.HistEndYear = int(cfg['HistEndYear'])
        self.GCAM_StartYear = self.ck_year(int(cfg['GCAM_StartYear']))
        self.GCAM_EndYear = int(cfg['GCAM_EndYear'])
        self.GCAM_YearStep = int(cfg['GCAM_YearStep'])
        self.MovingMeanWindow = int(cfg['MovingMeanWindow'])
        self.Env_FlowPercent = float(cfg['Env_FlowPercent'])
        if self.StartYear > self.GCAM_StartYear or self.EndYear < self.GCAM_EndYear:
            raise ValidationException('Accessible water range of GCAM years are outside the range of years in climate data.')

    def configure_hydropower(self, c, p):
        """[HydropowerPotential] / [HydropowerActual] (ini_reader.py:95-105, :488-504).  HydActDir is read whenever either
        switch is on (the reference reads it only with [HydropowerActual], so potential alone dies there)."""
        if 'HydActDir' not in p:
            raise ValidationException('CalculateHydropowerPotential / CalculateHydropowerActual = 1 needs HydActDir in '
                                      '[Project].')
        if self.routing_module == 'none':
            raise ValidationException('the hydropower post-processors read the routed channel flow (Avg_ChFlow): they need '
                                      'routing_module = mrtm, not none.')
        self.HydActDir = os.path.join(self.InputFolder, p['HydActDir'])
        self.GridData = os.path.join(self.HydActDir, 'gridData.csv')
        try:
            with open(self.GridData) as fh:
                nrows = sum(1 for line in fh if line.strip()) - 1
        except OSError as exc:
            raise ValidationException('cannot read the hydropower grid data {}: {}'.format(self.GridData, exc))
        if nrows != self.ncell:
            raise ValidationException('{} has {} rows; its rows are matched to the {} cells by position.'.format(
                self.GridData, nrows, self.ncell))
        if self.CalculateHydropowerPotential:
            m = self._hydro_section(c, 'HydropowerPotential')
            self.hpot_start_date = self._month(m, 'hpot_start_date', 'HydropowerPotential')
            try:
                self.q_ex = float(self._hydro_key(m, 'q_ex', 'HydropowerPotential'))
                self.ef = float(self._hydro_key(m, 'ef', 'HydropowerPotential'))
            except ValueError as exc:
                raise ValidationException('[HydropowerPotential]: {}'.format(exc))
            if not 0.0 <= self.q_ex <= 1.0:
                raise ValidationException('[HydropowerPotential] q_ex = {} is a quantile and must lie in [0, 1].'.format(
                    self.q_ex))
        if self.CalculateHydropowerActual:
            m = self._hydro_section(c, 'HydropowerActual')
            self.hact_start_date = self._month(m, 'hact_start_date', 'HydropowerActual')
            self.HydroDamData = os.path.join(self.HydActDir, 'resData_1593.csv')
            self.MissingCap = os.path.join(self.HydActDir, 'simulated_cap_by_country.csv')
            self.rule_curves = os.path.join(self.HydActDir, 'rule_curves_1593.npy')
            self.DrainArea = os.path.join(self.HydActDir, 'DRT_half_SourceArea_globe_float.txt')

    def configure_diagnostics(self, c, p):
        """DiagDir and [Diagnostics] (ini_reader.py:74-78, :439-445).  The reference skips this when the section or DiagDir is
        missing and then dies with an AttributeError in the loader; here that is refused by the flag's name."""
        m = c.get('Diagnostics')
        if not isinstance(m, dict):
            raise ValidationException('PerformDiagnostics = 1 but the config file has no [Diagnostics] section.')
        if 'DiagDir' not in p:
            raise ValidationException('PerformDiagnostics = 1 needs DiagDir in [Project].')
        self.DiagDir = os.path.join(self.InputFolder, p['DiagDir'])
        for key in ('VICDataFile', 'UNHDataFile', 'WBMDataFile', 'WBMCDataFile'):
            setattr(self, key, os.path.join(self.DiagDir, self._hydro_key(m, key, 'Diagnostics')))
        self.DiagnosticScale = self._int(m, 'Scale', 'Diagnostics')

    def configure_timeseries_plot(self, c):
        """[TimeSeriesPlot] (ini_reader.py:79-83, :447-458): Scale, and MapID as one integer (999: every row) or a list."""
        m = c.get('TimeSeriesPlot')
        if not isinstance(m, dict):
            raise ValidationException('CreateTimeSeriesPlot = 1 but the config file has no [TimeSeriesPlot] section.')
        self.TimeSeriesScale = self._int(m, 'Scale', 'TimeSeriesPlot')
        raw = self._hydro_key(m, 'MapID', 'TimeSeriesPlot')
        try:
            self.TimeSeriesMapID = [int(v) for v in raw] if isinstance(raw, list) else int(raw)
        except ValueError as exc:
            raise ValidationException('[TimeSeriesPlot] MapID = {!r} is not an integer or a list of integers: {}'.format(
                raw, exc))

    @classmethod
    def _int(cls, m, key, name):
        raw = cls._hydro_key(m, key, name)
        try:
            return int(raw)
        except (TypeError, ValueError):
            raise ValidationException('[{}] {} = {!r} is not an integer.'.format(name, key, raw))

    @staticmethod
    def _hydro_section(c, name):
        m = c.get(name)
        if not isinstance(m, dict):
            raise ValidationException('Calculate{0} = 1 but the config file has no [{0}] section.'.format(name))
        return m

    @staticmethod
    def _hydro_key(m, key, name):
        if key not in m:
            raise ValidationException('{} is required in the [{}] section of the config file.'.format(key, name))
        return m[key]

    @classmethod
    def _month(cls, m, key, name):
        """A start month in the reference's "M/YYYY" form, kept as written (the modules hand it to pd.period_range)."""
        text = str(cls._hydro_key(m, key, name)).strip()
        import pandas as pd
        try:
            pd.Period(text, freq='M')
        except (ValueError, TypeError) as exc:
            raise ValidationException('[{}] {} = {!r} is not a month ("M/YYYY"): {}'.format(name, key, text, exc))
        return text

    def ck_year(self, yr):
        """A year inside the run (ini_reader.py:547-551)."""
        if yr < self.StartYear or yr > self.EndYear:
            raise ValidationException('Accessible water year {0} is outside the range of years in the climate data.'.format(yr))
        return yr

    def configure_calibration(self, cfg):
        """[Calibrate] (ini_reader.py:506-519)."""
        self.set_calibrate = int(cfg['set_calibrate'])
        # stream gauges inside the network (set_calibrate = 1 only): `gauges` = csv gauge_id,cell_id[,weight] (cell_id
        # 1-based, as the coordinates' first column), `gauge_observed` = the four-column layout of `observed` with the
        # gauge id in column 0 (nmonths rows per gauge in month order, value in column 3, NaN = missing), `gauge_missing`
        # = a sentinel value also read as missing.  `observed` is not required when they are given.
        self.cal_gauges = cfg.get('gauges')
        self.cal_gauge_observed = cfg.get('gauge_observed')
        self.cal_gauge_missing = None if cfg.get('gauge_missing') is None else float(cfg['gauge_missing'])
        given = [k for k in ('gauges', 'gauge_observed', 'gauge_missing') if cfg.get(k) is not None]
        if given and self.set_calibrate != 1:
            raise ValidationException('[Calibrate] {} is valid only with set_calibrate = 1 (calibration against routed '
                                      'streamflow); set_calibrate = {}.'.format(', '.join(given), self.set_calibrate))
        if (self.cal_gauges is None) != (self.cal_gauge_observed is None):
            raise ValidationException('[Calibrate] gauges and gauge_observed go together: the stations and their records.')
        if self.cal_gauges is None and 'observed' not in cfg:
            raise ValidationException('[Calibrate] needs observed (or, with set_calibrate = 1, gauges and gauge_observed).')
        self.cal_observed = cfg.get('observed')
        # (not keys of the reference) calibrate_velocity = 1: the streamflow objective also calibrates one velocity scale
        # per basin inside velocity_scale_bounds = lo, hi (default 0.25, 4: a choice, not a measurement)
        try:
            self.calibrate_velocity = int(cfg.get('calibrate_velocity', 0))
        except (TypeError, ValueError):
            self.calibrate_velocity = -1
        if self.calibrate_velocity not in (0, 1):
            raise ValidationException('[Calibrate] calibrate_velocity = {!r} must be 0 or 1.'.format(
                cfg.get('calibrate_velocity')))
        if self.calibrate_velocity and self.set_calibrate != 1:
            raise ValidationException('[Calibrate] calibrate_velocity = 1 calibrates the channel velocity against routed '
                                      'streamflow and needs set_calibrate = 1; set_calibrate = {}.'.format(
                                          self.set_calibrate))
        raw = cfg.get('velocity_scale_bounds')
        if raw is not None and not self.calibrate_velocity:
            raise ValidationException('[Calibrate] velocity_scale_bounds is valid only with calibrate_velocity = 1.')
        self.velocity_scale_bounds = None
        if self.calibrate_velocity:
            from .calibrate.velocity_scale import DEFAULT_BOUNDS, check_bounds
            if raw is None:
                raw = DEFAULT_BOUNDS
            elif not isinstance(raw, (list, tuple)):
                raw = [x for x in str(raw).replace(',', ' ').split()]
            self.velocity_scale_bounds = check_bounds(raw, '[Calibrate] velocity_scale_bounds')
        self.obs_unit = self.ck_obs_unit(self.set_calibrate, cfg['obs_unit'])
        self.calib_out_dir = cfg['calib_out_dir']
        basins = cfg.get('calibration_basins')
        if basins is None:
            self.cal_basins = ['1-{}'.format(self.n_basins)]
        else:
            self.cal_basins = basins if isinstance(basins, list) else [basins]

    def forcing_settings(self):
        """{setting: directory attribute or None} of the forcing arrays of the configured PET and runoff modules."""
        out = dict(FORCING_SETTINGS.get(self.pet_module, {}))
        out.update(FORCING_SETTINGS.get(self.runoff_module, {}))
        return out

    def resolve_forcing_setting(self, key, value):
        """``value`` as the ini's ``key = value`` would be stored (a path joined to the module's directory, or as written)."""
        where = self.forcing_settings()
        if key not in where:
            raise ValidationException("'{}' does not name a forcing array of pet_module = {} / runoff_module = {}.".format(
                key, self.pet_module, self.runoff_module))
        return value if where[key] is None else os.path.join(getattr(self, where[key]), value)

    def configure_ensemble(self, cfg):
        """[Ensemble] (not a section of the reference): members = <csv> (header ``name`` + forcing settings, one row per
        member, an empty cell keeps the ini's value), statistics = mean, std, min, max, qNN (default: none),
        statistics_vars (default: output_vars), member_outputs = 1 | 0.  The table may have a column ``abcd_pars``: a
        member's own ABCD parameter table (.npy, resolved as calib_file is).  observed = <file> (the format of [Calibrate]
        observed: rows [basin id, *, *, value], months in order) with obs_unit = km3_per_mth | mm_per_mth: every member's
        KGE against it is written to ensemble/member_kge.csv (ensemble.load_observed checks both).  Kept as
        ``self.ensemble``; model.run_model hands a configuration that has it to ensemble.run_ensemble."""
        if self.calibrate:
            raise ValidationException('[Ensemble] and Calibrate = 1 ([Calibrate]) exclude each other: a calibration is '
                                      'not a member run.')
        if 'members' not in cfg:
            raise ValidationException('members is required in the [Ensemble] section of the config file.')
        path = cfg['members'] if isinstance(cfg['members'], str) else ','.join(cfg['members'])
        path = path if os.path.isabs(path) else os.path.join(self.root, path)

        def as_list(v):
            return [] if v in (None, '') else ([x for x in v if x != ''] if isinstance(v, list) else [v])
        stats = as_list(cfg.get('statistics'))
        for t in stats:
            parse_statistic(t)
        try:
            member_outputs = int(cfg.get('member_outputs', 1))
        except (TypeError, ValueError):
            member_outputs = -1
        if member_outputs not in (0, 1):
            raise ValidationException('[Ensemble] member_outputs = {!r} must be 0 or 1.'.format(cfg.get('member_outputs')))
        self.ensemble = {'members': path, 'statistics': stats,
                         'statistics_vars': as_list(cfg.get('statistics_vars')) or None, 'member_outputs': member_outputs}
        if 'observed' in cfg or 'obs_unit' in cfg:
            if 'observed' not in cfg:
                raise ValidationException('[Ensemble] obs_unit is given without observed.')
            obs = cfg['observed'] if isinstance(cfg['observed'], str) else ','.join(cfg['observed'])
            self.ensemble['observed'] = obs if os.path.isabs(obs) else os.path.join(self.root, obs)
            self.ensemble['obs_unit'] = cfg.get('obs_unit')

    def configure_evaluate(self, cfg):
        """[Evaluate] (not a section of the reference): gauges / gauge_observed / gauge_missing, the file formats, path
        resolution and meaning of the [Calibrate] keys of the same names (the weight column is read and ignored).  A
        forward run, or every member of an ensemble, is scored at these stream gauges on its routed flow
        (evaluate/gauge_skill.py).  Kept as ``self.evaluate``."""
        if self.calibrate:
            raise ValidationException('[Evaluate] gauges and Calibrate = 1 exclude each other: the calibration scores its own '
                                      'gauges and writes its own gauge_kge.csv.')
        if self.routing_module != 'mrtm':
            raise ValidationException("[Evaluate] gauges are scored on the routed channel flow (Avg_ChFlow): the run needs "
                                      "routing_module = mrtm, not '{}'.".format(self.routing_module))
        if (cfg.get('gauges') is None) != (cfg.get('gauge_observed') is None):
            raise ValidationException('[Evaluate] {} is missing: gauges and gauge_observed go together, the stations and their '
                                      'records.'.format('gauges' if cfg.get('gauges') is None else 'gauge_observed'))
        if cfg.get('gauges') is None:
            raise ValidationException('[Evaluate] needs gauges and gauge_observed.')
        try:
            missing = None if cfg.get('gauge_missing') is None else float(cfg['gauge_missing'])
        except (TypeError, ValueError):
            raise ValidationException('[Evaluate] gauge_missing = {!r} is not a number.'.format(cfg.get('gauge_missing')))
        self.evaluate = {'gauges': cfg['gauges'], 'gauge_observed': cfg['gauge_observed'], 'gauge_missing': missing}

    DROUGHT_INDEX_VARS = ('q', 'soilmoisture', 'avgchflow', 'precip', 'balance')
    DROUGHT_INDEX_DISTRIBUTIONS = ('gamma', 'empirical', 'loglogistic')

    def configure_drought_index(self, cfg):
        """[DroughtIndex] (not a section of the reference; drought/standardized.py): index_var = q | soilmoisture | avgchflow
        | precip | balance (SRI / SSI / SSFI of the run's results; SPI of its precipitation, SPEI of precipitation minus the
        PET module's PET), scales = up to 8 accumulation scales of 1 - 48 months, distribution = gamma (default) |
        empirical | loglogistic (SPEI's own: balance is negative half the time, where gamma fits nothing),
        reference_start_year / reference_end_year (default: the run's years), parameters = <stem> (gamma and loglogistic:
        index against the fit of an earlier run instead of fitting; <stem> = <that run's OutputFolder>/<its
        OutputNameStr>, the table of scale k being <folder>/drought_index_<var>_<k>m_parameters_<name>.npy as that run wrote
        it, ..._llparameters_... with loglogistic, whose tables hold other columns -- or any file name with ``{k}`` standing
        for the scale; relative to RootDir unless absolute), max_shape (default 1000).  Kept as ``self.drought_index``;
        'parameters' there is {k: file} or None."""
        def refuse(key, why):
            raise ValidationException('[DroughtIndex] {} {}'.format(key, why))
        var = str(cfg.get('index_var', '')).strip().lower()
        if var not in self.DROUGHT_INDEX_VARS:
            refuse('index_var', "= '{}' must be one of {}.".format(cfg.get('index_var'), ', '.join(self.DROUGHT_INDEX_VARS)))
        if var == 'avgchflow' and self.routing_module != 'mrtm':
            refuse('index_var', "= avgchflow is the routed channel flow: the run needs routing_module = mrtm, not '{}'.".format(
                self.routing_module))
        if var in ('precip', 'balance') and self.runoff_module == 'none':
            refuse('index_var', "= {} is the index of the run's precipitation, which the runoff module loads: the run needs a "
                   "runoff_module, not 'none'.".format(var))
        if var == 'balance' and self.pet_module == 'none':
            refuse('index_var', "= balance is precipitation minus PET: the run needs a pet_module, not 'none'.")
        if self.OutputInYear:
            refuse('needs OutputInYear = 0:', 'the index is monthly and is written with the monthly column labels.')
        if self.calibrate:
            refuse('and Calibrate = 1', 'exclude each other: a calibration writes no outputs to index.')
        raw = cfg.get('scales')
        raw = [] if raw in (None, '') else (raw if isinstance(raw, list) else [raw])
        try:
            scales = [int(x) for x in raw]
        except (TypeError, ValueError):
            refuse('scales', '= {!r} are not integers.'.format(cfg.get('scales')))
        if not 1 <= len(scales) <= 8 or any(k < 1 or k > 48 for k in scales) or len(set(scales)) != len(scales):
            refuse('scales', '= {!r}: 1 to 8 different accumulation scales of 1 to 48 months.'.format(cfg.get('scales')))
        dist = str(cfg.get('distribution', 'gamma')).strip().lower()
        if dist not in self.DROUGHT_INDEX_DISTRIBUTIONS:
            refuse('distribution', "= '{}' must be gamma, empirical or loglogistic.".format(cfg.get('distribution')))
        years = {}
        for key, default in (('reference_start_year', self.StartYear), ('reference_end_year', self.EndYear)):
            try:
                years[key] = int(cfg.get(key, default))
            except (TypeError, ValueError):
                refuse(key, '= {!r} is not a year.'.format(cfg.get(key)))
            if not self.StartYear <= years[key] <= self.EndYear:
                refuse(key, '= {} lies outside the years of the run, {} - {}.'.format(years[key], self.StartYear, self.EndYear))
        if years['reference_end_year'] < years['reference_start_year']:
            refuse('reference_end_year', '= {} lies before reference_start_year = {}.'.format(
                years['reference_end_year'], years['reference_start_year']))
        try:
            max_shape = float(cfg.get('max_shape', 1000.0))
        except (TypeError, ValueError):
            max_shape = float('nan')
        if not max_shape > 0:
            refuse('max_shape', '= {!r} must be a positive number.'.format(cfg.get('max_shape')))
        stem = cfg.get('parameters')
        files = None
        if stem is not None:
            if dist == 'empirical':
                refuse('parameters', 'has no meaning with distribution = empirical: nothing is fitted there.')
            import numpy as np
            stem = stem if isinstance(stem, str) else ','.join(stem)
            stem = stem if os.path.isabs(stem) else os.path.join(self.root, stem)
            files = {}
            # (a log-logistic table is (alpha, beta, gamma, n), a gamma table (q0, alpha, beta, n): each under its own name)
            word = 'llparameters' if dist == 'loglogistic' else 'parameters'
            for k in scales:
                path = stem.replace('{k}', str(k)) if '{k}' in stem else os.path.join(
                    os.path.dirname(stem), 'drought_index_{}_{}m_{}_{}.npy'.format(var, k, word, os.path.basename(stem)))
                try:
                    shape = np.load(path, mmap_mode='r').shape
                except (OSError, ValueError) as exc:
                    refuse('parameters', '= {}: cannot read {} for scale {}: {}'.format(cfg.get('parameters'), path, k, exc))
                if tuple(shape) != (self.ncell, 12, 4):
                    refuse('parameters', '= {}: {} has shape {}, the run needs [{}, 12, 4] (cells, calendar months, {}).'
                           .format(cfg.get('parameters'), path, tuple(shape), self.ncell,
                                   'alpha / beta / gamma / n' if dist == 'loglogistic' else 'q0 / alpha / beta / n'))
                files[k] = path
        self.drought_index = {'var': var, 'scales': scales, 'distribution': dist,
                              'reference_start_year': years['reference_start_year'],
                              'reference_end_year': years['reference_end_year'], 'max_shape': max_shape, 'parameters': files}

    def configure_trend(self, cfg):
        """[Trend] (not a section of the reference; trend/trend.py): trend_vars = a list from q | pet | aet | soilmoisture |
        avgchflow | precip; series = a list from annual (the yearly series, plain Mann-Kendall test) | seasonal (the monthly
        series, seasonal Kendall test over the 12 calendar months); annual = sum | mean (how a year is formed; default: sum
        for q, pet, aet and precip -- a NaN month makes the year NaN --, mean for soilmoisture and avgchflow);
        start_year / end_year (default: the run's years; whole years inside the run, at least 4); confidence (default 0.95)
        of the slope's interval.  Kept as ``self.trend``; 'annual' there is {var: 'sum' | 'mean'}."""
        from .trend.trend import ANNUAL_DEFAULT, MAX_COLS, MIN_YEARS, SERIES, VARS

        def refuse(key, why):
            raise ValidationException('[Trend] {} {}'.format(key, why))

        def words(key):
            raw = cfg.get(key)
            raw = [] if raw in (None, '') else (raw if isinstance(raw, list) else [raw])
            return [str(w).strip().lower() for w in raw]
        if self.calibrate:
            refuse('and Calibrate = 1', 'exclude each other: a calibration writes no outputs to test for a trend.')
        if getattr(self, 'ensemble', None) is not None:
            refuse('and an [Ensemble] section', 'exclude each other: per-member trends are not implemented.')
        tvars = words('trend_vars')
        if not tvars or len(set(tvars)) != len(tvars) or any(v not in VARS for v in tvars):
            refuse('trend_vars', '= {!r} must be different names from {}.'.format(cfg.get('trend_vars'), ', '.join(VARS)))
        if 'avgchflow' in tvars and self.routing_module != 'mrtm':
            refuse('trend_vars', "= avgchflow is the routed channel flow: the run needs routing_module = mrtm, not '{}'.".format(
                self.routing_module))
        for v in tvars:
            if v in ('q', 'aet', 'soilmoisture', 'precip') and self.runoff_module == 'none':
                refuse('trend_vars', "= {} comes from (precip: is loaded by) the runoff module: the run needs a runoff_module, not "
                       "'none'.".format(v))
            if v == 'pet' and self.pet_module == 'none':
                refuse('trend_vars', "= pet is the PET module's result: the run needs a pet_module, not 'none'.")
        series = words('series')
        if not series or len(set(series)) != len(series) or any(w not in SERIES for w in series):
            refuse('series', '= {!r} must be different names from {}.'.format(cfg.get('series'), ', '.join(SERIES)))
        annual = dict(ANNUAL_DEFAULT)
        if cfg.get('annual') is not None:
            how = str(cfg.get('annual')).strip().lower()
            if how not in ('sum', 'mean'):
                refuse('annual', "= '{}' must be sum or mean.".format(cfg.get('annual')))
            annual = {v: how for v in VARS}
        years = {}
        for key, default in (('start_year', self.StartYear), ('end_year', self.EndYear)):
            try:
                years[key] = int(cfg.get(key, default))
            except (TypeError, ValueError):
                refuse(key, '= {!r} is not a year.'.format(cfg.get(key)))
            if not self.StartYear <= years[key] <= self.EndYear:
                refuse(key, '= {} lies outside the years of the run, {} - {}.'.format(years[key], self.StartYear, self.EndYear))
        nyears = years['end_year'] - years['start_year'] + 1
        if nyears < MIN_YEARS:
            refuse('end_year', '= {}: the window {} - {} is shorter than the {} years a trend needs.'.format(
                years['end_year'], years['start_year'], years['end_year'], MIN_YEARS))
        if 'seasonal' in series and 12 * nyears > MAX_COLS:
            refuse('series', '= seasonal: the window {} - {} has {} months, more than the {} one row may take.'.format(
                years['start_year'], years['end_year'], 12 * nyears, MAX_COLS))
        try:
            confidence = float(cfg.get('confidence', 0.95))
        except (TypeError, ValueError):
            confidence = float('nan')
        if not 0.5 < confidence < 1.0:
            refuse('confidence', '= {!r} must lie between 0.5 and 1.'.format(cfg.get('confidence')))
        self.trend = {'vars': tvars, 'series': series, 'annual': annual, 'start_year': years['start_year'],
                      'end_year': years['end_year'], 'confidence': confidence}

    def configure_extremes(self, cfg):
        """[Extremes] (not a section of the reference; extremes/extremes.py): extreme_vars = a list from q | pet | aet |
        soilmoisture | avgchflow | precip; kinds = a list from max | min; return_periods (default 2, 5, 10, 20, 50, 100; at
        most 8, different, each > 1); start_year / end_year (default: the run's; the years in which the first and the last
        year of the window start); year_start_month (1 - 12, default 1: a hydrological year runs from that month to the month
        before it a year later, and the last one must end inside the run); min_years (default 10, at least 5): the years a
        fit needs; parameters (optional) = <OutputFolder>/<OutputNameStr> of a historic run, whose tables stand in for the
        fit.  Kept as ``self.extremes``; 'parameters' there is {(var, kind): file} or None.
        bootstrap (100 - 2048; absent or 0: off) = the replicates of the percentile-bootstrap confidence intervals of the shape
        and the return levels, confidence (default 0.90, strictly between 0 and 1) their level, bootstrap_seed
        (default 1, a whole number >= 0) what the draws start from.  Kept apart as ``self.extremes_bootstrap``: None or {'B',
        'confidence', 'seed'}.  Not together with parameters: a handed-in fit has no sample of this run to resample."""
        import numpy as np
        from .extremes.extremes import BOOTSTRAP_MAX, BOOTSTRAP_MIN, CONFIDENCE_DEFAULT, KINDS, MAX_COLS, MAX_PERIODS, MIN_YEARS, MIN_YEARS_DEFAULT, RETURN_PERIODS, VARS, parameter_file

        def refuse(key, why):
            raise ValidationException('[Extremes] {} {}'.format(key, why))

        def words(key):
            raw = cfg.get(key)
            raw = [] if raw in (None, '') else (raw if isinstance(raw, list) else [raw])
            return [str(w).strip().lower() for w in raw]
        if self.calibrate:
            refuse('and Calibrate = 1', 'exclude each other: a calibration writes no outputs to take extremes of.')
        if getattr(self, 'ensemble', None) is not None:
            refuse('and an [Ensemble] section', 'exclude each other: per-member extremes are not implemented.')
        if getattr(self, 'OutputInYear', 0) == 1:
            refuse('and OutputInYear = 1', 'exclude each other: the extremes are those of the monthly series.')
        evars = words('extreme_vars')
        if not evars or len(set(evars)) != len(evars) or any(v not in VARS for v in evars):
            refuse('extreme_vars', '= {!r} must be different names from {}.'.format(cfg.get('extreme_vars'), ', '.join(VARS)))
        if 'avgchflow' in evars and self.routing_module != 'mrtm':
            refuse('extreme_vars', "= avgchflow is the routed channel flow: the run needs routing_module = mrtm, not '{}'.".format(
                self.routing_module))
        for v in evars:
            if v in ('q', 'aet', 'soilmoisture', 'precip') and self.runoff_module == 'none':
                refuse('extreme_vars', "= {} comes from (precip: is loaded by) the runoff module: the run needs a runoff_module, "
                       "not 'none'.".format(v))
            if v == 'pet' and self.pet_module == 'none':
                refuse('extreme_vars', "= pet is the PET module's result: the run needs a pet_module, not 'none'.")
        kinds = words('kinds')
        if not kinds or len(set(kinds)) != len(kinds) or any(w not in KINDS for w in kinds):
            refuse('kinds', '= {!r} must be different names from {}.'.format(cfg.get('kinds'), ', '.join(KINDS)))
        periods = list(RETURN_PERIODS)
        if cfg.get('return_periods') not in (None, ''):
            raw = cfg.get('return_periods')
            try:
                periods = [float(w) for w in (raw if isinstance(raw, list) else [raw])]
            except (TypeError, ValueError):
                periods = []
            if not periods or len(periods) > MAX_PERIODS or len(set(periods)) != len(periods) or not all(
                    T > 1.0 and T < float('inf') for T in periods):
                refuse('return_periods', '= {!r} must be at most {} different numbers, each > 1.'.format(raw, MAX_PERIODS))
        try:
            month = int(cfg.get('year_start_month', 1))
        except (TypeError, ValueError):
            month = 0
        if not 1 <= month <= 12:
            refuse('year_start_month', '= {!r} must be a month, 1 - 12.'.format(cfg.get('year_start_month')))
        try:
            min_years = int(cfg.get('min_years', MIN_YEARS_DEFAULT))
        except (TypeError, ValueError):
            min_years = 0
        if min_years < MIN_YEARS:
            refuse('min_years', '= {!r} must be a whole number, at least {}.'.format(cfg.get('min_years'), MIN_YEARS))
        # the last year that starts in month `month` and ends inside the run
        last_start = self.EndYear if month == 1 else self.EndYear - 1
        years = {}
        for key, default in (('start_year', self.StartYear), ('end_year', last_start)):
            try:
                years[key] = int(cfg.get(key, default))
            except (TypeError, ValueError):
                refuse(key, '= {!r} is not a year.'.format(cfg.get(key)))
            if not self.StartYear <= years[key] <= self.EndYear:
                refuse(key, '= {} lies outside the years of the run, {} - {}.'.format(years[key], self.StartYear, self.EndYear))
        if years['end_year'] > last_start:
            refuse('end_year', '= {}: the year that starts in month {} of {} ends after the run ({}); the last complete one '
                   'starts in {}.'.format(years['end_year'], month, years['end_year'], self.EndYear, last_start))
        nyears = years['end_year'] - years['start_year'] + 1
        if nyears < min_years:
            refuse('end_year', '= {}: the window {} - {} has {} years, fewer than min_years = {}.'.format(
                years['end_year'], years['start_year'], years['end_year'], max(nyears, 0), min_years))
        if 12 * nyears > MAX_COLS:
            refuse('end_year', '= {}: the window {} - {} has {} months, more than the {} one row may take.'.format(
                years['end_year'], years['start_year'], years['end_year'], 12 * nyears, MAX_COLS))
        files = None
        if cfg.get('parameters') not in (None, ''):
            stem = str(cfg.get('parameters')).strip()
            files = {}
            for v in evars:
                for kind in kinds:
                    path = parameter_file(stem, v, kind)
                    if not os.path.isfile(path):
                        refuse('parameters', "= {}: the table of {} ({}), '{}', does not exist.".format(stem, v, kind, path))
                    shape = np.load(path, mmap_mode='r').shape
                    if len(shape) != 2 or shape[0] != self.ncell or shape[1] < 8:
                        refuse('parameters', '= {}: {} has shape {}, the run needs [{}, 8 or more] (cells; n, l1, l2, t3, t4, k, '
                               'alpha, xi).'.format(stem, path, tuple(shape), self.ncell))
                    files[(v, kind)] = path
        boot = None
        raw_b = cfg.get('bootstrap')
        try:
            nboot = 0 if raw_b in (None, '') else int(str(raw_b).strip())
        except (TypeError, ValueError):
            nboot = -1
        if nboot != 0 and not BOOTSTRAP_MIN <= nboot <= BOOTSTRAP_MAX:
            refuse('bootstrap', '= {!r} must be a whole number of replicates, {} - {} (0 or absent: no intervals).'.format(
                raw_b, BOOTSTRAP_MIN, BOOTSTRAP_MAX))
        if nboot == 0:
            for key in ('confidence', 'bootstrap_seed'):
                if cfg.get(key) not in (None, ''):
                    refuse(key, '= {!r} belongs to the bootstrap intervals, and the section asks for none (bootstrap).'.format(cfg.get(key)))
        else:
            if files is not None:
                refuse('bootstrap', '= {} and parameters exclude each other: a handed-in fit has no sample of this run to '
                       'resample.'.format(nboot))
            try:
                confidence = float(cfg.get('confidence', CONFIDENCE_DEFAULT))
            except (TypeError, ValueError):
                confidence = 0.0
            if not 0.0 < confidence < 1.0:
                refuse('confidence', '= {!r} must be a number strictly between 0 and 1.'.format(cfg.get('confidence')))
            try:
                bseed = int(str(cfg.get('bootstrap_seed', 1)).strip())
            except (TypeError, ValueError):
                bseed = -1
            if not 0 <= bseed < 2 ** 64:
                refuse('bootstrap_seed', '= {!r} must be a whole number, 0 or more (below 2^64).'.format(cfg.get('bootstrap_seed')))
            boot = {'B': nboot, 'confidence': confidence, 'seed': bseed}
        self.extremes_bootstrap = boot
        self.extremes = {'vars': evars, 'kinds': kinds, 'return_periods': periods, 'start_year': years['start_year'],
                         'end_year': years['end_year'], 'year_start_month': month, 'min_years': min_years, 'parameters': files}

    def configure_signatures(self, cfg):
        """[Signatures] (not a section of the reference; signatures/signatures.py): signature_vars = a list from q | pet | aet |
        soilmoisture | avgchflow | precip; exceedance (default 1, 5, 10, 20, 50, 80, 90, 95, 99; at most 16, different, each
        strictly between 0 and 100) = the percents of the time whose exceeded values make the duration curve; start_year /
        end_year (default: the run's; the years in which the first and the last year of the window start); year_start_month
        (1 - 12, default 1: the window starts in that month, and its last year must end inside the run).  Kept as
        ``self.signatures``."""
        from .signatures.signatures import EXCEEDANCE, MAX_COLS, MAX_EXCEEDANCE, VARS

        def refuse(key, why):
            raise ValidationException('[Signatures] {} {}'.format(key, why))

        known = ('signature_vars', 'exceedance', 'start_year', 'end_year', 'year_start_month')
        for key in cfg:
            if key not in known:
                refuse(key, 'is not a key of the section; it knows {}.'.format(', '.join(known)))
        if self.calibrate:
            refuse('and Calibrate = 1', 'exclude each other: a calibration writes no outputs to take signatures of.')
        if getattr(self, 'ensemble', None) is not None:
            refuse('and an [Ensemble] section', 'exclude each other: per-member signatures are not implemented.')
        if getattr(self, 'OutputInYear', 0) == 1:
            refuse('and OutputInYear = 1', 'exclude each other: the signatures are those of the monthly series.')
        raw = cfg.get('signature_vars')
        raw = [] if raw in (None, '') else (raw if isinstance(raw, list) else [raw])
        svars = [str(w).strip().lower() for w in raw]
        if not svars or len(set(svars)) != len(svars) or any(v not in VARS for v in svars):
            refuse('signature_vars', '= {!r} must be different names from {}.'.format(cfg.get('signature_vars'), ', '.join(VARS)))
        if 'avgchflow' in svars and self.routing_module != 'mrtm':
            refuse('signature_vars', "= avgchflow is the routed channel flow: the run needs routing_module = mrtm, not '{}'.".format(
                self.routing_module))
        for v in svars:
            if v in ('q', 'aet', 'soilmoisture', 'precip') and self.runoff_module == 'none':
                refuse('signature_vars', "= {} comes from (precip: is loaded by) the runoff module: the run needs a runoff_module, "
                       "not 'none'.".format(v))
            if v == 'pet' and self.pet_module == 'none':
                refuse('signature_vars', "= pet is the PET module's result: the run needs a pet_module, not 'none'.")
        percents = [float(p) for p in EXCEEDANCE]
        if cfg.get('exceedance') not in (None, ''):
            raw = cfg.get('exceedance')
            try:
                percents = [float(w) for w in (raw if isinstance(raw, list) else [raw])]
            except (TypeError, ValueError):
                percents = []
            if not percents or len(percents) > MAX_EXCEEDANCE or len(set(percents)) != len(percents) or not all(
                    0.0 < p < 100.0 and 0.0 < (100.0 - p) / 100.0 < 1.0 for p in percents):
                refuse('exceedance', '= {!r} must be at most {} different percents, each strictly between 0 and 100.'.format(
                    raw, MAX_EXCEEDANCE))
        try:
            month = int(cfg.get('year_start_month', 1))
        except (TypeError, ValueError):
            month = 0
        if not 1 <= month <= 12:
            refuse('year_start_month', '= {!r} must be a month, 1 - 12.'.format(cfg.get('year_start_month')))
        # the last year that starts in month `month` and ends inside the run
        last_start = self.EndYear if month == 1 else self.EndYear - 1
        years = {}
        for key, default in (('start_year', self.StartYear), ('end_year', last_start)):
            try:
                years[key] = int(cfg.get(key, default))
            except (TypeError, ValueError):
                refuse(key, '= {!r} is not a year.'.format(cfg.get(key)))
            if not self.StartYear <= years[key] <= self.EndYear:
                refuse(key, '= {} lies outside the years of the run, {} - {}.'.format(years[key], self.StartYear, self.EndYear))
        if years['end_year'] > last_start:
            refuse('end_year', '= {}: the year that starts in month {} of {} ends after the run ({}); the last complete one '
                   'starts in {}.'.format(years['end_year'], month, years['end_year'], self.EndYear, last_start))
        nyears = years['end_year'] - years['start_year'] + 1
        if nyears < 1:
            refuse('end_year', '= {} lies before start_year = {}.'.format(years['end_year'], years['start_year']))
        if 12 * nyears > MAX_COLS:
            refuse('end_year', '= {}: the window {} - {} has {} months, more than the {} one row may take.'.format(
                years['end_year'], years['start_year'], years['end_year'], 12 * nyears, MAX_COLS))
        self.signatures = {'vars': svars, 'exceedance': percents, 'start_year': years['start_year'],
                           'end_year': years['end_year'], 'year_start_month': month}

    def configure_water_balance(self, cfg):
        """[WaterBalance] (not a section of the reference; waterbalance/waterbalance.py): levels = a list from cell | basin
        (default cell); start_year / end_year (default: the run's; the years in which the first and the last year of the window
        start); year_start_month (1 - 12, default 1: the window starts in that month, and its last year must end inside the
        run); max_lag (0 - 12, default 6: the largest lag of runoff behind precipitation, in months); omega0 (> 1, default 2.6:
        Fu's parameter of the curve budyko_dev is measured from); annual = 1 | 0 (default 0: also write the annual totals).
        Kept as ``self.water_balance``."""
        from .waterbalance.waterbalance import LEVELS, MAX_COLS, MAX_LAG, OMEGA0

        def refuse(key, why):
            raise ValidationException('[WaterBalance] {} {}'.format(key, why))

        known = ('levels', 'start_year', 'end_year', 'year_start_month', 'max_lag', 'omega0', 'annual')
        for key in cfg:
            if key not in known:
                refuse(key, 'is not a key of the section; it knows {}.'.format(', '.join(known)))
        if self.calibrate:
            refuse('and Calibrate = 1', 'exclude each other: a calibration writes no outputs to take a water balance of.')
        if getattr(self, 'ensemble', None) is not None:
            refuse('and an [Ensemble] section', 'exclude each other: per-member water balances are not implemented.')
        if getattr(self, 'OutputInYear', 0) == 1:
            refuse('and OutputInYear = 1', 'exclude each other: the water balance is that of the monthly series.')
        if self.runoff_module == 'none':
            refuse('and runoff_module = none', 'exclude each other: the run needs a runoff_module, which makes the runoff and loads '
                   'the precipitation.')
        if self.pet_module == 'none':
            refuse('and pet_module = none', "exclude each other: the run needs a pet_module, which makes the PET.")
        raw = cfg.get('levels', 'cell')
        raw = [] if raw in (None, '') else (raw if isinstance(raw, list) else [raw])
        levels = [str(w).strip().lower() for w in raw]
        if not levels or len(set(levels)) != len(levels) or any(v not in LEVELS for v in levels):
            refuse('levels', '= {!r} must be different names from {}.'.format(cfg.get('levels'), ', '.join(LEVELS)))
        try:
            month = int(cfg.get('year_start_month', 1))
        except (TypeError, ValueError):
            month = 0
        if not 1 <= month <= 12:
            refuse('year_start_month', '= {!r} must be a month, 1 - 12.'.format(cfg.get('year_start_month')))
        # the last year that starts in month `month` and ends inside the run
        last_start = self.EndYear if month == 1 else self.EndYear - 1
        years = {}
        for key, default in (('start_year', self.StartYear), ('end_year', last_start)):
            try:
                years[key] = int(cfg.get(key, default))
            except (TypeError, ValueError):
                refuse(key, '= {!r} is not a year.'.format(cfg.get(key)))
            if not self.StartYear <= years[key] <= self.EndYear:
                refuse(key, '= {} lies outside the years of the run, {} - {}.'.format(years[key], self.StartYear, self.EndYear))
        if years['end_year'] > last_start:
            refuse('end_year', '= {}: the year that starts in month {} of {} ends after the run ({}); the last complete one '
                   'starts in {}.'.format(years['end_year'], month, years['end_year'], self.EndYear, last_start))
        nyears = years['end_year'] - years['start_year'] + 1
        if nyears < 2:
            refuse('end_year', '= {} with start_year = {}: the window has {} years, and the water balance needs at least 2.'.format(
                years['end_year'], years['start_year'], nyears))
        if 12 * nyears > MAX_COLS:
            refuse('end_year', '= {}: the window {} - {} has {} months, more than the {} one row may take.'.format(
                years['end_year'], years['start_year'], years['end_year'], 12 * nyears, MAX_COLS))
        try:
            max_lag = int(cfg.get('max_lag', 6))
        except (TypeError, ValueError):
            max_lag = -1
        if not 0 <= max_lag <= MAX_LAG:
            refuse('max_lag', '= {!r} must be a whole number of months, 0 - {}.'.format(cfg.get('max_lag'), MAX_LAG))
        try:
            omega0 = float(cfg.get('omega0', OMEGA0))
        except (TypeError, ValueError):
            omega0 = float('nan')
        if not (omega0 > 1.0 and omega0 != float('inf')):
            refuse('omega0', "= {!r} must be a finite number > 1 (Fu's parameter).".format(cfg.get('omega0')))
        raw_annual = str(cfg.get('annual', 0)).strip()
        if raw_annual not in ('0', '1'):
            refuse('annual', "= {!r} must be 0 or 1.".format(cfg.get('annual')))
        self.water_balance = {'levels': levels, 'start_year': years['start_year'], 'end_year': years['end_year'],
                              'year_start_month': month, 'max_lag': max_lag, 'omega0': omega0, 'annual': int(raw_annual)}

    @staticmethod
    def ck_obs_unit(set_calib, unit):
        """Units accepted for the observations (ini_reader.py:521-545)."""
        valid = ('km3_per_mth', 'mm_per_mth') if set_calib == 0 else ('m3_per_sec',)
        if unit not in valid:
            raise ValidationException("Calibration data input units '{}' not in required units '{}'".format(unit, valid))
        return unit

    def update(self, args):
        """Overwrite configuration options in memory (ini_reader.py:598-607)."""
        for k, v in args.items():
            if not hasattr(self, k):
                print('Warning: {} is not a valid parameter'.format(k))
            setattr(self, k, v)
