"""Public API (mirror of xanthos/model.py:21-132): ``Xanthos(ini).execute(args)`` and ``run_model(ini)``."""
import argparse
import logging
import os
import sys

from . import launch
from .configurations import ConfigRunner
from .ini_reader import ConfigReader


class Xanthos:
    """The pm_abcd_mrtm configuration of Xanthos on MI355X."""

    def __init__(self, ini):
        self.ini = ini
        self.config = None

    def stage(self, mem_args):
        self.config = ConfigReader(self.ini)
        self.config.update(mem_args)
        rank, local_rank, world = launch.env_world()
        if world > 1:                      # one process per GPU: this rank's device (XH_ONE_DEVICE=1: all on GPU 0, test boxes)
            self.config.device = 0 if os.environ.get('XH_ONE_DEVICE') == '1' else local_rank
        os.makedirs(self.config.OutputFolder, exist_ok=True)
        logger = logging.getLogger()
        logger.setLevel(logging.INFO)
        self._handlers = [logging.StreamHandler(sys.stdout)]
        if rank == 0:                      # (the log file belongs to the rank that writes the outputs)
            self._handlers.append(logging.FileHandler(os.path.join(self.config.OutputFolder, 'logfile.log')))
        for h in self._handlers:
            h.setFormatter(logging.Formatter('%(levelname)s: %(message)s'))
            logger.addHandler(h)

    def execute(self, args={}):
        """Run the configuration; ``args`` overrides settings in memory (model.py:82-98). Returns the Components."""
        self.stage(args)
        try:
            return ConfigRunner(self.config).run()
        finally:
            self.cleanup()

    def execute_ensemble(self, members=None, statistics=None, statistics_vars=None, member_outputs=None, overlap=True,
                         observed=None, obs_unit=None, gauges=None, gauge_observed=None, gauge_missing=None):
        """Run ``members`` (a list of (name, overrides) pairs or of dicts with a ``name`` key; overrides as ``execute``
        takes them, ``abcd_pars`` for a member's own parameter table; None: the [Ensemble] section's table) through one
        device-resident pass; ``observed`` / ``obs_unit``: score every member against observed basin runoff; ``gauges`` /
        ``gauge_observed`` / ``gauge_missing`` (default: the ini's [Evaluate]): score every member's routed flow at stream
        gauges; see ``ensemble.py``.  Returns the EnsembleResult."""
        from . import ensemble
        self.stage({})
        try:
            return ensemble.run(self.config, members, statistics, statistics_vars, member_outputs, overlap, observed, obs_unit,
                                gauges, gauge_observed, gauge_missing)
        finally:
            self.cleanup()

    def cleanup(self):
        logging.info('End of {0}'.format(self.config.ProjectName))
        logger = logging.getLogger()
        for h in getattr(self, '_handlers', []):
            logger.removeHandler(h)
            h.close()


def check_single_device(config):
    """Hargreaves, Hargreaves-Samani and Thornthwaite PET and GWAM run on one GPU: the basin sharding covers the pm / abcd /
    mrtm stages only."""
    from .ini_reader import ValidationException
    if config.pet_module in ('hargreaves', 'hs', 'thornthwaite') or config.runoff_module == 'gwam':
        raise ValidationException('{}: {} PET and {} runoff run on one GPU; sharding them over several GPUs is not '
                                  'implemented.'.format(config.mod_cfg, config.pet_module, config.runoff_module))


def run_ensemble(config_file, members=None, statistics=None, statistics_vars=None, member_outputs=None, overlap=True,
                 observed=None, obs_unit=None, gauges=None, gauge_observed=None, gauge_missing=None):
    """An ensemble of forcing scenarios through the configuration's grid in one device-resident pass: static data stays
    in HBM, the members stream through with their transfers and write-out overlapped, the across-member statistics are
    formed on the device.  ``members`` / ``statistics`` / ``statistics_vars`` / ``member_outputs`` default to the ini's
    [Ensemble] section; ``overlap=False`` runs the members strictly one after the other (same bits).  Member ``name`` is
    written to <OutputFolder>/<name>/, the statistics to <OutputFolder>/ensemble/.  A member may also (or only) carry
    ``abcd_pars``, its own ABCD parameter table: when no member overrides a forcing setting the run's forcing is uploaded
    once and PET is computed once, and a member costs one ABCD and one routing pass.  ``observed`` (a file or ndarray of
    rows [basin id, *, *, value]) with ``obs_unit`` ('km3_per_mth' | 'mm_per_mth') scores every member's runoff against
    it: ``result.kge`` [members, basins] and ensemble/member_kge.csv.  ``gauges`` / ``gauge_observed`` (files in the format of
    the [Evaluate] keys, which are the default; ``gauge_missing``: a sentinel) score every member's routed flow at stream
    gauges: ``result.gauge_kge`` [members, gauges], ``result.gauge_skill``, ``result.gauge_flow`` and
    ensemble/member_gauge_kge.csv, member_gauge_skill.csv.  Returns an EnsembleResult."""
    try:
        return Xanthos(config_file).execute_ensemble(members, statistics, statistics_vars, member_outputs, overlap,
                                                     observed, obs_unit, gauges, gauge_observed, gauge_missing)
    finally:
        launch.close_group()


def has_ensemble(config_file):
    from .ini_reader import parse_ini
    return isinstance(config_file, str) and isinstance(parse_ini(config_file).get('Ensemble'), dict)


def run_model(config_file, gpus=None):
    """Run Xanthos from a configuration file (model.py:111-121).

    ``gpus`` > 1 (or XH_GPUS in the environment) in a process that no launcher started: the 235 basins are sharded over that
    many GPUs of this node -- ``gpus`` rank processes are started (children of this one, before anything here touches a
    GPU), each runs this same function as one rank, rank 0 gathers and writes the outputs; returns None (the results are
    the files).  Under a launcher (RANK / WORLD_SIZE set) the call IS one rank."""
    if gpus is None and os.environ.get('XH_GPUS'):
        gpus = int(os.environ['XH_GPUS'])
    if has_ensemble(config_file):          # an ini with an [Ensemble] section runs the ensemble driver (one GPU)
        from . import ensemble
        if gpus and int(gpus) > 1:
            ensemble.validate(ConfigReader(config_file), [], gpus=gpus)      # refuses: members over several GPUs
        return run_ensemble(config_file)
    if gpus and int(gpus) > 1 and 'RANK' not in os.environ and 'WORLD_SIZE' not in os.environ:
        check_single_device(ConfigReader(config_file))
        env = dict(os.environ)             # the rank processes import this very package, wherever the caller found it
        pkg_parent = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env['PYTHONPATH'] = pkg_parent + (os.pathsep + env['PYTHONPATH'] if env.get('PYTHONPATH') else '')
        rc = launch.spawn(int(gpus), ['-m', 'xanthos_amd.model', os.path.abspath(config_file)], env=env,
                          one_device=os.environ.get('XH_ONE_DEVICE') == '1')
        if rc != 0:
            raise RuntimeError('run_model on {} GPUs: a rank exited with code {}'.format(gpus, rc))
        return None
    try:
        return Xanthos(config_file).execute()
    finally:
        launch.close_group()


if __name__ == '__main__':
    parser = argparse.ArgumentParser()
    parser.add_argument('config_file', type=str, help='Full path with file name to INI configuration file.')
    parser.add_argument('--gpus', type=int, default=None, help='GPUs of this node to shard the basins over (one process each)')
    a = parser.parse_args()
    run_model(a.config_file, gpus=a.gpus)
