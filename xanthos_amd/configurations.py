"""ConfigRunner (mirror of xanthos/configurations.py:17-141): validates the selectors and runs the components."""
import logging

from .components import Components


class ConfigRunner:
    PET_COMPONENTS = ['pm', 'hargreaves', 'hs', 'thornthwaite']   # (:61)
    RUNOFF_COMPONENTS = ['abcd', 'gwam']    # (:62)
    ROUTING_COMPONENTS = ['mrtm']           # (:63)

    def __init__(self, config):
        self.run_pet = config.pet_module in self.PET_COMPONENTS
        self.run_runoff = config.runoff_module in self.RUNOFF_COMPONENTS
        self.run_routing = config.routing_module in self.ROUTING_COMPONENTS
        # every stage iterates internally: all *_timestep are 0 and no whole-model spin-up (:69-85).  The reference runs
        # Hargreaves and GWAM month by month and GWAM's spin-up as a pass of the whole model (:104-113); here one
        # xh_gwam call does the spin-up pass and the simulation (components.Components.simulation)
        self.pet_timestep = self.runoff_timestep = self.routing_timestep = 0
        self.spinup = False
        self.config = config

    def run(self):
        if not (self.run_pet or self.run_runoff or self.run_routing):
            logging.warning('Selected configuration {0} not supported.'.format(self.config.mod_cfg))
            return None
        import time
        c = Components(self.config)
        c.simulation(run_pet=self.run_pet, run_runoff=self.run_runoff, run_routing=self.run_routing,
                     pet_num_steps=0, runoff_num_steps=0, routing_num_steps=0, notify='Simulation')
        t = time.time()
        c.accessible_water()          # post-processors, the outputs, the plots: the reference's order (configurations.py:117-139)
        c.drought()
        c.drought_index()             # ([DroughtIndex], not in the reference: standardized drought indices)
        c.trend()                     # ([Trend], not in the reference: Mann-Kendall test and Theil-Sen slope per cell)
        c.extremes()                  # ([Extremes], not in the reference: GEV by L-moments, return levels and periods per cell)
        c.signatures()                # ([Signatures], not in the reference: flow duration curve and regime signatures per cell)
        c.water_balance()             # ([WaterBalance], not in the reference: water balance and Budyko signatures per cell and basin)
        c.hydropower_potential()
        c.hydropower_actual()
        c.evaluate()                  # ([Evaluate], not in the reference: the routed flow scored at stream gauges)
        c.diagnostics()
        c.timings['post'] = time.time() - t
        t = time.time()
        c.output_simulation()
        c.timings['write'] = time.time() - t
        if self.config.CreateTimeSeriesPlot:
            t = time.time()
            c.plots()
            c.timings['plots'] = time.time() - t
        logging.info('run_model phases (s): ' + ', '.join('{} {:.3f}'.format(k, v) for k, v in c.timings.items()))
        return c
