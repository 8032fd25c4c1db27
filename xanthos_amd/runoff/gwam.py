"""GWAM runoff -- drop-in for xanthos/runoff/gwam.py on MI355X.

Same plugin entry point as the reference (components.py:229-232), one month per call:

    runoffgen(PET, P, settings, Sm, chstor, indexing=999) -> [PET, AET, Q, Sav], each [ncell]

plus ``gwam_device`` / ``gwam_execute`` for the whole series: the spin-up pass and the simulation as the reference's
driver runs them (configurations.py:104-121, components.py:342-357), in csrc/xh_gwam.hip.

Precipitation: the reference's driver hands GWAM the precipitation column the PET step loop left in ``self.P``
(components.py:230, :334) -- column ``spinup - 1`` for every month of the spin-up pass and column ``nmonths - 1`` for
every month of the simulation.  ``precipitation='reference'`` (the default) reproduces that; ``'monthly'`` reads month
m's precipitation in month m.
"""
import numpy as np

from .. import _hip

PRECIP_MODES = ('reference', 'monthly')


def precip_columns(mode, spinup, nmonths):
    """(spin-up column, simulation column) of xh_gwam for a precipitation mode; -1 = per month."""
    if mode == 'reference':
        return (spinup - 1 if spinup > 0 else -1), nmonths - 1
    if mode == 'monthly':
        return -1, -1
    raise ValueError("precipitation must be one of {}, not '{}'".format(PRECIP_MODES, mode))


def gwam_device(ctx, ncell, nmonths, spinup, d_pet, d_precip, d_sm_max, d_sm0, precipitation='reference', indexing=999,
                out=None, d_sm_end=None):
    """Device-resident variant: d_* are DeviceArrays in HBM; fills (or allocates) out['aet'], out['q'], out['sav']."""
    if not 0 <= spinup <= nmonths:
        raise ValueError('GWAM spin-up ({}) must lie in [0, {}]'.format(spinup, nmonths))
    if out is None:
        out = {k: ctx.empty((ncell, nmonths)) for k in ('aet', 'q', 'sav')}
    cs, cm = precip_columns(precipitation, spinup, nmonths)
    ctx.gwam(ncell, nmonths, spinup, cs, cm, indexing, d_pet, d_precip, d_sm_max, d_sm0, out.get('aet'), out.get('q'),
             out.get('sav'), d_sm_end)
    return out


def gwam_execute(pet, precip, sm_max, sm0, spinup, n_months=None, precipitation='reference', indexing=999, device=0):
    """Spin-up + simulation from host arrays.  Returns (PET, AET, Q, Sav), each [ncell, n_months]."""
    ctx = _hip.get_context(device)
    pet = np.asarray(pet, dtype=np.float64)
    n_months = pet.shape[1] if n_months is None else n_months
    pet = np.ascontiguousarray(pet[:, :n_months])
    ncell = pet.shape[0]
    bufs = [ctx.upload(pet), ctx.upload(np.asarray(precip, dtype=np.float64)[:, :n_months]),
            ctx.upload(np.asarray(sm_max, dtype=np.float64).reshape(-1)),
            ctx.upload(np.asarray(sm0, dtype=np.float64).reshape(-1))]
    out = gwam_device(ctx, ncell, n_months, spinup, *bufs, precipitation=precipitation, indexing=indexing)
    host = {k: v.download() for k, v in out.items()}
    for b in bufs + list(out.values()):
        b.free()
    return pet, host['aet'], host['q'], host['sav']


def runoffgen(PET, P, settings, Sm, chstor, indexing=999, device=0):
    """One month of GWAM (gwam.py:18-88): PET, P, Sm, chstor [ncell].  Returns [PET, AET, Q, Sav]."""
    PET = np.asarray(PET, dtype=np.float64).reshape(-1)
    two = lambda a: np.repeat(np.asarray(a, dtype=np.float64).reshape(-1, 1), 2, axis=1)     # noqa: E731 (the kernel marches pairs of months)
    _, aet, q, sav = gwam_execute(two(PET), two(P), Sm, chstor, 0, 2, precipitation='monthly', indexing=indexing,
                                  device=device)
    return [PET, aet[:, 0], q[:, 0], sav[:, 0]]
