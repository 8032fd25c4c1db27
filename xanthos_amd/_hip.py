"""ctypes binding of libxanthos_hip.so (include/xanthos_hip.h).

This is the only place the shared library is loaded.  There is NO CPU fallback: if the library is missing, or no
MI355X is visible, the calls raise :class:`HipUnavailable` -- the product path never routes through numpy.
"""
import contextlib
import ctypes
import os
import threading
from ctypes import POINTER, Structure, byref, c_char_p, c_double, c_int, c_int8, c_int32, c_int64, c_size_t, \
    c_uint64, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# XH_LIBRARY: another build of the library (A/B experiments: `make -C xanthos_amd/csrc exp EXPNAME=... EXPFLAGS=...`)
LIB_PATH = os.environ.get('XH_LIBRARY') or os.path.join(_HERE, 'libxanthos_hip.so')

XH_ROUTE_DEFAULT, XH_ROUTE_FORCE_FALLBACK, XH_ROUTE_ATOMIC, XH_ROUTE_NO_DATAFLOW, XH_ROUTE_NO_SKEW = 0, 1, 2, 4, 8
XH_ROUTE_TEST_FAULT, XH_ROUTE_VALIDATE = 16, 32
XH_ROUTE_REASSOC, XH_ROUTE_EXACT = 128, 256      # reassociated (tolerance) form of the routing kernel / the bit-exact kernels
XH_ROUTE_NO_PLAIN = 0x4000                       # (xh_common.h, what a guard trip re-routes with) pairs of sums in every unit: not the prepared plan
XH_DAYLIGHT_REFERENCE, XH_DAYLIGHT_MONTHLY = 0, 1  # Thornthwaite's daylight order: the reference's repeat / every month its own
XH_ERR_ARG, XH_ERR_HIP, XH_ERR_LIMIT, XH_ERR_DEVICE = 1, 2, 3, 4
XH_SRC_F32_LE, XH_SRC_F32_BE, XH_SRC_F64_BE = 1, 2, 3          # xh_widen's kinds: how the source values are stored
# dtype of a forcing array that may cross PCIe as stored -> (xh_widen kind, label of DevicePipeline.forcing_upload)
NARROW_KINDS = {np.dtype('<f4'): (XH_SRC_F32_LE, 'f32'), np.dtype('>f4'): (XH_SRC_F32_BE, 'f32be'),
                np.dtype('>f8'): (XH_SRC_F64_BE, 'f64be')}
STD_INDEX_DIST = {'gamma': 0, 'empirical': 1}                        # XH_STD_INDEX_* of xh_std_index
STD_INDEX_DIST2 = dict(STD_INDEX_DIST, loglogistic=2)                # ... and of xh_std_index2
EXTREMES_KIND = {'max': 0, 'min': 1}                                 # xh_extremes' kind
ENS_STAT_BITS = {'mean': 1, 'std': 2, 'min': 4, 'max': 8}       # XH_ENS_* of xh_ens_stats, in its output order


class HipUnavailable(RuntimeError):
    """The HIP library or device is not usable; nothing falls back to the CPU."""


class HipError(RuntimeError):
    """A libxanthos_hip call returned an error code."""


class PmTables(Structure):
    _fields_ = [('nlcs', c_int32)] + [(n, POINTER(c_double)) for n in (
        'cL', 'beta', 'rslimit', 'Tminopen', 'Tminclose', 'VPDclose', 'VPDopen', 'RBLmin', 'RBLmax', 'rc', 'emiss',
        'alpha', 'lai', 'laimin', 'laimax')]


class FusedArgs(Structure):
    """xh_fused_args (include/xanthos_hip.h)."""
    _fields_ = ([('ncell', c_int64), ('nmonths', c_int32), ('start_year', c_int32), ('pm', POINTER(PmTables)),
                 ('n_lc_years', c_int32), ('h_lc_years', c_void_p), ('water_idx', c_int32), ('snow_idx', c_int32)] +
                [(n, c_void_p) for n in ('d_tas', 'd_tmin', 'd_rhs', 'd_wind', 'd_rsds', 'd_rlds', 'd_tairprev', 'd_lct',
                                         'd_elev')] +
                [('abcd_spinup', c_int32), ('n_groups', c_int32), ('h_basin_index', c_void_p), ('h_par_index', c_void_p),
                 ('npar_rows', c_int64), ('d_pars', c_void_p), ('d_precip', c_void_p), ('d_abcd_tmin', c_void_p),
                 ('plan', c_void_p), ('routing_spinup', c_int32), ('h_ndays', c_void_p), ('dt', c_double),
                 ('d_flow_dist', c_void_p), ('d_velocity', c_void_p), ('d_area', c_void_p), ('d_S0', c_void_p),
                 ('route_flags', c_int32)] +
                [(n, c_void_p) for n in ('d_pet', 'd_aet', 'd_q', 'd_sav', 'd_chstorage', 'd_avgchflow')] +
                [('block_months', c_int32), ('mode', c_int32)])


class CalibFlowDesc(Structure):
    """xh_calib_flow_desc (include/xanthos_hip.h): closure tables of the streamflow objective."""
    _fields_ = [('routing_spinup', c_int32), ('dt', c_double)] + [(n, c_void_p) for n in (
        'h_ndays', 'h_closure_ptr', 'h_row_ptr', 'h_cols', 'h_sign', 'h_basin_col', 'h_outlet_rank', 'h_tauinv', 'h_area',
        'h_s0')]


def flow_desc(tables):
    """CalibFlowDesc over the arrays of ``tables`` (calibrate.flow_tables.FlowTables); keep ``tables`` alive."""
    t = tables
    return CalibFlowDesc(int(t.routing_spinup), float(t.dt), *[_host_ptr(a) for a in (
        t.ndays, t.closure_ptr, t.row_ptr, t.cols, t.sign, t.basin_col, t.outlet_rank, t.tauinv, t.area, t.s0)])


class CalibGaugeDesc(Structure):
    """xh_calib_gauge_desc (include/xanthos_hip.h): union-closure tables and gauges of the gauge form."""
    _fields_ = [('routing_spinup', c_int32), ('dt', c_double)] + [(n, c_void_p) for n in (
        'h_ndays', 'h_closure_ptr', 'h_row_ptr', 'h_cols', 'h_sign', 'h_basin_col', 'h_tauinv', 'h_area', 'h_s0',
        'h_gauge_ptr', 'h_gauge_row', 'h_gauge_weight')]


def gauge_desc(tables):
    """CalibGaugeDesc over the arrays of ``tables`` (calibrate.gauge_tables.GaugeTables); keep ``tables`` alive."""
    t = tables
    return CalibGaugeDesc(int(t.routing_spinup), float(t.dt), *[_host_ptr(a) for a in (
        t.ndays, t.closure_ptr, t.row_ptr, t.cols, t.sign, t.basin_col, t.tauinv, t.area, t.s0, t.gauge_ptr, t.gauge_row,
        t.gauge_weight)])


class CalibVelocityDesc(Structure):
    """xh_calib_velocity_desc (include/xanthos_hip.h): ChV and L of every closure row, for the velocity forms."""
    _fields_ = [('h_velocity', c_void_p), ('h_length', c_void_p)]


def velocity_desc(tables):
    """CalibVelocityDesc over ``tables.velocity`` and ``tables.length`` (FlowTables or GaugeTables); keep ``tables`` alive."""
    return CalibVelocityDesc(_host_ptr(tables.velocity), _host_ptr(tables.length))


_P = c_void_p
# name -> (restype, argtypes); mirrors include/xanthos_hip.h one to one
SIGNATURES = {
    'xh_abi_version': (c_int, []),
    'xh_device_count': (c_int, [POINTER(c_int)]),
    'xh_ctx_create': (c_int, [c_int, POINTER(c_void_p)]),
    'xh_ctx_destroy': (None, [_P]),
    'xh_last_error': (c_char_p, [_P]),
    'xh_device_name': (c_int, [_P, ctypes.c_char_p, c_size_t]),
    'xh_malloc': (c_int, [_P, c_size_t, POINTER(c_void_p)]),
    'xh_free': (c_int, [_P, _P]),
    'xh_mem_info': (c_int, [_P, POINTER(c_size_t), POINTER(c_size_t)]),
    'xh_memcpy_h2d': (c_int, [_P, _P, _P, c_size_t]),
    'xh_memcpy_d2h': (c_int, [_P, _P, _P, c_size_t]),
    'xh_memcpy_d2d': (c_int, [_P, _P, _P, c_size_t]),
    'xh_host_alloc': (c_int, [_P, c_size_t, POINTER(c_void_p)]),
    'xh_host_free': (c_int, [_P, _P]),
    'xh_memcpy_h2d_async': (c_int, [_P, _P, _P, c_size_t]),
    'xh_memcpy_d2h_async': (c_int, [_P, _P, _P, c_size_t]),
    'xh_upload_file': (c_int, [_P, _P, c_char_p, ctypes.c_uint64, c_size_t, c_int]),
    'xh_download_file': (c_int, [_P, _P, c_char_p, ctypes.c_uint64, c_size_t, c_int]),
    'xh_download_files': (c_int, [_P, c_int, POINTER(c_void_p), POINTER(c_char_p), POINTER(ctypes.c_uint64), POINTER(c_size_t)]),
    'xh_csv_format': (c_int, [_P, _P, c_int64, c_int64, c_int64, _P, c_size_t, _P]),
    'xh_csv_write': (c_int, [_P, _P, c_int64, c_int64, c_int64, c_char_p, ctypes.c_uint64, c_size_t, POINTER(ctypes.c_uint64)]),
    'xh_csv_write_many': (c_int, [_P, c_int, POINTER(c_void_p), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64),
                                  POINTER(c_char_p), POINTER(ctypes.c_uint64), c_size_t, POINTER(ctypes.c_uint64)]),
    'xh_pack_f32_be': (c_int, [_P, _P, c_int64, _P]),
    'xh_grid_pack_f32_be': (c_int, [_P, _P, c_int64, c_int64, _P, c_int64, ctypes.c_uint32, _P]),
    'xh_widen': (c_int, [_P, _P, c_int, c_int64, _P]),
    'xh_memset': (c_int, [_P, _P, c_int, c_size_t]),
    'xh_sync': (c_int, [_P]),
    'xh_gather_rows': (c_int, [_P, _P, _P, c_int64, c_int64, _P]),
    'xh_scatter_rows': (c_int, [_P, _P, _P, c_int64, c_int64, _P]),
    'xh_transpose': (c_int, [_P, _P, c_int64, c_int64, _P]),
    'xh_timing_reset': (c_int, [_P]),
    'xh_timing_enable': (c_int, [_P, c_int]),
    'xh_timing_get': (c_int, [_P, c_char_p, POINTER(c_double), POINTER(c_int64)]),
    'xh_pm_pet': (c_int, [_P, POINTER(PmTables), c_int64, c_int32, c_int32, c_int32, _P, c_int32, c_int32,
                          _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'xh_abcd': (c_int, [_P, c_int64, c_int32, c_int32, c_int32, _P, _P, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'xh_hargreaves_pet': (c_int, [_P, c_int64, c_int32, _P, _P, _P, _P, _P, _P, _P]),
    'xh_gwam': (c_int, [_P, c_int64, c_int32, c_int32, c_int32, c_int32, c_double, _P, _P, _P, _P, _P, _P, _P, _P]),
    'xh_hs_pet': (c_int, [_P, c_int64, c_int32, _P, _P, _P, _P, _P, _P]),
    'xh_thornthwaite_pet': (c_int, [_P, c_int64, c_int32, c_int32, c_int32, _P, _P, _P, _P]),
    'xh_route_plan_create': (c_int, [_P, c_int64, _P, _P, _P, POINTER(c_void_p)]),
    'xh_route_plan_destroy': (None, [_P]),
    'xh_route_plan_info': (c_int, [_P, POINTER(c_int64)]),
    'xh_route_plan_stats': (c_int, [_P, c_int64, _P, POINTER(c_int64)]),
    'xh_route_plan_rsum_info': (c_int, [_P, POINTER(c_int64)]),
    'xh_route_plan_linear_units': (c_int64, [_P]),
    'xh_route_plan_prepare': (c_int, [_P, _P, _P, _P, c_double]),
    'xh_mrtm_downstream': (c_int, [c_int64, c_int32, c_int32, _P, _P, _P, _P, _P]),
    'xh_mrtm_upstream': (c_int, [c_int64, c_int32, c_int32, _P, _P, _P, _P, _P]),
    'xh_mrtm_um_csr': (c_int, [c_int64, _P, _P, _P, _P]),
    'xh_route_series': (c_int, [_P, _P, c_int32, c_int32, _P, c_double, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int32]),
    'xh_run_fused': (c_int, [_P, POINTER(FusedArgs)]),
    'xh_calib_objective': (c_int, [_P, c_int64, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    'xh_calib_objective_multi': (c_int, [_P, c_int32, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    'xh_calib_de_create': (c_int, [_P, c_int32, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P,
                                   c_uint64, POINTER(c_void_p)]),
    'xh_calib_flow_objective_multi': (c_int, [_P, c_int32, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P,
                                              POINTER(CalibFlowDesc), _P, _P, _P]),
    'xh_calib_de_create_flow': (c_int, [_P, c_int32, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P,
                                        POINTER(CalibFlowDesc), _P, _P, _P, c_uint64, POINTER(c_void_p)]),
    'xh_calib_gauge_objective_multi': (c_int, [_P, c_int32, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P,
                                               POINTER(CalibGaugeDesc), _P, _P, _P, _P]),
    'xh_calib_de_create_gauge': (c_int, [_P, c_int32, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P,
                                         POINTER(CalibGaugeDesc), _P, _P, _P, c_uint64, POINTER(c_void_p)]),
    'xh_calib_flow_velocity_objective_multi': (c_int, [_P, c_int32, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P,
                                                       POINTER(CalibFlowDesc), POINTER(CalibVelocityDesc), _P, _P, _P]),
    'xh_calib_gauge_velocity_objective_multi': (c_int, [_P, c_int32, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P,
                                                        POINTER(CalibGaugeDesc), POINTER(CalibVelocityDesc), _P, _P, _P,
                                                        _P]),
    'xh_calib_de_create_flow_velocity': (c_int, [_P, c_int32, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P,
                                                 POINTER(CalibFlowDesc), POINTER(CalibVelocityDesc), _P, _P, _P, c_uint64,
                                                 POINTER(c_void_p)]),
    'xh_calib_de_create_gauge_velocity': (c_int, [_P, c_int32, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P,
                                                  POINTER(CalibGaugeDesc), POINTER(CalibVelocityDesc), _P, _P, _P, c_uint64,
                                                  POINTER(c_void_p)]),
    'xh_calib_de_destroy': (None, [_P]),
    'xh_calib_de_init': (c_int, [_P]),
    'xh_calib_de_step': (c_int, [_P, c_int32, c_double, c_double, c_double, c_double, c_double, POINTER(c_int32)]),
    'xh_calib_de_result': (c_int, [_P, _P, _P, _P, _P, _P]),
    'xh_calib_de_state': (c_int, [_P, c_int32, _P, _P]),
    'xh_calib_de_set_state': (c_int, [_P, _P, _P, c_int32]),
    'xh_comm_unique_id': (c_int, [ctypes.c_char_p, c_size_t]),
    'xh_comm_create': (c_int, [_P, c_int32, c_int32, ctypes.c_char_p, c_size_t, POINTER(c_void_p)]),
    'xh_comm_destroy': (None, [_P]),
    'xh_comm_info': (c_int, [_P, POINTER(c_int64)]),
    'xh_comm_gather_rows': (c_int, [_P, _P, c_int32, c_int32, _P, c_int64, _P, _P, _P]),
    'xh_comm_gather_rows_side': (c_int, [_P, _P, c_int32, c_int32, _P, c_int64, _P, _P, _P]),
    'xh_comm_join': (c_int, [_P]),
    'xh_mark_begin': (c_int, [_P, c_char_p]),
    'xh_mark_end': (c_int, [_P]),
    'xh_agg_time': (c_int, [_P, c_int64, c_int32, c_int32, c_int32, _P, _P, _P]),
    'xh_agg_spatial': (c_int, [_P, c_int64, c_int32, c_int32, _P, _P, _P]),
    'xh_nan_to_num': (c_int, [_P, _P, c_int64]),
    'xh_drought_thresholds': (c_int, [_P, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_double, _P, _P]),
    'xh_drought_stats': (c_int, [_P, c_int64, c_int32, c_int32, _P, _P, _P, _P, _P]),
    'xh_hpot_qmax': (c_int, [_P, c_int64, c_int32, c_int32, c_int32, c_double, _P, _P]),
    'xh_hpot_energy': (c_int, [_P, c_int64, c_int32, c_int32, _P, c_double, c_double, c_double, c_double, _P, _P, _P, _P]),
    'xh_hpot_region': (c_int, [_P, c_int32, c_int32, _P, _P, _P, _P]),
    'xh_hact_inflow': (c_int, [_P, c_int64, c_int32, c_int32, c_int32, _P, _P, _P, c_double, _P, _P, _P, _P]),
    'xh_hact_sim': (c_int, [_P, c_int32, c_int32, c_int32, c_int32, _P, c_double, c_double, _P, _P, _P, _P, _P, _P, _P]),
    'xh_diag_cell_total': (c_int, [_P, c_int64, c_int32, _P, c_double, _P, c_double, _P, c_int64]),
    'xh_diag_group_sum': (c_int, [_P, c_int64, c_int32, c_int32, _P, _P, _P, _P]),
    'xh_ens_stats': (c_int, [_P, c_int64, c_int32, POINTER(c_void_p), ctypes.c_uint32, c_int32, _P, POINTER(c_void_p)]),
    'xh_basin_kge': (c_int, [_P, c_int64, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P]),
    'xh_gauge_skill': (c_int, [_P, c_int64, c_int32, c_int32, _P, _P, _P, _P, _P]),
    'xh_std_index': (c_int, [_P, c_int64, c_int32, c_int32, POINTER(c_int32), c_int32, c_int32, c_int32, c_double, _P,
                            POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p)]),
    'xh_std_index2': (c_int, [_P, c_int64, c_int32, c_int32, POINTER(c_int32), c_int32, c_int32, c_int32, c_double, _P, _P,
                             POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p)]),
    'xh_trend': (c_int, [_P, c_int64, c_int32, c_int32, c_int32, c_int32, c_double, _P, _P]),
    'xh_extremes': (c_int, [_P, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P]),
    'xh_extremes_boot': (c_int, [_P, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, c_int32, c_double, c_uint64,
                                 c_int64, _P, _P, _P]),
    'xh_signatures': (c_int, [_P, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P]),
    'xh_water_balance': (c_int, [_P, c_int64, c_int32, c_int32, c_int32, c_int32, c_double, _P, _P, _P, _P, _P, _P, _P]),
    'xh_synth_forcing': (c_int, [_P, c_uint64, c_double, c_int64, c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
}

_lib = None


# Exports added without a change of any existing signature: a library from before them still loads (the parent's build beside
# this package through XH_LIBRARY, for an A/B), and the caller sees None
OPTIONAL_SYMBOLS = frozenset(['xh_route_plan_linear_units'])
ABI_VERSION = 7        # xh_abi_version() of the library these signatures describe


def lib():
    """Load libxanthos_hip.so (once) and declare every signature. Raises HipUnavailable if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise HipUnavailable(
                '{} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` or '
                '`make -C xanthos_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback.'.format(LIB_PATH))
        try:
            handle = ctypes.CDLL(LIB_PATH)
        except OSError as exc:
            raise HipUnavailable('cannot load {}: {}'.format(LIB_PATH, exc))
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError:          # a library built from older sources than these signatures
                if name in OPTIONAL_SYMBOLS:
                    continue
                raise HipUnavailable('{} lacks {}: it was built from older sources; rebuild it (make -C xanthos_amd/csrc)'
                                     .format(LIB_PATH, name))
            fn.restype = res
            fn.argtypes = args
        if handle.xh_abi_version() != ABI_VERSION:
            raise HipUnavailable('{} has ABI version {}, this package binds version {}: rebuild it (make -C xanthos_amd/csrc)'
                                 .format(LIB_PATH, handle.xh_abi_version(), ABI_VERSION))
        _lib = handle
    return _lib


def _host_ptr(arr):
    return arr.ctypes.data_as(c_void_p)


def as_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class DeviceArray:
    """A float64 (or raw) buffer in HBM owned by a Context."""

    def __init__(self, ctx, shape, dtype=np.float64):
        self.ctx = ctx
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = c_void_p()
        ctx._check(lib().xh_malloc(ctx.handle, self.nbytes, byref(p)))
        self.ptr = p.value
        ctx._live.add(self)

    @property
    def size(self):
        return int(np.prod(self.shape, dtype=np.int64))

    def upload(self, host):
        host = np.ascontiguousarray(host, dtype=self.dtype)
        if host.nbytes != self.nbytes:
            raise ValueError('size mismatch: host {} vs device {}'.format(host.shape, self.shape))
        self.ctx._check(lib().xh_memcpy_h2d(self.ctx.handle, self.ptr, _host_ptr(host), self.nbytes))
        return self

    def download(self, out=None):
        if out is None:
            out = np.empty(self.shape, dtype=self.dtype)
        if out.nbytes != self.nbytes or not out.flags.c_contiguous:
            raise ValueError('bad output buffer')
        self.ctx._check(lib().xh_memcpy_d2h(self.ctx.handle, _host_ptr(out), self.ptr, self.nbytes))
        return out

    def zero(self):
        self.ctx._check(lib().xh_memset(self.ctx.handle, self.ptr, 0, self.nbytes))
        return self

    def free(self):
        if self.ptr is not None and self.ctx.handle is not None:
            lib().xh_free(self.ctx.handle, self.ptr)
            self.ctx._live.discard(self)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _dptr(x):
    """Device pointer of a DeviceArray / raw int / None."""
    if x is None:
        return None
    if isinstance(x, DeviceArray):
        return x.ptr
    return int(x)


class Context:
    """One HIP device + stream (xh_ctx). Not thread-safe; use one per host thread."""

    def __init__(self, device=0):
        L = lib()
        h = c_void_p()
        rc = L.xh_ctx_create(int(device), byref(h))
        if rc != 0:
            msg = L.xh_last_error(None)
            raise HipUnavailable('xh_ctx_create(device={}) failed: {}. There is no CPU fallback.'.format(
                device, msg.decode() if msg else rc))
        self.handle = h.value
        self.device = int(device)
        self._live = set()
        self._pinned = {}

    # ---- plumbing
    def _check(self, rc):
        if rc != 0:
            msg = lib().xh_last_error(self.handle)
            raise HipError('libxanthos_hip error {}: {}'.format(rc, msg.decode() if msg else ''))

    def name(self):
        buf = ctypes.create_string_buffer(256)
        self._check(lib().xh_device_name(self.handle, buf, 256))
        return buf.value.decode()

    def cu_count(self):
        """Compute units of the device (xh_device_name ends in "(<arch>, <n> CUs)")."""
        import re
        m = re.search(r'(\d+) CUs\)', self.name())
        return int(m.group(1)) if m else 256

    def close(self):
        if self.handle is not None:
            for a in list(self._live):
                a.free()
            for p in list(self._pinned.values()):
                lib().xh_host_free(self.handle, p)
            self._pinned = {}
            lib().xh_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._check(lib().xh_sync(self.handle))

    def mem_info(self):
        """(free, total) bytes of the device's memory right now (xh_mem_info)."""
        free, total = c_size_t(), c_size_t()
        self._check(lib().xh_mem_info(self.handle, byref(free), byref(total)))
        return free.value, total.value

    def d2d(self, dst, src):
        """Enqueue device -> device on this context's stream (xh_memcpy_d2d); ``dst`` and ``src`` of one size."""
        if dst.nbytes != src.nbytes:
            raise ValueError('size mismatch: {} vs {}'.format(dst.shape, src.shape))
        self._check(lib().xh_memcpy_d2d(self.handle, _dptr(dst), _dptr(src), dst.nbytes))
        return dst

    def empty(self, shape, dtype=np.float64):
        return DeviceArray(self, shape, dtype)

    def upload(self, host, dtype=np.float64):
        host = np.ascontiguousarray(host, dtype=dtype)
        return DeviceArray(self, host.shape, dtype).upload(host)

    def pinned(self, shape, dtype=np.float64):
        """A numpy array in page-locked host memory (xh_host_alloc); release it with free_pinned()."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        p = c_void_p()
        self._check(lib().xh_host_alloc(self.handle, nbytes, byref(p)))
        buf = (ctypes.c_char * max(nbytes, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape, dtype=np.int64))).reshape(shape)
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def free_pinned(self, arr):
        p = self._pinned.pop(arr.ctypes.data, None)
        if p is not None and self.handle is not None:
            self._check(lib().xh_host_free(self.handle, p))

    def h2d_async(self, dst, host):
        """Enqueue host -> device without waiting; ``host`` must stay alive and unchanged until sync()."""
        self._check(lib().xh_memcpy_h2d_async(self.handle, _dptr(dst), _host_ptr(host), host.nbytes))

    def d2h_async(self, host, src):
        self._check(lib().xh_memcpy_d2h_async(self.handle, _host_ptr(host), _dptr(src), host.nbytes))

    def upload_file(self, dst, path, offset, nbytes, threads=0):
        """``nbytes`` of file ``path`` from byte ``offset`` -> DeviceArray ``dst`` (xh_upload_file: the range is mapped
        read-only and copied out of the mapping; no host copy of the data)."""
        if nbytes != dst.nbytes:
            raise ValueError('size mismatch: file range {} vs device {}'.format(nbytes, dst.nbytes))
        self._check(lib().xh_upload_file(self.handle, _dptr(dst), os.fsencode(path), int(offset), int(nbytes), threads))
        return dst

    def download_file(self, src, path, offset, threads=0):
        """DeviceArray ``src`` -> bytes ``offset ...`` of file ``path`` (xh_download_file)."""
        self._check(lib().xh_download_file(self.handle, _dptr(src), os.fsencode(path), int(offset), src.nbytes, threads))

    def save_npy(self, path, src):
        """np.save(path, src.download()) without the host array: header here, body by xh_download_file."""
        self.save_npy_many([(path, src)])

    def save_npy_many(self, items):
        """[(path, DeviceArray), ...] -> .npy files, the bodies written side by side (xh_download_files, <= 16 per call)."""
        items = list(items)
        for k in range(0, len(items), 16):
            part = items[k:k + 16]
            offsets = []
            for path, src in part:
                with open(path, 'wb') as fh:
                    np.lib.format.write_array_header_1_0(fh, {'descr': np.lib.format.dtype_to_descr(np.dtype(src.dtype)),
                                                              'fortran_order': False, 'shape': tuple(src.shape)})
                    offsets.append(fh.tell())
            n = len(part)
            srcs = (c_void_p * n)(*[_dptr(src) for _, src in part])
            paths = (c_char_p * n)(*[os.fsencode(path) for path, _ in part])
            offs = (ctypes.c_uint64 * n)(*offsets)
            sizes = (c_size_t * n)(*[src.nbytes for _, src in part])
            self._check(lib().xh_download_files(self.handle, n, srcs, paths, offs, sizes))

    def pack_f32_be(self, src, n, dst):
        """``n`` doubles at ``src`` -> ``n`` big-endian binary32 values at ``dst`` (xh_pack_f32_be: numpy's
        astype('>f4')), enqueued.  ``src`` / ``dst``: DeviceArrays or raw device addresses (a row slice); the source
        8-byte, the destination 16-byte aligned."""
        self._check(lib().xh_pack_f32_be(self.handle, _dptr(src), int(n), _dptr(dst)))

    def widen(self, src, kind, n, dst):
        """``n`` stored values at ``src`` (``kind``: XH_SRC_F32_LE / XH_SRC_F32_BE / XH_SRC_F64_BE) -> ``n`` native doubles
        at ``dst`` (xh_widen: numpy's astype(np.float64)), enqueued.  ``src`` / ``dst``: DeviceArrays or raw device addresses
        (a row slice); the source aligned to its element, the destination to 8 bytes; only XH_SRC_F64_BE may run in place."""
        self._check(lib().xh_widen(self.handle, _dptr(src), int(kind), int(n), _dptr(dst)))

    def _save_bodies(self, items, nbytes_of, form):
        """[(path, header bytes, DeviceArray [nrows, ncols], ...), ...] -> files of header + body, <= 16 at a time: the
        headers are written here, ``form(src, scratch, ...)`` enqueues the body of ``nbytes_of(src, ...)`` bytes into a
        scratch DeviceArray (``...``: what an item holds behind its array, e.g. the grid map of save_grid_nc_many), and the
        bodies leave side by side behind their headers (xh_download_files).  The scratch is freed after the flush."""
        items = list(items)
        for k in range(0, len(items), 16):
            part, bodies = items[k:k + 16], []
            try:
                for path, header, src, *more in part:
                    if src.dtype != np.float64 or len(src.shape) != 2:
                        raise ValueError('{}: a [nrows, ncols] float64 DeviceArray is expected'.format(path))
                    with open(path, 'wb') as fh:
                        fh.write(header)
                    bodies.append(self.empty((max(nbytes_of(src, *more), 1),), dtype=np.uint8))
                    if src.size:
                        form(src, bodies[-1], *more)
                n = len(part)
                srcs = (c_void_p * n)(*[_dptr(b) for b in bodies])
                paths = (c_char_p * n)(*[os.fsencode(item[0]) for item in part])
                offs = (ctypes.c_uint64 * n)(*[len(item[1]) for item in part])
                sizes = (c_size_t * n)(*[nbytes_of(*item[2:]) for item in part])
                self._check(lib().xh_download_files(self.handle, n, srcs, paths, offs, sizes))
            finally:
                for b in bodies:
                    b.free()

    def save_nc_many(self, items):
        """[(path, header, DeviceArray), ...] -> NetCDF-classic files: ``header`` is data_writer.formats.nc_header(...) of
        the array's shape, the body its values as big-endian binary32, row-major, packed in HBM (xh_pack_f32_be)."""
        self._save_bodies(items, lambda src: src.size * 4, lambda src, body: self.pack_f32_be(src, src.size, body))

    def save_mat_many(self, items):
        """[(path, header, DeviceArray), ...] -> MAT-5 files: ``header`` is data_writer.formats.mat_header(...) of the
        array's name and shape, the body its doubles column-major (xh_transpose in HBM)."""
        self._save_bodies(items, lambda src: src.nbytes,
                          lambda src, body: self.transpose(src, src.shape[0], src.shape[1], body))

    def grid_pack_f32_be(self, src, cell_of_slot, nslots, fill_bits, dst):
        """DeviceArray ``src`` [ncell, ncols] -> ``dst`` [ncols, nslots] big-endian binary32 (xh_grid_pack_f32_be), enqueued:
        slot s takes the row of cell ``cell_of_slot[s]`` (int32 in HBM, 0-based), narrowed as by pack_f32_be; a slot
        without a cell (-1) and every NaN take ``fill_bits``.  ``dst`` 16-byte aligned."""
        ncell, ncols = src.shape
        self._check(lib().xh_grid_pack_f32_be(self.handle, _dptr(src), ncell, ncols, _dptr(cell_of_slot), int(nslots),
                                              int(fill_bits), _dptr(dst)))

    def save_grid_nc_many(self, items):
        """[(path, header, DeviceArray [ncell, ncols], grid map), ...] -> gridded NetCDF-classic files: ``header`` is
        data_writer.gridded.grid_nc_header(...), the body [ncols, nslots] big-endian binary32 with the map's fill value
        where no cell lies, gathered and packed in HBM (xh_grid_pack_f32_be)."""
        self._save_bodies(items, lambda src, grid: src.shape[1] * grid.nslots * 4,
                          lambda src, body, grid: self.grid_pack_f32_be(src, grid.device_table(self), grid.nslots,
                                                                        grid.fill_bits, body))

    def csv_format(self, src, first_id=1, cap=None):
        """The csv lines of DeviceArray ``src`` [nrows, ncols] formatted in HBM (xh_csv_format), downloaded for inspection:
        (text as bytes, int64 offsets [nrows + 1] of the lines).  ``cap``: bytes of the text buffer (default: the most
        the shape can take)."""
        nrows, ncols = src.shape
        if cap is None:
            cap = nrows * (ncols * 25 + 21)
        text, offs = self.empty((max(int(cap), 1),), dtype=np.uint8), self.empty((nrows + 1,), dtype=np.int64)
        try:
            self._check(lib().xh_csv_format(self.handle, _dptr(src), nrows, ncols, int(first_id), _dptr(text), int(cap),
                                            _dptr(offs)))
            offsets = offs.download()
            return text.download()[:int(offsets[-1])].tobytes(), offsets
        finally:
            text.free()
            offs.free()

    def csv_write(self, path, src, first_id=1, offset=0, chunk_bytes=0):
        """The csv lines of DeviceArray ``src`` -> bytes ``offset ...`` of file ``path`` (xh_csv_write); returns their
        number.  The caller has written the header line."""
        return self.csv_write_many([(path, src, first_id, offset)], chunk_bytes)[0]

    def csv_write_many(self, items, chunk_bytes=0):
        """[(path, DeviceArray, first_id, offset), ...] -> the csv lines of each array into its file, the files written
        side by side (xh_csv_write_many, <= 16 per call); returns the bytes written per file."""
        items, written = list(items), []
        for k in range(0, len(items), 16):
            part = items[k:k + 16]
            n = len(part)
            srcs = (c_void_p * n)(*[_dptr(src) for _, src, _, _ in part])
            nrows = (c_int64 * n)(*[src.shape[0] for _, src, _, _ in part])
            ncols = (c_int64 * n)(*[src.shape[1] for _, src, _, _ in part])
            first = (c_int64 * n)(*[int(f) for _, _, f, _ in part])
            paths = (c_char_p * n)(*[os.fsencode(path) for path, _, _, _ in part])
            offs = (ctypes.c_uint64 * n)(*[int(o) for _, _, _, o in part])
            out = (ctypes.c_uint64 * n)()
            self._check(lib().xh_csv_write_many(self.handle, n, srcs, nrows, ncols, first, paths, offs, int(chunk_bytes), out))
            written += [int(v) for v in out]
        return written

    def timing_reset(self):
        self._check(lib().xh_timing_reset(self.handle))

    def comm_join(self):
        """Order the context's stream behind the side gather (xh_comm_join)."""
        self._check(lib().xh_comm_join(self.handle))

    def mark_begin(self, name):
        self._check(lib().xh_mark_begin(self.handle, name.encode()))

    def mark_end(self):
        self._check(lib().xh_mark_end(self.handle))

    def timing(self, name):
        ms, n = c_double(), c_int64()
        self._check(lib().xh_timing_get(self.handle, name.encode(), byref(ms), byref(n)))
        return ms.value, n.value

    def gather_rows(self, src, rows_dev, nrows, ncols, dst):
        self._check(lib().xh_gather_rows(self.handle, _dptr(src), _dptr(rows_dev), nrows, ncols, _dptr(dst)))

    def scatter_rows(self, src, rows_dev, nrows, ncols, dst):
        self._check(lib().xh_scatter_rows(self.handle, _dptr(src), _dptr(rows_dev), nrows, ncols, _dptr(dst)))

    def transpose(self, src, rows, cols, dst):
        self._check(lib().xh_transpose(self.handle, _dptr(src), rows, cols, _dptr(dst)))

    # ---- Penman-Monteith
    @staticmethod
    def _pm_tables(tables):
        """dict of host arrays (cL ... laimax) -> (PmTables, arrays to keep alive)."""
        keep = []
        t = PmTables()
        t.nlcs = int(np.asarray(tables['cL']).shape[0])
        for name, _ in PmTables._fields_[1:]:
            a = as_f64(tables[name]).ravel()
            want = t.nlcs * (12 if name in ('alpha', 'lai', 'laimin', 'laimax') else 1)
            if a.size != want:
                raise ValueError('PM table {} has {} values, expected {}'.format(name, a.size, want))
            keep.append(a)
            setattr(t, name, a.ctypes.data_as(POINTER(c_double)))
        return t, keep

    def run_fused(self, *, tables, ncell, nmonths, start_year, lc_years, water_idx, snow_idx, tas, tmin, rhs, wind, rsds,
                  rlds, tairprev, lct, elev, abcd_spinup, n_groups, basin_index, par_index, npar_rows, pars, precip,
                  abcd_tmin, pet, aet, q, sav, plan=None, routing_spinup=0, ndays=None, dt=10800.0, flow_dist=None,
                  velocity=None, area=None, S0=None, chs=None, avg=None, route_flags=0, block_months=0, mode=0):
        """PM -> ABCD -> MRTM as one pipelined call (xh_run_fused); arguments as in pm_pet / abcd / route_series.
        mode 1: the routing kernel starts after the first max(spin-ups) months and is fed the rest while it runs."""
        t, keep = self._pm_tables(tables)
        lcy = np.ascontiguousarray(lc_years, dtype=np.int32)
        bi = np.ascontiguousarray(basin_index, dtype=np.int32)
        pi = np.ascontiguousarray(par_index, dtype=np.int32)
        nd = None if ndays is None else np.ascontiguousarray(ndays, dtype=np.int32)
        if plan is not None and (nd is None or nd.size != nmonths):
            raise ValueError('ndays must have nmonths entries')
        a = FusedArgs()
        a.ncell, a.nmonths, a.start_year = ncell, nmonths, start_year
        a.pm = ctypes.pointer(t)
        a.n_lc_years, a.h_lc_years, a.water_idx, a.snow_idx = len(lcy), lcy.ctypes.data, water_idx, snow_idx
        for name, v in (('d_tas', tas), ('d_tmin', tmin), ('d_rhs', rhs), ('d_wind', wind), ('d_rsds', rsds),
                        ('d_rlds', rlds), ('d_tairprev', tairprev), ('d_lct', lct), ('d_elev', elev), ('d_pars', pars),
                        ('d_precip', precip), ('d_abcd_tmin', abcd_tmin), ('d_flow_dist', flow_dist),
                        ('d_velocity', velocity), ('d_area', area), ('d_S0', S0), ('d_pet', pet), ('d_aet', aet),
                        ('d_q', q), ('d_sav', sav), ('d_chstorage', chs), ('d_avgchflow', avg)):
            setattr(a, name, _dptr(v))
        a.abcd_spinup, a.n_groups, a.npar_rows = abcd_spinup, n_groups, npar_rows
        a.h_basin_index, a.h_par_index = bi.ctypes.data, pi.ctypes.data
        a.plan = None if plan is None else plan.handle
        a.routing_spinup, a.dt, a.route_flags, a.block_months = routing_spinup, float(dt), int(route_flags), int(block_months)
        a.h_ndays = None if nd is None else nd.ctypes.data
        a.mode = int(mode)
        self._check(lib().xh_run_fused(self.handle, byref(a)))

    def pm_pet(self, tables, ncell, nmonths, start_year, lc_years, water_idx, snow_idx, tas, tmin, rhs, wind, rsds,
               rlds, tairprev, lct, elev, pet):
        """tables: dict of host arrays (cL ... laimax); the rest device arrays / pointers."""
        t, keep = self._pm_tables(tables)
        lcy = np.ascontiguousarray(lc_years, dtype=np.int32)
        self._check(lib().xh_pm_pet(self.handle, byref(t), ncell, nmonths, start_year, len(lcy), _host_ptr(lcy),
                                    water_idx, snow_idx, _dptr(tas), _dptr(tmin), _dptr(rhs), _dptr(wind),
                                    _dptr(rsds), _dptr(rlds), _dptr(tairprev), _dptr(lct), _dptr(elev), _dptr(pet)))

    # ---- ABCD
    def abcd(self, ncell, nmonths, spinup, n_groups, basin_index, par_index, npar_rows, pars, pet, precip, tmin,
             aet, q, sav, sm0=None, gw0=None):
        bi = np.ascontiguousarray(basin_index, dtype=np.int32)
        pi = np.ascontiguousarray(par_index, dtype=np.int32)
        self._check(lib().xh_abcd(self.handle, ncell, nmonths, spinup, n_groups, _host_ptr(bi), _host_ptr(pi),
                                  npar_rows, _dptr(pars), _dptr(pet), _dptr(precip), _dptr(tmin), _dptr(aet),
                                  _dptr(q), _dptr(sav), _dptr(sm0), _dptr(gw0)))

    # ---- Hargreaves PET / GWAM runoff
    def hargreaves_pet(self, ncell, nmonths, temp, dtr, lat_rad, solar_dec, dr, ndays, pet):
        """temp / dtr / lat_rad / pet device arrays; solar_dec / dr / ndays host arrays of nmonths values."""
        tabs = [np.ascontiguousarray(a, dtype=np.float64) for a in (solar_dec, dr, ndays)]
        if any(t.size != nmonths for t in tabs):
            raise ValueError('solar_dec, dr and ndays must have nmonths entries')
        self._check(lib().xh_hargreaves_pet(self.handle, ncell, nmonths, _dptr(temp), _dptr(dtr), _dptr(lat_rad),
                                            _host_ptr(tabs[0]), _host_ptr(tabs[1]), _host_ptr(tabs[2]), _dptr(pet)))

    def gwam(self, ncell, nmonths, spinup, precip_col_spinup, precip_col_sim, indexing, pet, precip, sm_max, sm0, aet,
             q, sav, sm_end=None):
        self._check(lib().xh_gwam(self.handle, ncell, nmonths, spinup, precip_col_spinup, precip_col_sim, float(indexing),
                                  _dptr(pet), _dptr(precip), _dptr(sm_max), _dptr(sm0), _dptr(aet), _dptr(q), _dptr(sav),
                                  _dptr(sm_end)))

    # ---- Hargreaves-Samani / Thornthwaite PET
    def hs_pet(self, ncell, nmonths, tas, tmax, tmin, lat_deg, ndays, pet):
        """tas / tmax / tmin / lat_deg / pet device arrays; ndays a host array of nmonths values."""
        nd = np.ascontiguousarray(ndays, dtype=np.float64)
        if nd.size != nmonths:
            raise ValueError('ndays must have nmonths entries')
        self._check(lib().xh_hs_pet(self.handle, ncell, nmonths, _dptr(tas), _dptr(tmax), _dptr(tmin), _dptr(lat_deg),
                                    _host_ptr(nd), _dptr(pet)))

    def thornthwaite_pet(self, ncell, nmonths, start_year, daylight_mode, tas, lat_rad, pet, daylight=None):
        """tas / lat_rad / pet (/ daylight [ncell, 24]) device arrays; daylight_mode XH_DAYLIGHT_REFERENCE or _MONTHLY."""
        self._check(lib().xh_thornthwaite_pet(self.handle, ncell, nmonths, start_year, daylight_mode, _dptr(tas),
                                              _dptr(lat_rad), _dptr(pet), _dptr(daylight)))

    # ---- MRTM
    def route_plan(self, indptr, indices, sign):
        return RoutePlan(self, indptr, indices, sign)

    def route_series(self, plan, nmonths, spinup_months, ndays, dt, flow_dist, velocity, area, runoff, S0, chs, avg,
                     S_end=None, F_end=None, flags=XH_ROUTE_DEFAULT):
        nd = np.ascontiguousarray(ndays, dtype=np.int32)
        if nd.size != nmonths:
            raise ValueError('ndays must have nmonths entries')
        self._check(lib().xh_route_series(self.handle, plan.handle, nmonths, spinup_months, _host_ptr(nd), float(dt),
                                          _dptr(flow_dist), _dptr(velocity), _dptr(area), _dptr(runoff), _dptr(S0),
                                          _dptr(chs), _dptr(avg), _dptr(S_end), _dptr(F_end), int(flags)))

    # ---- calibration objective
    def calib_objective(self, ncell_b, nmonths, spinup, pars, pet_t, precip_t, tmin_t, area, obs, want_series=False):
        pars = as_f64(pars)
        nmem, npar = pars.shape
        obs = as_f64(obs)
        if obs.size != nmonths:
            raise ValueError('obs must have nmonths entries')
        ed = np.empty(nmem)
        series = np.empty((nmem, nmonths)) if want_series else None
        self._check(lib().xh_calib_objective(self.handle, ncell_b, nmonths, spinup, nmem, npar, _host_ptr(pars),
                                             _dptr(pet_t), _dptr(precip_t), _dptr(tmin_t), _dptr(area),
                                             _host_ptr(obs), _host_ptr(ed),
                                             _host_ptr(series) if want_series else None))
        return (ed, series) if want_series else ed

    def calib_objective_multi(self, ncells, nmonths, spinup, pars, pet_t, precip_t, tmin_t, area, obs, want_series=False):
        """Several basins at once. pars [nb, nmem, npar]; pet_t / precip_t / tmin_t / area: lists of DeviceArrays
        (tmin_t / area may be None); obs [nb, nmonths]. Returns ed [nb, nmem] (and series [nb, nmem, nmonths])."""
        pars = as_f64(pars)
        nb, nmem, npar = pars.shape
        obs = as_f64(obs)
        if obs.shape != (nb, nmonths):
            raise ValueError('obs must be [nbasins, nmonths]')
        nc = np.ascontiguousarray(ncells, dtype=np.int64)
        ptrs = lambda lst: None if lst is None else (c_void_p * nb)(*[_dptr(x) for x in lst])
        p_pet, p_pr, p_tn, p_ar = ptrs(pet_t), ptrs(precip_t), ptrs(tmin_t), ptrs(area)
        ed = np.empty((nb, nmem))
        series = np.empty((nb, nmem, nmonths)) if want_series else None
        self._check(lib().xh_calib_objective_multi(self.handle, nb, _host_ptr(nc), nmonths, spinup, nmem, npar,
                                                   _host_ptr(pars), p_pet, p_pr, p_tn, p_ar, _host_ptr(obs), _host_ptr(ed),
                                                   _host_ptr(series) if want_series else None))
        return (ed, series) if want_series else ed

    def calib_flow_objective_multi(self, ncells, nmonths, spinup, pars, pet_t, precip_t, tmin_t, tables, obs,
                                   want_series=False, velocity=False):
        """Streamflow objective (set_calibrate = 1) of several basins at once: as calib_objective_multi, with the
        closure tables ``tables`` (calibrate.flow_tables.FlowTables) instead of areas. series = outlet flow [m3/s].
        velocity: the rows of pars end in the basin's velocity scale v, [a, b, c, d, (m), v]."""
        pars = as_f64(pars)
        nb, nmem, npar = pars.shape
        npar -= 1 if velocity else 0            # the library counts the ABCD genes
        obs = as_f64(obs)
        if obs.shape != (nb, nmonths):
            raise ValueError('obs must be [nbasins, nmonths]')
        nc = np.ascontiguousarray(ncells, dtype=np.int64)
        ptrs = lambda lst: None if lst is None else (c_void_p * nb)(*[_dptr(x) for x in lst])
        desc = flow_desc(tables)
        ed = np.empty((nb, nmem))
        series = np.empty((nb, nmem, nmonths)) if want_series else None
        if velocity:
            vdesc = velocity_desc(tables)
            self._check(lib().xh_calib_flow_velocity_objective_multi(
                self.handle, nb, _host_ptr(nc), nmonths, spinup, nmem, npar, _host_ptr(pars), ptrs(pet_t), ptrs(precip_t),
                ptrs(tmin_t), byref(desc), byref(vdesc), _host_ptr(obs), _host_ptr(ed),
                _host_ptr(series) if want_series else None))
            return (ed, series) if want_series else ed
        self._check(lib().xh_calib_flow_objective_multi(self.handle, nb, _host_ptr(nc), nmonths, spinup, nmem, npar,
                                                        _host_ptr(pars), ptrs(pet_t), ptrs(precip_t), ptrs(tmin_t),
                                                        byref(desc), _host_ptr(obs), _host_ptr(ed),
                                                        _host_ptr(series) if want_series else None))
        return (ed, series) if want_series else ed

    def calib_gauge_objective_multi(self, ncells, nmonths, spinup, pars, pet_t, precip_t, tmin_t, tables, want_series=False,
                                    want_gauges=False, velocity=False):
        """Gauge form of the streamflow objective: ``tables`` = calibrate.gauge_tables.GaugeTables (union closures, gauges
        and their observations [ngauge, nmonths], NaN = missing).  Returns ed [nb, nmem] -- then, as asked, series
        [ngauge, nmem, nmonths] (the gauge flows, m3/s) and ed_gauge [ngauge, nmem].
        velocity: the rows of pars end in the basin's velocity scale v, [a, b, c, d, (m), v]."""
        pars = as_f64(pars)
        nb, nmem, npar = pars.shape
        npar -= 1 if velocity else 0
        obs = as_f64(tables.obs)
        ng = int(tables.gauge_ptr[-1])
        if obs.shape != (ng, nmonths) or len(tables.basins) != nb:
            raise ValueError('the gauge tables hold {} basins and observations {}, not {} basins and {}'.format(
                len(tables.basins), obs.shape, nb, (ng, nmonths)))
        nc = np.ascontiguousarray(ncells, dtype=np.int64)
        ptrs = lambda lst: None if lst is None else (c_void_p * nb)(*[_dptr(x) for x in lst])
        desc = gauge_desc(tables)
        ed = np.empty((nb, nmem))
        series = np.empty((ng, nmem, nmonths)) if want_series else None
        edg = np.empty((ng, nmem)) if want_gauges else None
        if velocity:
            vdesc = velocity_desc(tables)
            self._check(lib().xh_calib_gauge_velocity_objective_multi(
                self.handle, nb, _host_ptr(nc), nmonths, spinup, nmem, npar, _host_ptr(pars), ptrs(pet_t), ptrs(precip_t),
                ptrs(tmin_t), byref(desc), byref(vdesc), _host_ptr(obs), _host_ptr(ed),
                _host_ptr(edg) if want_gauges else None, _host_ptr(series) if want_series else None))
        else:
            self._check(lib().xh_calib_gauge_objective_multi(self.handle, nb, _host_ptr(nc), nmonths, spinup, nmem, npar,
                                                             _host_ptr(pars), ptrs(pet_t), ptrs(precip_t), ptrs(tmin_t),
                                                             byref(desc), _host_ptr(obs), _host_ptr(ed),
                                                             _host_ptr(edg) if want_gauges else None,
                                                             _host_ptr(series) if want_series else None))
        out = (ed,) + ((series,) if want_series else ()) + ((edg,) if want_gauges else ())
        return out if len(out) > 1 else ed

    # ---- output aggregation
    def agg_time(self, ncell, ncols, group, mode, scale, src, dst):
        self._check(lib().xh_agg_time(self.handle, ncell, ncols, group, mode, _dptr(scale), _dptr(src), _dptr(dst)))

    def agg_spatial(self, ncell, ncols, n_groups, group_index, src, dst):
        gi = np.ascontiguousarray(group_index, dtype=np.int32)
        self._check(lib().xh_agg_spatial(self.handle, ncell, ncols, n_groups, _host_ptr(gi), _dptr(src), _dptr(dst)))

    def nan_to_num(self, arr):
        """In-place np.nan_to_num of a DeviceArray."""
        self._check(lib().xh_nan_to_num(self.handle, _dptr(arr), arr.size))
        return arr

    def drought_thresholds(self, ncell, nmonths, month0, nyear, nper, k_prev, k_next, gamma, hydro, thresh):
        self._check(lib().xh_drought_thresholds(self.handle, ncell, nmonths, month0, nyear, nper, k_prev, k_next,
                                                float(gamma), _dptr(hydro), _dptr(thresh)))

    def drought_stats(self, ncell, nmonths, nthresh, hydro, thresh, severity, intensity, duration):
        self._check(lib().xh_drought_stats(self.handle, ncell, nmonths, nthresh, _dptr(hydro), _dptr(thresh),
                                           _dptr(severity), _dptr(intensity), _dptr(duration)))

    # ---- hydropower (csrc/xh_hydro.hip)
    def hpot_qmax(self, ncell, nmonths, k_prev, k_next, gamma, q, qmax):
        self._check(lib().xh_hpot_qmax(self.handle, ncell, nmonths, k_prev, k_next, float(gamma), _dptr(q), _dptr(qmax)))

    def hpot_energy(self, ncell, nmonths, nyears, year_of_month, c_ef_sww, c_hours, c_twh, c_ej, q, qmax, elev, E):
        self._check(lib().xh_hpot_energy(self.handle, ncell, nmonths, nyears, _dptr(year_of_month), float(c_ef_sww),
                                         float(c_hours), float(c_twh), float(c_ej), _dptr(q), _dptr(qmax), _dptr(elev),
                                         _dptr(E)))

    def hpot_region(self, ngroups, nyears, indptr, cells, E, R):
        self._check(lib().xh_hpot_region(self.handle, ngroups, nyears, _dptr(indptr), _dptr(cells), _dptr(E), _dptr(R)))

    def hact_inflow(self, ncell, nmonths, ndams, month0, dam_cell, catch, assumed, cumecs_to_mm3, q, inflow, env, bad):
        self._check(lib().xh_hact_inflow(self.handle, ncell, nmonths, ndams, month0, _dptr(dam_cell), _dptr(catch),
                                         _dptr(assumed), float(cumecs_to_mm3), _dptr(q), _dptr(inflow), _dptr(env),
                                         _dptr(bad)))

    def hact_sim(self, nmonths, ndams, nyears, month0, year_of_month, sww, secs_in_month, inflow, env, rc, par, power,
                 annual, bad_month):
        self._check(lib().xh_hact_sim(self.handle, nmonths, ndams, nyears, month0, _dptr(year_of_month), float(sww),
                                      float(secs_in_month), _dptr(inflow), _dptr(env), _dptr(rc), _dptr(par),
                                      _dptr(power), _dptr(annual), _dptr(bad_month)))

    # ---- diagnostics (csrc/xh_diag.hip)
    def diag_cell_total(self, ncell, ncols, src, div1, scale, div2, out, out_stride=1):
        self._check(lib().xh_diag_cell_total(self.handle, ncell, ncols, _dptr(src), float(div1), _dptr(scale), float(div2),
                                             _dptr(out), out_stride))

    def diag_group_sum(self, ncell, k, ngroups, group_index, vals, sums, counts):
        gi = np.ascontiguousarray(group_index, dtype=np.int32)
        self._check(lib().xh_diag_group_sum(self.handle, ncell, k, ngroups, _host_ptr(gi), _dptr(vals), _dptr(sums),
                                            _dptr(counts)))

    # ---- ensemble statistics (csrc/xh_ens.hip)
    def ens_stats(self, n, members, stats=(), quantiles=(), out=None):
        """Across-member statistics of ``members`` (DeviceArrays / device pointers of n float64 each): ``stats`` out of
        'mean', 'std', 'min', 'max' and ``quantiles`` in [0, 1].  ``out``: one DeviceArray / pointer per statistic, in the
        library's order -- mean, std, min, max as requested, then the quantiles as given.  Every member array is read once."""
        unknown = [s for s in stats if s not in ENS_STAT_BITS]
        if unknown:
            raise ValueError('unknown ensemble statistic {}'.format(unknown))
        mask = 0
        for s in stats:
            mask |= ENS_STAT_BITS[s]
        q = np.ascontiguousarray(quantiles, dtype=np.float64).reshape(-1)
        nout = bin(mask).count('1') + q.size
        if out is None or len(out) != nout:
            raise ValueError('{} statistics need {} output arrays'.format(nout, nout))
        nmem = len(members)
        p_mem = (c_void_p * max(nmem, 1))(*[_dptr(m) for m in members])
        p_out = (c_void_p * max(nout, 1))(*[_dptr(o) for o in out])
        self._check(lib().xh_ens_stats(self.handle, int(n), nmem, p_mem, mask, q.size, _host_ptr(q) if q.size else None,
                                       p_out))

    # ---- member skill (csrc/xh_skill.hip)
    def basin_kge(self, ncell, nmonths, nbasins, start, cells, q, area, obs, ed, series=None):
        """ED per basin of ``q`` [ncell, nmonths] against ``obs`` [nbasins, nmonths] (xh_basin_kge); all device arrays:
        ``start`` int64 [nbasins + 1] into ``cells`` int32 (ascending per basin), ``area`` None for mm_per_mth, ``series``
        an optional [nbasins, nmonths] output.  Asynchronous."""
        self._check(lib().xh_basin_kge(self.handle, int(ncell), int(nmonths), int(nbasins), _dptr(start), _dptr(cells),
                                       _dptr(q), _dptr(area), _dptr(obs), _dptr(series), _dptr(ed)))

    # ---- skill at stream gauges (csrc/xh_gauge_skill.hip)
    def gauge_skill(self, ncell, nmonths, ngauge, gauge_cell, flow, obs, metrics, series=None):
        """The eight columns of xh_gauge_skill per gauge -- n, ED, r, alpha, beta, NSE, PBIAS, RMSE -- of ``flow``
        [ncell, nmonths] (Avg_ChFlow, m3/s) at the cells ``gauge_cell`` (int32 [ngauge], 0-based) against ``obs`` [ngauge,
        nmonths] (NaN = no observation) into ``metrics`` [ngauge, 8]; ``series``: an optional [ngauge, nmonths] output, the
        flow rows of the gauge cells.  All DeviceArrays or raw device addresses (a member's slice).  Asynchronous."""
        self._check(lib().xh_gauge_skill(self.handle, int(ncell), int(nmonths), int(ngauge), _dptr(gauge_cell), _dptr(flow),
                                         _dptr(obs), _dptr(series), _dptr(metrics)))

    # ---- standardized drought indices (csrc/xh_sindex.hip)
    def std_index(self, ncell, nmonths, scales, ref_month0, ref_nyear, dist, max_shape, x, index, par_in=None, par_out=None,
                  minus=None):
        """SRI / SSI / SSFI / SPI / SPEI of ``x`` [ncell, nmonths] -- of ``x - minus`` with a subtrahend ``minus`` [ncell,
        nmonths], subtracted as the rows enter LDS -- at the accumulation ``scales`` (months) in one pass (xh_std_index2):
        ``index``: one [ncell, nmonths] array per scale; ``dist``: 'gamma', 'empirical' or 'loglogistic'; ``par_in`` /
        ``par_out``: None or one [ncell, 12, 4] table per scale ((q0, alpha, beta, n) of gamma, (alpha, beta, gamma, n) of
        loglogistic) -- used instead of fitting / receiving the fit.  All DeviceArrays or raw device addresses.
        Asynchronous."""
        if dist not in STD_INDEX_DIST2:
            raise ValueError("unknown distribution '{}' (gamma, empirical or loglogistic)".format(dist))
        k = np.ascontiguousarray(scales, dtype=np.int32).reshape(-1)
        for name, arrs in (('index', index), ('par_in', par_in), ('par_out', par_out)):
            if arrs is not None and len(arrs) != k.size:
                raise ValueError('{} scales need {} {} arrays, not {}'.format(k.size, k.size, name, len(arrs)))

        def table(arrs):
            return None if arrs is None else (c_void_p * max(k.size, 1))(*[_dptr(a) for a in arrs])
        self._check(lib().xh_std_index2(self.handle, int(ncell), int(nmonths), int(k.size), k.ctypes.data_as(POINTER(c_int32)),
                                        int(ref_month0), int(ref_nyear), STD_INDEX_DIST2[dist], float(max_shape), _dptr(x),
                                        _dptr(minus), table(par_in), table(par_out), table(index)))

    # ---- trend per row (csrc/xh_trend.hip)
    def trend(self, nrows, row_stride, col0, ncol, nseason, z_conf, x, out):
        """Mann-Kendall test and Theil-Sen slope of the window ``x[r, col0 : col0 + ncol]`` of every row of ``x`` [nrows,
        row_stride] into ``out`` [nrows, 10] = n, s, var_s, z, p, slope, intercept, slope_lo, slope_hi, npairs (xh_trend,
        which states the definition): column t is season ``t mod nseason`` at ``t / nseason`` years; ``z_conf`` is the
        normal quantile of (1 - confidence) / 2.  DeviceArrays or raw device addresses.  Asynchronous."""
        self._check(lib().xh_trend(self.handle, int(nrows), int(row_stride), int(col0), int(ncol), int(nseason), float(z_conf),
                                   _dptr(x), _dptr(out)))

    # ---- annual extremes per row (csrc/xh_extremes.hip)
    def extremes(self, nrows, row_stride, col0, nyear, kind, min_years, return_periods, x, table, annual=None, T_year=None,
                 par_in=None):
        """Annual maxima (``kind`` 'max' or 0) or minima ('min' or 1) of the monthly window ``x[r, col0 : col0 + 12 nyear]`` of
        every row of ``x`` [nrows, row_stride], the GEV fitted to them by L-moments, the return levels of ``return_periods``
        (at most 8, each > 1) and every year's return period (xh_extremes, which states the definition): ``table`` [nrows,
        8 + nT] = n, l1, l2, t3, t4, k, alpha, xi, x_T...; ``annual`` and ``T_year`` [nrows, nyear] or None; ``par_in`` [nrows,
        8]: the parameters of another call instead of a fit.  DeviceArrays or raw device addresses.  Asynchronous."""
        T = np.ascontiguousarray(return_periods, dtype=np.float64).ravel()
        kind = EXTREMES_KIND.get(kind, kind) if isinstance(kind, str) else kind
        self._check(lib().xh_extremes(self.handle, int(nrows), int(row_stride), int(col0), int(nyear), int(kind), int(min_years),
                                      int(T.size), T.ctypes.data_as(c_void_p) if T.size else None, _dptr(x), _dptr(par_in),
                                      _dptr(table), _dptr(annual), _dptr(T_year)))

    def extremes_boot(self, nrows, row_stride, col0, nyear, kind, min_years, return_periods, B, confidence, seed, x, ci, rep=None,
                      row0=0):
        """Bootstrap intervals of the GEV shape and the return levels of the window of ``extremes`` (xh_extremes_boot, which
        states the definition): ``B`` replicates (2 .. 2048) of every row's annual series, drawn from ``seed`` and the row's
        number ``row0 + r``, refitted, and the percentiles (1 -+ ``confidence``) / 2 of the refitted values: ``ci`` [nrows,
        3 + 2 nT] = nb, k_lo, k_hi, x_T_lo, x_T_hi, ...; ``rep`` [nrows, B, 5 + nT] or None: every replicate's l1, l2, t3, t4, k and
        levels.  DeviceArrays or raw device addresses.  Asynchronous."""
        T = np.ascontiguousarray(return_periods, dtype=np.float64).ravel()
        kind = EXTREMES_KIND.get(kind, kind) if isinstance(kind, str) else kind
        self._check(lib().xh_extremes_boot(self.handle, int(nrows), int(row_stride), int(col0), int(nyear), int(kind), int(min_years),
                                           int(T.size), T.ctypes.data_as(c_void_p) if T.size else None, int(B), float(confidence),
                                           int(seed), int(row0), _dptr(x), _dptr(ci), _dptr(rep)))

    # ---- flow duration curve and regime signatures per row (csrc/xh_signatures.hip)
    def signatures(self, nrows, row_stride, col0, nyear, cal0, probabilities, x, table, fdc=None, regime=None):
        """Flow duration curve and regime signatures of the monthly window ``x[r, col0 : col0 + 12 nyear]`` of every row of ``x``
        [nrows, row_stride], whose first column is calendar month ``cal0`` (0 = January) (xh_signatures, which states the
        definition): ``table`` [nrows, 18] = n, n_zero, mean, std, cv, median, lag1, flashiness, fdc_slope, regime_total,
        peak_month, low_month, seasonality, centroid, concentration, n_years, annual_mean, annual_cv; ``fdc`` [nrows, nP] or
        None: the linear quantiles of ``probabilities`` (at most 16, each strictly between 0 and 1); ``regime`` [nrows, 12]
        or None: the calendar months' means.  DeviceArrays or raw device addresses.  Asynchronous."""
        p = np.ascontiguousarray(probabilities, dtype=np.float64).ravel()
        self._check(lib().xh_signatures(self.handle, int(nrows), int(row_stride), int(col0), int(nyear), int(cal0), int(p.size),
                                        p.ctypes.data_as(c_void_p) if p.size else None, _dptr(x), _dptr(table), _dptr(fdc),
                                        _dptr(regime)))

    # ---- water balance and Budyko signatures per row (csrc/xh_wbalance.hip)
    def water_balance(self, nrows, row_stride, col0, nyear, max_lag, omega0, precip, pet, q, aet, table, annual=None, xcorr=None):
        """Water balance and Budyko signatures of the monthly window ``[r, col0 : col0 + 12 nyear]`` of every row of ``precip``,
        ``pet``, ``q`` and ``aet`` (or None) [nrows, row_stride] (xh_water_balance, which states the definition): ``table``
        [nrows, 21] = n_years, n_months, p_mean, pet_mean, aet_mean, q_mean, runoff_ratio, aridity, evaporative, residual,
        closure, omega, budyko_dev, elast_p, elast_pet, elast_p_ls, elast_pet_ls, r_pq, dry_fraction, lag_peak, r_peak;
        ``annual`` [nrows, 4, nyear] or None: the annual totals of P, PET, AET and Q; ``xcorr`` [nrows, max_lag + 1] or None:
        the correlation of P with Q ``k`` months later.  DeviceArrays or raw device addresses.  Asynchronous."""
        self._check(lib().xh_water_balance(self.handle, int(nrows), int(row_stride), int(col0), int(nyear), int(max_lag),
                                           float(omega0), _dptr(precip), _dptr(pet), _dptr(q), _dptr(aet), _dptr(table),
                                           _dptr(annual), _dptr(xcorr)))

    # ---- bench support
    def synth_forcing(self, seed, ncell, nmonths, lat, out, nan_frac=0.001, cell_ids=None):
        """out: dict name -> DeviceArray for synth.FORCING_NAMES (or only 'tas'). cell_ids: device int64 [ncell]
        global cell of each row (None = 0..ncell-1; -1 = a row of zeros)."""
        g = lambda k: _dptr(out.get(k))
        self._check(lib().xh_synth_forcing(self.handle, int(seed), float(nan_frac), ncell, nmonths, _dptr(lat),
                                           _dptr(cell_ids), g('tas'), g('tmin'), g('rhs'), g('wind'), g('rsds'),
                                           g('rlds'), g('precip'), g('abcd_tmin')))


class RoutePlan:
    """Device-side routing layout for one UM matrix (xh_route_plan)."""

    def __init__(self, ctx, indptr, indices, sign):
        self.ctx = ctx
        ip = np.ascontiguousarray(indptr, dtype=np.int64)
        ix = np.ascontiguousarray(indices, dtype=np.int32)
        sg = np.ascontiguousarray(sign, dtype=np.int8)
        self.ncell = ip.size - 1
        h = c_void_p()
        ctx._check(lib().xh_route_plan_create(ctx.handle, self.ncell, _host_ptr(ip), _host_ptr(ix), _host_ptr(sg),
                                              byref(h)))
        self.handle = h.value

    def info(self):
        arr = (c_int64 * 16)()
        self.ctx._check(lib().xh_route_plan_info(self.handle, arr))
        keys = ('networks', 'largest_network', 'units', 'fallback_cells', 'largest_unit', 'slots', 'single_downstream',
                'flow_units', 'flow_edges', 'flow_depth', 'flow_cells', 'flow_max_imports', 'skew_max_lag',
                'last_tree_kernel', 'reroutes', 'validated')
        return dict(zip(keys, list(arr)))

    def prepare(self, flow_dist, velocity, dt):
        """xh_route_plan_prepare: host copies of flow distance and velocity [ncell] and dt.  Makes the PREPARED plan of the
        default (reassociated) routing form -- folded leaves, single running sums: both rest on which cells can fire -- which
        calls with this dt then route on; a no-op in a process whose default form is the bit-exact one.  May be called again:
        the same data is a cheap no-op, data that changes which cells can fire replaces the prepared plan (and lifts a guard
        trip's ban on the old one)."""
        L = np.ascontiguousarray(flow_dist, dtype=np.float64)
        v = np.ascontiguousarray(velocity, dtype=np.float64)
        if L.size != self.ncell or v.size != self.ncell:
            raise ValueError('flow_dist / velocity must have one value per cell')
        self.ctx._check(lib().xh_route_plan_prepare(self.ctx.handle, self.handle, _host_ptr(L), _host_ptr(v), float(dt)))

    def rsum_info(self):
        """The reassociated plan the last call ran on (xh_route_plan_rsum_info)."""
        arr = (c_int64 * 8)()
        self.ctx._check(lib().xh_route_plan_rsum_info(self.handle, arr))
        out = dict(zip(('units', 'folded', 'fold_disabled', 'prepared_folded', 'pair_cells', 'prepared_pair_cells', 'guard_trips',
                        'pair_units'), list(arr)))
        fn = getattr(lib(), 'xh_route_plan_linear_units', None)      # (OPTIONAL_SYMBOLS: an older library has no such units)
        out['linear_units'] = int(fn(self.handle)) if fn is not None else 0
        return out

    def stats(self):
        """[units, 6] uint64 per-unit accounting of the last launch (needs XH_FLOW_STATS=1), or None."""
        n = c_int64(0)
        self.ctx._check(lib().xh_route_plan_stats(self.handle, 0, None, byref(n)))
        if n.value == 0:
            return None
        out = np.empty(n.value, dtype=np.uint64)
        self.ctx._check(lib().xh_route_plan_stats(self.handle, n.value, _host_ptr(out), byref(n)))
        return out.reshape(-1, 6)

    def close(self):
        if self.handle is not None and self.ctx.handle is not None:
            lib().xh_route_plan_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def comm_unique_id():
    """128-byte RCCL id made on rank 0; the launcher carries it to the other ranks (xh_comm_unique_id)."""
    buf = ctypes.create_string_buffer(128)
    _check_host(lib().xh_comm_unique_id(buf, 128))
    return buf.raw


class Comm:
    """RCCL communicator of one rank for the write-out gather (xh_comm)."""

    def __init__(self, ctx, nranks, rank, unique_id):
        self.ctx, self.nranks, self.rank = ctx, int(nranks), int(rank)
        h = c_void_p()
        # RCCL prints a version banner on stdout when a communicator is created; stdout belongs to the caller (bench.py
        # prints ONE JSON line there), so the banner is sent to stderr
        import sys
        sys.stdout.flush()
        saved = os.dup(1)
        try:
            os.dup2(2, 1)
            rc = lib().xh_comm_create(ctx.handle, self.nranks, self.rank, unique_id, len(unique_id), byref(h))
            ctypes.CDLL(None).fflush(None)          # the banner sits in C stdio's buffer until flushed
        finally:
            os.dup2(saved, 1)
            os.close(saved)
        ctx._check(rc)
        self.handle = h.value

    def info(self):
        """{'ranks', 'rank', 'sends', 'recvs'}: ncclSend / ncclRecv calls issued through this communicator (xh_comm_info)."""
        arr = (c_int64 * 4)()
        self.ctx._check(lib().xh_comm_info(self.handle, arr))
        return dict(zip(('ranks', 'rank', 'sends', 'recvs'), list(arr)))

    def gather_rows(self, local, counts, ncols, perm=None, out=None, root=0, side=False):
        """local: list of DeviceArrays [counts[rank], ncols]; on the root ``perm`` (device int64, rank-major destination
        rows) and ``out`` (list of DeviceArrays [sum(counts), ncols]). Asynchronous.  ``side``: on the context's gather
        stream, beside what the context's own stream does next (xh_comm_gather_rows_side; Context.comm_join orders the
        context's stream behind it)."""
        nvar = len(local)
        cn = np.ascontiguousarray(counts, dtype=np.int64)
        p_local = (c_void_p * nvar)(*[_dptr(x) for x in local])
        p_out = None if out is None else (c_void_p * nvar)(*[_dptr(x) for x in out])
        fn = lib().xh_comm_gather_rows_side if side else lib().xh_comm_gather_rows
        self.ctx._check(fn(self.ctx.handle, self.handle, int(root), nvar, p_local, int(ncols), _host_ptr(cn), _dptr(perm),
                           p_out))

    def close(self):
        if self.handle is not None:
            lib().xh_comm_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CalibDE:
    """Device-side differential evolution over several basins in lock-step (xh_calib_de).

    ncells [nb]; pet_t / precip_t / tmin_t / area: lists of DeviceArrays ([nmonths, ncell_b]; tmin_t / area may be
    None) that must stay alive as long as the session; obs [nb, nmonths]; bounds [(lo, hi)] * npar; keys [nb] RNG
    stream of each basin (e.g. the basin number) so that a basin's search does not depend on its companions.
    flow: calibrate.flow_tables.FlowTables (the streamflow objective at the outlets) or calibrate.gauge_tables.GaugeTables
    (at stream gauges; obs is then [ngauge, nmonths], NaN = missing).  velocity (with flow): the last of the bounds is
    that of the basins' velocity scale, which the search calibrates with the ABCD parameters."""

    def __init__(self, ctx, ncells, nmonths, spinup, nmembers, bounds, pet_t, precip_t, tmin_t, area, obs, seed=0,
                 keys=None, flow=None, velocity=False):
        self.ctx = ctx
        nc = np.ascontiguousarray(ncells, dtype=np.int64)
        self.nb, self.n, self.d = int(nc.size), int(nmembers), len(bounds)
        obs = as_f64(obs)
        gauge_form = flow is not None and hasattr(flow, 'gauge_ptr')
        if obs.shape != ((int(flow.gauge_ptr[-1]) if gauge_form else self.nb), nmonths):
            raise ValueError('obs must be [ngauge, nmonths]' if gauge_form else 'obs must be [nbasins, nmonths]')
        lo, hi = as_f64([b[0] for b in bounds]), as_f64([b[1] for b in bounds])
        kk = None if keys is None else np.ascontiguousarray(keys, dtype=np.uint64)
        ptrs = lambda lst: None if lst is None else (c_void_p * self.nb)(*[_dptr(x) for x in lst])
        self._keep = (pet_t, precip_t, tmin_t, area)
        h = c_void_p()
        if velocity:                # the velocity forms: d - 1 ABCD genes, then v
            if flow is None:
                raise ValueError('the velocity scale belongs to the streamflow objective: flow is None')
            create = lib().xh_calib_de_create_gauge_velocity if gauge_form else lib().xh_calib_de_create_flow_velocity
            desc = gauge_desc(flow) if gauge_form else flow_desc(flow)
            ctx._check(create(ctx.handle, self.nb, _host_ptr(nc), None if kk is None else _host_ptr(kk), nmonths, spinup,
                              self.n, self.d - 1, ptrs(pet_t), ptrs(precip_t), ptrs(tmin_t), byref(desc),
                              byref(velocity_desc(flow)), _host_ptr(obs), _host_ptr(lo), _host_ptr(hi),
                              int(seed) & 0xFFFFFFFFFFFFFFFF, byref(h)))
            self.handle = h.value
            return
        if gauge_form:              # the streamflow objective at gauges: flow = calibrate.gauge_tables.GaugeTables
            ctx._check(lib().xh_calib_de_create_gauge(ctx.handle, self.nb, _host_ptr(nc),
                                                      None if kk is None else _host_ptr(kk), nmonths, spinup, self.n, self.d,
                                                      ptrs(pet_t), ptrs(precip_t), ptrs(tmin_t), byref(gauge_desc(flow)),
                                                      _host_ptr(obs), _host_ptr(lo), _host_ptr(hi),
                                                      int(seed) & 0xFFFFFFFFFFFFFFFF, byref(h)))
            self.handle = h.value
            return
        if flow is not None:        # the streamflow objective: flow = calibrate.flow_tables.FlowTables (copied at creation)
            ctx._check(lib().xh_calib_de_create_flow(ctx.handle, self.nb, _host_ptr(nc),
                                                     None if kk is None else _host_ptr(kk), nmonths, spinup, self.n, self.d,
                                                     ptrs(pet_t), ptrs(precip_t), ptrs(tmin_t), byref(flow_desc(flow)),
                                                     _host_ptr(obs), _host_ptr(lo), _host_ptr(hi),
                                                     int(seed) & 0xFFFFFFFFFFFFFFFF, byref(h)))
            self.handle = h.value
            return
        ctx._check(lib().xh_calib_de_create(ctx.handle, self.nb, _host_ptr(nc), None if kk is None else _host_ptr(kk),
                                            nmonths, spinup, self.n, self.d, ptrs(pet_t), ptrs(precip_t), ptrs(tmin_t),
                                            ptrs(area), _host_ptr(obs), _host_ptr(lo), _host_ptr(hi),
                                            int(seed) & 0xFFFFFFFFFFFFFFFF, byref(h)))
        self.handle = h.value

    def init(self):
        self.ctx._check(lib().xh_calib_de_init(self.handle))

    def step(self, ngen=1, tol=0.01, atol=0.0, mutation=(0.5, 1.0), recombination=0.7):
        """Run ``ngen`` generations; returns the number of basins still searching."""
        left = c_int32(0)
        self.ctx._check(lib().xh_calib_de_step(self.handle, int(ngen), float(tol), float(atol), float(mutation[0]),
                                               float(mutation[1]), float(recombination), byref(left)))
        return left.value

    def result(self):
        """(x [nb, d], fun [nb], nfev [nb], nit [nb], active [nb])."""
        x, fun = np.empty((self.nb, self.d)), np.empty(self.nb)
        nfev, nit, act = np.empty(self.nb, dtype=np.int64), np.empty(self.nb, dtype=np.int32), \
            np.empty(self.nb, dtype=np.int32)
        self.ctx._check(lib().xh_calib_de_result(self.handle, _host_ptr(x), _host_ptr(fun), _host_ptr(nfev),
                                                 _host_ptr(nit), _host_ptr(act)))
        return x, fun, nfev, nit, act

    def state(self, which=0):
        """which: 0 population + energies, 1 last trial (unit cube) + energies, 2 last trial scaled + energies."""
        v, e = np.empty((self.nb, self.n, self.d)), np.empty((self.nb, self.n))
        self.ctx._check(lib().xh_calib_de_state(self.handle, int(which), _host_ptr(v), _host_ptr(e)))
        return v, e

    def set_state(self, pop, energies, generation=0):
        pop, energies = as_f64(pop), as_f64(energies)
        if pop.shape != (self.nb, self.n, self.d) or energies.shape != (self.nb, self.n):
            raise ValueError('bad state shape')
        self.ctx._check(lib().xh_calib_de_set_state(self.handle, _host_ptr(pop), _host_ptr(energies), int(generation)))

    def close(self):
        if self.handle is not None and self.ctx.handle is not None:
            lib().xh_calib_de_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- host-only topology helpers (no device needed)
def _topo_args(coords):
    coords = np.asarray(coords)
    ids = np.ascontiguousarray(coords[:, 0], dtype=np.int64)
    ilon = np.ascontiguousarray(coords[:, 3], dtype=np.int32)
    ilat = np.ascontiguousarray(coords[:, 4], dtype=np.int32)
    return ids, ilon, ilat


def _check_host(rc):
    if rc != 0:
        msg = lib().xh_last_error(None)
        raise HipError('libxanthos_hip error {}: {}'.format(rc, msg.decode() if msg else ''))


def mrtm_downstream(coords, flowdir, nrow, ncol):
    ids, ilon, ilat = _topo_args(coords)
    fd = as_f64(flowdir)
    out = np.empty(ids.size, dtype=np.int64)
    _check_host(lib().xh_mrtm_downstream(ids.size, nrow, ncol, _host_ptr(ids), _host_ptr(ilon), _host_ptr(ilat),
                                         _host_ptr(fd), _host_ptr(out)))
    return out


def mrtm_upstream(coords, dsid, nrow, ncol):
    ids, ilon, ilat = _topo_args(coords)
    ds = np.ascontiguousarray(dsid, dtype=np.int64)
    out = np.empty((ids.size, 9), dtype=np.int64)
    _check_host(lib().xh_mrtm_upstream(ids.size, nrow, ncol, _host_ptr(ids), _host_ptr(ilon), _host_ptr(ilat),
                                       _host_ptr(ds), _host_ptr(out)))
    return out


def mrtm_um_csr(upid):
    up = np.ascontiguousarray(upid, dtype=np.int64)
    n = up.shape[0]
    nnz = n + int(up[:, 8].sum())
    indptr = np.empty(n + 1, dtype=np.int64)
    indices = np.empty(nnz, dtype=np.int32)
    sign = np.empty(nnz, dtype=np.int8)
    _check_host(lib().xh_mrtm_um_csr(n, _host_ptr(up), _host_ptr(indptr), _host_ptr(indices), _host_ptr(sign)))
    return indptr, indices, sign


_contexts = {}
_thread = threading.local()


@contextlib.contextmanager
def thread_context(ctx):
    """Inside the block, get_context() of ``ctx``'s device gives ``ctx`` to THIS host thread: a worker thread of the
    ensemble driver runs the writer and the post-processors on a context of its own (a Context is not thread-safe)."""
    before = getattr(_thread, 'ctx', None)
    _thread.ctx = ctx
    try:
        yield ctx
    finally:
        _thread.ctx = before


def get_context(device=0):
    """Process-wide context per device (or the calling thread's own: thread_context)."""
    own = getattr(_thread, 'ctx', None)
    if own is not None and own.handle is not None and own.device == device:
        return own
    ctx = _contexts.get(device)
    if ctx is None or ctx.handle is None:
        ctx = _contexts[device] = Context(device)
    return ctx


def device_count():
    n = c_int(0)
    lib().xh_device_count(byref(n))
    return n.value
