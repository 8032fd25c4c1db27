"""The per-basin channel-velocity scale: its bounds, its csv file and its use on the velocity array.

A calibration with ``calibrate_velocity = 1`` finds, beside the ABCD parameters, one dimensionless scale v > 0 per basin
that multiplies the channel velocity of the basin's own cells.  ``velocity_scale.csv`` carries the scales from the
calibration to a forward run (``[[mrtm]] velocity_scale``): a header ``basin_id,scale`` and one row per basin; a basin
that is not listed has scale 1.  The loader multiplies ``str_velocity`` of every cell by its basin's scale right after
reading it, so everything downstream -- routing plans, calibration tables, the hydropower post-processors -- sees the
scaled array.

Pure numpy; nothing here touches the device.
"""
import os

import numpy as np

from ..ini_reader import ValidationException

DEFAULT_BOUNDS = (0.25, 4.0)          # a choice, not a measurement


def check_bounds(bounds, key='velocity_scale_bounds'):
    """(lo, hi) as floats; refused unless 0 < lo < hi, both finite."""
    try:
        lo, hi = (float(x) for x in bounds)
    except (TypeError, ValueError):
        raise ValidationException('{} = {!r} must be two numbers lo, hi.'.format(key, bounds))
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo < hi):
        raise ValidationException('{} = {!r}, {!r} must be finite with 0 < lo < hi.'.format(key, lo, hi))
    return lo, hi


def check_scales(scales, key='velocity_scale'):
    s = np.asarray(scales, dtype=np.float64)
    bad = ~(np.isfinite(s) & (s > 0))
    if bad.any():
        raise ValidationException('{}: the scale of basin {} must be positive and finite, not {!r}.'.format(
            key, int(np.argmax(bad)) + 1, float(s[np.argmax(bad)])))
    return s


def read_velocity_scale(path, n_basins, key='velocity_scale'):
    """scales [n_basins] of ``path`` (header basin_id,scale; basins not listed get 1).  Refused: a basin id outside
    1..n_basins, a duplicate id, a scale that is not positive and finite."""
    try:
        with open(path) as fh:
            lines = [ln.strip() for ln in fh.read().splitlines()]
    except OSError as exc:
        raise ValidationException('{}: cannot read {}: {}'.format(key, path, exc))
    rows = [ln for ln in lines if ln and not ln.startswith('#')]
    if rows and not rows[0][0].isdigit():
        rows = rows[1:]                                          # the header
    scales = np.ones(int(n_basins))
    seen = set()
    for ln in rows:
        parts = [p.strip() for p in ln.split(',')]
        try:
            if len(parts) != 2:
                raise ValueError('two columns expected')
            b_f, v = float(parts[0]), float(parts[1])
            b = int(b_f)
            if b != b_f:
                raise ValueError('basin_id is not an integer')
        except ValueError as exc:
            raise ValidationException('{}: {}: row {!r}: {}'.format(key, path, ln, exc))
        if not 1 <= b <= n_basins:
            raise ValidationException('{}: {}: basin_id {} lies outside 1..{}.'.format(key, path, b, int(n_basins)))
        if b in seen:
            raise ValidationException('{}: {}: duplicate basin_id {}.'.format(key, path, b))
        if not (np.isfinite(v) and v > 0):
            raise ValidationException('{}: {}: the scale of basin {} must be positive and finite, not {!r}.'.format(
                key, path, b, v))
        seen.add(b)
        scales[b - 1] = v
    return scales


def write_velocity_scale(path, scales):
    """``path`` with one row for every basin 1..len(scales); repr() keeps every bit of a scale."""
    scales = check_scales(scales)
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'w') as fh:
        fh.write('basin_id,scale\n')
        for b, v in enumerate(scales, start=1):
            fh.write('{},{!r}\n'.format(b, float(v)))


def cell_scales(basin_ids, scales):
    """[ncell] scale of every cell's basin (1 for a cell whose basin id lies outside 1..len(scales))."""
    bid = np.asarray(basin_ids).astype(np.int64).reshape(-1)
    scales = np.asarray(scales, dtype=np.float64)
    out = np.ones(bid.size)
    ok = (bid >= 1) & (bid <= scales.size)
    out[ok] = scales[bid[ok] - 1]
    return out


def apply_velocity_scale(str_velocity, basin_ids, scales):
    """ChV of every cell times the scale of its basin (one IEEE product per cell)."""
    return np.asarray(str_velocity, dtype=np.float64) * cell_scales(basin_ids, scales)


def combined_scales(loaded, basins, calibrated, n_basins):
    """What a calibration writes on a tree that already carried scales: loaded [n_basins] (None = ones) times the
    calibrated v for ``basins`` (1-based), the loaded value for every other basin -- the next run's input as it stands."""
    out = np.ones(int(n_basins)) if loaded is None else np.array(loaded, dtype=np.float64, copy=True)
    if out.shape != (int(n_basins),):
        raise ValueError('loaded scales must be [n_basins]')
    for b, v in zip(basins, calibrated):
        out[int(b) - 1] = out[int(b) - 1] * float(v)
    return out
