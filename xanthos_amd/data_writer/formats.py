"""File layouts of OutputFormat 0 (NetCDF) and 2 (MATLAB): the bytes in front of a body that is formed in HBM.

The reference writes both through scipy (xanthos/data_writer/out_writer.py:179-181 ``spio.savemat(filename, {var: data})``,
:196-223 ``spio.netcdf.netcdf_file``).  Either file is a short header that depends on the shape and a few names only,
followed by the array's values in one piece:

* NetCDF classic (CDF-1): ``nc_header`` + the values as big-endian binary32, row-major (``a.astype('>f4').tobytes()``);
* MAT-5, uncompressed: ``mat_header`` + the values as little-endian binary64, column-major (``a.tobytes(order='F')``).

The headers are pure functions (tests/test_outfmt_host.py compares them with files the reference wrote); the bodies are
made by ``Context.save_nc_many`` / ``save_mat_many`` (xh_pack_f32_be / xh_transpose).  The small tables with a ``name``
column are object (cell) arrays under MAT and go through ``scipy.io.savemat`` on the host.
"""
import os
import struct
import time

from ..ini_reader import ValidationException

NC_LIMIT = 1 << 31           # CDF-1 keeps a variable's size and offset in signed 32 bits
MAT_LIMIT = 1 << 32          # MAT-5 keeps an element's byte count in unsigned 32 bits
MAT_TEXT_BYTES = 116         # the descriptive text in front of a MAT-5 file: the only bytes that differ between two runs

_NC_DIMENSION, _NC_VARIABLE, _NC_ATTRIBUTE, _NC_CHAR, _NC_FLOAT = 10, 11, 12, 2, 5
_MI_INT8, _MI_INT32, _MI_UINT32, _MI_DOUBLE, _MI_MATRIX, _MX_DOUBLE_CLASS = 1, 5, 6, 9, 14, 6


def _nc_int(v):
    return struct.pack('>i', v)


def _nc_string(s):
    b = s.encode('latin1')
    return _nc_int(len(b)) + b + b'\x00' * (-len(b) % 4)


def _nc_text_attribute(name, value):
    b = value.encode('ascii')
    return _nc_string(name) + _nc_int(_NC_CHAR) + _nc_int(len(b)) + b + b'\x00' * (-len(b) % 4)


def nc_header(nrows, ncols, in_year, unit_str, var):
    """The bytes scipy's netcdf_file writes in front of the data for the reference's ``save_netcdf(filename, array, var)``
    of a [nrows, ncols] array: version 1, no record dimension, dimensions ``index`` and ``year`` / ``month``, one variable
    ``data`` of type f4 over them with the attributes ``units = unit_str`` and ``description = var + '_' + unit_str`` (for
    avgchflow too, whose file NAME says m3persec: out_writer.py:215-217), its size and the offset of its first byte."""
    nrows, ncols = int(nrows), int(ncols)
    vsize = nrows * ncols * 4                                  # a multiple of 4 already: no padding behind the data
    if vsize >= NC_LIMIT:
        raise ValidationException(
            "OutputFormat 0 (NetCDF classic) cannot hold variable '{}': {} x {} values are {} bytes, the format's limit is "
            '2 GiB per variable; use OutputInYear = 1, or OutputFormat 4 (npy)'.format(var, nrows, ncols, vsize))
    head = b'CDF\x01' + _nc_int(0)                             # no records
    head += _nc_int(_NC_DIMENSION) + _nc_int(2)
    head += _nc_string('index') + _nc_int(nrows) + _nc_string('year' if in_year else 'month') + _nc_int(ncols)
    head += _nc_int(0) * 2                                     # no global attributes
    head += _nc_int(_NC_VARIABLE) + _nc_int(1)
    head += _nc_string('data') + _nc_int(2) + _nc_int(0) + _nc_int(1)
    head += _nc_int(_NC_ATTRIBUTE) + _nc_int(2)
    head += _nc_text_attribute('units', unit_str) + _nc_text_attribute('description', var + '_' + unit_str)
    head += _nc_int(_NC_FLOAT) + _nc_int(vsize)
    return head + _nc_int(len(head) + 4)                       # begin: the data follow this field


def mat_text(now=None):
    """Bytes 0 .. 115 of a MAT-5 file as scipy writes them: the descriptive text, NUL-padded."""
    text = 'MATLAB 5.0 MAT-file Platform: {}, Created on: {}'.format(os.name, time.asctime() if now is None else now)
    return text.encode('latin1')[:MAT_TEXT_BYTES].ljust(MAT_TEXT_BYTES, b'\x00')


def _mat_element(mdtype, payload):
    """A data element: the small form (tag and data in 8 bytes) up to 4 bytes of data, tag + data padded to 8 otherwise."""
    if len(payload) <= 4:
        return struct.pack('<I', (len(payload) << 16) + mdtype) + payload.ljust(4, b'\x00')
    return struct.pack('<II', mdtype, len(payload)) + payload + b'\x00' * (-len(payload) % 8)


def mat_header(var, nrows, ncols, now=None):
    """The bytes ``scipy.io.savemat(filename, {var: array})`` writes in front of the real part of a [nrows, ncols] float64
    array: the 128-byte file header (text, subsystem offset, version 0x0100, endian mark 'IM'), the miMATRIX tag, the
    array flags (double class), the dimensions, the name and the miDOUBLE tag.  Little-endian, no compression."""
    nrows, ncols = int(nrows), int(ncols)
    body = nrows * ncols * 8
    name = var.encode('latin1')
    inner = struct.pack('<IIII', _MI_UINT32, 8, _MX_DOUBLE_CLASS, 0)
    inner += _mat_element(_MI_INT32, struct.pack('<ii', nrows, ncols))
    inner += _mat_element(_MI_INT8, name)
    total = len(inner) + 8 + body                              # ... and the miDOUBLE tag
    if total >= MAT_LIMIT:
        raise ValidationException(
            "OutputFormat 2 (MATLAB 5) cannot hold variable '{}': {} x {} values are {} bytes, the format's limit is "
            '4 GiB per variable; use OutputInYear = 1, or OutputFormat 4 (npy)'.format(var, nrows, ncols, body))
    inner += struct.pack('<II', _MI_DOUBLE, body) if body else _mat_element(_MI_DOUBLE, b'')      # (no cells: all in the tag)
    head = mat_text(now) + b'\x00' * 8 + struct.pack('<H', 0x0100) + b'IM'
    return head + struct.pack('<II', _MI_MATRIX, total) + inner


def save_mat_table(filename, var, data, names):
    """A table with names under MAT: the reference's DataFrame has the columns ``name`` and one per time step, which
    ``savemat`` writes as an object (cell) array [n_ids, 1 + t] of strings and doubles (the ``id`` index is not written).
    A few hundred rows: written on the host."""
    import numpy as np
    from scipy import io as spio
    cells = np.empty((data.shape[0], 1 + data.shape[1]), dtype=object)
    cells[:, 0] = [str(n) for n in names]
    cells[:, 1:] = np.asarray(data, dtype=np.float64)
    spio.savemat(filename, {var: cells})
