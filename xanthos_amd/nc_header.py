"""Where a variable's values lie in a NetCDF-classic file (host only): the mirror of ``data_writer/formats.nc_header``.

A classic file (CDF-1, or CDF-2 with 64-bit offsets) is a header -- magic, number of records, the dimensions, the global
attributes, the variables with their dimensions, attributes, type, size and the offset ``begin`` of their first byte --
followed by the data.  A variable without the record dimension is ONE contiguous block of big-endian values from
``begin`` on, row-major.  ``variable_range`` reads the header and says where that block is, so that the loader can map it
(``np.memmap``) and the pipeline can send its bytes to the GPU as they are stored (``xh_widen`` makes doubles of them in
HBM) instead of scipy reading the file, numpy swapping every value and widening it on the host.

Only what the loader can use comes back: a ``float`` or ``double`` variable that is not a record variable.  Everything else
-- another type, a record variable, a missing name, another file format, a header this parser does not fully understand --
is ``None``, and the loader then reads the file through scipy as before.
"""
import os
import struct

import numpy as np

_NC_DIMENSION, _NC_VARIABLE, _NC_ATTRIBUTE = 10, 11, 12
# nc_type -> bytes per value (byte, char, short, int, float, double)
_TYPE_BYTES = {1: 1, 2: 1, 3: 2, 4: 4, 5: 4, 6: 8}
_NC_FLOAT, _NC_DOUBLE = 5, 6
_DTYPES = {_NC_FLOAT: np.dtype('>f4'), _NC_DOUBLE: np.dtype('>f8')}
_MAX_HEADER = 64 << 20       # a header longer than this is not one of ours to understand


class _NotUnderstood(Exception):
    pass


class _Reader:
    """Big-endian fields of the header, read from the file as they are asked for."""

    def __init__(self, fh):
        self.fh, self.pos = fh, 0

    def take(self, n):
        if n < 0 or self.pos + n > _MAX_HEADER:
            raise _NotUnderstood()
        b = self.fh.read(n)
        if len(b) != n:
            raise _NotUnderstood()        # the header ends before it is complete
        self.pos += n
        return b

    def int32(self):
        return struct.unpack('>i', self.take(4))[0]

    def int64(self):
        return struct.unpack('>q', self.take(8))[0]

    def count(self):
        n = self.int32()
        if n < 0:
            raise _NotUnderstood()
        return n

    def name(self):
        n = self.count()
        b = self.take(n)
        self.take(-n % 4)
        return b.decode('latin1')

    def list_header(self, tag):
        """Number of entries of a dim / att / var list: ``tag`` and a count, or ABSENT (two zeros)."""
        t, n = self.int32(), self.count()
        if t == 0 and n == 0:
            return 0
        if t != tag:
            raise _NotUnderstood()
        return n

    def skip_attributes(self):
        for _ in range(self.list_header(_NC_ATTRIBUTE)):
            self.name()
            nc_type, n = self.int32(), self.count()
            if nc_type not in _TYPE_BYTES:
                raise _NotUnderstood()
            nbytes = n * _TYPE_BYTES[nc_type]
            self.take(nbytes + (-nbytes % 4))


def _parse(fh, key, file_bytes):
    r = _Reader(fh)
    magic = r.take(4)
    if magic[:3] != b'CDF' or magic[3] not in (1, 2):
        return None                      # not NetCDF classic (CDF-5, HDF5 / NetCDF-4, anything else)
    wide = magic[3] == 2
    r.int32()                            # numrecs (or the streaming mark): only record variables need it
    dims = []
    for _ in range(r.list_header(_NC_DIMENSION)):
        r.name()
        dims.append(r.count())
    r.skip_attributes()
    found = None
    for _ in range(r.list_header(_NC_VARIABLE)):
        name = r.name()
        dimids = [r.int32() for _ in range(r.count())]
        r.skip_attributes()
        nc_type = r.int32()
        r.int32()                        # vsize: redundant for a non-record variable (and capped at 2^32 - 4 in CDF-2)
        begin = r.int64() if wide else r.int32()
        if nc_type not in _TYPE_BYTES or any(d < 0 or d >= len(dims) for d in dimids):
            raise _NotUnderstood()
        if name == key and found is None:
            found = (nc_type, dimids, begin)
    if found is None:
        return None
    nc_type, dimids, begin = found
    shape = tuple(dims[d] for d in dimids)
    # the record dimension has length 0 in the header; a scalar has nothing to map
    if nc_type not in _DTYPES or not shape or any(n == 0 for n in shape):
        return None
    dtype = _DTYPES[nc_type]
    nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    if begin < r.pos or begin + nbytes > file_bytes:
        return None                      # the block is not where a complete file has it
    return dtype, shape, begin


def variable_range(path, key):
    """(numpy dtype '>f4' or '>f8', shape, byte offset) of the values of variable ``key`` in the NetCDF-classic file
    ``path`` -- ``np.memmap(path, dtype, 'r', offset, shape)`` is the variable -- or None (see the module's text)."""
    if not isinstance(key, str):
        return None
    try:
        with open(path, 'rb') as fh:
            return _parse(fh, key, os.fstat(fh.fileno()).st_size)
    except (_NotUnderstood, OSError, struct.error, UnicodeError):
        return None
