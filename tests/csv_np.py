"""The csv text of the writer as the host formulates it: CPython's own repr, one value at a time -- the loop of
xanthos_amd/data_writer/out_writer.py (write_data, csv branch), restated as the oracle of the device formatter."""
import struct

import numpy as np


def field(v):
    v = float(v)
    return '' if v != v else repr(v)                    # pandas writes NaN as an empty field


def body(data, first_id=1):
    """The lines below the header: str(id) + ',' + ','.join(fields) + newline per row, as bytes."""
    data = np.asarray(data, dtype=np.float64)
    out = []
    for k, row in enumerate(data.tolist()):
        out.append(str(first_id + k) + ',' + ','.join('' if v != v else repr(v) for v in row) + '\n')
    return ''.join(out).encode()


def row_offsets(data, first_id=1):
    """int64 [nrows + 1]: where each line of body() starts, and the length of the whole."""
    data = np.asarray(data, dtype=np.float64)
    lens = [len(str(first_id + k)) + 1 + sum(len('' if v != v else repr(v)) for v in row) + len(row)
            for k, row in enumerate(data.tolist())]
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)


def header(col_names, ncols, names=False):
    return ('id,' + ('name,' if names else '') + ','.join(col_names[:ncols]) + '\n').encode()


def file_bytes(data, col_names, first_id=1):
    data = np.asarray(data, dtype=np.float64)
    return header(col_names, data.shape[1]) + body(data, first_id)


def from_bits(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def hand_list():
    """The values at which a shortest-digits generator and the layout can go wrong."""
    inf, nan = float('inf'), float('nan')
    v = [0.0, -0.0, inf, -inf, nan,
         5e-324, from_bits([0x000FFFFFFFFFFFFF])[0], 2.2250738585072014e-308, 1.7976931348623157e308,
         9999999999999998.0, 1e16, 0.0001, 0.00009999999999999999, 1e15, 123456789012345680.0,
         0.1 + 0.2, 1 / 3, 9007199254740992.0, 9007199254740991.0, 9007199254740994.0,
         1.0, 1000000000000000.0, 1e-05, 1e22, 1e23, 9.5e-322, -1.2345678901234567e-308, -2.5, 100.0, 1e100]
    v += [2.0 ** e for e in range(-1074, 1024)]         # the rounding interval is asymmetric at a power of two
    for e in range(-323, 309):
        p = float('1e{}'.format(e))
        v += [np.nextafter(p, -inf), p, np.nextafter(p, inf)]
    v += [float(i) for i in range(0, 1200)] + [float(2 ** k + d) for k in range(10, 54) for d in (-1, 0, 1) if 2 ** k + d <= 2 ** 53]
    v += [float(10 ** k + d) for k in range(1, 16) for d in (-1, 1)]
    a = np.asarray(v, dtype=np.float64)
    return np.concatenate([a, -a[5:60]])


def random_bits(n, seed):
    rng = np.random.default_rng(seed)
    return from_bits(rng.integers(0, 2 ** 64, size=n, dtype=np.uint64))


def as_table(values, ncols, fill=np.nan):
    """1-d values -> [nrows, ncols], the last row padded with ``fill``."""
    values = np.asarray(values, dtype=np.float64)
    nrows = -(-values.size // ncols)
    out = np.full(nrows * ncols, fill, dtype=np.float64)
    out[:values.size] = values
    return out.reshape(nrows, ncols)


def fuzz_input(path, data, first_id):
    """The input file of tests/csv_fuzz: int64 ncols, int64 first_id, the raw doubles."""
    data = np.ascontiguousarray(data, dtype=np.float64)
    with open(path, 'wb') as fh:
        fh.write(struct.pack('=qq', data.shape[1], first_id))
        fh.write(data.tobytes())
