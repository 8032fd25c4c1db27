"""The csv digit generator on the host (xanthos_amd/csrc/xh_dtoa.h: shortest round-trip digits and repr's layout) against
CPython's own repr, restated in tests/csv_np.py.  tests/csv_fuzz is a plain executable around the header, built with
-fsanitize=address,undefined: it reads raw doubles and writes the csv body that the device kernels lay out the same way."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csv_np  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
FUZZ = os.path.join(ROOT, 'tests', 'csv_fuzz')


@pytest.fixture(scope='module')
def program():
    subprocess.run(['make', '-C', FUZZ], check=True, capture_output=True)
    return os.path.join(FUZZ, 'csv_fuzz')


def first_difference(got, want):
    for k, (a, b) in enumerate(zip(got.split(b'\n'), want.split(b'\n'))):
        if a != b:
            for x, y in zip(a.split(b','), b.split(b',')):
                if x != y:
                    return 'line {}: {!r} instead of {!r}'.format(k, x, y)
            return 'line {}: {!r} instead of {!r}'.format(k, a[:80], b[:80])
    return 'lengths {} and {}'.format(len(got), len(want))


def run(program, tmp_path, table, first_id):
    src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.csv')
    csv_np.fuzz_input(src, table, first_id)
    out = subprocess.run([program, src, dst], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    return open(dst, 'rb').read()


def test_oracle_is_the_writers_loop():
    """csv_np.body is the loop of OutWriter.write_data: one repr(float(v)) per value, NaN empty."""
    data = np.array([[1.0, np.nan, -0.0], [1e16, 5e-324, np.inf]])
    assert csv_np.body(data, 9) == b'9,1.0,,-0.0\n10,1e+16,5e-324,inf\n'
    assert list(csv_np.row_offsets(data, 9)) == [0, 12, 32]
    assert max(len(csv_np.field(v)) for v in csv_np.hand_list()) == 24


@pytest.mark.parametrize('ncols,first_id', [(1, 0), (7, 99995), (600, 1)])
def test_hand_list(program, tmp_path, ncols, first_id):
    """Specials, subnormals, both sides of every layout switch, every power of two and of ten with its neighbours,
    integers up to 2^53."""
    table = csv_np.as_table(csv_np.hand_list(), ncols)
    got, want = run(program, tmp_path, table, first_id), csv_np.body(table, first_id)
    assert got == want, first_difference(got, want)


def test_random_bit_patterns(program, tmp_path):
    """200,000 uniformly random 64-bit patterns: every binary exponent, NaN payloads and infinities among them."""
    table = csv_np.as_table(csv_np.random_bits(200000, 20240607), 64)
    got, want = run(program, tmp_path, table, 1), csv_np.body(table, 1)
    assert got == want, first_difference(got, want)
