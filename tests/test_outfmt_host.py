"""OutputFormat 0 (NetCDF) and 2 (MATLAB) without a GPU: the file layouts of data_writer/formats.py against files the
reference wrote (tests/golden/outfmt.npz, made by tests/golden/make_golden_outfmt.py), the numpy restatement of the two
bodies that tests/test_gpu_outfmt.py holds the device to, the table with names, and the refusals."""
import io
import re
from types import SimpleNamespace

import numpy as np
import pytest

from xanthos_amd.data_writer import formats
from xanthos_amd.ini_reader import ValidationException

VARS = ('q', 'avgchflow', 'soilmoisture')
CASES = {'m0': (0, 0), 'y1': (1, 1)}                 # (OutputInYear, OutputUnit)
ALL = [(c, v) for c in CASES for v in VARS]


def unit_str(case):
    in_year, unit = CASES[case]
    return '{}per{}'.format(('mm', 'km3')[unit], ('month', 'year')[in_year])


def settings(folder, fmt, case='m0', **extra):
    in_year, unit = CASES[case]
    return SimpleNamespace(output_vars=list(VARS), ProjectName='golden', OutputFolder=str(folder), OutputFormat=fmt,
                           OutputUnit=unit, OutputInYear=in_year, StartYear=2000, EndYear=2001, device=0, **extra)


@pytest.fixture(scope='module')
def fix(golden):
    return golden('outfmt')


def test_fixture_holds_the_deciding_values(fix):
    """The values that decide a float64 -> float32 narrowing reach the files of both cases, in both signs."""
    want = [np.nan, 0.0, 1e-40, 1e-45, 7e-46, 1e39, 3.4028235677973366e38, 3.4028234e38, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24]
    for case, var in ALL:
        bits = set(fix['{}_{}_written'.format(case, var)].view(np.uint64).ravel().tolist())
        for v in want:
            if v != v and case == 'y1' and var != 'avgchflow':              # (a yearly sum skips NaN; the mean of avgchflow keeps it)
                continue
            for s in ((v, -v) if case == 'm0' and v != 0.0 else (v,)):       # (a yearly sum of -0.0 and NaNs is +0.0)
                assert int(np.float64(s).view(np.uint64)) in bits, (case, var, s)


@pytest.mark.parametrize('case,var', ALL)
def test_nc_header_equals_the_reference_file(fix, case, var):
    written, ref = fix['{}_{}_written'.format(case, var)], fix['{}_{}_nc'.format(case, var)].tobytes()
    head = formats.nc_header(written.shape[0], written.shape[1], CASES[case][0], unit_str(case), var)
    assert head == ref[:len(head)]
    assert len(ref) == len(head) + written.size * 4
    assert head.startswith(b'CDF\x01') and int.from_bytes(head[-4:], 'big') == len(head)
    # the quirk of out_writer.py:215-217: avgchflow's attributes carry OutputUnitStr, its file name m3persec
    assert (var + '_' + unit_str(case)).encode() in head and b'm3persec' not in head
    assert ('m3persec' in str(fix['{}_{}_file'.format(case, var)])) == (var == 'avgchflow')


@pytest.mark.parametrize('case,var', ALL)
def test_mat_header_equals_the_reference_file(fix, case, var):
    written, ref = fix['{}_{}_written'.format(case, var)], fix['{}_{}_mat'.format(case, var)].tobytes()
    head = formats.mat_header(var, written.shape[0], written.shape[1])
    assert head[formats.MAT_TEXT_BYTES:] == ref[formats.MAT_TEXT_BYTES:len(head)]
    assert len(ref) == len(head) + written.size * 8
    pattern = rb'MATLAB 5\.0 MAT-file Platform: posix, Created on: \w{3} \w{3} [ \d]\d \d\d:\d\d:\d\d \d{4}\x00+'
    assert re.fullmatch(pattern, head[:formats.MAT_TEXT_BYTES]) and re.fullmatch(pattern, ref[:formats.MAT_TEXT_BYTES])
    assert len(head) == (184 if len(var) <= 4 else 200)          # the name as a small element / an ordinary padded one


@pytest.mark.parametrize('case,var', ALL)
def test_bodies_are_the_numpy_restatement(fix, case, var):
    """NetCDF: astype('>f4') row-major; MATLAB: the doubles column-major -- what the GPU tests compare the device with."""
    written = fix['{}_{}_written'.format(case, var)]
    nc, mat = fix['{}_{}_nc'.format(case, var)].tobytes(), fix['{}_{}_mat'.format(case, var)].tobytes()
    with np.errstate(over='ignore'):
        assert nc[len(nc) - written.size * 4:] == written.astype('>f4').tobytes()
    assert mat[len(mat) - written.size * 8:] == written.tobytes(order='F')


def test_narrowing_rules_of_the_restatement():
    """What xh_pack_f32_be promises, stated on numpy's astype('>f4'): overflow to inf from the midpoint on, binary32
    subnormals kept, ties to even, signed zero, the canonical NaN."""
    src = np.array([np.nan, -0.0, 1e-40, 1e-45, 7e-46, 1e39, 3.4028235677973366e38, 3.4028234e38, 1 + 2.0 ** -24,
                    1 + 3 * 2.0 ** -24])
    with np.errstate(over='ignore'):
        got = np.frombuffer(src.astype('>f4').tobytes(), dtype='>u4').tolist()
    assert got == [0x7fc00000, 0x80000000, 71362, 1, 0, 0x7f800000, 0x7f800000, 0x7f7fffff, 0x3f800000, 0x3f800002]


def test_name_table_loads_to_the_reference_cells(fix, tmp_path):
    from scipy import io as spio
    path = str(tmp_path / 'basin.mat')
    formats.save_mat_table(path, 'Basin_runoff', fix['basin_values'], fix['basin_names'])
    got = spio.loadmat(path)['Basin_runoff']
    ref = spio.loadmat(io.BytesIO(fix['basin_mat'].tobytes()))['Basin_runoff']
    assert got.shape == ref.shape == (3, 25) and got.dtype == ref.dtype == object
    for g, r in zip(got.ravel(), ref.ravel()):
        assert g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes()
    assert [str(c[0]) for c in got[:, 0]] == [str(n) for n in fix['basin_names']]
    assert np.isnan(np.array([c[0, 0] for c in got[2, 1:]])).all()          # the name without cells


def test_format_limits_are_refused_by_name():
    assert formats.nc_header(2 ** 20, 2 ** 9 - 1, 0, 'mmpermonth', 'q')       # 4 bytes x (2**29 - 2**20): below 2 GiB
    with pytest.raises(ValidationException, match=r"NetCDF.*'soilmoisture'"):
        formats.nc_header(2 ** 20, 2 ** 9, 0, 'mmpermonth', 'soilmoisture')
    assert formats.mat_header('q', 2 ** 20, 2 ** 9 - 1)
    with pytest.raises(ValidationException, match=r"MATLAB.*'avgchflow'"):
        formats.mat_header('avgchflow', 2 ** 20, 2 ** 9)
    with pytest.raises(ValidationException, match=r"MATLAB.*'q'"):
        formats.mat_header('q', 2 ** 29 - 6, 1)                               # the matrix element with its 56 bytes of tags


def test_netcdf_with_aggregates_is_refused_at_construction(tmp_path):
    from xanthos_amd.data_writer import out_writer
    for key in ('AggregateRunoffBasin', 'AggregateRunoffCountry', 'AggregateRunoffGCAMRegion'):
        with pytest.raises(ValidationException, match=key):
            out_writer.OutWriter(settings(tmp_path, out_writer.FORMAT_NETCDF, **{key: 1}), np.ones(3), {})


def test_parquet_stays_refused_and_says_so(tmp_path):
    from xanthos_amd.data_writer import out_writer
    w = out_writer.OutWriter.__new__(out_writer.OutWriter)
    w.out_folder, w.out_format = str(tmp_path), out_writer.FORMAT_PARQUET
    with pytest.raises(RuntimeError, match='parquet') as err:
        w.write_data(str(tmp_path / 'q'), 'q', np.zeros((2, 2)), ['200001', '200002'])
    assert 'NetCDF /' not in str(err.value) and 'MATLAB /' not in str(err.value)
