"""Host test (no GPU) of the month records the time-skewed routing kernels read (xanthos_amd/csrc/xh_mrtm_rec.h).

wave_fill_records is host code without any HIP in it; tests/rec_probe builds it into a stand-alone program under
-fsanitize=address,undefined, with record buffers of exactly the sizes the launch code allocates, and prints every record.
Checked here: the factors the reassociated kernel multiplies by instead of dividing -- 1 / nt (mrtm.py:80) against 1.0 / x and
1000 dt / seconds (mrtm.py:45, times dt) against the same expression in numpy, both to the bit, for every month length at
dt = 3 h and at dt = 4.8 h -- and the fields the lanes' next crossing is taken from (sub-steps of the iteration, first
sub-step of the next one), the look-ahead of two months, the write flag behind a spin-up and the records past the end.
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
PROBE = os.path.join(ROOT, 'tests', 'rec_probe')


def _records(dt, wr_from, days):
    subprocess.run(['make', '-C', PROBE], check=True, capture_output=True)
    r = subprocess.run([os.path.join(PROBE, 'rec_probe'), repr(float(dt)), str(wr_from)] + [str(d) for d in days],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout[-1000:] + r.stderr[-3000:]      # (a sanitizer report goes to stderr)
    rec, fin = [], []
    for line in r.stdout.splitlines():
        w = line.split()
        d = {k: (float.fromhex(x) if x.startswith(('0x', '-0x')) else int(x)) for k, x in zip(w[2::2], w[3::2])}
        (rec if w[0] == 'rec' else fin).append(d)
    return rec, fin


@pytest.mark.parametrize('dt', [10800.0, 17280.0])
def test_reciprocals_and_crossing_fields(dt):
    days = [31, 28, 29, 30, 31, 31, 30, 28, 31, 29, 30]      # every month length, next to every other
    spin = 3
    sched = days[:spin] + days
    nit = len(sched)
    rec, fin = _records(dt, spin, sched)
    assert len(rec) == nit + 3 and len(fin) == nit + 2
    nt = [int(d * 86400.0 / dt) for d in sched]
    g = np.concatenate([[0], np.cumsum(nt)])
    assert {28, 29, 30, 31} == set(sched) and len(set(nt)) == 4
    for it in range(nit + 1):
        f = fin[it]
        nt_prev = nt[it - 1] if it >= 1 else 1
        assert f['nt_prev'] == nt_prev
        assert f['inv_nt_prev'] == 1.0 / np.float64(nt_prev)                                    # to the bit
        secs_next1 = sched[it + 1] * 86400.0 if it + 1 < nit else 1.0
        assert f['secs_next1'] == secs_next1
        assert f['erl_scale_next1'] == np.float64(1000.0) * np.float64(dt) / np.float64(secs_next1)      # to the bit
        assert f['nt_cur'] == (nt[it] if it < nit else 0)
        assert f['g_next1'] == (g[it + 1] if it + 1 <= nit else g[nit])
        m_next2 = (it + 2 - spin if it + 2 >= spin else it + 2) if it + 2 < nit else 0
        assert f['m_next2'] == m_next2 and f['q_off_next2'] == 8 * m_next2
        if it >= 1:
            assert f['m_prev'] == rec[it - 1]['m'] and f['write_prev'] == (1 if it - 1 >= spin else 0)
    for it in range(nit):
        assert rec[it]['nt'] == nt[it] and rec[it]['g'] == g[it] and rec[it]['secs'] == sched[it] * 86400.0
        assert rec[it]['write'] == (1 if it >= spin else 0)
    assert rec[nit]['g'] == g[nit] and rec[nit]['nt'] == 0
    # the record one past the last bookkeeping: neutral factors, never a division by zero
    assert fin[nit + 1]['nt_prev'] == 1 and fin[nit + 1]['inv_nt_prev'] == 1.0 and fin[nit + 1]['secs_next1'] == 1.0
    assert fin[nit + 1]['erl_scale_next1'] == 1000.0 * dt


def test_shortest_series():
    """One month, no spin-up: the records the month bookkeeping of a one-month call reads (iterations 0, 1 and the one past)."""
    rec, fin = _records(10800.0, 0, [31])
    assert len(rec) == 4 and len(fin) == 3
    assert fin[0]['nt_cur'] == 248 and fin[0]['g_next1'] == 248 and fin[0]['m_next2'] == 0
    assert fin[1]['nt_prev'] == 248 and fin[1]['inv_nt_prev'] == 1.0 / 248 and fin[1]['write_prev'] == 1 and fin[1]['g_next1'] == 248
