"""Host tests (no GPU) of the flow-control rule of the dataflow routing kernels: xanthos_amd/csrc/xh_mrtm_flowctl.h decides what a
unit needs of its two stream counters for the next CH = 256 sub-steps and whether it has to look at a counter at all
(check() of xh_mrtm_wave_unit.h).  The header is plain integer code; tests/flowctl_probe builds it into a stand-alone program
under AddressSanitizer + UndefinedBehaviorSanitizer, which this file runs as a child process.

1. The header's expressions against the ones check() spelled out before: every n that is a multiple of 256 up to 8,192, lmax in
   {0, 2, 48}, rings of 512 and 4,096, import lags {0, 16, 48}, short and long series; the look rule against the condition
   under which the kernel's wait polled.
2. A model of chains of 2-5 units with random integer service times and rings of 2-16 check intervals: every unit publishes at
   every check and looks only by the header's rule; a look returns a value any number of publications old.  No consumer passes
   what its producer published, no producer overwrites what its consumer has not marked done, every chain finishes: 10,000
   seeded chains.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, 'tests', 'flowctl_probe')


def run_probe(*args):
    subprocess.run(['make', '-C', PROBE], check=True, capture_output=True)
    r = subprocess.run([os.path.join(PROBE, 'flowctl_probe')] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    return r


def test_expressions_agree_with_the_ones_check_spelled_out():
    r = run_probe('expr')
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.startswith('expr ok'), r.stdout


def test_ten_thousand_chains_stay_safe_and_finish():
    r = run_probe('chains', 10000, 4242)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.startswith('chains ok: 10000 chains'), r.stdout
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr
