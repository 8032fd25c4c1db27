"""SPEI in HBM (``xh_std_index2``, log-logistic, precipitation minus PET subtracted inside the kernel) against the path it
replaces, at full size (67,420 cells x 600 months, reference period: the whole series).

    python tools/bench_spei.py [--cells 67420] [--months 600] [--reps 7] [--no-host]      # writes the JSON and README

For the scales (1) and (1, 3, 12), on a seeded seasonal gamma precipitation field with 2 % zeros and a seasonal PET:
(a) ``xh_std_index2`` on the two arrays in HBM, all scales in one call, the fit written out as the product does: the library's
    ``std_index`` timer per call (minimum / median / maximum over the repetitions after a warm-up), the algorithmic HBM
    traffic (16 B in once, 8 B out per scale and cell-month), and the LDS reads of the ranking (n per element of the
    reference period and scale) beside the transcendental evaluations (one log, one exp, one ndtri per cell-month and
    scale): where the time goes;
(b) the same call with the tables of (a) handed back in (``par_in``): no ranking, no fit -- the difference to (a) is what the
    sort and the sums cost;
(c) the path it replaces, in the same process: both arrays downloaded (host clock), subtracted, then numpy per scale -- the
    definitions of DESIGN 4.19 vectorised over the cells (np.sort along the sample, the three sums as matrix-vector
    products).  (tests/spei_np.py states the same per cell and calendar month with the sums in the definition's order; at
    this size its Python loops would take hours.)  The two are compared on a sample of cells.
It records, it does not gate.  Results: profiles/spei/bench_spei.json and the table in profiles/spei/README.md (the README's
other sections are kept: the tool rewrites only the part between its two markers)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from xanthos_amd import _hip      # noqa: E402

SCALE_SETS = ((1,), (1, 3, 12))
CLIP = 3.09
BEGIN, END = '<!-- bench_spei: begin -->', '<!-- bench_spei: end -->'


def make_fields(ncell, nmonths, seed=5):
    rng = np.random.default_rng(seed)
    shape = rng.uniform(0.6, 8.0, (ncell, 1)).astype(np.float32)
    mon = np.arange(nmonths) % 12
    season = 1.0 + 0.6 * np.sin(2 * np.pi * mon / 12.0 + rng.uniform(0, 6.28, (ncell, 1)))
    p = rng.standard_gamma(shape, (ncell, nmonths)) * (30.0 / shape) * season
    p[rng.random((ncell, nmonths)) < 0.02] = 0.0
    pet = 28.0 * (1.0 + 0.5 * np.sin(2 * np.pi * mon / 12.0 + 1.0)) * rng.uniform(0.7, 1.3, (ncell, 1))
    return np.ascontiguousarray(p, dtype=np.float64), np.ascontiguousarray(np.broadcast_to(pet, p.shape), dtype=np.float64)


def accumulate(x, k):
    X = np.full(x.shape, np.nan)
    n = x.shape[1]
    acc = x[:, 0:n - k + 1].copy()
    for j in range(1, k):
        acc += x[:, j:n - k + 1 + j]
    X[:, k - 1:] = acc
    return X


def host_loglogistic(X, k, max_shape=1000.0):
    from scipy.special import ndtri
    ncell, nmonths = X.shape
    out = np.empty_like(X)
    for m in range(12):
        u = np.arange(m, nmonths, 12)
        s = np.sort(X[:, u[u >= k - 1]], axis=1)                                   # [ncell, n]; a NaN sorts last
        n = s.shape[1]
        i = np.arange(1, n + 1)
        c1, c2 = (n - i) / (n - 1.0), ((n - i) * (n - i - 1)) / ((n - 1.0) * (n - 2.0))
        with np.errstate(all='ignore'):
            w0, w1, w2 = s.sum(1) / n, (s @ c1) / n, (s @ c2) / n
            beta = (2.0 * w1 - w0) / (6.0 * w1 - w0 - 6.0 * w2)
            pb = np.pi / beta
            g = pb / np.sin(pb)
            alpha = (w0 - 2.0 * w1) * beta / g
            gamma = w0 - alpha * g
            ok = np.isfinite(alpha) & np.isfinite(beta) & np.isfinite(gamma) & (np.abs(beta) > 1) & (np.abs(beta) <= max_shape) \
                & (s[:, 0] != s[:, -1]) & (n >= 4)
            v = X[:, u]
            z = (v - gamma[:, None]) / alpha[:, None]
            inside = z > 0
            H = np.where(inside, 1.0 / (1.0 + np.exp(-beta[:, None] * np.log(np.where(inside, z, 1.0)))),
                         np.where(alpha[:, None] > 0, 0.0, 1.0))
            idx = np.clip(ndtri(H), -CLIP, CLIP)
        idx[~ok[:, None] | np.isnan(v)] = np.nan
        out[:, u] = idx
    return out


def timed(ctx, reps, call):
    """Per-call milliseconds of the library's std_index timer: one warm-up, then ``reps`` single calls."""
    call()
    ctx.sync()
    ms = []
    for _ in range(reps):
        ctx.timing_reset()
        call()
        ctx.sync()
        t, calls = ctx.timing('std_index')
        assert calls == 1
        ms.append(t)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=67420)
    ap.add_argument('--months', type=int, default=600)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'spei'))
    a = ap.parse_args()
    ctx = _hip.get_context(0)
    ncell, nmonths, nyr = a.cells, a.months, a.months // 12
    p, pet = make_fields(ncell, nmonths)
    d_p, d_pet = ctx.upload(p), ctx.upload(pet)
    res = {'device': ctx.name(), 'ncell': ncell, 'nmonths': nmonths, 'reps': a.reps, 'cases': []}
    t = time.time()
    host_p, host_pet = d_p.download(), d_pet.download()
    res['download_ms'] = download_ms = (time.time() - t) * 1e3
    for scales in SCALE_SETS:
        idx = [ctx.empty((ncell, nmonths)) for _ in scales]
        par = [ctx.empty((ncell, 12, 4)) for _ in scales]
        fit_ms = timed(ctx, a.reps, lambda: ctx.std_index(ncell, nmonths, scales, 0, nyr, 'loglogistic', 1000.0, d_p, idx,
                                                          par_out=par, minus=d_pet))
        fed_ms = timed(ctx, a.reps, lambda: ctx.std_index(ncell, nmonths, scales, 0, nyr, 'loglogistic', 1000.0, d_p, idx,
                                                          par_in=par, minus=d_pet))
        ctx.std_index(ncell, nmonths, scales, 0, nyr, 'loglogistic', 1000.0, d_p, idx, par_out=par, minus=d_pet)
        ctx.sync()
        traffic = 8 * ncell * nmonths * (2 + len(scales))
        n_of = lambda k: [len(range(max(m, m + 12 * ((k - 1 - m + 11) // 12)), nmonths, 12)) for m in range(12)]
        med = float(np.median(fit_ms))
        case = {'scales': list(scales), 'kernel_ms': {'min': min(fit_ms), 'median': med, 'max': max(fit_ms)},
                'kernel_ms_with_tables': {'min': min(fed_ms), 'median': float(np.median(fed_ms)), 'max': max(fed_ms)},
                'algorithmic_bytes': traffic, 'achieved_GBps': traffic / med / 1e6,
                'ranking_lds_reads': int(ncell * sum(sum(n * n for n in n_of(k)) for k in scales)),
                'transcendental_evaluations': int(3 * ncell * nmonths * len(scales))}
        if not a.no_host:
            t = time.time()
            balance = host_p - host_pet
            host = {k: host_loglogistic(accumulate(balance, k), k) for k in scales}
            case['host_numpy_ms'] = (time.time() - t) * 1e3
            case['host_path_ms'] = case['host_numpy_ms'] + download_ms
            rows = np.arange(0, ncell, max(ncell // 512, 1))
            worst, differ = 0.0, 0
            for k, d in zip(scales, idx):
                got, want = d.download()[rows], host[k][rows]
                differ += int((np.isnan(got) != np.isnan(want)).sum())
                m = ~np.isnan(want) & ~np.isnan(got)
                worst = max(worst, float(np.abs(got[m] - want[m]).max()))
            case['max_abs_difference_on_sampled_cells'] = worst
            case['nan_mask_differences_on_sampled_cells'] = differ      # (np.sum is pairwise: |beta| next to a limit may differ)
            case['speedup'] = case['host_path_ms'] / med
        print(json.dumps(case), flush=True)
        res['cases'].append(case)
        for d in idx + par:
            d.free()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'bench_spei.json'), 'w') as fh:
        json.dump(res, fh, indent=1)
    lines = [BEGIN, 'Written by `tools/bench_spei.py` on one MI355X ({}) at {} cells x {} months (reference period: the whole series; '
             '{} single calls after a warm-up; download of the two arrays: {:.1f} ms).  It records, it does not gate.'.format(
                 res['device'].strip().strip('()'), ncell, nmonths, a.reps, download_ms), '',
             '| scales | kernel ms (min / median / max) | with the tables handed in | GB/s of algorithmic traffic | LDS reads of the '
             'ranking | log + exp + ndtri | download + numpy ms | ratio | max abs difference (sampled cells) |',
             '|---|---|---|---|---|---|---|---|---|']
    for c in res['cases']:
        k, f = c['kernel_ms'], c['kernel_ms_with_tables']
        lines.append('| {} | {:.3f} / {:.3f} / {:.3f} | {:.3f} / {:.3f} / {:.3f} | {:.1f} | {:.3g} | {:.3g} | {} | {} | {} |'.format(
            ', '.join(str(s) for s in c['scales']), k['min'], k['median'], k['max'], f['min'], f['median'], f['max'],
            c['achieved_GBps'], c['ranking_lds_reads'], c['transcendental_evaluations'],
            '{:.0f}'.format(c['host_path_ms']) if 'host_path_ms' in c else '-',
            '{:.0f} x'.format(c['speedup']) if 'speedup' in c else '-',
            '{:.2g}'.format(c['max_abs_difference_on_sampled_cells']) if 'speedup' in c else '-'))
    lines += [END]
    readme = os.path.join(a.out, 'README.md')
    text = open(readme).read() if os.path.isfile(readme) else '# SPI / SPEI: `xh_std_index2` with the log-logistic distribution\n\n{}\n{}\n'.format(BEGIN, END)
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN)] + '\n'.join(lines) + text[text.index(END) + len(END):]
    else:
        text += '\n' + '\n'.join(lines) + '\n'
    with open(readme, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
