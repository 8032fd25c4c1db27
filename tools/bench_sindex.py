"""The standardized drought indices in HBM (``xh_std_index``) against the path they replace, at full size (67,420 cells x 600
months).

    python tools/bench_sindex.py [--cells 67420] [--months 600] [--reps 5] [--no-host]      # writes the JSON and README

For the scales (1) and (1, 3, 12) and both distributions, on a seeded seasonal gamma field with 2 % zeros (reference period:
the whole series):
(a) ``xh_std_index`` on the array in HBM, all scales in one call, the gamma fit written out as the product does: the
    library's ``std_index`` timer, and the algorithmic HBM traffic (8 B in once, 8 B out per scale and cell-month);
(b) the path it replaces, in the same process: the array downloaded (host clock), then numpy / scipy per scale -- the
    definitions of DESIGN 4.18 vectorised over the cells (``scipy.special.gammainc`` / ``ndtri``; the empirical counts as one
    comparison of every month against its calendar month's sample).  (tests/sindex_np.py states the same per cell and calendar
    month; at this size its Python loops would take hours.)  The two are compared on a sample of cells.
It records, it does not gate.  Results: profiles/drought_index/bench_sindex.json and the table in
profiles/drought_index/README.md."""
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
DISTS = ('gamma', 'empirical')
CLIP = 3.09


def make_field(ncell, nmonths, seed=5):
    rng = np.random.default_rng(seed)
    shape = rng.uniform(0.6, 8.0, (ncell, 1)).astype(np.float32)
    season = 1.0 + 0.6 * np.sin(2 * np.pi * (np.arange(nmonths) % 12) / 12.0 + rng.uniform(0, 6.28, (ncell, 1)))
    x = rng.standard_gamma(shape, (ncell, nmonths)) * (30.0 / shape) * season
    x[rng.random((ncell, nmonths)) < 0.02] = 0.0
    return np.ascontiguousarray(x, dtype=np.float64)


def accumulate(x, k):
    X = np.full(x.shape, np.nan)
    n = x.shape[1]
    acc = x[:, 0:n - k + 1].copy()
    for j in range(1, k):
        acc += x[:, j:n - k + 1 + j]
    X[:, k - 1:] = acc
    return X


def host_gamma(X, k, max_shape=1000.0):
    from scipy.special import gammainc, ndtri
    ncell, nmonths = X.shape
    Y = X.reshape(ncell, nmonths // 12, 12)
    valid = (np.arange(nmonths).reshape(-1, 12) >= k - 1)[None]                    # the sample: u >= k - 1
    with np.errstate(all='ignore'):
        bad = (valid & ~(Y >= 0)).any(1)
        pos = valid & (Y > 0)
        npos = pos.sum(1)
        n = valid.sum(1)
        q0 = (valid & (Y == 0)).sum(1) / n
        mu = np.where(pos, Y, 0.0).sum(1) / npos
        ml = np.where(pos, np.log(np.where(pos, Y, 1.0)), 0.0).sum(1) / npos
        A = np.log(mu) - ml
        alpha = (1.0 + np.sqrt(1.0 + 4.0 * A / 3.0)) / (4.0 * A)
        ok = ~bad & (npos >= 4) & (A > 0) & (alpha <= max_shape)
        alpha, beta, q0 = [np.where(ok, v, np.nan) for v in (alpha, mu / np.where(ok, alpha, 1.0), q0)]
        a, b, q = [np.broadcast_to(v[:, None, :], Y.shape) for v in (alpha, beta, q0)]
        H = np.where(Y == 0, q, q + (1.0 - q) * gammainc(a, Y / b))
        z = np.clip(ndtri(H), -CLIP, CLIP)
        z[~(Y >= 0)] = np.nan
    return z.reshape(ncell, nmonths)


def host_empirical(X, k):
    from scipy.special import ndtri
    ncell, nmonths = X.shape
    out = np.empty_like(X)
    for m in range(12):
        u = np.arange(m, nmonths, 12)
        s = X[:, u[u >= k - 1]]                                                     # [ncell, n]
        v = X[:, u]                                                                 # [ncell, years]
        L = (s[:, None, :] < v[:, :, None]).sum(2)
        E = (s[:, None, :] == v[:, :, None]).sum(2)
        n = s.shape[1]
        in_ref = (u >= k - 1).astype(np.float64)[None]                              # the reference period is the whole series
        with np.errstate(all='ignore'):
            p = (L + (E + 2 - in_ref) / 2.0 - 0.44) / (n + 1 - in_ref + 0.12)
            z = np.clip(ndtri(p), -CLIP, CLIP)
        z[np.isnan(v) | np.isnan(s).any(1)[:, None] | (n < 4)] = np.nan
        out[:, u] = z
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=67420)
    ap.add_argument('--months', type=int, default=600)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'drought_index'))
    a = ap.parse_args()
    ctx = _hip.get_context(0)
    ncell, nmonths = a.cells, a.months
    x = make_field(ncell, nmonths)
    d_x = ctx.upload(x)
    nyr = nmonths // 12
    res = {'device': ctx.name(), 'ncell': ncell, 'nmonths': nmonths, 'reps': a.reps, 'cases': []}
    t = time.time()
    host_x = d_x.download()
    download_ms = (time.time() - t) * 1e3
    res['download_ms'] = download_ms
    for dist in DISTS:
        for scales in SCALE_SETS:
            idx = [ctx.empty((ncell, nmonths)) for _ in scales]
            par = [ctx.empty((ncell, 12, 4)) for _ in scales] if dist == 'gamma' else None
            ctx.std_index(ncell, nmonths, scales, 0, nyr, dist, 1000.0, d_x, idx, par_out=par)      # warm-up
            ctx.sync()
            ctx.timing_reset()
            for _ in range(a.reps):
                ctx.std_index(ncell, nmonths, scales, 0, nyr, dist, 1000.0, d_x, idx, par_out=par)
            ctx.sync()
            ms, calls = ctx.timing('std_index')
            assert calls == a.reps
            kernel_ms = ms / calls
            traffic = 8 * ncell * nmonths * (1 + len(scales))
            case = {'distribution': dist, 'scales': list(scales), 'kernel_ms': kernel_ms, 'algorithmic_bytes': traffic,
                    'achieved_GBps': traffic / kernel_ms / 1e6}
            if not a.no_host:
                t = time.time()
                host = {k: (host_gamma if dist == 'gamma' else host_empirical)(accumulate(host_x, k), k) for k in scales}
                case['host_numpy_ms'] = (time.time() - t) * 1e3
                case['host_path_ms'] = case['host_numpy_ms'] + download_ms
                rows = np.arange(0, ncell, max(ncell // 512, 1))
                worst = 0.0
                for k, d in zip(scales, idx):
                    got = d.download()[rows]
                    want = host[k][rows]
                    assert np.array_equal(np.isnan(got), np.isnan(want)), (dist, k)
                    m = ~np.isnan(want)
                    worst = max(worst, float(np.abs(got[m] - want[m]).max()))
                case['max_abs_difference_on_sampled_cells'] = worst
                case['speedup'] = case['host_path_ms'] / kernel_ms
            print(json.dumps(case), flush=True)
            res['cases'].append(case)
            for d in idx + (par or []):
                d.free()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'bench_sindex.json'), 'w') as fh:
        json.dump(res, fh, indent=1)
    lines = ['# Standardized drought indices: `xh_std_index` against download + numpy / scipy', '',
             'Written by `tools/bench_sindex.py` on one MI355X{} at {} cells x {} months (reference period: the whole series; {} '
             'repetitions; download of the array: {:.1f} ms).  It records, it does not gate.'.format(
                 ' ' + res['device'].strip() if res['device'].strip().startswith('(') else ' (' + res['device'].strip() + ')', ncell, nmonths,
                 a.reps, download_ms), '',
             '| distribution | scales | kernel ms | GB/s of algorithmic traffic | download + numpy / scipy ms | ratio | max abs '
             'difference (sampled cells) |', '|---|---|---|---|---|---|---|']
    for c in res['cases']:
        lines.append('| {} | {} | {:.3f} | {:.1f} | {} | {} | {} |'.format(
            c['distribution'], ', '.join(str(k) for k in c['scales']), c['kernel_ms'], c['achieved_GBps'],
            '{:.0f}'.format(c['host_path_ms']) if 'host_path_ms' in c else '-',
            '{:.0f} x'.format(c['speedup']) if 'speedup' in c else '-',
            '{:.2g}'.format(c['max_abs_difference_on_sampled_cells']) if 'speedup' in c else '-'))
    lines += ['', 'The kernel is bound by the incomplete-gamma iterations (gamma) and by the LDS reads of the rank counts '
              '(empirical), not by HBM: the traffic column is far below the 8 TB/s of the device.  See DESIGN 4.18.', '']
    with open(os.path.join(a.out, 'README.md'), 'w') as fh:
        fh.write('\n'.join(lines))


if __name__ == '__main__':
    main()
