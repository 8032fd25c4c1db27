"""The across-member statistics of csrc/xh_ens.hip restated in numpy, operation for operation (no test file: helpers).

Each function takes the stacked members ``x`` [S, ...] and walks the member axis with the kernel's own loop, vectorised
over the elements only.  test_ensemble_host.py holds these loops to numpy's reductions (np.mean, np.std(ddof=1), np.min,
np.max, np.quantile(method='linear') over axis 0) bit for bit; test_gpu_ensemble.py holds the kernel to both."""
import numpy as np

STATS = ('mean', 'std', 'min', 'max')


def mean(x):
    s = np.zeros(x.shape[1:])
    for j in range(x.shape[0]):
        s = s + x[j]
    return s / float(x.shape[0])


def std(x):
    m = mean(x)
    ss = np.zeros(x.shape[1:])
    for j in range(x.shape[0]):
        d = x[j] - m
        ss = ss + d * d
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.sqrt(ss / float(x.shape[0] - 1))


def _fold(x, better):
    m = x[0].copy()
    for j in range(1, x.shape[0]):
        keep = better(m, x[j]) | np.isnan(m)
        m = np.where(keep, m, x[j])
    return m


def minimum(x):
    return _fold(x, np.less)


def maximum(x):
    return _fold(x, np.greater)


def quantile(x, q):
    S = x.shape[0]
    a = np.sort(x, axis=0)                      # ascending (NaN last; such elements are overwritten below)
    h = float(S - 1) * float(q)
    lo = int(np.floor(h))
    hi = min(lo + 1, S - 1)
    g = h - lo
    with np.errstate(invalid='ignore'):
        d = a[hi] - a[lo]
        r = a[lo] + d * g if g < 0.5 else a[hi] - d * (1.0 - g)
    return np.where(np.isnan(x).any(axis=0), np.nan, r)


def parse(stat):
    """'mean' / 'std' / 'min' / 'max' -> (name, None); 'qNN' -> ('q', NN / 100)."""
    if stat in STATS:
        return stat, None
    return 'q', int(stat[1:]) / 100.0


def stat(x, name):
    kind, q = parse(name)
    return {'mean': mean, 'std': std, 'min': minimum, 'max': maximum}[kind](x) if q is None else quantile(x, q)


def numpy_stat(x, name):
    """The same statistic by numpy's own reduction over axis 0."""
    kind, q = parse(name)
    with np.errstate(invalid='ignore', divide='ignore'):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            if q is not None:
                return np.quantile(x, q, axis=0, method='linear')
            return {'mean': lambda a: np.mean(a, axis=0), 'std': lambda a: np.std(a, axis=0, ddof=1),
                    'min': lambda a: np.min(a, axis=0), 'max': lambda a: np.max(a, axis=0)}[kind](x)


def stack(seed, S, n, nan_share=0.01):
    """Random [S, n] members for the kernel tests: finite values of mixed magnitude, ties across members, NaN in the
    first, a middle and the last member, and (n >= 4) one element NaN in every member."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((S, n)) * np.exp(rng.uniform(-3, 6, (1, n)))
    ties = rng.random((S, n)) < 0.2
    x[ties] = np.round(x[ties])                 # equal values across members
    if n >= 2 and S >= 2:
        x[:, 1] = x[0, 1]                       # an element all members agree on
    x[rng.random((S, n)) < nan_share] = np.nan
    if n >= 4:
        x[0, n // 4] = np.nan
        x[S // 2, n // 2] = np.nan
        x[S - 1, 3 * n // 4] = np.nan
        x[:, n - 1] = np.nan
    return x
