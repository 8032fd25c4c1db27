"""Inputs, references and the probe loader shared by test_math_host.py (CPU) and test_gpu_math.py (GPU).

Every input set is seeded and is built here once, so both suites see identical arrays: a dense random part of at least
2^22 values and a structured part (class boundaries, selects, neighbours of rounding edges).

"Equal in bits" throughout means `same_bits`: identical NaN masks and identical 64-bit patterns everywhere else (so the
sign of a zero counts).  The payload and sign of a NaN are not compared: IEEE 754 leaves them open, and x86 and gfx950
produce different ones for the same invalid operation.
"""
import ctypes
import itertools
import os

import numpy as np

from oracle import abcd as o_abcd

HERE = os.path.dirname(os.path.abspath(__file__))
PROBE_SO = os.path.join(HERE, 'math_probe', 'libmath_probe.so')

OP_XH_EXP, OP_LIB_EXP, OP_XH_EXP_NONPOS, OP_XH_SQRT, OP_LIB_SQRT, OP_FRCP = range(6)
OP_QUOT, OP_IEEE_DIV, OP_FDIV = range(3)

N_DENSE = 1 << 22
TINY = 2.0 ** -1074
LN2 = float(np.log(2.0))

_P = ctypes.POINTER(ctypes.c_double)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_P)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class Probe:
    """ctypes face of tests/math_probe/libmath_probe.so (built by build(); a missing library is an error)."""

    def __init__(self):
        if not os.path.isfile(PROBE_SO):
            raise RuntimeError('the math probe is not built: ' + PROBE_SO + ' (build() makes it)')
        self.lib = ctypes.CDLL(PROBE_SO)
        i64, i32 = ctypes.c_int64, ctypes.c_int32
        self.lib.probe_unary.argtypes = self.lib.probe_host_unary.argtypes = [ctypes.c_int, i64, _P, _P]
        self.lib.probe_binary.argtypes = self.lib.probe_host_binary.argtypes = [ctypes.c_int, i64, _P, _P, _P]
        self.lib.probe_split.argtypes = [i64, ctypes.c_int, _P, _P, _P, _P, _P, ctypes.POINTER(i32)]
        self.lib.probe_march.argtypes = [i64, i32, ctypes.c_int] + [_P] * 10

    @staticmethod
    def _ok(rc, what):
        if rc != 0:
            raise RuntimeError('{} failed with code {}'.format(what, rc))

    def unary(self, op, x, host=False):
        x = f64(x).ravel()
        out = np.empty_like(x)
        fn = self.lib.probe_host_unary if host else self.lib.probe_unary
        self._ok(fn(op, x.size, _ptr(x), _ptr(out)), 'probe_unary')
        return out

    def binary(self, op, x, d, host=False):
        x, d = f64(x).ravel(), f64(d).ravel()
        assert x.size == d.size
        out = np.empty_like(x)
        fn = self.lib.probe_host_binary if host else self.lib.probe_binary
        self._ok(fn(op, x.size, _ptr(x), _ptr(d), _ptr(out)), 'probe_binary')
        return out

    def split(self, snow_on, precip, tmin):
        precip, tmin = f64(precip).ravel(), f64(tmin).ravel()
        rain, snow, frac = (np.empty_like(precip) for _ in range(3))
        kind = np.empty(precip.size, dtype=np.int32)
        self._ok(self.lib.probe_split(precip.size, int(snow_on), _ptr(precip), _ptr(tmin), _ptr(rain), _ptr(snow), _ptr(frac),
                                      kind.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), 'probe_split')
        return rain, snow, frac, kind

    def march(self, pars, pet, precip, tmin, sm0, gw0, fastq=False, snowpack0=None):
        """pars [ncell, 5]; pet / precip / tmin [ncell, nmonths] (tmin None: no snow). Returns aet, q, sav, decay
        [ncell, nmonths] and the final state [3, ncell]."""
        pars, pet, precip = f64(pars), f64(pet), f64(precip)
        tmin = None if tmin is None else f64(tmin)
        ncell, nm = pet.shape
        assert pars.shape == (ncell, 5) and precip.shape == pet.shape and (tmin is None or tmin.shape == pet.shape)
        st0 = np.zeros((3, ncell))
        if snowpack0 is not None:
            st0[0] = snowpack0
        st0[1], st0[2] = sm0, gw0
        aet, q, sav, decay = (np.empty_like(pet) for _ in range(4))
        st1 = np.empty_like(st0)
        self._ok(self.lib.probe_march(ncell, nm, int(fastq), _ptr(pars), _ptr(pet), _ptr(precip), _ptr(tmin), _ptr(st0),
                                      _ptr(aet), _ptr(q), _ptr(sav), _ptr(decay), _ptr(st1)), 'probe_march')
        return aet, q, sav, decay, st1


_probe = None


def probe():
    global _probe
    if _probe is None:
        _probe = Probe()
    return _probe


# ------------------------------------------------------------------------------------------------ comparing
def bits(a):
    return f64(a).view(np.int64)


def same_bits(x, ref):
    x, ref = f64(x), f64(ref)
    if x.shape != ref.shape:
        return False
    nx, nr = np.isnan(x), np.isnan(ref)
    return bool(np.array_equal(nx, nr) and np.array_equal(bits(x)[~nr], bits(ref)[~nr]))


def describe_mismatch(x, ref, inputs=None, limit=5):
    """Text for an assertion message: how many differ and the first few with their inputs."""
    x, ref = f64(x).ravel(), f64(ref).ravel()
    nx, nr = np.isnan(x), np.isnan(ref)
    bad = np.flatnonzero((nx != nr) | (~nr & ~nx & (bits(x) != bits(ref))))
    lines = ['{} of {} differ'.format(bad.size, x.size)]
    for i in bad[:limit]:
        extra = '' if inputs is None else ' in=' + ', '.join(float(f64(a).ravel()[i]).hex() for a in inputs)
        lines.append('  [{}] got {} want {}{}'.format(i, float(x[i]).hex(), float(ref[i]).hex(), extra))
    return '\n'.join(lines)


def steps_apart(x, ref):
    """Distance in representable doubles (both finite, same sign or zero)."""
    def key(a):
        b = bits(a)
        return np.where(b < 0, np.int64(-2 ** 63) - b, b)       # monotone in the value
    return np.abs(key(x) - key(ref))


def ulp_of(t):
    """Spacing of float64 at |t| (t a longdouble or float64 array); 2^-1074 in the subnormal range."""
    return np.spacing(np.abs(np.asarray(t, dtype=np.float64))).astype(np.longdouble)


def ulp_error(e, true):
    """|e - true| in ulp of true; ``true`` a longdouble array (64-bit significand: good to 2^-11 ulp)."""
    e = np.asarray(e, dtype=np.float64)
    true = np.asarray(true, dtype=np.longdouble)
    ok = np.isfinite(true) & np.isfinite(e)
    err = np.zeros(e.shape, dtype=np.longdouble)
    err[ok] = np.abs(e[ok].astype(np.longdouble) - true[ok]) / ulp_of(true[ok])
    return err


def have_extended():
    return np.finfo(np.longdouble).nmant >= 63


def exp_true(x):
    """exp(x) to 64 significant bits (x87 extended), overflow / underflow beyond the double range included."""
    assert have_extended(), 'numpy.longdouble is not wider than float64 on this platform'
    with np.errstate(over='ignore', under='ignore'):
        return np.exp(np.asarray(x, dtype=np.float64).astype(np.longdouble))


def exp_true_mp(x):
    """The same from mpmath at 120 bits, rounded to longdouble (a sample's worth: slow)."""
    import mpmath
    out = np.empty(len(x), dtype=np.longdouble)
    with mpmath.workprec(120):
        for i, v in enumerate(x):
            m, e = mpmath.frexp(mpmath.exp(mpmath.mpf(float(v))))
            hi = float(m)                                       # m in [0.5, 1): split into two doubles
            lo = float(m - mpmath.mpf(hi))
            out[i] = np.ldexp(np.longdouble(hi) + np.longdouble(lo), int(e))
    return out


# ------------------------------------------------------------------------------------------------ input sets
def neighbours(v, k=3):
    """v and its k neighbours on each side."""
    v = f64(v).ravel()
    out = [v]
    lo, hi = v, v
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


def exp_inputs():
    """dict name -> array for xh_exp: the sweep of [-1080, 1030], every result class, ABCD's own arguments."""
    rng = np.random.default_rng(20240611)
    sets = {'dense': rng.uniform(-1080.0, 1030.0, N_DENSE)}
    n = np.arange(-1560, 1490, dtype=np.float64)               # (n + 1/2) ln 2 covers [-1080.9, 1032.4]
    half = (n + 0.5) * LN2
    sets['structured'] = np.concatenate([
        [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0],
        neighbours([2.0 ** -54, -2.0 ** -54, 2.0 ** -55, -2.0 ** -55, TINY, -TINY, 1e-300, -1e-300, 2.0 ** -1022]),
        neighbours([1024.0, -1075.0, 709.782712893384, -708.3964185322641, -745.1332191019412, -744.4400719213812], 4),
        np.linspace(-745.2, -708.3, 1 << 16),                  # subnormal results
        rng.uniform(-745.2, -708.3, 1 << 16),
        neighbours(half, 4),                                   # the reduction's k changes here
        np.arange(-1080.0, 1031.0),
        rng.uniform(-1.0, 1.0, 1 << 16) * 2.0 ** rng.integers(-60, 1, 1 << 16),
    ])
    pet = np.concatenate([[0.0], 10.0 ** rng.uniform(-6, 4, (1 << 20) - 1)])
    b = np.concatenate([10.0 ** rng.uniform(-1, np.log10(8000.0), (1 << 20) - 2), [0.1, 8000.0]])
    sets['abcd'] = -pet / b
    return sets


def exp_nonpos_inputs():
    rng = np.random.default_rng(20240612)
    return np.concatenate([
        rng.uniform(-1080.0, 0.0, N_DENSE),
        [0.0, -0.0, -np.inf, -TINY, -1075.0, -1080.0],
        neighbours([-1075.0, -745.1332191019412, -708.3964185322641, -2.0 ** -54], 4),
        np.linspace(-745.2, -708.3, 1 << 14),
        -10.0 ** rng.uniform(-12, 3, 1 << 16),
    ])


def _roots_mod_pow2(a, n):
    """Every y mod 2^n with y^2 = a (mod 2^n), for a = 1 (mod 8): Hensel lifting, four roots."""
    sols = {1, 3, 5, 7}
    for k in range(3, n):
        mod = 1 << (k + 1)
        cand = set()
        for y in sols:
            for c in (y, y + (1 << (k - 1))):
                cand.update((c % mod, -c % mod, (c + (1 << k)) % mod, (-c + (1 << k)) % mod))
        sols = {y for y in cand if (y * y - a) % mod == 0}
    return sorted(sols)


def sqrt_hard_cases():
    """Arguments whose square root lies next to a rounding boundary, where an iteration that is one correction short
    rounds the wrong way.  With Y odd in [2^53, 2^54), Y / 2 is a midpoint between two 53-bit significands; x = Y^2 - r is
    a double exactly when Y^2 = r modulo the spacing of doubles at Y^2 (2^54 or 2^55), which for every r = 1 (mod 8) has
    four roots.  sqrt(x) = Y - r / (2 Y): a midpoint minus (r > 0) or plus (r < 0) less than 2^-43 of a step.  Taken for
    |r| < 2048 and scaled by powers of 4; plus the classic 1 + j 2^-52 and 4 - j 2^-51 for odd j (r = j^2).  Any other
    argument keeps its root 2^-54 of a step or so from a boundary and cannot tell the last correction from none."""
    import math
    sig = []
    for r in range(-2047, 2048, 8):
        for n, lo, hi in ((55, math.isqrt(1 << 107) + 1, 1 << 54), (54, 1 << 53, math.isqrt(1 << 107))):
            for y in _roots_mod_pow2(r % (1 << n), n):
                for Y in range(y, 1 << 54, 1 << n):
                    m = (Y * Y - r) >> n
                    if lo <= Y < hi and (1 << 52) <= m < (1 << 53):
                        sig.append(math.ldexp(float(m), n - 106))             # in [1, 4)
    j = np.arange(1.0, 512.0, 2.0)
    sig = np.concatenate([sig, 1.0 + j * 2.0 ** -52, 4.0 - j * 2.0 ** -51])
    scale = 4.0 ** np.arange(-340.0, 505.0, 7.0)
    return np.outer(scale, sig).ravel()


def sqrt_inputs():
    rng = np.random.default_rng(20240613)
    n = rng.integers(1, 1 << 26, 1 << 18).astype(np.float64)
    sq = n * n                                                  # exact: below 2^52
    scale = 2.0 ** (2 * rng.integers(-300, 480, sq.size))
    return np.concatenate([
        2.0 ** rng.uniform(-700.0, 1023.0, N_DENSE),
        [0.0, -0.0, np.inf, np.nan, -np.inf, -1.0, -TINY, -1e300, 1.0, 2.0, 4.0, 2.0 ** 1023, 2.0 ** -700],
        -(2.0 ** rng.uniform(-700.0, 1023.0, 1 << 12)),
        neighbours(sq, 1), neighbours(sq * scale, 1),
        neighbours(2.0 ** np.arange(-700.0, 1024.0), 2)[:-2],
        sqrt_hard_cases(),
    ])


BOX_LO = np.array([1e-4, 1e-4, 1e-4, 1e-4, 1e-4])              # a, b, c, d, m: the box calibration searches
BOX_HI = np.array([1 - 1e-4, 8 - 1e-4, 1 - 1e-4, 1 - 1e-4, 1 - 1e-4])
TODAY_LO = np.array([0.9, 0.1, 0.01, 0.01, 0.1])               # golden/abcd.npz and synth.make_world
TODAY_HI = np.array([0.999, 2.0, 0.9, 0.9, 0.9])


def quot_inputs():
    """dict family -> (x, d): the month update's three divisor families with numerators it can form, + structured."""
    rng = np.random.default_rng(20240614)
    n = 1 << 21
    tspan = o_abcd.TRAIN - o_abcd.TSNOW
    tmin = np.concatenate([rng.uniform(0.6, 2.5, n - 14), neighbours([0.6, 2.5], 3)])
    precip = 10.0 ** rng.uniform(-3, 4, n)
    sets = {'tspan_frac': (o_abcd.TRAIN - tmin, np.full(n, tspan)),
            'tspan_snow': (precip * (o_abcd.TRAIN - tmin), np.full(n, tspan))}
    par = rng.uniform(BOX_LO, BOX_HI, (n, 5))
    par[:64] = np.array(list(itertools.product(*zip(BOX_LO, BOX_HI))) * 2)      # the corners too
    a, b, c, d = par[:, 0], par[:, 1] * 1000, par[:, 2], par[:, 3]
    w = np.concatenate([[0.0], 10.0 ** rng.uniform(-6, 4, n - 1)])
    pet = np.concatenate([[0.0], 10.0 ** rng.uniform(-6, 4, n - 1)])
    gw = 10.0 ** rng.uniform(-8, 5, n)
    awet = w * rng.uniform(0, 1, n)
    sets['two_a'] = (w + b, a * 2)
    sets['b'] = (0.0 - pet + 0.0, b)                           # +0 for pet = 0 (the signed zero is pinned separately)
    sets['d_plus_1'] = (gw + c * awet, d + 1)
    k = np.arange(-40.0, 41.0)
    dz = np.concatenate([2.0 ** k, np.nextafter(2.0 ** k, 0.0)])    # all-zeros and all-ones mantissas
    xs = np.concatenate([np.zeros(dz.size), rng.uniform(0.5, 2.0, dz.size * 64) * 2.0 ** rng.integers(-30, 31, dz.size * 64)])
    sets['mantissa_edges'] = (xs, np.concatenate([dz, np.tile(dz, 64)]))
    return sets


QUOT_DIVISORS = (1.9, 2e-4, 1.9999, 8000.0)


def quot_extreme_inputs():
    """(x_mid, x_small, d): |x| in [2^-960, 2^1000] where equality is claimed, and below 2^-1000 where it is not."""
    rng = np.random.default_rng(20240615)
    n = 1 << 18
    d = np.tile(QUOT_DIVISORS, n // 4)
    sgn = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    mid = sgn * rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-960, 1000, n)
    small = sgn * rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-1070, -1000, n)
    return mid, small, d


def check_quot(run):
    """The quot() contract, for `run(x, d) -> quot(x, d, 1 / d)` on the host or on the device."""
    for name, (x, d) in quot_inputs().items():
        got, want = run(x, d), x / d
        assert same_bits(got, want), name + ': ' + describe_mismatch(got, want, (x, d))
    mid, small, d = quot_extreme_inputs()
    got, want = run(mid, d), mid / d
    assert same_bits(got, want), '2^-960 <= |x| <= 2^1000: ' + describe_mismatch(got, want, (mid, d))
    got, want = run(small, d), small / d
    steps = steps_apart(got, want)
    print('quot, |x| < 2^-1000: {} of {} one step from x / d, worst {}'.format(int((steps > 0).sum()), steps.size, int(steps.max())))
    assert steps.max() <= 1
    # outside the claim, pinned: the sign of a zero numerator is lost, an infinite numerator gives NaN
    dd = np.array(QUOT_DIVISORS)
    z = run(np.full(4, -0.0), dd)
    assert np.all(z == 0.0) and not np.signbit(z).any(), 'quot(-0.0, d) is +0.0 (IEEE: -0.0)'
    z = run(np.zeros(4), dd)
    assert np.all(z == 0.0) and not np.signbit(z).any()
    assert np.isnan(run(np.full(4, np.inf), dd)).all() and np.isnan(run(np.full(4, -np.inf), dd)).all(), \
        'quot(+-inf, d) is NaN (IEEE: +-inf)'
    assert np.isnan(run(np.full(4, np.nan), dd)).all()


def fdiv_inputs():
    rng = np.random.default_rng(20240616)
    n = N_DENSE
    sgn = lambda: np.where(rng.random(n) < 0.5, -1.0, 1.0)
    den = sgn() * 10.0 ** rng.uniform(-6, 12, n)
    num = sgn() * 10.0 ** rng.uniform(-6, 12, n)
    den[:8] = [1e-6, -1e-6, 1e12, -1e12, 1.0, 3.0, 101300.0, 287.058]
    num[:8] = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    return num, den


def split_inputs():
    rng = np.random.default_rng(20240617)
    n = 1 << 20
    edge_t = np.concatenate([neighbours([o_abcd.TSNOW, o_abcd.TRAIN], 2), [np.nan, np.inf, -np.inf, 0.0, -0.0, -40.0, 40.0]])
    edge_p = np.array([0.0, np.nan, TINY, 2.0 ** -1060, 1e-310, 1.0, 123.456, 1e4])
    tt, pp = np.meshgrid(edge_t, edge_p)
    tmin = np.concatenate([rng.uniform(-6.0, 9.0, n), rng.uniform(0.6, 2.5, n), tt.ravel()])
    precip = np.concatenate([np.where(rng.random(2 * n) < 0.3, 0.0, rng.exponential(80.0, 2 * n)), pp.ravel()])
    return precip, tmin


def split_reference(precip, tmin):
    """rain, snow from the oracle's _split_rain_snow; the melt fraction of _march's mixed class; the class as kind."""
    rain, snow = o_abcd._split_rain_snow(precip[None, :], tmin[None, :])
    allrain = tmin > o_abcd.TRAIN
    mixed = (tmin <= o_abcd.TRAIN) & (tmin >= o_abcd.TSNOW)
    frac = (o_abcd.TRAIN - tmin) / (o_abcd.TRAIN - o_abcd.TSNOW)
    kind = np.where(allrain, 1, np.where(mixed, 2, 0)).astype(np.int32)
    return rain[0], snow[0], frac, kind, mixed


# ------------------------------------------------------------------------------------------------ ABCD cases
def box_parameters():
    """[n, 5] rows (a, b, c, d, m): 32 corners, 10 face centres, 2,000 random points of the box, 500 of today's range."""
    rng = np.random.default_rng(20240618)
    corners = np.array(list(itertools.product(*zip(BOX_LO, BOX_HI))))
    mid = 0.5 * (BOX_LO + BOX_HI)
    faces = np.tile(mid, (10, 1))
    for k in range(5):
        faces[2 * k, k], faces[2 * k + 1, k] = BOX_LO[k], BOX_HI[k]
    return np.concatenate([corners, faces, rng.uniform(BOX_LO, BOX_HI, (2000, 5)), rng.uniform(TODAY_LO, TODAY_HI, (500, 5))])


N_CORNERS, N_FACES = 32, 10
FORCINGS = ('wet30', 'wet15', 'dry', 'pet0', 'pet1e4', 'nan_precip', 'nan_tmin', 'tmin_edges', 'tiny_precip')


def forcing(kind, ncell, nmonths, seed):
    """pet, precip, tmin [ncell, nmonths] of one forcing family (FORCINGS, or 'inf_precip')."""
    rng = np.random.default_rng([20240619, seed, sum(map(ord, kind))])
    shape = (ncell, nmonths)
    pet = rng.uniform(0.0, 220.0, shape)
    wet = 0.15 if kind == 'wet15' else (0.0 if kind == 'dry' else 0.3)
    precip = np.where(rng.random(shape) < wet, rng.exponential(120.0, shape), 0.0)
    tmin = rng.normal(2.0, 5.0, shape)
    if kind == 'pet0':
        pet = np.where(rng.random(shape) < 0.5, 0.0, pet)
        pet[: ncell // 2] = 0.0
    elif kind == 'pet1e4':
        pet = np.where(rng.random(shape) < 0.5, 1e4, pet)
    elif kind == 'nan_precip':
        precip = np.where(rng.random(shape) < 0.02, np.nan, precip)
    elif kind == 'nan_tmin':
        tmin = np.where(rng.random(shape) < 0.1, np.nan, tmin)
    elif kind == 'tmin_edges':
        edges = neighbours([o_abcd.TSNOW, o_abcd.TRAIN], 1)
        tmin = np.where(rng.random(shape) < 0.6, edges[rng.integers(0, edges.size, shape)], tmin)
    elif kind == 'tiny_precip':
        precip = np.where(rng.random(shape) < 0.3, TINY * rng.integers(1, 1 << 20, shape), precip)
    elif kind == 'inf_precip':
        precip = np.where(rng.random(shape) < 0.01, np.inf, precip)
    elif kind not in ('wet30', 'wet15', 'dry'):
        raise ValueError(kind)
    return pet, precip, tmin


def box_cases(nmonths=120, n_random=None):
    """The committed case list of the month-update comparison: every parameter point under every forcing family.
    Returns pars [n, 5], pet, precip, tmin [n, nmonths], labels [n] (index into FORCINGS)."""
    P = box_parameters() if n_random is None else box_parameters()[:N_CORNERS + N_FACES + n_random]
    pars, pet, pr, tn, lab = [], [], [], [], []
    for k, kind in enumerate(FORCINGS):
        a, b, c = forcing(kind, len(P), nmonths, 1)
        pars.append(P), pet.append(a), pr.append(b), tn.append(c), lab.append(np.full(len(P), k))
    return tuple(np.concatenate(v) for v in (pars, pet, pr, tn, lab))


def oracle_march(pars, pet, precip, tmin, sm0, gw0, decay=None, gw_reciprocal=False):
    """oracle.abcd._march for per-cell rows [ncell, nmonths]; results transposed back to [ncell, nmonths]."""
    pars = f64(pars)
    nm = pet.shape[1]
    m = pars[:, 4] if tmin is not None else np.zeros(len(pars))
    res = o_abcd._march(pars[:, 0], pars[:, 1] * 1000, pars[:, 2], pars[:, 3], m, pet.T, precip.T,
                        None if tmin is None else tmin.T, f64(sm0), f64(gw0), nm,
                        decay=None if decay is None else decay.T, gw_reciprocal=gw_reciprocal)
    return tuple(np.ascontiguousarray(r.T) for r in res)


def restated_march(pars, pet, precip, tmin, sm0, gw0, rpt_ulps=0, exp_ulps=0, trace=None, dtype=np.float64):
    """A restatement of oracle.abcd._march (snow on) with two handles: rpt moved by ``rpt_ulps`` and exp by ``exp_ulps`` steps
    in the last place each month (alternating direction by month), and ``trace`` (a list) receiving the square root's
    argument of every month.  With both at 0 and float64 it is _march, bit for bit (asserted in test_math_host).
    dtype = numpy.longdouble gives the extended-precision march."""
    T = dtype
    pars = np.asarray(pars, dtype=T)
    a, b, c, d, m = pars[:, 0], pars[:, 1] * T(1000), pars[:, 2], pars[:, 3], pars[:, 4]
    pet, precip, tmin = (np.asarray(v, dtype=T).T for v in (pet, precip, tmin))
    rain, snow = o_abcd._split_rain_snow(precip, tmin)
    a2, b_over_a, d1 = a * 2, b / a, d + 1
    nm, ncell = pet.shape
    aet, q, sav = (np.empty((nm, ncell), dtype=T) for _ in range(3))
    pack = np.zeros(ncell, dtype=T)
    sm_prev, gw_prev = np.asarray(sm0, dtype=T), np.asarray(gw0, dtype=T)
    span = T(o_abcd.TRAIN) - T(o_abcd.TSNOW)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(nm):
            t = tmin[i]
            snm = np.zeros(ncell, dtype=T)
            pack = pack + snow[i]
            allrain = t > o_abcd.TRAIN
            mixed = (t <= o_abcd.TRAIN) & (t >= o_abcd.TSNOW)
            snm[allrain] = pack[allrain] * m[allrain]
            snm[mixed] = (pack[mixed] * m[mixed]) * ((T(o_abcd.TRAIN) - t[mixed]) / span)
            pack = pack - snm
            w = rain[i] + sm_prev if i == 0 else rain[i] + sm_prev + snm
            rpt = (w + b) / a2
            direction = np.inf if i % 2 == 0 else -np.inf
            for _ in range(rpt_ulps):
                rpt = np.nextafter(rpt, T(direction))
            arg = np.square(rpt) - (w * b_over_a)
            if trace is not None:
                trace.append(arg)
            y = rpt - np.sqrt(arg)
            e = np.exp(-pet[i] / b)
            for _ in range(exp_ulps):
                e = np.nextafter(e, T(direction))
            sm = y * e
            awet = w - y
            c_awet = c * awet
            gw = (gw_prev + c_awet) / d1
            ev = np.minimum(pet[i], np.maximum(0, y - sm))
            sm = y - ev
            aet[i], sav[i], q[i] = ev, sm, (awet - c_awet) + d * gw
            sm_prev, gw_prev = sm, gw
    return aet.T, q.T, sav.T


def bar_excess(x, ref):
    """max over the array of |x - ref| / (1e-9 |ref| + 1e-9): the stage tests' bar is 1."""
    x, ref = np.asarray(x, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    ok = np.isfinite(ref)
    return float(np.max(np.abs(x[ok] - ref[ok]) / (1e-9 * np.abs(ref[ok]) + 1e-9)))
