"""GWAM (xanthos/runoff/gwam.py:runoffgen, :18-88) restated in numpy with boolean masks, in float64 or long double.

``month`` is one call of runoffgen: the index sets (water bodies, no soil, B >= Sm, B < Sm; a NaN B or Sm matches none and
leaves zeros), the operation order of the original, and a record of every decision taken per cell.  ``series`` is the
reference driver's two passes (components.py:298-357): the spin-up pass, then the simulation, each reading one
precipitation column for all its months (``monthly=False``, the reference) or month m's column in month m.

The dtype is a parameter: np.float64 is the restatement the device kernel is held to in bits where no ``exp`` is taken;
np.longdouble (x86 extended, 64 mantissa bits) is the truth the tolerance tests measure against.  ``expf`` replaces
``np.exp`` (the tests move it by one ulp to see what an ``exp`` that rounds the other way does to a march).

np.minimum / np.maximum are spelled as selects with their scalar semantics (the first argument wins ties and NaN, a NaN
second argument is returned): numpy's vector loops may return either zero of a (+0, -0) tie, the selects may not.
"""
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, 'long double must be x86 extended precision (64-bit mantissa) or wider'

# decision record: kind + the partial branch's five decisions as bits
NOSOIL, LAKE, NANB, FULL, PART = 0, 1, 2, 3, 4        # Sm == 0 | Sm == indexing | NaN B or Sm | B >= Sm | B < Sm
T5_GE1, T5_LE01, A_TMP3, S_SM, S_LE0 = 8, 16, 32, 64, 128
KIND_MASK = 7
KIND_NAMES = {NOSOIL: 'nosoil', LAKE: 'lake', NANB: 'nan', FULL: 'full', PART: 'part'}


def describe(code):
    s = KIND_NAMES[code & KIND_MASK]
    for bit, name in ((T5_GE1, 'tmp5>=1'), (T5_LE01, 'tmp5<=0.1'), (A_TMP3, 'tmp3<=tmp7'), (S_SM, 'Sm<=tmp8'), (S_LE0, 'Sav<=0')):
        if code & bit:
            s += '+' + name
    return s


def _min(a, b):
    return np.where((a <= b) | (a != a), a, b)


def _max(a, b):
    return np.where((a >= b) | (a != a), a, b)


def exp_ulp(k):
    """np.exp moved k (-1, 0, 1) ulp."""
    if not k:
        return np.exp
    return lambda v: np.nextafter(np.exp(v), np.asarray(np.inf if k > 0 else -np.inf, dtype=v.dtype))


def month(pet, p, sm, ch, dtype=np.float64, expf=None, indexing=999.0):
    """One month for every cell.  Returns (aet, q, sav, rec); rec.code is the decision record, rec.gap_b = |B - Sm| on soil
    and rec.gap_8 = |tmp8| where AET took tmp7 (the distances to GWAM's two discontinuities; inf elsewhere)."""
    T = dtype
    pet, p, sm, ch = [np.asarray(a, dtype=T) for a in (pet, p, sm, ch)]
    expf = expf or np.exp
    aet, q, sav = np.zeros_like(pet), np.zeros_like(pet), np.zeros_like(pet)
    code = np.zeros(pet.shape, dtype=np.int32)
    gap_b = np.full(pet.shape, np.inf, dtype=T)
    gap_8 = np.full(pet.shape, np.inf, dtype=T)
    with np.errstate(all='ignore'):
        B = ch + p - pet
        lake = sm == T(indexing)
        soil = (sm != 0) & ~lake
        full = soil & (B >= sm)
        part = soil & (B < sm)
        code[lake], code[soil], code[full], code[part] = LAKE, NANB, FULL, PART
        gap_b[full | part] = np.abs(B - sm)[full | part]
        d = p - pet
        q[lake] = np.where(d[lake] > 0, d[lake], T(0))                   # np.maximum(0, d), NaN -> 0
        a = _min(p[lake], pet[lake])
        aet[lake] = np.where(np.isnan(a), pet[lake], a)
        q[full], sav[full], aet[full] = B[full] - sm[full], sm[full], pet[full]
        c, pp, e, s = ch[part], p[part], pet[part], sm[part]
        x = c / s
        t3 = c + pp
        t5 = (T(5) * c / s - T(2) * (x * x)) / T(3)
        t6 = _min(np.ones_like(t5), t5)
        t7 = e * _max(T(0.1) * np.ones_like(t6), t6)
        a = _min(t3, t7)
        t8 = c * (T(1) - expf(-x)) / (T(1) - np.exp(T(-1))) + (pp - a)
        sv = _min(s, t8)
        low = sv <= 0
        b = np.full(c.shape, PART, dtype=np.int32)
        b[t5 >= 1] |= T5_GE1
        b[t5 <= T(0.1)] |= T5_LE01
        b[(t3 <= t7) | (t3 != t3)] |= A_TMP3
        b[(s <= t8) | (s != s)] |= S_SM
        b[low] |= S_LE0
        code[part] = b
        # tmp8 = 0 is a discontinuity only where AET took tmp7 (otherwise both sides give AET = ch + P, Q = 0).  With
        # PET == 0 exactly and ch, P >= 0, tmp7 is 0 exactly and tmp8 is a sum of non-negative terms in every precision:
        # its sign is decided by the inputs, not by rounding, however small it is
        fixed = (e == 0) & (pp >= 0) & (c >= 0)
        gap_8[part] = np.where(((b & A_TMP3) == 0) & ~fixed, np.abs(t8), T(np.inf))
        sv, a = sv.copy(), a.copy()
        sv[low] = 0
        a[low] = pp[low] + c[low]
        aet[part], sav[part], q[part] = a, sv, _max(np.zeros_like(a), c + pp - a - sv)
    return aet, q, sav, SimpleNamespace(code=code, gap_b=gap_b, gap_8=gap_8)


def series(pet, precip, sm, sm0, spinup, monthly, dtype=np.float64, expf=None, indexing=999.0):
    """Spin-up pass (months [0, spinup)), then the simulation from the spin-up's end state.  Returns
    (aet, q, sav, rec): [ncell, nmonths] of the simulation pass; rec.code / rec.gap_b / rec.gap_8 as in ``month`` for the
    simulation, rec.sm_end the last state, rec.near the smallest gap a cell met in either pass."""
    T = dtype
    nc, nm = pet.shape
    st = np.asarray(sm0, dtype=T).copy()
    out = [np.zeros((nc, nm), dtype=T) for _ in range(3)]
    code = np.zeros((nc, nm), dtype=np.int32)
    gaps = [np.full((nc, nm), np.inf, dtype=T) for _ in range(2)]
    near = [np.full(nc, np.inf, dtype=T) for _ in range(2)]
    spin_codes = []
    for steps in (spinup, nm):
        for m in range(steps):
            a, q, s, r = month(pet[:, m], precip[:, m] if monthly else precip[:, steps - 1], sm, st, T, expf, indexing)
            for g, v in zip(near, (r.gap_b, r.gap_8)):
                np.minimum(g, np.where(v == 0, T(np.inf), v), out=g)     # an exact tie is structural, not "near"
            if steps == nm:
                out[0][:, m], out[1][:, m], out[2][:, m], code[:, m] = a, q, s, r.code
                gaps[0][:, m], gaps[1][:, m] = r.gap_b, r.gap_8
            else:
                spin_codes.append(r.code)
            st = s
    rec = SimpleNamespace(code=code, gap_b=gaps[0], gap_8=gaps[1], sm_end=st, near_b=near[0], near_8=near[1],
                          spin_code=np.array(spin_codes).T if spin_codes else np.zeros((nc, 0), dtype=np.int32))
    return out[0], out[1], out[2], rec


def worst_error(x, truth, scale, keep=None):
    """max |x - truth| / scale over the finite values of the truth (cells ``keep`` only).  What is not finite in the truth
    must be matched exactly: the same NaN mask and the same infinities."""
    x, truth = np.asarray(x), np.asarray(truth)
    sc = np.broadcast_to(scale[:, None] if truth.ndim == 2 else scale, truth.shape)
    if keep is not None:
        x, truth, sc = x[keep], truth[keep], sc[keep]
    assert np.array_equal(np.isnan(x), np.isnan(truth)), 'NaN masks differ'
    inf = np.isinf(truth)
    assert np.array_equal(np.isinf(x), inf) and np.array_equal(x[inf] > 0, truth[inf] > 0), 'infinities differ'
    fin = np.isfinite(truth)
    if not fin.any():
        return 0.0
    return float((np.abs(x[fin].astype(LD) - truth[fin]) / sc[fin]).max())


def same_bits(x, y):
    """Equal bit for bit, the sign of zero included; a NaN equals any NaN (its sign and payload depend on the hardware
    that made it)."""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and bool(np.all((x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))))

