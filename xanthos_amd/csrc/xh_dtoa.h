// double -> the characters of Python's repr(float) (sys.float_repr_style == 'short'), for the host and the device.
//
// Digits: Schubfach (R. Giulietti, "The Schubfach way to render doubles", 2020), written from the paper: the shortest
// decimal that reads back as the same double; of several of that length the closest one, a remaining tie to the even
// digit.  One pass of integer arithmetic on a 128-bit power of ten, no retry, no printf.  Layout: float_repr_style 'short'
// (fixed notation iff -4 <= e10 < 16, e10 the decimal exponent of the first digit; otherwise d[.ddd]e+XX), NaN as the EMPTY
// field, which is how pandas' to_csv and data_writer/out_writer.py write it.  The longest field is 24 characters
// (-1.2345678901234567e-308).
//
// The table of powers of ten (617 entries of 128 bits) is not written down: xh_dtoa_build_table computes it with exact
// multi-word integer arithmetic.  The host keeps one copy (xh_dtoa_host_table), the library uploads one per context.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XH_DTOA_HD __host__ __device__ inline
#else
#define XH_DTOA_HD inline
#endif

#define XH_DTOA_MAX_LEN 24
#define XH_DTOA_POW10_MIN (-292)
#define XH_DTOA_POW10_MAX 324
#define XH_DTOA_POW10_COUNT (XH_DTOA_POW10_MAX - XH_DTOA_POW10_MIN + 1)      // 617
#define XH_DTOA_TABLE_WORDS (2 * XH_DTOA_POW10_COUNT)                          // uint64: {high, low} per entry

// ---- the table: entry n (XH_DTOA_POW10_MIN <= n <= XH_DTOA_POW10_MAX) is g = ceil(10^n * 2^s), s such that 2^127 <= g < 2^128
// (exact where 10^n fits 128 bits, floor + 1 elsewhere: Schubfach's g of section 9.1, left-aligned).
inline void xh_dtoa_top128(const uint64_t *w, int nwords, bool round_up_inexact, bool always_plus_one, uint64_t *out) {
    int top = nwords - 1;
    while (top > 0 && w[top] == 0) --top;
    int lz = 0;
    while (!((w[top] << lz) >> 63)) ++lz;
    auto word = [&](int i) -> uint64_t { return i >= 0 ? w[i] : 0; };
    auto shifted = [&](int i) -> uint64_t {      // bits of the number from word i downwards, shifted left by lz
        return lz ? (word(i) << lz) | (word(i - 1) >> (64 - lz)) : word(i);
    };
    uint64_t hi = shifted(top), lo = shifted(top - 1);
    bool rest = (uint64_t)(word(top - 2) << lz) != 0;
    for (int i = top - 3; i >= 0 && !rest; --i) rest = w[i] != 0;
    if (always_plus_one || (round_up_inexact && rest)) {
        if (++lo == 0) ++hi;
    }
    out[0] = hi;
    out[1] = lo;
}

inline void xh_dtoa_build_table(uint64_t *table /* [XH_DTOA_TABLE_WORDS] */) {
    constexpr int W = 20;                                    // 1280 bits: 10^324 has 1077, the quotients start from 2^1279
    uint64_t big[W];
    // n >= 0: 10^n exactly, its leading 128 bits rounded up
    for (int i = 0; i < W; ++i) big[i] = 0;
    big[0] = 1;
    for (int n = 0; n <= XH_DTOA_POW10_MAX; ++n) {
        xh_dtoa_top128(big, W, true, false, table + 2 * (n - XH_DTOA_POW10_MIN));
        uint64_t carry = 0;
        for (int i = 0; i < W; ++i) {
            const unsigned __int128 p = (unsigned __int128)big[i] * 10u + carry;
            big[i] = (uint64_t)p;
            carry = (uint64_t)(p >> 64);
        }
    }
    // n < 0: floor(2^S / 10^m) for m = 1, 2, ... by dividing by ten again and again (floor(floor(x / a) / b) == floor(x / (a b))),
    // its leading 128 bits are floor(2^s / 10^m); never exact, so + 1
    for (int i = 0; i < W; ++i) big[i] = 0;
    big[W - 1] = (uint64_t)1 << 63;
    for (int m = 1; m <= -XH_DTOA_POW10_MIN; ++m) {
        uint64_t rem = 0;
        for (int i = W - 1; i >= 0; --i) {
            const unsigned __int128 cur = ((unsigned __int128)rem << 64) | big[i];
            big[i] = (uint64_t)(cur / 10u);
            rem = (uint64_t)(cur % 10u);
        }
        xh_dtoa_top128(big, W, false, true, table + 2 * (-m - XH_DTOA_POW10_MIN));
    }
}

inline const uint64_t *xh_dtoa_host_table() {
    static const struct Table {
        uint64_t w[XH_DTOA_TABLE_WORDS];
        Table() { xh_dtoa_build_table(w); }
    } t;
    return t.w;
}

// ---- digits
XH_DTOA_HD uint64_t xh_dtoa_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// floor(log10(2^e)), floor(log10(3/4 * 2^e)), floor(log2(10^e)): exact for the exponents a double gives (|e| <= 1233)
XH_DTOA_HD int xh_dtoa_flog10_pow2(int e) { return (int)(((int64_t)e * 1262611) >> 22); }
XH_DTOA_HD int xh_dtoa_flog10_34pow2(int e) { return (int)(((int64_t)e * 1262611 - 524031) >> 22); }
XH_DTOA_HD int xh_dtoa_flog2_pow10(int e) { return (int)(((int64_t)e * 1741647) >> 19); }

// the leading 64 bits of g * cp (g of 128 bits, cp < 2^64 such that the product is below 2^128 * 2^64 / 2^64), the bits below
// folded into the lowest one: enough to compare against every multiple of 1/2 (Schubfach section 9.4, "round to odd")
XH_DTOA_HD uint64_t xh_dtoa_round_to_odd(uint64_t ghi, uint64_t glo, uint64_t cp) {
    const uint64_t x1 = xh_dtoa_mulhi(glo, cp);
    const uint64_t y0 = ghi * cp;
    const uint64_t y1 = xh_dtoa_mulhi(ghi, cp);
    const uint64_t z = y0 + x1;
    return (y1 + (z < y0)) | (uint64_t)(z > 1);
}

enum { XH_DTOA_FINITE = 0, XH_DTOA_ZERO = 1, XH_DTOA_INF = 2, XH_DTOA_NAN = 3 };

struct xh_repr {
    uint64_t digits;      // the decimal digits as an integer, no trailing zero (XH_DTOA_FINITE only)
    int ndig;             // how many
    int e10;              // decimal exponent of the first digit: value = d.ddd x 10^e10
    int kind;
    bool neg;
};

XH_DTOA_HD int xh_dtoa_count_digits(uint64_t v) {      // v < 10^17
    int n = 1;
    if (v >= 10000000000000000ull) return 17;
    if (v >= 100000000ull) { v /= 100000000ull; n += 8; }
    if (v >= 10000ull) { v /= 10000ull; n += 4; }
    if (v >= 100ull) { v /= 100ull; n += 2; }
    if (v >= 10ull) n += 1;
    return n;
}

XH_DTOA_HD xh_repr xh_dtoa_repr(double value, const uint64_t *pow10) {
    union { double d; uint64_t u; } pun;
    pun.d = value;
    const uint64_t bits = pun.u;
    const uint64_t frac = bits & 0x000FFFFFFFFFFFFFull;
    const int bexp = (int)((bits >> 52) & 0x7FF);
    xh_repr r;
    r.digits = 0;
    r.ndig = 1;
    r.e10 = 0;
    r.neg = (bits >> 63) != 0;
    if (bexp == 0x7FF) {
        r.kind = frac ? XH_DTOA_NAN : XH_DTOA_INF;
        return r;
    }
    if (bexp == 0 && frac == 0) {
        r.kind = XH_DTOA_ZERO;
        return r;
    }
    r.kind = XH_DTOA_FINITE;
    // value = c * 2^q
    const uint64_t c = bexp ? (frac | 0x0010000000000000ull) : frac;
    const int q = bexp ? bexp - 1075 : -1074;
    const bool even = (c & 1) == 0;                       // the rounding interval is closed iff c is even
    const bool narrow = frac == 0 && bexp > 1;            // a power of two: the interval's lower half is half as wide
    const uint64_t cbl = 4 * c - 2 + (narrow ? 1 : 0);
    const uint64_t cb = 4 * c;
    const uint64_t cbr = 4 * c + 2;
    const int k = narrow ? xh_dtoa_flog10_34pow2(q) : xh_dtoa_flog10_pow2(q);
    const int h = q + xh_dtoa_flog2_pow10(-k) + 1;        // 1 .. 4
    const uint64_t ghi = pow10[2 * (-k - XH_DTOA_POW10_MIN)], glo = pow10[2 * (-k - XH_DTOA_POW10_MIN) + 1];
    const uint64_t vbl = xh_dtoa_round_to_odd(ghi, glo, cbl << h);
    const uint64_t vb = xh_dtoa_round_to_odd(ghi, glo, cb << h);
    const uint64_t vbr = xh_dtoa_round_to_odd(ghi, glo, cbr << h);
    const uint64_t lower = vbl + (even ? 0 : 1);
    const uint64_t upper = vbr - (even ? 0 : 1);
    const uint64_t s = vb >> 2;                           // floor(value / 10^k)
    uint64_t dig = 0;
    int e = k;
    bool done = false;
    if (s >= 10) {                                        // a multiple of 10^(k + 1) inside the interval is shorter
        const uint64_t sp = s / 10;
        const bool up_in = lower <= 40 * sp;
        const bool wp_in = 40 * sp + 40 <= upper;
        if (up_in != wp_in) {
            dig = sp + (wp_in ? 1 : 0);
            e = k + 1;
            done = true;
        }
    }
    if (!done) {
        const bool u_in = lower <= 4 * s;
        const bool w_in = 4 * s + 4 <= upper;
        if (u_in != w_in) {
            dig = s + (w_in ? 1 : 0);
        } else {                                          // both or neither: the closer one, a tie to the even one
            const uint64_t mid = 4 * s + 2;
            const bool up = vb > mid || (vb == mid && (s & 1));
            dig = s + (up ? 1 : 0);
        }
    }
    if (dig % 100000000ull == 0) { dig /= 100000000ull; e += 8; }
    if (dig % 10000ull == 0) { dig /= 10000ull; e += 4; }
    if (dig % 100ull == 0) { dig /= 100ull; e += 2; }
    while (dig % 10ull == 0) { dig /= 10ull; e += 1; }
    r.digits = dig;
    r.ndig = xh_dtoa_count_digits(dig);
    r.e10 = e + r.ndig - 1;
    return r;
}

// ---- layout
XH_DTOA_HD int xh_dtoa_len(const xh_repr &r) {
    if (r.kind == XH_DTOA_NAN) return 0;
    const int sign = r.neg ? 1 : 0;
    if (r.kind != XH_DTOA_FINITE) return sign + 3;                               // 0.0, inf
    const int n = r.ndig, e = r.e10;
    if (e >= 0 && e < 16) return sign + (n > e + 1 ? n + 1 : e + 3);              // ddd.ddd | ddd000.0
    if (e < 0 && e >= -4) return sign + 1 - e + n;                                // 0.000ddd
    const int a = e < 0 ? -e : e;
    return sign + n + (n > 1 ? 1 : 0) + 2 + (a >= 100 ? 3 : 2);                   // d[.ddd]e+XX
}

// writes xh_dtoa_len(r) characters at out, returns that length
XH_DTOA_HD int xh_dtoa_put(const xh_repr &r, char *out) {
    if (r.kind == XH_DTOA_NAN) return 0;
    char *p = out;
    if (r.neg) *p++ = '-';
    if (r.kind == XH_DTOA_ZERO) {
        p[0] = '0'; p[1] = '.'; p[2] = '0';
        return (int)(p - out) + 3;
    }
    if (r.kind == XH_DTOA_INF) {
        p[0] = 'i'; p[1] = 'n'; p[2] = 'f';
        return (int)(p - out) + 3;
    }
    const int n = r.ndig, e = r.e10;
    uint64_t dig = r.digits;
    int first, point;      // digit i goes to p[first + i + (i >= point)]
    int len;
    if (e >= 0 && e < 16) {
        first = 0;
        point = e + 1;
        for (int i = n; i < point; ++i) p[i] = '0';
        p[point] = '.';
        if (n <= point) p[point + 1] = '0';
        len = n > point ? n + 1 : point + 2;
    } else if (e < 0 && e >= -4) {
        p[0] = '0';
        p[1] = '.';
        for (int i = 0; i < -e - 1; ++i) p[2 + i] = '0';
        first = 1 - e;
        point = 32;
        len = first + n;
    } else {
        first = 0;
        point = 1;
        char *x = p + n + (n > 1 ? 1 : 0);
        if (n > 1) p[1] = '.';
        int a = e < 0 ? -e : e;
        *x++ = 'e';
        *x++ = e < 0 ? '-' : '+';
        if (a >= 100) { *x++ = (char)('0' + a / 100); a %= 100; }
        *x++ = (char)('0' + a / 10);
        *x++ = (char)('0' + a % 10);
        len = (int)(x - p);
    }
    for (int i = n - 1; i >= 0; --i) {
        p[first + i + (i >= point ? 1 : 0)] = (char)('0' + (int)(dig % 10));
        dig /= 10;
    }
    return (int)(p - out) + len;
}

// decimal digits of a non-negative integer (the id column)
XH_DTOA_HD int xh_dtoa_id_len(uint64_t v) {
    int n = 1;
    while (v >= 10) { v /= 10; ++n; }
    return n;
}
XH_DTOA_HD int xh_dtoa_id_put(uint64_t v, char *out) {
    const int n = xh_dtoa_id_len(v);
    for (int i = n - 1; i >= 0; --i) {
        out[i] = (char)('0' + (int)(v % 10));
        v /= 10;
    }
    return n;
}
