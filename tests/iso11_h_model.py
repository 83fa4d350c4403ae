"""Integer model of the G1 hash's 11-isogeny in its kernel-polynomial form (drand_amd/csrc/h2c.hpp iso11_jac) and of the
limb-level Montgomery body under it (fp_mul28.hpp M28_BODY, mont_mul), for tests/test_iso11_h_model.py. Test infrastructure only.

Where tests/fp28_model.py models a product as the exact integer (a b + m p) / R', this model walks M28_BODY column by
column on 14 limbs, as the device does, and asserts what the device relies on: every 64-bit accumulator stays below
2^64, the low 28 bits of a reduced column vanish, the top limb fits 28 bits (normalised output) and the value is the
one fp28_model.mont gives (which asserts the < 2p result bound). Sums follow f28_lin<0> limb by limb with its int32
carry. iso11_h follows iso11_jac line by line and asserts the value bounds its comments state.
"""
import fp28_model as M

p, RP = M.p, M.RP
MASK = (1 << 28) - 1
N0 = 0x0ffcfffd  # -p^-1 mod 2^28
U64 = 1 << 64


def limbs(v):
    assert 0 <= v < RP
    return [(v >> (28 * i)) & MASK for i in range(14)]


def value(L):
    return sum(x << (28 * i) for i, x in enumerate(L))


PL = limbs(p)
assert (N0 * PL[0] + 1) & MASK == 0


def m28_body(col, normalised=True):
    """fp_mul28.hpp M28_BODY over the column sums col(k), k = 0..26; returns the 14 result limbs. normalised=False
    (operands beyond the value bound X Y < 2^392 p, to load the columns fully): the top limb need only fit its 32-bit
    word."""
    mq = [0] * 14
    out = [0] * 14
    acc = 0
    for k in range(14):
        acc += col(k)
        for i in range(k):
            acc += mq[i] * PL[k - i]
        mq[k] = (((acc & 0xFFFFFFFF) * N0) & 0xFFFFFFFF) & MASK
        acc += mq[k] * PL[0]
        assert acc < U64, "column %d leaves 64 bits" % k  # every term is >= 0: the final sum bounds the partial ones
        assert acc & MASK == 0
        acc >>= 28
    for k in range(14, 27):
        acc += col(k)
        for i in range(k - 13, 14):
            acc += mq[i] * PL[k - i]
        assert acc < U64, "column %d leaves 64 bits" % k
        out[k - 14] = acc & MASK
        acc >>= 28
    assert acc <= (MASK if normalised else 0xFFFFFFFF), "top limb not normalised"
    out[13] = acc
    return out


def _col(X, Y):
    return lambda k: sum(X[i] * Y[k - i] for i in range(max(k - 13, 0), min(k, 13) + 1))


def mont_mul_limbs(X, Y, normalised=True):
    return m28_body(_col(X, Y), normalised)


def mul(a, b):
    """f28_mul on values: normalised limbs in, M28_BODY, the value fp28_model.mont gives (< 2p) out."""
    r = value(mont_mul_limbs(limbs(a), limbs(b)))
    assert r == M.mont(a, b)
    return r


def add(a, b):
    """f28_add = f28_lin<0>(a, 1, b, 1): limb sums with one signed carry pass, every sum inside int32."""
    A, B = limbs(a), limbs(b)
    out, c = [], 0
    for i in range(14):
        t = A[i] + B[i] + c
        assert -(1 << 31) <= t < (1 << 31)
        out.append(t & MASK)
        c = t >> 28
    assert c == 0, "sum leaves 2^392"
    assert value(out) == a + b
    return a + b


def below(v, k):
    assert 0 <= v < k * p, v / p
    return v


def iso11_h_core(X, Y, Zp, xnum, ynum, h):
    """iso11_jac between its conversions: X, Y, Zp are 28-bit-form values < 2p; coefficient lists low degree first,
    normal field elements, h monic of degree 5. Returns (X', Y', Z') as 28-bit-form values (< 4p, < 2p, < 2p)."""
    c = lambda v: v * RP % p  # noqa: E731
    assert h[-1] == 1 and len(h) == 6 and len(xnum) == 12 and len(ynum) == 16
    for v in (X, Y, Zp):
        below(v, 2)
    D = below(mul(Zp, Zp), 2)
    xn, yn, hh, zp = c(xnum[-1]), c(ynum[-1]), X, D
    step = lambda acc, co: below(add(below(mul(acc, X), 2), below(mul(co, zp), 2)), 4)  # noqa: E731
    for j in range(1, len(ynum)):
        if j > 1:
            zp = below(mul(zp, D), 2)
        yn = step(yn, c(ynum[-1 - j]))
        if j < len(xnum):
            xn = step(xn, c(xnum[-1 - j]))
        if j < len(h):
            if j > 1:
                hh = step(hh, c(h[-1 - j]))
            else:  # the leading coefficient is 1: X + c_4 D, no product by it
                hh = below(add(hh, below(mul(c(h[-1 - j]), zp), 2)), 4)
    return below(xn, 4), below(mul(Y, yn), 2), below(mul(Zp, hh), 2)


def from_fp(v):
    return mul(v, pow(2, 400, p))  # f28_from_fp on the stored 12 x 32-bit value (< p): < 2p


def to_fp(a):
    """f28_to_fp: one product by 2^384 mod p (any a < 4p gives < 2p), then the final subtraction."""
    o = mul(a, M.R % p)
    return o - p if o >= p else o


def iso11_h(X32, Y32, Z32, xnum, ynum, h):
    """iso11_jac on a Jacobian point in 12 x 32-bit Montgomery form (canonical values x 2^384 mod p); the same form out."""
    xo, yo, zo = iso11_h_core(from_fp(X32), from_fp(Y32), from_fp(Z32), xnum, ynum, h)
    return to_fp(xo), to_fp(yo), to_fp(zo)


# ---- polynomials over Fp (coefficient lists, low degree first) for the identities the map rests on
def poly_mul(a, b):
    r = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            r[i + j] = (r[i + j] + x * y) % p
    return r


def poly_trim(a):
    a = [x % p for x in a]
    while a and a[-1] == 0:
        a.pop()
    return a


def poly_mod(a, m):
    a = poly_trim(a)
    inv = pow(m[-1], -1, p)
    while len(a) >= len(m):
        q = a[-1] * inv % p
        s = len(a) - len(m)
        for i, x in enumerate(m):
            a[s + i] = (a[s + i] - q * x) % p
        a = poly_trim(a)
    return a


def poly_gcd(a, b):
    a, b = poly_trim(a), poly_trim(b)
    while b:
        a, b = b, poly_mod(a, b)
    inv = pow(a[-1], -1, p)
    return [x * inv % p for x in a]


def monic_sqrt(f):
    """the monic polynomial h with h^2 = f's top half of coefficients (the caller checks h^2 == f)"""
    d = (len(f) - 1) // 2
    h = [0] * d + [1]
    inv2 = (p + 1) // 2
    for k in range(1, d + 1):
        s = sum(h[i] * h[2 * d - k - i] for i in range(d - k + 1, d)) % p
        h[d - k] = (f[2 * d - k] - s) * inv2 % p
    return h


def roots_in_fp(h):
    """gcd(h, x^p - x): the product of (x - r) over h's roots r in Fp"""
    acc, base, e = [1], [0, 1], p
    while e:
        if e & 1:
            acc = poly_mod(poly_mul(acc, base), h)
        base = poly_mod(poly_mul(base, base), h)
        e >>= 1
    xp_minus_x = acc + [0] * (2 - len(acc)) if len(acc) < 2 else list(acc)
    xp_minus_x[1] = (xp_minus_x[1] - 1) % p
    g = poly_trim(xp_minus_x)
    return poly_gcd(h, g) if g else list(h)


def a_root(g, rng):
    """one root of g, a product of distinct linear factors over Fp (roots_in_fp's result), by equal-degree splitting:
    gcd(g, (x + a)^((p - 1) / 2) - 1) for random a separates the roots r by the quadratic character of r + a"""
    g = poly_trim(g)
    while len(g) > 2:
        acc, base, e = [1], poly_mod([rng.randrange(p), 1], g), (p - 1) // 2
        while e:
            if e & 1:
                acc = poly_mod(poly_mul(acc, base), g)
            base = poly_mod(poly_mul(base, base), g)
            e >>= 1
        acc = poly_trim([(acc[0] - 1) % p] + acc[1:]) if acc else [p - 1]
        if not acc:
            continue
        d = poly_gcd(g, acc)
        if 1 < len(d) < len(g):
            g = d
    return (-g[0]) * pow(g[1], -1, p) % p
