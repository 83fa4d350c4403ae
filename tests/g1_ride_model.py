"""Integer model of the G1 round's ride (drand_amd/csrc/h2c.hpp fp_sqrt_ride, g1_sum_pre, g1_sum_post, iso11_aff and
codec.hpp g1_decompress_ride), product by product in the header's order, on Python integers mod p. Every field product
goes through Counter.mul / Counter.sqr, so a test can pin the number the device code spends.

The SSWU map itself is not restated: sswu_parts returns the oracle's affine point as the header's (xn, xd, y) with a
denominator of the caller's choice, which is all the sum's formulas can see of it."""
import bls_py as B

p = B.P
E_RIDE = (p - 3) // 4  # SCHED_SR1_C1's exponent


class Counter:
    def __init__(self):
        self.n = 0

    def mul(self, a, b):
        self.n += 1
        return a * b % p

    def sqr(self, a):
        self.n += 1
        return a * a % p


def chain(t):
    """fp_pow_sched(t, SCHED_SR1_C1): the squarings and dictionary products of the chain are not counted here (they are
    the chain the signature decode runs anyway)."""
    return pow(t, E_RIDE, p)


def fp_sqrt_ride(K, a, c):
    """-> (is_square, y, inv_c)"""
    ac = K.mul(a, c)
    w = chain(K.mul(ac, c))
    y = K.mul(w, ac)
    ic = K.mul(K.sqr(w), ac)
    qr = K.sqr(y) == a % p
    return qr, y, ic if qr else (-ic) % p


def sswu_parts(u, xd=1):
    """The header's swu_out of u: x = xn / xd, y affine (the oracle's point, its x spread over a denominator)."""
    x, y = B.sswu_g1(u)
    return (x * xd % p, xd % p, y)


def g1_sum_pre(K, p0, p1):
    """-> (distinct, mid, c) with mid = (N, A + B, A, (y1 - y0) D^2, y0)"""
    xn0, xd0, y0 = p0
    xn1, xd1, y1 = p1
    a = K.mul(xn0, xd1)
    b = K.mul(xn1, xd0)
    d = K.mul(xd0, xd1)
    n = (b - a) % p
    s = (b + a) % p
    c = K.mul(n, d)
    dyd2 = K.mul((y1 - y0) % p, K.sqr(d))
    return n != 0, (n, s, a, dyd2, y0), c


def g1_sum_post(K, mid, inv_c):
    n, s, a, dyd2, y0 = mid
    inv_d = K.mul(n, inv_c)
    lam = K.mul(dyd2, inv_c)
    x3 = (K.sqr(lam) - K.mul(s, inv_d)) % p
    y3 = (K.mul(lam, (K.mul(a, inv_d) - x3) % p) - y0) % p
    return x3, y3


def iso11_aff(K, pt, xnum, ynum, h, conv=None):
    """Jacobian image (x_num(x), y y_num(x), h(x)); conv counts the 12 x 32 <-> 28-bit conversion products."""
    x, y = pt
    if conv is not None:
        conv.n += 1  # X in
    xn, yn, hh = xnum[-1], ynum[-1], x
    assert h[-1] == 1
    for j in range(1, len(ynum)):
        yn = (K.mul(yn, x) + ynum[len(ynum) - 1 - j]) % p
        if j < len(xnum):
            xn = (K.mul(xn, x) + xnum[len(xnum) - 1 - j]) % p
        if j < len(h):
            hh = ((K.mul(hh, x) if j > 1 else hh) + h[len(h) - 1 - j]) % p
    if conv is not None:
        conv.n += 4  # Y in; X', Y', Z' out
    return xn, K.mul(y, yn), hh


def jac_affine(P3):
    X, Y, Z = P3
    if Z % p == 0:
        return None
    zi = pow(Z, -1, p)
    return (X * zi * zi % p, Y * zi ** 3 % p)


def decode_ride(K, sig, c):
    """g1_decompress_ride -> (status, point or None, inv_c); status 1 = decoded, 2 = the infinity encoding, 0 = bad.
    Every encoding runs the chain: one rejected before the root rides on a = 1."""
    flags = sig[0] >> 5
    x = int.from_bytes(bytes([sig[0] & 0x1F]) + bytes(sig[1:]), "big")
    if not flags & 4:
        pre = 0
    elif flags & 2:
        pre = 0 if (x or flags & 1) else 2
    else:
        pre = 1 if x < p else 0
    xs = x if pre == 1 else 0
    a = (K.mul(K.sqr(xs), xs) + B.B1) % p if pre == 1 else 1
    qr, y, inv_c = fp_sqrt_ride(K, a, c)
    if pre != 1:
        return pre, None, inv_c
    if not qr:
        return 0, None, inv_c
    if (y > B.HALF_P) != bool(flags & 1):
        y = (-y) % p
    return 1, (x, y), inv_c


def hash_point(u0, u1, xnum, ynum, h, sig=None, xd0=1, xd1=1, K=None, conv=None):
    """The round as the kernel runs it from u0, u1 on: -> (status, sigma, affine hash point or None for the identity).
    Without a signature the chain rides on the stand-in a = 1, as a rejected encoding does."""
    K = K or Counter()
    distinct, mid, c = g1_sum_pre(K, sswu_parts(u0, xd0), sswu_parts(u1, xd1))
    if not distinct:
        c = 1
    if sig is None:
        st, pt = 0, None
        _, _, inv_c = fp_sqrt_ride(K, 1, c)
    else:
        st, pt, inv_c = decode_ride(K, sig, c)
    if st != 1:
        st, pt = 0, None
    if not distinct:
        q0, q1 = B.iso_map_g1(B.sswu_g1(u0)), B.iso_map_g1(B.sswu_g1(u1))  # h2c_g1_map's exceptional order
        return st, pt, B.ec_add(B.FP, q0, q1)
    assert inv_c * c % p == 1
    return st, pt, jac_affine(iso11_aff(K, g1_sum_post(K, mid, inv_c), xnum, ynum, h, conv))
