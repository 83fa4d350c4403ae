"""drand_amd/csrc/fp_mul30.hpp restated line by line on Python integers: the Montgomery product and squaring on 13 signed
30-bit digits (radix 2^390), the entry from and the exit to 12 x 32-bit words, and the constants the header writes out.
Every accumulation asserts |acc| < 2^63 (the device accumulator is an int64_t), the quotient columns assert that they
shift exactly, and every 32-bit intermediate asserts its range. tests/test_fp30_model.py drives it."""

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
N = 13
BITS = 30
MASK = (1 << BITS) - 1
HALF = 1 << (BITS - 1)
RADIX = 1 << (BITS * N)  # 2^390


def centred(v):
    """v -> 12 digits in [-2^29, 2^29) and the rest as the top digit"""
    d = []
    for _ in range(N - 1):
        r = v & MASK
        if r >= HALF:
            r -= 1 << BITS
        d.append(r)
        v = (v - r) >> BITS
    d.append(v)
    return d


def value(d):
    return sum(x << (BITS * i) for i, x in enumerate(d))


# the header's constants, derived
P_DIGITS = centred(P)
N0 = (-pow(P, -1, 1 << BITS)) % (1 << BITS)
K_IN = centred(pow(2, BITS * N + 6, P))  # x 2^384 -> x 2^390 through one product: 2^(390 + 6)
K_OUT = centred(pow(2, 384, P))          # x 2^390 -> x 2^384


def sext30(v):
    v &= MASK
    return v - (1 << BITS) if v >= HALF else v


def i32(v):
    assert -(1 << 31) <= v < 1 << 31, v
    return v


class Acc:
    """the int64_t column accumulator"""

    def __init__(self):
        self.v = 0
        self.peak = 0

    def mad(self, a, b):
        i32(a), i32(b)
        self.v += a * b
        self.check()

    def check(self):
        assert -(1 << 63) <= self.v < 1 << 63, self.v
        self.peak = max(self.peak, abs(self.v))


def _body(col, stats=None):
    """M30_BODY over the column sums col(k, acc)"""
    Mq = [0] * N
    R = [0] * N
    acc = Acc()
    for k in range(N):
        col(k, acc)
        for i in range(k):
            acc.mad(Mq[i], P_DIGITS[k - i])
        Mq[k] = sext30(((acc.v & 0xFFFFFFFF) * N0) & 0xFFFFFFFF)
        acc.mad(Mq[k], P_DIGITS[0])
        assert acc.v & MASK == 0, "a quotient column must shift exactly"
        acc.v >>= BITS
    for k in range(N, 2 * N - 1):
        col(k, acc)
        for i in range(k - (N - 1), N):
            acc.mad(Mq[i], P_DIGITS[k - i])
        R[k - N] = sext30(acc.v & 0xFFFFFFFF)
        acc.v += HALF
        acc.check()
        acc.v >>= BITS
    R[N - 1] = i32(acc.v)
    if stats is not None:
        stats["peak"] = max(stats.get("peak", 0), acc.peak)
    return R


def mont_mul(X, Y, stats=None):
    def col(k, acc):
        for i in range(max(0, k - (N - 1)), min(k, N - 1) + 1):
            acc.mad(X[i], Y[k - i])
    return _body(col, stats)


def mont_sqr(X, stats=None):
    X2 = [i32(x + x) for x in X]

    def col(k, acc):
        i = max(0, k - (N - 1))
        while 2 * i < k:
            acc.mad(X[i], X2[k - i])
            i += 1
        if k % 2 == 0:
            acc.mad(X[k // 2], X[k // 2])
    return _body(col, stats)


def words(v):
    assert 0 <= v < 1 << 384
    return [(v >> (32 * j)) & 0xFFFFFFFF for j in range(12)]


def slice_words(x):
    """m30::slice: 12 words -> centred digits of the same value"""
    L = [0] * N
    c = 0
    for i in range(N):
        b = BITS * i
        w, o = b >> 5, b & 31
        two = x[w] | ((x[w + 1] << 32) if w + 1 < 12 else 0)
        t = (((two >> o) & 0xFFFFFFFF) & MASK) + c
        assert t <= 1 << BITS
        c = ((t + HALF) >> BITS) if i < N - 1 else 0
        assert t + HALF < 1 << 32
        L[i] = i32(t - (c << BITS))
    return L


def unslice(A):
    """m30::unslice: centred digits of a value in (-p, p) -> 12 words of its residue in [0, p)"""
    c = 0
    for i in range(N):
        c = i32(A[i] + c) >> BITS
    assert c in (0, -1)
    neg = c
    U = [0] * N
    c = 0
    for i in range(N):
        t = i32(A[i] + (P_DIGITS[i] if neg else 0) + c)
        U[i] = t & MASK
        c = t >> BITS
    assert c == 0
    r = [0] * 12
    for j in range(12):
        b = 32 * j
        i, o = b // BITS, b % BITS
        v = U[i] >> o
        if i + 1 < N:
            v |= U[i + 1] << (BITS - o)
        if i + 2 < N and 2 * BITS - o < 32:
            v |= U[i + 2] << (2 * BITS - o)
        r[j] = v & 0xFFFFFFFF
    assert value(U) >> 384 == 0
    return r


def enter(x, stats=None):
    """m30::from on the integer x (the 12-word Montgomery value)"""
    return mont_mul(slice_words(words(x)), K_IN, stats)


def leave(A, stats=None):
    """m30::to, as an integer"""
    r = unslice(mont_mul(A, K_OUT, stats))
    return sum(w << (32 * j) for j, w in enumerate(r))
