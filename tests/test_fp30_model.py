"""CPU: the signed 30-bit Montgomery body of drand_amd/csrc/fp_mul30.hpp on Python integers (tests/fp30_model.py, which
asserts |acc| < 2^63 at every accumulation and the exact shift of every quotient column). Checked here, for every
product and squaring: output digits in [-2^29, 2^29) except the top one, value = X Y 2^-390 (mod p), and
|value| <= |X||Y| / 2^390 + p / 2; on the extreme digit patterns, mixed signs, 0, +-1, +-(p-1)/2 and 200 random pairs
each followed by 60 dependent operations (squarings, a product every fifth) whose values must stay below 0.51 p. The
entry is checked from 12-word inputs, the exit on negative, zero and positive chain values, and the header's p digits,
N0 and conversion constants are parsed out of the source and compared with what the model derives."""
import os
import random
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp30_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = M.P
RINV = pow(M.RADIX, -1, P)
LO, HI = -(1 << 29), (1 << 29) - 1


def check_op(X, Y, R):
    for d in R[:-1]:
        assert LO <= d <= HI, d
    x, y, r = M.value(X), M.value(Y), M.value(R)
    assert (r - x * y * RINV) % P == 0
    assert abs(r) * M.RADIX <= abs(x) * abs(y) + P * (M.RADIX >> 1), (x, y, r)
    return r


def mul(X, Y, stats=None):
    R = M.mont_mul(X, Y, stats)
    check_op(X, Y, R)
    return R


def sqr(X, stats=None):
    R = M.mont_sqr(X, stats)
    check_op(X, X, R)
    assert R == M.mont_mul(X, X)
    return R


def test_extreme_and_special_operands():
    lo, hi = [LO] * M.N, [HI] * M.N
    mixed = [LO if i % 2 else HI for i in range(M.N)]
    mixed2 = [HI if i % 3 else LO for i in range(M.N)]
    half = (P - 1) // 2
    special = [lo, hi, mixed, mixed2, M.centred(0), M.centred(1), M.centred(-1), M.centred(half), M.centred(-half)]
    stats = {}
    for X in special:
        sqr(X, stats)
        for Y in special:
            mul(X, Y, stats)
    # the largest column: 13 + 13 terms of at most 2^58 and a carry-in
    assert stats["peak"] < 26 * (1 << 58) + (1 << 35) < 1 << 63
    # a chain value stays a chain value: |v| < 0.51 p in, |v| < 0.51 p out, small top digit
    for X in (M.centred(half), M.centred(-half), M.centred(1), M.centred(0)):
        for Y in (M.centred(half), M.centred(-half), M.centred(-1)):
            R = mul(X, Y)
            assert abs(M.value(R)) * 100 < 51 * P and abs(R[-1]) < 1 << 20


def test_random_pairs_and_dependent_chains():
    rng = random.Random(30)
    stats = {}
    for n in range(200):
        if n % 2:
            X, Y = M.centred(rng.randrange(P) - P // 2), M.centred(rng.randrange(P) - P // 2)
        else:  # any digits the form admits
            X = [rng.randint(LO, HI) for _ in range(M.N - 1)] + [rng.randint(-(1 << 20) + 1, (1 << 20) - 1)]
            Y = [rng.randint(LO, HI) for _ in range(M.N - 1)] + [rng.randint(-(1 << 20) + 1, (1 << 20) - 1)]
        want = M.value(X) * M.value(Y) * RINV % P
        A = mul(X, Y, stats)
        for step in range(1, 61):
            if step % 5 == 0:
                A = mul(A, Y, stats)
                want = want * M.value(Y) * RINV % P
            else:
                A = sqr(A, stats)
                want = want * want * RINV % P
            v = M.value(A)
            assert abs(v) * 100 < 51 * P and abs(A[-1]) < 1 << 20
            assert v % P == want
    assert stats["peak"] < 1 << 63


def _slice_inputs():
    rng = random.Random(31)
    ones = (1 << 360) - 1  # every 30-bit slice below the top one at 2^30 - 1; p allows 0x1a0111 above them
    return [0, 1, P - 1, (1 << 384) % P, ones, ones | (0x1a0110 << 360), 1 << 29, (1 << 29) - 1,
            (1 << 384) - 1] + [rng.randrange(P) for _ in range(300)]


def test_entry_recentres_and_converts():
    for x in _slice_inputs():
        L = M.slice_words(M.words(x))
        assert M.value(L) == x
        for d in L[:-1]:
            assert LO <= d <= HI
        assert 0 <= L[-1] <= 1 << 24
        if x < P:
            A = M.enter(x)  # the bound asserts of the product run inside
            check_op(L, M.K_IN, A)
            v = M.value(A)
            assert v % P == x * 64 % P  # x 2^384 -> x 2^390
            assert abs(v) * 100 < 51 * P and abs(A[-1]) < 1 << 20


def test_exit_returns_the_canonical_words():
    rng = random.Random(32)
    k64 = pow(64, -1, P)
    vals = [0, 1, -1, (P - 1) // 2, -(P - 1) // 2, 51 * P // 100, -51 * P // 100]
    vals += [rng.randrange(P) - P // 2 for _ in range(300)]
    for v in vals:
        got = M.leave(M.centred(v))
        assert 0 <= got < P
        assert got == v * k64 % P  # x 2^390 -> x 2^384
    # the carry pass alone, on negative, zero and positive values
    for v in (-(P - 1), -1, 0, 1, P - 1, -(1 << 360), (1 << 360) - 1):
        r = M.unslice(M.centred(v))
        assert sum(w << (32 * j) for j, w in enumerate(r)) == v % P
    # a round trip through entry and exit is the identity on canonical values
    for x in _slice_inputs():
        if x < P:
            assert M.leave(M.enter(x)) == x


def _table(txt, name):
    m = re.search(r"int32_t %s\(int i\) \{\s*const int32_t t\[N\] = \{([^}]*)\};" % name, txt)
    return [int(v) for v in m.group(1).split(",")]


def test_header_constants_are_the_derived_ones():
    with open(os.path.join(ROOT, "drand_amd", "csrc", "fp_mul30.hpp")) as f:
        txt = f.read()
    assert int(re.search(r"constexpr int N = (\d+);", txt).group(1)) == M.N
    assert int(re.search(r"constexpr uint32_t MASK = (0x[0-9a-f]+)u;", txt).group(1), 16) == M.MASK
    assert int(re.search(r"constexpr uint32_t N0 = (0x[0-9a-f]+)u;", txt).group(1), 16) == M.N0
    assert (M.N0 * P + 1) % (1 << 30) == 0
    assert _table(txt, "P") == M.P_DIGITS and M.value(M.P_DIGITS) == P
    assert _table(txt, "K_IN") == M.K_IN and M.value(M.K_IN) == pow(2, 396, P)
    assert _table(txt, "K_OUT") == M.K_OUT and M.value(M.K_OUT) == pow(2, 384, P)
