"""CPU: the dependent-column body of drand_amd/csrc/fp_mul30.hpp (m30::mont_body: the carry of a column is the addend
of the next column's first MAD, the output columns round in pairs under one bias of 2^29 + 2^59) on Python integers.
tests/fp30_dep_model.py restates it in its accumulation order and asserts |acc| < 2^63 after every single
accumulation and after every bias add, and the exact shift of every quotient column. Checked here: the result digits
equal, digit for digit, those of the body it replaces (tests/fp30_model.py, product and squaring), for one operation
and for two in lockstep; and the peak of the accumulator stays below the derived bound: a column has at most 13 + 13
terms of at most 2^58, a carry-in below 2^35 (the biased carry of a first output column included), and the bias on
top, 26 * 2^58 + 2^35 + 2^59 + 2^29 < 2^63. Inputs: all digits at -2^29, all at 2^29 - 1, mixed signs, 0, +-1,
+-(p-1)/2, and 200 random pairs each followed by 60 dependent operations (squarings, a product every fifth)."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp30_dep_model as D  # noqa: E402
import fp30_model as M  # noqa: E402

P = M.P
LO, HI = -(1 << 29), (1 << 29) - 1
BOUND = 26 * (1 << 58) + (1 << 35) + D.BIAS


def mul(X, Y, stats):
    R = D.mont_mul(X, Y, stats)
    assert R == M.mont_mul(X, Y)
    return R


def sqr(X, stats):
    R = D.mont_sqr(X, stats)
    assert R == M.mont_sqr(X)
    return R


def _special():
    lo, hi = [LO] * M.N, [HI] * M.N
    mixed = [LO if i % 2 else HI for i in range(M.N)]
    mixed2 = [HI if i % 3 else LO for i in range(M.N)]
    half = (P - 1) // 2
    return [lo, hi, mixed, mixed2, M.centred(0), M.centred(1), M.centred(-1), M.centred(half), M.centred(-half)]


def test_bound_is_below_the_accumulator():
    assert BOUND < 1 << 63
    assert BOUND < 1.63 * 2 ** 62 + 2 ** 59 + 2 ** 36


def test_extreme_and_special_operands():
    stats = {}
    special = _special()
    for X in special:
        sqr(X, stats)
        for Y in special:
            mul(X, Y, stats)
    assert stats["peak"] < BOUND


def test_lockstep_pairs_equal_the_single_operations():
    stats = {}
    special = _special()
    for a, X0 in enumerate(special):
        X1 = special[(a + 3) % len(special)]
        assert D.mont_sqr2(X0, X1, stats) == [M.mont_sqr(X0), M.mont_sqr(X1)]
        for b, Y0 in enumerate(special):
            Y1 = special[(b + 5) % len(special)]
            assert D.mont_mul2(X0, X1, Y0, Y1, stats) == [M.mont_mul(X0, Y0), M.mont_mul(X1, Y1)]
    assert stats["peak"] < BOUND


def test_random_pairs_and_dependent_chains():
    rng = random.Random(3014)
    stats = {}
    for n in range(200):
        if n % 2:
            X, Y = M.centred(rng.randrange(P) - P // 2), M.centred(rng.randrange(P) - P // 2)
        else:  # any digits the form admits
            X = [rng.randint(LO, HI) for _ in range(M.N - 1)] + [rng.randint(-(1 << 20) + 1, (1 << 20) - 1)]
            Y = [rng.randint(LO, HI) for _ in range(M.N - 1)] + [rng.randint(-(1 << 20) + 1, (1 << 20) - 1)]
        A = mul(X, Y, stats)
        B = sqr(Y, stats)
        for step in range(1, 61):
            if step % 5 == 0:
                A = mul(A, Y, stats)
            else:
                A = sqr(A, stats)
            if n % 20 == 0:  # the same chain beside a second one, in lockstep
                two = D.mont_sqr2(A, B, stats) if step % 5 else D.mont_mul2(A, B, Y, X, stats)
                assert two == ([M.mont_sqr(A), M.mont_sqr(B)] if step % 5 else [M.mont_mul(A, Y), M.mont_mul(B, X)])
                B = two[1]
    assert stats["peak"] < BOUND
