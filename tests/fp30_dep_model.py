"""m30::mont_body of drand_amd/csrc/fp_mul30.hpp restated line by line on Python integers, in its accumulation order:
dependent columns (column k + 1 starts on acc >> 30 of column k, every MAD adds onto the running sum) and the paired
rounding of the output columns (the bias 2^29 + 2^59 added once per two columns). L operations run in lockstep, as
the template does for L = 1 and 2. Every single accumulation and every bias add asserts |acc| < 2^63 (the device
accumulator is an int64_t) and records the peak; every quotient column asserts that it shifts exactly; every 32-bit
intermediate asserts its range. Constants and helpers are those of tests/fp30_model.py, whose product and squaring
the results must equal digit for digit. tests/test_fp30_dep_model.py drives it."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fp30_model import BITS, HALF, MASK, N, N0, P_DIGITS, Acc, i32, sext30  # noqa: E402

BIAS = (1 << 29) + (1 << 59)


def mont_body(L, SQ, X, Y, stats=None):
    """mont_body<L, SQ>(R, X, Y): X, Y lists of L digit lists; returns the L results"""
    X2 = [[i32(x + x) if SQ else 0 for x in X[l]] for l in range(L)]
    Mq = [[0] * N for _ in range(L)]
    R = [[0] * N for _ in range(L)]
    acc = [Acc() for _ in range(L)]

    def mad(a, b):  # M30_MAD: one MAD of every operation
        for l in range(L):
            acc[l].mad(a(l), b(l))

    for k in range(2 * N - 1):
        lo, hi = max(0, k - (N - 1)), min(k, N - 1)
        if SQ:
            i = lo
            while 2 * i < k:
                mad(lambda l: X[l][i], lambda l: X2[l][k - i])
                i += 1
            if k & 1 == 0:
                mad(lambda l: X[l][k // 2], lambda l: X[l][k // 2])
        else:
            for i in range(lo, hi + 1):
                mad(lambda l: X[l][i], lambda l: Y[l][k - i])
        if k < N:
            for i in range(k):
                mad(lambda l: Mq[l][i], lambda l: P_DIGITS[k - i])
            for l in range(L):
                Mq[l][k] = sext30(((acc[l].v & 0xFFFFFFFF) * N0) & 0xFFFFFFFF)
            mad(lambda l: Mq[l][k], lambda l: P_DIGITS[0])
            for l in range(L):
                assert acc[l].v & MASK == 0, "a quotient column must shift exactly"
                acc[l].v >>= BITS
        else:
            for i in range(k - (N - 1), N):
                mad(lambda l: Mq[l][i], lambda l: P_DIGITS[k - i])
            for l in range(L):
                if (k - N) % 2 == 0:
                    R[l][k - N] = sext30(acc[l].v & 0xFFFFFFFF)
                    acc[l].v += BIAS
                    acc[l].check()
                    acc[l].v >>= BITS
                else:
                    R[l][k - N] = sext30((acc[l].v & 0xFFFFFFFF) ^ HALF)
                    acc[l].v >>= BITS
    for l in range(L):
        R[l][N - 1] = i32(acc[l].v)
        if stats is not None:
            stats["peak"] = max(stats.get("peak", 0), acc[l].peak)
    return R


def mont_mul(X, Y, stats=None):
    return mont_body(1, False, [X], [Y], stats)[0]


def mont_sqr(X, stats=None):
    return mont_body(1, True, [X], [X], stats)[0]


def mont_mul2(X0, X1, Y0, Y1, stats=None):
    return mont_body(2, False, [X0, X1], [Y0, Y1], stats)


def mont_sqr2(X0, X1, stats=None):
    return mont_body(2, True, [X0, X1], [X0, X1], stats)
