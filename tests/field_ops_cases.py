"""Operand records and expected result records for the field-layer op kernel (drand_amd/csrc/k_fieldops.hip,
dh_field_ops_debug), on Python integers only. Test infrastructure for tests/test_field_ops_cases.py (CPU: checks this
generator and runs the raw products through fp_mul28.hpp compiled for the host) and tests/test_gpu_field_ops.py.

A case is one lane: an opcode, an operand record and either the exact result record (`exp`: every word, the words an
operation does not write being zero) or a contract (`check(out)` raises AssertionError) where the representative is
free: f28_red / f2_red (limbs < 2^28, value in [0, 2p), congruent to the input) and the point formulas (coordinates
congruent to the affine reference once Z is divided out, below the bound the header states, the infinity flag equal).
Contract cases carry `model`, the result record of the integer models (fp28_model, fp2_28_model), so that the CPU test
can show that the contract is satisfiable and that the inputs are inside the stated entry bounds (the models assert
them). References: pow, %, the exact Montgomery quotient (X Y + m p) / 2^392 with m = -X Y / p mod 2^392, and the
oracle's affine curve arithmetic (oracle/bls_py.py). Nothing here imports the library.
"""
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

import bls_py as B  # noqa: E402
import fp28_model as M  # noqa: E402
import fp2_28_model as M2  # noqa: E402

P = M.p
FR = M.r
RP = 1 << 392       # the 28-bit form's Montgomery radix
R384 = 1 << 384     # the 12-word form's
RPINV = pow(RP, -1, P)
RINV = pow(R384, -1, P)
PINV = pow(P, -1, RP)
MASK = (1 << 28) - 1
N0 = 0x0ffcfffd
IN_WORDS, SCALARS = 176, 168
OUT_WORDS, OUT_FLAGS = 88, 84
KS = (2, 3, 4, 6, 7, 8, 9, 12, 16, 18, 21, 24, 26, 32, 48)  # the multiples of p with a constant (fp28.hpp DH_KP)
EXPONENTS = ((P + 1) // 4, (P - 3) // 4, P - 2, (P - 1) // 2)  # SCHED_SQRT, SCHED_SR1_C1, SCHED_INV, SCHED_LEGENDRE

# the op table of k_fieldops.hip (tests/test_field_ops_cases.py compares it with the enum's text)
OPS = {
    "FP_ADD": 0, "FP_SUB": 1, "FP_NEG": 2, "FP_DBL": 3, "FP_MUL": 4, "FP_SQR": 5, "FP_MUL_NR": 6, "FP_TO_MONT": 7,
    "FP_FROM_MONT": 8, "FP_MUL_CIOS": 9,
    "F28_MUL": 16, "F28_SQR": 17, "F28_MUL_INL": 18, "F28_SQR_INL": 19, "F28_FROM_FP": 20, "F28_TO_FP": 21,
    "F28_ZERO": 22, "F28_ADD_NC": 23, "F28_RED": 24,
    "F28_LIN": 32, "F28_LIN3": 48, "F28_SUB_NC": 64,
    "F2_MUL": 96, "F2_MUL_NC": 97, "F2_RED": 98, "F2_CONJ": 99, "F2_NEG3": 100, "F2_SQR": 104,
    "J28_DBL": 112, "J28_DBL_INL": 113, "J28_DBL_A": 114, "J28_MADD": 115, "J28_ADD": 116, "J28_MADD_FAST": 117,
    "J28_ADD_FAST": 118,
    "J228_DBL": 120, "J228_DBL_NC": 121, "J228_MADD": 122, "J228_ADD": 123,
    "M30_MUL": 128, "M30_SQR": 129, "M30_MUL2": 130, "M30_SQR2": 131, "M30_POW": 132,
    "BGCD_INV": 140, "FP2_INV": 141, "FP2_INV_VT": 142,
    "FR_MUL": 144, "FR_ADD": 145, "FR_SUB": 146, "FR_INV": 147, "FR_FROM_BE512": 148, "FR_IS_CANONICAL": 149,
    "CALL_LIVE": 152, "CALL_NESTED": 153,
}


class Case:
    __slots__ = ("name", "op", "rec", "exp", "check", "model")

    def __init__(self, name, op, rec, exp=None, check=None, model=None):
        assert len(rec) == IN_WORDS and all(0 <= w < 1 << 32 for w in rec), name
        assert (exp is None) != (check is None), name
        assert exp is None or (len(exp) == OUT_WORDS and all(0 <= w < 1 << 32 for w in exp)), name
        self.name, self.op, self.rec, self.exp, self.check, self.model = name, op, rec, exp, check, model


# ---------------------------------------------------------------------------------------------- words and records
def words(v, n):
    assert 0 <= v < 1 << (32 * n), v
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def limbs(v):
    """14 normalised 28-bit limbs of v < 2^392"""
    assert 0 <= v < RP, v
    return [(v >> (28 * i)) & MASK for i in range(14)]


def qlimbs(q):
    """a product's result: 13 masked limbs and whatever is left in the top one (R[13] = (uint32_t)acc)"""
    top = q >> 364
    assert 0 <= top < 1 << 32
    return [(q >> (28 * i)) & MASK for i in range(13)] + [top]


def val(l):
    return sum(int(x) << (28 * i) for i, x in enumerate(l))


def _slots(n, width, items, total):
    w = [0] * total
    for k, it in enumerate(items):
        if it is None:
            continue
        ws = list(it) if isinstance(it, (list, tuple)) else (limbs(it) if width == 14 else words(it, width))
        assert len(ws) == width
        w[width * k:width * k + width] = ws
    return w


def rec(width, items, scal=()):
    """operand record: slots of `width` words (12: fp, 14: limbs, ints are normalised; 8: Fr) and the scalars"""
    w = _slots(0, width, items, IN_WORDS)
    for j, s in enumerate(scal):
        w[SCALARS + j] = s & 0xFFFFFFFF
    return w


def out(width, items, flags=()):
    w = _slots(0, width, items, OUT_WORDS)
    for j, f in enumerate(flags):
        w[OUT_FLAGS + j] = int(f)
    return w


# ---------------------------------------------------------------------------------------------- integer references
def montq(x, y):
    """fp_mul28.hpp mont_mul on the integers x, y (the values of any limb vectors): the exact quotient"""
    t = x * y
    m = (-t * PINV) % RP
    q, rem = divmod(t + m * P, RP)
    assert rem == 0
    return q


def mul384(a, b):
    return a * b * RINV % P


PL = limbs(P)


def m28_emul(X, Y=None):
    """fp_mul28.hpp M28_BODY on limb vectors, column by column in 64 bits: asserts that no column leaves uint64 (the
    doubled limbs of the squaring stay in 32 bits) and returns R. Y = None: mont_sqr."""
    sq = Y is None
    X2 = [x << 1 for x in X]
    assert all(x < 1 << 32 for x in X2 + list(X) + list(Y or []))

    def col(k):
        if sq:
            s = sum(X[i] * X2[k - i] for i in range(max(0, k - 13), 14) if 2 * i < k)
            return s + (X[k // 2] ** 2 if k % 2 == 0 else 0)
        return sum(X[i] * Y[k - i] for i in range(max(0, k - 13), min(k, 13) + 1))

    acc, Mq, R = 0, [], [0] * 14
    for k in range(14):
        acc += col(k) + sum(Mq[i] * PL[k - i] for i in range(k))
        Mq.append((acc * N0) & MASK)
        acc += Mq[k] * PL[0]
        assert acc < 1 << 64, "column %d leaves 64 bits" % k
        acc >>= 28
    for k in range(14, 27):
        acc += col(k) + sum(Mq[i] * PL[k - i] for i in range(k - 13, 14))
        assert acc < 1 << 64, "column %d leaves 64 bits" % k
        R[k - 14] = acc & MASK
        acc >>= 28
    assert acc < 1 << 32
    R[13] = acc
    return R


def sub_nc_limbs(K, a, b):
    """f28_sub_nc<K>: a + K p - b limb by limb, K p in the redundant form the header describes (limb 0 + 2^28, limbs
    1 .. 12 + 2^28 - 1, limb 13 - 1)"""
    kp = limbs(K * P)
    red = [kp[0] + (1 << 28)] + [kp[i] + MASK for i in range(1, 13)] + [kp[13] - 1]
    r = [a[i] + red[i] - b[i] for i in range(14)]
    assert all(0 <= x < 1 << 32 for x in r), "f28_sub_nc: a limb leaves [0, 2^32)"
    return r


def kp_above(K):
    return min(k for k in KS if k > K)


def field_values():
    """0, 1, 2, p - 1, p - 2, (p +- 1) / 2, R, R^2, 2^k and 2^k - 1 at every limb boundary of the three
    representations (k a multiple of 28, 30, 32), and 200 random values"""
    v = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, R384 % P, R384 * R384 % P]
    for step in (28, 30, 32):
        for k in range(step, 381, step):
            v += [1 << k, (1 << k) - 1]
    rng = random.Random(2801)
    v += [rng.randrange(P) for _ in range(200)]
    seen, o = set(), []
    for x in v:
        if x not in seen:
            seen.add(x)
            o.append(x)
    return o


N_EDGE = 9  # the first values of field_values() are the edges proper


def pairs(vals, rng, cross=N_EDGE):
    """every value beside a random partner, and the edges against each other"""
    o = [(a, vals[rng.randrange(len(vals))]) for a in vals]
    o += [(a, b) for a in vals[:cross] for b in vals[:cross]]
    return o


# ---------------------------------------------------------------------------------------------- 12-word layer
def fam_fp():
    V = field_values()
    rng = random.Random(1201)
    c = []
    two = (("FP_ADD", lambda a, b: (a + b) % P), ("FP_SUB", lambda a, b: (a - b) % P), ("FP_MUL", mul384),
           ("FP_MUL_CIOS", mul384))
    for name, f in two:
        for i, (a, b) in enumerate(pairs(V, rng)):
            c.append(Case("%s[%d] %x, %x" % (name, i, a, b), OPS[name], rec(12, [a, b]), out(12, [f(a, b)])))
    one = (("FP_NEG", lambda a: (P - a) % P), ("FP_DBL", lambda a: 2 * a % P), ("FP_SQR", lambda a: mul384(a, a)),
           ("FP_TO_MONT", lambda a: a * R384 % P), ("FP_FROM_MONT", lambda a: a * RINV % P))
    for name, f in one:
        for i, a in enumerate(V):
            c.append(Case("%s[%d] %x" % (name, i, a), OPS[name], rec(12, [a]), out(12, [f(a)])))
    # unreduced sums in [p, 2p) (and below) feeding the product
    quads = [(P - 1, P - 1, P - 1, P - 1), (P - 1, 1, P - 1, 1), (P - 1, 0, P - 1, P - 1), (0, 0, P - 1, P - 1),
             ((P + 1) // 2, (P - 1) // 2, (P + 1) // 2, (P + 1) // 2), (P - 1, P - 1, 1, 0), (1, 0, P - 1, P - 1)]
    quads += [tuple(V[rng.randrange(len(V))] for _ in range(4)) for _ in range(100)]
    for i, (a, b, cc, d) in enumerate(quads):
        c.append(Case("FP_MUL_NR[%d] (%x + %x)(%x + %x)" % (i, a, b, cc, d), OPS["FP_MUL_NR"], rec(12, [a, b, cc, d]),
                      out(12, [mul384(a + b, cc + d)])))
    return c


# ---------------------------------------------------------------------------------------------- 28-bit products
def raw_product_inputs():
    """(name, X limbs, Y limbs or None, in_value_contract): the pairs of the bare 28-bit product"""
    rng = random.Random(2802)
    full = [MASK] * 14
    addnc_max = [2 * MASK] * 14                                   # f28_add_nc of two all-ones vectors
    subnc_max = sub_nc_limbs(48, full, [0] * 14)                  # f28_sub_nc<48>(all ones, 0)
    o = []
    x = 48 * P - 1
    o.append(("48p-1 x floor(2^392 p / x)", limbs(x), limbs(RP * P // x), True))
    y = 50 * P - 1
    o.append(("floor(2^392 p / y) x 50p-1", limbs(RP * P // y), limbs(y), True))
    o.append(("all ones x p", full, limbs(RP * P // (RP - 1)), True))
    o.append(("all ones x all ones", full, full, False))
    for nm, v in (("0", 0), ("1", 1), ("R' mod p", RP % P), ("p", P), ("2p-1", 2 * P - 1), ("48p-1", 48 * P - 1)):
        o.append(("0 x " + nm, limbs(0), limbs(v), True))
        o.append((nm + " x 1", limbs(v), limbs(1), True))
        o.append(("1 x " + nm, limbs(1), limbs(v), True))
    o.append(("add_nc max x sub_nc<48> max", addnc_max, subnc_max, False))
    o.append(("sub_nc<48> max x add_nc max", subnc_max, addnc_max, False))
    o.append(("add_nc max x add_nc max", addnc_max, addnc_max, False))
    for i in range(14):
        for j in range(14):
            hx, hy = [0] * 14, [0] * 14
            hx[i], hy[j] = (MASK, MASK) if (i + j) % 2 else (3 * MASK, 2 * MASK)
            o.append(("hot limbs %d x %d" % (i, j), hx, hy, False))
    for i in range(60):
        kx = rng.choice((1, 2, 8, 26, 48))
        a = rng.randrange(kx * P)
        b = rng.randrange(min(RP, RP * P // max(a, 1)))
        o.append(("random %d" % i, limbs(a), limbs(b), True))
    sq = [("sqr " + n, X, None, ok) for n, X, ok in (
        ("0", limbs(0), True), ("1", limbs(1), True), ("p", limbs(P), True), ("50p-1", limbs(50 * P - 1), True),
        ("all ones", full, False), ("add_nc max", addnc_max, False), ("sub_nc<48> max", subnc_max, False))]
    for i in range(14):
        h = [0] * 14
        h[i] = 3 * MASK if i % 2 else MASK
        sq.append(("sqr hot limb %d" % i, h, None, False))
    for i in range(40):
        sq.append(("sqr random %d" % i, limbs(rng.randrange(rng.choice((1, 2, 26, 50)) * P)), None, True))
    return o + sq


def fam_f28():
    c = []
    for i, (name, X, Y, ok) in enumerate(raw_product_inputs()):
        q = montq(val(X), val(X if Y is None else Y))
        assert not ok or q < 2 * P, name
        for op in (("F28_SQR", "F28_SQR_INL") if Y is None else ("F28_MUL", "F28_MUL_INL")):
            c.append(Case("%s[%d] %s" % (op, i, name), OPS[op], rec(14, [X] if Y is None else [X, Y]), out(14, [qlimbs(q)])))
    V = field_values()
    k400 = pow(2, 400, P)
    for i, a in enumerate(V):
        c.append(Case("F28_FROM_FP[%d] %x" % (i, a), OPS["F28_FROM_FP"], rec(12, [a]), out(14, [qlimbs(montq(a, k400))])))
    rng = random.Random(2803)
    lazy = [x + j * P for x in V[:N_EDGE] + V[-30:] for j in range(4)]
    for i, a in enumerate(lazy):  # f28_to_fp: any value < 4p
        c.append(Case("F28_TO_FP[%d] %x" % (i, a), OPS["F28_TO_FP"], rec(14, [a]), out(12, [a * (R384 % P) * RPINV % P])))
    zs = [k * P + d for k in (0, 1, 2, 3, 47, 48, 2519, 2520) for d in (-1, 0, 1) if 0 <= k * P + d < RP]
    zs += [RP - 1, RP - P] + [rng.randrange(RP) for _ in range(20)] + [rng.randrange(2520) * P for _ in range(20)]
    for i, a in enumerate(zs):
        c.append(Case("F28_ZERO[%d] %x" % (i, a), OPS["F28_ZERO"], rec(14, [a]), out(14, [], [a % P == 0])))
    return c


# ---------------------------------------------------------------------------------------------- 28-bit linear forms
def red_inputs():
    v = []
    for k in range(2521):
        v += [a for a in (k * P - 1, k * P, k * P + 1, k * P + P // 2) if 0 <= a < RP]
    return v + [RP - 1, RP - P]


def red_check(a, name):
    def check(o):
        l = o[:14]
        assert all(x <= MASK for x in l), "%s: a limb above 2^28" % name
        v = val(l)
        assert v < 2 * P, "%s: %.3f p" % (name, v / P)
        assert v % P == a % P, "%s: not congruent" % name
        assert not any(o[14:]), "%s: words beyond the result" % name
    return check


def fam_lin():
    rng = random.Random(2804)
    c = []
    full = RP - 1
    for ki, K in enumerate(KS):
        kp = K * P
        a0 = rng.randrange(2 * P)
        # a + K p - b = 0, 1, K p; a borrow through all 14 limbs (a = 0, b all ones below K p's top limb less one)
        borrow = ((kp >> 364) - 1 << 364) + (1 << 364) - 1
        two = [("-> 0", a0, 1, a0 + kp, -1), ("-> 1", a0, 1, a0 + kp - 1, -1), ("-> K p", a0, 1, a0, -1),
               ("borrow through every limb", 0, 1, borrow, -1), ("all ones - K p", full, 1, kp, -1),
               ("a - 8 b", 0, 1, kp // 8, -8), ("6 a - 8 b", P // 6, 6, (kp + P - 6) // 8, -8), ("3 a + 3 b", a0, 3, 2 * P - 1, 3),
               ("-a", 2 * P - 1 if K >= 2 else 0, -1, 0, 0)]
        for _ in range(6):
            ca, cb = rng.randrange(1, 4), -rng.randrange(1, 5)
            b = rng.randrange(kp // -cb)
            two.append(("random", rng.randrange(26 * P), ca, b, cb))
        for i, (nm, a, ca, b, cb) in enumerate(two):
            nm = "[%d] %s" % (i, nm)
            v = ca * a + cb * b + kp
            assert 0 <= v < RP and min(ca, 0) + min(cb, 0) >= -8 and max(ca, 0) + max(cb, 0) <= 6, (K, nm)
            c.append(Case("F28_LIN<%d> %s" % (K, nm), OPS["F28_LIN"] + ki, rec(14, [a, b], [ca, cb]), out(14, [limbs(v)])))
        three = [("-> 0", a0, 1, a0, -1, kp, -1), ("-> 1", a0, 1, kp - 1, -1, a0, -1), ("-> a + K p", a0, 1, 0, -1, 0, -1),
                 ("borrow through every limb", 0, 1, borrow, -1, 0, -2), ("2 (a - b - c)", 26 * P, 2, kp // 4, -2, kp // 4, -2),
                 ("a - b - 2 c", a0, 1, kp // 3, -1, kp // 3, -2), ("3 a + 2 b + c", a0, 3, 2 * P - 1, 2, P, 1),
                 ("a - 4 b - 4 c", 0, 1, kp // 8, -4, kp // 8, -4)]
        for _ in range(6):
            ca, cb, cc = rng.randrange(1, 4), -rng.randrange(1, 4), -rng.randrange(1, 4)
            three.append(("random", rng.randrange(26 * P), ca, rng.randrange(kp // (-2 * cb)), cb, rng.randrange(kp // (-2 * cc)), cc))
        for i, (nm, a, ca, b, cb, d, cc) in enumerate(three):
            nm = "[%d] %s" % (i, nm)
            v = ca * a + cb * b + cc * d + kp
            co = (ca, cb, cc)
            assert 0 <= v < RP and sum(min(x, 0) for x in co) >= -8 and sum(max(x, 0) for x in co) <= 6, (K, nm)
            c.append(Case("F28_LIN3<%d> %s" % (K, nm), OPS["F28_LIN3"] + ki, rec(14, [a, b, d], co), out(14, [limbs(v)])))
        # f28_sub_nc<K> and the products that consume it: (a, b, c, the squaring is inside the value contract)
        top = kp >> 364
        sub = [("random", rng.randrange(2 * P), rng.randrange((K - 1) * P), rng.randrange(2 * P), K <= 48),
               ("0 + K p - 0, x 1", 0, 0, 1, K <= 48),
               ("b's top limb one below K p's", 0, ((top - 1) << 364) + (1 << 364) - 1, 48 * P - 1, True),
               ("all ones - 0", full, 0, None, False)]
        for nm, a, b, cv, sq_ok in sub:
            assert (b >> 364) < top
            d = sub_nc_limbs(K, limbs(a), limbs(b))
            assert val(d) == a + kp - b and all(x < 3 << 28 for x in d)
            if cv is None:
                cv = RP * P // val(d)
            assert val(d) * cv < RP * P
            cl = limbs(cv)
            assert m28_emul(d, cl) == qlimbs(montq(val(d), cv)) and m28_emul(d) == qlimbs(montq(val(d), val(d)))
            assert not sq_ok or val(d) ** 2 < RP * P
            c.append(Case("F28_SUB_NC<%d> %s" % (K, nm), OPS["F28_SUB_NC"] + ki, rec(14, [a, b, cl]),
                          out(14, [qlimbs(montq(val(d), cv)), d, qlimbs(montq(val(d), val(d)))])))
    nc = [([MASK] * 14, [MASK] * 14), ([0] * 14, [0] * 14), (limbs(48 * P - 1), limbs(2 * P - 1))]
    nc += [(limbs(rng.randrange(RP)), limbs(rng.randrange(RP))) for _ in range(20)]
    for i, (a, b) in enumerate(nc):
        c.append(Case("F28_ADD_NC[%d]" % i, OPS["F28_ADD_NC"], rec(14, [a, b]), out(14, [[x + y for x, y in zip(a, b)]])))
    for i, a in enumerate(red_inputs()):
        nm = "F28_RED[%d] %d p %+d" % (i, (a + 1) // P, a - (a + 1) // P * P)
        c.append(Case(nm, OPS["F28_RED"], rec(14, [a]), check=red_check(a, nm), model=out(14, [M2.red(a)])))
    return c


# ---------------------------------------------------------------------------------------------- Fp2 on 28 bits
def f2_sqr_ref(a, K, nc):
    Kp = kp_above(K) if nc else K
    if nc:
        M2.sub_nc(Kp, a[0], a[1])  # asserts f28_sub_nc's condition on a1's top limb
    t0 = M.mont(a[0] + a[1], a[0] + Kp * P - a[1])
    return (t0, 2 * M.mont(a[0], a[1]))


def fam_f2():
    rng = random.Random(2805)
    c = []

    def lazy(k0, k1):  # a component pair just below (k0, k1) p
        return (rng.randrange(P) + (k0 - 1) * P, rng.randrange(P) + (k1 - 1) * P)

    mul_in = [((0, 0), (0, 0)), ((1, 0), lazy(2, 2)), (lazy(2, 2), (0, 1)), ((12 * P - 1, 12 * P - 1), (52 * P, 52 * P)),
              ((6 * P - 1, 12 * P - 1), (15 * P - 1, 27 * P - 1)), ((2 * P - 1, 3 * P - 1), (12 * P - 1, 12 * P - 1)),
              ((18 * P - 1, 18 * P - 1), (9 * P - 1, 9 * P - 1)), ((24 * P - 1, 24 * P - 1), (9 * P - 1, 9 * P - 1))]
    mul_in += [(lazy(2, 2), lazy(2, 2)) for _ in range(20)] + [(lazy(6, 12), lazy(15, 27)) for _ in range(10)]
    for i, (a, b) in enumerate(mul_in):
        assert (a[0] + a[1]) * (b[0] + b[1]) < 2500 * P * P
        e = M2.m2(a, b)
        assert e[0] < 4 * P and e[1] < 6 * P
        for nm in ("F2_MUL", "F2_MUL_NC"):
            c.append(Case("%s[%d] (%.2f, %.2f) x (%.2f, %.2f) p" % (nm, i, a[0] / P, a[1] / P, b[0] / P, b[1] / P), OPS[nm],
                          rec(14, [a[0], a[1], b[0], b[1]]), out(14, [limbs(e[0]), limbs(e[1])])))
    # f2_sqr<K>: a1 at K p - 1 (the formulas: Y < 3, B = (2, 4), X + B < (5, 7), E < (6, 12) and Z < (12, 12))
    for j, (K, a0s) in enumerate(((3, (3, 2)), (4, (2, 4)), (7, (5, 7)), (12, (6, 12)))):
        ins = [(0, 0), (1, 0), (0, 1), (a0s[0] * P - 1, K * P - 1), (K * P - 1, K * P - 1), (0, K * P - 1), (K * P - 1, 0)]
        ins += [lazy(a0s[0], K) for _ in range(10)]
        for nc in (0, 1):
            for i, a in enumerate(ins):
                e = f2_sqr_ref(a, K, nc)
                assert e[0] < 2 * P and e[1] < 4 * P
                c.append(Case("F2_SQR<%d, %d>[%d] (%.2f, %.2f) p" % (K, nc, i, a[0] / P, a[1] / P), OPS["F2_SQR"] + 2 * j + nc,
                              rec(14, [a[0], a[1]]), out(14, [limbs(e[0]), limbs(e[1])])))
    reds = red_inputs()
    rin = [(reds[rng.randrange(len(reds))], reds[rng.randrange(len(reds))]) for _ in range(200)] + [(RP - 1, 0), (0, RP - 1)]
    for i, a in enumerate(rin):
        nm = "F2_RED[%d]" % i

        def check(o, a=a, nm=nm):
            red_check(a[0], nm + ".c0")(o[:14] + [0] * (OUT_WORDS - 14))
            red_check(a[1], nm + ".c1")(o[14:28] + [0] * (OUT_WORDS - 14))
            assert not any(o[28:]), nm
        c.append(Case(nm, OPS["F2_RED"], rec(14, [a[0], a[1]]), check=check, model=out(14, [M2.red(a[0]), M2.red(a[1])])))
    for i, a in enumerate([(0, 0), (2 * P - 1, 2 * P - 1), (1, 1), (P, P), (0, 2 * P - 1)] + [lazy(2, 2) for _ in range(10)]):
        c.append(Case("F2_CONJ[%d]" % i, OPS["F2_CONJ"], rec(14, [a[0], a[1]]), out(14, [a[0], 2 * P - a[1]])))
    for i, a in enumerate([(0, 0), (3 * P - 1, 3 * P - 1), (1, P), (3 * P - 1, 0)] + [lazy(3, 3) for _ in range(10)]):
        c.append(Case("F2_NEG3[%d]" % i, OPS["F2_NEG3"], rec(14, [a[0], a[1]]), out(14, [3 * P - a[0], 3 * P - a[1]])))
    return c


# ---------------------------------------------------------------------------------------------- point formulas
def dbl_a_model(Pt, a28):
    """fp28.hpp j28_dbl_a on the integer model"""
    X, Y, Z, fl = Pt
    mont, lin, lin3 = M.mont, M.lin, M.lin3
    a = mont(X, X); b = mont(Y, Y); c = mont(b, b)
    xb = M.add(X, b); t = mont(xb, xb)
    d = lin3(8, t, 2, a, -2, c, -2)
    z2 = mont(Z, Z)
    e = lin(0, a, 3, mont(a28, mont(z2, z2)), 1)
    f = mont(e, e)
    x = lin(24, f, 1, d, -2)
    y = lin(16, mont(e, M.sub(26, d, x)), 1, c, -8)
    return (x, y, M.scale(mont(Y, Z), 2), fl)


def g1_lazy(pt, z, k):
    """affine pt (plain field) -> Jacobian (X, Y, Z) in the 28-bit Montgomery form with Z = z, each coordinate in
    [(k - 1) p, k p)"""
    x, y = pt
    return tuple(v * RP % P + (j - 1) * P for v, j in zip((x * z * z % P, y * z ** 3 % P, z), k))


def g1_affine(X, Y, Z):
    f = lambda v: v * RPINV % P  # noqa: E731
    zi = pow(f(Z), -1, P)
    return (f(X) * zi * zi % P, f(Y) * zi ** 3 % P)


def point_check(name, nf, F, want, bound, poisoned=None):
    """nf Fp components a coordinate (1: G1, 2: G2); want: the affine sum or None; bound: (X, Y, Z) in units of p"""
    def check(o):
        co = [val(o[14 * i:14 * i + 14]) for i in range(3 * nf)]
        assert all(x <= MASK for x in o[:42 * nf]), "%s: a limb above 2^28" % name
        assert not any(o[42 * nf:OUT_FLAGS]) and not any(o[OUT_FLAGS + 2:]), "%s: words beyond the result" % name
        if poisoned is not None:
            assert o[OUT_FLAGS + 1] == int(poisoned), "%s: poisoned = %d" % (name, o[OUT_FLAGS + 1])
            if poisoned:
                return
        assert o[OUT_FLAGS] == int(want is None), "%s: inf = %d" % (name, o[OUT_FLAGS])
        if want is None:
            return
        for i, v in enumerate(co):
            assert v < bound[i // nf] * P, "%s: coordinate %d at %.3f p, bound %d" % (name, i, v / P, bound[i // nf])
        if nf == 1:
            got = g1_affine(*co)
        else:
            f = lambda v: v * RPINV % P  # noqa: E731
            x, y, z = [(f(co[2 * i]), f(co[2 * i + 1])) for i in range(3)]
            zi = B.f2inv(z)
            zi2 = B.f2mul(zi, zi)
            got = (B.f2mul(x, zi2), B.f2mul(y, B.f2mul(zi2, zi)))
        assert got == want, "%s: not the affine reference" % name
    return check


def jrec(pts, infs):
    """the coordinates of the points in slot order, the infinity flags as scalars"""
    flat = []
    for pt in pts:
        for co in pt:
            flat += list(co) if isinstance(co, tuple) else [co]
    return rec(14, flat, infs)


def jout(Pt, nf, poisoned=None):
    X, Y, Z, fl = Pt
    flat = [X, Y, Z] if nf == 1 else [X[0], X[1], Y[0], Y[1], Z[0], Z[1]]
    return out(14, flat, [fl] + ([poisoned] if poisoned is not None else []))


def fam_points():
    rng = random.Random(2806)
    c = []
    F = B.FP
    G = [None] + [B.ec_mul(F, B.G1_GEN, k) for k in range(1, 12)]
    INF1 = (M.ONE, M.ONE, 0)
    # ---- j28_dbl: the formula never uses b, so any (x, y) with y != 0 is a point of some curve y^2 = x^3 + b
    zmax = lambda Y, zr: zr + ((2500 * P * P - 1) // Y - zr) // P * P  # noqa: E731  the largest Z = zr mod p with Y Z < 2500 p^2
    dbl_in = [("5G", g1_lazy(G[5], rng.randrange(1, P), (1, 1, 1))), ("5G at (48, 50, 50)", g1_lazy(G[5], rng.randrange(1, P), (48, 50, 50))),
              ("X = 48p-1, Y = 50p-1, Y Z < 2500 p^2", (48 * P - 1, 50 * P - 1, zmax(50 * P - 1, rng.randrange(P)))),
              ("X = 48p-1, Y = p+1, Z = 2499p", (48 * P - 1, P + 1, 2498 * P + rng.randrange(1, P))),
              ("X = 0, Y = 1, Z = 1", (0, 1, 1)), ("all at p-1", (P - 1, P - 1, P - 1))]
    dbl_in += [("random %d" % i, tuple(rng.randrange(1, k * P) for k in (48, 50, 50))) for i in range(6)]
    for nm, (X, Y, Z) in dbl_in:
        assert X < 48 * P and Y < 50 * P and Y * Z < 2500 * P * P and Z < RP
        aff = g1_affine(X, Y, Z)
        for op, a, model in (("J28_DBL", None, M.dbl), ("J28_DBL_INL", None, M.dbl), ("J28_DBL_A", B.A1P, None)):
            if a is not None and Z >= 50 * P:
                continue
            want = B.ec_dbl(F, aff, a)
            mo = model((X, Y, Z, False)) if model else dbl_a_model((X, Y, Z, False), B.A1P * RP % P)
            name = "%s %s" % (op, nm)
            c.append(Case(name, OPS[op], jrec([(X, Y, Z)], [0]), check=point_check(name, 1, F, want, (26, 18, 4)), model=jout(mo, 1)))
    for op in ("J28_DBL", "J28_DBL_INL", "J28_DBL_A"):
        name = op + " infinity"
        c.append(Case(name, OPS[op], jrec([INF1], [1]), check=point_check(name, 1, F, None, None), model=jout(M.inf(), 1)))
    # a point of E1' (the curve j28_dbl_a serves), doubled
    x = 1
    while not B.f_is_square((x ** 3 + B.A1P * x + B.B1P) % P):
        x += 1
    e1p = (x, B.fsqrt((x ** 3 + B.A1P * x + B.B1P) % P))
    for k in ((1, 1, 1), (48, 50, 50)):
        X, Y, Z = g1_lazy(e1p, rng.randrange(1, P), k)
        Z = min(Z, zmax(Y, Z % P))
        name = "J28_DBL_A a point of E1' at %s" % (k,)
        c.append(Case(name, OPS["J28_DBL_A"], jrec([(X, Y, Z)], [0]), check=point_check(name, 1, F, B.ec_dbl(F, e1p, B.A1P), (26, 18, 4)),
                      model=jout(dbl_a_model((X, Y, Z, False), B.A1P * RP % P), 1)))
    # ---- j28_madd / j28_add and their fast forms: in (26, 18, 6) [x (26, 18, 6)], q < 2
    qa = lambda pt, k: tuple(v * RP % P + (k - 1) * P for v in pt)  # noqa: E731
    z1, z2 = rng.randrange(1, P), rng.randrange(1, P)
    neg = lambda pt: B.ec_neg(F, pt)  # noqa: E731
    for nm, p1, k1, q1, kq in (("5G + 7G", G[5], (1, 1, 1), G[7], 1), ("5G + 7G at the bounds", G[5], (26, 18, 6), G[7], 2),
                               ("5G + 5G at the bounds", G[5], (26, 18, 6), G[5], 2), ("5G + 5G", G[5], (1, 1, 1), G[5], 1),
                               ("5G - 5G at the bounds", G[5], (26, 18, 6), neg(G[5]), 2), ("5G - 5G", G[5], (2, 3, 4), neg(G[5]), 1),
                               ("infinity + 7G", None, None, G[7], 2), ("G + 2G", G[1], (26, 1, 6), G[2], 1)):
        Pj = INF1 if p1 is None else g1_lazy(p1, z1, k1)
        q = qa(q1, kq)
        want = B.ec_add(F, p1, q1)
        same = p1 is not None and p1[0] == q1[0]
        bound = (26, 18, 4) if same else (8, 6, 6)
        for op, model in (("J28_MADD", M.madd), ("J28_MADD_FAST", M.madd_fast)):
            fast = op.endswith("FAST")
            mo = model(Pj + (p1 is None,), q[0], q[1])
            name = "%s %s" % (op, nm)
            if p1 is None:  # the affine point comes back as it is, Z = R' mod p
                c.append(Case(name, OPS[op], jrec([Pj, q], [1]), exp=jout((q[0], q[1], M.ONE, False), 1, False if fast else None)))
                continue
            chk = point_check(name, 1, F, want, bound, (same if fast else None))
            c.append(Case(name, OPS[op], jrec([Pj, q], [0]), check=chk, model=jout(mo, 1, M.poisoned(mo) if fast else None)))
    for nm, p1, k1, q1, k2 in (("5G + 7G", G[5], (1, 1, 1), G[7], (1, 1, 1)), ("5G + 7G at the bounds", G[5], (26, 18, 6), G[7], (26, 18, 6)),
                               ("5G + 5G at the bounds", G[5], (26, 18, 6), G[5], (26, 18, 6)), ("5G + 5G", G[5], (1, 2, 3), G[5], (3, 2, 1)),
                               ("5G - 5G at the bounds", G[5], (26, 18, 6), neg(G[5]), (26, 18, 6)), ("5G - 5G", G[5], (1, 1, 1), neg(G[5]), (1, 1, 1)),
                               ("infinity + 7G", None, None, G[7], (26, 18, 6)), ("5G + infinity", G[5], (26, 18, 6), None, None),
                               ("infinity + infinity", None, None, None, None), ("3G + 8G", G[3], (1, 18, 1), G[8], (26, 1, 6))):
        Pj = INF1 if p1 is None else g1_lazy(p1, z1, k1)
        Qj = INF1 if q1 is None else g1_lazy(q1, z2, k2)
        want = B.ec_add(F, p1, q1)
        same = p1 is not None and q1 is not None and p1[0] == q1[0]
        bound = (26, 18, 4) if same else (8, 6, 2)
        for op, model in (("J28_ADD", M.jadd), ("J28_ADD_FAST", M.jadd_fast)):
            fast = op.endswith("FAST")
            r = jrec([Pj, Qj], [p1 is None, q1 is None])
            name = "%s %s" % (op, nm)
            if p1 is None or q1 is None:  # the other operand comes back as it is
                back = Qj + (q1 is None,) if p1 is None else Pj + (False,)
                c.append(Case(name, OPS[op], r, exp=jout(back, 1, False if fast else None)))
                continue
            mo = model(Pj + (False,), Qj + (False,))
            chk = point_check(name, 1, F, want, bound, (same if fast else None))
            c.append(Case(name, OPS[op], r, check=chk, model=jout(mo, 1, M.poisoned(mo) if fast else None)))
    # ---- G2: X, Y < 2 (Y < 3 accepted), Z < 12 per component; q affine < 3
    F2 = B.FP2
    H = [None] + [B.ec_mul(F2, B.G2_GEN, k) for k in range(1, 9)]

    def g2_lazy(pt, z, k):
        x, y = pt
        z2 = B.f2mul(z, z)
        co = (B.f2mul(x, z2), B.f2mul(y, B.f2mul(z2, z)), z)
        return tuple(tuple(v * RP % P + (j - 1) * P for v in e) for e, j in zip(co, k))

    zz1 = (rng.randrange(1, P), rng.randrange(P))
    zz2 = (rng.randrange(P), rng.randrange(1, P))
    INF2 = (M2.ONE2, M2.ONE2, M2.ZERO2)
    neg2 = lambda pt: B.ec_neg(F2, pt)  # noqa: E731
    for nm, p1, k in (("3H", H[3], (1, 1, 1)), ("3H at (2, 2, 12)", H[3], (2, 2, 12)), ("3H at (2, 3, 12)", H[3], (2, 3, 12)),
                      ("H", H[1], (1, 2, 7)), ("infinity", None, None)):
        Pj = INF2 if p1 is None else g2_lazy(p1, zz1, k)
        want = B.ec_dbl(F2, p1)
        mo = M2.dbl(Pj + (p1 is None,))
        for op in ("J228_DBL", "J228_DBL_NC"):
            name = "%s %s" % (op, nm)
            c.append(Case(name, OPS[op], jrec([Pj], [p1 is None]), check=point_check(name, 2, F2, want, (2, 2, 12)), model=jout(mo, 2)))
    q2 = lambda pt, k: tuple(tuple(v * RP % P + (k - 1) * P for v in e) for e in pt)  # noqa: E731
    for nm, p1, k1, q1, kq in (("3H + 5H", H[3], (1, 1, 1), H[5], 1), ("3H + 5H at the bounds", H[3], (2, 2, 12), H[5], 3),
                               ("3H + 3H at the bounds", H[3], (2, 2, 12), H[3], 3), ("3H - 3H at the bounds", H[3], (2, 2, 12), neg2(H[3]), 3),
                               ("infinity + 5H", None, None, H[5], 3), ("H + 2H", H[1], (2, 1, 12), H[2], 2)):
        Pj = INF2 if p1 is None else g2_lazy(p1, zz1, k1)
        q = q2(q1, kq)
        name = "J228_MADD " + nm
        if p1 is None:
            c.append(Case(name, OPS["J228_MADD"], jrec([Pj, q], [1]), exp=jout((q[0], q[1], M2.ONE2, False), 2)))
            continue
        mo = M2.madd(Pj + (False,), q[0], q[1])
        c.append(Case(name, OPS["J228_MADD"], jrec([Pj, q], [0]), check=point_check(name, 2, F2, B.ec_add(F2, p1, q1), (2, 2, 12)),
                      model=jout(mo, 2)))
    for nm, p1, k1, q1, k2 in (("3H + 5H", H[3], (1, 1, 1), H[5], (1, 1, 1)), ("3H + 5H at the bounds", H[3], (2, 2, 12), H[5], (2, 2, 12)),
                               ("3H + 3H at the bounds", H[3], (2, 2, 12), H[3], (2, 2, 12)), ("3H - 3H at the bounds", H[3], (2, 2, 12), neg2(H[3]), (2, 2, 12)),
                               ("3H - 3H", H[3], (1, 1, 1), neg2(H[3]), (1, 2, 3)), ("infinity + 5H", None, None, H[5], (2, 2, 12)),
                               ("3H + infinity", H[3], (2, 2, 12), None, None), ("infinity + infinity", None, None, None, None),
                               ("2H + 6H", H[2], (2, 1, 12), H[6], (1, 2, 6))):
        Pj = INF2 if p1 is None else g2_lazy(p1, zz1, k1)
        Qj = INF2 if q1 is None else g2_lazy(q1, zz2, k2)
        r = jrec([Pj, Qj], [p1 is None, q1 is None])
        name = "J228_ADD " + nm
        if p1 is None or q1 is None:
            back = Qj + (q1 is None,) if p1 is None else Pj + (False,)
            c.append(Case(name, OPS["J228_ADD"], r, exp=jout(back, 2)))
            continue
        same = p1[0] == q1[0]
        mo = M2.jadd(Pj + (False,), Qj + (False,))
        c.append(Case(name, OPS["J228_ADD"], r, check=point_check(name, 2, F2, B.ec_add(F2, p1, q1), (2, 2, 12 if same else 6)),
                      model=jout(mo, 2)))
    return c


# ---------------------------------------------------------------------------------------------- 30-bit chains
def fam_m30():
    V = field_values()
    rng = random.Random(3001)
    c = []
    pr = pairs(V, rng)
    for i, (a, b) in enumerate(pr):
        c.append(Case("M30_MUL[%d] %x, %x" % (i, a, b), OPS["M30_MUL"], rec(12, [a, b]), out(12, [mul384(a, b)])))
    for i, a in enumerate(V):
        c.append(Case("M30_SQR[%d] %x" % (i, a), OPS["M30_SQR"], rec(12, [a]), out(12, [mul384(a, a)])))
    for i in range(0, len(pr) - 1, 2):
        (a, cc), (b, d) = pr[i], pr[i + 1]
        c.append(Case("M30_MUL2[%d]" % i, OPS["M30_MUL2"], rec(12, [a, b, cc, d]), out(12, [mul384(a, cc), mul384(b, d)])))
        c.append(Case("M30_SQR2[%d]" % i, OPS["M30_SQR2"], rec(12, [a, cc]), out(12, [mul384(a, a), mul384(cc, cc)])))
    xs = V[:N_EDGE] + V[-40:]
    for j, e in enumerate(EXPONENTS):
        for i, a in enumerate(xs):  # a = y R: y^e R
            c.append(Case("M30_POW<%d>[%d] %x" % (j, i, a), OPS["M30_POW"] + j, rec(12, [a]),
                          out(12, [pow(a * RINV % P, e, P) * R384 % P])))
    return c


# ---------------------------------------------------------------------------------------------- inverses
def fam_inv():
    V = field_values()
    c = []
    for i, a in enumerate(v for v in V if v):
        c.append(Case("BGCD_INV[%d] %x" % (i, a), OPS["BGCD_INV"], rec(12, [a]), out(12, [pow(a, -1, P)])))
    rng = random.Random(3002)
    two = [(0, 0), (1, 0), (0, 1), (R384 % P, 0), (0, R384 % P), (P - 1, P - 1), (P - 1, 0), (0, P - 1), (1, P - 1)]
    two += [(V[rng.randrange(len(V))], V[rng.randrange(len(V))]) for _ in range(60)]
    for i, (a0, a1) in enumerate(two):
        x0, x1 = a0 * RINV % P, a1 * RINV % P
        ni = pow((x0 * x0 + x1 * x1) % P, P - 2, P)
        e = [x0 * ni * R384 % P, (P - x1 * ni) % P * R384 % P]
        for nm in ("FP2_INV", "FP2_INV_VT"):
            c.append(Case("%s[%d] (%x, %x)" % (nm, i, a0, a1), OPS[nm], rec(12, [a0, a1]), out(12, e)))
    return c


# ---------------------------------------------------------------------------------------------- Fr
def fam_fr():
    rng = random.Random(3003)
    R256 = 1 << 256
    ri = pow(R256, -1, FR)
    V = [0, 1, 2, FR - 1, FR - 2, (FR - 1) // 2, (FR + 1) // 2, R256 % FR, R256 * R256 % FR]
    V += [x for k in range(32, 255, 32) for x in (1 << k, (1 << k) - 1)] + [rng.randrange(FR) for _ in range(100)]
    c = []
    pr = pairs(V, rng)
    for nm, f in (("FR_MUL", lambda a, b: a * b * ri % FR), ("FR_ADD", lambda a, b: (a + b) % FR), ("FR_SUB", lambda a, b: (a - b) % FR)):
        for i, (a, b) in enumerate(pr):
            c.append(Case("%s[%d] %x, %x" % (nm, i, a, b), OPS[nm], rec(8, [a, b]), out(8, [f(a, b)])))
    # the product takes any 256-bit operand beside one below r (fr_from_be512 relies on it)
    for i, a in enumerate([R256 - 1, FR, FR + 1, 2 * FR - 1, 2 * FR, R256 - 2] + [rng.randrange(R256) for _ in range(20)]):
        b = V[rng.randrange(len(V))]
        c.append(Case("FR_MUL wide[%d] %x, %x" % (i, a, b), OPS["FR_MUL"], rec(8, [a, b]), out(8, [a * b * ri % FR])))
    for i, a in enumerate(V[:9] + V[-20:]):  # a = x R: x^-1 R, and 0 -> 0
        c.append(Case("FR_INV[%d] %x" % (i, a), OPS["FR_INV"], rec(8, [a]), out(8, [pow(a * ri % FR, FR - 2, FR) * R256 % FR])))
    big = [0, 1, (1 << 512) - 1, FR, FR - 1, R256, R256 - 1, FR << 256, (FR << 256) - 1, (1 << 511), FR * FR, FR * FR - 1]
    big += [rng.randrange(1 << 512) for _ in range(60)]
    for i, d in enumerate(big):
        be = words(d, 16)[::-1]  # word 0 the most significant
        w = [0] * IN_WORDS
        w[:16] = be
        c.append(Case("FR_FROM_BE512[%d] %x" % (i, d), OPS["FR_FROM_BE512"], w, out(8, [d % FR])))
    for i, a in enumerate(V[:9] + [FR, FR + 1, R256 - 1, FR + (1 << 224), FR - (1 << 224)] + [rng.randrange(R256) for _ in range(30)]):
        c.append(Case("FR_IS_CANONICAL[%d] %x" % (i, a), OPS["FR_IS_CANONICAL"], rec(8, [a]), out(8, [], [a < FR])))
    return c


# ---------------------------------------------------------------------------------------------- call convention
def live_ref(v, trip):
    acc = (v[0] + v[1]) % P
    for i in range(min(trip, 64)):
        k = i + 2
        t = (mul384(acc, k) + k) % P
        acc = mul384(t, t)
    for x in v:
        acc = (mul384(acc, x) + x) % P
    t0, t1, t2 = mul384(v[8], v[10]), mul384(v[9], v[11]), mul384(v[8] + v[9], v[10] + v[11])
    return [acc, (t0 - t1) % P, (t2 - t0 - t1) % P]


def nested_ref(v, trip):
    acc = v[0]
    for _ in range(min(trip, 64)):
        if acc & 1:
            acc = mul384(acc, v[1])
        acc = (acc + v[2]) % P
    for x in v[3:8]:
        acc = (mul384(acc, x) + x) % P
    return [acc]


def fam_call():
    rng = random.Random(3004)
    V = field_values()
    c = []
    trips = [0, 1, 2, 3, 5, 8, 13, 33, 64, 65, 1000]
    for i in range(150):
        trip = trips[i % len(trips)] if i < 44 else rng.randrange(40)
        v = [V[rng.randrange(N_EDGE)] if rng.random() < 0.2 else rng.randrange(P) for _ in range(12)]
        c.append(Case("CALL_LIVE[%d] %d iterations" % (i, trip), OPS["CALL_LIVE"], rec(12, v, [trip]), out(12, live_ref(v, trip))))
        v = v[:8]
        c.append(Case("CALL_NESTED[%d] %d iterations" % (i, trip), OPS["CALL_NESTED"], rec(12, v, [trip]), out(12, nested_ref(v, trip))))
    return c


FAMILIES = {"fp": fam_fp, "f28": fam_f28, "lin": fam_lin, "f2": fam_f2, "points": fam_points, "m30": fam_m30,
            "inv": fam_inv, "fr": fam_fr, "call": fam_call}
_cache = {}


def family(name):
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]


def arrangements(cases):
    """the two lane orders of one family: by opcode (op-uniform waves; one lane is repeated where the count is a
    multiple of 64, so that the last wave is partial), and interleaved (every opcode spread evenly over the batch, so
    that neighbouring lanes carry different opcodes wherever the family has more than one left)"""
    idx = sorted(range(len(cases)), key=lambda i: (cases[i].op, i))
    uniform = idx + ([idx[0]] if len(idx) % 64 == 0 else [])
    count, seen, key = {}, {}, {}
    for i in idx:
        count[cases[i].op] = count.get(cases[i].op, 0) + 1
    for i in idx:
        k = seen.get(cases[i].op, 0)
        seen[cases[i].op] = k + 1
        key[i] = ((k + cases[i].op * 0.6180339887 % 1) / count[cases[i].op], cases[i].op)  # a phase per opcode
    return uniform, sorted(idx, key=lambda i: key[i])
