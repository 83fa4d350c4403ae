"""CPU: the fixed-exponent Fp chains (fp.hpp fp28_pow_sched) replayed on Python integers from the schedules that the
kernels read, parsed out of the generated consts.hpp: table build, first entry, squarings, table index, terminating
entry, exactly as the device loop runs them. Checks the result against pow(x, e, p), every table index against the
table size, the one-step-ahead read against the array length, and the cost of each schedule: at most 88 field
products beyond the chain squarings (table build and the two domain conversions included), and, since the dictionary
spends squarings on its all-ones entry, no more MADs (392 per product, 301 per squaring) than a plain w = 4 window.
The committed header must also be what the generator writes."""
import os
import random
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "drand_amd", "tools"))
import gen_consts as G  # noqa: E402

P = G.P
EXPONENTS = {"SCHED_SQRT": (P + 1) // 4, "SCHED_SR1_C1": (P - 3) // 4, "SCHED_INV": P - 2, "SCHED_LEGENDRE": (P - 1) // 2}
MAX_PRODUCTS = 88
MADS_MUL, MADS_SQR = 392, 301


def _header():
    with open(os.path.join(ROOT, "drand_amd", "csrc", "consts.hpp")) as f:
        return f.read()


def _int(txt, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, txt).group(1))


def _sched(txt, name):
    m = re.search(r"uint32_t %s\[(\d+)\] = \{([^}]*)\};" % name, txt)
    arr = [int(v, 16) for v in m.group(2).split(",")]
    assert len(arr) == int(m.group(1))
    return arr, _int(txt, name + "_LEN")


class Counter:
    def __init__(self):
        self.mul = self.sqr = 0

    def m(self, a, b):
        self.mul += 1
        return a * b % P

    def s(self, a):
        self.sqr += 1
        return a * a % P


def replay(x, arr, length, W, ODD, RUNS, TAB, c):
    """fp_pow_sched: conversion in, fp28_pow_sched's table build and loop, conversion out."""
    assert ODD == 1 << (W - 1) and TAB == ODD + RUNS
    x = c.m(x, 1)  # fp28_from: one product with 2^400 mod p
    tab = [None] * TAB
    x2 = c.s(x)
    t = x
    tab[0] = t
    for k in range(1, ODD):
        t = c.m(t, x2)
        tab[k] = t
    r = W
    for k in range(RUNS):
        h = t
        for _ in range(r):
            t = c.s(t)
        t = c.m(t, h)
        tab[ODD + k] = t
        r *= 2
    assert arr[0] < TAB
    acc = tab[arr[0]]
    assert 1 < len(arr)
    nxt = arr[1]
    chain_sq = 0
    for i in range(1, length):
        op = nxt
        assert i + 1 < len(arr), "read one step ahead leaves the array"
        nxt = arr[i + 1]
        nsq, k = op >> 8, op & 0xFF
        assert k == 0xFF or k < TAB, (i, k)
        e = tab[0 if k == 0xFF else k]
        for _ in range(nsq):
            acc = c.s(acc)
        chain_sq += nsq
        if k != 0xFF:
            acc = c.m(acc, e)
    assert arr[length] == 0  # the terminating entry
    return c.m(acc, 1), chain_sq  # fp28_to: one product with 2^384 mod p


def _values():
    rng = random.Random(2024)
    return [0, 1, 2, P - 1, P - 2] + [rng.randrange(P) for _ in range(20)]


def test_schedules_compute_the_exponents_within_the_product_limit():
    txt = _header()
    W, ODD, RUNS, TAB = (_int(txt, n) for n in ("SCHED_W", "SCHED_ODD", "SCHED_RUNS", "SCHED_TAB"))
    for name, e in EXPONENTS.items():
        arr, length = _sched(txt, name)
        for x in _values():
            c = Counter()
            got, chain_sq = replay(x, arr, length, W, ODD, RUNS, TAB, c)
            assert got == pow(x, e, P), (name, x)
        # the issue's limit: products beyond the chain squarings, table build and conversions included
        assert c.mul <= MAX_PRODUCTS, (name, c.mul)
        # squarings outside the parse (x^2 and the all-ones entries) are paid for: no more MADs than plain w = 4
        plain = G.dict_schedule(e, 4, 0)
        pm, ps = G.schedule_cost(plain, 4, 0)
        assert pm <= MAX_PRODUCTS
        assert c.mul * MADS_MUL + c.sqr * MADS_SQR <= pm * MADS_MUL + ps * MADS_SQR, (name, c.mul, c.sqr, pm, ps)
        assert (c.mul, c.sqr) == G.schedule_cost(arr[:length]), name
        assert chain_sq <= e.bit_length() - 1


def test_generator_parse_is_exact_for_other_dictionaries():
    """dict_schedule's own check (acc == e) over the window / run combinations the header's comment quotes."""
    for w, runs in ((3, 0), (3, 2), (4, 0), (4, 1), (4, 2), (5, 0)):
        words = G.dict_words(w, runs)
        for e in EXPONENTS.values():
            ops = G.dict_schedule(e, w, runs)
            acc = words[ops[0]]
            for op in ops[1:]:
                acc <<= op >> 8
                if op & 0xFF != 0xFF:
                    assert op & 0xFF < len(words)
                    acc += words[op & 0xFF]
            assert acc == e


def test_committed_header_matches_generator():
    txt = _header()
    for name, e in EXPONENTS.items():
        arr, length = _sched(txt, name)
        assert arr == G.dict_schedule(e) + [0] and length == len(arr) - 1
    assert _int(txt, "SCHED_W") == G.SCHED_W and _int(txt, "SCHED_RUNS") == G.SCHED_RUNS
