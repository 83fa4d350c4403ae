"""CPU: the integer model of the pairing interpreter (tests/vm_model.py) and the cases of tests/vm_cases.py.

* the model, run on the words of gen_pairing_vm.emit (parsed as the device reads them: phase descriptors, 32-word
  records in two halves, the running sum of the counts), gives the node graph's outputs (gen_pairing_vm.evaluate) for one
  record of every program, with the representation contract asserted at every store. This ties the emitted words to the
  node graph without a device. The committed pairing_vm.hpp parses to the same words.
* every hand-built case satisfies the contract under the model alone, in both arrangements, which agree.
* vm_finish at the edges, column by column, under both rounding forms of the quotient.
* no product path launches the debug kernel, and DH_VM_PROF stays off.
"""
import os
import random
import re
from fractions import Fraction

import pytest

import vm_cases as C
import vm_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drand_amd", "csrc")
P = M.P


@pytest.fixture(scope="module")
def emitted():
    import gen_pairing_vm as g
    text = g.emit([C.graph(tag) for tag in g.TAGS])
    return text, M.parse_hpp(text)


def test_tags_and_input_names():
    import gen_pairing_vm as g
    assert g.TAGS == M.TAGS and (g.REC, g.MAXT, g.MAXC) == (M.REC, M.MAXT, C.MAXC)
    for tag in M.TAGS:
        C.graph(tag)  # asserts the input names


def test_model_on_emitted_words_gives_the_graph_outputs(emitted):
    _, progs = emitted
    stores = 0
    for tag in M.TAGS:
        p = progs[tag]
        name, inputs = C.records(tag)[1]
        S = p.stage(inputs)
        writer, _ = M.run(p, S)  # asserts the contract at every store
        stores += p.nops
        got = [M.val(S[M.SW * s:M.SW * s + 14]) * C.RPINV % P for s in p.out_slot]
        assert got == C.evaluate(tag, inputs), "%s, record '%s'" % (tag, name)
        assert all(writer[s] >= 0 for s in p.out_slot)
    assert stores > 130000


def test_committed_header_parses_to_the_same_words(emitted):
    _, progs = emitted
    for tag in M.TAGS:
        a, b = progs[tag], M.committed(tag)
        for f in ("ph_words", "op_words", "nslots", "in_slot", "out_slot", "const_slot", "const_val"):
            assert getattr(a, f) == getattr(b, f), (tag, f)


def test_quotient_is_rounded_once():
    """the ratio of two integers that vm_model.quotient uses is the correctly rounded value of the exact expression"""
    rng = random.Random(7)
    c = Fraction(M.C)
    for _ in range(20000):
        top = rng.randrange(-(1 << rng.randrange(1, 40)), 1 << rng.randrange(1, 40))
        exact = float(Fraction(top) * c - Fraction(1, 1024))
        assert M.quotient(top) == int(exact // 1)


def test_boundary_cases_sit_on_the_rounding_boundary():
    """each BOUNDARY_TOPS entry: the quotient moves by one when vm_finish's constant moves by one unit in its last
    place, so a build with another digit there gives another representative on that case"""
    def q(top, cm):
        return int(((top * cm - (1 << (M.CE - 10))) / (1 << M.CE)) // 1)
    down = up = 0
    for t, s in zip(C.BOUNDARY_TOPS, C.BOUNDARY):
        assert (30 * C.MAXC * C.VALUES[s]) >> 364 == t
        assert q(t, M.CM) == M.quotient(t)
        down += q(t, M.CM - 1) != q(t, M.CM)
        up += q(t, M.CM + 1) != q(t, M.CM)
        assert q(t, M.CM - 1) != q(t, M.CM) or q(t, M.CM + 1) != q(t, M.CM)
    assert down >= 4 and up >= 4


@pytest.mark.parametrize("fam", list(C.FAMILIES))
def test_hand_built_cases_keep_the_contract(fam):
    cases = C.family(fam)
    assert len({c[0] for c in cases}) == len(cases), "case names are unique"
    pair, lane = C.arrange(fam, cases, "pair"), C.arrange(fam, cases, "lane")
    assert len(pair) == len(lane) and sum(len(h.names) for h in pair) == len(cases)
    for hp, hl in zip(pair, lane):
        for kind, cnt, _ in hp.program().phases:
            assert cnt <= 32
        for kind, cnt, _ in hl.program().phases:
            assert kind == M.PH_INV or 33 <= cnt <= 64
        sp, wp = hp.expect()
        sl, wl = hl.expect()
        assert hp.names == hl.names
        for dst in hp.names:
            assert wp[dst] >= 0 and wl[dst] >= 0
            assert sp[M.SW * dst:M.SW * dst + M.SW] == sl[M.SW * dst:M.SW * dst + M.SW], hp.names[dst]


def test_lin_cases_cross_the_word_boundary_of_the_exchange():
    """among the LIN cases whose halves differ in sign, limbs whose low 32-bit words carry into the high word when the
    pair's two partial sums are added, and limbs whose low words do not"""
    carry = nocarry = 0
    for name, kind, a, b in C.family("lin") + C.family("kp"):
        if not a or not b:
            continue
        for j in range(14):
            sa = sum(c * M.limbs(C.VALUES[s])[j] for s, c in a)
            sb = sum(c * M.limbs(C.VALUES[s])[j] for s, c in b)
            if (sa < 0) != (sb < 0) and sa and sb:
                if (sa & 0xFFFFFFFF) + (sb & 0xFFFFFFFF) >> 32:
                    carry += 1
                else:
                    nocarry += 1
    assert carry > 100 and nocarry > 100


def test_shapes_keep_the_contract():
    counts = set()
    for h in C.shapes() + [C.small()]:
        h.expect()
        counts |= {cnt for _, cnt, _ in h.program().phases}
    assert {1, 31, 32, 33, 63, 64} <= counts


def test_finish_at_the_edges_under_both_roundings():
    """slot values 0, 1, p - 1, p, p + 1, 2p - 1 and 1, 15, 16, 30 equal terms at +-32767 and +-1: the reduction, run
    column by column, leaves no carry and a value below 2p under the single rounding of the build and under a separate
    product and difference; the two agree. A V that is a multiple of p (0 among them) leaves p exactly: the quotient's
    bias of 2^-10 keeps one p. The largest result is p + 30 * 32767, from V = k p + k (30 terms of 32767 on p + 1, of
    -32767 on 2p - 1)."""
    largest = 0
    for v in C.EDGE:
        l = M.limbs(v)
        for n in (1, 15, 16, 30):
            for c in (32767, -32767, 1, -1):
                acc = [n * c * x for x in l]
                r1, r2 = M.finish(acc, True), M.finish(acc, False)  # both assert c + c2 == 0 and the 64-bit columns
                assert r1 == r2
                r = M.val(r1)
                assert r < 2 * P and r % P == n * c * v % P
                assert v % P or r == P
                largest = max(largest, r)
    assert largest == P + 30 * 32767
    rng = random.Random(11)
    for _ in range(3000):  # and on random sums: the two forms agree
        terms = [(rng.randrange(2 * P), rng.randint(-32767, 32767)) for _ in range(rng.randint(1, 30))]
        acc = [sum(c * M.limbs(v)[j] for v, c in terms) for j in range(14)]
        assert M.finish(acc, True) == M.finish(acc, False)


def test_from_fp_records():
    for n in (6, 14):
        recs = C.from_fp_records(n)
        assert all(len(r) == n and all(0 <= x < P for x in r) for r in recs)
        flat = [x for r in recs for x in r]
        assert {0, 1, P - 1} <= set(flat)
        for x in flat:
            assert M.val(M.from_fp(x)) % P == (x << 8) % P and M.val(M.from_fp(x)) < 2 * P


def test_debug_entry_is_the_only_caller():
    n = 0
    for name in os.listdir(CSRC):
        if name.endswith((".cpp", ".hip", ".hpp")):
            with open(os.path.join(CSRC, name)) as f:
                txt = f.read()
            assert not re.search(r"^\s*#\s*define\s+DH_VM_PROF", txt, re.M), name
            if name != "k_vm.hip":
                assert "k_vm_debug" not in txt, name
                n += len(re.findall(r"launch_vm_debug\(", txt))
    assert n == 2  # the declaration (kernels.hpp) and dh_vm_debug's call (drandhip.cpp)
    with open(os.path.join(CSRC, "k_vm.hip")) as f:
        txt = f.read()
    assert len(re.findall(r"k_vm_debug\b", txt)) == 2 and len(re.findall(r"launch_vm_debug\(", txt)) == 1  # defined, launched once
    with open(os.path.join(CSRC, "drandhip.cpp")) as f:
        txt = f.read()
    body = txt[txt.index("int dh_vm_debug("):txt.index("int dh_msm_level0_shape_debug(")]
    assert "launch_vm_debug(" in body
    with open(os.path.join(ROOT, "drand_amd", "Makefile")) as f:
        assert "DH_VM_PROF" not in f.read()
