"""GPU: the field layers op by op at their bounds (dh_field_ops_debug, drand_amd/csrc/k_fieldops.hip).

The suite otherwise reaches fp.hpp, fp_mul28.hpp, fp28.hpp, fp2_28.hpp, fp_mul30.hpp, inv_bingcd.hpp and fr.hpp only
through verifications, hashes and MSMs, whose operands are uniformly random. Here every operation runs alone, one
lane each, on the cases of tests/field_ops_cases.py: values at 0, 1, p - 1, the limb boundaries of the three
representations, lazy representatives at each formula's stated entry bound, unnormalised limbs at the worst pattern
the carry-free sums produce, f28_red on every multiple of p below 2^392 and its neighbours, and the product call
convention with twelve values live across a loop of calls and with a call under a divergent branch.

* one test per op family; the family's cases go to the device in one call per lane arrangement: by opcode (op-uniform
  waves, the last one partial) and interleaved (neighbouring lanes carry different opcodes, so every operation is
  entered with part of the wave masked off). Every record is compared (exact words, or the contract where the
  representative is free), the two arrangements must agree word for word, and a failure names its cases.
* one cheap op on 1, 63, 64, 65 and 257 lanes (wave and workgroup edges), once with records wider than the minimum.
* the entry's refusals.
The expected records are integers only (pow, %, the exact Montgomery quotient, the oracle's affine curve arithmetic);
tests/test_field_ops_cases.py checks the generator itself on the CPU.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import field_ops_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 257)
FILL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def lib():
    from test_gpu_h2c_chain import init_gpu
    return init_gpu()[1]


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run(lib, cases, order, in_words=C.IN_WORDS, out_words=C.OUT_WORDS):
    from drand_amd import _lib
    n = len(order)
    ops = np.array([cases[i].op for i in order], np.uint32)
    recs = np.zeros((n, in_words), np.uint32)
    recs[:, :C.IN_WORDS] = np.array([cases[i].rec for i in order], np.uint32)
    out = np.full((n, out_words), FILL, np.uint32)
    assert lib.dh_field_ops_debug(ptr(ops), ptr(recs), in_words, n, ptr(out), out_words) == 0, _lib.last_error()
    return out


def failures(cases, order, out):
    """the names of the cases whose record is wrong, with the first wrong word of each"""
    bad = []
    exact = [k for k, i in enumerate(order) if cases[i].exp is not None]
    if exact:
        want = np.array([cases[order[k]].exp for k in exact], np.uint32)
        got = out[exact][:, :C.OUT_WORDS]
        for r in np.nonzero((want != got).any(axis=1))[0]:
            w = int(np.nonzero(want[r] != got[r])[0][0])
            bad.append("%s: word %d is %08x, expected %08x" % (cases[order[exact[r]]].name, w, got[r, w], want[r, w]))
    for k, i in enumerate(order):
        if cases[i].check is not None:
            try:
                cases[i].check([int(x) for x in out[k, :C.OUT_WORDS]])
            except AssertionError as e:
                bad.append(str(e) or cases[i].name)
    return bad


def report(bad):
    return "%d cases fail:\n  %s" % (len(bad), "\n  ".join(bad[:25]))


@pytest.mark.parametrize("fam", list(C.FAMILIES))
def test_family(lib, fam):
    cases = C.family(fam)
    uniform, inter = C.arrangements(cases)
    assert len(uniform) % 64 != 0
    o1 = run(lib, cases, uniform)
    o2 = run(lib, cases, inter)
    bad = failures(cases, uniform, o1)
    assert not bad, "by opcode: " + report(bad)
    bad = failures(cases, inter, o2)
    assert not bad, "interleaved: " + report(bad)
    pos = {}
    for k, i in enumerate(uniform):
        pos.setdefault(i, k)
    differ = [cases[i].name for k, i in enumerate(inter) if not np.array_equal(o1[pos[i]], o2[k])]
    assert not differ, "the two lane arrangements disagree: " + report(differ)


@pytest.mark.parametrize("n", SIZES)
def test_sizes(lib, n):
    cases = [c for c in C.family("fp") if c.op == C.OPS["FP_ADD"]][:n]
    assert len(cases) == n
    out = run(lib, cases, list(range(n)))
    bad = failures(cases, list(range(n)), out)
    assert not bad, report(bad)


def test_wider_records(lib):
    cases = [c for c in C.family("fp") if c.op in (C.OPS["FP_SUB"], C.OPS["FP_MUL"])][:130]
    order = list(range(len(cases)))
    out = run(lib, cases, order, C.IN_WORDS + 5, C.OUT_WORDS + 9)
    bad = failures(cases, order, out)
    assert not bad, report(bad)
    assert not out[:, C.OUT_WORDS:].any(), "words beyond the result record's minimum are zero"


def test_refusals(lib):
    from drand_amd import _lib
    ops = np.array([C.OPS["FP_ADD"], C.OPS["FP_MUL"]], np.uint32)
    recs = np.zeros((2, C.IN_WORDS), np.uint32)
    out = np.zeros((2, C.OUT_WORDS), np.uint32)
    call = lib.dh_field_ops_debug
    assert call(None, None, 0, 0, None, 0) == 0
    assert call(ptr(ops), ptr(recs), C.IN_WORDS, 0, ptr(out), C.OUT_WORDS) == 0
    for args in ((None, ptr(recs), ptr(out)), (ptr(ops), None, ptr(out)), (ptr(ops), ptr(recs), None)):
        assert call(args[0], args[1], C.IN_WORDS, 2, args[2], C.OUT_WORDS) == _lib.DH_EINVAL
        assert "null" in _lib.last_error()
    assert call(ptr(ops), ptr(recs), C.IN_WORDS - 1, 2, ptr(out), C.OUT_WORDS) == _lib.DH_EINVAL
    assert "operand records" in _lib.last_error()
    assert call(ptr(ops), ptr(recs), C.IN_WORDS, 2, ptr(out), C.OUT_WORDS - 1) == _lib.DH_EINVAL
    assert "result records" in _lib.last_error()
    for op in (10, 25, 47, 63, 79, 101, 112 + 7, 124, 136, 143, 150, 154, 0xFFFFFFFF):
        bad = np.array([C.OPS["FP_ADD"], op], np.uint32)
        assert call(ptr(bad), ptr(recs), C.IN_WORDS, 2, ptr(out), C.OUT_WORDS) == _lib.DH_EINVAL, op
        assert "lane 1" in _lib.last_error() and str(op) in _lib.last_error()
    assert not out.any()
