"""GPU: the lane-parallel pairing interpreter op by op (dh_vm_debug, drand_amd/csrc/k_vm.hip k_vm_debug) against the
integer model of tests/vm_model.py, word for word.

Every verdict of the library ends in vm_exec running a program of pairing_vm.hpp, and the rest of the suite sees one bit
of it. Here the whole slot image comes back, after any number of phases:

* committed programs (the __constant__ / __device__ arrays themselves, through DH_VM_PROG): for every tag and record the
  full run's image equals the model's in every word, pad words included; the outputs times R'^-1 equal
  gen_pairing_vm.evaluate on the node graph; one record a tag is also compared at stop = 0, one phase after the first
  INV phase (the middle phase for ML1 and MUL12) and one phase short of the end. A failure names the tag, the record, the
  first wrong slot and the phase that last wrote it.
* hand-built programs (tests/vm_cases.py), one test per family: LIN ops of 1, 15, 16 and 30 terms at +-32767 on values
  next to 2p, halves of opposite sign, sums of 0 and -1; V = k p - 1, k p, k p + 1; product operands through the
  single-term fast path and beside it; inversions of 0, p and the rest; each LIN and product case on lane pairs and one
  op per lane, which must agree. Phase counts of 1, 31, 32, 33, 63, 64 and phases that read the phase before.
* vm_from_fp through committed programs stopped at phase 0; 1, 2 and 65 records; every stop of a small program; the
  entry's refusals (a stop beyond the program's phases is refused, not clamped).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import vm_cases as C  # noqa: E402
import vm_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
SW = M.SW
FILL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def lib():
    from test_gpu_h2c_chain import init_gpu
    return init_gpu()[1]


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def run_tag(lib, tag, recs, stop=None):
    """recs: [inputs] of a committed program -> (n, nslots * 16) words"""
    from drand_amd import _lib
    p = M.committed(tag)
    words = np.array([C.input_words(tag, r) for r in recs], np.uint32)
    out = np.full((len(recs), p.nslots * SW), FILL, np.uint32)
    stop = len(p.phases) if stop is None else stop
    rc = lib.dh_vm_debug(M.TAGS.index(tag), None, 0, None, 0, 0, stop, ptr(words), words.shape[1], len(recs), ptr(out), out.shape[1])
    assert rc == 0, _lib.last_error()
    return out


def run_hand(lib, h, images=None, stop=None):
    from drand_amd import _lib
    ph, ops = np.array(h.ph_words, np.uint32), np.array(h.op_words, np.uint32)
    img = np.array([h.image] if images is None else images, np.uint32)
    out = np.full(img.shape, FILL, np.uint32)
    stop = len(h.ph_words) // 2 if stop is None else stop
    rc = lib.dh_vm_debug(-1, ptr(ph), len(ph) // 2, ptr(ops), h.nops, h.nslots, stop, ptr(img), img.shape[1], img.shape[0], ptr(out),
                         out.shape[1])
    assert rc == 0, _lib.last_error()
    return out


def first_wrong(got, want, writer, names=None):
    """None, or a description of the first slot whose 16 words differ"""
    want = np.array(want, np.uint32)
    if np.array_equal(got, want):
        return None
    w = int(np.nonzero(got != want)[0][0])
    s = w // SW
    who = (names or {}).get(s)
    return "%sslot %d word %d is %08x, expected %08x; last written by %s" % (
        ("'%s': " % who) if who else "", s, w % SW, got[w], want[w], "phase %d" % writer[s] if writer[s] >= 0 else "the staging")


# ---------------------------------------------------------------------------------------------- committed programs
def _stops(p):
    kinds = [k for k, _, _ in p.phases]
    mid = kinds.index(M.PH_INV) + 2 if M.PH_INV in kinds else len(kinds) // 2
    return (0, mid, len(kinds) - 1)


@pytest.mark.parametrize("tag", M.TAGS)
def test_committed_program(lib, tag):
    p = M.committed(tag)
    recs = C.records(tag)
    got = run_tag(lib, tag, [inp for _, inp in recs])
    bad = []
    for i, (name, inp) in enumerate(recs):
        S = p.stage(inp)
        writer, snaps = M.run(p, S, snapshots=_stops(p) if i == 0 else ())
        d = first_wrong(got[i], S, writer)
        if d:
            bad.append("%s, record %d '%s': %s" % (tag, i, name, d))
        outs = [M.val(S[SW * s:SW * s + 14]) * C.RPINV % M.P for s in p.out_slot]
        assert outs == C.evaluate(tag, inp), "%s, record %d '%s': the model's outputs are not the node graph's" % (tag, i, name)
        if i == 0:
            for stop, want in sorted(snaps.items()):
                part = run_tag(lib, tag, [inp], stop)[0]
                w2, _ = M.run(p, p.stage(inp), stop)
                d = first_wrong(part, want, w2)
                if d:
                    bad.append("%s, record %d '%s', stop %d: %s" % (tag, i, name, stop, d))
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------- hand-built programs
def check_hand(lib, h):
    """the names of the program's wrong slots (at most one line a program: the first), and the device image"""
    got = run_hand(lib, h)[0]
    want, writer = h.expect()
    bad = []
    w = np.array(want, np.uint32)
    for s in np.unique(np.nonzero(got != w)[0] // SW)[:12]:
        k = int(np.nonzero(got[SW * s:SW * s + SW] != w[SW * s:SW * s + SW])[0][0])
        bad.append("%s: '%s' slot %d word %d is %08x, expected %08x (phase %d)" % (
            h.name, h.names.get(int(s), "not a case slot"), s, k, got[SW * s + k], w[SW * s + k], writer[s]))
    return bad, got


@pytest.mark.parametrize("fam", list(C.FAMILIES))
def test_hand_built_family(lib, fam):
    cases = C.family(fam)
    bad = []
    for hp, hl in zip(C.arrange(fam, cases, "pair"), C.arrange(fam, cases, "lane")):
        b1, g1 = check_hand(lib, hp)
        b2, g2 = check_hand(lib, hl)
        bad += b1 + b2
        for dst, name in hp.names.items():
            if not np.array_equal(g1[SW * dst:SW * dst + SW], g2[SW * dst:SW * dst + SW]):
                bad.append("%s: '%s': the lane-pair and the one-lane arrangement disagree" % (hp.name, name))
    assert not bad, "%d wrong slots:\n  %s" % (len(bad), "\n  ".join(bad[:30]))


def test_phase_shapes(lib):
    bad = []
    for h in C.shapes():
        bad += check_hand(lib, h)[0]
    assert not bad, "\n  ".join(bad[:30])


@pytest.mark.parametrize("tag", ("NP1", "NP2C", "NP2J"))
def test_from_fp(lib, tag):
    """vm_from_fp (and vm_load's constants) through a committed program stopped at phase 0: vm_stage_pairs for NP1, the
    check kernels' own staging for NP2C and NP2J"""
    p = M.committed(tag)
    recs = C.from_fp_records(len(p.in_slot))
    got = run_tag(lib, tag, recs, 0)
    bad = []
    for i, r in enumerate(recs):
        d = first_wrong(got[i], p.stage(r), [-1] * p.nslots)
        if d:
            bad.append("%s record %d: %s (inputs %s)" % (tag, i, d, ", ".join("%x" % x for x in r)))
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("n", (1, 2, 65))
def test_sizes(lib, n):
    h = C.shapes()[-1]  # the chain of phases: products, LIN ops and inversions on what the phase before wrote
    images = C.random_images(n, h.nslots, C.NV, 4000 + n)
    got = run_hand(lib, h, images)
    for i, img in enumerate(images):
        S = list(img)
        writer, _ = M.run(h.program(), S)
        d = first_wrong(got[i], S, writer, h.names)
        assert not d, "record %d of %d: %s" % (i, n, d)
    if n == 2:  # a committed program on two records at once
        recs = [inp for _, inp in C.records("MUL12")[:2]]
        p = M.committed("MUL12")
        out = run_tag(lib, "MUL12", recs)
        for i, inp in enumerate(recs):
            S = p.stage(inp)
            writer, _ = M.run(p, S)
            assert not first_wrong(out[i], S, writer)


def test_every_stop(lib):
    h = C.small()
    prog = h.program()
    n = len(prog.phases)
    S = list(h.image)
    _, snaps = M.run(prog, S, snapshots=range(n + 1))
    for stop in range(n + 1):
        w, _ = M.run(prog, list(h.image), stop)
        d = first_wrong(run_hand(lib, h, stop=stop)[0], snaps[stop], w, h.names)
        assert not d, "stop %d: %s" % (stop, d)


def test_refusals(lib):
    from drand_amd import _lib
    h = C.small()
    ph0, ops0 = np.array(h.ph_words, np.uint32), np.array(h.op_words, np.uint32)
    img = np.array([h.image], np.uint32)
    out = np.zeros_like(img)
    nph = len(ph0) // 2

    def call(ph=ph0, nphases=nph, ops=ops0, nops=h.nops, nslots=h.nslots, stop=nph, image=img, in_words=None, n=1, o=out, out_words=None, tag=-1):
        return lib.dh_vm_debug(tag, ptr(ph), nphases, ptr(ops), nops, nslots, stop, ptr(image), img.shape[1] if in_words is None else in_words,
                               n, ptr(o), out.shape[1] if out_words is None else out_words)

    def refused(what, **kw):
        assert call(**kw) == _lib.DH_EINVAL, what
        assert what in _lib.last_error(), (what, _lib.last_error())

    assert call() == 0, _lib.last_error()
    assert call(n=0, ph=None, ops=None, image=None, o=None) == 0
    assert lib.dh_vm_debug(0, None, 0, None, 0, 0, 0, None, 0, 0, None, 0) == 0
    out[:] = 0
    for kw in (dict(ph=None), dict(ops=None), dict(image=None), dict(o=None)):
        refused("null", **kw)
    many = np.zeros(2 * (C.VM_MAX_PHASES + 1), np.uint32)  # empty MUL phases
    refused("phases: at most", ph=many, nphases=C.VM_MAX_PHASES + 1, ops=ops0[:0], nops=0, stop=0)
    big = np.zeros((1, (C.VM_SLOTS + 1) * SW), np.uint32)
    refused("slots: 1 to", nslots=C.VM_SLOTS + 1, image=big, in_words=big.shape[1], o=big.copy(), out_words=big.shape[1])
    refused("slots: 1 to", nslots=0, in_words=0, out_words=0)

    def with_ph(i, v):
        p = ph0.copy()
        p[i] = v
        return p

    def with_op(i, v):
        o = ops0.copy()
        o[i] = v
        return o

    refused("kind 3", ph=with_ph(0, 3 | (2 << 8)))
    refused("at most 64", ph=with_ph(0, 0 | (65 << 8)))
    refused("INV phase of 2 ops", ph=with_ph(4, 2 | (2 << 8)))
    refused("INV phase of 0 ops", ph=with_ph(4, 2))
    refused("not the running sum", ph=with_ph(3, 1))
    refused("ops end at", nops=h.nops - 1, ops=ops0[:-32])
    refused("ops given", nops=h.nops + 1, ops=np.concatenate([ops0, np.zeros(32, np.uint32)]))
    refused("ops end at", ph=with_ph(4, 1 | (2 << 8)))
    refused("terms, at most", ops=with_op(0, int(ops0[0]) & 0xffff | (16 << 16) | (1 << 24)))
    refused("terms, at most", ops=with_op(0, int(ops0[0]) & 0xffff | (1 << 16) | (16 << 24)))
    refused("word 16", ops=with_op(16, 2 << 16))
    inv2 = ops0.copy()  # the INV op (record 3) given a second half of one term
    inv2[96] |= 1 << 24
    inv2[96 + 16], inv2[96 + 17] = 1 << 16, C.S1 | (1 << 16)
    refused("INV op with a second half", ops=inv2)
    refused("slot index", ops=with_op(0, h.nslots | (1 << 16) | (1 << 24)))           # a result slot
    refused("slot index", ops=with_op(1, h.nslots | (1 << 16)))                       # a term of the first half
    refused("slot index", ops=with_op(17, 0xffff | (1 << 16)))                        # a term of the second half
    refused("past its half's count", ops=with_op(2, C.S1 | (1 << 16)))
    refused("past its half's count", ops=with_op(31, 1))
    refused("two ops write", ops=with_op(32, int(ops0[32]) & 0xffff0000 | C.NV))
    refused("reads a slot the phase writes", ops=with_op(1, (C.NV + 1) | (1 << 16)))
    refused("stop 4 beyond", stop=nph + 1)
    refused("slot images of", in_words=img.shape[1] - 1)
    refused("result records of", out_words=out.shape[1] + 1)
    refused("program tag", tag=8)
    refused("program tag", tag=-2)
    refused("more than 65536", n=65537)
    # a committed program: its own record size, stop within its phases
    p = M.committed("MUL12")
    words = np.zeros((1, 24 * SW), np.uint32)
    o12 = np.zeros((1, p.nslots * SW), np.uint32)
    com = lambda **kw: lib.dh_vm_debug(3, None, 0, None, 0, 0, kw.get("stop", 3), ptr(words), kw.get("in_words", 24 * SW), 1, ptr(o12),  # noqa: E731
                                       kw.get("out_words", p.nslots * SW))
    assert com() == 0, _lib.last_error()
    assert com(stop=4) == _lib.DH_EINVAL and "beyond" in _lib.last_error()
    assert com(in_words=24 * 12) == _lib.DH_EINVAL and "input records" in _lib.last_error()
    assert com(out_words=p.nslots * SW - 1) == _lib.DH_EINVAL and "result records" in _lib.last_error()
    assert not out.any(), "a refused call writes nothing"
