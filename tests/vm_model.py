"""A limb-exact integer model of the lane-parallel pairing interpreter (drand_amd/csrc/k_vm.hip: vm_load_rec, vm_lin_acc,
vm_lin, vm_finish, vm_mul, vm_inv, vm_from_fp, vm_exec), on Python integers only. Test infrastructure for
tests/test_vm_model.py (CPU), tests/test_gpu_vm.py (the device's slot images against this model's, word for word) and
tests/test_pairing_program.py.

The model runs a program from its emitted words, as the device reads them, never from the generator's node graph:
PHASES words (kind | cnt << 8, then the phase's first op, which must be the running sum of the counts), OPS records of
REC = 32 words in two 16-word halves (word 0 = dst | na << 16 | nb << 24, words 1..15 the first half's terms; word 16
carries the second half's count at bits 16..23, words 17..31 its terms; a term = slot | (coefficient & 0xffff) << 16)
and a slot image of 16 words a slot (14 limbs of 28 bits, two pad words that no op writes).

The device runs a phase of at most 32 LIN or product ops on lane pairs (each lane one half, the partial sums or the
operand values exchanged) and wider phases one op per lane over both halves. Both give the same integers: a LIN op's two
halves are summed before the one reduction, a product's operands are reduced apart. The model has this one path.

While it runs the model asserts the representation contract at every store: limbs below 2^28, value below 2p (below
1.002 p for products and inversions), the reduction's remaining carry c + c2 == 0, its quotient inside int32, every
per-limb sum and carry inside int64.
"""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from field_ops_cases import MASK, P, PL, RP, limbs, montq, qlimbs, val  # noqa: E402,F401

REC, MAXT, SW = 32, 15, 16
PH_MUL, PH_LIN, PH_INV = 0, 1, 2
C_HEX = "0x1.3b06ba5e7993dp-17"  # vm_finish's 2^364 / p
C = float.fromhex(C_HEX)
RP3 = pow(RP, 3, P)
I64 = 1 << 63
TAGS = ("NP1", "NP2", "ML1", "MUL12", "FE", "NP2C", "NP1J", "NP2J")
F12_TAGS = ("MUL12", "FE")  # their inputs are VM-form slots (vm_f12_in), the others' 12-word Montgomery values


def _i64(x, what):
    assert -I64 <= x < I64, "%s leaves int64" % what
    return x


CM, CE = int(C * (1 << 69)), 69  # C = CM / 2^69 exactly (53 significant bits)
assert CM / (1 << CE) == C and CM < 1 << 53


def quotient(top, fused=True):
    """vm_finish's q = floor(fl(top * C - 2^-10)) for the exact integer top. fused: one rounding of the exact
    expression (v_fma_f64, what the gfx950 build does: the ratio of two Python integers is correctly rounded, as is
    float(Fraction)); otherwise a rounded product, then a rounded difference."""
    assert abs(top) < 1 << 53, "top is not exact in a double"
    if fused:
        qd = (top * CM - (1 << (CE - 10))) / (1 << CE)
    else:
        qd = float(top) * C - 2.0 ** -10
    q = int(qd // 1)
    assert -(1 << 31) <= q < 1 << 31, "q leaves int32"
    return q


def finish_value(V, fused=True):
    """vm_finish on the integer V = sum_j acc_j 2^(28 j): the signed carry pass leaves the unique l_j in [0, 2^28) and
    carry c with V = sum l_j 2^(28 j) + c 2^392, whatever the per-limb sums were; the second pass leaves V - q p in 14
    limbs exactly when its carry c2 = -c. Returns the reduced value (its limbs: limbs())."""
    c, low = V >> 392, V & (RP - 1)
    q = quotient(c * (1 << 28) + (low >> 364), fused)
    r = V - q * P
    assert 0 <= r < RP, "the reduced value left 14 limbs: c + c2 = %d" % (r >> 392)
    return r


def finish(acc, fused=True):
    """vm_finish on 14 signed per-limb sums, column by column as the device runs it -> 14 limbs"""
    l, c = [0] * 14, 0
    for j in range(14):
        t = _i64(_i64(acc[j], "a per-limb sum") + c, "a carry sum")
        l[j], c = t & MASK, t >> 28
    q = quotient(c * (1 << 28) + l[13], fused)
    c2 = 0
    for j in range(14):
        t = _i64(l[j] - q * PL[j] + c2, "a reduction column")
        l[j], c2 = t & MASK, t >> 28
    assert c + c2 == 0, "the reduced value left 14 limbs: c + c2 = %d" % (c + c2)
    assert val(l) == finish_value(sum(a << (28 * j) for j, a in enumerate(acc)), fused)
    return l


def coeff(t):
    """a term word's coefficient: (int32_t)(int16_t)(t >> 16)"""
    return (t >> 16) - (1 << 16) if t >> 31 else t >> 16


def mul(a, b):
    """vm_mul on limb vectors: fp_mul28.hpp mont_mul on raw limbs, the exact quotient (13 masked limbs and what is
    left on top)"""
    return qlimbs(montq(val(a), val(b)))


def inv_value(v):
    """vm_inv on a slot's value (below 2p): None when it is 0 or p (the slot comes back unchanged), else the integer
    inverse of the canonical value times R'^3 through one product"""
    assert v < 2 * P
    x = v - P if v >= P else v
    return None if x == 0 else montq(pow(x, -1, P), RP3)


def from_fp(x, fused=True):
    """vm_from_fp: a 12-word Montgomery value (integer below p) -> split<8> -> vm_finish; 14 limbs"""
    assert 0 <= x < P
    return limbs(finish_value(x << 8, fused))


class Program:
    """phases: [(kind, cnt, first)]; ops: the flat record words (the 16 pad words are not needed here)"""

    def __init__(self, ph_words, op_words, nslots, in_slot=(), out_slot=(), const_slot=(), const_val=(), tag=None):
        assert len(ph_words) % 2 == 0
        self.ph_words, self.op_words, self.nslots, self.tag = list(ph_words), op_words, nslots, tag
        self.in_slot, self.out_slot = list(in_slot), list(out_slot)
        self.const_slot, self.const_val = list(const_slot), [list(v) for v in const_val]
        self.phases, first = [], 0
        for d, f in zip(ph_words[0::2], ph_words[1::2]):
            kind, cnt = d & 0xff, d >> 8
            assert kind <= 2 and cnt <= 64 and (kind != PH_INV or cnt == 1) and d < 1 << 16
            assert f == first, "a phase's first op is not the running sum of the counts"
            self.phases.append((kind, cnt, first))
            first += cnt
        self.nops = first
        assert len(op_words) >= REC * first

    def stage(self, inputs):
        """the slot image before phase 0: zeros, the constants, the inputs as production hands them over"""
        S = [0] * (SW * self.nslots)
        for s, v in zip(self.const_slot, self.const_val):
            S[SW * s:SW * s + 14] = v
        assert len(inputs) == len(self.in_slot)
        for s, x in zip(self.in_slot, inputs):
            if self.tag in F12_TAGS:
                assert len(x) == SW
                S[SW * s:SW * s + SW] = x
            else:
                S[SW * s:SW * s + 14] = from_fp(x)
        return S


def run(prog, S, stop=None, snapshots=(), fused=True):
    """vm_exec on the image S (modified in place; its slots must hold valid values: limbs below 2^28, below 2p).
    Returns (writer, snaps): writer[slot] = the last phase that wrote it (-1: none) and snaps[k] = a copy of the image
    after k phases for every k of `snapshots`.

    Values are summed as integers: with every limb below 2^28 (asserted at every store and on the image) a half's
    per-limb sum is below 15 * 32768 * 2^28 < 2^47 in magnitude and a carry sum below 2^48, so the device's int64
    columns cannot overflow, and the carry pass depends on V alone (finish_value)."""
    W = prog.op_words
    ns = prog.nslots
    assert len(S) == SW * ns
    V = []
    for s in range(ns):
        l = S[SW * s:SW * s + 14]
        assert all(0 <= x <= MASK for x in l), "slot %d: a limb above 2^28" % s
        V.append(val(l))
        assert V[s] < 2 * P, "slot %d holds %.3f p" % (s, V[s] / P)
    assert MAXT * 32768 * (MASK + 1) < 1 << 47
    writer = [-1] * ns
    snaps = {}
    stop = len(prog.phases) if stop is None else stop
    assert 0 <= stop <= len(prog.phases)
    if 0 in snapshots:
        snaps[0] = list(S)

    def total(o, n):
        return sum(coeff(W[o + k]) * V[W[o + k] & 0xffff] for k in range(n))

    def operand(o, n):  # vm_lin: a single term of half-word 1 is the slot itself, unreduced
        if n == 1 and (W[o] >> 16) == 1:
            return V[W[o] & 0xffff]
        return finish_value(total(o, n), fused)

    for ph in range(stop):
        kind, cnt, first = prog.phases[ph]
        res = []
        for k in range(cnt):
            o = REC * (first + k)
            h = W[o]
            dst, na, nb = h & 0xffff, (h >> 16) & 0xff, h >> 24
            nb2 = (W[o + 16] >> 16) & 0xff  # what a pair's odd lane reads as its count
            assert na <= MAXT and nb <= MAXT and nb2 == nb and dst < ns
            assert not any(W[o + 1 + na:o + 16]) and not any(W[o + 17 + nb:o + 32]), "term words past the count"
            keep = None
            if kind == PH_MUL:
                r = montq(operand(o + 1, na), operand(o + 17, nb))
            elif kind == PH_LIN:
                r = finish_value(total(o + 1, na) + total(o + 17, nb), fused)
            else:
                a = operand(o + 1, na)
                r = inv_value(a)
                if r is None:  # a zero comes back as it went in, which may be the representative p
                    r, keep = a, True
            assert r < 2 * P and (kind == PH_LIN or keep or r * 1000 < 1002 * P), "phase %d op %d: %.4f p" % (ph, k, r / P)
            res.append((dst, r))
        for dst, r in res:  # every read of a phase comes before its writes
            S[SW * dst:SW * dst + 14] = limbs(r)
            V[dst] = r
            writer[dst] = ph
        if ph + 1 in snapshots:
            snaps[ph + 1] = list(S)
    return writer, snaps


# ---------------------------------------------------------------------------------------------- the emitted header
def _arrays(text):
    """name -> the words of every array the header defines (each definition is one line)"""
    out = {}
    for line in text.split("\n"):
        if line.startswith("__device__") and "] = {" in line:
            head, body = line.split("] = {", 1)
            name = re.search(r"(\w+)\[[^ ]*$", head).group(1)
            body = body[:body.rindex("};")].replace("{", "").replace("}", "").replace("u", "")
            out[name] = [int(x, 0) for x in body.split(",") if x.strip()]
    return out


def parse_hpp(text, tags=TAGS):
    """pairing_vm.hpp's text (or gen_pairing_vm.emit's) -> {tag: Program}, from the words the device reads"""
    arr = _arrays(text)
    progs = {}
    for tag in tags:
        m = re.search(r"\b%s_NPHASES = (\d+), %s_NSLOTS = (\d+), %s_NCONST = (\d+);" % (tag, tag, tag), text)
        nphases, nslots, nconst = (int(x) for x in m.groups())
        ph, ops, cv, cs = (arr[tag + "_" + n] for n in ("PHASES", "OPS", "CONST_VAL", "CONST_SLOT"))
        assert len(ph) == 2 * nphases and len(cs) == nconst and len(cv) == 14 * nconst
        p = Program(ph, ops, nslots, arr[tag + "_INPUT_SLOT"], arr[tag + "_OUTPUT_SLOT"], cs,
                    [cv[14 * i:14 * i + 14] for i in range(nconst)], tag)
        assert len(ops) == REC * p.nops + REC // 2 and not any(ops[REC * p.nops:]), "the 16 pad words"
        progs[tag] = p
    return progs


_committed = {}


def committed(tag):
    """the committed header's program, parsed once"""
    if not _committed:
        with open(os.path.join(os.path.dirname(HERE), "drand_amd", "csrc", "pairing_vm.hpp")) as f:
            _committed.update(parse_hpp(f.read()))
    return _committed[tag]
