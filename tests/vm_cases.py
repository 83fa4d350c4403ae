"""Records and hand-built programs for the pairing interpreter's debug entry (dh_vm_debug, drand_amd/csrc/k_vm.hip
k_vm_debug), on Python integers only. Test infrastructure for tests/test_vm_model.py (CPU) and tests/test_gpu_vm.py.

* committed programs: four records a tag from the oracle's points (oracle/bls_py.py), built as gen_pairing_vm's
  validate, validate_split and validate_np2c build theirs; MUL12 and FE are fed with the model's own ML1 / MUL12 outputs
  and with 0, 1 and p - 1 as coordinates.
* hand-built programs (the caller's mode): every case is one op on slots holding 0, 1, p - 1, p, p + 1, 2p - 1 and
  random values below 2p. A family's cases are packed into programs of at most 128 case ops (218 slots hold the values,
  one result slot a case and the filler ops' results), each emitted in two arrangements: phases of at most 32 ops (the
  device runs them on lane pairs) and phases of 33 to 64 ops, padded with filler ops (one op per lane). A case writes
  the same slot in both, so the two images must agree on every case slot.
The expected images come from tests/vm_model.py. Nothing here imports the library.
"""
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "drand_amd", "tools"))

import vm_model as M  # noqa: E402
from vm_model import MAXT, P, PH_INV, PH_LIN, PH_MUL, REC, RP, SW, limbs, val  # noqa: E402

R384 = 1 << 384
RPINV = pow(RP, -1, P)
MAXC = 32767
VM_SLOTS = 218         # k_vm.hip VM_SLOTS: the caller's limit
VM_MAX_PHASES = 951    # k_vm.hip VM_MAX_PHASES
CHUNK = 128            # case ops a hand-built program
FILL = 33              # result slots of the filler ops

# the inputs' names in INPUT_SLOT order (tests/test_vm_model.py compares them with the generator's)
_PAIR = ["P%d.x", "P%d.y", "Q%d.x0", "Q%d.x1", "Q%d.y0", "Q%d.y1"]
_PAIRJ = ["P%d.x", "P%d.y", "P%d.z", "Q%d.x0", "Q%d.x1", "Q%d.y0", "Q%d.y1"]
INPUT_NAMES = {
    "NP1": [n % 0 for n in _PAIR], "NP2": [n % k for k in (0, 1) for n in _PAIR], "ML1": [n % 0 for n in _PAIR],
    "MUL12": ["F%d" % i for i in range(12)] + ["G%d" % i for i in range(12)], "FE": ["F%d" % i for i in range(12)],
    "NP2C": ["P0.x", "P0.y", "B.x0", "B.x1", "B.y0", "B.y1", "B.z0", "B.z1", "P1.x", "P1.y", "Q1.x0", "Q1.x1", "Q1.y0", "Q1.y1"],
    "NP1J": [n % 0 for n in _PAIRJ], "NP2J": [n % k for k in (0, 1) for n in _PAIRJ],
}


# ---------------------------------------------------------------------------------------------- committed programs
def _pairs_record(pairs, jac, zs):
    d = {}
    for k, (Pt, Qt) in enumerate(pairs):
        if jac:
            z = zs[k]
            d["P%d.x" % k], d["P%d.y" % k], d["P%d.z" % k] = Pt[0] * z * z % P, Pt[1] * z * z * z % P, z
        else:
            d["P%d.x" % k], d["P%d.y" % k] = Pt
        d["Q%d.x0" % k], d["Q%d.x1" % k] = Qt[0]
        d["Q%d.y0" % k], d["Q%d.y1" % k] = Qt[1]
    return d


def _curve_records(tag):
    import bls_py as B
    rng = random.Random(3001)
    G1, G2 = B.G1_GEN, B.G2_GEN
    a = rng.randrange(2, 1 << 64)
    Pa, Qa = B.ec_mul(B.FP, G1, a), B.ec_mul(B.FP2, G2, a)
    nG1 = B.ec_neg(B.FP, G1)
    jac = tag.endswith("J")
    if tag.startswith("NP2"):
        recs = [("a product that is one", [(G1, G2), (nG1, G2)]), ("bilinearity", [(Pa, G2), (nG1, Qa)]),
                ("e(G1, G2)^2", [(G1, G2), (G1, G2)]), ("e(aG1, G2) e(-G1, G2)", [(Pa, G2), (nG1, G2)])]
    else:
        recs = [("the generators", [(G1, G2)]), ("a multiple of G1", [(Pa, G2)]), ("a multiple of G2", [(G1, Qa)]),
                ("-G1", [(nG1, G2)])]
    out = []
    for i, (name, pairs) in enumerate(recs):
        zs = [1 if i == 3 else rng.randrange(1, P) for _ in pairs]  # the J forms: random Z, and Z = 1
        out.append((name + (", Z = 1" if jac and i == 3 else ""), _pairs_record(pairs, jac, zs)))
    return out


def _np2c_records():
    """test_gpu_small._np2c_cases' records that reach the NP2C program: A and B finite (B + torsion and the small-order B
    whose cleared Z is 0 among them), B Jacobian with a random Z"""
    from test_gpu_small import _np2c_cases
    B, pk, cases = _np2c_cases()
    rng = random.Random(3002)
    ng1 = B.ec_neg(B.FP, B.G1_GEN)
    out = []
    for name, A, Bp, _ in cases:
        if A is None or Bp is None:
            continue
        z = (rng.randrange(1, P), rng.randrange(P))
        z2 = B.f2mul(z, z)
        jx, jy = B.f2mul(Bp[0], z2), B.f2mul(Bp[1], B.f2mul(z2, z))
        out.append((name, {"P0.x": pk[0], "P0.y": pk[1], "B.x0": jx[0], "B.x1": jx[1], "B.y0": jy[0], "B.y1": jy[1],
                           "B.z0": z[0], "B.z1": z[1], "P1.x": ng1[0], "P1.y": ng1[1], "Q1.x0": A[0][0], "Q1.x1": A[0][1],
                           "Q1.y0": A[1][0], "Q1.y1": A[1][1]}))
    assert [n for n, _ in out] == ["clean", "B_small_order_A_finite", "B_plus_torsion", "wrong_sig"]
    return out


def vm_slot(v, pad=(0, 0)):
    """a value below 2^392 as a slot's 16 words"""
    return limbs(v) + list(pad)


def _model_outputs(tag, inputs):
    p = M.committed(tag)
    S = p.stage(inputs)
    M.run(p, S)
    return [S[SW * s:SW * s + SW] for s in p.out_slot]


_records = {}


def records(tag):
    """[(name, inputs)]: the program's inputs in INPUT_SLOT order as the entry takes them: integers x R mod p (R =
    2^384, 12 words each), or for MUL12 and FE slots of 16 words"""
    if tag in _records:
        return _records[tag]
    if tag in ("MUL12", "FE"):
        ml = [_model_outputs("ML1", inp) for _, inp in records("ML1")]
        rng = random.Random(3003)
        edge = [vm_slot(v * RP % P) for v in (0, 1, P - 1)] + [vm_slot(v) for v in (P, P + 1, 2 * P - 1)]
        mul = [("e(G1, G2) x e(-G1, G2)", ml[0] + ml[3]), ("e(aG1, G2) x e(G1, aG2)", ml[1] + ml[2]),
               ("0, 1, p - 1 and their other representatives as coordinates", [edge[i % 6] for i in range(24)]),
               ("random values below 2p, pad words set", [vm_slot(rng.randrange(2 * P), (rng.getrandbits(32), rng.getrandbits(32)))
                                                          for _ in range(24)])]
        if tag == "MUL12":
            out = mul
        else:
            fe_in = [_model_outputs("MUL12", inp) for _, inp in mul[:2]]
            out = [("e(G1, G2) e(-G1, G2)", fe_in[0]), ("e(aG1, G2) e(G1, aG2)", fe_in[1]), ("e(G1, G2) alone", ml[0]),
                   ("0, 1, p - 1 as coordinates, pad words set", [list(edge[(5 * i + 1) % 6][:14]) + [0xA5A5A5A5, i] for i in range(12)])]
    else:
        named = _np2c_records() if tag == "NP2C" else _curve_records(tag)
        out = [(name, [d[k] * R384 % P for k in INPUT_NAMES[tag]]) for name, d in named]
    _records[tag] = out
    return out


def plain_inputs(tag, inputs):
    """the same record as gen_pairing_vm.evaluate takes it: name -> value mod p"""
    if tag in ("MUL12", "FE"):
        return {k: val(x[:14]) * RPINV % P for k, x in zip(INPUT_NAMES[tag], inputs)}
    return {k: x * pow(R384, -1, P) % P for k, x in zip(INPUT_NAMES[tag], inputs)}


_graphs = {}


def graph(tag):
    """the generator's scheduled, slot-allocated node graph of a program (no validation), built once a tag"""
    if tag not in _graphs:
        import gen_pairing_vm as g
        prog, outs = g.build_tag(tag)
        phases, live = g.schedule(prog, outs)
        slot, nslots = g.allocate(prog, outs, phases, live)
        assert [prog.nodes[i]["name"] for i in prog.inputs] == INPUT_NAMES[tag]
        _graphs[tag] = (tag, prog, outs, phases, slot, nslots)
    return _graphs[tag]


def evaluate(tag, inputs):
    """gen_pairing_vm.evaluate on a record: the outputs mod p, from the node graph"""
    import gen_pairing_vm as g
    return g.evaluate(*graph(tag)[1:], plain_inputs(tag, inputs))


def input_words(tag, inputs):
    """a record's words for dh_vm_debug"""
    if tag in ("MUL12", "FE"):
        return [w for x in inputs for w in x]
    return [(x >> (32 * i)) & 0xFFFFFFFF for x in inputs for i in range(12)]


def from_fp_records(n_inputs):
    """raw 12-word values for vm_from_fp, through a committed program stopped at phase 0: 0, 1, p - 1 and their
    neighbours, limb and word boundaries, random values below p"""
    rng = random.Random(3004)
    v = [0, 1, P - 1, 2, P - 2, (P - 1) // 2, R384 % P, (1 << 380), (1 << 380) - 1, (1 << 376) - 1]
    v += [1 << k for k in range(20, 381, 28)] + [(1 << k) - 1 for k in range(32, 381, 32)]
    v += [rng.randrange(P) for _ in range(60)]
    v = [x for x in v if x < P]
    while len(v) % n_inputs:
        v.append(rng.randrange(P))
    return [v[i:i + n_inputs] for i in range(0, len(v), n_inputs)]


# ---------------------------------------------------------------------------------------------- hand-built programs
class Hand:
    """a caller's program: phases = [(kind, [(dst, a_terms, b_terms)])], terms = [(slot, coefficient)]; names[dst] = the
    case whose result lands in slot dst; image = the initial slot words"""

    def __init__(self, name, phases, values, nslots, names):
        self.name, self.nslots, self.names = name, nslots, names
        assert len(values) <= nslots <= VM_SLOTS and len(phases) <= VM_MAX_PHASES
        self.image = [w for v in values for w in (v if isinstance(v, list) else vm_slot(v))] + [0] * (SW * (nslots - len(values)))
        self.ph_words, self.op_words, nops = [], [], 0
        for kind, ops in phases:
            assert len(ops) <= 64 and (kind != PH_INV or len(ops) == 1)
            self.ph_words += [kind | (len(ops) << 8), nops]
            written = {dst for dst, _, _ in ops}
            assert len(written) == len(ops)
            for dst, a, b in ops:
                assert len(a) <= MAXT and len(b) <= MAXT and 0 <= dst < nslots and (kind != PH_INV or not b)
                rec = [0] * REC
                rec[0] = dst | (len(a) << 16) | (len(b) << 24)
                rec[16] = len(b) << 16
                for h, terms in ((1, a), (17, b)):
                    for k, (s, c) in enumerate(terms):
                        assert 0 <= s < nslots and abs(c) <= MAXC and s not in written
                        rec[h + k] = s | ((c & 0xffff) << 16)
                self.op_words += rec
                nops += 1
        self.nops = nops

    def program(self):
        return M.Program(self.ph_words, self.op_words, self.nslots)

    def expect(self, stop=None):
        """(image, writer) of the model"""
        S = list(self.image)
        writer, _ = M.run(self.program(), S, stop)
        return S, writer


EDGE = [0, 1, P - 1, P, P + 1, 2 * P - 1]
S0, S1, SPM1, SP, SPP1, S2PM1 = range(6)
_rng = random.Random(3005)
VALUES = EDGE + [_rng.randrange(2 * P) for _ in range(10)]
RANDS = list(range(6, len(VALUES)))
# vm_finish's quotient estimate top * C - 2^-10 within 2^-32 of an integer: for these top = floor(V / 2^364) the floor
# moves by one when the constant C moves by one unit in its last place (found by a search over top < 2^37.6, the
# largest that 30 terms of 32767 on a value below 2p reach; tests/test_vm_model.py checks each). V = 30 * 32767 * x.
BOUNDARY_TOPS = (111281712156, 114514917904, 127057050773, 130290256521, 142832389390, 146065595138,
                 104815300660, 108048506408, 117357433529, 120590639277, 133132772146, 139599183642)
BOUNDARY = list(range(len(VALUES), len(VALUES) + len(BOUNDARY_TOPS)))
VALUES += [((t << 364) + (1 << 363)) // (30 * MAXC) for t in BOUNDARY_TOPS]
assert all(v < 2 * P and (30 * MAXC * v) >> 364 == t for v, t in zip(VALUES[len(RANDS) + 6:], BOUNDARY_TOPS))
NV = len(VALUES)


def _filler(kind, dst):
    return (dst, [(S1, 1)], [(SPM1, 1)] if kind == PH_MUL else [])


def arrange(fam, cases, mode):
    """cases: [(name, kind, a_terms, b_terms)] -> the programs holding them. Case i of a chunk writes slot NV + i in
    either mode. mode "pair": phases of at most 32 ops; "lane": phases of 33 to 64 ops, padded with fillers; INV ops
    take a phase each in both."""
    progs = []
    for c0 in range(0, len(cases), CHUNK):
        chunk = cases[c0:c0 + CHUNK]
        phases, names, cur = [], {}, []

        def flush():
            if not cur:
                return
            kind = cur[0][0]
            ops = [op for _, op in cur]
            if mode == "lane" and kind != PH_INV and len(ops) < 33:
                ops += [_filler(kind, NV + CHUNK + j) for j in range(33 - len(ops))]
            phases.append((kind, ops))
            del cur[:]

        width = 32 if mode == "pair" else 64
        for i, (name, kind, a, b) in enumerate(chunk):
            if cur and (cur[0][0] != kind or kind == PH_INV or len(cur) == width):
                flush()
            cur.append((kind, (NV + i, a, b)))
            names[NV + i] = name
        flush()
        progs.append(Hand("%s[%d..%d] %s" % (fam, c0, c0 + len(chunk) - 1, mode), phases, VALUES, NV + CHUNK + FILL, names))
    return progs


def _halves(terms):
    return terms[:MAXT], terms[MAXT:]


def fam_lin():
    c = []
    pats = (("+32767", lambda i: MAXC), ("-32767", lambda i: -MAXC), ("+-32767", lambda i: MAXC if i % 2 == 0 else -MAXC),
            ("-+32767", lambda i: -MAXC if i % 2 == 0 else MAXC), ("+1", lambda i: 1), ("-1", lambda i: -1))
    for n in (1, 15, 16, 30):
        for pn, pat in pats:
            for s in range(len(EDGE)):
                c.append(("LIN %d terms %s on slot %d" % (n, pn, s), PH_LIN) + _halves([(s, pat(i)) for i in range(n)]))
            c.append(("LIN %d terms %s on random values" % (n, pn), PH_LIN) + _halves([(RANDS[i % len(RANDS)], pat(i)) for i in range(n)]))
    # the halves' sums of opposite sign: a lane pair exchanges them as two 32-bit words a limb
    for ca, cb in ((-MAXC, MAXC), (MAXC, -MAXC), (-1, 1), (1, -1), (-MAXC, 1), (1, -MAXC), (-3, 2), (2, -3)):
        for sa, sb in ((S2PM1, S2PM1), (S2PM1, SP), (6, 7), (8, 9), (SPM1, SPP1), (7, 6)):
            for n in (15, 1):
                c.append(("LIN halves %d x (%d on slot %d | %d on slot %d)" % (n, ca, sa, cb, sb), PH_LIN, [(sa, ca)] * n, [(sb, cb)] * n))
    for s in (S2PM1, 6):
        for co in (MAXC, 1):
            c.append(("LIN exactly 0: 15 x %d on slot %d in each half" % (co, s), PH_LIN, [(s, co)] * 15, [(s, -co)] * 15))
            c.append(("LIN exactly 0 in one half, %d on slot %d" % (co, s), PH_LIN, [(s, co), (s, -co)], []))
    for s, t in zip(BOUNDARY, BOUNDARY_TOPS):
        c.append(("LIN 30 x 32767, the quotient estimate at an integer (top %d)" % t, PH_LIN, [(s, MAXC)] * 15, [(s, MAXC)] * 15))
    c += [("LIN -1: (p - 1) - p over the halves", PH_LIN, [(SPM1, 1)], [(SP, -1)]),
          ("LIN -1: -p + (p - 1) over the halves", PH_LIN, [(SP, -1)], [(SPM1, 1)]),
          ("LIN -1: (p - 1) - p in one half", PH_LIN, [(SPM1, 1), (SP, -1)], []),
          ("LIN -1: 0 - 1", PH_LIN, [(S0, 1), (S1, -1)], []), ("LIN -1: -1", PH_LIN, [(S1, -1)], []),
          ("LIN -15: 15 (p - 1) - 15 p", PH_LIN, [(SPM1, 1)] * 15, [(SP, -1)] * 15),
          ("LIN no terms", PH_LIN, [], [])]
    return c


def _kterms(k, slot):
    t = []
    while k:
        co = max(-MAXC, min(MAXC, k))
        t.append((slot, co))
        k -= co
    return t


def kp_values():
    """k for V = k p + d: 0, +-1, +-2, +-(2^j +- 1), the largest |k| that 30 (d = 0) and 29 terms reach, 200 random"""
    ks = [0, 1, -1, 2, -2]
    for j in range(2, 20):
        for k in ((1 << j) - 1, (1 << j) + 1):
            ks += [k, -k]
    ks += [30 * MAXC, -30 * MAXC, 29 * MAXC, -29 * MAXC]
    rng = random.Random(3006)
    ks += [rng.randrange(-29 * MAXC, 29 * MAXC + 1) for _ in range(200)]
    return ks


def fam_kp():
    """V = k p - 1, k p, k p + 1 from terms on the slots holding p, p - 1 and 1"""
    c = []
    for i, k in enumerate(kp_values()):
        for d in (-1, 0, 1):
            if d and abs(k) > 29 * MAXC:
                continue
            split = i % 2 == 1 and abs(k) <= 14 * MAXC  # k p as k (p - 1) + k
            t = (_kterms(k, SPM1) + _kterms(k, S1)) if split else _kterms(k, SP)
            if d:
                t.append((S1, d))
            assert len(t) <= 30
            h = (len(t) + 1) // 2
            c.append(("LIN %d p %+d%s" % (k, d, " as k (p - 1) + k" if split else ""), PH_LIN, t[:h], t[h:]))
    return c


def fam_mul():
    rng = random.Random(3008)
    ops = [("1 x slot %d" % s, [(s, 1)]) for s in range(NV)]
    ops += [("%d x slot %d" % (co, s), [(s, co)]) for s in range(len(EDGE)) for co in (-1, 3, MAXC, -MAXC)]
    ops += [("-1 x slot 6", [(6, -1)]), ("slot 6 + slot 7", [(6, 1), (7, 1)]), ("slot 8 - slot 9", [(8, 1), (9, -1)]),
            ("32767 (slot 5 - slot 10)", [(S2PM1, MAXC), (10, -MAXC)]), ("slot 3 - slot 3", [(SP, 1), (SP, -1)]),
            ("15 x 32767 on 2p - 1", [(S2PM1, MAXC)] * 15), ("15 x -32767 on 2p - 1", [(S2PM1, -MAXC)] * 15),
            ("15 x +-32767 on 2p - 1", [(S2PM1, MAXC if i % 2 == 0 else -MAXC) for i in range(15)]),
            ("15 random terms", [(RANDS[i % len(RANDS)], rng.randint(-MAXC, MAXC)) for i in range(15)]),
            ("4 terms", [(6, 5), (7, -7), (SP, 11), (S1, -1)]), ("5 terms", [(11, 1), (12, 1), (13, 1), (14, 1), (15, -4)]),
            ("no terms", [])]
    c = []
    for i, (na, a) in enumerate(ops):
        nb, b = ops[(7 * i + 3) % len(ops)]
        c.append(("MUL (%s) (%s)" % (na, nb), PH_MUL, a, b))
        c.append(("MUL (%s) squared" % na, PH_MUL, a, a))
    big = [o for o in ops if o[0].startswith("15 x")]
    c += [("MUL (%s) (%s) at the bounds" % (na, nb), PH_MUL, a, b) for na, a in big for nb, b in big if na != nb]
    return c


def fam_inv():
    rng = random.Random(3009)
    c = [("INV 1 x slot %d" % s, PH_INV, [(s, 1)], []) for s in range(NV)]
    c += [("INV -1 x slot %d" % s, PH_INV, [(s, -1)], []) for s in range(NV)]
    c += [("INV 15 x 32767 on slot %d" % s, PH_INV, [(s, MAXC)] * 15, []) for s in (SP, S2PM1, S1, 6)]
    c += [("INV 15 x +-32767 on slot %d" % s, PH_INV, [(s, MAXC if i % 2 == 0 else -MAXC) for i in range(15)], []) for s in (S2PM1, 7)]
    c += [("INV p - (p - 1) - 1", PH_INV, [(SP, 1), (SPM1, -1), (S1, -1)], []), ("INV (p + 1) - p", PH_INV, [(SPP1, 1), (SP, -1)], []),
          ("INV 15 random terms", PH_INV, [(RANDS[i % len(RANDS)], rng.randint(-MAXC, MAXC)) for i in range(15)], []),
          ("INV 7 (slot 6 - slot 6) + 7 p", PH_INV, [(6, 7), (6, -7), (SP, 7)], [])]
    return c


FAMILIES = {"lin": fam_lin, "kp": fam_kp, "mul": fam_mul, "inv": fam_inv}
_cache = {}


def family(name):
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]


def shapes():
    """phase shapes: counts of 1, 31, 32, 33, 63 and 64 for products and LIN ops; phases that read what earlier phases
    wrote; a LIN phase followed by an INV phase and a product phase (the next phase's record is fetched while the
    current one computes, across kinds and lane arrangements)"""
    rng = random.Random(3007)
    progs = []

    def op(kind, dst, pool):
        a = [(rng.choice(pool), rng.choice((1, 1, -1, 2, MAXC, -MAXC, rng.randint(-MAXC, MAXC)))) for _ in range(rng.choice((1, 1, 2, 3, 15)))]
        b = [(rng.choice(pool), rng.choice((1, 1, -1, rng.randint(-MAXC, MAXC)))) for _ in range(rng.choice((0, 1, 1, 2, 15)))]
        if kind == PH_MUL and not b:
            b = [(rng.choice(pool), 1)]
        return (dst, a, b)

    pool = list(range(NV))
    for kind, kn in ((PH_MUL, "MUL"), (PH_LIN, "LIN")):
        for counts in ((1, 31, 32), (33, 63), (64, 1, 33)):
            phases, names, dst = [], {}, NV
            for cnt in counts:
                ops = []
                for k in range(cnt):
                    ops.append(op(kind, dst, pool))
                    names[dst] = "%s phase of %d ops, op %d" % (kn, cnt, k)
                    dst += 1
                phases.append((kind, ops))
            progs.append(Hand("%s phases of %s ops" % (kn, counts), phases, VALUES, dst, names))
    # a chain: products, then LIN ops on them, then products of those, then one inversion, then a wide product phase
    phases, names, dst = [], {}, NV
    prev = pool
    for kind, cnt, kn in ((PH_MUL, 12, "MUL"), (PH_LIN, 3, "LIN"), (PH_INV, 1, "INV"), (PH_MUL, 40, "MUL"), (PH_LIN, 64, "LIN"),
                          (PH_INV, 1, "INV"), (PH_LIN, 32, "LIN"), (PH_MUL, 33, "MUL")):
        ops, new = [], []
        for k in range(cnt):
            o = op(kind, dst, prev)
            ops.append((o[0], o[1], [] if kind == PH_INV else o[2]))
            names[dst] = "chain phase %d (%s, %d ops), op %d" % (len(phases), kn, cnt, k)
            new.append(dst)
            dst += 1
        phases.append((kind, ops))
        prev = new + pool[:6]
    progs.append(Hand("a chain of phases that read the phase before", phases, VALUES, dst, names))
    return progs


def small():
    """a small valid program (a product phase, a LIN phase, an INV phase) for the sizes and the refusals"""
    return Hand("small", [(PH_MUL, [(NV, [(S1, 1)], [(6, 1)]), (NV + 1, [(7, 2), (8, -1)], [(9, 1)])]),
                          (PH_LIN, [(NV + 2, [(NV, 1)], [(NV + 1, 1)])]), (PH_INV, [(NV + 3, [(NV + 2, 1)], [])])],
                VALUES, NV + 4, {NV: "small MUL 0", NV + 1: "small MUL 1", NV + 2: "small LIN", NV + 3: "small INV"})


def random_images(n, nslots, nvalues, seed):
    """n slot images whose first nvalues slots hold random values below 2p (the edges mixed in)"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        vals = [rng.choice(EDGE) if rng.random() < 0.2 else rng.randrange(2 * P) for _ in range(nvalues)]
        out.append([w for v in vals for w in vm_slot(v)] + [0] * (SW * (nslots - nvalues)))
    return out
