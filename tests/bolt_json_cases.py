"""Shared builders of the untrimmed (hexjson) store cases of tests/test_bolt_json_host.py (CPU) and
tests/test_gpu_bolt_json.py (GPU): the same deterministic files on both sides. The CPU test computes the expected
faulty lists with check_past_beacons over BoltUntrimmedStore and the oracle and pins them in
tests/golden/bolt_json_cases.json (python tests/bolt_json_cases.py rewrites it); the GPU test compares the device
path against that record, never against the code under test."""
import hashlib
import json
import os

import bolt_cases as bc
from boltwrite2 import write_bolt2

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
CASES_JSON = os.path.join(GOLD, "bolt_json_cases.json")
REF_UNTRIMMED = os.path.join(GOLD, "boltdb", "untrimmed.db")
REF_TRIMMED = bc.REF_TRIMMED
SCHEMES = bc.SCHEMES
key = bc.key


def marshal(round_, sig, prev):
    """chain.Beacon.Marshal: hexjson, Go field order, a nil slice as null."""
    def f(b):
        return "null" if b is None else '"%s"' % bytes(b).hex()
    return ('{"PreviousSig":%s,"Round":%d,"Signature":%s}' % (f(prev), int(round_), f(sig))).encode()


# ------------------------------------------------------------------ column parity files (synthetic bytes)

def synth(n, sig_len, chained, tag):
    """{key: value} of rounds 0..n-1: a 32-byte genesis record with a null previous, then sig_len-byte signatures;
    chained records store the signature before them, unchained ones null."""
    kv, prev = {}, None
    for r in range(n):
        sig = bc.rand_bytes("%s%d" % (tag, r), 32 if r == 0 else sig_len)
        kv[key(r)] = marshal(r, sig, prev if chained else None)
        prev = sig
    return kv


DEFERRED_VALUES = [  # (what, value for key r): every class the device leaves to the host
    ("uppercase", lambda r: marshal(r, b"\xab" * 96, b"\xcd" * 96).replace(b"ab", b"AB")),
    ("odd digits", lambda r: marshal(r, b"\x11" * 96, None).replace(b'11"}', b'1"}')),
    ("non-hex", lambda r: marshal(r, b"\x22" * 96, None).replace(b'22"}', b'2g"}')),
    ("whitespace", lambda r: marshal(r, b"\x33" * 96, None).replace(b":", b": ", 1)),
    ("reordered", lambda r: ('{"Round":%d,"PreviousSig":null,"Signature":"%s"}' % (r, "44" * 96)).encode()),
    ("extra field", lambda r: marshal(r, b"\x55" * 96, None)[:-1] + b',"X":1}'),
    ("round != key", lambda r: marshal(r + 1, b"\x66" * 96, None)),
    ("truncated", lambda r: marshal(r, b"\x77" * 96, None)[:-7]),
    ("trailing", lambda r: marshal(r, b"\x88" * 96, None) + b"\n"),
    ("empty", lambda r: b""),
    ("raw signature", lambda r: b"\x99" * 96),
]


def parity_files(tmp):
    """[(id, path, deferred keys)]"""
    out = []

    def add(name, kv, deferred=(), **kw):
        path = os.path.join(str(tmp), name + ".db")
        write_bolt2(path, list(kv.items()), **kw)
        out.append((name, path, sorted(deferred)))

    for psz in (256, 512, 4096, 16384):  # 256: every leaf has overflow pages, read in place; 512: one record a leaf
        add("j96_p%d" % psz, synth(150, 96, True, "j%d" % psz), page_size=psz)
    add("j48_p16384", synth(300, 48, False, "g1"), page_size=16384)  # > 64 elements a leaf: two chunks through LDS
    add("inline3", synth(3, 96, True, "in"), inline=True)
    add("many_leaves", synth(8192, 96, True, "big"), page_size=512)  # > 4,096 leaves: the hierarchical scan
    gaps = synth(120, 96, True, "gap")
    for r in (0, 30, 31, 32, 119):
        del gaps[key(r)]
    add("gaps", gaps, page_size=1024)
    mixed = synth(100, 96, True, "mix")
    at = {}
    for i, (_what, make) in enumerate(DEFERRED_VALUES):
        r = 5 + 7 * i
        mixed[key(r)] = make(r)
        at[r] = True
    mixed[key(90)] = marshal(90, b"", b"")  # "" fields: canonical, zero lengths
    mixed[key(91)] = marshal(91, None, None)
    mixed[key(92)] = marshal(92, bc.rand_bytes("long", 200), bc.rand_bytes("longp", 130))  # longer than any stride used below
    add("mixed", mixed, deferred=at, page_size=4096)
    return out


def windows(rounds):
    return bc.windows(rounds)


# ------------------------------------------------------------------ replay cases: ~300 signed rounds per scheme

N_ROUNDS = 300
CORRUPT, WRONG_PREV, SHORT, MISSING, MISSING2, UNDECODABLE, ROUND_NE_KEY = 20, 40, 60, 80, 150, 120, 140
# (up_to, window)
REPLAY_CALLS = [(1000, 64), (1000, 1 << 20), (130, 64)]


def call_id(name, up_to, window):
    return "%s/up_to=%d/window=%d" % (name, up_to, window)


def replay_kv(name, oracle):
    """(pk, {key: value}, deferred keys) of one scheme's store: a signed chain of N_ROUNDS rounds after the genesis
    record, carrying a corrupted signature, a wrong stored PreviousSig, a signature two bytes short, two missing rounds
    (their successors intact, with the true PreviousSig stored) and two deferred records: one no decoder accepts, and
    one whose Round field (7) is not its key, which the host verifies and reports under 7."""
    chained = name == "pedersen-bls-chained"
    sk = hashlib.sha256(b"bolt json " + name.encode()).digest()
    sk = (int.from_bytes(sk, "big") % 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001).to_bytes(32, "big")
    pk = oracle.public_key(name, sk)
    genesis = hashlib.sha256(b"genesis " + name.encode()).digest()
    sigs = {0: genesis}
    for r in range(1, N_ROUNDS + 1):
        sigs[r] = oracle.sign(name, sk, oracle.digest_beacon(name, r, sigs[r - 1] if chained else b""))
    kv = {key(0): marshal(0, genesis, None)}
    for r in range(1, N_ROUNDS + 1):
        kv[key(r)] = marshal(r, sigs[r], sigs[r - 1] if chained else None)
    bad = bytearray(sigs[CORRUPT])
    bad[20] ^= 1
    kv[key(CORRUPT)] = marshal(CORRUPT, bad, sigs[CORRUPT - 1] if chained else None)
    kv[key(WRONG_PREV)] = marshal(WRONG_PREV, sigs[WRONG_PREV], bc.rand_bytes("wrong prev", 96))
    kv[key(SHORT)] = marshal(SHORT, sigs[SHORT][:-2], sigs[SHORT - 1] if chained else None)
    del kv[key(MISSING)]
    del kv[key(MISSING2)]
    kv[key(UNDECODABLE)] = kv[key(UNDECODABLE)][:-40]
    kv[key(ROUND_NE_KEY)] = marshal(7, sigs[ROUND_NE_KEY], sigs[ROUND_NE_KEY - 1] if chained else None)
    return pk, kv, [UNDECODABLE, ROUND_NE_KEY]


def replay_file(tmp, name, oracle):
    pk, kv, deferred = replay_kv(name, oracle)
    path = os.path.join(str(tmp), "%s_json.db" % name)
    write_bolt2(path, list(kv.items()), page_size=4096)
    return pk, path, deferred


def load_golden():
    return json.load(open(CASES_JSON))


if __name__ == "__main__":  # rewrite tests/golden/bolt_json_cases.json from the host reader and the oracle
    import sys
    import tempfile
    root = os.path.dirname(HERE)
    sys.path[:0] = [root, os.path.join(root, "oracle")]
    import oracle_ctypes
    import test_bolt_json_host as host
    oracle_ctypes.lib()
    with tempfile.TemporaryDirectory() as tmp:
        gold = {"replay": host.compute_golden(oracle_ctypes, tmp)}
    with open(CASES_JSON, "w") as f:
        json.dump(gold, f, indent=1, sort_keys=True)
        f.write("\n")
