"""Shared builders of the RandomData archive cases of tests/test_archive_host.py (CPU) and tests/test_gpu_archive.py
(GPU): the same deterministic archives on both sides. The signed chains (300 rounds per scheme, signed by the CPU
oracle) and the statuses check_random_data_host gives with the oracle verifying are pinned in
tests/golden/archive_cases.json (python tests/archive_cases.py rewrites it); the GPU test compares the device path
against that record, never against the code under test."""
import hashlib
import json
import os

from bolt_cases import SCHEMES, rand_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
CASES_JSON = os.path.join(HERE, "golden", "archive_cases.json")
N, FIRST = 300, 1  # rounds FIRST .. FIRST + N - 1; the anchor is round FIRST - 1 (the genesis)
SIG_LEN = {"pedersen-bls-chained": 96, "pedersen-bls-unchained": 96, "bls-unchained-on-g1": 48, "bls-unchained-g1-rfc9380": 48}


def secret(name):
    return hashlib.sha256(b"archive cases " + name.encode()).digest()


def anchor_sig(name):
    return rand_bytes("archive anchor " + name, SIG_LEN[name])


def sign_chain(name, oracle):
    """[signature] of the N rounds; the chained scheme links each round to the one before, the first to the anchor."""
    sk, chained = secret(name), name == "pedersen-bls-chained"
    sigs, prev = [], anchor_sig(name)
    for r in range(FIRST, FIRST + N):
        sigs.append(oracle.sign(name, sk, oracle.digest_beacon(name, r, prev if chained else b"")))
        prev = sigs[-1]
    return sigs


def line_of_length(n):
    """A canonical record of exactly n bytes (n >= 28): one long signature."""
    head = b'{"round":1,"signature":"' if n % 2 == 0 else b'{"round":12,"signature":"'
    return head + b"ab" * ((n - len(head) - 2) // 2) + b'"}'


def load_golden():
    return json.load(open(CASES_JSON))


def chain_records(name, gold):
    """The clean records of one scheme as dicts, from the recorded signatures."""
    sigs = [bytes.fromhex(s) for s in gold["chains"][name]["sigs"]]
    chained = name == "pedersen-bls-chained"
    out = []
    for i, s in enumerate(sigs):
        out.append({"round": FIRST + i, "randomness": hashlib.sha256(s).digest(), "signature": s,
                    "previous_signature": (sigs[i - 1] if i else anchor_sig(name)) if chained else b""})
    return out


def anchor(name):
    return (FIRST - 1, anchor_sig(name))


def bad_anchor(name):
    """An anchor the first record does not follow: another round, another signature."""
    return (FIRST - 2, rand_bytes("archive bad anchor " + name, SIG_LEN[name]))


ANCHORS = {"anchor": anchor, "no_anchor": lambda name: None, "bad_anchor": bad_anchor}


def clean_archive(name, gold):
    from drand_amd.store import random_data_line
    return b"".join(random_data_line(r) + b"\n" for r in chain_records(name, gold))


def faulty_archive(name, gold):
    """The 300 records with every fault of the issue's list injected; the bytes of the archive."""
    from drand_amd.store import random_data_line
    recs = chain_records(name, gold)
    lines = [random_data_line(r) for r in recs]

    def edit(i, **kw):
        lines[i] = random_data_line(dict(recs[i], **kw))

    s = recs[10]["signature"]
    edit(10, signature=s[:20] + bytes([s[20] ^ 1]) + s[21:])     # a corrupted signature
    edit(20, signature=recs[20]["signature"][:-1])               # a short signature
    edit(30, signature=b"")                                      # an empty signature
    edit(40, randomness=hashlib.sha256(b"not it").digest())      # a wrong randomness
    edit(70, previous_signature=rand_bytes("wrong prev", 96))    # a wrong previous_signature
    lines[80] = lines[80].upper().replace(b"ROUND", b"round").replace(b"RANDOMNESS", b"randomness").replace(
        b"PREVIOUS_SIGNATURE", b"previous_signature").replace(b"SIGNATURE", b"signature")  # uppercase hex
    lines[90] = b'{"round":%d,"signature":"zz"}' % (FIRST + 90)  # an undecodable line
    lines[100] += b"\r"                                          # a \r\n line
    for i in (127, 128, 191, 192):  # deferred records next to each other and at the windows' edges
        lines[i] = lines[i].replace(b'{"round"', b'{ "round"')
    out = []
    for i, l in enumerate(lines):
        if i == 50:  # a removed record
            continue
        out.append(l)
        if i == 60:  # a duplicated record
            out.append(l)
        if i == 110:  # a blank-space line
            out.append(b"   ")
    return b"\n".join(out) + b"\n"


def compute_golden(oracle):
    """{"chains": {scheme: {"pk", "sigs"}}, "status": {scheme: {"anchor" | "no_anchor" | "bad_anchor" | "clean": [status]}}}"""
    gold = {"chains": {}, "status": {}}
    for name in SCHEMES:
        gold["chains"][name] = {"pk": oracle.public_key(name, secret(name)).hex(), "sigs": [s.hex() for s in sign_chain(name, oracle)]}
    for name in SCHEMES:
        gold["status"][name] = host_status(name, gold, oracle)
    return gold


def oracle_verify(oracle, cache=None):
    cache = {} if cache is None else cache

    def verify(scheme, pubkey, recs):
        out = []
        for r in recs:
            k = (scheme.name, r["round"], r["signature"], r["previous_signature"] if scheme.chained else b"")
            if k not in cache:
                cache[k] = bool(oracle.verify_beacon(scheme.name, bytes(pubkey), r["round"], r["signature"], k[3]))
            out.append(cache[k])
        return out
    return verify


def host_status(name, gold, oracle):
    from drand_amd import scheme_from_name
    from drand_amd.store import check_random_data_host
    s = scheme_from_name(name)
    pk = bytes.fromhex(gold["chains"][name]["pk"])
    verify = oracle_verify(oracle)
    data = faulty_archive(name, gold)
    out = {k: [int(x) for x in check_random_data_host(data, s, pk, anchor=a(name), verify=verify)] for k, a in ANCHORS.items()}
    return {**out, "clean": [int(x) for x in check_random_data_host(clean_archive(name, gold), s, pk, anchor=anchor(name), verify=verify)]}


if __name__ == "__main__":  # rewrite tests/golden/archive_cases.json from the host check and the oracle
    import sys
    root = os.path.dirname(HERE)
    sys.path[:0] = [root, os.path.join(root, "oracle")]
    import oracle_ctypes
    oracle_ctypes.lib()
    with open(CASES_JSON, "w") as f:
        json.dump(compute_golden(oracle_ctypes), f, indent=1, sort_keys=True)
        f.write("\n")
