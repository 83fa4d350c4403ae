"""Shared builders of the assemble cases of tests/test_assemble_host.py (CPU) and tests/test_gpu_assemble.py (GPU): piles
of candidate records cut from the 300-round signed chains of tests/golden/archive_cases.json (nothing new is signed).
What store.assemble_host gives for the faulty pile WITH THE ORACLE VERIFYING is pinned in
tests/golden/assemble_cases.json (python tests/assemble_cases.py rewrites it); the GPU test compares the device path
against that record, never against the code under test."""
import json
import os
import random

import numpy as np

import archive_cases as ac
from bolt_cases import SCHEMES, rand_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
CASES_JSON = os.path.join(HERE, "golden", "assemble_cases.json")
N = ac.N
UP_TO = 290  # the faulty pile's up_to: rounds 291 .. 300 are stale, 289 and 290 are missing


def three_sources(name, gold):
    """[A, B, C]: rounds 1-200 in order, rounds 120-300 reversed, every third round shuffled by a seeded permutation.
    None is complete; A and B together hold every round."""
    recs = [{k: r[k] for k in ("round", "signature", "previous_signature")} for r in ac.chain_records(name, gold)]
    a = [dict(r) for r in recs[:200]]
    b = [dict(r) for r in reversed(recs[119:])]
    c = [dict(r) for r in recs[2::3]]
    random.Random(20).shuffle(c)
    return [a, b, c]


def clean_pile(name, gold):
    """(candidates, source ids) of the three sources, one after the other."""
    srcs = three_sources(name, gold)
    return [r for s in srcs for r in s], [k for k, s in enumerate(srcs) for _ in s]


def flip(sig, at):
    return sig[:at] + bytes([sig[at] ^ 1]) + sig[at + 1:]


def faulty_pile(name, gold):
    """The three sources with every fault of the issue's list. Rounds that are no multiple of 3 and below 120 lie in
    source A alone, so damaging A's copy leaves a gap; multiples of 3 between 120 and 200 lie in all three."""
    a, b, c = three_sources(name, gold)
    by_round = {r["round"]: r for r in ac.chain_records(name, gold)}
    sig = lambda r: by_round[r]["signature"]  # noqa: E731
    at = lambda src, r: next(x for x in src if x["round"] == r)  # noqa: E731

    at(a, 10)["signature"] = flip(sig(10), 20)         # corrupted, the round's only copy: a gap
    at(a, 150)["signature"] = flip(sig(150), 20)       # corrupted, intact in B and C: invalid, chosen elsewhere
    at(a, 20)["signature"] = sig(20)[:-1]              # a wrong length
    at(a, 25)["signature"] = b""                       # a zero length
    at(a, 40)["previous_signature"] = rand_bytes("foreign prev", 96)  # chained: invalid (a gap); else read by nobody
    at(a, 41)["previous_signature"] = b""                             # chained: no previous_signature at all
    b[:] = [x for x in b if x["round"] not in (289, 290)]             # missing up to UP_TO
    extra = [
        {"round": 0, "signature": sig(1), "previous_signature": b""},                      # round 0
        {"round": 7, "signature": rand_bytes("skipped", len(sig(7))), "previous_signature": b"", "skip": True},
        dict(by_round[28], signature=sig(28) + b"\0\0\0\0"),                               # longer than the stride
        dict(by_round[153], previous_signature=rand_bytes("other prev", 96)),              # chained: not a duplicate
        dict(by_round[156], signature=flip(sig(156), len(sig(156)) - 1)),                  # all but the last byte
    ]
    extra += [dict(by_round[159]) for _ in range(20)]                          # past the lookback
    first = [dict(by_round[5], signature=flip(sig(5), 3))]                                 # the corrupted copy comes first
    srcs = [first + a, b, c + extra]
    cands = [{"round": r["round"], "signature": r["signature"], "previous_signature": r["previous_signature"], "skip": bool(r.get("skip"))}
             for s in srcs for r in s]
    return cands, [k for k, s in enumerate(srcs) for _ in s]


def anchor(name, gold):
    """Round 2 of the chain: rounds 1 and 2 of the pile are below and at the anchor."""
    return (2, bytes.fromhex(gold["chains"][name]["sigs"][1]))


def bad_anchor(name, gold):
    """An anchor the chain does not follow: round 1 with another signature."""
    return (1, rand_bytes("assemble bad anchor " + name, ac.SIG_LEN[name]))


ANCHORS = {"anchor": anchor, "no_anchor": lambda name, gold: None, "bad_anchor": bad_anchor}


def columns(cands, stride, chained):
    """The candidates as the verifier's columns (numpy): rounds u64, sigs u8[n, stride], lens u32, prevs, prev_lens (None
    unless chained), skip u8. A value longer than the stride leaves a zero row and its true length."""
    n = len(cands)
    rounds = np.array([c["round"] for c in cands], np.uint64)
    skip = np.array([1 if c.get("skip") else 0 for c in cands], np.uint8)

    def rows(key):
        out, lens = np.zeros((n, stride), np.uint8), np.zeros(n, np.uint32)
        for i, c in enumerate(cands):
            v = c.get(key) or b""
            lens[i] = len(v)
            if len(v) <= stride:
                out[i, :len(v)] = np.frombuffer(v, np.uint8)
        return out, lens
    sigs, lens = rows("signature")
    prevs, prev_lens = rows("previous_signature") if chained else (None, None)
    return rounds, sigs, lens, prevs, prev_lens, skip


def plain(res):
    """An assemble_host / Assembled result as the JSON record holds it."""
    get = (lambda k: res[k]) if isinstance(res, dict) else (lambda k: getattr(res, k))
    return {"status": [int(x) for x in get("status")], "rounds": [int(x) for x in get("rounds")], "src": [int(x) for x in get("src")],
            "flags": [int(x) for x in get("flags")], "gaps": [[int(x), int(y)] for x, y in get("gaps")],
            "counts": {k: int(v) for k, v in get("counts").items()}, "contiguous_up_to": int(get("contiguous_up_to"))}


def host_record(name, gold, oracle):
    from drand_amd import scheme_from_name
    from drand_amd.store import assemble_host
    s = scheme_from_name(name)
    pk = bytes.fromhex(gold["chains"][name]["pk"])
    verify = ac.oracle_verify(oracle)
    cands, _ = faulty_pile(name, gold)
    return {k: plain(assemble_host(cands, s, pk, anchor=a(name, gold), up_to=UP_TO, verify=verify)) for k, a in ANCHORS.items()}


def load_golden():
    return json.load(open(CASES_JSON))


if __name__ == "__main__":  # rewrite tests/golden/assemble_cases.json from the host restatement and the oracle
    import sys
    root = os.path.dirname(HERE)
    sys.path[:0] = [root, os.path.join(root, "oracle")]
    import oracle_ctypes
    oracle_ctypes.lib()
    gold = ac.load_golden()
    with open(CASES_JSON, "w") as f:
        json.dump({name: host_record(name, gold, oracle_ctypes) for name in SCHEMES}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
