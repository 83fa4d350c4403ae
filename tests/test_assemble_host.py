"""CPU: one chain from many unordered sources on the host side.

* store.assemble_host, with the oracle verifying, on the faulty pile of tests/assemble_cases.py equals the record in
  tests/golden/assemble_cases.json, and shows every fault the pile holds; on the clean union of the three incomplete
  sources its output is ac.chain_records itself: ground truth that does not come from the restatement.
* drand_amd/csrc/assemble.hpp, the compare / class / status rules the assemble kernels share with the host, compiled
  into a stand-alone program under ASan + UBSan (tests/assemble_san) and run over exact-size heap rows: lengths 0, 1,
  stride - 1 and stride, rows equal except for the last byte or for the length, a value longer than the stride, a run
  past the lookback, seeded random piles; no sanitizer report, and status, output and flags equal assemble_host's."""
import os
import random
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import archive_cases as ac
import assemble_cases as asc
from drand_amd import scheme_from_name
from drand_amd import store

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = os.path.join(HERE, "assemble_san")
S, D, I, ST, SK, CF = store.AS_CHOSEN, store.AS_DUPLICATE, store.AS_INVALID, store.AS_STALE, store.AS_SKIPPED, store.AS_CONFLICT


@pytest.fixture(scope="module")
def gold_ar():
    return ac.load_golden()


@pytest.fixture(scope="module")
def gold():
    return asc.load_golden()


@pytest.mark.parametrize("name", asc.SCHEMES)
def test_recorded_cases(oracle, gold_ar, gold, name):
    got = asc.host_record(name, gold_ar, oracle)
    assert got == gold[name]
    chained = name == "pedersen-bls-chained"
    cands, ids = asc.faulty_pile(name, gold_ar)
    st = got["anchor"]["status"]
    where = lambda rnd, src: next(i for i, c in enumerate(cands) if c["round"] == rnd and ids[i] == src)  # noqa: E731
    assert st[0] == I and st[where(5, 0)] == I and cands[0]["round"] == 5                # the corrupted copy comes first ...
    assert st[[i for i, c in enumerate(cands) if c["round"] == 5][1]] == S                    # ... and the intact one is chosen
    assert st[where(10, 0)] == I and st[where(20, 0)] == I and st[where(25, 0)] == I          # corrupted / short / empty, only copies
    assert st[where(150, 0)] == I and st[where(150, 1)] == S and st[where(150, 2)] == D       # chosen elsewhere
    assert st[where(1, 0)] == ST and st[where(2, 0)] == ST and st[where(300, 1)] == ST        # below / at the anchor, above up_to
    tail = len(cands) - 25
    assert [c["round"] for c in cands[tail:tail + 5]] == [0, 7, 28, 153, 156]
    assert st[tail:tail + 5] == [ST, SK, I, I if chained else D, I] and st[tail + 5:] == [D] * 20
    assert st[where(40, 0)] == (I if chained else S) and st[where(41, 0)] == (I if chained else S)
    want_gaps = [[10, 10], [20, 20], [25, 25]] + ([[40, 41]] if chained else []) + [[289, 290]]
    for kind in asc.ANCHORS:
        assert got[kind]["gaps"] == want_gaps and got[kind]["counts"]["conflicts"] == 0
        assert got[kind]["counts"]["missing"] == sum(b - a + 1 for a, b in want_gaps)
    assert got["anchor"]["rounds"][0] == 3 and got["no_anchor"]["rounds"][0] == 1 and got["bad_anchor"]["rounds"][0] == 2
    assert got["anchor"]["contiguous_up_to"] == got["no_anchor"]["contiguous_up_to"] == 9
    assert got["bad_anchor"]["flags"][0] == (store.AS_LINK if chained else 0)
    assert got["bad_anchor"]["contiguous_up_to"] == (1 if chained else 9)  # nothing follows the anchor: its own round
    assert got["bad_anchor"]["counts"]["link_breaks"] == (1 if chained else 0)


@pytest.mark.parametrize("name", asc.SCHEMES)
def test_clean_union_is_the_chain(oracle, gold_ar, name):
    s, pk = scheme_from_name(name), bytes.fromhex(gold_ar["chains"][name]["pk"])
    cands, _ = asc.clean_pile(name, gold_ar)
    chain = ac.chain_records(name, gold_ar)
    assert all(len({r["round"] for r in src}) < ac.N for src in asc.three_sources(name, gold_ar))  # no source is complete
    res = store.assemble_host(cands, s, pk, anchor=ac.anchor(name), verify=ac.oracle_verify(oracle))
    assert res["rounds"] == [r["round"] for r in chain]
    assert [cands[i]["signature"] for i in res["src"]] == [r["signature"] for r in chain]
    assert not any(res["flags"]) and res["gaps"] == [] and res["contiguous_up_to"] == ac.N
    assert res["counts"]["verified"] == ac.N and res["counts"]["duplicates"] == len(cands) - ac.N


def test_conflicts_and_arguments():
    s = SimpleNamespace(sig_len=2, chained=False, name="toy")
    ok = lambda sc, pk, recs: [r["signature"][0] == 1 for r in recs]  # noqa: E731
    c = [{"round": 4, "signature": b"\x01a"}, {"round": 4, "signature": b"\x01b"}, {"round": 4, "signature": b"\x01a"},
         {"round": 2, "signature": b"\x00a"}, {"round": 2, "signature": b"\x00a"}, {"round": 9, "signature": b"\x01z"}]
    res = store.assemble_host(c, s, b"", up_to=12, verify=ok)
    assert list(res["status"]) == [S, CF, D, I, D | I, S] and res["rounds"] == [4, 9] and res["src"] == [0, 5]
    assert res["flags"] == [0, store.AS_GAP] and res["gaps"] == [(5, 8), (10, 12)] and res["contiguous_up_to"] == 4
    assert res["counts"]["missing"] == 7 and res["counts"]["conflicts"] == 1 and res["counts"]["verified"] == 4
    res = store.assemble_host(c, s, b"", anchor=(3, b"xx"), verify=ok)
    assert list(res["status"]) == [S, CF, D, ST, ST, S] and res["gaps"] == [(5, 8)] and res["contiguous_up_to"] == 4
    empty = store.assemble_host([], s, b"", anchor=(3, b"xx"), up_to=5, verify=ok)
    assert empty["gaps"] == [(4, 5)] and empty["contiguous_up_to"] == 3 and empty["rounds"] == []
    assert store.assemble_host([], s, b"", verify=ok)["gaps"] == []
    seen = []  # a signature of another length never reaches the verifier
    store.assemble_host([{"round": 1, "signature": b"x"}, {"round": 1, "signature": b""}], s, b"", verify=lambda sc, pk, r: seen.extend(r) or [])
    assert not seen


# ---- assemble.hpp under the sanitizers

STRIDE = 8


@pytest.fixture(scope="module")
def prog():
    subprocess.check_call(["make", "-s", "_build/assemble_check"], cwd=SAN)
    return os.path.join(SAN, "_build", "assemble_check")


def stub_verify(sc, pk, recs):
    """The verdict handed to both sides: decided by the first signature byte."""
    return [r["signature"][0] % 2 == 0 for r in recs]


def run_check(prog, tmp_path, cands, chained, anchor, up_to, dedupe=1):
    a_round, a_sig = anchor if anchor else (0, b"")
    blob = struct.pack("<8I2Q", len(cands), STRIDE, int(chained), STRIDE, dedupe, int(anchor is not None), int(up_to is not None), len(a_sig),
                       a_round, up_to or 0) + a_sig
    for c in cands:
        sig, prev = c["signature"], c.get("previous_signature", b"") if chained else b""
        verdict = int(len(sig) == STRIDE and stub_verify(None, None, [c])[0])
        blob += struct.pack("<Q4I", c["round"], int(bool(c.get("skip"))), verdict, len(sig), len(prev)) + sig + prev
    path = os.path.join(str(tmp_path), "pile.bin")
    open(path, "wb").write(blob)
    res = subprocess.run([prog, path], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-2000:])  # no sanitizer report, every compare agreed
    lines = res.stdout.splitlines()
    assert lines[0].startswith("S")
    rows = [tuple(int(x) for x in l.split()[1:]) for l in lines[1:]]
    return [int(x) for x in lines[0].split()[1:]], rows


def edge_pile():
    v = lambda *b: bytes(b)  # noqa: E731
    base = v(2, 2, 2, 2, 2, 2, 2, 2)
    p1, p2 = v(9) * 8, v(9) * 7 + v(8)
    out = []
    for rnd, sigs in ((1, [b"", v(2), base[:7], base, base[:7] + v(0), base[:7] + v(3), base, b"", v(2), base[:7]]),   # lengths 0, 1, 7, 8
                      (2, [base[:7] + v(0), base[:7], base[:7] + v(0)]),                                                  # equal except for the length
                      (3, [v(3) + base[1:], v(2) + base[1:], v(4) + base[1:]]),                                           # an invalid one first; a conflict
                      (5, [base + v(1, 1, 1, 1), base]),                                                                  # longer than the stride
                      (6, [base] * 20),                                                                                   # past the lookback
                      (0, [base]), (9, [base]), (12, [base])):                                                            # round 0, above up_to
        out += [{"round": rnd, "signature": s, "previous_signature": p1} for s in sigs]
    out += [{"round": 2, "signature": base[:7] + v(0), "previous_signature": p2},   # chained: all but the last prev byte
            {"round": 2, "signature": base[:7] + v(0), "previous_signature": p1[:7]},  # all but the prev length
            {"round": 2, "signature": base[:7] + v(0), "previous_signature": b""},
            {"round": 7, "signature": base, "previous_signature": base},              # follows round 6's signature
            {"round": 8, "signature": base, "previous_signature": p1},                # does not follow round 7's
            {"round": 4, "signature": base, "previous_signature": p1, "skip": True}]
    random.Random(3).shuffle(out)
    return out


def random_pile(seed):
    rng = random.Random(seed)
    pool = [bytes([rng.randrange(4)]) * rng.choice([0, 1, 7, 8, 8, 8]) for _ in range(6)] + [bytes([2] * 7 + [k]) for k in range(3)]
    out, per_round = [], {}
    for _ in range(120):
        rnd = rng.randrange(0, 14)
        if per_round.get(rnd, 0) == 16:  # a longer run may leave copies un-collapsed: the record would differ in DUPLICATE bits
            continue
        per_round[rnd] = per_round.get(rnd, 0) + 1
        out.append({"round": rnd, "signature": rng.choice(pool), "previous_signature": rng.choice(pool), "skip": rng.random() < 0.05})
    return out


@pytest.mark.parametrize("chained", [False, True])
@pytest.mark.parametrize("pile", ["edge", 1, 2, 3])
def test_header_agrees_with_the_restatement(prog, tmp_path, pile, chained):
    cands = edge_pile() if pile == "edge" else random_pile(pile)
    s = SimpleNamespace(sig_len=STRIDE, chained=chained, name="toy")
    seen = []
    for anchor, up_to in ((None, None), ((0, bytes([2] * 8)), 10), ((2, bytes([9] * 8)), None), ((5, bytes([2] * 8)), 11)):
        want = store.assemble_host(cands, s, b"", anchor=anchor, up_to=up_to, verify=stub_verify)
        status, rows = run_check(prog, tmp_path, cands, chained, anchor, up_to)
        assert status == [int(x) for x in want["status"]]
        assert rows == list(zip(want["rounds"], want["src"], want["flags"]))
        off, rows_off = run_check(prog, tmp_path, cands, chained, anchor, up_to, dedupe=0)  # the dedupe changes DUPLICATE bits only
        assert [x & ~D for x in off] == [x & ~D for x in status] and rows_off == rows
        seen.append((status, want["flags"]))
    if pile == "edge":  # the pile shows what it is meant to: a conflict and an invalid copy without an anchor, link breaks behind one
        assert CF in seen[0][0] and D | I in seen[0][0] and any(f & store.AS_LINK for f in seen[-1][1]) == chained
