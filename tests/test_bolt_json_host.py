"""CPU: the hexjson value parser shared by the host and the store kernels (drand_amd/csrc/bolt.hpp hexjson_parse,
DESIGN.md §18), as a stand-alone program under AddressSanitizer + UBSan (tests/hexjson_san), over values in exact-size
heap buffers:

* every value of the reference's untrimmed fixture, hand-written canonical edges, every deferred class, 21-digit and
  overflowing Rounds, the empty value, a record cut at each length, and a byte-mutation sweep over a G2 and a G1 record;
* no sanitizer report; a value classed canonical decodes to exactly what beacon_from_hexjson gives; a value
  beacon_from_hexjson rejects is classed deferred; every unmutated Marshal-form value is canonical;
* the expected faulty lists of the GPU replay cases (tests/test_gpu_bolt_json.py), computed here with
  check_past_beacons over BoltUntrimmedStore and the oracle, equal the record in tests/golden/bolt_json_cases.json."""
import os
import shutil
import struct
import subprocess

import pytest

import bolt_cases as bc
import bolt_json_cases as jc
from drand_amd.store import BoltFile, BoltUntrimmedStore, beacon_from_hexjson
from drand_amd.sync import check_past_beacons
from test_readers import OracleScheme

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "hexjson_san")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
MUTATIONS = [b'"', b"}", b"G", b"A", b" ", b"0", b"\0", b"\xff", b",", b"f", b"{", b":"]
U64_MAX = (1 << 64) - 1


@pytest.fixture(scope="module")
def hexjson_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ missing")
    r = subprocess.run(["make", "-s", "_build/hexjson_check"], cwd=SAN, env=ENV, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    tmp = tmp_path_factory.mktemp("hexjson")

    def run(corpus):
        """corpus: [(key, value)] -> one parsed line per record"""
        path = str(tmp / "corpus.bin")
        with open(path, "wb") as f:
            for k, v in corpus:
                f.write(struct.pack("<QI", k, len(v)) + v)
        r = subprocess.run([os.path.join(SAN, "_build", "hexjson_check"), path], env=ENV, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])  # a sanitizer report aborts
        lines = r.stdout.splitlines()
        assert len(lines) == len(corpus)
        return lines

    return run


def host_decode(value):
    """(round, signature, previous) by beacon_from_hexjson, or None when it rejects the value."""
    try:
        b = beacon_from_hexjson(value)
    except Exception:  # noqa: BLE001 - any exception is "the decoder refuses the value"
        return None
    return b.round, b.signature, b.previous_signature


def check(corpus, lines):
    """The properties required of every record; returns the number classed canonical."""
    canonical = 0
    for (k, v), line in zip(corpus, lines):
        want = host_decode(v)
        f = line.split()
        if f[0] == "D":
            continue
        assert f[0] == "C", (k, v, line)
        canonical += 1
        assert want is not None, ("canonical here, rejected by the host decoder", k, v)
        sig = b"" if f[3] == "-" else bytes.fromhex(f[3])
        prev = b"" if f[4] == "-" else bytes.fromhex(f[4])
        assert (int(f[1]), int(f[2])) == (len(sig), len(prev)), (k, v, line)
        assert want == (k, sig, prev), (k, v, line)  # the round is the key
    return canonical


def test_reference_fixture_values_are_canonical(hexjson_check):
    kv = BoltFile(jc.REF_UNTRIMMED).bucket(b"beacons")
    corpus = [(struct.unpack(">Q", k)[0], v) for k, v in sorted(kv.items())]
    assert len(corpus) == 27 and sorted(set(len(v) for _k, v in corpus)) == [109, 299, 427, 428]
    lines = hexjson_check(corpus)
    assert check(corpus, lines) == len(corpus)
    assert lines[0].split()[1:3] == ["32", "0"] and lines[1].split()[1:3] == ["96", "32"] and lines[2].split()[1:3] == ["96", "96"]


def test_canonical_edges_and_deferred_classes(hexjson_check):
    r96, r48, r32 = bc.rand_bytes("a", 96), bc.rand_bytes("b", 48), bc.rand_bytes("c", 32)
    canon = [(0, jc.marshal(0, r32, None)), (1, jc.marshal(1, r96, r32)), (2, jc.marshal(2, r96, r96)),
             (3, jc.marshal(3, r48, None)), (4, jc.marshal(4, r48, b"")), (5, jc.marshal(5, b"", b"")),
             (6, jc.marshal(6, None, None)), (7, jc.marshal(7, None, r48)), (U64_MAX, jc.marshal(U64_MAX, r96, r96)),
             (10, jc.marshal(10, r48, None)), (1234567890123, jc.marshal(1234567890123, r48, r96))]
    lines = hexjson_check(canon)
    assert check(canon, lines) == len(canon)  # a condition: the parser may not pass by deferring everything
    deferred = [(7 + i, make(7 + i)) for i, (_what, make) in enumerate(jc.DEFERRED_VALUES)]
    deferred += [
        (5, jc.marshal(5, r48, None).replace(b'"Round":5', b'"Round":05')),  # leading zero
        (0, jc.marshal(0, r48, None).replace(b'"Round":0', b'"Round":00')),
        (0, jc.marshal(0, r48, None).replace(b'"Round":0', b'"Round":-0')),
        (0, jc.marshal(0, r48, None).replace(b'"Round":0', b'"Round":')),
        (3, jc.marshal(3, r48, None).replace(b'"Round":3', b'"Round":3.0')),
        (3, jc.marshal(3, r48, None).replace(b'"Round":3', b'"Round":"3"')),
        (U64_MAX, jc.marshal(U64_MAX + 1, r48, None)),  # 20 digits, overflows
        (U64_MAX, jc.marshal(99999999999999999999, r48, None)),
        (0, jc.marshal(1 << 64, r48, None)),  # wraps to 0
        (100000000000000000000 & U64_MAX, jc.marshal(100000000000000000000, r48, None)),  # 21 digits
        (1, jc.marshal(1, r48, None).replace(b"null", b"nul")),
        (1, jc.marshal(1, r48, None).replace(b"null", b"NULL")),
        (1, jc.marshal(1, r48, None).replace(b"null", b"nulll")),
        (1, b" " + jc.marshal(1, r48, None)),
        (1, jc.marshal(1, r48, None) + b" "),
        (1, jc.marshal(1, r48, None) * 2),
        (1, jc.marshal(1, r48, None).replace(b"PreviousSig", b"previoussig")),
        (1, jc.marshal(1, r48, None).replace(b'"Signature":"', b'"Signature":"0x')),
        (1, b"{}"), (1, b"null"), (1, b"5"), (1, b"[]"), (1, b"{"), (1, b'"'), (1, b"\0"),
    ]
    lines = hexjson_check(deferred)
    check(deferred, lines)
    assert [l for l in lines if l != "D"] == [], [(v, l) for (_k, v), l in zip(deferred, lines) if l != "D"]
    # a record cut at each length
    rec = jc.marshal(9, r96, r96)
    cuts = [(9, rec[:n]) for n in range(len(rec))]
    lines = hexjson_check(cuts)
    assert check(cuts, lines) == 0


@pytest.mark.parametrize("kind", ["g2", "g1"])
def test_mutation_sweep(hexjson_check, kind):
    if kind == "g2":
        k, rec = 41, jc.marshal(41, bc.rand_bytes("s", 96), bc.rand_bytes("p", 96))
    else:
        k, rec = 18446744073709551615, jc.marshal(18446744073709551615, bc.rand_bytes("s", 48), None)
    corpus = [(k, rec)]
    for i in range(len(rec)):
        for mu in MUTATIONS:
            corpus.append((k, rec[:i] + mu + rec[i + 1:]))
    lines = hexjson_check(corpus)
    canonical = check(corpus, lines)
    assert lines[0].startswith("C ")
    # a replaced hex digit ('0', 'f') gives another canonical record, and a replacement by the byte already there
    # changes nothing; every other mutation must be deferred
    still = sum(1 for (_k, v), l in zip(corpus, lines) if l != "D" and v != rec)
    hexchars = (2 * 96 * 2) if kind == "g2" else 2 * 48
    assert 0 < still <= 2 * hexchars and canonical < len(corpus) // 4


# ---------------------------------------------------------------- expected faulty lists of the GPU cases

class CachedOracleScheme(OracleScheme):
    """The oracle's verdict on one (round, signature, previous) is computed once for all the calls."""

    def __init__(self, oracle, name, cache):
        super().__init__(oracle, name)
        self.cache = cache

    def verify_beacons(self, pk, rounds, sigs, prevs=None, seed=0, want_randomness=True):
        import numpy as np
        out = []
        for i, (r, s) in enumerate(zip(rounds, sigs)):
            item = (self.name, int(r), bytes(s), bytes(prevs[i]) if prevs else b"")
            if item not in self.cache:
                self.cache[item] = self.o.verify_beacon(self.name, pk, item[1], item[2], item[3])
            out.append(self.cache[item])
        return np.array(out, dtype=bool), None


def compute_golden(oracle, tmp):
    replay, cache = {}, {}
    for name in jc.SCHEMES:
        pk, path, _deferred = jc.replay_file(tmp, name, oracle)
        s = CachedOracleScheme(oracle, name, cache)
        for up_to, window in jc.REPLAY_CALLS:
            st = BoltUntrimmedStore(path, s.chained)
            replay[jc.call_id(name, up_to, window)] = check_past_beacons(st, s, pk, up_to, window=window)
    return replay


def test_recorded_faulty_lists(oracle, tmp_path):
    gold = jc.load_golden()["replay"]
    assert compute_golden(oracle, tmp_path) == gold
    # the shapes the cases exist for: the stored PreviousSig counts for the chained scheme only; a missing round marks
    # itself alone; the undecodable record is faulty under its key and the Round-7 record under 7, at its key's place
    for name in jc.SCHEMES:
        want = [jc.CORRUPT] + ([jc.WRONG_PREV] if name == "pedersen-bls-chained" else []) + \
            [jc.SHORT, jc.MISSING, jc.UNDECODABLE, 7, jc.MISSING2]
        assert gold[jc.call_id(name, 1000, 64)] == want == gold[jc.call_id(name, 1000, 1 << 20)], name
        assert gold[jc.call_id(name, 130, 64)] == [r for r in want[:want.index(7)]], name
