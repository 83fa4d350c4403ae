"""CPU: protobuf beacon records on the host side.

* drand_amd/csrc/pbwire.hpp, the record parser the packet kernels share with the host, compiled into a stand-alone
  program under ASan + UBSan (tests/pbwire_san) and run over exact-size heap buffers: the canonical edges, every deferred
  class, and a G1 and a chained G2 record of each kind cut at each length and with each of 12 byte values at each position.
* the pin against google.protobuf (message classes built from a FileDescriptorProto written in packet_cases.py): every
  record the C parser calls canonical parses there to the same fields; every packet_bytes output equals
  SerializeToString() and is canonical; packet_from_bytes and ParseFromString agree on 24,000 mutated records.
* dh_pb_frame_delimited through ctypes, with no GPU.
* store.check_packets_host, with the oracle verifying, on the faulty 300-record runs of tests/packet_cases.py equals the
  record in tests/golden/packet_cases.json."""
import ctypes
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import archive_cases as ac
import packet_cases as pc
from drand_amd import _lib, store

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = os.path.join(HERE, "pbwire_san")
MUTANTS = bytes([0x00, 0x01, 0x08, 0x0a, 0x10, 0x12, 0x1a, 0x22, 0x30, 0x7f, 0x80, 0xff])  # the 12 bytes of the mutation sweep
KINDS = (pc.BP, pc.PR)


@pytest.fixture(scope="module")
def prog():
    subprocess.check_call(["make", "-s", "_build/pbwire_check"], cwd=SAN)
    return os.path.join(SAN, "_build", "pbwire_check")


@pytest.fixture(scope="module")
def classes():
    return pc.message_classes()


def run_parser(prog, tmp_path, records):
    """records: [(kind, bytes)] -> the program's output lines; no sanitizer report."""
    corpus = os.path.join(str(tmp_path), "corpus.bin")
    with open(corpus, "wb") as f:
        for kind, b in records:
            f.write(struct.pack("<BI", kind, len(b)) + b)
    res = subprocess.run([prog, corpus], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, res.stderr[-2000:]
    got = res.stdout.splitlines()
    assert len(got) == len(records)
    return got


def line_of(fields):
    rnd, sig, prev, rand, has_meta, bid = fields
    return "C %d %s %s %s %d %s" % (rnd, sig.hex() or "-", prev.hex() or "-", rand.hex() or "-", has_meta, (bid or "").encode().hex() or "-")


def upb(classes, kind, b):
    """ParseFromString as the parser's output line, or None when it rejects the bytes."""
    from google.protobuf.message import DecodeError
    m = classes[kind]()
    try:
        m.ParseFromString(b)
    except DecodeError:
        return None
    return line_of(pc.message_fields(m, kind))


def canonical_records():
    out = []
    for kind in KINDS:
        out += [(kind, store.packet_bytes(kind, r)) for r in pc.edge_records(kind).values()]
        out += [(kind, pc.record_of_length(kind, 4096))]
    return out


def sweep_records():
    out = []
    for kind in KINDS:
        for rec in (store.packet_bytes(kind, pc.g1_rec(2, kind), pc.BEACON_ID), store.packet_bytes(kind, pc.g2_rec(2, kind), pc.BEACON_ID)):
            out += [(kind, rec[:k]) for k in range(len(rec))]
            out += [(kind, rec[:k] + bytes([m]) + rec[k + 1:]) for k in range(len(rec)) for m in MUTANTS]
    return out


def test_parser_under_sanitizers_agrees_with_protobuf(prog, tmp_path, classes):
    canon = canonical_records()
    deferred = [(kind, b) for kind in KINDS for b in pc.deferred_records(kind)]
    sweep = sweep_records()
    records = canon + deferred + sweep
    got = run_parser(prog, tmp_path, records)
    n_canon = 0
    for (kind, b), g in zip(records, got):
        want = upb(classes, kind, b)
        if g != "D":
            n_canon += 1
            assert g == want, (kind, b.hex(), g, want)  # canonical: exactly what google.protobuf gives
            r = store.packet_from_bytes(kind, b)
            assert line_of(pc.record_fields(r)) == g and store.packet_bytes(kind, r) == b  # and a fixed point of the writer
        assert want is not None or g == "D", (kind, b.hex(), g)  # rejected there: deferred here
    for (kind, b), g in zip(canon, got):
        assert g != "D", (kind, b.hex())  # so the parser cannot pass by deferring everything
    for (kind, b), g in zip(deferred, got[len(canon):]):
        assert g == "D", (kind, b.hex())
    assert n_canon > len(canon) + 1000  # payload-byte mutants stay canonical
    for kind in KINDS:
        assert len(pc.record_of_length(kind, 4096)) == 4096 and len(pc.record_of_length(kind, 4097)) == 4097


def test_writer_equals_serialize_to_string(classes):
    gold = pc.load_golden()
    for kname, kind in pc.KINDS.items():
        for name, r in pc.edge_records(kind).items():
            b = store.packet_bytes(kind, r)
            assert b == pc.to_message(classes[kind], kind, r).SerializeToString() == bytes.fromhex(gold["edge"][kname][name]), name
        assert store.packet_bytes(kind, {}) == b"" and store.packet_bytes(kind, {"round": 0, "signature": b""}, "") == bytes([0x22 if kind == pc.BP else 0x2a, 0])
        # the short form of the metadata
        assert store.packet_bytes(kind, {"round": 1}, "x") == store.packet_bytes(kind, {"round": 1, "metadata": {"beacon_id": "x"}})
    # varint sizes of the round: 1, 2, 5, 9 and 10 bytes
    for r, n in ((1, 1), (128, 2), ((1 << 28) + 5, 5), ((1 << 56) + 9, 9), ((1 << 64) - 1, 10)):
        assert len(store.packet_bytes(pc.BP, {"round": r})) == 1 + n
    with pytest.raises(ValueError):
        store.packet_bytes(pc.BP, {"round": 1 << 64})


def mutate(rng, kind, base):
    """One mutated record: flips, cuts, insertions, reorders, duplicates, a merged double metadata, unknown fields of
    every wire type, field number 0, overlong varints, invalid UTF-8."""
    b = bytearray(base)
    meta_tag = 0x22 if kind == pc.BP else 0x2a
    unknown = rng.choice([7, 15, 16, 1000])

    def tag(num, wt):
        out = bytearray()
        store._pb_put_varint(out, (num << 3) | wt)
        return bytes(out)

    def fields(buf):  # the top-level fields of a well-formed record
        out, i = [], 0
        while i < len(buf):
            j = i
            num, wt, i = store._pb_tag(buf, i)
            i = store._pb_skip(buf, i, num, wt)
            out.append(bytes(buf[j:i]))
        return out

    for _ in range(rng.choice([1, 1, 1, 2, 3])):
        op = rng.randrange(16)
        at = rng.randrange(len(b) + 1)
        if op == 0 and b:
            b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
        elif op == 1 and b:
            b[rng.randrange(len(b))] = rng.choice(MUTANTS)
        elif op == 2:
            del b[at:]
        elif op == 3:
            b[at:at] = bytes(rng.randrange(256) for _ in range(rng.randrange(1, 4)))
        elif op in (4, 5, 6):
            try:
                fs = fields(bytes(b))
            except ValueError:
                continue
            if not fs:
                continue
            if op == 4:
                rng.shuffle(fs)
            elif op == 5:
                fs.insert(rng.randrange(len(fs) + 1), rng.choice(fs))
            else:  # a second metadata that merges into the first
                fs.append(bytes([meta_tag]) + rng.choice([b"\x00", b"\x03\x12\x01z", b"\x04\x1a\x02\x01\x02", b"\x04\x0a\x02\x08\x07",
                                                           b"\x06\x0a\x04\x22\x02\xc3\xa9", b"\x05\x0a\x03\x22\x01\xff"]))
            b = bytearray(b"".join(fs))
        elif op == 7:
            b += tag(unknown, 0) + rng.choice([b"\x00", b"\x7f", b"\xff\x01", b"\xff" * 9 + b"\x01", b"\xff" * 9 + b"\x7f", b"\xff" * 10 + b"\x01"])
        elif op == 8:
            b += tag(unknown, 1) + bytes(rng.choice([8, 8, 8, 7]))
        elif op == 9:
            b += tag(unknown, 2) + rng.choice([b"\x00", b"\x02ab", b"\x05ab", b"\x80\x00", b"\xff\xff\xff\xff\x07", b"\xff\xff\xff\xff\x0f"])
        elif op == 10:
            inner = rng.choice([b"", tag(3, 0) + b"\x01", tag(unknown + 1, 3) + tag(unknown + 1, 4), tag(2, 2) + b"\x01a"])
            end = rng.choice([tag(unknown, 4), tag(unknown, 4), tag(unknown + 1, 4), b""])
            b[at if rng.random() < 0.3 else len(b):0] = tag(unknown, 3) + inner + end
        elif op == 11:
            b += tag(unknown, 5) + bytes(rng.choice([4, 4, 3]))
        elif op == 12:
            b[at if rng.random() < 0.5 else len(b):0] = rng.choice([b"\x00", b"\x00\x00", b"\x02\x00", b"\x80\x00", b"\x04", b"\x06\x00", b"\x07"])
        elif op == 13:  # overlong varints: the round, a tag, a length
            rnd_tag = 0x10 if kind == pc.BP else 0x08
            b += rng.choice([bytes([rnd_tag]) + b"\x85\x80\x00", bytes([rnd_tag]) + b"\x80" * 9 + b"\x00", bytes([rnd_tag]) + b"\x80" * 9 + b"\x02",
                             bytes([rnd_tag]) + b"\x80" * 10 + b"\x00", bytes([rnd_tag | 0x80, 0x00]) + b"\x05", bytes([rnd_tag | 0x80, 0x80, 0x80, 0x80, 0x00, 5]),
                             bytes([rnd_tag | 0x80, 0x80, 0x80, 0x80, 0x80, 0x00, 5]), bytes([0x1a, 0x81, 0x00, 0x55]),
                             bytes([0x80, 0x80, 0x80, 0x80, 0x10, 0x01])])
        elif op == 14:  # strings that are not UTF-8, in beaconID and in prerelease
            b += bytes([meta_tag]) + rng.choice([b"\x03\x12\x01\xff", b"\x04\x12\x02\xc3\x28", b"\x05\x12\x03\xed\xa0\x80", b"\x04\x12\x02\xc0\x80",
                                                 b"\x06\x12\x04\xf4\x90\x80\x80", b"\x06\x0a\x04\x22\x02\xc3\x28", b"\x04\x12\x02\xc3\xa9",
                                                 b"\x06\x1a\x04\xff\xfe\xfd\xfc"])
        else:  # a wrong wire type for a known field
            b += rng.choice([tag(2, 2) + b"\x01a", tag(3, 0) + b"\x05", tag(1, 5) + b"abcd", tag(4, 0) + b"\x01", tag(1, 1) + b"12345678"])
    return bytes(b)


def test_host_decoder_agrees_with_protobuf_on_mutants(classes):
    rng = random.Random(20261)
    n, n_ok, n_bad = 0, 0, 0
    for kind in KINDS:
        bases = [store.packet_bytes(kind, r) for r in pc.edge_records(kind).values()]
        for k in range(12000):
            b = mutate(rng, kind, bases[k % len(bases)])
            want = upb(classes, kind, b)
            try:
                got = line_of(pc.record_fields(store.packet_from_bytes(kind, b)))
            except store.DECODE_ERRORS:
                got = None
            assert got == want, (kind, b.hex(), got, want)
            n += 1
            n_ok += want is not None
            n_bad += want is None
    assert n >= 20000 and n_ok > 4000 and n_bad > 4000  # both outcomes are exercised


def frame(data, cap=None):
    lib = _lib.load()
    data = bytes(data)
    cap = 64 if cap is None else cap
    offs, lens = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint32)
    n, used = ctypes.c_size_t(99), ctypes.c_size_t(99)
    rc = lib.dh_pb_frame_delimited(data, len(data), ctypes.c_void_p(offs.ctypes.data), ctypes.c_void_p(lens.ctypes.data), cap, ctypes.byref(n),
                                   ctypes.byref(used))
    return rc, [data[int(o):int(o) + int(l)] for o, l in zip(offs[:min(n.value, cap)], lens)], n.value, used.value


def test_delimited_framing_without_a_device(prog, tmp_path):
    a, b200 = b"\x10\x05", b"\x1a\xc5\x01" + b"s" * 197  # a 1-byte prefix; 200 bytes: a 2-byte prefix
    assert len(b200) == 200
    cases = [
        (b"", [], 0),
        (store.delimited([a]), [a], 3),
        (store.delimited([a, b"", b200, a]), [a, b"", b200, a], 3 + 1 + 202 + 3),
        (store.delimited([a]) + b"\x80", [a], 3),                       # a cut prefix
        (store.delimited([a]) + b"\x05ab", [a], 3),                     # a cut payload
        (store.delimited([a]) + b"\x82\x00" + a, [a], 3),               # a non-minimal prefix
        (store.delimited([a]) + b"\x80\x80\x80\x80\x10", [a], 3),       # a prefix of 2^32
        (b"\xff" * 11, [], 0),
    ]
    for data, want, used in cases:
        assert frame(data) == (_lib.DH_OK, want, len(want), used), data
        assert store.frame_delimited(data) == (want, data[used:])
        path = os.path.join(str(tmp_path), "buf")
        open(path, "wb").write(data)
        out = subprocess.run([prog, "-f", path], capture_output=True, text=True)
        assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
        assert out.stdout.splitlines()[-1] == "consumed %d" % used and len(out.stdout.splitlines()) == len(want) + 1
    data = store.delimited([a, b200, a])
    rc, got, n, _ = frame(data, cap=2)
    assert rc == _lib.DH_EINVAL and n == 3 and got == [a, b200]  # too small: the count, and the first `cap` records
    assert frame(data, cap=0)[0] == _lib.DH_EINVAL and frame(data, cap=3)[:3] == (_lib.DH_OK, [a, b200, a], 3)


def test_host_check_refusals_and_the_beacon_id():
    from drand_amd import scheme_from_name
    s = scheme_from_name("bls-unchained-g1-rfc9380")
    seen = []
    recs = [store.packet_bytes(pc.BP, {"round": 1, "signature": b"\x00"}, "a"), store.packet_bytes(pc.BP, {"round": 2}, "b"), b"\xff",
            store.packet_bytes(pc.BP, {"round": 3}), b""]
    st = store.check_packets_host(pc.BP, recs, s, b"", beacon_id="a", verify=lambda sc, pk, r: seen.extend(r) or [])
    inv, nosig, seq, bid = store.AR_INVALID, store.AR_NO_SIGNATURE, store.AR_SEQUENCE, store.AR_BEACON_ID
    assert list(st) == [inv, inv | nosig | bid, inv, inv | nosig, inv | nosig | seq] and not seen
    st = store.check_packets_host(pc.BP, recs, s, b"", verify=lambda sc, pk, r: [])
    assert not any(x & bid for x in st)  # no expected ID: no comparison
    st = store.check_packets_host(pc.BP, recs[:2], s, b"", beacon_id=b"", verify=lambda sc, pk, r: [])
    assert all(x & bid for x in st)  # the empty ID is an ID
    assert store.packet_from_bytes(pc.BP, b"")["beacon_id"] is None and store.packet_from_bytes(pc.BP, b"\x22\x00")["beacon_id"] == ""


@pytest.mark.parametrize("name", ac.SCHEMES)
def test_recorded_statuses(oracle, name):
    """check_packets_host with the oracle verifying on the clean and the faulty run of both kinds: with the anchor, without
    one, with one the chain does not follow, and without an expected beacon ID."""
    gold, gold_ar = pc.load_golden(), ac.load_golden()
    got = pc.host_status(name, gold_ar, oracle, {})
    assert got == gold["status"][name]
    chained = name == "pedersen-bls-chained"
    inv, rnd, seq, link, bid = store.AR_INVALID, store.AR_RANDOMNESS, store.AR_SEQUENCE, store.AR_LINK if chained else 0, store.AR_BEACON_ID
    for kname, kind in pc.KINDS.items():
        st = {m: list(bytes.fromhex(h)) for m, h in got[kname].items()}
        assert not any(st["clean"]) and len(st["clean"]) == ac.N
        r = rnd if kind == pc.PR else 0  # a BeaconPacket carries no randomness
        want = {10: inv | r, 20: inv | r, 30: inv | r | store.AR_NO_SIGNATURE, 40: r, 50: seq | link, 60: seq | link, 75: bid, 76: bid, 78: bid,
                90: inv, 91: seq | link, 100: inv | store.AR_NO_SIGNATURE | seq | link, 101: seq | link, 140: bid}
        if chained:
            want.update({11: link, 21: link, 31: link, 70: inv | link})
        want = {k: v for k, v in want.items() if v}
        assert {i: x for i, x in enumerate(st["anchor"]) if x} == want
        assert st["no_anchor"] == st["anchor"] and st["bad_anchor"][0] == seq | link and st["bad_anchor"][1:] == st["anchor"][1:]
        assert st["id_unset"] == [x & ~bid for x in st["anchor"]]
