"""Shared builders of the protobuf packet cases of tests/test_packet_host.py (CPU) and tests/test_gpu_packet.py (GPU):
the same deterministic records on both sides. The signed chains are those of tests/golden/archive_cases.json (read, not
changed). The statuses check_packets_host gives with the oracle verifying, and the google.protobuf bytes of the edge
records, are pinned in tests/golden/packet_cases.json (python tests/packet_cases.py rewrites it); the GPU test compares
the device path against that record and against packet_bytes, never against the code under test, and never imports
google.protobuf."""
import hashlib
import json
import os

import archive_cases as ac
from bolt_cases import SCHEMES, rand_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
CASES_JSON = os.path.join(HERE, "golden", "packet_cases.json")
BP, PR = 1, 2  # DH_PB_BEACON_PACKET, DH_PB_PUBLIC_RAND
KINDS = {"beacon_packet": BP, "public_rand": PR}
BEACON_ID = "default"
MODES = {"anchor": (ac.anchor, BEACON_ID), "no_anchor": (lambda name: None, BEACON_ID), "bad_anchor": (ac.bad_anchor, BEACON_ID),
         "id_unset": (ac.anchor, None)}


def load_golden():
    return json.load(open(CASES_JSON))


def message_classes():
    """{kind: message class} of google.protobuf, built from a FileDescriptorProto written here with the field numbers of
    pbwire.hpp (CPU tests only)."""
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name="packet_cases.proto", package="pc", syntax="proto3")

    def msg(name, fields):
        m = fd.message_type.add(name=name)
        for num, (fname, ftype, tname, opt) in enumerate(fields, 1):
            f = m.field.add(name=fname, number=num, type=ftype, label=F.LABEL_OPTIONAL)
            if tname:
                f.type_name = ".pc." + tname
            if opt:  # explicit presence: a synthetic oneof
                m.oneof_decl.add(name="_" + fname)
                f.oneof_index = len(m.oneof_decl) - 1
                f.proto3_optional = True
    msg("NodeVersion", [("major", F.TYPE_UINT32, None, 0), ("minor", F.TYPE_UINT32, None, 0), ("patch", F.TYPE_UINT32, None, 0),
                        ("prerelease", F.TYPE_STRING, None, 1)])
    msg("Metadata", [("node_version", F.TYPE_MESSAGE, "NodeVersion", 0), ("beaconID", F.TYPE_STRING, None, 0), ("chain_hash", F.TYPE_BYTES, None, 0)])
    msg("BeaconPacket", [("previous_signature", F.TYPE_BYTES, None, 0), ("round", F.TYPE_UINT64, None, 0), ("signature", F.TYPE_BYTES, None, 0),
                         ("metadata", F.TYPE_MESSAGE, "Metadata", 0)])
    msg("PublicRandResponse", [("round", F.TYPE_UINT64, None, 0), ("signature", F.TYPE_BYTES, None, 0), ("previous_signature", F.TYPE_BYTES, None, 0),
                               ("randomness", F.TYPE_BYTES, None, 0), ("metadata", F.TYPE_MESSAGE, "Metadata", 0)])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    get = message_factory.GetMessageClass
    return {BP: get(pool.FindMessageTypeByName("pc.BeaconPacket")), PR: get(pool.FindMessageTypeByName("pc.PublicRandResponse"))}


def to_message(cls, kind, rec):
    """The google.protobuf message of a packet_bytes record dict."""
    m = cls()
    m.round = rec.get("round", 0)
    m.signature = rec.get("signature", b"")
    m.previous_signature = rec.get("previous_signature", b"")
    if kind == PR:
        m.randomness = rec.get("randomness", b"")
    md = rec.get("metadata")
    if md is not None:
        m.metadata.SetInParent()
        m.metadata.beaconID = md.get("beacon_id", "")
        m.metadata.chain_hash = md.get("chain_hash", b"")
        nv = md.get("node_version")
        if nv is not None:
            m.metadata.node_version.SetInParent()
            for k in ("major", "minor", "patch"):
                setattr(m.metadata.node_version, k, nv.get(k, 0))
            if nv.get("prerelease") is not None:
                m.metadata.node_version.prerelease = nv["prerelease"]
    return m


def message_fields(m, kind):
    """(round, signature, previous_signature, randomness, metadata present, beaconID) of a parsed message."""
    return (m.round, m.signature, m.previous_signature, m.randomness if kind == PR else b"", m.HasField("metadata"),
            m.metadata.beaconID if m.HasField("metadata") else None)


def record_fields(r):
    return (r["round"], r["signature"], r["previous_signature"], r["randomness"], r["metadata"] is not None, r["beacon_id"])


def g1_rec(i, kind=BP):
    s = rand_bytes("g1 sig %d" % i, 48)
    return {"round": 1 + i, "signature": s, "previous_signature": b"", "randomness": hashlib.sha256(s).digest() if kind == PR else b""}


def g2_rec(i, kind=BP):
    s = rand_bytes("g2 sig %d" % i, 96)
    return {"round": 2634945 + i, "signature": s, "previous_signature": rand_bytes("g2 sig %d" % (i - 1), 96),
            "randomness": hashlib.sha256(s).digest() if kind == PR else b""}


NODE_VERSION = {"major": 2, "minor": 1, "patch": 3, "prerelease": "rc1"}
FULL_META = {"node_version": NODE_VERSION, "beacon_id": BEACON_ID, "chain_hash": rand_bytes("chain hash", 32)}


def edge_records(kind):
    """{name: record dict} of the canonical edges: the empty record, each field alone, the empty sub-messages, node_version,
    rounds whose varints take 1, 2, 5, 9 and 10 bytes, lengths 127 / 128."""
    out = {"empty": {}, "round": {"round": 7}, "signature": {"signature": rand_bytes("e sig", 48)},
           "previous": {"previous_signature": rand_bytes("e prev", 96)}, "meta_empty": {"metadata": {}},
           "meta_id": {"metadata": {"beacon_id": "x"}}, "meta_chain_hash": {"metadata": {"chain_hash": b"\x01\x02"}},
           "meta_nv_empty": {"metadata": {"node_version": {}}}, "meta_nv_pre_empty": {"metadata": {"node_version": {"prerelease": ""}}},
           "meta_full": dict(g2_rec(3, kind), metadata=FULL_META), "g1": dict(g1_rec(5, kind), metadata={"beacon_id": BEACON_ID}),
           "g2": dict(g2_rec(5, kind), metadata={"beacon_id": BEACON_ID}), "g2_bare": g2_rec(6, kind)}
    if kind == PR:
        out["randomness"] = {"randomness": rand_bytes("e rand", 32)}
    for r in (1, 127, 128, (1 << 28) + 5, (1 << 35) - 1, (1 << 56) + 9, (1 << 63) - 1, 1 << 63, (1 << 64) - 1):
        out["round_%d" % r] = {"round": r, "signature": b"\x00"}
    for n in (1, 127, 128, 129):
        out["sig_len_%d" % n] = {"round": 9, "signature": rand_bytes("long sig", n)}
    out["id_len_127"] = {"round": 3, "metadata": {"beacon_id": "a" * 127}}
    out["id_len_128"] = {"round": 3, "metadata": {"beacon_id": "b" * 128}}
    return out


def record_of_length(kind, n):
    """A canonical record of exactly n bytes (n >= 200): one long signature."""
    from drand_amd.store import packet_bytes
    for pad in range(4):  # the length varint's size moves with the length
        b = packet_bytes(kind, {"round": 1, "signature": b"\xab" * (n - 8 + pad)})
        if len(b) >= n:
            b = packet_bytes(kind, {"round": 1, "signature": b"\xab" * (n - 8 + pad - (len(b) - n))})
            assert len(b) == n, (len(b), n)
            return b
    raise AssertionError(n)


def deferred_records(kind):
    """One record per deferred class of DESIGN.md §26; the host decoder accepts some of them, the device none."""
    from drand_amd.store import packet_bytes
    g2 = packet_bytes(kind, g2_rec(1, kind), BEACON_ID)
    rnd = b"\x10" if kind == BP else b"\x08"       # the round's tag
    sig = b"\x1a" if kind == BP else b"\x12"       # the signature's tag
    meta = b"\x22" if kind == BP else b"\x2a"
    last = 5 if kind == BP else 6                  # the first unknown field number
    out = [
        sig + b"\x01\x55" + rnd + b"\x05",  # another order: round after signature
        rnd + b"\x05" + rnd + b"\x06",                                 # a repeated scalar
        meta + b"\x00" + meta + b"\x00",                               # a repeated (merged) sub-message
        g2 + bytes([last << 3, 1]),                                    # an unknown varint field
        g2 + bytes([(last << 3) | 1]) + b"\x00" * 8,                   # unknown fixed64
        g2 + bytes([(last << 3) | 2, 2, 9, 9]),                        # unknown bytes
        g2 + bytes([(last << 3) | 3, (last << 3) | 4]),                # an unknown group
        g2 + bytes([(last << 3) | 5]) + b"\x00" * 4,                   # unknown fixed32
        bytes([rnd[0] | 2, 1, 5]),                                     # the round with wire type 2
        bytes([sig[0] & ~7 & 0xff, 5]),                                # the signature as a varint
        rnd + b"\x85\x00",                                             # a non-minimal varint
        rnd + b"\x00",                                                 # an explicit zero round
        sig + b"\x00",                                                 # an empty bytes field
        sig + b"\x81\x00\x55",                                         # a non-minimal length
        rnd + b"\xff" * 9 + b"\x02",                                   # a tenth byte above 1
        rnd + b"\xff" * 10 + b"\x01",                                  # eleven bytes
        sig + b"\x05\x01\x02",                                         # an extent past the record
        meta + b"\x05\x12\x01a",                                       # a sub-message past the record
        meta + b"\x04\x12\x05ab",                                      # a string past its sub-message
        meta + b"\x03\x12\x01\xc3",                                    # a byte above 0x7f in beaconID (invalid UTF-8 at that)
        meta + b"\x04\x12\x02\xc3\xa9",                                # valid UTF-8, still not ascii
        meta + b"\x02\x12\x00",                                        # an empty beaconID written out
        meta + b"\x04\x0a\x02\x08\x00",                                # node_version with an explicit zero
        meta + b"\x09\x0a\x07\x08\x80\x80\x80\x80\x10",                # a V32 of 2^32
        meta + b"\x06\x0a\x04\x22\x02\xc3\xa9",                        # prerelease not ascii
        meta + b"\x02\x1a\x00",                                        # an empty chain_hash written out
        meta + b"\x02\x20\x01",                                        # an unknown field inside metadata
        g2[:-1],                                                       # cut
        g2 + b"\x00",                                                  # field number 0 behind the record
        b"\x00",                                                       # field number 0
        b"\xff",                                                       # a cut tag
        record_of_length(kind, 4097),                                  # above PBWIRE_MAX_RECORD
        record_of_length(kind, 6000),
    ]
    return out


def chain_packets(name, gold_ar, kind, beacon_id=BEACON_ID):
    from drand_amd.store import packet_bytes
    recs = ac.chain_records(name, gold_ar)
    return recs, [packet_bytes(kind, r if kind == PR else dict(r, randomness=b""), beacon_id) for r in recs]


def faulty_run(name, gold_ar, kind):
    """The 300 records with a fault of every status bit injected; the list of records' bytes."""
    from drand_amd.store import packet_bytes
    recs, out = chain_packets(name, gold_ar, kind)

    def edit(i, beacon_id=BEACON_ID, **kw):
        r = dict(recs[i], **kw)
        out[i] = packet_bytes(kind, r if kind == PR else dict(r, randomness=b""), beacon_id)

    s = recs[10]["signature"]
    edit(10, signature=s[:20] + bytes([s[20] ^ 1]) + s[21:])     # a corrupted signature
    edit(20, signature=recs[20]["signature"][:-1])               # a short signature
    edit(30, signature=b"")                                      # an empty signature
    edit(40, randomness=hashlib.sha256(b"not it").digest())      # a wrong randomness (kind 2 carries it)
    edit(70, previous_signature=rand_bytes("wrong prev", 96))    # a wrong previous_signature
    edit(75, beacon_id="other")                                  # another beacon ID
    edit(76, beacon_id="")                                       # metadata without an ID
    edit(77, beacon_id=None)                                     # no metadata: never a mismatch
    edit(78, beacon_id=BEACON_ID + "x")                          # a longer ID with the same start
    out[90] = b"\xff\xff"                                        # an undecodable record
    out[100] = b""                                               # the empty record
    unknown = bytes([0x38, 1])                                   # field 7, a varint: decodes on the host, deferred on the device
    for i in (127, 128, 191, 192):  # deferred records next to each other and at the windows' edges
        out[i] = out[i] + unknown
    edit(140, beacon_id="other")                                 # a deferred record with another beacon ID
    out[140] = out[140] + unknown
    del out[50]                                                  # a removed record
    out.insert(60, out[59])                                      # a duplicated record
    return out


def host_status(name, gold_ar, oracle, cache):
    from drand_amd import scheme_from_name
    from drand_amd.store import check_packets_host
    s = scheme_from_name(name)
    pk = bytes.fromhex(gold_ar["chains"][name]["pk"])
    verify = ac.oracle_verify(oracle, cache)
    out = {}
    for kname, kind in KINDS.items():
        run = faulty_run(name, gold_ar, kind)
        out[kname] = {m: bytes(check_packets_host(kind, run, s, pk, anchor=a(name), beacon_id=bid, verify=verify)).hex() for m, (a, bid) in MODES.items()}
        out[kname]["clean"] = bytes(check_packets_host(kind, chain_packets(name, gold_ar, kind)[1], s, pk, anchor=ac.anchor(name), beacon_id=BEACON_ID,
                                                       verify=verify)).hex()
    return out


def compute_golden(oracle):
    """{"status": {scheme: {kind: {mode: hex of the status bytes}}}, "edge": {kind: {name: hex of the google.protobuf bytes}}}"""
    gold_ar = ac.load_golden()
    cls = message_classes()
    gold = {"status": {}, "edge": {}}
    for name in SCHEMES:
        gold["status"][name] = host_status(name, gold_ar, oracle, {})
    for kname, kind in KINDS.items():
        gold["edge"][kname] = {k: to_message(cls[kind], kind, r).SerializeToString().hex() for k, r in edge_records(kind).items()}
    return gold


if __name__ == "__main__":  # rewrite tests/golden/packet_cases.json from the host check, the oracle and google.protobuf
    import sys
    root = os.path.dirname(HERE)
    sys.path[:0] = [root, os.path.join(root, "oracle")]
    import oracle_ctypes
    oracle_ctypes.lib()
    with open(CASES_JSON, "w") as f:
        json.dump(compute_golden(oracle_ctypes), f, indent=1, sort_keys=True)
        f.write("\n")
