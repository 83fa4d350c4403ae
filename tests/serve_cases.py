"""Shared builders of the served-record cases of tests/test_serve_host.py (CPU) and tests/test_gpu_serve.py (GPU): rows of
every shape the encoders of DESIGN.md §28 write, and the bytes expected for them from store.random_data_line and
store.packet_bytes (pinned by the CPU suite, the latter against google.protobuf), never from the code under test. The
signed chains are those of tests/golden/archive_cases.json (read, not changed)."""
import hashlib

import archive_cases as ac
import packet_cases as pc
from bolt_cases import rand_bytes

# every digit count and every varint length, on both sides of each boundary
BOUNDARY_ROUNDS = [0, 1] + [v for k in range(1, 20) for v in (10 ** k - 1, 10 ** k)] + [1 << 32, 1 << 63, (1 << 64) - 1]
CORRUPTED = (10, 63, 64, 200, 299)  # the indices of the golden chain's records whose signature is corrupted below


def shaped_rows(n, seed):
    """Rows mixing G1 and chained G2 shapes with previous signatures of 96, 32 and 0 bytes, signature lengths 0, 1, 3 and
    47, round 0 and the boundary rounds."""
    out = []
    for i in range(n):
        k = (i + seed) % 13
        r = dict(pc.g2_rec(i) if i % 2 else pc.g1_rec(i))
        if k == 2:
            r["previous_signature"] = rand_bytes("serve seed %d" % i, 32)
        elif k == 3:
            r["round"] = 0
        elif k == 4:
            r["previous_signature"] = b""
        elif k == 5:
            r["signature"] = b""
        elif k in (6, 7, 8):
            r["signature"] = rand_bytes("serve odd %d" % i, {6: 1, 7: 3, 8: 47}[k])
        elif k == 9:
            r["round"] = BOUNDARY_ROUNDS[i % len(BOUNDARY_ROUNDS)]
        elif k == 10:
            r = {"round": 0, "signature": b"", "previous_signature": b""}
        r.pop("randomness", None)
        out.append(r)
    return out


def boundary_rows():
    return [dict(pc.g2_rec(i) if i % 3 else pc.g1_rec(i), round=r) for i, r in enumerate(BOUNDARY_ROUNDS)]


def with_randomness(rows, rands=None):
    """The record dicts the host writers take: randomness = the given 32-byte row, else SHA-256 of the signature."""
    return [dict(r, randomness=rands[i] if rands is not None else hashlib.sha256(r["signature"]).digest()) for i, r in enumerate(rows)]


def want_json(rows, rands=None, keep=None, newline=True, want_prev=True):
    """(the bytes dh_rand_encode_device must write for the JSON form, the record lengths it must report)."""
    from drand_amd.store import random_data_line
    recs = [random_data_line(r if want_prev else dict(r, previous_signature=b"")) for r in with_randomness(rows, rands)]
    kept = [b if keep is None or keep[i] else None for i, b in enumerate(recs)]
    return b"".join(b + (b"\n" if newline else b"") for b in kept if b is not None), [len(b) if b is not None else 0 for b in kept]


def want_pb(rows, rands=None, keep=None, delimited=False, metadata=None, want_prev=True):
    """The same for the PublicRandResponse form; metadata: None or the dict packet_bytes takes."""
    from drand_amd import store
    recs = [store.packet_bytes(pc.PR, dict(r if want_prev else dict(r, previous_signature=b""), metadata=metadata))
            for r in with_randomness(rows, rands)]
    kept = [b if keep is None or keep[i] else None for i, b in enumerate(recs)]
    live = [b for b in kept if b is not None]
    return (store.delimited(live) if delimited else b"".join(live)), [len(b) if b is not None else 0 for b in kept]


def corrupted_chain(name, gold_ar):
    """The golden chain of one scheme with one signature bit flipped in the records CORRUPTED; previous_signature fields
    keep the true predecessor, so exactly those rounds fail verification."""
    recs = [dict(r) for r in ac.chain_records(name, gold_ar)]
    for i in CORRUPTED:
        s = recs[i]["signature"]
        recs[i]["signature"] = s[:20] + bytes([s[20] ^ 1]) + s[21:]
    return recs


def columns(recs, sig_stride, prev_stride, want_prev=True):
    """The rows as the verifier's columns on the device: [rounds int64, sigs uint8[n, sig_stride], sig_lens int32, prevs,
    prev_lens] (the last two None without want_prev). The padding is 0xCD: it is never read."""
    import numpy as np
    import torch
    n = len(recs)
    rounds = np.array([r.get("round", 0) for r in recs], np.uint64)
    sigs, prevs = np.full((n, sig_stride), 0xCD, np.uint8), np.full((n, prev_stride), 0xCD, np.uint8)
    sl, pl = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i, r in enumerate(recs):
        s, p = r.get("signature", b""), r.get("previous_signature", b"")
        sigs[i, :len(s)], sl[i] = np.frombuffer(s, np.uint8), len(s)
        prevs[i, :len(p)], pl[i] = np.frombuffer(p, np.uint8), len(p)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    out = [dev(rounds.view(np.int64)), dev(sigs), dev(sl)]
    return out + ([dev(prevs), dev(pl)] if want_prev else [None, None])
