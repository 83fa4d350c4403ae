"""Batch sign.Scheme.Verify under many keys (dh_bls_verify_batch, dh_identity_verify_batch; drandhip.cpp auth_core):
the schemes' AuthScheme (crypto/schemes.go:102,143,183) and the identity self-signatures (key/keys.go:61-64) on the
device, for messages of any length. Every verdict is compared with the CPU oracle's bls.Verify on the same item, and
the two paths of the entry (per-item leaf checks; the random-linear-combination check with its per-key and per-item
fallback levels), forced through DRANDHIP_AUTH_PATH, must agree bit for bit."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

from kat import SIGN_KAT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SCHEMES = ["pedersen-bls-chained", "pedersen-bls-unchained", "bls-unchained-on-g1", "bls-unchained-g1-rfc9380"]
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
# the b_0 preimage of expand_message_xmd is 111 + len bytes: lengths = 8, 9, 16, 17 mod 64 sit on SHA-256's padding
# boundaries (one or two closing blocks; the tail ending exactly at a block)
LENGTHS = [0, 1, 8, 9, 16, 17, 18, 31, 32, 33, 72, 73, 80, 81, 200, 1000]


@pytest.fixture(scope="module")
def dh():
    import torch
    import drand_amd
    from drand_amd import _lib
    torch.zeros(1, device="cuda")
    lib = _lib.load()
    assert lib.dh_init(0) == 0, _lib.last_error()
    return drand_amd


def _sk(tag):
    return (int.from_bytes(hashlib.sha256(tag).digest(), "big") % R_ORDER).to_bytes(32, "big")


def _forced(path, fn):
    """fn() with DRANDHIP_AUTH_PATH = path (None: the library's own choice); the variable is read at every call."""
    old = os.environ.pop("DRANDHIP_AUTH_PATH", None)
    if path:
        os.environ["DRANDHIP_AUTH_PATH"] = path
    try:
        return fn()
    finally:
        os.environ.pop("DRANDHIP_AUTH_PATH", None)
        if old is not None:
            os.environ["DRANDHIP_AUTH_PATH"] = old


def _verify(s, path, keys, msgs, sigs, kidx=None, seed=1):
    sg = np.array([np.frombuffer(x, np.uint8) for x in sigs])
    v, kok, stats = _forced(path, lambda: s.verify_signatures(keys, msgs, sg, kidx, seed=seed, want_stats=True))
    return v.tolist(), kok.tolist(), stats


def _identities(dh):
    fx = json.load(open(os.path.join(GOLD, "identities.json")))
    s = dh.scheme_from_name(fx["scheme"])
    keys = [bytes.fromhex(x["key"]) for x in fx["nodes"]]
    sigs = np.array([np.frombuffer(bytes.fromhex(x["signature"]), np.uint8) for x in fx["nodes"]])
    return s, keys, sigs


@pytest.mark.parametrize("path", [None, "leaf", "rlc"])
def test_reference_identities(dh, path):
    """The three self-signed identities of the reference's test group (test/default.toml) are valid; with the
    signatures rotated by one, none is."""
    s, keys, sigs = _identities(dh)
    assert s.identity_hash(keys[0]) == hashlib.blake2b(keys[0], digest_size=32).digest()
    assert _forced(path, lambda: s.verify_identities(keys, sigs)).tolist() == [True] * 3
    assert _forced(path, lambda: s.verify_identities(keys, np.roll(sigs, 1, axis=0))).tolist() == [False] * 3


def test_sign_kat(dh, oracle):
    """The reference's own AuthScheme vector (crypto/curve_test.go:10-31): an 18-byte message, not a digest."""
    sk, msg, sig = SIGN_KAT
    s = dh.scheme_from_name("pedersen-bls-chained")
    key = s.public_key(sk)
    assert key == oracle.public_key(s.name, sk) and len(msg) == 18
    auth = dh.AuthScheme(s)
    auth.verify(key, msg, sig)
    bad = bytes([msg[0] ^ 1]) + msg[1:]
    with pytest.raises(dh.SchemeError, match="bls: invalid signature"):
        auth.verify(key, bad, sig)
    for path in ("leaf", "rlc"):
        assert _verify(s, path, [key], [msg, bad], [sig, sig], [0, 0])[0] == [True, False]


@pytest.mark.parametrize("scheme", SCHEMES)
def test_any_length_messages(dh, oracle, scheme):
    """96 items under 3 keys (and a fourth table entry that does not decode), the message lengths cycling through
    LENGTHS, with one item of each fault class; verdicts equal the oracle's on every item on both paths."""
    s = dh.scheme_from_name(scheme)
    rng = random.Random(scheme)
    sks = [_sk(b"auth-%d" % k) for k in range(3)]
    keys = [oracle.public_key(scheme, sk) for sk in sks] + [b"\xff" * s.key_len]
    kidx = [i % 3 for i in range(96)]
    msgs = [bytes(rng.getrandbits(8) for _ in range(LENGTHS[i % 16])) for i in range(96)]
    sigs = [oracle.sign(scheme, sks[kidx[i]], msgs[i]) for i in range(96)]
    sigs[5] = oracle.sign(scheme, sks[(kidx[5] + 1) % 3], msgs[5])         # valid under another key of the table
    msgs[10] = msgs[10][:40] + bytes([msgs[10][40] ^ 0x10]) + msgs[10][41:]  # one message byte changed (72 bytes)
    sigs[17] = sigs[17][:20] + bytes([sigs[17][20] ^ 1]) + sigs[17][21:]    # one signature bit flipped
    sigs[22] = b"\xc0" + bytes(s.sig_len - 1)                                # the infinity encoding
    sigs[29] = bytes([sigs[29][0] ^ 0x20]) + sigs[29][1:]                    # -sigma
    kidx[40] = 3                                                             # an item under the invalid key
    want = [oracle.verify(scheme, keys[kidx[i]], msgs[i], sigs[i]) for i in range(96)]
    assert [i for i, w in enumerate(want) if not w] == [5, 10, 17, 22, 29, 40]
    leaf = _verify(s, "leaf", keys, msgs, sigs, kidx)
    rlc = _verify(s, "rlc", keys, msgs, sigs, kidx)
    assert leaf[0] == want and rlc[0] == want
    assert leaf[1] == rlc[1] == [True, True, True, False]
    assert leaf[2][3] == rlc[2][3] == 6 and leaf[2][0] == 0 and rlc[2][0] == 3


@pytest.mark.parametrize("scheme", ["pedersen-bls-chained", "bls-unchained-g1-rfc9380"])
def test_key_table(dh, oracle, scheme):
    """6 keys: one that does not decode, one on-curve point outside the subgroup (a non-subgroup signature of a
    scheme that signs in this scheme's key group), one duplicate. key_ok is the oracle's decode result per key;
    items under bad keys get 0, every other item the oracle's verdict."""
    s = dh.scheme_from_name(scheme)
    neg = json.load(open(os.path.join(GOLD, "negatives.json")))
    donor = "bls-unchained-on-g1" if s.key_len == 48 else "pedersen-bls-unchained"
    outside = bytes.fromhex([c for c in neg[donor]["cases"] if c["name"] == "non_subgroup"][0]["sig"])
    sks = [_sk(b"table-%d" % k) for k in range(3)]
    pk = [oracle.public_key(scheme, sk) for sk in sks]
    undecodable = bytes([pk[0][0] & 0x7f]) + pk[0][1:]  # compression flag cleared
    keys = [pk[0], undecodable, pk[1], outside, pk[0], pk[2]]
    signer = {0: 0, 1: 0, 2: 1, 3: 1, 4: 0, 5: 2}
    key_g2 = s.key_len == 96
    assert len(outside) == s.key_len and [oracle.decode(key_g2, k) == 1 for k in keys] == [True, False, True, False, True, True]
    rng = random.Random(scheme + "/table")
    kidx = [i % 6 for i in range(36)]
    msgs = [bytes(rng.getrandbits(8) for _ in range((32, 5, 100)[i % 3])) for i in range(36)]
    sigs = [oracle.sign(scheme, sks[signer[kidx[i]]], msgs[i]) for i in range(36)]
    sigs[8] = sigs[14]  # another item's signature, under a good key
    want = [oracle.verify(scheme, keys[kidx[i]], msgs[i], sigs[i]) for i in range(36)]
    assert want == [kidx[i] not in (1, 3) and i != 8 for i in range(36)]
    for path in ("leaf", "rlc"):
        v, kok, _ = _verify(s, path, keys, msgs, sigs, kidx)
        assert kok == [oracle.decode(key_g2, k) == 1 for k in keys]
        assert v == want


@pytest.mark.parametrize("scheme", ["pedersen-bls-unchained", "bls-unchained-on-g1"])
def test_one_key_per_item(dh, oracle, scheme):
    """70 identities (above the small-batch limit of 64), each self-signed under its own key, 2 corrupted."""
    s = dh.scheme_from_name(scheme)
    sks = [_sk(b"id-%d" % k) for k in range(70)]
    keys = [oracle.public_key(scheme, sk) for sk in sks]
    hashes = [hashlib.blake2b(k, digest_size=32).digest() for k in keys]
    sigs = [oracle.sign(scheme, sk, h) for sk, h in zip(sks, hashes)]
    sigs[13] = sigs[14]
    sigs[69] = bytes([sigs[69][0] ^ 0x20]) + sigs[69][1:]  # -sigma: decodes, so its key reaches the per-key check
    want = [oracle.verify(scheme, k, h, x) for k, h, x in zip(keys, hashes, sigs)]
    assert [i for i, w in enumerate(want) if not w] == [13, 69]
    sg = np.array([np.frombuffer(x, np.uint8) for x in sigs])
    for path in (None, "leaf", "rlc"):
        assert _forced(path, lambda: s.verify_identities(keys, sg)).tolist() == want
    assert _verify(s, "rlc", keys, hashes, sigs)[2][:3] == (3, 2, 2)  # two failing keys, one item each


@pytest.mark.parametrize("scheme", ["pedersen-bls-unchained", "bls-unchained-g1-rfc9380"])
def test_isolation(dh, oracle, scheme):
    """192 items over 3 keys, 64 each, 32-byte messages; one bad item under key 1: the per-key level finds key 1 and
    only its 64 items get leaf checks. Without the bad item nothing falls back."""
    s = dh.scheme_from_name(scheme)
    sks = [_sk(b"iso-%d" % k) for k in range(3)]
    keys = [oracle.public_key(scheme, sk) for sk in sks]
    kidx = [i // 64 for i in range(192)]
    msgs = [hashlib.sha256(b"iso %d" % i).digest() for i in range(192)]
    good = [oracle.sign(scheme, sks[kidx[i]], msgs[i]) for i in range(192)]
    sigs = list(good)
    sigs[100] = good[101]
    want = [oracle.verify(scheme, keys[kidx[i]], msgs[i], sigs[i]) for i in range(192)]
    assert want == [i != 100 for i in range(192)]
    v, kok, stats = _verify(s, "rlc", keys, msgs, sigs, kidx)
    assert v == want and kok == [True] * 3
    assert stats == (3, 1, 64, 1)
    assert _verify(s, "leaf", keys, msgs, sigs, kidx)[0] == want
    # the same batch with no bad item (item 100's own signature verifies: the oracle, one call)
    assert oracle.verify(scheme, keys[1], msgs[100], good[100])
    v, _, stats = _verify(s, "rlc", keys, msgs, good, kidx)
    assert v == [True] * 192 and stats == (1, 0, 0, 0)


def test_arguments(dh):
    from drand_amd import _lib
    lib = _lib.load()
    s, keys, sigs = _identities(dh)
    n = 3
    ktab = np.frombuffer(b"".join(keys), np.uint8).copy()
    msgs = np.zeros(32 * n, np.uint8)
    off = np.arange(n + 1, dtype=np.uint32) * 32
    verdict = np.full(n, 7, np.uint8)

    def call(n_keys, kidx, off, n):
        return lib.dh_bls_verify_batch(s.id, ktab.ctypes.data, n_keys, kidx.ctypes.data if kidx is not None else None,
                                       msgs.ctypes.data, off.ctypes.data, sigs.ctypes.data, s.sig_len, n,
                                       verdict.ctypes.data, None, 1, None)

    assert call(3, np.array([0, 3, 1], np.uint32), off, n) == _lib.DH_EINVAL     # index out of range
    assert call(3, None, np.array([0, 64, 32, 96], np.uint32), n) == _lib.DH_EINVAL  # decreasing msg_off
    assert call(2, None, off, n) == _lib.DH_EINVAL                               # key_idx NULL, n_keys != n
    assert call(0, np.array([0, 0, 0], np.uint32), off, n) == _lib.DH_EINVAL     # items and no keys
    assert call(0, None, off, 0) == _lib.DH_OK                                   # n == 0
    assert call(3, np.zeros(0, np.uint32), off, 0) == _lib.DH_OK
    assert verdict.tolist() == [7] * n
    assert call(3, None, off, n) == _lib.DH_OK and verdict.tolist() == [0] * n   # zero messages: none is valid
