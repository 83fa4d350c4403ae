#!/usr/bin/env python3
"""Writes tests/golden/schnorr.json: Schnorr signatures over the key group of each scheme family, as DKGAuthScheme
(kyber v1.1.18 sign/schnorr with the kyber-bls12381 groups) is restated in DESIGN.md §11, with recorded verdicts.

Pure Python (hashlib.sha512 + oracle/bls_py.py); deterministic (seeded). No reference vector exists for this scheme,
so the fixture pins the restatement, not kyber's output. Per key group: 96 items under a table of 12 keys (8 good
ones, an undecodable one, an on-curve point outside the subgroup, the point at infinity, a duplicate of key 0); the
message lengths walk SHA-512's padding boundaries for preimages of 2K + len bytes; every other item is valid and the
rest carry one fault each.

    python3 tests/golden/make_schnorr_golden.py        # rewrites schnorr.json (a few minutes)
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import bls_py as B  # noqa: E402

LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 200, 1000]
# the first six classes get four items each (the swap needs an even count), the others three
FAULTS = ["swap", "wrong_msg", "wrong_key", "s_plus_1", "s_plus_r", "s_zero", "r_negated", "r_x_bit", "r_flag", "r_torsion",
          "key_undecodable", "key_not_in_subgroup", "key_infinity", "wrong_msg_len"]
H1 = (B.U_ABS + 1) ** 2 // 3  # cofactor of E(Fp)
H2 = 0x5d543a95414e7f1091d50792876a202cd91de4547085abaa68a205b2e5a7ddfa628f1cb4d9e82ef21537e293a6691ae1616ec6e786f0c70cf1c38e31c7238e5


class Group:
    def __init__(self, g2):
        self.g2 = g2
        self.K = 96 if g2 else 48
        self.F = B.FP2 if g2 else B.FP
        self.gen = B.G2_GEN if g2 else B.G1_GEN
        self.compress = B.g2_compress if g2 else B.g1_compress
        self.decompress = B.g2_decompress if g2 else B.g1_decompress
        # the scheme whose KEY group this is
        self.scheme = "bls-unchained-g1-rfc9380" if g2 else "pedersen-bls-unchained"

    def mul(self, pt, k):
        return B.ec_mul(self.F, pt, k)

    def add(self, a, b):
        return B.ec_add(self.F, a, b)

    def curve_point(self, rng):
        """a point of the whole curve group (outside the order-r subgroup with overwhelming probability)"""
        if self.g2:
            return B.iso_map_g2(B.sswu_g2((rng.randrange(B.P), rng.randrange(B.P))))
        return B.iso_map_g1(B.sswu_g1(rng.randrange(B.P)))

    def small_order_point(self, rng):
        """T of order 3 on E(Fp) / of order 13 on E'(Fp2)"""
        q, cof = (13, H2) if self.g2 else (3, H1)
        e = 0
        while cof % q == 0:
            cof //= q
            e += 1
        assert e >= 1
        while True:
            t = self.mul(self.curve_point(rng), cof * B.R)
            if t is None:
                continue
            while self.mul(t, q) is not None:
                t = self.mul(t, q)
            return t


_KEY_CACHE = {}


def decode_key(grp, key_bytes):
    """the key rule of dh_bls_verify_batch: a compressed subgroup point, infinity refused; None when refused"""
    ck = (grp.g2, key_bytes)
    if ck not in _KEY_CACHE:
        try:
            _KEY_CACHE[ck] = grp.decompress(key_bytes, True)
        except B.DecodeError:
            _KEY_CACHE[ck] = None
    return _KEY_CACHE[ck]


def challenge(grp, r_bytes, key_bytes, msg):
    return int.from_bytes(hashlib.sha512(r_bytes + key_bytes + msg).digest(), "big") % B.R


def verify(grp, key_bytes, msg, sig):
    """the normative check of DESIGN.md §11; returns 0 or 1"""
    K = grp.K
    if len(sig) != K + 32:
        return 0
    pk = decode_key(grp, key_bytes)
    if pk is None:
        return 0
    try:
        rp = grp.decompress(sig[:K], False)  # flags, x < p, on the curve; no subgroup test
    except B.DecodeError:
        return 0
    if rp is None:
        return 0
    s = int.from_bytes(sig[K:], "big")
    if s >= B.R:
        return 0
    h = challenge(grp, sig[:K], key_bytes, msg)
    return 1 if grp.mul(grp.gen, s) == grp.add(rp, grp.mul(pk, h)) else 0


def sign(grp, sk, key_bytes, msg, rng):
    k = rng.randrange(1, B.R)
    r_bytes = grp.compress(grp.mul(grp.gen, k))
    s = (k + challenge(grp, r_bytes, key_bytes, msg) * sk) % B.R
    return r_bytes + s.to_bytes(32, "big")


def undecodable_key(grp, rng):
    while True:
        b = bytearray(rng.getrandbits(8) for _ in range(grp.K))
        b[0] = 0x80 | (b[0] & 0x1F) % 0x1A  # compressed flag, x < p
        try:
            grp.decompress(bytes(b), False)
        except B.DecodeError:
            return bytes(b)


def make_group(g2, seed):
    grp = Group(g2)
    rng = random.Random(seed)
    K = grp.K
    sks = [rng.randrange(2, B.R) for _ in range(8)]
    keys = [grp.compress(grp.mul(grp.gen, sk)) for sk in sks]
    keys.append(undecodable_key(grp, rng))          # 8
    keys.append(grp.compress(grp.curve_point(rng)))  # 9: on the curve, outside the subgroup
    keys.append(grp.compress(None))                  # 10: infinity
    keys.append(keys[0])                             # 11: duplicate of key 0
    sks_of = {i: sks[i] for i in range(8)}
    sks_of[11] = sks[0]
    tors = grp.small_order_point(rng)
    items, nf = [], 0
    for i in range(96):
        msg = bytes(rng.getrandbits(8) for _ in range(LENGTHS[i % 16]))
        cls = "valid"
        if i % 2:
            cls = FAULTS[nf % len(FAULTS)]
            nf += 1
        kidx = 11 if cls == "valid" and i % 24 == 0 else rng.randrange(8)
        signed_kidx, signed_msg = kidx, msg
        if cls == "wrong_key":
            signed_kidx = (kidx + 1 + rng.randrange(7)) % 8
        elif cls == "wrong_msg":
            signed_msg = msg[:-1] + bytes([msg[-1] ^ 1]) if msg else b"\0"  # last bit flipped (empty: one zero byte)
        elif cls == "wrong_msg_len":
            signed_msg = msg + b"\0"
        sig = bytearray(sign(grp, sks_of[signed_kidx], keys[signed_kidx], signed_msg, rng))
        s = int.from_bytes(sig[K:], "big")
        if cls == "s_plus_1":
            sig[K:] = ((s + 1) % B.R).to_bytes(32, "big")
        elif cls == "s_plus_r":
            sig[K:] = (s + B.R).to_bytes(32, "big")
        elif cls == "s_zero":
            sig[K:] = bytes(32)
        elif cls == "r_negated":
            sig[0] ^= 0x20
        elif cls == "r_x_bit":
            sig[K - 1 - rng.randrange(8)] ^= 1 << rng.randrange(8)
        elif cls == "r_flag":
            which = nf % 3
            if which == 0:
                sig[0] &= 0x7F                      # the uncompressed form's flag
            elif which == 1:
                sig[0] |= 0x40                      # infinity flag on a nonzero x
            else:
                sig[:K] = grp.compress(None)        # the point at infinity itself
        elif cls == "r_torsion":
            rp = grp.decompress(bytes(sig[:K]), False)
            sig[:K] = grp.compress(grp.add(rp, tors))
        elif cls == "key_undecodable":
            kidx = 8
        elif cls == "key_not_in_subgroup":
            kidx = 9
        elif cls == "key_infinity":
            kidx = 10
        items.append({"class": cls, "key": kidx, "msg": msg, "sig": bytes(sig)})
    sw = [i for i, it in enumerate(items) if it["class"] == "swap"]
    assert len(sw) % 2 == 0 and len(sw) >= 2
    for a, b in zip(sw[::2], sw[1::2]):
        items[a]["sig"], items[b]["sig"] = items[b]["sig"], items[a]["sig"]
    out_items = []
    for it in items:
        v = verify(grp, keys[it["key"]], it["msg"], it["sig"])
        assert v == (1 if it["class"] == "valid" else 0), it["class"]
        out_items.append({"class": it["class"], "key": it["key"], "msg": it["msg"].hex(), "sig": it["sig"].hex(), "verdict": v})
    for cls in FAULTS:
        assert sum(1 for it in items if it["class"] == cls) >= 2, cls
    return {"scheme": grp.scheme, "key_len": K, "keys": [k.hex() for k in keys],
            "key_ok": [1 if decode_key(grp, k) is not None else 0 for k in keys], "items": out_items}


def main():
    fx = {"comment": "written by tests/golden/make_schnorr_golden.py; verdicts by the restated check of DESIGN.md "
                     "section 11 (pure Python), not by kyber",
          "groups": [make_group(False, 0x5C4E0001), make_group(True, 0x5C4E0002)]}
    path = os.path.join(HERE, "schnorr.json")
    with open(path, "w") as f:
        json.dump(fx, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
