"""Measurements of dh_schnorr_verify_batch on one MI355X (recorded in profiles/r07/schnorr_measure.json):
medians of 7 warm host calls at n = 64, 512 and 4,096 items with 32-byte messages (the size of group.Hash()), under
1 key, 8 keys and one key per item, for both key groups, on the default path (the joint chain over tables) and on
DRANDHIP_SCHNORR_PATH=plain (two jac_mul_words per item, the yardstick), alternating in one process, with the
dh_profile stage times of each.
  python bench/schnorr_measure.py [OUT.json]   (default: bench_outputs/schnorr_measure.json)
Signatures are made on the host: keys x_0 + i and nonces k_0 + i, their points by repeated addition of the generator
to one device-computed point each (oracle/bls_py.py), so every key and every R is distinct."""
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import numpy as np
import torch

torch.zeros(1, device="cuda")
import bls_py as B
import drand_amd
from drand_amd import _lib

lib = _lib.load()
assert lib.dh_init(0) == 0
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "bench_outputs", "schnorr_measure.json")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
NMAX = 4096
res = {"sizes": [64, 512, NMAX], "message_bytes": 32, "reps": 7, "groups": {}}


def scalar(tag):
    return int.from_bytes(hashlib.sha256(tag).digest(), "big") % B.R


def chain(s, g2, x0, count):
    """compressed [x0 + i] G for i < count: one device multiplication, then additions of G on the host"""
    F, gen = (B.FP2, B.G2_GEN) if g2 else (B.FP, B.G1_GEN)
    dec, comp = (B.g2_decompress, B.g2_compress) if g2 else (B.g1_decompress, B.g1_compress)
    pt = dec(s.public_key(x0.to_bytes(32, "big")), False)
    out = []
    for _ in range(count):
        out.append(comp(pt))
        pt = B.ec_add(F, pt, gen)
    return out


def call(s, ktab, n_keys, kidx, msgs, off, sigs, n, plain):
    if plain:
        os.environ["DRANDHIP_SCHNORR_PATH"] = "plain"
    else:
        os.environ.pop("DRANDHIP_SCHNORR_PATH", None)
    verdict = np.zeros(n, np.uint8)
    t = time.perf_counter()
    rc = lib.dh_schnorr_verify_batch(s.id, ktab.ctypes.data, n_keys, kidx.ctypes.data, msgs.ctypes.data, off.ctypes.data,
                                     sigs.ctypes.data, s.schnorr_sig_len, n, verdict.ctypes.data, None)
    dt = time.perf_counter() - t
    assert rc == 0, _lib.last_error()
    assert verdict.all(), "a valid signature was rejected"
    return dt * 1e3


def stages(fn, reps=3):
    lib.dh_profile(1)
    for _ in range(reps):
        fn()
    buf = ctypes.create_string_buffer(1 << 16)
    lib.dh_profile_read(buf, len(buf))
    lib.dh_profile(0)
    return {k: round(v["total_ms"] / v["count"], 4) for k, v in json.loads(buf.value.decode()).items()}


for name in ("pedersen-bls-unchained", "bls-unchained-g1-rfc9380"):
    s = drand_amd.scheme_from_name(name)
    g2 = s.key_len == 96
    x0, k0 = scalar(b"schnorr-measure-key-" + name.encode()), scalar(b"schnorr-measure-nonce-" + name.encode())
    keys, rs = chain(s, g2, x0, NMAX), chain(s, g2, k0, NMAX)
    msgs = np.frombuffer(b"".join(hashlib.sha256(b"group-%d" % i).digest() for i in range(NMAX)), np.uint8).copy()
    out = res["groups"][name] = {"key_group": "G2" if g2 else "G1"}
    for n in res["sizes"]:
        off = np.arange(n + 1, dtype=np.uint32) * 32
        for nk in (1, 8, n):
            kidx = (np.arange(n, dtype=np.uint32) % nk).astype(np.uint32)
            sigs = np.zeros((n, s.schnorr_sig_len), np.uint8)
            for i in range(n):
                k = int(kidx[i])
                h = int.from_bytes(hashlib.sha512(rs[i] + keys[k] + msgs[32 * i:32 * i + 32].tobytes()).digest(), "big") % B.R
                sigs[i] = np.frombuffer(rs[i] + ((k0 + i + h * (x0 + k)) % B.R).to_bytes(32, "big"), np.uint8)
            ktab = np.frombuffer(b"".join(keys[:nk]), np.uint8).copy()
            run = lambda plain: call(s, ktab, nk, kidx, msgs, off, sigs, n, plain)  # noqa: E731
            for _ in range(2):  # warm both
                run(False), run(True)
            joint, plain = [], []
            for _ in range(res["reps"]):  # alternating
                joint.append(run(False))
                plain.append(run(True))
            mj, mp = statistics.median(joint), statistics.median(plain)
            row = {"joint_ms": round(mj, 3), "plain_ms": round(mp, 3), "plain_over_joint": round(mp / mj, 3),
                   "joint_all": [round(x, 3) for x in joint], "plain_all": [round(x, 3) for x in plain],
                   "joint_stage_ms": stages(lambda: run(False)), "plain_stage_ms": stages(lambda: run(True))}
            out["n=%d keys=%s" % (n, "n" if nk == n and n > 8 else nk)] = row
            print(name, n, nk, {k: v for k, v in row.items() if not k.endswith("_all")}, flush=True)
            json.dump(res, open(OUT, "w"), indent=1)
print("done")
