"""Measurements of dh_bls_verify_batch on one MI355X (recorded in profiles/r07/auth_measure.json): the
items-per-key crossover T (per-item leaf checks against the combined check at n = 4096), the single-key call
against dh_verify_recovered_batch with the stage times of both, and the hash stage times.
  python bench/auth_measure.py [OUT.json]   (default: bench_outputs/auth_measure.json)"""
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
import drand_amd
from drand_amd import _lib

lib = _lib.load()
assert lib.dh_init(0) == 0
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "bench_outputs", "auth_measure.json")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
res = {"crossover": {}, "single_key": {}, "single_key_stage_ms": {}, "hash": {}}


def sk(i):
    return (int.from_bytes(hashlib.sha256(b"measure-%d" % i).digest(), "big") % R).to_bytes(32, "big")


def digests(rounds):
    return np.frombuffer(b"".join(hashlib.sha256(int(r).to_bytes(8, "big")).digest() for r in rounds), np.uint8).copy()


def call(s, ktab, n_keys, kidx, msgs, off, sigs, n, path, stats=None):
    if path:
        os.environ["DRANDHIP_AUTH_PATH"] = path
    else:
        os.environ.pop("DRANDHIP_AUTH_PATH", None)
    verdict = np.zeros(n, np.uint8)
    t = time.perf_counter()
    rc = lib.dh_bls_verify_batch(s.id, ktab.ctypes.data, n_keys, kidx.ctypes.data, msgs.ctypes.data, off.ctypes.data,
                                 sigs.ctypes.data, s.sig_len, n, verdict.ctypes.data, None, 0,
                                 stats.ctypes.data if stats is not None else None)
    dt = time.perf_counter() - t
    assert rc == 0, _lib.last_error()
    return dt * 1e3, verdict


def median_ms(fn, reps=7):
    fn()
    fn()
    return statistics.median(fn() for _ in range(reps))


def save():
    json.dump(res, open(OUT, "w"), indent=1)


# ---- 1. crossover: n = 4096, 32-byte messages, by number of keys
N = 4096
for name in ("bls-unchained-g1-rfc9380", "pedersen-bls-unchained"):
    s = drand_amd.scheme_from_name(name)
    rounds = np.arange(1, N + 1, dtype=np.uint64)
    msgs = digests(rounds)
    off = (np.arange(N + 1, dtype=np.uint32) * 32)
    res["crossover"][name] = {}
    for nk in (1, 8, 64, 512, 1024, 2048, 4096):
        per = N // nk
        keys, sigs = [], np.zeros((N, s.sig_len), np.uint8)
        for k in range(nk):
            keys.append(s.public_key(sk(k)))
            sigs[k * per:(k + 1) * per] = s.sign_beacons(sk(k), rounds[k * per:(k + 1) * per])
        ktab = np.frombuffer(b"".join(keys), np.uint8).copy()
        kidx = (np.arange(N, dtype=np.uint32) // per).astype(np.uint32)
        row = {}
        for path in ("leaf", "rlc"):
            stats = np.zeros(4, np.uint64)
            _, v = call(s, ktab, nk, kidx, msgs, off, sigs, N, path, stats)
            assert v.all(), (name, nk, path)
            row[path + "_ms"] = round(median_ms(lambda: call(s, ktab, nk, kidx, msgs, off, sigs, N, path)[0]), 3)
            row[path + "_stats"] = [int(x) for x in stats]
        res["crossover"][name][str(nk)] = row
        print(name, nk, row, flush=True)
        save()

# ---- 2. single key, n = 131072: the new entry against dh_verify_recovered_batch, same inputs, same process
N = 131072
big = {}
for name in ("bls-unchained-g1-rfc9380", "pedersen-bls-unchained"):
    s = drand_amd.scheme_from_name(name)
    rounds = np.arange(1, N + 1, dtype=np.uint64)
    msgs = digests(rounds)
    off = (np.arange(N + 1, dtype=np.uint32) * 32)
    key = s.public_key(sk(0))
    sigs = s.sign_beacons(sk(0), rounds)
    ktab = np.frombuffer(key, np.uint8).copy()
    kidx = np.zeros(N, np.uint32)
    big[name] = (s, msgs, off, ktab, kidx, sigs)
    verdict = np.zeros(N, np.uint8)

    def old():
        t = time.perf_counter()
        rc = lib.dh_verify_recovered_batch(s.id, key, len(key), msgs.ctypes.data, sigs.ctypes.data, s.sig_len, N,
                                           verdict.ctypes.data, 0)
        dt = time.perf_counter() - t
        assert rc == 0 and verdict.all()
        return dt * 1e3

    def new():
        dt, v = call(s, ktab, 1, kidx, msgs, off, sigs, N, None)
        assert v.all()
        return dt

    a = [old(), new()]  # warm both
    olds, news = [], []
    for _ in range(7):  # alternating
        olds.append(old())
        news.append(new())
    mo, mn = statistics.median(olds), statistics.median(news)
    res["single_key"][name] = {"n": N, "verify_recovered_batch_ms": round(mo, 3), "bls_verify_batch_ms": round(mn, 3),
                               "ratio": round(mn / mo, 4), "old_all": [round(x, 2) for x in olds],
                               "new_all": [round(x, 2) for x in news]}
    print(name, res["single_key"][name], flush=True)
    res["single_key_stage_ms"][name] = {}
    for tag, fn in (("verify_recovered_batch", old), ("bls_verify_batch", new)):
        lib.dh_profile(1)
        for _ in range(3):
            fn()
        buf = ctypes.create_string_buffer(1 << 16)
        lib.dh_profile_read(buf, len(buf))
        lib.dh_profile(0)
        prof = json.loads(buf.value.decode())
        res["single_key_stage_ms"][name][tag] = {k: round(v["total_ms"] / 3, 4) for k, v in prof.items()}
    save()

# ---- 3. hash stage times at n = 131072 (dh_profile): the fixed 32-byte kernels; the variable-length kernels on
# 32-byte messages (the last message is 33 bytes, signed by the oracle, which takes the call off the fixed-shape
# route) and on 200-byte messages (signatures of other messages: the check fails and every item gets its leaf,
# which the hash stage's time does not depend on).
import oracle_ctypes as orc
for name, (s, msgs, off, ktab, kidx, sigs) in big.items():
    out = {}
    m33 = np.concatenate([msgs, np.zeros(1, np.uint8)])
    o33 = off.copy()
    o33[-1] += 1
    s33 = sigs.copy()
    s33[-1] = np.frombuffer(orc.sign(name, sk(0), m33[-33:].tobytes()), np.uint8)
    m200 = np.random.default_rng(1).integers(0, 256, 200 * N, dtype=np.uint8)
    shapes = {"fixed32": (msgs, off, sigs, True), "var32": (m33, o33, s33, True),
              "var200": (m200, np.arange(N + 1, dtype=np.uint32) * 200, sigs, False)}
    for tag, (m, o, sg, valid) in shapes.items():
        _, v = call(s, ktab, 1, kidx, m, o, sg, N, "rlc")  # warm
        assert bool(v.all()) == valid and (valid or not v.any()), (name, tag)
        lib.dh_profile(1)
        for _ in range(3):
            call(s, ktab, 1, kidx, m, o, sg, N, "rlc")
        buf = ctypes.create_string_buffer(1 << 16)
        lib.dh_profile_read(buf, len(buf))
        lib.dh_profile(0)
        prof = json.loads(buf.value.decode())
        out[tag] = {k: round(v["total_ms"] / v["count"], 4) for k, v in prof.items() if "k_prep_msg" in k}
    res["hash"][name] = out
    print(name, out, flush=True)
    save()
print("done")
