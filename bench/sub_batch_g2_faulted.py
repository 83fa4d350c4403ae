#!/usr/bin/env python3
"""pedersen-bls-unchained rounds with 0.1% sigma + T13a (an order-13 point of E'(Fp2) outside G2), 8 batches in flight:
what the batched G2 subgroup test's fallback and its back-off cost. One JSON line; the first argument is
a label for it, the second the batch size (default 262,144 rounds, below the default minimum: set
DRANDHIP_SUB_BATCH_MIN_G2 to put it on the batched path).

    DRANDHIP_SUB_BATCH_MIN_G2=1 python bench/sub_batch_g2_faulted.py backoff
    DRANDHIP_SUB_BATCH_MIN_G2=1 DRANDHIP_SUB_BACKOFF=0 python bench/sub_batch_g2_faulted.py no_backoff
    DRANDHIP_SUBGROUP_BATCH=0 python bench/sub_batch_g2_faulted.py fused
"""
import ctypes, hashlib, json, os, sys, threading, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
os.environ["GPU_MAX_HW_QUEUES"] = "16"
import torch
import bls_py as b
from drand_amd import _lib, scheme_from_name
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
U = -b.U_ABS
H2 = (U ** 8 - 4 * U ** 7 + 5 * U ** 6 - 4 * U ** 4 + 6 * U ** 3 - 4 * U ** 2 - 4 * U + 13) // 9


def t13a():
    """(psi - 7) S for S of order 13: psi = 11 = -2 on it"""
    cx, cy = b.f2inv(b.f2pow((1, 1), (b.P - 1) // 3)), b.f2inv(b.f2pow((1, 1), (b.P - 1) // 2))
    x = (5, 1)
    while True:
        y = b.f2sqrt(b.f2add(b.f2mul(b.f2mul(x, x), x), b.B2))
        if y is not None:
            break
        x = (x[0] + 1, x[1])
    s = b.ec_mul(b.FP2, (x, y), R * H2 // 169)
    if b.ec_mul(b.FP2, s, 13) is not None:
        s = b.ec_mul(b.FP2, s, 13)
    psi_s = (b.f2mul(b.f2conj(s[0]), cx), b.f2mul(b.f2conj(s[1]), cy))
    t = b.ec_add(b.FP2, psi_s, b.ec_neg(b.FP2, b.ec_mul(b.FP2, s, 7)))
    assert t is not None and b.ec_mul(b.FP2, t, 13) is None
    return t


lib = _lib.load()
torch.zeros(1, device="cuda")
assert lib.dh_init(1) == 0
s = scheme_from_name("pedersen-bls-unchained")
sk = (int.from_bytes(hashlib.sha256(b"faulted").digest(), "big") % R).to_bytes(32, "big")
pk = s.public_key(sk)
n, S, steps = (int(sys.argv[2]) if len(sys.argv) > 2 else 262144), 8, 32
rounds = np.arange(1, n + 1, dtype=np.uint64)
sigs = s.sign_beacons(sk, rounds)
bad = np.sort(np.random.default_rng(5).choice(n, n // 1000, replace=False))
T = t13a()
for i in bad:
    p = b.g2_decompress(sigs[i].tobytes(), subgroup_check=False)
    sigs[i] = np.frombuffer(b.g2_compress(b.ec_add(b.FP2, p, T)), np.uint8)
dev = torch.device("cuda", 0)
d_r = torch.from_numpy(rounds.view(np.int64)).to(dev); d_s = torch.from_numpy(sigs).to(dev)
d_v = [torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(S)]
d_rand = [torch.zeros((n, 32), dtype=torch.uint8, device=dev) for _ in range(S)]
def one(t):
    rc = lib.dh_verify_batch_device(s.id, pk, len(pk), ctypes.c_void_p(d_r.data_ptr()), ctypes.c_void_p(d_s.data_ptr()), 96,
                                    None, 0, None, n, ctypes.c_void_p(d_v[t].data_ptr()), ctypes.c_void_p(d_rand[t].data_ptr()), 0, None, None)
    assert rc == 0, _lib.last_error()
def run(k):
    ths = [threading.Thread(target=lambda t=t: [one(t) for _ in range(t, k, S)]) for t in range(S)]
    t0 = time.perf_counter()
    for th in ths: th.start()
    for th in ths: th.join()
    torch.cuda.synchronize()
    return time.perf_counter() - t0
run(2 * S)
lib.dh_profile(1)
el = run(steps)
buf = ctypes.create_string_buffer(1 << 16); lib.dh_profile_read(buf, len(buf)); lib.dh_profile(0)
prof = {k: {"count": v["count"], "ms_per_batch": round(v["total_ms"] / steps, 3)} for k, v in json.loads(buf.value.decode()).items()}
v = d_v[0].cpu().numpy()
rej = np.flatnonzero(v == 0)
print(json.dumps({"what": "pedersen-bls-unchained %d rounds, 0.1%% sigma + T13a, %d in flight" % (n, S), "lib": sys.argv[1], "steps": steps,
                  "ms_per_batch": round(1000 * el / steps, 3), "beacons_per_s": round(n * steps / el, 1),
                  "rejected": int(len(rej)), "rejected_equals_corrupted": bool(np.array_equal(rej, bad)), "corrupted": int(len(bad)),
                  "stages": prof}))
