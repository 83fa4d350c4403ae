#!/usr/bin/env python3
"""262,144 quicknet rounds, 0.1% corrupted (sigma + T3 and a flipped bit in turn), 8 batches in flight: what the batched
subgroup test's fallback and its back-off cost. One JSON line; the argument is a label for it.

    python bench/sub_batch_faulted.py new
    DRANDHIP_SUB_BACKOFF=0 python bench/sub_batch_faulted.py no_backoff
    DRANDHIP_SUBGROUP_BATCH=0 python bench/sub_batch_faulted.py fused
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
lib = _lib.load()
torch.zeros(1, device="cuda")
assert lib.dh_init(1) == 0
s = scheme_from_name("bls-unchained-g1-rfc9380")
sk = (int.from_bytes(hashlib.sha256(b"faulted").digest(), "big") % R).to_bytes(32, "big")
pk = s.public_key(sk)
n, S, steps = 262144, 8, 32
rounds = np.arange(1, n + 1, dtype=np.uint64)
sigs = s.sign_beacons(sk, rounds)
bad = np.sort(np.random.default_rng(5).choice(n, n // 1000, replace=False))
for k, i in enumerate(bad):
    if k % 2 == 0:
        p = b.g1_decompress(sigs[i].tobytes(), subgroup_check=False)
        sigs[i] = np.frombuffer(b.g1_compress(b.ec_add(b.FP, p, (0, 2))), np.uint8)
    else:
        sigs[i, 30] ^= 4
dev = torch.device("cuda", 0)
d_r = torch.from_numpy(rounds.view(np.int64)).to(dev); d_s = torch.from_numpy(sigs).to(dev)
d_v = [torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(S)]
d_rand = [torch.zeros((n, 32), dtype=torch.uint8, device=dev) for _ in range(S)]
def one(t):
    rc = lib.dh_verify_batch_device(s.id, pk, len(pk), ctypes.c_void_p(d_r.data_ptr()), ctypes.c_void_p(d_s.data_ptr()), 48,
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
print(json.dumps({"what": "quicknet 262144 rounds, 0.1%% corrupted, %d in flight" % S, "lib": sys.argv[1], "steps": steps,
                  "ms_per_batch": round(1000 * el / steps, 3), "beacons_per_s": round(n * steps / el, 1),
                  "rejected": int(len(rej)), "rejected_subset_of_corrupted": bool(np.isin(rej, bad).all()), "corrupted": int(len(bad)),
                  "stages": prof}))
