#!/usr/bin/env python3
"""One-call time of a clean pedersen-bls-unchained batch around the batched G2 subgroup test's minimum size (DESIGN
§14): one stream, device inputs, median of 15 calls per size, one JSON line per size with the stage times of one more
call. The mode is a label; the library reads its switches once per process, so run it twice:

    DRANDHIP_SUB_BATCH_MIN_G2=1 python bench/sub_batch_g2_sweep.py batched
    DRANDHIP_SUBGROUP_BATCH=0 python bench/sub_batch_g2_sweep.py fused
"""
import ctypes, hashlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from drand_amd import _lib, scheme_from_name
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
lib = _lib.load()
torch.zeros(1, device="cuda")
assert lib.dh_init(1) == 0
s = scheme_from_name("pedersen-bls-unchained")
sk = (int.from_bytes(hashlib.sha256(b"sweep").digest(), "big") % R).to_bytes(32, "big")
pk = s.public_key(sk)
mode = sys.argv[1]
sizes = [int(a) for a in sys.argv[2:]] or [4096, 16384, 65536, 131072, 262144, 1048576]
dev = torch.device("cuda", 0)
for n in sizes:
    rounds = np.arange(1, n + 1, dtype=np.uint64)
    sigs = s.sign_beacons(sk, rounds)
    d_r = torch.from_numpy(rounds.view(np.int64)).to(dev)
    d_s = torch.from_numpy(sigs).to(dev)
    d_v = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_rand = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    def one():
        rc = lib.dh_verify_batch_device(s.id, pk, len(pk), ctypes.c_void_p(d_r.data_ptr()), ctypes.c_void_p(d_s.data_ptr()), 96,
                                        None, 0, None, n, ctypes.c_void_p(d_v.data_ptr()), ctypes.c_void_p(d_rand.data_ptr()), 0, None, None)
        assert rc == 0, _lib.last_error()
    for _ in range(3):
        one()
    ts = []
    for _ in range(15):
        t0 = time.perf_counter(); one(); ts.append(time.perf_counter() - t0)
    lib.dh_profile(1); one()
    buf = ctypes.create_string_buffer(1 << 16); lib.dh_profile_read(buf, len(buf)); lib.dh_profile(0)
    prof = {k: round(v["total_ms"], 3) for k, v in json.loads(buf.value.decode()).items()}
    assert bool(d_v.cpu().numpy().all())
    print(json.dumps({"mode": mode, "n": n, "ms_per_call_median": round(1000 * float(np.median(ts)), 3),
                      "ms_per_call_min": round(1000 * min(ts), 3), "stages_ms": prof}), flush=True)
