"""One chain from three overlapping RandomData archives on one MI355X: a signed chain per signature
size (quicknet: 48-byte G1 signatures; pedersen-bls-chained: 96-byte G2 signatures with previous_signature) written as
  A  every round, 0.1% of the signatures corrupted;
  B  the upper 60% of the rounds, another 0.1% corrupted;
  C  every round but 3, in shuffled blocks of 4096 records;
and turned into one trimmed store file two ways in one run:
  (a) what the library offered before dh_assemble_device: DeviceArchive.check on each archive, the valid records merged
      by round in a Python dict and sorted on the host, then write_trimmed_bolt;
  (b) store.assemble_to_trimmed_store over the three open archives.
The two files must be byte-identical, or the run is void (it raises). Also: the sort alone against torch.sort on the same
keys, and (b)'s verify stage against a single DeviceArchive.check of archive A.
  python bench/assemble_replay.py [--rounds N] [--out OUT.json] [--schemes A,B]   (default: bench_outputs/assemble_replay.json)"""
import argparse
import ctypes
import hashlib
import json
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bench")]
import numpy as np
import torch

torch.zeros(1, device="cuda")
import chainsynth
import drand_amd
from drand_amd import _lib
from drand_amd import store
from drand_amd.store import AR_RANDOMNESS, DeviceArchive, random_data_line

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
STAGES = ["archive_upload", "archive_index", "archive_stat", "archive_gather", "archive_verify", "archive_fold", "assemble_sort",
          "assemble_class", "assemble_verify", "assemble_select", "k_sort_orand", "k_sort_pass"]
BLOCK = 4096


def secret(name):
    return (int.from_bytes(hashlib.sha256(b"drandhip-sk-" + name.encode()).digest(), "big") % R).to_bytes(32, "big")


def profile_read(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    lib.dh_profile_read(buf, len(buf))
    return json.loads(buf.value.decode())


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def build(s, sk, n, log):
    """The three archives' bytes and the chain's (rounds, sigs)."""
    rounds = np.arange(1, n + 1, dtype=np.uint64)
    genesis = hashlib.sha256(b"assemble replay genesis").digest()
    prevs = plens = None
    if s.chained:
        # signed in about n / 1000 segments side by side (chainsynth): the round after each cut was signed over a random
        # head, so it verifies in no archive and is a gap in both legs
        sigs = chainsynth.sign_chain(s, sk, 1, n, genesis, chainsynth.corrupted_rounds(n, n // 1000), np.random.default_rng(5),
                                     progress=lambda p, q: log("  signing step %d / %d" % (p, q)))
        prevs, plens = chainsynth.stored_prevs(sigs, genesis)
    else:
        sigs = s.sign_beacons(sk, rounds)

    def lines(idx, bad, seed):
        rng, bad = random.Random(seed), set(int(i) for i in bad)
        out = []
        for i in idx:
            sig = sigs[i].tobytes()
            if i in bad:
                k = rng.randrange(len(sig))
                sig = sig[:k] + bytes([sig[k] ^ (1 << rng.randrange(8))]) + sig[k + 1:]
            out.append(random_data_line({"round": int(rounds[i]), "randomness": hashlib.sha256(sig).digest(), "signature": sig,
                                         "previous_signature": prevs[i, :int(plens[i])].tobytes() if s.chained else b""}))
        return out
    pick = np.random.default_rng(77)
    lower = n - (n * 6) // 10
    a = lines(range(n), pick.choice(n, n // 1000, replace=False), 1)
    b = lines(range(lower, n), lower + pick.choice(n - lower, n // 1000, replace=False), 2)
    gone = {n // 7, n // 2, n - 5000}
    c = lines([i for i in range(n) if i not in gone], [], 3)
    blocks = [c[k:k + BLOCK] for k in range(0, len(c), BLOCK)]
    random.Random(9).shuffle(blocks)
    c = [l for blk in blocks for l in blk]
    return [b"\n".join(x) + b"\n" for x in (a, b, c)], [len(a), len(b), len(c)]


def leg_a(datas, s, pk, path, seed):
    """check per archive, a dict by round over the valid records, a host sort, write_trimmed_bolt."""
    t = {"open_s": 0.0, "check_s": 0.0, "columns_to_host_s": 0.0, "merge_s": 0.0}
    best = {}
    stride = (s.sig_len + 3) & ~3
    for data in datas:
        dt, ar = timed(lambda: DeviceArchive(data))
        t["open_s"] += dt
        dt, status = timed(lambda: ar.check(s, pk, seed=seed))
        t["check_s"] += dt
        dt, (rounds, sigs) = timed(lambda: (lambda c: (c[0].cpu().numpy().view(np.uint64), c[1].cpu().numpy()))(
            ar.beacons_device(sig_stride=stride, want_prev=False, want_rand=False)))
        t["columns_to_host_s"] += dt
        ar.close()
        t0 = time.perf_counter()
        ok = np.flatnonzero((status & ~np.uint8(AR_RANDOMNESS) & ~np.uint8(store.AR_SEQUENCE) & ~np.uint8(store.AR_LINK)) == 0)
        for i in ok.tolist():  # the per-record host work: the first valid copy of a round wins
            r = int(rounds[i])
            if r not in best:
                best[r] = sigs[i]
        t["merge_s"] += time.perf_counter() - t0
    t0 = time.perf_counter()
    order = sorted(best)
    out_rounds = np.array(order, np.uint64)
    out_sigs = np.stack([best[r] for r in order]) if order else np.zeros((0, stride), np.uint8)
    t["merge_s"] += time.perf_counter() - t0
    t["write_s"], _ = timed(lambda: store.write_trimmed_bolt(path, out_rounds, out_sigs, np.full(len(order), s.sig_len, np.uint32)))
    t["total_s"] = sum(t.values())
    return t, len(order)


def leg_b(datas, s, pk, path, seed):
    t = {"open_s": 0.0}
    ars = []
    for data in datas:
        dt, ar = timed(lambda: DeviceArchive(data))
        t["open_s"] += dt
        ars.append(ar)
    t["assemble_to_trimmed_store_s"], out = timed(lambda: store.assemble_to_trimmed_store(ars, path, s, pk, allow_gaps=True, seed=seed))
    [ar.close() for ar in ars]
    t["total_s"] = sum(t.values())
    return t, out


def sort_alone(keys):
    """dh_sort_rounds_debug (keys uploaded and the permutation downloaded inside the call; k_sort_* are its kernels) and
    torch.sort(stable) on the same keys: kernel time from dh_profile against CUDA-event time, warm best of 3."""
    lib = _lib.load()
    n = len(keys)
    perm = np.zeros(n, np.uint32)
    ours = []
    for _ in range(4):
        lib.dh_profile(1)
        assert lib.dh_sort_rounds_debug(ctypes.c_void_p(keys.ctypes.data), n, ctypes.c_void_p(perm.ctypes.data)) == 0, _lib.last_error()
        prof = profile_read(lib)
        lib.dh_profile(0)
        ours.append({"k_sort_pass_ms": prof.get("k_sort_pass", {}).get("total_ms", 0.0), "passes": prof.get("k_sort_pass", {}).get("count", 0),
                     "k_sort_orand_ms": prof.get("k_sort_orand", {}).get("total_ms", 0.0)})
    d_keys = torch.from_numpy(keys.view(np.int64)).cuda()  # rounds below 2^63: the signed order is the unsigned one
    theirs = []
    for _ in range(4):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _v, t_perm = torch.sort(d_keys, stable=True)
        b.record()
        torch.cuda.synchronize()
        theirs.append(a.elapsed_time(b))
    if not np.array_equal(perm, t_perm.cpu().numpy().astype(np.uint32)):
        raise SystemExit("VOID: the two sorts give different permutations")
    best = min(ours[1:], key=lambda r: r["k_sort_pass_ms"] + r["k_sort_orand_ms"])
    return {"keys": n, "ours_warm_best_of_3": best, "torch_sort_ms_warm_best_of_3": min(theirs[1:]),
            "ours_over_torch": (best["k_sort_pass_ms"] + best["k_sort_orand_ms"]) / min(theirs[1:])}


def measure(name, n, log):
    lib = _lib.load()
    s = drand_amd.scheme_from_name(name)
    sk = secret(name)
    pk = s.public_key(sk)
    log("%s: building %d rounds" % (name, n))
    datas, counts = build(s, sk, n, log)
    res = {"rounds_signed": n, "records": counts, "archive_bytes": [len(d) for d in datas]}
    seed = 9
    tmp = tempfile.mkdtemp(prefix="assemble_replay_")
    pa, pb = os.path.join(tmp, "a.db"), os.path.join(tmp, "b.db")
    runs_a, runs_b = [], []
    for rep in range(3):  # one cold pair, then warm pairs, alternating
        for leg, runs, path in ((leg_a, runs_a, pa), (leg_b, runs_b, pb)):
            lib.dh_profile(1)
            t, out = leg(datas, s, pk, path, seed)
            prof = profile_read(lib)
            lib.dh_profile(0)
            t["stages_ms"] = {k: prof[k]["total_ms"] for k in STAGES if k in prof}
            t["stage_calls"] = {k: prof[k]["count"] for k in STAGES if k in prof}
            if leg is leg_b:
                t["counts"], t["gaps"] = out["assembled"].counts, out["assembled"].gaps[:8]
            else:
                t["rows"] = out
            runs.append(t)
            log("  (%s) rep %d: %s" % ("a" if leg is leg_a else "b", rep, json.dumps({k: v for k, v in t.items() if k.endswith("_s")})))
        if open(pa, "rb").read() != open(pb, "rb").read():
            raise SystemExit("VOID: the two store files differ")
    res["files_identical"] = True
    res["store_bytes"] = os.path.getsize(pb)
    wa, wb = min(runs_a[1:], key=lambda r: r["total_s"]), min(runs_b[1:], key=lambda r: r["total_s"])
    res["a_check_merge_write"] = {"cold": runs_a[0], "warm_best_of_2": wa}
    res["b_assemble_to_trimmed_store"] = {"cold": runs_b[0], "warm_best_of_2": wb}
    res["b_over_a_speedup"] = wa["total_s"] / wb["total_s"]
    # (b)'s verify stage against one check of the complete archive (about as many distinct records)
    single = []
    for rep in range(3):
        ar = DeviceArchive(datas[0])
        lib.dh_profile(1)
        dt, _st = timed(lambda: ar.check(s, pk, seed=seed))
        prof = profile_read(lib)
        lib.dh_profile(0)
        ar.close()
        single.append({"check_s": dt, "archive_verify_ms": prof["archive_verify"]["total_ms"]})
    one = min(single[1:], key=lambda r: r["archive_verify_ms"])
    st = wb["stages_ms"]
    around = st.get("assemble_sort", 0) + st.get("assemble_class", 0) + st.get("assemble_select", 0)
    res["single_check_of_A"] = one
    res["verify_stage_over_single_check"] = st.get("assemble_verify", 0) / one["archive_verify_ms"]
    res["sort_class_select_over_verify"] = around / st["assemble_verify"] if st.get("assemble_verify") else None
    keys = np.concatenate([np.arange(1, n + 1, dtype=np.uint64), np.arange(n - (n * 6) // 10 + 1, n + 1, dtype=np.uint64),
                           np.random.default_rng(3).permutation(np.arange(1, n + 1, dtype=np.uint64))])
    res["sort_alone"] = sort_alone(np.ascontiguousarray(keys))
    for p in (pa, pb):
        os.remove(p)
    os.rmdir(tmp)
    log("  %s" % json.dumps({k: v for k, v in res.items() if not isinstance(v, (dict, list))}))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "assemble_replay.json"))
    ap.add_argument("--schemes", default="bls-unchained-g1-rfc9380,pedersen-bls-chained")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    assert _lib.load().dh_init(0) == 0, _lib.last_error()

    def log(msg):
        print(msg, flush=True)

    res = {"device": torch.cuda.get_device_name(0), "version": _lib.load().dh_version().decode(), "schemes": {}}
    for name in a.schemes.split(","):
        res["schemes"][name] = measure(name, a.rounds, log)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({"assemble_replay": a.out, "speedup": {k: v.get("b_over_a_speedup") for k, v in res["schemes"].items()}}))


if __name__ == "__main__":
    main()
