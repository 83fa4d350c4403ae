"""Verifying a client.RandomData JSON-lines archive end to end on one MI355X (recorded in
profiles/r20/archive_replay.json): a 1,048,576-record signed archive per signature size (quicknet: 48-byte G1
signatures; pedersen-bls-chained: 96-byte G2 signatures with previous_signature), written with random_data_line, 0.1%
of the records corrupted and 3 removed, two ways in one run:
  (a) the host reader: read_random_data + random_data_columns + verify_beacons (one repetition);
  (b) the device reader: DeviceArchive(bytes).check, cold once, then warm best of 3, split by dh_profile stages.
(a) and (b) must mark the same records invalid, or the run is void (it raises).
  python bench/archive_replay.py [--rounds N] [--out OUT.json] [--schemes A,B]   (default: bench_outputs/archive_replay.json)"""
import argparse
import ctypes
import hashlib
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bench")]
import numpy as np
import torch

torch.zeros(1, device="cuda")
import chainsynth
import g1_synth
import drand_amd
from drand_amd import _lib
from drand_amd.store import AR_INVALID, DeviceArchive, random_data_columns, random_data_line, read_random_data

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
STAGES = ["archive_upload", "archive_index", "archive_stat", "archive_gather", "archive_verify", "archive_fold", "k_ndjson_gather"]
K_BOLT_GATHER_GBPS = 2300.0  # k_bolt_gather on a 48-byte trimmed store


def secret(name):
    return (int.from_bytes(hashlib.sha256(b"drandhip-sk-" + name.encode()).digest(), "big") % R).to_bytes(32, "big")


def profile_read(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    lib.dh_profile_read(buf, len(buf))
    return json.loads(buf.value.decode())


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def build(s, sk, n, log):
    """Sign rounds 1..n, corrupt 0.1%, drop 3 records; the archive's bytes, one random_data_line per record."""
    rounds = np.arange(1, n + 1, dtype=np.uint64)
    bad = chainsynth.corrupted_rounds(n, n // 1000)
    genesis = hashlib.sha256(b"archive replay genesis").digest()
    prevs = plens = None
    if s.chained:
        sigs = chainsynth.sign_chain(s, sk, 1, n, genesis, bad, np.random.default_rng(5),
                                     progress=lambda p, q: log("  signing step %d / %d" % (p, q)) if p % 500 == 0 else None)
        chainsynth.corrupt(sigs, bad, random.Random(31))
        prevs, plens = chainsynth.stored_prevs(sigs, genesis)
    else:
        sigs = s.sign_beacons(sk, rounds)
        g1_synth.corrupt(sigs, bad, random.Random(41))
    keep = np.ones(n, bool)
    keep[[n // 7, n // 2, n - 5000]] = False
    lines = []
    for i in np.flatnonzero(keep).tolist():
        sig = sigs[i].tobytes()
        lines.append(random_data_line({"round": int(rounds[i]), "randomness": hashlib.sha256(sig).digest(), "signature": sig,
                                       "previous_signature": prevs[i, :int(plens[i])].tobytes() if s.chained else b""}))
    return b"\n".join(lines) + b"\n", len(lines)


def measure(name, n, log):
    lib = _lib.load()
    s = drand_amd.scheme_from_name(name)
    sk = secret(name)
    pk = s.public_key(sk)
    log("%s: building %d rounds" % (name, n))
    data, nrec = build(s, sk, n, log)
    res = {"rounds_signed": n, "records": nrec, "archive_bytes": len(data)}
    seed = 9
    runs = []
    for rep in range(4):  # one cold call (code objects, first allocations), then warm repetitions
        lib.dh_profile(1)
        t_open, ar = timed(lambda: DeviceArchive(data))
        t_check, st_b = timed(lambda: ar.check(s, pk, seed=seed))
        prof = profile_read(lib)
        lib.dh_profile(0)
        res["stat"] = ar.stat()
        ar.close()
        runs.append({"open_s": t_open, "check_s": t_check, "total_s": t_open + t_check,
                     "stages_ms": {k: prof[k]["total_ms"] for k in STAGES if k in prof},
                     "stage_calls": {k: prof[k]["count"] for k in STAGES if k in prof}})
        log("  (b) rep %d: open %.3f s, check %.3f s, stages %s" % (rep, t_open, t_check, runs[-1]["stages_ms"]))
    warm = min(runs[1:], key=lambda r: r["total_s"])
    marked_b = np.flatnonzero(st_b & AR_INVALID)
    res["b_device_reader"] = {"cold": runs[0], "warm_best_of_3": warm, "invalid": int(len(marked_b)),
                              "status_histogram": {str(int(k)): int(v) for k, v in zip(*np.unique(st_b, return_counts=True))}}
    # (a) the host reader, all code of the parent commit
    text = data.decode()
    t_read, recs = timed(lambda: read_random_data(text))
    t_cols, (rounds, sigs, prevs, _rand) = timed(lambda: random_data_columns(recs, s.sig_len))
    t_ver, (ok, _) = timed(lambda: s.verify_beacons(pk, rounds, sigs, prevs if s.chained else None, seed=seed, want_randomness=False))
    bad_len = np.array([len(r["signature"]) != s.sig_len for r in recs])
    marked_a = np.flatnonzero(bad_len | ~np.asarray(ok, bool))
    res["a_host_reader"] = {"read_random_data_s": t_read, "random_data_columns_s": t_cols, "verify_beacons_s": t_ver,
                            "total_s": t_read + t_cols + t_ver, "invalid": int(len(marked_a))}
    log("  (a) read %.2f s, columns %.2f s, verify %.3f s" % (t_read, t_cols, t_ver))
    if len(st_b) != len(recs) or not np.array_equal(marked_a, marked_b):
        raise SystemExit("VOID: the host and the device reader mark different records (%d vs %d)" % (len(marked_a), len(marked_b)))
    res["equal_marked_records"] = True
    res["b_over_a_speedup"] = res["a_host_reader"]["total_s"] / warm["total_s"]
    st = warm["stages_ms"]
    ingest = sum(st.get(k, 0) for k in ("archive_upload", "archive_index", "archive_stat", "archive_gather"))
    res["ingest_ms"], res["verify_ms"], res["fold_ms"] = ingest, st.get("archive_verify", 0), st.get("archive_fold", 0)
    res["ingest_share_of_b"] = ingest / (1000 * warm["total_s"])
    # the gather reads the archive once and writes rounds, lens, flags and the rows
    stride = (max(s.sig_len, res["stat"]["longest_signature"], res["stat"]["longest_previous"] if s.chained else 0) + 3) & ~3
    moved = len(data) + nrec * (8 + 4 + 1 + stride + 32 + 4 + ((stride + 4) if s.chained else 0))
    g_ms = st.get("k_ndjson_gather")
    res["gather"] = {"bytes_read_plus_written": moved, "kernel_ms": g_ms, "GBps": moved / g_ms / 1e6 if g_ms else None,
                     "k_bolt_gather_GBps": K_BOLT_GATHER_GBPS}
    res["records_per_s_b"] = nrec / warm["total_s"]
    log("  %s" % json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "archive_replay.json"))
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
    print(json.dumps({"archive_replay": a.out, "speedup": {k: v.get("b_over_a_speedup") for k, v in res["schemes"].items()}}))


if __name__ == "__main__":
    main()
