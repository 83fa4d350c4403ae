"""End-to-end chain replay from a trimmed bbolt store file on one MI355X (recorded in
profiles/r10/store_replay.json): CheckPastBeacons over a 1,048,576-round quicknet store and a pedersen-bls-chained
one (4 KiB pages, 0.1% of the records corrupted, 3 records removed), four ways in one run:
  (a) the host reader: check_past_beacons(BoltTrimmedStore(path)) with the device verifying (one repetition);
  (b) the device reader: check_past_beacons(DeviceBoltStore(path)), split by dh_profile stages;
  (c) verify_beacons on the pre-built arrays: the floor;
  (d) a device-to-device copy moving the bytes the gather reads plus writes.
(a) and (b) must return equal faulty sets, or the run is void (it raises).
  python bench/store_replay.py [--rounds N] [--out OUT.json] [--skip-host]   (default: bench_outputs/store_replay.json)
--format untrimmed (recorded in profiles/r13/store_replay_untrimmed.json): the same chained chain in the
legacy hexjson layout, every record storing its PreviousSig: (a) check_past_beacons(BoltUntrimmedStore(path)), (b) the
device reader DeviceBoltStore(path, fmt="untrimmed"), (c) verify_beacons on the arrays; void unless (a) and (b) agree."""
import argparse
import ctypes
import hashlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "bench")]
import numpy as np
import torch

torch.zeros(1, device="cuda")
import chainsynth
import g1_synth
import drand_amd
from boltwrite2 import write_bolt2
from drand_amd import _lib
from drand_amd.store import BoltTrimmedStore, BoltUntrimmedStore, DeviceBoltStore
from drand_amd.sync import check_past_beacons

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
STAGES = ["store_index", "store_upload", "store_scan", "store_gather_link", "store_verify", "k_bolt_gather", "k_bolt_gather_json"]


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


def build(s, sk, n, path, log):
    """Sign rounds 1..n, corrupt 0.1%, drop 3 records, write the store. Returns the kept arrays."""
    rounds = np.arange(1, n + 1, dtype=np.uint64)
    bad = chainsynth.corrupted_rounds(n, n // 1000)
    genesis = hashlib.sha256(b"store replay genesis").digest()
    if s.chained:
        sigs = chainsynth.sign_chain(s, sk, 1, n, genesis, bad, np.random.default_rng(5),
                                     progress=lambda p, q: log("  signing step %d / %d" % (p, q)))
        chainsynth.corrupt(sigs, bad, random.Random(31))
    else:
        sigs = s.sign_beacons(sk, rounds)
        g1_synth.corrupt(sigs, bad, random.Random(41))
    keep = np.ones(n, bool)
    keep[[n // 7, n // 2, n - 5000]] = False
    rounds, sigs = rounds[keep], np.ascontiguousarray(sigs[keep])
    dt, lay = timed(lambda: write_bolt2(path, [(bytes(8), genesis)], rounds=rounds, sigs=sigs, page_size=4096))
    log("  wrote %s: %d bytes, %d leaves, depth %d, %.2f s" % (path, os.path.getsize(path), len(lay["leaves"]), lay["depth"], dt))
    return rounds, sigs, genesis, lay


def measure(name, n, out_dir, skip_host, log):
    lib = _lib.load()
    s = drand_amd.scheme_from_name(name)
    sk = secret(name)
    pk = s.public_key(sk)
    path = os.path.join(out_dir, "replay_%s.db" % name)
    log("%s: building %d rounds" % (name, n))
    rounds, sigs, genesis, lay = build(s, sk, n, path, log)
    res = {"rounds_signed": n, "records": int(len(rounds)) + 1, "file_bytes": os.path.getsize(path), "leaves": len(lay["leaves"]),
           "depth": lay["depth"], "page_size": 4096}
    seed = 9
    # (b) device reader: one cold call (code objects, first allocations), then warm repetitions
    runs = []
    for rep in range(4):
        lib.dh_profile(1)
        t_open, dev = timed(lambda: DeviceBoltStore(path, s.chained))
        t_check, fb = timed(lambda: check_past_beacons(dev, s, pk, 1 << 40, seed=seed))
        prof = profile_read(lib)
        lib.dh_profile(0)
        dev.close()
        runs.append({"open_s": t_open, "check_s": t_check, "total_s": t_open + t_check,
                     "stages_ms": {k: prof[k]["total_ms"] for k in STAGES if k in prof},
                     "stage_calls": {k: prof[k]["count"] for k in STAGES if k in prof}})
        log("  (b) rep %d: open %.3f s, check %.3f s, stages %s" % (rep, t_open, t_check, runs[-1]["stages_ms"]))
    warm = min(runs[1:], key=lambda r: r["total_s"])
    res["b_device_reader"] = {"cold": runs[0], "warm_best_of_3": warm, "faulty": len(fb)}
    # without profiling (the stage clocks add stream waits only where the path waits anyway)
    t_plain = []
    for rep in range(3):
        t, fb2 = timed(lambda: check_past_beacons(DeviceBoltStore(path, s.chained), s, pk, 1 << 40, seed=seed))
        assert fb2 == fb
        t_plain.append(t)
    res["b_device_reader"]["unprofiled_total_s"] = min(t_plain)
    # (a) host reader, as a user gets it today
    if not skip_host:
        t_open, host = timed(lambda: BoltTrimmedStore(path, s.chained))
        t_check, fa = timed(lambda: check_past_beacons(host, s, pk, 1 << 40, seed=seed))
        res["a_host_reader"] = {"open_s": t_open, "check_s": t_check, "total_s": t_open + t_check, "faulty": len(fa)}
        log("  (a) open %.2f s, check %.2f s" % (t_open, t_check))
        if fa != fb:
            raise SystemExit("VOID: faulty sets differ between the host and the device reader (%d vs %d rounds)" % (len(fa), len(fb)))
        res["equal_faulty_sets"] = True
        res["b_over_a_speedup"] = (t_open + t_check) / min(t_plain)
        del host
    # (c) the floor: verify_beacons on pre-built arrays (host arrays, copied in)
    prevs = plens = None
    if s.chained:
        prevs, plens = chainsynth.stored_prevs(sigs, genesis)
        # rows whose predecessor record was removed carry another round's signature here; verdicts are not compared
    tc = []
    for rep in range(4):
        t, _ = timed(lambda: s.verify_beacons(pk, rounds, sigs, prevs, seed=seed, want_randomness=False, previous_lengths=plens))
        tc.append(t)
    res["c_verify_arrays_s"] = min(tc[1:])
    # (d) a device-to-device copy of the gather's traffic: it reads the leaves and writes rounds + lens + rows
    stride = (s.sig_len + 3) & ~3
    moved = res["leaves"] * 4096 + len(rounds) * (stride + 12)
    # 16 buffer pairs in rotation (more than the 256 MiB Infinity Cache), written once first: a copy out of HBM
    pairs = [(torch.full((moved // 2,), k, dtype=torch.uint8, device="cuda"), torch.empty(moved // 2, dtype=torch.uint8, device="cuda"))
             for k in range(16)]
    td = []
    for rep in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for src, dst in pairs:
            dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        td.append(e0.elapsed_time(e1) / len(pairs))
    del pairs
    d_ms = statistics.median(td[1:])
    g_ms = warm["stages_ms"].get("k_bolt_gather")
    res["d_copy"] = {"bytes_read_plus_written": moved, "copy_ms": d_ms, "copy_GBps": moved / d_ms / 1e6,
                     "gather_kernel_ms": g_ms, "gather_GBps": moved / g_ms / 1e6 if g_ms else None}
    st = warm["stages_ms"]
    ingest = sum(st.get(k, 0) for k in ("store_index", "store_upload", "store_scan", "store_gather_link"))
    res["ingest_ms"], res["verify_ms"] = ingest, st.get("store_verify", 0)
    res["ingest_share_of_b"] = ingest / (ingest + res["verify_ms"]) if ingest + res["verify_ms"] else None
    res["rounds_per_s_b"] = res["records"] / min(t_plain)
    log("  %s" % json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}))
    os.remove(path)
    return res


def build_untrimmed(s, sk, n, path, log):
    """The chain of build() as Beacon.Marshal() values: record r stores the signature its predecessor record holds."""
    rounds = np.arange(1, n + 1, dtype=np.uint64)
    bad = chainsynth.corrupted_rounds(n, n // 1000)
    genesis = hashlib.sha256(b"store replay genesis").digest()
    sigs = chainsynth.sign_chain(s, sk, 1, n, genesis, bad, np.random.default_rng(5),
                                 progress=lambda p, q: log("  signing step %d / %d" % (p, q)))
    chainsynth.corrupt(sigs, bad, random.Random(31))
    prevs, plens = chainsynth.stored_prevs(sigs, genesis)
    keep = np.ones(n, bool)
    keep[[n // 7, n // 2, n - 5000]] = False
    rounds, sigs, prevs, plens = rounds[keep], np.ascontiguousarray(sigs[keep]), np.ascontiguousarray(prevs[keep]), plens[keep]
    sig_hex, prev_hex, L = sigs.tobytes().hex().encode(), prevs.tobytes().hex().encode(), 2 * s.sig_len
    items = [(bytes(8), b'{"PreviousSig":null,"Round":0,"Signature":"%s"}' % genesis.hex().encode())]
    for i, r in enumerate(rounds.tolist()):
        items.append((r.to_bytes(8, "big"), b'{"PreviousSig":"%s","Round":%d,"Signature":"%s"}' %
                      (prev_hex[192 * i:192 * i + 2 * int(plens[i])], r, sig_hex[L * i:L * (i + 1)])))
    dt, lay = timed(lambda: write_bolt2(path, items, page_size=4096))
    log("  wrote %s: %d bytes, %d leaves, depth %d, %.2f s" % (path, os.path.getsize(path), len(lay["leaves"]), lay["depth"], dt))
    return rounds, sigs, prevs, plens, lay


def measure_untrimmed(name, n, out_dir, skip_host, log):
    lib = _lib.load()
    s = drand_amd.scheme_from_name(name)
    sk = secret(name)
    pk = s.public_key(sk)
    path = os.path.join(out_dir, "replay_untrimmed_%s.db" % name)
    log("%s (untrimmed): building %d rounds" % (name, n))
    rounds, sigs, prevs, plens, lay = build_untrimmed(s, sk, n, path, log)
    res = {"format": "untrimmed", "rounds_signed": n, "records": int(len(rounds)) + 1, "file_bytes": os.path.getsize(path),
           "leaves": len(lay["leaves"]), "depth": lay["depth"], "page_size": 4096}
    seed = 9
    runs = []
    for rep in range(4):  # one cold call (code objects, first allocations), then warm repetitions
        lib.dh_profile(1)
        t_open, dev = timed(lambda: DeviceBoltStore(path, s.chained, fmt="untrimmed"))
        t_check, fb = timed(lambda: check_past_beacons(dev, s, pk, 1 << 40, seed=seed))
        prof = profile_read(lib)
        lib.dh_profile(0)
        res["format_stat"] = dev.format_stat()
        dev.close()
        runs.append({"open_s": t_open, "check_s": t_check, "total_s": t_open + t_check,
                     "stages_ms": {k: prof[k]["total_ms"] for k in STAGES if k in prof},
                     "stage_calls": {k: prof[k]["count"] for k in STAGES if k in prof}})
        log("  (b) rep %d: open %.3f s, check %.3f s, stages %s" % (rep, t_open, t_check, runs[-1]["stages_ms"]))
    warm = min(runs[1:], key=lambda r: r["total_s"])
    res["b_device_reader"] = {"cold": runs[0], "warm_best_of_3": warm, "faulty": len(fb)}
    t_plain = []
    for rep in range(3):
        t, fb2 = timed(lambda: check_past_beacons(DeviceBoltStore(path, s.chained, fmt="auto"), s, pk, 1 << 40, seed=seed))
        assert fb2 == fb
        t_plain.append(t)
    res["b_device_reader"]["unprofiled_total_s"] = min(t_plain)
    if not skip_host:  # (a) the host reader, as a user gets it today
        t_open, host = timed(lambda: BoltUntrimmedStore(path, s.chained))
        t_check, fa = timed(lambda: check_past_beacons(host, s, pk, 1 << 40, seed=seed))
        res["a_host_reader"] = {"open_s": t_open, "check_s": t_check, "total_s": t_open + t_check, "faulty": len(fa)}
        log("  (a) open %.2f s, check %.2f s" % (t_open, t_check))
        if fa != fb:
            raise SystemExit("VOID: faulty lists differ between the host and the device reader (%d vs %d rounds)" % (len(fa), len(fb)))
        res["equal_faulty_sets"] = True
        res["b_over_a_speedup"] = (t_open + t_check) / min(t_plain)
        del host
    tc = []
    for rep in range(4):  # (c) the floor: verify_beacons on pre-built arrays (host arrays, copied in)
        t, _ = timed(lambda: s.verify_beacons(pk, rounds, sigs, prevs, seed=seed, want_randomness=False, previous_lengths=plens))
        tc.append(t)
    res["c_verify_arrays_s"] = min(tc[1:])
    st = warm["stages_ms"]
    ingest = sum(st.get(k, 0) for k in ("store_index", "store_upload", "store_scan", "store_gather_link"))
    res["ingest_ms"], res["verify_ms"] = ingest, st.get("store_verify", 0)
    res["ingest_share_of_b"] = ingest / (ingest + res["verify_ms"]) if ingest + res["verify_ms"] else None
    res["rounds_per_s_b"] = res["records"] / min(t_plain)
    log("  %s" % json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}))
    os.remove(path)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--format", choices=["trimmed", "untrimmed"], default="trimmed")
    ap.add_argument("--skip-host", action="store_true", help="leave out (a), the slow host reader")
    ap.add_argument("--schemes", default=None, help="default: quicknet and chained (trimmed), chained (untrimmed)")
    a = ap.parse_args()
    untrimmed = a.format == "untrimmed"
    a.out = a.out or os.path.join(ROOT, "bench_outputs", "store_replay_untrimmed.json" if untrimmed else "store_replay.json")
    a.schemes = a.schemes or ("pedersen-bls-chained" if untrimmed else "bls-unchained-g1-rfc9380,pedersen-bls-chained")
    out_dir = os.path.dirname(os.path.abspath(a.out))
    os.makedirs(out_dir, exist_ok=True)
    assert _lib.load().dh_init(0) == 0, _lib.last_error()

    def log(msg):
        print(msg, flush=True)

    res = {"device": torch.cuda.get_device_name(0), "version": _lib.load().dh_version().decode(), "schemes": {}}
    for name in a.schemes.split(","):
        res["schemes"][name] = (measure_untrimmed if untrimmed else measure)(name, a.rounds, out_dir, a.skip_host, log)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({"store_replay": a.out, "speedup": {k: v.get("b_over_a_speedup") for k, v in res["schemes"].items()}}))


if __name__ == "__main__":
    main()
