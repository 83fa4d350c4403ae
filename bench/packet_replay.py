"""Checking a run of protobuf BeaconPacket frames end to end on one MI355X (recorded in
profiles/r21/packet_replay.json): 1,048,576 signed records per signature size (quicknet: 48-byte G1 signatures;
pedersen-bls-chained: 96-byte G2 signatures with previous_signature) from bench/chainsynth.py's chains, written with
packet_bytes, 0.1% of the records corrupted, two ways in one run:
  (a) the host path: a decode per record (google.protobuf when it imports, else packet_from_bytes; the result says
      which), random_data_columns-style copying, and the parent's verify_beacons (one repetition);
  (b) the device path: DeviceArchive.from_packets(bytes, lens).check, cold once, then warm best of 3, split by dh_profile
      stages.
(a) and (b) must mark the same records invalid, or the run is void (it raises). Also recorded: the encode of the same
columns back into frames (which must give the input bytes), and k_ndjson_gather on the JSON-lines form of the same chain
next to k_pb_gather.
  python bench/packet_replay.py [--rounds N] [--out OUT.json] [--schemes A,B]   (default: bench_outputs/packet_replay.json)"""
import argparse
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
from archive_replay import profile_read, secret, timed
from drand_amd import _lib
from drand_amd.store import (AR_INVALID, PB_BEACON_PACKET, DeviceArchive, encode_beacon_packets, packet_bytes, packet_from_bytes,
                             random_data_line)

STAGES = ["archive_upload", "archive_stat", "archive_gather", "archive_verify", "archive_fold", "k_pb_gather"]
BEACON_ID = "default"


def build(s, sk, n, log):
    """Sign rounds 1..n and corrupt 0.1%: ([frame bytes], the JSON-lines archive of the same records)."""
    rounds = np.arange(1, n + 1, dtype=np.uint64)
    bad = chainsynth.corrupted_rounds(n, n // 1000)
    genesis = hashlib.sha256(b"packet replay genesis").digest()
    prevs = plens = None
    if s.chained:
        sigs = chainsynth.sign_chain(s, sk, 1, n, genesis, bad, np.random.default_rng(5),
                                     progress=lambda p, q: log("  signing step %d / %d" % (p, q)) if p % 500 == 0 else None)
        chainsynth.corrupt(sigs, bad, random.Random(31))
        prevs, plens = chainsynth.stored_prevs(sigs, genesis)
    else:
        sigs = s.sign_beacons(sk, rounds)
        g1_synth.corrupt(sigs, bad, random.Random(41))
    frames, lines = [], []
    for i in range(n):
        r = {"round": int(rounds[i]), "signature": sigs[i].tobytes(), "previous_signature": prevs[i, :int(plens[i])].tobytes() if s.chained else b""}
        frames.append(packet_bytes(PB_BEACON_PACKET, r, BEACON_ID))
        lines.append(random_data_line(r))
    return frames, b"\n".join(lines) + b"\n"


def host_decoder():
    """(name, frame -> (round, signature, previous_signature))"""
    try:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import packet_cases
        cls = packet_cases.message_classes()[PB_BEACON_PACKET]
    except Exception:  # noqa: BLE001 - google.protobuf is not on the box
        def dec(b):
            r = packet_from_bytes(PB_BEACON_PACKET, b)
            return r["round"], r["signature"], r["previous_signature"]
        return "packet_from_bytes", dec
    import google.protobuf

    def dec(b):
        m = cls()
        m.ParseFromString(b)
        return m.round, m.signature, m.previous_signature
    return "google.protobuf %s (%s)" % (google.protobuf.__version__, "upb"), dec


def measure(name, n, log):
    lib = _lib.load()
    s = drand_amd.scheme_from_name(name)
    sk = secret(name)
    pk = s.public_key(sk)
    log("%s: building %d rounds" % (name, n))
    frames, json_lines = build(s, sk, n, log)
    data, lens = b"".join(frames), np.array([len(f) for f in frames], np.uint32)
    res = {"records": n, "frame_bytes": len(data), "json_bytes": len(json_lines)}
    seed = 9
    runs = []
    for rep in range(4):  # one cold call (code objects, first allocations), then warm repetitions
        lib.dh_profile(1)
        t_open, ar = timed(lambda: DeviceArchive.from_packets(PB_BEACON_PACKET, data, lens=lens))
        t_check, st_b = timed(lambda: ar.check(s, pk, seed=seed, beacon_id=BEACON_ID))
        prof = profile_read(lib)
        lib.dh_profile(0)
        res["stat"] = ar.stat()
        if rep < 3:
            ar.close()
        runs.append({"open_s": t_open, "check_s": t_check, "total_s": t_open + t_check,
                     "stages_ms": {k: prof[k]["total_ms"] for k in STAGES if k in prof},
                     "stage_calls": {k: prof[k]["count"] for k in STAGES if k in prof}})
        log("  (b) rep %d: open %.3f s, check %.3f s, stages %s" % (rep, t_open, t_check, runs[-1]["stages_ms"]))
    warm = min(runs[1:], key=lambda r: r["total_s"])
    marked_b = np.flatnonzero(st_b & AR_INVALID)
    res["b_device_path"] = {"cold": runs[0], "warm_best_of_3": warm, "invalid": int(len(marked_b)),
                            "status_histogram": {str(int(k)): int(v) for k, v in zip(*np.unique(st_b, return_counts=True))}}
    # the encode of the same columns: it must give the input bytes back
    stride = (s.sig_len + 3) & ~3
    rounds_d, sigs_d, sl_d, prevs_d, pl_d, _r, _rl, dfr = ar.beacons_device(sig_stride=stride, prev_stride=stride, want_prev=s.chained, want_rand=False)
    ar.close()
    assert not int(dfr.sum())
    enc = []
    for rep in range(4):
        lib.dh_profile(1)
        t_enc, (out, _l) = timed(lambda: encode_beacon_packets(rounds_d, sigs_d, sl_d, prevs_d, pl_d, beacon_id=BEACON_ID))
        prof = profile_read(lib)
        lib.dh_profile(0)
        enc.append({"wall_s": t_enc, "k_pb_size_ms": prof["k_pb_size"]["total_ms"], "k_pb_size_calls": prof["k_pb_size"]["count"],
                    "k_pb_encode_ms": prof["k_pb_encode"]["total_ms"]})
    if bytes(out.cpu().numpy()) != data:
        raise SystemExit("VOID: the encoder does not give the input frames back")
    best = min(enc[1:], key=lambda e: e["wall_s"])
    res["encode"] = {"cold": enc[0], "warm_best_of_3": best, "bytes_written": len(data), "round_trip_equal": True,
                     "k_pb_encode_GBps_written": len(data) / best["k_pb_encode_ms"] / 1e6}
    log("  encode: %s" % res["encode"]["warm_best_of_3"])
    del out, rounds_d, sigs_d, prevs_d
    # k_ndjson_gather on the JSON-lines form of the same chain, the same columns, in the same session
    gat = []
    for rep in range(3):
        with DeviceArchive(json_lines) as arj:
            lib.dh_profile(1)
            arj.beacons_device(sig_stride=stride, prev_stride=stride, want_prev=s.chained, want_rand=False)
            prof_j = profile_read(lib)
            lib.dh_profile(0)
        with DeviceArchive.from_packets(PB_BEACON_PACKET, data, lens=lens) as arp:
            lib.dh_profile(1)
            arp.beacons_device(sig_stride=stride, prev_stride=stride, want_prev=s.chained, want_rand=False)
            prof_p = profile_read(lib)
            lib.dh_profile(0)
        gat.append({"k_ndjson_gather_ms": prof_j["k_ndjson_gather"]["total_ms"], "k_pb_gather_ms": prof_p["k_pb_gather"]["total_ms"]})
    written = n * (8 + 4 + 1 + stride + ((stride + 4) if s.chained else 0))
    g = min(gat[1:], key=lambda x: x["k_pb_gather_ms"])
    res["gather_same_columns"] = {"runs": gat, "bytes_written": written,
                                  "k_pb_gather_GBps": (len(data) + n * 12 + written) / g["k_pb_gather_ms"] / 1e6,
                                  "k_ndjson_gather_GBps": (len(json_lines) + n * 12 + written) / g["k_ndjson_gather_ms"] / 1e6}
    log("  gather: %s" % res["gather_same_columns"])
    # (a) the host path: a decode per record, the copying, the parent's verifier
    dec_name, dec = host_decoder()
    t_dec, recs = timed(lambda: [dec(f) for f in frames])

    def cols():
        rounds = np.array([r[0] for r in recs], dtype=np.uint64)
        sigs = np.zeros((n, s.sig_len), dtype=np.uint8)
        for i, r in enumerate(recs):
            if len(r[1]) == s.sig_len:
                sigs[i] = np.frombuffer(r[1], np.uint8)
        return rounds, sigs, [r[2] for r in recs]
    t_cols, (rounds, sigs, prevs) = timed(cols)
    t_ver, (ok, _) = timed(lambda: s.verify_beacons(pk, rounds, sigs, prevs if s.chained else None, seed=seed, want_randomness=False))
    bad_len = np.array([len(r[1]) != s.sig_len for r in recs])
    marked_a = np.flatnonzero(bad_len | ~np.asarray(ok, bool))
    res["a_host_path"] = {"decoder": dec_name, "decode_s": t_dec, "columns_s": t_cols, "verify_beacons_s": t_ver,
                          "total_s": t_dec + t_cols + t_ver, "invalid": int(len(marked_a))}
    log("  (a) %s: decode %.2f s, columns %.2f s, verify %.3f s" % (dec_name, t_dec, t_cols, t_ver))
    if len(st_b) != len(recs) or not np.array_equal(marked_a, marked_b):
        raise SystemExit("VOID: the host and the device path mark different records (%d vs %d)" % (len(marked_a), len(marked_b)))
    res["equal_marked_records"] = True
    res["b_over_a_speedup"] = res["a_host_path"]["total_s"] / warm["total_s"]
    st = warm["stages_ms"]
    ingest = sum(st.get(k, 0) for k in ("archive_upload", "archive_stat", "archive_gather"))
    res["ingest_ms"], res["verify_ms"], res["fold_ms"] = ingest, st.get("archive_verify", 0), st.get("archive_fold", 0)
    res["ingest_share_of_b"] = ingest / (1000 * warm["total_s"])
    res["records_per_s_b"] = n / warm["total_s"]
    log("  %s" % json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "packet_replay.json"))
    ap.add_argument("--schemes", default="bls-unchained-g1-rfc9380,pedersen-bls-chained")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    assert _lib.load().dh_init(0) == 0, _lib.last_error()

    def log(msg):
        print(msg, flush=True)

    res = {"device": torch.cuda.get_device_name(0), "version": _lib.load().dh_version().decode(), "schemes": {}}
    if os.path.exists(a.out):  # schemes measured by an earlier call are kept
        res["schemes"] = json.load(open(a.out)).get("schemes", {})
    for name in a.schemes.split(","):
        res["schemes"][name] = measure(name, a.rounds, log)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({"packet_replay": a.out, "speedup": {k: v.get("b_over_a_speedup") for k, v in res["schemes"].items()}}))


if __name__ == "__main__":
    main()
