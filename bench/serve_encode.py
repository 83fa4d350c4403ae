"""The served-record encoders on one MI355X (recorded in profiles/r23/serve_encode.json): 1,048,576 rows
per shape (quicknet: 48-byte signatures, no previous signature; chained: 96-byte signatures with the stored previous
signature). The signatures are pseudo-random bytes: nothing here verifies them and no encoder's time depends on their
validity. In one run:
  kernels     k_serve_encode for RandomData JSON and PublicRandResponse, with the randomness computed (SHA-256 per row
              in the kernel) and with it given as a column, warm best of 3 by dh_profile; beside them k_pb_encode
              (BeaconPacket) on the same columns, the nearest sibling. GB/s are bytes written per kernel time.
  end to end  store.export_random_data of a trimmed store file holding the rows (encode, copy to the host, write the
              archive) against the host loop over the same file (BoltTrimmedStore.columns, then random_data_line with
              hashlib per record, written to a file); store.public_rand_frames copied to the host against a
              packet_bytes loop over the same records. The device's bytes must equal the host's, or the run is void.
  python bench/serve_encode.py [--rounds N] [--out OUT.json] [--host-rounds M]   (default: bench_outputs/serve_encode.json)
The host loops run over the first M rounds (default: all) and are scaled to N when M < N; the result says so."""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import torch

torch.zeros(1, device="cuda")
from drand_amd import _lib, store

META = {"beacon_id": "default"}
SHAPES = {"quicknet": (48, False), "chained": (96, True)}


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


def kernel_runs(lib, fn, kernels, reps=4):
    """fn() (a sizing call, then the encode: the size kernel runs twice) under dh_profile `reps` times: the first cold,
    then the best warm run by the last kernel's time."""
    runs = []
    for _ in range(reps):
        lib.dh_profile(1)
        wall, out = timed(fn)
        prof = profile_read(lib)
        lib.dh_profile(0)
        run = {"wall_s": wall}
        for k in kernels:
            run[k + "_ms"], run[k + "_calls"] = prof[k]["total_ms"], prof[k]["count"]
        runs.append(run)
        nbytes = int(out[0].numel())
        del out
    best = min(runs[1:], key=lambda r: r[kernels[-1] + "_ms"])
    return {"cold": runs[0], "warm_best_of_3": best, "bytes_written": nbytes, "GBps_written": nbytes / best[kernels[-1] + "_ms"] / 1e6}


def measure(shape, n, host_n, log):
    lib = _lib.load()
    sig_len, chained = SHAPES[shape]
    g = torch.Generator(device="cuda").manual_seed(7 + sig_len)
    all_sigs = torch.randint(0, 256, (n + 1, sig_len), dtype=torch.uint8, device="cuda", generator=g)  # row 0: the round before the first
    rounds = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
    sigs = all_sigs[1:].contiguous()
    lens = torch.full((n,), sig_len, dtype=torch.int32, device="cuda")
    prevs = all_sigs[:-1].contiguous() if chained else None
    prev_lens = lens.clone() if chained else None
    rands = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)  # any 32 bytes cost the same to copy
    read = n * (8 + 4 + sig_len + ((sig_len + 4) if chained else 0))
    res = {"rows": n, "signature_bytes": sig_len, "previous_signature": chained, "column_bytes_read": read, "kernels": {}}
    cases = {
        "random_data_json_computed": lambda: store.encode_random_data(rounds, sigs, lens, prevs, prev_lens),
        "random_data_json_given": lambda: store.encode_random_data(rounds, sigs, lens, prevs, prev_lens, rands=rands),
        "public_rand_pb_computed": lambda: store.encode_public_rand(rounds, sigs, lens, prevs, prev_lens, metadata=META),
        "public_rand_pb_given": lambda: store.encode_public_rand(rounds, sigs, lens, prevs, prev_lens, rands=rands, metadata=META),
    }
    for name, fn in cases.items():
        res["kernels"][name] = kernel_runs(lib, fn, ["k_serve_size", "k_serve_encode"])
        log("  %s: %s" % (name, json.dumps(res["kernels"][name]["warm_best_of_3"])) + " %.1f GB/s written" % res["kernels"][name]["GBps_written"])
    res["kernels"]["beacon_packet_k_pb_encode"] = kernel_runs(
        lib, lambda: store.encode_beacon_packets(rounds, sigs, lens, prevs, prev_lens, beacon_id="default"), ["k_pb_size", "k_pb_encode"])
    log("  k_pb_encode: %s %.1f GB/s written" % (json.dumps(res["kernels"]["beacon_packet_k_pb_encode"]["warm_best_of_3"]),
                                                res["kernels"]["beacon_packet_k_pb_encode"]["GBps_written"]))
    # ---- end to end over a store file
    with tempfile.TemporaryDirectory() as tmp:
        db, arch, host_arch = (os.path.join(tmp, f) for f in ("chain.db", "device.ndjson", "host.ndjson"))
        store.write_trimmed_bolt(db, np.arange(0, n + 1, dtype=np.uint64), all_sigs.cpu().numpy())
        with store.DeviceBoltStore(db, chained) as st:
            exports = [timed(lambda: store.export_random_data(st, arch)) for _ in range(3)]
            t_frames, frames = min((timed(lambda: [f.cpu().numpy() for f, _l in store.public_rand_frames(st, 1, metadata=META, delimited=True)])
                                    for _ in range(3)), key=lambda x: x[0])
        t_export, out = min(exports, key=lambda x: x[0])

        def host_columns():
            return store.BoltTrimmedStore(db, chained).columns(1, host_n, sig_len)

        def host_records(cols):
            r, s, p, _m = cols
            return [{"round": int(r[i]), "signature": s[i].tobytes(), "previous_signature": p[i] if chained else b"",
                     "randomness": hashlib.sha256(s[i].tobytes()).digest()} for i in range(len(r))]

        def host_export(recs):
            with open(host_arch, "wb") as f:
                for rec in recs:
                    f.write(store.random_data_line(rec) + b"\n")

        t_cols, cols = timed(host_columns)
        t_recs, recs = timed(lambda: host_records(cols))
        t_lines, _ = timed(lambda: host_export(recs))
        t_pb, host_frames = timed(lambda: store.delimited([store.packet_bytes(store.PB_PUBLIC_RAND, dict(rec, metadata=META)) for rec in recs]))
        host_bytes = open(host_arch, "rb").read()
        dev_bytes = open(arch, "rb").read()
        dev_frames = b"".join(f.tobytes() for f in frames)
        if dev_bytes[:len(host_bytes)] != host_bytes or dev_frames[:len(host_frames)] != host_frames or (host_n == n and (
                len(dev_bytes) != len(host_bytes) or len(dev_frames) != len(host_frames))):
            raise SystemExit("VOID: the device's records differ from the host writers'")
    scale = n / host_n
    res["export_random_data"] = {"device_s": t_export, "records": out["records"], "bytes": out["bytes"],
                                 "host_read_store_s": t_cols * scale, "host_records_and_sha256_s": t_recs * scale,
                                 "host_random_data_line_and_write_s": t_lines * scale, "host_total_s": (t_cols + t_recs + t_lines) * scale,
                                 "host_rounds_measured": host_n, "equal_bytes": True}
    res["export_random_data"]["speedup"] = res["export_random_data"]["host_total_s"] / t_export
    res["public_rand_frames"] = {"device_s": t_frames, "bytes": len(dev_frames), "host_packet_bytes_s": t_pb * scale,
                                 "host_total_s": (t_cols + t_recs + t_pb) * scale, "host_rounds_measured": host_n, "equal_bytes": True}
    res["public_rand_frames"]["speedup"] = res["public_rand_frames"]["host_total_s"] / t_frames
    log("  export_random_data: %s" % json.dumps(res["export_random_data"]))
    log("  public_rand_frames: %s" % json.dumps(res["public_rand_frames"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=1 << 20)
    ap.add_argument("--host-rounds", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "serve_encode.json"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    assert _lib.load().dh_init(0) == 0, _lib.last_error()

    def log(msg):
        print(msg, flush=True)

    res = {"device": torch.cuda.get_device_name(0), "version": _lib.load().dh_version().decode(), "shapes": {}}
    for shape in SHAPES:
        log("%s: %d rows" % (shape, a.rounds))
        res["shapes"][shape] = measure(shape, a.rounds, min(a.host_rounds or a.rounds, a.rounds), log)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({"serve_encode": a.out, "GBps_written": {s: {k: round(v["GBps_written"], 1) for k, v in r["kernels"].items()}
                                                             for s, r in res["shapes"].items()}}))


if __name__ == "__main__":
    main()
