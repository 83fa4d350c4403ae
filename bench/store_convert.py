"""Converting a legacy (untrimmed, hexjson) bbolt chain store to the trimmed format on one MI355X (DESIGN.md §22;
recorded in profiles/r17/store_convert.json). Input: the 1,048,576-round pedersen-bls-chained untrimmed file of §18, as
bench/store_replay.py builds it. Three measurements in one run:
  (a) what a user has without the device writer: BoltUntrimmedStore reads and decodes every record, then the vectorised
      boltwrite2.write_bolt2(rounds=, sigs=) writes them;
  (b) DeviceBoltStore(fmt="untrimmed").save_trimmed: the first call and the best of three warm ones, split by dh_profile
      stages (merge = gather + decode + merge, plan, pack, download) with the host's file write timed apart;
  (c) k_bolt_pack alone, in bytes read plus written per second, next to a device-to-device copy of as many bytes through
      rotating buffers.
The run is void (it raises) unless the files of (a) and (b) hold the same records through BoltTrimmedStore.
  python bench/store_convert.py [--rounds N] [--out OUT.json]     (default: bench_outputs/store_convert.json)"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "bench")]
import numpy as np
import torch

torch.zeros(1, device="cuda")
import drand_amd
import store_replay
from boltwrite2 import write_bolt2
from drand_amd import _lib
from drand_amd import store as dstore

STAGES = ["store_save_merge", "store_save_plan", "store_save_pack", "store_save_download", "k_bolt_gather_json", "k_bolt_pack"]
NAME = "pedersen-bls-chained"


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def host_convert(src, dst):
    """(a): (read + decode seconds, write seconds)."""
    def read():
        st = dstore.BoltUntrimmedStore(src, True)
        rounds = st.rounds()
        sigs = [st.get(r).signature for r in rounds]
        return rounds, sigs

    t_read, (rounds, sigs) = timed(read)
    assert rounds[0] == 0 and len(sigs[0]) == 32 and all(len(x) == 96 for x in sigs[1:])

    def write():
        arr = np.frombuffer(b"".join(sigs[1:]), np.uint8).reshape(-1, 96)
        write_bolt2(dst, [(bytes(8), sigs[0])], rounds=np.array(rounds[1:], np.uint64), sigs=arr, page_size=4096)

    t_write, _ = timed(write)
    return t_read, t_write


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "store_convert.json"))
    a = ap.parse_args()
    out_dir = os.path.dirname(os.path.abspath(a.out))
    work = os.path.join(ROOT, "bench_outputs")
    os.makedirs(out_dir, exist_ok=True)
    os.makedirs(work, exist_ok=True)
    lib = _lib.load()
    assert lib.dh_init(0) == 0, _lib.last_error()

    def log(msg):
        print(msg, flush=True)

    s = drand_amd.scheme_from_name(NAME)
    sk = store_replay.secret(NAME)
    src, dst_a, dst_b = (os.path.join(work, "convert_%s.db" % k) for k in ("src", "a", "b"))
    log("building %d rounds (untrimmed)" % a.rounds)
    rounds, _sigs, _prevs, _plens, lay = store_replay.build_untrimmed(s, sk, a.rounds, src, log)
    res = {"device": torch.cuda.get_device_name(0), "version": lib.dh_version().decode(), "scheme": NAME, "rounds_signed": a.rounds,
           "records": int(len(rounds)) + 1, "source_bytes": os.path.getsize(src), "source_leaves": len(lay["leaves"]), "page_size": 4096}

    # (b) the device path; the file write is timed apart from the library call
    write_s = []
    plain_replace = dstore._replace_file

    def timed_replace(path, image):
        t, _ = timed(lambda: plain_replace(path, image))
        write_s.append(t)

    dstore._replace_file = timed_replace
    runs = []
    for rep in range(4):
        lib.dh_profile(1)
        t_open, dev = timed(lambda: dstore.DeviceBoltStore(src, True, fmt="untrimmed"))
        t_save, info = timed(lambda: dev.save_trimmed(dst_b))
        prof = store_replay.profile_read(lib)
        lib.dh_profile(0)
        dev.close()
        runs.append({"open_s": t_open, "save_s": t_save, "file_write_s": write_s[-1], "total_s": t_open + t_save,
                     "stages_ms": {k: prof[k]["total_ms"] for k in STAGES if k in prof}})
        log("  (b) rep %d: open %.3f s, save %.3f s (file write %.3f s), stages %s" % (rep, t_open, t_save, write_s[-1], runs[-1]["stages_ms"]))
    dstore._replace_file = plain_replace
    warm = min(runs[1:], key=lambda r: r["total_s"])
    res["b_device"] = {"first_call": runs[0], "warm_best_of_3": warm, "result": {k: v for k, v in info.items() if k not in ("unlinked", "undecodable")},
                       "unlinked": len(info["unlinked"]), "undecodable": len(info["undecodable"]), "image_bytes": os.path.getsize(dst_b)}

    # (a) the host path
    t_read, t_write = host_convert(src, dst_a)
    res["a_host"] = {"read_decode_s": t_read, "write_s": t_write, "total_s": t_read + t_write, "image_bytes": os.path.getsize(dst_a)}
    log("  (a) read + decode %.2f s, write %.2f s" % (t_read, t_write))
    ka, kb = dstore.BoltTrimmedStore(dst_a, True)._kv, dstore.BoltTrimmedStore(dst_b, True)._kv
    if ka != kb:
        raise SystemExit("VOID: the host's and the device's files hold different records (%d vs %d)" % (len(ka), len(kb)))
    res["equal_records"] = True
    res["a_over_b_warm"] = (t_read + t_write) / warm["total_s"]

    # (c) the pack kernel against a device-to-device copy of as many bytes
    n = res["b_device"]["result"]["rows"]
    leaves, pages = res["b_device"]["result"]["leaves"], res["b_device"]["result"]["pages"]
    assert pages - 4 >= leaves
    # read: rows, rounds, lens and the leaf plan; written: the leaf pages (one page a leaf: no record passes 4 KiB)
    moved = n * (96 + 8 + 4) + leaves * 24 + leaves * 4096
    pairs = [(torch.full((moved // 2,), k, dtype=torch.uint8, device="cuda"), torch.empty(moved // 2, dtype=torch.uint8, device="cuda"))
             for k in range(16)]  # 16 pairs in rotation: more than the 256 MiB Infinity Cache
    td = []
    for rep in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for x, y in pairs:
            y.copy_(x)
        e1.record()
        torch.cuda.synchronize()
        td.append(e0.elapsed_time(e1) / len(pairs))
    del pairs
    d_ms = statistics.median(td[1:])
    packs = sorted(r["stages_ms"]["k_bolt_pack"] for r in runs[1:] if "k_bolt_pack" in r["stages_ms"])
    p_ms = packs[len(packs) // 2] if packs else None
    res["c_pack"] = {"bytes_read_plus_written": moved, "copy_ms": d_ms, "copy_GBps": moved / d_ms / 1e6, "pack_kernel_ms": p_ms,
                     "pack_GBps": moved / p_ms / 1e6 if p_ms else None}
    log("  (c) %s" % json.dumps(res["c_pack"]))
    for p in (src, dst_a, dst_b):
        os.remove(p)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({"store_convert": a.out, "a_host_s": res["a_host"]["total_s"], "b_device_warm_s": warm["total_s"],
                      "a_over_b_warm": res["a_over_b_warm"]}))


if __name__ == "__main__":
    main()
