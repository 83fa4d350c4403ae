"""The streaming trimmed-store writer on one MI355X (recorded in profiles/r18/store_stream.json).

  big    a quicknet-shaped trimmed store of 33,554,432 rounds with 48-byte values, built by the vectorised
         boltwrite2.write_bolt2, rewritten by DeviceBoltStore.save_trimmed with a handful of patches through the
         streaming path (BoltWriter over dh_store_split windows), in a process of its own whose peak resident set
         (VmHWM of /proc/self/status, which belongs to the process's own address space; ru_maxrss is inherited across
         exec from the process that built the source and is not used) is read after the open and after the rewrite. Void (it raises) unless the result passes check_image, holds the right number of records, and a
         sample of rounds read back through BoltTrimmedStore equals the source with the patches applied. With --parent
         DIR (a built tree of the parent commit) the same call is made there first and its error text is recorded.
  sweep  the cost of streaming where both forms exist: the 1,048,576-round chained untrimmed store of §22 converted,
         and an 8,388,608-row trimmed store rewritten; one-shot from --parent DIR, one-shot from this tree, and this
         tree with windows of 1M, 4M and 8M rows; the variants alternate (one process each, twice round), every process
         makes one cold and three warm calls and all of them are kept.
  python bench/store_stream.py big|sweep [--rounds N] [--parent DIR] [--out OUT.json]   (default: bench_outputs/store_stream.json;
                                                                                          each mode fills its own key)"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(HERE))
WORK = os.path.join(ROOT, "bench_outputs")
SEED = 20231
STAGES = ["store_save_merge", "store_save_plan", "store_save_pack", "store_save_download", "store_save_window", "k_bolt_pack", "k_bolt_carry"]


def log(msg):
    print(msg, file=sys.stderr, flush=True)


def peak_rss_kb():
    """VmHWM: the high-water mark of this process's own resident set, in KiB."""
    for line in open("/proc/self/status"):
        if line.startswith("VmHWM:"):
            return int(line.split()[1])
    raise RuntimeError("no VmHWM in /proc/self/status")


def source_values(n):
    import numpy as np
    return np.random.default_rng(SEED).integers(0, 256, (n, 48), dtype=np.uint8)


def big_patches(n):
    """{round: bytes | None}: three replaced, two deleted, one inserted above the last stored round n."""
    import numpy as np
    rng = np.random.default_rng(SEED + 1)
    new = lambda: rng.integers(0, 256, 48, dtype=np.uint8).tobytes()
    return {5: new(), n // 2: new(), n: new(), 6: None, n // 3: None, n + 1: new()}


# ------------------------------------------------------------------ one process: cold + warm save_trimmed calls

def child_run(a):
    """--tree's save_trimmed of --src to --dst, `--reps` times: one JSON line {"seconds": [...], "peak_rss_kb", ...}."""
    sys.path[:0] = [a.tree, os.path.join(a.tree, "tests")]
    import torch
    torch.zeros(1, device="cuda")
    from drand_amd import _lib
    from drand_amd import store as dstore
    lib = _lib.load()
    assert lib.dh_init(0) == 0, _lib.last_error()
    patches = {int(k): (bytes.fromhex(v) if v is not None else None) for k, v in json.loads(a.patches).items()}
    out = {"tree": a.label, "window": a.window, "seconds": [], "stages_ms": [], "peak_rss_start_kb": peak_rss_kb()}
    t = time.perf_counter()
    dev = dstore.DeviceBoltStore(a.src, a.fmt == "untrimmed", fmt=a.fmt)
    out["open_s"] = time.perf_counter() - t
    out["peak_rss_after_open_kb"] = peak_rss_kb()  # the open reads the whole source file
    kw = {"window": a.window} if a.window else {}
    try:
        for _ in range(a.reps):
            lib.dh_profile(1)
            t = time.perf_counter()
            info = dev.save_trimmed(a.dst, patches=patches, **kw)
            out["seconds"].append(time.perf_counter() - t)
            buf = __import__("ctypes").create_string_buffer(1 << 16)
            lib.dh_profile_read(buf, len(buf))
            prof = json.loads(buf.value.decode())
            lib.dh_profile(0)
            out["stages_ms"].append({k: [prof[k]["count"], prof[k]["total_ms"]] for k in STAGES if k in prof})
        out["result"] = {k: (len(v) if isinstance(v, list) else v) for k, v in info.items()}
        out["image_bytes"] = os.path.getsize(a.dst)
    except Exception as e:  # noqa: BLE001 - the refusal is the result
        out["error"] = "%s: %s" % (type(e).__name__, e)
    dev.close()
    out["peak_rss_kb"] = peak_rss_kb()
    print(json.dumps(out))


def wait_for(cmd, limit):
    """subprocess.run(capture_output) that says it is alive once a minute."""
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    t0 = time.time()
    while True:
        try:
            out, err = p.communicate(timeout=60)
            return p.returncode, out, err
        except subprocess.TimeoutExpired:
            log("  ... %s, %d s" % (cmd[2], time.time() - t0))
            if time.time() - t0 > limit:
                p.kill()
                raise SystemExit("child ran over %d s" % limit)


def run_child(tree, src, dst, fmt, window, patches, reps):
    enc = json.dumps({str(k): (v.hex() if v is not None else None) for k, v in patches.items()})
    cmd = [sys.executable, HERE, "_run", "--tree", tree, "--label", "this" if tree == ROOT else "parent", "--src", src, "--dst", dst, "--fmt", fmt, "--window", str(window or 0),
           "--patches", enc, "--reps", str(reps)]
    rc, out, err = wait_for(cmd, 1100)
    if rc != 0:
        raise SystemExit("child failed (%d): %s" % (rc, err[-2000:]))
    return json.loads(out.strip().splitlines()[-1])


def child_verify(a):
    """check_image, the record count and a sample through BoltTrimmedStore; one JSON line."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import bolt_write_cases as wc
    from drand_amd.store import BoltTrimmedStore
    n = a.rounds
    patches = big_patches(n)
    want_records = n - sum(v is None for v in patches.values()) + sum(r > n for r, v in patches.items() if v is not None)
    out = {}
    if a.what == "image":
        t = time.perf_counter()
        info = wc.check_image(open(a.dst, "rb").read())
        out = {"check_image": True, "records": len(info["records"]), "depth": info["depth"], "pages": info["pages"],
               "seconds": time.perf_counter() - t}
        if out["records"] != want_records:
            raise SystemExit("VOID: %d records, expected %d" % (out["records"], want_records))
    else:
        t = time.perf_counter()
        vals = source_values(n)
        st = BoltTrimmedStore(a.dst, False)
        rng = np.random.default_rng(SEED + 2)
        sample = sorted(set(int(x) for x in rng.integers(1, n + 1, 4096)) | set(patches) | {1, 2, n - 1, 4, 7})
        for r in sample:
            want = patches[r] if r in patches else vals[r - 1].tobytes()
            got = st._kv.get(r.to_bytes(8, "big"))
            if got != want:
                raise SystemExit("VOID: round %d reads back %r, expected %r" % (r, got, want))
        if st.len() != want_records:
            raise SystemExit("VOID: %d records, expected %d" % (st.len(), want_records))
        out = {"sample_equal": True, "sampled": len(sample), "records": st.len(), "seconds": time.perf_counter() - t}
    print(json.dumps(out))


def verify(dst, n, what):
    rc, out, err = wait_for([sys.executable, HERE, "_verify", "--dst", dst, "--rounds", str(n), "--what", what], 1100)
    if rc != 0:
        raise SystemExit("verification failed: %s %s" % (out[-500:], err[-2000:]))
    return json.loads(out.strip().splitlines()[-1])


# ------------------------------------------------------------------ big

def big(a):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    from boltwrite2 import write_bolt2
    n = a.rounds
    src, dst = os.path.join(WORK, "stream_big_src.db"), os.path.join(WORK, "stream_big_dst.db")
    t = time.perf_counter()
    write_bolt2(src, [], rounds=np.arange(1, n + 1, dtype=np.uint64), sigs=source_values(n), page_size=4096)
    log("built %d rounds, %d bytes, %.1f s" % (n, os.path.getsize(src), time.perf_counter() - t))
    res = {"rounds": n, "value_bytes": 48, "source_bytes": os.path.getsize(src), "patches": len(big_patches(n))}
    if a.parent:
        res["before_parent"] = run_child(a.parent, src, dst, "trimmed", None, big_patches(n), 1)
        log("parent: %s" % res["before_parent"].get("error", res["before_parent"]["seconds"]))
    res["streaming"] = run_child(ROOT, src, dst, "trimmed", None, big_patches(n), 1)
    log("this tree: %s" % json.dumps(res["streaming"]))
    if "error" in res["streaming"]:
        raise SystemExit("VOID: %s" % res["streaming"]["error"])
    st = res["streaming"]
    res["peak_rss_over_image"] = st["peak_rss_kb"] * 1024 / st["image_bytes"]
    res["peak_rss_growth_in_rewrite_bytes"] = (st["peak_rss_kb"] - st["peak_rss_after_open_kb"]) * 1024
    os.remove(src)
    res["verify_image"] = verify(dst, n, "image")
    log("check_image: %s" % json.dumps(res["verify_image"]))
    res["verify_sample"] = verify(dst, n, "sample")
    log("sample: %s" % json.dumps(res["verify_sample"]))
    os.remove(dst)
    return res


# ------------------------------------------------------------------ sweep

def sweep(a):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "bench")]
    import numpy as np
    import torch
    torch.zeros(1, device="cuda")
    import drand_amd
    import store_replay
    from boltwrite2 import write_bolt2
    from drand_amd import _lib
    assert _lib.load().dh_init(0) == 0
    res = {"windows": [1 << 20, 1 << 22, 1 << 23], "cases": {}}
    name = "pedersen-bls-chained"
    conv = os.path.join(WORK, "stream_conv_src.db")
    store_replay.build_untrimmed(drand_amd.scheme_from_name(name), store_replay.secret(name), 1 << 20, conv, log)
    rew = os.path.join(WORK, "stream_rew_src.db")
    n = 1 << 23
    write_bolt2(rew, [], rounds=np.arange(1, n + 1, dtype=np.uint64), sigs=source_values(n), page_size=4096)
    dst = os.path.join(WORK, "stream_sweep_dst.db")
    for case, src, fmt, patches in (("convert_1M_untrimmed", conv, "untrimmed", {}), ("rewrite_8M_trimmed", rew, "trimmed", big_patches(n))):
        variants = ([("parent_one_shot", a.parent, None)] if a.parent else []) + [("one_shot", ROOT, None)] + \
                   [("window_%dM" % (w >> 20), ROOT, w) for w in res["windows"]]
        runs = {v[0]: [] for v in variants}
        for _round in range(2):
            for label, tree, window in variants:
                r = run_child(tree, src, dst, fmt, window, patches, 4)
                runs[label].append(r)
                log("%s %s: %s" % (case, label, r.get("error", ["%.4f" % x for x in r["seconds"]])))
        summary = {}
        for label, rs in runs.items():
            warm = [x for r in rs for x in r["seconds"][1:]]
            summary[label] = {"warm_best": min(warm), "warm_all": warm, "cold": [r["seconds"][0] for r in rs if r["seconds"]],
                              "peak_rss_kb": max(r["peak_rss_kb"] for r in rs),
                              "peak_rss_after_open_kb": max(r["peak_rss_after_open_kb"] for r in rs)}
        base = summary.get("parent_one_shot", summary["one_shot"])
        spread = (max(base["warm_all"]) - min(base["warm_all"])) / min(base["warm_all"])
        for label, sm in summary.items():
            sm["over_yardstick"] = sm["warm_best"] / base["warm_best"]
            sm["inside_yardstick_spread"] = sm["warm_best"] <= max(base["warm_all"])
        res["cases"][case] = {"yardstick": "parent_one_shot" if a.parent else "one_shot", "yardstick_spread": spread, "summary": summary,
                              "runs": runs}
    for p in (conv, rew, dst):
        if os.path.exists(p):
            os.remove(p)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["big", "sweep", "_run", "_verify"])
    ap.add_argument("--rounds", type=int, default=1 << 25)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    for k in ("--tree", "--label", "--src", "--dst", "--fmt", "--patches", "--what"):
        ap.add_argument(k, default=None)
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--reps", type=int, default=4)
    a = ap.parse_args()
    if a.mode == "_run":
        return child_run(a)
    if a.mode == "_verify":
        return child_verify(a)
    os.makedirs(WORK, exist_ok=True)
    out = a.out or os.path.join(WORK, "store_stream.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = json.load(open(out)) if os.path.exists(out) else {}  # the two modes share one record
    res[a.mode] = big(a) if a.mode == "big" else sweep(a)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({"store_stream": out, "mode": a.mode}))


if __name__ == "__main__":
    main()
