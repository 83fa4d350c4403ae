"""Shared builders of the store-file cases of tests/test_bolt_host.py (CPU) and tests/test_gpu_bolt.py (GPU): the
same deterministic files on both sides. The CPU test computes the expected faulty sets with check_past_beacons over
BoltTrimmedStore and the oracle and pins them in tests/golden/bolt_cases.json (python tests/bolt_cases.py rewrites
it); the GPU test compares the device path against that record, never against the code under test."""
import hashlib
import json
import os
import struct

from boltwrite2 import write_bolt2

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
CASES_JSON = os.path.join(GOLD, "bolt_cases.json")
REF_TRIMMED = os.path.join(GOLD, "boltdb", "trimmed.db")
SCHEMES = ["pedersen-bls-chained", "pedersen-bls-unchained", "bls-unchained-on-g1", "bls-unchained-g1-rfc9380"]


def key(r):
    return int(r).to_bytes(8, "big")


def rand_bytes(tag, n):
    out = b""
    i = 0
    while len(out) < n:
        out += hashlib.sha256(b"%s-%d" % (tag.encode(), i)).digest()
        i += 1
    return out[:n]


def records(n, vlen=48, tag="rec", first=0):
    return {key(r): rand_bytes("%s%d" % (tag, r), vlen) for r in range(first, first + n)}


# ------------------------------------------------------------------ layout / parity files

def parity_files(tmp):
    """[(id, path)]: every page size, depths 1-3, inline and empty buckets, 64 / 65-element leaves, foreign keys,
    odd value lengths (one on overflow pages) and gaps."""
    out = []

    def add(name, items, **kw):
        path = os.path.join(str(tmp), name + ".db")
        lay = write_bolt2(path, items, **kw)
        out.append((name, path, lay))
        return lay

    out.append(("reference", REF_TRIMMED, None))
    for psz in (512, 1024, 4096, 16384):
        lay = add("p%d" % psz, list(records(300, 48, "p%d" % psz).items()), page_size=psz)
        assert lay["depth"] == (3 if psz == 512 else 2), lay
    assert add("p4096_d1", list(records(5, 48).items()), page_size=4096)["depth"] == 1
    assert add("p4096_d3", list(records(120, 96).items()), page_size=4096, max_leaf=7, max_branch=5)["depth"] == 3
    assert add("p16384_d3", list(records(90, 48).items()), page_size=16384, max_leaf=9, max_branch=4)["depth"] == 3
    assert add("p1024_d3", list(records(200, 48).items()), page_size=1024, max_branch=5)["depth"] == 3
    for n in (0, 1, 5):
        add("inline%d" % n, list(records(n, 48, "in").items()), inline=True)
    add("empty", [])
    for n in (64, 65):  # a wave's worth of elements, and one more
        add("leaf%d" % n, list(records(2 * n, 4, "short").items()), max_leaf=n)
    mixed = dict(records(40, 48, "mix"))
    foreign = [(b"\x00" * 6 + b"\x05", b"seven"), (b"\x00" * 7 + b"\x09\x01", b"nine-byte key"),
               (key(1000), struct.pack("<QQ", 0, 0) + struct.pack("<QHHI", 0, 2, 0, 0), 0x01)]
    add("foreign", list(mixed.items()) + foreign, page_size=1024)
    odd = dict(records(60, 48, "odd"))
    for r, n in ((5, 0), (9, 47), (10, 49), (20, 95), (21, 97), (33, 100), (40, 5000)):
        odd[key(r)] = rand_bytes("oddv%d" % r, n)
    add("oddlens", list(odd.items()))
    gaps = dict(records(80, 48, "gap"))
    for r in (0, 30, 31, 32, 79):
        del gaps[key(r)]
    add("gaps", list(gaps.items()), page_size=512)
    add("live_meta1", list(records(30, 48).items()), page_size=512, live_meta=1)
    return out


def windows(rounds):
    """(first, last) windows for a store holding `rounds` (sorted): whole, past both ends, mid-leaf cuts, inside a
    gap, inverted, past the end."""
    if not rounds:
        return [(0, 5), (3, 2)]
    lo, hi = rounds[0], rounds[-1]
    w = [(0, hi + 3), (lo, hi), (lo + 3, max(lo + 3, hi - 2)), (lo + 1, lo + 1), (hi, hi), (5, 2), (hi + 5, hi + 9)]
    have = set(rounds)
    gap = [r for r in range(lo, hi) if r not in have]
    if gap:
        w.append((gap[0], gap[0]))
        w.append((gap[0] - 2, gap[-1] + 2))
    return w


# ------------------------------------------------------------------ corrupt files

def corrupt_files(tmp):
    """[(id, path)] structurally broken variants of one 512-byte-page, depth-3 file, and the sweep's base."""
    base = os.path.join(str(tmp), "base.db")
    lay = write_bolt2(base, list(records(300, 48, "cor").items()), page_size=512)
    data = open(base, "rb").read()
    P = 512
    leaf, branch, root = lay["leaves"][3] * P, lay["branches"][0] * P, lay["root"] * P
    out = []

    def add(name, patch=None, cut=None):
        b = bytearray(data)
        for off, val in (patch or []):
            b[off:off + len(val)] = val
        if cut is not None:
            b = b[:cut]
        path = os.path.join(str(tmp), name + ".db")
        open(path, "wb").write(bytes(b))
        out.append((name, path))

    add("truncated", cut=len(data) - 300)
    add("count_large", [(leaf + 10, struct.pack("<H", 0xFFFF))])
    add("pos_past", [(leaf + 16 + 4, struct.pack("<I", 0x10000))])
    add("vsize_past", [(leaf + 16 + 12, struct.pack("<I", 0x100000))])
    add("child_past_hw", [(branch + 16 + 8, struct.pack("<Q", lay["pages"] + 5))])
    add("cycle", [(branch + 16 + 8, struct.pack("<Q", lay["root"]))])
    add("metas_bad", [(16, b"\0\0\0\0"), (P + 16, b"\0\0\0\0")])
    add("meta0_bad", [(72, b"\x01\x02\x03\x04")])
    # element 1's key lowered below element 0's: keys descend inside the leaf
    e1 = leaf + 16 + 16
    kpos = e1 + struct.unpack_from("<I", data, e1 + 4)[0]
    add("descending", [(kpos, key(0))])
    add("leaf_flags", [(leaf + 8, struct.pack("<H", 0x10))])
    return out, base, {"leaf": leaf, "branch": branch, "root": root}


# ------------------------------------------------------------------ replay cases over the golden chains

def chain(name):
    c = json.load(open(os.path.join(GOLD, "chains.json")))[name]
    genesis = bytes.fromhex(c["prevs"][0]) if c["prevs"][0] else hashlib.sha256(b"genesis " + name.encode()).digest()
    kv = {key(0): genesis}
    for r, s in zip(c["rounds"], c["sigs"]):
        kv[key(r)] = bytes.fromhex(s)
    return bytes.fromhex(c["pk"]), bytes.fromhex(c["sk"]), kv


def replay_files(tmp, name, oracle):
    """{kind: path} of the store files of one scheme: clean, rm7, swap, odd, mixed."""
    _pk, sk, kv = chain(name)
    chained = name == "pedersen-bls-chained"
    files = {}

    def put(kind, d):
        path = os.path.join(str(tmp), "%s_%s.db" % (name, kind))
        write_bolt2(path, list(d.items()), page_size=512)
        files[kind] = path

    put("clean", kv)
    rm7 = dict(kv)
    del rm7[key(7)]
    put("rm7", rm7)
    swap = dict(kv)
    swap[key(12)], swap[key(13)] = kv[key(13)], kv[key(12)]
    put("swap", swap)
    odd = dict(kv)
    odd[key(10)] = rand_bytes("odd record", len(kv[key(10)]) - 1)
    if chained:  # the chain goes on over the odd record as stored: only round 10 is faulty
        for r in range(11, 25):
            odd[key(r)] = oracle.sign(name, sk, oracle.digest_beacon(name, r, odd[key(r - 1)]))
    put("odd", odd)
    mixed = dict(swap)
    del mixed[key(7)]
    put("mixed", mixed)
    return files


# (kind, up_to, window)
REPLAY_CALLS = [("clean", 1000, 8), ("rm7", 1000, 8), ("rm7", 5, 8), ("rm7", 24, 8), ("rm7", 0, 8), ("swap", 1000, 8),
                ("odd", 1000, 8), ("mixed", 1000, 1), ("mixed", 1000, 8), ("mixed", 1000, 1 << 20), ("mixed", 13, 5)]


def call_id(name, kind, up_to, window):
    return "%s/%s/up_to=%d/window=%d" % (name, kind, up_to, window)


def load_golden():
    return json.load(open(CASES_JSON))


if __name__ == "__main__":  # rewrite tests/golden/bolt_cases.json from the host reader, the oracle and the CPU program
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(HERE)
    sys.path[:0] = [root, os.path.join(root, "oracle")]
    import oracle_ctypes
    import test_bolt_host as host
    oracle_ctypes.lib()
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.check_call(["make", "-s", "_build/bolt_check"], cwd=host.SAN)
        files, _base, _at = corrupt_files(tmp)
        lines = subprocess.check_output([os.path.join(host.SAN, "_build", "bolt_check")] + [p for _n, p in files],
                                        text=True).splitlines()
        gold = {"corrupt": {n: l.split()[0] for (n, _p), l in zip(files, lines)},
                "replay": host.compute_golden(oracle_ctypes, tmp)}
    with open(CASES_JSON, "w") as f:
        json.dump(gold, f, indent=1, sort_keys=True)
        f.write("\n")
