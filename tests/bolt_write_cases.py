"""Shared by tests/test_bolt_write_host.py (CPU) and tests/test_gpu_bolt_write.py (GPU): the case list of the
trimmed-store writer, each case {round: value} with a page size, and check_image, a structural
restatement of bbolt's consistency walk. The expected bytes of a case are what boltwrite2.write_bolt2 writes for it."""
import struct

import bolt_cases as bc
from boltwrite2 import fnv64a, write_bolt2

U64 = (1 << 64) - 1


def recs(rounds, vlen, tag):
    return {int(r): bc.rand_bytes("%s%d" % (tag, r), vlen) for r in rounds}


def per_leaf(P, vlen):
    return (P - 16) // (24 + vlen)


def cases():
    """[(id, page size, {round: value})]"""
    out = []
    for P in (256, 512, 4096, 16384):
        out.append(("one_p%d" % P, P, recs([7], 96, "one")))
        for L in (48, 96):
            full = per_leaf(P, L)
            out.append(("full%d_p%d" % (L, P), P, recs(range(1, full + 1), L, "f")))
            out.append(("full%d+1_p%d" % (L, P), P, recs(range(1, full + 2), L, "g")))
        # a 32-byte genesis value ahead of 96-byte records, a 95-byte and a zero-length value, gaps, the largest round
        mixed = recs(range(1, 40), 96, "m%d" % P)
        mixed[0] = bc.rand_bytes("genesis", 32)
        mixed[11] = bc.rand_bytes("odd", 95)
        mixed[12] = b""
        for r in (5, 20, 21, 22):
            del mixed[r]
        mixed[1000] = bc.rand_bytes("far", 96)
        mixed[U64] = bc.rand_bytes("last", 96)
        out.append(("mixed_p%d" % P, P, mixed))
    big = recs(range(1, 12), 96, "big")
    big[6] = bc.rand_bytes("600", 600)  # at 512: an overflow leaf with fitting records before and after it
    out.append(("overflow_p512", 512, big))
    only = {3: bc.rand_bytes("only", 600)}
    out.append(("overflow_only_p256", 256, only))
    out.append(("depth3_p512", 512, recs(range(0, 130), 96, "d3")))
    out.append(("depth4_p512", 512, recs(range(0, 2500), 96, "d4")))
    return out


DEPTHS = {"depth3_p512": 3, "depth4_p512": 4}


def expected(tmp, name, P, kv):
    """(bytes, layout) of write_bolt2 for the case."""
    path = str(tmp / ("want_%s.db" % name.replace("+", "p")))
    lay = write_bolt2(path, [(bc.key(r), v) for r, v in kv.items()], page_size=P)
    return open(path, "rb").read(), lay


# ------------------------------------------------------------------ the consistency walk

def check_image(data):
    """Every page below the high-water mark is reached exactly once from the live meta, or is a meta page, the freelist
    page or a page the freelist names free; keys ascend; a branch key equals the first key of its child; extents lie
    inside the file; the meta checksums are right. Returns {"page_size", "pages", "depth", "records"} (depth and
    records of the beacons bucket)."""
    P = struct.unpack_from("<I", data, 24)[0]
    assert P >= 256 and P & (P - 1) == 0 and len(data) % P == 0, P
    metas = []
    for pg in (0, 1):
        off = pg * P
        pid, flags, _c, _o = struct.unpack_from("<QHHI", data, off)
        magic, ver, psz, mflags = struct.unpack_from("<IIII", data, off + 16)
        root, seq, freelist, hw, txid, cks = struct.unpack_from("<QQQQQQ", data, off + 32)
        assert pid == pg and flags & 0x04 and magic == 0xED0CDAED and ver == 2 and psz == P, ("meta", pg)
        assert cks == fnv64a(data[off + 16:off + 72]), ("meta checksum", pg)
        metas.append({"root": root, "freelist": freelist, "hw": hw, "txid": txid})
    m = max(metas, key=lambda t: t["txid"])
    hw = m["hw"]
    assert hw * P <= len(data), "high-water mark beyond the file"
    owner = {0: "meta", 1: "meta"}

    def claim(pgid, what):
        assert 2 <= pgid < hw, (what, pgid)
        off = pgid * P
        span = struct.unpack_from("<I", data, off + 12)[0] + 1
        assert pgid + span <= hw and (pgid + span) * P <= len(data), ("extent", what, pgid)
        assert struct.unpack_from("<Q", data, off)[0] == pgid, ("page id", pgid)
        for p in range(pgid, pgid + span):
            assert p not in owner, ("page reached twice", p, what, owner.get(p))
            owner[p] = what
        return off, span * P

    # the freelist page and the pages it names
    off, ext = claim(m["freelist"], "freelist")
    _, flags, count, _ = struct.unpack_from("<QHHI", data, off)
    assert flags & 0x10
    ids_at = off + 16
    if count == 0xFFFF:
        count = struct.unpack_from("<Q", data, ids_at)[0]
        ids_at += 8
    assert ids_at + 8 * count <= off + ext
    for p in struct.unpack_from("<%dQ" % count, data, ids_at):
        assert 2 <= p < hw and p not in owner, ("free page", p)
        owner[p] = "free"

    def walk(pgid, depth, out):
        """Appends (key, value, flags) of the leaves under pgid; returns (first key, depth below)."""
        off, ext = claim(pgid, "tree")
        _, flags, count, _ = struct.unpack_from("<QHHI", data, off)
        assert 16 + 16 * count <= ext
        if flags & 0x02:
            first = None
            for i in range(count):
                e = off + 16 + 16 * i
                fl, pos, ks, vs = struct.unpack_from("<IIII", data, e)
                assert e + pos + ks + vs <= off + ext and pos >= 16 * (count - i), ("element", pgid, i)
                k = bytes(data[e + pos:e + pos + ks])
                out.append((k, bytes(data[e + pos + ks:e + pos + ks + vs]), fl))
                first = k if first is None else first
            return first, 1
        assert flags & 0x01 and count > 0, ("flags", pgid, flags)
        first, deep = None, 0
        for i in range(count):
            e = off + 16 + 16 * i
            pos, ks, child = struct.unpack_from("<IIQ", data, e)
            assert e + pos + ks <= off + ext
            k = bytes(data[e + pos:e + pos + ks])
            ck, d = walk(child, depth + 1, out)
            assert ck == k, ("branch key is not the first key of its child", pgid, i)
            assert deep in (0, d), "leaves at different depths"
            deep = d
            first = k if first is None else first
        return first, deep + 1

    def ascending(items):
        keys = [k for k, _v, _f in items]
        assert all(a < b for a, b in zip(keys, keys[1:])), "keys do not ascend"

    top = []
    walk(m["root"], 0, top)
    ascending(top)
    info = {"page_size": P, "pages": hw, "depth": 0, "records": []}
    for k, v, fl in top:
        if not fl & 0x01:
            continue
        broot = struct.unpack_from("<Q", v)[0]
        if broot == 0:  # an inline bucket lives inside its value
            continue
        items = []
        _first, depth = walk(broot, 0, items)
        ascending(items)
        assert not any(f & 0x01 for _k, _v, f in items)
        if k == b"beacons":
            info["depth"], info["records"] = depth, [(kk, vv) for kk, vv, _f in items]
    missing = [p for p in range(hw) if p not in owner]
    assert not missing, ("pages below the high-water mark that nothing reaches", missing[:8])
    return info
