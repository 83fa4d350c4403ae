"""Test helper: write bbolt (format v2) files of any shape, so that the store readers can be tested on page sizes,
tree depths and oddities that tests/boltwrite.py (one branch page, 4 KiB pages) cannot produce.

write_bolt2(path, items, ...) lays out: pages 0/1 meta, 2 freelist (empty), 3 the root bucket's leaf holding the bucket
entry, then the bucket's own pages: leaves in key order (a value that does not fit a page gets a leaf with overflow
pages), then branch levels up to one root. Options: page_size; max_leaf / max_branch (elements per page, to force a
depth with few records); inline (the bucket is one page image inside its bucket value, root pgid 0); live_meta (which
meta page carries the larger txid); items may carry element flags (0x01 = nested bucket) and keys of any length.
write_bolt2(path, rounds=..., sigs=...) is the vectorised form for large uniform stores (numpy arrays: ascending
rounds, one fixed-length value each): a 1M-round file in about a second. Its `items` are records that sort before
them (the genesis record, whose value has another length) and get leaves of their own.
Returns the layout {"page_size", "leaves": [pgid], "branches": [pgid], "root": pgid, "depth", "pages"}."""
import struct

import numpy as np


def fnv64a(b):
    h = 0xcbf29ce484222325
    for x in b:
        h ^= x
        h = (h * 0x100000001b3) & 0xffffffffffffffff
    return h


def meta_page(pgid, page_size, root, freelist, hw, txid):
    m = struct.pack("<IIII", 0xED0CDAED, 2, page_size, 0) + struct.pack("<QQQQQ", root, 0, freelist, hw, txid)
    return (struct.pack("<QHHI", pgid, 0x04, 0, 0) + m + struct.pack("<Q", fnv64a(m))).ljust(page_size, b"\0")


def leaf_image(pgid, items, overflow=0):
    """Header + elements + data of a leaf (unpadded). items: (key, value, flags)."""
    n = len(items)
    elems, data = [], []
    pos_data = 16 * n
    dlen = 0
    for i, (k, v, fl) in enumerate(items):
        elems.append(struct.pack("<IIII", fl, pos_data + dlen - 16 * i, len(k), len(v)))
        data.append(k + v)
        dlen += len(k) + len(v)
    return struct.pack("<QHHI", pgid, 0x02, n, overflow) + b"".join(elems) + b"".join(data)


def branch_image(pgid, children):
    n = len(children)
    elems, data, dlen = [], [], 0
    for i, (k, child) in enumerate(children):
        elems.append(struct.pack("<IIQ", 16 * n + dlen - 16 * i, len(k), child))
        data.append(k)
        dlen += len(k)
    return struct.pack("<QHHI", pgid, 0x01, n, 0) + b"".join(elems) + b"".join(data)


def _norm(items):
    out = []
    for it in items:
        k, v = bytes(it[0]), bytes(it[1])
        out.append((k, v, it[2] if len(it) > 2 else 0))
    return sorted(out, key=lambda t: t[0])


def _split_leaves(items, page_size, max_leaf):
    groups, cur, size = [], [], 16
    for it in items:
        need = 16 + len(it[0]) + len(it[1])
        if cur and (size + need > page_size or (max_leaf and len(cur) >= max_leaf)):
            groups.append(cur)
            cur, size = [], 16
        cur.append(it)
        size += need
    groups.append(cur)
    return groups


def _uniform_leaves(rounds, sigs, page_size, first_pgid):
    """Vectorised leaves of fixed-length records: (bytes of the full leaves, [(first key, pgid)], the rest as items)."""
    n, L = sigs.shape
    per = (page_size - 16) // (24 + L)
    nfull = n // per
    arr = np.zeros((nfull, page_size), np.uint8)
    hdr = np.zeros(nfull, dtype=[("id", "<u8"), ("flags", "<u2"), ("count", "<u2"), ("ov", "<u4")])
    hdr["id"] = first_pgid + np.arange(nfull, dtype=np.uint64)
    hdr["flags"], hdr["count"] = 2, per
    arr[:, :16] = hdr.view(np.uint8).reshape(nfull, 16)
    j = np.arange(per, dtype=np.uint32)
    el = np.zeros(per, dtype=[("fl", "<u4"), ("pos", "<u4"), ("ks", "<u4"), ("vs", "<u4")])
    el["pos"], el["ks"], el["vs"] = 16 * (per - j) + j * (8 + L), 8, L
    arr[:, 16:16 + 16 * per] = el.view(np.uint8)
    keys = np.ascontiguousarray(rounds[:nfull * per]).astype(">u8").view(np.uint8).reshape(nfull, per, 8)
    d0 = 16 + 16 * per
    data = arr[:, d0:d0 + per * (8 + L)].reshape(nfull, per, 8 + L)
    data[:, :, :8] = keys
    data[:, :, 8:] = sigs[:nfull * per].reshape(nfull, per, L)
    heads = [(keys[i, 0].tobytes(), first_pgid + i) for i in range(nfull)]
    rest = [(int(r).to_bytes(8, "big"), s.tobytes(), 0) for r, s in zip(rounds[nfull * per:], sigs[nfull * per:])]
    return arr.tobytes(), heads, rest


def write_bolt2(path, items=None, *, rounds=None, sigs=None, page_size=4096, max_leaf=None, max_branch=None, inline=False,
                live_meta=0, bucket=b"beacons"):
    P = page_size
    blobs = []  # (pgid, bytes spanning whole pages), consecutive from page 4
    nxt = 4
    level = []  # (first key, pgid) of the current level
    leaves, branches = [], []
    if rounds is not None:
        for grp in (_split_leaves(_norm(items), P, max_leaf) if items else []):
            img = leaf_image(nxt, grp)
            assert len(img) <= P
            blobs.append(img.ljust(P, b"\0"))
            level.append((grp[0][0], nxt))
            leaves.append(nxt)
            nxt += 1
        blob, heads, rest = _uniform_leaves(np.asarray(rounds, np.uint64), np.asarray(sigs, np.uint8), P, nxt)
        if heads:
            blobs.append(blob)
            level += heads
            leaves += [pg for _, pg in heads]
            nxt += len(heads)
        items = [rest] if rest else []
    else:
        items = _norm(items)
        if inline:
            items_inline, items = items, []
        else:
            items = _split_leaves(items, P, max_leaf)
    for grp in items:
        img = leaf_image(nxt, grp)
        span = max(1, -(-len(img) // P))
        if span > 1:
            img = leaf_image(nxt, grp, span - 1)
        blobs.append(img.ljust(span * P, b"\0"))
        level.append((grp[0][0] if grp else b"", nxt))
        leaves.append(nxt)
        nxt += span
    depth = 1
    fan = max_branch or (P - 16) // 24
    while len(level) > 1:
        up = []
        for i in range(0, len(level), fan):
            kids = level[i:i + fan]
            img = branch_image(nxt, kids)
            assert len(img) <= P, "branch overflow"
            blobs.append(img.ljust(P, b"\0"))
            up.append((kids[0][0], nxt))
            branches.append(nxt)
            nxt += 1
        level = up
        depth += 1
    if inline:
        value = struct.pack("<QQ", 0, 0) + leaf_image(0, items_inline)
        root = 0
    else:
        root = level[0][1]
        value = struct.pack("<QQ", root, 0)
    top = leaf_image(3, [(bucket, value, 0x01)])
    assert len(top) <= P, "root bucket page overflow"
    hw = nxt
    tx = (3, 2) if live_meta == 0 else (2, 3)
    with open(path, "wb") as f:
        f.write(meta_page(0, P, 3, 2, hw, tx[0]))
        f.write(meta_page(1, P, 3, 2, hw, tx[1]))
        f.write(struct.pack("<QHHI", 2, 0x10, 0, 0).ljust(P, b"\0"))
        f.write(top.ljust(P, b"\0"))
        for b in blobs:
            f.write(b)
    return {"page_size": P, "leaves": leaves, "branches": branches, "root": root, "depth": depth, "pages": hw}
