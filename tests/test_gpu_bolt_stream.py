"""GPU: the windowed trimmed-store writer (dh_bolt_writer_*, dh_store_save_trimmed_append, dh_store_split,
store.BoltWriter and the window= arguments).

The invariant under test: for every split of the rows into appends, head || runs || tail is byte for byte the one-shot
image, i.e. what boltwrite2.write_bolt2 lays out. Shapes are those of tests/bolt_write_cases.py (at most 2,500 rows,
page sizes 256-16384) and the 300-round signed stores of tests/test_gpu_bolt_write.py.

* the writer over every case and the windows {records per leaf - 1, records per leaf, + 1, 3, 64, all rows} (1 too for
  cases of at most 300 rows): bytes, contiguous runs from 4 * P, finish's stats;
* boundaries by construction: the 600-byte record first / last / alone in an append at P = 512, zero-length values at
  an edge, an n = 0 append, an append that closes no leaf, strides 48 / 96 / 4 in one file, round 2^64 - 1 last;
* refusals with canary bytes; the writer is unchanged by each and the file still comes out right;
* dh_store_save_trimmed_append over round windows and dh_store_split windows against dh_store_save_trimmed: image and
  unlinked list; the unlinked test across a window boundary; patches at window edges; DH_DEFERRED consumes nothing;
* the one-shot entries under DRANDHIP_STORE_WRITE_WINDOW: same bytes, stats and unlinked lists, and dh_profile counts
  the windows;
* Python: BoltWriter, window= of write_trimmed_bolt / save_trimmed / correct_store_file, replay parity, two threads."""
import ctypes
import json
import os
import threading

import numpy as np
import pytest

import bolt_cases as bc
import bolt_json_cases as jc
import bolt_write_cases as wc
import test_gpu_bolt_write as one
from boltwrite2 import write_bolt2

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
CHAINED = one.CHAINED
ENV = "DRANDHIP_STORE_WRITE_WINDOW"


@pytest.fixture(scope="module")
def dh():
    import torch
    import drand_amd
    from drand_amd import _lib
    torch.zeros(1, device="cuda")
    assert _lib.load().dh_init(0) == 0, _lib.last_error()
    return drand_amd


@pytest.fixture(scope="module")
def signed(oracle, tmp_path_factory):
    """(pk, true sigs, {key: hexjson value}, decoded {round: (signature, previous)}, path at P = 4096, path at P = 256) of
    the chained signed store of tests/test_gpu_bolt_write.py; computed once and not changed."""
    from drand_amd.store import beacon_from_hexjson
    tmp = tmp_path_factory.mktemp("signed_stream")
    pk, sigs, kv = one.signed_store(CHAINED, oracle)
    paths = []
    for P in (4096, 256):
        paths.append(str(tmp / ("chained_p%d.db" % P)))
        write_bolt2(paths[-1], list(kv.items()), page_size=P)
    dec = {}
    for k, v in kv.items():
        b = beacon_from_hexjson(v)
        dec[int.from_bytes(k, "big")] = (b.signature, b.previous_signature)
    return pk, sigs, kv, dec, paths[0], paths[1]


class RawWriter:
    """dh_bolt_writer_* through ctypes; every output buffer carries 16 canary bytes of 0xC3 behind `cap`."""

    def __init__(self, P):
        from drand_amd import _lib
        self.L, self.lib, self.P = _lib, _lib.load(), P
        self.h = ctypes.c_void_p()
        self.rc = self.lib.dh_bolt_writer_open(P, ctypes.byref(self.h))
        self.file = bytearray(4 * P)
        self.next = 4 * P

    def _place(self, off, buf, n):
        assert off == self.next, (off, self.next)  # runs are contiguous and start at 4 * P
        self.file += buf[:n].tobytes()
        self.next += n

    def append(self, rounds, rows, lens, cap=1 << 20, null_out=False):
        """(rc, len_out, stats); the run is placed when rc == 0."""
        import torch
        d_r = torch.from_numpy(np.ascontiguousarray(rounds).view(np.int64)).cuda()
        d_s = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
        d_l = torch.from_numpy(np.ascontiguousarray(lens).view(np.int32)).cuda()
        torch.cuda.synchronize()
        buf = np.full(cap + 16, 0xC3, np.uint8)
        n, off, stats = ctypes.c_size_t(7), ctypes.c_uint64(0), (ctypes.c_uint64 * 3)()
        rc = self.lib.dh_bolt_writer_append_device(self.h, d_r.data_ptr() or None, d_s.data_ptr() or None, rows.shape[1],
                                                   d_l.data_ptr() or None, len(rounds), None if null_out else ctypes.c_void_p(buf.ctypes.data),
                                                   cap, ctypes.byref(n), ctypes.byref(off), stats, None)
        if rc == 0:
            self._place(off.value, buf, n.value)
            assert (buf[n.value:] == 0xC3).all()
        else:
            assert (buf == 0xC3).all(), "a refused append wrote to its output"
        return rc, n.value, [int(x) for x in stats]

    def append_from(self, dev, first, last, patches=(), cap=1 << 20, ucap=64):
        """dh_store_save_trimmed_append with [(round, bytes | None)]: (rc, len_out, unlinked, stats)."""
        k = len(patches)
        stride = max([4] + [len(v) for _r, v in patches if v is not None])
        pr = np.array([r for r, _v in patches], np.uint64).reshape(-1)
        pl = np.array([self.L.DH_PATCH_DELETE if v is None else len(v) for _r, v in patches], np.uint32).reshape(-1)
        ps = np.zeros((k, stride), np.uint8)
        for i, (_r, v) in enumerate(patches):
            if v:
                ps[i, :len(v)] = np.frombuffer(v, np.uint8)
        buf = np.full(cap + 16, 0xC3, np.uint8)
        unl = np.zeros(max(1, ucap), np.uint64)
        n, nu, off, stats = ctypes.c_size_t(7), ctypes.c_size_t(0), ctypes.c_uint64(0), (ctypes.c_uint64 * 6)()
        rc = self.lib.dh_store_save_trimmed_append(dev._h, self.h, first, last, ctypes.c_void_p(pr.ctypes.data), ctypes.c_void_p(ps.ctypes.data),
                                                   stride, ctypes.c_void_p(pl.ctypes.data), k, ctypes.c_void_p(buf.ctypes.data), cap,
                                                   ctypes.byref(n), ctypes.byref(off), ctypes.c_void_p(unl.ctypes.data), ucap,
                                                   ctypes.byref(nu), stats)
        if rc == 0:
            self._place(off.value, buf, n.value)
            assert (buf[n.value:] == 0xC3).all()
        else:
            assert (buf == 0xC3).all(), "a refused append wrote to its output"
        return rc, n.value, [int(x) for x in unl[:min(nu.value, ucap)]], [int(x) for x in stats]

    def finish(self, cap=1 << 20, head=True):
        """(rc, len_out, stats); on success self.file is the whole file."""
        buf = np.full(cap + 16, 0xC3, np.uint8)
        hd = np.full(4 * self.P + 16, 0xC3, np.uint8)
        n, off, stats = ctypes.c_size_t(7), ctypes.c_uint64(0), (ctypes.c_uint64 * 3)()
        rc = self.lib.dh_bolt_writer_finish(self.h, ctypes.c_void_p(buf.ctypes.data), cap, ctypes.byref(n), ctypes.byref(off),
                                            ctypes.c_void_p(hd.ctypes.data) if head else None, stats)
        if rc == 0:
            self._place(off.value, buf, n.value)
            assert (buf[n.value:] == 0xC3).all() and (hd[4 * self.P:] == 0xC3).all()
            self.file[:4 * self.P] = hd[:4 * self.P].tobytes()
        else:
            assert (buf == 0xC3).all() and (hd == 0xC3).all(), "a refused finish wrote to its output"
        return rc, n.value, [int(x) for x in stats]

    def close(self):
        self.lib.dh_bolt_writer_close(self.h)
        self.h = ctypes.c_void_p()


def stream(P, parts):
    """parts: [(rounds, rows, lens)] appended in order -> (file bytes, finish stats, per-append (len, stats))."""
    from drand_amd import _lib
    w = RawWriter(P)
    assert w.rc == 0, _lib.last_error()
    log = []
    try:
        for rounds, rows, lens in parts:
            rc, n, stats = w.append(rounds, rows, lens)
            assert rc == 0, _lib.last_error()
            assert stats[0] == len(rounds) and stats[2] * P == n
            log.append((n, stats))
        rc, _n, stats = w.finish()
        assert rc == 0, _lib.last_error()
        return bytes(w.file), stats, log
    finally:
        w.close()


def cut(cols, window):
    rounds, rows, lens = cols
    return [(rounds[i:i + window], rows[i:i + window], lens[i:i + window]) for i in range(0, len(rounds), window)]


def part(kv):
    """{round: value} -> one append's columns at the stride of its own longest value."""
    return one.columns(kv)


# ------------------------------------------------------------------ 1. the writer over every case

@pytest.mark.parametrize("case", wc.cases(), ids=lambda c: c[0])
def test_writer_every_case(dh, tmp_path, case):
    from drand_amd import _lib
    name, P, kv = case
    want, lay = wc.expected(tmp_path, name, P, kv)
    cols = one.columns(kv)
    rc, size, buf, stats1 = one.raw_write(*cols, P)
    assert rc == 0 and buf[:size].tobytes() == want, _lib.last_error()  # the one-shot call's image
    per = wc.per_leaf(P, 96)
    windows = {max(1, per - 1), per, per + 1, 3, 64, len(kv)}
    if len(kv) <= 300:
        windows.add(1)
    for w in sorted(windows):
        got, stats, log = stream(P, cut(cols, w))
        assert got == want, (name, w)
        assert stats == stats1 == [len(kv), len(lay["leaves"]), lay["pages"]], (name, w)
        assert sum(s[1] for _n, s in log) <= len(lay["leaves"])


# ------------------------------------------------------------------ 2. boundaries, by construction

def test_boundaries(dh, tmp_path):
    P = 512
    base = wc.recs(range(1, 12), 96, "bnd")
    big = bc.rand_bytes("600", 600)
    kv = dict(base)
    kv[6] = big
    want, _lay = one.want_bytes(tmp_path, kv, P, "ovf")
    lo, hi = {r: v for r, v in kv.items() if r < 6}, {r: v for r, v in kv.items() if r > 6}
    # the 600-byte record as the first row of an append, as the last, and alone in one
    for parts in ([lo, {**{6: big}, **hi}], [{**lo, 6: big}, hi], [lo, {6: big}, hi]):
        got, _s, log = stream(P, [part(p) for p in parts])
        assert got == want
    # alone: it is a closed leaf of its own as soon as it arrives, and closes the leaf before it
    _g, _s, log = stream(P, [part(lo), part({6: big})])
    assert log[1][1][1] == 2 and log[1][0] == 3 * P  # rounds 5 (the open leaf) and 6 (two pages)
    # a zero-length value at an edge of an append, and as a whole append
    kv = wc.recs(range(1, 30), 96, "z")
    kv[10] = b""
    kv[11] = b""
    kv[20] = b""
    want, _lay = one.want_bytes(tmp_path, kv, P, "zero")
    a = {r: v for r, v in kv.items() if r <= 10}
    b = {r: v for r, v in kv.items() if 11 <= r <= 19}
    c = {20: b""}
    d = {r: v for r, v in kv.items() if r > 20}
    assert stream(P, [part(a), part(b), part(c), part(d)])[0] == want
    # an n = 0 append in the middle; an append that closes no leaf, followed by one that does
    cols = one.columns(kv)
    empty = (cols[0][:0], cols[1][:0], cols[2][:0])
    got, _s, log = stream(P, [(cols[0][:2], cols[1][:2], cols[2][:2]), empty, (cols[0][2:3], cols[1][2:3], cols[2][2:3]),
                              (cols[0][3:], cols[1][3:], cols[2][3:])])
    assert got == want
    assert [n for n, _s in log[:3]] == [0, 0, 0] and log[1][1] == [0, 0, 0] and log[3][0] > 0
    # strides 48, then 96, then 4 (zero-length values) in successive appends of one file
    kv = {**wc.recs(range(1, 20), 48, "s48"), **wc.recs(range(20, 40), 96, "s96"), **{r: b"" for r in range(40, 70)}}
    want, _lay = one.want_bytes(tmp_path, kv, P, "strides")
    parts = [part({r: v for r, v in kv.items() if r < 20}), part({r: v for r, v in kv.items() if 20 <= r < 40}),
             part({r: v for r, v in kv.items() if r >= 40})]
    assert [p[1].shape[1] for p in parts] == [48, 96, 4]
    assert stream(P, parts)[0] == want
    assert stream(P, [x for p in parts for x in cut(p, 7)])[0] == want
    # round 2^64 - 1 as the last row
    kv = wc.recs(range(1, 9), 96, "top")
    kv[U64] = bc.rand_bytes("last", 96)
    want, _lay = one.want_bytes(tmp_path, kv, 256, "top")
    cols = one.columns(kv)
    assert stream(256, cut(cols, 8))[0] == want and stream(256, cut(cols, 1))[0] == want


# ------------------------------------------------------------------ 3. refusals

def test_refusals_consume_nothing(dh, tmp_path):
    from drand_amd import _lib
    P = 512
    kv = wc.recs(range(1, 60), 96, "ref")
    want, lay = one.want_bytes(tmp_path, kv, P, "ref")
    rounds, rows, lens = one.columns(kv)
    w = RawWriter(P)
    assert w.rc == 0
    try:
        assert w.finish()[0] == _lib.DH_ENOBEACON  # a writer that never received a row
        assert w.append(rounds[:30], rows[:30], lens[:30])[0] == 0
        # the first round equal to the last appended round
        assert w.append(rounds[29:40], rows[29:40], lens[29:40])[0] == _lib.DH_EINVAL
        # a descending pair inside an append
        desc = rounds[30:].copy()
        desc[3], desc[4] = desc[4], desc[3]
        assert w.append(desc, rows[30:], lens[30:])[0] == _lib.DH_EINVAL
        # a length above the stride
        long_ = lens[30:].copy()
        long_[-1] = rows.shape[1] + 1
        assert w.append(rounds[30:], rows[30:], long_)[0] == _lib.DH_EINVAL
        # cap one byte short: the size is reported; cap 0 sizes; a null out with a nonzero cap
        rc, need, _s = w.append(rounds[30:], rows[30:], lens[30:], cap=0)
        assert rc == _lib.DH_EINVAL and need > 0 and need % P == 0
        rc, n, _s = w.append(rounds[30:], rows[30:], lens[30:], cap=need - 1)
        assert rc == _lib.DH_EINVAL and n == need
        assert w.append(rounds[30:], rows[30:], lens[30:], cap=need, null_out=True)[0] == _lib.DH_EINVAL
        # the correct append and finish still produce the expected bytes
        rc, n, _s = w.append(rounds[30:], rows[30:], lens[30:], cap=need)
        assert rc == 0 and n == need, _lib.last_error()
        rc, tail, _s = w.finish(cap=0)
        assert rc == _lib.DH_EINVAL and tail > 0
        assert w.finish(cap=tail - 1)[:2] == (_lib.DH_EINVAL, tail)
        assert w.finish(cap=tail, head=False)[0] == _lib.DH_EINVAL
        rc, n, stats = w.finish(cap=tail)
        assert rc == 0 and n == tail and stats == [len(kv), len(lay["leaves"]), lay["pages"]], _lib.last_error()
        assert bytes(w.file) == want
        assert w.append(rounds[:0], rows[:0], lens[:0])[0] == _lib.DH_EINVAL  # finished
    finally:
        w.close()
    bad = RawWriter(100)  # a page size of 100
    assert bad.rc == _lib.DH_EINVAL and not bad.h


# ------------------------------------------------------------------ 4. dh_store_save_trimmed_append

def save_windows(dev, P, windows, patches=()):
    """The windows [(first, last)] of an open store through one writer: (file bytes, unlinked, finish stats)."""
    from drand_amd import _lib
    w = RawWriter(P)
    assert w.rc == 0
    unlinked = []
    try:
        for lo, hi in windows:
            rc, _n, unl, _s = w.append_from(dev, lo, hi, [(r, v) for r, v in patches if lo <= r <= hi])
            assert rc == 0, (lo, hi, _lib.last_error())
            unlinked += unl
        rc, _n, stats = w.finish()
        assert rc == 0, _lib.last_error()
        return bytes(w.file), unlinked, stats
    finally:
        w.close()


def round_windows(step, last=300):
    out = [(lo, min(lo + step - 1, last)) for lo in range(0, last + 1, step)]
    return out[:-1] + [(out[-1][0], U64)]


def test_store_append_equals_save_trimmed(dh, signed, tmp_path):
    from drand_amd import _lib
    from drand_amd.store import DeviceBoltStore
    _pk, sigs, _kv, dec, src, src256 = signed
    with DeviceBoltStore(src, True, fmt="untrimmed") as dev:
        rc, n, buf, unl1, stats1 = one.raw_save(dev, [], P=512)
        assert rc == 0, _lib.last_error()
        want = buf[:n].tobytes()
        assert want == one.want_bytes(tmp_path, {r: v[0] for r, v in dec.items()}, 512)[0]
        assert unl1 == one.unlinked_by_definition(dec)
        for step in (1, 7, 50, 1000):
            got, unl, stats = save_windows(dev, 512, round_windows(step))
            assert got == want and unl == unl1 and stats == stats1[:3], step
        # the unlinked test across a window boundary. Unlinked as the first row of a window, because the row before it
        # was deleted by a patch of the window before ...
        for patches, boundary, linked in (([(49, None)], 50, False), ([(one.CORRUPT, sigs[one.CORRUPT])], one.CORRUPT + 1, True)):
            rc, n, buf, unl1, _s = one.raw_save(dev, patches, P=512)
            assert rc == 0
            got, unl, _s = save_windows(dev, 512, [(0, boundary - 1), (boundary, U64)], patches)
            assert got == buf[:n].tobytes() and unl == unl1
            assert (boundary not in unl) == linked  # ... and linked only because a patch of the window before replaced it
    with DeviceBoltStore(src256, True, fmt="untrimmed") as dev:  # every record a leaf of its own
        rc, n, buf, unl1, stats1 = one.raw_save(dev, [], P=256)
        assert rc == 0
        for max_rows in (1, 40):
            windows = dev.split(0, U64, max_rows)
            assert windows[0][0] == 0 and windows[-1][1] == U64
            assert all(a[1] + 1 == b[0] for a, b in zip(windows, windows[1:]))
            assert len(windows) == -(-len(dec) // max_rows)
            got, unl, stats = save_windows(dev, 256, windows)
            assert got == buf[:n].tobytes() and unl == unl1 and stats == stats1[:3]
        # too little room: the count needed
        lib, cnt = _lib.load(), ctypes.c_size_t(0)
        out = np.zeros(8, np.uint64)
        assert lib.dh_store_split(dev._h, 0, U64, 40, ctypes.c_void_p(out.ctypes.data), 3, ctypes.byref(cnt)) == _lib.DH_EINVAL
        assert cnt.value == len(windows) and not out.any()
        assert dev.split(5, 4, 10) == []


@pytest.mark.parametrize("fmt", ["trimmed", "untrimmed"])
def test_store_append_patches_at_window_edges(dh, tmp_path, fmt):
    from drand_amd import _lib
    from drand_amd.store import DeviceBoltStore
    base = wc.recs([r for r in range(10, 30) if r != 20], 96, "edge")
    src = str(tmp_path / "src.db")
    if fmt == "trimmed":
        write_bolt2(src, [(bc.key(r), v) for r, v in base.items()], page_size=512)
    else:
        write_bolt2(src, [(bc.key(r), jc.marshal(r, v, None)) for r, v in base.items()], page_size=512)
    new = {r: bc.rand_bytes("new%d" % r, n) for r, n in ((2, 96), (14, 100), (20, 48), (24, 96), (40, 96))}
    # windows (0, 14), (15, 24), (25, U64): insert below the first stored round, replace at the end of a window, delete
    # at the start of one, insert and replace at its end, delete at the start of the last, insert above the last round
    patches = sorted({2: new[2], 14: new[14], 15: None, 20: new[20], 24: new[24], 25: None, 40: new[40]}.items())
    edited = dict(base)
    del edited[15], edited[25]
    edited.update(new)
    with DeviceBoltStore(src, False, fmt=fmt) as dev:
        rc, n, buf, _u, stats1 = one.raw_save(dev, patches, P=512)
        assert rc == 0 and buf[:n].tobytes() == one.want_bytes(tmp_path, edited, 512)[0], _lib.last_error()
        got, unl, stats = save_windows(dev, 512, [(0, 14), (15, 24), (25, U64)], patches)
        assert got == buf[:n].tobytes() and unl == [] and stats == stats1[:3]
        # a window that produces no row: an empty range, and everything deleted
        w = RawWriter(512)
        try:
            assert w.append_from(dev, 0, 9)[:2] == (0, 0)
            assert w.append_from(dev, 10, 11, [(10, None), (11, None)])[:2] == (0, 0)
            assert w.finish()[0] == _lib.DH_ENOBEACON
            assert w.append_from(dev, 12, U64)[0] == 0
            assert w.append_from(dev, 12, U64)[0] == _lib.DH_EINVAL  # not above the rounds appended
            assert w.finish()[0] == 0
            assert bytes(w.file) == one.want_bytes(tmp_path, {r: v for r, v in base.items() if r >= 12}, 512, "tail")[0]
        finally:
            w.close()


def test_store_append_deferred_and_fixture(dh, tmp_path):
    from drand_amd import _lib
    from drand_amd.store import DeviceBoltStore, beacon_from_hexjson
    kv = jc.synth(40, 96, True, "defer")
    _what, make = jc.DEFERRED_VALUES[0]
    kv[bc.key(9)] = make(9)
    src = str(tmp_path / "one.db")
    write_bolt2(src, list(kv.items()), page_size=1024)
    fill = bc.rand_bytes("fill", 96)
    with DeviceBoltStore(src, True, fmt="untrimmed") as dev:
        rc, n, buf, unl1, _s = one.raw_save(dev, [(9, fill)], P=1024)
        assert rc == 0
        w = RawWriter(1024)
        try:
            assert w.append_from(dev, 0, 5)[0] == 0
            before = (bytes(w.file), w.next)
            assert w.append_from(dev, 6, 20)[0] == _lib.DH_DEFERRED  # no patch covers record 9
            assert w.append_from(dev, 6, 20, [(8, fill)])[0] == _lib.DH_DEFERRED
            assert (bytes(w.file), w.next) == before
            rc, _n, unl, _s = w.append_from(dev, 6, 20, [(9, fill)])
            assert rc == 0 and unl == [10], _lib.last_error()
            rc, _n, unl2, _s = w.append_from(dev, 21, U64, ucap=0)
            assert rc == 0 and unl2 == []
            assert w.finish()[0] == 0
            assert bytes(w.file) == buf[:n].tobytes() and unl1 == [10]
        finally:
            w.close()
        # an unlinked list that does not fit: the number comes back and nothing is consumed
        w = RawWriter(1024)
        try:
            rc, _n, unl, stats = w.append_from(dev, 0, U64, [(9, fill)], ucap=0)
            assert rc == _lib.DH_EINVAL and w.next == 4 * 1024
            assert w.append_from(dev, 0, U64, [(9, fill)])[0] == 0 and w.finish()[0] == 0
            assert bytes(w.file) == buf[:n].tobytes()
        finally:
            w.close()
    dec = {int.from_bytes(k, "big"): beacon_from_hexjson(v).signature for k, v in kv.items() if k != bc.key(9)}
    dec[9] = fill
    assert buf[:n].tobytes() == one.want_bytes(tmp_path, dec, 1024)[0]
    # the reference's trimmed fixture, round-tripped in windows
    with DeviceBoltStore(jc.REF_TRIMMED, True) as dev:
        rc, n, buf, _u, stats1 = one.raw_save(dev, [], P=256)
        assert rc == 0
        for windows in (dev.split(0, U64, 10), [(0, 9), (10, 19), (20, 29), (30, U64)]):
            got, unl, stats = save_windows(dev, 256, windows)
            assert got == buf[:n].tobytes() and unl == [] and stats == stats1[:3] and stats[0] == 46
    wc.check_image(got)


# ------------------------------------------------------------------ 5. the one-shot entries under DRANDHIP_STORE_WRITE_WINDOW

def profile_of(lib, fn):
    assert lib.dh_profile(1) == 0
    try:
        res = fn()
        buf = ctypes.create_string_buffer(1 << 16)
        lib.dh_profile_read(buf, len(buf))
        return res, json.loads(buf.value.decode())
    finally:
        lib.dh_profile(0)


@pytest.fixture
def window_env():
    old = os.environ.pop(ENV, None)
    yield lambda v: os.environ.__setitem__(ENV, str(v)) if v is not None else os.environ.pop(ENV, None)
    os.environ.pop(ENV, None)
    if old is not None:
        os.environ[ENV] = old


def test_one_shot_entries_in_windows(dh, signed, tmp_path, window_env):
    from drand_amd import _lib
    from drand_amd.store import DeviceBoltStore
    lib = _lib.load()
    cases = {c[0]: c for c in wc.cases()}
    for name, window, kv, P in (("sixty", 1, wc.recs(range(1, 61), 96, "sixty"), 512), ("mixed_p512", 5, cases["mixed_p512"][2], 512),
                                ("depth3_p512", 64, cases["depth3_p512"][2], 512), ("depth3_p512", -3, cases["depth3_p512"][2], 512)):
        cols = one.columns(kv)
        want, _lay = one.want_bytes(tmp_path, kv, P, "w_" + name)
        window_env(None)
        (rc, size, buf, stats1), prof = profile_of(lib, lambda: one.raw_write(*cols, P, cap=len(want)))  # one library call
        assert rc == 0 and buf[:size].tobytes() == want
        assert prof["bolt_write_window"]["count"] == 1
        window_env(window)
        (rc, size, buf, stats), prof = profile_of(lib, lambda: one.raw_write(*cols, P, cap=len(want), canary=16))
        assert rc == 0 and size == len(want) and buf[:size].tobytes() == want and stats == stats1, (name, _lib.last_error())
        assert (buf[size:] == 0xC3).all()
        assert prof["bolt_write_window"]["count"] == (-(-len(kv) // window) if window >= 1 else 1)  # values below 1 are ignored
        # the sizing protocol: one byte short, nothing written
        rc, size, buf, stats = one.raw_write(*cols, P, cap=len(want) - 1, canary=16)
        assert rc == _lib.DH_EINVAL and size == len(want) and (buf == 0xC3).all() and stats == stats1
    _pk, sigs, _kv, _dec, src, _src256 = signed
    patches = [(one.CORRUPT, sigs[one.CORRUPT]), (one.MISSING, sigs[one.MISSING]), (one.MISSING2, None)]
    with DeviceBoltStore(src, True, fmt="untrimmed") as dev:
        window_env(None)
        (rc, n, buf, unl1, stats1), prof = profile_of(lib, lambda: one.raw_save(dev, patches, P=512))
        assert rc == 0 and prof["store_save_window"]["count"] == 1
        want = buf[:n].tobytes()
        for window in (5, 64):
            window_env(window)
            (rc, n, buf, unl, stats), prof = profile_of(lib, lambda: one.raw_save(dev, patches, P=512))
            assert rc == 0 and buf[:n].tobytes() == want and (buf[n:] == 0xC3).all(), _lib.last_error()
            assert unl == unl1 and stats == stats1
            assert prof["store_save_window"]["count"] == len(dev.split(0, U64, window)) > 1
            rc, n, buf, _u, stats = one.raw_save(dev, patches, P=512, cap=len(want) - 1)
            assert rc == _lib.DH_EINVAL and n == len(want) and (buf == 0xC3).all() and stats == stats1
            rc, n, buf, _u, stats = one.raw_save(dev, patches, P=512, ucap=1)
            assert rc == _lib.DH_EINVAL and n == len(want) and (buf == 0xC3).all() and stats == stats1


# ------------------------------------------------------------------ 6. Python

def test_bolt_writer_python(dh, tmp_path):
    from drand_amd.store import BoltWriter, write_trimmed_bolt
    kv = wc.recs(range(1, 200), 48, "py")
    kv[7] = kv[7][:31]
    want, lay = one.want_bytes(tmp_path, kv, 512)
    rounds, rows, lens = one.columns(kv)
    out = str(tmp_path / "w.db")
    with BoltWriter(out, 512) as w:
        for i in range(0, len(rounds), 23):
            res = w.append(rounds[i:i + 23], rows[i:i + 23], lens[i:i + 23])
            assert res["rows"] == len(rounds[i:i + 23])
        assert os.path.exists(out + ".tmp") and not os.path.exists(out)
        stats = w.finish()
    assert stats == {"rows": len(kv), "leaves": len(lay["leaves"]), "pages": lay["pages"]}
    assert open(out, "rb").read() == want and not os.path.exists(out + ".tmp")
    # an exception inside the block, and a block left without finish(): no .tmp, no file
    for fail in (True, False):
        gone = str(tmp_path / ("gone%d.db" % fail))
        try:
            with BoltWriter(gone, 512) as w:
                w.append(rounds[:50], rows[:50], lens[:50])
                if fail:
                    w.append(rounds[10:20], rows[10:20], lens[10:20])  # not ascending: ValueError
        except ValueError:
            assert fail
        assert not os.path.exists(gone) and not os.path.exists(gone + ".tmp")
    # a rename that fails (the path is a directory) is an exception like any other: the .tmp goes
    isdir = tmp_path / "isdir.db"
    isdir.mkdir()
    with pytest.raises(OSError):
        with BoltWriter(str(isdir), 512) as w:
            w.append(rounds[:50], rows[:50], lens[:50])
            w.finish()
    assert isdir.is_dir() and not os.path.exists(str(isdir) + ".tmp")
    # write_trimmed_bolt(window=) is the unwindowed call
    a, b = str(tmp_path / "a.db"), str(tmp_path / "b.db")
    assert write_trimmed_bolt(a, rounds, rows, lens, page_size=512) == write_trimmed_bolt(b, rounds, rows, lens, page_size=512, window=5)
    assert open(a, "rb").read() == open(b, "rb").read() == want


def test_windowed_save_and_repair_python(dh, oracle, signed, tmp_path):
    from drand_amd.store import BoltTrimmedStore, DeviceBoltStore
    from drand_amd.sync import check_past_beacons, correct_store_file
    from test_readers import OracleScheme
    pk, sigs, _kv, _dec, src, _src256 = signed
    s = dh.scheme_from_name(CHAINED)
    a, b = str(tmp_path / "a.db"), str(tmp_path / "b.db")
    patches = {one.SHORT: sigs[one.SHORT], one.MISSING: sigs[one.MISSING], 7: None}
    with DeviceBoltStore(src, True, fmt="auto") as dev:
        res_a = dev.save_trimmed(a, patches=patches, page_size=512)
        from drand_amd import _lib
        res_b, prof = profile_of(_lib.load(), lambda: dev.save_trimmed(b, patches=patches, page_size=512, window=7))
        # every window is gathered and merged once: the run buffer is reserved, no window is sized by a refused call
        assert prof["store_save_merge"]["count"] == prof["store_save_window"]["count"] == len(dev.split(0, U64, 7)) > 10
        assert res_a == res_b and res_a["unlinked"] == sorted(res_a["unlinked"]) and len(res_a["unlinked"]) > 2
        assert open(a, "rb").read() == open(b, "rb").read()
        with pytest.raises(ValueError):
            dev.save_trimmed(src, window=7)  # the same-file refusal stays
    # replay parity on the windowed result
    UP_TO = 45  # past the corrupted and the wrong-PreviousSig record; the host replay verifies each round on the CPU
    with DeviceBoltStore(b, True) as conv:
        faulty_dev = check_past_beacons(conv, s, pk, UP_TO)
    assert faulty_dev == check_past_beacons(BoltTrimmedStore(b, True), OracleScheme(oracle, CHAINED), pk, UP_TO)
    assert one.CORRUPT in faulty_dev
    # correct_store_file(window=)
    stored = {r: sigs[r] for r in range(one.N_ROUNDS + 1)}
    x = bytearray(sigs[33])
    x[5] ^= 0x10
    stored[33] = bytes(x)
    del stored[222]
    bad = str(tmp_path / "bad.db")
    write_bolt2(bad, [(bc.key(r), v) for r, v in stored.items()])
    r1 = correct_store_file(bad, a, s, pk, lambda r: sigs[r], fmt="auto")
    r2 = correct_store_file(bad, b, s, pk, lambda r: sigs[r], fmt="auto", window=50)
    assert r1 == r2 == ([33, 34, 222, 223], [], [])
    assert open(a, "rb").read() == open(b, "rb").read() == one.want_bytes(tmp_path, {r: sigs[r] for r in stored | {222: b""}})[0]


def test_two_threads_a_writer_each(dh, tmp_path):
    from drand_amd.store import BoltWriter
    jobs = []
    for i, (vlen, P) in enumerate(((48, 512), (96, 256))):
        kv = wc.recs(range(1, 400), vlen, "th%d" % i)
        jobs.append((i, one.columns(kv), P, one.want_bytes(tmp_path, kv, P, "th%d" % i)[0]))
    errs = []

    def work(i, cols, P, want):
        try:
            out = str(tmp_path / ("th%d_out.db" % i))
            for _ in range(3):
                with BoltWriter(out, P) as w:
                    for part_ in cut(cols, 37):
                        w.append(*part_)
                    w.finish()
                assert open(out, "rb").read() == want
        except Exception as e:  # noqa: BLE001 - reported below
            errs.append((i, repr(e)))

    ths = [threading.Thread(target=work, args=j) for j in jobs]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs, errs
