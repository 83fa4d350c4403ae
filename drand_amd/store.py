"""Chain readers for batch replay: bbolt beacon stores and hexjson beacon records,
ingested into the columnar arrays dh_verify_batch takes.

* A minimal read-only bbolt (go.etcd.io/bbolt, file format v2) reader: meta pages 0/1 (the valid one with the
  larger txid), branch / leaf pages, nested and inline buckets, overflow pages.
* BoltTrimmedStore — the trimmed layout (/root/reference/chain/boltdb/trimmed.go:87-107,156-193): bucket
  "beacons", key = round as 8-byte big-endian (chain.RoundToBytes, /root/reference/chain/store.go:82-87),
  value = raw signature; for chained schemes Get(r) takes PreviousSig from the stored signature of r-1.
* BoltUntrimmedStore — the legacy layout (/root/reference/chain/boltdb/store.go:143-168): value = the hexjson
  encoding of chain.Beacon {"PreviousSig","Round","Signature"} (/root/reference/chain/beacon.go:14-39).
Both expose get / len / last like drand_amd.sync.TrimmedMemStore, so check_past_beacons runs over a real
store file, plus columns(first, last) for bulk ingestion.
* DeviceBoltStore — the trimmed layout parsed on the device (libdrandhip dh_store_*): the file image
  is uploaded once, columns(first, last) come out in device memory in the layout dh_verify_batch_device takes, and
  check_past_beacons over it is one library call. It agrees with BoltTrimmedStore on every file both accept.
  With fmt="untrimmed" (or "auto" on such a file) it reads the legacy layout the same way and agrees
  with BoltUntrimmedStore; records that are not canonical hexjson are decoded here, by beacon_from_hexjson.
* hexjson records: client.RandomData {"round","randomness","signature","previous_signature"}
  (/root/reference/client/random.go:5-25) and BeaconPacket-shaped JSON, one object per line or a JSON list.
* DeviceArchive — an archive of such records, one per line, parsed and checked on the device (libdrandhip
  dh_archive_*), with check_random_data_host as the serial host form of the same check and
  archive_to_trimmed_store writing a checked archive as a trimmed store file.
* encode_random_data / encode_public_rand — the records a node or relay serves, written on the device from the
  verifier's columns (libdrandhip dh_rand_encode_device), with random_data_frames, public_rand_frames
  and export_random_data over a DeviceBoltStore.
"""
import ctypes
import json
import os
import struct

import numpy as np

from . import _lib
from .chain import Beacon
from .sync import NoBeaconStored

BEACON_BUCKET = b"beacons"  # /root/reference/chain/boltdb/store.go:31
_MAGIC = 0xED0CDAED
_BRANCH, _LEAF, _META = 0x01, 0x02, 0x04
_BUCKET_LEAF = 0x01


class BoltError(ValueError):
    pass


def _fnv64a(b):
    h = 0xcbf29ce484222325
    for x in b:
        h ^= x
        h = (h * 0x100000001b3) & 0xffffffffffffffff
    return h


class BoltFile:
    """Read-only view of a bbolt database file."""

    def __init__(self, path_or_bytes):
        self.data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
        metas = []
        for pg in (0, 1):
            m = self._meta(pg * self._guess_page_size())
            if m:
                metas.append(m)
        if not metas:
            raise BoltError("no valid bbolt meta page")
        self.meta = max(metas, key=lambda m: m["txid"])
        self.page_size = self.meta["page_size"]

    def _guess_page_size(self):
        return struct.unpack_from("<I", self.data, 24)[0] if len(self.data) >= 28 else 4096

    def _meta(self, off):
        if off + 80 > len(self.data):
            return None
        _, flags, _, _ = struct.unpack_from("<QHHI", self.data, off)
        magic, version, psz, _ = struct.unpack_from("<IIII", self.data, off + 16)
        root, _seq, freelist, pgid, txid, cks = struct.unpack_from("<QQQQQQ", self.data, off + 32)
        if not flags & _META or magic != _MAGIC or version != 2:
            return None
        if _fnv64a(self.data[off + 16:off + 72]) != cks:
            return None
        return {"page_size": psz, "root": root, "txid": txid, "pgid": pgid}

    def _page(self, pgid):
        off = pgid * self.page_size
        if off + 16 > len(self.data):
            raise BoltError("page %d beyond end of file" % pgid)
        return self.data, off

    def _walk(self, buf, off):
        """Yield (key, value, flags) of the leaf elements under the page at buf[off:], in key order."""
        _, flags, count, _ = struct.unpack_from("<QHHI", buf, off)
        base = off + 16
        if flags & _LEAF:
            for i in range(count):
                e = base + 16 * i
                fl, pos, ks, vs = struct.unpack_from("<IIII", buf, e)
                k = bytes(buf[e + pos:e + pos + ks])
                v = bytes(buf[e + pos + ks:e + pos + ks + vs])
                yield k, v, fl
        elif flags & _BRANCH:
            for i in range(count):
                e = base + 16 * i
                _pos, _ks, child = struct.unpack_from("<IIQ", buf, e)
                cbuf, coff = self._page(child)
                yield from self._walk(cbuf, coff)
        else:
            raise BoltError("unexpected page flags 0x%x" % flags)

    def _bucket_items(self, root, inline=None):
        if root == 0:  # inline bucket: the page follows the 16-byte bucket header in the value
            return self._walk(inline, 16)
        buf, off = self._page(root)
        return self._walk(buf, off)

    def bucket(self, name):
        """{key: value} of a top-level bucket (sub-buckets are skipped)."""
        for k, v, fl in self._bucket_items(self.meta["root"]):
            if k == name and fl & _BUCKET_LEAF:
                root, _seq = struct.unpack_from("<QQ", v, 0)
                return {bk: bv for bk, bv, bfl in self._bucket_items(root, v) if not bfl & _BUCKET_LEAF}
        raise BoltError("bucket %r not found" % name)


class _BoltStoreBase:
    def __init__(self, path, requires_previous):
        self.requires_previous = bool(requires_previous)
        self._kv = BoltFile(path).bucket(BEACON_BUCKET)
        self._rounds = sorted(struct.unpack(">Q", k)[0] for k in self._kv if len(k) == 8)

    def len(self):
        return len(self._kv)

    def rounds(self):
        return list(self._rounds)

    def last(self):
        if not self._rounds:
            raise NoBeaconStored("empty store")
        return self.get(self._rounds[-1])


class BoltTrimmedStore(_BoltStoreBase):
    """trimmedStore read path (/root/reference/chain/boltdb/trimmed.go:156-193)."""

    def _sig(self, r):
        v = self._kv.get(struct.pack(">Q", r))
        if v is None:
            raise NoBeaconStored(r)
        return v

    def get(self, round_):
        round_ = int(round_)
        sig = self._sig(round_)
        prev = b""
        if self.requires_previous and round_ > 0:
            prev = self._sig(round_ - 1)
        return Beacon(round_, sig, prev)

    def columns(self, first, last, sig_len):
        """Rounds first..last as (rounds u64[n], sigs u8[n, sig_len], prevs list | None, missing rounds).
        Rounds whose record is missing (or whose previous record is missing, chained) are left out of the
        columns and returned in `missing`, which is what CheckPastBeacons reports as faulty for them. A stored
        signature of the wrong length is zero-filled, never cut to a prefix: kilic's UnmarshalBinary rejects
        any wrong-length point and an all-zero record never decodes, so the round is rejected as in Go."""
        rounds, sigs, prevs, missing = [], [], [], []
        for r in range(int(first), int(last) + 1):
            try:
                b = self.get(r)
            except NoBeaconStored:
                missing.append(r)
                continue
            rounds.append(r)
            s = np.zeros(sig_len, np.uint8)
            if len(b.signature) == sig_len:
                s[:] = np.frombuffer(b.signature, np.uint8)
            sigs.append(s)
            prevs.append(b.previous_signature)
        sig_arr = np.array(sigs, dtype=np.uint8).reshape(-1, sig_len)
        return (np.array(rounds, dtype=np.uint64), sig_arr, prevs if self.requires_previous else None, missing)


class StoreTooLarge(MemoryError):
    """DH_ENOMEM from dh_store_open_bolt: the file exceeds DRANDHIP_STORE_MAX_BYTES or device memory."""


class StrideTooLarge(ValueError):
    """DH_EINVAL from dh_store_check_past: a window's rows would exceed 64 KiB (a huge stored record)."""


_CB = ctypes.CFUNCTYPE(None, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p)


class DeviceBoltStore:
    """trimmedStore read path (chain/boltdb/trimmed.go:156-193 of the reference) with the bbolt file parsed on the
    device: len / last / columns like BoltTrimmedStore, columns_device for tensors that stay in device memory, and
    check_past (what sync.check_past_beacons calls for this store type): SyncManager.CheckPastBeacons in one
    dh_store_check_past call. A structurally invalid file raises BoltError from open(), as BoltFile does.

    Untrimmed stores (fmt="untrimmed", or "auto" on a file whose first value is a canonical hexjson beacon): the
    BoltStore read path (chain/boltdb/store.go:172-210) and what BoltUntrimmedStore returns. The device decodes the
    canonical records ({"PreviousSig":P,"Round":D,"Signature":S}, lowercase hex, Round equal to the key); every other
    record is deferred to the host, where beacon_from_hexjson decides it. That function is this project's restatement
    of Beacon.Unmarshal, not a decoder pinned to nikkolasg/hexjson: a verdict on a deferred record is the
    restatement's. Stores written by drand hold canonical records only."""

    FORMATS = {"trimmed": _lib.DH_STORE_TRIMMED, "untrimmed": _lib.DH_STORE_UNTRIMMED, "auto": _lib.DH_STORE_AUTO}

    def __init__(self, path, requires_previous, open_now=True, fmt="trimmed"):
        if fmt not in self.FORMATS:
            raise ValueError("fmt %r: one of %s" % (fmt, sorted(self.FORMATS)))
        self.path = path
        self.requires_previous = bool(requires_previous)
        self.fmt = fmt
        self.untrimmed = None  # known once open
        self._h = None
        self._stat = None
        self._jstat = None
        if open_now:
            self.open()

    # ---- handle
    def open(self):
        if self._h is not None:
            return self
        lib = _lib.load()
        data = np.fromfile(self.path, dtype=np.uint8)
        h = ctypes.c_void_p()
        if self.fmt == "trimmed":
            rc = lib.dh_store_open_bolt(ctypes.c_void_p(data.ctypes.data), data.size, ctypes.byref(h))
        else:
            rc = lib.dh_store_open_bolt_format(ctypes.c_void_p(data.ctypes.data), data.size, self.FORMATS[self.fmt],
                                               ctypes.byref(h))
        self._raise(rc)
        self._h = h
        st = (ctypes.c_uint64 * 6)()
        self._raise(lib.dh_store_stat(h, st))
        self._stat = [int(x) for x in st]
        js = (ctypes.c_uint64 * 4)()
        self._raise(lib.dh_store_format_stat(h, js))
        self._jstat = [int(x) for x in js]
        self.untrimmed = self._jstat[0] == _lib.DH_STORE_UNTRIMMED
        return self

    def close(self):
        if self._h is not None:
            _lib.load().dh_store_close(self._h)
            self._h = None

    def __enter__(self):
        return self.open()

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    @staticmethod
    def _raise(rc):
        if rc >= 0:
            return
        msg = _lib.last_error()
        if rc == _lib.DH_ECORRUPT:
            raise BoltError(msg)
        if rc == _lib.DH_ENOBEACON:
            raise NoBeaconStored(msg)
        if rc == _lib.DH_ENOMEM:
            raise StoreTooLarge(msg)
        if rc == _lib.DH_EINVAL:
            raise ValueError(msg)
        raise RuntimeError("libdrandhip error %d: %s" % (rc, msg))

    # ---- store interface
    def len(self):
        return self._stat[0]

    def rounds_range(self):
        """(first, last) stored round, or None for a store without round records."""
        return (self._stat[2], self._stat[3]) if self._stat[1] else None

    def longest_value(self):
        return self._stat[4]

    def last(self):
        if not self._stat[1]:
            raise NoBeaconStored("empty store")
        return self.get(self._stat[3])

    def get(self, round_):
        round_ = int(round_)
        if self.untrimmed:
            return beacon_from_hexjson(self._raw(round_))
        lo = round_ - 1 if self.requires_previous and round_ > 0 else round_
        rounds, rows, lens, _ = self._columns_host(lo, round_)
        have = {int(r): rows[i, :lens[i]].tobytes() for i, r in enumerate(rounds)}
        if round_ not in have:
            raise NoBeaconStored(round_)
        prev = b""
        if lo < round_:
            if lo not in have:
                raise NoBeaconStored(lo)
            prev = have[lo]
        return Beacon(round_, have[round_], prev)

    def _stride(self, sig_len=0):
        return max(4, (max(int(sig_len), self._stat[4]) + 3) & ~3)

    def columns_device(self, first, last, stride=None):
        """Rounds first..last in device memory: (rounds int64[n] (the u64 bit pattern), rows uint8[n, stride],
        lens int32[n], missing int64[m]) torch tensors; stride defaults to the store's longest value rounded up
        to 4, so every row holds its record in full."""
        import torch
        lib = _lib.load()
        stride = int(stride or self._stride())
        first, last = int(first), int(last)
        n, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
        rc = lib.dh_store_columns_device(self._h, first, last, stride, None, None, None, 0, ctypes.byref(n), None, 0,
                                         ctypes.byref(m), None)
        if rc != _lib.DH_EINVAL or not n.value:  # DH_EINVAL with the sizes needed, unless the window holds no row
            self._raise(rc)
        dev = torch.device("cuda")
        rounds = torch.empty(n.value, dtype=torch.int64, device=dev)
        rows = torch.empty((n.value, stride), dtype=torch.uint8, device=dev)
        lens = torch.empty(n.value, dtype=torch.int32, device=dev)
        missing = torch.empty(m.value, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        self._raise(lib.dh_store_columns_device(self._h, first, last, stride, rounds.data_ptr(), rows.data_ptr(),
                                                lens.data_ptr(), n.value, ctypes.byref(n), missing.data_ptr(), m.value,
                                                ctypes.byref(m), None))
        return rounds, rows, lens, missing

    def _columns_host(self, first, last, sig_len=0):
        rounds, rows, lens, missing = self.columns_device(first, last, self._stride(sig_len))
        return (rounds.cpu().numpy().view(np.uint64), rows.cpu().numpy(), lens.cpu().numpy().view(np.uint32),
                missing.cpu().numpy().view(np.uint64))

    def columns(self, first, last, sig_len):
        """The tuple of BoltTrimmedStore.columns, from the device columns copied back. Untrimmed: the same tuple over
        BoltUntrimmedStore.get (the stored PreviousSig; a record the host decoder rejects counts as missing)."""
        first, last = int(first), int(last)
        if self.untrimmed:
            return self._columns_untrimmed(first, last, sig_len)
        lo = first - 1 if self.requires_previous and first > 0 else first
        rounds, rows, lens, missing = self._columns_host(lo, last, sig_len)
        keep = rounds >= first
        if self.requires_previous:  # Get fails when the record of round - 1 is missing (round 0 has none)
            has_prev = np.zeros(len(rounds), bool)
            if len(rounds):
                has_prev[1:] = rounds[1:] == rounds[:-1] + 1
                has_prev[0] = rounds[0] == 0
            lost = rounds[keep & ~has_prev]
            keep &= has_prev
        else:
            lost = np.zeros(0, np.uint64)
        idx = np.flatnonzero(keep)
        sig_arr = np.zeros((len(idx), sig_len), np.uint8)
        good = lens[idx] == sig_len
        sig_arr[good] = rows[idx[good], :sig_len]
        prevs = None
        if self.requires_previous:
            prevs = [b"" if rounds[i] == 0 else rows[i - 1, :lens[i - 1]].tobytes() for i in idx]
        miss = sorted(set(int(r) for r in missing if r >= first) | set(int(r) for r in lost))
        return rounds[idx].astype(np.uint64), sig_arr, prevs, miss

    # ---- untrimmed stores
    def format_stat(self):
        """{"format", "deferred", "longest_signature", "longest_previous"} (dh_store_format_stat)."""
        return dict(zip(("format", "deferred", "longest_signature", "longest_previous"),
                        [["trimmed", "untrimmed"][self._jstat[0]]] + self._jstat[1:]))

    def _raw(self, round_):
        rounds, rows, lens, _ = self._columns_host(round_, round_)
        if not len(rounds):
            raise NoBeaconStored(round_)
        return rows[0, :lens[0]].tobytes()

    def beacons_device(self, first, last, sig_stride=None, prev_stride=None, want_prev=True):
        """Rounds first..last of an untrimmed store, decoded, in device memory: (rounds int64[n], sigs uint8[n, sig_stride],
        sig_lens int32[n], prevs uint8[n, prev_stride] | None, prev_lens int32[n] | None, deferred uint8[n],
        missing int64[m]) torch tensors in the layout dh_verify_batch_device takes. Strides default to the store's longest
        decoded field rounded up to 4. A deferred row is all zero with zero lengths."""
        import torch
        lib = _lib.load()
        sig_stride = int(sig_stride or max(4, (self._jstat[2] + 3) & ~3))
        prev_stride = int(prev_stride or max(4, (self._jstat[3] + 3) & ~3))
        first, last = int(first), int(last)
        n, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
        rc = lib.dh_store_beacons_device(self._h, first, last, sig_stride, prev_stride, None, None, None, None, None, None, 0,
                                         ctypes.byref(n), None, 0, ctypes.byref(m), None)
        if rc != _lib.DH_EINVAL or not n.value:  # DH_EINVAL with the sizes needed, unless the window holds no row
            self._raise(rc)
        dev = torch.device("cuda")
        rounds = torch.empty(n.value, dtype=torch.int64, device=dev)
        sigs = torch.empty((n.value, sig_stride), dtype=torch.uint8, device=dev)
        sig_lens = torch.empty(n.value, dtype=torch.int32, device=dev)
        prevs = torch.empty((n.value, prev_stride), dtype=torch.uint8, device=dev) if want_prev else None
        prev_lens = torch.empty(n.value, dtype=torch.int32, device=dev) if want_prev else None
        deferred = torch.empty(n.value, dtype=torch.uint8, device=dev)
        missing = torch.empty(m.value, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        self._raise(lib.dh_store_beacons_device(
            self._h, first, last, sig_stride, prev_stride, rounds.data_ptr(), sigs.data_ptr(), sig_lens.data_ptr(),
            prevs.data_ptr() if want_prev else None, prev_lens.data_ptr() if want_prev else None, deferred.data_ptr(), n.value,
            ctypes.byref(n), missing.data_ptr(), m.value, ctypes.byref(m), None))
        return rounds, sigs, sig_lens, prevs, prev_lens, deferred, missing

    def deferred(self, first=0, last=(1 << 64) - 1):
        """Keys of the records in first..last that the device leaves to the host decoder (dh_store_deferred)."""
        lib = _lib.load()
        cap = max(1, self._jstat[1])
        out = np.zeros(cap, np.uint64)
        n = ctypes.c_size_t(0)
        self._raise(lib.dh_store_deferred(self._h, int(first), int(last), ctypes.c_void_p(out.ctypes.data), cap, ctypes.byref(n)))
        return [int(x) for x in out[:n.value]]

    def _columns_untrimmed(self, first, last, sig_len):
        rounds, sigs, sig_lens, prevs, prev_lens, deferred, missing = self.beacons_device(first, last)
        rounds, sigs, sig_lens = rounds.cpu().numpy().view(np.uint64), sigs.cpu().numpy(), sig_lens.cpu().numpy()
        prevs, prev_lens, deferred = prevs.cpu().numpy(), prev_lens.cpu().numpy(), deferred.cpu().numpy()
        out_r, out_s, out_p = [], [], []
        miss = [int(r) for r in missing.cpu().numpy().view(np.uint64)]
        for i, r in enumerate(rounds):
            if deferred[i]:  # decided by the host decoder
                try:
                    b = beacon_from_hexjson(self._raw(int(r)))
                except DECODE_ERRORS:
                    miss.append(int(r))
                    continue
                rnd, sig, prev = b.round, b.signature, b.previous_signature
            else:
                rnd, sig, prev = int(r), sigs[i, :sig_lens[i]].tobytes(), prevs[i, :prev_lens[i]].tobytes()
            out_r.append(rnd)
            row = np.zeros(sig_len, np.uint8)
            if len(sig) == sig_len:
                row[:] = np.frombuffer(sig, np.uint8)
            out_s.append(row)
            out_p.append(prev)
        sig_arr = np.array(out_s, dtype=np.uint8).reshape(-1, sig_len)
        return np.array(out_r, dtype=np.uint64), sig_arr, out_p if self.requires_previous else None, sorted(miss)

    def _resolve_deferred(self, scheme, pubkey, up_to, seed):
        """[(key, reported round)] of the faulty ones among the deferred records the CheckPastBeacons loop visits: a
        value beacon_from_hexjson rejects is faulty under its key (the Get error, sync_manager.go:205-212); a decoded
        one is verified and reported under its Round field (:215-217)."""
        last = self._stat[3]
        up_to = min(int(up_to), last)
        hi = min(self._stat[0] - 1, max(up_to, 1))
        out, pend = [], []
        for k in (self.deferred(1, hi) if hi >= 1 else []):
            try:
                pend.append((k, beacon_from_hexjson(self._raw(k))))
            except DECODE_ERRORS:
                out.append((k, k))
        if pend:
            rounds = np.array([b.round for _, b in pend], dtype=np.uint64)
            sigs = np.zeros((len(pend), scheme.sig_len), dtype=np.uint8)
            bad_len = np.zeros(len(pend), dtype=bool)
            for i, (_, b) in enumerate(pend):
                if len(b.signature) == scheme.sig_len:
                    sigs[i] = np.frombuffer(b.signature, dtype=np.uint8)
                else:
                    bad_len[i] = True
            prevs = [b.previous_signature for _, b in pend] if scheme.chained else None
            ok, _ = scheme.verify_beacons(pubkey, rounds, sigs, prevs, seed=seed, want_randomness=False)
            out += [(k, b.round) for (k, b), v, bl in zip(pend, ok, bad_len) if bl or not v]
        return out

    def check_past(self, scheme, pubkey, up_to, cb=None, window=1 << 20, seed=0):
        """dh_store_check_past: the faulty rounds of sync.check_past_beacons over this store. cb(round, up_to) is
        called once per window. Raises StrideTooLarge when the library asks for the host path.

        Untrimmed stores: the library skips the records that are not canonical hexjson (DH_DEFERRED); those are
        decided HERE, by this module's restatement of the decoder (beacon_from_hexjson), not by a decoder pinned to
        nikkolasg/hexjson, verified in one small scheme.verify_beacons call and merged into the device's list at the
        position of their key. A deferred last record is a ValueError (Last().Round needs the host decoder: use
        BoltUntrimmedStore)."""
        lib = _lib.load()
        hook = _CB((lambda r, u, _a: cb(int(r), int(u))) if cb is not None else (lambda r, u, _a: None))
        cap = max(1, self.len())  # the rounds examined lie below len(): one call always has room
        while True:
            out = np.zeros(cap, np.uint64)
            n = ctypes.c_size_t(0)
            rc = lib.dh_store_check_past(self._h, scheme.id, bytes(pubkey), len(pubkey), int(up_to), int(window), int(seed),
                                         ctypes.c_void_p(out.ctypes.data), cap, ctypes.byref(n),
                                         hook if cb is not None else None, None)
            if rc == _lib.DH_EINVAL and n.value > cap:
                cap, cb = n.value, None  # the callback has seen every window already
                continue
            if rc == _lib.DH_EINVAL and "64 KiB" in _lib.last_error():
                raise StrideTooLarge(_lib.last_error())
            self._raise(rc)
            got = [int(x) for x in out[:n.value]]
            if rc == _lib.DH_DEFERRED:
                extra = self._resolve_deferred(scheme, pubkey, up_to, seed)
                got = [rep for _k, rep in sorted([(k, k) for k in got] + extra, key=lambda t: t[0])]
            return got


    # ---- writing
    def stored_signature(self, round_):
        """The signature stored for one round (untrimmed: the decoded Signature field), whatever its neighbours."""
        raw = self._raw(int(round_))
        return beacon_from_hexjson(raw).signature if self.untrimmed else raw

    def split(self, first=0, last=None, max_rows=1 << 20):
        """dh_store_split: [(first, last)] round windows covering first..last, cut at leaf boundaries of the file, each
        of at most max(max_rows, rows of its largest leaf) stored rows."""
        lib = _lib.load()
        first = int(first)
        last = (1 << 64) - 1 if last is None else int(last)
        n = ctypes.c_size_t(0)
        rc = lib.dh_store_split(self._h, first, last, int(max_rows), None, 0, ctypes.byref(n))
        if rc != _lib.DH_EINVAL or not n.value:
            self._raise(rc)
            return []
        out = np.zeros(2 * n.value, np.uint64)
        self._raise(lib.dh_store_split(self._h, first, last, int(max_rows), ctypes.c_void_p(out.ctypes.data), n.value, ctypes.byref(n)))
        return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n.value)]

    def _resolve(self, first, last, patches, undecodable):
        """After DH_DEFERRED: the deferred records of first..last that no patch covers, decoded by the host decoder into
        `patches` (None and listed in `undecodable` when it rejects them)."""
        todo = [k for k in self.deferred(first, last) if k not in patches]
        if not todo:
            raise RuntimeError("dh_store_save_trimmed keeps deferring records that are patched")
        for k in todo:
            try:
                patches[k] = beacon_from_hexjson(self._raw(k)).signature
            except DECODE_ERRORS:
                patches[k] = None
                undecodable.append(k)

    def _save_trimmed_windows(self, path, first, last, patches, page_size, window):
        stats = {"rows": 0, "leaves": 0, "pages": 0, "replaced_or_deleted": 0, "inserted": 0, "unlinked": [], "undecodable": []}
        with BoltWriter(path, page_size) as w:
            # a window's run: its records (16 B of element and 8 B of key each) plus the leaves' headers and padding,
            # below a twelfth more for the page sizes and values of beacon stores; an outgrown buffer only costs a retry
            longest = self._jstat[2] if self.untrimmed else self._stat[4]
            longest = max([longest] + [len(v) for v in patches.values() if v is not None])
            w.reserve((min(window, self._stat[1]) + len(patches) + 64) * (24 + longest) * 13 // 12 + 8 * page_size)
            for lo, hi in self.split(first, last, window):
                res = w.append_from(self, lo, hi, {r: v for r, v in patches.items() if lo <= r <= hi})
                for k in ("replaced_or_deleted", "inserted"):
                    stats[k] += res[k]
                stats["unlinked"] += res["unlinked"]
                stats["undecodable"] += res["undecodable"]
            stats.update(w.finish())
        return stats

    def save_trimmed(self, path, first=0, last=None, patches=None, page_size=4096, window=None):
        """dh_store_save_trimmed: the round records of first..last as a trimmed store file at `path` (written to
        path + ".tmp", then os.replace). A trimmed store is copied value by value; an untrimmed one is converted: each
        record's decoded Signature under the record's key. patches: {round: bytes | None} replaces or inserts the
        record of a round inside first..last, None deletes it.

        Records of an untrimmed store that are not canonical hexjson and that no patch covers are decoded here, by
        beacon_from_hexjson, and written under their KEY (a Round field that differs from the key is not followed); one
        that does not decode is dropped and listed under "undecodable".

        Returns {"rows", "leaves", "pages", "replaced_or_deleted", "inserted", "unlinked", "undecodable"}. "unlinked":
        the rounds whose record stored a PreviousSig that the written file's record of round - 1 does not equal (or does
        not hold): a chained verifier reading the new file sees another previous signature for them than the old record
        carried. Always empty for a trimmed source. `path` may not be the store's own file.

        window: stored rows per window of the streaming writer (BoltWriter over split()): the file is written to the
        disk run by run with one window in host and device memory, and is the same file; the result is the same dict.
        Without it the image is built in one call, unless the store holds more rows than one call takes."""
        lib = _lib.load()
        _refuse_same_file(path, self.path)
        first = int(first)
        last = (1 << 64) - 1 if last is None else int(last)
        patches = {int(r): v for r, v in dict(patches or {}).items()}
        if window is None and self._stat[1] + len(patches) > MAX_CALL_ROWS - 1:
            window = STREAM_WINDOW
        if window is not None:
            if int(window) < 1:
                raise ValueError("window: at least 1 row")
            return self._save_trimmed_windows(path, first, last, patches, int(page_size), int(window))
        undecodable = []
        cap = int(os.path.getsize(self.path)) + 2 * sum(len(v) for v in patches.values() if v is not None) + 64 * int(page_size)
        ucap = 1024
        while True:
            pr, ps, pl, stride = _patch_arrays(patches)
            image = np.empty(cap, np.uint8)
            unl = np.zeros(ucap, np.uint64)
            n, nu = ctypes.c_size_t(0), ctypes.c_size_t(0)
            stats = (ctypes.c_uint64 * 6)()
            rc = lib.dh_store_save_trimmed(self._h, first, last, ctypes.c_void_p(pr.ctypes.data), ctypes.c_void_p(ps.ctypes.data),
                                           stride, ctypes.c_void_p(pl.ctypes.data), len(patches), int(page_size),
                                           ctypes.c_void_p(image.ctypes.data), cap, ctypes.byref(n),
                                           ctypes.c_void_p(unl.ctypes.data), ucap, ctypes.byref(nu), stats)
            if rc == _lib.DH_DEFERRED:  # decided by the host decoder, once
                self._resolve(first, last, patches, undecodable)
                continue
            if rc == _lib.DH_EINVAL and (n.value > cap or nu.value > ucap):
                cap, ucap = max(cap, n.value), max(ucap, nu.value)
                continue
            self._raise(rc)
            break
        _replace_file(path, image[:n.value])
        return {"rows": int(stats[0]), "leaves": int(stats[1]), "pages": int(stats[2]), "replaced_or_deleted": int(stats[4]),
                "inserted": int(stats[5]), "unlinked": [int(x) for x in unl[:nu.value]], "undecodable": undecodable}


def _refuse_same_file(path, source):
    same = os.path.realpath(path) == os.path.realpath(source)
    if not same and os.path.exists(path):
        same = os.path.samefile(path, source)
    if same:
        raise ValueError("%r is the store's own source file: write to another name and rename" % (path,))


def _replace_file(path, image):
    tmp = str(path) + ".tmp"
    with open(tmp, "wb") as f:
        image.tofile(f)
    os.replace(tmp, path)


def _patch_arrays(patches):
    """(rounds u64[k], sigs u8[k, stride], lens u32[k], stride) of {round: bytes | None}, ascending."""
    keys = sorted(int(r) for r in patches)
    stride = max([4] + [len(patches[r]) for r in keys if patches[r] is not None])
    rounds = np.array(keys, dtype=np.uint64).reshape(-1)
    sigs = np.zeros((len(keys), stride), np.uint8)
    lens = np.zeros(len(keys), np.uint32)
    for i, r in enumerate(keys):
        v = patches[r]
        if v is None:
            lens[i] = _lib.DH_PATCH_DELETE
        else:
            lens[i] = len(v)
            sigs[i, :len(v)] = np.frombuffer(bytes(v), np.uint8)
    return rounds, sigs, lens, stride


def _device_columns(rounds, sigs, lens):
    """(d_rounds int64[n], d_sigs uint8[n, stride], d_lens int32[n]) on the device; tensors are used in place."""
    import torch
    dev = torch.device("cuda")

    def tensor(x, np_dtype, view):
        if isinstance(x, torch.Tensor):
            return x.to(dev).contiguous()
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np_dtype).view(view)).to(dev)

    d_rounds = tensor(rounds, np.uint64, np.int64).reshape(-1)
    d_sigs = tensor(sigs, np.uint8, np.uint8)
    n = d_rounds.numel()
    if d_sigs.dim() != 2 or d_sigs.shape[0] != n or d_sigs.dtype != torch.uint8 or d_rounds.dtype != torch.int64:
        raise ValueError("rounds int64/uint64 [n] and sigs uint8 [n, stride]")
    if lens is None:
        d_lens = torch.full((n,), int(d_sigs.shape[1]), dtype=torch.int32, device=dev)
    else:
        d_lens = tensor(lens, np.uint32, np.int32).reshape(-1)
        if d_lens.numel() != n or d_lens.dtype != torch.int32:
            raise ValueError("lens int32/uint32 [n]")
    torch.cuda.synchronize()
    return d_rounds, d_sigs, d_lens


# Rows per window of the streaming paths (write_trimmed_bolt / save_trimmed / correct_store_file with window=None and a
# source above one call's rows): the fastest window of the sweep of bench/store_stream.py (1M, 4M and 8M rows) in its
# 8M-row rewrite, the one case in which the windows differ; no larger one lies inside its spread (DESIGN.md §23,
# profiles/r18/store_stream.json).
STREAM_WINDOW = 1 << 20
MAX_CALL_ROWS = 4096 * 4096 - 2  # what one library call takes: the device scan's limit


class BoltWriter:
    """The windowed writer (dh_bolt_writer_*): a trimmed store file written from rows that arrive in
    windows. Each run of pages is written to path + ".tmp" at its offset as it arrives; finish() writes the tail, then
    the head, and os.replace()s. The file is byte for byte what write_trimmed_bolt gives for the concatenated rows.
    Host memory is one window's run, not the file. A context manager: on an exception, or on leaving the block without
    finish(), the .tmp file is removed and `path` is untouched."""

    def __init__(self, path, page_size=4096):
        lib = _lib.load()
        self.path, self.page_size = str(path), int(page_size)
        self._tmp = self.path + ".tmp"
        self._h = ctypes.c_void_p()
        self._f = None
        self._buf = np.empty(0, np.uint8)
        DeviceBoltStore._raise(lib.dh_bolt_writer_open(self.page_size, ctypes.byref(self._h)))
        try:
            self._f = open(self._tmp, "wb")
        except BaseException:
            self.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        """Frees the handle; an unfinished file is removed."""
        if self._h:
            _lib.load().dh_bolt_writer_close(self._h)
            self._h = ctypes.c_void_p()
        if self._f is not None:
            self._f.close()
            self._f = None
            if os.path.exists(self._tmp):
                os.remove(self._tmp)

    def _room(self, size):
        if self._buf.size < size:
            self._buf = np.empty(size, np.uint8)
        return self._buf

    def reserve(self, nbytes):
        """Room for runs of up to nbytes in the one host buffer the appends share. An append whose run outgrows the
        buffer is refused by the library, which consumes nothing, and is made again with the size it reported; for a
        window of a store that repeats the window's gather and merge, so a caller that knows its windows reserves."""
        self._room(int(nbytes))

    def _emit(self, call):
        """call(out, cap, len_ref, off_ref) -> rc, sized by a first refusal; the run is written at its offset."""
        size, off = ctypes.c_size_t(0), ctypes.c_uint64(0)
        buf = self._buf
        rc = call(ctypes.c_void_p(buf.ctypes.data) if buf.size else None, buf.size, ctypes.byref(size), ctypes.byref(off))
        if rc == _lib.DH_EINVAL and size.value > buf.size:  # nothing was consumed
            buf = self._room(size.value)
            rc = call(ctypes.c_void_p(buf.ctypes.data), buf.size, ctypes.byref(size), ctypes.byref(off))
        if rc in (_lib.DH_OK,) and size.value:
            self._f.seek(off.value)
            buf[:size.value].tofile(self._f)
        return rc

    def append(self, rounds, sigs, lens=None):
        """Rows as write_trimmed_bolt takes them, above every round appended so far. Returns {"rows", "leaves",
        "pages"}: the rows taken, the leaves this append closed and the pages it wrote."""
        lib = _lib.load()
        if self._f is None:
            raise ValueError("the writer is closed")
        d_rounds, d_sigs, d_lens = _device_columns(rounds, sigs, lens)
        stats = (ctypes.c_uint64 * 3)()
        args = (d_rounds.data_ptr() or None, d_sigs.data_ptr() or None, int(d_sigs.shape[1]), d_lens.data_ptr() or None, d_rounds.numel())
        DeviceBoltStore._raise(self._emit(lambda out, cap, n, off: lib.dh_bolt_writer_append_device(self._h, *args, out, cap, n, off,
                                                                                                  stats, None)))
        return {"rows": int(stats[0]), "leaves": int(stats[1]), "pages": int(stats[2])}

    def append_from(self, store, first, last, patches=None):
        """dh_store_save_trimmed_append: the round records of first..last of an open DeviceBoltStore, merged with
        patches {round: bytes | None} as save_trimmed takes them, deferred records resolved the same way. Windows come
        in ascending round order. Returns {"rows", "leaves", "pages", "replaced_or_deleted", "inserted", "unlinked",
        "undecodable"} of this window."""
        lib = _lib.load()
        if self._f is None:
            raise ValueError("the writer is closed")
        first, last = int(first), int(last)
        patches = {int(r): v for r, v in dict(patches or {}).items()}
        undecodable = []
        ucap = 1024
        while True:
            pr, ps, pl, stride = _patch_arrays(patches)
            unl = np.zeros(ucap, np.uint64)
            nu = ctypes.c_size_t(0)
            stats = (ctypes.c_uint64 * 6)()
            rc = self._emit(lambda out, cap, n, off: lib.dh_store_save_trimmed_append(
                store._h, self._h, first, last, ctypes.c_void_p(pr.ctypes.data), ctypes.c_void_p(ps.ctypes.data), stride,
                ctypes.c_void_p(pl.ctypes.data), len(patches), out, cap, n, off, ctypes.c_void_p(unl.ctypes.data), ucap,
                ctypes.byref(nu), stats))
            if rc == _lib.DH_DEFERRED:  # decided by the host decoder, once
                store._resolve(first, last, patches, undecodable)
                continue
            if rc == _lib.DH_EINVAL and nu.value > ucap:
                ucap = nu.value
                continue
            DeviceBoltStore._raise(rc)
            break
        return {"rows": int(stats[0]), "leaves": int(stats[1]), "pages": int(stats[2]), "replaced_or_deleted": int(stats[4]),
                "inserted": int(stats[5]), "unlinked": [int(x) for x in unl[:nu.value]], "undecodable": undecodable}

    def finish(self):
        """Writes the tail and the head, renames the file into place. Returns {"rows", "leaves", "pages"} of the file."""
        lib = _lib.load()
        if self._f is None:
            raise ValueError("the writer is closed")
        stats = (ctypes.c_uint64 * 3)()
        head = np.empty(4 * self.page_size, np.uint8)
        DeviceBoltStore._raise(self._emit(lambda out, cap, n, off: lib.dh_bolt_writer_finish(
            self._h, out, cap, n, off, ctypes.c_void_p(head.ctypes.data), stats)))
        self._f.seek(0)
        head.tofile(self._f)
        self._f.flush()
        os.replace(self._tmp, self.path)  # if this raises, close() (the context manager's exit) removes the .tmp
        self._f.close()
        self._f = None
        self.close()
        return {"rows": int(stats[0]), "leaves": int(stats[1]), "pages": int(stats[2])}


def write_trimmed_bolt(path, rounds, sigs, lens=None, page_size=4096, window=None):
    """dh_bolt_write_trimmed_device: a trimmed store file (chain/boltdb/trimmed.go:87-107 of the reference: bucket
    "beacons", key = round, value = signature) from columns: rounds u64[n] strictly ascending, sigs u8[n, stride],
    lens u32[n] (default: every value is the full row). numpy arrays are uploaded; torch tensors on the device (rounds
    int64 carrying the u64 bit pattern, lens int32, as DeviceBoltStore.columns_device returns them) are used in place.
    Written to path + ".tmp", then os.replace. Returns {"rows", "leaves", "pages"}.

    window: rows per append of a BoltWriter, which streams the file to the disk with one window's run in host memory;
    the file is the same. Without it the image is built in one call, unless there are more rows than one call takes."""
    lib = _lib.load()
    d_rounds, d_sigs, d_lens = _device_columns(rounds, sigs, lens)
    n = d_rounds.numel()
    if window is None and n > MAX_CALL_ROWS:
        window = STREAM_WINDOW
    if window is not None:
        window = int(window)
        if window < 1 or window > MAX_CALL_ROWS:
            raise ValueError("window: 1..%d rows" % MAX_CALL_ROWS)
        with BoltWriter(path, page_size) as w:
            for at in range(0, n, window):
                w.append(d_rounds[at:at + window], d_sigs[at:at + window], d_lens[at:at + window])
            return w.finish()
    stride = int(d_sigs.shape[1])
    size = ctypes.c_size_t(0)
    stats = (ctypes.c_uint64 * 3)()
    args = (d_rounds.data_ptr() or None, d_sigs.data_ptr() or None, stride, d_lens.data_ptr() or None, n, int(page_size))
    rc = lib.dh_bolt_write_trimmed_device(*args, None, 0, ctypes.byref(size), stats, None)
    if rc != _lib.DH_EINVAL or not size.value:  # DH_EINVAL with the size needed
        DeviceBoltStore._raise(rc)
    image = np.empty(size.value, np.uint8)
    DeviceBoltStore._raise(lib.dh_bolt_write_trimmed_device(*args, ctypes.c_void_p(image.ctypes.data), image.size,
                                                            ctypes.byref(size), stats, None))
    _replace_file(path, image[:size.value])
    return {"rows": int(stats[0]), "leaves": int(stats[1]), "pages": int(stats[2])}


class BoltUntrimmedStore(_BoltStoreBase):
    """BoltStore read path (/root/reference/chain/boltdb/store.go): hexjson-encoded chain.Beacon values."""

    def get(self, round_):
        v = self._kv.get(struct.pack(">Q", int(round_)))
        if v is None:
            raise NoBeaconStored(round_)
        return beacon_from_hexjson(v)


# what beacon_from_hexjson raises on a value it does not decode (bad JSON / hex, or JSON of another shape)
DECODE_ERRORS = (ValueError, TypeError, AttributeError)


def looks_untrimmed(path):
    """shouldUseTrimmedBolt (/root/reference/chain/boltdb/store.go:82-110), negated: the first value of the bucket
    decodes as a hexjson beacon."""
    kv = BoltFile(path).bucket(BEACON_BUCKET)
    if not kv:
        return False
    try:
        beacon_from_hexjson(kv[min(kv)])
    except DECODE_ERRORS:
        return False
    return True


def _hexbytes(x):
    return bytes.fromhex(x) if x else b""


def beacon_from_hexjson(text):
    """chain.Beacon.Unmarshal (/root/reference/chain/beacon.go:36-39): hexjson with Go field names."""
    d = json.loads(text)
    return Beacon(int(d.get("Round", 0)), _hexbytes(d.get("Signature")), _hexbytes(d.get("PreviousSig")))


def read_random_data(text):
    """client.RandomData records (/root/reference/client/random.go:5-10), as a JSON list or one object per
    line -> list of dicts {round, randomness, signature, previous_signature} with bytes values. BeaconPacket
    JSON field names (round, signature, previous_signature) read the same way."""
    text = text.strip()
    objs = json.loads(text) if text.startswith("[") else [json.loads(l) for l in text.splitlines() if l.strip()]
    out = []
    for o in objs:
        out.append({"round": int(o.get("round", 0)), "randomness": _hexbytes(o.get("randomness")),
                    "signature": _hexbytes(o.get("signature")),
                    "previous_signature": _hexbytes(o.get("previous_signature"))})
    return out


def random_data_columns(records, sig_len):
    """RandomData records -> (rounds u64[n], sigs u8[n, sig_len], prevs list, randomness list). A signature
    of the wrong length is zero-filled (an all-zero record never decodes, so it is rejected like kyber's
    length check)."""
    n = len(records)
    rounds = np.array([r["round"] for r in records], dtype=np.uint64)
    sigs = np.zeros((n, sig_len), dtype=np.uint8)
    for i, r in enumerate(records):
        if len(r["signature"]) == sig_len:
            sigs[i] = np.frombuffer(r["signature"], np.uint8)
    return rounds, sigs, [r["previous_signature"] for r in records], [r["randomness"] for r in records]


# ---- client.RandomData JSON-lines archives

_U64 = (1 << 64) - 1
AR_DEFERRED, AR_NO_SIGNATURE, AR_INVALID, AR_RANDOMNESS = (_lib.DH_AR_DEFERRED, _lib.DH_AR_NO_SIGNATURE, _lib.DH_AR_INVALID,
                                                          _lib.DH_AR_RANDOMNESS)
AR_SEQUENCE, AR_LINK, AR_PRED_DEFERRED = _lib.DH_AR_SEQUENCE, _lib.DH_AR_LINK, _lib.DH_AR_PRED_DEFERRED
AR_BEACON_ID = _lib.DH_AR_BEACON_ID
PB_BEACON_PACKET, PB_PUBLIC_RAND = _lib.DH_PB_BEACON_PACKET, _lib.DH_PB_PUBLIC_RAND
_RD_FIELDS = ("randomness", "signature", "previous_signature")


def random_data_from_line(line):
    """ONE client.RandomData record (one line of an archive, bytes or str) -> {round, randomness, signature,
    previous_signature} as read_random_data gives it: json.loads plus that function's field rules, with the round
    held to 64 bits. None for a whitespace-only line; raises one of DECODE_ERRORS for text that does not decode.
    This is the project's restatement of the record's JSON rules, not a decoder pinned to nikkolasg/hexjson: it decides
    the records the device defers."""
    text = bytes(line).decode("utf-8") if not isinstance(line, str) else line
    if not text.strip():
        return None
    o = json.loads(text)
    rnd = int(o.get("round", 0))
    if not 0 <= rnd <= _U64:
        raise ValueError("round %d does not fit 64 bits" % rnd)
    return {"round": rnd, "randomness": _hexbytes(o.get("randomness")), "signature": _hexbytes(o.get("signature")),
            "previous_signature": _hexbytes(o.get("previous_signature"))}


def random_data_line(rec):
    """The hexjson form the relays write (cmd/relay-s3/main.go:127-141 through nikkolasg/hexjson): the fields in the
    order of client/random.go:5-10, lowercase hex, omitempty; bytes without a newline."""
    parts = []
    if int(rec.get("round", 0)):
        parts.append(b'"round":%d' % int(rec["round"]))
    for k in _RD_FIELDS:
        v = rec.get(k)
        if v:
            parts.append(b'"%s":"%s"' % (k.encode(), bytes(v).hex().encode()))
    return b"{" + b",".join(parts) + b"}"


def archive_lines(data):
    """The framing of an archive: the non-empty runs of bytes between b"\\n" bytes, in file order."""
    return [l for l in bytes(data).split(b"\n") if l]


def _verify_records(scheme, pubkey, recs, seed=0):
    """[bool] for records whose signature has the scheme's length: one verify_beacons call, the chained scheme against
    each record's own previous_signature."""
    if not recs:
        return []
    rounds = np.array([r["round"] for r in recs], dtype=np.uint64)
    sigs = np.array([np.frombuffer(r["signature"], np.uint8) for r in recs], dtype=np.uint8).reshape(len(recs), scheme.sig_len)
    prevs = [r["previous_signature"] for r in recs] if scheme.chained else None
    ok, _ = scheme.verify_beacons(pubkey, rounds, sigs, prevs, seed=seed, want_randomness=False)
    return [bool(v) for v in ok]


def _own_bits(rec, sig_len, verdict):
    """Bits 2 / 4 / 8 of a decoded record; verdict: the verifier's, read only for a signature of the scheme's length."""
    import hashlib
    sig = rec["signature"]
    st = 0
    if not sig:
        st |= AR_NO_SIGNATURE | AR_INVALID
    elif len(sig) != sig_len or not verdict:
        st |= AR_INVALID
    if rec["randomness"] and rec["randomness"] != hashlib.sha256(sig).digest():
        st |= AR_RANDOMNESS
    return st


def _pred_bits(rec, pred, chained):
    """Bits 16 / 32 of a decoded record against its predecessor {round, signature} (None: it has none)."""
    st = 0
    if pred is not None:
        if rec["round"] != (pred["round"] + 1) & _U64:
            st |= AR_SEQUENCE
        if chained and rec["previous_signature"] != pred["signature"]:
            st |= AR_LINK
    return st


def _anchor_rec(anchor):
    if anchor is None:
        return None
    rnd, sig = anchor
    return {"round": int(rnd), "signature": bytes(sig)}


def check_random_data_host(lines, scheme, pubkey, anchor=None, verify=None):
    """The serial host check of an archive, the yardstick of DeviceArchive.check: one status byte (the DH_AR_* bits of
    include/drandhip.h, bits 1 and 64 never set) per record, as a numpy uint8 array. lines: the archive's bytes, or its
    lines already framed. Each line goes through random_data_from_line: a whitespace-only line is dropped from the
    result; one that does not decode gets DH_AR_INVALID and, having neither round nor signature, is no predecessor:
    the record after it is compared with the last record that decoded (the anchor (round, signature) before the first).
    verify(scheme, pubkey, records) -> [bool] replaces the device verifier (the CPU tests pass the oracle)."""
    if isinstance(lines, (bytes, bytearray, memoryview)):
        lines = archive_lines(lines)
    verify = verify or _verify_records
    recs = []
    for l in lines:
        try:
            r = random_data_from_line(l)
        except DECODE_ERRORS:
            r = False
        if r is not None:
            recs.append(r)
    todo = [r for r in recs if r and len(r["signature"]) == scheme.sig_len]
    verdict = dict(zip(map(id, todo), verify(scheme, pubkey, todo)))
    out = np.zeros(len(recs), np.uint8)
    pred = _anchor_rec(anchor)
    for i, r in enumerate(recs):
        if r is False:
            out[i] = AR_INVALID
            continue
        out[i] = _own_bits(r, scheme.sig_len, verdict.get(id(r), False)) | _pred_bits(r, pred, scheme.chained)
        pred = r
    return out


class DeviceArchive:
    """A client.RandomData JSON-lines archive parsed on the device (dh_archive_*): the image is uploaded
    and indexed once; beacons_device gives a window's columns as torch tensors in the layout dh_verify_batch_device and
    BoltWriter.append take; check verifies every record and resolves the records the device defers here, through
    random_data_from_line. A context manager. The JSON-array form raises ValueError: read_random_data reads it.
    from_packets opens the same handle over protobuf records."""

    STAT = ("records", "deferred", "longest_line", "longest_signature", "longest_previous", "longest_randomness", "tile_bytes")

    kind = 0       # 0: JSON lines; PB_BEACON_PACKET / PB_PUBLIC_RAND: protobuf records (from_packets)
    unframed = b""  # from_packets on a varint-delimited buffer: the trailing bytes that frame no record

    def __init__(self, path_or_bytes):
        self._data = self._read(path_or_bytes)
        self._h = None
        self._resolved = {}
        h = ctypes.c_void_p()
        DeviceBoltStore._raise(_lib.load().dh_archive_open_ndjson(self._data, len(self._data), ctypes.byref(h)))
        self._opened(h)

    @staticmethod
    def _read(path_or_bytes):
        if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
            return bytes(path_or_bytes)
        with open(path_or_bytes, "rb") as f:
            return f.read()

    def _opened(self, h):
        self._h = h
        st = (ctypes.c_uint64 * 7)()
        DeviceBoltStore._raise(_lib.load().dh_archive_stat(h, st))
        self._stat = [int(x) for x in st]

    @classmethod
    def from_packets(cls, kind, data, lens=None, offs=None):
        """Protobuf records of `kind` (PB_BEACON_PACKET: SyncChain's BeaconPacket, PB_PUBLIC_RAND: the
        relays' PublicRandResponse). data: bytes, a path, or a list of byte strings (joined here, one record each). lens
        (and optionally offs, the records' offsets; else they are packed from 0) frame the records of a buffer: a gossip
        subscriber or a raw gRPC codec holds them. With neither, the buffer is varint-delimited and framed on the host by
        dh_pb_frame_delimited (a convenience for files, off the hot path); the trailing bytes that frame no record are
        .unframed. Everything else is DeviceArchive's: deferred records go through packet_from_bytes."""
        lib = _lib.load()
        self = cls.__new__(cls)
        self._h = None
        self._resolved = {}
        self.kind = int(kind)
        if isinstance(data, (list, tuple)):
            if lens is not None or offs is not None:
                raise ValueError("a list of records frames itself")
            lens = np.array([len(b) for b in data], np.uint32)
            data = b"".join(bytes(b) for b in data)
        self._data = self._read(data)
        n_all = len(self._data)
        if lens is None:
            if offs is not None:
                raise ValueError("offs without lens")
            n, used = ctypes.c_size_t(0), ctypes.c_size_t(0)
            offs, lens = np.zeros(0, np.uint64), np.zeros(0, np.uint32)
            rc = lib.dh_pb_frame_delimited(self._data, n_all, None, None, 0, ctypes.byref(n), ctypes.byref(used))
            if n.value:  # DH_EINVAL with the count
                offs, lens = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint32)
                rc = lib.dh_pb_frame_delimited(self._data, n_all, ctypes.c_void_p(offs.ctypes.data), ctypes.c_void_p(lens.ctypes.data),
                                               n.value, ctypes.byref(n), ctypes.byref(used))
            DeviceBoltStore._raise(rc)
            self.unframed = self._data[used.value:]
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        if offs is not None:
            offs = np.ascontiguousarray(offs, dtype=np.uint64)
            if len(offs) != len(lens):
                raise ValueError("%d offsets, %d lengths" % (len(offs), len(lens)))
        h = ctypes.c_void_p()
        DeviceBoltStore._raise(lib.dh_archive_open_pb(self.kind, self._data, n_all, ctypes.c_void_p(offs.ctypes.data) if offs is not None and len(offs) else None,
                                                      ctypes.c_void_p(lens.ctypes.data) if len(lens) else None, len(lens), ctypes.byref(h)))
        self._opened(h)
        return self

    def close(self):
        if self._h is not None:
            _lib.load().dh_archive_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def __len__(self):
        return self._stat[0]

    def stat(self):
        return dict(zip(self.STAT, self._stat))

    def _window(self, first, n):
        first = int(first)
        n = max(0, len(self) - first) if n is None else int(n)
        return first, max(0, min(n, len(self) - first))

    def lines(self, first=0, n=None):
        """(byte offsets uint64[n], lengths uint32[n]) of records first .. first + n - 1; a line above 4096 bytes has
        length 4097 (a protobuf record: its payload's offset and true length, as the caller gave them)."""
        first, n = self._window(first, n)
        off, ln = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        DeviceBoltStore._raise(_lib.load().dh_archive_lines(self._h, first, n, ctypes.c_void_p(off.ctypes.data),
                                                            ctypes.c_void_p(ln.ctypes.data)))
        return off, ln

    def line(self, i):
        """The bytes of record i, from the host copy (whatever its length)."""
        off, ln = self.lines(i, 1)
        if not len(off):
            raise IndexError(i)
        if self.kind:
            return self._data[int(off[0]):int(off[0]) + int(ln[0])]
        end = self._data.find(b"\n", int(off[0]))
        return self._data[int(off[0]):end if end >= 0 else len(self._data)]

    def deferred(self, first=0, n=None):
        """Indices of the records the device leaves to the host decoder, ascending."""
        first, n = self._window(first, n)
        cap = max(1, self._stat[1])
        out = np.zeros(cap, np.uint64)
        k = ctypes.c_size_t(0)
        DeviceBoltStore._raise(_lib.load().dh_archive_deferred(self._h, first, n, ctypes.c_void_p(out.ctypes.data), cap, ctypes.byref(k)))
        return [int(x) for x in out[:k.value]]

    def default_stride(self, sig_len=0):
        return max(4, (max(int(sig_len), self._stat[3]) + 3) & ~3)

    def beacons_device(self, first=0, n=None, sig_stride=None, prev_stride=None, want_prev=True, want_rand=True):
        """Records first .. first + n - 1 in device memory: (rounds int64[n] (the u64 bit pattern), sigs uint8[n,
        sig_stride], sig_lens int32[n], prevs uint8[n, prev_stride] | None, prev_lens int32[n] | None, rands uint8[n, 32]
        | None, rand_lens int32[n] | None, deferred uint8[n]). Strides default to the archive's longest decoded field
        rounded up to 4. A value longer than its stride leaves a zero row and its true length; a deferred record is all
        zero."""
        import torch
        first, n = self._window(first, n)
        sig_stride = int(sig_stride or self.default_stride())
        prev_stride = int(prev_stride or max(4, (self._stat[4] + 3) & ~3))
        dev = torch.device("cuda")
        rounds = torch.empty(n, dtype=torch.int64, device=dev)
        sigs = torch.empty((n, sig_stride), dtype=torch.uint8, device=dev)
        sig_lens = torch.empty(n, dtype=torch.int32, device=dev)
        prevs = torch.empty((n, prev_stride), dtype=torch.uint8, device=dev) if want_prev else None
        prev_lens = torch.empty(n, dtype=torch.int32, device=dev) if want_prev else None
        rands = torch.empty((n, 32), dtype=torch.uint8, device=dev) if want_rand else None
        rand_lens = torch.empty(n, dtype=torch.int32, device=dev) if want_rand else None
        deferred = torch.empty(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ptr = lambda t: (t.data_ptr() or None) if t is not None else None  # noqa: E731
        k = ctypes.c_size_t(0)
        DeviceBoltStore._raise(_lib.load().dh_archive_beacons_device(
            self._h, first, n, sig_stride, prev_stride, ptr(rounds), ptr(sigs), ptr(sig_lens), ptr(prevs), ptr(prev_lens), ptr(rands),
            ptr(rand_lens), ptr(deferred), ctypes.byref(k), None))
        return rounds, sigs, sig_lens, prevs, prev_lens, rands, rand_lens, deferred

    def set_beacon_id(self, beacon_id):
        """The ID check() compares every record's metadata with (protobuf handles; None: no comparison)."""
        bid = _id_bytes(beacon_id)
        DeviceBoltStore._raise(_lib.load().dh_archive_set_beacon_id(self._h, bid, len(bid or b"")))

    def check_device(self, scheme, pubkey, anchor=None, window=1 << 20, seed=0):
        """dh_archive_check over the whole archive: (status uint8[records] with the deferred records marked
        DH_AR_DEFERRED and undecided, counts dict)."""
        n = len(self)
        status = np.zeros(n, np.uint8)
        counts = (ctypes.c_uint64 * 6)()
        a = _anchor_rec(anchor)
        ar = ctypes.c_uint64(a["round"]) if a else None
        rc = _lib.load().dh_archive_check(self._h, scheme.id, bytes(pubkey), len(pubkey), 0, n, ctypes.byref(ar) if a else None,
                                          a["signature"] if a else None, len(a["signature"]) if a else 0, int(window), int(seed),
                                          ctypes.c_void_p(status.ctypes.data), counts)
        if rc == _lib.DH_EINVAL and "64 KiB" in _lib.last_error():
            raise StrideTooLarge(_lib.last_error())
        DeviceBoltStore._raise(rc)
        return status, dict(zip(("checked", "deferred", "invalid", "randomness", "sequence", "link"), [int(x) for x in counts]))

    def resolve(self, i):
        """Record i through the host decoder: a dict, None (whitespace only) or False (it does not decode); cached."""
        if i not in self._resolved:
            try:
                self._resolved[i] = packet_from_bytes(self.kind, self.line(i)) if self.kind else random_data_from_line(self.line(i))
            except DECODE_ERRORS:
                self._resolved[i] = False
        return self._resolved[i]

    def check(self, scheme, pubkey, anchor=None, window=1 << 20, seed=0, beacon_id=None):
        """One status byte per record (numpy uint8; the DH_AR_* bits), equal to check_random_data_host over the same
        bytes. The device decides the canonical records; each deferred line is decided HERE, by random_data_from_line (this
        module's restatement, not a decoder pinned to nikkolasg/hexjson): a whitespace-only line is dropped from the
        result, one that does not decode gets DH_AR_INVALID, a decoded one is verified in one small verify_beacons call,
        and the predecessor bits are computed for it and for the record after it. A protobuf handle decides its deferred
        records with packet_from_bytes, equals check_packets_host, and compares each record's metadata with beacon_id
        (DH_AR_BEACON_ID; None: no comparison)."""
        if self.kind:
            self.set_beacon_id(beacon_id)
        elif beacon_id is not None:
            raise ValueError("a RandomData record carries no beacon ID")
        status, _ = self.check_device(scheme, pubkey, anchor, window, seed)
        todo = [int(i) for i in np.flatnonzero(status & (AR_DEFERRED | AR_PRED_DEFERRED))]
        if not todo:
            return status
        dec = {i: self.resolve(i) for i in todo if status[i] & AR_DEFERRED}
        ver = [r for r in dec.values() if r and len(r["signature"]) == scheme.sig_len]
        verdict = dict(zip(map(id, ver), _verify_records(scheme, pubkey, ver, seed)))

        def pred_of(i):  # the last record before i that decoded
            j = i - 1
            while j >= 0 and status[j] & AR_DEFERRED and not dec[j]:
                j -= 1
            return _anchor_rec(anchor) if j < 0 else (dec[j] if j in dec else self.resolve(j))

        out = status.copy()
        for i in todo:
            if status[i] & AR_DEFERRED:
                r = dec[i]
                out[i] = AR_INVALID if not r else (_own_bits(r, scheme.sig_len, verdict.get(id(r), False)) |
                                                   _pred_bits(r, pred_of(i), scheme.chained) | _id_bits(r, beacon_id))
            else:  # canonical, behind a deferred record
                out[i] = (int(status[i]) & ~AR_PRED_DEFERRED) | _pred_bits(self.resolve(i), pred_of(i), scheme.chained)
        keep = np.ones(len(out), bool)
        keep[[i for i, r in dec.items() if r is None]] = False
        return out[keep]


def archive_to_trimmed_store(archive, path, scheme, pubkey, anchor=None, window=STREAM_WINDOW, page_size=4096):
    """A RandomData archive -> a trimmed store file at `path` (the bulk form of appendStore / schemeStore Put,
    chain/beacon/store.go:55-77,99-124): DeviceArchive.check first, and a ValueError naming the first records when any
    bit but DH_AR_RANDOMNESS is set (the reference overwrites randomness, client/verify.go:197); then the windows' rounds
    / sigs / sig_lens columns go from the device into a BoltWriter (path + ".tmp", then os.replace). The file is byte for
    byte write_trimmed_bolt of the same rows. archive: a DeviceArchive, a path or the bytes. Returns BoltWriter.finish()'s
    dict."""
    import torch
    own = not isinstance(archive, DeviceArchive)
    ar = DeviceArchive(archive) if own else archive
    try:
        status = ar.check(scheme, pubkey, anchor=anchor, window=window)
        bad = np.flatnonzero(status & ~np.uint8(AR_RANDOMNESS))
        if len(bad):
            raise ValueError("%d of %d records do not pass: %s%s" % (len(bad), len(status), ", ".join(
                "#%d (status %d)" % (int(i), int(status[i])) for i in bad[:8]), ", ..." if len(bad) > 8 else ""))
        if not len(status):
            raise NoBeaconStored("the archive holds no record")
        window = max(1, min(int(window), MAX_CALL_ROWS))
        stride = max(4, (scheme.sig_len + 3) & ~3)
        with BoltWriter(path, page_size) as w:
            for at in range(0, len(ar), window):
                rounds, sigs, sig_lens, _p, _pl, _r, _rl, deferred = ar.beacons_device(at, window, sig_stride=stride, want_prev=False,
                                                                                       want_rand=False)
                idx = torch.nonzero(deferred).reshape(-1).cpu().tolist()
                if idx:  # decided by the host decoder in check(): patch the rows in, leave the blank lines out
                    keep = torch.ones(len(deferred), dtype=torch.bool, device=deferred.device)
                    for i in idx:
                        r = ar.resolve(at + i)
                        if r is None:
                            keep[i] = False
                            continue
                        rounds[i] = r["round"] - (1 << 64) if r["round"] >> 63 else r["round"]
                        sigs[i, :len(r["signature"])] = torch.frombuffer(bytearray(r["signature"]), dtype=torch.uint8).to(sigs.device)
                        sig_lens[i] = len(r["signature"])
                    rounds, sigs, sig_lens = rounds[keep], sigs[keep].contiguous(), sig_lens[keep]
                if len(rounds):
                    w.append(rounds, sigs, sig_lens)
            return w.finish()
    finally:
        if own:
            ar.close()


# ---- protobuf beacon records: BeaconPacket (protobuf/drand/protocol.proto:113-118 of the reference)
# and PublicRandResponse (protobuf/drand/api.proto:44-52), with common.Metadata / common.NodeVersion inside

_PB_NODE_VERSION = {1: ("u32", "major"), 2: ("u32", "minor"), 3: ("u32", "patch"), 4: ("str", "prerelease")}
_PB_METADATA = {1: ("msg", "node_version", _PB_NODE_VERSION), 2: ("str", "beacon_id"), 3: ("bytes", "chain_hash")}
_PB_SCHEMA = {
    PB_BEACON_PACKET: {1: ("bytes", "previous_signature"), 2: ("u64", "round"), 3: ("bytes", "signature"), 4: ("msg", "metadata", _PB_METADATA)},
    PB_PUBLIC_RAND: {1: ("u64", "round"), 2: ("bytes", "signature"), 3: ("bytes", "previous_signature"), 4: ("bytes", "randomness"),
                     5: ("msg", "metadata", _PB_METADATA)},
}
_PB_WIRE = {"u32": 0, "u64": 0, "str": 2, "bytes": 2, "msg": 2}


def _id_bytes(beacon_id):
    if beacon_id is None:
        return None
    return beacon_id.encode("utf-8") if isinstance(beacon_id, str) else bytes(beacon_id)


def _id_bits(rec, beacon_id):
    """DH_AR_BEACON_ID of a decoded record: metadata present and its beaconID is not the expected one (tryNode,
    chain/beacon/sync_manager.go:385-389); nothing without an expected ID."""
    if beacon_id is None or rec.get("beacon_id") is None:
        return 0
    return AR_BEACON_ID if _id_bytes(rec["beacon_id"]) != _id_bytes(beacon_id) else 0


def _pb_put_varint(out, v):
    while v >> 7:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)


def _pb_put(out, schema, rec):
    """proto.Marshal of a proto3 message: field-number order, zero / empty scalars left out, a sub-message written when
    it is present (not None), a string with explicit presence ("prerelease") likewise."""
    for num in sorted(schema):
        typ, name = schema[num][:2]
        v = rec.get(name)
        if typ == "msg":
            if v is None:
                continue
            body = bytearray()
            _pb_put(body, schema[num][2], v)
        elif typ in ("u32", "u64"):
            v = int(v or 0)
            if not 0 <= v < (1 << (32 if typ == "u32" else 64)):
                raise ValueError("%s = %d does not fit" % (name, v))
            if v:
                out.append(num << 3)
                _pb_put_varint(out, v)
            continue
        else:
            if name == "prerelease":
                if v is None:
                    continue
            elif not v:
                continue
            body = v.encode("utf-8") if isinstance(v, str) else bytes(v)
        out.append((num << 3) | 2)
        _pb_put_varint(out, len(body))
        out += body


def packet_bytes(kind, rec, beacon_id=None):
    """The wire form proto.Marshal writes for one record of `kind` (PB_BEACON_PACKET: beaconToProto,
    chain/beacon/convert.go:9-16; PB_PUBLIC_RAND). rec: {round, signature, previous_signature[, randomness][, metadata]};
    metadata: None (absent) or {beacon_id, chain_hash, node_version: None | {major, minor, patch, prerelease: None | str}}.
    beacon_id (str or bytes; "" writes the empty sub-message) is the short form of metadata = {"beacon_id": beacon_id}."""
    rec = dict(rec)
    if beacon_id is not None:
        rec["metadata"] = {"beacon_id": beacon_id}
    out = bytearray()
    _pb_put(out, _PB_SCHEMA[int(kind)], rec)
    return bytes(out)


def _pb_varint(b, i, most=10):
    """A varint of up to `most` bytes, minimal or not, cut to 64 bits: (value, the index after it)."""
    v = 0
    for k in range(most):
        if i + k >= len(b):
            raise ValueError("varint cut short")
        c = b[i + k]
        v |= (c & 0x7F) << (7 * k)
        if not c & 0x80:
            return v & _U64, i + k + 1
    raise ValueError("varint of more than %d bytes" % most)


def _pb_tag(b, i, in_group=False):
    tag, i = _pb_varint(b, i, 5)
    if tag >> 32 or not (tag >> 3 or in_group):  # upb lets number 0 pass inside a group it skips; Go does not
        raise ValueError("field number %d" % (tag >> 3))
    return tag >> 3, tag & 7, i


def _pb_skip(b, i, num, wt, depth=0):
    """The index after an unknown field's value (its tag already read); groups are walked to their end tag."""
    if wt == 0:
        return _pb_varint(b, i)[1]
    if wt == 1 or wt == 5:
        n = 8 if wt == 1 else 4
        if len(b) - i < n:
            raise ValueError("fixed value cut short")
        return i + n
    if wt == 2:
        n, i = _pb_len(b, i)
        return i + n
    if wt == 3:
        if depth >= 100:
            raise ValueError("groups nested too deep")
        while True:
            if i >= len(b):
                raise ValueError("group without end")
            n2, w2, i = _pb_tag(b, i, True)
            if w2 == 4:
                if n2 != num:
                    raise ValueError("end of another group")
                return i
            i = _pb_skip(b, i, n2, w2, depth + 1)
    raise ValueError("wire type %d" % wt)


def _pb_len(b, i):
    n, i = _pb_varint(b, i)
    if n >= (1 << 31) - 1 or n > len(b) - i:
        raise ValueError("length %d runs past the end" % n)
    return n, i


def _pb_merge(schema, b, into, depth=0):
    """Protobuf decoding of one message into `into`: last value wins, a repeated sub-message merges, unknown fields (and
    known numbers with another wire type) are skipped, strings are UTF-8."""
    if depth >= 100:
        raise ValueError("messages nested too deep")
    i = 0
    while i < len(b):
        num, wt, i = _pb_tag(b, i)
        f = schema.get(num)
        if f is None or _PB_WIRE[f[0]] != wt:
            i = _pb_skip(b, i, num, wt)
            continue
        typ, name = f[:2]
        if wt == 0:
            v, i = _pb_varint(b, i)
            into[name] = v & 0xFFFFFFFF if typ == "u32" else v
            continue
        n, i = _pb_len(b, i)
        body = bytes(b[i:i + n])
        i += n
        if typ == "msg":
            sub = into.get(name)
            if sub is None:
                sub = into[name] = {}
            _pb_merge(f[2], body, sub, depth + 1)
        else:
            into[name] = body.decode("utf-8") if typ == "str" else body
    return into


def packet_from_bytes(kind, b):
    """ONE protobuf record of `kind` -> {round, signature, previous_signature, randomness, metadata, beacon_id}: metadata
    None when absent, else {beacon_id, chain_hash, node_version} as far as they were sent; beacon_id = metadata's
    beaconID ("" when not sent), None without metadata. Raises ValueError for bytes that do not decode. This is the
    project's restatement of protobuf decoding for these two messages, not the Go decoder: it decides the records the
    device defers. Last value wins, a repeated sub-message merges, unknown fields of any wire type (groups included) and
    known numbers with another wire type are skipped, field number 0 is rejected, varints take up to 10 bytes, minimal
    or not, strings are validated as UTF-8."""
    d = _pb_merge(_PB_SCHEMA[int(kind)], bytes(b), {})
    meta = d.get("metadata")
    return {"round": d.get("round", 0), "signature": d.get("signature", b""), "previous_signature": d.get("previous_signature", b""),
            "randomness": d.get("randomness", b""), "metadata": meta, "beacon_id": None if meta is None else meta.get("beacon_id", "")}


def frame_delimited(data):
    """dh_pb_frame_delimited over bytes: ([payload], the trailing bytes that frame no record). Host only."""
    data = bytes(data)
    lib = _lib.load()
    n, used = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = lib.dh_pb_frame_delimited(data, len(data), None, None, 0, ctypes.byref(n), ctypes.byref(used))
    if not n.value:
        DeviceBoltStore._raise(rc)
        return [], data[used.value:]
    offs, lens = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint32)
    DeviceBoltStore._raise(lib.dh_pb_frame_delimited(data, len(data), ctypes.c_void_p(offs.ctypes.data), ctypes.c_void_p(lens.ctypes.data),
                                                     n.value, ctypes.byref(n), ctypes.byref(used)))
    return [data[int(o):int(o) + int(l)] for o, l in zip(offs, lens)], data[used.value:]


def delimited(records):
    """The records behind varint length prefixes, one buffer."""
    out = bytearray()
    for r in records:
        _pb_put_varint(out, len(r))
        out += r
    return bytes(out)


def check_packets_host(kind, records, scheme, pubkey, anchor=None, beacon_id=None, verify=None):
    """The serial host check of a run of protobuf records, the yardstick of DeviceArchive.from_packets(...).check: one
    status byte per record (the DH_AR_* bits, bits 1 and 64 never set), as check_random_data_host gives it, plus
    DH_AR_BEACON_ID for a record whose metadata is present with another beaconID than beacon_id (None: no comparison).
    records: the byte strings. One that packet_from_bytes rejects gets DH_AR_INVALID and is no predecessor."""
    verify = verify or _verify_records
    recs = []
    for b in records:
        try:
            recs.append(packet_from_bytes(kind, b))
        except DECODE_ERRORS:
            recs.append(False)
    todo = [r for r in recs if r and len(r["signature"]) == scheme.sig_len]
    verdict = dict(zip(map(id, todo), verify(scheme, pubkey, todo)))
    out = np.zeros(len(recs), np.uint8)
    pred = _anchor_rec(anchor)
    for i, r in enumerate(recs):
        if r is False:
            out[i] = AR_INVALID
            continue
        out[i] = _own_bits(r, scheme.sig_len, verdict.get(id(r), False)) | _pred_bits(r, pred, scheme.chained) | _id_bits(r, beacon_id)
        pred = r
    return out


def encode_beacon_packets(rounds, sigs, lens, prevs=None, prev_lens=None, beacon_id=None, delimited=False):
    """Verifier columns on the device -> beaconToProto's BeaconPacket bytes (dh_pb_encode_device): rounds int64[n], sigs
    uint8[n, stride], lens int32[n], prevs / prev_lens likewise or None (an unchained chain), as beacons_device gives them.
    beacon_id None: no metadata; "": the empty sub-message. delimited: a varint length before every packet. Returns
    (uint8 tensor on the device holding the packets back to back, int32 tensor of the packets' lengths without
    prefix)."""
    import torch
    n = len(rounds)
    bid = _id_bytes(beacon_id)
    rounds, sigs, lens = rounds.contiguous(), sigs.contiguous(), lens.contiguous()
    if prevs is not None:
        prevs, prev_lens = prevs.contiguous(), prev_lens.contiguous()
    rec_lens = torch.empty(n, dtype=torch.int32, device=rounds.device)
    torch.cuda.synchronize()
    ptr = lambda t: (t.data_ptr() or None) if t is not None else None  # noqa: E731
    total = ctypes.c_size_t(0)

    def call(out, cap):
        return _lib.load().dh_pb_encode_device(
            PB_BEACON_PACKET, ptr(rounds), ptr(sigs), sigs.shape[1] if sigs.dim() == 2 else 0, ptr(lens), ptr(prevs),
            prevs.shape[1] if prevs is not None else 0, ptr(prev_lens), n, bid, len(bid or b""), int(bool(delimited)), out, cap,
            ptr(rec_lens), ctypes.byref(total), None)
    DeviceBoltStore._raise(call(None, 0))
    out = torch.empty(total.value, dtype=torch.uint8, device=rounds.device)
    if total.value:
        torch.cuda.synchronize()
        DeviceBoltStore._raise(call(out.data_ptr(), total.value))
    return out, rec_lens


def _chain_windows(store, from_round, window, up_to=None):
    """The cursor loop the frame generators share: the stored rounds from from_round on (round 0 stands for the first
    stored round), a window of rounds at a time, as the columns the device encoders take: yields (rounds, sigs, lens,
    prevs, prev_lens) for every window that holds a row. A chained store's rows carry the stored previous signature: the
    row before in a trimmed store (NoBeaconStored when it is missing), PreviousSig in an untrimmed one; prevs and
    prev_lens are None for an unchained store. up_to: the last round wanted (default: the last stored)."""
    rng = store.rounds_range()
    if rng is None:
        return
    first, last = max(int(from_round), rng[0]), rng[1] if up_to is None else min(rng[1], int(up_to))
    window = max(1, min(int(window), MAX_CALL_ROWS - 1))
    while first <= last:
        hi = min(last, first + window - 1)
        if store.untrimmed:
            rounds, sigs, lens, prevs, prev_lens, deferred, _m = store.beacons_device(first, hi, want_prev=store.requires_previous)
            if int(deferred.sum()):
                raise ValueError("rounds %d..%d hold records the device defers" % (first, hi))
        else:
            lo = first - 1 if store.requires_previous and first > 0 else first
            rounds, rows, lens, _m = store.columns_device(lo, hi)
            prevs = prev_lens = None
            sigs = rows
            if store.requires_previous:
                k = int((rounds < first).sum()) if lo < first else 0  # the row of round first - 1, when stored
                r, rw, ln = rounds[k:], rows[k:], lens[k:]
                prevs, prev_lens = rw.new_zeros(rw.shape), ln.new_zeros(ln.shape)
                if len(r):
                    prevs[1:], prev_lens[1:] = rw[:-1], ln[:-1]
                    if k:
                        prevs[0], prev_lens[0] = rows[k - 1], lens[k - 1]
                    linked = r.new_zeros(len(r), dtype=bool)
                    linked[1:] = r[1:] == r[:-1] + 1
                    linked[0] = bool(k) and int(rounds[k - 1]) + 1 == int(r[0]) or int(r[0]) == 0
                    if not bool(linked.all()):
                        raise NoBeaconStored("round %d: the round before it is not stored" % int(r[~linked][0]))
                rounds, sigs, lens = r, rw.contiguous(), ln
        if len(rounds):
            yield rounds, sigs, lens, prevs, prev_lens
        first = hi + 1


def sync_chain_frames(store, from_round, beacon_id, window=STREAM_WINDOW, delimited=False):
    """SyncChain's cursor loop (chain/beacon/sync_manager.go:510-525) over a DeviceBoltStore, a window of rounds at a
    time: yields (frames uint8 tensor on the device, lengths int32 tensor) holding the BeaconPacket of every stored round
    from from_round on, in order (round 0 stands for the first stored round). A chained store's packets carry the stored
    previous signature: the row before in a trimmed store (NoBeaconStored when it is missing), PreviousSig in an
    untrimmed one."""
    for rounds, sigs, lens, prevs, prev_lens in _chain_windows(store, from_round, window):
        yield encode_beacon_packets(rounds, sigs, lens, prevs, prev_lens, beacon_id, delimited)


# ---- the records a node or relay serves, encoded on the device: client.RandomData through hexjson
# (http/server.go:336-342, cmd/relay-s3/main.go:127-141) and PublicRandResponse (core/convert.go:15-22)

def metadata_bytes(md):
    """proto.Marshal of common.Metadata from the dict packet_bytes takes under "metadata" ({beacon_id, chain_hash,
    node_version}): the body that follows a record's metadata tag and length. None (no metadata) gives None."""
    if md is None:
        return None
    out = bytearray()
    _pb_put(out, _PB_METADATA, md)
    return bytes(out)


def _encode_rand(form, rounds, sigs, lens, prevs, prev_lens, rands, keep, metadata, flags):
    import torch
    n = len(rounds)
    rounds, sigs, lens = rounds.contiguous(), sigs.contiguous(), lens.contiguous()
    if prevs is not None:
        prevs, prev_lens = prevs.contiguous(), prev_lens.contiguous()
    if rands is not None:
        rands = rands.contiguous()
        if rands.dtype != torch.uint8 or rands.numel() != 32 * n:
            raise ValueError("rands: uint8 rows of 32 bytes, one per row")
    if keep is not None:
        keep = keep.contiguous()
        if keep.dtype == torch.bool:
            keep = keep.view(torch.uint8)
        if keep.dtype != torch.uint8 or keep.numel() != n:
            raise ValueError("keep: one byte per row")
    if metadata is not None and not isinstance(metadata, (bytes, bytearray)):
        metadata = metadata_bytes(metadata)
    md = bytes(metadata) if metadata is not None else None
    rec_lens = torch.empty(n, dtype=torch.int32, device=rounds.device)
    torch.cuda.synchronize()
    ptr = lambda t: (t.data_ptr() or None) if t is not None else None  # noqa: E731
    total = ctypes.c_size_t(0)

    def call(out, cap):
        return _lib.load().dh_rand_encode_device(
            form, ptr(rounds), ptr(sigs), sigs.shape[1] if sigs.dim() == 2 else 0, ptr(lens), ptr(prevs),
            prevs.shape[1] if prevs is not None else 0, ptr(prev_lens), ptr(rands), ptr(keep), n, md, len(md or b""), flags, out, cap,
            ptr(rec_lens), ctypes.byref(total), None)
    DeviceBoltStore._raise(call(None, 0))
    out = torch.empty(total.value, dtype=torch.uint8, device=rounds.device)
    if total.value:
        torch.cuda.synchronize()
        DeviceBoltStore._raise(call(out.data_ptr(), total.value))
    return out, rec_lens


def encode_random_data(rounds, sigs, lens, prevs=None, prev_lens=None, rands=None, keep=None, newline=True):
    """Verifier columns on the device -> client.RandomData hexjson objects (dh_rand_encode_device), each byte for byte
    random_data_line of its row; the columns as for encode_beacon_packets. rands None: every record carries SHA-256 of
    its signature, computed on the device; else uint8[n, 32] copied as given (verify's randomness column). keep None:
    every row is written; else uint8[n] / bool[n], a row whose byte is 0 writes nothing (verify's verdict column).
    newline: b"\\n" after every record written. Returns (uint8 tensor on the device holding the records back to back,
    int32 tensor of the records' lengths without newline, 0 for a row left out)."""
    return _encode_rand(_lib.DH_ENC_RANDOM_DATA_JSON, rounds, sigs, lens, prevs, prev_lens, rands, keep, None,
                        _lib.DH_ENC_NEWLINE if newline else 0)


def encode_public_rand(rounds, sigs, lens, prevs=None, prev_lens=None, rands=None, keep=None, metadata=None, delimited=False):
    """Verifier columns on the device -> PublicRandResponse messages (dh_rand_encode_device), each byte for byte
    packet_bytes(PB_PUBLIC_RAND, ...) of its row. metadata: None (no field), the dict packet_bytes takes, or the
    marshalled common.Metadata bytes (b"" writes the empty sub-message). delimited: a varint length before every record
    written. Everything else as encode_random_data."""
    return _encode_rand(_lib.DH_ENC_PUBLIC_RAND_PB, rounds, sigs, lens, prevs, prev_lens, rands, keep, metadata,
                        _lib.DH_ENC_DELIMITED if delimited else 0)


def _keep_mask(rounds, skip):
    """The keep column for `rounds` (device, the u64 bit pattern) with the rounds of `skip` left out, built on the
    device; None when nothing is skipped."""
    import torch
    skip = np.array(sorted(set(int(r) for r in skip)), dtype=np.uint64)
    if not len(skip):
        return None
    return (~torch.isin(rounds, torch.from_numpy(skip.view(np.int64)).to(rounds.device))).to(torch.uint8)


def random_data_frames(store, from_round=1, window=STREAM_WINDOW, skip=(), newline=True, up_to=None):
    """The RandomData hexjson object of every stored round from from_round on (up to up_to, default the last), a window
    of rounds at a time, over a DeviceBoltStore of either format: yields (records uint8 tensor on the device, lengths
    int32 tensor) per window, with the windows and previous signatures of sync_chain_frames. skip: rounds to leave out
    (their length is 0, they write nothing)."""
    for rounds, sigs, lens, prevs, prev_lens in _chain_windows(store, from_round, window, up_to):
        yield encode_random_data(rounds, sigs, lens, prevs, prev_lens, keep=_keep_mask(rounds, skip), newline=newline)


def public_rand_frames(store, from_round, metadata=None, window=STREAM_WINDOW, skip=(), delimited=False, up_to=None):
    """PublicRand / PublicRandStream's backlog (core/drand_beacon_public.go:67-119) over a DeviceBoltStore: the
    PublicRandResponse of every stored round from from_round on, yielded as random_data_frames yields its records.
    metadata: None, the dict packet_bytes takes, or the marshalled common.Metadata bytes."""
    md = metadata_bytes(metadata) if isinstance(metadata, dict) else metadata
    for rounds, sigs, lens, prevs, prev_lens in _chain_windows(store, from_round, window, up_to):
        yield encode_public_rand(rounds, sigs, lens, prevs, prev_lens, keep=_keep_mask(rounds, skip), metadata=md, delimited=delimited)


def export_random_data(store, path, scheme=None, pubkey=None, up_to=None, window=STREAM_WINDOW):
    """A DeviceBoltStore written out as a RandomData JSON-lines archive: one hexjson object and b"\\n" per stored round
    from round 1 up to up_to (default the last). With a scheme and key store.check_past runs first and the faulty rounds
    are left out. The windows stream into path + ".tmp", which then replaces path. Returns {"records", "bytes",
    "faulty"}."""
    rng = store.rounds_range()
    last = rng[1] if rng else 0
    up_to = last if up_to is None else min(int(up_to), last)
    faulty = []
    if scheme is not None and rng:
        faulty = [int(r) for r in store.check_past(scheme, pubkey, up_to)]
    records = nbytes = 0
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            for out, rec_lens in random_data_frames(store, 1, window, skip=faulty, up_to=up_to):
                f.write(out.cpu().numpy().tobytes())
                records += int((rec_lens > 0).sum())
                nbytes += int(out.numel())
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return {"records": records, "bytes": nbytes, "faulty": faulty}


# ---- one chain from many unordered sources: dh_assemble_device and its host restatement

AS_CHOSEN, AS_DUPLICATE, AS_INVALID = _lib.DH_AS_CHOSEN, _lib.DH_AS_DUPLICATE, _lib.DH_AS_INVALID
AS_STALE, AS_SKIPPED, AS_CONFLICT = _lib.DH_AS_STALE, _lib.DH_AS_SKIPPED, _lib.DH_AS_CONFLICT
AS_GAP, AS_LINK = _lib.DH_AS_GAP, _lib.DH_AS_LINK
AS_COUNTS = ("candidates", "skipped", "stale", "verified", "invalid", "duplicates", "conflicts", "chosen", "missing", "link_breaks")


def _contiguous_up_to(rounds, flags, anchor):
    """Rule 8: the last round of the output rows' longest prefix with neither flag set; the anchor's round (0 without
    one) when that prefix is empty."""
    nz = np.flatnonzero(np.asarray(flags))
    k = int(nz[0]) if len(nz) else len(rounds)
    return int(rounds[k - 1]) if k else (int(anchor[0]) if anchor is not None else 0)


def assemble_host(candidates, scheme, pubkey, anchor=None, up_to=None, verify=None):
    """The serial definition of dh_assemble_device and the yardstick of assemble_columns: one chain from candidate
    records in any order. candidates: dicts {"round", "signature", "previous_signature" (chained), "skip" (optional)} in
    input order. Rules, in order: a candidate with `skip` is SKIPPED; round 0, a round at or below the anchor's or above
    up_to is STALE; a candidate whose (round, signature[, previous_signature]) an earlier live candidate has is a
    DUPLICATE with that one's INVALID bit; every other is a representative, verified once (against its OWN
    previous_signature), INVALID when its signature has another length than the scheme's or does not verify; the first
    valid representative of a round is CHOSEN, any other one a CONFLICT. The chosen rows ascend by round with flags GAP
    (not the row before's round + 1) and LINK (chained, consecutive: previous_signature is not that row's signature),
    the anchor (round, signature) standing before row 0. verify(scheme, pubkey, records) -> [bool] replaces the device
    verifier (the CPU tests pass the oracle). Returns {"status", "rounds", "src", "flags", "gaps", "counts",
    "contiguous_up_to"}."""
    verify = verify or _verify_records
    a = _anchor_rec(anchor)
    n = len(candidates)

    def key(c):
        return (int(c["round"]), bytes(c["signature"]), bytes(c.get("previous_signature") or b"") if scheme.chained else b"")

    status = [0] * n
    seen, reps = {}, []  # key -> its representative's position; the representatives in input order
    for i, c in enumerate(candidates):
        rnd = int(c["round"])
        if c.get("skip"):
            status[i] = AS_SKIPPED
        elif rnd == 0 or (a is not None and rnd <= a["round"]) or (up_to is not None and rnd > int(up_to)):
            status[i] = AS_STALE
        elif key(c) in seen:
            status[i] = AS_DUPLICATE  # its INVALID bit follows below
        else:
            seen[key(c)] = i
            reps.append(i)
    todo = [i for i in reps if len(candidates[i]["signature"]) == scheme.sig_len]
    recs = [dict(zip(("round", "signature", "previous_signature"), key(candidates[i]))) for i in todo]
    valid = dict(zip(todo, verify(scheme, pubkey, recs))) if todo else {}
    chosen = {}
    for i in reps:
        rnd = int(candidates[i]["round"])
        if not valid.get(i, False):
            status[i] = AS_INVALID
        elif rnd in chosen:
            status[i] = AS_CONFLICT
        else:
            chosen[rnd] = i
            status[i] = AS_CHOSEN
    for i, c in enumerate(candidates):
        if status[i] == AS_DUPLICATE and not valid.get(seen[key(c)], False):
            status[i] |= AS_INVALID
    rounds = sorted(chosen)
    src = [chosen[r] for r in rounds]
    flags, gaps = [], []
    before = a
    for r, i in zip(rounds, src):
        f = 0
        if before is not None:
            if r != before["round"] + 1:
                f = AS_GAP
                gaps.append((before["round"] + 1, r - 1))
            elif scheme.chained and bytes(candidates[i].get("previous_signature") or b"") != before["signature"]:
                f = AS_LINK
        flags.append(f)
        before = {"round": r, "signature": bytes(candidates[i]["signature"])}
    if up_to is not None and before is not None and before["round"] < int(up_to):
        gaps.append((before["round"] + 1, int(up_to)))
    st = np.array(status, np.uint8)
    counts = [n, int(((st & AS_SKIPPED) != 0).sum()), int(((st & AS_STALE) != 0).sum()), len(reps), int(((st & AS_INVALID) != 0).sum()),
              int(((st & AS_DUPLICATE) != 0).sum()), int(((st & AS_CONFLICT) != 0).sum()), len(rounds),
              sum(b - a_ + 1 for a_, b in gaps), sum(1 for f in flags if f & AS_LINK)]
    return {"status": st, "rounds": rounds, "src": src, "flags": flags, "gaps": gaps, "counts": dict(zip(AS_COUNTS, counts)),
            "contiguous_up_to": _contiguous_up_to(rounds, flags, anchor)}


class Assembled:
    """What assemble_columns returns: the chain's columns on the device (rounds int64 carrying the u64 bit pattern, sigs
    uint8[m, stride], lens int32, prevs / prev_lens for the chained scheme or None), src int32[m] (output row -> input
    position), flags uint8[m] (AS_GAP / AS_LINK), and on the host status uint8[n] (the AS_* bits per candidate), gaps
    [(first, last)], counts {AS_COUNTS} and contiguous_up_to."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __len__(self):
        return int(self.rounds.numel())

    def per_source(self, source_ids):
        """{source: {"candidates", "chosen", "duplicates", "invalid", "stale", "skipped", "conflicts"}} for source_ids, one
        small non-negative integer per candidate: numpy.bincount over the status."""
        ids = np.asarray(source_ids).reshape(-1).astype(np.int64)
        if len(ids) != len(self.status):
            raise ValueError("%d source ids for %d candidates" % (len(ids), len(self.status)))
        k = int(ids.max()) + 1 if len(ids) else 0
        cols = {"candidates": np.bincount(ids, minlength=k)}
        for name, bit in (("chosen", AS_CHOSEN), ("duplicates", AS_DUPLICATE), ("invalid", AS_INVALID), ("stale", AS_STALE),
                          ("skipped", AS_SKIPPED), ("conflicts", AS_CONFLICT)):
            cols[name] = np.bincount(ids, weights=(self.status & bit) != 0, minlength=k).astype(np.int64)
        return {s: {name: int(v[s]) for name, v in cols.items()} for s in range(k)}


def assemble_columns(scheme, pubkey, rounds, sigs, lens, prevs=None, prev_lens=None, skip=None, anchor=None, up_to=None, window=1 << 20,
                     seed=0, want_prev=True):
    """dh_assemble_device over torch device tensors (rounds int64[n] carrying the u64 bit pattern, sigs uint8[n, stride],
    lens int32[n], prevs / prev_lens likewise for the chained scheme, skip uint8[n] or None): candidates in any order,
    from any number of sources -> an Assembled. The rules are assemble_host's. want_prev=False leaves the chained
    scheme's previous_signature output columns out."""
    import torch
    lib = _lib.load()
    dev = torch.device("cuda")
    n = int(rounds.numel())
    if n > MAX_CALL_ROWS:
        raise ValueError("%d candidates: at most %d per call" % (n, MAX_CALL_ROWS))
    chained = bool(scheme.chained)
    if chained and n and (prevs is None or prev_lens is None):
        raise ValueError("the chained scheme needs prevs and prev_lens")
    if not chained:
        prevs = prev_lens = None
    cont = lambda t: t.contiguous() if t is not None else None  # noqa: E731
    rounds, sigs, lens, prevs, prev_lens, skip = cont(rounds), cont(sigs), cont(lens), cont(prevs), cont(prev_lens), cont(skip)
    stride = int(sigs.shape[1]) if sigs.dim() == 2 else 0
    pstride = int(prevs.shape[1]) if prevs is not None else 0
    out_prev = chained and want_prev
    o_rounds = torch.empty(n, dtype=torch.int64, device=dev)
    o_sigs = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    o_lens = torch.empty(n, dtype=torch.int32, device=dev)
    o_prevs = torch.empty((n, pstride), dtype=torch.uint8, device=dev) if out_prev else None
    o_prev_lens = torch.empty(n, dtype=torch.int32, device=dev) if out_prev else None
    o_src = torch.empty(n, dtype=torch.int32, device=dev)
    o_flags = torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ptr = lambda t: (t.data_ptr() or None) if t is not None else None  # noqa: E731
    a = _anchor_rec(anchor)
    ar = ctypes.c_uint64(a["round"]) if a else None
    ut = ctypes.c_uint64(int(up_to)) if up_to is not None else None
    status = np.zeros(n, np.uint8)
    counts = (ctypes.c_uint64 * 10)()
    m, ng = ctypes.c_size_t(0), ctypes.c_size_t(0)
    cap = 1024
    while True:
        gf, gl = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
        rc = lib.dh_assemble_device(
            scheme.id, bytes(pubkey), len(pubkey), ptr(rounds), ptr(sigs), stride, ptr(lens), ptr(prevs), pstride, ptr(prev_lens), ptr(skip), n,
            ctypes.byref(ar) if a else None, a["signature"] if a else None, len(a["signature"]) if a else 0,
            ctypes.byref(ut) if ut is not None else None, int(window), int(seed), ptr(o_rounds), ptr(o_sigs), ptr(o_lens), ptr(o_prevs),
            ptr(o_prev_lens), ptr(o_src), ptr(o_flags), ctypes.byref(m), ctypes.c_void_p(status.ctypes.data),
            ctypes.c_void_p(gf.ctypes.data), ctypes.c_void_p(gl.ctypes.data), cap, ctypes.byref(ng), counts, None)
        if rc == _lib.DH_EINVAL and ng.value > cap:  # the dh_archive_deferred convention: the number needed
            cap = ng.value
            continue
        DeviceBoltStore._raise(rc)
        break
    k = m.value
    flags = o_flags[:k]
    h_rounds, h_flags = o_rounds[:k].cpu().numpy().view(np.uint64), flags.cpu().numpy()
    return Assembled(rounds=o_rounds[:k], sigs=o_sigs[:k], lens=o_lens[:k], prevs=o_prevs[:k] if out_prev else None,
                     prev_lens=o_prev_lens[:k] if out_prev else None, src=o_src[:k], flags=flags, status=status,
                     gaps=[(int(x), int(y)) for x, y in zip(gf[:ng.value], gl[:ng.value])], counts=dict(zip(AS_COUNTS, [int(x) for x in counts])),
                     contiguous_up_to=_contiguous_up_to(h_rounds, h_flags, anchor))


def _u64_to_i64(r):
    r = int(r)
    return r - (1 << 64) if r >> 63 else r


def _source_columns(src, scheme, stride):
    """One source of assemble_archives as (rounds, sigs, lens, prevs | None, prev_lens | None, skip) device tensors at
    `stride`: a DeviceArchive (either kind; its deferred records resolved on the host and patched in, one that does not
    decode or is blank sets skip), a DeviceBoltStore (its round records), or a tuple of columns (host or device)."""
    import torch
    dev = torch.device("cuda")
    chained = bool(scheme.chained)

    def patch(cols, resolve_row):
        rounds, sigs, lens, prevs, prev_lens, deferred = cols
        skip = torch.zeros(len(rounds), dtype=torch.uint8, device=dev)
        for i in torch.nonzero(deferred).reshape(-1).cpu().tolist():
            r = resolve_row(i)
            if not r or len(r["signature"]) > stride or (chained and len(r["previous_signature"]) > stride):
                skip[i] = 1
                continue
            rounds[i] = _u64_to_i64(r["round"])
            sigs[i, :len(r["signature"])] = torch.frombuffer(bytearray(r["signature"]), dtype=torch.uint8).to(dev)
            lens[i] = len(r["signature"])
            if chained and r["previous_signature"]:
                prevs[i, :len(r["previous_signature"])] = torch.frombuffer(bytearray(r["previous_signature"]), dtype=torch.uint8).to(dev)
                prev_lens[i] = len(r["previous_signature"])
        return rounds, sigs, lens, prevs, prev_lens, skip

    if isinstance(src, DeviceArchive):
        parts = []
        for at in range(0, len(src), MAX_CALL_ROWS):
            rounds, sigs, lens, prevs, prev_lens, _r, _rl, deferred = src.beacons_device(at, MAX_CALL_ROWS, sig_stride=stride, prev_stride=stride,
                                                                                         want_prev=chained, want_rand=False)
            parts.append(patch((rounds, sigs, lens, prevs, prev_lens, deferred), lambda i, at=at: src.resolve(at + i)))
        if not parts:
            parts = [(torch.empty(0, dtype=torch.int64, device=dev), torch.empty((0, stride), dtype=torch.uint8, device=dev),
                      torch.empty(0, dtype=torch.int32, device=dev), torch.empty((0, stride), dtype=torch.uint8, device=dev) if chained else None,
                      torch.empty(0, dtype=torch.int32, device=dev) if chained else None, torch.empty(0, dtype=torch.uint8, device=dev))]
        cat = lambda k: torch.cat([p[k] for p in parts]) if parts[0][k] is not None else None  # noqa: E731
        return tuple(cat(k) for k in range(6))
    if isinstance(src, DeviceBoltStore):
        rng = src.rounds_range()
        if not rng:
            none = (np.zeros(0, np.uint64), np.zeros((0, stride), np.uint8), np.zeros(0, np.uint32))
            return _source_columns(none + (none[1:] if chained else ()), scheme, stride)
        if not src.untrimmed:  # a trimmed store implies its previous signatures: the row before, where it is round - 1
            rounds, sigs, lens, _missing = src.columns_device(rng[0], rng[1], max(stride, src._stride()))
            if sigs.shape[1] > stride:  # a value longer than the common stride: a zero row with its true length
                sigs = torch.where((lens <= stride)[:, None], sigs[:, :stride], torch.zeros_like(sigs[:, :stride])).contiguous()
            prevs = prev_lens = None
            if chained:
                prevs, prev_lens = torch.zeros_like(sigs), torch.zeros_like(lens)
                if len(rounds) > 1:
                    follows = (rounds[1:] == rounds[:-1] + 1) & (lens[:-1] <= stride)
                    prevs[1:][follows] = sigs[:-1][follows]
                    prev_lens[1:][follows] = lens[:-1][follows]
            return rounds, sigs, lens, prevs, prev_lens, torch.zeros(len(rounds), dtype=torch.uint8, device=dev)
        rounds, sigs, lens, prevs, prev_lens, deferred, _missing = src.beacons_device(rng[0], rng[1], sig_stride=stride, prev_stride=stride,
                                                                                      want_prev=chained)
        h_rounds = rounds.cpu().numpy().view(np.uint64)

        def resolve(i):
            try:
                b = beacon_from_hexjson(src._raw(int(h_rounds[i])))
            except DECODE_ERRORS:
                return False
            return {"round": int(b.round), "signature": bytes(b.signature), "previous_signature": bytes(b.previous_signature or b"")}
        return patch((rounds, sigs, lens, prevs, prev_lens, deferred), resolve)
    cols = tuple(src)
    if len(cols) not in (3, 5):
        raise ValueError("a column source is (rounds, sigs, lens) or (rounds, sigs, lens, prevs, prev_lens)")
    rounds, sigs, lens = _device_columns(*cols[:3])
    prevs = prev_lens = None
    if chained:
        if len(cols) != 5:
            raise ValueError("the chained scheme needs prevs and prev_lens")
        _r, prevs, prev_lens = _device_columns(rounds, cols[3], cols[4])

    def widen(t):  # to the common stride; a narrower source is zero-padded, a wider one must hold no longer value
        if t.shape[1] == stride:
            return t
        out = torch.zeros((t.shape[0], stride), dtype=torch.uint8, device=dev)
        w = min(stride, int(t.shape[1]))
        out[:, :w] = t[:, :w]
        return out
    skip = torch.zeros(len(rounds), dtype=torch.uint8, device=dev)
    for t, l in ((sigs, lens), (prevs, prev_lens)):
        if t is not None and t.shape[1] > stride and len(l) and int(l.max()) > stride:
            raise ValueError("a value of %d bytes in a column source: the common stride is %d" % (int(l.max()), stride))
    return rounds, widen(sigs), lens, widen(prevs) if prevs is not None else None, prev_lens, skip


def assemble_archives(sources, scheme, pubkey, anchor=None, up_to=None, window=1 << 20, seed=0, want_prev=True):
    """One assemble_columns call over any mix of sources: DeviceArchive handles (JSON lines or protobuf records),
    DeviceBoltStore handles, and (rounds, sigs, lens[, prevs, prev_lens]) column tuples. The columns are concatenated at
    one stride, roundup4(the scheme's signature length): a decoded value longer than that is an all-zero row with its
    true length (the device gather's rule) and so invalid. Records the device defers are decoded here and patched into
    the columns; one that does not decode, or a blank line, sets `skip`. Returns (Assembled, source_ids): source_ids
    int32[n] names each candidate's source, for Assembled.per_source."""
    import torch
    stride = max(4, (scheme.sig_len + 3) & ~3)
    parts = [_source_columns(s, scheme, stride) for s in sources]
    ids = np.concatenate([np.full(len(p[0]), k, np.int32) for k, p in enumerate(parts)]) if parts else np.zeros(0, np.int32)
    dev = torch.device("cuda")
    if not parts:
        parts = [(torch.empty(0, dtype=torch.int64, device=dev), torch.empty((0, stride), dtype=torch.uint8, device=dev),
                  torch.empty(0, dtype=torch.int32, device=dev), None, None, torch.empty(0, dtype=torch.uint8, device=dev))]
    cat = lambda k: torch.cat([p[k] for p in parts])  # noqa: E731
    chained = bool(scheme.chained)
    res = assemble_columns(scheme, pubkey, cat(0), cat(1), cat(2), cat(3) if chained else None, cat(4) if chained else None, cat(5),
                           anchor=anchor, up_to=up_to, window=window, seed=seed, want_prev=want_prev)
    return res, ids


def _assemble_refusal(res):
    breaks = [int(r) for r, f in zip(res.rounds.cpu().numpy().view(np.uint64), res.flags.cpu().numpy()) if f & AS_LINK]
    return "the sources do not support one chain: %d gaps (%s%s), %d link breaks (%s%s)" % (
        len(res.gaps), ", ".join("%d-%d" % g for g in res.gaps[:8]), ", ..." if len(res.gaps) > 8 else "",
        len(breaks), ", ".join(map(str, breaks[:8])), ", ..." if len(breaks) > 8 else "")


def assemble_to_trimmed_store(sources, path, scheme, pubkey, anchor=None, allow_gaps=False, up_to=None, window=STREAM_WINDOW, seed=0,
                              page_size=4096):
    """The chain that `sources` (as assemble_archives takes them) support -> a trimmed store file at `path`: one
    assemble, then the chosen rows stream from the device into a BoltWriter, `window` rows at a time. A gap or a link
    break raises ValueError naming the first of them unless allow_gaps; so does an empty chain (NoBeaconStored). With a
    clean result the file is byte for byte write_trimmed_bolt of the same rows. Returns BoltWriter.finish()'s dict with
    "assembled": the Assembled and "source_ids"."""
    res, ids = assemble_archives(sources, scheme, pubkey, anchor=anchor, up_to=up_to, window=window, seed=seed, want_prev=False)
    if not allow_gaps and (res.gaps or res.counts["link_breaks"] or bool((res.flags != 0).any())):
        raise ValueError(_assemble_refusal(res))
    if not len(res):
        raise NoBeaconStored("the sources hold no valid record")
    window = max(1, min(int(window), MAX_CALL_ROWS))
    with BoltWriter(path, page_size) as w:
        for at in range(0, len(res), window):
            w.append(res.rounds[at:at + window], res.sigs[at:at + window], res.lens[at:at + window])
        out = w.finish()
    return dict(out, assembled=res, source_ids=ids)
