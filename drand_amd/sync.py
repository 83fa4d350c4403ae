"""Batch caller for chain replay: SyncManager.CheckPastBeacons over libdrandhip.

Mirrors /root/reference/chain/beacon/sync_manager.go:170-235 exactly, except that the per-round
VerifyBeacon loop body becomes one dh_verify_batch per window of rounds:
  * up_to is clamped to the last stored round;
  * rounds 1 .. store_len-1 are visited in order (store_len counts stored beacons, genesis included —
    so, as in the reference, a missing beacon shortens the walk by one);
  * a store Get error makes the round faulty; a verification failure records the beacon's round;
  * the walk stops after round >= up_to; the result is ascending; the callback sees every round first.
The store model is the bbolt "trimmed" layout (/root/reference/chain/boltdb/trimmed.go:87-107,156-193):
key = round, value = signature; for chained schemes Get(r) rebuilds PreviousSig from the stored signature of
round r-1 and fails if that one is missing (the genesis "signature" at round 0 is the genesis seed).
"""
import queue
import threading
import time

import numpy as np

from .chain import Beacon


class NoBeaconStored(KeyError):
    """chain/errors.ErrNoBeaconStored"""


class TrimmedMemStore:
    """In-memory store with the trimmed-bolt Get semantics."""

    def __init__(self, requires_previous):
        self.requires_previous = requires_previous
        self._sigs = {}

    def put(self, round_, sig):
        self._sigs[int(round_)] = bytes(sig)

    def delete(self, round_):
        self._sigs.pop(int(round_), None)

    def len(self):
        return len(self._sigs)

    def last(self):
        if not self._sigs:
            raise NoBeaconStored("empty store")
        return self.get(max(self._sigs))

    def get(self, round_):
        round_ = int(round_)
        sig = self._sigs.get(round_)
        if sig is None:
            raise NoBeaconStored(round_)
        prev = b""
        if self.requires_previous and round_ > 0:
            prev = self._sigs.get(round_ - 1)
            if prev is None:
                raise NoBeaconStored(round_ - 1)
        return Beacon(round_, sig, prev)


def check_past_beacons(store, scheme, pubkey, up_to, cb=None, window=1 << 20, seed=0):
    """Faulty rounds (ascending) among the stored rounds 1 .. min(up_to, last); [] when all verify. A
    store.DeviceBoltStore takes the whole loop to the device in one dh_store_check_past call (cb then sees the first
    round of every window, not every round); only when the library refuses the file (too large for the device) or a
    window (a stored record above 64 KiB) does the loop below run, over a BoltTrimmedStore (BoltUntrimmedStore for an
    untrimmed store) of the same file. A record the store cannot decode is a Get error: the round is faulty."""
    from . import store as _store
    if isinstance(store, _store.DeviceBoltStore):
        try:
            return store.open().check_past(scheme, pubkey, up_to, cb=cb, window=window, seed=seed)
        except (_store.StoreTooLarge, _store.StrideTooLarge):
            untrimmed = store.untrimmed
            if untrimmed is None:  # refused at open: the file decides, as open() would have
                untrimmed = store.fmt == "untrimmed" or (store.fmt == "auto" and _store.looks_untrimmed(store.path))
            store = (_store.BoltUntrimmedStore if untrimmed else _store.BoltTrimmedStore)(store.path, store.requires_previous)
    last = store.last()
    if last.round < up_to:
        up_to = last.round
    store_len = store.len()
    faulty = []
    pending = []  # (round, beacon) awaiting batch verification, in order

    def flush():
        if not pending:
            return
        rounds = np.array([b.round for _, b in pending], dtype=np.uint64)
        sigs = np.zeros((len(pending), scheme.sig_len), dtype=np.uint8)
        bad_len = np.zeros(len(pending), dtype=bool)
        for k, (_, b) in enumerate(pending):
            if len(b.signature) == scheme.sig_len:
                sigs[k] = np.frombuffer(b.signature, dtype=np.uint8)
            else:
                bad_len[k] = True  # an all-zero record never decodes: rejected like kyber's length check
        prevs = [b.previous_signature for _, b in pending] if scheme.chained else None
        ok, _ = scheme.verify_beacons(pubkey, rounds, sigs, prevs, seed=seed, want_randomness=False)
        for (_, b), v, bl in zip(pending, ok, bad_len):
            if bl or not v:
                faulty.append(b.round)
        pending.clear()

    i = 1
    while i < store_len:
        if cb is not None:
            cb(i, up_to)
        try:
            b = store.get(i)
        except (NoBeaconStored,) + _store.DECODE_ERRORS:  # a stored record its decoder rejects: Beacon.Unmarshal's error
            flush()  # keep the faulty list ascending
            faulty.append(i)
            if i >= up_to:
                break
            i += 1
            continue
        pending.append((i, b))
        if len(pending) >= window:
            flush()
        if i >= up_to:
            break
        i += 1
    flush()
    return faulty


def correct_store_file(src, dst, scheme, pubkey, fetch, up_to=None, fmt="auto", window=None):
    """CheckPastBeacons followed by CorrectPastBeacons (chain/beacon/sync_manager.go:170-268 of the reference), offline,
    from the store file `src` to a new trimmed store file `dst` (the daemon is stopped, `dst` is renamed
    over `src` by the caller when it is satisfied):
      1. check_past over `src` on the device: the faulty rounds up to `up_to` (default: the last stored round);
      2. fetch(round) -> signature bytes | None, once per faulty round (the caller's network code);
      3. ONE scheme.verify_beacons call over the fetched records; for the chained scheme the previous signature of
         round r is the fetched signature of r - 1 when there is one, else the stored one;
      4. only the records that verify become patches of DeviceBoltStore.save_trimmed(dst);
      5. `dst` is reopened and checked again.
    Returns (faulty_before, faulty_after, unlinked): the two checks' lists and save_trimmed's unlinked rounds.
    window: save_trimmed's (stored rows per window of the streaming writer); the file is the same.

    Deviation from the reference: CorrectPastBeacons re-syncs the faulty rounds through the sync manager, where every
    streamed packet carries its own PreviousSig and is verified against it, and later packets can build on earlier
    ones as they are stored. This is one conservative pass: a fetched record is judged against its fetched or stored
    neighbour exactly once, a record that does not verify in that pass is not written, and nothing is retried; rounds
    left faulty are in faulty_after for the caller to fetch again."""
    from . import store as _store
    with _store.DeviceBoltStore(src, scheme.chained, fmt=fmt) as st:
        rng = st.rounds_range()
        if rng is None:
            raise NoBeaconStored("empty store")
        if up_to is None:
            up_to = rng[1]
        faulty_before = st.check_past(scheme, pubkey, up_to)
        fetched = {}
        for r in faulty_before:
            sig = fetch(r)
            if sig is not None:
                fetched[int(r)] = bytes(sig)
        cand = [r for r in sorted(fetched) if len(fetched[r]) == scheme.sig_len]
        patches = {}
        if cand:
            prevs = None
            if scheme.chained:
                prevs = []
                for r in cand:
                    if r - 1 in fetched:
                        prevs.append(fetched[r - 1])
                        continue
                    try:
                        prevs.append(st.stored_signature(r - 1))
                    except (NoBeaconStored,) + _store.DECODE_ERRORS:
                        prevs.append(b"")  # nothing to verify against: the record is not written
            rounds = np.array(cand, dtype=np.uint64)
            sigs = np.frombuffer(b"".join(fetched[r] for r in cand), np.uint8).reshape(len(cand), scheme.sig_len).copy()
            ok, _ = scheme.verify_beacons(pubkey, rounds, sigs, prevs, want_randomness=False)
            patches = {r: fetched[r] for r, v in zip(cand, ok) if v}
        res = st.save_trimmed(dst, patches=patches, window=window)
    with _store.DeviceBoltStore(dst, scheme.chained, fmt="trimmed") as out:
        faulty_after = out.check_past(scheme, pubkey, up_to)
    return faulty_before, faulty_after, res["unlinked"]


class WrongBeaconID(Exception):
    pass


class BeaconAlreadyStored(Exception):
    """chain/beacon.ErrBeaconAlreadyStored (/root/reference/chain/beacon/store.go:52-53)."""


class PutError(Exception):
    """Any other error of the chain store's Put (store.go:55-77, 99-124)."""


class ChainStore:
    """The Put checks of the beacon chain store stack that tryNode writes through (s.store,
    /root/reference/chain/beacon/chainstore.go:45-60: callbackStore -> appendStore -> schemeStore ->
    discrepancyStore -> the trimmed bolt store). `store` is the underlying trimmed store (TrimmedMemStore or a
    writable equivalent); both decorators start from its Last() beacon (newAppendStore / NewSchemeStore).
      appendStore.Put (store.go:55-77): same round as the last one -> ErrBeaconAlreadyStored if signature and
        previous signature are equal, an error if either differs; any round other than last+1 -> error.
      schemeStore.Put (store.go:99-124): chained (DefaultSchemeID) -> the previous signature must equal the last
        stored signature; other schemes -> the previous signature is dropped (b.PreviousSig = nil, on the same
        beacon object, so appendStore's `last` keeps no previous signature either).
    The discrepancy and callback stores only log and notify."""

    def __init__(self, store, scheme):
        from .scheme import DEFAULT_SCHEME
        self.store = store
        self._chained_name = scheme.name == DEFAULT_SCHEME
        last = store.last()
        self._append_last = Beacon(last.round, bytes(last.signature), bytes(last.previous_signature or b""))
        self._scheme_last = self._append_last

    def last(self):
        return self.store.last()

    def len(self):
        return self.store.len()

    def get(self, round_):
        return self.store.get(round_)

    def put(self, beacon):
        rnd, sig = int(beacon.round), bytes(beacon.signature)
        prev = bytes(beacon.previous_signature or b"")  # Go: bytes.Equal(nil, []byte{}) is true
        a = self._append_last
        if rnd == a.round:
            if a.signature == sig:
                if a.previous_signature == prev:
                    raise BeaconAlreadyStored("beacon value already stored round %d" % rnd)
                raise PutError("tried to store a duplicate beacon for round %d but the previous signature was "
                               "different" % rnd)
            raise PutError("tried to store a duplicate beacon for round %d but the signature was different" % rnd)
        if rnd != a.round + 1:
            raise PutError("invalid round inserted: last %d, new %d" % (a.round, rnd))
        if self._chained_name:
            if self._scheme_last.signature != prev:
                raise PutError("invalid previous signature for %d" % rnd)
        else:
            prev = b""
        self.store.put(rnd, sig)
        b = Beacon(rnd, sig, prev)
        self._scheme_last = b
        self._append_last = b


_END = object()


def _packet_queue(packets):
    """(queue.Queue of the packets ended by _END, stop function). The caller's own queue is used as is (a gRPC
    receive loop feeding it, the 500-deep channel of net/client_grpc.go:209-212); any other iterable is drained by a
    daemon reader thread, so the verifier can wait for the next packet with a timeout. stop() ends the reader and
    closes the iterator (tryNode's deferred cancel of the peer context, sync_manager.go:335-336): a sync that
    returns early leaves no thread blocked on a full queue and no stream open."""
    if isinstance(packets, queue.Queue):
        return packets, lambda: None
    q = queue.Queue(maxsize=500)
    halt = threading.Event()
    it = iter(packets)

    def reader():
        try:
            for p in it:
                while not halt.is_set():
                    try:
                        q.put(p, timeout=0.05)
                        break
                    except queue.Full:
                        continue
                if halt.is_set():
                    break
        finally:
            for name in ("close", "cancel"):
                fn = getattr(it, name, None) or getattr(packets, name, None)
                if callable(fn):
                    try:
                        fn()
                    except Exception:  # noqa: BLE001 - best effort, the peer is being dropped
                        pass
                    break
            try:
                q.put_nowait(_END)
            except queue.Full:
                pass

    th = threading.Thread(target=reader, daemon=True)
    th.start()

    def stop():
        halt.set()
        th.join(timeout=1.0)

    return q, stop


def sync_from_stream(packets, scheme, pubkey, store, up_to, beacon_id="", window=500, seed=0, idle=0.05,
                     max_delay=1.0, resync=False):
    """tryNode's receive loop (/root/reference/chain/beacon/sync_manager.go:376-445) with verify-ahead windows
    (SURVEY.md §8f row 4). Packets arrive in order; they are verified in batches of up to `window` (the 500-deep
    gRPC buffer, /root/reference/net/client_grpc.go:209), and also as soon as the stream goes quiet for `idle`
    seconds or the oldest waiting packet has waited `max_delay` seconds — a live follow (one beacon per period)
    stores each beacon right after it arrives instead of waiting for 500 more. After verification the packets are
    handled in order exactly as the serial loop handles them: a wrong beacon ID or a failed VerifyBeacon stops the
    peer; then Put — through the chain store's checks (ChainStore: appendStore + schemeStore) unless `resync`
    (from > 0: the insecure store, a plain write, sync_manager.go:410-416). ErrBeaconAlreadyStored ends the peer
    with done = (round == up_to); any other Put error ends it with done = False (:417-425). `store` is a
    ChainStore or a trimmed store (wrapped in a ChainStore here; its Last() must exist, as in tryNode :338-342).
    `packets` is an iterable or a queue.Queue of dicts {round, signature, previous_signature[, beacon_id]}, a queue
    ended by sync.END. Returns (done, stored rounds): done = the packet of round `up_to` was stored."""
    stored = []
    buf = []
    if not resync and not isinstance(store, ChainStore):
        try:
            store = ChainStore(store, scheme)
        except NoBeaconStored:
            return (False, stored)  # tryNode: "unable to fetch from store"

    def put(p):
        if resync:
            store.put(int(p["round"]), bytes(p["signature"]))
            return None
        try:
            store.put(Beacon(int(p["round"]), bytes(p["signature"]), bytes(p.get("previous_signature") or b"")))
        except BeaconAlreadyStored:
            return int(p["round"]) == up_to
        except PutError:
            return False
        return None

    def drain():
        if not buf:
            return None
        n = len(buf)
        rounds = np.array([int(p["round"]) for p in buf], dtype=np.uint64)
        sigs = np.zeros((n, scheme.sig_len), dtype=np.uint8)
        bad_len = np.zeros(n, dtype=bool)
        for k, p in enumerate(buf):
            if len(p["signature"]) == scheme.sig_len:
                sigs[k] = np.frombuffer(bytes(p["signature"]), np.uint8)
            else:
                bad_len[k] = True
        prevs = [bytes(p.get("previous_signature") or b"") for p in buf] if scheme.chained else None
        ok, _ = scheme.verify_beacons(pubkey, rounds, sigs, prevs, seed=seed, want_randomness=False)
        for k, p in enumerate(buf):
            if bad_len[k] or not ok[k]:
                return False
            r = put(p)
            if r is not None:
                return r
            stored.append(int(p["round"]))
            if int(p["round"]) == up_to:
                return True
        buf.clear()
        return None

    q, stop = _packet_queue(packets)
    try:
        first_at = 0.0
        while True:
            timeout = None
            if buf:
                timeout = max(0.0, min(idle, first_at + max_delay - time.monotonic()))
            try:
                p = q.get(timeout=timeout)
            except queue.Empty:  # the stream went quiet (or the oldest packet waited long enough): verify now
                r = drain()
                if r is not None:
                    return (r, stored)
                continue
            if p is _END:
                break
            bid = p.get("beacon_id")
            if bid is not None and bid != beacon_id:
                r = drain()  # packets before the mismatch were received first and are processed first
                return (bool(r), stored)
            if not buf:
                first_at = time.monotonic()
            buf.append(p)
            if len(buf) >= window:
                r = drain()
                if r is not None:
                    return (r, stored)
        r = drain()
        return (bool(r), stored)
    finally:
        stop()


def sync_from_frames(frames, scheme, pubkey, store, up_to, beacon_id="", resync=False, lens=None, window=1 << 20, seed=0):
    """tryNode (/root/reference/chain/beacon/sync_manager.go:376-445) over a buffered run of raw BeaconPacket frames, the
    bytes as they came off the wire: `frames` is a list of byte strings, or one buffer with the frames'
    lengths in `lens` (without lens: varint-delimited). One DeviceArchive check parses and verifies every frame on the
    device, with the store's Last() as the anchor unless `resync`; then the records are handled in order exactly as
    sync_from_stream handles the decoded packets: stop before the first record whose metadata carries another beacon ID,
    stop with False at the first one that does not decode or verify, Put through ChainStore (the plain write when
    resync) with BeaconAlreadyStored / PutError handled as there. Returns (done, stored rounds)."""
    from .store import AR_BEACON_ID, AR_INVALID, PB_BEACON_PACKET, DeviceArchive
    stored = []
    anchor = None
    if not resync:
        if not isinstance(store, ChainStore):
            try:
                store = ChainStore(store, scheme)
            except NoBeaconStored:
                return (False, stored)  # tryNode: "unable to fetch from store"
        last = store.last()
        anchor = (int(last.round), bytes(last.signature))
    with DeviceArchive.from_packets(PB_BEACON_PACKET, frames, lens=lens) as ar:
        status = ar.check(scheme, pubkey, anchor=anchor, window=window, seed=seed, beacon_id=beacon_id)
        n = len(ar)
        stride = max(4, (scheme.sig_len + 3) & ~3)
        for at in range(0, n, int(window)):
            rounds, sigs, sig_lens, prevs, prev_lens, _r, _rl, deferred = ar.beacons_device(at, int(window), sig_stride=stride, prev_stride=stride,
                                                                                           want_rand=False)
            rounds, sigs, prevs = rounds.cpu().numpy().view(np.uint64), sigs.cpu().numpy(), prevs.cpu().numpy()
            prev_lens, deferred = prev_lens.cpu().numpy(), deferred.cpu().numpy()
            for k in range(len(rounds)):
                st = int(status[at + k])
                if st & AR_BEACON_ID:
                    return (False, stored)
                if st & AR_INVALID:  # it does not decode, its signature has another length, or it does not verify
                    return (False, stored)
                if deferred[k]:
                    p = ar.resolve(at + k)
                    rnd, sig, prev = int(p["round"]), p["signature"], p["previous_signature"]
                else:  # a verified row: the signature has the scheme's length
                    rnd, sig = int(rounds[k]), sigs[k, :scheme.sig_len].tobytes()
                    prev = prevs[k, :prev_lens[k]].tobytes() if prev_lens[k] <= stride else ar.resolve(at + k)["previous_signature"]
                if resync:
                    store.put(rnd, sig)
                else:
                    try:
                        store.put(Beacon(rnd, sig, prev))
                    except BeaconAlreadyStored:
                        return (rnd == up_to, stored)
                    except PutError:
                        return (False, stored)
                stored.append(rnd)
                if rnd == up_to:
                    return (True, stored)
    return (False, stored)


def sync_from_sources(sources, scheme, pubkey, store, up_to, beacon_id="", window=1 << 20, seed=0):
    """The sync of a store from many sources at once: what the SyncManager reaches by walking its peers one
    after another (/root/reference/chain/beacon/sync_manager.go:299-323), from every peer's buffered records in one
    pass. `sources` is what store.assemble_archives takes: DeviceArchive handles (protobuf packet runs or RandomData
    archives), DeviceBoltStore handles and column tuples, in any order, overlapping, with holes and bad records. A protobuf
    source whose first record carries another beacon ID is dropped whole, as tryNode drops such a peer (:385-389). One
    assemble runs with the store's Last() as the anchor; the rows up to contiguous_up_to are Put through ChainStore with
    the BeaconAlreadyStored / PutError handling of sync_from_frames. Returns (done, stored rounds, gaps): done = up_to was
    reached, gaps = the ranges of rounds up to up_to that no source supports with a valid record."""
    from .store import AS_GAP, AS_LINK, DeviceArchive, _id_bits, assemble_archives
    stored = []
    if not isinstance(store, ChainStore):
        try:
            store = ChainStore(store, scheme)
        except NoBeaconStored:
            return (False, stored, [])  # tryNode: "unable to fetch from store"
    last = store.last()
    anchor = (int(last.round), bytes(last.signature))
    kept = []
    for s in sources:
        if isinstance(s, DeviceArchive) and s.kind and len(s):
            first = s.resolve(0)
            if first and _id_bits(first, beacon_id):
                continue
        kept.append(s)
    res, _ids = assemble_archives(kept, scheme, pubkey, anchor=anchor, up_to=up_to, window=window, seed=seed)
    flags = res.flags.cpu().numpy()
    bad = np.flatnonzero(flags & (AS_GAP | AS_LINK))
    k = int(bad[0]) if len(bad) else len(flags)
    rounds = res.rounds[:k].cpu().numpy().view(np.uint64)
    sigs, lens = res.sigs[:k].cpu().numpy(), res.lens[:k].cpu().numpy()
    prevs = res.prevs[:k].cpu().numpy() if res.prevs is not None else None
    prev_lens = res.prev_lens[:k].cpu().numpy() if res.prevs is not None else None
    for i in range(k):
        rnd = int(rounds[i])
        prev = prevs[i, :prev_lens[i]].tobytes() if prevs is not None else b""
        try:
            store.put(Beacon(rnd, sigs[i, :lens[i]].tobytes(), prev))
        except BeaconAlreadyStored:
            return (rnd == up_to, stored, res.gaps)
        except PutError:
            return (False, stored, res.gaps)
        stored.append(rnd)
        if rnd == up_to:
            return (True, stored, res.gaps)
    return (False, stored, res.gaps)


END = _END
