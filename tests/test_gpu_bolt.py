"""GPU: trimmed bbolt stores parsed on the device (DeviceBoltStore / dh_store_*).

* DeviceBoltStore.columns equals BoltTrimmedStore.columns byte for byte (rounds, signatures, previous signatures,
  missing rounds) on the reference's trimmed store and on written files of every page size, depth and bucket form,
  with 64 / 65-element leaves, foreign keys, odd value lengths (one on overflow pages) and gaps, over windows that cut
  leaves, lie in gaps, are inverted or lie past the end;
* check_past_beacons(DeviceBoltStore) equals the faulty sets recorded by the CPU test (tests/golden/bolt_cases.json:
  host reader + oracle) for all four schemes; the same through raw ctypes with too little room and a counted callback;
* corrupt files the CPU program classified: BoltError from open, and the library still serves a clean file;
* threads: one store each, and one handle shared; dh_shutdown invalidates a handle and a new one works;
* 131,072 device-signed quicknet rounds (the batched-subgroup threshold) with 0.1% corrupted and 3 records removed:
  the store path's faulty set equals verify_beacons' on the same arrays."""
import ctypes
import os
import random
import sys
import threading

import numpy as np
import pytest

import bolt_cases as bc
from boltwrite2 import write_bolt2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bench"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dh():
    import torch
    import drand_amd
    from drand_amd import _lib
    torch.zeros(1, device="cuda")
    assert _lib.load().dh_init(0) == 0, _lib.last_error()
    return drand_amd


@pytest.fixture(scope="module")
def parity(tmp_path_factory):
    return bc.parity_files(tmp_path_factory.mktemp("parity"))


def _same_columns(a, b, what):
    assert a[0].dtype == b[0].dtype and a[0].tolist() == b[0].tolist(), what
    assert a[1].shape == b[1].shape and a[1].tobytes() == b[1].tobytes(), what
    assert a[2] == b[2], what
    assert list(a[3]) == list(b[3]), what


def test_columns_parity(dh, parity):
    from drand_amd.store import BoltTrimmedStore, DeviceBoltStore
    from drand_amd.sync import NoBeaconStored
    for name, path, _lay in parity:
        for chained, sig_len in ((True, 96), (False, 48)):
            host = BoltTrimmedStore(path, chained)
            with DeviceBoltStore(path, chained) as dev:
                assert dev.len() == host.len(), name
                rounds = host.rounds()
                assert dev.rounds_range() == ((rounds[0], rounds[-1]) if rounds else None), name
                try:
                    want = host.last()
                except NoBeaconStored:
                    with pytest.raises(NoBeaconStored):
                        dev.last()
                else:
                    assert dev.last() == want, name
                for first, last in bc.windows(rounds):
                    _same_columns(dev.columns(first, last, sig_len), host.columns(first, last, sig_len),
                                  (name, chained, first, last))


def test_columns_device_layout(dh, parity):
    """The tensors themselves: key order, true lengths, zero padding, an over-long value left all zero, and the
    previous-signature view (row i - 1) the verifier is handed."""
    from drand_amd.store import BoltFile, DeviceBoltStore
    path = dict((n, p) for n, p, _l in parity)["oddlens"]
    kv = BoltFile(path).bucket(b"beacons")
    with DeviceBoltStore(path, True) as dev:
        for stride in (48, 100, 5000):
            rounds, rows, lens, missing = dev.columns_device(3, 45, stride)
            assert rounds.is_cuda and rows.shape == (43, stride) and missing.numel() == 0
            rows, lens = rows.cpu().numpy(), lens.cpu().numpy()
            for i, r in enumerate(rounds.cpu().tolist()):
                v = kv[bc.key(r)]
                assert r == 3 + i and lens[i] == len(v)
                want = v.ljust(stride, b"\0") if len(v) <= stride else b"\0" * stride
                assert rows[i].tobytes() == want, (stride, r)


@pytest.mark.parametrize("name", bc.SCHEMES)
def test_check_past_equals_recorded_sets(dh, oracle, tmp_path, name):
    from drand_amd.store import DeviceBoltStore
    from drand_amd.sync import check_past_beacons
    gold = bc.load_golden()["replay"]
    s = dh.scheme_from_name(name)
    pk, _sk, _kv = bc.chain(name)
    files = bc.replay_files(tmp_path, name, oracle)
    stores = {}
    try:
        for kind, up_to, window in bc.REPLAY_CALLS:
            if kind not in stores:
                stores[kind] = DeviceBoltStore(files[kind], s.chained)
            seen = []
            got = check_past_beacons(stores[kind], s, pk, up_to, cb=lambda r, u: seen.append((r, u)), window=window, seed=7)
            assert got == gold[bc.call_id(name, kind, up_to, window)], (name, kind, up_to, window)
            # one callback per window, first rounds ascending from 1
            assert [r for r, _u in seen] == list(range(1, seen[-1][0] + 1, window)) if seen else got == []
    finally:
        for st in stores.values():
            st.close()


def test_check_past_raw_abi(dh, oracle, tmp_path):
    """cap too small: every round is still counted, DH_EINVAL with the count needed; the callback once per window."""
    from drand_amd import _lib
    lib = _lib.load()
    name = "pedersen-bls-chained"
    pk, _sk, _kv = bc.chain(name)
    data = np.fromfile(bc.replay_files(tmp_path, name, oracle)["mixed"], np.uint8)
    want = bc.load_golden()["replay"][bc.call_id(name, "mixed", 1000, 8)]
    assert len(want) >= 3
    h = ctypes.c_void_p()
    assert lib.dh_store_open_bolt(data.ctypes.data, data.size, ctypes.byref(h)) == 0, _lib.last_error()
    st = (ctypes.c_uint64 * 6)()
    assert lib.dh_store_stat(h, st) == 0 and list(st)[:4] == [24, 24, 0, 24]
    calls = []
    hook = ctypes.CFUNCTYPE(None, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p)(lambda r, u, a: calls.append((r, u)))
    out = np.zeros(16, np.uint64)
    n = ctypes.c_size_t(0)
    rc = lib.dh_store_check_past(h, 0, pk, len(pk), 1000, 8, 7, out.ctypes.data, 2, ctypes.byref(n), hook, None)
    assert rc == _lib.DH_EINVAL and n.value == len(want) and out[:2].tolist() == want[:2] and out[2] == 0
    assert calls == [(1, 24), (9, 24), (17, 24)]  # rounds 1..23 (len() = 24), up_to clamped to the last round
    rc = lib.dh_store_check_past(h, 0, pk, len(pk), 1000, 8, 7, out.ctypes.data, 16, ctypes.byref(n), None, None)
    assert rc == 0 and out[:n.value].tolist() == want
    assert lib.dh_store_check_past(h, 0, pk, len(pk), 1000, 0, 7, out.ctypes.data, 16, ctypes.byref(n), None, None) == _lib.DH_EINVAL
    lib.dh_store_close(h)
    # a chained store whose last record has no predecessor: Last() fails (trimmed.go:183-190), as does an empty store
    for kv in ({bc.key(3): b"x" * 96, bc.key(5): b"y" * 96}, {}):
        path = str(tmp_path / "nolast.db")
        write_bolt2(path, list(kv.items()))
        data = np.fromfile(path, np.uint8)
        assert lib.dh_store_open_bolt(data.ctypes.data, data.size, ctypes.byref(h)) == 0, _lib.last_error()
        assert lib.dh_store_check_past(h, 0, pk, len(pk), 10, 8, 7, out.ctypes.data, 16, ctypes.byref(n), None,
                                       None) == _lib.DH_ENOBEACON
        lib.dh_store_close(h)


def test_corrupt_files_are_refused(dh, tmp_path, parity):
    from drand_amd.store import BoltError, BoltTrimmedStore, DeviceBoltStore, StoreTooLarge
    files, _base, _at = bc.corrupt_files(tmp_path)
    verdicts = bc.load_golden()["corrupt"]  # classified by the CPU program under the sanitizers
    clean = dict((n, p) for n, p, _l in parity)["p512"]
    for name, path in files:
        if verdicts[name] == "ERR":
            with pytest.raises(BoltError):
                DeviceBoltStore(path, False)
        else:
            with DeviceBoltStore(path, False) as dev:
                assert dev.len() == BoltTrimmedStore(path, False).len()
        with DeviceBoltStore(clean, False) as dev:  # the library still serves a clean file
            _same_columns(dev.columns(0, 299, 48), BoltTrimmedStore(clean, False).columns(0, 299, 48), name)
    # a file above DRANDHIP_STORE_MAX_BYTES: DH_ENOMEM, the caller keeps the host reader
    os.environ["DRANDHIP_STORE_MAX_BYTES"] = "4096"
    try:
        with pytest.raises(StoreTooLarge):
            DeviceBoltStore(clean, False)
    finally:
        del os.environ["DRANDHIP_STORE_MAX_BYTES"]


def test_threads(dh, oracle, tmp_path):
    from drand_amd.store import DeviceBoltStore
    from drand_amd.sync import check_past_beacons
    gold = bc.load_golden()["replay"]
    jobs = []
    for name in ("pedersen-bls-chained", "bls-unchained-g1-rfc9380"):
        jobs.append((name, bc.replay_files(tmp_path, name, oracle)["mixed"], gold[bc.call_id(name, "mixed", 1000, 8)]))
    errs = []

    def replay(store, name, want):
        try:
            s = dh.scheme_from_name(name)
            for _ in range(3):
                got = check_past_beacons(store, s, bc.chain(name)[0], 1000, window=8, seed=3)
                assert got == want, (name, got)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    # each thread its own store
    stores = [DeviceBoltStore(p, n == "pedersen-bls-chained") for n, p, _w in jobs]
    ths = [threading.Thread(target=replay, args=(st, n, w)) for st, (n, _p, w) in zip(stores, jobs)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not errs, errs
    # one handle shared by two threads: calls are serialised inside the handle
    ths = [threading.Thread(target=replay, args=(stores[0], jobs[0][0], jobs[0][2])) for _ in range(2)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not errs, errs
    [st.close() for st in stores]


def test_quicknet_131072_through_the_store(dh, tmp_path):
    """Crosses DRANDHIP_SUB_BATCH_MIN (131,072 rounds: the batched subgroup test) with store-produced strides."""
    import chainsynth
    import g1_synth
    from drand_amd.store import DeviceBoltStore
    from drand_amd.sync import check_past_beacons
    import hashlib
    name = "bls-unchained-g1-rfc9380"
    s = dh.scheme_from_name(name)
    sk = hashlib.sha256(b"store-131072").digest()
    sk = (int.from_bytes(sk, "big") % 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001).to_bytes(32, "big")
    pk = s.public_key(sk)
    # 131,078 signed rounds, 3 records removed, plus the genesis record: len() = 131,076, so the walk examines rounds
    # 1 .. 131,075 (CheckPastBeacons' i < len), of which 131,072 are stored: one window at the threshold
    n = 131072 + 6
    rounds = np.arange(1, n + 1, dtype=np.uint64)
    sigs = s.sign_beacons(sk, rounds)
    bad = chainsynth.corrupted_rounds(n, n // 1000)
    g1_synth.corrupt(sigs, bad, random.Random(41))
    removed = [4097, 70001, 131000]  # rounds
    keep = np.ones(n, bool)
    keep[np.array(removed) - 1] = False
    v, _ = s.verify_beacons(pk, rounds[keep], sigs[keep], seed=11, want_randomness=False)
    hi = n - 3
    want = sorted(r for r in set(rounds[keep][~v].tolist()) | set(removed) if r <= hi)
    assert len(want) > 100
    path = str(tmp_path / "quicknet.db")
    all_rounds = np.concatenate([np.zeros(1, np.uint64), rounds[keep]])
    all_sigs = np.concatenate([np.zeros((1, 48), np.uint8), sigs[keep]])
    write_bolt2(path, rounds=all_rounds, sigs=all_sigs)
    with DeviceBoltStore(path, False) as dev:
        assert dev.len() == hi + 1 and dev.rounds_range() == (0, n)
        seen = []
        got = check_past_beacons(dev, s, pk, 1 << 40, cb=lambda r, u: seen.append((r, u)), seed=12)
    assert seen == [(1, n)]  # one window: 131,072 rows in one verification batch
    assert got == want


def test_shutdown_invalidates_handles(dh, parity):
    """dh_shutdown releases a store's device memory: its handle then only accepts close, and a new one works."""
    from drand_amd import _lib
    from drand_amd.store import BoltTrimmedStore, DeviceBoltStore
    lib = _lib.load()
    path = dict((n, p) for n, p, _l in parity)["p1024"]
    dev = DeviceBoltStore(path, False)
    want = BoltTrimmedStore(path, False).columns(0, 299, 48)
    _same_columns(dev.columns(0, 299, 48), want, "before")
    lib.dh_shutdown()
    try:
        with pytest.raises(ValueError, match="dh_shutdown"):
            dev.columns(0, 299, 48)
        assert dev.len() == 300  # fixed at open
        dev.close()
    finally:
        assert lib.dh_init(0) == 0, _lib.last_error()
    with DeviceBoltStore(path, False) as again:
        _same_columns(again.columns(0, 299, 48), want, "after")
