"""GPU: legacy untrimmed (hexjson) bbolt stores parsed on the device (DeviceBoltStore(fmt=...) /
dh_store_open_bolt_format, dh_store_beacons_device, dh_store_deferred).

* the reference's untrimmed fixture opened as UNTRIMMED and AUTO (and its trimmed one as AUTO): the decoded columns of
  rounds 0..26 equal BoltUntrimmedStore field by field; dh_store_format_stat;
* column parity on written stores: 96-byte records at page sizes 256 (overflow pages: read in place), 512, 4096 and
  16384, 48-byte records at 16384 (two chunks a leaf through LDS), an inline bucket, 8,192 leaves (the hierarchical
  scan), gaps, every deferred class, windows that cut leaves, d_prevs = NULL, a stride shorter than a decoded value,
  too little room;
* check_past against the lists recorded by the CPU test (tests/golden/bolt_json_cases.json: host reader + oracle) for
  all four schemes; the raw ABI returns DH_DEFERRED and dh_store_deferred lists the two deferred keys;
* refusals, and threads on separate and shared handles."""
import ctypes
import os
import threading

import numpy as np
import pytest

import bolt_cases as bc
import bolt_json_cases as jc
from boltwrite2 import write_bolt2

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
    return jc.parity_files(tmp_path_factory.mktemp("json_parity"))


def expected_columns(path, deferred, first, last, sig_stride, prev_stride):
    """The columns dh_store_beacons_device must write, from BoltFile and beacon_from_hexjson (BoltUntrimmedStore.get)."""
    from drand_amd.store import BoltFile, beacon_from_hexjson
    kv = BoltFile(path).bucket(b"beacons")
    have = sorted(int.from_bytes(k, "big") for k in kv if len(k) == 8)
    rows = [r for r in have if first <= r <= last]
    n = len(rows)
    sigs, prevs = np.zeros((n, sig_stride), np.uint8), np.zeros((n, prev_stride), np.uint8)
    sig_lens, prev_lens, dfr = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    for i, r in enumerate(rows):
        if r in deferred:
            dfr[i] = 1
            continue
        b = beacon_from_hexjson(kv[bc.key(r)])
        assert b.round == r
        sig_lens[i], prev_lens[i] = len(b.signature), len(b.previous_signature)
        if len(b.signature) <= sig_stride:  # a longer value leaves the row zero, never a prefix
            sigs[i, :len(b.signature)] = np.frombuffer(b.signature, np.uint8)
        if len(b.previous_signature) <= prev_stride:
            prevs[i, :len(b.previous_signature)] = np.frombuffer(b.previous_signature, np.uint8)
    stored = set(have)
    missing = [r for r in range(first, last + 1) if r not in stored] if first <= last else []
    return rows, sigs, sig_lens, prevs, prev_lens, dfr, missing


def same_columns(dev, path, deferred, first, last, sig_stride=None, prev_stride=None, want_prev=True, what=None):
    got = dev.beacons_device(first, last, sig_stride, prev_stride, want_prev)
    rounds, sigs, sig_lens, prevs, prev_lens, dfr, missing = got
    assert rounds.is_cuda and sigs.is_cuda
    want = expected_columns(path, set(deferred), first, last, sigs.shape[1], prevs.shape[1] if want_prev else 4)
    assert rounds.cpu().tolist() == want[0], what
    assert sigs.cpu().numpy().tobytes() == want[1].tobytes(), what
    assert sig_lens.cpu().tolist() == want[2].tolist(), what
    if want_prev:
        assert prevs.cpu().numpy().tobytes() == want[3].tobytes(), what
        assert prev_lens.cpu().tolist() == want[4].tolist(), what
    else:
        assert prevs is None and prev_lens is None
    assert dfr.cpu().tolist() == want[5].tolist(), what
    assert missing.cpu().tolist() == want[6], what
    return want


def test_reference_fixture(dh):
    from drand_amd.store import BoltUntrimmedStore, DeviceBoltStore
    host = BoltUntrimmedStore(jc.REF_UNTRIMMED, True)
    for fmt in ("untrimmed", "auto"):
        with DeviceBoltStore(jc.REF_UNTRIMMED, True, fmt=fmt) as dev:
            assert dev.untrimmed and dev.format_stat() == {"format": "untrimmed", "deferred": 0, "longest_signature": 96,
                                                           "longest_previous": 96}
            assert dev.len() == host.len() == 27 and dev.rounds_range() == (0, 26) and dev.deferred() == []
            want = same_columns(dev, jc.REF_UNTRIMMED, [], 0, 26, what=fmt)
            assert want[2][0] == 32 and want[4][0] == 0 and want[4][1] == 32  # the genesis record, its null previous
            for r in range(27):
                assert dev.get(r) == host.get(r)
            assert dev.last() == host.last()
    with DeviceBoltStore(jc.REF_TRIMMED, True, fmt="auto") as dev:
        assert dev.untrimmed is False and dev.format_stat()["format"] == "trimmed" and dev.len() == 46
        with pytest.raises(ValueError, match="untrimmed"):
            dev.beacons_device(0, 5)
        assert dev.deferred() == []


def test_column_parity_on_written_stores(dh, parity):
    from drand_amd.store import BoltUntrimmedStore, DeviceBoltStore
    for name, path, deferred in parity:
        host = BoltUntrimmedStore(path, True)
        rounds = host.rounds()
        with DeviceBoltStore(path, True, fmt="untrimmed") as dev:
            assert dev.len() == host.len() and dev.rounds_range() == (rounds[0], rounds[-1]), name
            assert dev.deferred() == deferred and dev.format_stat()["deferred"] == len(deferred), name
            if name == "many_leaves":  # 8,192 leaves: the whole store, and a window that cuts into it
                wins = [(0, 9000), (4090, 4200)]
            else:
                wins = jc.windows(rounds)
            for first, last in wins:
                same_columns(dev, path, deferred, first, last, what=(name, first, last))
            # no previous column; strides shorter than one decoded value: an all-zero row with the true length
            lo, hi = rounds[0] + 1, min(rounds[-1], rounds[0] + 70)
            same_columns(dev, path, deferred, lo, hi, want_prev=False, what=(name, "no prevs"))
            want = same_columns(dev, path, deferred, lo, hi, sig_stride=44, prev_stride=32, what=(name, "short strides"))
            assert not want[1][want[2] > 44].any() and (want[2] > 44).any()
            # the deferred keys of a sub-range
            assert dev.deferred(lo, hi) == [r for r in deferred if lo <= r <= hi], name


def test_mixed_store_matches_the_host_reader(dh, parity):
    """get / last / columns on a store with deferred records: what BoltUntrimmedStore returns, errors included."""
    from drand_amd.store import DECODE_ERRORS, BoltUntrimmedStore, DeviceBoltStore
    from drand_amd.sync import NoBeaconStored
    _name, path, deferred = [p for p in parity if p[0] == "mixed"][0]
    host = BoltUntrimmedStore(path, True)
    with DeviceBoltStore(path, True, fmt="untrimmed") as dev:
        assert dev.format_stat() == {"format": "untrimmed", "deferred": len(deferred), "longest_signature": 200,
                                     "longest_previous": 130}
        for r in list(range(0, 100)) + [500]:
            try:
                want = host.get(r)
            except (NoBeaconStored,) + DECODE_ERRORS as e:
                with pytest.raises(type(e)):
                    dev.get(r)
            else:
                assert dev.get(r) == want, r
        assert dev.last() == host.last()
        rounds, sigs, prevs, missing = dev.columns(0, 110, 96)
        want_r, want_s, want_p, want_m = [], [], [], list(range(100, 111))
        for r in range(100):
            try:
                b = host.get(r)
            except DECODE_ERRORS:
                want_m.append(r)
                continue
            want_r.append(b.round)
            want_s.append(b.signature if len(b.signature) == 96 else b"\0" * 96)
            want_p.append(b.previous_signature)
        assert rounds.tolist() == want_r and [s.tobytes() for s in sigs] == want_s and prevs == want_p
        assert missing == sorted(want_m)
        # dh_store_columns_device keeps returning the raw stored values
        raw_rounds, rows, lens, _ = dev._columns_host(0, 10)
        kv = host._kv
        assert [rows[i, :lens[i]].tobytes() for i in range(len(raw_rounds))] == [kv[bc.key(int(r))] for r in raw_rounds]


def test_capacity_too_small(dh, parity):
    import torch
    from drand_amd import _lib
    lib = _lib.load()
    _name, path, _d = [p for p in parity if p[0] == "gaps"][0]
    data = np.fromfile(path, np.uint8)
    h = ctypes.c_void_p()
    assert lib.dh_store_open_bolt_format(data.ctypes.data, data.size, _lib.DH_STORE_UNTRIMMED, ctypes.byref(h)) == 0
    try:
        n, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
        cap = 8
        rounds = torch.full((cap,), -1, dtype=torch.int64, device="cuda")
        sigs = torch.full((cap, 96), 0xAA, dtype=torch.uint8, device="cuda")
        lens = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
        dfr = torch.full((cap,), 0xAA, dtype=torch.uint8, device="cuda")
        miss = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def call(cap_rows, cap_missing, sig_stride=96, prev_stride=96, prevs=None, prev_lens=None):
            return lib.dh_store_beacons_device(h, 20, 40, sig_stride, prev_stride, rounds.data_ptr(), sigs.data_ptr(),
                                               lens.data_ptr(), prevs, prev_lens, dfr.data_ptr(), cap_rows, ctypes.byref(n),
                                               miss.data_ptr(), cap_missing, ctypes.byref(m), None)

        # rounds 20..40 with 30, 31, 32 removed: 18 rows, 3 missing
        assert call(cap, 2) == _lib.DH_EINVAL and (n.value, m.value) == (18, 3)
        assert call(18, 2) == _lib.DH_EINVAL and (n.value, m.value) == (18, 3)
        torch.cuda.synchronize()
        assert (rounds == -1).all() and (sigs == 0xAA).all() and (lens == -1).all() and (dfr == 0xAA).all() and (miss == -1).all()
        # strides: multiples of 4, at most 1 MiB; d_prevs and d_prev_lens together
        assert call(cap, 2, sig_stride=94) == _lib.DH_EINVAL and "stride" in _lib.last_error()
        assert call(cap, 2, sig_stride=(1 << 20) + 4) == _lib.DH_EINVAL
        assert call(cap, 2, prev_stride=6, prevs=sigs.data_ptr(), prev_lens=lens.data_ptr()) == _lib.DH_EINVAL
        assert call(cap, 2, prevs=sigs.data_ptr()) == _lib.DH_EINVAL and "together" in _lib.last_error()
    finally:
        lib.dh_store_close(h)


@pytest.mark.parametrize("name", jc.SCHEMES)
def test_check_past_equals_recorded_lists(dh, oracle, tmp_path, name):
    from drand_amd import _lib
    from drand_amd.store import DeviceBoltStore
    from drand_amd.sync import check_past_beacons
    lib = _lib.load()
    gold = jc.load_golden()["replay"]
    s = dh.scheme_from_name(name)
    pk, path, deferred = jc.replay_file(tmp_path, name, oracle)
    assert pk == s.public_key(hashlib_sk(name))
    with DeviceBoltStore(path, s.chained, fmt="auto") as dev:
        assert dev.untrimmed and dev.deferred() == deferred == [jc.UNDECODABLE, jc.ROUND_NE_KEY]
        for up_to, window in jc.REPLAY_CALLS:
            seen = []
            got = check_past_beacons(dev, s, pk, up_to, cb=lambda r, u: seen.append((r, u)), window=window, seed=7)
            assert got == gold[jc.call_id(name, up_to, window)], (name, up_to, window)
            assert [r for r, _u in seen] == list(range(1, seen[-1][0] + 1, window))  # one callback per window
        # the raw ABI: the device's own list leaves the deferred records out and says so
        out = np.zeros(16, np.uint64)
        n = ctypes.c_size_t(0)
        rc = lib.dh_store_check_past(dev._h, s.id, pk, len(pk), 1000, 64, 7, out.ctypes.data, 16, ctypes.byref(n), None, None)
        assert rc == _lib.DH_DEFERRED == 1, _lib.last_error()
        want = [r for r in gold[jc.call_id(name, 1000, 64)] if r not in (jc.UNDECODABLE, 7)]
        assert out[:n.value].tolist() == want
        rc = lib.dh_store_check_past(dev._h, s.id, pk, len(pk), 100, 64, 7, out.ctypes.data, 16, ctypes.byref(n), None, None)
        assert rc == 0 and out[:n.value].tolist() == [r for r in want if r <= 100]  # no deferred record below 100
        rc = lib.dh_store_check_past(dev._h, s.id, pk, len(pk), 1000, 64, 7, out.ctypes.data, 2, ctypes.byref(n), None, None)
        assert rc == _lib.DH_EINVAL and n.value == len(want) and out[:2].tolist() == want[:2]
        keys = np.zeros(4, np.uint64)
        assert lib.dh_store_deferred(dev._h, 0, 1 << 40, keys.ctypes.data, 4, ctypes.byref(n)) == 0
        assert keys[:n.value].tolist() == deferred
        assert lib.dh_store_deferred(dev._h, 0, 1 << 40, keys.ctypes.data, 1, ctypes.byref(n)) == _lib.DH_EINVAL and n.value == 2
        assert lib.dh_store_deferred(dev._h, 121, 139, keys.ctypes.data, 4, ctypes.byref(n)) == 0 and n.value == 0


def hashlib_sk(name):
    import hashlib
    sk = hashlib.sha256(b"bolt json " + name.encode()).digest()
    return (int.from_bytes(sk, "big") % 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001).to_bytes(32, "big")


def test_refusals(dh, tmp_path, parity):
    from drand_amd import _lib
    from drand_amd.store import BoltError, BoltUntrimmedStore, DeviceBoltStore
    from drand_amd.sync import NoBeaconStored
    lib = _lib.load()
    s = dh.scheme_from_name("pedersen-bls-chained")
    pk = s.public_key(hashlib_sk(s.name))
    # the structurally corrupt files of the trimmed cases, opened as untrimmed
    files, _base, _at = bc.corrupt_files(tmp_path)
    verdicts = bc.load_golden()["corrupt"]
    assert "ERR" in verdicts.values()
    for name, path in files:
        if verdicts[name] == "ERR":
            with pytest.raises(BoltError):
                DeviceBoltStore(path, True, fmt="untrimmed")
        else:
            with DeviceBoltStore(path, True, fmt="untrimmed") as dev:  # raw signatures: every record deferred
                assert dev.len() == BoltUntrimmedStore(path, True).len() == dev.format_stat()["deferred"]
    # dh_store_beacons_device on a trimmed handle
    _n, clean, _d = [p for p in parity if p[0] == "j96_p4096"][0]
    with DeviceBoltStore(clean, True) as dev:
        with pytest.raises(ValueError, match="untrimmed"):
            dev.beacons_device(0, 10)
    with pytest.raises(ValueError, match="fmt"):
        DeviceBoltStore(clean, True, fmt="json")
    h = ctypes.c_void_p()
    data = np.fromfile(clean, np.uint8)
    assert lib.dh_store_open_bolt_format(data.ctypes.data, data.size, 3, ctypes.byref(h)) == _lib.DH_EINVAL and not h.value
    # AUTO on a first value that starts with '{' but is not canonical
    kv = jc.synth(10, 96, True, "auto")
    kv[bc.key(0)] = kv[bc.key(0)].replace(b":", b": ", 1)
    path = str(tmp_path / "brace.db")
    write_bolt2(path, list(kv.items()))
    with pytest.raises(ValueError, match="name the format"):
        DeviceBoltStore(path, True, fmt="auto")
    with DeviceBoltStore(path, True, fmt="untrimmed") as dev:
        assert dev.deferred() == [0]
    # a deferred last record: Last().Round needs the host decoder
    kv = jc.synth(10, 96, True, "last")
    kv[bc.key(9)] = kv[bc.key(9)] + b" "
    path = str(tmp_path / "deferred_last.db")
    write_bolt2(path, list(kv.items()))
    with DeviceBoltStore(path, True, fmt="auto") as dev:
        with pytest.raises(ValueError, match="last record"):
            dev.check_past(s, pk, 100)
    # an empty bucket: AUTO takes it as trimmed; named untrimmed it has no beacon either
    path = str(tmp_path / "empty.db")
    write_bolt2(path, [])
    for fmt in ("auto", "untrimmed"):
        with DeviceBoltStore(path, True, fmt=fmt) as dev:
            assert dev.untrimmed == (fmt == "untrimmed") and dev.len() == 0
            with pytest.raises(NoBeaconStored):
                dev.check_past(s, pk, 100)
            with pytest.raises(NoBeaconStored):
                dev.last()


def test_threads(dh, oracle, tmp_path):
    from drand_amd.store import DeviceBoltStore
    from drand_amd.sync import check_past_beacons
    gold = jc.load_golden()["replay"]
    jobs = []
    for name in ("pedersen-bls-chained", "bls-unchained-g1-rfc9380"):
        pk, path, _d = jc.replay_file(tmp_path, name, oracle)
        jobs.append((name, path, pk, gold[jc.call_id(name, 1000, 64)]))
    errs = []

    def replay(store, name, pk, want):
        try:
            s = dh.scheme_from_name(name)
            for _ in range(2):
                got = check_past_beacons(store, s, pk, 1000, window=64, seed=3)
                assert got == want, (name, got)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    stores = [DeviceBoltStore(p, n == "pedersen-bls-chained", fmt="untrimmed") for n, p, _k, _w in jobs]
    ths = [threading.Thread(target=replay, args=(st, n, k, w)) for st, (n, _p, k, w) in zip(stores, jobs)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not errs, errs
    # one handle shared by two threads: calls are serialised inside the handle
    ths = [threading.Thread(target=replay, args=(stores[0], jobs[0][0], jobs[0][2], jobs[0][3])) for _ in range(2)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not errs, errs
    [st.close() for st in stores]
