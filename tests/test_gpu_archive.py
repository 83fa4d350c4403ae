"""GPU: client.RandomData JSON-lines archives parsed on the device (DeviceArchive / dh_archive_*).

* framing and column parity with store.random_data_from_line, field by field: 1, 63, 64, 65 and 257 records of G1 and
  chained G2 shape, no trailing newline, the empty buffer, only newlines, runs of blank lines, records ending at,
  starting at and straddling a tile edge (the tile size dh_archive_stat reports), more tiles than one scan workgroup
  covers, lines of 4096 and 4097 bytes, every deferred class, windows that cut chunks, d_prevs = NULL and d_rands =
  NULL, strides shorter than a value, '['-first buffers refused;
* check for all four schemes against the statuses recorded by the CPU test (tests/golden/archive_cases.json: host
  check + oracle), with and without an anchor, window 64 and 2^20; the raw ABI returns DH_DEFERRED and
  dh_archive_deferred lists exactly the deferred indices;
* archive_to_trimmed_store equals write_trimmed_bolt byte for byte and raises on the faulty archive;
* threads on separate and shared handles; use after dh_shutdown."""
import ctypes
import os
import threading

import numpy as np
import pytest

import archive_cases as ac

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
def gold():
    return ac.load_golden()


def g1_line(i):
    from drand_amd.store import random_data_line
    s = ac.rand_bytes("g1 sig %d" % i, 48)
    return random_data_line({"round": 1 + i, "randomness": ac.rand_bytes("g1 rand %d" % i, 32), "signature": s})


def g2_line(i):
    from drand_amd.store import random_data_line
    return random_data_line({"round": 2634945 + i, "randomness": ac.rand_bytes("g2 rand %d" % i, 32),
                             "signature": ac.rand_bytes("g2 sig %d" % i, 96), "previous_signature": ac.rand_bytes("g2 sig %d" % (i - 1), 96)})


def deferred_lines():
    """One line per deferred class (tests/test_archive_host.py runs the same classes through the sanitizer build)."""
    g1 = g1_line(7)
    sig = ac.rand_bytes("g1 sig 7", 48).hex().encode()
    return [g1.replace(sig, sig.upper()), g1.replace(sig, sig[:-1]), b'{"round":5,"signature":""}', b'{"round":0,"signature":"00"}',
            g1 + b"\r", b" " + g1, g1.replace(b":", b": ", 1), b"   ", b'{"signature":"00","round":5}', b'{"round":5,"round":6}',
            g1[:-1] + b',"metadata":{"beaconID":"default"}}', b'{"round":123456789012345678901}', b'{"round":18446744073709551616}',
            g1[:-1], g1 + b"x", g1.replace(sig, b"zz" + sig[2:]), b"nope", ac.line_of_length(4097), ac.line_of_length(6000)]


def expected(data, first, n, sig_stride, prev_stride):
    """(lines, columns) dh_archive_beacons_device must write for records first .. first + n - 1, from the host framing
    and random_data_from_line; a record is deferred here exactly when its line is not what random_data_line writes."""
    from drand_amd.store import DECODE_ERRORS, archive_lines, random_data_from_line, random_data_line
    lines = archive_lines(data)[first:first + n]
    m = len(lines)
    rounds, dfr = np.zeros(m, np.uint64), np.zeros(m, np.uint8)
    cols = {k: np.zeros((m, s), np.uint8) for k, s in (("signature", sig_stride), ("previous_signature", prev_stride), ("randomness", 32))}
    lens = {k: np.zeros(m, np.int32) for k in cols}
    for i, l in enumerate(lines):
        try:
            r = random_data_from_line(l)
        except DECODE_ERRORS:
            r = None
        if r is None or random_data_line(r) != l or len(l) > 4096:
            dfr[i] = 1
            continue
        rounds[i] = r["round"]
        for k in cols:
            lens[k][i] = len(r[k])
            if len(r[k]) <= cols[k].shape[1]:  # a longer value leaves the row zero, never a prefix
                cols[k][i, :len(r[k])] = np.frombuffer(r[k], np.uint8)
    return lines, rounds, cols, lens, dfr


def check_parity(dh, data, windows=None, sig_stride=None, prev_stride=None, want_prev=True, want_rand=True):
    from drand_amd.store import DeviceArchive, archive_lines
    lines = archive_lines(data)
    with DeviceArchive(data) as ar:
        st = ar.stat()
        assert len(ar) == len(lines) == st["records"]
        off, ln = ar.lines()
        at, want_off = 0, []
        for run in data.split(b"\n"):
            if run:
                want_off.append(at)
            at += len(run) + 1
        assert list(off) == want_off and list(ln) == [min(len(l), 4097) for l in lines]
        for first, n in windows or [(0, len(lines))]:
            got = ar.beacons_device(first, n, sig_stride=sig_stride, prev_stride=prev_stride, want_prev=want_prev, want_rand=want_rand)
            rounds, sigs, sig_lens, prevs, prev_lens, rands, rand_lens, dfr = [None if t is None else t.cpu().numpy() for t in got]
            _l, w_rounds, cols, lens, w_dfr = expected(data, first, n, sigs.shape[1], prevs.shape[1] if want_prev else 4)
            assert list(dfr) == list(w_dfr), (first, n)
            assert list(rounds.view(np.uint64)) == list(w_rounds), (first, n)
            assert np.array_equal(sigs, cols["signature"]) and list(sig_lens) == list(lens["signature"]), (first, n)
            if want_prev:
                assert np.array_equal(prevs, cols["previous_signature"]) and list(prev_lens) == list(lens["previous_signature"])
            else:
                assert prevs is None and prev_lens is None
            if want_rand:
                assert np.array_equal(rands, cols["randomness"]) and list(rand_lens) == list(lens["randomness"])
            else:
                assert rands is None and rand_lens is None
            assert ar.deferred(first, n) == [first + int(i) for i in np.flatnonzero(w_dfr)]
        if not windows:
            assert st["deferred"] == int(w_dfr.sum())
            assert st["longest_line"] == max([0] + [min(len(l), 4097) for l in lines])
            for k, name in (("signature", "longest_signature"), ("previous_signature", "longest_previous"), ("randomness", "longest_randomness")):
                assert st[name] == int(lens[k].max()) if len(lines) else st[name] == 0
        return st


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("shape", ["g1", "g2"])
def test_column_parity_wave_and_workgroup_edges(dh, n, shape):
    line = g1_line if shape == "g1" else g2_line
    data = b"\n".join(line(i) for i in range(n))
    check_parity(dh, data + b"\n")
    check_parity(dh, data)  # no trailing newline


def test_empty_and_blank_buffers(dh):
    for data in (b"", b"\n", b"\n" * 5000):
        assert check_parity(dh, data)["records"] == 0
    data = b"\n\n" + g1_line(0) + b"\n\n\n\n" + g1_line(1) + b"\n" + b"\n" * 300 + g2_line(2) + b"\n\n"
    assert check_parity(dh, data)["records"] == 3
    assert check_parity(dh, b"\n" * 9000 + g1_line(3))["records"] == 1


def test_tile_edges(dh):
    from drand_amd.store import DeviceArchive
    with DeviceArchive(b"{}\n") as ar:
        tile = ar.stat()["tile_bytes"]
    assert tile >= 512
    fill = [g1_line(i) for i in range(64)]

    def upto(size):  # whole lines, then one padded with blank runs so that the buffer is exactly `size` bytes
        out, i = b"", 0
        while len(out) + len(fill[i % 64]) + 1 <= size - 300:
            out += fill[i % 64] + b"\n"
            i += 1
        return out + b"\n" * (size - len(out))

    a = g2_line(1)
    # a record ending exactly at a tile's last byte, the next starting at the next tile's first byte
    data = upto(tile - len(a) - 1) + a + b"\n" + g1_line(5) + b"\n"
    assert data[tile - 1:tile] == b"\n" and data[tile - 2:tile - 1] == b"}" and data[tile:tile + 1] == b"{"
    check_parity(dh, data)
    data = upto(tile - len(a)) + a + b"\n" + g1_line(5) + b"\n"  # the record's last byte is the tile's last byte
    assert data[tile - 1:tile] == b"}" and data[tile:tile + 1] == b"\n"
    check_parity(dh, data)
    for cut in (1, 17, len(a) - 1):  # straddling two tiles
        data = upto(tile - cut) + a + b"\n" + g1_line(5)
        assert data[tile - cut:tile - cut + 1] == b"{"
        check_parity(dh, data)
    # a line that spans more than two tiles, deferred by its length, between two records
    check_parity(dh, g1_line(1) + b"\n" + b"x" * (2 * tile + 50) + b"\n" + g1_line(2) + b"\n")


def test_hierarchical_scan(dh):
    """More tiles than one scan workgroup covers (4096): short records spread over blank runs keep the record count
    small while the image passes 4096 tiles."""
    from drand_amd.store import DeviceArchive
    with DeviceArchive(b"{}\n") as ar:
        tile = ar.stat()["tile_bytes"]
    ntiles = 4096 + 3
    buf = np.full(ntiles * tile, 10, np.uint8)
    want = []
    for t in list(range(0, ntiles, 97)) + [4095, 4096, ntiles - 1]:
        rec = b'{"round":%d}' % (1000000000 + t)  # 20 bytes
        at = t * tile + (t % 50)
        buf[at:at + len(rec)] = np.frombuffer(rec, np.uint8)
        want.append((at, 1000000000 + t))
    want = sorted(set(want))
    with DeviceArchive(buf.tobytes()) as ar:
        assert len(ar) == len(want)
        off, ln = ar.lines()
        assert list(off) == [a for a, _ in want] and set(ln) == {20}
        rounds = ar.beacons_device(want_prev=False, want_rand=False)[0].cpu().numpy()
        assert list(rounds) == [r for _, r in want]


def test_long_lines_and_deferred_classes(dh):
    ok, long = ac.line_of_length(4096), ac.line_of_length(4097)
    st = check_parity(dh, g1_line(0) + b"\n" + ok + b"\n" + long + b"\n" + g1_line(1) + b"\n")
    assert st["deferred"] == 1 and st["longest_line"] == 4097 and st["longest_signature"] == (4096 - 26) // 2
    lines = []
    for i, d in enumerate(deferred_lines()):
        lines += [g1_line(i), d]
    st = check_parity(dh, b"\n".join(lines))
    assert st["deferred"] == len(deferred_lines())
    check_parity(dh, b"\n".join(deferred_lines()) + b"\n")  # a chunk without one canonical record


def test_windows_null_columns_and_short_strides(dh):
    lines = [g2_line(i) if i % 3 else g1_line(i) for i in range(200)]
    lines[70], lines[130] = b'{ "round":1}', b"{}"
    data = b"\n".join(lines) + b"\n"
    windows = [(0, 200), (1, 63), (1, 64), (63, 2), (64, 64), (65, 135), (199, 1), (199, 50), (200, 5), (500, 1), (10, 0)]
    check_parity(dh, data, windows)
    check_parity(dh, data, windows[:4], want_prev=False)
    check_parity(dh, data, windows[:4], want_rand=False)
    check_parity(dh, data, windows[:4], want_prev=False, want_rand=False)
    # strides shorter than a value: the row is zero, the length is kept
    check_parity(dh, data, windows[:3], sig_stride=48, prev_stride=92)
    check_parity(dh, data, windows[:3], sig_stride=4, prev_stride=4)


def test_refusals(dh):
    from drand_amd import _lib
    from drand_amd.store import DeviceArchive, StoreTooLarge
    lib = _lib.load()
    for data in (b"[", b"\n\n[{}]\n", b'[{"round":1}]\n'):
        with pytest.raises(ValueError, match="JSON-array"):
            DeviceArchive(data)
    h = ctypes.c_void_p()
    assert lib.dh_archive_open_ndjson(None, 5, ctypes.byref(h)) == _lib.DH_EINVAL
    assert lib.dh_archive_open_ndjson(b"{}", 2, None) == _lib.DH_EINVAL
    os.environ["DRANDHIP_STORE_MAX_BYTES"] = "100"
    try:
        with pytest.raises(StoreTooLarge):
            DeviceArchive(b"\n".join(g1_line(i) for i in range(3)))
    finally:
        del os.environ["DRANDHIP_STORE_MAX_BYTES"]
    with DeviceArchive(g1_line(0) + b"\n" + g2_line(1)) as ar:
        import torch
        n = ctypes.c_size_t(0)
        t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        p = t.data_ptr()
        for sig_stride, prev_stride, prevs, prev_lens, rands, rand_lens in (
                (0, 96, p, p, p, p), (50, 96, p, p, p, p), ((1 << 20) + 4, 96, p, p, p, p), (96, 0, p, p, p, p), (96, 98, p, p, p, p),
                (96, 96, p, None, p, p), (96, 96, None, p, p, p), (96, 96, p, p, None, p), (96, 96, p, p, p, None)):
            assert lib.dh_archive_beacons_device(ar._h, 0, 2, sig_stride, prev_stride, p, p, p, prevs, prev_lens, rands, rand_lens, p,
                                                 ctypes.byref(n), None) == _lib.DH_EINVAL, (sig_stride, prev_stride)
        assert lib.dh_archive_beacons_device(ar._h, 0, 2, 96, 96, None, p, p, None, None, None, None, p, ctypes.byref(n), None) == _lib.DH_EINVAL
        assert lib.dh_archive_beacons_device(ar._h, 0, 2, 96, 96, p, p, p, None, None, None, None, p, None, None) == _lib.DH_EINVAL
        st, cnt = np.zeros(2, np.uint8), (ctypes.c_uint64 * 6)()
        sp = ctypes.c_void_p(st.ctypes.data)
        pk = b"\x00" * 96
        assert lib.dh_archive_check(ar._h, 9, pk, 96, 0, 2, None, None, 0, 64, 0, sp, cnt) == _lib.DH_EINVAL
        assert lib.dh_archive_check(ar._h, 1, pk, 96, 0, 2, None, None, 0, 0, 0, sp, cnt) == _lib.DH_EINVAL
        assert lib.dh_archive_check(ar._h, 1, pk, 96, 0, 2, None, None, 0, 64, 0, None, cnt) == _lib.DH_EINVAL
        assert lib.dh_archive_check(ar._h, 1, None, 96, 0, 2, None, None, 0, 64, 0, sp, cnt) == _lib.DH_EINVAL
        rnd = ctypes.c_uint64(5)
        assert lib.dh_archive_check(ar._h, 1, pk, 96, 0, 2, ctypes.byref(rnd), None, 96, 64, 0, sp, cnt) == _lib.DH_EINVAL
        assert lib.dh_archive_check(ar._h, 1, pk, 96, 5, 2, None, None, 0, 64, 0, sp, cnt) == _lib.DH_OK and cnt[0] == 0  # clamped


@pytest.mark.parametrize("window", [64, 1 << 20])
@pytest.mark.parametrize("name", ac.SCHEMES)
def test_check_against_recorded_statuses(dh, gold, name, window):
    from drand_amd import _lib, scheme_from_name
    from drand_amd.store import AR_DEFERRED, AR_PRED_DEFERRED, DeviceArchive, archive_lines
    s = scheme_from_name(name)
    pk = bytes.fromhex(gold["chains"][name]["pk"])
    data = ac.faulty_archive(name, gold)
    lines = archive_lines(data)
    blank = [i for i, l in enumerate(lines) if not l.strip()]
    want_deferred = [i for i, l in enumerate(lines) if i in blank or l.endswith(b"\r") or l.startswith(b"{ ") or b"zz" in l
                     or l != l.lower()]
    assert len(blank) == 1 and len(want_deferred) == 8
    with DeviceArchive(data) as ar:
        for kind, anchor in ac.ANCHORS.items():
            assert [int(x) for x in ar.check(s, pk, anchor=anchor(name), window=window)] == gold["status"][name][kind], kind
        # the raw ABI: DH_DEFERRED, the deferred records marked and undecided, their successors flagged
        st, cnt = np.zeros(len(ar), np.uint8), (ctypes.c_uint64 * 6)()
        rc = _lib.load().dh_archive_check(ar._h, s.id, pk, len(pk), 0, len(ar), None, None, 0, window, 0, ctypes.c_void_p(st.ctypes.data), cnt)
        assert rc == _lib.DH_DEFERRED, _lib.last_error()
        assert [int(i) for i in np.flatnonzero(st == AR_DEFERRED)] == want_deferred == ar.deferred()
        assert not any(st[want_deferred] & ~np.uint8(AR_DEFERRED))
        succ = [i + 1 for i in want_deferred if i + 1 not in want_deferred]
        assert [int(i) for i in np.flatnonzero(st & AR_PRED_DEFERRED)] == succ
        assert cnt[0] == len(ar) and cnt[1] == 8
        # a window that starts inside the archive takes the record before it as predecessor
        part, cnt2 = np.zeros(40, np.uint8), (ctypes.c_uint64 * 6)()
        rc = _lib.load().dh_archive_check(ar._h, s.id, pk, len(pk), 45, 40, None, None, 0, window, 0, ctypes.c_void_p(part.ctypes.data), cnt2)
        assert rc == _lib.DH_DEFERRED and list(part) == list(st[45:85])
    with DeviceArchive(ac.clean_archive(name, gold)) as ar:
        st, counts = ar.check_device(s, pk, anchor=ac.anchor(name), window=window)
        assert not st.any() and counts == {"checked": ac.N, "deferred": 0, "invalid": 0, "randomness": 0, "sequence": 0, "link": 0}


@pytest.mark.parametrize("name", ["pedersen-bls-chained", "bls-unchained-g1-rfc9380"])
def test_archive_to_trimmed_store(dh, gold, name, tmp_path):
    from drand_amd import scheme_from_name
    from drand_amd.store import DeviceBoltStore, archive_to_trimmed_store, write_trimmed_bolt
    s = scheme_from_name(name)
    pk = bytes.fromhex(gold["chains"][name]["pk"])
    recs = ac.chain_records(name, gold)
    clean = ac.clean_archive(name, gold).replace(b'{"round":101,', b'{ "round":101,').replace(b"\n", b"\n\n   \n", 1)
    got, want = str(tmp_path / "got.db"), str(tmp_path / "want.db")
    for window in (64, 1 << 20):
        res = archive_to_trimmed_store(clean, got, s, pk, anchor=ac.anchor(name), window=window)
        rounds = np.array([r["round"] for r in recs], np.uint64)
        sigs = np.array([np.frombuffer(r["signature"], np.uint8) for r in recs], np.uint8)
        assert write_trimmed_bolt(want, rounds, sigs) == res and res["rows"] == ac.N
        assert open(got, "rb").read() == open(want, "rb").read() and not os.path.exists(got + ".tmp")
    with DeviceBoltStore(got, s.chained) as st:
        # the archive holds no round 0: a chained reader has no previous signature for round 1, and reports only that
        assert st.check_past(s, pk, ac.FIRST + ac.N) == ([ac.FIRST] if s.chained else [])
    os.remove(got)
    with pytest.raises(ValueError, match="#10 "):
        archive_to_trimmed_store(ac.faulty_archive(name, gold), got, s, pk, anchor=ac.anchor(name))
    assert not os.path.exists(got) and not os.path.exists(got + ".tmp")


def test_threads(dh, gold):
    from drand_amd import scheme_from_name
    from drand_amd.store import DeviceArchive
    errs = []

    def run(ar, name):
        try:
            s = scheme_from_name(name)
            pk = bytes.fromhex(gold["chains"][name]["pk"])
            got = [int(x) for x in ar.check(s, pk, anchor=ac.anchor(name), window=64)]
            if got != gold["status"][name]["anchor"]:
                errs.append((name, got))
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    names = ["pedersen-bls-chained", "bls-unchained-g1-rfc9380"]
    ars = [DeviceArchive(ac.faulty_archive(n, gold)) for n in names]
    ths = [threading.Thread(target=run, args=(a, n)) for a, n in zip(ars, names)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not errs, errs
    ths = [threading.Thread(target=run, args=(ars[1], names[1])) for _ in range(2)]  # one handle, two threads
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not errs, errs
    [a.close() for a in ars]


def test_shutdown_invalidates_handles(dh):
    from drand_amd import _lib
    from drand_amd.store import DeviceArchive
    lib = _lib.load()
    data = b"\n".join(g1_line(i) for i in range(100))
    ar = DeviceArchive(data)
    check_parity(dh, data)
    lib.dh_shutdown()
    try:
        for call in (ar.lines, ar.deferred, lambda: ar.beacons_device(0, 10)):
            with pytest.raises(ValueError, match="dh_shutdown"):
                call()
        assert len(ar) == 100  # fixed at open
        ar.close()
    finally:
        assert lib.dh_init(0) == 0, _lib.last_error()
    check_parity(dh, data)
