"""GPU: protobuf beacon records parsed, checked and encoded on the device (DeviceArchive.from_packets / dh_archive_open_pb /
dh_pb_encode_device).

* gather parity with store.packet_from_bytes, field by field: 1, 63, 64, 65 and 257 records of both kinds and both
  signature sizes, signatures at each of the four byte alignments, empty records inside a run, rec_off with gaps, a chunk
  of 64 records of 4096 bytes (read in place) beside a staged one, records of 4096 and 4097 bytes, every deferred class,
  windows that cut chunks, null columns, strides shorter than a value, open errors;
* check for all four schemes against the statuses recorded by the CPU test (tests/golden/packet_cases.json: host check +
  oracle), with the anchor, without one, with one the chain does not follow, windows 64 and 2^20, the beacon ID set and
  matching / not matching / unset / metadata absent, the raw ABI's DH_DEFERRED and deferred list, and an ndjson handle of
  the same chain giving the same bits below 128;
* the encoder byte for byte against packet_bytes, plain and delimited, guard bytes, the sizing call, refusals, the round
  trip through from_packets, and sync_chain_frames -> archive_to_trimmed_store reproducing a store file;
* sync_from_frames equal to sync_from_stream on the decoded packets;
* threads on one handle; use after dh_shutdown."""
import ctypes
import os
import threading

import numpy as np
import pytest

import archive_cases as ac
import packet_cases as pc

pytestmark = pytest.mark.gpu
KINDS = (pc.BP, pc.PR)


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
    return pc.load_golden()


@pytest.fixture(scope="module")
def gold_ar():
    return ac.load_golden()


def ascii_only(r):
    md = r["metadata"] or {}
    return all(ord(c) < 128 for c in md.get("beacon_id", "") + ((md.get("node_version") or {}).get("prerelease") or ""))


def expected(kind, records, sig_stride, prev_stride):
    """The columns dh_archive_beacons_device must write, from packet_from_bytes (pinned against google.protobuf by the CPU
    test); a record is deferred here exactly when it is not what packet_bytes writes for its fields, holds a string byte
    above 0x7f, or is longer than 4096 bytes."""
    from drand_amd.store import DECODE_ERRORS, packet_bytes, packet_from_bytes
    m = len(records)
    rounds, dfr = np.zeros(m, np.uint64), np.zeros(m, np.uint8)
    cols = {k: np.zeros((m, s), np.uint8) for k, s in (("signature", sig_stride), ("previous_signature", prev_stride), ("randomness", 32))}
    lens = {k: np.zeros(m, np.int32) for k in cols}
    for i, b in enumerate(records):
        try:
            r = packet_from_bytes(kind, b)
        except DECODE_ERRORS:
            r = None
        if r is None or packet_bytes(kind, r) != b or len(b) > 4096 or not ascii_only(r):
            dfr[i] = 1
            continue
        rounds[i] = r["round"]
        for k in cols:
            lens[k][i] = len(r[k])
            if len(r[k]) <= cols[k].shape[1]:  # a longer value leaves the row zero, never a prefix
                cols[k][i, :len(r[k])] = np.frombuffer(r[k], np.uint8)
    return rounds, cols, lens, dfr


def check_parity(dh, kind, records, windows=None, sig_stride=None, prev_stride=None, want_prev=True, want_rand=True, gaps=None):
    """records: the byte strings; gaps: bytes of filler before each record (rec_off with gaps)."""
    from drand_amd.store import DeviceArchive
    if gaps:
        data, offs = b"", []
        for i, b in enumerate(records):
            data += b"\xee" * gaps[i % len(gaps)]
            offs.append(len(data))
            data += b
        data += b"\xee" * 5
        ar = DeviceArchive.from_packets(kind, data, lens=[len(b) for b in records], offs=offs)
    else:
        offs = list(np.cumsum([0] + [len(b) for b in records[:-1]])) if records else []
        ar = DeviceArchive.from_packets(kind, records)
    with ar:
        st = ar.stat()
        assert len(ar) == len(records) == st["records"] and ar.kind == kind and st["tile_bytes"] == 0
        off, ln = ar.lines()
        assert list(off) == offs and list(ln) == [len(b) for b in records]
        for first, n in windows or [(0, len(records))]:
            got = ar.beacons_device(first, n, sig_stride=sig_stride, prev_stride=prev_stride, want_prev=want_prev, want_rand=want_rand)
            rounds, sigs, sig_lens, prevs, prev_lens, rands, rand_lens, dfr = [None if t is None else t.cpu().numpy() for t in got]
            w_rounds, cols, lens, w_dfr = expected(kind, records[first:first + n], sigs.shape[1], prevs.shape[1] if want_prev else 4)
            assert list(dfr) == list(w_dfr), (first, n)
            assert list(rounds.view(np.uint64)) == list(w_rounds), (first, n)
            assert np.array_equal(sigs, cols["signature"]) and list(sig_lens) == list(lens["signature"]), (first, n)
            if want_prev:
                assert np.array_equal(prevs, cols["previous_signature"]) and list(prev_lens) == list(lens["previous_signature"])
            else:
                assert prevs is None and prev_lens is None
            if want_rand:
                assert np.array_equal(rands, cols["randomness"]) and list(rand_lens) == list(lens["randomness"])
                assert kind == pc.PR or not rand_lens.any()
            else:
                assert rands is None and rand_lens is None
            assert ar.deferred(first, n) == [first + int(i) for i in np.flatnonzero(w_dfr)]
        if not windows:
            assert st["deferred"] == int(w_dfr.sum())
            assert st["longest_line"] == max([0] + [min(len(b), 4097) for b in records])
            for k, name in (("signature", "longest_signature"), ("previous_signature", "longest_previous"), ("randomness", "longest_randomness")):
                assert st[name] == (int(lens[k].max()) if len(records) else 0)
        return st


def rec_bytes(kind, shape, i, bid=pc.BEACON_ID):
    from drand_amd.store import packet_bytes
    return packet_bytes(kind, (pc.g1_rec if shape == "g1" else pc.g2_rec)(i, kind), bid)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("shape", ["g1", "g2"])
@pytest.mark.parametrize("kind", KINDS)
def test_column_parity_wave_and_workgroup_edges(dh, kind, shape, n):
    check_parity(dh, kind, [rec_bytes(kind, shape, i) for i in range(n)])


@pytest.mark.parametrize("kind", KINDS)
def test_alignments_empty_records_and_gaps(dh, kind):
    from drand_amd.store import packet_bytes
    # a beaconID of 0-3 bytes moves every later record, and with it each signature, through the four byte alignments
    recs = [rec_bytes(kind, "g2" if i % 3 else "g1", i, "abc"[:i % 4]) for i in range(150)]
    check_parity(dh, kind, recs)
    for i in (0, 5, 6, 64, 100, 149):
        recs[i] = b""  # empty records: canonical, round 0
    check_parity(dh, kind, recs)
    check_parity(dh, kind, [b""] * 70)  # an empty buffer of 70 records
    check_parity(dh, kind, [])
    check_parity(dh, kind, recs, gaps=[0, 1, 2, 3, 5, 17])
    check_parity(dh, kind, recs[:3], gaps=[40000])  # a chunk spread wider than the staging limit: read in place
    edge = [packet_bytes(kind, r) for r in pc.edge_records(kind).values()]
    st = check_parity(dh, kind, edge)
    assert st["deferred"] == 0


@pytest.mark.parametrize("kind", KINDS)
def test_long_records_and_deferred_classes(dh, kind):
    big = [pc.record_of_length(kind, 4096)] * 64
    st = check_parity(dh, kind, [rec_bytes(kind, "g1", i) for i in range(64)] + big + [rec_bytes(kind, "g2", 1)])
    assert st["deferred"] == 0 and st["longest_line"] == 4096
    st = check_parity(dh, kind, [rec_bytes(kind, "g1", 0), pc.record_of_length(kind, 4096), pc.record_of_length(kind, 4097), rec_bytes(kind, "g1", 1)])
    assert st["deferred"] == 1 and st["longest_line"] == 4097
    deferred = pc.deferred_records(kind)
    recs = []
    for i, d in enumerate(deferred):
        recs += [rec_bytes(kind, "g1", i), d]
    st = check_parity(dh, kind, recs)
    assert st["deferred"] == len(deferred)
    check_parity(dh, kind, deferred)  # a chunk without one canonical record


def test_windows_null_columns_and_short_strides(dh):
    kind = pc.PR
    recs = [rec_bytes(kind, "g2" if i % 3 else "g1", i) for i in range(200)]
    recs[70], recs[130] = b"\x08\x00", b""
    windows = [(0, 200), (1, 63), (1, 64), (63, 2), (64, 64), (65, 135), (199, 1), (199, 50), (200, 5), (500, 1), (10, 0)]
    check_parity(dh, kind, recs, windows)
    check_parity(dh, kind, recs, windows[:4], want_prev=False)
    check_parity(dh, kind, recs, windows[:4], want_rand=False)
    check_parity(dh, kind, recs, windows[:4], want_prev=False, want_rand=False)
    check_parity(dh, kind, recs, windows[:3], sig_stride=48, prev_stride=92)
    check_parity(dh, kind, recs, windows[:3], sig_stride=4, prev_stride=4)
    check_parity(dh, pc.BP, [rec_bytes(pc.BP, "g2", i) for i in range(70)], windows[:3], sig_stride=92, prev_stride=100)


def test_open_refusals_and_delimited_input(dh, tmp_path):
    from drand_amd import _lib
    from drand_amd.store import DeviceArchive, delimited
    lib = _lib.load()
    a, b = rec_bytes(pc.BP, "g1", 0), rec_bytes(pc.BP, "g2", 1)
    with pytest.raises(ValueError, match="sum to"):
        DeviceArchive.from_packets(pc.BP, a + b, lens=[len(a), len(b) - 1])
    with pytest.raises(ValueError, match="outside the buffer"):
        DeviceArchive.from_packets(pc.BP, a + b, lens=[len(a), len(b) + 1])
    with pytest.raises(ValueError, match="outside the buffer"):
        DeviceArchive.from_packets(pc.BP, a + b, lens=[len(a), len(b)], offs=[0, len(a) + 1])
    with pytest.raises(ValueError, match="outside the buffer"):
        DeviceArchive.from_packets(pc.BP, a + b, lens=[len(a), 4], offs=[0, len(a) - 1])  # overlapping
    with pytest.raises(ValueError, match="kind"):
        DeviceArchive.from_packets(3, a, lens=[len(a)])
    h = ctypes.c_void_p()
    ln = (ctypes.c_uint32 * 1)(5)
    assert lib.dh_archive_open_pb(1, None, 5, None, ln, 1, ctypes.byref(h)) == _lib.DH_EINVAL
    assert lib.dh_archive_open_pb(1, b"12345", 5, None, None, 1, ctypes.byref(h)) == _lib.DH_EINVAL
    assert lib.dh_archive_open_pb(1, b"12345", 5, None, ln, 1, None) == _lib.DH_EINVAL
    assert lib.dh_archive_kind(None) == _lib.DH_EINVAL
    # a varint-delimited buffer and file, with a cut frame behind the last record
    data = delimited([a, b"", b, a]) + b"\x30abc"
    path = str(tmp_path / "frames.bin")
    open(path, "wb").write(data)
    for src in (data, path):
        with DeviceArchive.from_packets(pc.BP, src) as ar:
            assert len(ar) == 4 and ar.unframed == b"\x30abc" and [ar.line(i) for i in range(4)] == [a, b"", b, a]
            assert lib.dh_archive_kind(ar._h) == 1 and ar.deferred() == []
    with DeviceArchive(b"{}\n") as ar:
        assert lib.dh_archive_kind(ar._h) == 0


def same_chain_ndjson(name, gold_ar, run):
    """The JSON-lines archive of the decodable records of a run of packets."""
    from drand_amd.store import packet_from_bytes, random_data_line
    return b"\n".join(random_data_line(packet_from_bytes(pc.PR, b)) for b in run) + b"\n"


@pytest.mark.parametrize("window", [64, 1 << 20])
@pytest.mark.parametrize("name", ac.SCHEMES)
def test_check_against_recorded_statuses(dh, gold, gold_ar, name, window):
    from drand_amd import _lib, scheme_from_name
    from drand_amd.store import AR_BEACON_ID, AR_DEFERRED, AR_PRED_DEFERRED, DeviceArchive
    s = scheme_from_name(name)
    pk = bytes.fromhex(gold_ar["chains"][name]["pk"])
    for kname, kind in pc.KINDS.items():
        run = pc.faulty_run(name, gold_ar, kind)
        want = {m: list(bytes.fromhex(h)) for m, h in gold["status"][name][kname].items()}
        want_deferred = [90, 127, 128, 140, 191, 192]
        with DeviceArchive.from_packets(kind, run) as ar:
            for mode, (anchor, bid) in pc.MODES.items():
                assert [int(x) for x in ar.check(s, pk, anchor=anchor(name), window=window, beacon_id=bid)] == want[mode], (kname, mode)
            # bytes instead of str, and an ID nothing matches: every record with metadata is marked
            assert [int(x) for x in ar.check(s, pk, anchor=ac.anchor(name), window=window, beacon_id=pc.BEACON_ID.encode())] == want["anchor"]
            other = ar.check(s, pk, anchor=ac.anchor(name), window=window, beacon_id="")
            assert [i for i, x in enumerate(other) if not x & AR_BEACON_ID] == [76, 77, 90, 100]  # the empty ID, no metadata, undecodable, empty
            # the raw ABI: DH_DEFERRED, the deferred records marked and undecided, their successors flagged
            ar.set_beacon_id(pc.BEACON_ID)
            st, cnt = np.zeros(len(ar), np.uint8), (ctypes.c_uint64 * 6)()
            rc = _lib.load().dh_archive_check(ar._h, s.id, pk, len(pk), 0, len(ar), None, None, 0, window, 0, ctypes.c_void_p(st.ctypes.data), cnt)
            assert rc == _lib.DH_DEFERRED, _lib.last_error()
            assert [int(i) for i in np.flatnonzero(st == AR_DEFERRED)] == want_deferred == ar.deferred()
            succ = [i + 1 for i in want_deferred if i + 1 not in want_deferred]
            assert [int(i) for i in np.flatnonzero(st & AR_PRED_DEFERRED)] == succ
            assert cnt[0] == len(ar) and cnt[1] == len(want_deferred)
            assert [int(i) for i in np.flatnonzero(st & AR_BEACON_ID)] == [75, 76, 78]
            part, cnt2 = np.zeros(40, np.uint8), (ctypes.c_uint64 * 6)()
            rc = _lib.load().dh_archive_check(ar._h, s.id, pk, len(pk), 45, 40, None, None, 0, window, 0, ctypes.c_void_p(part.ctypes.data), cnt2)
            assert rc == _lib.DH_OK and list(part) == list(st[45:85])
        if kind == pc.PR:  # an ndjson handle of the same chain: the same bits below 128, and never bit 128
            keep = [i for i in range(len(run)) if i != 90]
            with DeviceArchive(same_chain_ndjson(name, gold_ar, [run[i] for i in keep])) as ar:
                got = [int(x) for x in ar.check(s, pk, anchor=ac.anchor(name), window=window)]
            host = want["id_unset"]
            # record 91's predecessor is the undecodable record 90's predecessor on both sides
            assert got == [host[i] for i in keep]
        with DeviceArchive.from_packets(kind, pc.chain_packets(name, gold_ar, kind)[1]) as ar:
            ar.set_beacon_id(pc.BEACON_ID)
            st, counts = ar.check_device(s, pk, anchor=ac.anchor(name), window=window)
            assert not st.any() and counts == {"checked": ac.N, "deferred": 0, "invalid": 0, "randomness": 0, "sequence": 0, "link": 0}


# ---- the encoder

def columns(recs, sig_stride, prev_stride, want_prev=True):
    import torch
    n = len(recs)
    rounds = np.array([r.get("round", 0) for r in recs], np.uint64)
    sigs, prevs = np.full((n, sig_stride), 0xCD, np.uint8), np.full((n, prev_stride), 0xCD, np.uint8)  # the padding is never read
    sl, pl = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i, r in enumerate(recs):
        s, p = r.get("signature", b""), r.get("previous_signature", b"")
        sigs[i, :len(s)], sl[i] = np.frombuffer(s, np.uint8), len(s)
        prevs[i, :len(p)], pl[i] = np.frombuffer(p, np.uint8), len(p)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    out = [dev(rounds.view(np.int64)), dev(sigs), dev(sl)]
    return out + ([dev(prevs), dev(pl)] if want_prev else [None, None])


def mixed_rows(n, seed):
    """Rows of every shape the encoder writes: G1 and chained G2, round 0, signature length 0, lengths across 127 / 128,
    rounds of every varint size."""
    out = []
    for i in range(n):
        k = (i + seed) % 11
        r = dict(pc.g2_rec(i) if i % 2 else pc.g1_rec(i), randomness=b"")
        if k == 3:
            r["round"] = 0
        elif k == 5:
            r["signature"] = b""
        elif k == 7:
            r["signature"] = pc.rand_bytes("enc sig %d" % i, 126 + i % 4)
        elif k == 8:
            r["round"] = [(1 << 64) - 1, 1 << 63, (1 << 35) + i, 127, 128][i % 5]
        elif k == 9:
            r = {"round": 0, "signature": b"", "previous_signature": b""}
        out.append(r)
    return out


def encode(recs, beacon_id, delimited, sig_stride=132, prev_stride=96, want_prev=True):
    from drand_amd.store import encode_beacon_packets
    rounds, sigs, sl, prevs, pl = columns(recs, sig_stride, prev_stride, want_prev)
    out, lens = encode_beacon_packets(rounds, sigs, sl, prevs, pl, beacon_id=beacon_id, delimited=delimited)
    return bytes(out.cpu().numpy()), [int(x) for x in lens.cpu().numpy()]


def want_bytes(recs, beacon_id, delim, want_prev=True):
    from drand_amd.store import delimited, packet_bytes
    pk = [packet_bytes(pc.BP, r if want_prev else dict(r, previous_signature=b""), beacon_id) for r in recs]
    return (delimited(pk) if delim else b"".join(pk)), [len(b) for b in pk]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 257])
@pytest.mark.parametrize("delim", [False, True])
def test_encoder_equals_packet_bytes(dh, n, delim):
    # a beacon ID of NULL, "" and 1-4 bytes moves every chunk's region through the byte alignments
    for k, bid in enumerate([None, "", "a", "ab", "abc", "abcd"]):
        recs = mixed_rows(n, k)
        assert encode(recs, bid, delim) == want_bytes(recs, bid, delim), (bid, n)
    for shape, stride in ((pc.g1_rec, 48), (pc.g2_rec, 96)):  # the schemes' own shapes; unchained: no previous_signature column
        recs = [dict(shape(i), randomness=b"") for i in range(n)]
        assert encode(recs, "default", delim, stride, 96) == want_bytes(recs, "default", delim)
        assert encode(recs, "default", delim, stride, 96, want_prev=False) == want_bytes(recs, "default", delim, want_prev=False)


def test_encoder_bytewise_path_guards_and_refusals(dh):
    import torch
    from drand_amd import _lib
    lib = _lib.load()
    # 64 rows of about 1 KiB: the chunk is wider than the staging limit and is written row by row, beside a staged chunk
    recs = [{"round": 1 + i, "signature": pc.rand_bytes("wide %d" % i, 1000 + i % 7), "previous_signature": b""} for i in range(64)]
    recs += [dict(pc.g2_rec(i), randomness=b"") for i in range(70)]
    for delim in (False, True):
        assert encode(recs, "x", delim, sig_stride=1008) == want_bytes(recs, "x", delim)
    # the raw ABI: sizing, guard bytes around the region at every alignment of its start, refusals
    recs = mixed_rows(130, 1)
    want, want_lens = want_bytes(recs, "id", False)
    rounds, sigs, sl, prevs, pl = columns(recs, 132, 96)
    total, lens = ctypes.c_size_t(0), torch.zeros(len(recs), dtype=torch.int32, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731

    def call(out, cap, n=len(recs), kind=1, sig_stride=132, pv=p(prevs), pvl=p(pl), bid=b"id"):
        torch.cuda.synchronize()
        return lib.dh_pb_encode_device(kind, p(rounds), p(sigs), sig_stride, p(sl), pv, 96, pvl, n, bid, len(bid or b""), 0, out, cap, p(lens),
                                       ctypes.byref(total), None)
    assert call(None, 0) == _lib.DH_OK and total.value == len(want) and [int(x) for x in lens.cpu()] == want_lens
    for shift in range(4):
        buf = torch.full((len(want) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        assert call(buf.data_ptr() + 16 + shift, len(want)) == _lib.DH_OK, _lib.last_error()
        got = bytes(buf.cpu().numpy())
        assert got[16 + shift:16 + shift + len(want)] == want
        assert got[:16 + shift] == b"\xa5" * (16 + shift) and got[16 + shift + len(want):] == b"\xa5" * (48 - shift)
    buf = torch.zeros(len(want), dtype=torch.uint8, device="cuda")
    assert call(buf.data_ptr(), len(want) - 1) == _lib.DH_EINVAL and total.value == len(want)  # cap too small: the size is still given
    assert call(buf.data_ptr(), len(want), kind=2) == _lib.DH_EINVAL
    assert call(buf.data_ptr(), len(want), pv=None) == _lib.DH_EINVAL and call(buf.data_ptr(), len(want), pvl=None) == _lib.DH_EINVAL
    assert call(buf.data_ptr(), len(want), sig_stride=130) == _lib.DH_EINVAL
    assert call(buf.data_ptr(), len(want), n=(1 << 24)) == _lib.DH_EINVAL and "split" in _lib.last_error()
    assert call(buf.data_ptr(), len(want), n=0) == _lib.DH_OK and total.value == 0
    # an oversized row: 4090 signature bytes and the rest pass 4096; a length above its stride
    big = [dict(pc.g1_rec(i), randomness=b"") for i in range(70)]
    big[66]["signature"] = b"\x11" * 4090
    with pytest.raises(ValueError, match="row 66"):
        encode(big, "a-long-beacon-id", False, sig_stride=4092)
    big[66]["signature"] = b"\x11" * 4080
    assert encode(big, "x", True, sig_stride=4092) == want_bytes(big, "x", True)
    sl2 = sl.clone()
    sl2[5] = 133
    torch.cuda.synchronize()
    assert lib.dh_pb_encode_device(1, p(rounds), p(sigs), 132, p(sl2), p(prevs), 96, p(pl), len(recs), None, 0, 0, None, 0, None, ctypes.byref(total),
                                   None) == _lib.DH_EINVAL and "row 5" in _lib.last_error()


@pytest.mark.parametrize("name", ["pedersen-bls-chained", "bls-unchained-g1-rfc9380"])
def test_round_trip_and_store_to_frames_to_store(dh, gold_ar, name, tmp_path):
    import torch
    from drand_amd import scheme_from_name
    from drand_amd.store import (DeviceArchive, DeviceBoltStore, archive_to_trimmed_store, delimited, packet_bytes, sync_chain_frames,
                                 write_trimmed_bolt)
    s = scheme_from_name(name)
    pk = bytes.fromhex(gold_ar["chains"][name]["pk"])
    recs = ac.chain_records(name, gold_ar)
    # encode -> from_packets -> the same columns
    rows = mixed_rows(150, 2)
    rounds, sigs, sl, prevs, pl = columns(rows, 132, 96)
    from drand_amd.store import encode_beacon_packets
    out, lens = encode_beacon_packets(rounds, sigs, sl, prevs, pl, beacon_id="rt")
    with DeviceArchive.from_packets(pc.BP, bytes(out.cpu().numpy()), lens=lens.cpu().numpy()) as ar:
        g = ar.beacons_device(sig_stride=132, prev_stride=96)
        assert torch.equal(g[0], rounds) and torch.equal(g[2], sl) and torch.equal(g[4], pl) and not g[7].any()
        mask = lambda rows_, ln: rows_ * (torch.arange(rows_.shape[1], device="cuda")[None, :] < ln[:, None])  # noqa: E731
        assert torch.equal(g[1], mask(sigs, sl)) and torch.equal(g[3], mask(prevs, pl))
    # a store (the anchor as round 0, then the signed chain) -> SyncChain's frames -> checked -> the same store file
    src, got = str(tmp_path / "src.db"), str(tmp_path / "got.db")
    all_rounds = np.array([ac.FIRST - 1] + [r["round"] for r in recs], np.uint64)
    all_sigs = np.array([np.frombuffer(ac.anchor_sig(name), np.uint8)] + [np.frombuffer(r["signature"], np.uint8) for r in recs], np.uint8)
    write_trimmed_bolt(src, all_rounds, all_sigs)
    for window in (64, 1 << 20):
        with DeviceBoltStore(src, s.chained) as st:
            frames = [bytes(f.cpu().numpy()) for f, _l in sync_chain_frames(st, ac.FIRST, pc.BEACON_ID, window=window, delimited=True)]
        assert len(frames) == (5 if window == 64 else 1)
        want = [packet_bytes(pc.BP, dict(r, randomness=b"", previous_signature=r["previous_signature"] if s.chained else b""), pc.BEACON_ID)
                for r in recs]
        assert b"".join(frames) == delimited(want)
        with DeviceArchive.from_packets(pc.BP, b"".join(frames)) as ar:
            assert not ar.check(s, pk, anchor=ac.anchor(name), beacon_id=pc.BEACON_ID).any()
            archive_to_trimmed_store(ar, got, s, pk, anchor=ac.anchor(name), window=window)
        want_db = str(tmp_path / "want.db")
        write_trimmed_bolt(want_db, all_rounds[1:], all_sigs[1:])
        assert open(got, "rb").read() == open(want_db, "rb").read()


# ---- sync_from_frames

def genesis_store(name, upto=0, gold_ar=None):
    from drand_amd.sync import TrimmedMemStore
    st = TrimmedMemStore(name == "pedersen-bls-chained")
    st.put(ac.FIRST - 1, ac.anchor_sig(name))
    for r in (ac.chain_records(name, gold_ar)[:upto] if upto else []):
        st.put(r["round"], r["signature"])
    return st


@pytest.mark.parametrize("name", ["pedersen-bls-chained", "bls-unchained-g1-rfc9380"])
def test_sync_from_frames_equals_sync_from_stream(dh, gold_ar, name):
    from drand_amd import scheme_from_name
    from drand_amd.store import delimited, packet_bytes, packet_from_bytes
    from drand_amd.sync import sync_from_frames, sync_from_stream
    s = scheme_from_name(name)
    pk = bytes.fromhex(gold_ar["chains"][name]["pk"])
    recs = [dict(r, randomness=b"") for r in ac.chain_records(name, gold_ar)[:200]]

    def frames_of(rs, ids=None):
        return [packet_bytes(pc.BP, r, (ids or {}).get(i, pc.BEACON_ID)) for i, r in enumerate(rs)]

    def both(frames, up_to, stored_before=0, resync=False, cut=None):
        """(done, stored, the store's content) of both paths; the stream sees the frames before an undecodable one."""
        out = []
        for path in ("frames", "stream"):
            st = genesis_store(name, stored_before, gold_ar)
            if path == "frames":
                res = sync_from_frames(frames, s, pk, st, up_to, beacon_id=pc.BEACON_ID, resync=resync, window=64)
            else:
                pkts = [packet_from_bytes(pc.BP, f) for f in frames[:cut]]
                res = sync_from_stream(iter(pkts), s, pk, st, up_to, beacon_id=pc.BEACON_ID, window=64, resync=resync)
            out.append((res[0], res[1], dict(st._sigs)))
        assert out[0] == out[1]
        return out[0]

    clean = frames_of(recs)
    done, stored, _ = both(clean, 150)
    assert done and stored == list(range(ac.FIRST, 151))
    assert both(clean, 5000)[:2] == (False, list(range(ac.FIRST, ac.FIRST + 200)))  # the stream ends first
    bad = list(recs)
    sig = bad[120]["signature"]
    bad[120] = dict(bad[120], signature=sig[:7] + bytes([sig[7] ^ 4]) + sig[8:])
    assert both(frames_of(bad), 180)[:2] == (False, list(range(ac.FIRST, ac.FIRST + 120)))
    short = list(recs)
    short[33] = dict(short[33], signature=short[33]["signature"][:-1])
    assert both(frames_of(short), 180)[:2] == (False, list(range(ac.FIRST, ac.FIRST + 33)))
    assert both(frames_of(recs, {77: "other"}), 180)[:2] == (False, list(range(ac.FIRST, ac.FIRST + 77)))  # a wrong beacon ID
    assert both(frames_of(recs, {77: None}), 100)[0]  # no metadata is no mismatch
    gap = frames_of(recs[:60] + recs[61:])
    assert both(gap, 180)[:2] == (False, list(range(ac.FIRST, ac.FIRST + 60)))
    # packets already stored: the first frame is the store's last beacon (ErrBeaconAlreadyStored ends the peer)
    assert both(clean[9:], 10, stored_before=10)[:2] == (True, [])
    assert both(clean[9:], 50, stored_before=10)[:2] == (False, [])
    undecodable = clean[:90] + [b"\xff\xff"] + clean[91:]
    assert both(undecodable, 180, cut=90)[:2] == (False, list(range(ac.FIRST, ac.FIRST + 90)))
    deferred = clean[:40] + [clean[40] + b"\x38\x01"] + clean[41:]  # an unknown field: decoded on the host, stored like the rest
    assert both(deferred, 100)[:2] == (True, list(range(ac.FIRST, 101)))
    done, stored, content = both(clean[100:], 180, resync=True)
    assert done and stored == list(range(ac.FIRST + 100, 181)) and len(content) == 81
    # one buffer with lengths, and a varint-delimited buffer, read the same frames
    for kw in ({"frames": b"".join(clean), "lens": [len(f) for f in clean]}, {"frames": delimited(clean)}):
        st = genesis_store(name)
        assert sync_from_frames(scheme=s, pubkey=pk, store=st, up_to=20, beacon_id=pc.BEACON_ID, **kw) == (True, list(range(ac.FIRST, 21)))


# ---- handles

def test_threads_on_one_handle(dh, gold, gold_ar):
    from drand_amd import scheme_from_name
    from drand_amd.store import DeviceArchive
    name, errs = "bls-unchained-g1-rfc9380", []
    s, pk = scheme_from_name(name), bytes.fromhex(gold_ar["chains"][name]["pk"])
    want = list(bytes.fromhex(gold["status"][name]["beacon_packet"]["anchor"]))

    def run(ar):
        try:
            got = [int(x) for x in ar.check(s, pk, anchor=ac.anchor(name), window=64, beacon_id=pc.BEACON_ID)]
            if got != want:
                errs.append(got)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    with DeviceArchive.from_packets(pc.BP, pc.faulty_run(name, gold_ar, pc.BP)) as ar:
        ths = [threading.Thread(target=run, args=(ar,)) for _ in range(2)]
        [t.start() for t in ths]
        [t.join() for t in ths]
    assert not errs, errs


def test_shutdown_invalidates_handles(dh):
    from drand_amd import _lib
    from drand_amd.store import DeviceArchive
    lib = _lib.load()
    recs = [rec_bytes(pc.BP, "g1", i) for i in range(100)]
    ar = DeviceArchive.from_packets(pc.BP, recs)
    lib.dh_shutdown()
    try:
        for call in (ar.lines, ar.deferred, lambda: ar.beacons_device(0, 10), lambda: ar.set_beacon_id("x")):
            with pytest.raises(ValueError, match="dh_shutdown"):
                call()
        assert len(ar) == 100 and lib.dh_archive_kind(ar._h) == 1  # fixed at open
        ar.close()
    finally:
        assert lib.dh_init(0) == 0, _lib.last_error()
    check_parity(dh, pc.BP, recs)
