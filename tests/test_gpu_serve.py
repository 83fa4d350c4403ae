"""GPU: the records a node or relay serves, encoded on the device (dh_rand_encode_device, store.encode_random_data /
encode_public_rand and what is built on them).

The yardsticks are store.random_data_line and store.packet_bytes(PB_PUBLIC_RAND, ...) (tests/serve_cases.py), which the
CPU suite pins, the latter against google.protobuf; never the code under test.

* byte for byte, both forms: 1, 63, 64, 65 and 257 rows; G1 rows with strides 48 and 64; G2 rows with previous signatures
  of 96, 32 and 0 bytes in one chunk; signature lengths 0, 1, 3 and 47; no previous-signature column; every digit count
  and varint length of the round on both sides of each boundary;
* the randomness computed (hashlib per row), given (arbitrary rows), and the verifier's column agreeing with the computed
  one; the keep mask (all, none, alternating, a whole chunk, the verifier's verdicts, a skipped over-long row);
* newline / delimited / metadata; the output at the four byte alignments between guard bytes, the sizing call, the
  lengths, a short cap; the in-place path of a chunk above 36 KiB; the refusals decided on the device;
* round trips through DeviceArchive (no record deferred, the same columns, the recorded statuses), store -> archive ->
  store and store -> PublicRandResponse -> store byte for byte, the reference's store fixtures, export and
  relay_s3_sync_store leaving the faulty rounds out, sync_chain_frames unchanged;
* two identical calls, four threads, a call after dh_shutdown (it re-initialises the library, as dh_pb_encode_device
  does)."""
import ctypes
import hashlib
import threading

import numpy as np
import pytest

import archive_cases as ac
import bolt_json_cases as jc
import packet_cases as pc
import serve_cases as sc

pytestmark = pytest.mark.gpu
JSON, PB = 1, 2
FORMS = (JSON, PB)
META = {"beacon_id": pc.BEACON_ID}


@pytest.fixture(scope="module")
def dh():
    import torch
    import drand_amd
    from drand_amd import _lib
    torch.zeros(1, device="cuda")
    assert _lib.load().dh_init(0) == 0, _lib.last_error()
    assert "dh_rand_encode_device" in _lib.SIGNATURES
    return drand_amd


@pytest.fixture(scope="module")
def gold_ar():
    return ac.load_golden()


@pytest.fixture(scope="module")
def gold_pc():
    return pc.load_golden()


def to_dev(rows32):
    import torch
    return torch.from_numpy(np.frombuffer(b"".join(rows32), np.uint8).reshape(-1, 32).copy()).cuda()


def encode(form, rows, sig_stride=132, prev_stride=96, want_prev=True, rands=None, keep=None, framed=False, metadata=None):
    """(bytes, lengths) from the device for `rows` (record dicts)."""
    import torch
    from drand_amd import store
    rounds, sigs, sl, prevs, pl = sc.columns(rows, sig_stride, prev_stride, want_prev)
    d_rands = to_dev(rands) if rands is not None else None
    d_keep = torch.tensor(keep, dtype=torch.uint8, device="cuda") if keep is not None else None
    if form == JSON:
        out, lens = store.encode_random_data(rounds, sigs, sl, prevs, pl, rands=d_rands, keep=d_keep, newline=framed)
    else:
        out, lens = store.encode_public_rand(rounds, sigs, sl, prevs, pl, rands=d_rands, keep=d_keep, metadata=metadata, delimited=framed)
    return bytes(out.cpu().numpy()), [int(x) for x in lens.cpu().numpy()]


def want(form, rows, want_prev=True, rands=None, keep=None, framed=False, metadata=None):
    if form == JSON:
        return sc.want_json(rows, rands, keep, framed, want_prev)
    return sc.want_pb(rows, rands, keep, framed, metadata, want_prev)


def same(form, rows, sig_stride=132, prev_stride=96, **kw):
    got = encode(form, rows, sig_stride, prev_stride, **kw)
    exp = want(form, rows, **kw)
    assert got[1] == exp[1], (form, kw.keys())
    assert got[0] == exp[0], (form, kw.keys())


def unframed(form):
    """The Python entry point of a form, writing the records back to back."""
    from drand_amd import store
    if form == JSON:
        return lambda *a, **kw: store.encode_random_data(*a, newline=False, **kw)
    return store.encode_public_rand


# ---- byte for byte

@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("form", FORMS)
def test_byte_for_byte(dh, form, n):
    for seed in (0, 5):  # the shapes move through the lanes
        rows = sc.shaped_rows(n, seed)
        same(form, rows, framed=bool(seed))
    same(form, sc.shaped_rows(n, 3), want_prev=False)  # d_prevs NULL
    g1 = [dict(pc.g1_rec(i), randomness=b"") for i in range(n)]
    for stride in (48, 64):
        same(form, g1, sig_stride=stride, want_prev=False, framed=True)
    g2 = [dict(pc.g2_rec(i), randomness=b"") for i in range(n)]
    same(form, g2, sig_stride=96, framed=True)


@pytest.mark.parametrize("form", FORMS)
def test_rounds_of_every_digit_count_and_varint_length(dh, form):
    rows = sc.boundary_rows()
    assert len(rows) == 43
    same(form, rows, framed=True)
    same(form, [{"round": r, "signature": b"", "previous_signature": b""} for r in sc.BOUNDARY_ROUNDS])


def verify_device(s, pk, rounds, sigs, prevs, pl, seed=1):
    import torch
    from drand_amd import _lib
    n = len(rounds)
    verdict = torch.zeros(n, dtype=torch.uint8, device="cuda")
    rand = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = _lib.load().dh_verify_batch_device(s.id, pk, len(pk), rounds.data_ptr(), sigs.data_ptr(), sigs.shape[1],
                                            prevs.data_ptr() if s.chained else None, prevs.shape[1] if s.chained else 0,
                                            pl.data_ptr() if s.chained else None, n, verdict.data_ptr(), rand.data_ptr(), seed, None, None)
    assert rc == 0, _lib.last_error()
    return verdict, rand


@pytest.mark.parametrize("form", FORMS)
def test_randomness_computed_given_and_the_verifiers(dh, gold_ar, form):
    from drand_amd import scheme_from_name, store
    rows = sc.shaped_rows(130, 1)
    got, lens = encode(form, rows)
    at = 0
    for r, ln in zip(rows, lens):  # computed: SHA-256 of the row's signature, the empty string's for length 0
        rec = store.random_data_from_line(got[at:at + ln]) if form == JSON else store.packet_from_bytes(pc.PR, got[at:at + ln])
        assert rec["randomness"] == hashlib.sha256(r["signature"]).digest()
        at += ln
    given = [pc.rand_bytes("given randomness %d" % i, 32) for i in range(len(rows))]
    given[7] = b"\x00" * 32
    same(form, rows, rands=given, framed=True)
    for name in ("pedersen-bls-chained", "bls-unchained-g1-rfc9380"):  # the verifier's column for a golden chain
        s, pk = scheme_from_name(name), bytes.fromhex(gold_ar["chains"][name]["pk"])
        recs = ac.chain_records(name, gold_ar)
        rounds, sigs, sl, prevs, pl = sc.columns(recs, s.sig_len, 96, s.chained)
        verdict, rand = verify_device(s, pk, rounds, sigs, prevs, pl)
        assert bool(verdict.all())
        enc = unframed(form)
        a, la = enc(rounds, sigs, sl, prevs, pl, rands=rand)
        b, lb = enc(rounds, sigs, sl, prevs, pl)
        assert bytes(a.cpu().numpy()) == bytes(b.cpu().numpy()) == want(form, recs, want_prev=s.chained)[0]
        assert la.tolist() == lb.tolist()


@pytest.mark.parametrize("form", FORMS)
def test_keep_mask(dh, gold_ar, form):
    import torch
    from drand_amd import _lib, scheme_from_name, store
    rows = sc.shaped_rows(200, 2)
    n = len(rows)
    block = [0 if 64 <= i < 128 else 1 for i in range(n)]  # a whole chunk of 64 skipped between kept chunks
    for keep in ([1] * n, [i % 2 for i in range(n)], [(i + 1) % 2 for i in range(n)], block, [1 if i == 77 else 0 for i in range(n)]):
        same(form, rows, keep=keep, framed=True)
        same(form, rows, keep=keep)
    assert encode(form, rows, keep=[0] * n, framed=True) == (b"", [0] * n)
    # all zeros through the raw ABI: length 0 and no store to d_out
    rounds, sigs, sl, prevs, pl = sc.columns(rows, 132, 96)
    keep0 = torch.zeros(n, dtype=torch.uint8, device="cuda")
    buf = torch.full((256,), 0xA5, dtype=torch.uint8, device="cuda")
    total = ctypes.c_size_t(9)
    torch.cuda.synchronize()
    rc = _lib.load().dh_rand_encode_device(form, rounds.data_ptr(), sigs.data_ptr(), 132, sl.data_ptr(), prevs.data_ptr(), 96, pl.data_ptr(), None,
                                           keep0.data_ptr(), n, None, 0, 0, buf.data_ptr() + 1, 200, None, ctypes.byref(total), None)
    assert rc == 0 and total.value == 0 and bytes(buf.cpu().numpy()) == b"\xa5" * 256
    # a skipped row with an over-long length does not refuse the call; kept, it does
    sl2, keep1 = sl.clone(), torch.ones(n, dtype=torch.uint8, device="cuda")
    sl2[70], keep1[70] = 5000, 0
    enc = unframed(form)
    out, lens = enc(rounds, sigs, sl2, prevs, pl, keep=keep1)
    exp = want(form, rows, keep=[0 if i == 70 else 1 for i in range(n)])
    assert (bytes(out.cpu().numpy()), lens.tolist()) == exp
    with pytest.raises(ValueError, match="row 70"):
        enc(rounds, sigs, sl2, prevs, pl)
    # the verifier's verdict column for the corrupted golden chain: the output holds exactly the valid rounds
    for name in ("pedersen-bls-chained", "bls-unchained-on-g1"):
        s, pk = scheme_from_name(name), bytes.fromhex(gold_ar["chains"][name]["pk"])
        recs = sc.corrupted_chain(name, gold_ar)
        rounds, sigs, sl, prevs, pl = sc.columns(recs, s.sig_len, 96, s.chained)
        verdict, rand = verify_device(s, pk, rounds, sigs, prevs, pl)
        valid = [0 if i in sc.CORRUPTED else 1 for i in range(len(recs))]
        assert verdict.tolist() == valid
        out, lens = enc(rounds, sigs, sl, prevs, pl, rands=rand, keep=verdict)
        assert (bytes(out.cpu().numpy()), lens.tolist()) == want(form, recs, want_prev=s.chained, keep=valid)


def test_flags_and_metadata(dh):
    rows = sc.shaped_rows(70, 4)
    for framed in (False, True):
        same(JSON, rows, framed=framed)
        for md in (None, {}, META, pc.FULL_META):  # absent, empty (2A 00), the ID only, everything
            same(PB, rows, framed=framed, metadata=md)
    # the marshalled bytes are taken as they are
    from drand_amd import store
    rounds, sigs, sl, prevs, pl = sc.columns(rows, 132, 96)
    a, _ = store.encode_public_rand(rounds, sigs, sl, prevs, pl, metadata=store.metadata_bytes(pc.FULL_META))
    assert bytes(a.cpu().numpy()) == sc.want_pb(rows, metadata=pc.FULL_META)[0]


@pytest.mark.parametrize("form", FORMS)
def test_output_placement_sizing_and_cap(dh, form):
    import torch
    from drand_amd import _lib
    lib = _lib.load()
    rows = sc.shaped_rows(130, 6)
    exp, exp_lens = want(form, rows, framed=True)
    rounds, sigs, sl, prevs, pl = sc.columns(rows, 132, 96)
    total, lens = ctypes.c_size_t(0), torch.zeros(len(rows), dtype=torch.int32, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731

    def call(out, cap, n=len(rows)):
        torch.cuda.synchronize()
        return lib.dh_rand_encode_device(form, p(rounds), p(sigs), 132, p(sl), p(prevs), 96, p(pl), None, None, n, None, 0, form, out, cap, p(lens),
                                         ctypes.byref(total), None)
    assert call(None, 0) == _lib.DH_OK and total.value == len(exp) and lens.tolist() == exp_lens  # the sizing call
    for shift in range(4):
        buf = torch.full((len(exp) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        lens.zero_()
        assert call(buf.data_ptr() + 16 + shift, len(exp)) == _lib.DH_OK, _lib.last_error()
        got = bytes(buf.cpu().numpy())
        assert total.value == len(exp) and lens.tolist() == exp_lens
        assert got[16 + shift:16 + shift + len(exp)] == exp
        assert got[:16 + shift] == b"\xa5" * (16 + shift) and got[16 + shift + len(exp):] == b"\xa5" * (48 - shift)
    buf = torch.zeros(len(exp), dtype=torch.uint8, device="cuda")
    assert call(buf.data_ptr(), len(exp) - 1) == _lib.DH_EINVAL and total.value == len(exp)  # cap too small: the size is still given
    assert not buf.any()
    assert call(buf.data_ptr(), len(exp), n=0) == _lib.DH_OK and total.value == 0


def test_in_place_path_and_device_refusals(dh):
    # 64 rows with 400-byte signatures: 64 JSON records of 900 bytes pass 36 KiB and are written row by row, beside staged
    # chunks; the protobuf chunk of the same rows is staged, one of 1000-byte signatures is not
    wide = [{"round": 1 + i, "signature": pc.rand_bytes("wide %d" % i, 400), "previous_signature": b""} for i in range(64)]
    rows = sc.shaped_rows(70, 0) + wide + sc.shaped_rows(70, 1)
    given = [pc.rand_bytes("wide randomness %d" % i, 32) for i in range(len(rows))]
    for form in FORMS:
        same(form, rows, sig_stride=400, framed=True)
        same(form, rows, sig_stride=400, rands=given, keep=[i % 3 != 0 for i in range(len(rows))])
    wider = [{"round": 1 + i, "signature": pc.rand_bytes("wider %d" % i, 1000 + i % 7), "previous_signature": pc.rand_bytes("p %d" % i, 96)}
             for i in range(64)]
    for form in FORMS:
        same(form, wider + sc.shaped_rows(5, 0), sig_stride=1008, framed=True, **({"metadata": META} if form == PB else {}))
    # a 2,100-byte signature: its JSON record exceeds 4096 bytes and the error names the row; protobuf takes it
    big = sc.shaped_rows(70, 0)
    big[66] = dict(big[66], signature=b"\x11" * 2100)
    with pytest.raises(ValueError, match="row 66"):
        encode(JSON, big, sig_stride=2100)
    same(PB, big, sig_stride=2100, framed=True)
    big[66] = dict(big[66], signature=b"\x11" * 1900)
    same(JSON, big, sig_stride=2100)
    big[3] = dict(big[3], signature=b"\x22" * 4000)  # 4000 + 96 + 34 + tags pass 4096 in protobuf form too
    with pytest.raises(ValueError, match="row 3"):
        encode(PB, big, sig_stride=4000)
    # a length above its stride
    import torch
    from drand_amd import store
    rounds, sigs, sl, prevs, pl = sc.columns(sc.shaped_rows(70, 0), 132, 96)
    pl2 = pl.clone()
    pl2[65] = 97
    for enc in (store.encode_random_data, store.encode_public_rand):
        with pytest.raises(ValueError, match="row 65"):
            enc(rounds, sigs, sl, prevs, pl2)
    torch.cuda.synchronize()


# ---- round trips

@pytest.mark.parametrize("name", ac.SCHEMES)
def test_round_trip_through_the_archive(dh, gold_ar, gold_pc, name):
    import torch
    from drand_amd import scheme_from_name, store
    s, pk = scheme_from_name(name), bytes.fromhex(gold_ar["chains"][name]["pk"])
    recs = ac.chain_records(name, gold_ar)
    rounds, sigs, sl, prevs, pl = sc.columns(recs, s.sig_len, 96, s.chained)
    want_rand = to_dev([r["randomness"] for r in recs])
    mask = lambda rows_, ln: rows_ * (torch.arange(rows_.shape[1], device="cuda")[None, :] < ln[:, None])  # noqa: E731

    def same_columns(ar):
        assert len(ar) == len(recs) and ar.stat()["deferred"] == 0 and ar.deferred() == []
        g = ar.beacons_device(sig_stride=s.sig_len, prev_stride=96)
        assert torch.equal(g[0], rounds) and torch.equal(g[1], mask(sigs, sl)) and torch.equal(g[2], sl) and not g[7].any()
        if s.chained:
            assert torch.equal(g[3], mask(prevs, pl)) and torch.equal(g[4], pl)
        else:
            assert not g[4].any()
        assert torch.equal(g[5], want_rand) and g[6].tolist() == [32] * len(recs)

    out, lens = store.encode_random_data(rounds, sigs, sl, prevs, pl)
    with store.DeviceArchive(bytes(out.cpu().numpy())) as ar:
        same_columns(ar)
        status = [int(x) for x in ar.check(s, pk, anchor=ac.anchor(name))]
        assert status == gold_ar["status"][name]["clean"] and not any(x & store.AR_RANDOMNESS for x in status)
    for delim in (False, True):
        out, lens = store.encode_public_rand(rounds, sigs, sl, prevs, pl, metadata=META, delimited=delim)
        data = bytes(out.cpu().numpy())
        with (store.DeviceArchive.from_packets(pc.PR, data) if delim else store.DeviceArchive.from_packets(pc.PR, data, lens=lens.cpu().numpy())) as ar:
            assert ar.unframed == b""
            same_columns(ar)
            status = bytes(ar.check(s, pk, anchor=ac.anchor(name), beacon_id=pc.BEACON_ID))
            assert status.hex() == gold_pc["status"][name]["public_rand"]["clean"] and not any(x & store.AR_RANDOMNESS for x in status)


def chain_store(path, name, recs):
    """The anchor as round 0, then the records' signatures, as a trimmed store file; (rounds, sigs) written."""
    from drand_amd.store import write_trimmed_bolt
    rounds = np.array([ac.FIRST - 1] + [r["round"] for r in recs], np.uint64)
    sigs = np.array([np.frombuffer(ac.anchor_sig(name), np.uint8)] + [np.frombuffer(r["signature"], np.uint8) for r in recs], np.uint8)
    write_trimmed_bolt(path, rounds, sigs)
    return rounds, sigs


@pytest.mark.parametrize("name", ac.SCHEMES)
def test_store_to_records_to_store(dh, gold_ar, name, tmp_path):
    from drand_amd import scheme_from_name, store
    s, pk = scheme_from_name(name), bytes.fromhex(gold_ar["chains"][name]["pk"])
    recs = ac.chain_records(name, gold_ar)
    src, got, want_db, arch = (str(tmp_path / f) for f in ("src.db", "got.db", "want.db", "chain.ndjson"))
    all_rounds, all_sigs = chain_store(src, name, recs)
    store.write_trimmed_bolt(want_db, all_rounds[1:], all_sigs[1:])  # the file the checked records make: the chain without its anchor
    want_file = open(want_db, "rb").read()
    shown = [dict(r, previous_signature=r["previous_signature"] if s.chained else b"") for r in recs]
    lines = sc.want_json(shown, newline=True)[0]
    for window in (64, 1 << 20):
        with store.DeviceBoltStore(src, s.chained) as st:
            res = store.export_random_data(st, arch, window=window)
            assert res == {"records": len(recs), "bytes": len(lines), "faulty": []}
            assert open(arch, "rb").read() == lines
            assert store.export_random_data(st, arch, s, pk, window=window) == res  # checked first: nothing faulty
            store.archive_to_trimmed_store(arch, got, s, pk, anchor=ac.anchor(name), window=window)
            assert open(got, "rb").read() == want_file
            frames = list(store.public_rand_frames(st, ac.FIRST, metadata=META, window=window, delimited=True))
            assert len(frames) == (5 if window == 64 else 1)
            data = b"".join(bytes(f.cpu().numpy()) for f, _l in frames)
            assert data == sc.want_pb(shown, delimited=True, metadata=META)[0]
            with store.DeviceArchive.from_packets(pc.PR, data) as ar:
                assert ar.stat()["deferred"] == 0
                store.archive_to_trimmed_store(ar, got, s, pk, anchor=ac.anchor(name), window=window)
            assert open(got, "rb").read() == want_file
            # the refactor's guard: SyncChain's frames are what they were, packet_bytes of every stored round
            sync = b"".join(bytes(f.cpu().numpy()) for f, _l in store.sync_chain_frames(st, ac.FIRST, pc.BEACON_ID, window=window, delimited=True))
            assert sync == store.delimited([store.packet_bytes(pc.BP, dict(r, randomness=b""), pc.BEACON_ID) for r in shown])
            plain = [bytes(f.cpu().numpy()) for f, _l in store.random_data_frames(st, 100, window=window, skip=(150, 163, 164), newline=False)]
            keep = [0 if r["round"] in (150, 163, 164) else 1 for r in shown[99:]]
            assert b"".join(plain) == sc.want_json(shown[99:], keep=keep, newline=False)[0]


def test_reference_store_fixtures_export_without_a_key(dh, tmp_path):
    from drand_amd import store
    arch = str(tmp_path / "ref.ndjson")
    for path, fmt, host in ((jc.REF_TRIMMED, "trimmed", store.BoltTrimmedStore(jc.REF_TRIMMED, True)),
                            (jc.REF_UNTRIMMED, "untrimmed", store.BoltUntrimmedStore(jc.REF_UNTRIMMED, True))):
        rounds = [r for r in host.rounds() if r >= 1]
        beacons = [host.get(r) for r in rounds]
        rows = [{"round": b.round, "signature": b.signature, "previous_signature": b.previous_signature} for b in beacons]
        assert len(rows) in (45, 26) and len(rows[0]["previous_signature"]) == 32
        with store.DeviceBoltStore(path, True, fmt=fmt) as st:
            for window in (7, 1 << 20):
                res = store.export_random_data(st, arch, window=window)
                assert open(arch, "rb").read() == sc.want_json(rows, newline=True)[0] and res["records"] == len(rows)
            res = store.export_random_data(st, arch, up_to=9)
            assert open(arch, "rb").read() == sc.want_json(rows[:9], newline=True)[0] and res["records"] == 9
            frames = b"".join(bytes(f.cpu().numpy()) for f, _l in store.public_rand_frames(st, 1, metadata=pc.FULL_META, window=7))
            assert frames == sc.want_pb(rows, metadata=pc.FULL_META)[0]


@pytest.mark.parametrize("name", ["pedersen-bls-chained", "bls-unchained-g1-rfc9380"])
def test_faulty_rounds_stay_out_of_the_archive_and_the_bucket(dh, gold_ar, name, tmp_path):
    from drand_amd import scheme_from_name, store
    from drand_amd.client import relay_s3_sync_store
    s, pk = scheme_from_name(name), bytes.fromhex(gold_ar["chains"][name]["pk"])
    recs = sc.corrupted_chain(name, gold_ar)
    src, arch = str(tmp_path / "src.db"), str(tmp_path / "chain.ndjson")
    chain_store(src, name, recs)
    # the store shows each round with the signature stored before it: a corrupted round spoils the next one of a chained chain
    shown = [dict(r, previous_signature=(recs[i - 1]["signature"] if i else ac.anchor_sig(name)) if s.chained else b"") for i, r in enumerate(recs)]
    bad = sorted(set(ac.FIRST + i for i in sc.CORRUPTED) | set(ac.FIRST + i + 1 for i in sc.CORRUPTED if s.chained and i + 1 < len(recs)))
    keep = [0 if r["round"] in bad else 1 for r in shown]
    with store.DeviceBoltStore(src, s.chained) as st:
        res = store.export_random_data(st, arch, s, pk, window=64)
        lines = sc.want_json(shown, keep=keep, newline=True)[0]
        assert res == {"records": sum(keep), "bytes": len(lines), "faulty": bad} and open(arch, "rb").read() == lines
        bucket, log = {}, []

        def upload(key, body):
            if key == "public/120":
                raise IOError("no such bucket")
            bucket[key] = body

        begin, end = 5, 250
        done = relay_s3_sync_store(st, s, pk, upload, begin, end, window=64, log=lambda *a: log.append(a))
        ok = [r for r in shown if begin <= r["round"] <= end and r["round"] not in bad and r["round"] != 120]
        assert done == [r["round"] for r in ok]
        assert bucket == {"public/%d" % r["round"]: sc.want_json([r], newline=False)[0] for r in ok}  # the hexjson object, not base64
        assert len(log) == len([r for r in bad if begin <= r <= end]) + 1
        assert relay_s3_sync_store(st, s, pk, upload, 400, 500) == []


# ---- calls

def test_identical_calls_threads_and_shutdown(dh):
    from drand_amd import _lib, store
    rows = sc.shaped_rows(256, 7)
    cols = sc.columns(rows, 132, 96)
    for form in FORMS:
        assert encode(form, rows, framed=True) == encode(form, rows, framed=True) == want(form, rows, framed=True)
    got, errs = {}, []

    def run(k):  # four threads encode disjoint windows of the same columns concurrently
        try:
            a, b = 64 * k, 64 * k + 64
            part = [c[a:b] for c in cols]
            for _ in range(3):
                j, _l = store.encode_random_data(*part)
                p, _l = store.encode_public_rand(*part, metadata=META, delimited=True)
                got[k] = (bytes(j.cpu().numpy()), bytes(p.cpu().numpy()))
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ths = [threading.Thread(target=run, args=(k,)) for k in range(4)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not errs, errs
    for k in range(4):
        part = rows[64 * k:64 * k + 64]
        assert got[k] == (sc.want_json(part)[0], sc.want_pb(part, delimited=True, metadata=META)[0])
    # after dh_shutdown the call re-initialises the library, as dh_pb_encode_device does
    lib = _lib.load()
    lib.dh_shutdown()
    try:
        assert encode(JSON, rows[:70], framed=True) == want(JSON, rows[:70], framed=True)
    finally:
        assert lib.dh_init(0) == 0, _lib.last_error()
    assert encode(PB, rows[:70]) == want(PB, rows[:70])
