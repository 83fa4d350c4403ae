"""GPU: trimmed bbolt store files written from device columns (dh_bolt_write_trimmed_device, dh_store_save_trimmed,
store.write_trimmed_bolt, DeviceBoltStore.save_trimmed, sync.correct_store_file).

* the primitive over the case list of tests/bolt_write_cases.py: bytes equal boltwrite2.write_bolt2, the image reopens
  with dh_store_open_bolt with the expected dh_store_stat, BoltTrimmedStore reads the same records back;
* the reference's two Go-written fixtures, converted / saved: the same records as the host readers give;
* conversion of 300-round signed untrimmed stores (chained and quicknet) carrying a corrupted signature, a wrong stored
  PreviousSig, a short signature and two missing rounds: bytes equal write_bolt2 over the decoded signatures, the device
  and the host replay of the converted file agree, the unchained faulty set equals the source's, and the unlinked list
  is the one the definition gives (computed here from the host reader's records). For the chained store that list is
  [21, 40, 61, 81, 151]: the wrong-PreviousSig round and the rounds after each gap, AND the successors of the corrupted
  and of the short record, whose stored (true) PreviousSig is not what the file holds for the round before them;
* patches: replace, insert (inside, before the first and after the last record), delete; invalid lists are DH_EINVAL;
* deferred records: DH_DEFERRED with nothing written until a patch covers them; the Python layer resolves them;
* refusals with canary buffers; correct_store_file; two threads on two handles."""
import ctypes
import os
import threading

import numpy as np
import pytest

import bolt_cases as bc
import bolt_json_cases as jc
import bolt_write_cases as wc
from boltwrite2 import write_bolt2

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
CHAINED, QUICKNET = "pedersen-bls-chained", "bls-unchained-g1-rfc9380"
CORRUPT, WRONG_PREV, SHORT, MISSING, MISSING2, N_ROUNDS = 20, 40, 60, 80, 150, 300


@pytest.fixture(scope="module")
def dh():
    import torch
    import drand_amd
    from drand_amd import _lib
    torch.zeros(1, device="cuda")
    assert _lib.load().dh_init(0) == 0, _lib.last_error()
    return drand_amd


def columns(kv):
    """{round: value} -> (rounds u64[n], rows u8[n, stride], lens u32[n]) with stride = the longest value rounded up to 4."""
    keys = sorted(kv)
    stride = max(4, (max(len(v) for v in kv.values()) + 3) & ~3)
    rows = np.zeros((len(keys), stride), np.uint8)
    for i, r in enumerate(keys):
        rows[i, :len(kv[r])] = np.frombuffer(kv[r], np.uint8)
    return np.array(keys, np.uint64), rows, np.array([len(kv[r]) for r in keys], np.uint32)


def raw_write(rounds, rows, lens, P, cap=None, canary=0):
    """dh_bolt_write_trimmed_device on uploaded columns: (rc, len_out, image buffer incl. `canary` bytes of 0xC3, stats)."""
    import torch
    from drand_amd import _lib
    lib = _lib.load()
    d_r = torch.from_numpy(rounds.view(np.int64)).cuda()
    d_s = torch.from_numpy(rows).cuda()
    d_l = torch.from_numpy(lens.view(np.int32)).cuda()
    torch.cuda.synchronize()
    size, stats = ctypes.c_size_t(0), (ctypes.c_uint64 * 3)()
    if cap is None:
        rc = lib.dh_bolt_write_trimmed_device(d_r.data_ptr(), d_s.data_ptr(), rows.shape[1], d_l.data_ptr(), len(rounds), P, None, 0,
                                              ctypes.byref(size), stats, None)
        assert rc == _lib.DH_EINVAL and size.value, _lib.last_error()
        cap = size.value
    buf = np.full(cap + canary, 0xC3, np.uint8)
    rc = lib.dh_bolt_write_trimmed_device(d_r.data_ptr() or None, d_s.data_ptr() or None, rows.shape[1], d_l.data_ptr() or None,
                                          len(rounds), P, ctypes.c_void_p(buf.ctypes.data), cap, ctypes.byref(size), stats, None)
    return rc, size.value, buf, [int(x) for x in stats]


def want_bytes(tmp, kv, P=4096, name="want"):
    path = str(tmp / (name + ".db"))
    lay = write_bolt2(path, [(bc.key(r), v) for r, v in kv.items()], page_size=P)
    return open(path, "rb").read(), lay


def trimmed_records(path):
    from drand_amd.store import BoltFile
    return {int.from_bytes(k, "big"): v for k, v in BoltFile(path).bucket(b"beacons").items() if len(k) == 8}


# ------------------------------------------------------------------ the primitive, byte-exact

@pytest.mark.parametrize("case", wc.cases(), ids=lambda c: c[0])
def test_primitive_equals_write_bolt2(dh, tmp_path, case):
    from drand_amd import _lib
    from drand_amd.store import BoltTrimmedStore
    name, P, kv = case
    want, lay = wc.expected(tmp_path, name, P, kv)
    rounds, rows, lens = columns(kv)
    rc, size, buf, stats = raw_write(rounds, rows, lens, P, canary=64)
    assert rc == 0, _lib.last_error()
    assert size == len(want) and stats == [len(kv), len(lay["leaves"]), lay["pages"]]
    assert buf[:size].tobytes() == want
    assert (buf[size:] == 0xC3).all()
    assert lay["depth"] == wc.DEPTHS.get(name, lay["depth"])
    # the image reopens on the device and through the host reader
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.dh_store_open_bolt(ctypes.c_void_p(buf.ctypes.data), size, ctypes.byref(h)) == 0, _lib.last_error()
    st = (ctypes.c_uint64 * 6)()
    assert lib.dh_store_stat(h, st) == 0
    lib.dh_store_close(h)
    assert [int(x) for x in st] == [len(kv), len(kv), min(kv), max(kv), max(len(v) for v in kv.values()), len(lay["leaves"])]
    path = tmp_path / "img.db"
    path.write_bytes(buf[:size].tobytes())
    host = BoltTrimmedStore(str(path), False)
    assert host.rounds() == sorted(kv) and all(host.get(r).signature == kv[r] for r in kv)


def test_write_trimmed_bolt_python(dh, tmp_path):
    import torch
    from drand_amd.store import write_trimmed_bolt
    kv = wc.recs(range(1, 200), 48, "py")
    want, lay = want_bytes(tmp_path, kv, 4096)
    rounds, rows, lens = columns(kv)
    out = str(tmp_path / "np.db")
    assert write_trimmed_bolt(out, rounds, rows) == {"rows": 199, "leaves": len(lay["leaves"]), "pages": lay["pages"]}
    assert open(out, "rb").read() == want and not os.path.exists(out + ".tmp")
    # device tensors, with lens, a stride wider than the values and another page size
    kv[7] = kv[7][:31]
    want, _lay = want_bytes(tmp_path, kv, 512, "want512")
    rounds, rows, lens = columns(kv)
    wide = np.zeros((len(rounds), 64), np.uint8)
    wide[:, :48] = rows
    t = [torch.from_numpy(a).cuda() for a in (rounds.view(np.int64), wide, lens.view(np.int32))]
    write_trimmed_bolt(out, t[0], t[1], t[2], page_size=512)
    assert open(out, "rb").read() == want


# ------------------------------------------------------------------ the reference's fixtures

def test_reference_fixtures(dh, tmp_path):
    from drand_amd.store import BoltTrimmedStore, BoltUntrimmedStore, DeviceBoltStore
    src = BoltUntrimmedStore(jc.REF_UNTRIMMED, True)
    out = str(tmp_path / "conv.db")
    with DeviceBoltStore(jc.REF_UNTRIMMED, True, fmt="untrimmed") as dev:
        res = dev.save_trimmed(out)
    got = trimmed_records(out)
    assert sorted(got) == src.rounds() == list(range(27))
    for r in src.rounds():
        assert got[r] == src.get(r).signature, r
    assert len(got[0]) == 32 and all(len(got[r]) == 96 for r in range(1, 27))
    assert res["rows"] == 27 and res["unlinked"] == [] and res["undecodable"] == []
    conv = BoltTrimmedStore(out, True)
    for r in range(1, 27):  # the rebuilt previous signature is the one the record stored
        assert conv.get(r).previous_signature == src.get(r).previous_signature
    wc.check_image(open(out, "rb").read())
    with DeviceBoltStore(jc.REF_TRIMMED, True) as dev:
        res = dev.save_trimmed(out)
    assert trimmed_records(out) == trimmed_records(jc.REF_TRIMMED) and res["rows"] == 46 and res["unlinked"] == []
    wc.check_image(open(out, "rb").read())


# ------------------------------------------------------------------ conversion of signed stores

def signed_store(name, oracle):
    """(pk, true signatures {round: bytes}, {key: hexjson value}): bolt_json_cases.replay_kv without its deferred records."""
    import hashlib
    chained = name == CHAINED
    sk = hashlib.sha256(b"bolt write " + name.encode()).digest()
    sk = (int.from_bytes(sk, "big") % 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001).to_bytes(32, "big")
    pk = oracle.public_key(name, sk)
    sigs = {0: hashlib.sha256(b"genesis " + name.encode()).digest()}
    for r in range(1, N_ROUNDS + 1):
        sigs[r] = oracle.sign(name, sk, oracle.digest_beacon(name, r, sigs[r - 1] if chained else b""))
    kv = {bc.key(0): jc.marshal(0, sigs[0], None)}
    for r in range(1, N_ROUNDS + 1):
        kv[bc.key(r)] = jc.marshal(r, sigs[r], sigs[r - 1] if chained else None)
    bad = bytearray(sigs[CORRUPT])
    bad[20] ^= 1
    kv[bc.key(CORRUPT)] = jc.marshal(CORRUPT, bad, sigs[CORRUPT - 1] if chained else None)
    kv[bc.key(WRONG_PREV)] = jc.marshal(WRONG_PREV, sigs[WRONG_PREV], bc.rand_bytes("wrong prev", 96))
    kv[bc.key(SHORT)] = jc.marshal(SHORT, sigs[SHORT][:-2], sigs[SHORT - 1] if chained else None)
    del kv[bc.key(MISSING)]
    del kv[bc.key(MISSING2)]
    return pk, sigs, kv


@pytest.fixture(scope="module")
def signed(oracle, tmp_path_factory):
    """{scheme: (pk, true sigs, untrimmed path, decoded {round: (signature, previous)})}, computed once and not changed."""
    from drand_amd.store import beacon_from_hexjson
    tmp = tmp_path_factory.mktemp("signed")
    out = {}
    for name in (CHAINED, QUICKNET):
        pk, sigs, kv = signed_store(name, oracle)
        path = str(tmp / (name + ".db"))
        write_bolt2(path, list(kv.items()), page_size=4096)
        dec = {}
        for k, v in kv.items():
            b = beacon_from_hexjson(v)
            dec[int.from_bytes(k, "big")] = (b.signature, b.previous_signature)
        out[name] = (pk, sigs, path, dec)
    return out


def unlinked_by_definition(dec):
    """Rounds whose stored PreviousSig has nonzero length and is not the value the output holds for round - 1."""
    return [r for r in sorted(dec) if dec[r][1] and (r - 1 not in dec or dec[r - 1][0] != dec[r][1])]


@pytest.mark.parametrize("name", [CHAINED, QUICKNET])
def test_conversion_of_signed_stores(dh, oracle, signed, tmp_path, name):
    from drand_amd.store import BoltTrimmedStore, DeviceBoltStore
    from drand_amd.sync import check_past_beacons
    from test_readers import OracleScheme
    pk, _sigs, src, dec = signed[name]
    s = dh.scheme_from_name(name)
    out = str(tmp_path / "conv.db")
    UP_TO = 160  # past every defect; the host replay below verifies each round on the CPU
    with DeviceBoltStore(src, s.chained, fmt="auto") as dev:
        assert dev.untrimmed
        faulty_src = dev.check_past(s, pk, UP_TO)
        res = dev.save_trimmed(out)
    want, lay = want_bytes(tmp_path, {r: v[0] for r, v in dec.items()})
    assert open(out, "rb").read() == want
    assert (res["rows"], res["leaves"], res["pages"]) == (len(dec), len(lay["leaves"]), lay["pages"])
    assert res["undecodable"] == [] and res["replaced_or_deleted"] == 0 and res["inserted"] == 0
    # the unlinked list
    assert res["unlinked"] == unlinked_by_definition(dec)
    if s.chained:
        assert res["unlinked"] == [CORRUPT + 1, WRONG_PREV, SHORT + 1, MISSING + 1, MISSING2 + 1]
    else:
        assert res["unlinked"] == [WRONG_PREV]  # the only record of this store that carries a PreviousSig
    # the converted file replays alike on the device and on the host
    with DeviceBoltStore(out, s.chained) as conv:
        faulty_dev = check_past_beacons(conv, s, pk, UP_TO)
    faulty_host = check_past_beacons(BoltTrimmedStore(out, s.chained), OracleScheme(oracle, name), pk, UP_TO)
    assert faulty_dev == faulty_host
    if s.chained:  # a faulty or missing record now also fails its successor; the wrong PreviousSig is gone
        assert faulty_src == [CORRUPT, WRONG_PREV, SHORT, MISSING, MISSING2]
        assert faulty_dev == [CORRUPT, CORRUPT + 1, SHORT, SHORT + 1, MISSING, MISSING + 1, MISSING2, MISSING2 + 1]
    else:
        assert faulty_dev == faulty_src == [CORRUPT, SHORT, MISSING, MISSING2]


# ------------------------------------------------------------------ patches

def raw_save(dev, patches, first=0, last=U64, P=4096, cap=1 << 20, ucap=64):
    """dh_store_save_trimmed with a patch list [(round, bytes | None)] passed in the order given:
    (rc, len_out, image buffer with 64 canary bytes, unlinked, stats)."""
    from drand_amd import _lib
    lib = _lib.load()
    k = len(patches)
    stride = max([4] + [len(v) for _r, v in patches if v is not None])
    pr = np.array([r for r, _v in patches], np.uint64).reshape(-1)
    pl = np.array([_lib.DH_PATCH_DELETE if v is None else len(v) for _r, v in patches], np.uint32).reshape(-1)
    ps = np.zeros((k, stride), np.uint8)
    for i, (_r, v) in enumerate(patches):
        if v:
            ps[i, :len(v)] = np.frombuffer(v, np.uint8)
    buf = np.full(cap + 64, 0xC3, np.uint8)
    unl = np.zeros(max(1, ucap), np.uint64)
    n, nu, stats = ctypes.c_size_t(7), ctypes.c_size_t(0), (ctypes.c_uint64 * 6)()
    rc = lib.dh_store_save_trimmed(dev._h, first, last, ctypes.c_void_p(pr.ctypes.data), ctypes.c_void_p(ps.ctypes.data), stride,
                                   ctypes.c_void_p(pl.ctypes.data), k, P, ctypes.c_void_p(buf.ctypes.data), cap, ctypes.byref(n),
                                   ctypes.c_void_p(unl.ctypes.data), ucap, ctypes.byref(nu), stats)
    return rc, n.value, buf, [int(x) for x in unl[:min(nu.value, ucap)]], [int(x) for x in stats]


@pytest.mark.parametrize("fmt", ["trimmed", "untrimmed"])
def test_patches(dh, tmp_path, fmt):
    from drand_amd import _lib
    from drand_amd.store import DeviceBoltStore
    base = wc.recs([r for r in range(10, 30) if r != 20], 96, "patch")
    src = str(tmp_path / "src.db")
    if fmt == "trimmed":
        write_bolt2(src, [(bc.key(r), v) for r, v in base.items()], page_size=512)
    else:
        write_bolt2(src, [(bc.key(r), jc.marshal(r, v, None)) for r, v in base.items()], page_size=512)
    new = {r: bc.rand_bytes("new%d" % r, n) for r, n in ((2, 96), (12, 96), (20, 100), (40, 48))}
    patches = {2: new[2], 12: new[12], 15: None, 20: new[20], 40: new[40], 41: None}
    edited = dict(base)
    del edited[15]
    edited.update(new)
    out = str(tmp_path / "out.db")
    with DeviceBoltStore(src, False, fmt=fmt) as dev:
        for P in (512, 4096):
            res = dev.save_trimmed(out, patches=patches, page_size=P)
            want, _lay = want_bytes(tmp_path, edited, P)
            assert open(out, "rb").read() == want
            assert (res["rows"], res["replaced_or_deleted"], res["inserted"]) == (len(edited), 2, 3) and res["unlinked"] == []
        # a window: records and patches inside it only
        res = dev.save_trimmed(out, first=12, last=25, patches={12: new[12], 20: new[20]}, page_size=512)
        sub = {r: v for r, v in base.items() if 12 <= r <= 25}
        sub.update({12: new[12], 20: new[20]})
        assert open(out, "rb").read() == want_bytes(tmp_path, sub, 512)[0]
        # deleting everything leaves nothing to write
        with pytest.raises(KeyError):
            dev.save_trimmed(out, first=10, last=11, patches={10: None, 11: None})
        # invalid lists: unsorted, duplicate, outside [first, last]; nothing is written
        for bad, first, last in (([(12, new[12]), (2, new[2])], 0, U64), ([(12, new[12]), (12, new[12])], 0, U64),
                                 ([(40, new[40])], 0, 39), ([(2, new[2])], 3, U64)):
            rc, n, buf, _u, _s = raw_save(dev, bad, first, last)
            assert rc == _lib.DH_EINVAL and n == 0 and (buf == 0xC3).all(), (bad, _lib.last_error())
        rc, n, buf, _u, stats = raw_save(dev, sorted(patches.items()), P=512)
        assert rc == 0 and buf[:n].tobytes() == want_bytes(tmp_path, edited, 512)[0] and (buf[n:] == 0xC3).all()
        assert stats[0] == len(edited) and stats[3:] == [0, 2, 3]


def test_patches_repair_a_signed_store(dh, signed, tmp_path):
    from drand_amd.store import DeviceBoltStore
    pk, sigs, src, dec = signed[CHAINED]
    s = dh.scheme_from_name(CHAINED)
    out = str(tmp_path / "fixed.db")
    fix = {CORRUPT: sigs[CORRUPT], SHORT: sigs[SHORT], MISSING: sigs[MISSING], MISSING2: sigs[MISSING2]}
    with DeviceBoltStore(src, True, fmt="untrimmed") as dev:
        res = dev.save_trimmed(out, patches=fix)
    assert open(out, "rb").read() == want_bytes(tmp_path, {r: sigs[r] for r in range(N_ROUNDS + 1)})[0]
    assert res["replaced_or_deleted"] == 2 and res["inserted"] == 2 and res["unlinked"] == [WRONG_PREV]
    with DeviceBoltStore(out, True) as conv:
        assert conv.check_past(s, pk, 1000) == []


# ------------------------------------------------------------------ deferred records

def test_deferred_records(dh, oracle, tmp_path):
    from drand_amd import _lib
    from drand_amd.store import DeviceBoltStore
    kv = jc.synth(40, 96, True, "defer")
    what, make = jc.DEFERRED_VALUES[0]
    kv[bc.key(9)] = make(9)
    src = str(tmp_path / "one.db")
    write_bolt2(src, list(kv.items()), page_size=1024)
    fill = bc.rand_bytes("fill", 96)
    with DeviceBoltStore(src, True, fmt="untrimmed") as dev:
        assert dev.deferred() == [9]
        rc, n, buf, _u, _s = raw_save(dev, [])
        assert rc == _lib.DH_DEFERRED and n == 0 and (buf == 0xC3).all()
        rc, n, buf, _u, _s = raw_save(dev, [(8, fill)])  # a patch elsewhere does not cover it
        assert rc == _lib.DH_DEFERRED and n == 0 and (buf == 0xC3).all()
        rc, n, buf, _u, _s = raw_save(dev, [], first=10)  # outside the range it does not matter
        assert rc == 0 and n > 0
        rc, n, buf, unl, stats = raw_save(dev, [(9, fill)], P=1024)
        assert rc == 0, _lib.last_error()
        from drand_amd.store import beacon_from_hexjson
        dec = {int.from_bytes(k, "big"): beacon_from_hexjson(v).signature for k, v in kv.items() if k != bc.key(9)}
        dec[9] = fill
        assert buf[:n].tobytes() == want_bytes(tmp_path, dec, 1024)[0]
        assert unl == [10] and stats[3:] == [1, 1, 0]  # round 10 stored the signature the deferred record does not hold
        rc, n, buf, unl, stats = raw_save(dev, [(9, None)], P=1024)
        del dec[9]
        assert rc == 0 and buf[:n].tobytes() == want_bytes(tmp_path, dec, 1024)[0] and unl == [10]
    # the Python layer decodes what it can and reports what it cannot
    name = QUICKNET
    _pk, rkv, deferred = jc.replay_kv(name, oracle)
    src = str(tmp_path / "replay.db")
    write_bolt2(src, list(rkv.items()), page_size=4096)
    out = str(tmp_path / "replay_out.db")
    with DeviceBoltStore(src, False, fmt="untrimmed") as dev:
        assert dev.deferred() == sorted(deferred)
        res = dev.save_trimmed(out)
    want = {}
    for k, v in rkv.items():
        try:
            want[int.from_bytes(k, "big")] = beacon_from_hexjson(v).signature
        except ValueError:
            pass
    assert res["undecodable"] == [jc.UNDECODABLE] and jc.UNDECODABLE not in want and jc.ROUND_NE_KEY in want
    assert open(out, "rb").read() == want_bytes(tmp_path, want)[0]
    assert res["replaced_or_deleted"] == 2 and res["rows"] == len(want)


# ------------------------------------------------------------------ refusals

def test_refusals(dh, tmp_path):
    from drand_amd import _lib
    from drand_amd.store import DeviceBoltStore, write_trimmed_bolt
    kv = wc.recs(range(1, 60), 96, "ref")
    rounds, rows, lens = columns(kv)
    want, _lay = want_bytes(tmp_path, kv, 4096)
    # one byte short: the size comes back and nothing is written
    rc, size, buf, _s = raw_write(rounds, rows, lens, 4096, cap=len(want) - 1, canary=16)
    assert rc == _lib.DH_EINVAL and size == len(want) and (buf == 0xC3).all()
    for P in (0, 128, 4095, 6144, 131072):
        rc, size, buf, _s = raw_write(rounds, rows, lens, P, cap=len(want))
        assert rc == _lib.DH_EINVAL and size == 0 and (buf == 0xC3).all(), P
    desc = rounds.copy()
    desc[10], desc[11] = rounds[11], rounds[10]
    dup = rounds.copy()
    dup[30] = dup[29]
    long_ = lens.copy()
    long_[58] = rows.shape[1] + 1
    for r, l in ((desc, lens), (dup, lens), (rounds, long_)):
        rc, size, buf, _s = raw_write(r, rows, l, 4096, cap=len(want))
        assert rc == _lib.DH_EINVAL and (buf == 0xC3).all(), _lib.last_error()
    rc, size, buf, _s = raw_write(rounds[:0], rows[:0], lens[:0], 4096, cap=len(want))
    assert rc == _lib.DH_ENOBEACON and size == 0 and (buf == 0xC3).all()
    with pytest.raises(ValueError):
        write_trimmed_bolt(str(tmp_path / "x.db"), desc, rows)
    assert not os.path.exists(str(tmp_path / "x.db")) and not os.path.exists(str(tmp_path / "x.db.tmp"))
    # the store's own file, by name and through a link
    src = str(tmp_path / "src.db")
    open(src, "wb").write(want)
    os.symlink(src, str(tmp_path / "link.db"))
    with DeviceBoltStore(src, False) as dev:
        for p in (src, str(tmp_path / "." / "src.db"), str(tmp_path / "link.db")):
            with pytest.raises(ValueError):
                dev.save_trimmed(p)
        assert open(src, "rb").read() == want
        with pytest.raises(ValueError):
            dev.save_trimmed(str(tmp_path / "y.db"), page_size=1000)
        # cap one byte short through the handle; too little room for the unlinked list is covered below
        rc, n, buf, _u, _s = raw_save(dev, [], cap=len(want) - 1)
        assert rc == _lib.DH_EINVAL and n == len(want) and (buf == 0xC3).all()
    # more unlinked rounds than room: the count and the size come back, nothing is written
    ukv = {bc.key(r): jc.marshal(r, bc.rand_bytes("u%d" % r, 96), bc.rand_bytes("p%d" % r, 96)) for r in range(1, 9)}
    usrc = str(tmp_path / "u.db")
    write_bolt2(usrc, list(ukv.items()))
    with DeviceBoltStore(usrc, True, fmt="untrimmed") as dev:
        from drand_amd import _lib as L
        lib = L.load()
        buf = np.full(1 << 16, 0xC3, np.uint8)
        unl = np.zeros(4, np.uint64)
        n, nu = ctypes.c_size_t(0), ctypes.c_size_t(0)
        rc = lib.dh_store_save_trimmed(dev._h, 0, U64, None, None, 0, None, 0, 4096, ctypes.c_void_p(buf.ctypes.data), buf.size,
                                       ctypes.byref(n), ctypes.c_void_p(unl.ctypes.data), 4, ctypes.byref(nu), None)
        assert rc == L.DH_EINVAL and nu.value == 8 and n.value == 5 * 4096 and (buf == 0xC3).all() and not unl.any()
        assert dev.save_trimmed(str(tmp_path / "u_out.db"))["unlinked"] == list(range(1, 9))


# ------------------------------------------------------------------ correct_store_file

def test_correct_store_file(dh, signed, tmp_path):
    from drand_amd.sync import correct_store_file
    pk, sigs, _src, _dec = signed[CHAINED]
    s = dh.scheme_from_name(CHAINED)
    a, b, c = 33, 111, 222
    stored = {r: sigs[r] for r in range(N_ROUNDS + 1)}
    for r in (a, b):
        x = bytearray(sigs[r])
        x[5] ^= 0x10
        stored[r] = bytes(x)
    del stored[c]
    src, dst = str(tmp_path / "src.db"), str(tmp_path / "dst.db")
    write_bolt2(src, [(bc.key(r), v) for r, v in stored.items()])
    asked = []

    def fetch(r):
        asked.append(r)
        return bc.rand_bytes("not a signature", 96) if r == b else sigs[r]

    before, after, unlinked = correct_store_file(src, dst, s, pk, fetch, fmt="auto")
    assert before == asked == [a, a + 1, b, b + 1, c, c + 1]
    assert after == [b, b + 1] and unlinked == []
    got = trimmed_records(dst)
    assert {r for r in set(got) | set(stored) if got.get(r) != stored.get(r)} == {a, c}
    assert got[a] == sigs[a] and got[c] == sigs[c] and got[b] == stored[b]
    assert open(src, "rb").read() == want_bytes(tmp_path, stored)[0]  # the source is not touched


# ------------------------------------------------------------------ threads

def test_two_threads_two_handles(dh, signed, tmp_path):
    from drand_amd.store import DeviceBoltStore
    jobs = []
    for name in (CHAINED, QUICKNET):
        _pk, _sigs, src, dec = signed[name]
        jobs.append((name, src, want_bytes(tmp_path, {r: v[0] for r, v in dec.items()}, 512, name)[0]))
    errs = []

    def work(name, src, want):
        try:
            out = str(tmp_path / (name + "_out.db"))
            with DeviceBoltStore(src, False, fmt="untrimmed") as dev:
                for _ in range(3):
                    dev.save_trimmed(out, page_size=512)
                    assert open(out, "rb").read() == want
        except Exception as e:  # noqa: BLE001 - reported below
            errs.append((name, repr(e)))

    ths = [threading.Thread(target=work, args=j) for j in jobs]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs, errs


# ------------------------------------------------------------------ dh_shutdown

def test_shutdown_invalidates_writer(dh, tmp_path):
    """dh_shutdown releases an open writer's device memory (closed leaves' keys, the open leaf's carried rows): its
    handle then only accepts close, and a new writer over the same rows gives the file."""
    from drand_amd import _lib
    from drand_amd.store import BoltWriter, write_trimmed_bolt
    lib = _lib.load()
    rounds, rows, lens = columns(wc.recs(range(1, 311), 48, "down"))
    more = [c[300:] for c in (rounds, rows, lens)]
    rounds, rows, lens = rounds[:300], rows[:300], lens[:300]
    out = str(tmp_path / "out.db")
    w = BoltWriter(out, 256)
    res = w.append(rounds, rows, lens)  # 72-byte records in 256-byte pages: many closed leaves and one open
    assert res["rows"] == 300 and res["leaves"] > 1
    lib.dh_shutdown()
    try:
        with pytest.raises(ValueError, match="dh_shutdown"):
            w.append(*more)
        w.close()
    finally:
        assert lib.dh_init(0) == 0, _lib.last_error()
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
    with BoltWriter(out, 256) as again:
        again.append(rounds, rows, lens)
        again.finish()
    want = str(tmp_path / "want.db")
    write_trimmed_bolt(want, rounds, rows, lens, page_size=256)
    assert open(out, "rb").read() == open(want, "rb").read()
