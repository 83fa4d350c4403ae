"""GPU: one chain from many unordered sources (dh_assemble_device, k_assemble.hip).

* the stable radix sort alone (dh_sort_rounds_debug) against numpy.argsort(kind="stable"), element for element: key counts
  around the wave, the tile and the hierarchical scan, key sets that skip seven passes, none, and that need unsigned order;
* the clean union of three incomplete sources equals the signed chain byte for byte, with every copy collapsed;
* the faulty pile against tests/golden/assemble_cases.json (assemble_host + the oracle): with an anchor, without one,
  with one the chain does not follow, window 64 and 2^20, d_prevs_out NULL;
* DRANDHIP_ASSEMBLE_DEDUPE=0 changes the DUPLICATE bits only;
* assemble_archives over a JSON archive, a protobuf packet run and a bolt store; assemble_to_trimmed_store byte for byte
  against write_trimmed_bolt; sync.sync_from_sources; the ABI's refusals, two threads, a call after dh_shutdown."""
import ctypes
import os
import threading

import numpy as np
import pytest

import archive_cases as ac
import assemble_cases as asc

pytestmark = pytest.mark.gpu
SORT_TILE = 2048  # kernels.hpp


@pytest.fixture(scope="module")
def dh():
    import torch
    import drand_amd
    from drand_amd import _lib
    torch.zeros(1, device="cuda")
    assert _lib.load().dh_init(0) == 0, _lib.last_error()
    return drand_amd


@pytest.fixture(scope="module")
def gold_ar():
    return ac.load_golden()


@pytest.fixture(scope="module")
def gold():
    return asc.load_golden()


def key_sets(n):
    i = np.arange(n, dtype=np.uint64)
    rng = np.random.default_rng(n)
    mixed = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    ends = mixed.copy()
    if n >= 2:
        ends[0], ends[-1] = np.uint64((1 << 64) - 1), np.uint64(0)
    return {
        "ascending": i * np.uint64(3) + np.uint64(5),
        "descending": (np.uint64(n) - i) * np.uint64(3),
        "all equal": np.full(n, 0x0123456789ABCDEF, np.uint64),
        "two values": np.where(i % np.uint64(2) == 0, np.uint64(9), np.uint64(4)),
        "top byte, bit 63 set": ((np.uint64(0x80) + (i * np.uint64(7)) % np.uint64(128)) << np.uint64(56)) | np.uint64(0x1234),
        "byte 0 only": np.uint64(0xABCD00) + (i * np.uint64(37)) % np.uint64(256),
        "every byte": mixed,
        "0 and 2^64 - 1": ends,
    }


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 2 * SORT_TILE + 1, 40001])
def test_sort_is_numpy_stable_argsort(dh, n):
    """40001 keys: 20 tiles, 5120 digit-major counts, so launch_scan runs its hierarchical path (above 4096 counts)."""
    from drand_amd import _lib
    lib = _lib.load()
    for what, keys in key_sets(n).items():
        keys = np.ascontiguousarray(keys, np.uint64)
        perm = np.full(n, 0xFFFFFFFF, np.uint32)
        rc = lib.dh_sort_rounds_debug(ctypes.c_void_p(keys.ctypes.data) if n else None, n, ctypes.c_void_p(perm.ctypes.data) if n else None)
        assert rc == 0, (what, _lib.last_error())
        assert np.array_equal(perm, np.argsort(keys, kind="stable").astype(np.uint32)), what


def test_sort_refusals(dh):
    from drand_amd import _lib
    lib = _lib.load()
    keys, perm = np.zeros(4, np.uint64), np.zeros(4, np.uint32)
    assert lib.dh_sort_rounds_debug(None, 4, ctypes.c_void_p(perm.ctypes.data)) == _lib.DH_EINVAL
    assert lib.dh_sort_rounds_debug(ctypes.c_void_p(keys.ctypes.data), 4096 * 4096 - 1, ctypes.c_void_p(perm.ctypes.data)) == _lib.DH_EINVAL


def stride_of(name):
    return (ac.SIG_LEN[name] + 3) & ~3


def device_columns(cands, name):
    import torch
    from drand_amd import scheme_from_name
    s = scheme_from_name(name)
    rounds, sigs, lens, prevs, prev_lens, skip = asc.columns(cands, stride_of(name), s.chained)
    up = lambda a, view=None: torch.from_numpy(a.view(view) if view else a).cuda() if a is not None else None  # noqa: E731
    return up(rounds, np.int64), up(sigs), up(lens, np.int32), up(prevs), up(prev_lens, np.int32), up(skip)


def assemble(dh, name, gold_ar, cands, **kw):
    from drand_amd import scheme_from_name, store
    rounds, sigs, lens, prevs, prev_lens, skip = device_columns(cands, name)
    pk = bytes.fromhex(gold_ar["chains"][name]["pk"])
    return store.assemble_columns(scheme_from_name(name), pk, rounds, sigs, lens, prevs, prev_lens, skip, **kw)


def check_rows(res, cands, name, want_prev=True):
    """Every output row is its source candidate, whole and zero-padded."""
    stride = stride_of(name)
    src = res.src.cpu().numpy()
    sigs, lens = res.sigs.cpu().numpy(), res.lens.cpu().numpy()
    assert sigs.shape == (len(src), stride)
    for k, i in enumerate(src):
        s = cands[i]["signature"]
        assert lens[k] == len(s) and sigs[k].tobytes() == s + bytes(stride - len(s))
    if name == "pedersen-bls-chained" and want_prev:
        prevs, prev_lens = res.prevs.cpu().numpy(), res.prev_lens.cpu().numpy()
        for k, i in enumerate(src):
            p = cands[i]["previous_signature"]
            assert prev_lens[k] == len(p) and prevs[k].tobytes() == p + bytes(stride - len(p))
    else:
        assert res.prevs is None and res.prev_lens is None


@pytest.mark.parametrize("name", asc.SCHEMES)
def test_clean_union_is_the_chain(dh, gold_ar, name):
    cands, ids = asc.clean_pile(name, gold_ar)
    res = assemble(dh, name, gold_ar, cands, anchor=ac.anchor(name))
    chain = ac.chain_records(name, gold_ar)
    assert [int(x) for x in res.rounds.cpu().numpy().view(np.uint64)] == [r["round"] for r in chain]
    assert res.sigs.cpu().numpy()[:, :ac.SIG_LEN[name]].tobytes() == b"".join(r["signature"] for r in chain)
    check_rows(res, cands, name)
    if name == "pedersen-bls-chained":
        assert res.prevs.cpu().numpy().tobytes() == b"".join(r["previous_signature"] for r in chain)
    assert not res.flags.cpu().numpy().any() and res.gaps == [] and res.contiguous_up_to == ac.N
    assert res.counts["verified"] == ac.N and res.counts["duplicates"] == len(cands) - ac.N  # exact: every copy collapsed
    assert res.counts["chosen"] == ac.N and not res.counts["invalid"] and not res.counts["conflicts"] and not res.counts["missing"]
    # the first copy in input order is the chosen one: rounds 1 .. 200 come from source A
    assert [int(x) for x in res.src.cpu().numpy()[:200]] == list(range(200))
    per = res.per_source(ids)
    assert per[0]["chosen"] == 200 and per[1]["chosen"] == 100 and per[2]["chosen"] == 0 and per[2]["duplicates"] == 100


CALLS = [(name, kind, 64 if kind == "anchor" else 1 << 20, not (kind == "bad_anchor")) for name in asc.SCHEMES for kind in asc.ANCHORS]


@pytest.mark.parametrize("name,kind,window,want_prev", CALLS, ids=["%s-%s-w%d" % c[:3] for c in CALLS])
def test_faulty_pile_equals_the_record(dh, gold_ar, gold, name, kind, window, want_prev):
    cands, _ = asc.faulty_pile(name, gold_ar)
    res = assemble(dh, name, gold_ar, cands, anchor=asc.ANCHORS[kind](name, gold_ar), up_to=asc.UP_TO, window=window, want_prev=want_prev)
    got, want = asc.plain(res), gold[name][kind]
    for k in ("status", "rounds", "src", "flags", "gaps", "counts", "contiguous_up_to"):
        assert got[k] == want[k], k
    check_rows(res, cands, name, want_prev)


@pytest.mark.parametrize("name", ["pedersen-bls-chained", "bls-unchained-g1-rfc9380"])
def test_dedupe_does_not_change_the_result(dh, gold_ar, gold, name):
    from drand_amd import store
    cands, _ = asc.faulty_pile(name, gold_ar)
    kw = dict(anchor=asc.anchor(name, gold_ar), up_to=asc.UP_TO)
    on = assemble(dh, name, gold_ar, cands, **kw)
    os.environ["DRANDHIP_ASSEMBLE_DEDUPE"] = "0"
    try:
        off = assemble(dh, name, gold_ar, cands, **kw)
    finally:
        del os.environ["DRANDHIP_ASSEMBLE_DEDUPE"]
    dup = np.uint8(store.AS_DUPLICATE)
    assert np.array_equal(on.status & ~dup, off.status & ~dup)
    assert off.counts["verified"] == len(cands) - off.counts["stale"] - off.counts["skipped"] > on.counts["verified"]
    for k in ("rounds", "sigs", "lens", "src", "flags"):
        assert np.array_equal(getattr(on, k).cpu().numpy(), getattr(off, k).cpu().numpy()), k
    assert on.gaps == off.gaps and on.contiguous_up_to == off.contiguous_up_to
    assert {k: v for k, v in on.counts.items() if k not in ("verified", "duplicates")} == \
        {k: v for k, v in off.counts.items() if k not in ("verified", "duplicates")}
    again = assemble(dh, name, gold_ar, cands, **kw)  # read at every call
    assert np.array_equal(again.status, on.status) and again.counts == on.counts


# ---- end to end

BEACON_ID = "default"


def mixed_sources(name, gold_ar, tmp_path, beacon_id=BEACON_ID, drop=()):
    """The three sources of the clean pile as a JSON archive (with one deferred record and one blank line), a protobuf
    packet run and an untrimmed bolt store; `drop`: rounds left out of every source."""
    import boltwrite
    import bolt_cases as bc
    import bolt_json_cases as jc
    from drand_amd import scheme_from_name
    from drand_amd.store import PB_BEACON_PACKET, DeviceArchive, DeviceBoltStore, packet_bytes, random_data_line
    chained = scheme_from_name(name).chained
    a, b, c = [[r for r in s if r["round"] not in drop] for s in asc.three_sources(name, gold_ar)]
    lines = [random_data_line(r) for r in a]
    lines[7] = lines[7].replace(b'{"round"', b'{ "round"')  # deferred: the host decoder patches it in
    lines.insert(20, b"   ")                                  # a blank line: skipped
    json_ar = DeviceArchive(b"\n".join(lines) + b"\n")
    pb_ar = DeviceArchive.from_packets(PB_BEACON_PACKET, [packet_bytes(PB_BEACON_PACKET, dict(r, randomness=b""), beacon_id) for r in b])
    path = os.path.join(str(tmp_path), "c-%s-%d.db" % (name, len(drop)))
    boltwrite.write_bolt(path, b"beacons", {bc.key(r["round"]): jc.marshal(r["round"], r["signature"], r["previous_signature"] if chained else None)
                                            for r in c})
    return [json_ar, pb_ar, DeviceBoltStore(path, chained, fmt="untrimmed")], len(lines)


E2E = ["pedersen-bls-chained", "bls-unchained-g1-rfc9380"]


@pytest.mark.parametrize("name", E2E)
def test_assemble_archives_and_store_file(dh, gold_ar, tmp_path, name):
    from drand_amd import scheme_from_name, store
    s, pk = scheme_from_name(name), bytes.fromhex(gold_ar["chains"][name]["pk"])
    chain = ac.chain_records(name, gold_ar)
    sources, n_json = mixed_sources(name, gold_ar, tmp_path)
    try:
        res, ids = store.assemble_archives(sources, s, pk, anchor=ac.anchor(name))
        assert [int(x) for x in res.rounds.cpu().numpy().view(np.uint64)] == [r["round"] for r in chain]
        assert res.sigs.cpu().numpy()[:, :s.sig_len].tobytes() == b"".join(r["signature"] for r in chain)
        assert res.counts["skipped"] == 1 and res.counts["verified"] == ac.N and res.contiguous_up_to == ac.N and res.gaps == []
        assert res.status[20] == store.AS_SKIPPED and res.status[7] == store.AS_CHOSEN  # the blank line; the deferred record
        assert list(np.bincount(ids)) == [n_json, 181, 100] and res.per_source(ids)[0]["chosen"] == 200
        want = os.path.join(str(tmp_path), "want.db")
        store.write_trimmed_bolt(want, np.array([r["round"] for r in chain], np.uint64),
                                 np.array([np.frombuffer(r["signature"], np.uint8) for r in chain]))
        got = os.path.join(str(tmp_path), "got.db")
        out = store.assemble_to_trimmed_store(sources, got, s, pk, anchor=ac.anchor(name))
        assert out["rows"] == ac.N and open(got, "rb").read() == open(want, "rb").read()
    finally:
        [x.close() for x in sources]
    # a round no source holds: refused, then written with allow_gaps
    sources, _ = mixed_sources(name, gold_ar, tmp_path, drop=(150,))
    try:
        holed = os.path.join(str(tmp_path), "holed.db")
        with pytest.raises(ValueError, match="150-150"):
            store.assemble_to_trimmed_store(sources, holed, s, pk, anchor=ac.anchor(name))
        assert not os.path.exists(holed) and not os.path.exists(holed + ".tmp")
        out = store.assemble_to_trimmed_store(sources, holed, s, pk, anchor=ac.anchor(name), allow_gaps=True)
        assert out["rows"] == ac.N - 1 and out["assembled"].gaps == [(150, 150)]
        rest = [r for r in chain if r["round"] != 150]
        store.write_trimmed_bolt(want, np.array([r["round"] for r in rest], np.uint64),
                                 np.array([np.frombuffer(r["signature"], np.uint8) for r in rest]))
        assert open(holed, "rb").read() == open(want, "rb").read()
    finally:
        [x.close() for x in sources]


@pytest.mark.parametrize("name", E2E)
def test_sync_from_sources(dh, gold_ar, tmp_path, name):
    from drand_amd import scheme_from_name, sync
    from drand_amd.store import PB_BEACON_PACKET, DeviceArchive, packet_bytes
    s, pk = scheme_from_name(name), bytes.fromhex(gold_ar["chains"][name]["pk"])
    chain = ac.chain_records(name, gold_ar)

    def fresh():
        st = sync.TrimmedMemStore(s.chained)
        st.put(*ac.anchor(name))
        return st
    sources, _ = mixed_sources(name, gold_ar, tmp_path, drop=(150, 151))
    try:
        st = fresh()
        done, stored, gaps = sync.sync_from_sources(sources, s, pk, st, up_to=ac.N, beacon_id=BEACON_ID)
        assert not done and stored == list(range(1, 150)) and gaps == [(150, 151)]  # exactly the contiguous prefix
        assert st.len() == 150 and st.get(149).signature == chain[148]["signature"]
        with pytest.raises(sync.NoBeaconStored):
            st.get(152)
        st = fresh()
        done, stored, gaps = sync.sync_from_sources(sources, s, pk, st, up_to=100, beacon_id=BEACON_ID)
        assert done and stored == list(range(1, 101)) and gaps == []
        # a protobuf source of another beacon ID is dropped whole: the rounds only it held are gaps
        foreign = DeviceArchive.from_packets(PB_BEACON_PACKET, [packet_bytes(PB_BEACON_PACKET, dict(r, randomness=b""), "other")
                                                                 for r in chain[149:151]])
        sources.append(foreign)
        st = fresh()
        done, stored, gaps = sync.sync_from_sources(sources, s, pk, st, up_to=ac.N, beacon_id=BEACON_ID)
        assert not done and stored == list(range(1, 150)) and gaps == [(150, 151)]
        st = fresh()  # with its own ID expected it fills the hole
        done, stored, gaps = sync.sync_from_sources(sources[2:], s, pk, st, up_to=ac.N, beacon_id="other")
        assert not done and stored == [] and gaps[0][0] == 1
        assert sync.sync_from_sources(sources, s, pk, sync.TrimmedMemStore(s.chained), up_to=ac.N) == (False, [], [])  # an empty store
    finally:
        [x.close() for x in sources]


def raw_call(dh, name, gold_ar, cands, sig_stride=None, n=None, gap_cap=16, anchor=None, up_to=None):
    """dh_assemble_device itself: (rc, m, n_gaps, counts, gap_first)."""
    import torch
    from drand_amd import _lib, scheme_from_name
    lib = _lib.load()
    s = scheme_from_name(name)
    pk = bytes.fromhex(gold_ar["chains"][name]["pk"])
    rounds, sigs, lens, prevs, prev_lens, skip = device_columns(cands, name)
    rows = len(cands)
    n = rows if n is None else n
    stride = int(sigs.shape[1]) if sig_stride is None else sig_stride
    out = [torch.zeros(rows, dtype=torch.int64, device="cuda"), torch.zeros((rows, sigs.shape[1]), dtype=torch.uint8, device="cuda"),
           torch.zeros(rows, dtype=torch.int32, device="cuda"), torch.zeros(rows, dtype=torch.int32, device="cuda"),
           torch.zeros(rows, dtype=torch.uint8, device="cuda")]
    torch.cuda.synchronize()
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    status = np.zeros(max(rows, 1), np.uint8)
    gf, gl = np.zeros(max(gap_cap, 1), np.uint64), np.zeros(max(gap_cap, 1), np.uint64)
    m, ng, counts = ctypes.c_size_t(0), ctypes.c_size_t(0), (ctypes.c_uint64 * 10)()
    ar = ctypes.c_uint64(anchor[0]) if anchor else None
    ut = ctypes.c_uint64(up_to) if up_to is not None else None
    rc = lib.dh_assemble_device(s.id, pk, len(pk), ptr(rounds), ptr(sigs), stride, ptr(lens), ptr(prevs), stride, ptr(prev_lens), ptr(skip), n,
                                ctypes.byref(ar) if anchor else None, anchor[1] if anchor else None, len(anchor[1]) if anchor else 0,
                                ctypes.byref(ut) if ut is not None else None, 1 << 20, 0, ptr(out[0]), ptr(out[1]), ptr(out[2]), None, None,
                                ptr(out[3]), ptr(out[4]), ctypes.byref(m), ctypes.c_void_p(status.ctypes.data), ctypes.c_void_p(gf.ctypes.data),
                                ctypes.c_void_p(gl.ctypes.data), gap_cap, ctypes.byref(ng), counts, None)
    return rc, m.value, ng.value, [int(x) for x in counts], [int(x) for x in gf]


def test_abi_refusals(dh, gold_ar, gold):
    from drand_amd import _lib, store
    name = "bls-unchained-g1-rfc9380"
    cands, _ = asc.faulty_pile(name, gold_ar)
    kw = dict(anchor=asc.anchor(name, gold_ar), up_to=asc.UP_TO)
    want = gold[name]["anchor"]
    rc, m, ng, counts, gf = raw_call(dh, name, gold_ar, cands, **kw)
    assert rc == 0 and m == len(want["rounds"]) and ng == len(want["gaps"]) and gf[:ng] == [g[0] for g in want["gaps"]]
    assert counts == [want["counts"][k] for k in store.AS_COUNTS]
    for stride in (0, 6, 50, (1 << 20) + 4):
        assert raw_call(dh, name, gold_ar, cands, sig_stride=stride, **kw)[0] == _lib.DH_EINVAL, stride
    assert raw_call(dh, name, gold_ar, cands, n=4096 * 4096 - 1, **kw)[0] == _lib.DH_EINVAL  # refused before a row is read
    rc, m, ng, counts, gf = raw_call(dh, name, gold_ar, cands, gap_cap=1, **kw)  # too few gap entries: the number needed
    assert rc == _lib.DH_EINVAL and ng == len(want["gaps"]) > 1 and m == len(want["rounds"]) and gf[0] == want["gaps"][0][0]
    assert raw_call(dh, name, gold_ar, [])[:3] == (0, 0, 0)  # n = 0
    assert raw_call(dh, name, gold_ar, [], anchor=(5, b"x" * 48), up_to=9)[:3] == (0, 0, 1)  # nothing but the gap 6 .. 9


def test_threads_and_shutdown(dh, gold_ar, gold):
    from drand_amd import _lib
    names = ["pedersen-bls-chained", "bls-unchained-g1-rfc9380"]
    piles = {name: asc.faulty_pile(name, gold_ar)[0] for name in names}
    got, errs = {}, []

    def run(name):
        try:
            got[name] = asc.plain(assemble(dh, name, gold_ar, piles[name], anchor=asc.anchor(name, gold_ar), up_to=asc.UP_TO))
        except Exception as e:  # noqa: BLE001
            errs.append((name, repr(e)))
    ths = [threading.Thread(target=run, args=(name,)) for name in names]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not errs, errs
    assert all(got[name] == gold[name]["anchor"] for name in names)
    lib = _lib.load()
    lib.dh_shutdown()
    try:  # a call after dh_shutdown re-initialises the library, as the other column calls do
        run(names[1])
        assert not errs and got[names[1]] == gold[names[1]]["anchor"]
    finally:
        assert lib.dh_init(0) == 0, _lib.last_error()
