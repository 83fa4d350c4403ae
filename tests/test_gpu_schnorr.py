"""Batch Schnorr verification for DKG packets on the device (dh_schnorr_verify_batch; drandhip.cpp schnorr_core,
k_schnorr.hip): the schemes' DKGAuthScheme (crypto/schemes.go:103,144,184). Every verdict is compared with the one
recorded in tests/golden/schnorr.json (computed by the pure-Python check of its generator, re-verified in
tests/test_schnorr_host.py), and the two forms of the check (the joint chain over tables; two plain scalar
multiplications, DRANDHIP_SCHNORR_PATH=plain) must agree bit for bit."""
import json
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PATHS = [None, "plain"]


@pytest.fixture(scope="module")
def dh():
    import torch
    import drand_amd
    from drand_amd import _lib
    torch.zeros(1, device="cuda")
    lib = _lib.load()
    assert lib.dh_init(0) == 0, _lib.last_error()
    return drand_amd


@pytest.fixture(scope="module")
def fx():
    """per key group: (scheme name, keys, key_ok, items) with items = (class, key index, msg, sig, verdict)"""
    raw = json.load(open(os.path.join(GOLD, "schnorr.json")))
    out = []
    for g in raw["groups"]:
        items = [(it["class"], it["key"], bytes.fromhex(it["msg"]), bytes.fromhex(it["sig"]), bool(it["verdict"]))
                 for it in g["items"]]
        out.append((g["scheme"], [bytes.fromhex(k) for k in g["keys"]], [bool(x) for x in g["key_ok"]], items))
    return out


def _forced(path, fn):
    """fn() with DRANDHIP_SCHNORR_PATH = path (None: the default form); the variable is read at every call."""
    old = os.environ.pop("DRANDHIP_SCHNORR_PATH", None)
    if path:
        os.environ["DRANDHIP_SCHNORR_PATH"] = path
    try:
        return fn()
    finally:
        os.environ.pop("DRANDHIP_SCHNORR_PATH", None)
        if old is not None:
            os.environ["DRANDHIP_SCHNORR_PATH"] = old


def _verify(s, path, keys, items, kidx="items"):
    """verdicts (and key_ok) of the items; kidx = "items": their own key indices into keys"""
    sg = np.array([np.frombuffer(it[3], np.uint8) for it in items]).reshape(len(items), s.schnorr_sig_len)
    ki = [it[1] for it in items] if kidx == "items" else kidx
    v, kok = _forced(path, lambda: s.verify_dkg_signatures(keys, [it[2] for it in items], sg, ki, want_key_ok=True))
    return v.tolist(), kok.tolist()


@pytest.mark.parametrize("gi", [0, 1])
def test_full_fixture_both_paths(dh, fx, gi):
    """All 96 items of the key group under its 12-key table: verdicts and key_ok as recorded, on the default path and
    on plain, and the two equal bit for bit."""
    name, keys, key_ok, items = fx[gi]
    s = dh.scheme_from_name(name)
    assert s.schnorr_sig_len == s.key_len + 32
    want = [it[4] for it in items]
    got = {p: _verify(s, p, keys, items) for p in PATHS}
    for p in PATHS:
        bad = [(i, items[i][0]) for i in range(len(items)) if got[p][0][i] != want[i]]
        assert not bad, (p, bad)
        assert got[p][1] == key_ok, p
    assert got[None] == got["plain"]


@pytest.mark.parametrize("gi", [0, 1])
def test_schemes_sharing_a_key_group_agree(dh, fx, gi):
    """Only the key group matters: pedersen-bls-chained gives the verdicts of pedersen-bls-unchained on the G1-key
    fixture, bls-unchained-on-g1 those of bls-unchained-g1-rfc9380 on the G2-key one."""
    name, keys, key_ok, items = fx[gi]
    other = dh.scheme_from_name(["pedersen-bls-chained", "bls-unchained-on-g1"][gi])
    assert other.key_len == dh.scheme_from_name(name).key_len
    v, kok = _verify(other, None, keys, items)
    assert v == [it[4] for it in items] and kok == key_ok


@pytest.mark.parametrize("gi", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wave_and_workgroup_edges(dh, fx, gi, n):
    """n items cut from the fixture (cycled past 96) around the wave (64) and workgroup (256) sizes of the kernels."""
    name, keys, key_ok, items = fx[gi]
    s = dh.scheme_from_name(name)
    cut = [items[(5 * i + n) % len(items)] for i in range(n)]
    for p in PATHS:
        v, kok = _verify(s, p, keys, cut)
        assert v == [it[4] for it in cut], p
        assert kok == key_ok


@pytest.mark.parametrize("gi", [0, 1])
def test_one_key_per_item_and_empty(dh, fx, gi):
    """key_idx = NULL: item i under key i of a 70-entry table (each item's own key copied out, bad keys included);
    n = 0 returns empty verdicts."""
    name, keys, key_ok, items = fx[gi]
    s = dh.scheme_from_name(name)
    cut = [items[(7 * i + 3) % len(items)] for i in range(70)]
    tab = [keys[it[1]] for it in cut]
    for p in PATHS:
        v, kok = _verify(s, p, tab, cut, kidx=None)
        assert v == [it[4] for it in cut], p
        assert kok == [key_ok[it[1]] for it in cut]
    v, kok = _forced(None, lambda: s.verify_dkg_signatures([], [], np.zeros((0, s.schnorr_sig_len), np.uint8), None, True))
    assert v.tolist() == [] and kok.tolist() == []
    v = s.verify_dkg_signatures(keys, [], np.zeros((0, s.schnorr_sig_len), np.uint8), [])
    assert v.tolist() == []


@pytest.mark.parametrize("gi", [0, 1])
@pytest.mark.parametrize("cls", ["r_torsion", "s_plus_r"])
def test_sixteen_faults_alone(dh, fx, gi, cls):
    """16 items of one fault class alone in a call (the fixture's items of the class, repeated): R + T for a
    small-order T never satisfies the equation without a subgroup test of R, and s + r is refused by the range check;
    nothing valid shares the call, so no neighbour can lend them a verdict."""
    name, keys, key_ok, items = fx[gi]
    s = dh.scheme_from_name(name)
    mine = [it for it in items if it[0] == cls]
    assert len(mine) >= 2
    cut = [mine[i % len(mine)] for i in range(16)]
    for p in PATHS:
        v, _ = _verify(s, p, keys, cut)
        assert v == [False] * 16, p


def test_two_threads_get_their_own_verdicts(dh, fx):
    """Two threads call concurrently, one with the G1-key fixture and one with the G2-key fixture, four times each:
    each gets its own fixture's verdicts (the calls lease separate workers and share only the generator tables)."""
    out, err = {}, []

    def work(gi):
        try:
            name, keys, key_ok, items = fx[gi]
            s = dh.scheme_from_name(name)
            sg = np.array([np.frombuffer(it[3], np.uint8) for it in items])
            res = []
            for _ in range(4):
                res.append(s.verify_dkg_signatures(keys, [it[2] for it in items], sg, [it[1] for it in items]).tolist())
            out[gi] = res
        except Exception as e:  # noqa: BLE001
            err.append(repr(e))

    ts = [threading.Thread(target=work, args=(gi,)) for gi in (0, 1)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not err, err
    for gi in (0, 1):
        assert out[gi] == [[it[4] for it in fx[gi][3]]] * 4
