"""GPU: level 0 of a large local G1-signature batch on one 63-bit scalar half, behind DRANDHIP_G1_RLC_HALF.

Two child processes (the library reads its switches once) with DRANDHIP_SUB_BATCH_MIN=65 and DRANDHIP_SUB_BACKOFF=0, the
switch 1 and 0, for quicknet and bls-unchained-on-g1:

* valid chains of 2, 64 (the small path, untouched), 65, 256 and 300 rounds (the batched path: c = 5, 6 and 6);
* on 300 rounds: one signature of each rejected-encoding class, non-residues and other rounds' signatures; one valid G1
  point that is the wrong signature (level 0 fails, the fallback and the bisection name exactly that round, the stats
  show the work below level 0); one curve point outside G1, sigma + T3 (the batched subgroup test fails the batch, the
  exact test flags the round);
* quicknet: verify_recovered_batch on 300 messages, one of them twice with its valid signature (equal hash points meet
  in a bucket: the doubling on E1'), and the same batch with one wrong signature;
* dh_msm_level0_shape_debug after every batched call: nwin rows per set and n x nwin entries on the a-half alone with
  the switch on, 2 nwin and 2 n x nwin on both halves with it off.

Verdicts equal to the oracle's and between the two settings, randomness the SHA-256 of the signature and equal between
the two."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
NAMES = ("bls-unchained-g1-rfc9380", "bls-unchained-on-g1")
QUICKNET = NAMES[0]
N = 300
SIZES = (2, 64, 65, 256, 300)
SUB_MIN = 65
CASES = ("classes", "wrong", "outside")
WRONG, OUTSIDE = 100, 131
DUP, DUP_OF = 200, 10


def nwin_of(n):
    """drandhip.cpp geom_for(n, 2): the windows of a 63-bit half for a group of n rounds."""
    c = max(3, min(16, (2 * n).bit_length() - 1 - 2))

    def window_ok(c):
        nw = (63 + 1 + c - 1) // c
        return 63 - c * (nw - 1) >= c - 4

    while c > 3 and not window_ok(c):
        c -= 1
    return (63 + 1 + c - 1) // c


def build_case(name, sigs):
    from test_gpu_g1_ride import corrupt
    from test_gpu_subgroup_batch import add_point
    s = sigs.copy()
    if name == "classes":
        s = corrupt(sigs)
    elif name == "wrong":
        s[WRONG] = sigs[WRONG + 1]
    elif name == "outside":
        s[OUTSIDE] = add_point(sigs[OUTSIDE], (0, 2))  # a point of order 3 added: on the curve, outside G1
    return s


def run_child(path):
    import torch
    from test_gpu_h2c_chain import init_gpu, secret
    from drand_amd import _lib
    drand_amd, lib = init_gpu()
    out = {}

    def shape(key):
        rows, entries = ctypes.c_uint64(), ctypes.c_uint64()
        ha, hb = ctypes.c_int(), ctypes.c_int()
        assert lib.dh_msm_level0_shape_debug(ctypes.byref(rows), ctypes.byref(entries), ctypes.byref(ha), ctypes.byref(hb)) == 0
        out[key + "/shape"] = np.array([rows.value, entries.value, ha.value, hb.value], np.int64)

    sk = secret()
    dev = torch.device("cuda", 0)
    for name in NAMES:
        s = drand_amd.scheme_from_name(name)
        pk = s.public_key(sk)
        rounds = np.arange(1, N + 1, dtype=np.uint64)
        base = s.sign_beacons(sk, rounds)
        out[name + "/pk"] = np.frombuffer(pk, np.uint8)
        out[name + "/base"] = base
        for n in SIZES:
            key = "%s/valid%d" % (name, n)
            v, rand = s.verify_beacons(pk, rounds[:n], base[:n], seed=5)
            out[key + "/v"], out[key + "/rand"] = np.asarray(v, bool), np.asarray(rand)
            shape(key)
        for case in CASES:
            sigs = build_case(case, base)
            key = name + "/" + case
            v, rand = s.verify_beacons(pk, rounds, sigs, seed=5)
            out[key + "/v"], out[key + "/rand"], out[key + "/sigs"] = np.asarray(v, bool), np.asarray(rand), sigs
            shape(key)
        # the wrong signature once more on device arrays, for the call's stats {levels, failing groups, leaves, rejected}
        sigs = build_case("wrong", base)
        d_r, d_s = torch.from_numpy(rounds.view(np.int64)).to(dev), torch.from_numpy(sigs).to(dev)
        d_v = torch.zeros(N, dtype=torch.uint8, device=dev)
        stats = (ctypes.c_uint64 * 4)()
        for tag, d in (("wrong", d_s), ("valid", torch.from_numpy(base).to(dev))):
            rc = lib.dh_verify_batch_device(s.id, pk, len(pk), ctypes.c_void_p(d_r.data_ptr()), ctypes.c_void_p(d.data_ptr()), 48,
                                            None, 0, None, N, ctypes.c_void_p(d_v.data_ptr()), None, 5, None, stats)
            assert rc == 0, _lib.last_error()
            out["%s/%s/stats" % (name, tag)] = np.array(list(stats), np.int64)
            out["%s/%s/dv" % (name, tag)] = d_v.cpu().numpy().astype(bool)
    s = drand_amd.scheme_from_name(QUICKNET)
    pk = s.public_key(sk)
    base = out[QUICKNET + "/base"]
    msgs = [s.digest_beacon(r) for r in range(1, N + 1)]
    sigs = base.copy()
    msgs[DUP], sigs[DUP] = msgs[DUP_OF], base[DUP_OF]
    out["recovered/v"] = s.verify_recovered_batch(pk, msgs, sigs, seed=7)
    shape("recovered")
    bad = sigs.copy()
    bad[DUP + 1] = base[3]  # the same batch with one wrong signature: the duplicate pair through the fallback too
    out["recovered_bad/v"] = s.verify_recovered_batch(pk, msgs, bad, seed=7)
    shape("recovered_bad")
    np.savez(path, **out)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("g1_rlc_half")
    res = {}
    for half in ("1", "0"):
        out = d / ("half%s.npz" % half)
        env = {k: v for k, v in os.environ.items() if not k.startswith("DRANDHIP_SUB") and not k.startswith("DRANDHIP_G1_")}
        env.update(DRANDHIP_SUB_BATCH_MIN=str(SUB_MIN), DRANDHIP_SUB_BACKOFF="0", DRANDHIP_G1_RLC_HALF=half)
        assert subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, timeout=300).returncode == 0
        res[half] = dict(np.load(str(out)))
    return res


def shape_ok(runs, key, n):
    nwin = nwin_of(n)
    assert runs["1"][key + "/shape"].tolist() == [nwin, n * nwin, 1, 0], key
    assert runs["0"][key + "/shape"].tolist() == [2 * nwin, 2 * n * nwin, 1, 1], key


def test_window_counts():
    assert [nwin_of(n) for n in (65, 256, 300, 1 << 20)] == [13, 11, 11, 4]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_valid_chains(runs, name, n):
    on, off = runs["1"], runs["0"]
    key = "%s/valid%d" % (name, n)
    base = on[name + "/base"]
    for r in (on, off):
        assert r[key + "/v"].all() and len(r[key + "/v"]) == n
        for i in range(n):
            assert r[key + "/rand"][i].tobytes() == hashlib.sha256(base[i].tobytes()).digest(), i
    if n >= SUB_MIN:
        shape_ok(runs, key, n)


@pytest.fixture(scope="module")
def valid_verdicts(oracle, runs):
    """The oracle on the untouched chains, once: a case's other rounds keep these verdicts."""
    want = {}
    for name in NAMES:
        rounds = np.arange(1, N + 1, dtype=np.uint64)
        v, _ = oracle.verify_batch(name, runs["1"][name + "/pk"].tobytes(), rounds, runs["1"][name + "/base"], nthreads=8,
                                   want_rand=False)
        want[name] = [bool(x) for x in v]
        assert all(want[name])
    return want


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", NAMES)
def test_rejected_rounds_match_the_oracle(oracle, runs, valid_verdicts, name, case):
    on, off = runs["1"], runs["0"]
    key = name + "/" + case
    sigs, base = on[key + "/sigs"], on[name + "/base"]
    assert np.array_equal(sigs, off[key + "/sigs"]) and len(sigs) == N
    pk = on[name + "/pk"].tobytes()
    want = list(valid_verdicts[name])
    changed = [i for i in range(N) if not np.array_equal(sigs[i], base[i])]
    for i in changed:
        want[i] = bool(oracle.verify_beacon(name, pk, i + 1, sigs[i].tobytes()))
    assert not any(want[i] for i in changed)
    assert len(changed) == {"classes": 14, "wrong": 1, "outside": 1}[case]
    for r in (on, off):
        v = r[key + "/v"]
        assert [bool(x) for x in v] == want
        for i in np.flatnonzero(v):
            assert r[key + "/rand"][i].tobytes() == hashlib.sha256(sigs[i].tobytes()).digest(), i
    assert np.array_equal(on[key + "/v"], off[key + "/v"])
    assert np.array_equal(on[key + "/rand"], off[key + "/rand"])
    shape_ok(runs, key, N)


@pytest.mark.parametrize("name", NAMES)
def test_wrong_signature_goes_below_level_0(runs, name):
    for r in (runs["1"], runs["0"]):
        levels, failing, leaves, rejected = r[name + "/wrong/stats"].tolist()
        assert np.flatnonzero(~r[name + "/wrong/dv"]).tolist() == [WRONG]
        assert rejected == 1 and failing >= 1
        assert levels >= 2 or leaves > 0  # a bisection level or the leaves after the failed level 0
        assert r[name + "/valid/stats"].tolist() == [1, 0, 0, 0] and r[name + "/valid/dv"].all()
    assert runs["1"][name + "/wrong/stats"].tolist() == runs["0"][name + "/wrong/stats"].tolist()


def test_recovered_batch_with_one_message_twice(oracle, runs):
    on, off = runs["1"], runs["0"]
    base, pk = on[QUICKNET + "/base"], on[QUICKNET + "/pk"].tobytes()
    assert oracle.verify_beacon(QUICKNET, pk, DUP_OF + 1, base[DUP_OF].tobytes())
    assert not oracle.verify_beacon(QUICKNET, pk, DUP + 2, base[3].tobytes())
    for r in (on, off):
        assert r["recovered/v"].all() and len(r["recovered/v"]) == N
        assert np.flatnonzero(~r["recovered_bad/v"]).tolist() == [DUP + 1]
    shape_ok(runs, "recovered", N)
    shape_ok(runs, "recovered_bad", N)


if __name__ == "__main__":
    run_child(sys.argv[1])
