"""GPU: a large local G1-signature batch with the hash's 11-isogeny left to the MSM, behind
DRANDHIP_G1_ISO_LATE: the per-round kernel stores the affine E1' sum, level 0 runs with the scalar halves in window rows
of their own and maps eight row sums to E1, and a batch that level 0 does not end falls back to the isogeny per round.

* debug entry: dh_g1_round_prep_late_debug on 1, 64, 65 and 300 rounds (prefixes of test_gpu_g1_ride's input set, one
  lane added): the stored E1' point of every round against swu(u0) + swu(u1) computed by the oracle's group law with
  the curve's A', every rejected signature class included; u1 = u0 (the doubling, lane 6) and u1 = -u0 (the identity:
  zeros and a rejected round, lane 7 under a rejected and lane 9 under a valid signature); sigma as the decode's.
* verify_beacons in child processes (the library reads its switches once) with DRANDHIP_SUB_BATCH_MIN=256
  DRANDHIP_SUB_BACKOFF=0 and the switch 1 and 0, a 320-round quicknet chain and a 300-round bls-unchained-on-g1 chain:
  all valid; one signature of each rejected-encoding class, non-residues and other rounds' signatures; one valid G1
  point that is the wrong signature (forces the fallback and the bisection); one curve point outside G1 (the batched
  subgroup test has to fail the batch); for quicknet a VerifyRecovered-shaped batch of 260 messages in which one
  message appears twice with its valid signature (equal hash points meet in the reduction), and a batch of exactly 256
  rounds. Verdicts equal to the oracle's and between the two settings, randomness the SHA-256 of the signature and
  equal between the two, and the k_msm_prep28 launch count: none on the new path unless the batch fell back.
"""
import ctypes
import hashlib
import json
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
CHAINS = (("bls-unchained-g1-rfc9380", 320), ("bls-unchained-on-g1", 300))
QUICKNET = CHAINS[0][0]
CASES = ("valid", "classes", "wrong", "outside")
WRONG, OUTSIDE = 100, 131
N_REC, DUP, DUP_OF = 260, 200, 10
STAGES = ("k_msm_prep28<fp>", "k_sub_batch_level0", "k_sub_exact", "k_leaf_check")
DEBUG_SIZES = (1, 64, 65, 300)
IDENTITY_UNDER_VALID = 9


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
    from test_gpu_h2c_chain import init_gpu, secret
    drand_amd, lib = init_gpu()
    out = {}

    def profiled(key, f):
        lib.dh_profile(1)
        r = f()
        buf = ctypes.create_string_buffer(1 << 16)
        lib.dh_profile_read(buf, len(buf))
        lib.dh_profile(0)
        prof = json.loads(buf.value.decode())
        out[key + "/counts"] = np.array([prof.get(k, {}).get("count", 0) for k in STAGES])
        return r

    sk = secret()
    for name, n in CHAINS:
        s = drand_amd.scheme_from_name(name)
        pk = s.public_key(sk)
        rounds = np.arange(1, n + 1, dtype=np.uint64)
        base = s.sign_beacons(sk, rounds)
        out[name + "/pk"] = np.frombuffer(pk, np.uint8)
        out[name + "/base"] = base
        for case in CASES:
            sigs = build_case(case, base)
            key = name + "/" + case
            v, rand = profiled(key, lambda: s.verify_beacons(pk, rounds, sigs, seed=5))
            out[key + "/v"] = np.asarray(v, bool)
            out[key + "/rand"] = np.asarray(rand)
            out[key + "/sigs"] = sigs
    s = drand_amd.scheme_from_name(QUICKNET)
    pk = s.public_key(sk)
    base = out[QUICKNET + "/base"]
    v, rand = profiled("exact256", lambda: s.verify_beacons(pk, np.arange(1, 257, dtype=np.uint64), base[:256], seed=6))
    out["exact256/v"] = np.asarray(v, bool)
    msgs = [s.digest_beacon(r) for r in range(1, N_REC + 1)]
    sigs = base[:N_REC].copy()
    msgs[DUP], sigs[DUP] = msgs[DUP_OF], base[DUP_OF]
    out["recovered/v"] = profiled("recovered", lambda: s.verify_recovered_batch(pk, msgs, sigs, seed=7))
    bad = sigs.copy()
    bad[DUP + 1] = base[3]  # the same batch with one wrong signature: the duplicate pair through the fallback too
    out["recovered_bad/v"] = profiled("recovered_bad", lambda: s.verify_recovered_batch(pk, msgs, bad, seed=7))
    np.savez(path, **out)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("g1_iso_late")
    res = {}
    for late in ("1", "0"):
        out = d / ("late%s.npz" % late)
        env = {k: v for k, v in os.environ.items() if not k.startswith("DRANDHIP_SUB") and not k.startswith("DRANDHIP_G1_")}
        env.update(DRANDHIP_SUB_BATCH_MIN="256", DRANDHIP_SUB_BACKOFF="0", DRANDHIP_G1_ISO_LATE=late)
        assert subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, timeout=300).returncode == 0
        res[late] = dict(np.load(str(out)))
    return res


@pytest.fixture(scope="module")
def valid_verdicts(oracle, runs):
    """The oracle on the untouched chains, once: a case's other rounds keep these verdicts."""
    want = {}
    for name, n in CHAINS:
        rounds = np.arange(1, n + 1, dtype=np.uint64)
        v, _ = oracle.verify_batch(name, runs["1"][name + "/pk"].tobytes(), rounds, runs["1"][name + "/base"], nthreads=8,
                                   want_rand=False)
        want[name] = [bool(x) for x in v]
        assert all(want[name])
    return want


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name,n", CHAINS)
def test_verify_matches_oracle_with_the_isogeny_late_and_per_round(oracle, runs, valid_verdicts, name, n, case):
    on, off = runs["1"], runs["0"]
    key = name + "/" + case
    sigs, base = on[key + "/sigs"], on[name + "/base"]
    assert np.array_equal(sigs, off[key + "/sigs"]) and len(sigs) == n
    pk = on[name + "/pk"].tobytes()
    want = list(valid_verdicts[name])
    changed = [i for i in range(n) if not np.array_equal(sigs[i], base[i])]
    for i in changed:
        want[i] = bool(oracle.verify_beacon(name, pk, i + 1, sigs[i].tobytes()))
    assert not any(want[i] for i in changed)
    assert len(changed) == {"valid": 0, "classes": 14, "wrong": 1, "outside": 1}[case]
    for r in (on, off):
        v = r[key + "/v"]
        assert [bool(x) for x in v] == want
        for i in np.flatnonzero(v):
            assert r[key + "/rand"][i].tobytes() == hashlib.sha256(sigs[i].tobytes()).digest(), i
    assert np.array_equal(on[key + "/v"], off[key + "/v"])
    assert np.array_equal(on[key + "/rand"], off[key + "/rand"])
    # k_msm_prep28: per batch without the deferral; with it only when level 0 did not end the batch
    prep_on, sub_on, exact_on, leaf_on = on[key + "/counts"].tolist()
    assert off[key + "/counts"].tolist()[0] == 1 and sub_on == 1
    assert prep_on == (0 if case == "valid" else 1)
    assert exact_on == (1 if case == "outside" else 0)
    assert off[key + "/counts"].tolist()[1:3] == [sub_on, exact_on]


def test_exactly_256_rounds(runs):
    for late in ("1", "0"):
        assert runs[late]["exact256/v"].all() and len(runs[late]["exact256/v"]) == 256
    assert runs["1"]["exact256/counts"].tolist()[:2] == [0, 1]
    assert runs["0"]["exact256/counts"].tolist()[:2] == [1, 1]


def test_recovered_batch_with_one_message_twice(oracle, runs):
    on, off = runs["1"], runs["0"]
    base, pk = on[QUICKNET + "/base"], on[QUICKNET + "/pk"].tobytes()
    # the duplicated pair is round DUP_OF + 1's valid beacon, and the wrong one is round 4's signature on another message
    assert oracle.verify_beacon(QUICKNET, pk, DUP_OF + 1, base[DUP_OF].tobytes())
    assert not oracle.verify_beacon(QUICKNET, pk, DUP + 2, base[3].tobytes())
    for r in (on, off):
        assert r["recovered/v"].all() and len(r["recovered/v"]) == N_REC
        assert np.flatnonzero(~r["recovered_bad/v"]).tolist() == [DUP + 1]
    assert on["recovered/counts"].tolist()[:2] == [0, 1] and off["recovered/counts"].tolist()[:2] == [1, 1]
    assert on["recovered_bad/counts"].tolist()[:2] == [1, 1]


# ---------------------------------------------------------------- the debug entry

@pytest.fixture(scope="module")
def debug_reference():
    import bls_py as B
    import g1_ride_model as M
    import iso11_h_model as H
    from test_gpu_g1_ride import debug_inputs
    us, sigs, kinds = debug_inputs()
    assert IDENTITY_UNDER_VALID not in kinds
    us[IDENTITY_UNDER_VALID] = (us[IDENTITY_UNDER_VALID][0], (B.P - us[IDENTITY_UNDER_VALID][0]) % B.P)
    h = H.monic_sqrt(B.ISO11_XDEN)
    xnum, ynum = [c % B.P for c in B.ISO11_XNUM], [c % B.P for c in B.ISO11_YNUM]
    ref = []
    for (u0, u1), sig in zip(us, sigs):
        st, sigma, _ = M.hash_point(u0, u1, xnum, ynum, h, sig)
        q = B.ec_add(B.FP, B.sswu_g1(u0), B.sswu_g1(u1), B.A1P)  # on E1', before the isogeny
        ref.append((st if q is not None else 0, sigma, q))
    assert ref[6][2] == B.ec_dbl(B.FP, B.sswu_g1(us[6][0]), B.A1P) and ref[7][2] is None
    assert ref[IDENTITY_UNDER_VALID][1:] == (B.g1_decompress(sigs[IDENTITY_UNDER_VALID], subgroup_check=False), None)
    return us, sigs, kinds, ref


@pytest.mark.parametrize("n", DEBUG_SIZES)
def test_debug_entry_stores_the_e1p_sum(debug_reference, n):
    from test_gpu_g1_ride import xy_bytes
    from test_gpu_h2c_chain import init_gpu
    from drand_amd import _lib
    us, sigs, kinds, ref = debug_reference
    _, lib = init_gpu()
    ub = np.frombuffer(b"".join(u0.to_bytes(48, "big") + u1.to_bytes(48, "big") for u0, u1 in us[:n]), np.uint8).copy()
    sb = np.frombuffer(b"".join(sigs[:n]), np.uint8).copy()
    status = np.zeros(n, np.uint8)
    sig_out = np.zeros((n, 96), np.uint8)
    hash_out = np.zeros((n, 96), np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.dh_g1_round_prep_late_debug(p(ub), p(sb), n, p(status), p(sig_out), p(hash_out)) == 0, _lib.last_error()
    for i in range(n):
        st, sigma, q = ref[i]
        assert int(status[i]) == st, (i, kinds.get(i))
        assert (st == 0) == (i in kinds or i == IDENTITY_UNDER_VALID)
        assert hash_out[i].tobytes() == xy_bytes(q), (i, kinds.get(i))
        assert sig_out[i].tobytes() == xy_bytes(sigma), (i, kinds.get(i))


if __name__ == "__main__":
    run_child(sys.argv[1])
