"""GPU: the per-round kernel of a large local G1-signature batch (k_prep.hip k_round_g1_ride: the signature decode's
square-root chain carries the inverse that makes the hash point's sum affine), behind DRANDHIP_G1_RIDE.

* verify: a signed 320-round quicknet chain (a full 256-lane block and a ragged one) and a 300-round
  bls-unchained-on-g1 chain, each with 14 replaced signatures: five x whose x^3 + 4 is a non-residue, five other
  rounds' signatures, and one each of compression bit clear, the infinity encoding, the infinity flag with a stray bit
  and x >= p. Through verify_beacons in child processes (the library reads its switches once) with
  DRANDHIP_SUB_BATCH_MIN=256 DRANDHIP_SUB_BACKOFF=0 and DRANDHIP_G1_RIDE 1 and 0: verdicts equal to the oracle's round
  for round and equal between the two settings, randomness the SHA-256 of the signature for accepted rounds, and
  the launch counts: the batched subgroup test ran once and its exact fallback never, the one-launch form reports
  under k_prep_msg<fp> alone and the previous form under both stage names.
* debug entry: dh_g1_round_prep_debug on 1, 64, 65 and 300 rounds (prefixes of one input set): the hash point of
  every round against the integer model (tests/g1_ride_model.py), every rejected signature class included, sigma
  against bls_py for the valid ones, zeros for the rejected ones; lane 6 has u1 = u0 (the doubling) and lane 7
  u1 = -u0 (the identity), which no hashed input reaches.
  A round whose sum lands in the isogeny's kernel is not included: it needs the SSWU map inverted for a chosen point,
  which the model has no cheap way to do (tests/test_iso11_h_model.py covers the kernel point on the isogeny alone).
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
NON_RESIDUE = (3, 40, 64, 100, 129)
SWAPPED = ((0, 1), (17, 90), (63, 64 + 128), (65, 2), (128, 127))  # round index <- another round's signature
CLASSES = ((5, "compression bit clear"), (66, "infinity"), (130, "infinity with a stray bit"), (299, "x >= p"))
STAGES = ("k_sub_batch_level0", "k_sub_exact", "k_prep_sig<fp>", "k_prep_msg<fp>")
DEBUG_SIZES = (1, 64, 65, 300)


def corrupt(sigs):
    from test_g1_ride_model import rejected_encodings
    from test_gpu_h2c_chain import non_residue_x
    s = sigs.copy()
    for i in NON_RESIDUE:
        s[i] = non_residue_x(sigs[i])
    for i, j in SWAPPED:
        s[i] = sigs[j]
    for i, name in CLASSES:
        s[i] = np.frombuffer(rejected_encodings(sigs[i].tobytes())[name], np.uint8)
    return s


BAD = sorted(NON_RESIDUE + tuple(i for i, _ in SWAPPED) + tuple(i for i, _ in CLASSES))


def run_child(path):
    """Child process: both chains through verify_beacons with the stage launch counts."""
    from test_gpu_h2c_chain import init_gpu, secret
    drand_amd, lib = init_gpu()
    out = {}
    for name, n in CHAINS:
        s = drand_amd.scheme_from_name(name)
        sk = secret()
        rounds = np.arange(1, n + 1, dtype=np.uint64)
        sigs = corrupt(s.sign_beacons(sk, rounds))
        lib.dh_profile(1)
        v, rand = s.verify_beacons(s.public_key(sk), rounds, sigs, seed=5)
        buf = ctypes.create_string_buffer(1 << 16)
        lib.dh_profile_read(buf, len(buf))
        lib.dh_profile(0)
        prof = json.loads(buf.value.decode())
        out[name + "/v"] = np.asarray(v, bool)
        out[name + "/rand"] = np.asarray(rand)
        out[name + "/sigs"] = sigs
        out[name + "/pk"] = np.frombuffer(s.public_key(sk), np.uint8)
        out[name + "/counts"] = np.array([prof.get(k, {}).get("count", 0) for k in STAGES])
    np.savez(path, **out)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("g1_ride")
    res = {}
    for ride in ("1", "0"):
        out = d / ("ride%s.npz" % ride)
        env = {k: v for k, v in os.environ.items() if not k.startswith("DRANDHIP_SUB") and k != "DRANDHIP_G1_RIDE"}
        env.update(DRANDHIP_SUB_BATCH_MIN="256", DRANDHIP_SUB_BACKOFF="0", DRANDHIP_G1_RIDE=ride)
        assert subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, timeout=300).returncode == 0
        res[ride] = dict(np.load(str(out)))
    return res


@pytest.mark.parametrize("name,n", CHAINS)
def test_verify_matches_oracle_with_and_without_the_ride(oracle, runs, name, n):
    on, off = runs["1"], runs["0"]
    sigs = on[name + "/sigs"]
    assert np.array_equal(sigs, off[name + "/sigs"]) and len(sigs) == n
    rounds = np.arange(1, n + 1, dtype=np.uint64)
    want, _ = oracle.verify_batch(name, on[name + "/pk"].tobytes(), rounds, sigs, nthreads=8, want_rand=False)
    for r in (on, off):
        v = r[name + "/v"]
        assert [bool(x) for x in want] == [bool(x) for x in v]
        assert np.flatnonzero(~v).tolist() == BAD
        for i in np.flatnonzero(v):
            assert r[name + "/rand"][i].tobytes() == hashlib.sha256(sigs[i].tobytes()).digest(), i
    assert np.array_equal(on[name + "/v"], off[name + "/v"])
    # the batched subgroup test ran (once, no exact fallback); one launch under the hash's stage name, or the two
    assert on[name + "/counts"].tolist() == [1, 0, 0, 1]
    assert off[name + "/counts"].tolist() == [1, 0, 1, 1]


# ---------------------------------------------------------------- the debug entry

def debug_inputs():
    """300 rounds: (u0, u1) and signatures, with the special lanes of the module docstring."""
    import random
    import bls_py as B
    from test_g1_ride_model import non_residue, rejected_encodings
    rng = random.Random(3001)
    n = DEBUG_SIZES[-1]
    us = [(rng.randrange(B.P), rng.randrange(B.P)) for _ in range(n)]
    us[6] = (us[6][0], us[6][0])
    us[7] = (us[7][0], (B.P - us[7][0]) % B.P)
    us[8] = (0, 0)
    pt, sigs = None, []
    for i in range(n):
        pt = B.ec_add(B.FP, pt, B.G1_GEN)
        sigs.append(B.g1_compress(pt if i % 3 else B.ec_neg(B.FP, pt)))
    kinds = {}
    for i, name in ((2, "compression bit clear"), (3, "infinity"), (4, "infinity with a stray bit"), (5, "x >= p"),
                    (70, "infinity"), (299, "x >= p")):
        sigs[i] = rejected_encodings(sigs[i])[name]
        kinds[i] = name
    for i in (1, 7, 64, 200):
        sigs[i] = non_residue(sigs[i])
        kinds[i] = "non-residue"
    return us, sigs, kinds


@pytest.fixture(scope="module")
def debug_reference():
    import bls_py as B
    import g1_ride_model as M
    import iso11_h_model as H
    us, sigs, kinds = debug_inputs()
    h = H.monic_sqrt(B.ISO11_XDEN)
    xnum, ynum = [c % B.P for c in B.ISO11_XNUM], [c % B.P for c in B.ISO11_YNUM]
    ref = [M.hash_point(u0, u1, xnum, ynum, h, sig) for (u0, u1), sig in zip(us, sigs)]
    assert ref[6][2] is not None and ref[7][2] is None
    return us, sigs, kinds, ref


def xy_bytes(pt):
    return bytes(96) if pt is None else pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")


@pytest.mark.parametrize("n", DEBUG_SIZES)
def test_debug_entry_matches_model(debug_reference, n):
    import bls_py as B
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
    assert lib.dh_g1_round_prep_debug(p(ub), p(sb), n, p(status), p(sig_out), p(hash_out)) == 0, _lib.last_error()
    for i in range(n):
        st, sigma, q = ref[i]
        assert int(status[i]) == st, (i, kinds.get(i))
        assert (st == 0) == (i in kinds)
        assert hash_out[i].tobytes() == xy_bytes(q), (i, kinds.get(i))
        assert sig_out[i].tobytes() == xy_bytes(sigma), (i, kinds.get(i))
        if st:
            assert sigma == B.g1_decompress(sigs[i], subgroup_check=False)


if __name__ == "__main__":
    run_child(sys.argv[1])
