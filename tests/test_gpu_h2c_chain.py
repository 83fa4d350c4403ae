"""The fixed-exponent Fp chains (fp.hpp fp28_pow_sched: dictionary schedule, table in per-lane scratch) through the two
kernels they dominate, against the oracle:

* hash: dh_hash_to_curve for G1 on 130 messages of 0-200 bytes (two full waves and a partial one) with quicknet's
  DST, point for point against bls_py.hash_to_g1 (two sqrt_ratio chains per message);
* decode and verify: dh_verify_batch for quicknet on a signed synthetic chain in which 10 signatures are replaced, 5
  by an x whose x^3 + 4 is a non-residue (the square-root chain's reject path) and 5 by another round's signature
  (decodes, fails the pairing check), once on 130 rounds through the fused k_prep_sig<fp> and once on a 320-round copy
  through k_dec_sig_g1_batch (DRANDHIP_SUB_BATCH_MIN=256; the library reads the switch once, so that run is a child
  process: this module as a script). Verdicts must match the oracle round for round and the randomness must be the
  SHA-256 of the signature for every accepted round.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu
QUICKNET = "bls-unchained-g1-rfc9380"
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
N_FUSED, N_BATCH = 130, 320
NON_RESIDUE = (3, 40, 64, 100, 129)
SWAPPED = ((0, 1), (17, 90), (63, 64 + 128), (65, 2), (128, 127))  # round index <- another round's signature


def secret():
    return (int.from_bytes(hashlib.sha256(b"h2c-chain").digest(), "big") % R_ORDER).to_bytes(32, "big")


def non_residue_x(sig_row):
    """The same flags with an x for which x^3 + 4 has no square root."""
    import bls_py as b
    raw = bytearray(sig_row.tobytes())
    x = int.from_bytes(bytes([raw[0] & 0x1F]) + bytes(raw[1:]), "big")
    while b.fsqrt((x * x * x + b.B1) % b.P) is not None:
        x += 1
    out = bytearray(x.to_bytes(48, "big"))
    out[0] |= raw[0] & 0xE0
    return np.frombuffer(bytes(out), np.uint8)


def corrupt(sigs):
    s = sigs.copy()
    for i in NON_RESIDUE:
        s[i] = non_residue_x(sigs[i])
    for i, j in SWAPPED:
        s[i] = sigs[j]
    return s


def chain(s):
    sk = secret()
    rounds = np.arange(1, N_BATCH + 1, dtype=np.uint64)
    return s.public_key(sk), rounds, corrupt(s.sign_beacons(sk, rounds))


def init_gpu():
    import torch
    import drand_amd
    from drand_amd import _lib
    torch.zeros(1, device="cuda")
    lib = _lib.load()
    assert lib.dh_init(0) == 0, _lib.last_error()
    return drand_amd, lib


def run_batched(path):
    """Child process (DRANDHIP_SUB_BATCH_MIN=256): the 320-round chain, with the launch counts of the batched subgroup
    test, which only the k_dec_sig_g1_batch path reaches."""
    from test_gpu_subgroup_batch import profiled_verify
    drand_amd, lib = init_gpu()
    s = drand_amd.scheme_from_name(QUICKNET)
    pk, rounds, sigs = chain(s)
    v, rand, counts = profiled_verify(lib, s, pk, rounds, sigs, 5)
    np.savez(path, v=v, rand=rand, counts=np.array(counts), sigs=sigs, pk=np.frombuffer(pk, np.uint8))


def check(v, rand, sigs, want):
    bad = sorted(NON_RESIDUE + tuple(i for i, _ in SWAPPED))
    assert [bool(x) for x in want] == [bool(x) for x in v]
    assert np.flatnonzero(~np.asarray(v, bool)).tolist() == bad
    for i in np.flatnonzero(np.asarray(v, bool)):
        assert rand[i].tobytes() == hashlib.sha256(sigs[i].tobytes()).digest(), i


def test_hash_to_curve_g1_matches_oracle():
    import bls_py as b
    drand_amd, _ = init_gpu()
    rng = np.random.default_rng(9380)
    lens = [0, 1, 31, 32, 33, 55, 56, 63, 64, 65, 119, 120, 128, 199, 200] + rng.integers(0, 201, N_FUSED - 15).tolist()
    msgs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    assert len(msgs) == N_FUSED
    got = drand_amd.hash_to_curve(1, msgs, b.DST_G1)
    for m, c in zip(msgs, got):
        assert c == b.g1_compress(b.hash_to_g1(m, b.DST_G1)), len(m)


def test_fused_decode_and_verify_match_oracle(oracle):
    drand_amd, _ = init_gpu()
    s = drand_amd.scheme_from_name(QUICKNET)
    pk, rounds, sigs = chain(s)
    rounds, sigs = rounds[:N_FUSED], sigs[:N_FUSED]
    v, rand = s.verify_beacons(pk, rounds, sigs, seed=5)
    want, _ = oracle.verify_batch(QUICKNET, pk, rounds, sigs, nthreads=8, want_rand=False)
    check(v, np.asarray(rand), sigs, want)


def test_batched_decode_and_verify_match_oracle(oracle, tmp_path):
    out = tmp_path / "batched.npz"
    env = {k: v for k, v in os.environ.items() if not k.startswith("DRANDHIP_SUB")}
    env.update(DRANDHIP_SUB_BATCH_MIN="256", DRANDHIP_SUB_BACKOFF="0")
    assert subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, timeout=300).returncode == 0
    r = dict(np.load(str(out)))
    assert r["counts"].tolist() == [1, 0]  # the batched subgroup test ran: the decode was k_dec_sig_g1_batch
    rounds = np.arange(1, N_BATCH + 1, dtype=np.uint64)
    want, _ = oracle.verify_batch(QUICKNET, r["pk"].tobytes(), rounds, r["sigs"], nthreads=8, want_rand=False)
    check(r["v"], r["rand"], r["sigs"], want)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    run_batched(sys.argv[1])
