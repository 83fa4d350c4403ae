"""The G1 hash's 11-isogeny in its kernel-polynomial form (h2c.hpp iso11_jac: x_num, y_num and h with x_den = h^2,
y_den = h^3; Jacobian image (xn_h, Y yn_h, Z h_h)) through every kernel that evaluates it, against the oracle:

* dh_hash_to_curve for G1 (k_h2c_generic<fp>, 64 lanes a block) at 1, 64, 65 and 300 messages of 0-200 bytes (one
  lane, a full wave, a wave and one lane, a ragged last block), under quicknet's DST and under the G2 DST that the
  legacy bls-unchained-on-g1 scheme hashes to G1 with, point for point against the oracle's hash_to_curve (the C
  oracle: the pure-Python one takes 26 ms a point), a sample of it held to bls_py.hash_to_g1 as well;
* one signed 300-round quicknet chain with six replaced signatures through dh_verify_batch: all 300 rounds (the batch
  path: k_prep_msg_g1, two blocks of 256 with a ragged second one) and its first 64 rounds (the small path:
  k_add_iso_g1_small), verdicts equal to the oracle's round for round. The chain is signed by k_sign_g1, which hashes
  through the same map.

The oracle's points and verdicts are computed once per module; the smaller sizes are prefixes.
"""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu
QUICKNET = "bls-unchained-g1-rfc9380"
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
N = 300
SIZES = (1, 64, 65, 300)
SWAPPED = ((0, 7), (31, 200), (63, 64), (64, 63), (255, 256), (299, 1))  # round index <- another round's signature


def init_gpu():
    import torch
    import drand_amd
    from drand_amd import _lib
    torch.zeros(1, device="cuda")
    lib = _lib.load()
    assert lib.dh_init(0) == 0, _lib.last_error()
    return drand_amd


def messages():
    rng = np.random.default_rng(1112)
    lens = [0, 1, 31, 32, 33, 55, 56, 63, 64, 65, 119, 120, 128, 199, 200] + rng.integers(0, 201, N - 15).tolist()
    return [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in lens]


@pytest.fixture(scope="module")
def g1_reference(oracle):
    import bls_py as b
    msgs = messages()
    want = {name: [oracle.hash_to_curve(False, m, dst) for m in msgs]
            for name, dst in (("quicknet", b.DST_G1), ("legacy", b.DST_G2))}
    for name, dst in (("quicknet", b.DST_G1), ("legacy", b.DST_G2)):
        for i in (0, 64, 299):
            assert want[name][i] == b.g1_compress(b.hash_to_g1(msgs[i], dst))
    return msgs, want


@pytest.mark.parametrize("dst_name", ["quicknet", "legacy"])
@pytest.mark.parametrize("n", SIZES)
def test_hash_to_curve_g1_sizes_and_dsts(g1_reference, n, dst_name):
    import bls_py as b
    drand_amd = init_gpu()
    msgs, want = g1_reference
    got = drand_amd.hash_to_curve(1, msgs[:n], b.DST_G1 if dst_name == "quicknet" else b.DST_G2)
    assert got == want[dst_name][:n]


@pytest.fixture(scope="module")
def chain(oracle):
    """the signed chain with its replaced signatures and the oracle's verdicts"""
    drand_amd = init_gpu()
    s = drand_amd.scheme_from_name(QUICKNET)
    sk = (int.from_bytes(hashlib.sha256(b"iso11-h").digest(), "big") % R_ORDER).to_bytes(32, "big")
    rounds = np.arange(1, N + 1, dtype=np.uint64)
    good = s.sign_beacons(sk, rounds)
    sigs = good.copy()
    for i, j in SWAPPED:
        sigs[i] = good[j]
    pk = s.public_key(sk)
    want, _ = oracle.verify_batch(QUICKNET, pk, rounds, sigs, nthreads=8, want_rand=False)
    want = [bool(x) for x in want]
    assert [i for i, w in enumerate(want) if not w] == sorted(i for i, _ in SWAPPED)
    return s, pk, rounds, sigs, want


@pytest.mark.parametrize("n", [N, 64])
def test_quicknet_verify_batch_and_small_path(chain, n):
    s, pk, rounds, sigs, want = chain
    v, rand = s.verify_beacons(pk, rounds[:n], sigs[:n], seed=12)
    assert [bool(x) for x in v] == want[:n]
    for i in np.flatnonzero(np.asarray(v, bool)):
        assert np.asarray(rand)[i].tobytes() == hashlib.sha256(sigs[i].tobytes()).digest(), i
