"""The dependent-column body of the fixed-exponent Fp chains (fp_mul30.hpp m30::mont_body: the carry of a column is the
addend of the next column's first MAD, the output columns round in pairs) through the kernels that run the chains,
against the oracle. The lockstep form of the body (two operations side by side) is measured by
bench/microbench_fp30.hip and not used by a kernel; the cases are the ones set for it all the same.

* The G1 hash (two square-root chains a message) at 1, 63, 64, 65 and 130 messages of 0-200 bytes (a partial wave, a
  wave less one lane, a full wave, a wave and one lane, two waves and two lanes) under quicknet's DST and under the G2
  DST of the legacy scheme, point for point against the oracle's hash_to_curve.
* One signed 300-round quicknet chain with six replaced signatures through dh_verify_batch, all 300 rounds (the batch
  path) and the first 64 (the small path): verdicts and randomness equal to the oracle's round for round. Five of the
  six are other rounds' signatures; the sixth is a compressed point whose x is not on the curve (x^3 + 4 is not a
  square), which the square-root chain of the decode must reject.
* The G2 hash (its Fp chains run the same body) on the first 5 messages of tests/golden/h2c_g2_fp30.json.

The oracle's points and verdicts are computed once per module; the smaller sizes are prefixes.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu
QUICKNET = "bls-unchained-g1-rfc9380"
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
N_MSG = 130
SIZES = (1, 63, 64, 65, 130)
N = 300
SWAPPED = ((0, 7), (31, 200), (64, 63), (255, 256), (299, 1))  # round index <- another round's signature
OFF_CURVE = 63                                                  # round index <- an x that is not on the curve
GOLDEN_G2 = os.path.join(ROOT, "tests", "golden", "h2c_g2_fp30.json")


def init_gpu():
    import torch
    import drand_amd
    from drand_amd import _lib
    torch.zeros(1, device="cuda")
    lib = _lib.load()
    assert lib.dh_init(0) == 0, _lib.last_error()
    return drand_amd


def messages():
    rng = np.random.default_rng(1419)
    lens = [0, 1, 31, 32, 33, 55, 56, 63, 64, 65, 119, 120, 128, 199, 200] + rng.integers(0, 201, N_MSG - 15).tolist()
    return [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in lens]


@pytest.fixture(scope="module")
def g1_reference(oracle):
    import bls_py as b
    msgs = messages()
    want = {name: [oracle.hash_to_curve(False, m, dst) for m in msgs]
            for name, dst in (("quicknet", b.DST_G1), ("legacy", b.DST_G2))}
    for name, dst in (("quicknet", b.DST_G1), ("legacy", b.DST_G2)):
        assert want[name][N_MSG - 1] == b.g1_compress(b.hash_to_g1(msgs[N_MSG - 1], dst))
    return msgs, want


@pytest.mark.parametrize("dst_name", ["quicknet", "legacy"])
@pytest.mark.parametrize("n", SIZES)
def test_hash_to_curve_g1_sizes_and_dsts(g1_reference, n, dst_name):
    import bls_py as b
    drand_amd = init_gpu()
    msgs, want = g1_reference
    got = drand_amd.hash_to_curve(1, msgs[:n], b.DST_G1 if dst_name == "quicknet" else b.DST_G2)
    assert got == want[dst_name][:n]


def off_curve_signature(sig):
    """the compressed G1 point next to sig whose x has no y: x^3 + 4 is not a square mod p"""
    flags = sig[0] & 0xe0
    x = int.from_bytes(bytes([sig[0] & 0x1f]) + bytes(sig[1:]), "big")
    while True:
        x = (x + 1) % P
        if pow((x * x * x + 4) % P, (P - 1) // 2, P) == P - 1:
            break
    out = bytearray(x.to_bytes(48, "big"))
    out[0] |= flags
    return np.frombuffer(bytes(out), dtype=np.uint8)


@pytest.fixture(scope="module")
def chain(oracle):
    """the signed chain with its replaced signatures and the oracle's verdicts"""
    drand_amd = init_gpu()
    s = drand_amd.scheme_from_name(QUICKNET)
    sk = (int.from_bytes(hashlib.sha256(b"chain-dependent").digest(), "big") % R_ORDER).to_bytes(32, "big")
    rounds = np.arange(1, N + 1, dtype=np.uint64)
    good = s.sign_beacons(sk, rounds)
    sigs = good.copy()
    for i, j in SWAPPED:
        sigs[i] = good[j]
    sigs[OFF_CURVE] = off_curve_signature(good[OFF_CURVE].tobytes())
    pk = s.public_key(sk)
    want, _ = oracle.verify_batch(QUICKNET, pk, rounds, sigs, nthreads=8, want_rand=False)
    want = [bool(x) for x in want]
    assert [i for i, w in enumerate(want) if not w] == sorted([i for i, _ in SWAPPED] + [OFF_CURVE])
    return s, pk, rounds, sigs, want


@pytest.mark.parametrize("n", [N, 64])
def test_quicknet_verify_batch_and_small_path(chain, n):
    s, pk, rounds, sigs, want = chain
    v, rand = s.verify_beacons(pk, rounds[:n], sigs[:n], seed=14)
    assert [bool(x) for x in v] == want[:n]
    assert not v[OFF_CURVE]
    for i in np.flatnonzero(np.asarray(v, bool)):
        assert np.asarray(rand)[i].tobytes() == hashlib.sha256(sigs[i].tobytes()).digest(), i


def test_hash_to_curve_g2_first_golden_messages():
    import bls_py as b
    drand_amd = init_gpu()
    with open(GOLDEN_G2) as f:
        want = json.load(f)
    msgs = [bytes.fromhex(m) for m in want["messages"][:5]]
    got = drand_amd.hash_to_curve(2, msgs, b.DST_G2)
    assert [c.hex() for c in got] == want["hash_to_g2"][:5]
