"""The fixed-exponent Fp chains on signed 30-bit digits (fp_mul30.hpp, fp.hpp fp_pow_sched) where
tests/test_gpu_h2c_chain.py does not reach them directly:

* the Fp chains inside fp2.hpp (Fp2 inverse, norm square roots and Legendre symbols of the G2 map): dh_hash_to_curve for
  G2 on 70 messages of 0-200 bytes (one full wave and a partial one), point for point against bls_py.hash_to_g2. The
  pure-Python oracle takes 0.4 s a point (an affine scalar product by the 636-bit h_eff), so its 70 points are
  recorded in tests/golden/h2c_g2_fp30.json; tests/test_fp30_h2c_golden.py (CPU) pins the record to the messages
  generated here and re-derives a sample of it with bls_py.hash_to_g2, and regenerates it when run as a script;
* the G1 hash at the single-message and the 64- and 65-message edge sizes (a lone lane, exactly one wave, one wave and
  one lane), against bls_py.hash_to_g1.
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu
N_G2 = 70
SEED_G2 = 3070
GOLDEN_G2 = os.path.join(ROOT, "tests", "golden", "h2c_g2_fp30.json")


def init_gpu():
    import torch
    import drand_amd
    from drand_amd import _lib
    torch.zeros(1, device="cuda")
    lib = _lib.load()
    assert lib.dh_init(0) == 0, _lib.last_error()
    return drand_amd


def messages(seed, n):
    rng = np.random.default_rng(seed)
    lens = ([0, 1, 31, 32, 33, 55, 56, 63, 64, 65, 119, 120, 128, 199, 200] + rng.integers(0, 201, max(n - 15, 0)).tolist())[:n]
    return [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in lens]


@pytest.fixture(scope="module")
def g1_reference():
    """65 messages and their oracle points, computed once; the smaller sizes are prefixes"""
    import bls_py as b
    msgs = messages(3065, 65)
    return msgs, [b.g1_compress(b.hash_to_g1(m, b.DST_G1)) for m in msgs]


def test_hash_to_curve_g2_matches_oracle():
    import bls_py as b
    drand_amd = init_gpu()
    msgs = messages(SEED_G2, N_G2)
    with open(GOLDEN_G2) as f:
        want = json.load(f)
    assert len(msgs) == N_G2 and [m.hex() for m in msgs] == want["messages"]
    got = drand_amd.hash_to_curve(2, msgs, b.DST_G2)
    assert len(got) == N_G2
    for m, c, w in zip(msgs, got, want["hash_to_g2"]):
        assert c.hex() == w, len(m)


@pytest.mark.parametrize("n", [1, 64, 65])
def test_hash_to_curve_g1_edge_sizes(g1_reference, n):
    import bls_py as b
    drand_amd = init_gpu()
    msgs, want = g1_reference
    got = drand_amd.hash_to_curve(1, msgs[:n], b.DST_G1)
    assert got == want[:n]
