"""The batched G1 subgroup test through the C ABI: a large local quicknet batch decodes its signatures
without the per-round test, tests the bit-subset sums of its level-0 sigma buckets (k_sub_batch_level0) and falls back
to the exact per-round test (k_sub_exact) when one of them is outside G1. Verdicts must be exactly the per-round ones.

Signatures outside G1 are sigma + T for a valid sigma and a torsion point T of E(Fp) (cofactor h = 3 * 11^2 * 10177^2 *
859267^2 * 52437899^2): T3 = (0, 2), points of order 11 and 10177, and a full random curve point. The q-part of E(Fp)
is Z_q x Z_q for q = 11 and 10177, so [r h / q] of a curve point is the identity; the order-q points here are
[r h / q^2] of a curve point (order checked).

The library reads its switches once per process, and the measured default of DRANDHIP_SUB_BATCH_MIN is 131,072 rounds,
so the cases run in two child processes (this module as a script): one with DRANDHIP_SUB_BATCH_MIN=256 and
DRANDHIP_SUB_BACKOFF=0 (every batch on the batched path, also after a dense fallback), one with
DRANDHIP_SUBGROUP_BATCH=0 (the fused per-round test). Sizes: 300 (c = 6, 11 window rows), 4,096 (c = 11) and 131,072
(c = 16, 32,769 buckets per row: the geometry of the benchmark's batches, and the default minimum). Three explicit RLC
seeds each. The default configuration (131,072 rounds on the batched path, the back-off after a dense fallback) is
checked in this process.
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

pytestmark = pytest.mark.gpu
QUICKNET = "bls-unchained-g1-rfc9380"
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
H_COF = 0x396c8c005555e1568c00aaab0000aaab
SEEDS = (1, 7, 2024)
N_TINY, N_SMALL, N_BENCH = 300, 4096, 131072
SIZES = (N_TINY, N_SMALL, N_BENCH)
POINTS = ("T3", "T11", "T10177", "Trand")
ORACLE_CASES = ("mixed", "half_T3", "one_Trand")


def torsion_points():
    import bls_py as b
    assert H_COF == 3 * 11 ** 2 * 10177 ** 2 * 859267 ** 2 * 52437899 ** 2

    def curve_point(x):
        while True:
            y = b.fsqrt((x * x * x + b.B1) % b.P)
            if y is not None:
                return (x, y)
            x += 1

    def of_order(q, x0):
        x = x0
        while True:
            t = b.ec_mul(b.FP, curve_point(x), R_ORDER * H_COF // (q * q))
            if t is not None:
                assert b.ec_mul(b.FP, t, q) is None
                return t
            x += 1

    t3 = (0, 2)
    assert b.g1_on_curve(t3) and b.ec_mul(b.FP, t3, 3) is None
    full = curve_point(0x1234567)
    assert b.ec_mul(b.FP, full, R_ORDER) is not None
    return {"T3": t3, "T11": of_order(11, 5), "T10177": of_order(10177, 9), "Trand": full}


def add_point(sig_row, T):
    import bls_py as b
    s = b.g1_decompress(sig_row.tobytes(), subgroup_check=False)
    return np.frombuffer(b.g1_compress(b.ec_add(b.FP, s, T)), np.uint8)


def off_curve(sig_row):
    """The same flags with an x that has no y on the curve."""
    import bls_py as b
    raw = bytearray(sig_row.tobytes())
    x = int.from_bytes(bytes([raw[0] & 0x1F]) + bytes(raw[1:]), "big")
    while b.fsqrt((x * x * x + b.B1) % b.P) is not None:
        x += 1
    out = bytearray(x.to_bytes(48, "big"))
    out[0] |= raw[0] & 0xE0
    return np.frombuffer(bytes(out), np.uint8)


def case_names(n):
    return ["clean"] + ["one_" + p for p in POINTS] + ["pm_T3"] + (["half_T3"] if n == N_SMALL else []) + ["mixed"]


def rejected(n, name):
    """The rounds (0-based) a case corrupts: its exact rejected set."""
    if name == "clean":
        return []
    if name.startswith("one_"):
        return [n // 3 + 1]
    if name == "pm_T3":
        return [17, n - 5]
    if name == "half_T3":
        return list(range(0, n, 2))
    if name == "dense_T3":
        return list(range(5, n, n // 80))
    assert name == "mixed"
    return sorted([40, 100, n // 2, n - 1])


def build_case(n, name, sigs, T):
    import bls_py as b
    s = sigs.copy()
    bad = rejected(n, name)
    if name.startswith("one_"):
        s[bad[0]] = add_point(sigs[bad[0]], T[name[4:]])
    elif name == "pm_T3":
        s[bad[0]] = add_point(sigs[bad[0]], T["T3"])
        s[bad[1]] = add_point(sigs[bad[1]], b.ec_neg(b.FP, T["T3"]))
    elif name in ("half_T3", "dense_T3"):
        for i in bad:
            s[i] = add_point(sigs[i], T["T3"])
    elif name == "mixed":
        s[40] = add_point(sigs[40], T["T3"])
        s[100] = sigs[101]  # another round's signature: in G1, wrong message
        s[n // 2] = sigs[7]
        s[n - 1] = off_curve(sigs[n - 1])
    return s


def secret():
    return (int.from_bytes(hashlib.sha256(b"sub-batch").digest(), "big") % R_ORDER).to_bytes(32, "big")


def init_gpu():
    import torch
    import drand_amd
    from drand_amd import _lib
    torch.zeros(1, device="cuda")
    lib = _lib.load()
    assert lib.dh_init(0) == 0, _lib.last_error()
    return drand_amd, lib


def profiled_verify(lib, s, pk, rounds, sigs, seed):
    lib.dh_profile(1)
    v, rand = s.verify_beacons(pk, rounds, sigs, seed=seed)
    buf = ctypes.create_string_buffer(1 << 16)
    lib.dh_profile_read(buf, len(buf))
    lib.dh_profile(0)
    prof = json.loads(buf.value.decode())
    counts = [prof.get(k, {}).get("count", 0) for k in ("k_sub_batch_level0", "k_sub_exact")]
    return np.asarray(v, bool), np.asarray(rand), counts


def run_all(path):
    """Every case of every size and seed -> OUT.npz: verdicts v/, SHA-256 of the randomness r/, the launch counts of
    (k_sub_batch_level0, k_sub_exact) p/, the public key, and the signatures of the cases the oracle re-checks s/."""
    drand_amd, lib = init_gpu()
    s = drand_amd.scheme_from_name(QUICKNET)
    sk = secret()
    pk = s.public_key(sk)
    T = torsion_points()
    arrs = {"pk": np.frombuffer(pk, np.uint8)}
    for n in SIZES:
        rounds = np.arange(1, n + 1, dtype=np.uint64)
        sigs = s.sign_beacons(sk, rounds)
        for name in case_names(n):
            cs = build_case(n, name, sigs, T)
            if n == N_SMALL and name in ORACLE_CASES:
                arrs["s/%s" % name] = cs
            for seed in SEEDS:
                v, rand, counts = profiled_verify(lib, s, pk, rounds, cs, seed)
                tag = "%d/%s/%d" % (n, name, seed)
                arrs["v/" + tag] = v
                arrs["r/" + tag] = np.frombuffer(hashlib.sha256(rand.tobytes()).digest(), np.uint8)
                arrs["p/" + tag] = np.array(counts)
                if seed == SEEDS[0] and name == "mixed":
                    for i in (0, 40, n - 1):
                        assert rand[i].tobytes() == hashlib.sha256(cs[i].tobytes()).digest()
    np.savez(path, **arrs)


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """(batched, fused): the two child processes' outputs, started side by side."""
    d = tmp_path_factory.mktemp("subgroup_batch")
    base = {k: v for k, v in os.environ.items() if not k.startswith("DRANDHIP_SUB")}
    envs = {"batched": dict(base, DRANDHIP_SUB_BATCH_MIN="256", DRANDHIP_SUB_BACKOFF="0"),
            "fused": dict(base, DRANDHIP_SUBGROUP_BATCH="0")}
    procs = {k: subprocess.Popen([sys.executable, os.path.abspath(__file__), str(d / (k + ".npz"))], env=e)
             for k, e in envs.items()}
    for k, p in procs.items():
        assert p.wait(timeout=600) == 0, k
    return tuple(dict(np.load(str(d / (k + ".npz")))) for k in ("batched", "fused"))


def all_tags():
    return [(n, name, seed) for n in SIZES for name in case_names(n) for seed in SEEDS]


def test_clean_chain_takes_batched_test_only(children):
    batched, fused = children
    for n in SIZES:
        for seed in SEEDS:
            tag = "%d/clean/%d" % (n, seed)
            assert batched["v/" + tag].all(), tag
            assert batched["p/" + tag].tolist() == [1, 0], tag  # k_sub_batch_level0 ran, k_sub_exact did not
            assert fused["p/" + tag].tolist() == [0, 0], tag


@pytest.mark.parametrize("point", POINTS)
def test_one_round_outside_subgroup(children, point):
    batched, _ = children
    for n in SIZES:
        for seed in SEEDS:
            tag = "%d/one_%s/%d" % (n, point, seed)
            assert np.flatnonzero(~batched["v/" + tag]).tolist() == rejected(n, "one_" + point), tag
            assert batched["p/" + tag].tolist() == [1, 1], tag  # the batched test failed, the exact test ran


@pytest.mark.parametrize("case", ["pm_T3", "half_T3", "mixed"])
def test_exact_rejected_set(children, case):
    """+T3 and -T3 in two rounds; every second round sigma + T3 (4,096 rounds); one sigma + T3, two wrong-message
    signatures and one off-curve x."""
    batched, _ = children
    for n in SIZES:
        if case not in case_names(n):
            continue
        for seed in SEEDS:
            tag = "%d/%s/%d" % (n, case, seed)
            assert np.flatnonzero(~batched["v/" + tag]).tolist() == rejected(n, case), tag
            assert batched["p/" + tag].tolist() == [1, 1], tag


@pytest.mark.parametrize("case", ORACLE_CASES)
def test_small_size_agrees_with_oracle(children, oracle, case):
    batched, _ = children
    n = N_SMALL
    want, _ = oracle.verify_batch(QUICKNET, batched["pk"].tobytes(), np.arange(1, n + 1, dtype=np.uint64),
                                  batched["s/" + case], nthreads=8, want_rand=False)
    for seed in SEEDS:
        assert batched["v/%d/%s/%d" % (n, case, seed)].tolist() == [bool(x) for x in want], seed


def test_switch_off_gives_identical_outputs(children):
    """DRANDHIP_SUBGROUP_BATCH=0 (the fused per-round test everywhere): every case's verdicts and randomness are the
    same bytes, and no batched test was launched."""
    batched, fused = children
    for n, name, seed in all_tags():
        tag = "%d/%s/%d" % (n, name, seed)
        assert fused["p/" + tag].tolist() == [0, 0], tag
        assert (fused["v/" + tag] == batched["v/" + tag]).all(), tag
        assert fused["r/" + tag].tobytes() == batched["r/" + tag].tobytes(), tag


def test_default_configuration_and_backoff():
    """This process, no switches: 131,072 rounds take the batched test; a sparse fault leaves the next batch on it; a
    dense fallback (more than one flagged round in 2,000) sends the next batch through the fused kernel, with the
    same verdicts."""
    drand_amd, lib = init_gpu()
    s = drand_amd.scheme_from_name(QUICKNET)
    sk = secret()
    pk = s.public_key(sk)
    T = torsion_points()
    n = N_BENCH
    rounds = np.arange(1, n + 1, dtype=np.uint64)
    sigs = s.sign_beacons(sk, rounds)
    s.verify_beacons(pk, rounds, sigs, seed=99)  # a clean batch clears the dense-fault hint earlier modules may have left
    v, _, counts = profiled_verify(lib, s, pk, rounds, sigs, SEEDS[0])
    if counts == [0, 0]:  # a worker still backing off from an earlier module's dense batch: 15 batches at most
        for _ in range(15):
            s.verify_beacons(pk, rounds, sigs, seed=99)
        v, _, counts = profiled_verify(lib, s, pk, rounds, sigs, SEEDS[0])
    assert v.all() and counts == [1, 0]
    one = build_case(n, "one_Trand", sigs, T)
    for seed in SEEDS[:2]:
        v, _, counts = profiled_verify(lib, s, pk, rounds, one, seed)
        assert np.flatnonzero(~v).tolist() == rejected(n, "one_Trand") and counts == [1, 1], seed
    dense = build_case(n, "dense_T3", sigs, T)
    v1, _, c1 = profiled_verify(lib, s, pk, rounds, dense, SEEDS[0])
    v2, _, c2 = profiled_verify(lib, s, pk, rounds, dense, SEEDS[1])
    assert c1 == [1, 1] and c2 == [0, 0]
    assert np.flatnonzero(~v1).tolist() == rejected(n, "dense_T3")
    assert (v1 == v2).all()


if __name__ == "__main__":
    run_all(sys.argv[1])
