"""The batched G2 subgroup test through the C ABI: a large local batch of G2 signatures
(pedersen-bls-unchained, pedersen-bls-chained) decodes without k_sub_sig_g2, runs its MSMs on two 63-bit psi halves,
tests the bit-subset sums of its level-0 sigma buckets (k_sub_batch_level0) and falls back to the exact per-round test
(k_sub_exact) when one of them is outside G2. Verdicts must be exactly the per-round ones.

Signatures outside G2 are sigma + T for a valid sigma and a point T of E'(Fp2) outside G2 (cofactor h2 = 13^2 * 23^2 *
2713 * 11953 * 262069 * a 448-bit prime), each built with the Python oracle and its order asserted:
  T13a = (psi - 7) S   an order-13 eigenvector with psi = 11 = -2,
  T13b = (psi - 11) S  an order-13 eigenvector with psi = 7 = 1/2   (S = [r h2 / 169] Q of order 13),
  T23  = [r h2 / 529] Q, of order 23 (psi has no eigenvalue there),
  Trand = a curve point outside G2.
The order-13 eigenvectors carry exactly the small psi ratios for which only the first half of the soundness proof
applies (one k1 per k2).

The library reads its switches once per process, so the cases run in two child processes (this module as a script),
started side by side: one with DRANDHIP_SUB_BATCH_MIN_G2=256 and DRANDHIP_SUB_BACKOFF=0 (every batch on the batched
path, also after a dense fallback), one with DRANDHIP_SUBGROUP_BATCH=0 (the fused per-round test). Sizes: 300 and
4,096 rounds with three RLC seeds, 131,072 rounds (c = 16 window rows, the production geometry) with one. The default
configuration (DEFAULT_MIN_G2 rounds, the back-off after a dense fallback) is checked in this process.
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
UNCHAINED, CHAINED = "pedersen-bls-unchained", "pedersen-bls-chained"
P_MOD = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
U_PARAM = -0xd201000000010000
H2 = (U_PARAM ** 8 - 4 * U_PARAM ** 7 + 5 * U_PARAM ** 6 - 4 * U_PARAM ** 4 + 6 * U_PARAM ** 3 - 4 * U_PARAM ** 2
      - 4 * U_PARAM + 13) // 9
SEEDS = (1, 7, 2024)
N_TINY, N_SMALL, N_BENCH = 300, 4096, 131072
POINTS = ("T13a", "T13b", "T23", "Trand")
ORACLE_CASES = ("mixed", "half_T13a", "one_Trand")
DEFAULT_MIN_G2 = 393216  # the shipped default of DRANDHIP_SUB_BATCH_MIN_G2 (drandhip.cpp SUB_BATCH_MIN_G2_DEFAULT)


def torsion_points():
    import bls_py as b
    F = b.FP2
    xi = (1, 1)
    cx, cy = b.f2inv(b.f2pow(xi, (P_MOD - 1) // 3)), b.f2inv(b.f2pow(xi, (P_MOD - 1) // 2))

    def psi(pt):
        return (b.f2mul(b.f2conj(pt[0]), cx), b.f2mul(b.f2conj(pt[1]), cy))

    def curve_point(x):
        while True:
            y = b.f2sqrt(b.f2add(b.f2mul(b.f2mul(x, x), x), b.B2))
            if y is not None:
                return (x, y)
            x = (x[0] + 1, x[1])

    assert H2 % (169 * 529) == 0
    q = curve_point((5, 1))
    assert b.g2_on_curve(q) and b.ec_mul(F, q, R_ORDER) is not None  # outside G2
    s = b.ec_mul(F, q, R_ORDER * H2 // 169)
    assert s is not None
    if b.ec_mul(F, s, 13) is not None:
        s = b.ec_mul(F, s, 13)
    assert b.ec_mul(F, s, 13) is None
    t13a = b.ec_add(F, psi(s), b.ec_neg(F, b.ec_mul(F, s, 7)))
    t13b = b.ec_add(F, psi(s), b.ec_neg(F, b.ec_mul(F, s, 11)))
    for t, lam in ((t13a, 11), (t13b, 7)):
        assert t is not None and b.ec_mul(F, t, 13) is None and psi(t) == b.ec_mul(F, t, lam)
    t23 = b.ec_mul(F, q, R_ORDER * H2 // 529)
    assert t23 is not None
    if b.ec_mul(F, t23, 23) is not None:
        t23 = b.ec_mul(F, t23, 23)
    assert b.ec_mul(F, t23, 23) is None
    return {"T13a": t13a, "T13b": t13b, "T23": t23, "Trand": q}


def add_point(sig_row, T):
    import bls_py as b
    s = b.g2_decompress(sig_row.tobytes(), subgroup_check=False)
    return np.frombuffer(b.g2_compress(b.ec_add(b.FP2, s, T)), np.uint8)


def off_curve(sig_row):
    """The same flags with an x (c0 stepped) that has no y on the curve. Compressed G2: x.c1 first, then x.c0."""
    import bls_py as b
    raw = bytearray(sig_row.tobytes())
    c1 = int.from_bytes(bytes([raw[0] & 0x1F]) + bytes(raw[1:48]), "big")
    c0 = int.from_bytes(bytes(raw[48:]), "big")
    while True:
        x = (c0, c1)
        if c0 < P_MOD and b.f2sqrt(b.f2add(b.f2mul(b.f2mul(x, x), x), b.B2)) is None:
            break
        c0 = (c0 + 1) % P_MOD
    out = bytearray(c1.to_bytes(48, "big") + c0.to_bytes(48, "big"))
    out[0] |= raw[0] & 0xE0
    return np.frombuffer(bytes(out), np.uint8)


def case_names(n):
    if n == N_BENCH:
        return ["clean", "one_T13a"]
    return ["clean"] + ["one_" + p for p in POINTS] + ["pm_T13a"] + (["half_T13a"] if n == N_SMALL else []) + ["mixed"]


def seeds_of(n):
    return SEEDS[:1] if n == N_BENCH else SEEDS


def rejected(n, name):
    """The rounds (0-based) a case corrupts: its exact rejected set."""
    if name == "clean":
        return []
    if name.startswith("one_"):
        return [n // 3 + 1]
    if name == "pm_T13a":
        return [17, n - 5]
    if name == "half_T13a":
        return list(range(0, n, 2))
    if name == "dense_T13a":
        return list(range(5, n, 80))
    assert name == "mixed"
    return sorted([40, 100, n // 2, n - 1])


def build_case(n, name, sigs, T):
    import bls_py as b
    s = sigs.copy()
    bad = rejected(n, name)
    if name.startswith("one_"):
        s[bad[0]] = add_point(sigs[bad[0]], T[name[4:]])
    elif name == "pm_T13a":
        s[bad[0]] = add_point(sigs[bad[0]], T["T13a"])
        s[bad[1]] = add_point(sigs[bad[1]], b.ec_neg(b.FP2, T["T13a"]))
    elif name in ("half_T13a", "dense_T13a"):
        for i in bad:
            s[i] = add_point(sigs[i], T["T13a"])
    elif name == "mixed":
        s[40] = add_point(sigs[40], T["T13a"])
        s[100] = sigs[101]  # another round's signature: in G2, wrong message
        s[n // 2] = sigs[7]
        s[n - 1] = off_curve(sigs[n - 1])
    return s


def secret():
    return (int.from_bytes(hashlib.sha256(b"sub-batch-g2").digest(), "big") % R_ORDER).to_bytes(32, "big")


def chained_prevs(n):
    """96 arbitrary bytes per round: the chained digest hashes whatever the store holds"""
    return np.random.default_rng(5).integers(0, 256, (n, 96), dtype=np.uint8)


def init_gpu():
    import torch
    import drand_amd
    from drand_amd import _lib
    torch.zeros(1, device="cuda")
    lib = _lib.load()
    assert lib.dh_init(0) == 0, _lib.last_error()
    return drand_amd, lib


def profiled_verify(lib, s, pk, rounds, sigs, seed, prevs=None):
    lib.dh_profile(1)
    v, rand = s.verify_beacons(pk, rounds, sigs, prevs, seed=seed)
    buf = ctypes.create_string_buffer(1 << 16)
    lib.dh_profile_read(buf, len(buf))
    lib.dh_profile(0)
    prof = json.loads(buf.value.decode())
    counts = [prof.get(k, {}).get("count", 0) for k in ("k_sub_batch_level0", "k_sub_exact")]
    return np.asarray(v, bool), np.asarray(rand), counts


def run_all(path):
    """Every case of every size and seed -> OUT.npz: verdicts v/, SHA-256 of the randomness r/, the launch counts of
    (k_sub_batch_level0, k_sub_exact) p/, the public key, and the signatures of the cases the oracle re-checks s/.
    Tags: <scheme letter u|c>/<n>/<case>/<seed>."""
    drand_amd, lib = init_gpu()
    sk = secret()
    T = torsion_points()
    arrs = {}
    plan = [("u", UNCHAINED, n, case_names(n)) for n in (N_TINY, N_SMALL, N_BENCH)] + [("c", CHAINED, N_SMALL, ["clean", "mixed"])]
    for letter, name_s, n, names in plan:
        s = drand_amd.scheme_from_name(name_s)
        pk = s.public_key(sk)
        arrs["pk"] = np.frombuffer(pk, np.uint8)  # one key for both schemes (same secret, same group)
        rounds = np.arange(1, n + 1, dtype=np.uint64)
        prevs = chained_prevs(n) if letter == "c" else None
        sigs = s.sign_beacons(sk, rounds, prevs)
        for name in names:
            cs = build_case(n, name, sigs, T)
            if n == N_SMALL and (name in ORACLE_CASES or letter == "c"):
                arrs["s/%s/%s" % (letter, name)] = cs
            for seed in seeds_of(n):
                v, rand, counts = profiled_verify(lib, s, pk, rounds, cs, seed, prevs)
                tag = "%s/%d/%s/%d" % (letter, n, name, seed)
                arrs["v/" + tag] = v
                arrs["r/" + tag] = np.frombuffer(hashlib.sha256(rand.tobytes()).digest(), np.uint8)
                arrs["p/" + tag] = np.array(counts)
                if seed == SEEDS[0] and name == "mixed":
                    for i in (0, 40, n - 1):
                        assert rand[i].tobytes() == hashlib.sha256(cs[i].tobytes()).digest()
    np.savez(path, **arrs)


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """(batched, fused): the two child processes' outputs, started side by side, each under its own time limit."""
    d = tmp_path_factory.mktemp("subgroup_batch_g2")
    base = {k: v for k, v in os.environ.items() if not k.startswith("DRANDHIP_SUB")}
    envs = {"batched": dict(base, DRANDHIP_SUB_BATCH_MIN_G2="256", DRANDHIP_SUB_BACKOFF="0"),
            "fused": dict(base, DRANDHIP_SUBGROUP_BATCH="0")}
    procs = {k: subprocess.Popen(["timeout", "-k", "10", "600", sys.executable, os.path.abspath(__file__),
                                  str(d / (k + ".npz"))], env=e)
             for k, e in envs.items()}
    for k, p in procs.items():
        assert p.wait(timeout=700) == 0, k
    return tuple(dict(np.load(str(d / (k + ".npz")))) for k in ("batched", "fused"))


def all_tags():
    tags = [("u", n, name, seed) for n in (N_TINY, N_SMALL, N_BENCH) for name in case_names(n) for seed in seeds_of(n)]
    return tags + [("c", N_SMALL, name, seed) for name in ("clean", "mixed") for seed in SEEDS]


def tag_of(letter, n, name, seed):
    return "%s/%d/%s/%d" % (letter, n, name, seed)


def test_clean_chain_takes_batched_test_only(children):
    """Fails without the feature: there G2 signatures never launch the batched test."""
    batched, fused = children
    for letter, n, name, seed in all_tags():
        if name != "clean":
            continue
        tag = tag_of(letter, n, name, seed)
        assert batched["v/" + tag].all(), tag
        assert batched["p/" + tag].tolist() == [1, 0], tag  # k_sub_batch_level0 ran, k_sub_exact did not
        assert fused["p/" + tag].tolist() == [0, 0], tag


@pytest.mark.parametrize("point", POINTS)
def test_one_round_outside_subgroup(children, point):
    batched, _ = children
    for n in (N_TINY, N_SMALL, N_BENCH):
        if "one_" + point not in case_names(n):
            continue
        for seed in seeds_of(n):
            tag = tag_of("u", n, "one_" + point, seed)
            assert np.flatnonzero(~batched["v/" + tag]).tolist() == rejected(n, "one_" + point), tag
            assert batched["p/" + tag].tolist() == [1, 1], tag  # the batched test failed, the exact test ran


@pytest.mark.parametrize("case", ["pm_T13a", "half_T13a", "mixed"])
def test_exact_rejected_set(children, case):
    """+T13a and -T13a in two rounds; every second round sigma + T13a (4,096 rounds); one sigma + T13a, two
    wrong-message signatures and one off-curve x."""
    batched, _ = children
    for n in (N_TINY, N_SMALL):
        if case not in case_names(n):
            continue
        for seed in SEEDS:
            tag = tag_of("u", n, case, seed)
            assert np.flatnonzero(~batched["v/" + tag]).tolist() == rejected(n, case), tag
            assert batched["p/" + tag].tolist() == [1, 1], tag


def test_chained_with_previous_signatures(children):
    batched, _ = children
    for seed in SEEDS:
        tag = tag_of("c", N_SMALL, "mixed", seed)
        assert np.flatnonzero(~batched["v/" + tag]).tolist() == rejected(N_SMALL, "mixed"), tag
        assert batched["p/" + tag].tolist() == [1, 1], tag


@pytest.mark.parametrize("case", ORACLE_CASES)
def test_small_size_agrees_with_oracle(children, oracle, case):
    batched, _ = children
    n = N_SMALL
    want, _ = oracle.verify_batch(UNCHAINED, batched["pk"].tobytes(), np.arange(1, n + 1, dtype=np.uint64),
                                  batched["s/u/" + case], nthreads=8, want_rand=False)
    for seed in SEEDS:
        assert batched["v/" + tag_of("u", n, case, seed)].tolist() == [bool(x) for x in want], seed


def test_chained_mixed_agrees_with_oracle(children, oracle):
    batched, _ = children
    n = N_SMALL
    want, _ = oracle.verify_batch(CHAINED, batched["pk"].tobytes(), np.arange(1, n + 1, dtype=np.uint64),
                                  batched["s/c/mixed"], prevs=chained_prevs(n), nthreads=8, want_rand=False)
    for seed in SEEDS:
        assert batched["v/" + tag_of("c", n, "mixed", seed)].tolist() == [bool(x) for x in want], seed


def test_switch_off_gives_identical_outputs(children):
    """DRANDHIP_SUBGROUP_BATCH=0 (the fused per-round test everywhere): every case's verdicts and randomness are the
    same bytes, and no batched test was launched."""
    batched, fused = children
    for letter, n, name, seed in all_tags():
        tag = tag_of(letter, n, name, seed)
        assert fused["p/" + tag].tolist() == [0, 0], tag
        assert (fused["v/" + tag] == batched["v/" + tag]).all(), tag
        assert fused["r/" + tag].tobytes() == batched["r/" + tag].tobytes(), tag


def test_default_configuration_and_backoff():
    """This process, no switches: a clean batch of the shipped default size takes the batched test; a dense fallback
    (one bad round in 80: more than one flagged round in 2,000) sends the next batch through the fused kernel, with
    the same verdicts."""
    drand_amd, lib = init_gpu()
    s = drand_amd.scheme_from_name(UNCHAINED)
    sk = secret()
    pk = s.public_key(sk)
    T = torsion_points()
    n = DEFAULT_MIN_G2
    rounds = np.arange(1, n + 1, dtype=np.uint64)
    sigs = s.sign_beacons(sk, rounds)
    s.verify_beacons(pk, rounds, sigs, seed=99)  # a clean batch clears the dense-fault hint earlier modules may have left
    v, _, counts = profiled_verify(lib, s, pk, rounds, sigs, SEEDS[0])
    if counts == [0, 0]:  # a worker still backing off from an earlier module's dense batch: 15 batches at most
        for _ in range(15):
            s.verify_beacons(pk, rounds, sigs, seed=99)
        v, _, counts = profiled_verify(lib, s, pk, rounds, sigs, SEEDS[0])
    assert v.all() and counts == [1, 0]
    dense = build_case(n, "dense_T13a", sigs, T)
    v1, _, c1 = profiled_verify(lib, s, pk, rounds, dense, SEEDS[0])
    v2, _, c2 = profiled_verify(lib, s, pk, rounds, dense, SEEDS[1])
    assert c1 == [1, 1] and c2 == [0, 0]
    assert np.flatnonzero(~v1).tolist() == rejected(n, "dense_T13a")
    assert (v1 == v2).all()


if __name__ == "__main__":
    run_all(sys.argv[1])
