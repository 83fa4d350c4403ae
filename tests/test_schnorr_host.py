"""Host side of the DKGAuthScheme path (dh_schnorr_verify_batch): SHA-512 and the 512-bit reduction mod r compiled for
the host from the kernels' own headers, the fixture tests/golden/schnorr.json against its generator's check, and the
argument errors of the entry that need no device. The device side is tests/test_gpu_schnorr.py."""
import hashlib
import importlib.util
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 200, 1000]

HOST_PRELUDE = r"""
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#define __device__
#define __constant__ static const
#define __forceinline__ inline
#define __restrict__
static inline uint32_t host_addc(uint32_t a, uint32_t b, unsigned c, unsigned* co) {
  const uint64_t s = (uint64_t)a + b + c;
  *co = (unsigned)(s >> 32);
  return (uint32_t)s;
}
static inline uint32_t host_subc(uint32_t a, uint32_t b, unsigned c, unsigned* co) {
  const uint64_t s = (uint64_t)a - b - c;
  *co = (unsigned)(s >> 63);
  return (uint32_t)s;
}
#define __builtin_addc host_addc
#define __builtin_subc host_subc
"""

SHA512_HOST_SRC = HOST_PRELUDE + r"""
#include "sha512.hpp"
// argv: K, length; R byte i = (7 i + K) mod 256, P byte i = (11 i + 3 + len) mod 256, message byte i = (131 i + 7 len + K) mod 256
int main(int argc, char** argv) {
  const int K = atoi(argv[1]), L = atoi(argv[2]);
  uint8_t Rb[96], Pb[96];
  uint8_t* m = (uint8_t*)malloc(L + 1);
  for (int i = 0; i < K; i++) { Rb[i] = (uint8_t)(7 * i + K); Pb[i] = (uint8_t)(11 * i + 3 + L); }
  for (int i = 0; i < L; i++) m[i] = (uint8_t)(i * 131 + 7 * L + K);
  const dh::sha512_h d = dh::sha512_rpm(Rb, Pb, (uint32_t)K, m, (uint32_t)L);
  for (int j = 0; j < 8; j++) printf("%016llx", (unsigned long long)d.h[j]);
  printf("\n");
  free(m);
  return 0;
}
"""

FR_HOST_SRC = HOST_PRELUDE + r"""
#include "fr.hpp"
// stdin: one 128-digit hex number per line (a 512-bit big-endian digest); stdout: its residue mod r, 64 hex digits
int main() {
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    uint32_t d[16], out[8];
    for (int i = 0; i < 16; i++) {
      char w[9];
      memcpy(w, line + 8 * i, 8);
      w[8] = 0;
      d[i] = (uint32_t)strtoul(w, 0, 16);
    }
    dh::fr_from_be512(d, out);
    for (int i = 7; i >= 0; i--) printf("%08x", out[i]);
    printf("\n");
  }
  return 0;
}
"""


def _host_build(tmp_path, name, src):
    (tmp_path / "hip").mkdir(exist_ok=True)
    (tmp_path / "hip" / "hip_runtime.h").write_text("")
    cpp, exe = tmp_path / (name + ".cpp"), tmp_path / name
    cpp.write_text(src)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", str(tmp_path), "-I", os.path.join(ROOT, "drand_amd", "csrc"),
                           str(cpp), "-o", str(exe)])
    return str(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_sha512_host_build(tmp_path):
    """sha512_rpm (drand_amd/csrc/sha512.hpp, the challenge hash of k_schnorr_scalars) compiled for the host from the
    same source: equal to hashlib.sha512(R || P || msg) for both point lengths and every fixture length. The preimage
    is 2K + len bytes: with K = 48 the lengths 15, 16 and 17 sit on the one-or-two-closing-blocks boundary
    ((96 + len) % 128 = 111, 112, 113), 31/32/33 on the end of a block; with K = 96, 47/48/49 and 63/64/65 do."""
    exe = _host_build(tmp_path, "sha512_host", SHA512_HOST_SRC)
    for K in (48, 96):
        for n in LENGTHS + [14, 127, 128, 129, 255, 256, 257]:
            rb = bytes((7 * i + K) & 255 for i in range(K))
            pb = bytes((11 * i + 3 + n) & 255 for i in range(K))
            msg = bytes((131 * i + 7 * n + K) & 255 for i in range(n))
            got = subprocess.run([exe, str(K), str(n)], capture_output=True, text=True, check=True).stdout.strip()
            assert got == hashlib.sha512(rb + pb + msg).hexdigest(), (K, n)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_fr_from_be512_host_build(tmp_path):
    """fr_from_be512 (drand_amd/csrc/fr.hpp) compiled for the host: a 512-bit big-endian integer mod r against Python
    integers, on 1,000 random digests and the edges 0, r - 1, r, 2^256 - 1, 2^512 - 1 (and a few around them)."""
    exe = _host_build(tmp_path, "fr_host", FR_HOST_SRC)
    rng = random.Random(512)
    vals = [0, R_ORDER - 1, R_ORDER, R_ORDER + 1, 2 ** 256 - 1, 2 ** 256, 2 ** 512 - 1, R_ORDER << 256, (R_ORDER << 256) - 1,
            R_ORDER * R_ORDER, 1]
    vals += [rng.getrandbits(512) for _ in range(1000)]
    p = subprocess.run([exe], input="".join("%0128x\n" % v for v in vals), capture_output=True, text=True, check=True)
    got = p.stdout.split()
    assert len(got) == len(vals)
    for v, g in zip(vals, got):
        assert int(g, 16) == v % R_ORDER, hex(v)


def _generator():
    spec = importlib.util.spec_from_file_location("make_schnorr_golden", os.path.join(GOLD, "make_schnorr_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_shape_and_live_reverification():
    """tests/golden/schnorr.json holds, per key group, 96 items under 12 keys with every length and fault class of its
    generator, about half of them valid; eight items per group (the first valid one, then one per fault family) are
    verified again here with oracle/bls_py.py through the generator's own check, so the file cannot drift from it."""
    gen = _generator()
    path = os.path.join(GOLD, "schnorr.json")
    assert os.path.getsize(path) < 300 * 1024
    fx = json.load(open(path))
    assert [g["scheme"] for g in fx["groups"]] == ["pedersen-bls-unchained", "bls-unchained-g1-rfc9380"]
    for gi, g in enumerate(fx["groups"]):
        K = g["key_len"]
        assert K == (48, 96)[gi] and len(g["keys"]) == 12 and len(g["items"]) == 96
        assert g["key_ok"] == [1] * 8 + [0, 0, 0, 1] and g["keys"][11] == g["keys"][0]
        items = g["items"]
        assert sorted({len(it["msg"]) // 2 for it in items}) == LENGTHS
        assert all(len(it["sig"]) == 2 * (K + 32) for it in items)
        assert 40 <= sum(it["verdict"] for it in items) <= 56
        classes = {}
        for it in items:
            classes.setdefault(it["class"], []).append(it)
            assert it["verdict"] == (1 if it["class"] == "valid" else 0)
        assert set(classes) == set(gen.FAULTS) | {"valid"}
        assert all(len(classes[c]) >= 2 for c in gen.FAULTS)
        # s + r really is s + r of a signature that would verify, and s = 0 is all zero
        assert all(int(it["sig"][2 * K:], 16) >= R_ORDER for it in classes["s_plus_r"])
        assert all(int(it["sig"][2 * K:], 16) == 0 for it in classes["s_zero"])
        grp = gen.Group(bool(gi))
        live = [classes["valid"][0]] + [classes[c][0] for c in ("wrong_msg", "wrong_key", "s_plus_1", "s_plus_r", "r_negated",
                                                               "r_torsion", "swap")]
        for it in live:
            v = gen.verify(grp, bytes.fromhex(g["keys"][it["key"]]), bytes.fromhex(it["msg"]), bytes.fromhex(it["sig"]))
            assert v == it["verdict"], it["class"]
        # the s + r item does verify once r is taken off again: the rejection is the range check, nothing else
        it = classes["s_plus_r"][0]
        sig = bytes.fromhex(it["sig"])
        sig = sig[:K] + (int.from_bytes(sig[K:], "big") - R_ORDER).to_bytes(32, "big")
        assert gen.verify(grp, bytes.fromhex(g["keys"][it["key"]]), bytes.fromhex(it["msg"]), sig) == 1


def test_schnorr_argument_errors():
    """The argument checks of dh_schnorr_verify_batch run before any device work, so they hold where there is no
    device: the rules of dh_bls_verify_batch, and dh_schnorr_sig_len = dh_key_len + 32."""
    from drand_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libdrandhip.so is not built (make -C drand_amd)")
    lib = _lib.load()
    E = _lib.DH_EINVAL
    for sid in range(4):
        assert lib.dh_schnorr_sig_len(sid) == lib.dh_key_len(sid) + 32
    assert lib.dh_schnorr_sig_len(0) == 80 and lib.dh_schnorr_sig_len(3) == 128
    assert lib.dh_schnorr_sig_len(4) == E and lib.dh_schnorr_sig_len(-1) == E
    keys = np.zeros(2 * 48, np.uint8)
    sigs = np.zeros(3 * 80, np.uint8)
    msgs = np.zeros(8, np.uint8)
    off = np.array([0, 2, 4, 8], np.uint32)
    verdict = np.full(3, 7, np.uint8)
    p = lambda a: a.ctypes.data  # noqa: E731

    def call(scheme=0, keys_p=p(keys), n_keys=2, kidx=np.array([0, 1, 1], np.uint32), off_=off, stride=80, n=3):
        return lib.dh_schnorr_verify_batch(scheme, keys_p, n_keys, p(kidx) if kidx is not None else None, p(msgs), p(off_),
                                           p(sigs), stride, n, p(verdict), None)

    assert call(scheme=4) == E
    assert call(kidx=np.array([0, 2, 1], np.uint32)) == E and b"key index" in lib.dh_last_error_string()
    assert call(off_=np.array([0, 4, 2, 8], np.uint32)) == E and b"non-decreasing" in lib.dh_last_error_string()
    assert call(kidx=None) == E and b"one key per item" in lib.dh_last_error_string()
    assert call(stride=79) == E and call(stride=48) == E and b"stride" in lib.dh_last_error_string()
    assert call(stride=82) == E  # not a multiple of 4
    assert call(n_keys=0, keys_p=None) == E and b"no keys" in lib.dh_last_error_string()
    assert call(keys_p=None) == E
    assert call(scheme=2, stride=80) == E  # G2 keys: 128-byte signatures
    assert verdict.tolist() == [7, 7, 7]
    # n = 0 is DH_OK, with or without a key table, and writes nothing
    assert lib.dh_schnorr_verify_batch(0, None, 0, None, None, None, None, 80, 0, None, None) == 0
    assert lib.dh_schnorr_verify_batch(3, p(keys), 1, p(np.zeros(1, np.uint32)), None, None, None, 128, 0, None, None) == 0
