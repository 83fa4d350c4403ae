"""Host side of the AuthScheme path (dh_bls_verify_batch and the identity entries): Identity.Hash on the host
(dh_identity_hash_batch, no device) and the known-answer identities of tests/golden/identities.json under the CPU
oracle. The device side is tests/test_gpu_auth.py."""
import hashlib
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SCHEMES = {"pedersen-bls-chained": 48, "pedersen-bls-unchained": 48, "bls-unchained-on-g1": 96,
           "bls-unchained-g1-rfc9380": 96}


def _built_lib():
    from drand_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libdrandhip.so is not built (make -C drand_amd)")
    return _lib


def test_identity_hash_is_blake2b_256():
    """dh_identity_hash_batch == BLAKE2b-256 for 16 random byte strings of each key length (key/keys.go:53-57 hashes
    the marshalled key, whatever point it is), in one call per scheme. Not marked gpu: the entry is host code and must
    run where there is no device."""
    _lib = _built_lib()
    lib = _lib.load()
    rng = random.Random(7)
    for name, kl in SCHEMES.items():
        sid = lib.dh_scheme_from_name(name.encode())
        keys = [bytes(rng.getrandbits(8) for _ in range(kl)) for _ in range(16)]
        tab = np.frombuffer(b"".join(keys), dtype=np.uint8).copy()
        out = np.zeros((16, 32), dtype=np.uint8)
        assert lib.dh_identity_hash_batch(sid, tab.ctypes.data, 16, out.ctypes.data) == 0, _lib.last_error()
        for k, o in zip(keys, out):
            assert o.tobytes() == hashlib.blake2b(k, digest_size=32).digest()
    assert lib.dh_identity_hash_batch(7, None, 0, None) == _lib.DH_EINVAL
    assert lib.dh_identity_hash_batch(0, None, 0, None) == 0


def test_reference_identities_under_the_oracle(oracle):
    """The three identities of the reference's test group verify against msg = BLAKE2b-256(key) (Identity.Hash), and
    each signature fails under the next identity's key."""
    fx = json.load(open(os.path.join(GOLD, "identities.json")))
    nodes = [(bytes.fromhex(x["key"]), bytes.fromhex(x["signature"])) for x in fx["nodes"]]
    assert len(nodes) == 3 and [x["index"] for x in fx["nodes"]] == [0, 1, 2] and len(fx["coefficients"]) == 2
    for i, (key, sig) in enumerate(nodes):
        msg = hashlib.blake2b(key, digest_size=32).digest()
        assert oracle.verify(fx["scheme"], key, msg, sig)
        other = nodes[(i + 1) % 3][0]
        assert not oracle.verify(fx["scheme"], other, msg, sig)
        assert not oracle.verify(fx["scheme"], other, hashlib.blake2b(other, digest_size=32).digest(), sig)


XMD_HOST_SRC = r"""
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#define __device__
#define __constant__ static const
#define __forceinline__ inline
#define __restrict__
#define __builtin_rotateright32(x, n) (((x) >> (n)) | ((x) << (32 - (n))))
#include "sha256.hpp"
// argv: length, dst_id; message byte i = (131 i + 7 len + dst_id) mod 256; prints b_1..b_4 and b_1..b_8 as hex
int main(int argc, char** argv) {
  const int L = atoi(argv[1]), d = atoi(argv[2]);
  uint8_t* m = (uint8_t*)malloc(L + 1);
  for (int i = 0; i < L; i++) m[i] = (uint8_t)(i * 131 + 7 * L + d);
  uint32_t a[4][8], b[8][8];
  dh::xmd_any<4>(a, m, (uint32_t)L, d);
  dh::xmd_any<8>(b, m, (uint32_t)L, d);
  for (int i = 0; i < 4; i++) for (int j = 0; j < 8; j++) printf("%08x", a[i][j]);
  printf(" ");
  for (int i = 0; i < 8; i++) for (int j = 0; j < 8; j++) printf("%08x", b[i][j]);
  printf("\n");
  if (L == 32) {  // the fixed-shape form on the same 32 bytes
    dh::sha_h h;
    for (int j = 0; j < 8; j++) h.h[j] = dh::ld_be32(m + 4 * j);
    uint32_t c[4][8];
    dh::xmd32<4>(c, h, d);
    if (memcmp(a, c, sizeof a)) return 3;
  }
  free(m);
  return 0;
}
"""


def _xmd(msg, dst, nbytes):
    """RFC 9380 5.3.1 expand_message_xmd with SHA-256."""
    dst_prime = dst + bytes([len(dst)])
    b0 = hashlib.sha256(bytes(64) + msg + nbytes.to_bytes(2, "big") + b"\0" + dst_prime).digest()
    out, prev = b"", bytes(32)
    for i in range(1, nbytes // 32 + 1):
        prev = hashlib.sha256(bytes(x ^ y for x, y in zip(b0, prev)) + bytes([i]) + dst_prime).digest()
        out += prev
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_xmd_any_host_build(tmp_path):
    """xmd_any (drand_amd/csrc/sha256.hpp, the batch path's variable-length expand_message_xmd) compiled for the host
    from the same source: equal to hashlib for the test lengths of tests/test_gpu_auth.py and the block boundaries
    around them (b_0's preimage is 111 + len bytes), both DSTs, both output sizes, and to xmd32 at 32 bytes."""
    (tmp_path / "hip").mkdir()
    (tmp_path / "hip" / "hip_runtime.h").write_text("")
    src, exe = tmp_path / "xmd_host.cpp", tmp_path / "xmd_host"
    src.write_text(XMD_HOST_SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", str(tmp_path), "-I", os.path.join(ROOT, "drand_amd", "csrc"),
                           str(src), "-o", str(exe)])
    dsts = [b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_", b"BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_"]
    lengths = [0, 1, 7, 8, 9, 16, 17, 18, 31, 32, 33, 55, 56, 63, 64, 65, 72, 73, 80, 81, 127, 128, 129, 200, 1000]
    for n in lengths:
        for d in (0, 1):
            msg = bytes((131 * i + 7 * n + d) & 255 for i in range(n))
            got = subprocess.run([str(exe), str(n), str(d)], capture_output=True, text=True, check=True).stdout.split()
            assert got == [_xmd(msg, dsts[d], 128).hex(), _xmd(msg, dsts[d], 256).hex()], (n, d)
