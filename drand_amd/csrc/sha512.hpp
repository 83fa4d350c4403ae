// SHA-512 (FIPS 180-4) per lane, for the Schnorr challenge of DKGAuthScheme (kyber v1.1.18 sign/schnorr as the
// schemes' DKGAuthScheme, crypto/schemes.go:103,144,184):
//   h = SHA-512(R_bytes || P_bytes || msg)  with R, P the K-byte compressed points as given (K = 48 or 96).
// The message streams from global memory in 128-byte blocks behind the two point encodings; the last
// (2K + len) % 128 bytes and SHA-512's own padding are assembled in registers (one closing block when that
// remainder is <= 111, else two): no scratch row per lane, as sha256.hpp xmd_any. Compiles for the host as well
// (tests/test_schnorr_host.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace dh {

#ifndef DH_DEV
#define DH_DEV __device__ __forceinline__
#endif

__device__ __constant__ uint64_t SHA512_K[80] = {
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull,
    0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull,
    0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull, 0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull,
    0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
    0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull, 0x983e5152ee66dfabull,
    0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
    0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull,
    0x53380d139d95b3dfull, 0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
    0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull,
    0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull, 0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull,
    0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull,
    0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull,
    0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull,
    0x113f9804bef90daeull, 0x1b710b35131c471bull, 0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull,
    0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};

struct sha512_h {
  uint64_t h[8];
};

DH_DEV sha512_h sha512_iv() {
  return {{0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
           0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull}};
}

DH_DEV uint64_t ror64(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

// one compression; w = 16 big-endian message words (consumed)
DH_DEV void sha512_compress(sha512_h& s, uint64_t w[16]) {
  uint64_t a = s.h[0], b = s.h[1], c = s.h[2], d = s.h[3], e = s.h[4], f = s.h[5], g = s.h[6], h = s.h[7];
#pragma unroll
  for (int i = 0; i < 80; i++) {
    uint64_t wi;
    if (i < 16) {
      wi = w[i];
    } else {
      const uint64_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
      const uint64_t s0 = ror64(w15, 1) ^ ror64(w15, 8) ^ (w15 >> 7);
      const uint64_t s1 = ror64(w2, 19) ^ ror64(w2, 61) ^ (w2 >> 6);
      wi = w[i & 15] + s0 + w[(i - 7) & 15] + s1;
      w[i & 15] = wi;
    }
    const uint64_t t1 = h + (ror64(e, 14) ^ ror64(e, 18) ^ ror64(e, 41)) + ((e & f) ^ (~e & g)) + SHA512_K[i] + wi;
    const uint64_t t2 = (ror64(a, 28) ^ ror64(a, 34) ^ ror64(a, 39)) + ((a & b) ^ (a & c) ^ (b & c));
    h = g;
    g = f;
    f = e;
    e = d + t1;
    d = c;
    c = b;
    b = a;
    a = t1 + t2;
  }
  s.h[0] += a; s.h[1] += b; s.h[2] += c; s.h[3] += d;
  s.h[4] += e; s.h[5] += f; s.h[6] += g; s.h[7] += h;
}

// SHA-512(R [K bytes] || P [K bytes] || msg [len bytes]), any alignment. Byte pos of the preimage comes from R, P or
// msg; a block of the stream is 16 words of 8 such bytes. After the nfull = (2K + len) / 128 full blocks the closing
// block(s) hold the remaining rem bytes, 0x80, zeros and the bit length in the last 16 bytes (the high 8 are zero:
// len < 2^32): rem + 1 + 16 <= 128 exactly when rem <= 111.
DH_DEV sha512_h sha512_rpm(const uint8_t* __restrict__ R, const uint8_t* __restrict__ P, uint32_t K,
                           const uint8_t* __restrict__ msg, uint32_t len) {
  const uint64_t total = 2ull * K + len;
  const uint64_t nfull = total >> 7;
  const uint32_t rem = (uint32_t)(total & 127u);
  auto byte_at = [&](uint64_t pos) -> uint64_t {
    if (pos < K) return R[pos];
    if (pos < 2ull * K) return P[pos - K];
    return msg[pos - 2ull * K];
  };
  sha512_h s = sha512_iv();
#pragma unroll 1
  for (uint64_t blk = 0; blk < nfull; blk++) {
    uint64_t w[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      uint64_t v = 0;
#pragma unroll
      for (int b = 0; b < 8; b++) v = (v << 8) | byte_at(blk * 128 + (uint64_t)(8 * j + b));
      w[j] = v;
    }
    sha512_compress(s, w);
  }
  const uint32_t ntail = rem <= 111 ? 1 : 2;
#pragma unroll 1
  for (uint32_t t = 0; t < ntail; t++) {
    uint64_t w[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      uint64_t v = 0;
#pragma unroll
      for (int b = 0; b < 8; b++) {
        const uint32_t pos = t * 128 + (uint32_t)(8 * j + b);
        uint64_t byte = 0;
        if (pos < rem) byte = byte_at(nfull * 128 + pos);
        else if (pos == rem) byte = 0x80u;
        v = (v << 8) | byte;
      }
      if (t == ntail - 1 && j == 15) v = total * 8;
      w[j] = v;
    }
    sha512_compress(s, w);
  }
  return s;
}

}  // namespace dh
