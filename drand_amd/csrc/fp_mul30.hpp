// Fp Montgomery product and squaring on 13 SIGNED 30-bit digits, and the fixed-exponent chains that run on them.
//
// A value is sum d[i] 2^(30 i) with centred digits d[0..11] in [-2^29, 2^29) and a small top digit d[12]
// (|d[12]| < 2^20 for the chain's values, |value| < 0.51 p); the Montgomery radix is R' = 2^390. p is held in the same
// centred digits. Against fp_mul28.hpp (14 unsigned 28-bit limbs, 392 MADs a product, 301 a squaring) the same
// product-scanning reduction takes 13 x 13 + 13 x 13 = 338 MADs (v_mad_i64_i32) for a product and 91 + 169 = 260 for
// a squaring. Unsigned 30-bit digits would not fit: 26 terms of 2^60 overflow the 64-bit column accumulator.
// Centred, every term is <= 2^58 in magnitude, so a column of at most 13 + 13 terms plus the carry-in (< 2^34) stays
// below 1.63 * 2^62 < 2^63, and the rounding bias of the output columns (2^29 + 2^59, see mont_body) fits on top
// (tests/fp30_dep_model.py restates the body on Python integers in its accumulation order and asserts the bound at
// every accumulation, the all-digits-at--2^29 operands included; tests/fp30_model.py is the body it replaced, column
// sums from zero and one rounding add per column, which it must equal digit for digit).
//
// mont_mul(X, Y) = (X Y + m p) / 2^390 with m the centred quotient, |m| <= 2^389 (1 + 2^-30): for |X|, |Y| < 0.51 p
// the result is within |X Y| / 2^390 + p / 2 + eps < 0.5006 p (p / 2^390 < 2^-9), so the chain needs no final
// subtraction and its values never grow. The quotient columns shift exactly (acc + Mq[k] p[0] = 0 mod 2^30); the
// output columns round to the nearest digit, R = sext30(acc), carry = (acc + 2^29) >> 30 (an arithmetic shift; the
// body adds the 2^29 of two columns at once).
//
// Entry (from): the 12 x 32-bit Montgomery value x 2^384 (< 2^384) is cut into 30-bit slices, which are recentred by a
// carry pass BEFORE the conversion product (unsigned slices against a centred constant reach 13 (2^59 + 2^58)
// > 2^63), then one product with 2^396 mod p gives x 2^390. Exit (to): one product with 2^384 mod p gives x 2^384
// in (-0.51 p, 0.51 p); p is added where it is negative, the carries are propagated to unsigned digits and the
// digits joined to 12 words, canonical (< p).
//
// Branch-free throughout (fp_inv of the signing helpers runs through this path). Plain integer code behind one
// qualifier macro: the library compiles it for the device, tests/test_fp30_host.py compiles the same source for the
// host (also with -fsanitize=signed-integer-overflow,shift) and checks the chains against pow(x, e, p). Digits are
// doubled by addition: a left shift of a negative value is undefined in C++17.
#pragma once
#include <stdint.h>

#ifndef DH_HD
#define DH_HD __device__ __forceinline__
#endif
#ifndef DH_COUNT_PROD
#define DH_COUNT_PROD() ((void)0)
#endif

namespace dh {
namespace m30 {
constexpr int N = 13;
constexpr uint32_t MASK = 0x3fffffffu;
constexpr uint32_t N0 = 0x3ffcfffdu;  // -p^-1 mod 2^30

struct el {
  int32_t l[N];
};

// The constants below are derived in tests/fp30_model.py (centred(v): digit = v mod 2^30 taken in [-2^29, 2^29),
// v = (v - digit) / 2^30, twelve times; the rest is the top digit) and pinned against this text by
// tests/test_fp30_model.py.
// p
DH_HD int32_t P(int i) {
  const int32_t t[N] = {-21845, -402915328, 356515836, -352321620, -252304353, 55215067, 288093811,
                        316751073, -321428361, 517541167, -375082566, -91332614, 1704210};
  return t[i];
}
// 2^396 mod p: x 2^384 -> x 2^390
DH_HD int32_t K_IN(int i) {
  const int32_t t[N] = {-192885889, -32767999, -532500185, -13403472, -35343150, 503405810, 6050829,
                        -194530918, -181768796, 433626394, -273043482, -129447912, 620336};
  return t[i];
}
// 2^384 mod p: x 2^390 -> x 2^384
DH_HD int32_t K_OUT(int i) {
  const int32_t t[N] = {196605, 405012480, 12582951, -50330895, 123255532, -496935601, -445360651,
                        370465813, -328370226, -362903204, 154517618, -251748295, 1439327};
  return t[i];
}

// the low 30 bits of v as a signed value in [-2^29, 2^29)
DH_HD int32_t sext30(uint32_t v) { return (int32_t)(v << 2) >> 2; }

// Pins the running column sums of the L lockstep operations on the device, after every MAD. Left to itself the
// optimiser reassociates a column: it sums the products from zero and adds the carry of the column below afterwards,
// one more 64-bit add per column (25 a body). A second use of every partial sum keeps the sum in source order, so the
// carry is the addend of the column's first v_mad_i64_i32. One asm reads the sums of both operations, which also holds
// the two MAD chains in lockstep (the scheduler otherwise runs twenty MADs of one chain, then twenty of the other).
// The asm is empty and only reads. An asm that also wrote the sum ("+v") would pin as well, but the compiler then
// guards every MAD that follows one with an s_nop (it must assume the asm's result needs a wait state), 242 a
// squaring, and the body measured slower than the one it replaces (profiles/r14/microbench_fp30_dep.txt). A no-op on
// the host.
template <int L>
DH_HD void pin(const int64_t acc[L]) {
#if defined(__AMDGCN__)
  if (L == 1)
    asm volatile("" ::"v"(acc[0]));
  else
    asm volatile("" ::"v"(acc[0]), "v"(acc[L - 1]));
#else
  (void)acc;
#endif
}

// Product-scanning Montgomery reduction of L independent operations in lockstep: every step of the body is written
// once per operation, side by side, so a wave carries L independent MAD chains. The chains run L = 1. L = 2 (a pair
// of chains walking one schedule, as the two square roots of the G1 hash could) is what bench/microbench_fp30.hip
// measures beside it; it did not beat L = 1 there or in the hash kernel, so no kernel uses it.
// SQ: the squaring, the off-diagonal products once against the doubled digits (in
// [-2^30, 2^30)), 91 products instead of 169; Y is not read. R[l] may be X[l] or Y[l] (column k reads digits
// >= k - 12 and writes digit k - 13).
// The columns are dependent: column k + 1 starts on acc >> 30 of column k, with no separate carry add. The output
// columns N .. 2N - 2 round in pairs. The first of a pair holds the true sum: its digit is sext30(acc), and
// (acc + 2^29 + 2^59) >> 30 is the rounded carry plus 2^29. The second then holds true + 2^29: its digit is
// sext30(acc ^ 2^29) and its plain shift is the rounded carry. That is one 64-bit add per two columns, and the bias
// keeps |acc| < 1.63 * 2^62 + 2^59 (tests/fp30_dep_model.py restates this body and asserts it).
constexpr int64_t BIAS = ((int64_t)1 << 29) + ((int64_t)1 << 59);
// one MAD of every operation l, A and B being expressions in l
#define M30_MAD(A, B)                                                             \
  {                                                                               \
    _Pragma("unroll") for (int l = 0; l < L; l++) acc[l] += (int64_t)(A) * (B);   \
    pin<L>(acc);                                                                  \
  }
template <int L, bool SQ>
DH_HD void mont_body(int32_t* const R[L], const int32_t* const X[L], const int32_t* const Y[L]) {
  int32_t X2[L][N], Mq[L][N];
  int64_t acc[L];
#pragma unroll
  for (int l = 0; l < L; l++) {
    acc[l] = 0;
#pragma unroll
    for (int i = 0; i < N; i++) X2[l][i] = SQ ? X[l][i] + X[l][i] : 0;
  }
#pragma unroll
  for (int k = 0; k < 2 * N - 1; k++) {
    const int lo = k > N - 1 ? k - (N - 1) : 0, hi = k < N - 1 ? k : N - 1;
    if (SQ) {
#pragma unroll
      for (int i = lo; 2 * i < k; i++) M30_MAD(X[l][i], X2[l][k - i])
      if ((k & 1) == 0) M30_MAD(X[l][k / 2], X[l][k / 2])
    } else {
#pragma unroll
      for (int i = lo; i <= hi; i++) M30_MAD(X[l][i], Y[l][k - i])
    }
    if (k < N) {  // a quotient column: shifts exactly
#pragma unroll
      for (int i = 0; i < k; i++) M30_MAD(Mq[l][i], P(k - i))
#pragma unroll
      for (int l = 0; l < L; l++) Mq[l][k] = sext30((uint32_t)acc[l] * N0);
      M30_MAD(Mq[l][k], P(0))
#pragma unroll
      for (int l = 0; l < L; l++) acc[l] >>= 30;
    } else {  // an output column
#pragma unroll
      for (int i = k - (N - 1); i < N; i++) M30_MAD(Mq[l][i], P(k - i))
#pragma unroll
      for (int l = 0; l < L; l++) {
        if ((k - N) % 2 == 0) {
          R[l][k - N] = sext30((uint32_t)acc[l]);
          acc[l] = (acc[l] + BIAS) >> 30;
        } else {
          R[l][k - N] = sext30((uint32_t)acc[l] ^ (1u << 29));
          acc[l] >>= 30;
        }
      }
    }
  }
#pragma unroll
  for (int l = 0; l < L; l++) R[l][N - 1] = (int32_t)acc[l];
}
#undef M30_MAD

// R = X Y / 2^390 (mod p), |R| <= |X Y| / 2^390 + p / 2
DH_HD void mont_mul(int32_t R[N], const int32_t X[N], const int32_t Y[N]) {
  int32_t* const r[1] = {R};
  const int32_t* const x[1] = {X};
  const int32_t* const y[1] = {Y};
  mont_body<1, false>(r, x, y);
}

// R = X^2 / 2^390
DH_HD void mont_sqr(int32_t R[N], const int32_t X[N]) {
  int32_t* const r[1] = {R};
  const int32_t* const x[1] = {X};
  mont_body<1, true>(r, x, x);
}

// (R0, R1) = (X0 Y0, X1 Y1) / 2^390 and (X0^2, X1^2) / 2^390, the two in lockstep
DH_HD void mont_mul2(int32_t R0[N], int32_t R1[N], const int32_t X0[N], const int32_t X1[N], const int32_t Y0[N],
                     const int32_t Y1[N]) {
  int32_t* const r[2] = {R0, R1};
  const int32_t* const x[2] = {X0, X1};
  const int32_t* const y[2] = {Y0, Y1};
  mont_body<2, false>(r, x, y);
}
DH_HD void mont_sqr2(int32_t R0[N], int32_t R1[N], const int32_t X0[N], const int32_t X1[N]) {
  int32_t* const r[2] = {R0, R1};
  const int32_t* const x[2] = {X0, X1};
  mont_body<2, true>(r, x, x);
}

DH_HD el mul(const el& a, const el& b) {
  DH_COUNT_PROD();
  el r;
  mont_mul(r.l, a.l, b.l);
  return r;
}
DH_HD el sqr(const el& a) {
  DH_COUNT_PROD();
  el r;
  mont_sqr(r.l, a.l);
  return r;
}

// An empty asm on the device pins the digits as the 32-bit values they are: the table-build loop multiplies by the
// loop-invariant x^2, whose sign extensions to 64 bits the optimiser otherwise hoists out of the loop, after which
// every product of the loop is expanded into 64 x 32-bit pieces (958 VALU instructions where the same product
// elsewhere takes 445); a no-op on the host
DH_HD void opaque(el& a) {
#if defined(__AMDGCN__)
#pragma unroll
  for (int i = 0; i < N; i++) asm volatile("" : "+v"(a.l[i]));
#else
  (void)a;
#endif
}

// 12 x 32-bit words (any value < 2^384) -> the same value in centred digits: digit i = bits [30 i, 30 i + 30) plus
// the carry of the digit below, less 2^30 (and a carry up) where that is >= 2^29; the top digit keeps its carry
DH_HD void slice(int32_t L[N], const uint32_t x[12]) {
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    const int b = 30 * i, w = b >> 5, o = b & 31;
    const uint64_t two = (uint64_t)x[w] | ((w + 1 < 12) ? ((uint64_t)x[w + 1] << 32) : 0);
    const uint32_t t = ((uint32_t)(two >> o) & MASK) + c;  // <= 2^30
    c = (i < N - 1) ? (t + (1u << 29)) >> 30 : 0;
    L[i] = (int32_t)t - (int32_t)(c << 30);
  }
}

// centred digits of a value in (-p, p) -> its residue in [0, p) as 12 x 32-bit words
DH_HD void unslice(uint32_t r[12], const int32_t A[N]) {
  // the sign: the carry out of the top digit is floor(value / 2^390), -1 or 0
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < N; i++) c = (A[i] + c) >> 30;
  const int32_t neg = c;
  // + p where negative, carries propagated to unsigned digits (each sum is within (-2^30 - 2, 2^30))
  uint32_t U[N];
  c = 0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    const int32_t t = A[i] + (P(i) & neg) + c;
    U[i] = (uint32_t)t & MASK;
    c = t >> 30;
  }
#pragma unroll
  for (int j = 0; j < 12; j++) {
    const int b = 32 * j, i = b / 30, o = b % 30;
    uint64_t v = (uint64_t)U[i] >> o;
    if (i + 1 < N) v |= (uint64_t)U[i + 1] << (30 - o);
    if (i + 2 < N && 60 - o < 32) v |= (uint64_t)U[i + 2] << (60 - o);
    r[j] = (uint32_t)v;
  }
}

// x 2^384 (12 words, < 2^384) -> x 2^390 in the chain's form
DH_HD el from(const uint32_t x[12]) {
  el a, k;
  slice(a.l, x);
#pragma unroll
  for (int i = 0; i < N; i++) k.l[i] = K_IN(i);
  return mul(a, k);
}

// x 2^390 in the chain's form -> x 2^384 (12 words), canonical
DH_HD void to(uint32_t r[12], const el& a) {
  el k;
#pragma unroll
  for (int i = 0; i < N; i++) k.l[i] = K_OUT(i);
  const el v = mul(a, k);
  unslice(r, v.l);
}

// x^e for a fixed exponent given as a dictionary schedule (consts.hpp SCHED_*; W, ODD, RUNS = SCHED_W, SCHED_ODD,
// SCHED_RUNS): the table x, x^3, ..., x^(2^W - 1) and RUNS all-ones entries, each doubling the run; sched[0] = first
// table index, then (squarings << 8 | index), index 0xff = squarings only, and a terminating 0 entry so that the
// read one step ahead stays in bounds. See fp.hpp fp_pow_sched for where the table lives and why.
template <int W, int ODD, int RUNS>
DH_HD el pow_sched(const el& x, const uint32_t* sched, int len) {
  el tab[ODD + RUNS];
  {
    const el x2 = sqr(x);
    el t = x;
    tab[0] = t;
#pragma unroll 1
    for (int k = 1; k < ODD; k++) {
      el y = x2;
      opaque(y);
      t = mul(t, y);
      tab[k] = t;
    }
    // t = x^(2^r - 1), r = W: each run entry doubles r
#pragma unroll 1
    for (int k = 0, r = W; k < RUNS; k++, r *= 2) {
      const el h = t;
#pragma unroll 1
      for (int j = 0; j < r; j++) t = sqr(t);
      t = mul(t, h);
      tab[ODD + k] = t;
    }
  }
  el acc = tab[sched[0]];
  uint32_t next = sched[1];
#pragma unroll 1
  for (int i = 1; i < len; i++) {
    const uint32_t op = next;
    next = sched[i + 1];  // scalar load issued a whole step before its use
    const uint32_t nsq = op >> 8, k = op & 0xff;
    const el e = tab[k == 0xff ? 0 : k];  // issued before the squarings
#pragma unroll 1
    for (uint32_t j = 0; j < nsq; j++) acc = sqr(acc);
    if (k != 0xff) acc = mul(acc, e);
  }
  return acc;
}
}  // namespace m30
}  // namespace dh
