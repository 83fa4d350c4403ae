// Batch Schnorr verification for DKG packets on gfx950: kyber v1.1.18 sign/schnorr over the schemes' key group, the
// schemes' DKGAuthScheme (crypto/schemes.go:103,144,184), as dkg.VerifyPacketSignature uses it on
// every deal, response and justification bundle (core/drand_beacon_control.go:354,476) and the
// leader's signature over group.Hash() (core/group_setup.go:384). Specification: DESIGN.md §11.
//
//   [key table decoded and subgroup-tested by k_prep_sig / k_dec_sig_g2 + k_sub_sig_g2, R decoded by k_dec_sig_*]
//   k_schnorr_scalars   per item: s < r, h = SHA-512(R || P || msg) mod r, the regular 4-bit windows of s and -h
//   k_schnorr_table     per key (and once per process for the generator): P, 3P, ..., 15P affine, 28-bit form
//   k_schnorr_check     per item: [s]G - [h]P as one joint Straus chain (shared doublings), compared with R
//   k_schnorr_plain     per item: the same check from two jac_mul_words, an addition and jac_eq (the cross-check)
// s and h are public, so every step may take variable time.
#include "kcommon.hpp"
#include "fr.hpp"
#include "sha512.hpp"

namespace dh {

// per item: s (8 little-endian words), h (8), the window digits of s (8, fr_reg4), the window digits of -h (8)
constexpr int SN_WORDS = 32;
constexpr int SN_ENTRIES = 8;  // table entries per point: the odd multiples up to 15 P

// one lane per item. status[i] comes from R's decode (and the key's, k_mark_bad_key); an s >= r rejects the item
// here (kyber's mod.Int.UnmarshalBinary refuses it: s + r must not pass). Rejected items get no scalars.
__global__ __launch_bounds__(256) void k_schnorr_scalars(const uint8_t* __restrict__ sigs, size_t stride, uint32_t K,
                                                         const uint8_t* __restrict__ keys, const uint32_t* __restrict__ key_idx,
                                                         const uint8_t* __restrict__ msgs, const uint32_t* __restrict__ msg_off,
                                                         size_t n, uint8_t* __restrict__ status, uint32_t* __restrict__ sc) {
  const size_t i = gtid();
  if (i >= n || status[i] != DEC_OK) return;
  const uint8_t* sg = sigs + i * stride;
  uint32_t s[8];
#pragma unroll
  for (int j = 0; j < 8; j++) s[j] = ld_be32a(sg + K + 28 - 4 * j);
  if (!fr_is_canonical(s)) {
    status[i] = DEC_BAD;
    return;
  }
  const sha512_h d = sha512_rpm(sg, keys + (size_t)key_idx[i] * K, K, msgs + msg_off[i], msg_off[i + 1] - msg_off[i]);
  uint32_t dw[16], h[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    dw[2 * j] = (uint32_t)(d.h[j] >> 32);
    dw[2 * j + 1] = (uint32_t)d.h[j];
  }
  fr_from_be512(dw, h);
  uint32_t* o = sc + i * SN_WORDS;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    o[j] = s[j];
    o[8 + j] = h[j];
  }
  // fr_reg4 recodes 0 as r (every digit of r, negated): [-r] P is the identity on the order-r subgroup, which the
  // exact chain reaches through its exceptional cases
  fr_reg4(s, o + 16);
  fr_reg4(h, o + 24);
#pragma unroll
  for (int j = 0; j < 8; j++) o[24 + j] ^= 0x88888888u;  // every digit is nonzero: the sign bits flipped give -h
}

// a 28-bit value in 16 words (14 limbs + 2 pad), as the Lagrange tables of k_recover.hip hold theirs
DH_DEV f28 sn_ld28(const uint32_t* p) {
  f28 a;
  const uint4* q = (const uint4*)p;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint4 t = q[i];
    a.l[4 * i] = t.x;
    a.l[4 * i + 1] = t.y;
    if (4 * i + 2 < 14) a.l[4 * i + 2] = t.z;
    if (4 * i + 3 < 14) a.l[4 * i + 3] = t.w;
  }
  return a;
}
DH_DEV void sn_st28(uint32_t* p, const f28& a) {
  uint4* q = (uint4*)p;
#pragma unroll
  for (int i = 0; i < 4; i++)
    q[i] = make_uint4(a.l[4 * i], a.l[4 * i + 1], 4 * i + 2 < 14 ? a.l[4 * i + 2] : 0u, 4 * i + 3 < 14 ? a.l[4 * i + 3] : 0u);
}

// The lazily reduced point arithmetic of each key group behind one interface (fp28.hpp j28, fp2_28.hpp j228).
// An affine table entry is EW words: x then y, each coordinate component 16 words.
template <class F>
struct lazy;
template <>
struct lazy<fp> {
  using J = j28;
  static constexpr int EW = 32;
  static DH_DEV void st_entry(uint32_t* p, const aff<fp>& a) {
    sn_st28(p, f28_from_fp(a.x));
    sn_st28(p + 16, f28_from_fp(a.y));
  }
  static DH_DEV J inf() { return j28_inf(); }
  static DH_DEV J dbl(const J& p) { return j28_dbl<true>(p); }
  // bounds (fp28.hpp): dbl and madd both accept what either returns; a negated y is 2p - y <= 2p
  template <bool EXACT>
  static DH_DEV J madd(const J& p, const uint32_t* e, bool neg) {
    const f28 x = sn_ld28(e), y0 = sn_ld28(e + 16);
    const f28 y = neg ? f28_neg2(y0) : y0;
    return EXACT ? j28_madd(p, x, y) : j28_madd_fast(p, x, y);
  }
  static DH_DEV bool poisoned(const J& p) { return j28_poisoned(p); }
  // q == (x, y) affine: X == x Z^2 and Y == y Z^3; q's X <= 26, Y <= 18 after either formula
  static DH_DEV bool eq_aff(const J& q, const aff<fp>& r) {
    if (q.inf) return false;
    const f28 z2 = f28_sqr(q.z), z3 = f28_mul(z2, q.z);
    if (!f28_zero(f28_sub<26>(f28_mul(f28_from_fp(r.x), z2), q.x))) return false;
    return f28_zero(f28_sub<18>(f28_mul(f28_from_fp(r.y), z3), q.y));
  }
};
template <>
struct lazy<fp2> {
  using J = j228;
  static constexpr int EW = 64;
  static DH_DEV void st_entry(uint32_t* p, const aff<fp2>& a) {
    sn_st28(p, f28_from_fp(a.x.c0));
    sn_st28(p + 16, f28_from_fp(a.x.c1));
    sn_st28(p + 32, f28_from_fp(a.y.c0));
    sn_st28(p + 48, f28_from_fp(a.y.c1));
  }
  static DH_DEV J inf() { return j228_inf(); }
  static DH_DEV J dbl(const J& p) { return j228_dbl<true>(p); }
  template <bool EXACT>
  static DH_DEV J madd(const J& p, const uint32_t* e, bool neg) {
    return j228_madd_ld<EXACT, true>(p, [e, neg](int k) {
      const f228 c{sn_ld28(e + 32 * k), sn_ld28(e + 32 * k + 16)};
      return k && neg ? f2_neg3(c) : c;
    });
  }
  static DH_DEV bool poisoned(const J& p) { return j228_poisoned(p); }
  // X, Y < 2, Z < 12 per component (fp2_28.hpp): Z^2 (2, 4), x Z^2 and y Z^3 (4, 6), the differences + 3p
  static DH_DEV bool eq_aff(const J& q, const aff<fp2>& r) {
    if (q.inf) return false;
    const f228 z2 = f2_sqr<12>(q.z);
    if (!f2_zero(f2_lin<3, 3>(f2_mul(f2_from_fp2(r.x), z2), 1, q.x, -1))) return false;
    const f228 z3 = f2_mul(z2, q.z);
    return f2_zero(f2_lin<3, 3>(f2_mul(f2_from_fp2(r.y), z3), 1, q.y, -1));
  }
};

// one lane per table: the odd multiples P, 3P, ..., 15P of key k, affine in the 28-bit form (SN_ENTRIES entries of
// lazy<F>::EW words), so the items sharing a key share its table. gen: the single table of the group's generator.
// A key that did not decode has no table; its items are rejected before they read one. The keys are subgroup points
// other than the identity (order r), so no multiple up to 16 P is the identity.
template <class F>
__global__ __launch_bounds__(64) void k_schnorr_table(const uint32_t* __restrict__ key_aff, const uint8_t* __restrict__ kstatus,
                                                      size_t n_keys, int gen, uint32_t* __restrict__ tbl) {
  const size_t k = gtid();
  if (k >= n_keys || (!gen && kstatus[k] != DEC_OK)) return;
  aff<F> a;
  if (gen) {
    if constexpr (sizeof(F) == sizeof(fp)) a = aff<fp>{g1_gen().x, g1_gen().y};
    else a = aff<fp2>{g2_gen().x, g2_gen().y};
  } else {
    a = ld_aff_aos<F>(key_aff, k);
  }
  uint32_t* o = tbl + k * (size_t)(SN_ENTRIES * lazy<F>::EW);
  lazy<F>::st_entry(o, a);
  const jac<F> p2 = jac_dbl(jac_from_aff(a));
  jac<F> cur = jac_from_aff(a);
#pragma unroll 1
  for (int j = 1; j < SN_ENTRIES; j++) {
    cur = jac_add(cur, p2);
    lazy<F>::st_entry(o + j * lazy<F>::EW, jac_to_aff_vt(cur));
  }
}

// [s]G - [h]P over the regular windows of s and -h: at each of the 64 windows four doublings and two mixed additions,
// no digit-dependent branch (fr_reg4: every digit odd and nonzero). EXACT = false takes the additions without their
// exceptional-case tests; a chain that met one ends with Z = 0 mod p (fp28.hpp j28_madd_fast) and runs again exact.
template <class F, bool EXACT>
DH_DEV typename lazy<F>::J schnorr_chain(const uint32_t* __restrict__ dig, const uint32_t* __restrict__ gtab,
                                         const uint32_t* __restrict__ ktab) {
  using L = lazy<F>;
  typename L::J acc = L::inf();
  uint32_t ws = 0, wh = 0;
#pragma unroll 1
  for (int wi = 63; wi >= 0; wi--) {
    if ((wi & 7) == 7) {
      ws = dig[wi >> 3];
      wh = dig[8 + (wi >> 3)];
    }
    if (!acc.inf) {
#pragma unroll 1
      for (int d = 0; d < 4; d++) acc = L::dbl(acc);
    }
    const uint32_t vs = (ws >> (4 * (wi & 7))) & 15, vh = (wh >> (4 * (wi & 7))) & 15;
    acc = L::template madd<EXACT>(acc, gtab + L::EW * (vs & 7), vs & 8);
    acc = L::template madd<EXACT>(acc, ktab + L::EW * (vh & 7), vh & 8);
  }
  return acc;
}

// one lane per item: verdict[i] = 1 exactly when [s]G - [h]P == R. R decoded to a curve point without a subgroup
// test: the left side lies in the subgroup, so an R outside it never matches.
template <class F>
__global__ __launch_bounds__(64) void k_schnorr_check(const uint32_t* __restrict__ sc, const uint8_t* __restrict__ status,
                                                      const uint32_t* __restrict__ r_aff, const uint32_t* __restrict__ key_idx,
                                                      const uint32_t* __restrict__ gtab, const uint32_t* __restrict__ ktabs,
                                                      size_t n, uint8_t* __restrict__ verdict) {
  using L = lazy<F>;
  const size_t i = gtid();
  if (i >= n) return;
  if (status[i] != DEC_OK) {
    verdict[i] = 0;
    return;
  }
  const uint32_t* dig = sc + i * SN_WORDS + 16;
  const uint32_t* ktab = ktabs + (size_t)key_idx[i] * (SN_ENTRIES * L::EW);
  typename L::J q = schnorr_chain<F, false>(dig, gtab, ktab);
  if (L::poisoned(q)) q = schnorr_chain<F, true>(dig, gtab, ktab);
  verdict[i] = L::eq_aff(q, ld_aff_aos<F>(r_aff, i)) ? 1 : 0;
}

// the same verdict from the 32-bit point code alone: two plain double-and-add multiplications
template <class F>
__global__ __launch_bounds__(64) void k_schnorr_plain(const uint32_t* __restrict__ sc, const uint8_t* __restrict__ status,
                                                      const uint32_t* __restrict__ r_aff, const uint32_t* __restrict__ key_idx,
                                                      const uint32_t* __restrict__ key_aff, size_t n,
                                                      uint8_t* __restrict__ verdict) {
  const size_t i = gtid();
  if (i >= n) return;
  if (status[i] != DEC_OK) {
    verdict[i] = 0;
    return;
  }
  const uint32_t* w = sc + i * SN_WORDS;
  jac<F> g;
  if constexpr (sizeof(F) == sizeof(fp)) g = g1_gen();
  else g = g2_gen();
  const jac<F> a = jac_mul_words(g, w, 256);
  const jac<F> b = jac_mul_words(jac_from_aff(ld_aff_aos<F>(key_aff, key_idx[i])), w + 8, 256);
  verdict[i] = jac_eq(jac_add(a, jac_neg(b)), jac_from_aff(ld_aff_aos<F>(r_aff, i))) ? 1 : 0;
}

// ---------------------------------------------------------------- launchers
size_t schnorr_scalar_words() { return SN_WORDS; }
size_t schnorr_table_words(int key_g2) { return (size_t)SN_ENTRIES * (key_g2 ? lazy<fp2>::EW : lazy<fp>::EW); }

hipError_t launch_schnorr_scalars(const uint8_t* sigs, size_t stride, int key_len, const uint8_t* keys, const uint32_t* key_idx,
                                  const uint8_t* msgs, const uint32_t* msg_off, size_t n, uint8_t* status, uint32_t* sc,
                                  hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_schnorr_scalars, dim3(nblk(n, 256)), dim3(256), 0, st, sigs, stride, (uint32_t)key_len, keys, key_idx, msgs,
                     msg_off, n, status, sc);
  return hipGetLastError();
}

hipError_t launch_schnorr_table(int key_g2, const uint32_t* key_aff, const uint8_t* kstatus, size_t n_keys, int gen, uint32_t* tbl,
                                hipStream_t st) {
  if (!n_keys) return hipSuccess;
  if (key_g2)
    hipLaunchKernelGGL(k_schnorr_table<fp2>, dim3(nblk(n_keys, 64)), dim3(64), 0, st, key_aff, kstatus, n_keys, gen, tbl);
  else
    hipLaunchKernelGGL(k_schnorr_table<fp>, dim3(nblk(n_keys, 64)), dim3(64), 0, st, key_aff, kstatus, n_keys, gen, tbl);
  return hipGetLastError();
}

hipError_t launch_schnorr_check(int key_g2, const uint32_t* sc, const uint8_t* status, const uint32_t* r_aff,
                                const uint32_t* key_idx, const uint32_t* gtab, const uint32_t* ktabs, size_t n, uint8_t* verdict,
                                hipStream_t st) {
  if (!n) return hipSuccess;
  if (key_g2)
    hipLaunchKernelGGL(k_schnorr_check<fp2>, dim3(nblk(n, 64)), dim3(64), 0, st, sc, status, r_aff, key_idx, gtab, ktabs, n, verdict);
  else
    hipLaunchKernelGGL(k_schnorr_check<fp>, dim3(nblk(n, 64)), dim3(64), 0, st, sc, status, r_aff, key_idx, gtab, ktabs, n, verdict);
  return hipGetLastError();
}

hipError_t launch_schnorr_plain(int key_g2, const uint32_t* sc, const uint8_t* status, const uint32_t* r_aff,
                                const uint32_t* key_idx, const uint32_t* key_aff, size_t n, uint8_t* verdict, hipStream_t st) {
  if (!n) return hipSuccess;
  if (key_g2)
    hipLaunchKernelGGL(k_schnorr_plain<fp2>, dim3(nblk(n, 64)), dim3(64), 0, st, sc, status, r_aff, key_idx, key_aff, n, verdict);
  else
    hipLaunchKernelGGL(k_schnorr_plain<fp>, dim3(nblk(n, 64)), dim3(64), 0, st, sc, status, r_aff, key_idx, key_aff, n, verdict);
  return hipGetLastError();
}

DH_COUNTER_ACCESSOR(schnorr)

}  // namespace dh
