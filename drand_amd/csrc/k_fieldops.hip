// Test infrastructure: one lane, one field operation (dh_field_ops_debug, DESIGN.md "Field-layer op kernel").
//
// The arithmetic layers (fp.hpp, fp_mul28.hpp, fp28.hpp, fp2_28.hpp, fp_mul30.hpp, inv_bingcd.hpp, fr.hpp) are reached
// by the library's kernels only with hash outputs and curve coordinates as operands. This kernel runs each of their
// operations alone on caller-given words, so that tests/test_gpu_field_ops.py can put every operation at the bounds
// its header states. Each lane reads its own opcode and one operand record and writes one result record; every case
// calls the headers directly. No other path of the library launches it.
//
// Operand record (in_words >= FO_IN_WORDS 32-bit words a lane): 12-word operands (fp, 12 x 32-bit) at words 12 k,
// 14-limb operands (f28, one limb a word, not masked) at words 14 k, 8-word Fr operands at words 8 k; the scalars
// s0 .. s7 (coefficients, flags, trip counts) at words FO_SCALARS + j. Result record (out_words >= FO_OUT_WORDS): results
// in the same slot layout, flags at words FO_OUT_FLAGS + j; words an operation does not write are zero.
#include "kcommon.hpp"
#include "fr.hpp"

namespace dh {

// the op table (mirrored by tests/field_ops_cases.py, which tests/test_field_ops_cases.py compares with this text)
enum field_op : uint32_t {
  FO_FP_ADD = 0,         // fp_add(a, b)
  FO_FP_SUB = 1,         // fp_sub(a, b)
  FO_FP_NEG = 2,         // fp_neg(a)
  FO_FP_DBL = 3,         // fp_dbl(a)
  FO_FP_MUL = 4,         // fp_mul(a, b), the out-of-line call
  FO_FP_SQR = 5,         // fp_sqr(a)
  FO_FP_MUL_NR = 6,      // fp_mul(fp_add_nr(a, b), fp_add_nr(c, d))
  FO_FP_TO_MONT = 7,     // fp_to_mont(a)
  FO_FP_FROM_MONT = 8,   // fp_from_mont(a)
  FO_FP_MUL_CIOS = 9,    // fp_mul_cios(a, b)
  FO_F28_MUL = 16,       // f28_mul(a, b) on raw limbs
  FO_F28_SQR = 17,       // f28_sqr(a)
  FO_F28_MUL_INL = 18,   // f28_mul_inl(a, b)
  FO_F28_SQR_INL = 19,   // f28_sqr_inl(a)
  FO_F28_FROM_FP = 20,   // f28_from_fp(fp a)
  FO_F28_TO_FP = 21,     // f28_to_fp(a)
  FO_F28_ZERO = 22,      // f28_zero(a) -> flag 0
  FO_F28_ADD_NC = 23,    // f28_add_nc(a, b), the raw limbs
  FO_F28_RED = 24,       // f28_red(a)
  FO_F28_LIN = 32,       // + k: f28_lin<K>(a, s0, b, s1), K the k-th multiple of fo_with_k
  FO_F28_LIN3 = 48,      // + k: f28_lin3<K>(a, s0, b, s1, c, s2)
  FO_F28_SUB_NC = 64,    // + k: d = f28_sub_nc<K>(a, b): slot 0 f28_mul(d, c), slot 1 d's raw limbs, slot 2 f28_sqr(d)
  FO_F2_MUL = 96,        // f2_mul<false>(a, b), a = slots 0, 1, b = slots 2, 3
  FO_F2_MUL_NC = 97,     // f2_mul<true>(a, b)
  FO_F2_RED = 98,        // f2_red(a)
  FO_F2_CONJ = 99,       // f2_conj(a)
  FO_F2_NEG3 = 100,      // f2_neg3(a)
  FO_F2_SQR = 104,       // + 2 j + nc: f2_sqr<K, NC>(a), K = 3, 4, 7, 12 for j = 0 .. 3
  FO_J28_DBL = 112,      // j28_dbl<false>(P), P = slots 0 .. 2 and s0 = inf
  FO_J28_DBL_INL = 113,  // j28_dbl<true>(P)
  FO_J28_DBL_A = 114,    // j28_dbl_a(P, f28_e1p_a())
  FO_J28_MADD = 115,     // j28_madd(P, q), q = slots 3, 4
  FO_J28_ADD = 116,      // j28_add(P, Q), Q = slots 3 .. 5 and s1 = inf
  FO_J28_MADD_FAST = 117,  // j28_madd_fast(P, q), flag 1 = j28_poisoned
  FO_J28_ADD_FAST = 118,   // j28_add_fast(P, Q), flag 1 = j28_poisoned
  FO_J228_DBL = 120,     // j228_dbl<false>(P), P = slots 0 .. 5 and s0 = inf
  FO_J228_DBL_NC = 121,  // j228_dbl<true>(P)
  FO_J228_MADD = 122,    // j228_madd<true>(P, q), q = slots 6 .. 9
  FO_J228_ADD = 123,     // j228_add<true>(P, Q), Q = slots 6 .. 11 and s1 = inf
  FO_M30_MUL = 128,      // m30::to(m30::mul(from(a), from(b)))
  FO_M30_SQR = 129,      // m30::to(m30::sqr(from(a)))
  FO_M30_MUL2 = 130,     // mont_mul2 on (from(a), from(b)) x (from(c), from(d)), both through to()
  FO_M30_SQR2 = 131,     // mont_sqr2 on (from(a), from(b))
  FO_M30_POW = 132,      // + j: fp_pow_sched(a, S), S = SCHED_SQRT, SCHED_SR1_C1, SCHED_INV, SCHED_LEGENDRE
  FO_BGCD_INV = 140,     // bgcd::inverse(a), a a plain integer in [1, p)
  FO_FP2_INV = 141,      // fp2_inv(a), a = slots 0, 1
  FO_FP2_INV_VT = 142,   // fp2_inv_vt(a)
  FO_FR_MUL = 144,       // fr_mul(a, b)
  FO_FR_ADD = 145,       // fr_add(a, b)
  FO_FR_SUB = 146,       // fr_sub(a, b)
  FO_FR_INV = 147,       // fr_inv(a)
  FO_FR_FROM_BE512 = 148,   // fr_from_be512(words 0 .. 15)
  FO_FR_IS_CANONICAL = 149, // fr_is_canonical(a) -> flag 0
  FO_CALL_LIVE = 152,    // twelve fp values live across a loop of s0 products (see below)
  FO_CALL_NESTED = 153,  // a product inside a data-dependent branch inside that loop
};
constexpr int FO_NK = 15;
constexpr uint32_t FO_MAX_TRIP = 64;  // iterations of the call-convention loops

bool field_op_known(uint32_t op) {
  return op <= FO_FP_MUL_CIOS || (op >= FO_F28_MUL && op <= FO_F28_RED) || (op >= FO_F28_LIN && op < FO_F28_LIN + FO_NK) ||
         (op >= FO_F28_LIN3 && op < FO_F28_LIN3 + FO_NK) || (op >= FO_F28_SUB_NC && op < FO_F28_SUB_NC + FO_NK) ||
         (op >= FO_F2_MUL && op <= FO_F2_NEG3) || (op >= FO_F2_SQR && op < FO_F2_SQR + 8) ||
         (op >= FO_J28_DBL && op <= FO_J28_ADD_FAST) || (op >= FO_J228_DBL && op <= FO_J228_ADD) ||
         (op >= FO_M30_MUL && op < FO_M30_POW + 4) || (op >= FO_BGCD_INV && op <= FO_FP2_INV_VT) ||
         (op >= FO_FR_MUL && op <= FO_FR_IS_CANONICAL) || op == FO_CALL_LIVE || op == FO_CALL_NESTED;
}

template <int K>
struct fo_kc {
  static constexpr int value = K;
};
// f(K) for the k-th multiple of p that has a constant (fp28.hpp DH_KP)
template <class F>
DH_DEV void fo_with_k(uint32_t k, F f) {
  switch (k) {
    case 0: f(fo_kc<2>{}); break;
    case 1: f(fo_kc<3>{}); break;
    case 2: f(fo_kc<4>{}); break;
    case 3: f(fo_kc<6>{}); break;
    case 4: f(fo_kc<7>{}); break;
    case 5: f(fo_kc<8>{}); break;
    case 6: f(fo_kc<9>{}); break;
    case 7: f(fo_kc<12>{}); break;
    case 8: f(fo_kc<16>{}); break;
    case 9: f(fo_kc<18>{}); break;
    case 10: f(fo_kc<21>{}); break;
    case 11: f(fo_kc<24>{}); break;
    case 12: f(fo_kc<26>{}); break;
    case 13: f(fo_kc<32>{}); break;
    default: f(fo_kc<48>{}); break;
  }
}

DH_DEV fp fo_fp(const uint32_t* in, int k) {
  fp a;
#pragma unroll
  for (int j = 0; j < 12; j++) a.v[j] = in[12 * k + j];
  return a;
}
DH_DEV f28 fo_f28(const uint32_t* in, int k) {
  f28 a;
#pragma unroll
  for (int j = 0; j < 14; j++) a.l[j] = in[14 * k + j];
  return a;
}
DH_DEV f228 fo_f2(const uint32_t* in, int k) { return {fo_f28(in, 2 * k), fo_f28(in, 2 * k + 1)}; }
DH_DEV fr fo_fr(const uint32_t* in, int k) {
  fr a;
#pragma unroll
  for (int j = 0; j < 8; j++) a.v[j] = in[8 * k + j];
  return a;
}
DH_DEV void fo_st(uint32_t* out, int k, const fp& a) {
#pragma unroll
  for (int j = 0; j < 12; j++) out[12 * k + j] = a.v[j];
}
DH_DEV void fo_st(uint32_t* out, int k, const f28& a) {
#pragma unroll
  for (int j = 0; j < 14; j++) out[14 * k + j] = a.l[j];
}
DH_DEV void fo_st(uint32_t* out, int k, const f228& a) {
  fo_st(out, 2 * k, a.c0);
  fo_st(out, 2 * k + 1, a.c1);
}
DH_DEV void fo_st(uint32_t* out, int k, const fr& a) {
#pragma unroll
  for (int j = 0; j < 8; j++) out[8 * k + j] = a.v[j];
}
DH_DEV void fo_st(uint32_t* out, const j28& p) {
  fo_st(out, 0, p.x);
  fo_st(out, 1, p.y);
  fo_st(out, 2, p.z);
  out[FO_OUT_FLAGS] = p.inf;
}
DH_DEV void fo_st(uint32_t* out, const j228& p) {
  fo_st(out, 0, p.x);
  fo_st(out, 1, p.y);
  fo_st(out, 2, p.z);
  out[FO_OUT_FLAGS] = p.inf;
}
// a value the compiler can neither reload nor recompute later: it stays in registers from here on
DH_DEV void fo_pin(fp& a) {
#pragma unroll
  for (int j = 0; j < 12; j++) asm volatile("" : "+v"(a.v[j]));
}
DH_DEV fp fo_fold(fp r, const fp& v) { return fp_add(fp_mul(r, v), v); }

__global__ __launch_bounds__(64) void k_field_ops(const uint32_t* __restrict__ ops, const uint32_t* __restrict__ in_all,
                                                  size_t in_words, size_t n, uint32_t* __restrict__ out_all,
                                                  size_t out_words) {
  const size_t lane = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (lane >= n) return;
  const uint32_t op = ops[lane];
  const uint32_t* in = in_all + lane * in_words;
  uint32_t* out = out_all + lane * out_words;
  const uint32_t* s = in + FO_SCALARS;
  if (op >= FO_F28_LIN && op < FO_F28_LIN + FO_NK) {
    fo_with_k(op - FO_F28_LIN, [&](auto K) {
      fo_st(out, 0, f28_lin<decltype(K)::value>(fo_f28(in, 0), (int)s[0], fo_f28(in, 1), (int)s[1]));
    });
    return;
  }
  if (op >= FO_F28_LIN3 && op < FO_F28_LIN3 + FO_NK) {
    fo_with_k(op - FO_F28_LIN3, [&](auto K) {
      fo_st(out, 0, f28_lin3<decltype(K)::value>(fo_f28(in, 0), (int)s[0], fo_f28(in, 1), (int)s[1], fo_f28(in, 2), (int)s[2]));
    });
    return;
  }
  if (op >= FO_F28_SUB_NC && op < FO_F28_SUB_NC + FO_NK) {
    f28 d;
    fo_with_k(op - FO_F28_SUB_NC, [&](auto K) { d = f28_sub_nc<decltype(K)::value>(fo_f28(in, 0), fo_f28(in, 1)); });
    fo_st(out, 0, f28_mul(d, fo_f28(in, 2)));
    fo_st(out, 1, d);
    fo_st(out, 2, f28_sqr(d));
    return;
  }
  if (op >= FO_M30_POW && op < FO_M30_POW + 4) {
    const uint32_t j = op - FO_M30_POW;
    const uint32_t* sched = j == 0 ? cst::SCHED_SQRT : j == 1 ? cst::SCHED_SR1_C1 : j == 2 ? cst::SCHED_INV : cst::SCHED_LEGENDRE;
    const int len = j == 0 ? cst::SCHED_SQRT_LEN : j == 1 ? cst::SCHED_SR1_C1_LEN : j == 2 ? cst::SCHED_INV_LEN : cst::SCHED_LEGENDRE_LEN;
    fo_st(out, 0, fp_pow_sched(fo_fp(in, 0), sched, len));
    return;
  }
  switch (op) {
    case FO_FP_ADD: fo_st(out, 0, fp_add(fo_fp(in, 0), fo_fp(in, 1))); break;
    case FO_FP_SUB: fo_st(out, 0, fp_sub(fo_fp(in, 0), fo_fp(in, 1))); break;
    case FO_FP_NEG: fo_st(out, 0, fp_neg(fo_fp(in, 0))); break;
    case FO_FP_DBL: fo_st(out, 0, fp_dbl(fo_fp(in, 0))); break;
    case FO_FP_MUL: fo_st(out, 0, fp_mul(fo_fp(in, 0), fo_fp(in, 1))); break;
    case FO_FP_SQR: fo_st(out, 0, fp_sqr(fo_fp(in, 0))); break;
    case FO_FP_MUL_NR:
      fo_st(out, 0, fp_mul(fp_add_nr(fo_fp(in, 0), fo_fp(in, 1)), fp_add_nr(fo_fp(in, 2), fo_fp(in, 3))));
      break;
    case FO_FP_TO_MONT: fo_st(out, 0, fp_to_mont(fo_fp(in, 0))); break;
    case FO_FP_FROM_MONT: fo_st(out, 0, fp_from_mont(fo_fp(in, 0))); break;
    case FO_FP_MUL_CIOS: fo_st(out, 0, fp_mul_cios(fo_fp(in, 0), fo_fp(in, 1))); break;
    case FO_F28_MUL: fo_st(out, 0, f28_mul(fo_f28(in, 0), fo_f28(in, 1))); break;
    case FO_F28_SQR: fo_st(out, 0, f28_sqr(fo_f28(in, 0))); break;
    case FO_F28_MUL_INL: fo_st(out, 0, f28_mul_inl(fo_f28(in, 0), fo_f28(in, 1))); break;
    case FO_F28_SQR_INL: fo_st(out, 0, f28_sqr_inl(fo_f28(in, 0))); break;
    case FO_F28_FROM_FP: fo_st(out, 0, f28_from_fp(fo_fp(in, 0))); break;
    case FO_F28_TO_FP: fo_st(out, 0, f28_to_fp(fo_f28(in, 0))); break;
    case FO_F28_ZERO: out[FO_OUT_FLAGS] = f28_zero(fo_f28(in, 0)); break;
    case FO_F28_ADD_NC: fo_st(out, 0, f28_add_nc(fo_f28(in, 0), fo_f28(in, 1))); break;
    case FO_F28_RED: fo_st(out, 0, f28_red(fo_f28(in, 0))); break;
    case FO_F2_MUL: fo_st(out, 0, f2_mul<false>(fo_f2(in, 0), fo_f2(in, 1))); break;
    case FO_F2_MUL_NC: fo_st(out, 0, f2_mul<true>(fo_f2(in, 0), fo_f2(in, 1))); break;
    case FO_F2_RED: fo_st(out, 0, f2_red(fo_f2(in, 0))); break;
    case FO_F2_CONJ: fo_st(out, 0, f2_conj(fo_f2(in, 0))); break;
    case FO_F2_NEG3: fo_st(out, 0, f2_neg3(fo_f2(in, 0))); break;
    case FO_F2_SQR + 0: fo_st(out, 0, f2_sqr<3, false>(fo_f2(in, 0))); break;
    case FO_F2_SQR + 1: fo_st(out, 0, f2_sqr<3, true>(fo_f2(in, 0))); break;
    case FO_F2_SQR + 2: fo_st(out, 0, f2_sqr<4, false>(fo_f2(in, 0))); break;
    case FO_F2_SQR + 3: fo_st(out, 0, f2_sqr<4, true>(fo_f2(in, 0))); break;
    case FO_F2_SQR + 4: fo_st(out, 0, f2_sqr<7, false>(fo_f2(in, 0))); break;
    case FO_F2_SQR + 5: fo_st(out, 0, f2_sqr<7, true>(fo_f2(in, 0))); break;
    case FO_F2_SQR + 6: fo_st(out, 0, f2_sqr<12, false>(fo_f2(in, 0))); break;
    case FO_F2_SQR + 7: fo_st(out, 0, f2_sqr<12, true>(fo_f2(in, 0))); break;
    case FO_J28_DBL:
    case FO_J28_DBL_INL:
    case FO_J28_DBL_A:
    case FO_J28_MADD:
    case FO_J28_ADD:
    case FO_J28_MADD_FAST:
    case FO_J28_ADD_FAST: {
      const j28 p{fo_f28(in, 0), fo_f28(in, 1), fo_f28(in, 2), s[0] != 0};
      j28 r;
      if (op == FO_J28_DBL) r = j28_dbl<false>(p);
      else if (op == FO_J28_DBL_INL) r = j28_dbl<true>(p);
      else if (op == FO_J28_DBL_A) r = j28_dbl_a(p, f28_e1p_a());
      else if (op == FO_J28_MADD) r = j28_madd(p, fo_f28(in, 3), fo_f28(in, 4));
      else if (op == FO_J28_MADD_FAST) r = j28_madd_fast(p, fo_f28(in, 3), fo_f28(in, 4));
      else {
        const j28 q{fo_f28(in, 3), fo_f28(in, 4), fo_f28(in, 5), s[1] != 0};
        r = op == FO_J28_ADD ? j28_add(p, q) : j28_add_fast(p, q);
      }
      fo_st(out, r);
      if (op == FO_J28_MADD_FAST || op == FO_J28_ADD_FAST) out[FO_OUT_FLAGS + 1] = j28_poisoned(r);
      break;
    }
    case FO_J228_DBL:
    case FO_J228_DBL_NC:
    case FO_J228_MADD:
    case FO_J228_ADD: {
      const j228 p{fo_f2(in, 0), fo_f2(in, 1), fo_f2(in, 2), s[0] != 0};
      j228 r;
      if (op == FO_J228_DBL) r = j228_dbl<false>(p);
      else if (op == FO_J228_DBL_NC) r = j228_dbl<true>(p);
      else if (op == FO_J228_MADD) r = j228_madd<true>(p, fo_f2(in, 3), fo_f2(in, 4));
      else r = j228_add<true>(p, j228{fo_f2(in, 3), fo_f2(in, 4), fo_f2(in, 5), s[1] != 0});
      fo_st(out, r);
      break;
    }
    case FO_M30_MUL: fo_st(out, 0, fp30_to(m30::mul(fp30_from(fo_fp(in, 0)), fp30_from(fo_fp(in, 1))))); break;
    case FO_M30_SQR: fo_st(out, 0, fp30_to(m30::sqr(fp30_from(fo_fp(in, 0))))); break;
    case FO_M30_MUL2:
    case FO_M30_SQR2: {
      const fp30 x0 = fp30_from(fo_fp(in, 0)), x1 = fp30_from(fo_fp(in, 1));
      fp30 r0, r1;
      if (op == FO_M30_MUL2) {
        const fp30 y0 = fp30_from(fo_fp(in, 2)), y1 = fp30_from(fo_fp(in, 3));
        m30::mont_mul2(r0.l, r1.l, x0.l, x1.l, y0.l, y1.l);
      } else {
        m30::mont_sqr2(r0.l, r1.l, x0.l, x1.l);
      }
      fo_st(out, 0, fp30_to(r0));
      fo_st(out, 1, fp30_to(r1));
      break;
    }
    case FO_BGCD_INV: {
      fp a = fo_fp(in, 0);
      bgcd::inverse(a.v);
      fo_st(out, 0, a);
      break;
    }
    case FO_FP2_INV:
    case FO_FP2_INV_VT: {
      const fp2 a{fo_fp(in, 0), fo_fp(in, 1)};
      const fp2 r = op == FO_FP2_INV ? fp2_inv(a) : fp2_inv_vt(a);
      fo_st(out, 0, r.c0);
      fo_st(out, 1, r.c1);
      break;
    }
    case FO_FR_MUL: fo_st(out, 0, fr_mul(fo_fr(in, 0), fo_fr(in, 1))); break;
    case FO_FR_ADD: fo_st(out, 0, fr_add(fo_fr(in, 0), fo_fr(in, 1))); break;
    case FO_FR_SUB: fo_st(out, 0, fr_sub(fo_fr(in, 0), fo_fr(in, 1))); break;
    case FO_FR_INV: fo_st(out, 0, fr_inv(fo_fr(in, 0))); break;
    case FO_FR_FROM_BE512: {
      uint32_t d[16];
      fr r;
#pragma unroll
      for (int j = 0; j < 16; j++) d[j] = in[j];
      fr_from_be512(d, r.v);
      fo_st(out, 0, r);
      break;
    }
    case FO_FR_IS_CANONICAL: out[FO_OUT_FLAGS] = fr_is_canonical(fo_fr(in, 0).v); break;
    // The call convention (fp.hpp DH_FP_CALL): twelve values are loaded and pinned BEFORE a loop of s0 (at most 64)
    // iterations whose products depend on the loop index, acc = ((acc * k) + k)^2 with k the plain word i + 2; after
    // the loop every one of them is folded into the result, r = r * v + v in slot order, and slots 8 .. 11 also go
    // through fp2_mul as two Fp2 values. A register the clobber list misses, or a loop condition lost across a
    // product, changes the result. The loop itself counts to FO_MAX_TRIP in a scalar register and the lane's own
    // count s0 is a condition inside it, live across both products: were the lane's count the loop's bound, the
    // compiler would keep the remaining count in a VGPR, and a product that overwrote it would make the loop endless
    // where it should make the result wrong.
    case FO_CALL_LIVE: {
      fp v[12];
#pragma unroll
      for (int j = 0; j < 12; j++) {
        v[j] = fo_fp(in, j);
        fo_pin(v[j]);
      }
      const uint32_t trip = s[0];
      fp acc = fp_add(v[0], v[1]);
#pragma unroll 1
      for (uint32_t i = 0; i < FO_MAX_TRIP; i++) {
        if (i >= trip) continue;
        fp k = fp_zero();
        k.v[0] = i + 2;
        acc = fp_sqr(fp_add(fp_mul(acc, k), k));
      }
#pragma unroll
      for (int j = 0; j < 12; j++) acc = fo_fold(acc, v[j]);
      const fp2 f = fp2_mul(fp2{v[8], v[9]}, fp2{v[10], v[11]});
      fo_st(out, 0, acc);
      fo_st(out, 1, f.c0);
      fo_st(out, 2, f.c1);
      break;
    }
    // the same loop with its product under a condition on the running value (part of the wave enters the call, and the
    // lanes' trip counts differ): acc = acc * v1 where acc's word 0 is odd, then acc + v2; v3 .. v7 are folded in after
    case FO_CALL_NESTED: {
      fp v[8];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        v[j] = fo_fp(in, j);
        fo_pin(v[j]);
      }
      const uint32_t trip = s[0];
      fp acc = v[0];
#pragma unroll 1
      for (uint32_t i = 0; i < FO_MAX_TRIP; i++) {
        if (i >= trip) continue;
        if (acc.v[0] & 1) acc = fp_mul(acc, v[1]);
        acc = fp_add(acc, v[2]);
      }
#pragma unroll
      for (int j = 3; j < 8; j++) acc = fo_fold(acc, v[j]);
      fo_st(out, 0, acc);
      break;
    }
    default: break;
  }
}

hipError_t launch_field_ops(const uint32_t* ops, const uint32_t* in, size_t in_words, size_t n, uint32_t* out,
                            size_t out_words, hipStream_t st) {
  hipLaunchKernelGGL(k_field_ops, dim3(nblk(n, 64)), dim3(64), 0, st, ops, in, in_words, n, out, out_words);
  return hipGetLastError();
}

}  // namespace dh
