// Batch beacon-verification kernels for gfx950 — per-round preparation (this file), see also
// k_msm.hip, k_check.hip, k_sign.hip.
//
// Path (one call of dh_verify_batch, see drandhip.cpp):
//   k_prep_sig     decode + subgroup-check every signature, randomness = SHA-256(sig)    [A4a, A5]
//                  (a large local G1 batch: decode only, k_dec_sig_g1_batch; its subgroup test runs once per batch
//                  on the level-0 sigma buckets, k_msm.hip launch_sub_batch; a large local G2 batch
//                  likewise: k_dec_sig_g2 without k_sub_sig_g2)
//   k_prep_msg     DigestBeacon + hash_to_curve without cofactor clearing               [A2, A3, A4b]
//                  (a large local G1 batch: k_round_g1_ride does this and the decode above on one lane, the hash
//                  point's inversion riding the decode's square-root chain; by default it also leaves the
//                  hash's 11-isogeny to the MSM and writes the MSM's 28-bit points itself)
//   k_scalars      128-bit random-linear-combination scalars r_i = SHA-256(seed || i)   [batching, new]
//   MSM (grouped Pippenger, shared sort for both point sets):
//     k_msm_hist -> scan -> k_msm_scatter -> k_msm_bucket28<S>, k_msm_bucket28<Q> -> k_msm_segsum28 -> k_msm_tree28
//     -> k_msm_windows       per group g:  A_g = sum r_i sigma_i,  B_g = sum r_i Q_i
//     (level 0 of the batch above: the hash set stays on E1' up to its row sums, k_msm_iso_rows28 ->
//     k_msm_windows28_split)
//   k_group_check  e(A_g, g2) == e([h_eff] B_g, pk)  (or the G2-signature mirror), one lane per group [A4c]
//   k_leaf_check   per-round 2-pairing check for rounds left in failing groups (bisection leaves)
// All scheme semantics follow /root/reference/crypto/schemes.go:70-72 (VerifyBeacon) and the kyber /
// kilic behaviour restated in oracle/bls_oracle.c.
#include "kcommon.hpp"

namespace dh {

// ---------------------------------------------------------------- prep: signatures
template <class F>
__global__ __launch_bounds__(256, occ<F>::W) void k_prep_sig(const uint8_t* __restrict__ sigs, size_t stride, size_t n,
                                                  uint8_t* __restrict__ status, uint32_t* __restrict__ sig_aff,
                                                  uint8_t* __restrict__ rand_out) {
  size_t i = gtid();
  if (i >= n) return;
  const uint8_t* s = sigs + i * stride;
  aff<F> a;
  uint8_t st;
  if constexpr (sizeof(F) == sizeof(fp)) {
    // the point goes to HBM first and the subgroup test reloads it when it needs it (fp28.hpp g1_in_subgroup28)
    st = g1_decompress(a, s, false);
    if (st == DEC_OK) st_aff_aos<F>(sig_aff, i, a);
    if (rand_out) st_digest(rand_out + 32 * i, sha256_aligned<48>(s));
    if (st == DEC_OK && !g1_in_subgroup28([&] { return ld_aff_aos<fp>(sig_aff, i); })) st = DEC_BAD;
    if (st == DEC_OK) {
      status[i] = st;
      return;
    }
  } else {
    st = g2_decompress(a, s, true);
    if (rand_out) st_digest(rand_out + 32 * i, sha256_aligned<96>(s));
  }
  if (st != DEC_OK) {
    a.x = F{};
    a.y = F{};
    st = DEC_BAD;  // infinity signatures are rejected like kilic's engine + kyber's verify
  }
  status[i] = st;
  st_aff_aos<F>(sig_aff, i, a);
}

// G2 signatures in two passes: decompression (Fp2 square root) and the psi subgroup test each fit one lane's
// registers, the fused kernel spilled 1.1 KB per lane. The affine point and status go through HBM between them
// (96 + 1 B per round, written and read once).
__global__ __launch_bounds__(256, occ<fp2>::W) void k_dec_sig_g2(const uint8_t* __restrict__ sigs, size_t stride, size_t n,
                                                             uint8_t* __restrict__ status, uint32_t* __restrict__ sig_aff,
                                                             uint8_t* __restrict__ rand_out) {
  size_t i = gtid();
  if (i >= n) return;
  const uint8_t* s = sigs + i * stride;
  aff<fp2> a;
  uint8_t st = g2_decompress(a, s, false);
  if (rand_out) st_digest(rand_out + 32 * i, sha256_aligned<96>(s));
  if (st != DEC_OK) {
    a.x = fp2{};
    a.y = fp2{};
    st = DEC_BAD;  // infinity signatures are rejected like kilic's engine + kyber's verify
  }
  status[i] = st;
  st_aff_aos<fp2>(sig_aff, i, a);
}

// two waves per SIMD (some scratch) measured 5% faster over the whole unchained batch than one wave with the
// lazy-form test's values in VGPRs + AGPRs and no scratch (gpurun_out r03g: 80.1 against 84.1 ms per 1M rounds)
__global__ __launch_bounds__(256, 2) void k_sub_sig_g2(size_t n, uint8_t* __restrict__ status, uint32_t* __restrict__ sig_aff) {
  size_t i = gtid();
  if (i >= n || status[i] != DEC_OK) return;
  // P stays in HBM: the lazy-form test reloads it where it needs its coordinates (fp2_28.hpp g2_in_subgroup28)
  if (!g2_in_subgroup28([&] { return ld_aff_aos<fp2>(sig_aff, i); })) {
    status[i] = DEC_BAD;
    st_aff_aos<fp2>(sig_aff, i, aff<fp2>{fp2{}, fp2{}});
  }
}

// ---------------------------------------------------------------- small-batch path (drandhip.cpp verify_small)
// The signature pass split at the decoded point: the per-round pairing check needs only the point, so it starts as soon
// as the decode finishes and runs beside the subgroup test, whose result is ANDed into the verdict at the end
// (k_and_subgroup). A G1 round's decode is a fraction of k_prep_sig<fp> (one square root); the test (two [|u|] chains)
// is the rest. The subgroup kernels write only sub_bad (the point and status stay as the pairing check reads them).
DH_DEV void dec_sig_g1(const uint8_t* __restrict__ sigs, size_t stride, size_t n, uint8_t* __restrict__ status,
                       uint32_t* __restrict__ sig_aff, uint8_t* __restrict__ rand_out) {
  size_t i = gtid();
  if (i >= n) return;
  const uint8_t* s = sigs + i * stride;
  aff<fp> a;
  uint8_t st = g1_decompress(a, s, false);
  if (rand_out) st_digest(rand_out + 32 * i, sha256_aligned<48>(s));
  if (st != DEC_OK) {
    a.x = fp{};
    a.y = fp{};
    st = DEC_BAD;  // infinity signatures are rejected like kilic's engine + kyber's verify
  }
  status[i] = st;
  st_aff_aos<fp>(sig_aff, i, a);
}
__global__ __launch_bounds__(64) void k_dec_sig_g1(const uint8_t* __restrict__ sigs, size_t stride, size_t n,
                                                   uint8_t* __restrict__ status, uint32_t* __restrict__ sig_aff,
                                                   uint8_t* __restrict__ rand_out) {
  dec_sig_g1(sigs, stride, n, status, sig_aff, rand_out);
}
// the same decode for the large local batch whose subgroup test is batched (launch_prep defer_sub, k_msm.hip
// launch_sub_batch): k_prep_sig<fp>'s blocks and occupancy, without its two [|u|] chains
__global__ __launch_bounds__(256, occ<fp>::W) void k_dec_sig_g1_batch(const uint8_t* __restrict__ sigs, size_t stride, size_t n,
                                                                      uint8_t* __restrict__ status, uint32_t* __restrict__ sig_aff,
                                                                      uint8_t* __restrict__ rand_out) {
  dec_sig_g1(sigs, stride, n, status, sig_aff, rand_out);
}

template <class F>
DH_DEV void sub_flag(size_t n, const uint8_t* __restrict__ status, const uint32_t* __restrict__ sig_aff,
                     uint8_t* __restrict__ sub_bad) {
  size_t i = gtid();
  if (i >= n) return;
  bool bad = false;
  if (status[i] == DEC_OK) {
    if constexpr (sizeof(F) == sizeof(fp)) bad = !g1_in_subgroup28([&] { return ld_aff_aos<fp>(sig_aff, i); });
    else bad = !g2_in_subgroup28([&] { return ld_aff_aos<fp2>(sig_aff, i); });
  }
  sub_bad[i] = bad ? 1 : 0;
}
template <class F>
__global__ __launch_bounds__(64) void k_sub_flag(size_t n, const uint8_t* __restrict__ status, const uint32_t* __restrict__ sig_aff,
                                                 uint8_t* __restrict__ sub_bad) {
  sub_flag<F>(n, status, sig_aff, sub_bad);
}
// the batched test's exact fallback over a whole batch (launch_sub_exact): k_prep_sig<fp>'s blocks and occupancy
__global__ __launch_bounds__(256, occ<fp>::W) void k_sub_flag_batch(size_t n, const uint8_t* __restrict__ status,
                                                                    const uint32_t* __restrict__ sig_aff,
                                                                    uint8_t* __restrict__ sub_bad) {
  sub_flag<fp>(n, status, sig_aff, sub_bad);
}
// the G2 fallback: k_sub_sig_g2's blocks and occupancy
__global__ __launch_bounds__(256, 2) void k_sub_flag_batch_g2(size_t n, const uint8_t* __restrict__ status,
                                                              const uint32_t* __restrict__ sig_aff,
                                                              uint8_t* __restrict__ sub_bad) {
  sub_flag<fp2>(n, status, sig_aff, sub_bad);
}
// a round the exact test flagged leaves as the fused k_prep_sig<fp> / k_sub_sig_g2 leaves it: DEC_BAD and the zero point
template <class F>
__global__ __launch_bounds__(256) void k_sub_reject(size_t n, const uint8_t* __restrict__ sub_bad, uint8_t* __restrict__ status,
                                                    uint32_t* __restrict__ sig_aff, uint32_t* __restrict__ nbad) {
  size_t i = gtid();
  if (i >= n || !sub_bad[i]) return;
  atomicAdd(nbad, 1u);
  status[i] = DEC_BAD;
  st_aff_aos<F>(sig_aff, i, aff<F>{F{}, F{}});
}

__global__ __launch_bounds__(64) void k_and_subgroup(size_t n, const uint8_t* __restrict__ sub_bad, uint8_t* __restrict__ verdict) {
  size_t i = gtid();
  if (i >= n) return;
  if (sub_bad[i]) verdict[i] = 0;
}

// small-batch path, G1 hash in three launches, as the G2 hash runs (k_h2f_g2 -> k_sswu_g2 -> k_add_iso_g2): the
// round's two SSWU maps (each a square-root exponentiation, the bulk of the hash) run in two workgroups of their own,
// so on two SIMDs side by side, instead of one after the other on one lane (k_prep_msg_g1). Two waves of ONE
// workgroup measured no faster (1.24 ms against 1.1: they shared a SIMD, and a dependent MAD chain needs one SIMD's
// issue slots to itself). The hash is the small path's critical step for G1 signatures (decode 0.44-0.57 ms beside it).
// tmp: per round u0, u1 (2 x 12 words), then the two SSWU points (2 x 36 words) — hash_small_tmp_bytes.
__global__ __launch_bounds__(64) void k_h2f_g1_small(const uint64_t* __restrict__ rounds, const uint8_t* __restrict__ prevs,
                                                     size_t prev_stride, const uint32_t* __restrict__ prev_lens,
                                                     const uint8_t* __restrict__ msgs32, size_t n, int chained, int dst_id,
                                                     uint8_t* __restrict__ status, uint32_t* __restrict__ u_out) {
  const size_t i = gtid();
  if (i >= n) return;
  const sha_h d = message_of(rounds, prevs, prev_stride, prev_lens, msgs32, chained, i, status);
  uint32_t b[4][8];
  xmd32<4>(b, d, dst_id);
  st_f<fp>(u_out + 24 * i, fp_from_be512(b[0], b[1]));
  st_f<fp>(u_out + 24 * i + 12, fp_from_be512(b[2], b[3]));
}

// one SSWU map per workgroup (lane 0): map j of round j / 2
__global__ __launch_bounds__(64) void k_sswu_g1_small(const uint32_t* __restrict__ u, size_t m, uint32_t* __restrict__ pts) {
  const size_t j = blockIdx.x;
  if (j >= m || threadIdx.x) return;
  fp x;
  ld_f<fp>(x, u + 12 * j);
  st_jac_aos<fp>(pts, j, swu_jac(sswu_g1(x)));
}

__global__ __launch_bounds__(64) void k_add_iso_g1_small(const uint32_t* __restrict__ pts, size_t n, uint32_t* __restrict__ q_out) {
  const size_t i = gtid();
  if (i >= n) return;
  const jac<fp> p0 = ld_jac_aos<fp>(pts, 2 * i), p1 = ld_jac_aos<fp>(pts, 2 * i + 1);
  jac<fp> s;
  const jac<fp> q = jac_add_distinct(s, p0, p1) ? iso11_jac(s) : jac_add(iso11_jac(p0), iso11_jac(p1));
  st_jac_aos<fp>(q_out, i, q);
}

size_t hash_small_tmp_bytes(int sig_g2, size_t n) {
  return sig_g2 ? hash_tmp_bytes(1, n) : n * (24 + 72) * 4;
}

hipError_t launch_hash_small(int sig_g2, const uint64_t* rounds, const uint8_t* prevs, size_t prev_stride, const uint32_t* prev_lens,
                             const uint8_t* msgs32, size_t n, int chained, int dst_id, uint8_t* status, uint32_t* q_out,
                             uint32_t* tmp, hipStream_t st) {
  if (!n) return hipSuccess;
  if (sig_g2) return launch_hash(1, rounds, prevs, prev_stride, prev_lens, msgs32, n, chained, dst_id, status, q_out, tmp, st);
  uint32_t* pts = tmp + 24 * n;
  hipLaunchKernelGGL(k_h2f_g1_small, dim3(nblk(n, 64)), dim3(64), 0, st, rounds, prevs, prev_stride, prev_lens, msgs32, n,
                     chained, dst_id, status, tmp);
  hipLaunchKernelGGL(k_sswu_g1_small, dim3((unsigned)(2 * n)), dim3(64), 0, st, (const uint32_t*)tmp, 2 * n, pts);
  hipLaunchKernelGGL(k_add_iso_g1_small, dim3(nblk(n, 64)), dim3(64), 0, st, (const uint32_t*)pts, n, q_out);
  return hipGetLastError();
}

hipError_t launch_dec_sig(int sig_g2, const uint8_t* sigs, size_t stride, size_t n, uint8_t* status, uint32_t* sig_aff,
                          uint8_t* rand_out, hipStream_t st) {
  if (!n) return hipSuccess;
  if (sig_g2)
    hipLaunchKernelGGL(k_dec_sig_g2, dim3(nblk(n, 256)), dim3(256), 0, st, sigs, stride, n, status, sig_aff, rand_out);
  else
    hipLaunchKernelGGL(k_dec_sig_g1, dim3(nblk(n, 64)), dim3(64), 0, st, sigs, stride, n, status, sig_aff, rand_out);
  return hipGetLastError();
}

hipError_t launch_sub_flag(int sig_g2, size_t n, const uint8_t* status, const uint32_t* sig_aff, uint8_t* sub_bad, hipStream_t st) {
  if (!n) return hipSuccess;
  if (sig_g2) hipLaunchKernelGGL(k_sub_flag<fp2>, dim3(nblk(n, 64)), dim3(64), 0, st, n, status, sig_aff, sub_bad);
  else hipLaunchKernelGGL(k_sub_flag<fp>, dim3(nblk(n, 64)), dim3(64), 0, st, n, status, sig_aff, sub_bad);
  return hipGetLastError();
}

hipError_t launch_and_subgroup(size_t n, const uint8_t* sub_bad, uint8_t* verdict, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_and_subgroup, dim3(nblk(n, 64)), dim3(64), 0, st, n, sub_bad, verdict);
  return hipGetLastError();
}

// ---------------------------------------------------------------- prep: messages -> hash points (no cofactor)
// G1 (fused): hash_to_curve without clear_cofactor, one round per lane
__global__ __launch_bounds__(256, occ<fp>::W) void k_prep_msg_g1(const uint64_t* __restrict__ rounds, const uint8_t* __restrict__ prevs,
                                                            size_t prev_stride, const uint32_t* __restrict__ prev_lens,
                                                            const uint8_t* __restrict__ msgs32, size_t n, int chained, int dst_id,
                                                            uint8_t* __restrict__ status, uint32_t* __restrict__ q_out) {
  size_t i = gtid();
  if (i >= n) return;
  const sha_h d = message_of(rounds, prevs, prev_stride, prev_lens, msgs32, chained, i, status);
  st_jac_aos<fp>(q_out, i, h2c_g1_noclear(d, dst_id));
}

// G1, a large local batch (launch_round_g1_ride): the round's hash and its signature decode on one lane, so that the
// decode's square-root chain carries the inverse that makes the sum of the two SSWU points affine (h2c.hpp
// fp_sqrt_ride, g1_sum_pre / g1_sum_post) and the 11-isogeny three plain Horner evaluations (iso11_aff). Outputs are
// dec_sig_g1's (status, the affine sigma, randomness) and k_prep_msg_g1's (a Jacobian representative of the same hash
// point: k_msm_prep28 makes both affine). msg_ok: false rejects the round as message_of does. When the two SSWU points
// share x (never for hashed inputs) the chain rides on c = 1 and the lane takes h2c_g1_map in a divergent branch, on
// the u0, u1 it parked in its q_out slot (24 of the slot's 36 words, as the G2 passes park theirs): with the branch
// recomputing them from the message the kernel's scratch frame was 1,088 B a lane against 688.
// LATE: the isogeny is left to the batch, once per MSM row sum. The lane stops after g1_sum_post and
// stores the affine E1' point in the MSM's 28-bit form at q28 + 32 i, and sigma there too (s28 + 32 i): no
// k_msm_prep28 launch follows. q_out then holds only the parking slot. When the two SSWU points share x the divergent
// branch doubles on E1' (the curve's own A', one in-lane inversion) or, for opposite points, rejects the round: the
// identity is no valid signature's message (k_msm_prep28's verdict for it on the other path).
template <bool LATE>
DH_DEV void round_g1_ride(const fp& u0, const fp& u1, bool msg_ok, const uint8_t* __restrict__ s, size_t i,
                          uint8_t* __restrict__ status, uint32_t* __restrict__ sig_aff, uint8_t* __restrict__ rand_out,
                          uint32_t* __restrict__ q_out, uint32_t* __restrict__ s28, uint32_t* __restrict__ q28) {
  st_f<fp>(q_out + 36 * i, u0);
  st_f<fp>(q_out + 36 * i + 12, u1);
  g1_sum_mid m;
  fp c;
  const bool distinct = g1_sum_pre(m, c, sswu_g1(u0), sswu_g1(u1));
  c = fp_select(distinct, c, fp_one());
  fp inv_c;
  {
    aff<fp> a;
    uint8_t st = g1_decompress_ride(a, inv_c, s, c);
    if (rand_out) st_digest(rand_out + 32 * i, sha256_aligned<48>(s));
    if (st != DEC_OK) {
      a.x = fp{};
      a.y = fp{};
      st = DEC_BAD;  // infinity signatures are rejected like kilic's engine + kyber's verify
    }
    status[i] = msg_ok ? st : (uint8_t)DEC_BAD;
    st_aff_aos<fp>(sig_aff, i, a);
    if constexpr (LATE) {
      st28(s28 + 2 * W28 * i, f28_from_fp(a.x));
      st28(s28 + 2 * W28 * i + W28, f28_from_fp(a.y));
    }
  }
  if constexpr (LATE) {
    aff<fp> q;
    if (distinct) {
      q = g1_sum_post(m, inv_c);
    } else {
      fp v0, v1;
      ld_f<fp>(v0, q_out + 36 * i);
      ld_f<fp>(v1, q_out + 36 * i + 12);
      const swu_out<fp> p0 = sswu_g1(v0);
      const fp y1 = sswu_g1(v1).y;
      if (fp_eq(p0.y, y1)) {
        q = e1p_dbl_aff(p0);
      } else {
        q = aff<fp>{fp{}, fp{}};
        status[i] = DEC_BAD;
      }
    }
    st28(q28 + 2 * W28 * i, f28_from_fp(q.x));
    st28(q28 + 2 * W28 * i + W28, f28_from_fp(q.y));
  } else {
    if (distinct) {
      st_jac_aos<fp>(q_out, i, iso11_aff(g1_sum_post(m, inv_c)));
    } else {
      fp v0, v1;
      ld_f<fp>(v0, q_out + 36 * i);
      ld_f<fp>(v1, q_out + 36 * i + 12);
      st_jac_aos<fp>(q_out, i, h2c_g1_map(v0, v1));
    }
  }
}

template <bool LATE>
__global__ __launch_bounds__(256, occ<fp>::W) void k_round_g1_ride(const uint64_t* __restrict__ rounds, const uint8_t* __restrict__ prevs,
                                                              size_t prev_stride, const uint32_t* __restrict__ prev_lens,
                                                              const uint8_t* __restrict__ msgs32, size_t n, int chained, int dst_id,
                                                              const uint8_t* __restrict__ sigs, size_t stride,
                                                              uint8_t* __restrict__ status, uint32_t* __restrict__ sig_aff,
                                                              uint8_t* __restrict__ rand_out, uint32_t* __restrict__ q_out,
                                                              uint32_t* __restrict__ s28, uint32_t* __restrict__ q28) {
  size_t i = gtid();
  if (i >= n) return;
  sha_h d;
  bool msg_ok = true;
  if (msgs32) d = message_of(nullptr, nullptr, 0, nullptr, msgs32, 0, i, nullptr);
  else msg_ok = beacon_digest(d, rounds, prevs, prev_stride, prev_lens, chained, i);
  uint32_t b[4][8];
  xmd32<4>(b, d, dst_id);
  round_g1_ride<LATE>(fp_from_be512(b[0], b[1]), fp_from_be512(b[2], b[3]), msg_ok, sigs + i * stride, i, status, sig_aff,
                      rand_out, q_out, s28, q28);
}

// the test entry's kernels (dh_g1_round_prep_debug): round_g1_ride from given u0, u1 (2 x 48 big-endian bytes a round,
// canonical), then sigma and the hash point as canonical affine x || y (2 x 48 big-endian bytes each; the identity,
// and a rejected signature, as zeros)
template <bool LATE>
__global__ __launch_bounds__(256, occ<fp>::W) void k_round_g1_ride_debug(const uint8_t* __restrict__ u, size_t n,
                                                                    const uint8_t* __restrict__ sigs, size_t stride,
                                                                    uint8_t* __restrict__ status, uint32_t* __restrict__ sig_aff,
                                                                    uint32_t* __restrict__ q_out, uint32_t* __restrict__ s28,
                                                                    uint32_t* __restrict__ q28) {
  size_t i = gtid();
  if (i >= n) return;
  fp u0, u1;
  be48_words(u0.v, u + 96 * i, false);
  be48_words(u1.v, u + 96 * i + 48, false);
  round_g1_ride<LATE>(fp_to_mont(u0), fp_to_mont(u1), true, sigs + i * stride, i, status, sig_aff, nullptr, q_out, s28, q28);
}
__global__ __launch_bounds__(64) void k_round_g1_debug_out(size_t n, const uint32_t* __restrict__ sig_aff,
                                                           const uint32_t* __restrict__ q_pts, uint8_t* __restrict__ sig_out,
                                                           uint8_t* __restrict__ q_out) {
  size_t i = gtid();
  if (i >= n) return;
  const aff<fp> s = ld_aff_aos<fp>(sig_aff, i);
  st_be48(sig_out + 96 * i, fp_from_mont(s.x));
  st_be48(sig_out + 96 * i + 48, fp_from_mont(s.y));
  const jac<fp> q = ld_jac_aos<fp>(q_pts, i);
  aff<fp> a{fp{}, fp{}};
  if (!jac_is_inf(q)) a = jac_to_aff(q);
  st_be48(q_out + 96 * i, fp_from_mont(a.x));
  st_be48(q_out + 96 * i + 48, fp_from_mont(a.y));
}

// the LATE form's outputs (dh_g1_round_prep_late_debug): sigma and the E1' point read back from the 28-bit arrays the
// MSM reads, canonical affine x || y; the identity (a rejected round) is stored as zeros
__global__ __launch_bounds__(64) void k_round_g1_late_debug_out(size_t n, const uint32_t* __restrict__ s28,
                                                                const uint32_t* __restrict__ q28, uint8_t* __restrict__ sig_out,
                                                                uint8_t* __restrict__ q_out) {
  size_t i = gtid();
  if (i >= n) return;
  st_be48(sig_out + 96 * i, fp_from_mont(f28_to_fp(ld28(s28 + 2 * W28 * i))));
  st_be48(sig_out + 96 * i + 48, fp_from_mont(f28_to_fp(ld28(s28 + 2 * W28 * i + W28))));
  st_be48(q_out + 96 * i, fp_from_mont(f28_to_fp(ld28(q28 + 2 * W28 * i))));
  st_be48(q_out + 96 * i + 48, fp_from_mont(f28_to_fp(ld28(q28 + 2 * W28 * i + W28))));
}

// the LATE form's fallback (verify_core, level 0 did not end the batch): the isogeny per round after all, into the
// Jacobian hash points the other form writes; k_msm_prep28 follows and rejects a point in the isogeny's kernel (Z = 0)
__global__ __launch_bounds__(256, occ<fp>::W) void k_iso_late_fallback(size_t n, const uint8_t* __restrict__ status,
                                                                  const uint32_t* __restrict__ q28, uint32_t* __restrict__ q_pts) {
  size_t i = gtid();
  if (i >= n || status[i] != DEC_OK) return;
  const aff<fp> q{f28_to_fp(ld28(q28 + 2 * W28 * i)), f28_to_fp(ld28(q28 + 2 * W28 * i + W28))};
  st_jac_aos<fp>(q_pts, i, iso11_aff(q));
}

// G2 in three passes. The G2 map keeps more Fp2 values live than one lane's 256 VGPRs hold (fused, the kernel
// needed 19.3 KB of scratch per lane, and 8 such 1M-round dispatches in flight failed to launch), so the state
// between the passes goes through HBM: u0, u1 (192 B per round) and the two SSWU points on E2' (576 B per
// round), each written and read once (~1.5 KB per round against ~1.3 M integer products of work).
// pass 1: message -> expand_message_xmd -> hash_to_field: u0, u1 (Montgomery Fp2), 48 words per round
__global__ __launch_bounds__(256) void k_h2f_g2(const uint64_t* __restrict__ rounds, const uint8_t* __restrict__ prevs,
                                                size_t prev_stride, const uint32_t* __restrict__ prev_lens,
                                                const uint8_t* __restrict__ msgs32, size_t n, int chained, int dst_id,
                                                uint8_t* __restrict__ status, uint32_t* __restrict__ u_out) {
  size_t i = gtid();
  if (i >= n) return;
  const sha_h d = message_of(rounds, prevs, prev_stride, prev_lens, msgs32, chained, i, status);
  uint32_t b[8][8];
  xmd32<8>(b, d, dst_id);
  const fp2 u0 = {fp_from_be512(b[0], b[1]), fp_from_be512(b[2], b[3])};
  const fp2 u1 = {fp_from_be512(b[4], b[5]), fp_from_be512(b[6], b[7])};
  st_f<fp2>(u_out + 48 * i, u0);
  st_f<fp2>(u_out + 48 * i + 24, u1);
}

// pass 2: one SSWU map per lane (2 per round), the point on E2' as Jacobian (Z = xd)
__global__ __launch_bounds__(256, 2) void k_sswu_g2(const uint32_t* __restrict__ u, size_t m, uint32_t* __restrict__ pts) {
  size_t j = gtid();
  if (j >= m) return;
  fp2 x;
  ld_f<fp2>(x, u + 24 * j);
  st_jac_aos<fp2>(pts, j, swu_jac(sswu_g2(x)));
}

// pass 3: Q = iso3(P0 + P1) (h2c_g2_noclear's order: one isogeny after the addition on E2'). When the two SSWU
// points share x (never for honest inputs) the round is listed in exc[] and k_add_iso_g2_exc takes the textbook
// order, two isogenies then the addition on E2, on a small grid.
__global__ __launch_bounds__(256, 2) void k_add_iso_g2(const uint32_t* __restrict__ pts, size_t n, uint32_t* __restrict__ q_out,
                                                       uint32_t* __restrict__ exc) {
  size_t i = gtid();
  if (i >= n) return;
  jac<fp2> s;
  if (!jac_add_distinct_mem(s, pts + 144 * i, pts + 144 * i + 72)) {
    exc[1 + atomicAdd(exc, 1u)] = (uint32_t)i;
    return;
  }
  st_jac_aos<fp2>(q_out, i, iso3_jac_lean(s));
}

constexpr unsigned EXC_THREADS = 64;
__global__ __launch_bounds__(EXC_THREADS, 1) void k_add_iso_g2_exc(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ exc,
                                                                   uint32_t* __restrict__ q_out) {
  const uint32_t cnt = exc[0];
  for (uint32_t k = threadIdx.x; k < cnt; k += EXC_THREADS) {
    const uint32_t i = exc[1 + k];
    const jac<fp2> p0 = ld_jac_aos<fp2>(pts, 2 * (size_t)i), p1 = ld_jac_aos<fp2>(pts, 2 * (size_t)i + 1);
    st_jac_aos<fp2>(q_out, i, jac_add(iso3_jac(p0), iso3_jac(p1)));
  }
}

// ---------------------------------------------------------------- prep: messages of any length (AuthScheme)
// The same two kernels for message i = msgs[msg_off[i] .. msg_off[i + 1]) instead of a 32-byte digest (xmd_any,
// sha256.hpp): kyber's sign/bls Verify hashes the message as given. Outputs as above: G1 the hash point before
// cofactor clearing, G2 u0, u1 for the unchanged k_sswu_g2 / k_add_iso_g2 passes.
__global__ __launch_bounds__(256, occ<fp>::W) void k_prep_msgv_g1(const uint8_t* __restrict__ msgs, const uint32_t* __restrict__ msg_off,
                                                             size_t n, int dst_id, uint32_t* __restrict__ q_out) {
  size_t i = gtid();
  if (i >= n) return;
  const uint32_t lo = msg_off[i];
  uint32_t b[4][8];
  xmd_any<4>(b, msgs + lo, msg_off[i + 1] - lo, dst_id);
  st_jac_aos<fp>(q_out, i, h2c_g1_map(fp_from_be512(b[0], b[1]), fp_from_be512(b[2], b[3])));
}

__global__ __launch_bounds__(256) void k_h2fv_g2(const uint8_t* __restrict__ msgs, const uint32_t* __restrict__ msg_off, size_t n,
                                                 int dst_id, uint32_t* __restrict__ u_out) {
  size_t i = gtid();
  if (i >= n) return;
  const uint32_t lo = msg_off[i];
  uint32_t b[8][8];
  xmd_any<8>(b, msgs + lo, msg_off[i + 1] - lo, dst_id);
  const fp2 u0 = {fp_from_be512(b[0], b[1]), fp_from_be512(b[2], b[3])};
  const fp2 u1 = {fp_from_be512(b[4], b[5]), fp_from_be512(b[6], b[7])};
  st_f<fp2>(u_out + 48 * i, u0);
  st_f<fp2>(u_out + 48 * i + 24, u1);
}

// ---------------------------------------------------------------- RLC scalars
// r_i = first 16 bytes of SHA-256(seed[32] || i_be64), 0 for rounds that failed decoding.
__global__ __launch_bounds__(256) void k_scalars(const uint32_t* __restrict__ seed_words, size_t n,
                                                 const uint8_t* __restrict__ status, int parts, uint4* __restrict__ scal) {
  size_t i = gtid();
  if (i >= n) return;
  uint32_t w[16];
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = seed_words[j];
  w[8] = (uint32_t)((uint64_t)i >> 32);
  w[9] = (uint32_t)i;
  w[10] = 0x80000000u;
#pragma unroll
  for (int j = 11; j < 15; j++) w[j] = 0;
  w[15] = 40 * 8;
  sha_h s = sha_iv();
  sha_compress(s, w);
  // little-endian words of a 127-bit integer (top bit cleared: the MSM's signed window digits need one spare
  // bit; the batch check's soundness error is 2^-127 per group), or with the endomorphism split two 63-bit
  // halves a, b: the round's scalar is a + b*mu mod r (mu = the endomorphism's eigenvalue, -z^2 on G1 or z on
  // G2, |mu| > 2^63, so distinct (a, b) give distinct scalars: soundness error 2^-126 per group), or on G2 four
  // 31-bit parts a, b, c, d: the scalar a + b z + c z^2 + d z^3 (psi = [z] on G2), |value| < 2^31 (1 + 2^64 +
  // 2^128 + 2^192) < r / 2, so distinct parts give distinct scalars: soundness error 2^-124 per group
  uint4 r = parts == 4   ? make_uint4(s.h[3] & 0x7fffffffu, s.h[2] & 0x7fffffffu, s.h[1] & 0x7fffffffu, s.h[0] & 0x7fffffffu)
            : parts == 2 ? make_uint4(s.h[3], s.h[2] & 0x7fffffffu, s.h[1], s.h[0] & 0x7fffffffu)
                         : make_uint4(s.h[3], s.h[2], s.h[1], s.h[0] & 0x7fffffffu);
  if (status && status[i] != DEC_OK) r = make_uint4(0, 0, 0, 0);
  scal[i] = r;
}

// ---------------------------------------------------------------- key decode
// Thread 0 decodes the point (square root, no subgroup test), then two waves run side by side: wave 0's first lane the
// subgroup test, wave 1's first lane (G2 keys: the G1-signature schemes) [h_eff] pk, so the batch check can read
// e([h_eff] B, pk) as e(B, [h_eff] pk) and skip the per-check cofactor clearing (k_vm_prep_groups). One lane did all
// three in a row: 6.8 ms for a G2 key (k_decode_key<fp2>, profiles/r06/rocprof_single_beacon_r06d.csv), the cost
// of a key-cache miss.
template <class K>
__global__ __launch_bounds__(128) void k_decode_key(const uint8_t* __restrict__ pk, uint32_t* __restrict__ key_aff,
                                                    uint8_t* __restrict__ ok) {
  __shared__ int st_sh, sub_sh;
  const int t = threadIdx.x;
  if (t == 0) {
    aff<K> a;
    uint8_t st;
    if constexpr (sizeof(K) == sizeof(fp)) st = g1_decompress(a, pk, false);
    else st = g2_decompress(a, pk, false);
    if (st != DEC_OK) {
      a.x = K{};
      a.y = K{};
    }
    st_aff_aos<K>(key_aff, 0, a);
    st_sh = st;
    sub_sh = 1;
  }
  __syncthreads();
  const bool dec_ok = st_sh == DEC_OK;
  if (t == 0 && dec_ok) {
    bool in;
    if constexpr (sizeof(K) == sizeof(fp)) in = g1_in_subgroup28([&] { return ld_aff_aos<fp>(key_aff, 0); });
    else in = g2_in_subgroup28([&] { return ld_aff_aos<fp2>(key_aff, 0); });
    sub_sh = in ? 1 : 0;
  }
  if constexpr (sizeof(K) == sizeof(fp2)) {
    if (t == 64) {
      aff<fp2> h{fp2{}, fp2{}};
      if (dec_ok) {
        const aff<fp2> a = ld_aff_aos<fp2>(key_aff, 0);
        h = jac_to_aff(jac_add(jac_mul_uabs(a), jac_from_aff(a)));  // G1's h_eff = 1 - z = |z| + 1, applied to pk
      }
      st_aff_aos<fp2>(key_aff, 1, h);
    }
  }
  __syncthreads();
  if (t == 0) {
    const uint8_t st = (uint8_t)st_sh == DEC_OK && !sub_sh ? (uint8_t)DEC_BAD : (uint8_t)st_sh;
    *ok = st;
    if (st != DEC_OK) st_aff_aos<K>(key_aff, 0, aff<K>{K{}, K{}});
  }
}


hipError_t launch_prep(int sig_g2, const uint8_t* sigs, size_t stride, size_t n, uint8_t* status, uint32_t* sig_aff,
                       uint8_t* rand_out, hipStream_t st, bool defer_sub) {
  if (!n) return hipSuccess;
  if (sig_g2) {
    hipLaunchKernelGGL(k_dec_sig_g2, dim3(nblk(n, 256)), dim3(256), 0, st, sigs, stride, n, status, sig_aff, rand_out);
    if (!defer_sub) hipLaunchKernelGGL(k_sub_sig_g2, dim3(nblk(n, 256)), dim3(256), 0, st, n, status, sig_aff);
  } else if (defer_sub)
    hipLaunchKernelGGL(k_dec_sig_g1_batch, dim3(nblk(n, 256)), dim3(256), 0, st, sigs, stride, n, status, sig_aff, rand_out);
  else
    hipLaunchKernelGGL(k_prep_sig<fp>, dim3(nblk(n, 256)), dim3(256), 0, st, sigs, stride, n, status, sig_aff, rand_out);
  return hipGetLastError();
}

hipError_t launch_sub_exact(int sig_g2, size_t n, uint8_t* status, uint32_t* sig_aff, uint8_t* sub_bad, uint32_t* nbad,
                            hipStream_t st) {
  hipError_t e = hipMemsetAsync(nbad, 0, 4, st);
  if (e != hipSuccess || !n) return e;
  if (sig_g2) {
    hipLaunchKernelGGL(k_sub_flag_batch_g2, dim3(nblk(n, 256)), dim3(256), 0, st, n, (const uint8_t*)status,
                       (const uint32_t*)sig_aff, sub_bad);
    hipLaunchKernelGGL(k_sub_reject<fp2>, dim3(nblk(n, 256)), dim3(256), 0, st, n, (const uint8_t*)sub_bad, status, sig_aff, nbad);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_sub_flag_batch, dim3(nblk(n, 256)), dim3(256), 0, st, n, (const uint8_t*)status, (const uint32_t*)sig_aff,
                     sub_bad);
  hipLaunchKernelGGL(k_sub_reject<fp>, dim3(nblk(n, 256)), dim3(256), 0, st, n, (const uint8_t*)sub_bad, status, sig_aff, nbad);
  return hipGetLastError();
}


hipError_t launch_scalars(const uint32_t* seed_words, size_t n, const uint8_t* status, uint4* scal, int parts, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_scalars, dim3(nblk(n, 256)), dim3(256), 0, st, seed_words, n, status, parts, scal);
  return hipGetLastError();
}

hipError_t launch_decode_key(int key_g2, const uint8_t* pk, uint32_t* key_aff, uint8_t* ok, hipStream_t st) {
  if (key_g2) hipLaunchKernelGGL(k_decode_key<fp2>, dim3(1), dim3(128), 0, st, pk, key_aff, ok);
  else hipLaunchKernelGGL(k_decode_key<fp>, dim3(1), dim3(128), 0, st, pk, key_aff, ok);
  return hipGetLastError();
}


// G2: the SSWU points (2 x 72 words per round), then the exceptional-round list (count + n indices)
size_t hash_tmp_bytes(int sig_g2, size_t n) { return sig_g2 ? n * 2 * 72 * 4 + (n + 1) * 4 : 0; }

// G2 passes 2 and 3 over the u0, u1 that pass 1 left in q_out
static hipError_t hash_g2_map(size_t n, uint32_t* q_out, uint32_t* tmp, hipStream_t st) {
  hipLaunchKernelGGL(k_sswu_g2, dim3(nblk(2 * n, 256)), dim3(256), 0, st, (const uint32_t*)q_out, 2 * n, tmp);
  uint32_t* exc = tmp + n * 2 * 72;
  hipError_t e = hipMemsetAsync(exc, 0, 4, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_add_iso_g2, dim3(nblk(n, 256)), dim3(256), 0, st, (const uint32_t*)tmp, n, q_out, exc);
  hipLaunchKernelGGL(k_add_iso_g2_exc, dim3(1), dim3(EXC_THREADS), 0, st, (const uint32_t*)tmp, (const uint32_t*)exc, q_out);
  return hipGetLastError();
}

hipError_t launch_hash(int sig_g2, const uint64_t* rounds, const uint8_t* prevs, size_t prev_stride, const uint32_t* prev_lens,
                       const uint8_t* msgs32, size_t n, int chained, int dst_id, uint8_t* status, uint32_t* q_out, uint32_t* tmp,
                       hipStream_t st) {
  if (!n) return hipSuccess;
  if (!sig_g2) {
    hipLaunchKernelGGL(k_prep_msg_g1, dim3(nblk(n, 256)), dim3(256), 0, st, rounds, prevs, prev_stride, prev_lens, msgs32, n,
                       chained, dst_id, status, q_out);
    return hipGetLastError();
  }
  // u0, u1 of round i go to q_out (48 of its 72 words per round), the SSWU points to tmp
  hipLaunchKernelGGL(k_h2f_g2, dim3(nblk(n, 256)), dim3(256), 0, st, rounds, prevs, prev_stride, prev_lens, msgs32, n, chained,
                     dst_id, status, q_out);
  return hash_g2_map(n, q_out, tmp, st);
}

hipError_t launch_round_g1_ride(const uint64_t* rounds, const uint8_t* prevs, size_t prev_stride, const uint32_t* prev_lens,
                                const uint8_t* msgs32, size_t n, int chained, int dst_id, const uint8_t* sigs, size_t stride,
                                uint8_t* status, uint32_t* sig_aff, uint8_t* rand_out, uint32_t* q_out, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_round_g1_ride<false>, dim3(nblk(n, 256)), dim3(256), 0, st, rounds, prevs, prev_stride, prev_lens, msgs32, n,
                     chained, dst_id, sigs, stride, status, sig_aff, rand_out, q_out, (uint32_t*)nullptr, (uint32_t*)nullptr);
  return hipGetLastError();
}

hipError_t launch_round_g1_ride_late(const uint64_t* rounds, const uint8_t* prevs, size_t prev_stride, const uint32_t* prev_lens,
                                     const uint8_t* msgs32, size_t n, int chained, int dst_id, const uint8_t* sigs, size_t stride,
                                     uint8_t* status, uint32_t* sig_aff, uint8_t* rand_out, uint32_t* q_out, uint32_t* s28,
                                     uint32_t* q28, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_round_g1_ride<true>, dim3(nblk(n, 256)), dim3(256), 0, st, rounds, prevs, prev_stride, prev_lens, msgs32, n,
                     chained, dst_id, sigs, stride, status, sig_aff, rand_out, q_out, s28, q28);
  return hipGetLastError();
}

hipError_t launch_iso_late_fallback(size_t n, const uint8_t* status, const uint32_t* q28, uint32_t* q_pts, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_iso_late_fallback, dim3(nblk(n, 256)), dim3(256), 0, st, n, status, q28, q_pts);
  return hipGetLastError();
}

hipError_t launch_round_g1_ride_debug(const uint8_t* u, const uint8_t* sigs, size_t n, uint8_t* status, uint32_t* sig_aff,
                                      uint32_t* q_pts, uint8_t* sig_out, uint8_t* q_out, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_round_g1_ride_debug<false>, dim3(nblk(n, 256)), dim3(256), 0, st, u, n, sigs, (size_t)48, status, sig_aff,
                     q_pts, (uint32_t*)nullptr, (uint32_t*)nullptr);
  hipLaunchKernelGGL(k_round_g1_debug_out, dim3(nblk(n, 64)), dim3(64), 0, st, n, (const uint32_t*)sig_aff,
                     (const uint32_t*)q_pts, sig_out, q_out);
  return hipGetLastError();
}

hipError_t launch_round_g1_ride_late_debug(const uint8_t* u, const uint8_t* sigs, size_t n, uint8_t* status, uint32_t* sig_aff,
                                           uint32_t* q_pts, uint32_t* s28, uint32_t* q28, uint8_t* sig_out, uint8_t* q_out,
                                           hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_round_g1_ride_debug<true>, dim3(nblk(n, 256)), dim3(256), 0, st, u, n, sigs, (size_t)48, status, sig_aff,
                     q_pts, s28, q28);
  hipLaunchKernelGGL(k_round_g1_late_debug_out, dim3(nblk(n, 64)), dim3(64), 0, st, n, (const uint32_t*)s28, (const uint32_t*)q28,
                     sig_out, q_out);
  return hipGetLastError();
}

hipError_t launch_hash_var(int sig_g2, const uint8_t* msgs, const uint32_t* msg_off, size_t n, int dst_id, uint32_t* q_out,
                           uint32_t* tmp, hipStream_t st) {
  if (!n) return hipSuccess;
  if (!sig_g2) {
    hipLaunchKernelGGL(k_prep_msgv_g1, dim3(nblk(n, 256)), dim3(256), 0, st, msgs, msg_off, n, dst_id, q_out);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_h2fv_g2, dim3(nblk(n, 256)), dim3(256), 0, st, msgs, msg_off, n, dst_id, q_out);
  return hash_g2_map(n, q_out, tmp, st);
}

DH_COUNTER_ACCESSOR(prep)

}  // namespace dh
