// Host-side declarations of the kernel launchers in kernels.hip (internal to libdrandhip).
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace dh {

// Pippenger geometry for one MSM level: entries are cut into groups of `gsize` consecutive entries;
// each group has nwin windows of c bits (signed digits) with nbuck = 2^(c-1) + 1 buckets (index = |digit|,
// 0 unused); bucket reduction splits the digits of a window into nseg segments of seglen digits.
// Scalars: 127-bit integers (halves = 1), or with the endomorphism split (halves = 2) a pair (a, b) of 63-bit
// integers in one uint4 (x, y = a; z, w = b): entry e then stands for two points, P_e with scalar a and
// endo(P_e) (stored half_stride points further on) with scalar b, i.e. P_e with the scalar a + b*mu mod r.
// G2 (halves = 4): four 31-bit parts (x, y, z, w) for P_e, psi(P_e), psi^2(P_e), psi^3(P_e) (part h at h * half_stride
// points on), i.e. the scalar a + b z + c z^2 + d z^3 (psi = [z] on G2). A G2 batch that takes the batched subgroup
// test runs with halves = 2: P_e and psi(P_e) with two 63-bit halves, the scalar a + b z.
struct msm_geom {
  uint32_t gsize;
  int c;
  int nwin;
  uint32_t nbuck;
  uint32_t nseg;
  uint32_t seglen;
  uint32_t halves;       // 1; 2 for the endomorphism split (G1 phi, G2 psi); 4 for the G2 four-part psi split
  uint32_t half_stride;  // point index offset of endo(P) (halves = 2) / of each psi power (halves = 4)
  // 1 (halves = 2, G1 level 0 with the hash set on E1'): half h of a scalar keys window row h * nwin + w of
  // its group and its entry is the point index itself: no image, the endomorphism is applied once to the sum of rows
  // nwin .. 2 nwin - 1 (k_msm_windows28_split). Each half is recoded on its own, as for split = 0. half_stride stays
  // the round count (the bucket pass's skip test).
  uint32_t split = 0;
  // 1 (split = 1, the G1 level 0 on one scalar half): only half 0 of a scalar is keyed, the round's scalar
  // is a alone. nwin window rows per group and nwin entries per point, the row sums are plain rows of one scalar
  // (k_msm_windows28 after the hash rows' isogeny). halves stays 2: half_scalar and the 63-bit recoding are a half's.
  uint32_t half0 = 0;
};
// halves of a scalar that key window rows
__host__ __device__ inline uint32_t msm_keyed(const msm_geom& g) { return g.half0 ? 1u : g.halves; }
inline size_t msm_entries(const msm_geom& g, size_t m) { return m * (size_t)g.nwin * msm_keyed(g); }
// window rows (of nbuck keys) per group
__host__ __device__ inline uint32_t msm_rows(const msm_geom& g) { return (uint32_t)g.nwin * (g.split ? msm_keyed(g) : 1u); }

// device workspace of one MSM level (sized by the caller from msm_geom)
struct msm_ws {
  uint32_t* cnt;       // nkeys
  uint32_t* off;       // nkeys + 1
  uint32_t* scan_tmp;  // ceil(nkeys / 4096)
  uint32_t* list;      // msm_entries(g, m)
  uint32_t* buckets;   // nkeys Jacobian points (x2 for launch_msm28: both point sets)
  uint32_t* segs;      // ngroups * nwin * nseg Jacobian points (x2 for launch_msm28)
  uint32_t* out2;      // launch_msm28: 2 * ngroups Jacobian points (sigma sums, then hash sums)
  uint32_t* part;      // balanced bucket pass: 2 Jacobian partial sums per chunk (x2 for launch_msm28)
  uint32_t* meta;      // balanced bucket pass: 2 words per chunk (head kind, tail key)
  size_t max_entries;  // set by launch_msm_sort: upper bound of sorted-list entries (msm_entries)
  uint32_t* runs = nullptr;  // MSM28: the segments' running sums (as many points as segs)
  uint32_t* sub = nullptr;   // batched subgroup test (launch_sub_batch): sub_batch_tmp_bytes of scratch
};

// balanced bucket accumulation: entries per chunk, and workspace sizes for `max_entries` list entries
inline uint32_t msm_chunk_len(size_t max_entries, size_t cap = 32, size_t target_chunks = 262144) {
  // the shortest chunk: 8 entries (a 131k-round shard at c = 16 holds ~8 entries per bucket, so shorter chunks cut
  // most buckets and leave their sums to k_msm_bucket_fix: 4 -> 8 took the shard's MSM from 2.75 to 2.42 ms,
  // profiles/r03k); DRANDHIP_MSM_LMIN overrides it for experiments
  static const size_t lmin = [] {
    const char* e = getenv("DRANDHIP_MSM_LMIN");
    const long v = e ? atol(e) : 0;
    return (size_t)(v >= 1 && v <= 64 ? v : 8);
  }();
  size_t L = max_entries / target_chunks;
  if (L < lmin) L = lmin;
  return (uint32_t)(L > cap ? cap : L);
}
inline size_t msm_nchunks(size_t max_entries) { return max_entries / msm_chunk_len(max_entries) + 2; }
inline size_t msm_part_bytes(size_t max_entries, size_t jac_words, int nsets) {
  return msm_nchunks(max_entries) * 2 * jac_words * 4 * (size_t)nsets;
}
inline size_t msm_meta_bytes(size_t max_entries) { return msm_nchunks(max_entries) * 2 * 4; }

// defer_sub: decode, curve check, randomness and status only (G2: k_dec_sig_g2 without k_sub_sig_g2); the subgroup
// test is left to the batch (launch_sub_batch, or launch_sub_exact when that fails)
hipError_t launch_prep(int sig_g2, const uint8_t* sigs, size_t stride, size_t n, uint8_t* status, uint32_t* sig_aff,
                       uint8_t* rand_out, hipStream_t st, bool defer_sub = false);
// the exact fallback of the batched subgroup test: the per-round test over the n decoded rounds (sub_bad: n bytes of
// scratch); a failing round gets what the fused launch_prep leaves (status DEC_BAD, the zero point); *nbad (device
// word) = the number of failing rounds
hipError_t launch_sub_exact(int sig_g2, size_t n, uint8_t* status, uint32_t* sig_aff, uint8_t* sub_bad, uint32_t* nbad, hipStream_t st);
// small-batch path: the signature pass split at the decoded point (decode + randomness; subgroup test -> sub_bad[i]
// = 1 when a decoded point is not in the subgroup; verdict[i] = 0 where sub_bad[i])
hipError_t launch_dec_sig(int sig_g2, const uint8_t* sigs, size_t stride, size_t n, uint8_t* status, uint32_t* sig_aff,
                          uint8_t* rand_out, hipStream_t st);
hipError_t launch_sub_flag(int sig_g2, size_t n, const uint8_t* status, const uint32_t* sig_aff, uint8_t* sub_bad, hipStream_t st);
hipError_t launch_and_subgroup(size_t n, const uint8_t* sub_bad, uint8_t* verdict, hipStream_t st);
// small-batch path: launch_hash with the G1 hash's two SSWU maps in workgroups of their own (G2: launch_hash);
// tmp: hash_small_tmp_bytes
size_t hash_small_tmp_bytes(int sig_g2, size_t n);
hipError_t launch_hash_small(int sig_g2, const uint64_t* rounds, const uint8_t* prevs, size_t prev_stride, const uint32_t* prev_lens,
                             const uint8_t* msgs32, size_t n, int chained, int dst_id, uint8_t* status, uint32_t* q_out,
                             uint32_t* tmp, hipStream_t st);
// hash points Q_i (before cofactor clearing) of the beacon digests of (rounds, prevs) or of the given 32-byte
// msgs32; a chained record longer than its slot marks status[i] = DEC_BAD. tmp: hash_tmp_bytes(sig_g2, n).
size_t hash_tmp_bytes(int sig_g2, size_t n);
hipError_t launch_hash(int sig_g2, const uint64_t* rounds, const uint8_t* prevs, size_t prev_stride, const uint32_t* prev_lens,
                       const uint8_t* msgs32, size_t n, int chained, int dst_id, uint8_t* status, uint32_t* q_out, uint32_t* tmp,
                       hipStream_t st);
// G1 signatures, a large local batch: launch_prep(defer_sub = true) and launch_hash in one launch, one round per lane,
// the hash point's affine sum on an inverse carried by the signature's square-root chain (k_prep.hip round_g1_ride).
// Same status, sig_aff and rand_out; q_out holds another Jacobian representative of the same hash points.
hipError_t launch_round_g1_ride(const uint64_t* rounds, const uint8_t* prevs, size_t prev_stride, const uint32_t* prev_lens,
                                const uint8_t* msgs32, size_t n, int chained, int dst_id, const uint8_t* sigs, size_t stride,
                                uint8_t* status, uint32_t* sig_aff, uint8_t* rand_out, uint32_t* q_out, hipStream_t st);
// The same launch with the isogeny left to the batch: the hash point leaves as the affine sum of the two
// SSWU points on E1', in the MSM's 28-bit form at q28 + 32 i, and sigma also at s28 + 32 i (launch_msm_prep28's layout
// for the first n points; no images), for the rounds whose status is DEC_OK. q_out keeps only the u0, u1 parking
// slots. A round whose two SSWU points are opposite (the identity; never for hashed inputs) is DEC_BAD.
hipError_t launch_round_g1_ride_late(const uint64_t* rounds, const uint8_t* prevs, size_t prev_stride, const uint32_t* prev_lens,
                                     const uint8_t* msgs32, size_t n, int chained, int dst_id, const uint8_t* sigs, size_t stride,
                                     uint8_t* status, uint32_t* sig_aff, uint8_t* rand_out, uint32_t* q_out, uint32_t* s28,
                                     uint32_t* q28, hipStream_t st);
// the fallback to launch_round_g1_ride's arrays: q_pts[i] = the 11-isogeny's image of the E1' point at q28 + 32 i,
// Jacobian, for the rounds whose status is DEC_OK (launch_msm_prep28 then refills s28 and q28)
hipError_t launch_iso_late_fallback(size_t n, const uint8_t* status, const uint32_t* q28, uint32_t* q_pts, hipStream_t st);
// the same per-round code from given u0 || u1 (96 canonical big-endian bytes a round) and 48-byte signatures; sig_out
// and q_out: canonical affine x || y (96 bytes a round), zeros for the identity; sig_aff / q_pts: n x 24 / 36 words
hipError_t launch_round_g1_ride_debug(const uint8_t* u, const uint8_t* sigs, size_t n, uint8_t* status, uint32_t* sig_aff,
                                      uint32_t* q_pts, uint8_t* sig_out, uint8_t* q_out, hipStream_t st);
// launch_round_g1_ride_late's code the same way: q_out = the stored E1' point, s28 / q28: n x 32 words each
hipError_t launch_round_g1_ride_late_debug(const uint8_t* u, const uint8_t* sigs, size_t n, uint8_t* status, uint32_t* sig_aff,
                                           uint32_t* q_pts, uint32_t* s28, uint32_t* q28, uint8_t* sig_out, uint8_t* q_out,
                                           hipStream_t st);
// test infrastructure (k_fieldops.hip, dh_field_ops_debug): lane i runs field operation ops[i] on the operand record
// in + i in_words and writes the result record out + i out_words (zeroed by the caller). Record words a lane may touch:
constexpr size_t FO_SCALARS = 168;    // twelve 14-limb slots, then the scalars s0 .. s7
constexpr size_t FO_IN_WORDS = 176;
constexpr size_t FO_OUT_FLAGS = 84;   // six 14-limb slots, then four flag words
constexpr size_t FO_OUT_WORDS = 88;
bool field_op_known(uint32_t op);
hipError_t launch_field_ops(const uint32_t* ops, const uint32_t* in, size_t in_words, size_t n, uint32_t* out,
                            size_t out_words, hipStream_t st);
// the same hash points for messages of any length, message i = msgs[msg_off[i] .. msg_off[i + 1]) (sign.Scheme.Verify
// in batch: xmd_any, sha256.hpp); tmp: hash_tmp_bytes(sig_g2, n)
hipError_t launch_hash_var(int sig_g2, const uint8_t* msgs, const uint32_t* msg_off, size_t n, int dst_id, uint32_t* q_out,
                           uint32_t* tmp, hipStream_t st);
// RLC scalars from SHA-256(seed || i): 127-bit (glv = 0) or a pair of 63-bit halves (glv = 1, msm_geom.halves = 2);
// 0 for rounds whose status is not DEC_OK (status null: every round gets its scalar)
// parts: 1 = one 127-bit scalar, 2 = two 63-bit halves, 4 = four 31-bit parts (msm_geom halves)
hipError_t launch_scalars(const uint32_t* seed_words, size_t n, const uint8_t* status, uint4* scal, int parts, hipStream_t st);
hipError_t launch_decode_key(int key_g2, const uint8_t* pk, uint32_t* key_aff, uint8_t* ok, hipStream_t st);
hipError_t launch_iota(uint32_t* v, size_t n, hipStream_t st);
hipError_t launch_scan(const uint32_t* cnt, size_t nk, uint32_t* off, uint32_t* tmp, hipStream_t st);
// The RLC MSM on lazily reduced 28-bit points (k_msm.hip MSM28): launch_msm_prep28 converts the batch's sigma
// (affine) and hash points (Jacobian, made affine) with their endomorphism images into S and Q (G1 32 / G2 64 words
// per point, parts x n points each: the images of point i at i + h n; a hash point at infinity marks its round
// DEC_BAD); the workspace's bucket / partial / segment arrays hold 48 / 96-word Jacobian points. parts: 0 = the
// group's usual split (G1 2, G2 4); 2 for a G2 batch on two psi halves (S and Q then hold 2 n points)
hipError_t launch_msm_prep28(int sig_g2, size_t n, uint8_t* status, const uint32_t* sig_aff, const uint32_t* q_pts,
                             uint32_t* S, uint32_t* Q, hipStream_t st, uint32_t sets = 3, int parts = 0);
// one point set (S of launch_msm_prep28) with point / scalar / group indices: ngroups 12 x 32-bit Jacobian sums into out
hipError_t launch_msm28_set(int sig_g2, const msm_geom& g, const uint32_t* pidx, const uint32_t* sidx, const uint32_t* grp,
                            size_t m, size_t ngroups, const uint4* scal, const uint32_t* P, msm_ws& ws, uint32_t* out,
                            hipStream_t st);
hipError_t launch_msm28(int sig_g2, const msm_geom& g, const uint32_t* entries, size_t m, size_t ngroups, const uint4* scal,
                        const uint32_t* S, const uint32_t* Q, msm_ws& ws, uint32_t* outA, uint32_t* outB, hipStream_t st,
                        const uint8_t* skip, bool presorted);
// The batched subgroup test on the sigma buckets a level-0 launch_msm28 of ONE group left in ws (g: that launch's
// geometry, halves == 2 for either group; ws.sub: sub_batch_tmp_bytes(sig_g2, g)): the bit-subset sums T[w][b] of the buckets, each tested for membership.
// A failing T clears pass[0] (the level-0 group) and sub_pass[0], which the launch first sets to 1.
size_t sub_batch_tmp_bytes(int sig_g2, const msm_geom& g);
hipError_t launch_sub_batch(int sig_g2, const msm_geom& g, const msm_ws& ws, uint8_t* pass, uint8_t* sub_pass, hipStream_t st);
hipError_t launch_msm_sort(const msm_geom& g, const uint32_t* pidx, const uint32_t* sidx, const uint32_t* grp, size_t m,
                           size_t ngroups, const uint4* scal, msm_ws& ws, hipStream_t st);
hipError_t launch_group_check(int sig_g2, const uint32_t* A, const uint32_t* B, size_t ngroups, const uint32_t* key_aff,
                              uint8_t* pass, hipStream_t st);
// node-wide check: sum the k (A, B) level-0 partial-sum pairs, record i = [A_i | B_i | status word | pad] at
// parts + i * rec_words (Jacobian AoS); flag[0] (nullable) = 1 when any record's status word is nonzero
hipError_t launch_sum_partials(int sig_g2, const uint32_t* parts, size_t k, size_t rec_words, uint32_t* outA, uint32_t* outB,
                               uint8_t* flag, hipStream_t st);
// res[0] = abandon flag, res[1] = pairing check -> res[2] = 2 abandoned / 1 passed / 0 failed; passed: verdict[i] =
// (status[i] == DEC_OK) for i < n
hipError_t launch_node_mark(size_t n, uint8_t* res, const uint8_t* status, uint8_t* verdict, hipStream_t st);
hipError_t launch_mark_groups(const uint32_t* entries, size_t m, size_t gsize, const uint8_t* pass, const uint8_t* status,
                              uint8_t* verdict, hipStream_t st);
// bisection: out = the entries of the groups with pass == 0, in order; rank[ngroups] = the number of failing groups
// (flags: ngroups words, rank: ngroups + 1, scan_tmp: launch_scan's)
hipError_t launch_compact_failing(const uint32_t* entries, size_t m, size_t gsize, size_t ngroups, const uint8_t* pass,
                                  uint32_t* flags, uint32_t* rank, uint32_t* scan_tmp, uint32_t* out, hipStream_t st);
hipError_t launch_leaf_check(int sig_g2, const uint32_t* entries, size_t m, const uint32_t* sig_aff, const uint32_t* q_pts,
                             const uint32_t* key_aff, const uint8_t* status, uint8_t* verdict, hipStream_t st);

// lane-parallel pairing checks (k_vm.hip): pairs = 2 x 72 words per check, live = 2 bytes, done = 1 byte
// key_h: [h_eff] pk for G1-signature schemes (k_decode_key writes it after the key), or null for [h_eff] B
hipError_t launch_group_check_vm(int sig_g2, const uint32_t* A, const uint32_t* B, size_t ngroups, const uint32_t* key_aff,
                                 const uint32_t* key_h,
                                 uint32_t* pairs, uint8_t* live, uint8_t* pass, hipStream_t st);
// G2-signature group checks with the cofactor clearing inside the pairing program (k_vm.hip k_vm_pairing_c)
size_t group_check_c_pair_words();
hipError_t launch_group_check_vm_c(const uint32_t* A, const uint32_t* B, size_t ngroups, const uint32_t* key_aff, uint32_t* pairs,
                                   uint8_t* live, uint8_t* done, uint8_t* pass, hipStream_t st);
hipError_t launch_leaf_check_vm(int sig_g2, const uint32_t* entries, size_t m, const uint32_t* sig_aff, const uint32_t* q_pts,
                                const uint32_t* key_aff, const uint32_t* key_h, const uint8_t* status, uint32_t* pairs,
                                uint8_t* live, uint8_t* done, uint8_t* verdict, hipStream_t st);

// G2-signature leaves with the hash point's clearing inside the program (NP2C); same buffers as launch_group_check_vm_c
hipError_t launch_leaf_check_vm_c(const uint32_t* entries, size_t m, const uint32_t* sig_aff, const uint32_t* q_pts,
                                  const uint32_t* key_aff, const uint8_t* status, uint32_t* pairs, uint8_t* live, uint8_t* done,
                                  uint8_t* verdict, hipStream_t st);

// G1-signature checks on Jacobian G1 sides (NP2J, no prep kernel): groups (A, B Jacobian AoS) and leaves;
// key_h = [h_eff] pk (affine)
hipError_t launch_group_check_g1j(const uint32_t* A, const uint32_t* B, size_t ngroups, const uint32_t* key_h, uint8_t* pass,
                                  hipStream_t st);
hipError_t launch_leaf_check_g1j(const uint32_t* entries, size_t m, const uint32_t* sig_aff, const uint32_t* q_pts,
                                 const uint32_t* key_h, const uint8_t* status, uint8_t* verdict, hipStream_t st);

hipError_t launch_multi_pairing_vm(const uint32_t* P, const uint32_t* Q, size_t n, uint32_t* pairs, uint8_t* live,
                                   uint32_t* f_tmp, uint8_t* pass, hipStream_t st);

// test infrastructure (k_vm.hip, dh_vm_debug): one workgroup per record runs the pairing interpreter on a
// committed program (tag 0..7: NP1 NP2 ML1 MUL12 FE NP2C NP1J NP2J) or on the caller's (tag < 0: phases = 2 words a
// phase, ops = REC words an op followed by 16 pad words, 16-byte aligned, both already checked), cut to `stop` phases,
// and writes the slot image, nslots x 16 words a record. vm_debug_shape: a committed program's phase count, slot count
// and input words per record (true), or for any other tag the caller's limits VM_MAX_PHASES and VM_SLOTS (false).
constexpr int VM_DEBUG_REC = 32, VM_DEBUG_MAXT = 15, VM_DEBUG_SLOT_WORDS = 16;  // pairing_vm.hpp REC, MAXT; k_vm.hip SW
struct vm_debug_dims {
  int nphases, nslots, in_words;
};
bool vm_debug_shape(int tag, vm_debug_dims* d);
hipError_t launch_vm_debug(int tag, const uint32_t* phases, int nphases, const uint32_t* ops, int nslots, int stop,
                           const uint32_t* in, size_t in_words, size_t n, uint32_t* out, hipStream_t st);

// synthetic signer: q_tmp n x 72 words and h_tmp hash_tmp_bytes(1, n) for G2 signatures (unused for G1)
hipError_t launch_sign(int sig_g2, const uint32_t* sk, const uint64_t* rounds, const uint8_t* prevs, size_t prev_stride,
                       const uint32_t* prev_lens, const uint8_t* msgs32, size_t n, int chained, int dst_id, uint8_t* out,
                       uint32_t* q_tmp, uint32_t* h_tmp, hipStream_t st);
// RFC 9380 hash_to_curve of arbitrary messages / DST, compressed (k_sign.hip)
hipError_t launch_h2c_generic(int g2, const uint8_t* msgs, const uint32_t* off, size_t n, const uint8_t* dst, uint32_t dlen,
                              uint8_t* scratch, size_t sstride, uint8_t* out, hipStream_t st);
hipError_t launch_pubkey(int key_g2, const uint32_t* sk, uint8_t* out, hipStream_t st);

// tbls Recover (k_recover.hip)
hipError_t launch_repack_partials(const uint8_t* raw, size_t n, int sig_len, uint8_t* sigs, uint32_t* idx, hipStream_t st);
hipError_t launch_pubpoly_eval(int key_g2, const uint32_t* commits, int t, int n_nodes, uint32_t* out, hipStream_t st);
hipError_t launch_pair_check(const uint32_t* P, const uint32_t* Q, size_t npairs, int clear_p, int clear_q,
                             const uint8_t* live, uint32_t* f_tmp, uint8_t* skip_tmp, uint8_t* pass, hipStream_t st);
hipError_t launch_partial_leaf(int sig_g2, const uint32_t* list, size_t m, const uint32_t* sig_aff, const uint8_t* status,
                               const uint32_t* share_idx, const uint32_t* round_of, const uint32_t* q_pts,
                               const uint32_t* shares, int n_nodes, uint8_t* ok_out, hipStream_t st);
// per round: round_of for its partials, indices >= n_nodes rejected (status); ok from status after a passed batch
hipError_t launch_partial_meta(const uint32_t* off, size_t n_rounds, const uint32_t* share_idx, int n_nodes, uint32_t* round_of,
                               uint8_t* status, hipStream_t st);
hipError_t launch_clamp_group(const uint32_t* share_idx, size_t np, uint32_t hi, uint32_t* grp, hipStream_t st);
hipError_t launch_ok_from_status(const uint8_t* status, size_t np, uint8_t* ok, hipStream_t st);
// per round: Recover's selection + Lagrange coefficients (sel/key: t words, den: 8t words, lam: lam_words() t words
// per round); lam_set[j] = the round whose lambda rows round j uses (0 when its selected indices equal round 0's, else
// j); *own = the number of rounds j > 0 with their own rows (device word)
size_t lam_words();
hipError_t launch_select_lagrange(const uint32_t* off, const uint8_t* ok, const uint32_t* share_idx, int t, size_t n_rounds,
                                  uint32_t* sel, uint32_t* key, uint32_t* den, uint32_t* lam, uint32_t* lam_set, uint8_t* rok,
                                  uint32_t* own, int g1, hipStream_t st);
// tbl (G2): per valid partial (ok) the odd multiples P, 3P, ..., (2 entries - 1) P affine 28-bit (entries = 4 or 8,
// 64 words each) from the partials' affine points (12 x 32-bit AOS); zs: wnaf_table_scratch_bytes(n, entries) of
// scratch (the batched inversion's Z's); unused for G1
hipError_t launch_mark_selected(const uint32_t* sel, const uint8_t* rok, int t, size_t n_rounds, size_t np, uint8_t* need,
                                hipStream_t st);
hipError_t launch_wnaf_table_g2(const uint32_t* paff, const uint8_t* ok, size_t n, int entries, uint32_t* tbl, uint32_t* zs,
                                hipStream_t st);
size_t wnaf_table_scratch_bytes(size_t n, int entries);
// tmp: lagrange_tmp_bytes(sig_g2) of scratch for the sliced last wave of workgroups (null: no slicing)
// entries: the G2 tables' width (8: waves whose rounds use different bases run the regular windows)
hipError_t launch_lagrange(int sig_g2, const uint32_t* sel, const uint32_t* lam, const uint32_t* lam_set, const uint8_t* ok,
                           int t, size_t n_rounds, const uint32_t* sig_aff, const uint32_t* tbl, int entries, uint32_t* out,
                           uint32_t* tmp, hipStream_t st);
size_t lagrange_tmp_bytes(int sig_g2);
// compressed bytes of n Jacobian points; aff_out / status_out (nullable): their affine form and a decode status
// (DEC_OK, DEC_BAD for infinity) — what decoding the bytes of a subgroup point gives
hipError_t launch_compress(int sig_g2, const uint32_t* pts, size_t n, uint8_t* out, uint32_t* aff_out, uint8_t* status_out,
                           hipStream_t st);
hipError_t launch_recover_pairs(int sig_g2, const uint32_t* shares, const uint32_t* B, const uint32_t* A, int n_nodes,
                                uint32_t* P, uint32_t* Q, hipStream_t st);
// batch Verify under many keys: the decoded key table (affine, launch_prep's status) as per-key Jacobian points in
// launch_pubpoly_eval's layout (a bad key: the identity), and status[i] = DEC_BAD for the items under a bad key
hipError_t launch_key_shares(int key_g2, const uint32_t* key_aff, const uint8_t* kstatus, size_t n_keys, uint32_t* out,
                             hipStream_t st);
hipError_t launch_mark_bad_key(const uint32_t* key_idx, size_t n, const uint8_t* kstatus, uint8_t* status, hipStream_t st);

// batch Schnorr verification (k_schnorr.hip, DKGAuthScheme). status: n bytes from launch_dec_sig of R (without a
// subgroup test) and launch_mark_bad_key. launch_schnorr_scalars rejects s >= r in status and writes, for the items
// still DEC_OK, schnorr_scalar_words() words each: s, h = SHA-512(R || P || msg) mod r and the window digits of s and
// -h. launch_schnorr_table: schnorr_table_words(key_g2) words per decoded key of the affine table (gen = 1: one table,
// of the group's generator; key_aff and kstatus unused). launch_schnorr_check: verdict[i] = ([s]G - [h]P == R) from
// the joint chain over the tables; launch_schnorr_plain: the same from two jac_mul_words on the affine keys.
size_t schnorr_scalar_words();
size_t schnorr_table_words(int key_g2);
hipError_t launch_schnorr_scalars(const uint8_t* sigs, size_t stride, int key_len, const uint8_t* keys, const uint32_t* key_idx,
                                  const uint8_t* msgs, const uint32_t* msg_off, size_t n, uint8_t* status, uint32_t* sc,
                                  hipStream_t st);
hipError_t launch_schnorr_table(int key_g2, const uint32_t* key_aff, const uint8_t* kstatus, size_t n_keys, int gen, uint32_t* tbl,
                                hipStream_t st);
hipError_t launch_schnorr_check(int key_g2, const uint32_t* sc, const uint8_t* status, const uint32_t* r_aff,
                                const uint32_t* key_idx, const uint32_t* gtab, const uint32_t* ktabs, size_t n, uint8_t* verdict,
                                hipStream_t st);
hipError_t launch_schnorr_plain(int key_g2, const uint32_t* sc, const uint8_t* status, const uint32_t* r_aff,
                                const uint32_t* key_idx, const uint32_t* key_aff, size_t n, uint8_t* verdict, hipStream_t st);

// trimmed bbolt store -> verifier columns (k_bolt.hip). leaves: bolt::leaf_ref records {offset, extent},
// info: bolt::leaf_info records (40 B), both for the leaves the launch covers (one wave each). count writes the
// in-range round elements per leaf (then launch_scan: base, n + 1 words); gather writes rounds / lens / value rows of
// `stride` bytes (a multiple of 4) at base[leaf] + rank; link writes miss_prev (n bytes) and the gaps of [first, last]
// (n + 1 words; then launch_scan: moff, n + 2 words); fill writes the `total` missing rounds, ascending; fold writes
// bad[row] (prev_layout: row 0 carries round a - 1, row r was verified as item r - 1).
hipError_t launch_bolt_scan(const uint8_t* file, const void* leaves, size_t n, void* info, uint32_t* err_word, hipStream_t st);
hipError_t launch_bolt_count(const uint8_t* file, const void* leaves, const void* info, size_t n, uint64_t first, uint64_t last,
                             uint32_t* cnt, hipStream_t st);
hipError_t launch_bolt_gather(const uint8_t* file, const void* leaves, const uint32_t* base, size_t n, uint64_t first, uint64_t last,
                              uint32_t stride, uint64_t* rounds, uint8_t* rows, uint32_t* lens, uint64_t cap_rows, hipStream_t st);
hipError_t launch_bolt_link(const uint64_t* rounds, size_t n, uint64_t first, uint64_t last, uint8_t* miss_prev, uint32_t* gap,
                            hipStream_t st);
hipError_t launch_bolt_fill(const uint64_t* rounds, size_t n, uint64_t first, const uint32_t* moff, size_t total, uint64_t* missing,
                            hipStream_t st);
hipError_t launch_bolt_fold(const uint64_t* rounds, const uint32_t* lens, const uint8_t* miss_prev, const uint8_t* verdict, size_t n,
                            uint32_t sig_len, int prev_layout, uint64_t a, uint8_t* bad, hipStream_t st);

// The legacy hexjson store. scan_json: one leaf_json (16 bytes) per leaf. gather_json: for the window's
// rows at base[leaf] + rank, rounds, deferred (1 = the value is not canonical hexjson: zero row, zero lengths) and the
// hex-decoded Signature / PreviousSig rows (strides multiples of 4; sigs + sig_lens and prevs + prev_lens nullable).
// fold_json: bad[row] = not deferred and (decoded length != sig_len or verdict 0).
struct json_cols {
  uint64_t* rounds;
  uint8_t* deferred;
  uint8_t* sigs;
  uint32_t* sig_lens;
  uint8_t* prevs;
  uint32_t* prev_lens;
  uint32_t sig_stride, prev_stride;
  uint64_t cap_rows;
};
hipError_t launch_bolt_scan_json(const uint8_t* file, const void* leaves, size_t n, void* jinfo, hipStream_t st);
hipError_t launch_bolt_gather_json(const uint8_t* file, const void* leaves, const uint32_t* base, size_t n, uint64_t first,
                                   uint64_t last, const json_cols& c, hipStream_t st);
hipError_t launch_bolt_fold_json(const uint32_t* sig_lens, const uint8_t* deferred, const uint8_t* verdict, size_t n, uint32_t sig_len,
                                 uint8_t* bad, hipStream_t st);

// client.RandomData JSON-lines archives (k_archive.hip). `file`: the image, 16-byte aligned. count: the
// record starts per tile of ARCHIVE_TILE bytes (then launch_scan: base, ntiles + 1 words); index: line_off / line_len
// per record in file order (a line above 4096 bytes: length 4097). stat: chunks = one archive_stat per 64 records
// (scratch), out5 = {deferred, longest line, longest decoded signature / previous_signature / randomness}. gather:
// records [0, n) of the line_off / line_len handed in, one row each; sigs / sig_lens, prevs / prev_lens and rands /
// rand_lens are nullable in pairs, strides multiples of 4, rands rows are 32 bytes. fold: dh_archive_check's status byte per row.
constexpr uint32_t ARCHIVE_TILE = 4096;
struct archive_stat {
  uint32_t n_deferred, max_line, max_sig, max_prev, max_rand, pad;
};
struct archive_cols {
  uint64_t* rounds;
  uint8_t* deferred;
  uint8_t* sigs;
  uint32_t* sig_lens;
  uint8_t* prevs;
  uint32_t* prev_lens;
  uint8_t* rands;
  uint32_t* rand_lens;
  uint32_t sig_stride, prev_stride;
};
enum : uint32_t { AR_DEFERRED = 1, AR_NO_SIGNATURE = 2, AR_INVALID = 4, AR_RANDOMNESS = 8, AR_SEQUENCE = 16, AR_LINK = 32, AR_PRED_DEFERRED = 64, AR_BEACON_ID = 128 };
struct archive_fold_in {
  size_t n;
  uint32_t want_sig_len, chained, sig_stride, prev_stride;
  const uint8_t* verdict;
  const uint8_t* rand_out;  // 32 bytes per row: SHA-256 of the row's first want_sig_len bytes
  const uint64_t* rounds;
  const uint8_t* deferred;
  const uint8_t* sigs;
  const uint32_t* sig_lens;
  const uint8_t* prevs;  // chained only
  const uint32_t* prev_lens;
  const uint8_t* rands;
  const uint32_t* rand_lens;
  // the record before row 0: carry = {there is one, it is deferred}, its round, signature length and signature row
  const uint8_t* carry;
  const uint64_t* carry_round;
  const uint32_t* carry_len;
  const uint8_t* carry_sig;
  // protobuf handles with an expected beacon ID (else NULL): pb_meta_out's byte per row; AR_BEACON_ID = bit 0 without bit 1
  const uint8_t* meta;
};
hipError_t launch_ndjson_count(const uint8_t* file, uint64_t len, size_t ntiles, uint32_t* cnt, hipStream_t st);
hipError_t launch_ndjson_index(const uint8_t* file, uint64_t len, size_t ntiles, const uint32_t* base, uint64_t* line_off, uint32_t* line_len,
                               hipStream_t st);
hipError_t launch_ndjson_stat(const uint8_t* file, uint64_t len, const uint64_t* line_off, const uint32_t* line_len, size_t n, void* chunks,
                              uint64_t* out5, hipStream_t st);
hipError_t launch_ndjson_gather(const uint8_t* file, uint64_t len, const uint64_t* line_off, const uint32_t* line_len, size_t n,
                                const archive_cols& c, hipStream_t st);
hipError_t launch_archive_fold(const archive_fold_in& f, uint8_t* status, hipStream_t st);
hipError_t launch_ndjson_stat_fold(const void* chunks, size_t n_chunks, uint64_t* out5, hipStream_t st);

// protobuf beacon records (k_packet.hip, pbwire.hpp). kind: 1 BeaconPacket, 2 PublicRandResponse. The
// caller gives rec_off / rec_len (ascending, inside the image); stat and gather are launch_ndjson_stat / _gather for
// these records, with the same columns and rules. pb_meta_out (meta nullable): per record bit 0 = metadata present,
// bit 1 = its beaconID equals want[0, want_len). The encoder: size gives each row's BeaconPacket length (rec_len,
// nullable; 0 for a row that cannot be encoded), its frame length (with the varint prefix when delimited) and one
// pb_size_sum per 256 rows; then launch_scan over frame_len (off, n + 1 words) and encode. sigs / prevs rows are
// 4-byte aligned with strides that are multiples of 4; prevs / prev_lens NULL together; meta = the metadata field's
// bytes (tag 0x22 included), meta_len 0 for none.
struct pb_meta_out {
  uint8_t* meta;
  const uint8_t* want;
  uint32_t want_len;
};
struct pb_encode_in {
  const uint64_t* rounds;
  const uint8_t* sigs;
  const uint32_t* sig_lens;
  const uint8_t* prevs;
  const uint32_t* prev_lens;
  const uint8_t* meta;
  uint32_t sig_stride, prev_stride, meta_len, delimited;
};
struct pb_size_sum {
  uint64_t bytes, first_bad;  // first_bad: the first row that cannot be encoded, ~0 for none
};
hipError_t launch_pb_stat(int kind, const uint8_t* file, uint64_t len, const uint64_t* rec_off, const uint32_t* rec_len, size_t n, void* chunks,
                          uint64_t* out5, hipStream_t st);
hipError_t launch_pb_gather(int kind, const uint8_t* file, uint64_t len, const uint64_t* rec_off, const uint32_t* rec_len, size_t n,
                            const archive_cols& c, const pb_meta_out& x, hipStream_t st);
hipError_t launch_pb_size(const pb_encode_in& e, size_t n, uint32_t* rec_len, uint32_t* frame_len, pb_size_sum* sums, hipStream_t st);
hipError_t launch_pb_encode(const pb_encode_in& e, size_t n, const uint32_t* off, uint8_t* out, hipStream_t st);

// the records a node or relay serves (k_serve.hip): verifier columns -> client.RandomData hexjson
// objects (form 1) or PublicRandResponse messages (form 2), each with randomness = SHA-256(signature). The passes are
// those of the BeaconPacket encoder above, pb_size_sum included. rands (nullable): 32 bytes per row, copied as given;
// NULL: the digest of the row's sig_len signature bytes, computed in the encode pass and never stored as a column.
// keep (nullable): a row whose byte is 0 writes nothing, has lengths 0 and is not measured. meta: the metadata field's
// bytes (tag 0x2A included), meta_len 0 for none; form 2 only. framed: '\n' after a JSON record, a varint length
// before a protobuf one.
enum : uint32_t { SERVE_RANDOM_DATA_JSON = 1, SERVE_PUBLIC_RAND_PB = 2 };
struct serve_encode_in {
  const uint64_t* rounds;
  const uint8_t* sigs;
  const uint32_t* sig_lens;
  const uint8_t* prevs;
  const uint32_t* prev_lens;
  const uint8_t* rands;
  const uint8_t* keep;
  const uint8_t* meta;
  uint32_t sig_stride, prev_stride, meta_len, form, framed;
};
hipError_t launch_serve_size(const serve_encode_in& e, size_t n, uint32_t* rec_len, uint32_t* frame_len, pb_size_sum* sums, hipStream_t st);
hipError_t launch_serve_encode(const serve_encode_in& e, size_t n, const uint32_t* off, uint8_t* out, hipStream_t st);

// verifier columns -> the leaf pages of a trimmed bbolt store (k_bolt_write.hip). need: the record
// sizes 24 + lens[i] (then launch_scan), err_word set when rounds do not ascend or a length passes the stride. pack:
// leaves = boltw::leaf_desc records (24 B, one wave each); `image` starts at page 4 and holds every leaf extent;
// first_key[leaf] = its first round. merge: slots [0, n) the stored rows, [n, n + np) the ascending patches (p_lens
// 0xFFFFFFFF = delete); flag / lb per slot (n + np words each), hit per patch, err_word set by a deferred row no patch
// covers; then launch_scan over flag (pos, n + np + 1 words) and scatter into merge_out (stride a multiple of 4
// holding every value; src = the stored row a merged row came from, 0xFFFFFFFF for a patch). unlinked: flag per
// merged row (then launch_scan and compact: the flagged rounds, ascending); pred (nullable) = the row before the first
// merged row, in the layout of carry_out.last.
struct merge_in {
  const uint64_t* rounds;
  const uint8_t* rows;
  const uint32_t* lens;
  const uint8_t* defer;  // nullable
  size_t n;
  uint32_t stride;
  const uint64_t* p_rounds;
  const uint8_t* p_rows;
  const uint32_t* p_lens;
  size_t np;
  uint32_t p_stride;
};
struct merge_out {
  uint64_t* rounds;
  uint8_t* rows;
  uint32_t* lens;
  uint32_t* src;
  uint32_t stride;
};
// The windowed writer: need sizes and checks a window's n new rows (boltw::cols), the first of them
// against last[0] (nullable here; the kernel always gets a readable address). pack and carry take the rows as
// boltw::cols2 (bolt_write.hpp): the carried rows, then the caller's columns; n_carry = 0 is the one-shot call. pack: `image` starts at page page_base. carry: rows [first, first + count) into the
// other carry set (stride a multiple of 4 holding their values) and row last_row into `last` = {round, length, then
// the value from byte 16 at last_stride}; it reads nothing that it or the pack writes.
namespace boltw {
struct cols;
struct cols2;
}
struct carry_out {
  uint64_t* rounds;
  uint32_t* lens;
  uint8_t* rows;
  uint32_t stride;
  uint64_t* last;
  uint32_t last_stride;
};
hipError_t launch_bolt_need(const boltw::cols& c, size_t n, const uint64_t* last, uint32_t* need, uint32_t* err_word, hipStream_t st);
hipError_t launch_bolt_pack(const void* leaves, size_t n_leaves, const boltw::cols2& c, uint32_t page_size, uint64_t page_base,
                            uint8_t* image, uint64_t* first_key, hipStream_t st);
hipError_t launch_bolt_carry(const boltw::cols2& c, uint64_t first, uint64_t count, uint64_t last_row, const carry_out& o, hipStream_t st);
hipError_t launch_bolt_merge(const merge_in& m, uint32_t* flag, uint32_t* lb, uint8_t* hit, uint32_t* err_word, hipStream_t st);
hipError_t launch_bolt_scatter(const merge_in& m, const uint32_t* flag, const uint32_t* lb, const uint32_t* pos, const merge_out& o,
                               hipStream_t st);
hipError_t launch_bolt_unlinked(const merge_out& o, size_t n_out, const uint8_t* prevs, uint32_t prev_stride, const uint32_t* prev_lens,
                                const uint64_t* pred, uint32_t* flag, hipStream_t st);
hipError_t launch_bolt_compact(const uint64_t* rounds, const uint32_t* off, size_t n, uint64_t* out, hipStream_t st);

// Unordered candidate columns -> one chain (k_assemble.hip, assemble.hpp). pre: the status byte of a
// skipped / stale candidate and the live flag (then launch_scan: pos, n + 1 words); cut: the live candidates' keys and
// input positions in input order. The sort is a stable LSD radix sort of (u64 key, u32 payload) by 8-bit digits:
// sort_orand ORs / ANDs every key into orand[0] / orand[1] (set to {0, ~0} by the caller), which names the passes
// whose digit is constant; sort_pass is one pass at bit `shift` from (keys, idx) into (keys_out, idx_out), with cnt and
// off of 256 x tiles (+ 1) words, digit-major. launch_scan takes 4096^2 counts, so 65536 tiles of SORT_TILE keys, 2^27
// keys, eight times the 16M rows a column call takes. heads / runs: the rounds' runs of the sorted entries (head -> scan
// -> run_start per run). class: rep[j] = the sorted entry that entry j repeats, is_rep[j] (then launch_scan: rpos);
// reps: rep_cand[place in the verifier's columns] = candidate; gather: rows [0, k) of one window of those columns.
// pick: chosen[run]; select: the live candidates' status bytes and the chosen flags (then launch_scan: opos); emit:
// the output columns at sig_stride / prev_stride of the input; link: the rows' flags and gap[n_out + 1] (then
// launch_scan: goff); gaps: the ranges of missing rounds.
namespace assemble {
struct cols;
struct bounds;
}
constexpr uint32_t SORT_TILE = 2048;
struct assemble_verify_cols {
  uint64_t* rounds;
  uint8_t* sigs;
  uint8_t* prevs;
  uint32_t* prev_lens;
  uint32_t sig_stride, prev_stride;
};
struct assemble_out {
  uint64_t* rounds;
  uint8_t* sigs;
  uint32_t* sig_lens;
  uint8_t* prevs;  // nullable with prev_lens
  uint32_t* prev_lens;
  uint32_t* src;
  uint8_t* flags;
};
hipError_t launch_assemble_pre(const assemble::cols& c, size_t n, const assemble::bounds& b, uint8_t* status, uint32_t* live, hipStream_t st);
hipError_t launch_assemble_cut(const uint64_t* rounds, size_t n, const uint32_t* pos, uint64_t* keys, uint32_t* idx, hipStream_t st);
hipError_t launch_sort_orand(const uint64_t* keys, size_t n, uint64_t* orand, hipStream_t st);
hipError_t launch_sort_pass(const uint64_t* keys, const uint32_t* idx, size_t n, uint32_t shift, uint32_t* cnt, uint32_t* off,
                            uint32_t* scan_tmp, uint64_t* keys_out, uint32_t* idx_out, hipStream_t st);
hipError_t launch_assemble_heads(const uint64_t* keys, size_t m, uint32_t* head, hipStream_t st);
hipError_t launch_assemble_runs(const uint32_t* runs, size_t m, uint32_t* run_start, hipStream_t st);
hipError_t launch_assemble_class(const assemble::cols& c, const uint32_t* idx, const uint32_t* runs, const uint32_t* run_start, size_t m,
                                 bool dedupe, uint32_t* rep, uint32_t* is_rep, hipStream_t st);
hipError_t launch_assemble_reps(const uint32_t* idx, const uint32_t* rpos, size_t m, uint32_t* rep_cand, hipStream_t st);
hipError_t launch_assemble_gather(const assemble::cols& c, const uint32_t* rep_cand, size_t k, uint32_t want_sig_len,
                                  const assemble_verify_cols& v, hipStream_t st);
hipError_t launch_assemble_pick(const assemble::cols& c, const uint32_t* idx, const uint32_t* run_start, size_t n_runs, size_t m,
                                const uint32_t* rpos, const uint8_t* verdict, uint32_t want_sig_len, uint32_t* chosen, hipStream_t st);
hipError_t launch_assemble_select(const assemble::cols& c, const uint32_t* idx, const uint32_t* runs, const uint32_t* run_start,
                                  const uint32_t* rep, const uint32_t* rpos,
                                  const uint8_t* verdict, const uint32_t* chosen, size_t m, uint32_t want_sig_len, uint8_t* status,
                                  uint32_t* out_flag, hipStream_t st);
hipError_t launch_assemble_emit(const assemble::cols& c, const uint32_t* idx, const uint32_t* opos, size_t m, const assemble_out& o,
                                hipStream_t st);
hipError_t launch_assemble_link(const assemble::cols& c, const assemble_out& o, size_t n_out, const assemble::bounds& b, const uint64_t* anchor,
                                bool chained, uint32_t* gap, hipStream_t st);
hipError_t launch_assemble_gaps(const assemble_out& o, size_t n_out, const assemble::bounds& b, const uint32_t* goff, uint64_t* gap_first,
                                uint64_t* gap_last, hipStream_t st);

#ifdef DH_COUNT_PRODUCTS
// counting build: field products executed since the last take, per translation unit (fp_mul28.hpp)
hipError_t count_take_prep(unsigned long long* v);
hipError_t count_take_msm(unsigned long long* v);
hipError_t count_take_check(unsigned long long* v);
hipError_t count_take_sign(unsigned long long* v);
hipError_t count_take_recover(unsigned long long* v);
hipError_t count_take_vm(unsigned long long* v);
hipError_t count_take_schnorr(unsigned long long* v);
#endif

}  // namespace dh
