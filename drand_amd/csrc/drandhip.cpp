// libdrandhip host side: the C ABI of include/drandhip.h over the gfx950 kernels in kernels.hip.
//
// Threading model (SURVEY.md §8b "Threading"): one global device context (dh_init, idempotent), and a
// pool of workers, each = {hipStream_t, growable device workspace}. A call takes a free worker for its
// duration, so concurrent goroutines / threads never share a stream or a buffer; results are copied
// into caller memory before the call returns. No global mutable state is visible to callers.
//
// Verification flow of one batch (dh_verify_batch_device):
//   decode pk -> prep signatures (status, affine sigma, randomness) -> prep messages (Q_i, pre-cofactor)
//   -> RLC scalars -> level 0: one group = every round: MSM + pairing check
//   -> on failure, bisection levels with smaller groups (sizes from an expected-cost model: 1024, then 256/64/16/4
//      as the observed fault density says, or straight to leaves) over the failing groups only
//   -> leaves: per-round 2-pairing checks. Verdict = decode ok AND (group passed OR leaf passed),
//   which is the per-round VerifyBeacon verdict of /root/reference/crypto/schemes.go:70-72.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <sys/random.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cmath>
#include <functional>
#include <map>
#include <memory>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/drandhip.h"
#include "assemble.hpp"
#include "bolt.hpp"
#include "bolt_write.hpp"
#include "kernels.hpp"
#include "pbwire.hpp"
#include "rdjson.hpp"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(x)                                                                     \
  do {                                                                                 \
    hipError_t e__ = (x);                                                              \
    if (e__ != hipSuccess)                                                             \
      return fail(e__ == hipErrorOutOfMemory ? DH_ENOMEM : DH_EDEVICE, "%s: %s (%s:%d)", #x, \
                  hipGetErrorString(e__), __FILE__, __LINE__);                         \
  } while (0)

bool sig_on_g2(int scheme) { return scheme == DH_SCHEME_CHAINED || scheme == DH_SCHEME_UNCHAINED; }
int dst_id(int scheme) { return scheme == DH_SCHEME_G1_RFC9380 ? 1 : 0; }

// growable device buffer
struct dbuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = std::max(bytes, (size_t)4096);
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  template <class T>
  T* as() const {
    return (T*)p;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct dbuf_pool {  // a call's own buffers and stream: nothing is shared between calls
  std::vector<dbuf*> bufs;
  hipStream_t st = nullptr;  // stays null in a call that runs on its caller's stream
  ~dbuf_pool() {
    for (dbuf* b : bufs) b->release();
    if (st) (void)hipStreamDestroy(st);
  }
};

// Environment knobs. Each helper reads the variable when it is called: an accessor that keeps the result in a
// `static const` reads its knob once per process, one that returns the call's value reads it at every call (the knobs
// that tests set between calls).
// A switch: a value starting with '0' turns a default-on knob off, one starting with '1' turns a default-off knob on.
bool env_on(const char* name, bool def) {
  const char* e = getenv(name);
  return e && e[0] == (def ? '0' : '1') ? !def : def;
}
// A number as atol reads it; `unset` when the variable is not set.
long env_long(const char* name, long unset) {
  const char* e = getenv(name);
  return e ? atol(e) : unset;
}
// A size as atoll reads it when that is at least `min` (>= 0); otherwise, and when the variable is not set, `def`.
size_t env_size(const char* name, size_t def, long long min) {
  const char* e = getenv(name);
  const long long v = e ? atoll(e) : -1;
  return v >= min ? (size_t)v : def;
}

struct worker {
  hipStream_t stream = nullptr;
  // high-priority stream for a batch's latency-bound tail (MSM, pairing checks, bisection): its small kernels
  // get wave slots ahead of other batches' saturating per-round kernels (verify_core)
  hipStream_t tail = nullptr;
  hipEvent_t handoff = nullptr;
  // node-wide batch (dh_batch_begin / dh_batch_check): the partial sums are complete (ordered onto the caller's
  // stream), and the gathered records are complete on the caller's stream (the tail waits for it)
  hipEvent_t part_ready = nullptr, gath_ready = nullptr;
  // small-batch path (verify_small): the hash kernels fork onto the tail stream beside the signature kernels and
  // join back (join); host inputs and outputs cross PCIe through one pinned staging buffer each way
  hipEvent_t join = nullptr, ev_dec = nullptr, ev_sub = nullptr;
  void* h_stage = nullptr;
  size_t h_stage_cap = 0;
  dbuf d_stage, sub_bad;
  bool busy = false;
  // leased by a node batch (dh_batch_begin until dh_batch_finish): held across calls, released only by the caller
  bool node_held = false;
  // per-round state
  dbuf status, sig_aff, q_pts, scal, entries, verdict_tmp, rand_tmp, h2c_tmp;
  // the MSM's 28-bit points (launch_msm_prep28, G1): sigma and its phi image (32 words each), hash points (48 words)
  dbuf s28, q28;
  // bisection on the device: the next level's entries, fail flags, their ranks and the scan's block sums
  dbuf entries_alt, cflags, crank, cscan;
  // host-API staging
  dbuf in_rounds, in_sigs, in_prevs, in_prev_lens, out_verdict, out_rand;
  // key
  dbuf key_raw, key_aff, key_ok;
  // node-wide check: the summed (A, B) of the gathered records, and {abandon flag, pairing check, result}
  dbuf node_sum, node_res;
  // MSM
  dbuf cnt, off, scan_tmp, list, buckets, segs, outA, outB, out2, pass, part, meta;
  // batched G1 subgroup test (verify_core): the bit-subset sums' scratch, and the result byte the host reads
  dbuf sub_tmp, sub_pass;
  // lane-parallel pairing checks
  dbuf vm_pairs, vm_live, vm_done;
  // tbls Recover
  dbuf r_commits, r_cstatus, r_caff, r_shares, r_raw, r_psigs, r_pidx, r_pstatus, r_paff, r_msgs, r_q, r_scal,
      r_round_of, r_e_pidx, r_e_sidx, r_e_grp, r_P, r_Q, r_f, r_skip, r_ok, r_sel, r_lam, r_lamset, r_rok, r_sig,
      r_sigbytes, r_status2, r_aff2, r_entries2, r_off, r_key, r_den, r_zs, r_tbl, r_rstat, r_ltmp, r_own, r_need;
  // batch Verify under many keys (auth_core): the key table (raw, decode status, affine, per-key Jacobian), the items'
  // key indices and message offsets, the per-key signature sums (Jacobian, compressed, affine, status), the per-key
  // check results and the leaf list
  dbuf a_keys, a_kstatus, a_kaff, a_shares, a_kidx, a_moff, a_Ak, a_Akbytes, a_Akaff, a_Akstat, a_kpass, a_list;
  // batch Schnorr verification (schnorr_core): the items' scalars and window digits, the per-key tables
  dbuf s_sc, s_ktab;
  std::vector<uint8_t> h_verdict;
  // Recover: the (scheme, t, n_nodes, commits) whose decoded commits and public shares r_caff / r_shares hold
  std::vector<uint8_t> r_pub_key;
  // decoded group keys, KEY_SLOTS per worker (least recently used replaced): a chain's batches all use one key, and a
  // node or relay serving several chains alternates between a few; key_cur = the slot ensure_key selected (96 words:
  // the affine point, then [h_eff] pk for G1-signature schemes)
  static constexpr int KEY_SLOTS = 4;
  struct key_slot {
    uint8_t bytes[96];
    size_t len = 0;  // 0: empty
    int g2 = -1;
    uint8_t ok = 0;
    uint64_t used = 0;
  } keys[KEY_SLOTS];
  uint64_t key_clock = 0;
  dbuf key_tab;
  uint32_t* key_cur = nullptr;
  // fault density (faults per round) the last bisection of this worker observed at its first level: a replay's
  // consecutive windows fail alike, so a dense one starts its next bisection with smaller groups (next_group_size)
  double fault_density = 0;
  // eligible batches this worker still sends through the fused subgroup test after a dense fallback (sub_backoff)
  int sub_fused_left = 0;
  // set by dh_batch_begin while it queues a node batch on one stream (node_one_stream): no tail-stream handoff
  bool begin_one_stream = false;
  void release_all() {
    key_tab.release();
    dbuf* all[] = {&s28, &q28, &entries_alt, &cflags, &crank, &cscan, &status, &sig_aff, &q_pts, &scal, &entries, &verdict_tmp, &rand_tmp, &h2c_tmp, &in_rounds, &in_sigs,
                   &in_prevs, &in_prev_lens, &out_verdict, &out_rand, &key_raw, &key_aff, &key_ok, &cnt, &off,
                   &scan_tmp, &list, &buckets, &segs, &outA, &outB, &out2, &pass, &part, &meta, &vm_pairs, &vm_live, &vm_done, &r_commits, &r_cstatus, &r_caff, &r_shares,
                   &r_raw, &r_psigs, &r_pidx, &r_pstatus, &r_paff, &r_msgs, &r_q, &r_scal, &r_round_of, &r_e_pidx,
                   &r_e_sidx, &r_e_grp, &r_P, &r_Q, &r_f, &r_skip, &r_ok, &r_sel, &r_lam, &r_lamset, &r_rok, &r_sig,
                   &r_sigbytes, &r_status2, &r_aff2, &r_entries2, &r_off, &r_key, &r_den, &r_zs, &r_tbl, &r_rstat, &r_ltmp, &r_own, &r_need, &node_sum, &node_res,
                   &a_keys, &a_kstatus, &a_kaff, &a_shares, &a_kidx, &a_moff, &a_Ak, &a_Akbytes, &a_Akaff, &a_Akstat, &a_kpass,
                   &a_list, &s_sc, &s_ktab, &sub_tmp, &sub_pass};
    for (dbuf* b : all) b->release();
    d_stage.release();
    sub_bad.release();
    if (h_stage) (void)hipHostFree(h_stage);
    h_stage = nullptr;
    h_stage_cap = 0;
    for (hipEvent_t* e : {&join, &ev_dec, &ev_sub}) {
      if (*e) (void)hipEventDestroy(*e);
      *e = nullptr;
    }
    if (stream) (void)hipStreamDestroy(stream);
    if (tail) (void)hipStreamDestroy(tail);
    if (handoff) (void)hipEventDestroy(handoff);
    if (part_ready) (void)hipEventDestroy(part_ready);
    if (gath_ready) (void)hipEventDestroy(gath_ready);
    stream = tail = nullptr;
    handoff = part_ready = gath_ready = nullptr;
  }
};

struct context {
  std::mutex mu;
  std::condition_variable freed;  // a worker became idle
  bool inited = false;
  int device = 0;
  // at most this many workers (2 HIP streams each): a burst of callers waits for an idle worker instead of creating
  // streams until the runtime runs out of hardware-queue resources (r03: 16 node batches in flight, each holding two
  // workers, aborted HSA queues with HSA_STATUS_ERROR_OUT_OF_RESOURCES); DRANDHIP_MAX_WORKERS overrides
  size_t max_workers = [] {
    const long v = env_long("DRANDHIP_MAX_WORKERS", 0);
    return (size_t)(v >= 1 && v <= 256 ? v : 24);
  }();
  std::vector<worker*> pool;     // idle or leased workers
  std::vector<worker*> retired;  // leased when dh_shutdown ran: freed by their lease's end
  // batch Schnorr verification: the table of odd multiples of each key group's generator ([0] G1, [1] G2), built by
  // the first call that needs it and then read by every worker's check kernel. dh_shutdown drops them; while a call
  // is still running they wait in gen_old for the next dh_shutdown that finds every worker idle.
  std::mutex gen_mu;
  dbuf gen_tab[2];
  bool gen_ready[2] = {false, false};
  std::vector<void*> gen_old;
};
context g_ctx;

// One device per process (the multi-GPU layout is one process per GPU): the mask must name at
// most one device; 0 means "device 0, or the device already selected".
int ensure_init_locked(uint32_t mask) {
  if (mask & (mask - 1)) return fail(DH_EINVAL, "device mask 0x%x names more than one device (one process per GPU)", mask);
  const int want = mask ? __builtin_ctz(mask) : -1;
  if (g_ctx.inited) {
    if (want >= 0 && want != g_ctx.device)
      return fail(DH_EINVAL, "already initialised on device %d (dh_shutdown first)", g_ctx.device);
    return DH_OK;
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) return fail(DH_EDEVICE, "no HIP device available (%s)", hipGetErrorString(e));
  const int dev = want >= 0 ? want : 0;
  if (dev >= ndev) return fail(DH_EINVAL, "device %d not present (%d devices)", dev, ndev);
  g_ctx.device = dev;
  g_ctx.inited = true;
  return DH_OK;
}

// How long a blocking call waits for a worker while EVERY worker is held by an unfinished node batch (those are
// released only by their callers' dh_batch_finish, possibly on the waiting thread itself): then DH_EBUSY, not a
// deadlock. DRANDHIP_LEASE_TIMEOUT_MS overrides (default 30 s).
static std::chrono::milliseconds node_held_timeout() {
  static const long v = [] {
    const long x = env_long("DRANDHIP_LEASE_TIMEOUT_MS", 0);
    return x > 0 ? x : 30000L;
  }();
  return std::chrono::milliseconds(v);
}

// A worker for the duration of a call. The pool holds at most g_ctx.max_workers: a blocking call waits for an idle
// one; wait = false (dh_batch_begin, whose lease spans a collective with the other ranks, so waiting could deadlock
// the node) fails with DH_EBUSY instead, and its worker is marked node_held until dh_batch_finish. A blocking call
// that finds every worker node_held waits at most node_held_timeout() and then fails with DH_EBUSY.
struct lease {
  worker* w = nullptr;
  int rc = DH_OK;
  explicit lease(bool wait = true) {
    std::unique_lock<std::mutex> lk(g_ctx.mu);
    rc = ensure_init_locked(0);
    if (rc != DH_OK) return;
    for (;;) {
      for (worker* x : g_ctx.pool)
        if (!x->busy) {
          w = x;
          break;
        }
      if (w) break;
      if (g_ctx.pool.size() < g_ctx.max_workers) {
        w = new worker();
        g_ctx.pool.push_back(w);
        break;
      }
      if (!wait) {
        rc = fail(DH_EBUSY, "all %zu library workers are busy (DRANDHIP_MAX_WORKERS)", g_ctx.max_workers);
        return;
      }
      const bool all_node_held =
          std::all_of(g_ctx.pool.begin(), g_ctx.pool.end(), [](const worker* x) { return x->node_held; });
      if (!all_node_held) {
        g_ctx.freed.wait(lk);
      } else if (g_ctx.freed.wait_for(lk, node_held_timeout()) == std::cv_status::timeout) {
        rc = fail(DH_EBUSY, "all %zu library workers are held by unfinished node batches (dh_batch_finish them first)",
                  g_ctx.max_workers);
        return;
      }
    }
    w->busy = true;
    w->node_held = !wait;
  }
  ~lease() {
    if (!w) return;
    std::lock_guard<std::mutex> lk(g_ctx.mu);
    w->busy = false;
    w->node_held = false;
    g_ctx.freed.notify_all();
    auto it = std::find(g_ctx.retired.begin(), g_ctx.retired.end(), w);
    if (it != g_ctx.retired.end()) {  // dh_shutdown ran during this call
      g_ctx.retired.erase(it);
      if (w->stream) (void)hipStreamSynchronize(w->stream);
      w->release_all();
      delete w;
    }
  }
};

// The tail stream is created on a worker's first local call: a worker that only ever runs node batches (one stream
// per batch) holds one stream. HIP hands a process's streams its hardware queues in creation order, round robin; with
// two streams per worker, the node batches' streams landed on every other queue (8 of 16), so more than 8 batches in
// flight doubled some queues up and not others, and the one host thread retiring batches in order waited on the
// doubled ones: 131k-round node batches 21.5 M/s at 8-11 in flight, 16.3 at 12, 19.5 at 16 (19.8 at 12 over 8
// queues, 16.7 at 8 over 4: profiles/r05/node_131072_sweep_r05k).
int set_device_and_stream(worker* w, bool need_tail = true) {
  HIP_TRY(hipSetDevice(g_ctx.device));
  if (!w->stream) HIP_TRY(hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking));
  if (!w->tail && need_tail) {
    int least = 0, greatest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIP_TRY(hipStreamCreateWithPriority(&w->tail, hipStreamNonBlocking, greatest));
  }
  if (!w->handoff) HIP_TRY(hipEventCreateWithFlags(&w->handoff, hipEventDisableTiming));
  if (!w->part_ready) HIP_TRY(hipEventCreateWithFlags(&w->part_ready, hipEventDisableTiming));
  if (!w->gath_ready) HIP_TRY(hipEventCreateWithFlags(&w->gath_ready, hipEventDisableTiming));
  for (hipEvent_t* e : {&w->join, &w->ev_dec, &w->ev_sub})
    if (!*e) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
  return DH_OK;
}

// The group key decoded on the device (a key_tab slot: the affine point, then [h_eff] pk for G1-signature schemes),
// cached per worker in KEY_SLOTS slots: a chain's batches all use one key, and decoding a G2 key is a one-lane kernel
// of a few ms. On a miss the stream is synchronised once to read the key's status; DH_EKEY when it is not a
// compressed subgroup point. Sets w->key_cur.
int ensure_key(worker* w, bool g2, const uint8_t* pk, size_t pk_len, hipStream_t st) {
  HIP_TRY(w->key_raw.ensure(96));
  HIP_TRY(w->key_ok.ensure(64));  // [0] key status, [32..63] RLC seed
  HIP_TRY(w->key_tab.ensure(worker::KEY_SLOTS * 96 * 4));  // fixed size keeps the slots valid
  const int kg = g2 ? 0 : 1;
  int slot = -1, victim = 0;
  for (int i = 0; i < worker::KEY_SLOTS; i++) {
    const worker::key_slot& k = w->keys[i];
    if (k.len == pk_len && k.g2 == kg && !memcmp(k.bytes, pk, pk_len)) slot = i;
    if (k.used < w->keys[victim].used) victim = i;
  }
  if (slot < 0) {
    slot = victim;
    worker::key_slot& k = w->keys[slot];
    k.len = 0;
    uint8_t ok = 0;
    uint32_t* dst = w->key_tab.as<uint32_t>() + (size_t)slot * 96;
    HIP_TRY(hipMemcpyAsync(w->key_raw.p, pk, pk_len, hipMemcpyHostToDevice, st));
    HIP_TRY(dh::launch_decode_key(g2 ? 0 : 1, w->key_raw.as<uint8_t>(), dst, w->key_ok.as<uint8_t>(), st));
    HIP_TRY(hipMemcpyAsync(&ok, w->key_ok.p, 1, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(k.bytes, pk, pk_len);
    k.len = pk_len;
    k.g2 = kg;
    k.ok = ok;
  }
  w->keys[slot].used = ++w->key_clock;
  w->key_cur = w->key_tab.as<uint32_t>() + (size_t)slot * 96;
  if (w->keys[slot].ok != 1) return fail(DH_EKEY, "group public key is not a valid compressed subgroup point");
  return DH_OK;
}

// ---- host SHA-256 (DigestBeacon for dh_digest_batch; not used by the device path)
struct sha256_host {
  uint32_t h[8];
  uint8_t buf[64];
  uint64_t len;
  size_t n;
  static uint32_t ror(uint32_t x, int k) { return (x >> k) | (x << (32 - k)); }
  void init() {
    static const uint32_t iv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                                   0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    memcpy(h, iv, sizeof h);
    len = 0;
    n = 0;
  }
  void block(const uint8_t* p) {
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
        0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
        0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
        0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
        0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
        0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
        0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
        0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t w[64];
    for (int i = 0; i < 16; i++) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
    for (int i = 16; i < 64; i++)
      w[i] = w[i - 16] + (ror(w[i - 15], 7) ^ ror(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] +
             (ror(w[i - 2], 17) ^ ror(w[i - 2], 19) ^ (w[i - 2] >> 10));
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; i++) {
      uint32_t t1 = hh + (ror(e, 6) ^ ror(e, 11) ^ ror(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
      uint32_t t2 = (ror(a, 2) ^ ror(a, 13) ^ ror(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
  }
  void update(const uint8_t* d, size_t k) {
    len += k;
    while (k) {
      size_t t = std::min(k, 64 - n);
      memcpy(buf + n, d, t);
      n += t;
      d += t;
      k -= t;
      if (n == 64) {
        block(buf);
        n = 0;
      }
    }
  }
  void final(uint8_t out[32]) {
    uint64_t bits = len * 8;
    uint8_t pad = 0x80, z = 0;
    update(&pad, 1);
    while (n != 56) update(&z, 1);
    uint8_t l[8];
    for (int i = 0; i < 8; i++) l[i] = (uint8_t)(bits >> (56 - 8 * i));
    update(l, 8);
    for (int i = 0; i < 8; i++) {
      out[4 * i] = h[i] >> 24; out[4 * i + 1] = h[i] >> 16; out[4 * i + 2] = h[i] >> 8; out[4 * i + 3] = h[i];
    }
  }
};

// ---- host BLAKE2b-256 (RFC 7693, unkeyed): Identity.Hash of key/keys.go:53-57 for dh_identity_hash_batch
void blake2b_256(const uint8_t* in, size_t len, uint8_t out[32]) {
  static const uint64_t iv[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                                 0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
  static const uint8_t sigma[12][16] = {
      {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
      {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
      {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
      {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
      {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
      {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};
  auto ror = [](uint64_t x, int k) { return (x >> k) | (x << (64 - k)); };
  uint64_t h[8];
  memcpy(h, iv, sizeof h);
  h[0] ^= 0x01010000ULL ^ 32;  // digest length 32, no key, fanout = depth = 1
  size_t done = 0;
  for (bool last = false; !last;) {
    uint8_t blk[128] = {0};
    const size_t take = std::min<size_t>(128, len - done);
    memcpy(blk, in + done, take);
    done += take;
    last = done == len;  // the last block may be full; an empty input is one zero block
    uint64_t m[16], v[16];
    for (int i = 0; i < 16; i++) {
      m[i] = 0;
      for (int b = 7; b >= 0; b--) m[i] = (m[i] << 8) | blk[8 * i + b];
    }
    memcpy(v, h, sizeof h);
    memcpy(v + 8, iv, sizeof iv);
    v[12] ^= (uint64_t)done;
    if (last) v[14] = ~v[14];
    for (int r = 0; r < 12; r++) {
      const uint8_t* s = sigma[r];
      auto G = [&](int a, int b, int c, int d, uint64_t x, uint64_t y) {
        v[a] = v[a] + v[b] + x; v[d] = ror(v[d] ^ v[a], 32);
        v[c] = v[c] + v[d];     v[b] = ror(v[b] ^ v[c], 24);
        v[a] = v[a] + v[b] + y; v[d] = ror(v[d] ^ v[a], 16);
        v[c] = v[c] + v[d];     v[b] = ror(v[b] ^ v[c], 63);
      };
      G(0, 4, 8, 12, m[s[0]], m[s[1]]);
      G(1, 5, 9, 13, m[s[2]], m[s[3]]);
      G(2, 6, 10, 14, m[s[4]], m[s[5]]);
      G(3, 7, 11, 15, m[s[6]], m[s[7]]);
      G(0, 5, 10, 15, m[s[8]], m[s[9]]);
      G(1, 6, 11, 12, m[s[10]], m[s[11]]);
      G(2, 7, 8, 13, m[s[12]], m[s[13]]);
      G(3, 4, 9, 14, m[s[14]], m[s[15]]);
    }
    for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[i + 8];
  }
  for (int i = 0; i < 32; i++) out[i] = (uint8_t)(h[i / 8] >> (8 * (i % 8)));
}

uint64_t splitmix64(uint64_t& x) {
  uint64_t z = (x += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

int make_seed(uint64_t seed, uint32_t words[8]) {
  if (seed == 0) {
    uint8_t b[32];
    size_t got = 0;
    while (got < sizeof b) {
      ssize_t r = getrandom(b + got, sizeof b - got, 0);
      if (r <= 0) return fail(DH_EDEVICE, "getrandom failed");
      got += (size_t)r;
    }
    memcpy(words, b, 32);
  } else {
    uint64_t x = seed;
    for (int i = 0; i < 4; i++) {
      uint64_t v = splitmix64(x);
      words[2 * i] = (uint32_t)(v >> 32);
      words[2 * i + 1] = (uint32_t)v;
    }
  }
  return DH_OK;
}

// MSM geometry for groups of gsize rounds; parts: 1 = 127-bit scalars, 2 = the endomorphism split (2 x gsize points,
// 63-bit scalar halves), 4 = the G2 psi split (4 x gsize points, 31-bit scalar parts)
static bool window_ok(int sbits, int c) {
  // keep the top window's t bits at >= c - 4, since each of its 2^(t-1) buckets collects ~m / 2^(t-1) entries
  // and a bucket that spans many chunks is summed serially by k_msm_bucket_fix (127-bit scalars at c = 14 would
  // leave t = 1: two buckets holding the whole set)
  const int nw = (sbits + 1 + c - 1) / c, t = sbits - c * (nw - 1);
  return t >= c - 4;
}
dh::msm_geom geom_for(size_t gsize, int parts = 1) {
  const size_t npts = (size_t)parts * gsize;
  const int sbits = parts == 4 ? 31 : parts == 2 ? 63 : 127;  // scalar bits (k_scalars)
  int lg = 0;
  while (((size_t)1 << (lg + 1)) <= npts) lg++;
  int c = std::max(3, std::min(16, lg - 2));
  // DRANDHIP_MSM_C (experiments): the window width of batch-sized groups (>= 65,536 rounds)
  static const int c_env = [] {
    const char* e = getenv("DRANDHIP_MSM_C");
    const int v = e ? atoi(e) : 0;
    return v >= 4 && v <= 16 ? v : 0;
  }();
  if (c_env && gsize >= 65536) c = c_env;
  // c = lg(npts) - 2 (a 131k-round shard keeps c = 16: a cost model trading bucket-pass additions against the
  // reduction picked c = 13 there and measured 8.5 ms against 6.7, gpurun_out r03g)
  while (c > 3 && !window_ok(sbits, c)) c--;
  dh::msm_geom g;
  g.gsize = (uint32_t)gsize;
  g.c = c;
  g.nwin = (sbits + 1 + c - 1) / c;
  g.nbuck = (1u << (c - 1)) + 1;  // signed digits: |d| in [1, 2^(c-1)] (k_msm.hip: signed_digit)
  // bucket reduction: segments of ~8 digits, one thread each (k_msm_segsum): 16 additions + the segment's offset
  // multiple per thread, then a log-depth tree
  uint32_t nseg = std::max(1u, std::min(8192u, g.nbuck / 8));  // a power of two (nbuck = 2^(c-1) + 1)
  g.nseg = nseg;
  g.seglen = (g.nbuck - 1 + nseg - 1) / nseg;
  g.halves = (uint32_t)parts;
  g.half_stride = 0;  // set by the caller: the point-array offset of the endomorphism images
  return g;
}

// Bucket-reduction segments for a level of ngroups groups (nsets point sets): as many segments per (set, group, window)
// row as keep ~256k segment threads busy, at most nbuck / 8. Each extra segment costs its offset multiple (segoff:
// ~log2 k doublings) and a tree level; with thousands of groups (the bisection's 256- and 32-round levels) the rows
// alone fill the chip, and geom_for's fixed 8-bucket segments had doubled the reduction's additions there (a
// 129-bucket row: 16 segments = 256 + ~150 segoff additions against 256 + 7 for 2).
static void fit_segments(dh::msm_geom& g, size_t ngroups, size_t nsets) {
  const size_t rows = std::max<size_t>(1, nsets * ngroups * (size_t)dh::msm_rows(g));
  const size_t want = ((size_t)1 << 18) / rows + 1;
  size_t nseg = std::max<size_t>(1, std::min<size_t>({want, (size_t)g.nseg}));
  if (nseg > 512) nseg &= ~(size_t)511;  // rows of more than 64 lanes of 8 segments fill whole waves (k_msm_rowtree28)
  g.nseg = (uint32_t)nseg;
  g.seglen = (g.nbuck - 1 + g.nseg - 1) / g.nseg;
}

constexpr size_t JAC_WORDS_G1 = 36, JAC_WORDS_G2 = 72;

// ---- live per-kernel timing with HIP events on the launching stream (dh_profile / dh_profile_read)
struct prof_entry {
  uint64_t count = 0;
  double ms = 0;
  unsigned long long prods = 0;  // field products executed (counting build only)
};
struct prof_pending {
  const char* name;
  hipEvent_t a, b;
  unsigned long long prods;
};
struct profiler {
  std::mutex mu;
  std::atomic<bool> on{false};  // read on every launch without the lock
  std::vector<std::pair<std::string, prof_entry>> table;
  std::vector<prof_pending> pending;  // launches whose end event had not completed when their call returned
  void add(const char* name, float ms, unsigned long long prods = 0) {
    std::lock_guard<std::mutex> lk(mu);
    add_locked(name, ms, prods);
  }
  void add_locked(const char* name, float ms, unsigned long long prods) {
    for (auto& e : table)
      if (e.first == name) {
        e.second.count++;
        e.second.ms += ms;
        e.second.prods += prods;
        return;
      }
    prof_entry pe;
    pe.count = 1;
    pe.ms = ms;
    pe.prods = prods;
    table.emplace_back(name, pe);
  }
};
profiler g_prof;

static void prof_settle(const char* name, hipEvent_t a, hipEvent_t b, unsigned long long prods) {
  float ms = 0;
  if (hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess) g_prof.add(name, ms, prods);
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
}
// resolve the deferred launches (waits for them); called with g_prof.mu held
static void prof_drain_locked() {
  for (auto& r : g_prof.pending) {
    float ms = 0;
    if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess)
      g_prof.add_locked(r.name, ms, r.prods);
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  g_prof.pending.clear();
}

#ifdef DH_COUNT_PRODUCTS
// counting build: products executed by every translation unit's kernels since the last take
static unsigned long long count_take_all() {
  unsigned long long t = 0, v = 0;
  hipError_t (*take[])(unsigned long long*) = {dh::count_take_prep, dh::count_take_msm, dh::count_take_check,
                                               dh::count_take_sign, dh::count_take_recover, dh::count_take_vm,
                                               dh::count_take_schnorr};
  for (auto f : take)
    if (f(&v) == hipSuccess) t += v;
  return t;
}
#endif

// records a launch bracketed by events when profiling is on; resolved after the stream syncs. The counting build
// also synchronises after each launch and attributes the products executed to it (one batch at a time).
struct timed_launches {
  struct rec {
    const char* name;
    hipEvent_t a, b;
    unsigned long long prods;
  };
  std::vector<rec> recs;
  hipStream_t st;
  explicit timed_launches(hipStream_t s) : st(s) {}
  template <class F>
  hipError_t run(const char* name, F&& f) {
    if (!g_prof.on.load(std::memory_order_relaxed)) return f();
    rec r{name, nullptr, nullptr, 0};
    (void)hipEventCreate(&r.a);
    (void)hipEventCreate(&r.b);
#ifdef DH_COUNT_PRODUCTS
    (void)hipDeviceSynchronize();
    (void)count_take_all();
#endif
    (void)hipEventRecord(r.a, st);
    hipError_t e = f();
    (void)hipEventRecord(r.b, st);
#ifdef DH_COUNT_PRODUCTS
    (void)hipDeviceSynchronize();
    r.prods = count_take_all();
#endif
    recs.push_back(r);
    return e;
  }
  // launches still running (a node batch's begin returns with its kernels queued) are resolved later, when the
  // profile is read, so timing never adds a host wait
  void resolve() {
    for (auto& r : recs) {
      if (hipEventQuery(r.b) == hipErrorNotReady) {
        std::lock_guard<std::mutex> lk(g_prof.mu);
        g_prof.pending.push_back({r.name, r.a, r.b, r.prods});
        continue;
      }
      prof_settle(r.name, r.a, r.b, r.prods);
    }
    recs.clear();
  }
  ~timed_launches() { resolve(); }
};

// Pairing checks: the lane-parallel program (k_vm.hip) unless DRANDHIP_LANE_PAIRING=1 selects the one-lane
// tower code (k_check.hip), kept as the independent second implementation the parity tests compare against.
static bool lane_pairing() {
  static const bool v = env_on("DRANDHIP_LANE_PAIRING", false);
  return v;
}

// key_h: [h_eff] pk next to a decoded G2 key (k_decode_key), or null (the check clears B's cofactor itself)
// G2-signature group checks of up to this many groups clear B's cofactor inside the pairing program (NP2C: the
// clearing's doublings spread over the lanes) instead of on one lane before it; DRANDHIP_NP2C=0 turns it off. Above
// it the one-lane clearing wins: every group's lane runs in parallel, the NP2C workgroups queue for the CUs.
static size_t np2c_max_groups() {
  static const size_t v = env_on("DRANDHIP_NP2C", true) ? 4096 : 0;
  return v;
}

// G2-signature leaves (per-round checks: bisection leaves and the small-batch path) likewise, up to this many per
// launch; DRANDHIP_NP2C_LEAVES overrides (0: every leaf clears its hash point on one lane first)
static size_t np2c_max_leaves() {
  static const size_t v = (size_t)env_long("DRANDHIP_NP2C_LEAVES", 4096);
  return v;
}

// G1-signature checks with [h_eff] pk at hand take their G1 sides in Jacobian form (NP2J: no prep kernel, no
// inversion before the program); DRANDHIP_G1_JAC=0 keeps the affine prep (k_vm_prep_groups / _leaves) for A/B runs
static bool g1_jac() {
  static const bool v = env_on("DRANDHIP_G1_JAC", true);
  return v;
}

static hipError_t group_check(worker* w, bool g2, const uint32_t* A, const uint32_t* B, size_t ngroups, const uint32_t* key,
                              uint8_t* pass, hipStream_t st, const uint32_t* key_h = nullptr) {
  if (lane_pairing()) return dh::launch_group_check(g2, A, B, ngroups, key, pass, st);
  if (!g2 && key_h && g1_jac()) return dh::launch_group_check_g1j(A, B, ngroups, key_h, pass, st);
  hipError_t e;
  if (g2 && ngroups <= np2c_max_groups()) {
    if ((e = w->vm_pairs.ensure(ngroups * dh::group_check_c_pair_words() * 4)) != hipSuccess) return e;
    if ((e = w->vm_live.ensure(ngroups * 3)) != hipSuccess) return e;
    if ((e = w->vm_done.ensure(ngroups)) != hipSuccess) return e;
    return dh::launch_group_check_vm_c(A, B, ngroups, key, w->vm_pairs.as<uint32_t>(), w->vm_live.as<uint8_t>(),
                                       w->vm_done.as<uint8_t>(), pass, st);
  }
  if ((e = w->vm_pairs.ensure(ngroups * 2 * 72 * 4)) != hipSuccess) return e;
  if ((e = w->vm_live.ensure(ngroups * 2)) != hipSuccess) return e;
  return dh::launch_group_check_vm(g2, A, B, ngroups, key, g2 ? nullptr : key_h, w->vm_pairs.as<uint32_t>(),
                                   w->vm_live.as<uint8_t>(), pass, st);
}

// key_h as for group_check: the leaves of G1-signature schemes pair the uncleared hash point with [h_eff] pk
static hipError_t leaf_check(worker* w, bool g2, const uint32_t* entries, size_t m, const uint32_t* sig_aff,
                             const uint32_t* q_pts, const uint32_t* key, const uint8_t* status, uint8_t* verdict,
                             hipStream_t st, const uint32_t* key_h = nullptr) {
  if (lane_pairing()) return dh::launch_leaf_check(g2, entries, m, sig_aff, q_pts, key, status, verdict, st);
  if (!g2 && key_h && g1_jac()) return dh::launch_leaf_check_g1j(entries, m, sig_aff, q_pts, key_h, status, verdict, st);
  hipError_t e;
  if (g2 && m <= np2c_max_leaves()) {
    if ((e = w->vm_pairs.ensure(m * dh::group_check_c_pair_words() * 4)) != hipSuccess) return e;
    if ((e = w->vm_live.ensure(m * 3)) != hipSuccess) return e;
    if ((e = w->vm_done.ensure(m)) != hipSuccess) return e;
    return dh::launch_leaf_check_vm_c(entries, m, sig_aff, q_pts, key, status, w->vm_pairs.as<uint32_t>(),
                                      w->vm_live.as<uint8_t>(), w->vm_done.as<uint8_t>(), verdict, st);
  }
  if ((e = w->vm_pairs.ensure(m * 2 * 72 * 4)) != hipSuccess) return e;
  if ((e = w->vm_live.ensure(m * 2)) != hipSuccess) return e;
  if ((e = w->vm_done.ensure(m)) != hipSuccess) return e;
  return dh::launch_leaf_check_vm(g2, entries, m, sig_aff, q_pts, key, g2 ? nullptr : key_h, status,
                                  w->vm_pairs.as<uint32_t>(), w->vm_live.as<uint8_t>(), w->vm_done.as<uint8_t>(), verdict,
                                  st);
}

// Bisection ladder. DRANDHIP_BISECT="4096,256,16,2" fixes the group sizes after level 0 (tests, experiments);
// otherwise next_group_size picks each level from the failure rate the previous level observed.
static const std::vector<size_t>& fixed_ladder() {
  static const std::vector<size_t> v = [] {
    std::vector<size_t> r;
    const char* e = getenv("DRANDHIP_BISECT");
    while (e && *e) {
      char* end = nullptr;
      unsigned long x = strtoul(e, &end, 10);
      if (end == e) break;
      if (x >= 2) r.push_back(x);
      e = *end ? end + 1 : end;
    }
    return r;
  }();
  return v;
}

// Expected-cost choice of the next bisection level (group size; 1 = per-round leaf checks). Level costs
// fitted to the chained-replay sweep on one MI355X (bench/bisect_sweep.sh, ms at 1M G2 rounds): an MSM over m
// rounds costs ~9 + 1.8e-6 m nwin(g), a group-check launch ~12 + 0.0025 groups (the pairing program's
// latency floor), per-round leaf checks ~12 + 0.005 m. Faults are modelled as Poisson at the density the last
// level observed (faulty groups -> -ln(1 - f) faults per group, at least one per failing group; when every
// group failed, 5 per group). The next size minimises the expected cost of the rest of the descent.
static double msm_cost_ms(double m, size_t g) {
  const dh::msm_geom gg = geom_for(g, 2);
  // fitted on 127-bit entries (8 per round at c = 16). Only the levels below level 0 are priced here, and they keep
  // both scalar halves (the one-half level 0 of DESIGN §24 is never a candidate), so the entry count stays nwin x halves
  return 9.0 + 1.8e-6 * m * (double)(gg.nwin * gg.halves) / 2.0;
}
static double check_cost_ms(double groups) { return 12.0 + 0.0025 * groups; }
static double leaf_cost_ms(double m) { return 12.0 + 0.005 * m; }

static double descent_cost(double m, double d, size_t gprev, size_t* best) {
  double c_best = leaf_cost_ms(m);
  if (best) *best = 1;
  for (size_t g = 4; g < gprev && (double)g < m; g *= 4) {
    const double q = -std::expm1(-d * (double)g);  // P(group of g holds a fault)
    const double m_next = m * q;
    const double c = msm_cost_ms(m, g) + check_cost_ms(m / (double)g) +
                     (m_next < 1.0 ? 0.0 : descent_cost(m_next, d / std::max(q, 1e-12), g, nullptr));
    if (c < c_best) {
      c_best = c;
      if (best) *best = g;
    }
  }
  return c_best;
}

static size_t next_group_size(size_t gsize, size_t ngroups, size_t nfail, size_t m_prev, size_t m_next, double hint) {
  // level 0 (one group) says only that some round is bad: 1024 costs about what 4096 does over 1M rounds and
  // its groups still pass at a 0.1% fault density (4096-round groups then all fail). When the worker's previous
  // bisection saw dense faults (> 1 per 2000 rounds: most 1024-groups fail), 256-round groups first: the ladder
  // sweep on a 0.2%-faulty chained window put 256-first ladders 5-9% ahead of 1024-first ones
  // (profiles/bisect_sweep_r03s.txt)
  const bool dense = hint > 1.0 / 2000;
  if (gsize == m_prev && m_prev > 4096) return dense ? 256 : 1024;
  // ... and continues 256 -> 32 -> 4 -> per-round leaves, the best ladder of that sweep (231.7 ms per 1M window
  // against 240-259 for the others); the cost model below was fitted on sparser failures
  if (dense && (gsize == 256 || gsize == 32)) return gsize == 256 ? 32 : 4;
  if (dense && gsize == 4) return 1;
  const double f = (double)nfail / (double)ngroups;
  const double per_group = nfail == ngroups ? 5.0 : -std::log1p(-f);
  const double faults = std::max((double)nfail, per_group * (double)ngroups);
  const double density = std::min(1.0, faults / (double)std::max<size_t>(m_next, 1));
  size_t g = 1;
  descent_cost((double)m_next, density, gsize, &g);
  return g;
}

static bool prep_sync() {
  static const bool v = env_on("DRANDHIP_PREP_SYNC", true);
  return v;
}

// DRANDHIP_SKIP_LEVEL0=0 keeps level 0 on dense-fault workers (comparison runs)
static bool skip_level0() {
  static const bool v = env_on("DRANDHIP_SKIP_LEVEL0", true);
  return v;
}


// core pipeline on device-resident inputs
// Phases of one batch (the node-wide check of dh_batch_begin / dh_batch_finish runs them separately):
enum verify_mode {
  VM_FULL = 0,        // prepare, then every level (local level-0 check)
  VM_BEGIN = 1,       // prepare and the level-0 MSM only: the partial sums are left in outA / outB
  VM_FINISH = 2,      // after VM_BEGIN: local level-0 check and bisection
  VM_FINISH_PASS = 3  // after VM_BEGIN, the node-wide check passed: every decoded round is valid
};

// One-call pipelining (run_split): the per-round kernels of consecutive chunks run one after another, each chunk's
// alone on the chip, while the latency-bound tails of earlier chunks (MSM reduction, pairing checks) run beside
// them on their own streams. A chunk's per-round kernels wait for the previous chunk's (an event), and it records
// its own event once they are queued.
struct prep_gate {
  hipEvent_t wait = nullptr;  // the previous chunk's per-round kernels (null: first chunk)
  hipEvent_t done = nullptr;  // this chunk's
  std::function<void()> recorded;  // host side: `done` is recorded, the next chunk may queue behind it
};

// The batched subgroup test (G2: §14, below): a large local batch of G1 signatures decodes without the
// per-round test
// and tests the bit-subset sums of its level-0 sigma buckets instead. DRANDHIP_SUBGROUP_BATCH=0 keeps the fused
// per-round test everywhere; DRANDHIP_SUB_BATCH_MIN is the smallest batch that takes the batched test. Its default,
// 131,072 rounds, is the first size of the one-call sweep (profiles/r07/sub_batch_min_sweep.jsonl) at which the
// batched path is not slower: the test is one wave's two [|u|] chains on the batch's latency path (1.2-1.8 ms), and
// below ~100k rounds the fused kernel's per-round test costs one call less than that (4,096 rounds: 7.36 ms fused,
// 7.72 batched; 65,536: 8.94 / 9.27; 131,072: 11.10 / 10.96; 1M: 45.7 / 34.2).
static bool subgroup_batch_on() {
  static const bool v = env_on("DRANDHIP_SUBGROUP_BATCH", true);
  return v;
}
static size_t sub_batch_min() {
  static const size_t v = env_size("DRANDHIP_SUB_BATCH_MIN", 131072, 1);
  return v;
}
// The same for G2 signatures: an eligible batch runs its MSMs on two 63-bit psi halves instead of four
// 31-bit parts (the claim needs the halves) and decodes without k_sub_sig_g2. DRANDHIP_SUB_BATCH_MIN_G2 is the
// smallest such batch; DRANDHIP_SUB_BATCH_MIN stays the G1 minimum. Default: SUB_BATCH_MIN_G2_DEFAULT = 393,216
// rounds, the first size of the one-call sweep (profiles/r09/sub_batch_g2_min_sweep.jsonl) from which the batched path
// is not slower at every larger size: the two-half geometry has twice the window rows and the test is 2.8-5.5 ms on
// the latency path (262,144 rounds: 30.5 ms fused, 30.8 batched; 393,216: 39.6-40.2 / 37.9; 1M: 84.4-84.9 / 69.8-70.0).
constexpr size_t SUB_BATCH_MIN_G2_DEFAULT = 393216;
static size_t sub_batch_min_g2() {
  static const size_t v = env_size("DRANDHIP_SUB_BATCH_MIN_G2", SUB_BATCH_MIN_G2_DEFAULT, 1);
  return v;
}
// A batch whose fallback flagged more than one round in 2000 (a replay over a store with corrupted signatures: the
// windows that follow fail alike) sends the worker's next DRANDHIP_SUB_BACKOFF eligible batches (default 15) through
// the fused kernel: such a batch pays the batched test, the exact test and one more MSM level, about 1.4x the fused
// path (profiles/r07/faulted_quicknet_262144_no_backoff.jsonl); sparse faults (the odd bad round) do not start it.
static int sub_backoff() {
  static const int v = [] {
    const long d = env_long("DRANDHIP_SUB_BACKOFF", -1);
    return (int)(d >= 0 && d <= 1 << 20 ? d : 15);
  }();
  return v;
}

// A G1 batch that takes the batched subgroup test runs its decode and its hash as one per-round kernel, the hash
// point's inversion riding on the decode's square-root chain (k_prep.hip round_g1_ride).
// DRANDHIP_G1_RIDE=0 launches the two previous kernels (comparison runs).
static bool g1_ride_on() {
  static const bool v = env_on("DRANDHIP_G1_RIDE", true);
  return v;
}

// Such a batch also leaves the hash's 11-isogeny to the MSM: the per-round kernel stores the affine sum
// of the two SSWU points on E1' straight into the MSM's arrays (no k_msm_prep28 at level 0), level 0 runs with the
// scalar halves in window rows of their own (msm_geom split) and maps the hash set's eight row sums to E1. A batch
// that level 0 does not end falls back to the isogeny per round and the usual arrays (points beside their images) before level 1.
// DRANDHIP_G1_ISO_LATE=0 keeps the isogeny in the per-round kernel (comparison runs).
static bool g1_iso_late_on() {
  static const bool v = env_on("DRANDHIP_G1_ISO_LATE", true);
  return v;
}

// Level 0 of such a batch keys the a-half of each round's scalar alone: r_i = a_i, 63 bits, half the
// sorted-list entries and window rows and no phi of a row sum. A level-0 accept is then wrong with probability at most
// 2^-62 (the batched subgroup test's 2^-63 and the check's 2^-63); a batch that level 0 does not end is re-checked by
// the fallback and the bisection on r_i = a_i + mu b_i, as before. DRANDHIP_G1_RLC_HALF=0 keeps both halves at level 0.
static bool g1_rlc_half_on() {
  static const bool v = env_on("DRANDHIP_G1_RLC_HALF", true);
  return v;
}
// the shape of the calling thread's last level-0 MSM (dh_msm_level0_shape_debug)
struct level0_shape {
  uint64_t rows = 0, entries = 0;
  int half_a = 0, half_b = 0;
};
static thread_local level0_shape g_level0;

// MSM workspace of one bisection level (m entries in ngroups groups of geometry g, Jacobian width jw words); sub: also
// the batched subgroup test's scratch (ws.sub)
static int msm_workspace(worker* w, const dh::msm_geom& g, size_t m, size_t ngroups, size_t jw, dh::msm_ws& ws,
                         bool sub = false, bool g2 = false) {
  const size_t nk = ngroups * dh::msm_rows(g) * (size_t)g.nbuck;
  HIP_TRY(w->cnt.ensure(nk * 4));
  HIP_TRY(w->off.ensure((nk + 1) * 4));
  HIP_TRY(w->scan_tmp.ensure(((nk + 4095) / 4096 + 1) * 4));
  HIP_TRY(w->list.ensure(dh::msm_entries(g, m) * 4));
  HIP_TRY(w->buckets.ensure(2 * nk * jw * 4));
  const size_t segs_bytes = 2 * ngroups * dh::msm_rows(g) * g.nseg * jw * 4;
  HIP_TRY(w->segs.ensure(2 * segs_bytes));  // segment sums, then (MSM28) the segments' running sums
  HIP_TRY(w->outA.ensure(ngroups * jw * 4));
  HIP_TRY(w->outB.ensure(ngroups * jw * 4));
  HIP_TRY(w->out2.ensure(2 * ngroups * jw * 4));
  HIP_TRY(w->pass.ensure(ngroups));
  HIP_TRY(w->part.ensure(dh::msm_part_bytes(dh::msm_entries(g, m), jw, 2)));
  HIP_TRY(w->meta.ensure(dh::msm_meta_bytes(dh::msm_entries(g, m))));
  ws = dh::msm_ws{w->cnt.as<uint32_t>(), w->off.as<uint32_t>(), w->scan_tmp.as<uint32_t>(), w->list.as<uint32_t>(),
                  w->buckets.as<uint32_t>(), w->segs.as<uint32_t>(), w->out2.as<uint32_t>(), w->part.as<uint32_t>(),
                  w->meta.as<uint32_t>(), 0, (uint32_t*)((uint8_t*)w->segs.p + segs_bytes)};
  if (sub) {
    HIP_TRY(w->sub_tmp.ensure(dh::sub_batch_tmp_bytes(g2, g)));
    HIP_TRY(w->sub_pass.ensure(8));  // the result byte, and at byte 4 the fallback's count of flagged rounds
    ws.sub = w->sub_tmp.as<uint32_t>();
  }
  return DH_OK;
}

int verify_core(worker* w, int scheme, const uint8_t* pk, size_t pk_len, const uint64_t* d_rounds, const uint8_t* d_sigs,
                size_t sig_stride, const uint8_t* d_prevs, size_t prev_stride, const uint32_t* d_prev_lens, size_t n,
                uint8_t* d_verdict, uint8_t* d_rand, uint64_t seed, hipStream_t st, uint64_t* stats,
                const uint8_t* d_msgs32 = nullptr, int mode = VM_FULL, prep_gate* gate = nullptr) {
  const bool g2 = sig_on_g2(scheme);
  const int sig_len = g2 ? 96 : 48, key_len = g2 ? 48 : 96;
  if ((int)pk_len != key_len) return fail(DH_EINVAL, "public key must be %d bytes for scheme %d", key_len, scheme);
  if (sig_stride < (size_t)sig_len || sig_stride % 4) return fail(DH_EINVAL, "bad signature stride %zu", sig_stride);
  if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
  if (n == 0) return DH_OK;
  // the MSM runs on lazily reduced 28-bit points (k_msm.hip MSM28), whose workspace points take 48 (G1) / 96 (G2)
  // words; G2 splits each scalar in four psi parts, G1 in two endomorphism halves; a G2 batch that takes the batched
  // subgroup test runs on two 63-bit psi halves at every level (parts, below). (r01-r03 also kept a 12 x 32-bit
  // Pippenger behind DRANDHIP_MSM32 as a second implementation; removed in r04, git history has it.)
  const size_t jw = g2 ? JAC_WORDS_G2 : JAC_WORDS_G1;
  const size_t aw = jw * 2 / 3;
  const size_t wsw = g2 ? 96 : 48;

  timed_launches T(st);
  // the whole batch on st (no tail-stream handoff, no level-0 presort there): a node batch's begin (begin_one_stream).
  // A local batch keeps the handoff after its host wait: measured on one stream too (gpurun_out r04aa), 1M rounds
  // 26.58 -> 26.41 M/s and one 1M call 46.2 -> 47.5 ms (the presort no longer overlaps the per-round kernels), 131k
  // rounds 20.76 -> 21.46 M/s.
  const bool one_stream = mode == VM_BEGIN && w->begin_one_stream;
  bool presorted = false;  // level-0 sorted lists already built on the tail stream
  // A local batch on a worker whose last bisection saw dense faults skips level 0: its one group is expected to fail,
  // so the batch starts at the dense ladder's 256-round groups (their check also answers "is the batch clean": a
  // batch whose groups all pass clears the hint). Saves the level-0 MSM and pairing check per dense window.
  // (with a fixed ladder, DRANDHIP_BISECT, its first size)
  const bool skip0 = mode == VM_FULL && w->fault_density > 1.0 / 2000 && n > 4096 && skip_level0();
  // the batched subgroup test: a local batch with its own level 0, large enough (sub_batch_min, sub_batch_min_g2).
  // Node batches (VM_BEGIN and the VM_FINISH modes resuming them) never take it, so both halves of such a batch
  // compute the same parts.
  const bool sub_eligible = mode == VM_FULL && !skip0 && n >= 2 && n >= (g2 ? sub_batch_min_g2() : sub_batch_min()) &&
                            subgroup_batch_on();
  const bool sub_batch = sub_eligible && w->sub_fused_left == 0;
  if (sub_eligible && w->sub_fused_left > 0) w->sub_fused_left--;  // after a dense fallback (sub_backoff)
  const int parts = g2 && !sub_batch ? 4 : 2;
  const bool g1_ride = !g2 && sub_batch && g1_ride_on();
  const bool iso_late = g1_ride && g1_iso_late_on();  // level 0 on split rows, the hash set on E1'
  const bool rlc_half = iso_late && g1_rlc_half_on();  // and on the scalars' a-halves alone
  // sorted-list entries keep a sign bit and address parts * n points (the endomorphism images follow the n points)
  if (n >= ((size_t)1 << 31) / parts) return fail(DH_EINVAL, "batch too large");
  dh::msm_geom g0{};
  dh::msm_ws ws0{};
  if (mode <= VM_BEGIN) {
    // key (cached per worker; a miss synchronises once, before any per-round kernel is queued)
    int rc = ensure_key(w, g2, pk, pk_len, st);
    if (rc) return rc;

    // per-round prep
    HIP_TRY(w->status.ensure(n));
    HIP_TRY(w->sig_aff.ensure(n * aw * 4));
    HIP_TRY(w->q_pts.ensure(n * jw * 4));
    HIP_TRY(w->scal.ensure(n * 16));
    HIP_TRY(w->entries.ensure(n * 4));
    uint32_t seedw[8];
    rc = make_seed(seed, seedw);
    if (rc) return rc;
    uint32_t* d_seed = (uint32_t*)((uint8_t*)w->key_ok.p + 32);
    // The level-0 sort needs only the scalars, and the scalars only the seed: with a tail stream it runs there
    // while the per-round kernels decode and hash (its ~1 ms of small kernels left the one-call latency path).
    // Every round then carries a scalar; the bucket passes skip rounds whose status is not DEC_OK. A batch that skips
    // level 0 (skip0) has no level-0 sort.
    presorted = w->tail && st == w->stream && !skip0 && !one_stream;
    if (presorted) {
      hipStream_t ts = w->tail;
      HIP_TRY(hipMemcpyAsync(d_seed, seedw, 32, hipMemcpyHostToDevice, ts));
      HIP_TRY(dh::launch_scalars(d_seed, n, nullptr, w->scal.as<uint4>(), parts, ts));
      HIP_TRY(dh::launch_iota(w->entries.as<uint32_t>(), n, ts));
      g0 = geom_for(n, parts);
      g0.half_stride = (uint32_t)n;
      g0.split = iso_late ? 1 : 0;
      g0.half0 = rlc_half ? 1 : 0;
      rc = msm_workspace(w, g0, n, 1, wsw, ws0, sub_batch, g2);
      if (rc) return rc;
      HIP_TRY(dh::launch_msm_sort(g0, w->entries.as<uint32_t>(), nullptr, nullptr, n, 1, w->scal.as<uint4>(), ws0, ts));
    }
    if (gate && gate->wait) HIP_TRY(hipStreamWaitEvent(st, gate->wait, 0));
    const int chained = scheme == DH_SCHEME_CHAINED && d_prevs && !d_msgs32 ? 1 : 0;
    HIP_TRY(w->s28.ensure(parts * n * (g2 ? 64 : 32) * 4));
    HIP_TRY(w->q28.ensure(parts * n * (g2 ? 64 : 32) * 4));
    if (iso_late) {
      // decode and hash in one launch, sigma and the E1' hash point straight into the MSM's arrays
      HIP_TRY(T.run(d_msgs32 ? "k_prep_msg32<fp>" : "k_prep_msg<fp>", [&] {
        return dh::launch_round_g1_ride_late(d_rounds, d_prevs, prev_stride, d_prev_lens, d_msgs32, n, chained, dst_id(scheme),
                                             d_sigs, sig_stride, w->status.as<uint8_t>(), w->sig_aff.as<uint32_t>(), d_rand,
                                             w->q_pts.as<uint32_t>(), w->s28.as<uint32_t>(), w->q28.as<uint32_t>(), st);
      }));
    } else if (g1_ride) {
      // decode and hash in one launch (reported under the hash's stage name)
      HIP_TRY(T.run(d_msgs32 ? "k_prep_msg32<fp>" : "k_prep_msg<fp>", [&] {
        return dh::launch_round_g1_ride(d_rounds, d_prevs, prev_stride, d_prev_lens, d_msgs32, n, chained, dst_id(scheme), d_sigs,
                                        sig_stride, w->status.as<uint8_t>(), w->sig_aff.as<uint32_t>(), d_rand,
                                        w->q_pts.as<uint32_t>(), st);
      }));
    } else {
      HIP_TRY(T.run(g2 ? "k_prep_sig<fp2>" : "k_prep_sig<fp>", [&] {
        return dh::launch_prep(g2, d_sigs, sig_stride, n, w->status.as<uint8_t>(), w->sig_aff.as<uint32_t>(), d_rand, st,
                               sub_batch);
      }));
      // hash points: of the beacon digests, or of the given 32-byte messages (VerifyRecovered); a chained record
      // longer than its slot rejects its round (status)
      HIP_TRY(w->h2c_tmp.ensure(dh::hash_tmp_bytes(g2, n)));
      HIP_TRY(T.run(d_msgs32 ? (g2 ? "k_prep_msg32<fp2>" : "k_prep_msg32<fp>") : (g2 ? "k_prep_msg<fp2>" : "k_prep_msg<fp>"), [&] {
        return dh::launch_hash(g2, d_rounds, d_prevs, prev_stride, d_prev_lens, d_msgs32, n, chained, dst_id(scheme),
                               w->status.as<uint8_t>(), w->q_pts.as<uint32_t>(), w->h2c_tmp.as<uint32_t>(), st);
      }));
    }
    if (!presorted) {
      HIP_TRY(hipMemcpyAsync(d_seed, seedw, 32, hipMemcpyHostToDevice, st));
      HIP_TRY(dh::launch_scalars(d_seed, n, w->status.as<uint8_t>(), w->scal.as<uint4>(), parts, st));
    }
    if (!iso_late) {
      HIP_TRY(T.run(g2 ? "k_msm_prep28<fp2>" : "k_msm_prep28<fp>", [&] {
        return dh::launch_msm_prep28(g2, n, w->status.as<uint8_t>(), w->sig_aff.as<uint32_t>(), w->q_pts.as<uint32_t>(),
                                     w->s28.as<uint32_t>(), w->q28.as<uint32_t>(), st, 3, parts);
      }));
    }
    HIP_TRY(hipMemsetAsync(d_verdict, 0, n, st));
    if (gate) {
      HIP_TRY(hipEventRecord(gate->done, st));
      gate->recorded();
    }
    // The node batch (VM_BEGIN) queues its tail behind the per-round kernels with no host wait. A local batch
    // (VM_FULL) waits here first, as r03 did: its tail stream then carries no event wait while the per-round kernels
    // run, and with 8 batches in flight (16+ streams on 16 hardware queues) a queue blocked on such a wait holds up
    // the streams that share it (quicknet 1M: 25.5-25.9 M/s without this wait, 26.4-26.5 with it; DRANDHIP_PREP_SYNC=0
    // drops it for comparison).
    if (mode == VM_FULL && w->tail && st == w->stream && !one_stream && prep_sync()) HIP_TRY(hipStreamSynchronize(st));
    if (!presorted) HIP_TRY(dh::launch_iota(w->entries.as<uint32_t>(), n, st));
  }
  // the tail (MSM, checks, bisection) runs on the worker's high-priority stream, after the per-round kernels
  if (w->tail && st == w->stream && !one_stream) {
    if (mode <= VM_BEGIN) {
      HIP_TRY(hipEventRecord(w->handoff, st));
      HIP_TRY(hipStreamWaitEvent(w->tail, w->handoff, 0));
    }
    st = w->tail;
    T.st = st;
  }

  // bisection levels: group sizes n, then next_group_size() per level, then per-round leaves (a failing group is re-checked
  // as smaller groups with the same scalars; only rounds of failing pairs reach a per-round pairing check)
  size_t m = n;
  static const char* const msm_names[8] = {"msm_level0", "msm_bisect1", "msm_bisect2", "msm_bisect3",
                                           "msm_bisect4", "msm_bisect5", "msm_bisect6", "msm_bisect7+"};
  static const char* const chk_names[8] = {"k_group_check_level0", "k_group_check_bisect1", "k_group_check_bisect2",
                                           "k_group_check_bisect3", "k_group_check_bisect4", "k_group_check_bisect5",
                                           "k_group_check_bisect6", "k_group_check_bisect7+"};
  const std::vector<size_t>& fixed = fixed_ladder();
  size_t gsize = skip0 ? (fixed.empty() ? 256 : fixed[0]) : n;
  int level = skip0 ? 1 : 0;
  if (mode == VM_BEGIN && n < 2) {
    // a one-round batch has no level-0 group: it contributes the identity (Z = 0) to the node-wide sums, and
    // dh_batch_finish gives the round its own leaf check whatever the node check says
    HIP_TRY(w->outA.ensure(jw * 4));
    HIP_TRY(w->outB.ensure(jw * 4));
    HIP_TRY(hipMemsetAsync(w->outA.p, 0, jw * 4, st));
    HIP_TRY(hipMemsetAsync(w->outB.p, 0, jw * 4, st));
    return DH_OK;  // queued: dh_batch_begin orders the caller after it (or waits)
  }
  while (m > 0 && gsize > 1) {
    gsize = std::min(gsize, m);
    dh::msm_geom g = geom_for(gsize, parts);
    g.half_stride = (uint32_t)n;
    g.split = level == 0 && iso_late ? 1 : 0;
    g.half0 = level == 0 && rlc_half ? 1 : 0;
    const size_t ngroups = (m + gsize - 1) / gsize;
    fit_segments(g, ngroups, 2);
    const bool pre = level == 0 && presorted;
    dh::msm_ws ws{};
    if (pre) {
      ws = ws0;
    } else {
      const int rc = msm_workspace(w, g, m, ngroups, wsw, ws, level == 0 && sub_batch, g2);
      if (rc) return rc;
    }
    if (level == 0 && mode == VM_FULL) {
      const dh::msm_geom& gl = pre ? g0 : g;
      g_level0 = level0_shape{dh::msm_rows(gl), dh::msm_entries(gl, m), 1, dh::msm_keyed(gl) > 1 ? 1 : 0};
    }
    if (!(level == 0 && mode >= VM_FINISH)) {  // a resumed batch has its level-0 sums from dh_batch_begin
      // every level skips the rounds whose status is not DEC_OK (their scalars are nonzero after a presort)
      HIP_TRY(T.run(msm_names[std::min(level, 7)], [&] {
        return dh::launch_msm28(g2, pre ? g0 : g, w->entries.as<uint32_t>(), m, ngroups, w->scal.as<uint4>(),
                                w->s28.as<uint32_t>(), w->q28.as<uint32_t>(), ws, w->outA.as<uint32_t>(),
                                w->outB.as<uint32_t>(), st, w->status.as<uint8_t>(), pre);
      }));
    }
    if (level == 0 && mode == VM_BEGIN) return DH_OK;  // queued; dh_batch_begin orders the caller after it
    if (level == 0 && mode == VM_FINISH_PASS) {  // the node-wide check covers this batch's single level-0 group
      HIP_TRY(hipMemsetAsync(w->pass.p, 1, 1, st));
    } else {
      HIP_TRY(T.run(chk_names[std::min(level, 7)], [&] {
        return group_check(w, g2, w->outA.as<uint32_t>(), w->outB.as<uint32_t>(), ngroups, w->key_cur, w->pass.as<uint8_t>(),
                           st, w->key_cur + 48);
      }));
    }
    // level 0 of a batch that decoded without the per-round subgroup test: the test of the sigma buckets' bit-subset
    // sums, ANDed into the group's pass before the marking and the compaction below read it
    const bool sub0 = level == 0 && sub_batch;
    if (sub0) {
      HIP_TRY(T.run("k_sub_batch_level0", [&] {
        return dh::launch_sub_batch(g2, pre ? g0 : g, ws, w->pass.as<uint8_t>(), w->sub_pass.as<uint8_t>(), st);
      }));
    }
    HIP_TRY(dh::launch_mark_groups(w->entries.as<uint32_t>(), m, gsize, w->pass.as<uint8_t>(), w->status.as<uint8_t>(),
                                   d_verdict, st));
    // failing groups' entries compacted on the device; only the failing-group count and the last group's flag
    // come back to the host (they size the next level)
    HIP_TRY(w->cflags.ensure(ngroups * 4));
    HIP_TRY(w->crank.ensure((ngroups + 1) * 4));
    HIP_TRY(w->cscan.ensure(((ngroups + 4095) / 4096 + 1) * 4));
    HIP_TRY(w->entries_alt.ensure(m * 4));
    HIP_TRY(dh::launch_compact_failing(w->entries.as<uint32_t>(), m, gsize, ngroups, w->pass.as<uint8_t>(),
                                       w->cflags.as<uint32_t>(), w->crank.as<uint32_t>(), w->cscan.as<uint32_t>(),
                                       w->entries_alt.as<uint32_t>(), st));
    uint32_t nfail32 = 0;
    uint8_t last_pass = 1;
    HIP_TRY(hipMemcpyAsync(&nfail32, w->crank.as<uint32_t>() + ngroups, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&last_pass, w->pass.as<uint8_t>() + ngroups - 1, 1, hipMemcpyDeviceToHost, st));
    uint8_t sub_pass = 1;
    if (sub0) HIP_TRY(hipMemcpyAsync(&sub_pass, w->sub_pass.p, 1, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!sub_pass) {
      // some T is outside the signature group: the exact per-round test, before the next level's MSM. The flagged rounds
      // become DEC_BAD as the fused kernel leaves them, the bisection's bucket passes and leaves skip them: the verdicts
      // of the fused path
      HIP_TRY(w->sub_bad.ensure(n));
      HIP_TRY(T.run("k_sub_exact", [&] {
        return dh::launch_sub_exact(g2, n, w->status.as<uint8_t>(), w->sig_aff.as<uint32_t>(), w->sub_bad.as<uint8_t>(),
                                    (uint32_t*)((uint8_t*)w->sub_pass.p + 4), st);
      }));
      uint32_t nbad = 0;
      HIP_TRY(hipMemcpyAsync(&nbad, (uint8_t*)w->sub_pass.p + 4, 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if ((double)nbad * 2000 > (double)n) w->sub_fused_left = sub_backoff();
    }
    if (level == 0 && iso_late && nfail32) {
      // level 0 did not end the batch: the isogeny per round after all, then the usual arrays (both sets with their
      // images), so that the bisection and the leaves see what they see without the deferral
      HIP_TRY(T.run("k_msm_prep28<fp>", [&] {
        hipError_t e = dh::launch_iso_late_fallback(n, w->status.as<uint8_t>(), w->q28.as<uint32_t>(), w->q_pts.as<uint32_t>(), st);
        if (e != hipSuccess) return e;
        return dh::launch_msm_prep28(0, n, w->status.as<uint8_t>(), w->sig_aff.as<uint32_t>(), w->q_pts.as<uint32_t>(),
                                     w->s28.as<uint32_t>(), w->q28.as<uint32_t>(), st, 3, parts);
      }));
    }
    level++;
    const size_t nfail = nfail32;
    if (stats) stats[1] += nfail;
    if (level == 1 && nfail == 0) w->fault_density = 0;  // a clean batch clears the density hint
    if (level == 2) {  // the first bisection level's failure rate: the density hint of the worker's next batch
      const double f = (double)nfail / (double)ngroups;
      w->fault_density = (f >= 1.0 ? 5.0 : -std::log1p(-f)) / (double)gsize;
    }
    if (nfail == 0) {
      m = 0;
      break;
    }
    std::swap(w->entries, w->entries_alt);
    const size_t m_prev = m;
    m = nfail * gsize - (last_pass ? 0 : ngroups * gsize - m_prev);  // only the last group may be short
    gsize = fixed.empty() ? next_group_size(gsize, ngroups, nfail, m_prev, m, w->fault_density)
                          : (size_t)(level - 1 < (int)fixed.size() ? fixed[level - 1] : 1);
  }
  if (m > 0) {
    HIP_TRY(T.run("k_leaf_check", [&] {
      return leaf_check(w, g2, w->entries.as<uint32_t>(), m, w->sig_aff.as<uint32_t>(), w->q_pts.as<uint32_t>(),
                        w->key_cur, w->status.as<uint8_t>(), d_verdict, st, w->key_cur + 48);
    }));
    if (stats) stats[2] = m;
  }
  if (stats) {  // rejected = decode/subgroup failures + failed leaves (1 MB D2H per 1M rounds, only when asked)
    w->h_verdict.resize(n);
    HIP_TRY(hipMemcpyAsync(w->h_verdict.data(), d_verdict, n, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  if (stats) {
    stats[0] = (uint64_t)level;
    size_t ok = 0;
    for (uint8_t v : w->h_verdict) ok += v ? 1 : 0;
    stats[3] = n - ok;
  }
  return DH_OK;
}

// ---- small batches: the one-beacon calls of the drop-in (VerifyBeacon from the gossip validator and the client,
// VerifyRecovered from the aggregator) and any batch of at most small_batch_max() rounds. No scalars, sort or MSM: the
// signature kernels (decode, subgroup test, randomness) on the worker's stream and the hash kernels on its tail stream
// run side by side, then every round gets its own 2-pairing check (the leaves of the batch path: bit-exact per-round
// verdicts by construction). A round's check is one wave per round, so up to a few hundred rounds cost what one does;
// larger batches amortise one group check over an MSM instead (verify_core). DRANDHIP_SMALL_N overrides (0: off).
static size_t small_batch_max() {
  static const size_t v = (size_t)env_long("DRANDHIP_SMALL_N", 64);
  return v;
}

// Queues the whole check on st (and the worker's tail stream); the caller reads the outputs after a stream sync.
// Lengths d_prev_lens the host has not checked (lens_checked): the hash kernels stay on st, behind the signature
// kernels, because a chained record longer than its slot marks its round in status (launch_hash).
int verify_small(worker* w, int scheme, const uint8_t* pk, size_t pk_len, const uint64_t* d_rounds, const uint8_t* d_sigs,
                 size_t sig_stride, const uint8_t* d_prevs, size_t prev_stride, const uint32_t* d_prev_lens, size_t n,
                 uint8_t* d_verdict, uint8_t* d_rand, const uint8_t* d_msgs32, hipStream_t st, bool lens_checked) {
  const bool g2 = sig_on_g2(scheme);
  const int sig_len = g2 ? 96 : 48, key_len = g2 ? 48 : 96;
  if ((int)pk_len != key_len) return fail(DH_EINVAL, "public key must be %d bytes for scheme %d", key_len, scheme);
  if (sig_stride < (size_t)sig_len || sig_stride % 4) return fail(DH_EINVAL, "bad signature stride %zu", sig_stride);
  if (n == 0) return DH_OK;
  int rc = ensure_key(w, g2, pk, pk_len, st);
  if (rc) return rc;
  const size_t jw = g2 ? JAC_WORDS_G2 : JAC_WORDS_G1;
  const size_t aw = jw * 2 / 3;
  HIP_TRY(w->status.ensure(n));
  HIP_TRY(w->sig_aff.ensure(n * aw * 4));
  HIP_TRY(w->q_pts.ensure(n * jw * 4));
  HIP_TRY(w->entries.ensure(n * 4));
  HIP_TRY(w->h2c_tmp.ensure(dh::hash_small_tmp_bytes(g2, n)));
  const bool chained = scheme == DH_SCHEME_CHAINED && d_prevs && !d_msgs32;
  const bool fork = w->tail && !(chained && d_prev_lens && !lens_checked);
  HIP_TRY(w->sub_bad.ensure(n));
  // Two streams: A = st decodes the signatures, then runs their subgroup tests; B = the tail stream hashes the
  // messages, waits for the decode, runs the per-round pairing checks beside the subgroup tests, then ANDs their
  // result into the verdicts; st joins B. Unforked (unchecked lengths): all of it on st, the hash after the decode.
  hipStream_t hs = fork ? w->tail : st;
  if (fork) {
    HIP_TRY(hipEventRecord(w->handoff, st));
    HIP_TRY(hipStreamWaitEvent(hs, w->handoff, 0));
  }
  timed_launches T(st), TH(hs);
  HIP_TRY(T.run(g2 ? "k_dec_sig_small<fp2>" : "k_dec_sig_small<fp>", [&] {
    return dh::launch_dec_sig(g2, d_sigs, sig_stride, n, w->status.as<uint8_t>(), w->sig_aff.as<uint32_t>(), d_rand, st);
  }));
  if (fork) HIP_TRY(hipEventRecord(w->ev_dec, st));
  HIP_TRY(TH.run(d_msgs32 ? (g2 ? "k_prep_msg32<fp2>" : "k_prep_msg32<fp>") : (g2 ? "k_prep_msg<fp2>" : "k_prep_msg<fp>"), [&] {
    return dh::launch_hash_small(g2, d_rounds, d_prevs, prev_stride, d_prev_lens, d_msgs32, n, chained ? 1 : 0, dst_id(scheme),
                                 fork ? nullptr : w->status.as<uint8_t>(), w->q_pts.as<uint32_t>(), w->h2c_tmp.as<uint32_t>(), hs);
  }));
  HIP_TRY(T.run(g2 ? "k_sub_sig_small<fp2>" : "k_sub_sig_small<fp>", [&] {
    return dh::launch_sub_flag(g2, n, w->status.as<uint8_t>(), w->sig_aff.as<uint32_t>(), w->sub_bad.as<uint8_t>(), st);
  }));
  if (fork) {
    HIP_TRY(hipEventRecord(w->ev_sub, st));
    HIP_TRY(hipStreamWaitEvent(hs, w->ev_dec, 0));
  }
  HIP_TRY(dh::launch_iota(w->entries.as<uint32_t>(), n, hs));
  HIP_TRY(TH.run("k_leaf_check", [&] {
    return leaf_check(w, g2, w->entries.as<uint32_t>(), n, w->sig_aff.as<uint32_t>(), w->q_pts.as<uint32_t>(),
                      w->key_cur, w->status.as<uint8_t>(), d_verdict, hs, w->key_cur + 48);
  }));
  if (fork) HIP_TRY(hipStreamWaitEvent(hs, w->ev_sub, 0));
  HIP_TRY(dh::launch_and_subgroup(n, w->sub_bad.as<uint8_t>(), d_verdict, hs));
  if (fork) {
    HIP_TRY(hipEventRecord(w->join, hs));
    HIP_TRY(hipStreamWaitEvent(st, w->join, 0));
  }
  return DH_OK;
}

// host-side staging of a small batch: the arrays packed into the worker's pinned buffer, one copy each way
struct stage_part {
  const void* src;
  size_t bytes;
  size_t slack = 0;  // zeroed bytes after the part (the digest kernel's word loads past the last chained record)
  size_t off = 0;
};
static int stage_in(worker* w, stage_part* parts, int k, size_t out_bytes, hipStream_t st, uint8_t** d_base, size_t* out_off) {
  size_t tot = 0;
  for (int i = 0; i < k; i++) {
    parts[i].off = tot;
    tot += (parts[i].bytes + parts[i].slack + 15) & ~(size_t)15;
  }
  *out_off = tot;
  const size_t need = tot + out_bytes;
  if (need > w->h_stage_cap) {
    if (w->h_stage) (void)hipHostFree(w->h_stage);
    w->h_stage = nullptr;
    w->h_stage_cap = 0;
    const size_t cap = std::max(need, (size_t)65536);
    HIP_TRY(hipHostMalloc(&w->h_stage, cap, hipHostMallocDefault));
    w->h_stage_cap = cap;
  }
  HIP_TRY(w->d_stage.ensure(need));
  uint8_t* h = (uint8_t*)w->h_stage;
  for (int i = 0; i < k; i++)
    if (parts[i].src && parts[i].bytes) {
      memcpy(h + parts[i].off, parts[i].src, parts[i].bytes);
      memset(h + parts[i].off + parts[i].bytes, 0, parts[i].slack);
    }
  if (tot) HIP_TRY(hipMemcpyAsync(w->d_stage.p, h, tot, hipMemcpyHostToDevice, st));
  *d_base = w->d_stage.as<uint8_t>();
  return DH_OK;
}

// the small-batch path behind the host-memory entry points (dh_verify_batch, dh_verify_recovered_batch): chained
// lengths were checked by the caller (dh_verify_batch)
static int verify_small_host(int scheme, const uint8_t* pk, size_t pk_len, const uint64_t* rounds, const uint8_t* sigs,
                             size_t sig_stride, const uint8_t* prevs, size_t prev_stride, const uint32_t* prev_lens,
                             const uint8_t* msgs32, size_t n, uint8_t* verdict_out, uint8_t* rand_out) {
  lease L;
  if (L.rc) return L.rc;
  worker* w = L.w;
  int rc = set_device_and_stream(w);
  if (rc) return rc;
  hipStream_t st = w->stream;
  stage_part parts[5] = {{rounds, rounds ? n * 8 : 0},
                         {sigs, n * sig_stride},
                         {prevs, prevs ? n * prev_stride : 0, 4},
                         {prev_lens, prevs && prev_lens ? n * 4 : 0},
                         {msgs32, msgs32 ? n * 32 : 0}};
  const size_t vbytes = (n + 15) & ~(size_t)15;
  uint8_t* d = nullptr;
  size_t out_off = 0;
  rc = stage_in(w, parts, 5, vbytes + (rand_out ? n * 32 : 0), st, &d, &out_off);
  if (rc) return rc;
  uint8_t* d_verdict = d + out_off;
  uint8_t* d_rand = rand_out ? d + out_off + vbytes : nullptr;
  rc = verify_small(w, scheme, pk, pk_len, rounds ? (const uint64_t*)(d + parts[0].off) : nullptr, d + parts[1].off, sig_stride,
                    prevs ? d + parts[2].off : nullptr, prev_stride, prevs && prev_lens ? (const uint32_t*)(d + parts[3].off) : nullptr,
                    n, d_verdict, d_rand, msgs32 ? d + parts[4].off : nullptr, st, true);
  if (rc) {
    (void)hipStreamSynchronize(st);
    if (w->tail) (void)hipStreamSynchronize(w->tail);
    return rc;
  }
  uint8_t* h_out = (uint8_t*)w->h_stage + out_off;
  HIP_TRY(hipMemcpyAsync(h_out, d_verdict, vbytes + (rand_out ? n * 32 : 0), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  memcpy(verdict_out, h_out, n);
  if (rand_out) memcpy(rand_out, h_out + vbytes, n * 32);
  return DH_OK;
}

int recover_core(worker* w, int scheme, const uint8_t* commits, int t, int n_nodes, const uint8_t* msgs32,
                 const uint8_t* partials, const uint32_t* part_off, size_t n_rounds, uint8_t* sig_out, uint8_t* status_out,
                 hipStream_t st, uint8_t* partial_ok_out = nullptr) {
  const bool g2 = sig_on_g2(scheme);
  const int sl = g2 ? 96 : 48, kl = g2 ? 48 : 96;
  const size_t jw = g2 ? JAC_WORDS_G2 : JAC_WORDS_G1, aw = jw * 2 / 3;
  const size_t kjw = g2 ? JAC_WORDS_G1 : JAC_WORDS_G2, kaw = kjw * 2 / 3;
  const size_t np = part_off[n_rounds] - part_off[0];
  const uint32_t base = part_off[0];
  memset(status_out, 0, n_rounds);
  if (n_rounds == 0) return DH_OK;
  timed_launches T(st);
  // 1./2. commits -> affine key-group points (all must decode) -> the public shares PubPoly.Eval(i), i < n_nodes.
  // Cached per worker under (scheme, t, n_nodes, commits): a node recovers every round against one group's
  // polynomial, and the evaluation is a ~6 ms latency-bound kernel (one lane per signer, 33-term Horner).
  std::vector<uint8_t> pub_key(9 + (size_t)t * kl);
  pub_key[0] = (uint8_t)scheme;
  memcpy(&pub_key[1], &t, 4);
  memcpy(&pub_key[5], &n_nodes, 4);
  memcpy(&pub_key[9], commits, (size_t)t * kl);
  const bool pub_hit = w->r_pub_key == pub_key;
  std::vector<uint8_t> cst(t, 1);
  if (!pub_hit) {
    w->r_pub_key.clear();
    HIP_TRY(w->r_commits.ensure((size_t)t * kl));
    HIP_TRY(w->r_cstatus.ensure(t));
    HIP_TRY(w->r_caff.ensure((size_t)t * kaw * 4));
    HIP_TRY(hipMemcpyAsync(w->r_commits.p, commits, (size_t)t * kl, hipMemcpyHostToDevice, st));
    HIP_TRY(dh::launch_prep(g2 ? 0 : 1, w->r_commits.as<uint8_t>(), kl, t, w->r_cstatus.as<uint8_t>(),
                            w->r_caff.as<uint32_t>(), nullptr, st));
    HIP_TRY(hipMemcpyAsync(cst.data(), w->r_cstatus.p, t, hipMemcpyDeviceToHost, st));
    HIP_TRY(w->r_shares.ensure((size_t)n_nodes * kjw * 4));
    HIP_TRY(T.run("k_pubpoly_eval", [&] {
      return dh::launch_pubpoly_eval(g2 ? 0 : 1, w->r_caff.as<uint32_t>(), t, n_nodes, w->r_shares.as<uint32_t>(), st);
    }));
  }
  // 3./4. partials: repack, decode + subgroup check
  HIP_TRY(w->r_raw.ensure(np * (2 + sl) + 4));
  HIP_TRY(w->r_psigs.ensure(np * sl + 4));
  HIP_TRY(w->r_pidx.ensure(np * 4 + 4));
  HIP_TRY(w->r_pstatus.ensure(np + 4));
  HIP_TRY(w->r_paff.ensure(np * aw * 4 + 16));
  // The partial records (98 B each for G2: 323 MB at 3.3M partials) come from pageable host memory. They cross in
  // chunks on the worker's tail stream, each chunk's repack + decode queued behind its copy on st, so the copy of
  // chunk c + 1 overlaps the decoding of chunk c instead of preceding all of it.
  const size_t pchunk = (w->tail && st == w->stream && np > ((size_t)1 << 19)) ? ((size_t)1 << 19) : np;
  for (size_t c0 = 0; c0 < np; c0 += pchunk) {
    const size_t cn = std::min(pchunk, np - c0);
    hipStream_t cs = pchunk < np ? w->tail : st;
    HIP_TRY(hipMemcpyAsync(w->r_raw.as<uint8_t>() + c0 * (2 + sl), partials + (size_t)(base + c0) * (2 + sl), cn * (2 + sl),
                           hipMemcpyHostToDevice, cs));
    if (cs != st) {
      HIP_TRY(hipEventRecord(w->handoff, cs));
      HIP_TRY(hipStreamWaitEvent(st, w->handoff, 0));
    }
    HIP_TRY(dh::launch_repack_partials(w->r_raw.as<uint8_t>() + c0 * (2 + sl), cn, sl, w->r_psigs.as<uint8_t>() + c0 * sl,
                                       w->r_pidx.as<uint32_t>() + c0, st));
    HIP_TRY(T.run(g2 ? "k_prep_sig<fp2>(partials)" : "k_prep_sig<fp>(partials)", [&] {
      return dh::launch_prep(g2, w->r_psigs.as<uint8_t>() + c0 * sl, sl, cn, w->r_pstatus.as<uint8_t>() + c0,
                             w->r_paff.as<uint32_t>() + c0 * aw, nullptr, st);
    }));
  }
  // 5. hash points of the round messages
  HIP_TRY(w->r_msgs.ensure(n_rounds * 32));
  HIP_TRY(w->r_q.ensure(n_rounds * jw * 4));
  HIP_TRY(hipMemcpyAsync(w->r_msgs.p, msgs32, n_rounds * 32, hipMemcpyHostToDevice, st));
  HIP_TRY(w->h2c_tmp.ensure(dh::hash_tmp_bytes(g2, n_rounds)));
  HIP_TRY(T.run(g2 ? "k_prep_msg32<fp2>" : "k_prep_msg32<fp>", [&] {
    return dh::launch_hash(g2, nullptr, nullptr, 0, nullptr, w->r_msgs.as<uint8_t>(), n_rounds, 0, dst_id(scheme), nullptr,
                           w->r_q.as<uint32_t>(), w->h2c_tmp.as<uint32_t>(), st);
  }));
  // 6. per-partial round and the group-membership rule, on the device (offsets relative to the first partial)
  std::vector<uint32_t> off_rel(n_rounds + 1);
  for (size_t j = 0; j <= n_rounds; j++) off_rel[j] = part_off[j] - base;
  HIP_TRY(w->r_off.ensure((n_rounds + 1) * 4));
  HIP_TRY(w->r_round_of.ensure(np * 4 + 4));
  HIP_TRY(hipMemcpyAsync(w->r_off.p, off_rel.data(), (n_rounds + 1) * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(dh::launch_partial_meta(w->r_off.as<uint32_t>(), n_rounds, w->r_pidx.as<uint32_t>(), n_nodes,
                                  w->r_round_of.as<uint32_t>(), w->r_pstatus.as<uint8_t>(), st));
  // 7. RLC scalars per partial (0 for partials that failed decoding or lie outside the group), split as the 28-bit MSM
  // takes them: four 31-bit psi parts (G2 signatures) or two 63-bit phi halves (G1)
  const int parts = g2 ? 4 : 2;
  const size_t pw28 = g2 ? 64 : 32, wsw = g2 ? 96 : 48;  // words per 28-bit affine point / workspace Jacobian point
  uint32_t seedw[8];
  int rc = make_seed(0, seedw);
  if (rc) return rc;
  HIP_TRY(w->key_ok.ensure(64));
  uint32_t* d_seed = (uint32_t*)((uint8_t*)w->key_ok.p + 32);
  HIP_TRY(hipMemcpyAsync(d_seed, seedw, 32, hipMemcpyHostToDevice, st));
  HIP_TRY(w->r_scal.ensure(std::max(np, n_rounds) * 16 + 16));
  HIP_TRY(dh::launch_scalars(d_seed, np, w->r_pstatus.as<uint8_t>(), w->r_scal.as<uint4>(), parts, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int c = 0; c < t; c++)
    if (cst[c] != 1) return fail(DH_EKEY, "public polynomial commitment %d does not decode to a subgroup point", c);
  if (!pub_hit) w->r_pub_key = pub_key;  // r_caff / r_shares hold this polynomial until a call with another one
  // 8./9. MSMs: A = sum r sigma (one group), B_i = sum r Q_round per signer i: entry e -> point round_of[e], scalar e,
  // group min(share, n-1) (the sort keys by (group, window, digit), so the entries need no order; a zero scalar
  // contributes nothing)
  HIP_TRY(w->r_ok.ensure(np + 4));
  bool batch_ok = false;
  {
    HIP_TRY(w->entries.ensure(np * 4 + 4));
    HIP_TRY(dh::launch_iota(w->entries.as<uint32_t>(), np, st));
    HIP_TRY(w->r_e_grp.ensure(np * 4 + 4));
    HIP_TRY(dh::launch_clamp_group(w->r_pidx.as<uint32_t>(), np, (uint32_t)n_nodes - 1, w->r_e_grp.as<uint32_t>(), st));
    // the partials' sigmas and the rounds' hash points in the 28-bit form with their endomorphism images (a hash point
    // at infinity, probability ~2^-255, leaves its round's slot unwritten: the batch check then fails and the partials
    // get their leaf checks on the 32-bit points)
    HIP_TRY(w->s28.ensure(parts * std::max<size_t>(np, 1) * pw28 * 4));
    HIP_TRY(w->q28.ensure(parts * n_rounds * pw28 * 4));
    HIP_TRY(w->r_rstat.ensure(n_rounds));
    HIP_TRY(hipMemsetAsync(w->r_rstat.p, 1 /* DEC_OK */, n_rounds, st));
    HIP_TRY(dh::launch_msm_prep28(g2, np, w->r_pstatus.as<uint8_t>(), w->r_paff.as<uint32_t>(), nullptr, w->s28.as<uint32_t>(),
                                  nullptr, st, 1));
    HIP_TRY(dh::launch_msm_prep28(g2, n_rounds, w->r_rstat.as<uint8_t>(), nullptr, w->r_q.as<uint32_t>(), nullptr,
                                  w->q28.as<uint32_t>(), st, 2));
    dh::msm_geom gA = geom_for(std::max<size_t>(np, 1), parts);
    gA.half_stride = (uint32_t)np;
    // window geometry of the per-signer groups from the partials per signer that answered, the signers counted over
    // the first 65,536 records (np / n_nodes undercounted a group when the same t signers answer every round, and picked
    // 3 windows of c = 15 where 2 of c = 16 do a third fewer bucket additions: 43.1 -> 38.7 ms at n = 64, t = 33; with
    // every signer answering, np / t overcounted and c = 16 was slower, 39.4 -> 52.0 ms, profiles/r04/config_recover_*_r04p)
    size_t active = 0;
    {
      std::vector<uint8_t> seen((size_t)n_nodes, 0);
      const size_t ns = std::min<size_t>(np, 65536);
      for (size_t e = 0; e < ns; e++) {
        const uint8_t* r = partials + (size_t)(base + e) * (2 + sl);
        const size_t i = ((size_t)r[0] << 8) | r[1];
        if (i < (size_t)n_nodes && !seen[i]) {
          seen[i] = 1;
          active++;
        }
      }
    }
    size_t avg = std::max<size_t>(1, np / std::max<size_t>(1, active));
    dh::msm_geom gB = geom_for(avg, parts);
    while (gB.c > 3 && (size_t)n_nodes * gB.nwin * gB.nbuck > ((size_t)1 << 24))
      gB = geom_for(std::max<size_t>(1, ((size_t)1 << (gB.c + 1)) / parts), parts);
    gB.half_stride = (uint32_t)n_rounds;
    // one workspace for both (sized for each before anything is queued on it), used one MSM after the other
    dh::msm_ws wsA{}, wsB{};
    int rcw = msm_workspace(w, gA, np, 1, wsw, wsA);
    if (!rcw) rcw = msm_workspace(w, gB, np, n_nodes, wsw, wsB);
    if (!rcw) rcw = msm_workspace(w, gA, np, 1, wsw, wsA);
    if (rcw) return rcw;
    HIP_TRY(w->outA.ensure(jw * 4));
    HIP_TRY(w->outB.ensure((size_t)n_nodes * jw * 4));
    HIP_TRY(T.run("recover_msm_sigs", [&] {
      return dh::launch_msm28_set(g2, gA, w->entries.as<uint32_t>(), nullptr, nullptr, np, 1, w->r_scal.as<uint4>(),
                                  w->s28.as<uint32_t>(), wsA, w->outA.as<uint32_t>(), st);
    }));
    HIP_TRY(T.run("recover_msm_hash_by_signer", [&] {
      return dh::launch_msm28_set(g2, gB, w->r_round_of.as<uint32_t>(), w->entries.as<uint32_t>(), w->r_e_grp.as<uint32_t>(),
                                  np, n_nodes, w->r_scal.as<uint4>(), w->q28.as<uint32_t>(), wsB, w->outB.as<uint32_t>(), st);
    }));
    // 10. multi-pairing: n_nodes + 1 pairs
    const size_t npairs = (size_t)n_nodes + 1;
    HIP_TRY(w->r_P.ensure(npairs * JAC_WORDS_G1 * 4));
    HIP_TRY(w->r_Q.ensure(npairs * JAC_WORDS_G2 * 4));
    HIP_TRY(w->r_f.ensure(npairs * 192 * 4));  // k_vm.hip F12_WORDS (the one-lane path uses 144)
    HIP_TRY(w->r_skip.ensure(npairs + 4));
    HIP_TRY(w->pass.ensure(16));
    HIP_TRY(T.run("recover_pair_check", [&] {
      hipError_t e = dh::launch_recover_pairs(g2, w->r_shares.as<uint32_t>(), w->outB.as<uint32_t>(), w->outA.as<uint32_t>(),
                                              n_nodes, w->r_P.as<uint32_t>(), w->r_Q.as<uint32_t>(), st);
      if (e != hipSuccess) return e;
      if (lane_pairing())
        return dh::launch_pair_check(w->r_P.as<uint32_t>(), w->r_Q.as<uint32_t>(), npairs, 0, 0, nullptr,
                                     w->r_f.as<uint32_t>(), w->r_skip.as<uint8_t>(), w->pass.as<uint8_t>(), st);
      if ((e = w->vm_pairs.ensure(npairs * 72 * 4)) != hipSuccess) return e;
      if ((e = w->vm_live.ensure(npairs)) != hipSuccess) return e;
      return dh::launch_multi_pairing_vm(w->r_P.as<uint32_t>(), w->r_Q.as<uint32_t>(), npairs, w->vm_pairs.as<uint32_t>(),
                                         w->vm_live.as<uint8_t>(), w->r_f.as<uint32_t>(), w->pass.as<uint8_t>(), st);
    }));
    uint8_t pass = 0;
    HIP_TRY(hipMemcpyAsync(&pass, w->pass.p, 1, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    batch_ok = pass == 1;
  }
  // 11. per-partial validity, on the device
  if (batch_ok) {
    HIP_TRY(dh::launch_ok_from_status(w->r_pstatus.as<uint8_t>(), np, w->r_ok.as<uint8_t>(), st));
  } else {
    HIP_TRY(T.run("k_partial_leaf", [&] {
      return dh::launch_partial_leaf(g2, w->entries.as<uint32_t>(), np, w->r_paff.as<uint32_t>(), w->r_pstatus.as<uint8_t>(),
                                     w->r_pidx.as<uint32_t>(), w->r_round_of.as<uint32_t>(), w->r_q.as<uint32_t>(),
                                     w->r_shares.as<uint32_t>(), n_nodes, w->r_ok.as<uint8_t>(), st);
    }));
  }
  if (partial_ok_out) {  // dh_verify_partials_batch: per-partial VerifyPartial verdicts only
    HIP_TRY(hipMemcpyAsync(partial_ok_out, w->r_ok.p, np, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
  }
  // 12. selection (first t valid in the given order; sorted by index; duplicates dropped) + Lagrange coefficients,
  // one lane per round
  HIP_TRY(w->r_sel.ensure(n_rounds * (size_t)t * 4));
  HIP_TRY(w->r_key.ensure(n_rounds * (size_t)t * 4));
  HIP_TRY(w->r_den.ensure(n_rounds * (size_t)t * 32));
  HIP_TRY(w->r_lam.ensure(n_rounds * (size_t)t * dh::lam_words() * 4));
  HIP_TRY(w->r_rok.ensure(n_rounds));
  HIP_TRY(w->r_lamset.ensure(n_rounds * 4));
  HIP_TRY(w->r_own.ensure(4));
  HIP_TRY(w->r_sig.ensure(n_rounds * jw * 4));
  HIP_TRY(T.run("k_select_lagrange", [&] {
    return dh::launch_select_lagrange(w->r_off.as<uint32_t>(), w->r_ok.as<uint8_t>(), w->r_pidx.as<uint32_t>(), t, n_rounds,
                                      w->r_sel.as<uint32_t>(), w->r_key.as<uint32_t>(), w->r_den.as<uint32_t>(),
                                      w->r_lam.as<uint32_t>(), w->r_lamset.as<uint32_t>(), w->r_rok.as<uint8_t>(),
                                      w->r_own.as<uint32_t>(), g2 ? 0 : 1, st);
  }));
  // tables of 8 odd multiples when some round has a Lagrange basis of its own (its wave then runs the regular windows
  // in k_lagrange), else of 4 for the width-4 NAF: one word back from the device. k_lagrange depends on this: k_lambda
  // writes width-4 NAF nibbles for round 0's basis only, so entries == 4 is valid only when every round uses basis 0
  // (own == 0); k_lagrange leaves a wave at infinity (not recovered) if that ever fails to hold
  int entries = 4;
  if (g2) {
    uint32_t own = 0;
    HIP_TRY(hipMemcpyAsync(&own, w->r_own.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (own) entries = 8;
  }
  // 13. interpolation on the device
  if (g2) {  // the selected partials' points in the 28-bit form and their tables of odd multiples, once per partial
    HIP_TRY(w->r_zs.ensure(dh::wnaf_table_scratch_bytes(np, entries) + 256));
    HIP_TRY(w->r_tbl.ensure(np * (size_t)entries * 64 * 4 + 1024));
    HIP_TRY(w->r_need.ensure(np + 4));
    HIP_TRY(dh::launch_mark_selected(w->r_sel.as<uint32_t>(), w->r_rok.as<uint8_t>(), t, n_rounds, np, w->r_need.as<uint8_t>(),
                                     st));
    HIP_TRY(T.run("k_wnaf_table", [&] {
      return dh::launch_wnaf_table_g2(w->r_paff.as<uint32_t>(), w->r_need.as<uint8_t>(), np, entries, w->r_tbl.as<uint32_t>(),
                                      w->r_zs.as<uint32_t>(), st);
    }));
  }
  HIP_TRY(w->r_ltmp.ensure(dh::lagrange_tmp_bytes(g2)));
  HIP_TRY(T.run("k_lagrange", [&] {
    return dh::launch_lagrange(g2, w->r_sel.as<uint32_t>(), w->r_lam.as<uint32_t>(), w->r_lamset.as<uint32_t>(),
                               w->r_rok.as<uint8_t>(), t,
                               n_rounds, w->r_paff.as<uint32_t>(), g2 ? w->r_tbl.as<uint32_t>() : nullptr, entries,
                               w->r_sig.as<uint32_t>(), w->r_ltmp.as<uint32_t>(), st);
  }));
  std::vector<uint8_t> rok(n_rounds, 0);
  HIP_TRY(hipMemcpyAsync(rok.data(), w->r_rok.p, n_rounds, hipMemcpyDeviceToHost, st));
  // 14./15. compress, then VerifyRecovered (chainstore.go:207) as one batch against the group key (commit 0)
  HIP_TRY(w->r_sigbytes.ensure(n_rounds * sl));
  HIP_TRY(w->r_status2.ensure(n_rounds));
  HIP_TRY(w->r_aff2.ensure(n_rounds * aw * 4));
  // the compression also leaves the affine points and decode statuses the VerifyRecovered batch takes (decoding the
  // bytes again — an Fp(2) square root and a subgroup test per round — would return the same points)
  HIP_TRY(dh::launch_compress(g2, w->r_sig.as<uint32_t>(), n_rounds, w->r_sigbytes.as<uint8_t>(), w->r_aff2.as<uint32_t>(),
                              w->r_status2.as<uint8_t>(), st));
  HIP_TRY(hipMemcpyAsync(sig_out, w->r_sigbytes.p, n_rounds * sl, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  // verify through the regular batch path (messages are given digests: use the per-round hash points)
  std::vector<uint8_t> vv(n_rounds, 0);
  {
    HIP_TRY(w->r_entries2.ensure(n_rounds * 4));
    HIP_TRY(w->r_scal.ensure(std::max(np, n_rounds) * 16 + 16));  // rounds may outnumber the partials
    HIP_TRY(dh::launch_scalars(d_seed, n_rounds, w->r_status2.as<uint8_t>(), w->r_scal.as<uint4>(), parts, st));
    HIP_TRY(dh::launch_iota(w->r_entries2.as<uint32_t>(), n_rounds, st));
    // group key = commit 0 (affine, key group) — staged where the group check expects it
    HIP_TRY(w->key_aff.ensure(96 * 4));
    HIP_TRY(hipMemcpyAsync(w->key_aff.p, w->r_caff.p, kaw * 4, hipMemcpyDeviceToDevice, st));
    dh::msm_geom g = geom_for(n_rounds, parts);
    g.half_stride = (uint32_t)n_rounds;
    dh::msm_ws ws{};
    int rcw = msm_workspace(w, g, n_rounds, 1, wsw, ws);
    if (rcw) return rcw;
    HIP_TRY(w->s28.ensure(parts * n_rounds * pw28 * 4));
    HIP_TRY(w->q28.ensure(parts * n_rounds * pw28 * 4));
    HIP_TRY(dh::launch_msm_prep28(g2, n_rounds, w->r_status2.as<uint8_t>(), w->r_aff2.as<uint32_t>(), w->r_q.as<uint32_t>(),
                                  w->s28.as<uint32_t>(), w->q28.as<uint32_t>(), st));
    HIP_TRY(T.run("recover_verify", [&] {
      hipError_t e = dh::launch_msm28(g2, g, w->r_entries2.as<uint32_t>(), n_rounds, 1, w->r_scal.as<uint4>(),
                                      w->s28.as<uint32_t>(), w->q28.as<uint32_t>(), ws, w->outA.as<uint32_t>(),
                                      w->outB.as<uint32_t>(), st, w->r_status2.as<uint8_t>(), false);
      if (e != hipSuccess) return e;
      return group_check(w, g2, w->outA.as<uint32_t>(), w->outB.as<uint32_t>(), 1, w->key_aff.as<uint32_t>(),
                         w->pass.as<uint8_t>(), st);
    }));
    uint8_t pass = 0, dummy = 0;
    (void)dummy;
    HIP_TRY(hipMemcpyAsync(&pass, w->pass.p, 1, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(w->r_ok.ensure(std::max(np, n_rounds) + 4));
    if (pass == 1) {
      HIP_TRY(hipMemcpyAsync(vv.data(), w->r_status2.p, n_rounds, hipMemcpyDeviceToHost, st));
    } else {
      HIP_TRY(hipMemsetAsync(w->r_ok.p, 0, n_rounds, st));
      HIP_TRY(leaf_check(w, g2, w->r_entries2.as<uint32_t>(), n_rounds, w->r_aff2.as<uint32_t>(), w->r_q.as<uint32_t>(),
                         w->key_aff.as<uint32_t>(), w->r_status2.as<uint8_t>(), w->r_ok.as<uint8_t>(), st));
      HIP_TRY(hipMemcpyAsync(vv.data(), w->r_ok.p, n_rounds, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
  }
  for (size_t j = 0; j < n_rounds; j++) status_out[j] = (rok[j] && vv[j] == 1) ? 1 : 0;
  return DH_OK;
}

// ---- sign.Scheme.Verify in batch under keys the caller passes (dh_bls_verify_batch: the schemes' AuthScheme,
// crypto/schemes.go:102,143,183, and the identity self-signatures of key/keys.go:61-64). recover_core's batched
// VerifyPartial with a key table in place of the public polynomial's shares, one hash point per item and messages of
// any length. Three levels, verdicts exact at each:
//   1  A = sum r_i sigma_i, B_k = sum over the items of key k of r_i Q_i, one (n_keys + 1)-pair product check
//   2  (level 1 failed, more than one key in use) A_k per key, one 2-pair check per key: the failing keys
//   3  leaf checks of the items under failing keys; the items of passing keys are valid when they decoded
// Leaf checks only (no scalars, no MSM) for n <= small_batch_max() or fewer than auth_rlc_min_per_key() items per key
// in use. DRANDHIP_AUTH_PATH=leaf|rlc forces either path; it is read at every call.
// T = 2 items per key, measured at n = 4096 (profiles/r07/auth_measure.json): leaf checks 50.7 ms (quicknet) / 54.2 ms
// (pedersen-bls-unchained) whatever the keys; rlc 12.4 / 20.9 ms under one key, 29.8 / 37.7 ms at 2 items per key,
// 48.6 / 55.5 ms at one item per key (the product's n_keys + 1 Miller loops), where it no longer wins for both.
static size_t auth_rlc_min_per_key() { return 2; }

enum { AUTH_AUTO = 0, AUTH_LEAF, AUTH_RLC };
static int auth_path_env() {
  const char* e = getenv("DRANDHIP_AUTH_PATH");
  if (e && !strcmp(e, "leaf")) return AUTH_LEAF;
  if (e && !strcmp(e, "rlc")) return AUTH_RLC;
  return AUTH_AUTO;
}

// kidx: n key indices < n_keys (host); keys_used: distinct values among them; off: n + 1 message offsets from 0 (host)
int auth_core(worker* w, int scheme, const uint8_t* keys, size_t n_keys, const uint32_t* kidx, size_t keys_used,
              const uint8_t* msgs, const uint32_t* off, const uint8_t* sigs, size_t sig_stride, size_t n, uint8_t* verdict_out,
              uint8_t* key_ok_out, uint64_t seed, uint64_t stats[4], hipStream_t st) {
  const bool g2 = sig_on_g2(scheme);
  const int sl = g2 ? 96 : 48, kl = g2 ? 48 : 96;
  const size_t jw = g2 ? JAC_WORDS_G2 : JAC_WORDS_G1, aw = jw * 2 / 3;
  const size_t kjw = g2 ? JAC_WORDS_G1 : JAC_WORDS_G2, kaw = kjw * 2 / 3;
  const size_t total = off[n], nmax = std::max(n, n_keys);
  timed_launches T(st);
  // 1. the key table: decode + subgroup test, one lane per key (the signature kernels of the key group), then the
  // per-key layout of the pair and leaf kernels
  HIP_TRY(w->a_keys.ensure(n_keys * kl + 4));
  HIP_TRY(w->a_kstatus.ensure(n_keys + 4));
  HIP_TRY(w->a_kaff.ensure(n_keys * kaw * 4 + 16));
  HIP_TRY(w->a_shares.ensure(n_keys * kjw * 4));
  HIP_TRY(hipMemcpyAsync(w->a_keys.p, keys, n_keys * kl, hipMemcpyHostToDevice, st));
  HIP_TRY(T.run(g2 ? "k_prep_sig<fp>(keys)" : "k_prep_sig<fp2>(keys)", [&] {
    return dh::launch_prep(g2 ? 0 : 1, w->a_keys.as<uint8_t>(), kl, n_keys, w->a_kstatus.as<uint8_t>(), w->a_kaff.as<uint32_t>(),
                           nullptr, st);
  }));
  HIP_TRY(dh::launch_key_shares(g2 ? 0 : 1, w->a_kaff.as<uint32_t>(), w->a_kstatus.as<uint8_t>(), n_keys,
                                w->a_shares.as<uint32_t>(), st));
  // 2. signatures: decode + subgroup test; an item under a bad key is rejected with them
  HIP_TRY(w->r_raw.ensure(n * sig_stride + 4));
  HIP_TRY(w->r_pstatus.ensure(n + 4));
  HIP_TRY(w->r_paff.ensure(n * aw * 4 + 16));
  HIP_TRY(w->a_kidx.ensure(n * 4 + 4));
  HIP_TRY(hipMemcpyAsync(w->r_raw.p, sigs, n * sig_stride, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w->a_kidx.p, kidx, n * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(T.run(g2 ? "k_prep_sig<fp2>(auth)" : "k_prep_sig<fp>(auth)", [&] {
    return dh::launch_prep(g2, w->r_raw.as<uint8_t>(), sig_stride, n, w->r_pstatus.as<uint8_t>(), w->r_paff.as<uint32_t>(),
                           nullptr, st);
  }));
  HIP_TRY(dh::launch_mark_bad_key(w->a_kidx.as<uint32_t>(), n, w->a_kstatus.as<uint8_t>(), w->r_pstatus.as<uint8_t>(), st));
  // 3. hash points: the fixed-shape kernels when every message is 32 bytes (identity hashes, beacon digests), else the
  // variable-length form
  bool all32 = true;
  for (size_t i = 0; i < n && all32; i++) all32 = off[i + 1] - off[i] == 32;
  HIP_TRY(w->r_msgs.ensure(total + 4));
  HIP_TRY(w->r_q.ensure(n * jw * 4));
  HIP_TRY(w->h2c_tmp.ensure(dh::hash_tmp_bytes(g2, n)));
  if (total) HIP_TRY(hipMemcpyAsync(w->r_msgs.p, msgs, total, hipMemcpyHostToDevice, st));
  if (all32) {
    HIP_TRY(T.run(g2 ? "k_prep_msg32<fp2>" : "k_prep_msg32<fp>", [&] {
      return dh::launch_hash(g2, nullptr, nullptr, 0, nullptr, w->r_msgs.as<uint8_t>(), n, 0, dst_id(scheme), nullptr,
                             w->r_q.as<uint32_t>(), w->h2c_tmp.as<uint32_t>(), st);
    }));
  } else {
    HIP_TRY(w->a_moff.ensure((n + 1) * 4));
    HIP_TRY(hipMemcpyAsync(w->a_moff.p, off, (n + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(T.run(g2 ? "k_prep_msgv<fp2>" : "k_prep_msgv<fp>", [&] {
      return dh::launch_hash_var(g2, w->r_msgs.as<uint8_t>(), w->a_moff.as<uint32_t>(), n, dst_id(scheme), w->r_q.as<uint32_t>(),
                                 w->h2c_tmp.as<uint32_t>(), st);
    }));
  }
  // item i is entry i, its own hash point i, under key kidx[i]
  HIP_TRY(w->entries.ensure(nmax * 4 + 4));
  HIP_TRY(dh::launch_iota(w->entries.as<uint32_t>(), nmax, st));
  HIP_TRY(w->r_ok.ensure(n + 4));
  const uint32_t* iota = w->entries.as<uint32_t>();
  auto leaves = [&](const uint32_t* list, size_t m) {
    return T.run("k_partial_leaf(auth)", [&] {
      return dh::launch_partial_leaf(g2, list, m, w->r_paff.as<uint32_t>(), w->r_pstatus.as<uint8_t>(), w->a_kidx.as<uint32_t>(),
                                     iota, w->r_q.as<uint32_t>(), w->a_shares.as<uint32_t>(), (int)n_keys, w->r_ok.as<uint8_t>(), st);
    });
  };
  uint64_t levels = 0, keys_failed = 0, leaf_items = 0;
  const int forced = auth_path_env();
  const bool leaf_only =
      forced == AUTH_LEAF || (forced == AUTH_AUTO && (n <= small_batch_max() || n < auth_rlc_min_per_key() * keys_used));
  if (leaf_only) {
    HIP_TRY(leaves(iota, n));
    leaf_items = n;
  } else {
    // level 1: RLC scalars (0 for rejected items), the two MSMs, the product check
    const int parts = g2 ? 4 : 2;
    const size_t pw28 = g2 ? 64 : 32, wsw = g2 ? 96 : 48;
    uint32_t seedw[8];
    int rc = make_seed(seed, seedw);
    if (rc) return rc;
    HIP_TRY(w->key_ok.ensure(64));
    uint32_t* d_seed = (uint32_t*)((uint8_t*)w->key_ok.p + 32);
    HIP_TRY(hipMemcpyAsync(d_seed, seedw, 32, hipMemcpyHostToDevice, st));
    HIP_TRY(w->r_scal.ensure(n * 16 + 16));
    HIP_TRY(dh::launch_scalars(d_seed, n, w->r_pstatus.as<uint8_t>(), w->r_scal.as<uint4>(), parts, st));
    HIP_TRY(w->s28.ensure(parts * n * pw28 * 4));
    HIP_TRY(w->q28.ensure(parts * n * pw28 * 4));
    HIP_TRY(w->r_rstat.ensure(n));
    HIP_TRY(hipMemsetAsync(w->r_rstat.p, 1 /* DEC_OK */, n, st));
    HIP_TRY(dh::launch_msm_prep28(g2, n, w->r_pstatus.as<uint8_t>(), w->r_paff.as<uint32_t>(), nullptr, w->s28.as<uint32_t>(),
                                  nullptr, st, 1));
    HIP_TRY(dh::launch_msm_prep28(g2, n, w->r_rstat.as<uint8_t>(), nullptr, w->r_q.as<uint32_t>(), nullptr, w->q28.as<uint32_t>(),
                                  st, 2));
    dh::msm_geom gA = geom_for(n, parts);
    gA.half_stride = (uint32_t)n;
    dh::msm_geom gB = geom_for(std::max<size_t>(1, n / keys_used), parts);  // window geometry from the items per key in use
    while (gB.c > 3 && n_keys * gB.nwin * gB.nbuck > ((size_t)1 << 24))
      gB = geom_for(std::max<size_t>(1, ((size_t)1 << (gB.c + 1)) / parts), parts);
    gB.half_stride = (uint32_t)n;
    // one workspace for both (sized for each before anything is queued on it), used one MSM after the other
    dh::msm_ws wsA{}, wsB{};
    int rcw = msm_workspace(w, gA, n, 1, wsw, wsA);
    if (!rcw) rcw = msm_workspace(w, gB, n, n_keys, wsw, wsB);
    if (!rcw) rcw = msm_workspace(w, gA, n, 1, wsw, wsA);
    if (rcw) return rcw;
    HIP_TRY(T.run("auth_msm_sigs", [&] {
      return dh::launch_msm28_set(g2, gA, iota, nullptr, nullptr, n, 1, w->r_scal.as<uint4>(), w->s28.as<uint32_t>(), wsA,
                                  w->outA.as<uint32_t>(), st);
    }));
    HIP_TRY(T.run("auth_msm_hash_by_key", [&] {
      return dh::launch_msm28_set(g2, gB, iota, nullptr, w->a_kidx.as<uint32_t>(), n, n_keys, w->r_scal.as<uint4>(),
                                  w->q28.as<uint32_t>(), wsB, w->outB.as<uint32_t>(), st);
    }));
    const size_t npairs = n_keys + 1;
    HIP_TRY(w->r_P.ensure(npairs * JAC_WORDS_G1 * 4));
    HIP_TRY(w->r_Q.ensure(npairs * JAC_WORDS_G2 * 4));
    HIP_TRY(w->r_f.ensure(npairs * 192 * 4));
    HIP_TRY(w->r_skip.ensure(npairs + 4));
    HIP_TRY(w->pass.ensure(16));
    HIP_TRY(T.run("auth_pair_check", [&] {
      hipError_t e = dh::launch_recover_pairs(g2, w->a_shares.as<uint32_t>(), w->outB.as<uint32_t>(), w->outA.as<uint32_t>(),
                                              (int)n_keys, w->r_P.as<uint32_t>(), w->r_Q.as<uint32_t>(), st);
      if (e != hipSuccess) return e;
      if (lane_pairing())
        return dh::launch_pair_check(w->r_P.as<uint32_t>(), w->r_Q.as<uint32_t>(), npairs, 0, 0, nullptr, w->r_f.as<uint32_t>(),
                                     w->r_skip.as<uint8_t>(), w->pass.as<uint8_t>(), st);
      if ((e = w->vm_pairs.ensure(npairs * 72 * 4)) != hipSuccess) return e;
      if ((e = w->vm_live.ensure(npairs)) != hipSuccess) return e;
      return dh::launch_multi_pairing_vm(w->r_P.as<uint32_t>(), w->r_Q.as<uint32_t>(), npairs, w->vm_pairs.as<uint32_t>(),
                                         w->vm_live.as<uint8_t>(), w->r_f.as<uint32_t>(), w->pass.as<uint8_t>(), st);
    }));
    uint8_t pass = 0;
    HIP_TRY(hipMemcpyAsync(&pass, w->pass.p, 1, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    levels = 1;
    // every item that decoded is valid when its key's check passed; the leaves below overwrite the others
    HIP_TRY(dh::launch_ok_from_status(w->r_pstatus.as<uint8_t>(), n, w->r_ok.as<uint8_t>(), st));
    if (pass != 1) {
      std::vector<uint8_t> failing(n_keys, 1);
      if (keys_used > 1) {
        // level 2: A_k = the signature sum of key k's items (the hash MSM's grouping and geometry), then the check
        // e(pk_k, [h] B_k) = e(g, A_k) as a leaf over n_keys virtual items (A_k, B_k, key k). A_k at infinity: the
        // key has no live item (every scalar 0), nothing to check
        levels = 2;
        HIP_TRY(w->a_Ak.ensure(n_keys * jw * 4));
        HIP_TRY(w->a_Akbytes.ensure(n_keys * (size_t)sl));
        HIP_TRY(w->a_Akaff.ensure(n_keys * aw * 4 + 16));
        HIP_TRY(w->a_Akstat.ensure(n_keys + 4));
        HIP_TRY(w->a_kpass.ensure(n_keys + 4));
        HIP_TRY(T.run("auth_msm_sigs_by_key", [&] {
          return dh::launch_msm28_set(g2, gB, iota, nullptr, w->a_kidx.as<uint32_t>(), n, n_keys, w->r_scal.as<uint4>(),
                                      w->s28.as<uint32_t>(), wsB, w->a_Ak.as<uint32_t>(), st);
        }));
        HIP_TRY(dh::launch_compress(g2, w->a_Ak.as<uint32_t>(), n_keys, w->a_Akbytes.as<uint8_t>(), w->a_Akaff.as<uint32_t>(),
                                    w->a_Akstat.as<uint8_t>(), st));
        HIP_TRY(hipMemsetAsync(w->a_kpass.p, 0, n_keys, st));
        HIP_TRY(T.run("k_partial_leaf(auth keys)", [&] {
          return dh::launch_partial_leaf(g2, iota, n_keys, w->a_Akaff.as<uint32_t>(), w->a_Akstat.as<uint8_t>(), iota, iota,
                                         w->outB.as<uint32_t>(), w->a_shares.as<uint32_t>(), (int)n_keys,
                                         w->a_kpass.as<uint8_t>(), st);
        }));
        std::vector<uint8_t> kpass(n_keys), akstat(n_keys);
        HIP_TRY(hipMemcpyAsync(kpass.data(), w->a_kpass.p, n_keys, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(akstat.data(), w->a_Akstat.p, n_keys, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        size_t nf = 0;
        for (size_t k = 0; k < n_keys; k++) nf += failing[k] = akstat[k] == 1 && kpass[k] != 1;
        // the product failed yet every key's own check passed: only possible through a sum at infinity; check them all
        if (!nf) failing.assign(n_keys, 1);
      }
      // level 3: leaf checks for the items under failing keys
      levels = 3;
      std::vector<uint32_t> list;
      std::vector<uint8_t> seen(n_keys, 0);
      for (size_t i = 0; i < n; i++)
        if (failing[kidx[i]]) {
          list.push_back((uint32_t)i);
          if (!seen[kidx[i]]) seen[kidx[i]] = 1, keys_failed++;
        }
      HIP_TRY(w->a_list.ensure(list.size() * 4 + 4));
      HIP_TRY(hipMemcpyAsync(w->a_list.p, list.data(), list.size() * 4, hipMemcpyHostToDevice, st));
      HIP_TRY(leaves(w->a_list.as<uint32_t>(), list.size()));
      leaf_items = list.size();
      HIP_TRY(hipStreamSynchronize(st));  // list is read by the copy above
    }
  }
  std::vector<uint8_t> kst(n_keys);
  HIP_TRY(hipMemcpyAsync(verdict_out, w->r_ok.p, n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(kst.data(), w->a_kstatus.p, n_keys, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  uint64_t rejected = 0;
  for (size_t i = 0; i < n; i++) rejected += verdict_out[i] != 1;
  if (key_ok_out)
    for (size_t k = 0; k < n_keys; k++) key_ok_out[k] = kst[k] == 1 ? 1 : 0;
  if (stats) {
    stats[0] = levels;
    stats[1] = keys_failed;
    stats[2] = leaf_items;
    stats[3] = rejected;
  }
  return DH_OK;
}

// ---- schnorr.Verify in batch (dh_schnorr_verify_batch: the schemes' DKGAuthScheme, crypto/schemes.go:103,144,184;
// dkg.VerifyPacketSignature, core/drand_beacon_control.go:354,476, and the leader's signature over group.Hash(),
// core/group_setup.go:384). Per item [s]G == R + [h]P with h = SHA-512(R || P || msg) mod r: no
// pairing and nothing shared between items but the tables, so the call is a fixed sequence of one-lane-per-item
// kernels and one copy back. DRANDHIP_SCHNORR_PATH=plain, read at every call, takes the check from two plain
// scalar multiplications instead of the joint chain over the tables.
static bool schnorr_plain_env() {
  const char* e = getenv("DRANDHIP_SCHNORR_PATH");
  return e && !strcmp(e, "plain");
}

// the generator's table of the key group, built once per process (context::gen_tab)
int schnorr_gen_table(bool key_g2, hipStream_t st, const uint32_t** out) {
  std::lock_guard<std::mutex> lk(g_ctx.gen_mu);
  const int g = key_g2 ? 1 : 0;
  if (!g_ctx.gen_ready[g]) {
    HIP_TRY(g_ctx.gen_tab[g].ensure(dh::schnorr_table_words(g) * 4));
    HIP_TRY(dh::launch_schnorr_table(g, nullptr, nullptr, 1, 1, g_ctx.gen_tab[g].as<uint32_t>(), st));
    HIP_TRY(hipStreamSynchronize(st));  // other workers' streams read it from now on
    g_ctx.gen_ready[g] = true;
  }
  *out = g_ctx.gen_tab[g].as<uint32_t>();
  return DH_OK;
}

// kidx: n key indices < n_keys (host); off: n + 1 message offsets from 0 (host)
int schnorr_core(worker* w, int scheme, const uint8_t* keys, size_t n_keys, const uint32_t* kidx, const uint8_t* msgs,
                 const uint32_t* off, const uint8_t* sigs, size_t sig_stride, size_t n, uint8_t* verdict_out,
                 uint8_t* key_ok_out, hipStream_t st) {
  const bool kg2 = !sig_on_g2(scheme);  // the key group is the other group of the beacon signatures
  const size_t kl = kg2 ? 96 : 48;
  const size_t kaw = (kg2 ? JAC_WORDS_G2 : JAC_WORDS_G1) * 2 / 3;
  const size_t total = off[n];
  const bool plain = schnorr_plain_env();
  timed_launches T(st);
  // 1. the key table: decode + subgroup test, one lane per key (dh_bls_verify_batch's rule)
  HIP_TRY(w->a_keys.ensure(n_keys * kl + 4));
  HIP_TRY(w->a_kstatus.ensure(n_keys + 4));
  HIP_TRY(w->a_kaff.ensure(n_keys * kaw * 4 + 16));
  HIP_TRY(hipMemcpyAsync(w->a_keys.p, keys, n_keys * kl, hipMemcpyHostToDevice, st));
  HIP_TRY(T.run(kg2 ? "k_prep_sig<fp2>(schnorr keys)" : "k_prep_sig<fp>(schnorr keys)", [&] {
    return dh::launch_prep(kg2, w->a_keys.as<uint8_t>(), kl, n_keys, w->a_kstatus.as<uint8_t>(), w->a_kaff.as<uint32_t>(), nullptr,
                           st);
  }));
  // 2. R of every item: decoded to a curve point, no subgroup test; infinity and the items of a bad key rejected
  HIP_TRY(w->r_raw.ensure(n * sig_stride + 4));
  HIP_TRY(w->r_pstatus.ensure(n + 4));
  HIP_TRY(w->r_paff.ensure(n * kaw * 4 + 16));
  HIP_TRY(w->a_kidx.ensure(n * 4 + 4));
  HIP_TRY(hipMemcpyAsync(w->r_raw.p, sigs, n * sig_stride, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w->a_kidx.p, kidx, n * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(T.run(kg2 ? "k_dec_sig_g2(schnorr R)" : "k_dec_sig_g1(schnorr R)", [&] {
    return dh::launch_dec_sig(kg2, w->r_raw.as<uint8_t>(), sig_stride, n, w->r_pstatus.as<uint8_t>(), w->r_paff.as<uint32_t>(),
                              nullptr, st);
  }));
  HIP_TRY(dh::launch_mark_bad_key(w->a_kidx.as<uint32_t>(), n, w->a_kstatus.as<uint8_t>(), w->r_pstatus.as<uint8_t>(), st));
  // 3. s < r, the challenge and the window digits
  HIP_TRY(w->r_msgs.ensure(total + 4));
  HIP_TRY(w->a_moff.ensure((n + 1) * 4));
  HIP_TRY(w->s_sc.ensure(n * dh::schnorr_scalar_words() * 4));
  if (total) HIP_TRY(hipMemcpyAsync(w->r_msgs.p, msgs, total, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w->a_moff.p, off, (n + 1) * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(T.run("k_schnorr_scalars", [&] {
    return dh::launch_schnorr_scalars(w->r_raw.as<uint8_t>(), sig_stride, (int)kl, w->a_keys.as<uint8_t>(), w->a_kidx.as<uint32_t>(),
                                      w->r_msgs.as<uint8_t>(), w->a_moff.as<uint32_t>(), n, w->r_pstatus.as<uint8_t>(),
                                      w->s_sc.as<uint32_t>(), st);
  }));
  // 4. the check
  HIP_TRY(w->r_ok.ensure(n + 4));
  if (plain) {
    HIP_TRY(T.run(kg2 ? "k_schnorr_plain<fp2>" : "k_schnorr_plain<fp>", [&] {
      return dh::launch_schnorr_plain(kg2, w->s_sc.as<uint32_t>(), w->r_pstatus.as<uint8_t>(), w->r_paff.as<uint32_t>(),
                                      w->a_kidx.as<uint32_t>(), w->a_kaff.as<uint32_t>(), n, w->r_ok.as<uint8_t>(), st);
    }));
  } else {
    const uint32_t* gtab = nullptr;
    int rc = schnorr_gen_table(kg2, st, &gtab);
    if (rc) return rc;
    HIP_TRY(w->s_ktab.ensure(n_keys * dh::schnorr_table_words(kg2) * 4));
    HIP_TRY(T.run(kg2 ? "k_schnorr_table<fp2>" : "k_schnorr_table<fp>", [&] {
      return dh::launch_schnorr_table(kg2, w->a_kaff.as<uint32_t>(), w->a_kstatus.as<uint8_t>(), n_keys, 0,
                                      w->s_ktab.as<uint32_t>(), st);
    }));
    HIP_TRY(T.run(kg2 ? "k_schnorr_check<fp2>" : "k_schnorr_check<fp>", [&] {
      return dh::launch_schnorr_check(kg2, w->s_sc.as<uint32_t>(), w->r_pstatus.as<uint8_t>(), w->r_paff.as<uint32_t>(),
                                      w->a_kidx.as<uint32_t>(), gtab, w->s_ktab.as<uint32_t>(), n, w->r_ok.as<uint8_t>(), st);
    }));
  }
  std::vector<uint8_t> kst(key_ok_out ? n_keys : 0);
  HIP_TRY(hipMemcpyAsync(verdict_out, w->r_ok.p, n, hipMemcpyDeviceToHost, st));
  if (key_ok_out) HIP_TRY(hipMemcpyAsync(kst.data(), w->a_kstatus.p, n_keys, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (key_ok_out)
    for (size_t k = 0; k < n_keys; k++) key_ok_out[k] = kst[k] == 1 ? 1 : 0;
  return DH_OK;
}

// ---- one call over several internal streams (the drop-in callers make ONE call per window)
// Off by default: measured on the MI355X (profiles/split_sweep_r02k_*.jsonl), one stream per call is the fastest
// form of a call (1M rounds 64.9 ms, 4M 225.8 ms = 92% of the 8-batches-in-flight rate) — a chunk's per-round
// kernels alone on the chip are no faster than one large launch, and the chunks' latency-bound tails, made of
// many small kernels, wait for wave slots the per-round kernels hold and slow them. When enabled
// (DRANDHIP_SPLIT="chunk,workers" or dh_set_split), a batch is cut into chunks, each a complete batch check (its own
// RLC scalars: seed + chunk index when the caller fixed a seed, fresh CSPRNG seeds otherwise, so verdicts stay
// bit-exact per round), verified by up to `workers` leased workers; the chunks' per-round kernels are chained in
// chunk order across the workers' streams (prep_gate) and each chunk's tail runs on its worker's high-priority
// stream. Streams share the process's hardware queues (GPU_MAX_HW_QUEUES, 4 by default per priority).
struct split_cfg {
  size_t chunk = 0;  // 0: one stream per call
  int workers = 3;
};
std::mutex g_split_mu;
split_cfg g_split = [] {
  split_cfg r;
  const char* e = getenv("DRANDHIP_SPLIT");
  if (e && *e) {
    char* end = nullptr;
    r.chunk = strtoull(e, &end, 10);
    if (end && *end == ',') r.workers = std::max(1, atoi(end + 1));
  }
  return r;
}();
static split_cfg split_config() {
  std::lock_guard<std::mutex> lk(g_split_mu);
  return g_split;
}

int ensure_device() {
  std::lock_guard<std::mutex> lk(g_ctx.mu);
  int rc = ensure_init_locked(0);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(g_ctx.device));
  return DH_OK;
}

template <class F>
int run_split(size_t n, F&& fn, uint64_t seed) {
  const split_cfg cfg = split_config();
  size_t nchunks = 1;
  if (cfg.chunk && cfg.workers > 1 && n >= 2 * cfg.chunk) nchunks = (n + cfg.chunk - 1) / cfg.chunk;
  const size_t per = (n + nchunks - 1) / std::max<size_t>(nchunks, 1);
  const int nthreads = (int)std::min<size_t>(nchunks, (size_t)cfg.workers);
  std::atomic<size_t> next{0};
  std::atomic<int> first_rc{DH_OK};
  std::mutex err_mu;
  std::string err;
  // prep chain: chunk c's per-round kernels queue behind chunk c-1's (event ev[c-1], recorded by its thread)
  std::vector<hipEvent_t> ev(nchunks > 1 ? nchunks : 0, nullptr);
  std::vector<char> rec(nchunks, 0);
  std::mutex gate_mu;
  std::condition_variable gate_cv;
  for (auto& e : ev) {
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      for (auto& x : ev)
        if (x) (void)hipEventDestroy(x);
      return fail(DH_EDEVICE, "hipEventCreate failed");
    }
  }
  auto mark = [&](size_t c) {
    std::lock_guard<std::mutex> lk(gate_mu);
    rec[c] = 1;
    gate_cv.notify_all();
  };
  auto body = [&]() {
    lease L;
    int rc = L.rc ? L.rc : set_device_and_stream(L.w);
    for (size_t c; !rc && (c = next.fetch_add(1)) < nchunks;) {
      const size_t lo = c * per, hi = std::min(n, lo + per);
      prep_gate g;
      prep_gate* gp = nullptr;
      if (nchunks > 1) {
        if (c > 0) {  // chunk c-1 is held by a running thread that never waits on a later chunk: no deadlock
          std::unique_lock<std::mutex> lk(gate_mu);
          gate_cv.wait(lk, [&] { return rec[c - 1] != 0; });
          g.wait = ev[c - 1];
        }
        g.done = ev[c];
        g.recorded = [&mark, c] { mark(c); };
        gp = &g;
      }
      if (lo < hi) rc = fn(L.w, lo, hi, seed ? seed + 0x9e3779b97f4a7c15ULL * c : 0, gp);
      if (nchunks > 1) mark(c);  // also on failure: the next chunk must not wait forever
    }
    if (rc) {
      int expect = DH_OK;
      if (first_rc.compare_exchange_strong(expect, rc)) {
        std::lock_guard<std::mutex> lk(err_mu);
        err = g_err;  // the message lives in this thread's g_err: hand it to the caller's
      }
      next.store(nchunks);  // stop the other workers early
    }
  };
  if (nthreads <= 1) {
    body();
  } else {
    std::vector<std::thread> ths;
    for (int t = 1; t < nthreads; t++) ths.emplace_back(body);
    body();
    for (auto& th : ths) th.join();
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  const int rc = first_rc.load();
  if (rc) g_err = err;
  return rc;
}

}  // namespace

static void handles_shutdown();  // store, writer and archive handles, below

extern "C" {

int dh_init(uint32_t device_mask) {
  std::lock_guard<std::mutex> lk(g_ctx.mu);
  return ensure_init_locked(device_mask);
}

void dh_shutdown(void) {
  handles_shutdown();  // store, writer and archive handles are invalidated; one inside a call when that call ends
  // idle workers are freed now; a worker leased by a call still running on another thread is retired and freed
  // when that call returns, so the call never touches freed memory
  std::lock_guard<std::mutex> lk(g_ctx.mu);
  for (worker* w : g_ctx.pool) {
    if (w->busy) {
      g_ctx.retired.push_back(w);
      continue;
    }
    w->release_all();
    delete w;
  }
  {
    std::lock_guard<std::mutex> gk(g_ctx.gen_mu);
    for (int g = 0; g < 2; g++) {
      if (g_ctx.gen_tab[g].p) g_ctx.gen_old.push_back(g_ctx.gen_tab[g].p);
      g_ctx.gen_tab[g].p = nullptr;
      g_ctx.gen_tab[g].cap = 0;
      g_ctx.gen_ready[g] = false;
    }
    if (g_ctx.retired.empty()) {
      for (void* q : g_ctx.gen_old) (void)hipFree(q);
      g_ctx.gen_old.clear();
    }
  }
  g_ctx.pool.clear();
  g_ctx.inited = false;
}

int dh_scheme_from_name(const char* name) {
  if (!name) return fail(DH_EINVAL, "null scheme name");
  static const char* names[4] = {"pedersen-bls-chained", "pedersen-bls-unchained", "bls-unchained-on-g1",
                                 "bls-unchained-g1-rfc9380"};
  for (int i = 0; i < 4; i++)
    if (!strcmp(name, names[i])) return i;
  return fail(DH_EINVAL, "invalid scheme name '%s'", name);
}

int dh_sig_len(int scheme) {
  if (scheme < 0 || scheme > 3) return fail(DH_EINVAL, "unknown scheme %d", scheme);
  return sig_on_g2(scheme) ? 96 : 48;
}
int dh_key_len(int scheme) {
  if (scheme < 0 || scheme > 3) return fail(DH_EINVAL, "unknown scheme %d", scheme);
  return sig_on_g2(scheme) ? 48 : 96;
}

int dh_verify_batch_device(int scheme, const uint8_t* pk, size_t pk_len, const uint64_t* d_rounds, const uint8_t* d_sigs,
                           size_t sig_stride, const uint8_t* d_prevs, size_t prev_stride, const uint32_t* d_prev_lens,
                           size_t n, uint8_t* d_verdict_out, uint8_t* d_rand_out, uint64_t seed, void* hip_stream,
                           uint64_t stats_out[4]) {
  if (scheme < 0 || scheme > 3) return fail(DH_EINVAL, "unknown scheme %d", scheme);
  if (!pk || (n && (!d_rounds || !d_sigs || !d_verdict_out))) return fail(DH_EINVAL, "null argument");
  if (stats_out) memset(stats_out, 0, 4 * sizeof(uint64_t));
  if (n && n <= small_batch_max()) {  // the small-batch path: every round its own check (stats: 0 levels, n leaves)
    lease L;
    if (L.rc) return L.rc;
    worker* w = L.w;
    int rc = set_device_and_stream(w);
    if (rc) return rc;
    hipStream_t st = w->stream;
    if (hip_stream) {
      HIP_TRY(hipEventRecord(w->part_ready, (hipStream_t)hip_stream));
      HIP_TRY(hipStreamWaitEvent(st, w->part_ready, 0));
    }
    const bool chained = scheme == DH_SCHEME_CHAINED && d_prevs;
    rc = verify_small(w, scheme, pk, pk_len, d_rounds, d_sigs, sig_stride, chained ? d_prevs : nullptr, prev_stride,
                      chained ? d_prev_lens : nullptr, n, d_verdict_out, d_rand_out, nullptr, st, false);
    if (rc) {
      (void)hipStreamSynchronize(st);
      if (w->tail) (void)hipStreamSynchronize(w->tail);
      return rc;
    }
    if (stats_out) {
      w->h_verdict.resize(n);
      HIP_TRY(hipMemcpyAsync(w->h_verdict.data(), d_verdict_out, n, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (stats_out) {
      size_t ok = 0;
      for (size_t i = 0; i < n; i++) ok += w->h_verdict[i] ? 1 : 0;
      stats_out[2] = n;
      stats_out[3] = n - ok;
    }
    return DH_OK;
  }
  // inputs produced on the caller's stream: every internal stream waits for that stream's work first
  hipEvent_t ready = nullptr;
  if (hip_stream) {
    int rc0 = ensure_device();
    if (rc0) return rc0;
    HIP_TRY(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ready, (hipStream_t)hip_stream));
  }
  std::mutex stats_mu;
  int rc = run_split(n, [&](worker* w, size_t lo, size_t hi, uint64_t chunk_seed, prep_gate* gate) -> int {
    if (ready) HIP_TRY(hipStreamWaitEvent(w->stream, ready, 0));
    uint64_t st4[4];
    const bool chained = scheme == DH_SCHEME_CHAINED && d_prevs;
    int r = verify_core(w, scheme, pk, pk_len, d_rounds + lo, d_sigs + lo * sig_stride, sig_stride,
                        chained ? d_prevs + lo * prev_stride : nullptr,
                        prev_stride, chained && d_prev_lens ? d_prev_lens + lo : nullptr, hi - lo, d_verdict_out + lo,
                        d_rand_out ? d_rand_out + lo * 32 : nullptr, chunk_seed, w->stream, stats_out ? st4 : nullptr,
                        nullptr, VM_FULL, gate);
    if (!r && stats_out) {
      std::lock_guard<std::mutex> lk(stats_mu);
      stats_out[0] = std::max(stats_out[0], st4[0]);
      for (int k = 1; k < 4; k++) stats_out[k] += st4[k];
    }
    return r;
  }, seed);
  if (ready) (void)hipEventDestroy(ready);
  return rc;
}

int dh_verify_batch(int scheme, const uint8_t* pk, size_t pk_len, const uint64_t* rounds, const uint8_t* sigs,
                    size_t sig_stride, const uint8_t* prevs, size_t prev_stride, const uint32_t* prev_lens, size_t n,
                    uint8_t* verdict_out, uint8_t* rand_out, uint64_t seed) {
  if (scheme < 0 || scheme > 3) return fail(DH_EINVAL, "unknown scheme %d", scheme);
  if (!pk || (n && (!rounds || !sigs || !verdict_out))) return fail(DH_EINVAL, "null argument");
  if (n == 0) return DH_OK;
  const bool chained = scheme == DH_SCHEME_CHAINED && prevs;
  if (chained && prev_lens)
    for (size_t i = 0; i < n; i++)
      if (prev_lens[i] > prev_stride)
        return fail(DH_EINVAL, "previous signature %zu: length %u exceeds the record stride %zu", i, prev_lens[i], prev_stride);
  if (n <= small_batch_max()) return verify_small_host(scheme, pk, pk_len, rounds, sigs, sig_stride, chained ? prevs : nullptr,
                                                       prev_stride, chained ? prev_lens : nullptr, nullptr, n, verdict_out,
                                                       rand_out);
  // one chunk per worker at a time: its host->device copies overlap the other chunks' kernels
  return run_split(n, [&](worker* w, size_t lo, size_t hi, uint64_t chunk_seed, prep_gate* gate) -> int {
    const size_t m = hi - lo;
    hipStream_t st = w->stream;
    HIP_TRY(w->in_rounds.ensure(m * 8));
    HIP_TRY(w->in_sigs.ensure(m * sig_stride));
    HIP_TRY(w->out_verdict.ensure(m));
    if (rand_out) HIP_TRY(w->out_rand.ensure(m * 32));
    HIP_TRY(hipMemcpyAsync(w->in_rounds.p, rounds + lo, m * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(w->in_sigs.p, sigs + lo * sig_stride, m * sig_stride, hipMemcpyHostToDevice, st));
    if (chained) {
      HIP_TRY(w->in_prevs.ensure(m * prev_stride + 4));
      HIP_TRY(hipMemcpyAsync(w->in_prevs.p, prevs + lo * prev_stride, m * prev_stride, hipMemcpyHostToDevice, st));
      if (prev_lens) {
        HIP_TRY(w->in_prev_lens.ensure(m * 4));
        HIP_TRY(hipMemcpyAsync(w->in_prev_lens.p, prev_lens + lo, m * 4, hipMemcpyHostToDevice, st));
      }
    }
    int rc = verify_core(w, scheme, pk, pk_len, w->in_rounds.as<uint64_t>(), w->in_sigs.as<uint8_t>(), sig_stride,
                         chained ? w->in_prevs.as<uint8_t>() : nullptr, prev_stride,
                         chained && prev_lens ? w->in_prev_lens.as<uint32_t>() : nullptr, m, w->out_verdict.as<uint8_t>(),
                         rand_out ? w->out_rand.as<uint8_t>() : nullptr, chunk_seed, st, nullptr, nullptr, VM_FULL, gate);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(verdict_out + lo, w->out_verdict.p, m, hipMemcpyDeviceToHost, st));
    if (rand_out) HIP_TRY(hipMemcpyAsync(rand_out + lo * 32, w->out_rand.p, m * 32, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DH_OK;
  }, seed);
}

// ---- node-wide batch check over several processes (one per GPU)
// A node batch holds ONE worker from dh_batch_begin to dh_batch_finish and runs everything on it: the per-round
// kernels on its stream, the level-0 MSM, the record, the node-wide check of the gathered records and the bisection
// on its high-priority tail stream (dh_batch_stream), where the caller also queues the collective. Nothing in begin
// or check waits on the host, and with one rank nothing crosses streams at all.
struct dh_batch {
  lease* L = nullptr;
  int scheme = 0;
  std::vector<uint8_t> pk;
  const uint64_t* d_rounds = nullptr;
  const uint8_t* d_sigs = nullptr;
  size_t sig_stride = 0;
  const uint8_t* d_prevs = nullptr;
  size_t prev_stride = 0;
  const uint32_t* d_prev_lens = nullptr;
  size_t n = 0;
  uint8_t* d_verdict = nullptr;
  uint8_t* d_rand = nullptr;
  hipStream_t st = nullptr;
  bool checked = false;  // dh_batch_check queued: its result is in the worker's node_res[2]
};

// one record: A, B (Jacobian AoS) + a status word (0 = this rank's batch began; nonzero = abandoned) + 3 pad words
static size_t partial_words(bool g2) { return 2 * (g2 ? JAC_WORDS_G2 : JAC_WORDS_G1) + 4; }

int dh_partial_bytes(int scheme) {
  if (scheme < 0 || scheme > 3) return fail(DH_EINVAL, "unknown scheme %d", scheme);
  return (int)(partial_words(sig_on_g2(scheme)) * 4);
}

// A node batch queues its level-0 tail, record, exchange and check on the worker's normal stream behind its per-round
// kernels, with the level-0 sort there too, instead of handing the tail to the high-priority stream behind an event
// wait: 8 batches in flight, one GPU (gpurun_out r04y, one box): 1M rounds 25.75 -> 26.36 M/s (local check 26.48),
// 131k rounds 18.09 -> 21.42 M/s. A high-priority queue holding a batch's pending wait for the whole of its per-round
// kernels cost the other batches' dispatch (the local path's host wait before queueing its tail is the same fix).
// DRANDHIP_NODE_ONE_STREAM=0 restores the tail-stream handoff (comparison runs).
static bool node_one_stream() {
  static const bool v = env_on("DRANDHIP_NODE_ONE_STREAM", true);
  return v;
}
static hipStream_t batch_stream(worker* w) { return node_one_stream() ? w->stream : w->tail; }

int dh_batch_begin(int scheme, const uint8_t* pk, size_t pk_len, const uint64_t* d_rounds, const uint8_t* d_sigs,
                   size_t sig_stride, const uint8_t* d_prevs, size_t prev_stride, const uint32_t* d_prev_lens, size_t n,
                   uint8_t* d_verdict_out, uint8_t* d_rand_out, uint64_t seed, void* hip_stream, dh_batch** batch_out,
                   uint8_t* d_partials_out) {
  if (!batch_out) return fail(DH_EINVAL, "null batch handle");
  *batch_out = nullptr;
  if (scheme < 0 || scheme > 3) return fail(DH_EINVAL, "unknown scheme %d", scheme);
  if (!pk || !d_partials_out || (n && (!d_rounds || !d_sigs || !d_verdict_out))) return fail(DH_EINVAL, "null argument");
  std::unique_ptr<dh_batch> b(new dh_batch());
  b->L = new lease(false);  // the lease spans the collective: fail (DH_EBUSY) rather than wait for a worker
  if (b->L->rc) {
    int rc = b->L->rc;
    delete b->L;
    return rc;
  }
  worker* w = b->L->w;
  int rc = set_device_and_stream(w, !node_one_stream());
  if (!rc && hip_stream) {  // inputs produced on the caller's stream
    if (hipEventRecord(w->part_ready, (hipStream_t)hip_stream) != hipSuccess ||
        hipStreamWaitEvent(w->stream, w->part_ready, 0) != hipSuccess)
      rc = fail(DH_EDEVICE, "cannot order the batch after the caller's stream");
  }
  b->scheme = scheme;
  b->pk.assign(pk, pk + pk_len);
  b->d_rounds = d_rounds;
  b->d_sigs = d_sigs;
  b->sig_stride = sig_stride;
  b->d_prevs = d_prevs;
  b->prev_stride = prev_stride;
  b->d_prev_lens = d_prev_lens;
  b->n = n;
  b->d_verdict = d_verdict_out;
  b->d_rand = d_rand_out;
  b->st = w->stream;
  const size_t jw = sig_on_g2(scheme) ? JAC_WORDS_G2 : JAC_WORDS_G1;
  if (!rc) {
    w->begin_one_stream = node_one_stream();
    rc = verify_core(w, scheme, pk, pk_len, d_rounds, d_sigs, sig_stride, d_prevs, prev_stride, d_prev_lens, n, d_verdict_out,
                     d_rand_out, seed, b->st, nullptr, nullptr, VM_BEGIN);
    w->begin_one_stream = false;
  }
  if (!rc) {
    // the record (A, B, status 0) on the batch stream, where the level-0 MSM wrote the sums (an empty batch
    // contributes the identity, Z = 0)
    hipStream_t ts = batch_stream(w);
    const bool ok = (n ? hipMemcpyAsync(d_partials_out, w->outA.p, jw * 4, hipMemcpyDeviceToDevice, ts) == hipSuccess &&
                             hipMemcpyAsync(d_partials_out + jw * 4, w->outB.p, jw * 4, hipMemcpyDeviceToDevice, ts) == hipSuccess
                       : hipMemsetAsync(d_partials_out, 0, 2 * jw * 4, ts) == hipSuccess) &&
                    hipMemsetAsync(d_partials_out + 2 * jw * 4, 0, 16, ts) == hipSuccess;
    if (!ok) {
      rc = fail(DH_EDEVICE, "writing the partial sums failed");
    }
  }
  if (rc) {
    if (w->stream) (void)hipStreamSynchronize(w->stream);  // nothing queued may outlive the lease
    if (w->tail) (void)hipStreamSynchronize(w->tail);
    delete b->L;
    return rc;
  }
  *batch_out = b.release();
  return DH_OK;
}

// the node-wide check of k gathered records on the batch stream: sum, one pairing check, res = w->node_res
static int queue_node_check(worker* w, bool g2, const uint8_t* pk, size_t pk_len, const uint8_t* d_partials, size_t k,
                            hipStream_t ts) {
  int rc = ensure_key(w, g2, pk, pk_len, ts);
  if (rc) return rc;
  const size_t jw = g2 ? JAC_WORDS_G2 : JAC_WORDS_G1;
  HIP_TRY(w->node_sum.ensure(2 * jw * 4));
  HIP_TRY(w->node_res.ensure(16));
  HIP_TRY(hipMemsetAsync(w->node_res.p, 0, 16, ts));
  uint32_t* sA = w->node_sum.as<uint32_t>();
  uint8_t* res = w->node_res.as<uint8_t>();
  HIP_TRY(dh::launch_sum_partials(g2, (const uint32_t*)d_partials, k, partial_words(g2), sA, sA + jw, res, ts));
  HIP_TRY(group_check(w, g2, sA, sA + jw, 1, w->key_cur, res + 1, ts, w->key_cur + 48));
  return DH_OK;
}

void* dh_batch_stream(dh_batch* b) { return b ? (void*)batch_stream(b->L->w) : nullptr; }

int dh_batch_check(dh_batch* b, const uint8_t* d_partials, size_t k, void* hip_stream) {
  if (!b || !d_partials || !k) return fail(DH_EINVAL, "bad node-check arguments");
  worker* w = b->L->w;
  const bool g2 = sig_on_g2(b->scheme);
  hipStream_t bs = batch_stream(w);
  if (hip_stream && (hipStream_t)hip_stream != bs) {  // the gathered records are produced on the caller's stream
    HIP_TRY(hipEventRecord(w->gath_ready, (hipStream_t)hip_stream));
    HIP_TRY(hipStreamWaitEvent(bs, w->gath_ready, 0));
  }
  int rc = queue_node_check(w, g2, b->pk.data(), b->pk.size(), d_partials, k, bs);
  if (rc) return rc;
  // the node-wide result (node_res[2]) and, when it passed, every decoded round of this batch marked valid on the
  // device. A one-round batch put only the identity into the node-wide sums (verify_core VM_BEGIN, n < 2), so the check
  // says nothing about its round: none is marked here, and dh_batch_finish always gives it its leaf check.
  HIP_TRY(dh::launch_node_mark(b->n >= 2 ? b->n : 0, w->node_res.as<uint8_t>(), w->status.as<uint8_t>(), b->d_verdict, bs));
  b->checked = true;
  return DH_OK;
}

int dh_check_partials(int scheme, const uint8_t* pk, size_t pk_len, const uint8_t* d_partials, size_t k, int* pass_out) {
  if (scheme < 0 || scheme > 3) return fail(DH_EINVAL, "unknown scheme %d", scheme);
  if (!pk || !d_partials || !pass_out || !k) return fail(DH_EINVAL, "bad node-check arguments");
  const bool g2 = sig_on_g2(scheme);
  const size_t key_len = g2 ? 48 : 96;
  if (pk_len != key_len) return fail(DH_EINVAL, "public key must be %zu bytes for scheme %d", key_len, scheme);
  lease L;
  if (L.rc) return L.rc;
  worker* w = L.w;
  int rc = set_device_and_stream(w);
  if (rc) return rc;
  rc = queue_node_check(w, g2, pk, pk_len, d_partials, k, w->tail);
  if (rc) return rc;
  uint8_t res[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(res, w->node_res.p, 2, hipMemcpyDeviceToHost, w->tail));
  HIP_TRY(hipStreamSynchronize(w->tail));
  *pass_out = 0;
  if (res[0]) return fail(DH_EABANDONED, "a rank abandoned the node batch (nonzero status word)");
  *pass_out = res[1] == 1 ? 1 : 0;
  return DH_OK;
}

int dh_batch_finish(dh_batch* b, int node_pass, uint64_t stats_out[4]) {
  if (!b) return fail(DH_EINVAL, "null batch handle");
  worker* w = b->L->w;
  int rc = DH_OK, ret = DH_OK;
  if (stats_out) memset(stats_out, 0, 4 * sizeof(uint64_t));
  if (node_pass == DH_NODE_CHECKED) {
    uint8_t res = 0;
    if (!b->checked) {
      rc = fail(DH_EINVAL, "dh_batch_finish(DH_NODE_CHECKED) without dh_batch_check");
    } else if (hipMemcpyAsync(&res, w->node_res.as<uint8_t>() + 2, 1, hipMemcpyDeviceToHost, batch_stream(w)) != hipSuccess ||
               hipStreamSynchronize(batch_stream(w)) != hipSuccess) {
      rc = fail(DH_EDEVICE, "reading the node-wide check failed");
    } else if (res == 2) {
      rc = fail(DH_EABANDONED, "node batch abandoned: dh_batch_begin failed on another rank");
    } else {
      ret = res == 1 ? 1 : 0;
      // passed: the verdicts are already marked (dh_batch_check); the level bookkeeping only when stats are asked.
      // A one-round batch is never covered by the node check: its leaf check runs in every case.
      if (res != 1 || stats_out || b->n < 2)
        rc = verify_core(w, b->scheme, b->pk.data(), b->pk.size(), b->d_rounds, b->d_sigs, b->sig_stride, b->d_prevs,
                         b->prev_stride, b->d_prev_lens, b->n, b->d_verdict, b->d_rand, 0, b->st, stats_out, nullptr,
                         res == 1 ? VM_FINISH_PASS : VM_FINISH);
    }
  } else if (node_pass >= 0) {
    rc = verify_core(w, b->scheme, b->pk.data(), b->pk.size(), b->d_rounds, b->d_sigs, b->sig_stride, b->d_prevs,
                     b->prev_stride, b->d_prev_lens, b->n, b->d_verdict, b->d_rand, 0, b->st, stats_out, nullptr,
                     node_pass ? VM_FINISH_PASS : VM_FINISH);
  }
  // abandoned or failed: nothing this batch queued may outlive its lease
  if (w->stream) (void)hipStreamSynchronize(w->stream);
  if (w->tail) (void)hipStreamSynchronize(w->tail);
  delete b->L;
  delete b;
  return rc ? rc : ret;
}

int dh_verify_beacon(int scheme, const uint8_t* pk, size_t pk_len, uint64_t round, const uint8_t* sig, size_t sig_len,
                     const uint8_t* prev, size_t prev_len) {
  int sl = dh_sig_len(scheme);
  if (sl < 0) return sl;
  if (!sig || sig_len != (size_t)sl) return 0;  // kyber: wrong-length signature is an invalid signature
  uint8_t sbuf[96] __attribute__((aligned(16)));
  memcpy(sbuf, sig, sig_len);
  // the previous signature is hashed whatever its length (crypto/schemes.go:106-114)
  if (scheme == DH_SCHEME_CHAINED && prev_len > 0xffffffffu) return fail(DH_EINVAL, "previous signature too long");
  std::vector<uint8_t> pbuf(std::max<size_t>(96, (prev_len + 3) & ~(size_t)3), 0);
  uint32_t plen = 0;
  if (scheme == DH_SCHEME_CHAINED && prev && prev_len) {
    memcpy(pbuf.data(), prev, prev_len);
    plen = (uint32_t)prev_len;
  }
  uint8_t verdict = 0;
  int rc = dh_verify_batch(scheme, pk, pk_len, &round, sbuf, (size_t)sl, scheme == DH_SCHEME_CHAINED ? pbuf.data() : nullptr,
                           pbuf.size(), scheme == DH_SCHEME_CHAINED ? &plen : nullptr, 1, &verdict, nullptr, 0);
  return rc < 0 ? rc : verdict;
}

int dh_verify_recovered_batch(int scheme, const uint8_t* pk, size_t pk_len, const uint8_t* msgs32, const uint8_t* sigs,
                              size_t sig_stride, size_t n, uint8_t* verdict_out, uint64_t seed) {
  if (scheme < 0 || scheme > 3) return fail(DH_EINVAL, "unknown scheme %d", scheme);
  if (!pk || (n && (!msgs32 || !sigs || !verdict_out))) return fail(DH_EINVAL, "null argument");
  if (n == 0) return DH_OK;
  if (n <= small_batch_max())
    return verify_small_host(scheme, pk, pk_len, nullptr, sigs, sig_stride, nullptr, 0, nullptr, msgs32, n, verdict_out, nullptr);
  lease L;
  if (L.rc) return L.rc;
  worker* w = L.w;
  int rc = set_device_and_stream(w);
  if (rc) return rc;
  hipStream_t st = w->stream;
  HIP_TRY(w->in_sigs.ensure(n * sig_stride));
  HIP_TRY(w->r_msgs.ensure(n * 32));
  HIP_TRY(w->out_verdict.ensure(n));
  HIP_TRY(hipMemcpyAsync(w->in_sigs.p, sigs, n * sig_stride, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w->r_msgs.p, msgs32, n * 32, hipMemcpyHostToDevice, st));
  rc = verify_core(w, scheme, pk, pk_len, nullptr, w->in_sigs.as<uint8_t>(), sig_stride, nullptr, 0, nullptr, n,
                   w->out_verdict.as<uint8_t>(), nullptr, seed, st, nullptr, w->r_msgs.as<uint8_t>());
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(verdict_out, w->out_verdict.p, n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DH_OK;
}

int dh_verify_recovered(int scheme, const uint8_t* pk, size_t pk_len, const uint8_t* msg32, const uint8_t* sig,
                        size_t sig_len) {
  int sl = dh_sig_len(scheme);
  if (sl < 0) return sl;
  if (!msg32) return fail(DH_EINVAL, "null argument");
  if (!sig || sig_len != (size_t)sl) return 0;  // kyber: wrong-length signature is an invalid signature
  uint8_t sbuf[96] __attribute__((aligned(16)));
  memcpy(sbuf, sig, sig_len);
  uint8_t verdict = 0;
  int rc = dh_verify_recovered_batch(scheme, pk, pk_len, msg32, sbuf, (size_t)sl, 1, &verdict, 0);
  return rc < 0 ? rc : verdict;
}

int dh_digest_batch(int scheme, const uint64_t* rounds, const uint8_t* prevs, size_t prev_stride,
                    const uint32_t* prev_lens, size_t n, uint8_t* out) {
  if (scheme < 0 || scheme > 3) return fail(DH_EINVAL, "unknown scheme %d", scheme);
  for (size_t i = 0; i < n; i++) {
    sha256_host s;
    s.init();
    if (scheme == DH_SCHEME_CHAINED && prevs) {
      size_t pl = prev_lens ? prev_lens[i] : prev_stride;
      if (pl > prev_stride) return fail(DH_EINVAL, "previous signature %zu: length %zu exceeds the record stride %zu", i, pl, prev_stride);
      s.update(prevs + i * prev_stride, pl);
    }
    uint8_t r[8];
    for (int k = 0; k < 8; k++) r[k] = (uint8_t)(rounds[i] >> (56 - 8 * k));
    s.update(r, 8);
    s.final(out + 32 * i);
  }
  return DH_OK;
}

int dh_randomness_batch(int scheme, const uint8_t* sigs, size_t sig_stride, size_t n, uint8_t* out) {
  int sl = dh_sig_len(scheme);
  if (sl < 0) return sl;
  if (n == 0) return DH_OK;
  if (sig_stride < (size_t)sl || sig_stride % 4) return fail(DH_EINVAL, "bad signature stride %zu", sig_stride);
  lease L;
  if (L.rc) return L.rc;
  worker* w = L.w;
  int rc = set_device_and_stream(w);
  if (rc) return rc;
  hipStream_t st = w->stream;
  HIP_TRY(w->in_sigs.ensure(n * sig_stride));
  HIP_TRY(w->out_rand.ensure(n * 32));
  HIP_TRY(w->status.ensure(n));
  HIP_TRY(w->sig_aff.ensure(n * (sl == 96 ? 48 : 24) * 4));
  HIP_TRY(hipMemcpyAsync(w->in_sigs.p, sigs, n * sig_stride, hipMemcpyHostToDevice, st));
  HIP_TRY(dh::launch_prep(sl == 96, w->in_sigs.as<uint8_t>(), sig_stride, n, w->status.as<uint8_t>(),
                          w->sig_aff.as<uint32_t>(), w->out_rand.as<uint8_t>(), st));
  HIP_TRY(hipMemcpyAsync(out, w->out_rand.p, n * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DH_OK;
}

int dh_recover_batch(int scheme, const uint8_t* commits, int t, int n_nodes, const uint8_t* msgs32,
                     const uint8_t* partials, const uint32_t* part_off, size_t n_rounds, uint8_t* sig_out,
                     uint8_t* status_out) {
  if (scheme < 0 || scheme > 3) return fail(DH_EINVAL, "unknown scheme %d", scheme);
  if (t < 1 || n_nodes < 1 || n_nodes > 65536 || !commits || (n_rounds && (!msgs32 || !partials || !part_off ||
                                                                          !sig_out || !status_out)))
    return fail(DH_EINVAL, "bad Recover arguments");
  for (size_t j = 0; j < n_rounds; j++)
    if (part_off[j + 1] < part_off[j]) return fail(DH_EINVAL, "part_off must be non-decreasing");
  lease L;
  if (L.rc) return L.rc;
  int rc = set_device_and_stream(L.w);
  if (rc) return rc;
  return recover_core(L.w, scheme, commits, t, n_nodes, msgs32, partials, part_off, n_rounds, sig_out, status_out,
                      L.w->stream);
}

int dh_verify_partials_batch(int scheme, const uint8_t* commits, int t, int n_nodes, const uint8_t* msgs32,
                             const uint8_t* partials, const uint32_t* part_off, size_t n_rounds, uint8_t* ok_out) {
  if (scheme < 0 || scheme > 3) return fail(DH_EINVAL, "unknown scheme %d", scheme);
  if (t < 1 || n_nodes < 1 || n_nodes > 65536 || !commits || (n_rounds && (!msgs32 || !partials || !part_off || !ok_out)))
    return fail(DH_EINVAL, "bad VerifyPartial arguments");
  for (size_t j = 0; j < n_rounds; j++)
    if (part_off[j + 1] < part_off[j]) return fail(DH_EINVAL, "part_off must be non-decreasing");
  if (n_rounds == 0 || part_off[n_rounds] == part_off[0]) return DH_OK;
  lease L;
  if (L.rc) return L.rc;
  int rc = set_device_and_stream(L.w);
  if (rc) return rc;
  std::vector<uint8_t> status(n_rounds);
  return recover_core(L.w, scheme, commits, t, n_nodes, msgs32, partials, part_off, n_rounds, nullptr, status.data(),
                      L.w->stream, ok_out);
}

// The items of dh_bls_verify_batch and dh_schnorr_verify_batch: the refusals the two calls share (sl: the scheme's
// signature length, n_limit: the caller's bound on n), each item's key index, its message offset from msg_off[0], and
// the number of distinct keys the items name.
struct keyed_items {
  std::vector<uint32_t> kidx, off;
  size_t keys_used = 0;
  int check(const uint8_t* keys, size_t n_keys, const uint32_t* key_idx, const uint8_t* msgs, const uint32_t* msg_off, const uint8_t* sigs,
            size_t sig_stride, size_t sl, size_t n, size_t n_limit, const uint8_t* verdict_out) {
    if (n_keys && !keys) return fail(DH_EINVAL, "null key table");
    if (!key_idx && n_keys != n) return fail(DH_EINVAL, "key_idx is null: one key per item, yet %zu keys for %zu items", n_keys, n);
    if (n && !n_keys) return fail(DH_EINVAL, "%zu items and no keys", n);
    if (n && (!msg_off || !sigs || !verdict_out)) return fail(DH_EINVAL, "null argument");
    if (sig_stride < sl || sig_stride % 4) return fail(DH_EINVAL, "bad signature stride %zu", sig_stride);
    if (n >= n_limit || n_keys > ((size_t)1 << 24)) return fail(DH_EINVAL, "batch too large");
    kidx.assign(n, 0);
    off.assign(n + 1, 0);
    std::vector<uint8_t> used(n_keys, 0);
    for (size_t i = 0; i < n; i++) {
      if (msg_off[i + 1] < msg_off[i]) return fail(DH_EINVAL, "msg_off must be non-decreasing");
      const uint32_t k = key_idx ? key_idx[i] : (uint32_t)i;
      if (k >= n_keys) return fail(DH_EINVAL, "item %zu: key index %u outside the table of %zu keys", i, k, n_keys);
      kidx[i] = k;
      off[i + 1] = msg_off[i + 1] - msg_off[0];
      if (!used[k]) used[k] = 1, keys_used++;
    }
    if (off[n] && !msgs) return fail(DH_EINVAL, "null messages");
    return DH_OK;
  }
};

int dh_bls_verify_batch(int scheme, const uint8_t* keys, size_t n_keys, const uint32_t* key_idx, const uint8_t* msgs,
                        const uint32_t* msg_off, const uint8_t* sigs, size_t sig_stride, size_t n, uint8_t* verdict_out,
                        uint8_t* key_ok_out, uint64_t seed, uint64_t stats_out[4]) {
  if (scheme < 0 || scheme > 3) return fail(DH_EINVAL, "unknown scheme %d", scheme);
  const bool g2 = sig_on_g2(scheme);
  const size_t sl = g2 ? 96 : 48;
  if (stats_out) memset(stats_out, 0, 4 * sizeof(uint64_t));
  // entries of the MSM's sorted list keep a sign bit and address parts * n points; the key table feeds int-sized kernels
  keyed_items it;
  int rc = it.check(keys, n_keys, key_idx, msgs, msg_off, sigs, sig_stride, sl, n, ((size_t)1 << 31) / (g2 ? 4 : 2), verdict_out);
  if (rc || n == 0) return rc;
  lease L;
  if (L.rc) return L.rc;
  if ((rc = set_device_and_stream(L.w))) return rc;
  rc = auth_core(L.w, scheme, keys, n_keys, it.kidx.data(), it.keys_used, msgs ? msgs + msg_off[0] : nullptr, it.off.data(), sigs, sig_stride,
                 n, verdict_out, key_ok_out, seed, stats_out, L.w->stream);
  if (rc) (void)hipStreamSynchronize(L.w->stream);  // nothing of this call stays queued on the worker
  return rc;
}

int dh_schnorr_sig_len(int scheme) {
  const int kl = dh_key_len(scheme);
  return kl < 0 ? kl : kl + 32;
}

int dh_schnorr_verify_batch(int scheme, const uint8_t* keys, size_t n_keys, const uint32_t* key_idx, const uint8_t* msgs,
                            const uint32_t* msg_off, const uint8_t* sigs, size_t sig_stride, size_t n, uint8_t* verdict_out,
                            uint8_t* key_ok_out) {
  if (scheme < 0 || scheme > 3) return fail(DH_EINVAL, "unknown scheme %d", scheme);
  const size_t sl = (size_t)dh_schnorr_sig_len(scheme);
  keyed_items it;
  int rc = it.check(keys, n_keys, key_idx, msgs, msg_off, sigs, sig_stride, sl, n, (size_t)1 << 31, verdict_out);
  if (rc || n == 0) return rc;
  lease L;
  if (L.rc) return L.rc;
  if ((rc = set_device_and_stream(L.w))) return rc;
  rc = schnorr_core(L.w, scheme, keys, n_keys, it.kidx.data(), msgs ? msgs + msg_off[0] : nullptr, it.off.data(), sigs, sig_stride, n,
                    verdict_out, key_ok_out, L.w->stream);
  if (rc) (void)hipStreamSynchronize(L.w->stream);  // nothing of this call stays queued on the worker
  return rc;
}

int dh_identity_hash_batch(int scheme, const uint8_t* keys, size_t n, uint8_t* out32) {
  const int kl = dh_key_len(scheme);
  if (kl < 0) return kl;
  if (n && (!keys || !out32)) return fail(DH_EINVAL, "null argument");
  for (size_t i = 0; i < n; i++) blake2b_256(keys + i * (size_t)kl, (size_t)kl, out32 + 32 * i);
  return DH_OK;
}

int dh_identity_verify_batch(int scheme, const uint8_t* keys, const uint8_t* sigs, size_t sig_stride, size_t n,
                             uint8_t* verdict_out) {
  std::vector<uint8_t> msgs(n * 32);
  std::vector<uint32_t> off(n + 1);
  int rc = dh_identity_hash_batch(scheme, keys, n, msgs.data());
  if (rc) return rc;
  for (size_t i = 0; i <= n; i++) off[i] = (uint32_t)(32 * i);
  return dh_bls_verify_batch(scheme, keys, n, nullptr, msgs.data(), off.data(), sigs, sig_stride, n, verdict_out, nullptr, 0,
                             nullptr);
}

static void sk_words(const uint8_t* sk32, uint32_t w[8]) {
  for (int i = 0; i < 8; i++) {
    const uint8_t* q = sk32 + 28 - 4 * i;
    w[i] = (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | q[3];
  }
}

int dh_sign_batch(int scheme, const uint8_t* sk32, const uint64_t* rounds, const uint8_t* prevs, size_t n,
                  const uint32_t* prev_lens, size_t prev_stride, uint8_t* sigs_out) {
  int sl = dh_sig_len(scheme);
  if (sl < 0) return sl;
  if (!sk32 || (n && (!rounds || !sigs_out))) return fail(DH_EINVAL, "null argument");
  if (n == 0) return DH_OK;
  const bool chained = scheme == DH_SCHEME_CHAINED && prevs;
  lease L;
  if (L.rc) return L.rc;
  worker* w = L.w;
  int rc = set_device_and_stream(w);
  if (rc) return rc;
  hipStream_t st = w->stream;
  uint32_t skw[8];
  sk_words(sk32, skw);
  HIP_TRY(w->key_ok.ensure(64));
  HIP_TRY(w->in_rounds.ensure(n * 8));
  HIP_TRY(w->in_sigs.ensure(n * sl));
  HIP_TRY(hipMemcpyAsync(w->key_ok.p, skw, 32, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w->in_rounds.p, rounds, n * 8, hipMemcpyHostToDevice, st));
  if (chained) {
    HIP_TRY(w->in_prevs.ensure(n * prev_stride + 4));
    HIP_TRY(hipMemcpyAsync(w->in_prevs.p, prevs, n * prev_stride, hipMemcpyHostToDevice, st));
    if (prev_lens) {
      for (size_t i = 0; i < n; i++)
        if (prev_lens[i] > prev_stride)
          return fail(DH_EINVAL, "previous signature %zu: length %u exceeds the record stride %zu", i, prev_lens[i], prev_stride);
      HIP_TRY(w->in_prev_lens.ensure(n * 4));
      HIP_TRY(hipMemcpyAsync(w->in_prev_lens.p, prev_lens, n * 4, hipMemcpyHostToDevice, st));
    }
  }
  if (sl == 96) {
    HIP_TRY(w->q_pts.ensure(n * JAC_WORDS_G2 * 4));
    HIP_TRY(w->h2c_tmp.ensure(dh::hash_tmp_bytes(1, n)));
  }
  HIP_TRY(dh::launch_sign(sl == 96, w->key_ok.as<uint32_t>(), w->in_rounds.as<uint64_t>(),
                          chained ? w->in_prevs.as<uint8_t>() : nullptr, prev_stride,
                          chained && prev_lens ? w->in_prev_lens.as<uint32_t>() : nullptr, nullptr, n, chained ? 1 : 0,
                          dst_id(scheme), w->in_sigs.as<uint8_t>(), w->q_pts.as<uint32_t>(), w->h2c_tmp.as<uint32_t>(), st));
  HIP_TRY(hipMemcpyAsync(sigs_out, w->in_sigs.p, n * sl, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DH_OK;
}

int dh_hash_to_curve(int group, const uint8_t* msgs, const uint32_t* msg_off, size_t n, const uint8_t* dst, size_t dst_len,
                     uint8_t* out) {
  if (group != 1 && group != 2) return fail(DH_EINVAL, "group must be 1 (G1) or 2 (G2)");
  if (!msg_off || !out || (n && !msgs) || !dst || dst_len == 0 || dst_len > 255)
    return fail(DH_EINVAL, "bad hash_to_curve arguments (DST must be 1..255 bytes)");
  if (n == 0) return DH_OK;
  size_t maxm = 0;
  for (size_t i = 0; i < n; i++) {
    if (msg_off[i + 1] < msg_off[i]) return fail(DH_EINVAL, "msg_off must be non-decreasing");
    maxm = std::max<size_t>(maxm, msg_off[i + 1] - msg_off[i]);
  }
  const size_t total = msg_off[n] - msg_off[0];
  const size_t stride = (64 + maxm + 4 + dst_len + 63) & ~(size_t)63;
  const size_t outlen = group == 1 ? 48 : 96;
  std::vector<uint32_t> off(n + 1);
  for (size_t i = 0; i <= n; i++) off[i] = msg_off[i] - msg_off[0];
  lease L;
  if (L.rc) return L.rc;
  worker* w = L.w;
  int rc = set_device_and_stream(w);
  if (rc) return rc;
  hipStream_t st = w->stream;
  HIP_TRY(w->in_sigs.ensure(total + 4));
  HIP_TRY(w->in_prev_lens.ensure((n + 1) * 4));
  HIP_TRY(w->key_raw.ensure(256));
  HIP_TRY(w->h2c_tmp.ensure(n * stride));
  HIP_TRY(w->out_rand.ensure(n * outlen));
  if (total) HIP_TRY(hipMemcpyAsync(w->in_sigs.p, msgs + msg_off[0], total, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w->in_prev_lens.p, off.data(), (n + 1) * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w->key_raw.p, dst, dst_len, hipMemcpyHostToDevice, st));
  HIP_TRY(dh::launch_h2c_generic(group == 2, w->in_sigs.as<uint8_t>(), w->in_prev_lens.as<uint32_t>(), n,
                                 w->key_raw.as<uint8_t>(), (uint32_t)dst_len, w->h2c_tmp.as<uint8_t>(), stride,
                                 w->out_rand.as<uint8_t>(), st));
  HIP_TRY(hipMemcpyAsync(out, w->out_rand.p, n * outlen, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DH_OK;
}

// 48 big-endian bytes < p
static bool fp_bytes_canonical(const uint8_t* b) {
  static const uint8_t P[48] = {0x1a, 0x01, 0x11, 0xea, 0x39, 0x7f, 0xe6, 0x9a, 0x4b, 0x1b, 0xa7, 0xb6, 0x43, 0x4b, 0xac, 0xd7,
                                0x64, 0x77, 0x4b, 0x84, 0xf3, 0x85, 0x12, 0xbf, 0x67, 0x30, 0xd2, 0xa0, 0xf6, 0xb0, 0xf6, 0x24,
                                0x1e, 0xab, 0xff, 0xfe, 0xb1, 0x53, 0xff, 0xff, 0xb9, 0xfe, 0xff, 0xff, 0xff, 0xff, 0xaa, 0xab};
  return memcmp(b, P, 48) < 0;
}

// the fused per-round G1 kernel on given field elements; late: the form that leaves the isogeny to the MSM (28-bit
// columns beside the points)
static int g1_round_prep_debug(bool late, const uint8_t* us, const uint8_t* sigs, size_t n, uint8_t* status_out, uint8_t* sig_out,
                               uint8_t* hash_out) {
  if (!us || !sigs || !status_out || !sig_out || !hash_out) return fail(DH_EINVAL, "null argument");
  if (n == 0) return DH_OK;
  for (size_t i = 0; i < 2 * n; i++)
    if (!fp_bytes_canonical(us + 48 * i)) return fail(DH_EINVAL, "field element %zu is not below p", i);
  lease L;
  if (L.rc) return L.rc;
  worker* w = L.w;
  int rc = set_device_and_stream(w);
  if (rc) return rc;
  hipStream_t st = w->stream;
  HIP_TRY(w->in_prevs.ensure(n * 96));
  HIP_TRY(w->in_sigs.ensure(n * 48));
  HIP_TRY(w->status.ensure(n));
  HIP_TRY(w->sig_aff.ensure(n * JAC_WORDS_G1 * 2 / 3 * 4));
  HIP_TRY(w->q_pts.ensure(n * JAC_WORDS_G1 * 4));
  if (late) {
    HIP_TRY(w->s28.ensure(n * 32 * 4));
    HIP_TRY(w->q28.ensure(n * 32 * 4));
  }
  HIP_TRY(w->out_rand.ensure(n * 192));
  HIP_TRY(hipMemcpyAsync(w->in_prevs.p, us, n * 96, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w->in_sigs.p, sigs, n * 48, hipMemcpyHostToDevice, st));
  uint8_t* out = w->out_rand.as<uint8_t>();
  if (late)
    HIP_TRY(dh::launch_round_g1_ride_late_debug(w->in_prevs.as<uint8_t>(), w->in_sigs.as<uint8_t>(), n, w->status.as<uint8_t>(),
                                                w->sig_aff.as<uint32_t>(), w->q_pts.as<uint32_t>(), w->s28.as<uint32_t>(),
                                                w->q28.as<uint32_t>(), out, out + n * 96, st));
  else
    HIP_TRY(dh::launch_round_g1_ride_debug(w->in_prevs.as<uint8_t>(), w->in_sigs.as<uint8_t>(), n, w->status.as<uint8_t>(),
                                           w->sig_aff.as<uint32_t>(), w->q_pts.as<uint32_t>(), out, out + n * 96, st));
  HIP_TRY(hipMemcpyAsync(status_out, w->status.p, n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(sig_out, out, n * 96, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(hash_out, out + n * 96, n * 96, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DH_OK;
}

int dh_g1_round_prep_debug(const uint8_t* us, const uint8_t* sigs, size_t n, uint8_t* status_out, uint8_t* sig_out,
                           uint8_t* hash_out) {
  return g1_round_prep_debug(false, us, sigs, n, status_out, sig_out, hash_out);
}

int dh_g1_round_prep_late_debug(const uint8_t* us, const uint8_t* sigs, size_t n, uint8_t* status_out, uint8_t* sig_out,
                                uint8_t* hash_out) {
  return g1_round_prep_debug(true, us, sigs, n, status_out, sig_out, hash_out);
}

int dh_field_ops_debug(const uint32_t* ops, const uint32_t* in, size_t in_words, size_t n, uint32_t* out, size_t out_words) {
  if (n == 0) return DH_OK;
  if (!ops || !in || !out) return fail(DH_EINVAL, "null argument");
  if (in_words < dh::FO_IN_WORDS) return fail(DH_EINVAL, "operand records of %zu words: at least %zu", in_words, dh::FO_IN_WORDS);
  if (out_words < dh::FO_OUT_WORDS) return fail(DH_EINVAL, "result records of %zu words: at least %zu", out_words, dh::FO_OUT_WORDS);
  if (in_words > 4096 || out_words > 4096 || n > ((size_t)1 << 24)) return fail(DH_EINVAL, "records above 4096 words or more than 2^24 lanes");
  for (size_t i = 0; i < n; i++)
    if (!dh::field_op_known(ops[i])) return fail(DH_EINVAL, "lane %zu: unknown field op %u", i, ops[i]);
  lease L;
  if (L.rc) return L.rc;
  worker* w = L.w;
  int rc = set_device_and_stream(w);
  if (rc) return rc;
  hipStream_t st = w->stream;
  HIP_TRY(w->in_sigs.ensure(n * 4));
  HIP_TRY(w->in_prevs.ensure(n * in_words * 4));
  HIP_TRY(w->out_rand.ensure(n * out_words * 4));
  HIP_TRY(hipMemcpyAsync(w->in_sigs.p, ops, n * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w->in_prevs.p, in, n * in_words * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(w->out_rand.p, 0, n * out_words * 4, st));
  HIP_TRY(dh::launch_field_ops(w->in_sigs.as<uint32_t>(), w->in_prevs.as<uint32_t>(), in_words, n, w->out_rand.as<uint32_t>(),
                               out_words, st));
  HIP_TRY(hipMemcpyAsync(out, w->out_rand.p, n * out_words * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DH_OK;
}

// the caller's program of dh_vm_debug, as k_vm.hip's decoder reads it: nothing it loads may lie outside the buffers
static int vm_debug_check_program(const uint32_t* phases, size_t nphases, const uint32_t* ops, size_t nops, size_t nslots) {
  constexpr size_t REC = dh::VM_DEBUG_REC, MAXT = dh::VM_DEBUG_MAXT, HALF = REC / 2;
  std::vector<uint8_t> written(nslots);
  size_t first = 0;
  for (size_t ph = 0; ph < nphases; ph++) {
    const uint32_t d = phases[2 * ph], kind = d & 0xff, cnt = d >> 8;
    if (kind > 2) return fail(DH_EINVAL, "phase %zu: kind %u", ph, kind);
    if (cnt > 64) return fail(DH_EINVAL, "phase %zu: %u ops, at most 64", ph, cnt);
    if (kind == 2 && cnt != 1) return fail(DH_EINVAL, "phase %zu: an INV phase of %u ops", ph, cnt);
    if (phases[2 * ph + 1] != first) return fail(DH_EINVAL, "phase %zu: first op %u is not the running sum %zu", ph, phases[2 * ph + 1], first);
    if (first + cnt > nops) return fail(DH_EINVAL, "phase %zu: its ops end at %zu of %zu", ph, first + cnt, nops);
    std::fill(written.begin(), written.end(), 0);
    for (size_t k = 0; k < cnt; k++) {
      const uint32_t* r = ops + REC * (first + k);
      const uint32_t dst = r[0] & 0xffffu, na = (r[0] >> 16) & 0xff, nb = r[0] >> 24;
      if (na > MAXT || nb > MAXT) return fail(DH_EINVAL, "op %zu: %u + %u terms, at most %zu a half", first + k, na, nb, MAXT);
      if (r[HALF] != nb << 16) return fail(DH_EINVAL, "op %zu: word 16 is not the second half's count", first + k);
      if (kind == 2 && nb) return fail(DH_EINVAL, "op %zu: an INV op with a second half", first + k);
      if (dst >= nslots) return fail(DH_EINVAL, "op %zu: slot index %u of %zu", first + k, dst, nslots);
      if (written[dst]) return fail(DH_EINVAL, "phase %zu: two ops write slot %u", ph, dst);
      written[dst] = 1;
      for (size_t j = 0; j < MAXT; j++)
        for (size_t h = 0; h < 2; h++) {
          const uint32_t t = r[1 + HALF * h + j];
          if (j >= (h ? nb : na) && t) return fail(DH_EINVAL, "op %zu: a term word past its half's count is not 0", first + k);
          if ((t & 0xffffu) >= nslots) return fail(DH_EINVAL, "op %zu: slot index %u of %zu", first + k, t & 0xffffu, nslots);
        }
    }
    for (size_t k = 0; k < cnt; k++) {
      const uint32_t* r = ops + REC * (first + k);
      const uint32_t na = (r[0] >> 16) & 0xff, nb = r[0] >> 24;
      for (size_t j = 0; j < MAXT; j++)
        if ((j < na && written[r[1 + j] & 0xffffu]) || (j < nb && written[r[1 + HALF + j] & 0xffffu]))
          return fail(DH_EINVAL, "phase %zu: op %zu reads a slot the phase writes", ph, first + k);
    }
    first += cnt;
  }
  if (first != nops) return fail(DH_EINVAL, "%zu ops given, the phases hold %zu", nops, first);
  return DH_OK;
}

int dh_vm_debug(int tag, const uint32_t* phases, size_t nphases, const uint32_t* ops, size_t nops, size_t nslots, size_t stop,
                const uint32_t* in, size_t in_words, size_t n, uint32_t* out, size_t out_words) {
  if (n == 0) return DH_OK;
  dh::vm_debug_dims d;
  const bool committed = dh::vm_debug_shape(tag, &d);
  if (!committed && tag != -1) return fail(DH_EINVAL, "program tag %d: 0 to 7, or -1 for the caller's program", tag);
  if (!in || !out) return fail(DH_EINVAL, "null argument");
  if (n > ((size_t)1 << 16)) return fail(DH_EINVAL, "more than 65536 records");
  if (committed) {
    nphases = (size_t)d.nphases;
    nslots = (size_t)d.nslots;
    nops = 0;
    if (in_words != (size_t)d.in_words) return fail(DH_EINVAL, "input records of %zu words: the program takes %d", in_words, d.in_words);
  } else {
    if ((nphases && !phases) || (nops && !ops)) return fail(DH_EINVAL, "null argument");
    if (nphases > (size_t)d.nphases) return fail(DH_EINVAL, "%zu phases: at most %d", nphases, d.nphases);
    if (nslots == 0 || nslots > (size_t)d.nslots) return fail(DH_EINVAL, "%zu slots: 1 to %d", nslots, d.nslots);
    if (nops > 64 * nphases) return fail(DH_EINVAL, "%zu ops given, the phases hold at most %zu", nops, 64 * nphases);
    if (in_words != nslots * dh::VM_DEBUG_SLOT_WORDS)
      return fail(DH_EINVAL, "slot images of %zu words: %zu slots take %zu", in_words, nslots, nslots * dh::VM_DEBUG_SLOT_WORDS);
    int rc = vm_debug_check_program(phases, nphases, ops, nops, nslots);
    if (rc) return rc;
  }
  if (stop > nphases) return fail(DH_EINVAL, "stop %zu beyond the program's %zu phases", stop, nphases);
  if (out_words != nslots * dh::VM_DEBUG_SLOT_WORDS)
    return fail(DH_EINVAL, "result records of %zu words: %zu slots take %zu", out_words, nslots, nslots * dh::VM_DEBUG_SLOT_WORDS);
  lease L;
  if (L.rc) return L.rc;
  worker* w = L.w;
  int rc = set_device_and_stream(w);
  if (rc) return rc;
  hipStream_t st = w->stream;
  const size_t op_bytes = (nops * dh::VM_DEBUG_REC + dh::VM_DEBUG_REC / 2) * 4;  // the records, then the 16 pad words
  HIP_TRY(w->in_sigs.ensure(2 * nphases * 4 + 4));
  HIP_TRY(w->in_prevs.ensure(op_bytes));  // hipMalloc's alignment (256 bytes) is the records' 16
  HIP_TRY(w->in_rounds.ensure(n * in_words * 4));
  HIP_TRY(w->out_rand.ensure(n * out_words * 4));
  if (!committed) {
    if (nphases) HIP_TRY(hipMemcpyAsync(w->in_sigs.p, phases, 2 * nphases * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(w->in_prevs.p, 0, op_bytes, st));
    if (nops) HIP_TRY(hipMemcpyAsync(w->in_prevs.p, ops, nops * dh::VM_DEBUG_REC * 4, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(hipMemcpyAsync(w->in_rounds.p, in, n * in_words * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(w->out_rand.p, 0, n * out_words * 4, st));
  HIP_TRY(dh::launch_vm_debug(tag, w->in_sigs.as<uint32_t>(), (int)nphases, w->in_prevs.as<uint32_t>(), (int)nslots, (int)stop,
                              w->in_rounds.as<uint32_t>(), in_words, n, w->out_rand.as<uint32_t>(), st));
  HIP_TRY(hipMemcpyAsync(out, w->out_rand.p, n * out_words * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DH_OK;
}

int dh_msm_level0_shape_debug(uint64_t* rows_per_set, uint64_t* entries, int* half_a, int* half_b) {
  if (!rows_per_set || !entries || !half_a || !half_b) return fail(DH_EINVAL, "null argument");
  *rows_per_set = g_level0.rows;
  *entries = g_level0.entries;
  *half_a = g_level0.half_a;
  *half_b = g_level0.half_b;
  return DH_OK;
}

int dh_public_key(int scheme, const uint8_t* sk32, uint8_t* key_out) {
  int kl = dh_key_len(scheme);
  if (kl < 0) return kl;
  if (!sk32 || !key_out) return fail(DH_EINVAL, "null argument");
  lease L;
  if (L.rc) return L.rc;
  worker* w = L.w;
  int rc = set_device_and_stream(w);
  if (rc) return rc;
  hipStream_t st = w->stream;
  uint32_t skw[8];
  sk_words(sk32, skw);
  HIP_TRY(w->key_ok.ensure(64));
  HIP_TRY(w->key_raw.ensure(96));
  HIP_TRY(hipMemcpyAsync(w->key_ok.p, skw, 32, hipMemcpyHostToDevice, st));
  HIP_TRY(dh::launch_pubkey(kl == 96, w->key_ok.as<uint32_t>(), w->key_raw.as<uint8_t>(), st));
  HIP_TRY(hipMemcpyAsync(key_out, w->key_raw.p, kl, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DH_OK;
}

}  // extern "C"

// ---- trimmed bbolt store on the device: chain/boltdb/trimmed.go's read path and the CheckPastBeacons
// loop over it (chain/beacon/sync_manager.go:170-235). The file image is uploaded once per open store; a window's
// columns are cut from it by k_bolt.hip in the layout dh_verify_batch_device takes, previous signatures included.

static size_t store_max_bytes() {  // read at every call
  return env_size("DRANDHIP_STORE_MAX_BYTES", (size_t)16 << 30, 1);
}

struct prof_wall {  // host wall time of one store stage (each ends in a stream wait), recorded when profiling is on
  const char* name;
  std::chrono::steady_clock::time_point t0;
  explicit prof_wall(const char* n) : name(n), t0(std::chrono::steady_clock::now()) {}
  ~prof_wall() {
    if (g_prof.on.load(std::memory_order_relaxed))
      g_prof.add(name, std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
};

// The windowed writer: rows arrive in windows; the leaves a window closes are packed and emitted, the
// open leaf's rows are carried to the next window in one of two carry sets (the pack and the carry-out of a window read
// set `cur` and write the other), the branch levels and pages 0-3 are written at the end.
struct bw_plan {  // what decides the layout of the rows to come; the host's 16 bytes per leaf are in bw_state
  std::vector<uint32_t> carry_need;  // record sizes of the open leaf's rows: at most P - 40 bytes, below MAX_LEAF_RECS rows
  uint64_t next_page = dh::boltw::FIRST_LEAF_PAGE, leaves = 0, rows = 0;
};
struct bw_window {  // one window's plan
  std::vector<uint32_t> sums;  // exclusive sums over (carried rows || new rows)
  std::vector<dh::boltw::leaf_desc> leaves;
  std::vector<uint64_t> keys;  // the closed leaves' first keys, downloaded
  uint64_t m = 0, open_row = 0, next_page = 0;
};
struct bw_state {
  uint32_t P = 0;
  bw_plan plan;
  bool has_last = false, finished = false;
  uint64_t call_base = 0;  // a one-shot call: the bytes of its image in front of the window's run (DRANDHIP_STORE_MAX_BYTES)
  int cur = 0;
  size_t carry_stride = 4;
  struct carry_set {
    dbuf rounds, rows, lens, last;  // last: {u64 round, u64 length, value bytes} of the last row appended
  } set[2];
  static_assert(dh::boltw::MAX_LEAF_RECS * 24 + 16 >= 65536 - 24, "an open leaf (at most P - 24 bytes) stays below MAX_LEAF_RECS rows");
  dbuf need, sums, scan_tmp, err, leaves, image, keys;
  std::vector<uint64_t> h_keys, h_pgids;  // first key and page of every closed leaf
  bw_window win;
  void reset(uint32_t page_size) {
    P = page_size;
    plan = bw_plan();
    has_last = finished = false;
    call_base = 0;
    h_keys.clear();
    h_pgids.clear();
  }
  void release() {
    for (dbuf* b : {&need, &sums, &scan_tmp, &err, &leaves, &image, &keys, &set[0].rounds, &set[0].rows, &set[0].lens, &set[0].last,
                    &set[1].rounds, &set[1].rows, &set[1].lens, &set[1].last})
      b->release();
  }
};

// device scratch of dh_store_save_trimmed: the uploaded patches, the merge's slots and the merged columns
struct write_ws {
  bw_state bw;
  dbuf scan_tmp, err, pred[2];  // pred: the sizing pass's last merged row (the layout of carry_out.last)
  dbuf p_rounds, p_rows, p_lens, flag, lb, pos, hit, o_rounds, o_rows, o_lens, o_src, unl;
  void release() {
    bw.release();
    for (dbuf* b : {&scan_tmp, &err, &pred[0], &pred[1], &p_rounds, &p_rows, &p_lens, &flag, &lb, &pos, &hit, &o_rounds, &o_rows, &o_lens, &o_src, &unl})
      b->release();
  }
};

// What dh_store, dh_bolt_writer and dh_archive share: locking, and their lifetime across dh_shutdown
struct dh_handle {
  std::mutex mu;                    // calls on one handle are serialised
  std::atomic<bool> retire{false};  // dh_shutdown ran while a call held the handle: that call (or the next) releases
  bool dead = false;                // device memory released by dh_shutdown: every call fails, dh_*_close frees
  hipStream_t st = nullptr;
  virtual ~dh_handle() = default;
  virtual void release_buffers() = 0;
  void release() {
    release_buffers();
    if (st) (void)hipStreamDestroy(st);
    st = nullptr;
    dead = true;
  }
};
static std::mutex g_stores_mu;
static std::vector<dh_handle*> g_handles;  // every open store, writer and archive, under g_stores_mu

// dh_shutdown: idle handles lose their device memory now, a handle inside a call when that call ends
static void handles_shutdown() {
  std::lock_guard<std::mutex> lk(g_stores_mu);
  for (dh_handle* h : g_handles) {
    if (h->mu.try_lock()) {
      h->release();
      h->mu.unlock();
    } else {
      h->retire = true;
    }
  }
}

static void handle_register(dh_handle* h) {
  std::lock_guard<std::mutex> lk(g_stores_mu);
  g_handles.push_back(h);
}

// entered with h->mu held; what / close_fn: the handle's word and its close function in the refusal
static int handle_enter(dh_handle* h, const char* what, const char* close_fn) {
  if (h->retire.exchange(false)) h->release();
  if (h->dead) return fail(DH_EINVAL, "%s handle invalidated by dh_shutdown (%s it and open again)", what, close_fn);
  HIP_TRY(hipSetDevice(g_ctx.device));
  return DH_OK;
}
struct handle_guard {
  dh_handle* h;
  explicit handle_guard(dh_handle* x) : h(x) { h->mu.lock(); }
  ~handle_guard() {
    if (h->retire.exchange(false)) h->release();
    h->mu.unlock();
  }
};

static void handle_close(dh_handle* h) {
  if (!h) return;
  {
    std::lock_guard<std::mutex> lk(g_stores_mu);
    g_handles.erase(std::remove(g_handles.begin(), g_handles.end(), h), g_handles.end());
  }
  {
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->dead && hipSetDevice(g_ctx.device) == hipSuccess) h->release();
  }
  delete h;
}

struct dh_store : dh_handle {
  size_t len = 0;
  uint32_t page_size = 0;
  uint64_t stat[6] = {0, 0, 0, 0, 0, 0};
  int format = DH_STORE_TRIMMED;          // fixed at open
  uint64_t jstat[3] = {0, 0, 0};          // untrimmed: deferred records, longest decoded Signature / PreviousSig
  std::vector<dh::bolt::leaf_json> jinfo;  // untrimmed: the hexjson scan's table
  std::vector<dh::bolt::leaf_info> info;  // the scan's table, one record per leaf in key order
  std::vector<uint32_t> rleaf;            // the leaves that hold rounds (ascending first / last): the search index
  dbuf d_file, d_leaves, d_info, err, cnt, base, scan_tmp, rounds, rows, lens, miss_prev, gap, moff, missing, verdict, bad;
  dbuf d_jinfo, prevs, prev_lens, defer;  // untrimmed: rows / lens above hold the decoded Signature column
  std::vector<uint8_t> h_defer;
  std::vector<uint8_t> h_bad;
  std::vector<uint64_t> h_rounds, h_missing;
  write_ws wws;  // dh_store_save_trimmed
  void release_buffers() override {
    wws.release();
    for (dbuf* b : {&d_file, &d_leaves, &d_info, &err, &cnt, &base, &scan_tmp, &rounds, &rows, &lens, &miss_prev, &gap, &moff,
                    &missing, &verdict, &bad, &d_jinfo, &prevs, &prev_lens, &defer})
      b->release();
  }
};
struct dh_bolt_writer : dh_handle {
  bw_state bw;
  void release_buffers() override { bw.release(); }
};
static int store_enter(dh_store* s) { return handle_enter(s, "store", "dh_store_close"); }
static int writer_enter(dh_bolt_writer* w) { return handle_enter(w, "writer", "dh_bolt_writer_close"); }

static int bolt_index(const uint8_t* file, size_t len, dh::bolt::meta* m, std::vector<dh::bolt::leaf_ref>* leaves) {
  using namespace dh::bolt;
  const view f{file, (uint64_t)len};
  uint32_t rc = bolt_meta(f, m);
  if (!rc) rc = bolt_find_bucket(f, *m, (const uint8_t*)"beacons", 7, leaves);
  if (rc) return fail(DH_ECORRUPT, "bbolt store: %s", err_name(rc));
  return DH_OK;
}

// shouldUseTrimmedBolt (chain/boltdb/store.go:82-110) on the first value of the bucket: a canonical hexjson record ->
// untrimmed; an empty bucket or any other value -> trimmed, except that a value starting with '{' that is not
// canonical is not decided here
static int store_detect(const uint8_t* file, const std::vector<dh::bolt::leaf_ref>& leaves, int* format) {
  using namespace dh::bolt;
  *format = DH_STORE_TRIMMED;
  for (const leaf_ref& lr : leaves) {
    const view leaf{file + lr.off, lr.ext};
    uint32_t count = 0;
    if (bolt_leaf_head(leaf, &count)) return DH_OK;  // the scan names the defect
    for (uint32_t i = 0; i < count; i++) {
      elem e;
      if (bolt_leaf_elem(leaf, i, &e)) return DH_OK;
      if (e.flags & F_BUCKET) continue;
      hexjson h;
      if (e.ksize == 8 && hexjson_parse(elem_value(leaf, e), rd64be(leaf, e.koff), &h)) {
        *format = DH_STORE_UNTRIMMED;
      } else if (e.vsize && leaf.p[e.koff + e.ksize] == '{') {
        return fail(DH_EINVAL, "bbolt store: the first value starts with '{' but is not a canonical hexjson beacon: name the format");
      }
      return DH_OK;
    }
  }
  return DH_OK;
}

static int store_open(dh_store* s, const uint8_t* file, size_t len, int format) {
  using namespace dh::bolt;
  meta m;
  std::vector<leaf_ref> leaves;
  {
    prof_wall p("store_index");
    int rc = bolt_index(file, len, &m, &leaves);
    if (rc) return rc;
    if (format == DH_STORE_AUTO && (rc = store_detect(file, leaves, &format))) return rc;
  }
  s->format = format;
  int rc = ensure_device();
  if (rc) return rc;
  const size_t nl = leaves.size();
  s->len = len;
  s->page_size = m.page_size;
  HIP_TRY(hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking));
  {
    prof_wall p("store_upload");
    HIP_TRY(s->d_file.ensure(len));
    HIP_TRY(hipMemcpyAsync(s->d_file.p, file, len, hipMemcpyHostToDevice, s->st));
    HIP_TRY(hipStreamSynchronize(s->st));
  }
  prof_wall p("store_scan");
  s->info.resize(nl);
  HIP_TRY(s->d_leaves.ensure(nl * sizeof(leaf_ref)));
  HIP_TRY(s->d_info.ensure(nl * sizeof(leaf_info)));
  HIP_TRY(s->err.ensure(4));
  uint32_t err_word = 0;
  HIP_TRY(hipMemcpyAsync(s->d_leaves.p, leaves.data(), nl * sizeof(leaf_ref), hipMemcpyHostToDevice, s->st));
  HIP_TRY(hipMemsetAsync(s->err.p, 0, 4, s->st));
  HIP_TRY(dh::launch_bolt_scan(s->d_file.as<uint8_t>(), s->d_leaves.p, nl, s->d_info.p, s->err.as<uint32_t>(), s->st));
  HIP_TRY(hipMemcpyAsync(s->info.data(), s->d_info.p, nl * sizeof(leaf_info), hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipMemcpyAsync(&err_word, s->err.p, 4, hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  uint64_t n_all = 0, n_round = 0, longest = 0;
  for (size_t i = 0; i < nl; i++) {
    const leaf_info& li = s->info[i];
    if (li.err) return fail(DH_ECORRUPT, "bbolt store: leaf %zu at offset %llu: %s", i, (unsigned long long)li.off, err_name(li.err));
    n_all += li.n_all;
    n_round += li.n_round;
    longest = std::max<uint64_t>(longest, li.max_vsize);
    if (!li.n_round) continue;
    if (!s->rleaf.empty() && s->info[s->rleaf.back()].last >= li.first)
      return fail(DH_ECORRUPT, "bbolt store: leaf %zu at offset %llu: %s", i, (unsigned long long)li.off, err_name(E_ORDER));
    s->rleaf.push_back((uint32_t)i);
  }
  if (err_word) return fail(DH_ECORRUPT, "bbolt store: %s", err_name(err_word));
  s->stat[0] = n_all;
  s->stat[1] = n_round;
  s->stat[2] = n_round ? s->info[s->rleaf.front()].first : 0;
  s->stat[3] = n_round ? s->info[s->rleaf.back()].last : 0;
  s->stat[4] = longest;
  s->stat[5] = nl;
  if (format != DH_STORE_UNTRIMMED) return DH_OK;
  s->jinfo.resize(nl);
  HIP_TRY(s->d_jinfo.ensure(nl * sizeof(leaf_json)));
  HIP_TRY(dh::launch_bolt_scan_json(s->d_file.as<uint8_t>(), s->d_leaves.p, nl, s->d_jinfo.p, s->st));
  HIP_TRY(hipMemcpyAsync(s->jinfo.data(), s->d_jinfo.p, nl * sizeof(leaf_json), hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  for (const leaf_json& lj : s->jinfo) {
    s->jstat[0] += lj.n_deferred;
    s->jstat[1] = std::max<uint64_t>(s->jstat[1], lj.max_sig);
    s->jstat[2] = std::max<uint64_t>(s->jstat[2], lj.max_prev);
  }
  return DH_OK;
}

// the window's leaves [lo, lo + nw), its row count (device count + scan; base stays in s->base) and its longest value
static int store_window(dh_store* s, uint64_t first, uint64_t last, size_t* lo, size_t* nw, size_t* total, uint32_t* longest) {
  *lo = *nw = *total = 0;
  *longest = 0;
  if (first > last) return DH_OK;
  const auto& rl = s->rleaf;
  // first leaf whose last round >= first; one past the last leaf whose first round <= last
  const size_t a = std::partition_point(rl.begin(), rl.end(), [&](uint32_t i) { return s->info[i].last < first; }) - rl.begin();
  const size_t b = std::partition_point(rl.begin(), rl.end(), [&](uint32_t i) { return s->info[i].first <= last; }) - rl.begin();
  if (a >= b) return DH_OK;
  *lo = rl[a];
  *nw = rl[b - 1] + 1 - rl[a];
  for (size_t i = *lo; i < *lo + *nw; i++) *longest = std::max(*longest, s->info[i].max_vsize);
  HIP_TRY(s->cnt.ensure(*nw * 4));
  HIP_TRY(s->base.ensure((*nw + 1) * 4));
  HIP_TRY(s->scan_tmp.ensure((*nw / 4096 + 2) * 4));
  HIP_TRY(dh::launch_bolt_count(s->d_file.as<uint8_t>(), s->d_leaves.as<dh::bolt::leaf_ref>() + *lo,
                                s->d_info.as<dh::bolt::leaf_info>() + *lo, *nw, first, last, s->cnt.as<uint32_t>(), s->st));
  HIP_TRY(dh::launch_scan(s->cnt.as<uint32_t>(), *nw, s->base.as<uint32_t>(), s->scan_tmp.as<uint32_t>(), s->st));
  uint32_t t = 0;
  HIP_TRY(hipMemcpyAsync(&t, s->base.as<uint32_t>() + *nw, 4, hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  *total = t;
  return DH_OK;
}

static size_t window_missing(uint64_t first, uint64_t last, size_t total) {
  if (first > last) return 0;
  const uint64_t span = last - first;  // rounds in the window, minus one
  if (total > span) return 0;  // every round of the window is stored
  if (span - total == UINT64_MAX) return SIZE_MAX;
  return (size_t)(span - total + 1);
}

// after store_window: the rows (total <= cap_rows), miss_prev into s->miss_prev, and the nmiss missing rounds into
// d_missing when it is given; waits for the stream
static int store_gather(dh_store* s, size_t lo, size_t nw, size_t total, uint64_t first, uint64_t last, size_t stride,
                        uint64_t* d_rounds, uint8_t* d_rows, uint32_t* d_lens, size_t cap_rows, uint64_t* d_missing, size_t nmiss) {
  if (total + 2 > (size_t)4096 * 4096) return fail(DH_EINVAL, "window of %zu rows: at most 16M rows per call", total);
  timed_launches tl(s->st);  // resolved after the stream wait below
  if (total)
    HIP_TRY(tl.run("k_bolt_gather", [&] {
      return dh::launch_bolt_gather(s->d_file.as<uint8_t>(), s->d_leaves.as<dh::bolt::leaf_ref>() + lo, s->base.as<uint32_t>(), nw, first,
                                    last, (uint32_t)stride, d_rounds, d_rows, d_lens, cap_rows, s->st);
    }));
  HIP_TRY(s->miss_prev.ensure(total + 1));
  HIP_TRY(s->gap.ensure((total + 1) * 4));
  HIP_TRY(dh::launch_bolt_link(d_rounds, total, first, last, s->miss_prev.as<uint8_t>(), s->gap.as<uint32_t>(), s->st));
  if (d_missing && nmiss) {
    HIP_TRY(s->moff.ensure((total + 2) * 4));
    HIP_TRY(s->scan_tmp.ensure(((total + 1) / 4096 + 2) * 4));
    HIP_TRY(dh::launch_scan(s->gap.as<uint32_t>(), total + 1, s->moff.as<uint32_t>(), s->scan_tmp.as<uint32_t>(), s->st));
    HIP_TRY(dh::launch_bolt_fill(d_rounds, total, first, s->moff.as<uint32_t>(), nmiss, d_missing, s->st));
  }
  HIP_TRY(hipStreamSynchronize(s->st));
  return DH_OK;
}

// the untrimmed form of store_gather: c.rounds is required, the other columns as launch_bolt_gather_json takes them
static int store_gather_json(dh_store* s, size_t lo, size_t nw, size_t total, uint64_t first, uint64_t last, const dh::json_cols& c,
                             uint64_t* d_missing, size_t nmiss) {
  if (total + 2 > (size_t)4096 * 4096) return fail(DH_EINVAL, "window of %zu rows: at most 16M rows per call", total);
  timed_launches tl(s->st);  // resolved after the stream wait below
  if (total)
    HIP_TRY(tl.run("k_bolt_gather_json", [&] {
      return dh::launch_bolt_gather_json(s->d_file.as<uint8_t>(), s->d_leaves.as<dh::bolt::leaf_ref>() + lo, s->base.as<uint32_t>(), nw,
                                         first, last, c, s->st);
    }));
  if (d_missing && nmiss) {
    HIP_TRY(s->miss_prev.ensure(total + 1));
    HIP_TRY(s->gap.ensure((total + 1) * 4));
    HIP_TRY(dh::launch_bolt_link(c.rounds, total, first, last, s->miss_prev.as<uint8_t>(), s->gap.as<uint32_t>(), s->st));
    HIP_TRY(s->moff.ensure((total + 2) * 4));
    HIP_TRY(s->scan_tmp.ensure(((total + 1) / 4096 + 2) * 4));
    HIP_TRY(dh::launch_scan(s->gap.as<uint32_t>(), total + 1, s->moff.as<uint32_t>(), s->scan_tmp.as<uint32_t>(), s->st));
    HIP_TRY(dh::launch_bolt_fill(c.rounds, total, first, s->moff.as<uint32_t>(), nmiss, d_missing, s->st));
  }
  HIP_TRY(hipStreamSynchronize(s->st));
  return DH_OK;
}

// the longest decoded Signature / PreviousSig in the leaves [lo, lo + nw)
static uint32_t window_longest_json(const dh_store* s, size_t lo, size_t nw) {
  uint32_t m = 0;
  for (size_t i = lo; i < lo + nw; i++) m = std::max(m, std::max(s->jinfo[i].max_sig, s->jinfo[i].max_prev));
  return m;
}

// store.Last() of a trimmed store: the largest round; the chained Get also needs the record before it
// (trimmed.go:156-193)
static int store_last_trimmed(dh_store* s, bool chained, uint64_t last_round) {
  if (!chained || !last_round) return DH_OK;
  size_t lo, nw, total;
  uint32_t longest;
  int rc = store_window(s, last_round - 1, last_round, &lo, &nw, &total, &longest);
  if (rc) return rc;
  if (total != 2) return fail(DH_ENOBEACON, "no beacon stored: round %llu, before the last", (unsigned long long)(last_round - 1));
  return DH_OK;
}

// Last() of an untrimmed store fails on an empty bucket only, but Last().Round is the last record's Round field: known
// here only when the record is canonical
static int store_last_json(dh_store* s, uint64_t last_round) {
  if (!s->jstat[0]) return DH_OK;
  size_t lo, nw, total;
  uint32_t longest;
  int rc = store_window(s, last_round, last_round, &lo, &nw, &total, &longest);
  if (rc) return rc;
  HIP_TRY(s->rounds.ensure(total * 8 + 8));
  HIP_TRY(s->defer.ensure(total + 8));
  const dh::json_cols c{s->rounds.as<uint64_t>(), s->defer.as<uint8_t>(), nullptr, nullptr, nullptr, nullptr, 4, 4, total};
  if ((rc = store_gather_json(s, lo, nw, total, last_round, last_round, c, nullptr, 0))) return rc;
  uint8_t d = 0;
  if (total) HIP_TRY(hipMemcpy(&d, s->defer.p, 1, hipMemcpyDeviceToHost));
  if (d)
    return fail(DH_EINVAL, "the last record (key %llu) is not canonical hexjson: Last() needs the host decoder",
                (unsigned long long)last_round);
  return DH_OK;
}

extern "C" {

int dh_bolt_index(const uint8_t* file, size_t len, uint32_t* page_size_out, uint64_t* leaf_off_out, size_t cap,
                  size_t* n_leaves_out) {
  if (!file || !n_leaves_out) return fail(DH_EINVAL, "null argument");
  dh::bolt::meta m;
  std::vector<dh::bolt::leaf_ref> leaves;
  int rc = bolt_index(file, len, &m, &leaves);
  if (rc) return rc;
  if (page_size_out) *page_size_out = m.page_size;
  *n_leaves_out = leaves.size();
  if (leaves.size() > cap || (leaves.size() && !leaf_off_out))
    return fail(DH_EINVAL, "%zu leaves, room for %zu", leaves.size(), cap);
  for (size_t i = 0; i < leaves.size(); i++) leaf_off_out[i] = leaves[i].off;
  return DH_OK;
}

int dh_store_open_bolt(const uint8_t* file, size_t len, dh_store** out) {
  return dh_store_open_bolt_format(file, len, DH_STORE_TRIMMED, out);
}

int dh_store_open_bolt_format(const uint8_t* file, size_t len, int format, dh_store** out) {
  if (!file || !out) return fail(DH_EINVAL, "null argument");
  *out = nullptr;
  if (format != DH_STORE_TRIMMED && format != DH_STORE_UNTRIMMED && format != DH_STORE_AUTO)
    return fail(DH_EINVAL, "unknown store format %d", format);
  if (len > store_max_bytes())
    return fail(DH_ENOMEM, "store file of %zu bytes exceeds DRANDHIP_STORE_MAX_BYTES (%zu): keep the host reader", len,
                store_max_bytes());
  dh_store* s = new dh_store();
  int rc = store_open(s, file, len, format);
  if (rc) {
    s->release();
    delete s;
    return rc;
  }
  handle_register(s);
  *out = s;
  return DH_OK;
}

int dh_store_stat(const dh_store* s, uint64_t out[6]) {
  if (!s || !out) return fail(DH_EINVAL, "null argument");
  memcpy(out, s->stat, sizeof s->stat);  // fixed at open
  return DH_OK;
}

int dh_store_format_stat(const dh_store* s, uint64_t out[4]) {
  if (!s || !out) return fail(DH_EINVAL, "null argument");
  out[0] = (uint64_t)s->format;  // fixed at open
  memcpy(out + 1, s->jstat, sizeof s->jstat);
  return DH_OK;
}

void dh_store_close(dh_store* s) { handle_close(s); }

int dh_store_columns_device(dh_store* s, uint64_t first, uint64_t last, size_t row_stride, uint64_t* d_rounds, uint8_t* d_rows,
                            uint32_t* d_lens, size_t cap_rows, size_t* n_rows_out, uint64_t* d_missing, size_t cap_missing,
                            size_t* n_missing_out, void* hip_stream) {
  if (!s || !n_rows_out) return fail(DH_EINVAL, "null argument");
  if (!row_stride || (row_stride & 3) || row_stride > ((size_t)1 << 20))
    return fail(DH_EINVAL, "row stride %zu: a positive multiple of 4, at most 1 MiB", row_stride);
  handle_guard g(s);
  int rc = store_enter(s);
  if (rc) return rc;
  prof_wall p("store_gather_link");
  if (hip_stream) HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));  // the output buffers may be in use there
  size_t lo, nw, total;
  uint32_t longest;
  if ((rc = store_window(s, first, last, &lo, &nw, &total, &longest))) return rc;
  const size_t nmiss = window_missing(first, last, total);
  *n_rows_out = total;
  if (n_missing_out) *n_missing_out = nmiss;
  if (total > cap_rows || (d_missing && nmiss > cap_missing))
    return fail(DH_EINVAL, "%zu rows and %zu missing rounds, room for %zu and %zu", total, nmiss, cap_rows, d_missing ? cap_missing : 0);
  if (total && (!d_rounds || !d_rows || !d_lens)) return fail(DH_EINVAL, "null output");
  if (d_missing && nmiss > 0xffffffffull) return fail(DH_EINVAL, "%zu missing rounds", nmiss);
  if (!total && !(d_missing && nmiss)) return DH_OK;
  return store_gather(s, lo, nw, total, first, last, row_stride, d_rounds, d_rows, d_lens, cap_rows, d_missing, nmiss);
}

int dh_store_check_past(dh_store* s, int scheme, const uint8_t* pk, size_t pk_len, uint64_t up_to, size_t window, uint64_t seed,
                        uint64_t* faulty_out, size_t cap, size_t* n_faulty_out,
                        void (*cb)(uint64_t round, uint64_t up_to, void* arg), void* cb_arg) {
  if (!s || !pk || !n_faulty_out || (cap && !faulty_out)) return fail(DH_EINVAL, "null argument");
  if (scheme < 0 || scheme > 3) return fail(DH_EINVAL, "unknown scheme %d", scheme);
  if (!window) return fail(DH_EINVAL, "window must be >= 1");
  const uint32_t sig_len = (uint32_t)dh_sig_len(scheme);
  const bool chained = scheme == DH_SCHEME_CHAINED;
  handle_guard g(s);
  int rc = store_enter(s);
  if (rc) return rc;
  *n_faulty_out = 0;
  const bool json = s->format == DH_STORE_UNTRIMMED;
  if (!s->stat[1]) return fail(DH_ENOBEACON, "no beacon stored");
  const uint64_t last_round = s->stat[3];
  if ((rc = json ? store_last_json(s, last_round) : store_last_trimmed(s, chained, last_round))) return rc;
  // What the formats do differently inside a window. Trimmed (trimmed.go:183): the previous signature of row i is row
  // i - 1 of the same buffer, nothing is copied twice, so a chained window is gathered from the carrier round a - 1,
  // which is not examined. Untrimmed (BoltStore's read path, chain/boltdb/store.go:172-210): PreviousSig is the record's
  // own field, so a missing round makes only itself faulty; a record that is not canonical is deferred (DH_DEFERRED).
  const bool carrier = chained && !json;
  const dbuf& prev_rows = json ? s->prevs : s->rows;
  const dbuf& prev_lens = json ? s->prev_lens : s->lens;
  auto gather = [&](size_t lo, size_t nw, size_t total, uint64_t g0, uint64_t b, size_t stride, size_t nmiss) {
    if (!json)
      return store_gather(s, lo, nw, total, g0, b, stride, s->rounds.as<uint64_t>(), s->rows.as<uint8_t>(), s->lens.as<uint32_t>(), total,
                          s->missing.as<uint64_t>(), nmiss);
    const dh::json_cols c{s->rounds.as<uint64_t>(), s->defer.as<uint8_t>(), s->rows.as<uint8_t>(), s->lens.as<uint32_t>(),
                          chained ? s->prevs.as<uint8_t>() : nullptr, chained ? s->prev_lens.as<uint32_t>() : nullptr,
                          (uint32_t)stride, (uint32_t)stride, total};
    return store_gather_json(s, lo, nw, total, g0, b, c, s->missing.as<uint64_t>(), nmiss);
  };
  auto fold = [&](size_t total, uint64_t a) {
    if (!json)
      return dh::launch_bolt_fold(s->rounds.as<uint64_t>(), s->lens.as<uint32_t>(), s->miss_prev.as<uint8_t>(), s->verdict.as<uint8_t>(),
                                  total, sig_len, chained ? 1 : 0, a, s->bad.as<uint8_t>(), s->st);
    return dh::launch_bolt_fold_json(s->lens.as<uint32_t>(), s->defer.as<uint8_t>(), s->verdict.as<uint8_t>(), total, sig_len,
                                     s->bad.as<uint8_t>(), s->st);
  };
  if (last_round < up_to) up_to = last_round;
  const uint64_t store_len = s->stat[0];
  if (store_len <= 1) return DH_OK;
  const uint64_t hi = std::min<uint64_t>(store_len - 1, std::max<uint64_t>(up_to, 1));  // the loop's i < len and i >= up_to
  size_t nf = 0, ndef = 0;
  auto emit = [&](uint64_t r) {
    if (nf < cap) faulty_out[nf] = r;
    nf++;
  };
  for (uint64_t a = 1; a <= hi;) {
    const uint64_t b = hi - a < window - 1 ? hi : a + (window - 1);
    if (cb) cb(a, up_to, cb_arg);
    const uint64_t g0 = carrier ? a - 1 : a;
    size_t lo, nw, total, nmiss, stride;
    {
      prof_wall p("store_gather_link");
      uint32_t longest;
      if ((rc = store_window(s, g0, b, &lo, &nw, &total, &longest))) return rc;
      if (json) longest = window_longest_json(s, lo, nw);  // rows hold the decoded fields
      stride = ((size_t)std::max(sig_len, longest) + 3) & ~(size_t)3;
      if (stride > 65536)
        return fail(DH_EINVAL, "row stride %zu above 64 KiB (a %u-byte %s in rounds %llu..%llu): keep the host reader", stride, longest,
                    json ? "field" : "record", (unsigned long long)g0, (unsigned long long)b);
      nmiss = window_missing(g0, b, total);
      HIP_TRY(s->rounds.ensure(total * 8 + 8));
      HIP_TRY(s->rows.ensure(total * stride + 8));
      HIP_TRY(s->lens.ensure(total * 4 + 4));
      if (json) HIP_TRY(s->defer.ensure(total + 8));
      if (json && chained) {
        HIP_TRY(s->prevs.ensure(total * stride + 8));
        HIP_TRY(s->prev_lens.ensure(total * 4 + 4));
      }
      HIP_TRY(s->missing.ensure(nmiss * 8 + 8));
      if ((rc = gather(lo, nw, total, g0, b, stride, nmiss))) return rc;
    }
    const size_t off = carrier && total ? 1 : 0, nver = total - off;
    if (nver) {
      prof_wall p("store_verify");
      HIP_TRY(s->verdict.ensure(nver));
      // a deferred row is verified as the all-zero record it was left as, and its verdict is not read
      rc = dh_verify_batch_device(scheme, pk, pk_len, s->rounds.as<uint64_t>() + off, s->rows.as<uint8_t>() + off * stride, stride,
                                  chained ? prev_rows.as<uint8_t>() : nullptr, stride, chained ? prev_lens.as<uint32_t>() : nullptr, nver,
                                  s->verdict.as<uint8_t>(), nullptr, seed, nullptr, nullptr);
      if (rc) return rc;
    }
    s->h_bad.resize(total);
    s->h_defer.resize(json ? total : 0);
    s->h_rounds.resize(total);
    s->h_missing.resize(nmiss);
    if (total) {
      HIP_TRY(s->bad.ensure(total));
      HIP_TRY(fold(total, a));
      HIP_TRY(hipMemcpyAsync(s->h_bad.data(), s->bad.p, total, hipMemcpyDeviceToHost, s->st));
      if (json) HIP_TRY(hipMemcpyAsync(s->h_defer.data(), s->defer.p, total, hipMemcpyDeviceToHost, s->st));
      HIP_TRY(hipMemcpyAsync(s->h_rounds.data(), s->rounds.p, total * 8, hipMemcpyDeviceToHost, s->st));
    }
    if (nmiss) HIP_TRY(hipMemcpyAsync(s->h_missing.data(), s->missing.p, nmiss * 8, hipMemcpyDeviceToHost, s->st));
    HIP_TRY(hipStreamSynchronize(s->st));
    for (uint8_t d : s->h_defer) ndef += d;
    // ascending merge of the missing rounds (the carrier round a - 1 is not examined) and the rows marked bad
    size_t im = 0;
    while (carrier && im < nmiss && s->h_missing[im] < a) im++;
    for (size_t i = 0; i < total; i++) {
      if (!s->h_bad[i]) continue;
      while (im < nmiss && s->h_missing[im] < s->h_rounds[i]) emit(s->h_missing[im++]);
      emit(s->h_rounds[i]);
    }
    while (im < nmiss) emit(s->h_missing[im++]);
    if (b == hi) break;
    a = b + 1;
  }
  *n_faulty_out = nf;
  if (nf > cap) return fail(DH_EINVAL, "%zu faulty rounds, room for %zu", nf, cap);
  return ndef ? DH_DEFERRED : DH_OK;
}

int dh_store_beacons_device(dh_store* s, uint64_t first, uint64_t last, size_t sig_stride, size_t prev_stride, uint64_t* d_rounds,
                            uint8_t* d_sigs, uint32_t* d_sig_lens, uint8_t* d_prevs, uint32_t* d_prev_lens, uint8_t* d_deferred,
                            size_t cap_rows, size_t* n_rows_out, uint64_t* d_missing, size_t cap_missing, size_t* n_missing_out,
                            void* hip_stream) {
  if (!s || !n_rows_out) return fail(DH_EINVAL, "null argument");
  const bool want_prev = d_prevs || d_prev_lens;
  if (!sig_stride || (sig_stride & 3) || sig_stride > ((size_t)1 << 20) ||
      (want_prev && (!prev_stride || (prev_stride & 3) || prev_stride > ((size_t)1 << 20))))
    return fail(DH_EINVAL, "row strides %zu / %zu: positive multiples of 4, at most 1 MiB", sig_stride, prev_stride);
  if (!d_prevs != !d_prev_lens) return fail(DH_EINVAL, "d_prevs and d_prev_lens are given together or not at all");
  handle_guard g(s);
  int rc = store_enter(s);
  if (rc) return rc;
  if (s->format != DH_STORE_UNTRIMMED) return fail(DH_EINVAL, "not an untrimmed (hexjson) store: dh_store_columns_device serves it");
  prof_wall p("store_gather_link");
  if (hip_stream) HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));  // the output buffers may be in use there
  size_t lo, nw, total;
  uint32_t longest;
  if ((rc = store_window(s, first, last, &lo, &nw, &total, &longest))) return rc;
  const size_t nmiss = window_missing(first, last, total);
  *n_rows_out = total;
  if (n_missing_out) *n_missing_out = nmiss;
  if (total > cap_rows || (d_missing && nmiss > cap_missing))
    return fail(DH_EINVAL, "%zu rows and %zu missing rounds, room for %zu and %zu", total, nmiss, cap_rows, d_missing ? cap_missing : 0);
  if (total && (!d_rounds || !d_sigs || !d_sig_lens || !d_deferred)) return fail(DH_EINVAL, "null output");
  if (d_missing && nmiss > 0xffffffffull) return fail(DH_EINVAL, "%zu missing rounds", nmiss);
  if (!total && !(d_missing && nmiss)) return DH_OK;
  uint64_t* rounds = d_rounds;
  if (!rounds) {  // no row: the gaps are still counted from a rounds column
    HIP_TRY(s->rounds.ensure(8));
    rounds = s->rounds.as<uint64_t>();
  }
  const dh::json_cols c{rounds, d_deferred, d_sigs, d_sig_lens, d_prevs, d_prev_lens, (uint32_t)sig_stride,
                        (uint32_t)(want_prev ? prev_stride : 4), cap_rows};
  return store_gather_json(s, lo, nw, total, first, last, c, d_missing, nmiss);
}

int dh_store_deferred(dh_store* s, uint64_t first, uint64_t last, uint64_t* out, size_t cap, size_t* n_out) {
  if (!s || !n_out || (cap && !out)) return fail(DH_EINVAL, "null argument");
  handle_guard g(s);
  int rc = store_enter(s);
  if (rc) return rc;
  *n_out = 0;
  if (s->format != DH_STORE_UNTRIMMED || !s->jstat[0]) return DH_OK;  // a trimmed store defers nothing
  size_t lo, nw, total;
  uint32_t longest;
  if ((rc = store_window(s, first, last, &lo, &nw, &total, &longest))) return rc;
  if (!total) return DH_OK;
  HIP_TRY(s->rounds.ensure(total * 8 + 8));
  HIP_TRY(s->defer.ensure(total + 8));
  const dh::json_cols c{s->rounds.as<uint64_t>(), s->defer.as<uint8_t>(), nullptr, nullptr, nullptr, nullptr, 4, 4, total};
  if ((rc = store_gather_json(s, lo, nw, total, first, last, c, nullptr, 0))) return rc;
  s->h_defer.resize(total);
  s->h_rounds.resize(total);
  HIP_TRY(hipMemcpy(s->h_defer.data(), s->defer.p, total, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(s->h_rounds.data(), s->rounds.p, total * 8, hipMemcpyDeviceToHost));
  size_t n = 0;
  for (size_t i = 0; i < total; i++) {
    if (!s->h_defer[i]) continue;
    if (n < cap) out[n] = s->h_rounds[i];
    n++;
  }
  *n_out = n;
  if (n > cap) return fail(DH_EINVAL, "%zu deferred records, room for %zu", n, cap);
  return DH_OK;
}

}  // extern "C"

// ---- trimmed bbolt store files written from device columns: bolt_write.hpp decides every byte; the
// device packs the leaf pages (k_bolt_write.hip), the host plans them from the scanned record sizes and writes the
// branch levels and pages 0-3.

static size_t write_window_rows() {  // DRANDHIP_STORE_WRITE_WINDOW, read at every call; default: the scan's limit
  const size_t lim = (size_t)4096 * 4096 - 2;
  return std::min(env_size("DRANDHIP_STORE_WRITE_WINDOW", lim, 1), lim);
}

// One window's plan against `pl`, which is not changed: the record sizes of the n new rows on the device, their scan,
// and the host walk over (carried rows || new rows). `last` (device, nullable): the round the first new row must pass.
static int bw_plan_window(bw_state& w, hipStream_t st, const bw_plan& pl, const dh::boltw::cols& fresh, size_t n, const uint64_t* last,
                          bool final, bw_window& out) {
  using namespace dh::boltw;
  if (n + 2 > (size_t)4096 * 4096) return fail(DH_EINVAL, "window of %zu rows: at most 16M rows per window", n);
  const size_t nc = pl.carry_need.size();
  out.m = nc + n;
  out.sums.resize(out.m + 1);
  uint32_t* sums = out.sums.data();
  sums[nc] = 0;
  if (n) {
    uint32_t err_word = 0;
    HIP_TRY(w.need.ensure(n * 4));
    HIP_TRY(w.sums.ensure((n + 1) * 4));
    HIP_TRY(w.scan_tmp.ensure((n / 4096 + 2) * 4));
    HIP_TRY(w.err.ensure(4));
    HIP_TRY(hipMemsetAsync(w.err.p, 0, 4, st));
    HIP_TRY(dh::launch_bolt_need(fresh, n, last, w.need.as<uint32_t>(), w.err.as<uint32_t>(), st));
    HIP_TRY(dh::launch_scan(w.need.as<uint32_t>(), n, w.sums.as<uint32_t>(), w.scan_tmp.as<uint32_t>(), st));
    HIP_TRY(hipMemcpyAsync(sums + nc, w.sums.p, (n + 1) * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&err_word, w.err.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (err_word)
      return fail(DH_EINVAL, "rounds not strictly ascending, or a value longer than the row stride %llu", (unsigned long long)fresh.stride);
  }
  if (nc) {  // the carried rows' sizes in front (modulo 2^32, as the scan leaves the rest)
    uint32_t base = 0;
    for (size_t i = 0; i < nc; i++) {
      sums[i] = base;
      base += pl.carry_need[i];
    }
    for (size_t i = nc; i <= out.m; i++) sums[i] += base;
  }
  // the greedy leaf boundaries: plan_window's host walk over the sums (8 bytes a row with the copy, well below the
  // pack's time), into the room the last window's plan left; walked again only when this one closes more leaves
  out.leaves.resize(out.leaves.capacity());
  window_plan wp = plan_window(sums, out.m, w.P, pl.next_page, final, out.leaves.data(), out.leaves.size());
  if (wp.leaves > out.leaves.size()) {
    out.leaves.resize(wp.leaves);
    wp = plan_window(sums, out.m, w.P, pl.next_page, final, out.leaves.data(), out.leaves.size());
  }
  out.leaves.resize(wp.leaves);
  out.open_row = wp.open_row;
  out.next_page = wp.next_page;
  return DH_OK;
}

// the plan state behind a planned window of n new rows
static void bw_advance(bw_plan& pl, const bw_window& win, size_t n) {
  std::vector<uint32_t> need(win.m - win.open_row);
  for (uint64_t i = win.open_row; i < win.m; i++) need[i - win.open_row] = win.sums[i + 1] - win.sums[i];
  pl.carry_need.swap(need);
  pl.next_page = win.next_page;
  pl.leaves += win.leaves.size();
  pl.rows += n;
}

// One window into the writer: the closed leaves' pages to out[0, *len_out), which belong at *file_off_out. With
// `final` the open leaf is closed too, the branch pages follow the run in `out`, pages 0-3 go to `head` and st3 is the
// file's {rows, leaves, pages}; otherwise st3 is this window's {rows taken, leaves closed, pages emitted}. On every
// failure the writer is as before the call; cap too small (cap 0 sizes): DH_EINVAL with *len_out set.
static int bw_append(bw_state& w, hipStream_t st, const dh::boltw::cols& fresh, size_t n, bool final, uint8_t* out, size_t cap,
                     size_t* len_out, uint64_t* file_off_out, uint8_t* head, uint64_t st3[3], const char* const stage[3]) {
  using namespace dh::boltw;
  *len_out = 0;
  const uint32_t P = w.P;
  if (file_off_out) *file_off_out = w.plan.next_page * P;
  if (st3) st3[0] = st3[1] = st3[2] = 0;
  if (w.finished) return fail(DH_EINVAL, "the writer is finished");
  if (final && !(w.plan.rows + n)) return fail(DH_ENOBEACON, "no beacon to write: an empty store is not written");
  if (!n && !final) return DH_OK;
  bw_window& win = w.win;
  bw_state::carry_set& old = w.set[w.cur];
  bw_state::carry_set& nxt = w.set[w.cur ^ 1];
  const size_t nc = w.plan.carry_need.size();
  {
    prof_wall p(stage[0]);
    int rc = bw_plan_window(w, st, w.plan, fresh, n, w.has_last ? old.last.as<uint64_t>() : nullptr, final, win);
    if (rc) return rc;
  }
  const size_t nl = win.leaves.size();
  const uint64_t run_bytes = (win.next_page - w.plan.next_page) * P;
  const uint64_t all_leaves = w.plan.leaves + nl;
  const uint64_t pages = win.next_page + (final ? branch_pages(all_leaves, P) : 0);
  const uint64_t bytes = (pages - w.plan.next_page) * P;
  *len_out = (size_t)bytes;
  if (st3) {
    st3[0] = final ? w.plan.rows + n : n;
    st3[1] = final ? all_leaves : nl;
    st3[2] = final ? pages : win.next_page - w.plan.next_page;
  }
  if (bytes + w.call_base > store_max_bytes())  // what the call emits: a one-shot call's image from byte 0
    return fail(DH_ENOMEM, "store image of %llu bytes exceeds DRANDHIP_STORE_MAX_BYTES (%zu)", (unsigned long long)(bytes + w.call_base),
                store_max_bytes());
  if (cap < bytes || (bytes && !out) || (final && !head))
    return fail(DH_EINVAL, "store image of %llu bytes, room for %zu", (unsigned long long)bytes, cap);
  // a segment without rows still gets the other segment's (readable) addresses, never null ones: a wave-uniform address
  // is read by scalar loads, which no lane mask holds back (k_bolt_write.hip, k_bolt_unlinked)
  const cols carried{old.rounds.as<uint64_t>(), old.rows.as<uint8_t>(), w.carry_stride, old.lens.as<uint32_t>()};
  const cols2 c{nc ? carried : fresh, n ? fresh : carried, nc};
  const uint64_t n_open = win.m - win.open_row;
  uint32_t longest = 0;
  for (uint64_t i = win.open_row; i < win.m; i++) longest = std::max(longest, win.sums[i + 1] - win.sums[i] - 24);
  const size_t nxt_stride = std::max<size_t>(4, ((size_t)longest + 3) & ~(size_t)3);
  {
    prof_wall p(stage[1]);
    HIP_TRY(w.leaves.ensure(nl * sizeof(leaf_desc)));
    HIP_TRY(w.image.ensure(run_bytes));
    HIP_TRY(w.keys.ensure(nl * 8));
    if (nl) HIP_TRY(hipMemcpyAsync(w.leaves.p, win.leaves.data(), nl * sizeof(leaf_desc), hipMemcpyHostToDevice, st));
    timed_launches tl(st);
    HIP_TRY(tl.run("k_bolt_pack", [&] {
      return dh::launch_bolt_pack(w.leaves.p, nl, c, P, w.plan.next_page, w.image.as<uint8_t>(), w.keys.as<uint64_t>(), st);
    }));
    if (n) {  // the open leaf's rows and the last row appended, into the other carry set
      const uint32_t last_len = win.sums[win.m] - win.sums[win.m - 1] - 24;
      const size_t last_stride = std::max<size_t>(4, ((size_t)last_len + 3) & ~(size_t)3);
      HIP_TRY(nxt.rounds.ensure(n_open * 8));
      HIP_TRY(nxt.lens.ensure(n_open * 4));
      HIP_TRY(nxt.rows.ensure(n_open * nxt_stride));
      HIP_TRY(nxt.last.ensure(16 + last_stride));
      const dh::carry_out o{nxt.rounds.as<uint64_t>(), nxt.lens.as<uint32_t>(), nxt.rows.as<uint8_t>(), (uint32_t)nxt_stride,
                            nxt.last.as<uint64_t>(), (uint32_t)last_stride};
      HIP_TRY(tl.run("k_bolt_carry", [&] { return dh::launch_bolt_carry(c, win.open_row, n_open, win.m - 1, o, st); }));
    }
    HIP_TRY(hipStreamSynchronize(st));
  }
  {
    prof_wall p(stage[2]);
    win.keys.resize(nl);
    if (run_bytes) HIP_TRY(hipMemcpyAsync(out, w.image.p, run_bytes, hipMemcpyDeviceToHost, st));
    if (nl) HIP_TRY(hipMemcpyAsync(win.keys.data(), w.keys.p, nl * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  // committed: nothing below fails
  w.h_keys.insert(w.h_keys.end(), win.keys.begin(), win.keys.end());
  for (size_t i = 0; i < nl; i++) w.h_pgids.push_back(win.leaves[i].page);
  bw_advance(w.plan, win, n);
  if (n) {
    w.cur ^= 1;
    w.carry_stride = nxt_stride;
    w.has_last = true;
  }
  if (final) {
    finish_tail(out + run_bytes, head, P, pages, win.next_page, w.h_keys.data(), w.h_pgids.data(), all_leaves);
    w.finished = true;
  }
  return DH_OK;
}

// The one-shot image over n rows in device memory, as a loop over the writer: windows of DRANDHIP_STORE_WRITE_WINDOW
// rows, the last of them final. Entered with the device set. With cap too small (cap 0 sizes only): DH_EINVAL,
// *len_out set, nothing written; more than one window is sized by a planning pass of its own first.
static int bolt_write_core(hipStream_t st, bw_state& w, const uint64_t* d_rounds, const uint8_t* d_rows, size_t stride,
                           const uint32_t* d_lens, size_t n, uint32_t P, uint8_t* image_out, size_t cap, size_t* len_out,
                           uint64_t stats[3], const char* const stage[4]) {
  using namespace dh::boltw;
  *len_out = 0;
  if (!n) return fail(DH_ENOBEACON, "no beacon to write: an empty store is not written");
  const size_t W = write_window_rows();
  auto cut = [&](size_t off) {
    return cols{d_rounds + off, d_rows ? d_rows + off * stride : nullptr, (uint64_t)stride, d_lens + off};
  };
  w.reset(P);
  if (n > W) {  // the whole image's size, before a byte is written
    prof_wall p(stage[0]);
    bw_plan shadow;
    for (size_t off = 0; off < n; off += W) {
      const size_t k = std::min(W, n - off);
      int rc = bw_plan_window(w, st, shadow, cut(off), k, off ? d_rounds + off - 1 : nullptr, off + k == n, w.win);
      if (rc) return rc;
      bw_advance(shadow, w.win, k);
    }
    const uint64_t pages = shadow.next_page + branch_pages(shadow.leaves, P), bytes = pages * P;
    *len_out = (size_t)bytes;
    if (stats) {
      stats[0] = n;
      stats[1] = shadow.leaves;
      stats[2] = pages;
    }
    if (bytes > store_max_bytes())
      return fail(DH_ENOMEM, "store image of %llu bytes exceeds DRANDHIP_STORE_MAX_BYTES (%zu)", (unsigned long long)bytes, store_max_bytes());
    if (cap < bytes || !image_out) return fail(DH_EINVAL, "store image of %llu bytes, room for %zu", (unsigned long long)bytes, cap);
  }
  for (size_t off = 0; off < n; off += W) {
    prof_wall p(stage[3]);
    const size_t k = std::min(W, n - off);
    const bool final = off + k == n;
    const uint64_t at = w.plan.next_page * P;  // the run's place in the image
    size_t len = 0;
    w.call_base = at;
    int rc = bw_append(w, st, cut(off), k, final, image_out ? image_out + at : nullptr, cap > at ? cap - at : 0, &len, nullptr, image_out,
                       final ? stats : nullptr, stage);
    if (n <= W) {  // one window: sized here; the run starts at page 4
      *len_out = len ? (size_t)at + len : 0;
      if (rc == DH_EINVAL && len && (cap < at + len || !image_out))
        return fail(DH_EINVAL, "store image of %llu bytes, room for %zu", (unsigned long long)(at + len), cap);
    }
    if (rc) return rc;
  }
  return DH_OK;
}

extern "C" {

int dh_bolt_write_trimmed_device(const uint64_t* d_rounds, const uint8_t* d_rows, size_t row_stride, const uint32_t* d_lens, size_t n,
                                 uint32_t page_size, uint8_t* image_out, size_t cap, size_t* len_out, uint64_t stats_out[3],
                                 void* hip_stream) {
  if (!len_out) return fail(DH_EINVAL, "null argument");
  *len_out = 0;
  if (!dh::boltw::page_size_ok(page_size)) return fail(DH_EINVAL, "page size %u: a power of two from 256 to 65536", page_size);
  if (!n) return fail(DH_ENOBEACON, "no beacon to write: an empty store is not written");
  if (!d_rounds || !d_lens || (row_stride && !d_rows) || (cap && !image_out)) return fail(DH_EINVAL, "null argument");
  int rc = ensure_device();
  if (rc) return rc;
  if (hip_stream) HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));  // the columns may still be written there
  hipStream_t st = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  bw_state w;
  static const char* const stage[4] = {"bolt_write_plan", "bolt_write_pack", "bolt_write_download", "bolt_write_window"};
  rc = bolt_write_core(st, w, d_rounds, d_rows, row_stride, d_lens, n, page_size, image_out, cap, len_out, stats_out, stage);
  w.release();
  (void)hipStreamDestroy(st);
  return rc;
}

static const char* const g_writer_stage[4] = {"bolt_write_plan", "bolt_write_pack", "bolt_write_download", "bolt_write_window"};

int dh_bolt_writer_open(uint32_t page_size, dh_bolt_writer** out) {
  if (!out) return fail(DH_EINVAL, "null argument");
  *out = nullptr;
  if (!dh::boltw::page_size_ok(page_size)) return fail(DH_EINVAL, "page size %u: a power of two from 256 to 65536", page_size);
  int rc = ensure_device();
  if (rc) return rc;
  dh_bolt_writer* w = new dh_bolt_writer();
  hipError_t e = hipStreamCreateWithFlags(&w->st, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete w;
    return fail(DH_EDEVICE, "hipStreamCreateWithFlags: %s", hipGetErrorString(e));
  }
  w->bw.reset(page_size);
  handle_register(w);
  *out = w;
  return DH_OK;
}

int dh_bolt_writer_append_device(dh_bolt_writer* w, const uint64_t* d_rounds, const uint8_t* d_rows, size_t row_stride,
                                 const uint32_t* d_lens, size_t n, uint8_t* out, size_t cap, size_t* len_out, uint64_t* file_off_out,
                                 uint64_t stats_out[3], void* hip_stream) {
  if (!w || !len_out) return fail(DH_EINVAL, "null argument");
  *len_out = 0;
  if ((n && (!d_rounds || !d_lens || (row_stride && !d_rows))) || (cap && !out)) return fail(DH_EINVAL, "null argument");
  handle_guard g(w);
  int rc = writer_enter(w);
  if (rc) return rc;
  if (n && hip_stream) HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));  // the columns may still be written there
  prof_wall p(g_writer_stage[3]);
  const dh::boltw::cols fresh{d_rounds, d_rows, (uint64_t)row_stride, d_lens};
  return bw_append(w->bw, w->st, fresh, n, false, out, cap, len_out, file_off_out, nullptr, stats_out, g_writer_stage);
}

int dh_bolt_writer_finish(dh_bolt_writer* w, uint8_t* tail_out, size_t cap, size_t* len_out, uint64_t* file_off_out, uint8_t* head_out,
                          uint64_t stats_out[3]) {
  if (!w || !len_out) return fail(DH_EINVAL, "null argument");
  *len_out = 0;
  if (cap && !tail_out) return fail(DH_EINVAL, "null argument");
  handle_guard g(w);
  int rc = writer_enter(w);
  if (rc) return rc;
  const dh::boltw::cols none{nullptr, nullptr, 0, nullptr};
  return bw_append(w->bw, w->st, none, 0, true, tail_out, cap, len_out, file_off_out, head_out, stats_out, g_writer_stage);
}

void dh_bolt_writer_close(dh_bolt_writer* w) { handle_close(w); }

struct patch_list {
  const uint64_t* rounds;
  const uint8_t* sigs;
  size_t stride;
  const uint32_t* lens;
  size_t n;
  uint32_t longest;
};

// patches strictly ascending and inside [first, last]; sets p->longest
static int patches_check(patch_list* p, uint64_t first, uint64_t last) {
  if (p->n > ((size_t)1 << 20)) return fail(DH_EINVAL, "%zu patches: at most 2^20", p->n);
  if (p->n && (!p->rounds || !p->lens)) return fail(DH_EINVAL, "null patch list");
  if (p->stride > ((size_t)1 << 20)) return fail(DH_EINVAL, "patch stride %zu above 1 MiB", p->stride);
  p->longest = 0;
  for (size_t i = 0; i < p->n; i++) {
    if (p->rounds[i] < first || p->rounds[i] > last || (i && p->rounds[i - 1] >= p->rounds[i]))
      return fail(DH_EINVAL, "patch %zu (round %llu): patches are strictly ascending and inside [first, last]", i,
                  (unsigned long long)p->rounds[i]);
    if (p->lens[i] == DH_PATCH_DELETE) continue;
    if (p->lens[i] > p->stride || (p->lens[i] && !p->sigs))
      return fail(DH_EINVAL, "patch %zu: %u bytes, patch stride %zu", i, p->lens[i], p->stride);
    p->longest = std::max(p->longest, p->lens[i]);
  }
  return DH_OK;
}

// the patches of [lo, hi] out of a checked list
static patch_list patches_cut(const patch_list& p, uint64_t lo, uint64_t hi) {
  const size_t a = std::lower_bound(p.rounds, p.rounds + p.n, lo) - p.rounds;
  const size_t b = std::upper_bound(p.rounds, p.rounds + p.n, hi) - p.rounds;
  patch_list q = p;
  q.rounds = p.rounds + a;
  q.lens = p.lens + a;
  q.sigs = p.sigs ? p.sigs + a * p.stride : nullptr;
  q.n = b - a;
  return q;
}

struct merged {  // one round window merged with its patches: the columns are ws.o_*, the unlinked rounds ws.unl
  size_t slots = 0, n_out = 0, n_unl = 0, n_hit = 0, n_ins = 0, o_stride = 4;
};

// The round records of first..last merged with the patches into s->wws.o_* (DESIGN.md §22). pred (device, nullable):
// the row before the window, in the layout of carry_out.last, for the first merged row's unlinked test. A window
// without a row is DH_OK with n_out = 0. Entered with the store held and the device set.
static int store_merge_window(dh_store* s, uint64_t first, uint64_t last, const patch_list& pt, const uint64_t* pred, merged* out) {
  write_ws& ws = s->wws;
  const bool json = s->format == DH_STORE_UNTRIMMED;
  const size_t n_patch = pt.n, patch_stride = pt.stride;
  *out = merged();
  prof_wall p("store_save_merge");
  int rc;
  size_t lo, nw, total;
  uint32_t longest;
  if ((rc = store_window(s, first, last, &lo, &nw, &total, &longest))) return rc;
  if (total + n_patch + 3 > (size_t)4096 * 4096)
    return fail(DH_EINVAL, "%zu rows and %zu patches: at most 16M per window", total, n_patch);
  if (json) longest = window_longest_json(s, lo, nw);
  const size_t stride = std::max<size_t>(4, ((size_t)longest + 3) & ~(size_t)3);
  if (stride > ((size_t)1 << 20)) return fail(DH_EINVAL, "a %u-byte record in rounds %llu..%llu: keep the host reader", longest,
                                              (unsigned long long)first, (unsigned long long)last);
  HIP_TRY(s->rounds.ensure(total * 8 + 8));
  HIP_TRY(s->rows.ensure(total * stride + 8));
  HIP_TRY(s->lens.ensure(total * 4 + 4));
  if (json) {
    HIP_TRY(s->defer.ensure(total + 8));
    HIP_TRY(s->prevs.ensure(total * stride + 8));
    HIP_TRY(s->prev_lens.ensure(total * 4 + 4));
    const dh::json_cols c{s->rounds.as<uint64_t>(), s->defer.as<uint8_t>(), s->rows.as<uint8_t>(), s->lens.as<uint32_t>(),
                          s->prevs.as<uint8_t>(), s->prev_lens.as<uint32_t>(), (uint32_t)stride, (uint32_t)stride, total};
    if ((rc = store_gather_json(s, lo, nw, total, first, last, c, nullptr, 0))) return rc;
  } else if ((rc = store_gather(s, lo, nw, total, first, last, stride, s->rounds.as<uint64_t>(), s->rows.as<uint8_t>(),
                                s->lens.as<uint32_t>(), total, nullptr, 0))) {
    return rc;
  }
  // the patches, uploaded as given
  const size_t slots = total + n_patch;
  out->slots = slots;
  if (!slots) return DH_OK;
  HIP_TRY(ws.p_rounds.ensure(n_patch * 8 + 8));
  HIP_TRY(ws.p_lens.ensure(n_patch * 4 + 4));
  HIP_TRY(ws.p_rows.ensure(n_patch * patch_stride + 8));
  HIP_TRY(ws.flag.ensure(slots * 4 + 4));
  HIP_TRY(ws.lb.ensure(slots * 4 + 4));
  HIP_TRY(ws.pos.ensure((slots + 1) * 4));
  HIP_TRY(ws.scan_tmp.ensure((slots / 4096 + 2) * 4));
  HIP_TRY(ws.hit.ensure(n_patch + 8));
  HIP_TRY(ws.err.ensure(4));
  if (n_patch) {
    HIP_TRY(hipMemcpyAsync(ws.p_rounds.p, pt.rounds, n_patch * 8, hipMemcpyHostToDevice, s->st));
    HIP_TRY(hipMemcpyAsync(ws.p_lens.p, pt.lens, n_patch * 4, hipMemcpyHostToDevice, s->st));
    if (pt.sigs && patch_stride) HIP_TRY(hipMemcpyAsync(ws.p_rows.p, pt.sigs, n_patch * patch_stride, hipMemcpyHostToDevice, s->st));
  }
  HIP_TRY(hipMemsetAsync(ws.err.p, 0, 4, s->st));
  const dh::merge_in m{s->rounds.as<uint64_t>(), s->rows.as<uint8_t>(), s->lens.as<uint32_t>(),
                       json ? s->defer.as<uint8_t>() : nullptr, total, (uint32_t)stride, ws.p_rounds.as<uint64_t>(),
                       ws.p_rows.as<uint8_t>(), ws.p_lens.as<uint32_t>(), n_patch, (uint32_t)patch_stride};
  HIP_TRY(dh::launch_bolt_merge(m, ws.flag.as<uint32_t>(), ws.lb.as<uint32_t>(), ws.hit.as<uint8_t>(), ws.err.as<uint32_t>(), s->st));
  HIP_TRY(dh::launch_scan(ws.flag.as<uint32_t>(), slots, ws.pos.as<uint32_t>(), ws.scan_tmp.as<uint32_t>(), s->st));
  uint32_t err_word = 0, tot = 0;
  std::vector<uint8_t> hit(n_patch);
  HIP_TRY(hipMemcpyAsync(&err_word, ws.err.p, 4, hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipMemcpyAsync(&tot, ws.pos.as<uint32_t>() + slots, 4, hipMemcpyDeviceToHost, s->st));
  if (n_patch) HIP_TRY(hipMemcpyAsync(hit.data(), ws.hit.p, n_patch, hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  if (err_word) {
    g_err = "a deferred record in the range is not covered by a patch (dh_store_deferred lists them)";
    return DH_DEFERRED;
  }
  for (uint8_t h : hit) {
    out->n_hit += h == 1;
    out->n_ins += h == 2;
  }
  const size_t n_out = out->n_out = tot;
  if (!n_out) return DH_OK;
  const size_t o_stride = out->o_stride = std::max<size_t>(stride, ((size_t)pt.longest + 3) & ~(size_t)3);
  HIP_TRY(ws.o_rounds.ensure(n_out * 8));
  HIP_TRY(ws.o_rows.ensure(n_out * o_stride));
  HIP_TRY(ws.o_lens.ensure(n_out * 4));
  HIP_TRY(ws.o_src.ensure(n_out * 4));
  const dh::merge_out o{ws.o_rounds.as<uint64_t>(), ws.o_rows.as<uint8_t>(), ws.o_lens.as<uint32_t>(), ws.o_src.as<uint32_t>(),
                        (uint32_t)o_stride};
  HIP_TRY(dh::launch_bolt_scatter(m, ws.flag.as<uint32_t>(), ws.lb.as<uint32_t>(), ws.pos.as<uint32_t>(), o, s->st));
  if (json) {  // flag / pos are free again: the unlinked rows and their ranks
    HIP_TRY(ws.flag.ensure(n_out * 4 + 4));
    HIP_TRY(ws.pos.ensure((n_out + 1) * 4));
    HIP_TRY(ws.unl.ensure(n_out * 8));
    HIP_TRY(dh::launch_bolt_unlinked(o, n_out, s->prevs.as<uint8_t>(), (uint32_t)stride, s->prev_lens.as<uint32_t>(), pred,
                                     ws.flag.as<uint32_t>(), s->st));
    HIP_TRY(dh::launch_scan(ws.flag.as<uint32_t>(), n_out, ws.pos.as<uint32_t>(), ws.scan_tmp.as<uint32_t>(), s->st));
    HIP_TRY(dh::launch_bolt_compact(ws.o_rounds.as<uint64_t>(), ws.pos.as<uint32_t>(), n_out, ws.unl.as<uint64_t>(), s->st));
    HIP_TRY(hipMemcpyAsync(&tot, ws.pos.as<uint32_t>() + n_out, 4, hipMemcpyDeviceToHost, s->st));
    HIP_TRY(hipStreamSynchronize(s->st));
    out->n_unl = tot;
  } else {
    HIP_TRY(hipStreamSynchronize(s->st));
  }
  return DH_OK;
}

static dh::boltw::cols merged_cols(const write_ws& ws, const merged& m) {
  return dh::boltw::cols{ws.o_rounds.as<uint64_t>(), ws.o_rows.as<uint8_t>(), (uint64_t)m.o_stride, ws.o_lens.as<uint32_t>()};
}

// [first, last] cut into round windows at leaf boundaries of the source, each of at most max(max_rows, rows of its
// largest leaf) stored rows: window i = [b[2i], b[2i + 1]], the first from `first`, the last to `last`, no round between
// two windows. From the leaf index and the scan's counts alone.
static void store_split(const dh_store* s, uint64_t first, uint64_t last, size_t max_rows, std::vector<uint64_t>* b) {
  b->clear();
  if (first > last) return;
  const auto& rl = s->rleaf;
  const size_t lo = std::partition_point(rl.begin(), rl.end(), [&](uint32_t i) { return s->info[i].last < first; }) - rl.begin();
  const size_t hi = std::partition_point(rl.begin(), rl.end(), [&](uint32_t i) { return s->info[i].first <= last; }) - rl.begin();
  uint64_t start = first;
  size_t rows = 0;
  for (size_t k = lo; k < hi; k++) {
    const auto& li = s->info[rl[k]];
    if (rows && rows + li.n_round > max_rows) {  // cut behind the leaf before this one
      const uint64_t end = s->info[rl[k - 1]].last;
      b->push_back(start);
      b->push_back(end);
      start = end + 1;  // end < li.first <= last
      rows = 0;
    }
    rows += li.n_round;
  }
  b->push_back(start);
  b->push_back(last);
}

static const char* const g_save_stage[4] = {"store_save_plan", "store_save_pack", "store_save_download", "store_save_window"};

int dh_store_split(dh_store* s, uint64_t first, uint64_t last, size_t max_rows, uint64_t* bounds_out, size_t cap, size_t* n_out) {
  if (!s || !n_out || (cap && !bounds_out)) return fail(DH_EINVAL, "null argument");
  *n_out = 0;
  handle_guard g(s);
  int rc = store_enter(s);
  if (rc) return rc;
  std::vector<uint64_t> b;
  store_split(s, first, last, std::max<size_t>(1, max_rows), &b);
  *n_out = b.size() / 2;
  if (*n_out > cap) return fail(DH_EINVAL, "%zu windows, room for %zu", *n_out, cap);
  if (!b.empty()) memcpy(bounds_out, b.data(), b.size() * 8);
  return DH_OK;
}

int dh_store_save_trimmed_append(dh_store* s, dh_bolt_writer* w, uint64_t first, uint64_t last, const uint64_t* patch_rounds,
                                 const uint8_t* patch_sigs, size_t patch_stride, const uint32_t* patch_lens, size_t n_patch,
                                 uint8_t* out, size_t cap, size_t* len_out, uint64_t* file_off_out, uint64_t* unlinked_out,
                                 size_t unlinked_cap, size_t* n_unlinked_out, uint64_t stats_out[6]) {
  if (!s || !w || !len_out || !n_unlinked_out || (cap && !out) || (unlinked_cap && !unlinked_out)) return fail(DH_EINVAL, "null argument");
  *len_out = 0;
  *n_unlinked_out = 0;
  if (stats_out) memset(stats_out, 0, 6 * sizeof(uint64_t));
  patch_list pt{patch_rounds, patch_sigs, patch_stride, patch_lens, n_patch, 0};
  int rc = patches_check(&pt, first, last);
  if (rc) return rc;
  handle_guard g(s);
  if ((rc = store_enter(s))) return rc;
  handle_guard gw(w);
  if ((rc = writer_enter(w))) return rc;
  bw_state& bw = w->bw;
  if (file_off_out) *file_off_out = bw.plan.next_page * bw.P;
  if (bw.finished) return fail(DH_EINVAL, "the writer is finished");
  prof_wall p(g_save_stage[3]);
  write_ws& ws = s->wws;
  merged m;
  const uint64_t* pred = bw.has_last ? bw.set[bw.cur].last.as<uint64_t>() : nullptr;
  if ((rc = store_merge_window(s, first, last, pt, pred, &m))) return rc;
  *n_unlinked_out = m.n_unl;
  uint64_t st3[3] = {0, 0, 0};
  if (m.n_out) {
    const dh::boltw::cols fresh = merged_cols(ws, m);
    if (m.n_unl > unlinked_cap) {  // sized without being taken
      if ((rc = bw_plan_window(bw, s->st, bw.plan, fresh, m.n_out, pred, false, bw.win))) return rc;
      *len_out = (size_t)((bw.win.next_page - bw.plan.next_page) * bw.P);
      return fail(DH_EINVAL, "%zu unlinked rounds, room for %zu", m.n_unl, unlinked_cap);
    }
    if ((rc = bw_append(bw, s->st, fresh, m.n_out, false, out, cap, len_out, file_off_out, nullptr, st3, g_save_stage))) return rc;
    if (m.n_unl) HIP_TRY(hipMemcpy(unlinked_out, ws.unl.p, m.n_unl * 8, hipMemcpyDeviceToHost));
  }
  if (stats_out) {
    memcpy(stats_out, st3, sizeof st3);
    stats_out[3] = m.n_unl;
    stats_out[4] = m.n_hit;
    stats_out[5] = m.n_ins;
  }
  return DH_OK;
}

int dh_store_save_trimmed(dh_store* s, uint64_t first, uint64_t last, const uint64_t* patch_rounds, const uint8_t* patch_sigs,
                          size_t patch_stride, const uint32_t* patch_lens, size_t n_patch, uint32_t page_size, uint8_t* image_out,
                          size_t cap, size_t* len_out, uint64_t* unlinked_out, size_t unlinked_cap, size_t* n_unlinked_out,
                          uint64_t stats_out[6]) {
  using namespace dh::boltw;
  if (!s || !len_out || !n_unlinked_out || (cap && !image_out) || (unlinked_cap && !unlinked_out)) return fail(DH_EINVAL, "null argument");
  *len_out = 0;
  *n_unlinked_out = 0;
  if (!page_size_ok(page_size)) return fail(DH_EINVAL, "page size %u: a power of two from 256 to 65536", page_size);
  patch_list pt{patch_rounds, patch_sigs, patch_stride, patch_lens, n_patch, 0};
  int rc = patches_check(&pt, first, last);
  if (rc) return rc;
  handle_guard g(s);
  if ((rc = store_enter(s))) return rc;
  write_ws& ws = s->wws;
  bw_state& bw = ws.bw;
  const uint32_t P = page_size;
  // the windows: rows and patches of one window stay within the scan's reach
  const size_t W = write_window_rows(), reach = (size_t)4096 * 4096 - 3 - n_patch;
  std::vector<uint64_t> b;
  store_split(s, first, last, std::max<size_t>(1, std::min(W, reach)), &b);
  if (b.empty()) b = {first, last};  // first > last: the empty window, refused below
  const size_t nwin = b.size() / 2;
  bw.reset(P);
  size_t slots = 0, rows = 0, n_unl = 0, n_hit = 0, n_ins = 0;
  if (nwin > 1) {  // the whole image's size and the unlinked count, before a byte is written
    bw_plan shadow;
    HIP_TRY(ws.pred[0].ensure(16 + ((size_t)1 << 20)));
    HIP_TRY(ws.pred[1].ensure(16 + ((size_t)1 << 20)));
    int k = 0;
    bool have = false;
    for (size_t i = 0; i < nwin; i++) {
      merged m;
      const uint64_t* pred = have ? ws.pred[k].as<uint64_t>() : nullptr;
      if ((rc = store_merge_window(s, b[2 * i], b[2 * i + 1], patches_cut(pt, b[2 * i], b[2 * i + 1]), pred, &m))) return rc;
      slots += m.slots;
      n_unl += m.n_unl;
      n_hit += m.n_hit;
      n_ins += m.n_ins;
      if (!m.n_out) continue;
      rows += m.n_out;
      const cols fresh = merged_cols(ws, m);
      prof_wall p(g_save_stage[0]);
      if ((rc = bw_plan_window(bw, s->st, shadow, fresh, m.n_out, pred, false, bw.win))) return rc;
      bw_advance(shadow, bw.win, m.n_out);
      // the window's last row, for the next window's first
      const cols2 c{fresh, fresh, 0};  // no carried rows: their segment gets readable addresses all the same
      const dh::carry_out o{nullptr, nullptr, nullptr, 4, ws.pred[k ^ 1].as<uint64_t>(), (uint32_t)m.o_stride};
      HIP_TRY(dh::launch_bolt_carry(c, 0, 0, m.n_out - 1, o, s->st));
      HIP_TRY(hipStreamSynchronize(s->st));
      k ^= 1;
      have = true;
    }
    if (rows) {
      bw_window fin;  // the open leaf, closed
      if ((rc = bw_plan_window(bw, s->st, shadow, cols{nullptr, nullptr, 0, nullptr}, 0, nullptr, true, fin))) return rc;
      bw_advance(shadow, fin, 0);
      const uint64_t pages = shadow.next_page + branch_pages(shadow.leaves, P), bytes = pages * P;
      *len_out = (size_t)bytes;
      *n_unlinked_out = n_unl;
      if (stats_out) {
        const uint64_t st6[6] = {rows, shadow.leaves, pages, n_unl, n_hit, n_ins};
        memcpy(stats_out, st6, sizeof st6);
      }
      if (n_unl > unlinked_cap) return fail(DH_EINVAL, "%zu unlinked rounds, room for %zu", n_unl, unlinked_cap);
      if (bytes > store_max_bytes())
        return fail(DH_ENOMEM, "store image of %llu bytes exceeds DRANDHIP_STORE_MAX_BYTES (%zu)", (unsigned long long)bytes, store_max_bytes());
      if (cap < bytes || !image_out) return fail(DH_EINVAL, "store image of %llu bytes, room for %zu", (unsigned long long)bytes, cap);
    }
    slots = rows = n_unl = n_hit = n_ins = 0;
  }
  uint64_t st3[3] = {0, 0, 0};
  for (size_t i = 0; i < nwin; i++) {
    prof_wall p(g_save_stage[3]);
    const bool final = i + 1 == nwin;
    merged m;
    const uint64_t* pred = bw.has_last ? bw.set[bw.cur].last.as<uint64_t>() : nullptr;
    if ((rc = store_merge_window(s, b[2 * i], b[2 * i + 1], patches_cut(pt, b[2 * i], b[2 * i + 1]), pred, &m))) return rc;
    slots += m.slots;
    n_hit += m.n_hit;
    n_ins += m.n_ins;
    rows += m.n_out;
    if (final && !rows) {
      if (!slots) return fail(DH_ENOBEACON, "no beacon stored in rounds %llu..%llu", (unsigned long long)first, (unsigned long long)last);
      return fail(DH_ENOBEACON, "no beacon left to write in rounds %llu..%llu", (unsigned long long)first, (unsigned long long)last);
    }
    if (!m.n_out && !final) continue;
    const cols fresh = m.n_out ? merged_cols(ws, m) : cols{nullptr, nullptr, 0, nullptr};
    const uint64_t at = bw.plan.next_page * P;  // the run's place in the image
    const bool room = n_unl + m.n_unl <= unlinked_cap;  // more than one window: settled by the sizing pass
    size_t len = 0;
    bw.call_base = at;
    rc = bw_append(bw, s->st, fresh, m.n_out, final, room && image_out ? image_out + at : nullptr, room && cap > at ? cap - at : 0, &len,
                   nullptr, room ? image_out : nullptr, final ? st3 : nullptr, g_save_stage);
    if (nwin == 1) {  // one window: sized here
      *len_out = len ? (size_t)at + len : 0;
      *n_unlinked_out = m.n_unl;
      if (stats_out) {
        const uint64_t st6[6] = {st3[0], st3[1], st3[2], m.n_unl, n_hit, n_ins};
        memcpy(stats_out, st6, sizeof st6);
      }
      if (!room) return fail(DH_EINVAL, "%zu unlinked rounds, room for %zu", m.n_unl, unlinked_cap);
      if (rc == DH_EINVAL && len && (cap < at + len || !image_out))
        return fail(DH_EINVAL, "store image of %llu bytes, room for %zu", (unsigned long long)(at + len), cap);
    }
    if (rc) return rc;
    if (m.n_unl) HIP_TRY(hipMemcpy(unlinked_out + n_unl, ws.unl.p, m.n_unl * 8, hipMemcpyDeviceToHost));
    n_unl += m.n_unl;
  }
  return DH_OK;
}

}  // extern "C"

// ---- client.RandomData JSON-lines archives on the device: the records every HTTP relay serves
// (client/random.go:5-10, hexjson), one per line. The image is uploaded once per open archive and indexed there
// (k_archive.hip); a window's columns come out in the layout dh_verify_batch_device takes. Locking and lifetime as
// dh_store.

struct dh_archive : dh_handle {
  uint64_t len = 0, nrec = 0;
  uint64_t stat[7] = {0, 0, 0, 0, 0, 0, dh::ARCHIVE_TILE};
  dbuf d_file, cnt, base, scan_tmp, line_off, line_len, chunks, d_stat;
  // dh_archive_check / dh_archive_deferred: one window's columns
  dbuf rounds, sigs, sig_lens, prevs, prev_lens, rands, rand_lens, defer, verdict, rand_out, status;
  dbuf carry, carry_round, carry_len, carry_sig;  // the record before the window
  std::vector<uint8_t> h_defer;
  // protobuf handles (dh_archive_open_pb): the record kind, the expected beacon ID and the window's metadata bytes
  int kind = 0;
  bool has_id = false;
  uint32_t id_len = 0;
  dbuf d_id, meta;
  void release_buffers() override {
    for (dbuf* b : {&d_file, &cnt, &base, &scan_tmp, &line_off, &line_len, &chunks, &d_stat, &rounds, &sigs, &sig_lens, &prevs, &prev_lens,
                    &rands, &rand_lens, &defer, &verdict, &rand_out, &status, &carry, &carry_round, &carry_len, &carry_sig, &d_id, &meta})
      b->release();
  }
};
static int archive_enter(dh_archive* a) { return handle_enter(a, "archive", "dh_archive_close"); }

constexpr size_t ARCHIVE_CALL_ROWS = (size_t)4096 * 4096 - 2;  // as one store call

static int archive_open(dh_archive* a, const uint8_t* buf, size_t len) {
  int rc = ensure_device();
  if (rc) return rc;
  a->len = len;
  HIP_TRY(hipStreamCreateWithFlags(&a->st, hipStreamNonBlocking));
  if (!len) return DH_OK;
  {
    prof_wall p("archive_upload");
    HIP_TRY(a->d_file.ensure(len));
    HIP_TRY(hipMemcpyAsync(a->d_file.p, buf, len, hipMemcpyHostToDevice, a->st));
    HIP_TRY(hipStreamSynchronize(a->st));
  }
  const size_t ntiles = (len + dh::ARCHIVE_TILE - 1) / dh::ARCHIVE_TILE;
  {
    prof_wall p("archive_index");
    HIP_TRY(a->cnt.ensure(ntiles * 4));
    HIP_TRY(a->base.ensure((ntiles + 1) * 4));
    HIP_TRY(a->scan_tmp.ensure((ntiles / 4096 + 2) * 4));
    HIP_TRY(dh::launch_ndjson_count(a->d_file.as<uint8_t>(), len, ntiles, a->cnt.as<uint32_t>(), a->st));
    HIP_TRY(dh::launch_scan(a->cnt.as<uint32_t>(), ntiles, a->base.as<uint32_t>(), a->scan_tmp.as<uint32_t>(), a->st));
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, a->base.as<uint32_t>() + ntiles, 4, hipMemcpyDeviceToHost, a->st));
    HIP_TRY(hipStreamSynchronize(a->st));
    a->nrec = total;
    HIP_TRY(a->line_off.ensure((size_t)total * 8 + 8));
    HIP_TRY(a->line_len.ensure((size_t)total * 4 + 4));
    HIP_TRY(dh::launch_ndjson_index(a->d_file.as<uint8_t>(), len, ntiles, a->base.as<uint32_t>(), a->line_off.as<uint64_t>(),
                                    a->line_len.as<uint32_t>(), a->st));
    HIP_TRY(hipStreamSynchronize(a->st));
  }
  prof_wall p("archive_stat");
  uint64_t st5[5];
  HIP_TRY(a->chunks.ensure((a->nrec / 64 + 1) * sizeof(dh::archive_stat)));
  HIP_TRY(a->d_stat.ensure(sizeof st5));
  HIP_TRY(dh::launch_ndjson_stat(a->d_file.as<uint8_t>(), len, a->line_off.as<uint64_t>(), a->line_len.as<uint32_t>(), a->nrec, a->chunks.p,
                                 a->d_stat.as<uint64_t>(), a->st));
  HIP_TRY(hipMemcpyAsync(st5, a->d_stat.p, sizeof st5, hipMemcpyDeviceToHost, a->st));
  HIP_TRY(hipStreamSynchronize(a->st));
  a->stat[0] = a->nrec;
  memcpy(a->stat + 1, st5, sizeof st5);
  return DH_OK;
}

// records [first, first + n) of the archive into the columns; waits for the stream
static int archive_gather(dh_archive* a, uint64_t first, size_t n, const dh::archive_cols& c, uint8_t* meta = nullptr) {
  if (!n) return DH_OK;
  timed_launches tl(a->st);  // resolved after the stream wait below
  if (a->kind) {
    const dh::pb_meta_out x{meta, a->d_id.as<uint8_t>(), a->id_len};
    HIP_TRY(tl.run("k_pb_gather", [&] {
      return dh::launch_pb_gather(a->kind, a->d_file.as<uint8_t>(), a->len, a->line_off.as<uint64_t>() + first,
                                  a->line_len.as<uint32_t>() + first, n, c, x, a->st);
    }));
    HIP_TRY(hipStreamSynchronize(a->st));
    return DH_OK;
  }
  HIP_TRY(tl.run("k_ndjson_gather", [&] {
    return dh::launch_ndjson_gather(a->d_file.as<uint8_t>(), a->len, a->line_off.as<uint64_t>() + first, a->line_len.as<uint32_t>() + first, n,
                                    c, a->st);
  }));
  HIP_TRY(hipStreamSynchronize(a->st));
  return DH_OK;
}

static void archive_clamp(const dh_archive* a, uint64_t first, size_t* n) {
  if (first >= a->nrec) *n = 0;
  else if (*n > a->nrec - first) *n = (size_t)(a->nrec - first);
}

// the column refusals of the two chunk encoders; d_rands: the served form's digest column (null: none to align)
static int encode_cols_check(const uint64_t* d_rounds, const uint8_t* d_sigs, size_t sig_stride, const uint32_t* d_sig_lens, const uint8_t* d_prevs,
                             size_t prev_stride, const uint32_t* d_prev_lens, const uint8_t* d_rands, size_t n) {
  if (!d_prevs != !d_prev_lens) return fail(DH_EINVAL, "d_prevs and d_prev_lens are given together or not at all");
  if (n > ARCHIVE_CALL_ROWS) return fail(DH_EINVAL, "%zu rows: at most 16M rows per call: split the call", n);
  if (n && (!d_rounds || !d_sigs || !d_sig_lens)) return fail(DH_EINVAL, "null column");
  if (!sig_stride || (sig_stride & 3) || sig_stride > ((size_t)1 << 20) || ((uintptr_t)d_sigs & 3) || ((uintptr_t)d_rands & 3) ||
      (d_prevs && (!prev_stride || (prev_stride & 3) || prev_stride > ((size_t)1 << 20) || ((uintptr_t)d_prevs & 3))))
    return fail(DH_EINVAL, "rows are 4-byte aligned with strides %zu / %zu that are positive multiples of 4, at most 1 MiB", sig_stride, prev_stride);
  return DH_OK;
}

// The chunk encoders' driver (dh_pb_encode_device, dh_rand_encode_device) on the caller's stream: upload the metadata
// bytes (*meta_slot = their device address, read by both launches), measure every row (size), add up the chunks' bytes,
// scan the frame lengths and write the records (encode). want_out: false measures only.
struct encode_form {
  const char *wall, *size_name, *encode_name;  // dh_profile stages
  const char *one, *many;                      // what the refusals call a record
  bool stop_empty;                             // a call that measures 0 bytes ends before the scan
};
template <class Size, class Encode>
static int encode_chunks(const encode_form& f, const std::vector<uint8_t>& meta, const uint8_t** meta_slot, size_t n, hipStream_t st, Size size,
                         Encode encode, bool want_out, size_t cap, size_t* len_out) {
  int rc = ensure_device();
  if (rc) return rc;
  if (!n) return DH_OK;
  HIP_TRY(hipSetDevice(g_ctx.device));
  prof_wall p(f.wall);
  HIP_TRY(hipStreamSynchronize(st));  // the columns may be written there
  const size_t nsum = (n + 255) / 256;
  dbuf d_meta, frame, off, scan_tmp, sums;
  dbuf_pool pool{{&d_meta, &frame, &off, &scan_tmp, &sums}};
  HIP_TRY(d_meta.ensure(std::max<size_t>(meta.size(), 4)));
  HIP_TRY(frame.ensure(n * 4));
  HIP_TRY(off.ensure((n + 1) * 4));
  HIP_TRY(scan_tmp.ensure((n / 4096 + 2) * 4));
  HIP_TRY(sums.ensure(nsum * sizeof(dh::pb_size_sum)));
  if (!meta.empty()) HIP_TRY(hipMemcpyAsync(d_meta.p, meta.data(), meta.size(), hipMemcpyHostToDevice, st));
  *meta_slot = d_meta.as<uint8_t>();
  timed_launches tl(st);
  HIP_TRY(tl.run(f.size_name, [&] { return size(frame.as<uint32_t>(), sums.as<dh::pb_size_sum>()); }));
  std::vector<dh::pb_size_sum> h_sums(nsum);
  HIP_TRY(hipMemcpyAsync(h_sums.data(), sums.p, nsum * sizeof(dh::pb_size_sum), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  uint64_t total = 0;
  for (const dh::pb_size_sum& x : h_sums) {
    if (x.first_bad != ~0ull)
      return fail(DH_EINVAL, "row %llu: its %s would exceed 4096 bytes, or a length passes its row's stride", (unsigned long long)x.first_bad, f.one);
    total += x.bytes;
  }
  if (total >> 32) return fail(DH_EINVAL, "%llu bytes of %s: 4 GiB or more in one call: split the call", (unsigned long long)total, f.many);
  *len_out = (size_t)total;
  if (!want_out) return DH_OK;
  if (cap < total) return fail(DH_EINVAL, "%llu bytes of %s, room for %zu", (unsigned long long)total, f.many, cap);
  if (f.stop_empty && !total) return DH_OK;
  HIP_TRY(dh::launch_scan(frame.as<uint32_t>(), n, off.as<uint32_t>(), scan_tmp.as<uint32_t>(), st));
  HIP_TRY(tl.run(f.encode_name, [&] { return encode(off.as<uint32_t>()); }));
  HIP_TRY(hipStreamSynchronize(st));
  return DH_OK;
}

extern "C" {

int dh_archive_open_ndjson(const uint8_t* buf, size_t len, dh_archive** out) {
  if (!out || (len && !buf)) return fail(DH_EINVAL, "null argument");
  *out = nullptr;
  if (len > store_max_bytes())
    return fail(DH_ENOMEM, "archive of %zu bytes exceeds DRANDHIP_STORE_MAX_BYTES (%zu): keep the host reader", len, store_max_bytes());
  if (len >> 33) return fail(DH_ENOMEM, "archive of %zu bytes: at most 8 GiB per handle (the record index is 32 bits wide): split it at a newline", len);
  if (len && dh::bolt::rdjson_is_array(dh::bolt::view{buf, (uint64_t)len}))
    return fail(DH_EINVAL, "the archive starts with '[': the JSON-array form is not framed on the device, keep the host reader");
  dh_archive* a = new dh_archive();
  int rc = archive_open(a, buf, len);
  if (rc) {
    a->release();
    delete a;
    return rc;
  }
  handle_register(a);
  *out = a;
  return DH_OK;
}

int dh_archive_open_pb(int kind, const uint8_t* buf, size_t len, const uint64_t* rec_off, const uint32_t* rec_len, size_t n_rec, dh_archive** out) {
  if (!out || (len && !buf) || (n_rec && !rec_len)) return fail(DH_EINVAL, "null argument");
  *out = nullptr;
  if (kind != DH_PB_BEACON_PACKET && kind != DH_PB_PUBLIC_RAND) return fail(DH_EINVAL, "unknown record kind %d", kind);
  if (len > store_max_bytes())
    return fail(DH_ENOMEM, "archive of %zu bytes exceeds DRANDHIP_STORE_MAX_BYTES (%zu): keep the host reader", len, store_max_bytes());
  if (len >> 33) return fail(DH_ENOMEM, "archive of %zu bytes: at most 8 GiB per handle: split it between two records", len);
  if (n_rec >> 32) return fail(DH_ENOMEM, "%zu records: the record index is 32 bits wide: split the buffer", n_rec);
  // the offsets, summed or checked here in 64 bits: ascending, no overlap, every record inside the buffer
  std::vector<uint64_t> off(n_rec + 1);
  uint64_t at = 0;
  for (size_t i = 0; i < n_rec; i++) {
    const uint64_t o = rec_off ? rec_off[i] : at;
    if (o < at || o > len || rec_len[i] > len - o)
      return fail(DH_EINVAL, "record %zu ([%llu, +%u)) lies outside the buffer of %zu bytes or before the end of record %zu - 1", i,
                  (unsigned long long)o, rec_len[i], len, i);
    off[i] = o;
    at = o + rec_len[i];
  }
  if (!rec_off && at != len) return fail(DH_EINVAL, "the %zu record lengths sum to %llu, the buffer holds %zu bytes", n_rec, (unsigned long long)at, len);
  int rc = ensure_device();
  if (rc) return rc;
  dh_archive* a = new dh_archive();
  a->kind = kind;
  a->len = len;
  a->nrec = n_rec;
  a->stat[6] = 0;
  auto open = [&]() -> int {
    HIP_TRY(hipStreamCreateWithFlags(&a->st, hipStreamNonBlocking));
    {
      prof_wall p("archive_upload");
      HIP_TRY(a->d_file.ensure(std::max<size_t>(len, 16)));
      HIP_TRY(a->line_off.ensure(n_rec * 8 + 8));
      HIP_TRY(a->line_len.ensure(n_rec * 4 + 4));
      HIP_TRY(a->d_id.ensure(16));
      if (len) HIP_TRY(hipMemcpyAsync(a->d_file.p, buf, len, hipMemcpyHostToDevice, a->st));
      if (n_rec) {
        HIP_TRY(hipMemcpyAsync(a->line_off.p, off.data(), n_rec * 8, hipMemcpyHostToDevice, a->st));
        HIP_TRY(hipMemcpyAsync(a->line_len.p, rec_len, n_rec * 4, hipMemcpyHostToDevice, a->st));
      }
      HIP_TRY(hipStreamSynchronize(a->st));
    }
    prof_wall p("archive_stat");
    uint64_t st5[5];
    HIP_TRY(a->chunks.ensure((n_rec / 64 + 1) * sizeof(dh::archive_stat)));
    HIP_TRY(a->d_stat.ensure(sizeof st5));
    HIP_TRY(dh::launch_pb_stat(kind, a->d_file.as<uint8_t>(), len, a->line_off.as<uint64_t>(), a->line_len.as<uint32_t>(), n_rec, a->chunks.p,
                               a->d_stat.as<uint64_t>(), a->st));
    HIP_TRY(hipMemcpyAsync(st5, a->d_stat.p, sizeof st5, hipMemcpyDeviceToHost, a->st));
    HIP_TRY(hipStreamSynchronize(a->st));
    a->stat[0] = n_rec;
    memcpy(a->stat + 1, st5, sizeof st5);
    return DH_OK;
  };
  if ((rc = open())) {
    a->release();
    delete a;
    return rc;
  }
  handle_register(a);
  *out = a;
  return DH_OK;
}

int dh_archive_kind(const dh_archive* a) { return a ? a->kind : fail(DH_EINVAL, "null argument"); }

int dh_archive_set_beacon_id(dh_archive* a, const uint8_t* id, size_t id_len) {
  if (!a) return fail(DH_EINVAL, "null argument");
  if (id_len > dh::bolt::PBWIRE_MAX_RECORD) return fail(DH_EINVAL, "beacon ID of %zu bytes: no record of 4096 bytes holds it", id_len);
  handle_guard g(a);
  int rc = archive_enter(a);
  if (rc) return rc;
  a->has_id = id != nullptr;
  a->id_len = id ? (uint32_t)id_len : 0;
  if (a->id_len) {
    HIP_TRY(a->d_id.ensure(a->id_len));
    HIP_TRY(hipMemcpy(a->d_id.p, id, a->id_len, hipMemcpyHostToDevice));
  }
  return DH_OK;
}

int dh_pb_frame_delimited(const uint8_t* buf, size_t len, uint64_t* off_out, uint32_t* len_out, size_t cap, size_t* n_out,
                          size_t* consumed_out) {
  if (!n_out || !consumed_out || (len && !buf) || (cap && (!off_out || !len_out))) return fail(DH_EINVAL, "null argument");
  uint64_t consumed = 0;
  const uint64_t n = dh::bolt::pb_frame_delimited(dh::bolt::view{buf, (uint64_t)len}, off_out, len_out, cap, &consumed);
  *n_out = (size_t)n;
  if (n > cap) {
    *consumed_out = 0;
    return fail(DH_EINVAL, "%llu records, room for %zu", (unsigned long long)n, cap);
  }
  *consumed_out = (size_t)consumed;
  return DH_OK;
}

int dh_pb_encode_device(int kind, const uint64_t* d_rounds, const uint8_t* d_sigs, size_t sig_stride, const uint32_t* d_sig_lens,
                        const uint8_t* d_prevs, size_t prev_stride, const uint32_t* d_prev_lens, size_t n, const uint8_t* beacon_id,
                        size_t beacon_id_len, int delimited, uint8_t* d_out, size_t cap, uint32_t* d_rec_len_out, size_t* len_out,
                        void* hip_stream) {
  if (!len_out) return fail(DH_EINVAL, "null argument");
  *len_out = 0;
  if (kind != DH_PB_BEACON_PACKET)
    return fail(DH_EINVAL, "record kind %d: only BeaconPacket (%d) is encoded (PublicRandResponse needs the randomness digest)", kind,
                DH_PB_BEACON_PACKET);
  int rc = encode_cols_check(d_rounds, d_sigs, sig_stride, d_sig_lens, d_prevs, prev_stride, d_prev_lens, nullptr, n);
  if (rc) return rc;
  // the metadata field, the same for every row: 22 M [12 L id]
  std::vector<uint8_t> meta;
  auto varint = [&](uint64_t v) {
    for (; v >> 7; v >>= 7) meta.push_back((uint8_t)(v | 0x80));
    meta.push_back((uint8_t)v);
  };
  if (beacon_id) {
    if (beacon_id_len > dh::bolt::PBWIRE_MAX_RECORD) return fail(DH_EINVAL, "beacon ID of %zu bytes: a record holds at most 4096", beacon_id_len);
    std::vector<uint8_t> inner;
    std::swap(inner, meta);
    if (beacon_id_len) {
      meta.push_back(0x12);
      varint(beacon_id_len);
      meta.insert(meta.end(), beacon_id, beacon_id + beacon_id_len);
    }
    std::swap(inner, meta);
    meta.push_back(0x22);
    varint(inner.size());
    meta.insert(meta.end(), inner.begin(), inner.end());
  }
  dh::pb_encode_in e{d_rounds, d_sigs, d_sig_lens, d_prevs, d_prev_lens, nullptr, (uint32_t)sig_stride,
                     (uint32_t)(d_prevs ? prev_stride : 4), (uint32_t)meta.size(), delimited ? 1u : 0u};
  const hipStream_t st = (hipStream_t)hip_stream;
  static const encode_form enc{"packet_encode", "k_pb_size", "k_pb_encode", "packet", "packets", false};
  return encode_chunks(
      enc, meta, &e.meta, n, st,
      [&](uint32_t* frame, dh::pb_size_sum* sums) { return dh::launch_pb_size(e, n, d_rec_len_out, frame, sums, st); },
      [&](const uint32_t* off) { return dh::launch_pb_encode(e, n, off, d_out, st); }, d_out != nullptr, cap, len_out);
}

int dh_rand_encode_device(int form, const uint64_t* d_rounds, const uint8_t* d_sigs, size_t sig_stride, const uint32_t* d_sig_lens,
                          const uint8_t* d_prevs, size_t prev_stride, const uint32_t* d_prev_lens, const uint8_t* d_rands, const uint8_t* d_keep,
                          size_t n, const uint8_t* metadata, size_t metadata_len, int flags, uint8_t* d_out, size_t cap, uint32_t* d_rec_len_out,
                          size_t* len_out, void* hip_stream) {
  if (!len_out) return fail(DH_EINVAL, "null argument");
  *len_out = 0;
  if (form != DH_ENC_RANDOM_DATA_JSON && form != DH_ENC_PUBLIC_RAND_PB)
    return fail(DH_EINVAL, "form %d: RandomData JSON (%d) and PublicRandResponse (%d) are encoded", form, DH_ENC_RANDOM_DATA_JSON, DH_ENC_PUBLIC_RAND_PB);
  const bool json = form == DH_ENC_RANDOM_DATA_JSON;
  if (json && metadata) return fail(DH_EINVAL, "a RandomData record holds no metadata");
  if (flags & ~(json ? DH_ENC_NEWLINE : DH_ENC_DELIMITED))
    return fail(DH_EINVAL, "flags %d: DH_ENC_NEWLINE goes with the JSON form only, DH_ENC_DELIMITED with the protobuf form only", flags);
  int rc = encode_cols_check(d_rounds, d_sigs, sig_stride, d_sig_lens, d_prevs, prev_stride, d_prev_lens, d_rands, n);
  if (rc) return rc;
  // the metadata field, the same for every row: 2A M and the caller's marshalled common.Metadata
  std::vector<uint8_t> meta;
  if (metadata) {
    if (metadata_len > dh::bolt::PBWIRE_MAX_RECORD) return fail(DH_EINVAL, "metadata of %zu bytes: a record holds at most 4096", metadata_len);
    meta.push_back(0x2A);
    for (size_t v = metadata_len; ; v >>= 7) {
      meta.push_back((uint8_t)(v >> 7 ? (v | 0x80) : v));
      if (!(v >> 7)) break;
    }
    meta.insert(meta.end(), metadata, metadata + metadata_len);
  }
  dh::serve_encode_in e{d_rounds, d_sigs, d_sig_lens, d_prevs, d_prev_lens, d_rands, d_keep, nullptr, (uint32_t)sig_stride,
                        (uint32_t)(d_prevs ? prev_stride : 4), (uint32_t)meta.size(),
                        json ? dh::SERVE_RANDOM_DATA_JSON : dh::SERVE_PUBLIC_RAND_PB, flags ? 1u : 0u};
  const hipStream_t st = (hipStream_t)hip_stream;
  // stop_empty: a call whose rows are all dropped (d_keep) writes nothing, so no scan and no encode pass
  static const encode_form enc{"serve_encode", "k_serve_size", "k_serve_encode", "record", "records", true};
  return encode_chunks(
      enc, meta, &e.meta, n, st,
      [&](uint32_t* frame, dh::pb_size_sum* sums) { return dh::launch_serve_size(e, n, d_rec_len_out, frame, sums, st); },
      [&](const uint32_t* off) { return dh::launch_serve_encode(e, n, off, d_out, st); }, d_out != nullptr, cap, len_out);
}

int dh_archive_stat(const dh_archive* a, uint64_t out[7]) {
  if (!a || !out) return fail(DH_EINVAL, "null argument");
  memcpy(out, a->stat, sizeof a->stat);  // fixed at open
  return DH_OK;
}

void dh_archive_close(dh_archive* a) { handle_close(a); }

int dh_archive_lines(dh_archive* a, uint64_t first_rec, size_t n_rec, uint64_t* off_out, uint32_t* len_out) {
  if (!a) return fail(DH_EINVAL, "null argument");
  handle_guard g(a);
  int rc = archive_enter(a);
  if (rc) return rc;
  archive_clamp(a, first_rec, &n_rec);
  if (!n_rec) return DH_OK;
  if (!off_out || !len_out) return fail(DH_EINVAL, "null output");
  HIP_TRY(hipMemcpy(off_out, a->line_off.as<uint64_t>() + first_rec, n_rec * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(len_out, a->line_len.as<uint32_t>() + first_rec, n_rec * 4, hipMemcpyDeviceToHost));
  return DH_OK;
}

int dh_archive_deferred(dh_archive* a, uint64_t first_rec, size_t n_rec, uint64_t* idx_out, size_t cap, size_t* n_out) {
  if (!a || !n_out || (cap && !idx_out)) return fail(DH_EINVAL, "null argument");
  handle_guard g(a);
  int rc = archive_enter(a);
  if (rc) return rc;
  *n_out = 0;
  archive_clamp(a, first_rec, &n_rec);
  if (!n_rec || !a->stat[1]) return DH_OK;
  size_t n = 0;
  const size_t win = (size_t)1 << 20;
  for (size_t at = 0; at < n_rec; at += win) {
    const size_t m = std::min(win, n_rec - at);
    HIP_TRY(a->rounds.ensure(m * 8));
    HIP_TRY(a->defer.ensure(m));
    const dh::archive_cols c{a->rounds.as<uint64_t>(), a->defer.as<uint8_t>(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 4, 4};
    if ((rc = archive_gather(a, first_rec + at, m, c))) return rc;
    a->h_defer.resize(m);
    HIP_TRY(hipMemcpy(a->h_defer.data(), a->defer.p, m, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < m; i++) {
      if (!a->h_defer[i]) continue;
      if (n < cap) idx_out[n] = first_rec + at + i;
      n++;
    }
  }
  *n_out = n;
  if (n > cap) return fail(DH_EINVAL, "%zu deferred records, room for %zu", n, cap);
  return DH_OK;
}

int dh_archive_beacons_device(dh_archive* a, uint64_t first_rec, size_t n_rec, size_t sig_stride, size_t prev_stride, uint64_t* d_rounds,
                              uint8_t* d_sigs, uint32_t* d_sig_lens, uint8_t* d_prevs, uint32_t* d_prev_lens, uint8_t* d_rands,
                              uint32_t* d_rand_lens, uint8_t* d_deferred, size_t* n_out, void* hip_stream) {
  if (!a || !n_out) return fail(DH_EINVAL, "null argument");
  const bool want_prev = d_prevs || d_prev_lens;
  if (!sig_stride || (sig_stride & 3) || sig_stride > ((size_t)1 << 20) ||
      (want_prev && (!prev_stride || (prev_stride & 3) || prev_stride > ((size_t)1 << 20))))
    return fail(DH_EINVAL, "row strides %zu / %zu: positive multiples of 4, at most 1 MiB", sig_stride, prev_stride);
  if (!d_prevs != !d_prev_lens) return fail(DH_EINVAL, "d_prevs and d_prev_lens are given together or not at all");
  if (!d_rands != !d_rand_lens) return fail(DH_EINVAL, "d_rands and d_rand_lens are given together or not at all");
  handle_guard g(a);
  int rc = archive_enter(a);
  if (rc) return rc;
  prof_wall p("archive_gather");
  if (hip_stream) HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));  // the output buffers may be in use there
  archive_clamp(a, first_rec, &n_rec);
  *n_out = n_rec;
  if (n_rec > ARCHIVE_CALL_ROWS) return fail(DH_EINVAL, "window of %zu records: at most 16M records per call", n_rec);
  if (n_rec && (!d_rounds || !d_sigs || !d_sig_lens || !d_deferred)) return fail(DH_EINVAL, "null output");
  const dh::archive_cols c{d_rounds, d_deferred, d_sigs, d_sig_lens, d_prevs, d_prev_lens, d_rands, d_rand_lens, (uint32_t)sig_stride,
                           (uint32_t)(want_prev ? prev_stride : 4)};
  return archive_gather(a, first_rec, n_rec, c);
}

int dh_archive_check(dh_archive* a, int scheme, const uint8_t* pk, size_t pk_len, uint64_t first_rec, size_t n_rec,
                     const uint64_t* anchor_round, const uint8_t* anchor_sig, size_t anchor_sig_len, size_t window, uint64_t seed,
                     uint8_t* status_out, uint64_t counts_out[6]) {
  if (!a || !pk || !counts_out) return fail(DH_EINVAL, "null argument");
  if (scheme < 0 || scheme > 3) return fail(DH_EINVAL, "unknown scheme %d", scheme);
  if (!window) return fail(DH_EINVAL, "window must be >= 1");
  if (anchor_round && anchor_sig_len && !anchor_sig) return fail(DH_EINVAL, "null anchor signature");
  const uint32_t sig_len = (uint32_t)dh_sig_len(scheme);
  const bool chained = scheme == DH_SCHEME_CHAINED;
  handle_guard g(a);
  int rc = archive_enter(a);
  if (rc) return rc;
  memset(counts_out, 0, 6 * sizeof(uint64_t));
  archive_clamp(a, first_rec, &n_rec);
  if (!n_rec) return DH_OK;
  if (!status_out) return fail(DH_EINVAL, "null output");
  window = std::min(window, ARCHIVE_CALL_ROWS);
  const bool use_anchor = first_rec == 0 && anchor_round;
  const uint64_t longest = std::max<uint64_t>(std::max<uint64_t>(sig_len, a->stat[3]),
                                              std::max<uint64_t>(chained ? a->stat[4] : 0, use_anchor ? anchor_sig_len : 0));
  const size_t stride = ((size_t)longest + 3) & ~(size_t)3;
  if (stride > 65536)
    return fail(DH_EINVAL, "row stride %zu above 64 KiB (a %llu-byte field): keep the host reader", stride, (unsigned long long)longest);
  HIP_TRY(a->carry.ensure(8));
  HIP_TRY(a->carry_round.ensure(8));
  HIP_TRY(a->carry_len.ensure(8));
  HIP_TRY(a->carry_sig.ensure(stride));
  const size_t wmax = std::min(window, n_rec);
  HIP_TRY(a->rounds.ensure(wmax * 8));
  HIP_TRY(a->sigs.ensure(wmax * stride));
  HIP_TRY(a->sig_lens.ensure(wmax * 4));
  if (chained) {
    HIP_TRY(a->prevs.ensure(wmax * stride));
    HIP_TRY(a->prev_lens.ensure(wmax * 4));
  }
  HIP_TRY(a->rands.ensure(wmax * 32));
  HIP_TRY(a->rand_lens.ensure(wmax * 4));
  HIP_TRY(a->defer.ensure(wmax));
  HIP_TRY(a->verdict.ensure(wmax));
  HIP_TRY(a->rand_out.ensure(wmax * 32));
  HIP_TRY(a->status.ensure(wmax));
  uint8_t* meta = nullptr;  // the beacon-ID check of tryNode: protobuf handles with an expected ID only
  if (a->kind && a->has_id) {
    HIP_TRY(a->meta.ensure(wmax));
    meta = a->meta.as<uint8_t>();
  }
  const dh::archive_cols c{a->rounds.as<uint64_t>(), a->defer.as<uint8_t>(), a->sigs.as<uint8_t>(), a->sig_lens.as<uint32_t>(),
                           chained ? a->prevs.as<uint8_t>() : nullptr, chained ? a->prev_lens.as<uint32_t>() : nullptr,
                           a->rands.as<uint8_t>(), a->rand_lens.as<uint32_t>(), (uint32_t)stride, (uint32_t)stride};
  // row `last` of the window's columns becomes the carried predecessor (stream order: before the next gather)
  auto carry_row = [&](size_t last) -> int {
    HIP_TRY(hipMemsetAsync(a->carry.p, 1, 1, a->st));
    HIP_TRY(hipMemcpyAsync(a->carry.as<uint8_t>() + 1, a->defer.as<uint8_t>() + last, 1, hipMemcpyDeviceToDevice, a->st));
    HIP_TRY(hipMemcpyAsync(a->carry_round.p, a->rounds.as<uint64_t>() + last, 8, hipMemcpyDeviceToDevice, a->st));
    HIP_TRY(hipMemcpyAsync(a->carry_len.p, a->sig_lens.as<uint32_t>() + last, 4, hipMemcpyDeviceToDevice, a->st));
    HIP_TRY(hipMemcpyAsync(a->carry_sig.p, a->sigs.as<uint8_t>() + last * stride, stride, hipMemcpyDeviceToDevice, a->st));
    return DH_OK;
  };
  HIP_TRY(hipMemsetAsync(a->carry.p, 0, 8, a->st));
  if (first_rec > 0) {  // the predecessor of the first record checked is the archive's record before it
    if ((rc = archive_gather(a, first_rec - 1, 1, c)) || (rc = carry_row(0))) return rc;
  } else if (use_anchor) {
    const uint32_t al = (uint32_t)anchor_sig_len;
    HIP_TRY(hipMemsetAsync(a->carry.p, 1, 1, a->st));
    HIP_TRY(hipMemsetAsync(a->carry_sig.p, 0, stride, a->st));
    HIP_TRY(hipMemcpyAsync(a->carry_round.p, anchor_round, 8, hipMemcpyHostToDevice, a->st));
    HIP_TRY(hipMemcpyAsync(a->carry_len.p, &al, 4, hipMemcpyHostToDevice, a->st));
    if (al) HIP_TRY(hipMemcpyAsync(a->carry_sig.p, anchor_sig, al, hipMemcpyHostToDevice, a->st));
    HIP_TRY(hipStreamSynchronize(a->st));  // `al` is on this frame
  }
  for (size_t at = 0; at < n_rec; at += window) {
    const size_t m = std::min(window, n_rec - at);
    {
      prof_wall p("archive_gather");
      if ((rc = archive_gather(a, first_rec + at, m, c, meta))) return rc;
    }
    {
      prof_wall p("archive_verify");
      // a deferred row is verified as the all-zero record it was left as, and its verdict is not read; the chained
      // scheme verifies each record against its OWN previous_signature (client/verify.go:171-199, non-strict)
      rc = dh_verify_batch_device(scheme, pk, pk_len, a->rounds.as<uint64_t>(), a->sigs.as<uint8_t>(), stride,
                                  chained ? a->prevs.as<uint8_t>() : nullptr, stride, chained ? a->prev_lens.as<uint32_t>() : nullptr, m,
                                  a->verdict.as<uint8_t>(), a->rand_out.as<uint8_t>(), seed, nullptr, nullptr);
      if (rc) return rc;
    }
    prof_wall p("archive_fold");
    const dh::archive_fold_in f{m, sig_len, chained ? 1u : 0u, (uint32_t)stride, (uint32_t)stride, a->verdict.as<uint8_t>(),
                                a->rand_out.as<uint8_t>(), c.rounds, c.deferred, c.sigs, c.sig_lens, c.prevs, c.prev_lens, c.rands, c.rand_lens,
                                a->carry.as<uint8_t>(), a->carry_round.as<uint64_t>(), a->carry_len.as<uint32_t>(), a->carry_sig.as<uint8_t>(), meta};
    HIP_TRY(dh::launch_archive_fold(f, a->status.as<uint8_t>(), a->st));
    HIP_TRY(hipMemcpyAsync(status_out + at, a->status.p, m, hipMemcpyDeviceToHost, a->st));
    if ((rc = carry_row(m - 1))) return rc;
    HIP_TRY(hipStreamSynchronize(a->st));
  }
  for (size_t i = 0; i < n_rec; i++) {
    const uint8_t s = status_out[i];
    counts_out[1] += s & DH_AR_DEFERRED ? 1 : 0;
    counts_out[2] += s & DH_AR_INVALID ? 1 : 0;
    counts_out[3] += s & DH_AR_RANDOMNESS ? 1 : 0;
    counts_out[4] += s & DH_AR_SEQUENCE ? 1 : 0;
    counts_out[5] += s & DH_AR_LINK ? 1 : 0;
  }
  counts_out[0] = n_rec;
  return counts_out[1] ? DH_DEFERRED : DH_OK;
}

}  // extern "C"

// ---- one chain from unordered candidate columns (k_assemble.hip): cut the skipped and stale
// candidates, sort the rest by round (stable, so a run keeps the input order), collapse the copies inside a run, verify
// each representative once through dh_verify_batch_device, pick the first valid representative per round

namespace {

// (keys, idx)[0, n) sorted by key, stably, through (keys_alt, idx_alt); *in_alt: the result lies in the alt pair. A
// pass whose digit is the same in every key moves nothing and is skipped. Ends with the stream idle only when n < 2.
int sort_pairs(uint64_t* keys, uint32_t* idx, uint64_t* keys_alt, uint32_t* idx_alt, size_t n, dbuf& cnt, dbuf& off, dbuf& scan_tmp, dbuf& orand,
               hipStream_t st, bool* in_alt) {
  *in_alt = false;
  if (n < 2) return DH_OK;
  uint64_t h[2] = {0, ~0ull};
  HIP_TRY(orand.ensure(16));
  HIP_TRY(hipMemcpyAsync(orand.p, h, 16, hipMemcpyHostToDevice, st));
  timed_launches tl(st);
  HIP_TRY(tl.run("k_sort_orand", [&] { return dh::launch_sort_orand(keys, n, orand.as<uint64_t>(), st); }));
  HIP_TRY(hipStreamSynchronize(st));  // `h` was read by then
  HIP_TRY(hipMemcpyAsync(h, orand.p, 16, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint64_t varies = h[0] ^ h[1];
  const size_t nk = 256 * ((n + dh::SORT_TILE - 1) / dh::SORT_TILE);
  HIP_TRY(cnt.ensure(nk * 4));
  HIP_TRY(off.ensure((nk + 1) * 4));
  HIP_TRY(scan_tmp.ensure((nk / 4096 + 2) * 4));
  for (uint32_t shift = 0; shift < 64; shift += 8) {
    if (!((varies >> shift) & 255)) continue;
    HIP_TRY(tl.run("k_sort_pass", [&] {  // histogram, scan and scatter of one digit
      return dh::launch_sort_pass(keys, idx, n, shift, cnt.as<uint32_t>(), off.as<uint32_t>(), scan_tmp.as<uint32_t>(), keys_alt, idx_alt, st);
    }));
    std::swap(keys, keys_alt);
    std::swap(idx, idx_alt);
    *in_alt = !*in_alt;
  }
  return DH_OK;
}

}  // namespace

extern "C" {

int dh_sort_rounds_debug(const uint64_t* keys, size_t n, uint32_t* perm_out) {
  if (n == 0) return DH_OK;
  if (!keys || !perm_out) return fail(DH_EINVAL, "null argument");
  if (n > ARCHIVE_CALL_ROWS) return fail(DH_EINVAL, "%zu keys: at most 16M per call", n);
  int rc = ensure_device();
  if (rc) return rc;
  dbuf k[2], ix[2], cnt, off, scan_tmp, orand;
  dbuf_pool pool{{&k[0], &k[1], &ix[0], &ix[1], &cnt, &off, &scan_tmp, &orand}};
  HIP_TRY(hipStreamCreateWithFlags(&pool.st, hipStreamNonBlocking));
  hipStream_t st = pool.st;
  for (int i = 0; i < 2; i++) {
    HIP_TRY(k[i].ensure(n * 8));
    HIP_TRY(ix[i].ensure(n * 4));
  }
  HIP_TRY(hipMemcpyAsync(k[0].p, keys, n * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(dh::launch_iota(ix[0].as<uint32_t>(), n, st));
  bool in_alt = false;
  if ((rc = sort_pairs(k[0].as<uint64_t>(), ix[0].as<uint32_t>(), k[1].as<uint64_t>(), ix[1].as<uint32_t>(), n, cnt, off, scan_tmp, orand, st,
                       &in_alt)))
    return rc;
  HIP_TRY(hipMemcpyAsync(perm_out, ix[in_alt].p, n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DH_OK;
}

int dh_assemble_device(int scheme, const uint8_t* pk, size_t pk_len, const uint64_t* d_rounds, const uint8_t* d_sigs, size_t sig_stride,
                       const uint32_t* d_sig_lens, const uint8_t* d_prevs, size_t prev_stride, const uint32_t* d_prev_lens, const uint8_t* d_skip,
                       size_t n, const uint64_t* anchor_round, const uint8_t* anchor_sig, size_t anchor_sig_len, const uint64_t* up_to,
                       size_t window, uint64_t seed, uint64_t* d_rounds_out, uint8_t* d_sigs_out, uint32_t* d_sig_lens_out, uint8_t* d_prevs_out,
                       uint32_t* d_prev_lens_out, uint32_t* d_src_out, uint8_t* d_flags_out, size_t* m_out, uint8_t* status_out,
                       uint64_t* gap_first_out, uint64_t* gap_last_out, size_t gap_cap, size_t* n_gaps_out, uint64_t counts_out[10],
                       void* hip_stream) {
  if (!pk || !m_out || !n_gaps_out || !counts_out) return fail(DH_EINVAL, "null argument");
  *m_out = 0;
  *n_gaps_out = 0;
  memset(counts_out, 0, 10 * sizeof(uint64_t));
  if (scheme < 0 || scheme > 3) return fail(DH_EINVAL, "unknown scheme %d", scheme);
  if (!window) return fail(DH_EINVAL, "window must be >= 1");
  if (n > ARCHIVE_CALL_ROWS) return fail(DH_EINVAL, "%zu candidates: at most 16M rows per call", n);
  const bool chained = scheme == DH_SCHEME_CHAINED;
  if (!d_prevs != !d_prev_lens) return fail(DH_EINVAL, "d_prevs and d_prev_lens are given together or not at all");
  if (!d_prevs_out != !d_prev_lens_out) return fail(DH_EINVAL, "d_prevs_out and d_prev_lens_out are given together or not at all");
  if (!chained) d_prevs = nullptr, d_prev_lens = nullptr;  // the unchained schemes read no previous signature
  if (chained && n && !d_prevs) return fail(DH_EINVAL, "the chained scheme needs the previous_signature columns");
  if (!chained && d_prevs_out) return fail(DH_EINVAL, "previous_signature output columns go with the chained scheme only");
  if (!sig_stride || (sig_stride & 3) || sig_stride > ((size_t)1 << 20) || ((uintptr_t)d_sigs & 3) || ((uintptr_t)d_sigs_out & 3) ||
      (d_prevs && (!prev_stride || (prev_stride & 3) || prev_stride > ((size_t)1 << 20) || ((uintptr_t)d_prevs & 3) || ((uintptr_t)d_prevs_out & 3))))
    return fail(DH_EINVAL, "rows are 4-byte aligned with strides %zu / %zu that are positive multiples of 4, at most 1 MiB", sig_stride, prev_stride);
  if (n && (!d_rounds || !d_sigs || !d_sig_lens)) return fail(DH_EINVAL, "null column");
  if (n && (!d_rounds_out || !d_sigs_out || !d_sig_lens_out || !d_src_out || !d_flags_out || !status_out)) return fail(DH_EINVAL, "null output");
  if (anchor_round && anchor_sig_len && !anchor_sig) return fail(DH_EINVAL, "null anchor signature");
  if (anchor_sig_len > ((size_t)1 << 20)) return fail(DH_EINVAL, "anchor signature of %zu bytes: at most 1 MiB", anchor_sig_len);
  if (gap_cap && (!gap_first_out || !gap_last_out)) return fail(DH_EINVAL, "null gap arrays");
  const uint32_t want = (uint32_t)dh_sig_len(scheme);
  const char* env = getenv("DRANDHIP_ASSEMBLE_DEDUPE");  // read at every call: 0 makes every candidate a representative
  const bool dedupe = !(env && env[0] == '0' && !env[1]);
  window = std::min(window, ARCHIVE_CALL_ROWS);
  int rc = ensure_device();
  if (rc) return rc;
  if (hip_stream) HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));  // the columns may be written there
  dbuf status, live, pos, k[2], ix[2], cnt, off, scan_tmp, orand, run_start, rep, rpos, rep_cand, chosen, opos, v_rounds, v_sigs, v_prevs,
      v_prev_lens, verdict, anchor, gaps;
  dbuf_pool pool{{&status, &live, &pos, &k[0], &k[1], &ix[0], &ix[1], &cnt, &off, &scan_tmp, &orand, &run_start, &rep, &rpos, &rep_cand,
                  &chosen, &opos, &v_rounds, &v_sigs, &v_prevs, &v_prev_lens, &verdict, &anchor, &gaps}};
  HIP_TRY(hipStreamCreateWithFlags(&pool.st, hipStreamNonBlocking));
  hipStream_t st = pool.st;
  const dh::assemble::cols c{d_rounds, d_sigs, d_sig_lens, d_prevs, d_prev_lens, d_skip, (uint32_t)sig_stride, (uint32_t)(d_prevs ? prev_stride : 4)};
  const dh::assemble::bounds b{anchor_round ? *anchor_round : 0, up_to ? *up_to : 0, anchor_round ? 1u : 0u, up_to ? 1u : 0u};
  size_t m = 0, n_runs = 0, n_rep = 0, n_out = 0;
  bool in_alt = false;
  HIP_TRY(scan_tmp.ensure(((std::max(n, (size_t)256 * ((n + dh::SORT_TILE - 1) / dh::SORT_TILE)) + 2) / 4096 + 2) * 4));
  {
    prof_wall p("assemble_sort");
    HIP_TRY(status.ensure(n));
    HIP_TRY(live.ensure((n + 2) * 4));
    HIP_TRY(pos.ensure((n + 2) * 4));
    HIP_TRY(dh::launch_assemble_pre(c, n, b, status.as<uint8_t>(), live.as<uint32_t>(), st));
    if (n) {
      HIP_TRY(dh::launch_scan(live.as<uint32_t>(), n, pos.as<uint32_t>(), scan_tmp.as<uint32_t>(), st));
      uint32_t total = 0;
      HIP_TRY(hipMemcpyAsync(&total, pos.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      m = total;
    }
    for (int i = 0; i < 2; i++) {
      HIP_TRY(k[i].ensure(m * 8));
      HIP_TRY(ix[i].ensure(m * 4));
    }
    if (m) HIP_TRY(dh::launch_assemble_cut(d_rounds, n, pos.as<uint32_t>(), k[0].as<uint64_t>(), ix[0].as<uint32_t>(), st));
    if ((rc = sort_pairs(k[0].as<uint64_t>(), ix[0].as<uint32_t>(), k[1].as<uint64_t>(), ix[1].as<uint32_t>(), m, cnt, off, scan_tmp, orand, st,
                         &in_alt)))
      return rc;
    HIP_TRY(hipStreamSynchronize(st));
  }
  const uint64_t* keys = k[in_alt].as<uint64_t>();
  const uint32_t* idx = ix[in_alt].as<uint32_t>();
  uint32_t* flag = live.as<uint32_t>();   // heads, then representatives, then chosen rows, then gaps: m + 1 words at most
  uint32_t* runs = pos.as<uint32_t>();    // the scanned heads: the cut has read pos by now (stream order)
  {
    prof_wall p("assemble_class");
    HIP_TRY(dh::launch_assemble_heads(keys, m, flag, st));
    if (m) {
      HIP_TRY(dh::launch_scan(flag, m, runs, scan_tmp.as<uint32_t>(), st));
      uint32_t total = 0;
      HIP_TRY(hipMemcpyAsync(&total, runs + m, 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      n_runs = total;
    }
    HIP_TRY(run_start.ensure(n_runs * 4));
    HIP_TRY(rep.ensure(m * 4));
    HIP_TRY(rpos.ensure((m + 1) * 4));
    HIP_TRY(dh::launch_assemble_runs(runs, m, run_start.as<uint32_t>(), st));
    HIP_TRY(dh::launch_assemble_class(c, idx, runs, run_start.as<uint32_t>(), m, dedupe, rep.as<uint32_t>(), flag, st));
    if (m) {
      HIP_TRY(dh::launch_scan(flag, m, rpos.as<uint32_t>(), scan_tmp.as<uint32_t>(), st));
      uint32_t total = 0;
      HIP_TRY(hipMemcpyAsync(&total, rpos.as<uint32_t>() + m, 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      n_rep = total;
    }
    HIP_TRY(rep_cand.ensure(n_rep * 4));
    HIP_TRY(dh::launch_assemble_reps(idx, rpos.as<uint32_t>(), m, rep_cand.as<uint32_t>(), st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  {
    prof_wall p("assemble_verify");
    // the representatives in the verifier's columns, `window` rows at a time, as dh_archive_check verifies a window:
    // the chained scheme against each candidate's OWN previous_signature; a row of another length is left zero and its
    // verdict is not read
    const size_t wmax = std::min(window, n_rep);
    const dh::assemble_verify_cols v{nullptr, nullptr, nullptr, nullptr, (uint32_t)std::max(sig_stride, ((size_t)want + 3) & ~(size_t)3),
                                     (uint32_t)(d_prevs ? prev_stride : 4)};
    HIP_TRY(v_rounds.ensure(wmax * 8));
    HIP_TRY(v_sigs.ensure(wmax * (size_t)v.sig_stride));
    if (chained) {
      HIP_TRY(v_prevs.ensure(wmax * (size_t)v.prev_stride));
      HIP_TRY(v_prev_lens.ensure(wmax * 4));
    }
    HIP_TRY(verdict.ensure(n_rep));
    dh::assemble_verify_cols vw = v;
    vw.rounds = v_rounds.as<uint64_t>();
    vw.sigs = v_sigs.as<uint8_t>();
    vw.prevs = v_prevs.as<uint8_t>();
    vw.prev_lens = v_prev_lens.as<uint32_t>();
    for (size_t at = 0; at < n_rep; at += window) {
      const size_t kk = std::min(window, n_rep - at);
      HIP_TRY(dh::launch_assemble_gather(c, rep_cand.as<uint32_t>() + at, kk, want, vw, st));
      rc = dh_verify_batch_device(scheme, pk, pk_len, vw.rounds, vw.sigs, vw.sig_stride, chained ? vw.prevs : nullptr, vw.prev_stride,
                                  chained ? vw.prev_lens : nullptr, kk, verdict.as<uint8_t>() + at, nullptr, seed, st, nullptr);
      if (rc) return rc;
    }
  }
  uint64_t n_gaps = 0;
  std::vector<uint8_t> h_flags;
  std::vector<uint64_t> h_gaps;
  {
    prof_wall p("assemble_select");
    HIP_TRY(chosen.ensure(n_runs * 4));
    HIP_TRY(opos.ensure((n + 3) * 4));
    HIP_TRY(dh::launch_assemble_pick(c, idx, run_start.as<uint32_t>(), n_runs, m, rpos.as<uint32_t>(), verdict.as<uint8_t>(), want,
                                     chosen.as<uint32_t>(), st));
    HIP_TRY(dh::launch_assemble_select(c, idx, runs, run_start.as<uint32_t>(), rep.as<uint32_t>(), rpos.as<uint32_t>(), verdict.as<uint8_t>(), chosen.as<uint32_t>(), m,
                                       want, status.as<uint8_t>(), flag, st));
    if (n) HIP_TRY(hipMemcpyAsync(status_out, status.p, n, hipMemcpyDeviceToHost, st));
    if (m) {
      HIP_TRY(dh::launch_scan(flag, m, opos.as<uint32_t>(), scan_tmp.as<uint32_t>(), st));
      uint32_t total = 0;
      HIP_TRY(hipMemcpyAsync(&total, opos.as<uint32_t>() + m, 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      n_out = total;
    }
    const dh::assemble_out o{d_rounds_out, d_sigs_out, d_sig_lens_out, d_prevs_out, d_prev_lens_out, d_src_out, d_flags_out};
    HIP_TRY(dh::launch_assemble_emit(c, idx, opos.as<uint32_t>(), m, o, st));
    // the anchor as row -1: {round, signature length, the signature from byte 16}; always allocated, so that the link
    // kernel's uniform loads have an address
    const size_t a_len = anchor_round ? anchor_sig_len : 0;
    std::vector<uint64_t> h_anchor(2 + (a_len + 7) / 8, 0);
    h_anchor[0] = b.anchor_round;
    h_anchor[1] = a_len;
    if (a_len) memcpy(h_anchor.data() + 2, anchor_sig, a_len);
    HIP_TRY(anchor.ensure(h_anchor.size() * 8));
    HIP_TRY(hipMemcpyAsync(anchor.p, h_anchor.data(), h_anchor.size() * 8, hipMemcpyHostToDevice, st));
    uint32_t* goff = opos.as<uint32_t>();  // the emit has read opos by then (stream order)
    HIP_TRY(dh::launch_assemble_link(c, o, n_out, b, anchor.as<uint64_t>(), chained, flag, st));
    HIP_TRY(dh::launch_scan(flag, n_out + 1, goff, scan_tmp.as<uint32_t>(), st));
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, goff + n_out + 1, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // h_anchor was read by then
    n_gaps = total;
    if (n_gaps) {
      HIP_TRY(gaps.ensure(n_gaps * 16));
      HIP_TRY(dh::launch_assemble_gaps(o, n_out, b, goff, gaps.as<uint64_t>(), gaps.as<uint64_t>() + n_gaps, st));
      h_gaps.resize(2 * n_gaps);
      HIP_TRY(hipMemcpyAsync(h_gaps.data(), gaps.p, n_gaps * 16, hipMemcpyDeviceToHost, st));
    }
    h_flags.resize(n_out);
    if (n_out) HIP_TRY(hipMemcpyAsync(h_flags.data(), d_flags_out, n_out, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  *m_out = n_out;
  *n_gaps_out = (size_t)n_gaps;
  counts_out[0] = n;
  counts_out[3] = n_rep;
  for (size_t i = 0; i < n; i++) {
    const uint8_t s = status_out[i];
    counts_out[1] += s & DH_AS_SKIPPED ? 1 : 0;
    counts_out[2] += s & DH_AS_STALE ? 1 : 0;
    counts_out[4] += s & DH_AS_INVALID ? 1 : 0;
    counts_out[5] += s & DH_AS_DUPLICATE ? 1 : 0;
    counts_out[6] += s & DH_AS_CONFLICT ? 1 : 0;
    counts_out[7] += s & DH_AS_CHOSEN ? 1 : 0;
  }
  for (uint64_t g = 0; g < n_gaps; g++) {
    const uint64_t span = h_gaps[n_gaps + g] - h_gaps[g] + 1;  // 0: all 2^64 rounds, which no u64 range holds
    counts_out[8] = counts_out[8] + span < span ? ~0ull : counts_out[8] + span;
    if (g < gap_cap) {
      gap_first_out[g] = h_gaps[g];
      gap_last_out[g] = h_gaps[n_gaps + g];
    }
  }
  for (uint8_t f : h_flags) counts_out[9] += f & DH_AS_LINK ? 1 : 0;
  if (n_gaps > gap_cap) return fail(DH_EINVAL, "%llu gaps, room for %zu", (unsigned long long)n_gaps, gap_cap);
  return DH_OK;
}

}  // extern "C"

extern "C" {

int dh_set_split(uint64_t chunk_rounds, int workers) {
  if (workers < 1) return fail(DH_EINVAL, "workers must be >= 1");
  std::lock_guard<std::mutex> lk(g_split_mu);
  g_split.chunk = (size_t)chunk_rounds;
  g_split.workers = workers;
  return DH_OK;
}

int dh_profile(int enable) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  prof_drain_locked();
  g_prof.on = enable != 0;
  g_prof.table.clear();
  return DH_OK;
}

int dh_profile_read(char* buf, size_t cap) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  prof_drain_locked();
  std::string out = "{";
  bool first = true;
  for (auto& e : g_prof.table) {
    char tmp[256];
    snprintf(tmp, sizeof tmp, "%s\"%s\": {\"count\": %llu, \"total_ms\": %.6f, \"products\": %llu}", first ? "" : ", ",
             e.first.c_str(), (unsigned long long)e.second.count, e.second.ms, e.second.prods);
    out += tmp;
    first = false;
  }
  out += "}";
  if (buf && cap) {
    size_t k = std::min(cap - 1, out.size());
    memcpy(buf, out.data(), k);
    buf[k] = 0;
  }
  return (int)out.size();
}

const char* dh_last_error_string(void) { return g_err.c_str(); }

const char* dh_version(void) { return "libdrandhip 0.1 gfx950 (BLS12-381 batch beacon verification)"; }

}  // extern "C"
