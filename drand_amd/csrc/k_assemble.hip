// Candidate records in any order, from any number of sources -> the one chain they support. What a
// row compare, a class or a status bit is, is decided by assemble.hpp, which the host runs unchanged under sanitizers.
//   k_assemble_pre     per candidate: SKIPPED / STALE or live (then launch_scan: the live candidates are cut out, in
//                      input order, BEFORE the sort: no sentinel key, and 2^64 - 1 stays an ordinary round)
//   k_assemble_cut     the live candidates' keys (rounds) and payloads (input positions) at their scanned places
//   k_sort_orand       the OR and the AND of all keys: a pass whose digit is the same in every key is skipped
//   k_sort_hist        one workgroup per tile of SORT_TILE keys: its count per 8-bit digit, digit-major (then launch_scan)
//   k_sort_scatter     the stable scatter of one pass: wave bases from the scanned counts, the rank inside a wave's 64
//                      keys from ballots over the digit's bits and a popcount below the lane
//   k_assemble_heads   per sorted entry: does a new round's run start here (then launch_scan: run numbers)
//   k_assemble_runs    run number -> its first sorted entry
//   k_assemble_class   per sorted entry: the representative it repeats, or itself (then launch_scan over the
//                      representatives: their places in the verifier's columns)
//   k_assemble_reps    place in the verifier's columns -> candidate
//   k_assemble_gather  one window of the verifier's columns, a thread per dword, zero-padded rows
//   k_assemble_pick    per run: its first valid representative (a serial walk of the run by one lane)
//   k_assemble_select  per sorted entry: the candidate's status byte, the chosen flag (then launch_scan: output rows)
//   k_assemble_emit    the output columns, a thread per dword
//   k_assemble_link    per output row: GAP / LINK against the row before it (the anchor before row 0), and whether a
//                      range of missing rounds lies in front of it (then launch_scan, k_assemble_gaps)
//   k_assemble_gaps    the ranges of missing rounds at their scanned places
// Memory-bound; plain C++, vector stores only. The LDS histograms are built with atomic adds, whose sum does not depend
// on their order; the OR / AND words likewise. No address and no output depends on the order of an atomic.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "assemble.hpp"
#include "kernels.hpp"

namespace dh {
using namespace assemble;

namespace {
inline unsigned nblk(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }
constexpr uint32_t SORT_WAVES = 4, SORT_THREADS = 64 * SORT_WAVES, SORT_WAVE_KEYS = SORT_TILE / SORT_WAVES;
static_assert(SORT_WAVE_KEYS % 64 == 0, "a wave takes its keys 64 at a time");
}  // namespace

__global__ __launch_bounds__(256) void k_assemble_pre(const cols c, size_t n, const bounds b, uint8_t* __restrict__ status,
                                                      uint32_t* __restrict__ live) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = pre_status(c.rounds[i], c.skip && c.skip[i], b);
  status[i] = (uint8_t)s;
  live[i] = s == 0;
}

__global__ __launch_bounds__(256) void k_assemble_cut(const uint64_t* __restrict__ rounds, size_t n, const uint32_t* __restrict__ pos,
                                                      uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || pos[i + 1] == pos[i]) return;
  keys[pos[i]] = rounds[i];
  idx[pos[i]] = (uint32_t)i;
}

// orand[0] |= every key, orand[1] &= every key (the host sets {0, ~0} first)
__global__ __launch_bounds__(256) void k_sort_orand(const uint64_t* __restrict__ keys, size_t n, unsigned long long* __restrict__ orand) {
  __shared__ unsigned long long sh_or[256], sh_and[256];
  unsigned long long o = 0, a = ~0ull;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    o |= keys[i];
    a &= keys[i];
  }
  sh_or[threadIdx.x] = o;
  sh_and[threadIdx.x] = a;
  __syncthreads();
  for (uint32_t s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      sh_or[threadIdx.x] |= sh_or[threadIdx.x + s];
      sh_and[threadIdx.x] &= sh_and[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    atomicOr(orand, sh_or[0]);
    atomicAnd(orand + 1, sh_and[0]);
  }
}

// cnt[d * ntiles + tile] = the tile's keys whose digit (bits shift .. shift + 7) is d
__global__ __launch_bounds__(SORT_THREADS) void k_sort_hist(const uint64_t* __restrict__ keys, size_t n, uint32_t shift, uint32_t ntiles,
                                                            uint32_t* __restrict__ cnt) {
  __shared__ uint32_t hist[256];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * SORT_TILE;
  for (uint32_t k = threadIdx.x; k < SORT_TILE; k += SORT_THREADS)
    if (base + k < n) atomicAdd(&hist[(uint32_t)(keys[base + k] >> shift) & 255u], 1u);
  __syncthreads();
  cnt[(size_t)threadIdx.x * ntiles + blockIdx.x] = hist[threadIdx.x];
}

// off: the exclusive scan of cnt. Wave w of a tile holds the tile's keys [w, w + 1) SORT_WAVE_KEYS, in order, 64 at a
// step; wbase[w][d] = where the wave's next key of digit d goes. Inside a step the keys of one digit keep their lane
// order: the rank is the count of lanes below with the same digit.
__global__ __launch_bounds__(SORT_THREADS) void k_sort_scatter(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx, size_t n,
                                                               uint32_t shift, uint32_t ntiles, const uint32_t* __restrict__ off,
                                                               uint64_t* __restrict__ keys_out, uint32_t* __restrict__ idx_out) {
  __shared__ uint32_t wbase[SORT_WAVES][256];
  const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63;
  for (uint32_t w = 0; w < SORT_WAVES; w++) wbase[w][t] = 0;
  __syncthreads();
  const size_t tile0 = (size_t)blockIdx.x * SORT_TILE, wave0 = tile0 + (size_t)wave * SORT_WAVE_KEYS;
  for (uint32_t k = lane; k < SORT_WAVE_KEYS; k += 64)
    if (wave0 + k < n) atomicAdd(&wbase[wave][(uint32_t)(keys[wave0 + k] >> shift) & 255u], 1u);
  __syncthreads();
  {  // thread t owns digit t: the waves' counts become their bases
    uint32_t at = off[(size_t)t * ntiles + blockIdx.x];
    for (uint32_t w = 0; w < SORT_WAVES; w++) {
      const uint32_t c = wbase[w][t];
      wbase[w][t] = at;
      at += c;
    }
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1;
  for (uint32_t s = 0; s < SORT_WAVE_KEYS; s += 64) {  // the same trip count in every wave: the barriers are uniform
    const size_t i = wave0 + s + lane;
    const bool have = i < n;
    const uint64_t key = have ? keys[i] : 0;
    const uint32_t d = (uint32_t)(key >> shift) & 255u;
    unsigned long long same = __ballot(have);
    for (uint32_t bit = 0; bit < 8; bit++) {
      const unsigned long long m = __ballot((d >> bit) & 1u);
      same &= (d >> bit) & 1u ? m : ~m;
    }
    const uint32_t rank = (uint32_t)__popcll(same & below);
    uint32_t at = 0;
    if (have) at = wbase[wave][d] + rank;
    __syncthreads();  // every lane has read its base
    if (have) {
      keys_out[at] = key;
      idx_out[at] = idx[i];
      if (rank == 0) wbase[wave][d] += (uint32_t)__popcll(same);  // one lane per digit
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_assemble_heads(const uint64_t* __restrict__ keys, size_t m, uint32_t* __restrict__ head) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j < m) head[j] = j == 0 || keys[j] != keys[j - 1];
}

// runs: the exclusive scan of head; entry j lies in run runs[j + 1] - 1
__global__ __launch_bounds__(256) void k_assemble_runs(const uint32_t* __restrict__ runs, size_t m, uint32_t* __restrict__ run_start) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j < m && runs[j + 1] != runs[j]) run_start[runs[j]] = (uint32_t)j;
}

// rep[j] = the sorted entry j repeats (j itself: a representative), is_rep[j] its flag; dedupe 0: every entry is one
__global__ __launch_bounds__(256) void k_assemble_class(const cols c, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ runs,
                                                        const uint32_t* __restrict__ run_start, size_t m, uint32_t dedupe,
                                                        uint32_t* __restrict__ rep, uint32_t* __restrict__ is_rep) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const size_t r = dedupe ? class_of(c, idx, run_start[runs[j + 1] - 1], j) : j;
  rep[j] = (uint32_t)r;
  is_rep[j] = r == j;
}

__global__ __launch_bounds__(256) void k_assemble_reps(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ rpos, size_t m,
                                                       uint32_t* __restrict__ rep_cand) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j < m && rpos[j + 1] != rpos[j]) rep_cand[rpos[j]] = idx[j];
}

// rows [0, k) of a window of the verifier's columns = candidates rep_cand[0 .. k); a row that cannot verify (its length)
// is left zero with its verdict unread; thread (row, w) writes dword w of the signature row and of the prev row
__global__ __launch_bounds__(256) void k_assemble_gather(const cols c, const uint32_t* __restrict__ rep_cand, size_t k, uint32_t want_sig_len,
                                                         const assemble_verify_cols v) {
  const uint32_t sdw = v.sig_stride / 4, pdw = c.prevs ? v.prev_stride / 4 : 0, dw = sdw + pdw;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t row = t / dw;
  const uint32_t w = (uint32_t)(t - row * dw);
  if (row >= k) return;
  const size_t i = rep_cand[row];
  const bool ok = row_verifiable(c, i, want_sig_len);
  const bool is_sig = w < sdw;
  const uint32_t ww = is_sig ? w : w - sdw;
  const uint8_t* src = is_sig ? c.sigs + i * (size_t)c.sig_stride : c.prevs + i * (size_t)c.prev_stride;
  const uint32_t len = !ok ? 0 : is_sig ? c.sig_lens[i] : c.prev_lens[i];
  uint32_t word = 0;
  for (uint32_t b = 0; b < 4; b++)
    if (4 * ww + b < len) word |= (uint32_t)src[4 * ww + b] << (8 * b);
  if (is_sig) ((uint32_t*)v.sigs)[row * sdw + ww] = word;
  else ((uint32_t*)v.prevs)[row * pdw + ww] = word;
  if (w == 0) {
    v.rounds[row] = c.rounds[i];
    if (c.prevs) v.prev_lens[row] = len ? c.prev_lens[i] : 0;
  }
}

// chosen[run] = the run's first valid representative (a sorted entry), 0xFFFFFFFF for none. One lane walks its run: the
// runs of real input are as long as there are sources.
__global__ __launch_bounds__(256) void k_assemble_pick(const cols c, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ run_start,
                                                       size_t n_runs, size_t m, const uint32_t* __restrict__ rpos,
                                                       const uint8_t* __restrict__ verdict, uint32_t want_sig_len, uint32_t* __restrict__ chosen) {
  const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_runs) return;
  const size_t end = r + 1 < n_runs ? run_start[r + 1] : m;
  uint32_t pick = 0xFFFFFFFFu;
  for (size_t j = run_start[r]; j < end; j++)
    if (rpos[j + 1] != rpos[j] && verdict[rpos[j]] && row_verifiable(c, idx[j], want_sig_len)) {
      pick = (uint32_t)j;
      break;
    }
  chosen[r] = pick;
}

__global__ __launch_bounds__(256) void k_assemble_select(const cols c, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ runs,
                                                         const uint32_t* __restrict__ run_start, const uint32_t* __restrict__ rep, const uint32_t* __restrict__ rpos,
                                                         const uint8_t* __restrict__ verdict, const uint32_t* __restrict__ chosen, size_t m,
                                                         uint32_t want_sig_len, uint8_t* __restrict__ status, uint32_t* __restrict__ out_flag) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const size_t r = rep[j];
  const bool valid = verdict[rpos[r]] && row_verifiable(c, idx[r], want_sig_len);
  uint32_t s;
  if (r != j) {
    s = dup_status(valid);
  } else {
    const uint32_t run = runs[j + 1] - 1;
    const bool is_chosen = chosen[run] == (uint32_t)j;
    s = rep_status(valid, is_chosen, valid && !is_chosen && repeats_earlier(c, idx, run_start[run], j));
  }
  status[idx[j]] = (uint8_t)s;
  out_flag[j] = (s & AS_CHOSEN) != 0;
}

// opos: the exclusive scan of out_flag; thread (sorted entry, w) writes dword w of the chosen entry's output rows
__global__ __launch_bounds__(256) void k_assemble_emit(const cols c, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ opos, size_t m,
                                                       const assemble_out o) {
  const uint32_t sdw = c.sig_stride / 4, pdw = o.prevs ? c.prev_stride / 4 : 0, dw = sdw + pdw;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t j = t / dw;
  const uint32_t w = (uint32_t)(t - j * dw);
  if (j >= m || opos[j + 1] == opos[j]) return;
  const size_t at = opos[j], i = idx[j];
  const bool is_sig = w < sdw;
  const uint32_t ww = is_sig ? w : w - sdw;
  const uint8_t* src = is_sig ? c.sigs + i * (size_t)c.sig_stride : c.prevs + i * (size_t)c.prev_stride;
  uint32_t len = is_sig ? c.sig_lens[i] : c.prev_lens[i];
  if (len > (is_sig ? c.sig_stride : c.prev_stride)) len = 0;  // a chosen row fits: never a prefix
  uint32_t word = 0;
  for (uint32_t b = 0; b < 4; b++)
    if (4 * ww + b < len) word |= (uint32_t)src[4 * ww + b] << (8 * b);
  if (is_sig) ((uint32_t*)o.sigs)[at * sdw + ww] = word;
  else ((uint32_t*)o.prevs)[at * pdw + ww] = word;
  if (w == 0) {
    o.rounds[at] = c.rounds[i];
    o.sig_lens[at] = c.sig_lens[i];
    o.src[at] = (uint32_t)i;
    if (o.prevs) o.prev_lens[at] = c.prev_lens[i];
  }
}

// Slot r < n_out: output row r against the row before it, the anchor before row 0 (anchor = {round, signature length,
// then the signature from byte 16}: always a readable address, b.has_anchor says whether it is one; its loads are
// wave-uniform). gap[r] = a range of missing rounds ends in front of row r. Slot n_out: the range behind the last row
// up to up_to.
__global__ __launch_bounds__(256) void k_assemble_link(const cols c, const assemble_out o, size_t n_out, const bounds b,
                                                       const uint64_t* __restrict__ anchor, uint32_t chained, uint32_t* __restrict__ gap) {
  const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (r > n_out) return;
  const bool have = r > 0 || b.has_anchor;
  const uint64_t before = r > 0 ? o.rounds[r - 1] : b.anchor_round;
  if (r == n_out) {
    gap[r] = have && b.has_up_to && before < b.up_to;
    return;
  }
  const uint64_t round = o.rounds[r];
  bool differs = false;
  if (chained && have && round == before + 1) {
    const size_t i = o.src[r];
    const uint8_t* sig = r > 0 ? o.sigs + (r - 1) * (size_t)c.sig_stride : (const uint8_t*)(anchor + 2);
    const uint32_t sig_len = r > 0 ? o.sig_lens[r - 1] : (uint32_t)anchor[1];
    // the two rows may have different strides: compared over the length, which fits both when it is equal
    differs = c.prev_lens[i] != sig_len || c.prev_lens[i] > c.prev_stride ||
              !value_equal(c.prevs + i * (size_t)c.prev_stride, sig_len, sig, sig_len, sig_len);
  }
  const uint32_t f = row_flags(round, have, before, chained != 0, differs);
  o.flags[r] = (uint8_t)f;
  gap[r] = (f & AS_GAP) != 0;
}

// goff: the exclusive scan of gap; the range in front of slot r is [before + 1, round - 1] (slot n_out: up to up_to)
__global__ __launch_bounds__(256) void k_assemble_gaps(const assemble_out o, size_t n_out, const bounds b, const uint32_t* __restrict__ goff,
                                                       uint64_t* __restrict__ gap_first, uint64_t* __restrict__ gap_last) {
  const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (r > n_out || goff[r + 1] == goff[r]) return;
  const uint64_t before = r > 0 ? o.rounds[r - 1] : b.anchor_round;
  gap_first[goff[r]] = before + 1;
  gap_last[goff[r]] = r == n_out ? b.up_to : o.rounds[r] - 1;
}

hipError_t launch_assemble_pre(const cols& c, size_t n, const bounds& b, uint8_t* status, uint32_t* live, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_assemble_pre, dim3(nblk(n, 256)), dim3(256), 0, st, c, n, b, status, live);
  return hipGetLastError();
}
hipError_t launch_assemble_cut(const uint64_t* rounds, size_t n, const uint32_t* pos, uint64_t* keys, uint32_t* idx, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_assemble_cut, dim3(nblk(n, 256)), dim3(256), 0, st, rounds, n, pos, keys, idx);
  return hipGetLastError();
}
hipError_t launch_sort_orand(const uint64_t* keys, size_t n, uint64_t* orand, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_sort_orand, dim3(std::min(nblk(n, 256), 1024u)), dim3(256), 0, st, keys, n, (unsigned long long*)orand);
  return hipGetLastError();
}
hipError_t launch_sort_pass(const uint64_t* keys, const uint32_t* idx, size_t n, uint32_t shift, uint32_t* cnt, uint32_t* off,
                            uint32_t* scan_tmp, uint64_t* keys_out, uint32_t* idx_out, hipStream_t st) {
  if (!n) return hipSuccess;
  if (shift > 56 || (shift & 7)) return hipErrorInvalidValue;
  const uint32_t ntiles = nblk(n, SORT_TILE);
  hipLaunchKernelGGL(k_sort_hist, dim3(ntiles), dim3(SORT_THREADS), 0, st, keys, n, shift, ntiles, cnt);
  hipError_t e = launch_scan(cnt, (size_t)256 * ntiles, off, scan_tmp, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_sort_scatter, dim3(ntiles), dim3(SORT_THREADS), 0, st, keys, idx, n, shift, ntiles, off, keys_out, idx_out);
  return hipGetLastError();
}
hipError_t launch_assemble_heads(const uint64_t* keys, size_t m, uint32_t* head, hipStream_t st) {
  if (m) hipLaunchKernelGGL(k_assemble_heads, dim3(nblk(m, 256)), dim3(256), 0, st, keys, m, head);
  return hipGetLastError();
}
hipError_t launch_assemble_runs(const uint32_t* runs, size_t m, uint32_t* run_start, hipStream_t st) {
  if (m) hipLaunchKernelGGL(k_assemble_runs, dim3(nblk(m, 256)), dim3(256), 0, st, runs, m, run_start);
  return hipGetLastError();
}
hipError_t launch_assemble_class(const cols& c, const uint32_t* idx, const uint32_t* runs, const uint32_t* run_start, size_t m, bool dedupe,
                                 uint32_t* rep, uint32_t* is_rep, hipStream_t st) {
  if (m) hipLaunchKernelGGL(k_assemble_class, dim3(nblk(m, 256)), dim3(256), 0, st, c, idx, runs, run_start, m, dedupe ? 1u : 0u, rep, is_rep);
  return hipGetLastError();
}
hipError_t launch_assemble_reps(const uint32_t* idx, const uint32_t* rpos, size_t m, uint32_t* rep_cand, hipStream_t st) {
  if (m) hipLaunchKernelGGL(k_assemble_reps, dim3(nblk(m, 256)), dim3(256), 0, st, idx, rpos, m, rep_cand);
  return hipGetLastError();
}
hipError_t launch_assemble_gather(const cols& c, const uint32_t* rep_cand, size_t k, uint32_t want_sig_len, const assemble_verify_cols& v,
                                  hipStream_t st) {
  if (v.sig_stride < 4 || (v.sig_stride & 3) || (c.prevs && (v.prev_stride < 4 || (v.prev_stride & 3)))) return hipErrorInvalidValue;
  const size_t threads = k * (size_t)(v.sig_stride / 4 + (c.prevs ? v.prev_stride / 4 : 0));
  if (threads) hipLaunchKernelGGL(k_assemble_gather, dim3(nblk(threads, 256)), dim3(256), 0, st, c, rep_cand, k, want_sig_len, v);
  return hipGetLastError();
}
hipError_t launch_assemble_pick(const cols& c, const uint32_t* idx, const uint32_t* run_start, size_t n_runs, size_t m, const uint32_t* rpos,
                                const uint8_t* verdict, uint32_t want_sig_len, uint32_t* chosen, hipStream_t st) {
  if (n_runs) hipLaunchKernelGGL(k_assemble_pick, dim3(nblk(n_runs, 256)), dim3(256), 0, st, c, idx, run_start, n_runs, m, rpos, verdict,
                                 want_sig_len, chosen);
  return hipGetLastError();
}
hipError_t launch_assemble_select(const cols& c, const uint32_t* idx, const uint32_t* runs, const uint32_t* run_start, const uint32_t* rep,
                                  const uint32_t* rpos,
                                  const uint8_t* verdict, const uint32_t* chosen, size_t m, uint32_t want_sig_len, uint8_t* status,
                                  uint32_t* out_flag, hipStream_t st) {
  if (m) hipLaunchKernelGGL(k_assemble_select, dim3(nblk(m, 256)), dim3(256), 0, st, c, idx, runs, run_start, rep, rpos, verdict, chosen, m, want_sig_len,
                            status, out_flag);
  return hipGetLastError();
}
hipError_t launch_assemble_emit(const cols& c, const uint32_t* idx, const uint32_t* opos, size_t m, const assemble_out& o, hipStream_t st) {
  if (c.sig_stride < 4 || (c.sig_stride & 3) || (o.prevs && (!c.prevs || c.prev_stride < 4 || (c.prev_stride & 3)))) return hipErrorInvalidValue;
  const size_t threads = m * (size_t)(c.sig_stride / 4 + (o.prevs ? c.prev_stride / 4 : 0));
  if (threads) hipLaunchKernelGGL(k_assemble_emit, dim3(nblk(threads, 256)), dim3(256), 0, st, c, idx, opos, m, o);
  return hipGetLastError();
}
hipError_t launch_assemble_link(const cols& c, const assemble_out& o, size_t n_out, const bounds& b, const uint64_t* anchor, bool chained,
                                uint32_t* gap, hipStream_t st) {
  hipLaunchKernelGGL(k_assemble_link, dim3(nblk(n_out + 1, 256)), dim3(256), 0, st, c, o, n_out, b, anchor, chained ? 1u : 0u, gap);
  return hipGetLastError();
}
hipError_t launch_assemble_gaps(const assemble_out& o, size_t n_out, const bounds& b, const uint32_t* goff, uint64_t* gap_first,
                                uint64_t* gap_last, hipStream_t st) {
  hipLaunchKernelGGL(k_assemble_gaps, dim3(nblk(n_out + 1, 256)), dim3(256), 0, st, o, n_out, b, goff, gap_first, gap_last);
  return hipGetLastError();
}

}  // namespace dh
