// Trimmed bbolt beacon store -> verifier columns on the device. The file image is resident in device
// memory; the host has walked the branch pages (bolt.hpp bolt_find_bucket) and hands the kernels one {offset, extent}
// per leaf, both checked against the file length, so every read below stays inside the image: the kernels read
// through bolt.hpp's bounds-checked accessors over a view of one leaf's extent.
//   k_bolt_scan    one wave per leaf: validate, per-leaf table (rounds, elements, first / last round, longest value)
//   k_bolt_count   one wave per leaf of a window: round elements with first <= round <= last (then launch_scan)
//   k_bolt_gather  one wave per leaf of a window: rounds / lens / value rows at base[leaf] + rank, in key order
//   k_bolt_link    per row: is the predecessor row round - 1; the gaps of [first, last] (then launch_scan, k_bolt_fill)
//   k_bolt_fold    per row: faulty = predecessor missing | stored length != signature length | verdict 0
// The legacy hexjson store (§18) adds k_bolt_scan_json (deferred records, longest decoded fields per leaf),
// k_bolt_gather_json (the hex-decoded Signature / PreviousSig rows) and k_bolt_fold_json (no predecessor term).
// Memory-bound and small next to verification; plain C++, no atomics on the output order.
#include <hip/hip_runtime.h>

#include "bolt.hpp"
#include "kernels.hpp"

namespace dh {
using namespace bolt;

namespace {
constexpr uint32_t LDS_LEAF = 16384;  // a leaf of up to 16 KiB is staged in LDS; larger ones are read in place
inline unsigned nblk(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }
}  // namespace

__global__ __launch_bounds__(64) void k_bolt_scan(const uint8_t* __restrict__ file, const leaf_ref* __restrict__ leaves,
                                                  leaf_info* __restrict__ out, uint32_t* __restrict__ err_word) {
  __shared__ leaf_info sh[64];
  const uint32_t lane = threadIdx.x;
  const leaf_ref lr = leaves[blockIdx.x];
  const view v{file + lr.off, lr.ext};
  leaf_info acc;
  info_init(&acc);
  uint32_t count = 0;
  const uint32_t rc = bolt_leaf_head(v, &count);
  if (rc)
    acc.err = rc;
  else
    bolt_leaf_check(v, count, lane, 64, &acc);
  sh[lane] = acc;
  __syncthreads();
  if (lane == 0) {
    leaf_info t;
    info_init(&t);
    for (int k = 0; k < 64; k++) info_merge(&t, sh[k].first, sh[k].last, sh[k].n_round, sh[k].n_all, sh[k].max_vsize, sh[k].err);
    t.off = lr.off;
    out[blockIdx.x] = t;
    if (t.err) atomicMax(err_word, t.err);
  }
}

// in-range round element i of the leaf: its element and round
template <class V>
__device__ __forceinline__ bool pick(const V& v, uint32_t i, uint32_t count, uint64_t first, uint64_t last, elem* e,
                                     uint64_t* r) {
  if (i >= count || bolt_leaf_elem(v, i, e) || !is_round(*e)) return false;
  *r = rd64be(v, e->koff);
  return *r >= first && *r <= last;
}

__global__ __launch_bounds__(64) void k_bolt_count(const uint8_t* __restrict__ file, const leaf_ref* __restrict__ leaves,
                                                   const leaf_info* __restrict__ info, uint64_t first, uint64_t last,
                                                   uint32_t* __restrict__ cnt) {
  const uint32_t lane = threadIdx.x;
  const leaf_info li = info[blockIdx.x];
  uint32_t c = 0;
  if (li.n_round == 0 || li.last < first || li.first > last) {
    c = 0;
  } else if (li.first >= first && li.last <= last) {
    c = li.n_round;
  } else {  // a leaf the window cuts
    const leaf_ref lr = leaves[blockIdx.x];
    const view v{file + lr.off, lr.ext};
    uint32_t count = 0;
    if (bolt_leaf_head(v, &count)) count = 0;
    for (uint32_t c0 = 0; c0 < count; c0 += 64) {
      elem e;
      uint64_t r;
      c += __popcll(__ballot(pick(v, c0 + lane, count, first, last, &e, &r)));
    }
  }
  if (lane == 0) cnt[blockIdx.x] = c;
}

__device__ __forceinline__ void gather_leaf(const view v, uint64_t run, uint64_t first, uint64_t last, uint32_t stride,
                                            uint64_t* __restrict__ rounds, uint8_t* __restrict__ rows,
                                            uint32_t* __restrict__ lens, uint64_t cap_rows, uint64_t* sel_off,
                                            uint32_t* sel_len) {
  const uint32_t lane = threadIdx.x, dw = stride / 4;
  uint32_t count = 0;
  if (bolt_leaf_head(v, &count)) return;
  for (uint32_t c0 = 0; c0 < count; c0 += 64) {
    elem e;
    uint64_t r = 0;
    const bool take = pick(v, c0 + lane, count, first, last, &e, &r);
    const uint64_t m = __ballot(take);
    const uint32_t rank = __popcll(m & ((1ull << lane) - 1)), nsel = __popcll(m);
    if (take) {
      const uint64_t row = run + rank;
      if (row < cap_rows) {
        rounds[row] = r;
        lens[row] = e.vsize;
      }
      sel_off[rank] = e.koff + 8;
      sel_len[rank] = e.vsize;
    }
    __syncthreads();
    // the chunk's rows are consecutive in the output: lane t writes dword t of them
    for (uint32_t t = lane; t < nsel * dw; t += 64) {
      const uint32_t s = t / dw, w = t - s * dw;
      const uint64_t row = run + s;
      if (row >= cap_rows) continue;
      const uint32_t vs = sel_len[s];
      uint32_t word = 0;
      if (vs <= stride) {  // a longer value leaves the row zero, never a prefix
        const uint64_t k = sel_off[s] + 4 * (uint64_t)w;
        for (uint32_t j = 0; j < 4; j++)
          if (4 * w + j < vs) word |= (uint32_t)v.p[k + j] << (8 * j);
      }
      ((uint32_t*)rows)[row * dw + w] = word;
    }
    __syncthreads();
    run += nsel;
  }
}

__global__ __launch_bounds__(64) void k_bolt_gather(const uint8_t* __restrict__ file, const leaf_ref* __restrict__ leaves,
                                                    const uint32_t* __restrict__ base, uint64_t first, uint64_t last,
                                                    uint32_t stride, uint64_t* __restrict__ rounds, uint8_t* __restrict__ rows,
                                                    uint32_t* __restrict__ lens, uint64_t cap_rows) {
  __shared__ uint4 lds[LDS_LEAF / 16];
  __shared__ uint64_t sel_off[64];
  __shared__ uint32_t sel_len[64];
  const uint32_t lane = threadIdx.x;
  if (base[blockIdx.x + 1] == base[blockIdx.x]) return;  // no row of the window in this leaf
  const leaf_ref lr = leaves[blockIdx.x];
  const uint64_t run = base[blockIdx.x];
  // pages are 16-byte aligned in the image; an inline bucket's page is not, and takes the in-place path
  if (lr.ext <= LDS_LEAF && !(lr.off & 15) && !(lr.ext & 15)) {
    const uint4* src = (const uint4*)(file + lr.off);
    for (uint32_t i = lane; i < (uint32_t)(lr.ext / 16); i += 64) lds[i] = src[i];
    __syncthreads();
    gather_leaf(view{(const uint8_t*)lds, lr.ext}, run, first, last, stride, rounds, rows, lens, cap_rows, sel_off, sel_len);
  } else {
    gather_leaf(view{file + lr.off, lr.ext}, run, first, last, stride, rounds, rows, lens, cap_rows, sel_off, sel_len);
  }
}

// ---- the legacy hexjson store: the same walk, the values decoded by bolt.hpp's hexjson_parse

// a leaf of up to LDS_LEAF bytes, 16-byte aligned at both ends, is copied to `lds` and viewed there; others in place
__device__ __forceinline__ view stage_leaf(const uint8_t* __restrict__ file, const leaf_ref lr, uint4* lds) {
  if (lr.ext <= LDS_LEAF && !(lr.off & 15) && !(lr.ext & 15)) {
    const uint4* src = (const uint4*)(file + lr.off);
    for (uint32_t i = threadIdx.x; i < (uint32_t)(lr.ext / 16); i += 64) lds[i] = src[i];
    __syncthreads();
    return view{(const uint8_t*)lds, lr.ext};
  }
  return view{file + lr.off, lr.ext};
}

// after k_bolt_scan: per leaf, the deferred round records and the longest decoded Signature / PreviousSig (bytes)
__global__ __launch_bounds__(64) void k_bolt_scan_json(const uint8_t* __restrict__ file, const leaf_ref* __restrict__ leaves,
                                                       leaf_json* __restrict__ out) {
  __shared__ uint4 lds[LDS_LEAF / 16];
  __shared__ leaf_json sh[64];
  const uint32_t lane = threadIdx.x;
  const view v = stage_leaf(file, leaves[blockIdx.x], lds);
  leaf_json acc{0, 0, 0, 0};
  uint32_t count = 0;
  if (bolt_leaf_head(v, &count)) count = 0;
  for (uint32_t i = lane; i < count; i += 64) {
    elem e;
    if (bolt_leaf_elem(v, i, &e) || !is_round(e)) continue;
    hexjson h;
    if (!hexjson_parse(elem_value(v, e), rd64be(v, e.koff), &h)) {
      acc.n_deferred++;
      continue;
    }
    if (h.sig_hex / 2 > acc.max_sig) acc.max_sig = h.sig_hex / 2;
    if (h.prev_hex / 2 > acc.max_prev) acc.max_prev = h.prev_hex / 2;
  }
  sh[lane] = acc;
  __syncthreads();
  if (lane == 0) {
    leaf_json t{0, 0, 0, 0};
    for (int k = 0; k < 64; k++) {
      t.n_deferred += sh[k].n_deferred;
      if (sh[k].max_sig > t.max_sig) t.max_sig = sh[k].max_sig;
      if (sh[k].max_prev > t.max_prev) t.max_prev = sh[k].max_prev;
    }
    out[blockIdx.x] = t;
  }
}

// the chunk's rows are consecutive in the output: lane t writes dword t of them, decoded from 8 hex characters
__device__ __forceinline__ void write_hex_rows(const view v, uint8_t* __restrict__ rows, uint32_t stride, uint64_t run, uint32_t nsel,
                                               uint64_t cap_rows, const uint64_t* sel_off, const uint32_t* sel_hex) {
  const uint32_t dw = stride / 4;
  for (uint32_t t = threadIdx.x; t < nsel * dw; t += 64) {
    const uint32_t s = t / dw, w = t - s * dw;
    const uint64_t row = run + s;
    if (row >= cap_rows) continue;
    const uint32_t nb = sel_hex[s] / 2;
    uint32_t word = 0;
    if (nb <= stride) {  // a longer value leaves the row zero, never a prefix
      const uint64_t k = sel_off[s] + 8 * (uint64_t)w;
      for (uint32_t j = 0; j < 4; j++)
        if (4 * w + j < nb) word |= hj_byte(v, k + 2 * j) << (8 * j);
    }
    ((uint32_t*)rows)[row * dw + w] = word;
  }
}

__global__ __launch_bounds__(64) void k_bolt_gather_json(const uint8_t* __restrict__ file, const leaf_ref* __restrict__ leaves,
                                                         const uint32_t* __restrict__ base, uint64_t first, uint64_t last,
                                                         const json_cols c) {
  __shared__ uint4 lds[LDS_LEAF / 16];
  __shared__ uint64_t sig_off[64], prev_off[64];
  __shared__ uint32_t sig_hex[64], prev_hex[64];
  const uint32_t lane = threadIdx.x;
  if (base[blockIdx.x + 1] == base[blockIdx.x]) return;  // no row of the window in this leaf
  uint64_t run = base[blockIdx.x];
  const view v = stage_leaf(file, leaves[blockIdx.x], lds);
  uint32_t count = 0;
  if (bolt_leaf_head(v, &count)) return;
  for (uint32_t c0 = 0; c0 < count; c0 += 64) {
    elem e;
    uint64_t r = 0;
    hexjson h{0, 0, 0, 0};
    const bool take = pick(v, c0 + lane, count, first, last, &e, &r);
    const bool canon = take && hexjson_parse(elem_value(v, e), r, &h);
    const uint64_t m = __ballot(take);
    const uint32_t rank = __popcll(m & ((1ull << lane) - 1)), nsel = __popcll(m);
    if (take) {
      const uint64_t row = run + rank;
      if (row < c.cap_rows) {  // a deferred record: zero lengths and (below) zero rows
        c.rounds[row] = r;
        c.deferred[row] = !canon;
        if (c.sig_lens) c.sig_lens[row] = h.sig_hex / 2;
        if (c.prev_lens) c.prev_lens[row] = h.prev_hex / 2;
      }
      sig_off[rank] = e.koff + 8 + h.sig_off;
      sig_hex[rank] = h.sig_hex;
      prev_off[rank] = e.koff + 8 + h.prev_off;
      prev_hex[rank] = h.prev_hex;
    }
    __syncthreads();
    if (c.sigs) write_hex_rows(v, c.sigs, c.sig_stride, run, nsel, c.cap_rows, sig_off, sig_hex);
    if (c.prevs) write_hex_rows(v, c.prevs, c.prev_stride, run, nsel, c.cap_rows, prev_off, prev_hex);
    __syncthreads();
    run += nsel;
  }
}

// the hexjson store's fold: the stored PreviousSig was verified with the row, so there is no predecessor term; a
// deferred row is not decided here
__global__ __launch_bounds__(256) void k_bolt_fold_json(const uint32_t* __restrict__ sig_lens, const uint8_t* __restrict__ deferred,
                                                        const uint8_t* __restrict__ verdict, size_t n, uint32_t sig_len,
                                                        uint8_t* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  bad[i] = !deferred[i] && (sig_lens[i] != sig_len || !verdict[i]);
}

// slot i of n + 1: the rounds of [first, last] missing before row i (slot n: after the last row)
__global__ __launch_bounds__(256) void k_bolt_link(const uint64_t* __restrict__ rounds, size_t n, uint64_t first, uint64_t last,
                                                   uint8_t* __restrict__ miss_prev, uint32_t* __restrict__ gap) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  uint64_t g;
  if (n == 0) {
    g = last - first + 1;
  } else if (i == 0) {
    g = rounds[0] - first;
  } else if (i == n) {
    g = last - rounds[n - 1];
  } else {
    g = rounds[i] - rounds[i - 1] - 1;
  }
  gap[i] = g > 0xffffffffull ? 0xffffffffu : (uint32_t)g;  // the host bounds the total first
  // the first row has no predecessor row: missing, unless it is round 0, which has none by definition
  if (i < n) miss_prev[i] = i == 0 ? (rounds[0] != 0) : (rounds[i - 1] != rounds[i] - 1);
}

// missing round j: the slot s with moff[s] <= j < moff[s + 1], counted from the row before it
__global__ __launch_bounds__(256) void k_bolt_fill(const uint64_t* __restrict__ rounds, size_t n, uint64_t first,
                                                   const uint32_t* __restrict__ moff, size_t total, uint64_t* __restrict__ missing) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= total) return;
  size_t lo = 0, hi = n + 1;  // moff[lo] <= j < moff[hi]
  while (hi - lo > 1) {
    const size_t mid = (lo + hi) / 2;
    if (moff[mid] <= j) lo = mid; else hi = mid;
  }
  missing[j] = (lo == 0 ? first : rounds[lo - 1] + 1) + (j - moff[lo]);
}

// chained (prev_layout): row 0 carries round a - 1 (the previous signature of a) and is not reported; when it is a
// later round its predecessor is missing. Row r >= 1 was verified as item r - 1.
__global__ __launch_bounds__(256) void k_bolt_fold(const uint64_t* __restrict__ rounds, const uint32_t* __restrict__ lens,
                                                   const uint8_t* __restrict__ miss_prev, const uint8_t* __restrict__ verdict,
                                                   size_t n, uint32_t sig_len, int prev_layout, uint64_t a, uint8_t* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint8_t b;
  if (!prev_layout)
    b = lens[i] != sig_len || !verdict[i];
  else if (i == 0)
    b = rounds[0] >= a;
  else
    b = miss_prev[i] || lens[i] != sig_len || !verdict[i - 1];
  bad[i] = b;
}

hipError_t launch_bolt_scan(const uint8_t* file, const void* leaves, size_t n, void* info, uint32_t* err_word, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_bolt_scan, dim3((unsigned)n), dim3(64), 0, st, file, (const leaf_ref*)leaves, (leaf_info*)info, err_word);
  return hipGetLastError();
}
hipError_t launch_bolt_count(const uint8_t* file, const void* leaves, const void* info, size_t n, uint64_t first, uint64_t last,
                             uint32_t* cnt, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_bolt_count, dim3((unsigned)n), dim3(64), 0, st, file, (const leaf_ref*)leaves, (const leaf_info*)info, first, last, cnt);
  return hipGetLastError();
}
hipError_t launch_bolt_gather(const uint8_t* file, const void* leaves, const uint32_t* base, size_t n, uint64_t first, uint64_t last,
                              uint32_t stride, uint64_t* rounds, uint8_t* rows, uint32_t* lens, uint64_t cap_rows, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_bolt_gather, dim3((unsigned)n), dim3(64), 0, st, file, (const leaf_ref*)leaves, base, first, last, stride, rounds, rows, lens, cap_rows);
  return hipGetLastError();
}
hipError_t launch_bolt_link(const uint64_t* rounds, size_t n, uint64_t first, uint64_t last, uint8_t* miss_prev, uint32_t* gap,
                            hipStream_t st) {
  hipLaunchKernelGGL(k_bolt_link, dim3(nblk(n + 1, 256)), dim3(256), 0, st, rounds, n, first, last, miss_prev, gap);
  return hipGetLastError();
}
hipError_t launch_bolt_fill(const uint64_t* rounds, size_t n, uint64_t first, const uint32_t* moff, size_t total, uint64_t* missing,
                            hipStream_t st) {
  if (total) hipLaunchKernelGGL(k_bolt_fill, dim3(nblk(total, 256)), dim3(256), 0, st, rounds, n, first, moff, total, missing);
  return hipGetLastError();
}
hipError_t launch_bolt_fold(const uint64_t* rounds, const uint32_t* lens, const uint8_t* miss_prev, const uint8_t* verdict, size_t n,
                            uint32_t sig_len, int prev_layout, uint64_t a, uint8_t* bad, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_bolt_fold, dim3(nblk(n, 256)), dim3(256), 0, st, rounds, lens, miss_prev, verdict, n, sig_len, prev_layout, a, bad);
  return hipGetLastError();
}

hipError_t launch_bolt_scan_json(const uint8_t* file, const void* leaves, size_t n, void* jinfo, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_bolt_scan_json, dim3((unsigned)n), dim3(64), 0, st, file, (const leaf_ref*)leaves, (leaf_json*)jinfo);
  return hipGetLastError();
}
hipError_t launch_bolt_gather_json(const uint8_t* file, const void* leaves, const uint32_t* base, size_t n, uint64_t first,
                                   uint64_t last, const json_cols& c, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_bolt_gather_json, dim3((unsigned)n), dim3(64), 0, st, file, (const leaf_ref*)leaves, base, first, last, c);
  return hipGetLastError();
}
hipError_t launch_bolt_fold_json(const uint32_t* sig_lens, const uint8_t* deferred, const uint8_t* verdict, size_t n, uint32_t sig_len,
                                 uint8_t* bad, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_bolt_fold_json, dim3(nblk(n, 256)), dim3(256), 0, st, sig_lens, deferred, verdict, n, sig_len, bad);
  return hipGetLastError();
}

}  // namespace dh
