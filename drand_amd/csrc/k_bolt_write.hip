// Verifier columns in device memory -> the leaf pages of a trimmed bbolt beacon store, the mirror of
// k_bolt.hip's gather. Where a byte goes is decided by bolt_write.hpp, which the host runs unchanged under sanitizers;
// the host has planned the leaves from the scanned record sizes and checked that the image holds every extent.
//   k_bolt_need     per row: the record size 24 + lens[i] (then launch_scan); rounds ascending and lens <= stride, or err
//   k_bolt_pack     one wave per leaf extent: lane t writes dword t, zeros included, so no memset; the leaf's first key
//   k_bolt_carry    the windowed writer (§23): the open leaf's rows into the next carry set, the last row appended
//   k_bolt_merge    per row and per patch: a binary search of the other list; kept / emitted flags (then launch_scan)
//   k_bolt_scatter  per dword of a kept row or an emitted patch: the merged columns at the scanned positions
//   k_bolt_unlinked per merged row taken from a hexjson record: does the row before it differ from its PreviousSig
//   k_bolt_compact  the flagged rounds, ascending, at their scanned positions
// Memory-bound; plain C++, no atomics on any output order.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bolt_write.hpp"
#include "kernels.hpp"

namespace dh {
using namespace boltw;

namespace {
inline unsigned nblk(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }
constexpr uint32_t SRC_NONE = 0xFFFFFFFFu;  // merged row not taken from a stored record
}  // namespace

// The n new rows of a window: a length is held to the columns' stride and a round to the row before it, the first
// row's to `last` (the last row appended so far: always a readable address, has_last says whether there is such a row;
// see k_bolt_unlinked on the scalar loads).
__global__ __launch_bounds__(256) void k_bolt_need(const cols c, size_t n, const uint64_t* __restrict__ last, uint32_t has_last,
                                                   uint32_t* __restrict__ need, uint32_t* __restrict__ err_word) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t l = c.lens[i];
  const bool bad = l > c.stride || (i ? c.rounds[i - 1] >= c.rounds[i] : (has_last && last[0] >= c.rounds[0]));
  need[i] = bad ? 24 : 24 + l;
  if (bad) atomicOr(err_word, 1u);
}

// C = cols: one row segment (a one-shot image); cols2: a window behind the writer's carried rows. page_base is the
// page `image` starts at.
template <class C>
__global__ __launch_bounds__(64) void k_bolt_pack(const leaf_desc* __restrict__ leaves, const C c, uint32_t page_size, uint64_t page_base,
                                                  uint8_t* __restrict__ image, uint64_t* __restrict__ first_key) {
  __shared__ uint32_t offs[MAX_LEAF_RECS + 1];
  const uint32_t lane = threadIdx.x;
  const leaf_desc L = leaves[blockIdx.x];
  if (L.vlen == MIXED) {  // rare: the record offsets, summed by one lane
    if (lane == 0) leaf_offsets(L, c, offs);
    __syncthreads();
  }
  uint32_t* out = (uint32_t*)(image + (L.page - page_base) * page_size);
  const uint32_t ndw = L.span * (page_size / 4);
  for (uint32_t w = lane; w < ndw; w += 64) out[w] = leaf_dword(L, c, offs, w);
  if (lane == 0) first_key[blockIdx.x] = c.round(L.row0);
}

// The open leaf's rows [first, first + count) of (carried rows || new rows) into the writer's other carry set, and row
// last_row (the last row appended) into its `last` record; thread (row, w) writes dword w, zeros behind the value.
__global__ __launch_bounds__(256) void k_bolt_carry(const cols2 c, uint64_t first, uint64_t count, uint64_t last_row, const carry_out o) {
  const uint32_t dw = (o.stride > o.last_stride ? o.stride : o.last_stride) / 4;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t j = t / dw;
  const uint32_t w = (uint32_t)(t - j * dw);
  if (j > count) return;
  const bool is_last = j == count;
  if (4 * w >= (is_last ? o.last_stride : o.stride)) return;
  const uint64_t row = is_last ? last_row : first + j;
  const uint32_t len = c.len(row);
  uint32_t word = 0;
  for (uint32_t b = 0; b < 4; b++)
    if (4 * w + b < len) word |= (uint32_t)c.byte(row, 4 * w + b) << (8 * b);
  if (is_last) {
    ((uint32_t*)(o.last + 2))[w] = word;
    if (w == 0) {
      o.last[0] = c.round(row);
      o.last[1] = len;
    }
  } else {
    ((uint32_t*)o.rows)[j * (o.stride / 4) + w] = word;
    if (w == 0) {
      o.rounds[j] = c.round(row);
      o.lens[j] = len;
    }
  }
}

// first index in a[0, n) with a[i] >= x
__device__ __forceinline__ size_t lower_bound(const uint64_t* __restrict__ a, size_t n, uint64_t x) {
  size_t lo = 0, hi = n;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// slots [0, n): rows; [n, n + np): patches. flag = the slot goes to the output; lb = its lower bound in the other list.
// A deferred row no patch covers sets err_word. hit[j]: 1 = patch j replaced or deleted a row, 2 = it inserted, 0 = a
// delete of nothing.
__global__ __launch_bounds__(256) void k_bolt_merge(const merge_in m, uint32_t* __restrict__ flag, uint32_t* __restrict__ lb,
                                                    uint8_t* __restrict__ hit, uint32_t* __restrict__ err_word) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= m.n + m.np) return;
  if (idx < m.n) {
    const uint64_t r = m.rounds[idx];
    const size_t k = lower_bound(m.p_rounds, m.np, r);
    const bool covered = k < m.np && m.p_rounds[k] == r;
    flag[idx] = !covered;
    lb[idx] = (uint32_t)k;
    if (!covered && m.defer && m.defer[idx]) atomicOr(err_word, 1u);
  } else {
    const size_t j = idx - m.n;
    const uint64_t r = m.p_rounds[j];
    const size_t k = lower_bound(m.rounds, m.n, r);
    const bool found = k < m.n && m.rounds[k] == r, emit = m.p_lens[j] != 0xFFFFFFFFu;
    flag[idx] = emit;
    lb[idx] = (uint32_t)k;
    hit[j] = found ? 1 : (emit ? 2 : 0);
  }
}

// pos: the exclusive scan of flag (n + np + 1 words). A kept row lands behind the kept rows before it and the emitted
// patches of smaller rounds, a patch likewise; thread (slot, w) writes dword w of the slot's output row.
__global__ __launch_bounds__(256) void k_bolt_scatter(const merge_in m, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ lb,
                                                      const uint32_t* __restrict__ pos, const merge_out o) {
  const uint32_t dw = o.stride / 4;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t idx = t / dw;
  const uint32_t w = (uint32_t)(t - idx * dw);
  if (idx >= m.n + m.np || !flag[idx]) return;
  const bool is_row = idx < m.n;
  const size_t j = idx - m.n;
  const size_t at = is_row ? (size_t)pos[idx] + (pos[m.n + lb[idx]] - pos[m.n]) : (size_t)(pos[idx] - pos[m.n]) + pos[lb[idx]];
  const uint8_t* src = is_row ? m.rows + idx * (size_t)m.stride : m.p_rows + j * (size_t)m.p_stride;
  uint32_t len = is_row ? m.lens[idx] : m.p_lens[j];
  if (len > o.stride) len = 0;  // the host sized the stride for every value: never a prefix
  uint32_t word = 0;
  for (uint32_t b = 0; b < 4; b++)
    if (4 * w + b < len) word |= (uint32_t)src[4 * w + b] << (8 * b);
  ((uint32_t*)o.rows)[at * dw + w] = word;
  if (w == 0) {
    o.rounds[at] = is_row ? m.rounds[idx] : m.p_rounds[j];
    o.lens[at] = len;
    o.src[at] = is_row ? (uint32_t)idx : SRC_NONE;
  }
}

// merged row `at` taken from the hexjson record src[at] with a PreviousSig of nonzero length: unlinked unless the row
// before it is round - 1 and holds exactly those bytes. The row before the first is `pred` = {round, length, value
// from byte 16}: the last row of the window before this one. pred is always a readable address of 16 bytes, has_pred
// says whether it is that row: the pointer is wave-uniform, so its loads are scalar loads, which the compiler issues
// whatever the lanes' conditions are (no exec mask applies to them); a null pointer there faults.
__global__ __launch_bounds__(256) void k_bolt_unlinked(const merge_out o, size_t n_out, const uint8_t* __restrict__ prevs,
                                                       uint32_t prev_stride, const uint32_t* __restrict__ prev_lens,
                                                       const uint64_t* __restrict__ pred, uint32_t has_pred,
                                                       uint32_t* __restrict__ flag) {
  const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (at >= n_out) return;
  uint32_t f = 0;
  const uint32_t i = o.src[at];
  const uint32_t pl = i == SRC_NONE ? 0 : prev_lens[i];
  if (pl) {
    f = 1;
    const bool have = at > 0 || has_pred;
    const uint64_t before = !have ? 0 : at > 0 ? o.rounds[at - 1] : pred[0];
    const uint64_t before_len = !have ? 0 : at > 0 ? o.lens[at - 1] : pred[1];
    if (pl <= prev_stride && have && before + 1 == o.rounds[at] && before_len == pl) {
      const uint8_t* a = prevs + (size_t)i * prev_stride;
      const uint8_t* b = at > 0 ? o.rows + (at - 1) * (size_t)o.stride : (const uint8_t*)(pred + 2);
      f = 0;
      for (uint32_t k = 0; k < pl; k++) f |= a[k] != b[k];
    }
  }
  flag[at] = f;
}

__global__ __launch_bounds__(256) void k_bolt_compact(const uint64_t* __restrict__ rounds, const uint32_t* __restrict__ off, size_t n,
                                                      uint64_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (off[i + 1] != off[i]) out[off[i]] = rounds[i];
}

hipError_t launch_bolt_need(const cols& c, size_t n, const uint64_t* last, uint32_t* need, uint32_t* err_word, hipStream_t st) {
  if (n)  // without a row appended so far the kernel still gets a readable address: the new rounds
    hipLaunchKernelGGL(k_bolt_need, dim3(nblk(n, 256)), dim3(256), 0, st, c, n, last ? last : c.rounds, last ? 1u : 0u, need, err_word);
  return hipGetLastError();
}
hipError_t launch_bolt_pack(const void* leaves, size_t n_leaves, const cols2& c, uint32_t page_size, uint64_t page_base, uint8_t* image,
                            uint64_t* first_key, hipStream_t st) {
  if (!n_leaves) return hipGetLastError();
  if (c.n_carry)
    hipLaunchKernelGGL(k_bolt_pack<cols2>, dim3((unsigned)n_leaves), dim3(64), 0, st, (const leaf_desc*)leaves, c, page_size, page_base,
                       image, first_key);
  else  // one segment: the one-shot image's kernel
    hipLaunchKernelGGL(k_bolt_pack<cols>, dim3((unsigned)n_leaves), dim3(64), 0, st, (const leaf_desc*)leaves, c.fresh, page_size,
                       page_base, image, first_key);
  return hipGetLastError();
}
hipError_t launch_bolt_carry(const cols2& c, uint64_t first, uint64_t count, uint64_t last_row, const carry_out& o, hipStream_t st) {
  if (o.stride < 4 || o.last_stride < 4 || (o.stride | o.last_stride) & 3) return hipErrorInvalidValue;
  const size_t threads = (size_t)(count + 1) * (std::max(o.stride, o.last_stride) / 4);
  hipLaunchKernelGGL(k_bolt_carry, dim3(nblk(threads, 256)), dim3(256), 0, st, c, first, count, last_row, o);
  return hipGetLastError();
}
hipError_t launch_bolt_merge(const merge_in& m, uint32_t* flag, uint32_t* lb, uint8_t* hit, uint32_t* err_word, hipStream_t st) {
  if (m.n + m.np) hipLaunchKernelGGL(k_bolt_merge, dim3(nblk(m.n + m.np, 256)), dim3(256), 0, st, m, flag, lb, hit, err_word);
  return hipGetLastError();
}
hipError_t launch_bolt_scatter(const merge_in& m, const uint32_t* flag, const uint32_t* lb, const uint32_t* pos, const merge_out& o,
                               hipStream_t st) {
  const size_t threads = (m.n + m.np) * (size_t)(o.stride / 4);
  if (threads) hipLaunchKernelGGL(k_bolt_scatter, dim3(nblk(threads, 256)), dim3(256), 0, st, m, flag, lb, pos, o);
  return hipGetLastError();
}
hipError_t launch_bolt_unlinked(const merge_out& o, size_t n_out, const uint8_t* prevs, uint32_t prev_stride, const uint32_t* prev_lens,
                                const uint64_t* pred, uint32_t* flag, hipStream_t st) {
  // without a row before the window the kernel still gets a readable address: the merged rounds (n_out >= 1: 16 bytes
  // lie inside every device buffer of this library, which allocates 4 KiB at least)
  if (n_out)
    hipLaunchKernelGGL(k_bolt_unlinked, dim3(nblk(n_out, 256)), dim3(256), 0, st, o, n_out, prevs, prev_stride, prev_lens,
                       pred ? pred : o.rounds, pred ? 1u : 0u, flag);
  return hipGetLastError();
}
hipError_t launch_bolt_compact(const uint64_t* rounds, const uint32_t* off, size_t n, uint64_t* out, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_bolt_compact, dim3(nblk(n, 256)), dim3(256), 0, st, rounds, off, n, out);
  return hipGetLastError();
}

}  // namespace dh
