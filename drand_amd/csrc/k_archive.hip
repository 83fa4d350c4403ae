// client.RandomData JSON-lines archive -> verifier columns on the device. The archive image is
// resident in device memory (16-byte aligned, `len` bytes); every read below stays inside [file, file + len).
//   k_ndjson_count   one wave per tile of ARCHIVE_TILE bytes: the record starts in it (then launch_scan: tile bases)
//   k_ndjson_index   the same walk: line_off / line_len at base[tile] + rank, in file order (ballot + popcount rank)
//   k_ndjson_stat    one wave per chunk of 64 records: deferred records, longest line and decoded fields; then
//   k_ndjson_stat_fold folds the chunks
//   k_ndjson_gather  one wave per chunk of 64 records of a window: the columns dh_verify_batch_device takes
//   k_archive_fold   per record: the status byte of dh_archive_check (also behind k_packet.hip's protobuf gather)
// Memory-bound and small next to verification; plain C++, vector stores, no atomics anywhere.
#include <hip/hip_runtime.h>

#include "archive_chunk.hpp"
#include "kernels.hpp"
#include "rdjson.hpp"
#include "sha256.hpp"

namespace dh {
using namespace bolt;

namespace {
constexpr uint32_t TILE = ARCHIVE_TILE, ROW = 256;  // a wave reads a tile in rows of 64 dwords
constexpr uint32_t MAX_LEN = RDJSON_MAX_LINE + 1;   // the length recorded for every longer line

// the dword at pos (a multiple of 4); bytes at or beyond len read as '\n'
__device__ __forceinline__ uint32_t tile_word(const uint8_t* __restrict__ file, uint64_t len, uint64_t pos) {
  if (pos + 4 <= len) return *(const uint32_t*)(file + pos);
  uint32_t w = 0x0a0a0a0au;
  for (uint32_t k = 0; k < 4; k++)
    if (pos + k < len) w = (w & ~(0xffu << (8 * k))) | ((uint32_t)file[pos + k] << (8 * k));
  return w;
}
// bit k: byte k of w starts a record, pb being the byte before byte 0
__device__ __forceinline__ uint32_t start_bits(uint32_t w, uint32_t pb) {
  uint32_t m = 0;
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t b = (w >> (8 * k)) & 0xff;
    m |= (uint32_t)(b != '\n' && pb == '\n') << k;
    pb = b;
  }
  return m;
}
// the tile's rows: f(row offset in the tile, this lane's start bits)
template <class F>
__device__ __forceinline__ void tile_rows(const uint8_t* __restrict__ file, uint64_t len, uint64_t tile, F&& f) {
  const uint32_t lane = threadIdx.x;
  const uint64_t t0 = tile * TILE;
  uint32_t carry = t0 == 0 ? '\n' : file[t0 - 1];  // offset 0 starts a record like a byte after '\n'
  for (uint32_t r = 0; r < TILE && t0 + r < len; r += ROW) {
    const uint32_t w = tile_word(file, len, t0 + r + 4 * lane);
    uint32_t pb = __shfl_up(w >> 24, 1);
    if (lane == 0) pb = carry;
    carry = __shfl(w >> 24, 63);
    f(r, start_bits(w, pb));
  }
}
}  // namespace

__global__ __launch_bounds__(64) void k_ndjson_count(const uint8_t* __restrict__ file, uint64_t len, uint32_t* __restrict__ cnt) {
  uint32_t c = 0;
  tile_rows(file, len, blockIdx.x, [&](uint32_t, uint32_t bits) { c += __popc(bits); });
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (threadIdx.x == 0) cnt[blockIdx.x] = c;
}

__global__ __launch_bounds__(64) void k_ndjson_index(const uint8_t* __restrict__ file, uint64_t len, const uint32_t* __restrict__ base,
                                                     uint64_t* __restrict__ line_off, uint32_t* __restrict__ line_len) {
  __shared__ uint16_t start[TILE / 2 + 1];  // a record start needs a '\n' before it: at most TILE / 2 + 1 in a tile
  const uint32_t lane = threadIdx.x;
  uint32_t run = 0;
  tile_rows(file, len, blockIdx.x, [&](uint32_t r, uint32_t bits) {
    // file order is (lane, byte): the starts of lower lanes, then the lower bytes of this lane
    uint32_t lower = 0, total = 0;
    for (uint32_t k = 0; k < 4; k++) {
      const uint64_t m = __ballot((bits >> k) & 1);
      lower += __popcll(m & ((1ull << lane) - 1));
      total += __popcll(m);
    }
    for (uint32_t k = 0; k < 4; k++)
      if ((bits >> k) & 1) start[run + lower + __popc(bits & ((1u << k) - 1))] = (uint16_t)(r + 4 * lane + k);
    run += total;
  });
  __syncthreads();
  // a line that runs past the tile is measured here, by the workgroup that owns its start
  const uint64_t t0 = (uint64_t)blockIdx.x * TILE, rec0 = base[blockIdx.x];
  for (uint32_t s = lane; s < run; s += 64) {
    const uint64_t off = t0 + start[s];
    uint32_t n = 0;
    while (n < MAX_LEN) {
      const uint64_t p = off + n;
      if (p >= len) break;
      if (!(p & 3) && p + 4 <= len) {  // four bytes without a '\n' at once
        const uint32_t w = *(const uint32_t*)(file + p) ^ 0x0a0a0a0au;
        if (!((w - 0x01010101u) & ~w & 0x80808080u)) {
          n += 4;
          continue;
        }
      }
      if (file[p] == '\n') break;
      n++;
    }
    line_off[rec0 + s] = off;
    line_len[rec0 + s] = n < MAX_LEN ? n : MAX_LEN;
  }
}

namespace {
// the chunk's rows are consecutive in the output: lane t writes dword t of them, decoded from 8 hex characters
__device__ __forceinline__ void write_hex_rows(const uint8_t* src, uint8_t* __restrict__ rows, uint32_t stride, uint64_t row0, uint32_t cnt,
                                               const uint64_t* sel_off, const uint32_t* sel_hex) {
  const uint32_t dw = stride / 4;
  const view v{src, ~0ull};  // the offsets were bounds-checked by the parser
  for (uint32_t t = threadIdx.x; t < cnt * dw; t += 64) {
    const uint32_t s = t / dw, w = t - s * dw;
    const uint32_t nb = sel_hex[s] / 2;
    uint32_t word = 0;
    if (nb <= stride) {  // a longer value leaves the row zero, never a prefix
      const uint64_t k = sel_off[s] + 8 * (uint64_t)w;
      for (uint32_t j = 0; j < 4; j++)
        if (4 * w + j < nb) word |= hj_byte(v, k + 2 * j) << (8 * j);
    }
    ((uint32_t*)rows)[(row0 + s) * dw + w] = word;
  }
}
}  // namespace

__global__ __launch_bounds__(64) void k_ndjson_stat(const uint8_t* __restrict__ file, uint64_t len, const uint64_t* __restrict__ line_off,
                                                    const uint32_t* __restrict__ line_len, uint64_t n, archive_stat* __restrict__ out) {
  __shared__ uint4 lds[LDS_CHUNK / 16];
  const uint32_t lane = threadIdx.x;
  const uint64_t r0 = (uint64_t)blockIdx.x * 64;
  const uint32_t cnt = (uint32_t)(n - r0 < 64 ? n - r0 : 64);
  uint64_t origin;
  const uint8_t* src = stage_chunk(file, len, line_off + r0, line_len + r0, cnt, lds, &origin);
  uint32_t def = 0, ml = 0, ms = 0, mp = 0, mr = 0;
  if (lane < cnt) {
    rdjson r;
    ml = line_len[r0 + lane];
    def = !rdjson_parse(view{src + (line_off[r0 + lane] - origin), ml}, &r);
    ms = r.sig_hex / 2;
    mp = r.prev_hex / 2;
    mr = r.rand_hex / 2;
  }
  for (int o = 32; o > 0; o >>= 1) {
    def += __shfl_xor(def, o);
    ml = max(ml, (uint32_t)__shfl_xor(ml, o));
    ms = max(ms, (uint32_t)__shfl_xor(ms, o));
    mp = max(mp, (uint32_t)__shfl_xor(mp, o));
    mr = max(mr, (uint32_t)__shfl_xor(mr, o));
  }
  if (lane == 0) out[blockIdx.x] = archive_stat{def, ml, ms, mp, mr, 0};
}

// one workgroup: out[0] = the fold of in[0..n) (deferred records summed in 64 bits, the rest maxima)
__global__ __launch_bounds__(256) void k_ndjson_stat_fold(const archive_stat* __restrict__ in, size_t n, uint64_t* __restrict__ out) {
  __shared__ uint64_t sh[256][5];
  uint64_t a[5] = {0, 0, 0, 0, 0};
  for (size_t i = threadIdx.x; i < n; i += 256) {
    const archive_stat s = in[i];
    a[0] += s.n_deferred;
    a[1] = max(a[1], (uint64_t)s.max_line);
    a[2] = max(a[2], (uint64_t)s.max_sig);
    a[3] = max(a[3], (uint64_t)s.max_prev);
    a[4] = max(a[4], (uint64_t)s.max_rand);
  }
  for (int k = 0; k < 5; k++) sh[threadIdx.x][k] = a[k];
  __syncthreads();
  if (threadIdx.x < 5) {
    const int k = threadIdx.x;
    uint64_t t = 0;
    for (int j = 0; j < 256; j++) t = k == 0 ? t + sh[j][k] : max(t, sh[j][k]);
    out[k] = t;
  }
}

__global__ __launch_bounds__(64) void k_ndjson_gather(const uint8_t* __restrict__ file, uint64_t len, const uint64_t* __restrict__ line_off,
                                                      const uint32_t* __restrict__ line_len, uint64_t n, const archive_cols c) {
  __shared__ uint4 lds[LDS_CHUNK / 16];
  __shared__ uint64_t sig_off[64], prev_off[64], rand_off[64];  // from `src`: in place a chunk may span any distance
  __shared__ uint32_t sig_hex[64], prev_hex[64], rand_hex[64];
  const uint32_t lane = threadIdx.x;
  const uint64_t r0 = (uint64_t)blockIdx.x * 64;
  const uint32_t cnt = (uint32_t)(n - r0 < 64 ? n - r0 : 64);
  uint64_t origin;
  const uint8_t* src = stage_chunk(file, len, line_off + r0, line_len + r0, cnt, lds, &origin);
  if (lane < cnt) {
    // the structure of one record per lane: literals and field extents. A deferred record: zero lengths, zero rows
    rdjson r;
    const uint64_t at = line_off[r0 + lane] - origin;
    const bool canon = rdjson_parse(view{src + at, line_len[r0 + lane]}, &r);
    const uint64_t row = r0 + lane;
    c.rounds[row] = r.round;
    c.deferred[row] = !canon;
    if (c.sig_lens) c.sig_lens[row] = r.sig_hex / 2;
    if (c.prev_lens) c.prev_lens[row] = r.prev_hex / 2;
    if (c.rand_lens) c.rand_lens[row] = r.rand_hex / 2;
    sig_off[lane] = at + r.sig_off;
    prev_off[lane] = at + r.prev_off;
    rand_off[lane] = at + r.rand_off;
    sig_hex[lane] = r.sig_hex;
    prev_hex[lane] = r.prev_hex;
    rand_hex[lane] = r.rand_hex;
  }
  __syncthreads();
  if (c.sigs) write_hex_rows(src, c.sigs, c.sig_stride, r0, cnt, sig_off, sig_hex);
  if (c.prevs) write_hex_rows(src, c.prevs, c.prev_stride, r0, cnt, prev_off, prev_hex);
  if (c.rands) write_hex_rows(src, c.rands, 32, r0, cnt, rand_off, rand_hex);
}

namespace {
// is `expect` SHA-256 of the n bytes at p (the rare row whose signature has another length than the scheme's: the
// verifier's digest covers the scheme's length only)
__device__ bool sha256_is(const uint8_t* p, uint32_t n, const uint8_t* expect) {
  sha_h s = sha_iv();
  const uint32_t nb = (n + 9 + 63) / 64;
  for (uint32_t blk = 0; blk < nb; blk++) {
    uint32_t w[16];
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
      uint32_t v = 0;
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) {
        const uint32_t at = 64 * blk + 4 * j + k;
        const uint32_t b = at < n ? p[at] : (at == n ? 0x80u : 0u);
        v = (v << 8) | b;
      }
      if (blk == nb - 1 && j == 15) v = n * 8;
      w[j] = v;
    }
    sha_compress(s, w);
  }
  bool same = true;
#pragma unroll
  for (int i = 0; i < 8; i++) same = same && ld_be32(expect + 4 * i) == s.h[i];
  return same;
}
__device__ __forceinline__ bool same_bytes(const uint8_t* a, const uint8_t* b, uint32_t n) {
  for (uint32_t k = 0; k < n; k++)
    if (a[k] != b[k]) return false;
  return true;
}
}  // namespace

__global__ __launch_bounds__(256) void k_archive_fold(const archive_fold_in f, uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= f.n) return;
  if (f.deferred[i]) {
    status[i] = AR_DEFERRED;
    return;
  }
  const uint32_t sl = f.sig_lens[i];
  const uint8_t* sig = f.sigs + i * f.sig_stride;
  uint32_t st = 0;
  if (sl == 0) st |= AR_NO_SIGNATURE;
  if (sl != f.want_sig_len || !f.verdict[i]) st |= AR_INVALID;
  if (f.rand_lens[i]) {
    bool same = f.rand_lens[i] == 32;
    if (same && sl == f.want_sig_len) {
      same = same_bytes(f.rands + i * 32, f.rand_out + i * 32, 32);
    } else if (same) {
      same = sha256_is(sig, sl, f.rands + i * 32);  // sl <= sig_stride: the caller sized the rows by the longest value
    }
    if (!same) st |= AR_RANDOMNESS;
  }
  // the predecessor: the row before, or the carried row for row 0
  const bool has_pred = i > 0 || f.carry[0];
  if (has_pred) {
    const bool pdef = i > 0 ? f.deferred[i - 1] : f.carry[1];
    if (pdef) {
      st |= AR_PRED_DEFERRED;
    } else {
      const uint64_t pround = i > 0 ? f.rounds[i - 1] : *f.carry_round;
      const uint32_t plen = i > 0 ? f.sig_lens[i - 1] : *f.carry_len;
      const uint8_t* psig = i > 0 ? sig - f.sig_stride : f.carry_sig;
      if (f.rounds[i] != pround + 1) st |= AR_SEQUENCE;
      if (f.chained && (f.prev_lens[i] != plen || plen > f.sig_stride || plen > f.prev_stride ||
                        !same_bytes(f.prevs + i * f.prev_stride, psig, plen)))
        st |= AR_LINK;
    }
  }
  if (f.meta && (f.meta[i] & 3) == 1) st |= AR_BEACON_ID;  // metadata with another beaconID (sync_manager.go:385-389)
  status[i] = (uint8_t)st;
}

hipError_t launch_ndjson_count(const uint8_t* file, uint64_t len, size_t ntiles, uint32_t* cnt, hipStream_t st) {
  if (ntiles) hipLaunchKernelGGL(k_ndjson_count, dim3((unsigned)ntiles), dim3(64), 0, st, file, len, cnt);
  return hipGetLastError();
}
hipError_t launch_ndjson_index(const uint8_t* file, uint64_t len, size_t ntiles, const uint32_t* base, uint64_t* line_off, uint32_t* line_len,
                               hipStream_t st) {
  if (ntiles) hipLaunchKernelGGL(k_ndjson_index, dim3((unsigned)ntiles), dim3(64), 0, st, file, len, base, line_off, line_len);
  return hipGetLastError();
}
hipError_t launch_ndjson_stat(const uint8_t* file, uint64_t len, const uint64_t* line_off, const uint32_t* line_len, size_t n, void* chunks,
                              uint64_t* out5, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_ndjson_stat, dim3(nblk(n, 64)), dim3(64), 0, st, file, len, line_off, line_len, (uint64_t)n, (archive_stat*)chunks);
  return launch_ndjson_stat_fold(chunks, nblk(n, 64), out5, st);
}
hipError_t launch_ndjson_stat_fold(const void* chunks, size_t n_chunks, uint64_t* out5, hipStream_t st) {
  hipLaunchKernelGGL(k_ndjson_stat_fold, dim3(1), dim3(256), 0, st, (const archive_stat*)chunks, n_chunks, out5);
  return hipGetLastError();
}
hipError_t launch_ndjson_gather(const uint8_t* file, uint64_t len, const uint64_t* line_off, const uint32_t* line_len, size_t n,
                                const archive_cols& c, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_ndjson_gather, dim3(nblk(n, 64)), dim3(64), 0, st, file, len, line_off, line_len, (uint64_t)n, c);
  return hipGetLastError();
}
hipError_t launch_archive_fold(const archive_fold_in& f, uint8_t* status, hipStream_t st) {
  if (f.n) hipLaunchKernelGGL(k_archive_fold, dim3(nblk(f.n, 256)), dim3(256), 0, st, f, status);
  return hipGetLastError();
}

}  // namespace dh
