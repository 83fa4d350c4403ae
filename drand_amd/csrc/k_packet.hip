// Protobuf beacon records (BeaconPacket / PublicRandResponse, pbwire.hpp) <-> verifier columns on the device
// (DESIGN.md §26). The image is resident in device memory (16-byte aligned, `len` bytes); the caller gave every
// record's extent and the host checked that each lies inside [file, file + len).
//   k_pb_stat    one wave per chunk of 64 records: deferred records, longest record and fields (then k_ndjson_stat_fold)
//   k_pb_gather  one wave per chunk of 64 records of a window: the columns dh_verify_batch_device takes, and per
//                record whether metadata is present and whether its beaconID is the expected one
//   k_pb_size    per row of the verifier's columns: the length of its BeaconPacket and of its frame; per workgroup
//                the 64-bit sum and the first row that cannot be encoded
//   k_pb_encode  one wave per chunk of 64 rows: the packets, built in LDS and streamed out with dword stores
// Memory-bound and small next to verification; plain C++, vector stores, no atomics anywhere.
#include <hip/hip_runtime.h>

#include "archive_chunk.hpp"
#include "encode_chunk.hpp"
#include "kernels.hpp"
#include "pbwire.hpp"

namespace dh {
using namespace bolt;

namespace {
constexpr uint32_t MAX_LEN = PBWIRE_MAX_RECORD + 1;  // the length recorded for every longer record

// the aligned dword at apos (a multiple of 4) of src[0, limit); bytes at or beyond limit read as 0
__device__ __forceinline__ uint32_t src_word(const uint8_t* src, uint64_t limit, uint64_t apos) {
  if (apos + 4 <= limit) return *(const uint32_t*)(src + apos);
  uint32_t w = 0;
  for (uint32_t k = 0; k < 4; k++)
    if (apos + k < limit) w |= (uint32_t)src[apos + k] << (8 * k);
  return w;
}

// the chunk's rows are consecutive in the output: lane t writes dword t of them. The value's bytes sit at any
// alignment in src (LDS or the image, both 4-byte aligned): a dword is the byte-aligned cut of the two aligned dwords
// around it.
__device__ __forceinline__ void write_raw_rows(const uint8_t* src, uint64_t limit, uint8_t* __restrict__ rows, uint32_t stride, uint64_t row0,
                                               uint32_t cnt, const uint64_t* sel_off, const uint32_t* sel_len) {
  const uint32_t dw = stride / 4;
  for (uint32_t t = threadIdx.x; t < cnt * dw; t += 64) {
    const uint32_t s = t / dw, w = t - s * dw;
    const uint32_t nb = sel_len[s];
    uint32_t word = 0;
    if (nb <= stride && 4 * w < nb) {  // a longer value leaves the row zero, never a prefix
      const uint64_t pos = sel_off[s] + 4 * (uint64_t)w, apos = pos & ~3ull;
      const uint32_t sh = (uint32_t)(pos & 3);
      const uint32_t lo = src_word(src, limit, apos);
      const uint32_t hi = sh ? src_word(src, limit, apos + 4) : 0;
      word = __builtin_amdgcn_alignbyte(hi, lo, sh);
      const uint32_t left = nb - 4 * w;
      if (left < 4) word &= (1u << (8 * left)) - 1;
    }
    ((uint32_t*)rows)[(row0 + s) * dw + w] = word;
  }
}
}  // namespace

__global__ __launch_bounds__(64) void k_pb_stat(int kind, const uint8_t* __restrict__ file, uint64_t len, const uint64_t* __restrict__ rec_off,
                                                const uint32_t* __restrict__ rec_len, uint64_t n, archive_stat* __restrict__ out) {
  __shared__ uint4 lds[LDS_CHUNK / 16];
  const uint32_t lane = threadIdx.x;
  const uint64_t r0 = (uint64_t)blockIdx.x * 64;
  const uint32_t cnt = (uint32_t)(n - r0 < 64 ? n - r0 : 64);
  uint64_t origin;
  const uint8_t* src = stage_chunk(file, len, rec_off + r0, rec_len + r0, cnt, lds, &origin);
  uint32_t def = 0, ml = 0, ms = 0, mp = 0, mr = 0;
  if (lane < cnt) {
    pbrec r;
    const uint32_t l = rec_len[r0 + lane];
    ml = l < MAX_LEN ? l : MAX_LEN;
    def = !pbwire_parse(kind, view{src + (rec_off[r0 + lane] - origin), l}, &r);
    ms = r.sig_len;
    mp = r.prev_len;
    mr = r.rand_len;
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

__global__ __launch_bounds__(64) void k_pb_gather(int kind, const uint8_t* __restrict__ file, uint64_t len, const uint64_t* __restrict__ rec_off,
                                                  const uint32_t* __restrict__ rec_len, uint64_t n, const archive_cols c, const pb_meta_out x) {
  __shared__ uint4 lds[LDS_CHUNK / 16];
  __shared__ uint64_t sig_off[64], prev_off[64], rand_off[64];  // from `src`: in place a chunk may span any distance
  __shared__ uint32_t sig_len[64], prev_len[64], rand_len[64];
  const uint32_t lane = threadIdx.x;
  const uint64_t r0 = (uint64_t)blockIdx.x * 64;
  const uint32_t cnt = (uint32_t)(n - r0 < 64 ? n - r0 : 64);
  uint64_t origin;
  const uint8_t* src = stage_chunk(file, len, rec_off + r0, rec_len + r0, cnt, lds, &origin);
  const uint64_t limit = src == file ? len : LDS_CHUNK;
  if (lane < cnt) {
    // the structure of one record per lane: tags, lengths and field extents. A deferred record: zero lengths, zero rows
    pbrec r;
    const uint64_t at = rec_off[r0 + lane] - origin;
    const bool canon = pbwire_parse(kind, view{src + at, rec_len[r0 + lane]}, &r);
    const uint64_t row = r0 + lane;
    c.rounds[row] = r.round;
    c.deferred[row] = !canon;
    if (c.sig_lens) c.sig_lens[row] = r.sig_len;
    if (c.prev_lens) c.prev_lens[row] = r.prev_len;
    if (c.rand_lens) c.rand_lens[row] = r.rand_len;
    if (x.meta) {  // bit 0: metadata is present; bit 1: its beaconID is the expected one, byte for byte
      bool same = r.id_len == x.want_len;
      for (uint32_t k = 0; same && k < r.id_len; k++) same = src[at + r.id_off + k] == x.want[k];
      x.meta[row] = (uint8_t)(r.has_meta | (same ? 2u : 0u));
    }
    sig_off[lane] = at + r.sig_off;
    prev_off[lane] = at + r.prev_off;
    rand_off[lane] = at + r.rand_off;
    sig_len[lane] = r.sig_len;
    prev_len[lane] = r.prev_len;
    rand_len[lane] = r.rand_len;
  }
  __syncthreads();
  if (c.sigs) write_raw_rows(src, limit, c.sigs, c.sig_stride, r0, cnt, sig_off, sig_len);
  if (c.prevs) write_raw_rows(src, limit, c.prevs, c.prev_stride, r0, cnt, prev_off, prev_len);
  if (c.rands) write_raw_rows(src, limit, c.rands, 32, r0, cnt, rand_off, rand_len);
}

// ---- the encoder: verifier columns -> BeaconPacket bytes (beaconToProto, chain/beacon/convert.go:9-16 of the reference)

namespace {
struct pb_row {
  uint64_t round;
  uint32_t sig_len, prev_len;
};
__device__ __forceinline__ pb_row load_row(const pb_encode_in& e, uint64_t i) {
  return pb_row{e.rounds[i], e.sig_lens[i], e.prev_lens ? e.prev_lens[i] : 0u};
}
__device__ __forceinline__ uint32_t record_len(const pb_encode_in& e, const pb_row& r) {
  return field_len(r.prev_len) + (r.round ? 1 + varint_len(r.round) : 0) + field_len(r.sig_len) + e.meta_len;
}

// Row i's frame at dst[0, frame length): every byte but the two payloads, whose places are returned (offsets in dst);
// with `whole` the payloads are copied here too, byte by byte.
__device__ __forceinline__ void put_frame(const pb_encode_in& e, uint64_t i, uint8_t* dst, bool whole, uint32_t* sig_at, uint32_t* prev_at) {
  const pb_row r = load_row(e, i);
  uint32_t at = 0;
  if (e.delimited) at = put_varint(dst, at, record_len(e, r));
  *prev_at = *sig_at = 0;
  if (r.prev_len) {
    dst[at++] = 0x0A;
    at = put_varint(dst, at, r.prev_len);
    *prev_at = at;
    if (whole)
      for (uint32_t k = 0; k < r.prev_len; k++) dst[at + k] = e.prevs[i * e.prev_stride + k];
    at += r.prev_len;
  }
  if (r.round) {
    dst[at++] = 0x10;
    at = put_varint(dst, at, r.round);
  }
  if (r.sig_len) {
    dst[at++] = 0x1A;
    at = put_varint(dst, at, r.sig_len);
    *sig_at = at;
    if (whole)
      for (uint32_t k = 0; k < r.sig_len; k++) dst[at + k] = e.sigs[i * e.sig_stride + k];
    at += r.sig_len;
  }
  for (uint32_t k = 0; k < e.meta_len; k++) dst[at + k] = e.meta[k];
}
}  // namespace

__global__ __launch_bounds__(256) void k_pb_size(const pb_encode_in e, uint64_t n, uint32_t* __restrict__ rec_len, uint32_t* __restrict__ frame_len,
                                                 pb_size_sum* __restrict__ sums) {
  __shared__ uint64_t sh_sum[256];
  __shared__ uint64_t sh_bad[256];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t sum = 0, bad = ~0ull;
  if (i < n) {
    const pb_row r = load_row(e, i);
    // a value longer than its row cannot be read; a record above 4096 bytes is not written
    const bool fits = r.sig_len <= e.sig_stride && r.prev_len <= e.prev_stride && r.sig_len <= PBWIRE_MAX_RECORD && r.prev_len <= PBWIRE_MAX_RECORD;
    const uint32_t l = fits ? record_len(e, r) : MAX_LEN;
    const bool ok = l <= PBWIRE_MAX_RECORD;
    const uint32_t f = !ok ? 0 : (e.delimited ? varint_len(l) + l : l);
    if (rec_len) rec_len[i] = ok ? l : 0;
    frame_len[i] = f;
    sum = f;
    if (!ok) bad = i;
  }
  sh_sum[threadIdx.x] = sum;
  sh_bad[threadIdx.x] = bad;
  __syncthreads();
  for (uint32_t o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      sh_sum[threadIdx.x] += sh_sum[threadIdx.x + o];
      sh_bad[threadIdx.x] = min(sh_bad[threadIdx.x], sh_bad[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = pb_size_sum{sh_sum[0], sh_bad[0]};
}

// off: the exclusive scan of frame_len (n + 1 words). The chunk's region of `out` is [off[r0], off[r0 + cnt]): it starts
// and ends at any byte, and the dwords it shares with the neighbouring chunks are written with byte stores only, so no
// two workgroups ever store the same dword.
__global__ __launch_bounds__(64) void k_pb_encode(const pb_encode_in e, uint64_t n, const uint32_t* __restrict__ off, uint8_t* __restrict__ out) {
  __shared__ uint32_t lds[LDS_CHUNK / 4 + 2];  // the region, shifted so that LDS dwords are the output's aligned dwords
  __shared__ uint32_t sig_at[64], prev_at[64], sig_len[64], prev_len[64];
  const uint32_t lane = threadIdx.x;
  const uint64_t r0 = (uint64_t)blockIdx.x * 64;
  const uint32_t cnt = (uint32_t)(n - r0 < 64 ? n - r0 : 64);
  const uint32_t a = off[r0], b = off[r0 + cnt];
  if (b - a > LDS_CHUNK) {  // never with records of ordinary size: each lane writes its own frame byte by byte
    if (lane < cnt) {
      uint32_t s_at, p_at;
      put_frame(e, r0 + lane, out + off[r0 + lane], true, &s_at, &p_at);
    }
    return;
  }
  const uint32_t shift = (uint32_t)(((uintptr_t)out + a) & 3);
  uint8_t* img = (uint8_t*)lds + shift;  // img[k] = byte a + k of the output
  if (lane < cnt) {
    const uint32_t base = off[r0 + lane] - a;
    uint32_t s_at, p_at;
    put_frame(e, r0 + lane, img + base, false, &s_at, &p_at);
    sig_at[lane] = base + s_at;
    prev_at[lane] = base + p_at;
    sig_len[lane] = e.sig_lens[r0 + lane];
    prev_len[lane] = e.prev_lens ? e.prev_lens[r0 + lane] : 0;
  }
  __syncthreads();
  copy_rows(e.sigs, e.sig_stride, r0, cnt, img, sig_at, sig_len);
  if (e.prev_lens) copy_rows(e.prevs, e.prev_stride, r0, cnt, img, prev_at, prev_len);
  __syncthreads();
  store_chunk(lds, out, a, b, shift);
}

hipError_t launch_pb_stat(int kind, const uint8_t* file, uint64_t len, const uint64_t* rec_off, const uint32_t* rec_len, size_t n, void* chunks,
                          uint64_t* out5, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_pb_stat, dim3(nblk(n, 64)), dim3(64), 0, st, kind, file, len, rec_off, rec_len, (uint64_t)n, (archive_stat*)chunks);
  return launch_ndjson_stat_fold(chunks, nblk(n, 64), out5, st);
}
hipError_t launch_pb_gather(int kind, const uint8_t* file, uint64_t len, const uint64_t* rec_off, const uint32_t* rec_len, size_t n,
                            const archive_cols& c, const pb_meta_out& x, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_pb_gather, dim3(nblk(n, 64)), dim3(64), 0, st, kind, file, len, rec_off, rec_len, (uint64_t)n, c, x);
  return hipGetLastError();
}
hipError_t launch_pb_size(const pb_encode_in& e, size_t n, uint32_t* rec_len, uint32_t* frame_len, pb_size_sum* sums, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_pb_size, dim3(nblk(n, 256)), dim3(256), 0, st, e, (uint64_t)n, rec_len, frame_len, sums);
  return hipGetLastError();
}
hipError_t launch_pb_encode(const pb_encode_in& e, size_t n, const uint32_t* off, uint8_t* out, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_pb_encode, dim3(nblk(n, 64)), dim3(64), 0, st, e, (uint64_t)n, off, out);
  return hipGetLastError();
}

}  // namespace dh
