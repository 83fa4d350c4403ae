// Verifier columns on the device -> the records a node or relay serves:
//   form 1  client.RandomData through hexjson: {"round":D,"randomness":"H","signature":"H","previous_signature":"H"}
//   form 2  proto.Marshal of drand.PublicRandResponse: [08 V][12 L sig][1A L prev][22 20 rand][2A M metadata]
// every field left out when empty, randomness = SHA-256(signature) (RandomnessFromSignature) always 32 bytes.
//   k_serve_size    per row: the length of its record and of its frame; per workgroup the 64-bit sum and the first
//                   row that cannot be encoded
//   k_serve_encode  one wave per chunk of 64 rows: the records, built in LDS and streamed out with dword stores
// The passes and the output's dword discipline are k_pb_size / k_pb_encode's (k_packet.hip, encode_chunk.hpp); new
// here are the hex expansion of the payload rows and the digest computed by the lane that owns the row.
// Memory-bound and small next to verification; plain C++, vector stores, no atomics anywhere.
#include <hip/hip_runtime.h>

#include "encode_chunk.hpp"
#include "kernels.hpp"
#include "sha256.hpp"

namespace dh {

namespace {
constexpr uint32_t MAX_RECORD = 4096;         // a longer record is not written
constexpr uint32_t MAX_LEN = MAX_RECORD + 1;  // the length recorded for every longer record

// the count of decimal digits of v (1..20): comparisons against the powers of ten, no division
__device__ __forceinline__ uint32_t dec_digits(uint64_t v) {
  uint32_t d = 1;
  uint64_t p = 10;
#pragma unroll
  for (int k = 1; k < 20; k++) {
    d += v >= p;
    p *= 10;  // 10^19 < 2^64; the last product is not used
  }
  return d;
}
__device__ __forceinline__ uint32_t put_decimal(uint8_t* dst, uint32_t at, uint64_t v) {
  const uint32_t nd = dec_digits(v);
  for (uint32_t k = nd; k-- > 0;) {
    dst[at + k] = (uint8_t)('0' + v % 10);
    v /= 10;
  }
  return at + nd;
}
template <uint32_t N>
__device__ __forceinline__ uint32_t put_text(uint8_t* dst, uint32_t at, const char (&s)[N]) {
#pragma unroll
  for (uint32_t k = 0; k + 1 < N; k++) dst[at + k] = (uint8_t)s[k];
  return at + N - 1;
}
__device__ __forceinline__ uint8_t hex_digit(uint32_t x) { return (uint8_t)(x + (x < 10 ? '0' : 'a' - 10)); }
__device__ __forceinline__ void put_hex_byte(uint8_t* dst, uint32_t at, uint32_t byte) {
  dst[at] = hex_digit((byte >> 4) & 15);
  dst[at + 1] = hex_digit(byte & 15);
}

struct serve_row {
  uint64_t round;
  uint32_t sig_len, prev_len;
  bool keep;
};
__device__ __forceinline__ serve_row load_row(const serve_encode_in& e, uint64_t i) {
  return serve_row{e.rounds[i], e.sig_lens[i], e.prev_lens ? e.prev_lens[i] : 0u, !e.keep || e.keep[i] != 0};
}
// lengths at most MAX_RECORD each: no sum below passes 32 bits
__device__ __forceinline__ uint32_t record_len(const serve_encode_in& e, const serve_row& r) {
  if (e.form == SERVE_PUBLIC_RAND_PB) return (r.round ? 1 + varint_len(r.round) : 0) + field_len(r.sig_len) + field_len(r.prev_len) + 34 + e.meta_len;
  // {} 2; "round": 8 + digits; "randomness":"" 15 + 64; "signature":"" 14 + 2L; "previous_signature":"" 23 + 2L; commas between
  const uint32_t fields = (r.round ? 1 : 0) + 1 + (r.sig_len ? 1 : 0) + (r.prev_len ? 1 : 0);
  return 2 + (fields - 1) + (r.round ? 8 + dec_digits(r.round) : 0) + 79 + (r.sig_len ? 14 + 2 * r.sig_len : 0) +
         (r.prev_len ? 23 + 2 * r.prev_len : 0);
}
__device__ __forceinline__ uint32_t frame_len_of(const serve_encode_in& e, uint32_t l) {
  if (!e.framed) return l;
  return e.form == SERVE_PUBLIC_RAND_PB ? varint_len(l) + l : l + 1;
}

// a payload of nb bytes at src -> dst[at, ...): as it is for protobuf, 2 nb lowercase hex characters for JSON
__device__ __forceinline__ void put_payload(bool hex, uint8_t* dst, uint32_t at, const uint8_t* __restrict__ src, uint32_t nb) {
  if (hex)
    for (uint32_t k = 0; k < nb; k++) put_hex_byte(dst, at + 2 * k, src[k]);
  else
    for (uint32_t k = 0; k < nb; k++) dst[at + k] = src[k];
}

// Row i's frame at dst[0, frame length): every byte but the payloads taken from columns, whose places are returned
// (offsets in dst); with `whole` those payloads are written here too, byte by byte. The randomness is written here
// whenever it is computed (no rands column): it never exists outside the lane's registers and the record.
__device__ __forceinline__ void put_frame(const serve_encode_in& e, uint64_t i, const serve_row& r, uint8_t* dst, bool whole, uint32_t* sig_at,
                                          uint32_t* prev_at, uint32_t* rand_at) {
  const bool json = e.form != SERVE_PUBLIC_RAND_PB;
  const uint8_t* sig = e.sigs + i * e.sig_stride;
  uint32_t at = 0;
  *sig_at = *prev_at = 0;
  if (json) {
    dst[at++] = '{';
    if (r.round) {
      at = put_text(dst, at, "\"round\":");
      at = put_decimal(dst, at, r.round);
      dst[at++] = ',';
    }
    at = put_text(dst, at, "\"randomness\":\"");
    *rand_at = at;
    at += 64;
    dst[at++] = '"';
    if (r.sig_len) {
      at = put_text(dst, at, ",\"signature\":\"");
      *sig_at = at;
      at += 2 * r.sig_len;
      dst[at++] = '"';
    }
    if (r.prev_len) {
      at = put_text(dst, at, ",\"previous_signature\":\"");
      *prev_at = at;
      at += 2 * r.prev_len;
      dst[at++] = '"';
    }
    dst[at++] = '}';
    if (e.framed) dst[at++] = '\n';
  } else {
    if (e.framed) at = put_varint(dst, at, record_len(e, r));
    if (r.round) {
      dst[at++] = 0x08;
      at = put_varint(dst, at, r.round);
    }
    if (r.sig_len) {
      dst[at++] = 0x12;
      at = put_varint(dst, at, r.sig_len);
      *sig_at = at;
      at += r.sig_len;
    }
    if (r.prev_len) {
      dst[at++] = 0x1A;
      at = put_varint(dst, at, r.prev_len);
      *prev_at = at;
      at += r.prev_len;
    }
    dst[at++] = 0x22;
    dst[at++] = 0x20;
    *rand_at = at;
    at += 32;
    for (uint32_t k = 0; k < e.meta_len; k++) dst[at + k] = e.meta[k];
  }
  if (!e.rands) {
    const sha_h h = sha256_bytes(sig, r.sig_len);
#pragma unroll
    for (uint32_t k = 0; k < 32; k++) {
      const uint32_t byte = (h.h[k / 4] >> (8 * (3 - (k & 3)))) & 0xffu;
      if (json)
        put_hex_byte(dst, *rand_at + 2 * k, byte);
      else
        dst[*rand_at + k] = (uint8_t)byte;
    }
  } else if (whole) {
    put_payload(json, dst, *rand_at, e.rands + i * 32, 32);
  }
  if (whole) {
    put_payload(json, dst, *sig_at, sig, r.sig_len);
    if (r.prev_len) put_payload(json, dst, *prev_at, e.prevs + i * e.prev_stride, r.prev_len);
  }
}

// copy_rows with every byte expanded to two lowercase hex characters: lane t reads dword t of the rows (aligned) and
// writes its 8 characters (fewer for a row's partial last dword) at the row's place in the chunk (LDS, any alignment)
__device__ __forceinline__ void hex_rows(const uint8_t* __restrict__ rows, uint32_t stride, uint64_t row0, uint32_t cnt, uint8_t* dst,
                                         const uint32_t* at, const uint32_t* lens) {
  const uint32_t dw = stride / 4;
  for (uint32_t t = threadIdx.x; t < cnt * dw; t += 64) {
    const uint32_t s = t / dw, w = t - s * dw, nb = lens[s];
    if (4 * w >= nb) continue;
    const uint32_t word = ((const uint32_t*)rows)[(row0 + s) * dw + w];
    const uint32_t left = nb - 4 * w < 4 ? nb - 4 * w : 4;
    for (uint32_t k = 0; k < left; k++) put_hex_byte(dst, at[s] + 8 * w + 2 * k, (word >> (8 * k)) & 0xffu);
  }
}
}  // namespace

__global__ __launch_bounds__(256) void k_serve_size(const serve_encode_in e, uint64_t n, uint32_t* __restrict__ rec_len,
                                                    uint32_t* __restrict__ frame_len, pb_size_sum* __restrict__ sums) {
  __shared__ uint64_t sh_sum[256];
  __shared__ uint64_t sh_bad[256];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t sum = 0, bad = ~0ull;
  if (i < n) {
    const serve_row r = load_row(e, i);
    uint32_t l = 0, f = 0;
    if (r.keep) {  // a skipped row is not measured or refused
      // a value longer than its row cannot be read; a record above 4096 bytes is not written
      const bool fits = r.sig_len <= e.sig_stride && r.prev_len <= e.prev_stride && r.sig_len <= MAX_RECORD && r.prev_len <= MAX_RECORD;
      l = fits ? record_len(e, r) : MAX_LEN;
      if (l <= MAX_RECORD) {
        f = frame_len_of(e, l);
      } else {
        l = 0;
        bad = i;
      }
    }
    if (rec_len) rec_len[i] = l;
    frame_len[i] = f;
    sum = f;
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

// off: the exclusive scan of frame_len (n + 1 words). The chunk's region of `out` is [off[r0], off[r0 + cnt]), as in
// k_pb_encode; a chunk whose rows are all skipped has an empty region and stores nothing.
__global__ __launch_bounds__(64) void k_serve_encode(const serve_encode_in e, uint64_t n, const uint32_t* __restrict__ off, uint8_t* __restrict__ out) {
  __shared__ uint32_t lds[LDS_CHUNK / 4 + 2];  // the region, shifted so that LDS dwords are the output's aligned dwords
  __shared__ uint32_t sig_at[64], prev_at[64], rand_at[64], sig_len[64], prev_len[64], rand_len[64];
  const uint32_t lane = threadIdx.x;
  const uint64_t r0 = (uint64_t)blockIdx.x * 64;
  const uint32_t cnt = (uint32_t)(n - r0 < 64 ? n - r0 : 64);
  const uint32_t a = off[r0], b = off[r0 + cnt];
  if (a == b) return;
  const bool json = e.form != SERVE_PUBLIC_RAND_PB;
  serve_row r{0, 0, 0, false};
  if (lane < cnt) r = load_row(e, r0 + lane);
  if (b - a > LDS_CHUNK) {  // never with records of ordinary size: each lane writes its own frame byte by byte
    if (r.keep) {
      uint32_t s_at, p_at, d_at;
      put_frame(e, r0 + lane, r, out + off[r0 + lane], true, &s_at, &p_at, &d_at);
    }
    return;
  }
  const uint32_t shift = (uint32_t)(((uintptr_t)out + a) & 3);
  uint8_t* img = (uint8_t*)lds + shift;  // img[k] = byte a + k of the output
  if (lane < cnt) {
    uint32_t s_at = 0, p_at = 0, d_at = 0;
    const uint32_t base = off[r0 + lane] - a;
    if (r.keep) put_frame(e, r0 + lane, r, img + base, false, &s_at, &p_at, &d_at);
    sig_at[lane] = base + s_at;
    prev_at[lane] = base + p_at;
    rand_at[lane] = base + d_at;
    sig_len[lane] = r.keep ? r.sig_len : 0;
    prev_len[lane] = r.keep ? r.prev_len : 0;
    rand_len[lane] = r.keep ? 32 : 0;
  }
  __syncthreads();
  if (json) {
    hex_rows(e.sigs, e.sig_stride, r0, cnt, img, sig_at, sig_len);
    if (e.prev_lens) hex_rows(e.prevs, e.prev_stride, r0, cnt, img, prev_at, prev_len);
    if (e.rands) hex_rows(e.rands, 32, r0, cnt, img, rand_at, rand_len);
  } else {
    copy_rows(e.sigs, e.sig_stride, r0, cnt, img, sig_at, sig_len);
    if (e.prev_lens) copy_rows(e.prevs, e.prev_stride, r0, cnt, img, prev_at, prev_len);
    if (e.rands) copy_rows(e.rands, 32, r0, cnt, img, rand_at, rand_len);
  }
  __syncthreads();
  store_chunk(lds, out, a, b, shift);
}

hipError_t launch_serve_size(const serve_encode_in& e, size_t n, uint32_t* rec_len, uint32_t* frame_len, pb_size_sum* sums, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_serve_size, dim3(nblk(n, 256)), dim3(256), 0, st, e, (uint64_t)n, rec_len, frame_len, sums);
  return hipGetLastError();
}
hipError_t launch_serve_encode(const serve_encode_in& e, size_t n, const uint32_t* off, uint8_t* out, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_serve_encode, dim3(nblk(n, 64)), dim3(64), 0, st, e, (uint64_t)n, off, out);
  return hipGetLastError();
}

}  // namespace dh
