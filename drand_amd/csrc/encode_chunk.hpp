// What the encoders of k_packet.hip (BeaconPacket) and k_serve.hip (RandomData JSON, PublicRandResponse) share: minimal
// varints, the copy of a chunk's payload rows into its LDS image, and the store of that image to the output. Device only.
#pragma once
#include <hip/hip_runtime.h>

#include "archive_chunk.hpp"

namespace dh {
namespace {
__device__ __forceinline__ uint32_t varint_len(uint64_t v) {
  uint32_t k = 1;
  while (v >>= 7) k++;
  return k;
}
__device__ __forceinline__ uint32_t put_varint(uint8_t* dst, uint32_t at, uint64_t v) {
  while (v >> 7) {
    dst[at++] = (uint8_t)(v | 0x80);
    v >>= 7;
  }
  dst[at++] = (uint8_t)v;
  return at;
}
__device__ __forceinline__ uint32_t field_len(uint32_t l) { return l ? 1 + varint_len(l) + l : 0; }

// rows [0, cnt) of a column, whose places in the chunk are dst + at[s]: lane t reads dword t of the rows (aligned) and
// writes its bytes (LDS, any alignment)
__device__ __forceinline__ void copy_rows(const uint8_t* __restrict__ rows, uint32_t stride, uint64_t row0, uint32_t cnt, uint8_t* dst,
                                          const uint32_t* at, const uint32_t* lens) {
  const uint32_t dw = stride / 4;
  for (uint32_t t = threadIdx.x; t < cnt * dw; t += 64) {
    const uint32_t s = t / dw, w = t - s * dw, nb = lens[s];
    if (4 * w >= nb) continue;
    const uint32_t word = ((const uint32_t*)rows)[(row0 + s) * dw + w];
    const uint32_t left = nb - 4 * w < 4 ? nb - 4 * w : 4;
    for (uint32_t k = 0; k < left; k++) dst[at[s] + 4 * w + k] = (uint8_t)(word >> (8 * k));
  }
}

// The chunk's region of `out` is bytes [a, b), b - a <= LDS_CHUNK: it starts and ends at any byte. lds holds it shifted
// by shift = (out + a) & 3, so that LDS dwords are the output's aligned dwords: LDS byte j is the output's byte
// a - shift + j. The dwords wholly inside go out with dword stores; the dwords shared with the neighbouring chunks are
// written with byte stores only, so no two workgroups ever store the same dword. One wave; call after a barrier.
__device__ __forceinline__ void store_chunk(const uint32_t* lds, uint8_t* __restrict__ out, uint32_t a, uint32_t b, uint32_t shift) {
  const uint32_t lane = threadIdx.x;
  uint8_t* g = out + a - shift;  // 4-byte aligned
  const uint32_t end = shift + (b - a);
  const uint32_t w0 = shift ? 1 : 0, w1 = end / 4;  // the dwords wholly inside the region
  for (uint32_t w = w0 + lane; w < w1; w += 64) ((uint32_t*)g)[w] = lds[w];
  // the partial dwords at both ends: the head [shift, 4) when shift != 0, the tail [4 * w1, end) when it is another dword
  // than the head (w1 >= w0; a region inside one dword is all head)
  if (lane < 4) {
    if (shift && lane >= shift && lane < end) g[lane] = ((const uint8_t*)lds)[lane];
  } else if (lane < 8) {
    const uint32_t j = 4 * w1 + (lane - 4);
    if (w1 >= w0 && j < end) g[j] = ((const uint8_t*)lds)[j];
  }
}

}  // namespace
}  // namespace dh
