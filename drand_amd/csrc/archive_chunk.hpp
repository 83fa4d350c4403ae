// What the archive kernels of k_archive.hip (JSON lines) and k_packet.hip (protobuf records) share: the staging of a
// chunk of 64 consecutive records in LDS. Device only.
#pragma once
#include <hip/hip_runtime.h>

#include "bolt.hpp"

namespace dh {
namespace {
constexpr uint32_t LDS_CHUNK = 36864;  // a chunk of up to 36 KiB is staged in LDS; larger ones are read in place
inline unsigned nblk(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

// The bytes of records [0, cnt) of a chunk (cnt <= 64, consecutive in the file) behind one pointer: staged in LDS
// with 16-byte loads when they fit, else the file itself. *origin = the file offset of the returned pointer.
__device__ __forceinline__ const uint8_t* stage_chunk(const uint8_t* __restrict__ file, uint64_t len, const uint64_t* __restrict__ line_off,
                                                      const uint32_t* __restrict__ line_len, uint32_t cnt, uint4* lds, uint64_t* origin) {
  const uint64_t a = line_off[0] & ~15ull, b = line_off[cnt - 1] + line_len[cnt - 1];  // b <= len: the index measured it, or the host checked the caller's extents
  if (b - a > LDS_CHUNK) {
    *origin = 0;
    return file;
  }
  const uint32_t nq = (uint32_t)((b - a + 15) / 16);
  for (uint32_t i = threadIdx.x; i < nq; i += 64) {
    const uint64_t p = a + 16 * (uint64_t)i;
    uint4 q;
    if (p + 16 <= len) {
      q = *(const uint4*)(file + p);
    } else {  // the image's last bytes
      uint32_t w[4] = {0, 0, 0, 0};
      for (uint32_t k = 0; k < 16 && p + k < len; k++) w[k / 4] |= (uint32_t)file[p + k] << (8 * (k & 3));
      q = make_uint4(w[0], w[1], w[2], w[3]);
    }
    lds[i] = q;
  }
  __syncthreads();
  *origin = a;
  return (const uint8_t*)lds;
}

}  // namespace
}  // namespace dh
