// Microbenchmark: the Fp chain bodies on gfx950, 13 signed 30-bit digits against 14 unsigned 28-bit limbs.
//   sqr28 / mul28        fp_mul28.hpp m28::mont_sqr / mont_mul (v_mad_u64_u32, 301 / 392 MADs)
//   sqr30 / mul30        fp_mul30.hpp m30::mont_sqr / mont_mul (v_mad_i64_i32, 260 / 338 MADs)
//   mad_u64 / mad_i64    one bare dependent v_mad_u64_u32 / v_mad_i64_i32 chain (the premise: both issue at one rate)
// Each lane runs ONE dependent chain x = x^2 (or x = x * y) of IT steps between the library's entry and exit
// conversions, as an exponentiation does, at 1, 2 and 8 waves per SIMD (blocks of 256 threads = 1 wave per SIMD per
// CU). Both forms return x^(2^IT) (or x y^IT) in the canonical 12-word form, compared word for word.
// Build: hipcc --offload-arch=gfx950 -O3 -o bench/microbench_fp30 bench/microbench_fp30.hip
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../drand_amd/csrc/fp.hpp"
#include "../drand_amd/csrc/fp_mul30.hpp"

#define CHECK(x)                                                       \
  do {                                                                 \
    hipError_t e = (x);                                                \
    if (e != hipSuccess) {                                             \
      printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

using namespace dh;

constexpr int IT = 512;

struct F28 {
  typedef fp28 T;
  static __device__ __forceinline__ T in(const fp& x) { return fp28_from(x); }
  static __device__ __forceinline__ fp out(const T& x) { return fp28_to(x); }
  static __device__ __forceinline__ void sqr(T& x) { m28::mont_sqr(x.l, x.l); }
  static __device__ __forceinline__ void mul(T& x, const T& y) { m28::mont_mul(x.l, x.l, y.l); }
};
struct F30 {
  typedef m30::el T;
  static __device__ __forceinline__ T in(const fp& x) { return m30::from(x.v); }
  static __device__ __forceinline__ fp out(const T& x) {
    fp r;
    m30::to(r.v, x);
    return r;
  }
  static __device__ __forceinline__ void sqr(T& x) { m30::mont_sqr(x.l, x.l); }
  // the second operand is loop-invariant here, which the chains' products never are (a table entry loaded per step):
  // pinned to 32 bits per step as fp_mul30.hpp does for its one invariant operand, x^2 of the table build
  static __device__ __forceinline__ void mul(T& x, const T& y) {
    T e = y;
    m30::opaque(e);
    m30::mont_mul(x.l, x.l, e.l);
  }
};

template <class F, bool SQ>
__global__ __launch_bounds__(256) void k_chain(fp* out, const fp* in) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  typename F::T x = F::in(in[gid & 1023]);
  const typename F::T y = F::in(in[(gid + 1) & 1023]);
#pragma unroll 1
  for (int it = 0; it < IT; it++) {
    if (SQ)
      F::sqr(x);
    else
      F::mul(x, y);
  }
  out[gid] = F::out(x);
}

constexpr int MAD_ITERS = 1024;  // x 32 MADs per iteration
#define Q4(M) M M M M
__global__ void k_mad_u64(uint64_t* out, uint32_t seed) {
  uint64_t a0 = threadIdx.x + seed;
  const uint32_t b = blockIdx.x * 7 + 13, x = threadIdx.x * 3 + seed;
  uint64_t c;
  for (int it = 0; it < MAD_ITERS; it++) {
#define MD "v_mad_u64_u32 %0, %1, %3, %2, %0\n\t"
    asm volatile(Q4(Q4(MD)) Q4(Q4(MD)) : "+v"(a0), "=&s"(c) : "v"(b), "v"(x));
#undef MD
  }
  out[blockIdx.x * blockDim.x + threadIdx.x] = a0;
}
__global__ void k_mad_i64(uint64_t* out, uint32_t seed) {
  uint64_t a0 = threadIdx.x + seed;
  const uint32_t b = blockIdx.x * 7 + 13, x = threadIdx.x * 3 + seed;
  uint64_t c;
  for (int it = 0; it < MAD_ITERS; it++) {
#define MD "v_mad_i64_i32 %0, %1, %3, %2, %0\n\t"
    asm volatile(Q4(Q4(MD)) Q4(Q4(MD)) : "+v"(a0), "=&s"(c) : "v"(b), "v"(x));
#undef MD
  }
  out[blockIdx.x * blockDim.x + threadIdx.x] = a0;
}

template <typename K, typename A, typename B>
float time_kernel(K k, int blocks, A a, B b) {
  hipEvent_t s, e;
  (void)hipEventCreate(&s);
  (void)hipEventCreate(&e);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, a, b);
  (void)hipDeviceSynchronize();
  (void)hipEventRecord(s);
  for (int r = 0; r < 3; r++) hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, a, b);
  (void)hipEventRecord(e);
  (void)hipEventSynchronize(e);
  float ms;
  (void)hipEventElapsedTime(&ms, s, e);
  (void)hipEventDestroy(s);
  (void)hipEventDestroy(e);
  return ms / 3;
}

int main() {
  const int max_blocks = 256 * 8;
  const size_t n = (size_t)max_blocks * 256;
  fp *ref, *out, *in;
  uint64_t* buf;
  CHECK(hipMalloc(&ref, n * sizeof(fp)));
  CHECK(hipMalloc(&out, n * sizeof(fp)));
  CHECK(hipMalloc(&in, 1024 * sizeof(fp)));
  CHECK(hipMalloc(&buf, n * sizeof(uint64_t)));
  static fp hin[1024];
  uint64_t s = 0x9e3779b97f4a7c15ull;
  for (int i = 0; i < 1024; i++) {
    for (int j = 0; j < 12; j++) {
      s ^= s << 13; s ^= s >> 7; s ^= s << 17;
      hin[i].v[j] = (uint32_t)s;
    }
    hin[i].v[11] &= 0x0fffffffu;  // < p
  }
  CHECK(hipMemcpy(in, hin, sizeof(hin), hipMemcpyHostToDevice));
  std::vector<fp> hr(n), ho(n);
  struct Form {
    const char* name;
    void (*k)(fp*, const fp*);
    void (*ref)(fp*, const fp*);
  } forms[] = {{"sqr28", k_chain<F28, true>, nullptr},
               {"sqr30", k_chain<F30, true>, k_chain<F28, true>},
               {"mul28", k_chain<F28, false>, nullptr},
               {"mul30", k_chain<F30, false>, k_chain<F28, false>}};
  for (int wps : {1, 2, 8}) {
    const int blocks = 256 * wps;
    const double ops = (double)blocks * 256 * IT;
    for (auto& f : forms) {
      const float ms = time_kernel(f.k, blocks, out, (const fp*)in);
      long bad = -1;
      if (f.ref && wps == 2) {  // compare with the 28-bit form of the same operation
        hipLaunchKernelGGL(f.ref, dim3(blocks), dim3(256), 0, 0, ref, (const fp*)in);
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(hr.data(), ref, (size_t)blocks * 256 * sizeof(fp), hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(ho.data(), out, (size_t)blocks * 256 * sizeof(fp), hipMemcpyDeviceToHost));
        bad = 0;
        for (size_t i = 0; i < (size_t)blocks * 256; i++) bad += memcmp(&hr[i], &ho[i], sizeof(fp)) != 0;
      }
      printf("{\"op\": \"%s\", \"waves_per_simd\": %d, \"G_per_s\": %.2f, \"ms\": %.3f, \"mismatch\": %ld}\n", f.name, wps,
             ops / ms / 1e6, ms, bad);
    }
    const double steps = (double)blocks * 256 * MAD_ITERS * 32;
    const float mu = time_kernel(k_mad_u64, blocks, buf, 1u), mi = time_kernel(k_mad_i64, blocks, buf, 1u);
    printf("{\"op\": \"mad_u64\", \"waves_per_simd\": %d, \"T_mad_per_s\": %.2f}\n", wps, steps / mu / 1e9);
    printf("{\"op\": \"mad_i64\", \"waves_per_simd\": %d, \"T_mad_per_s\": %.2f, \"ratio_to_u64\": %.3f}\n", wps,
           steps / mi / 1e9, mu / mi);
  }
  CHECK(hipDeviceSynchronize());
  return 0;
}
