// Microbenchmark: the Fp chain bodies on gfx950, 13 signed 30-bit digits against 14 unsigned 28-bit limbs.
//   sqr28 / mul28        fp_mul28.hpp m28::mont_sqr / mont_mul (v_mad_u64_u32, 301 / 392 MADs)
//   sqr30sep / mul30sep  the 30-bit body as it was before the columns were made dependent, kept here for comparison:
//                        every column summed from zero, the carry of the column below added afterwards, every output
//                        column rounded by its own 64-bit add (v_mad_i64_i32, 260 / 338 MADs, 61 other 64-bit ops)
//   sqr30 / mul30        fp_mul30.hpp m30::mont_sqr / mont_mul: dependent columns, paired rounding (37 other 64-bit ops)
//   sqr30x2 / mul30x2    fp_mul30.hpp m30::mont_sqr2 / mont_mul2: two such operations per lane in lockstep, as the
//                        G1 hash runs its two square-root chains; counted as two operations per step
//   mad_u64 / mad_i64    one bare dependent v_mad_u64_u32 / v_mad_i64_i32 chain (the premise: both issue at one rate)
// Each lane runs ONE dependent chain x = x^2 (or x = x * y) of IT steps (the x2 forms: two) between the library's
// entry and exit conversions, as an exponentiation does, at 1, 2 and 8 waves per SIMD (blocks of 256 threads = 1 wave
// per SIMD per CU). All forms return x^(2^IT) (or x y^IT) in the canonical 12-word form, compared word for word.
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
// the body before the dependent columns (see the head of this file)
namespace sep30 {
using m30::N;
using m30::N0;
using m30::P;
using m30::sext30;
#define SEP30_BODY(COL)                                                                  \
  int32_t Mq[N];                                                                         \
  int64_t acc = 0;                                                                       \
  _Pragma("unroll") for (int k = 0; k < N; k++) {                                        \
    COL(k, acc);                                                                         \
    _Pragma("unroll") for (int i = 0; i < k; i++) acc += (int64_t)Mq[i] * P(k - i);      \
    Mq[k] = sext30((uint32_t)acc * N0);                                                  \
    acc += (int64_t)Mq[k] * P(0);                                                        \
    acc >>= 30;                                                                          \
  }                                                                                      \
  _Pragma("unroll") for (int k = N; k < 2 * N - 1; k++) {                                \
    COL(k, acc);                                                                         \
    _Pragma("unroll") for (int i = k - (N - 1); i < N; i++) acc += (int64_t)Mq[i] * P(k - i); \
    R[k - N] = sext30((uint32_t)acc);                                                    \
    acc = (acc + (1 << 29)) >> 30;                                                       \
  }                                                                                      \
  R[N - 1] = (int32_t)acc;
__device__ __forceinline__ void mont_mul(int32_t R[N], const int32_t X[N], const int32_t Y[N]) {
#define COLM(k, acc)                                                                                  \
  _Pragma("unroll") for (int i = ((k) > N - 1 ? (k) - (N - 1) : 0); i <= ((k) < N - 1 ? (k) : N - 1); i++) \
      acc += (int64_t)X[i] * Y[(k) - i];
  SEP30_BODY(COLM)
#undef COLM
}
__device__ __forceinline__ void mont_sqr(int32_t R[N], const int32_t X[N]) {
  int32_t X2[N];
#pragma unroll
  for (int i = 0; i < N; i++) X2[i] = X[i] + X[i];
#define COLS(k, acc)                                                                        \
  _Pragma("unroll") for (int i = ((k) > N - 1 ? (k) - (N - 1) : 0); 2 * i < (k); i++)       \
      acc += (int64_t)X[i] * X2[(k) - i];                                                   \
  if (((k) & 1) == 0) acc += (int64_t)X[(k) / 2] * X[(k) / 2];
  SEP30_BODY(COLS)
#undef COLS
}
}  // namespace sep30

struct F30SEP {
  typedef m30::el T;
  static __device__ __forceinline__ T in(const fp& x) { return m30::from(x.v); }
  static __device__ __forceinline__ fp out(const T& x) {
    fp r;
    m30::to(r.v, x);
    return r;
  }
  static __device__ __forceinline__ void sqr(T& x) { sep30::mont_sqr(x.l, x.l); }
  static __device__ __forceinline__ void mul(T& x, const T& y) {
    T e = y;
    m30::opaque(e);
    sep30::mont_mul(x.l, x.l, e.l);
  }
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

// two chains per lane in lockstep: lane gid runs the chains of lanes gid and gid + 1 of k_chain
template <bool SQ>
__global__ __launch_bounds__(256) void k_chain2(fp* out, fp* out1, const fp* in) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  m30::el x0 = m30::from(in[gid & 1023].v), x1 = m30::from(in[(gid + 1) & 1023].v);
  const m30::el y0 = x1, y1 = m30::from(in[(gid + 2) & 1023].v);
#pragma unroll 1
  for (int it = 0; it < IT; it++) {
    if (SQ) {
      m30::mont_sqr2(x0.l, x1.l, x0.l, x1.l);
    } else {
      m30::el e0 = y0, e1 = y1;
      m30::opaque(e0);
      m30::opaque(e1);
      m30::mont_mul2(x0.l, x1.l, x0.l, x1.l, e0.l, e1.l);
    }
  }
  m30::to(out[gid].v, x0);
  m30::to(out1[gid].v, x1);
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

template <typename K, typename... A>
float time_kernel(K k, int blocks, A... a) {
  hipEvent_t s, e;
  (void)hipEventCreate(&s);
  (void)hipEventCreate(&e);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, a...);
  (void)hipDeviceSynchronize();
  (void)hipEventRecord(s);
  for (int r = 0; r < 3; r++) hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, a...);
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
  fp *ref, *out, *out1, *in;
  uint64_t* buf;
  CHECK(hipMalloc(&ref, n * sizeof(fp)));
  CHECK(hipMalloc(&out, n * sizeof(fp)));
  CHECK(hipMalloc(&out1, n * sizeof(fp)));
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
    void (*k2)(fp*, fp*, const fp*);  // the lockstep form, where k is null
    void (*ref)(fp*, const fp*);
  } forms[] = {{"sqr28", k_chain<F28, true>, nullptr, nullptr},
               {"sqr30sep", k_chain<F30SEP, true>, nullptr, k_chain<F28, true>},
               {"sqr30", k_chain<F30, true>, nullptr, k_chain<F28, true>},
               {"sqr30x2", nullptr, k_chain2<true>, k_chain<F28, true>},
               {"mul28", k_chain<F28, false>, nullptr, nullptr},
               {"mul30sep", k_chain<F30SEP, false>, nullptr, k_chain<F28, false>},
               {"mul30", k_chain<F30, false>, nullptr, k_chain<F28, false>},
               {"mul30x2", nullptr, k_chain2<false>, k_chain<F28, false>}};
  for (int wps : {1, 2, 8}) {
    const int blocks = 256 * wps;
    const size_t lanes = (size_t)blocks * 256;
    for (auto& f : forms) {
      const double ops = (double)lanes * IT * (f.k ? 1 : 2);
      const float ms = f.k ? time_kernel(f.k, blocks, out, (const fp*)in) : time_kernel(f.k2, blocks, out, out1, (const fp*)in);
      long bad = -1;
      if (f.ref && wps == 2) {  // compare with the 28-bit form of the same operation
        hipLaunchKernelGGL(f.ref, dim3(blocks), dim3(256), 0, 0, ref, (const fp*)in);
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(hr.data(), ref, lanes * sizeof(fp), hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(ho.data(), out, lanes * sizeof(fp), hipMemcpyDeviceToHost));
        bad = 0;
        for (size_t i = 0; i < lanes; i++) bad += memcmp(&hr[i], &ho[i], sizeof(fp)) != 0;
        if (!f.k) {  // the second chain of lane i is the chain of lane i + 1
          CHECK(hipMemcpy(ho.data(), out1, lanes * sizeof(fp), hipMemcpyDeviceToHost));
          for (size_t i = 0; i + 1 < lanes; i++) bad += memcmp(&hr[i + 1], &ho[i], sizeof(fp)) != 0;
        }
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
