// Shared device/host helpers for the gfx950 kernels of librehrseg_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "rehrseg_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Launch bookkeeping.  hipGetLastError() is sticky per thread and may still hold
// an unrelated, harmless error from the host framework's own start-up; every
// launch therefore clears it first and records only its own outcome.
static thread_local int rehr_launch_failed = 0;
extern thread_local int rehr_last_hip_error_code;  // defined in elementwise.hip
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernelName, numBlocks, numThreads, memPerBlock, streamId, ...)           \
  do {                                                                                              \
    (void)hipGetLastError();                                                                        \
    kernelName<<<(numBlocks), (numThreads), (memPerBlock), (streamId)>>>(__VA_ARGS__);              \
    hipError_t e__ = hipGetLastError();                                                             \
    if (e__ != hipSuccess) { rehr_launch_failed = 1; rehr_last_hip_error_code = (int)e__; }         \
  } while (0)
#define REHR_LAUNCH_CHECK()                                   \
  do {                                                        \
    if (rehr_launch_failed) {                                 \
      rehr_launch_failed = 0;                                 \
      return REHR_EHIP;                                       \
    }                                                         \
  } while (0)

// Raises the dynamic-LDS limit of KERN to `bytes` at the first call of each instantiation (per process, not per device).
template <auto KERN>
int set_dyn_lds_once(int bytes) {
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) !=
        hipSuccess)
      return REHR_EHIP;
    attr_set = true;
  }
  return REHR_OK;
}
// The same for a kernel whose dynamic LDS depends on the problem: the limit only ever grows.
template <auto KERN>
int grow_dyn_lds(size_t bytes) {
  static size_t attr_bytes = 0;
  if (bytes > attr_bytes) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) !=
        hipSuccess)
      return REHR_EHIP;
    attr_bytes = bytes;
  }
  return REHR_OK;
}

// Bijective XCD-aware remap of a 1-D grid: blocks that the dispatcher places on
// the same XCD (b % 8 equal) become consecutive logical ids, so neighbouring
// tiles (shared halo / shared weight panel) hit the same 4 MiB L2.
__device__ __forceinline__ int xcd_remap(int b, int nb) {
  const int q = nb >> 3, r = nb & 7, xcd = b & 7;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (b >> 3);
}

__device__ __forceinline__ float apply_act(float v, int act, float slope) {
  if (act == REHR_ACT_RELU) return v > 0.f ? v : 0.f;
  if (act == REHR_ACT_LRELU) return v > 0.f ? v : v * slope;
  return v;
}
// derivative factor given the OUTPUT of the activation (slope > 0 keeps sign)
__device__ __forceinline__ float act_grad(float y, int act, float slope) {
  if (act == REHR_ACT_RELU) return y > 0.f ? 1.f : 0.f;
  if (act == REHR_ACT_LRELU) return y > 0.f ? 1.f : slope;
  return 1.f;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// integer counts (exact, so the order does not matter)
template <typename T, typename = std::enable_if_t<std::is_integral<T>::value>>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Fixed-order fp64 sums of a block of kSumThreads: a butterfly per wave, the four waves' partials through LDS, then
// ((w0 + w1) + w2) + w3.  The deterministic reductions of the metric, loss and validation kernels go through these
// functions, so that order is written once.
constexpr int kSumThreads = 256;
template <int K>
__device__ __forceinline__ double wave_order_sum(const double (*red)[K], const int k) {
  return ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}
// red[wave][k] = the wave's sum of v[k]; ends with the barrier after which every thread may read red
template <int K>
__device__ __forceinline__ void block_partials(double (&v)[K], double (*red)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum_d(v[k]);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave][k] = v[k];
  }
  __syncthreads();
}
// thread k < K writes the block's sum of value k to out[k]
template <int K>
__device__ __forceinline__ void block_sums(double (&v)[K], double (*red)[K], double* out) {
  block_partials(v, red);
  if (threadIdx.x < K) out[threadIdx.x] = wave_order_sum(red, threadIdx.x);
}
// one block per sample: out[k] = the sum of slot k of the sample's `per` tiles in w[per][K], in a fixed order
template <int K>
__device__ __forceinline__ void block_sums_of_tiles(const double* __restrict__ w, const int per, double (*red)[K],
                                                    double* out) {
  double v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = 0.0;
  for (int i = threadIdx.x; i < per; i += kSumThreads) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += w[(int64_t)i * K + k];
  }
  block_sums(v, red, out);
}

// Unsigned codes that order like the floats they encode: all bits of a negative flipped, the sign bit of the rest
// (-0 < +0).  A NaN has a code but no place in the order: it must not be fed to a min / max, and a select has to
// look for it on its own.
__device__ __forceinline__ uint32_t ord_of_bits(uint32_t bits) {
  return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ uint32_t bits_of_ord(uint32_t code) {
  return code ^ ((code >> 31) ? 0x80000000u : 0xffffffffu);
}
__device__ __forceinline__ uint32_t f2ord(float f) { return ord_of_bits(__float_as_uint(f)); }
__device__ __forceinline__ float ord2f(uint32_t code) { return __uint_as_float(bits_of_ord(code)); }

// 4 consecutive channels of one voxel in the activations' dtype (fp32, or bf16 on the mixed-precision path)
__device__ __forceinline__ void store4(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void store4(__bf16* p, const f32x4& v) {
  typedef __bf16 bf4_t __attribute__((ext_vector_type(4)));
  bf4_t o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (__bf16)v[e];
  *reinterpret_cast<bf4_t*>(p) = o;
}
__device__ __forceinline__ f32x4 load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 load4(const __bf16* p) {
  typedef __bf16 bf4_t __attribute__((ext_vector_type(4)));
  const bf4_t o = *reinterpret_cast<const bf4_t*>(p);
  return f32x4{(float)o[0], (float)o[1], (float)o[2], (float)o[3]};
}
