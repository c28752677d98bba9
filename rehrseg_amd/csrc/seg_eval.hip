// Stage-2 validation on the device (utils/seg_utils.py:240-287 + :736-784, evaluate_case): the per-tile work of the
// tiled predictor with 8x mirror TTA, and the end of a case.
//
//   rehr_tta_gather_f32         the (8, 1, d, h, w) network input of one tile straight out of the un-padded volume:
//                               the identity, then the mirrorings of (D, H, W) in itertools.combinations order; a
//                               voxel outside the volume reads 0 (pad_nd_image 'constant', value 0).
//   rehr_tta_blend_f16acc       un-mirror the 8 outputs of a tile, sum them in the reference's order, / 8, * the fp16
//                               Gaussian weight, and add into the fp16 logits / count accumulators.  One thread per
//                               voxel, tiles in stream order: no atomics, deterministic.
//   rehr_seg_eval_finalize_f16  logits /= counts in place (fp16), the inf check over the whole padded volume, the
//                               argmax inside the un-padding crop, and the three integer Dice terms against a label map.
//
// Rounding contract: the fp32 operations torch performs on the same operands, each rounded once to fp16 on the store.
// The mirror sum runs p0 + p1 + ... + p7 left to right in fp32 and is divided by 8; `acc += p * g` is an fp32 product
// and an fp32 sum rounded once to fp16 (nothing contracted to an FMA); the count update is fp32(cnt) + fp32(g) and the
// normalisation an fp32 quotient, each rounded to fp16.  This is _internal_predict_sliding_window_return_logits with
// torch on the CPU, bit for bit.  On the device torch's `fp16 += fp32` rounds the fp32 operand to fp16 first for some
// operand layouts, so the device predictor differs from these kernels by one fp16 ulp on a few voxels.
#include <hip/hip_fp16.h>

#include "common.h"
#include "host_util.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;

// an fp32 value the compiler must materialise: keeps the backend from fusing `acc + p * g` into one v_fma_mix, or a
// fp32 sum / quotient and its fp16 rounding into one single-rounding instruction (contract(off) does not stop it)
__device__ __forceinline__ float f32_barrier(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// variant v of the TTA batch flips the axes of bit mask kFlip[v] (bit 0: depth, 1: height, 2: width): the identity,
// then itertools.combinations((2, 3, 4), r) for r = 1, 2, 3
__constant__ int kFlip[8] = {0, 1, 2, 4, 3, 5, 6, 1 | 2 | 4};

// grid-stride over the tile's rows of 4 voxels along w; VEC (w % 4 == 0): one 16-byte store per variant
template <bool VEC>
__global__ __launch_bounds__(kThreads) void tta_gather_kernel(const float* __restrict__ vol, float* __restrict__ out,
                                                              const int D, const int H, const int W, const int z0,
                                                              const int y0, const int x0, const int d, const int h,
                                                              const int w) {
  const int w4 = (w + 3) >> 2;
  const int64_t n = (int64_t)d * h * w4;
  const int64_t vstride = (int64_t)d * h * w;
  for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < n; t += (int64_t)gridDim.x * kThreads) {
    const int k0 = (int)(t % w4) * 4;
    const int j = (int)((t / w4) % h);
    const int i = (int)(t / ((int64_t)w4 * h));
    const int z = z0 + i, y = y0 + j;
    const bool row_in = z >= 0 && z < D && y >= 0 && y < H;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int x = x0 + k0 + e;
      v[e] = row_in && k0 + e < w && x >= 0 && x < W ? vol[((int64_t)z * H + y) * W + x] : 0.f;
    }
#pragma unroll
    for (int var = 0; var < 8; ++var) {
      const int m = kFlip[var];
      const int oi = (m & 1) ? d - 1 - i : i;
      const int oj = (m & 2) ? h - 1 - j : j;
      float* row = out + var * vstride + ((int64_t)oi * h + oj) * w;
      if (VEC) {
        const f32x4 o = (m & 4) ? f32x4{v[3], v[2], v[1], v[0]} : f32x4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(row + ((m & 4) ? w - 4 - k0 : k0)) = o;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k0 + e < w) row[(m & 4) ? w - 1 - (k0 + e) : k0 + e] = v[e];
      }
    }
  }
}

// one thread per voxel of the tile; the prediction is read through its strides (channels-last or contiguous)
__global__ __launch_bounds__(kThreads) void tta_blend_kernel(const float* __restrict__ pred, const int64_t sv,
                                                             const int64_t sc, const int64_t sd, const int64_t sh,
                                                             const int64_t sw, const int C, const int d, const int h,
                                                             const int w, const __half* __restrict__ gauss,
                                                             __half* __restrict__ acc, __half* __restrict__ cnt,
                                                             const int Do, const int Ho, const int Wo, const int od,
                                                             const int oh, const int ow) {
  const int64_t n = (int64_t)d * h * w;
  const int64_t plane = (int64_t)Do * Ho * Wo;
  for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < n; t += (int64_t)gridDim.x * kThreads) {
    const int k = (int)(t % w);
    const int j = (int)((t / w) % h);
    const int i = (int)(t / ((int64_t)w * h));
    int64_t off[8];
#pragma unroll
    for (int var = 0; var < 8; ++var) {
      const int m = kFlip[var];
      off[var] = var * sv + ((m & 1) ? d - 1 - i : i) * sd + ((m & 2) ? h - 1 - j : j) * sh +
                 ((m & 4) ? w - 1 - k : k) * sw;
    }
    const float g = gauss != nullptr ? __half2float(gauss[t]) : 1.0f;
    const int64_t o = ((int64_t)(od + i) * Ho + (oh + j)) * Wo + (ow + k);
    for (int c = 0; c < C; ++c) {
      const float* pc = pred + c * sc;
      float p = pc[off[0]];
#pragma unroll
      for (int var = 1; var < 8; ++var) p = __fadd_rn(p, pc[off[var]]);
      p = p / 8.0f;
      __half* a = acc + c * plane + o;
      *a = __float2half_rn(f32_barrier(__fadd_rn(__half2float(*a), f32_barrier(__fmul_rn(p, g)))));
    }
    cnt[o] = __float2half_rn(f32_barrier(__fadd_rn(__half2float(cnt[o]), g)));
  }
}

// V consecutive voxels per thread (V = 8: 16-byte loads and stores of the fp16 planes), grid-stride; the Dice terms
// are reduced over the wave and added with one atomic per wave; stats[0] is set on a normalised +-inf
template <int V>
__global__ __launch_bounds__(kThreads) void finalize_kernel(__half* __restrict__ logits,
                                                            const __half* __restrict__ cnt, const int D, const int H,
                                                            const int W, const int cd0, const int ch0, const int cw0,
                                                            const int CD, const int CH, const int CW,
                                                            uint8_t* __restrict__ labels,
                                                            const uint8_t* __restrict__ gt,
                                                            unsigned long long* __restrict__ stats) {
  typedef _Float16 h8_t __attribute__((ext_vector_type(V)));
  const int64_t HW = (int64_t)H * W, N = (int64_t)D * HW;
  const int64_t groups = N / V;
  __half* l1p = logits + N;
  uint64_t inter = 0, sp = 0, sg = 0;
  bool inf = false;
  for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < groups; t += (int64_t)gridDim.x * kThreads) {
    const int64_t f0 = t * V;
    h8_t a0, a1, nn;
    if (V == 8) {
      a0 = *reinterpret_cast<const h8_t*>(logits + f0);
      a1 = *reinterpret_cast<const h8_t*>(l1p + f0);
      nn = *reinterpret_cast<const h8_t*>(cnt + f0);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        a0[e] = (_Float16)__half2float(logits[f0 + e]);
        a1[e] = (_Float16)__half2float(l1p[f0 + e]);
        nn[e] = (_Float16)__half2float(cnt[f0 + e]);
      }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float c = (float)nn[e];
      const _Float16 q0 = (_Float16)f32_barrier((float)a0[e] / c), q1 = (_Float16)f32_barrier((float)a1[e] / c);
      a0[e] = q0;
      a1[e] = q1;
      inf |= __builtin_isinf((float)q0) || __builtin_isinf((float)q1);
      if (labels == nullptr) continue;
      const int64_t f = f0 + e;
      const int z = (int)(f / HW) - cd0, y = (int)((f % HW) / W) - ch0, x = (int)(f % W) - cw0;
      if (z < 0 || z >= CD || y < 0 || y >= CH || x < 0 || x >= CW) continue;
      const int64_t lo = ((int64_t)z * CH + y) * CW + x;
      const uint8_t p = (float)q1 > (float)q0 ? 1 : 0;  // ties (and NaN) go to class 0, as torch.argmax
      labels[lo] = p;
      if (gt != nullptr) {
        const uint8_t g = gt[lo];
        inter += p * g;
        sp += p;
        sg += g;
      }
    }
    if (V == 8) {
      *reinterpret_cast<h8_t*>(logits + f0) = a0;
      *reinterpret_cast<h8_t*>(l1p + f0) = a1;
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        logits[f0 + e] = __float2half_rn((float)a0[e]);
        l1p[f0 + e] = __float2half_rn((float)a1[e]);
      }
    }
  }
  if (inf) stats[0] = 1ull;  // plain vector store; every writer stores the same value
  if (gt != nullptr) {
    inter = wave_sum(inter);
    sp = wave_sum(sp);
    sg = wave_sum(sg);
    if ((threadIdx.x & 63) == 0) {
      if (inter) atomicAdd(stats + 1, (unsigned long long)inter);
      if (sp) atomicAdd(stats + 2, (unsigned long long)sp);
      if (sg) atomicAdd(stats + 3, (unsigned long long)sg);
    }
  }
}

}  // namespace

extern "C" int rehr_tta_gather_f32(const float* vol, float* out, int32_t D, int32_t H, int32_t W, int32_t pad_d,
                                   int32_t pad_h, int32_t pad_w, int32_t start_d, int32_t start_h, int32_t start_w,
                                   int32_t d, int32_t h, int32_t w, void* stream) {
  if (vol == nullptr || out == nullptr) return REHR_EINVAL;
  if (D < 1 || H < 1 || W < 1 || d < 1 || h < 1 || w < 1) return REHR_EINVAL;
  if (pad_d < 0 || pad_h < 0 || pad_w < 0 || start_d < 0 || start_h < 0 || start_w < 0) return REHR_EINVAL;
  // every read is checked against the un-padded volume and every write lands inside `out`, so the tile's position in
  // the padded volume needs no further check here
  if ((int64_t)d * h * w * 8 >= ((int64_t)1 << 40)) return REHR_EINVAL;
  const int64_t n = (int64_t)d * h * ((w + 3) / 4);
  const unsigned g = grid_for(n, kThreads, 8192);
  const int z0 = start_d - pad_d, y0 = start_h - pad_h, x0 = start_w - pad_w;
  if (w % 4 == 0)
    hipLaunchKernelGGL(tta_gather_kernel<true>, dim3(g), dim3(kThreads), 0, (hipStream_t)stream, vol, out, D, H, W,
                       z0, y0, x0, d, h, w);
  else
    hipLaunchKernelGGL(tta_gather_kernel<false>, dim3(g), dim3(kThreads), 0, (hipStream_t)stream, vol, out, D, H, W,
                       z0, y0, x0, d, h, w);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_tta_blend_f16acc(const float* pred, const int64_t* strides, int32_t C, int32_t d, int32_t h,
                                     int32_t w, const void* gaussian, void* logits, void* counts, int32_t Do,
                                     int32_t Ho, int32_t Wo, int32_t od, int32_t oh, int32_t ow, void* stream) {
  if (pred == nullptr || strides == nullptr || logits == nullptr || counts == nullptr) return REHR_EINVAL;
  if (C < 1 || C > 64 || d < 1 || h < 1 || w < 1 || Do < 1 || Ho < 1 || Wo < 1) return REHR_EINVAL;
  if (od < 0 || oh < 0 || ow < 0 || od + d > Do || oh + h > Ho || ow + w > Wo) return REHR_EINVAL;
  for (int a = 0; a < 5; ++a)
    if (strides[a] < 0) return REHR_EINVAL;
  const int64_t n = (int64_t)d * h * w;
  hipLaunchKernelGGL(tta_blend_kernel, dim3(grid_for(n, kThreads, 8192)), dim3(kThreads), 0, (hipStream_t)stream, pred,
                     strides[0], strides[1], strides[2], strides[3], strides[4], C, d, h, w,
                     (const __half*)gaussian, (__half*)logits, (__half*)counts, Do, Ho, Wo, od, oh, ow);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_seg_eval_finalize_f16(void* logits, const void* counts, int32_t D, int32_t H, int32_t W,
                                          int32_t crop_d, int32_t crop_h, int32_t crop_w, int32_t CD, int32_t CH,
                                          int32_t CW, uint8_t* labels, const uint8_t* gt, uint64_t* stats,
                                          void* stream) {
  if (logits == nullptr || counts == nullptr || stats == nullptr) return REHR_EINVAL;
  if (D < 1 || H < 1 || W < 1 || CD < 1 || CH < 1 || CW < 1) return REHR_EINVAL;
  if (crop_d < 0 || crop_h < 0 || crop_w < 0 || crop_d + CD > D || crop_h + CH > H || crop_w + CW > W)
    return REHR_EINVAL;
  if (gt != nullptr && labels == nullptr) return REHR_EINVAL;
  if (misaligned(2, logits, counts)) return REHR_EINVAL;
  const int64_t N = (int64_t)D * H * W;
  const bool vec = N % 8 == 0 && !misaligned(16, logits, counts);
  unsigned long long* st = reinterpret_cast<unsigned long long*>(stats);
  if (vec)
    hipLaunchKernelGGL(finalize_kernel<8>, dim3(grid_for(N / 8, kThreads, 2048)), dim3(kThreads), 0, (hipStream_t)stream,
                       (__half*)logits, (const __half*)counts, D, H, W, crop_d, crop_h, crop_w, CD, CH, CW, labels, gt,
                       st);
  else
    hipLaunchKernelGGL(finalize_kernel<1>, dim3(grid_for(N, kThreads, 2048)), dim3(kThreads), 0, (hipStream_t)stream,
                       (__half*)logits, (const __half*)counts, D, H, W, crop_d, crop_h, crop_w, CD, CH, CW, labels, gt,
                       st);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}
