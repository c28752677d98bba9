// Stage-1 volume preparation on the device (utils/sr_utils.py:244-277 postprocess_smore, the default path of
// train_all.py:321-330; rehrseg_amd/utils/sr_utils.py drives it).  All of it is streaming, HBM-bound work.
//
//   rehr_zoom_depth_f32                     scipy.ndimage.zoom(order=3) of the image channel and zoom(order=0) of the
//                                           label channel of the stored (X, Y, n, C) volume along its slice axis: an
//                                           exact recursive cubic B-spline prefilter with mirror boundaries carried in
//                                           fp64, then the 4-tap spline of a host-built table per output slice.
//   rehr_bspline_prefilter_axis_f64acc_f32  the prefilter alone along any axis of an (outer, n, inner) view.
//   rehr_blur_to_slices_f32                 the in-plane slice-profile blur of the (X, Y, Z) image along x or y, written
//                                           slice-major, (Z, X, Y) or (Z, Y, X): the tap-table resampling, the permute
//                                           and the copy of the data set's own route in one pass.
//
// Zoom kernel: a block owns LB consecutive (x, y) lines, so what it reads (LB * n * C floats) and what it writes
// (LB * Z floats, LB * Z bytes) are single contiguous runs.  The samples go from 16-byte loads into one fp64 LDS row per
// line (row stride n | 1 doubles: the lanes of a 32-lane group land on 32 different bank pairs), one lane per line runs
// the recursion over its row, and the outputs are evaluated by all threads in output order -- thread t takes 4
// consecutive output voxels -- so they leave in 16-byte stores with no second staging buffer.
//
// Rounding contract: ndimage's own fp64 operations in ndimage's order (ni_splines.c apply_filter / _init_causal_mirror /
// _init_anticausal_mirror, ni_interpolation.c NI_ZoomShift), one rounding each, nothing contracted; the result is rounded
// to fp32 once.  z^(n-1) and the other constants of the line come from the host's libm.  The blur is one fmaf per tap in
// tap order, as rehr_axis_resample_f32, so both routes to the blurred copies give the same bits.
#include <math.h>

#include "common.h"
#include "host_util.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kLdsBlock = 160 * 1024;  // what one workgroup may declare
constexpr int kLdsTarget = 40 * 1024;  // four workgroups per CU when the lines are short enough
constexpr int kMaxN = 283;             // 64 lines of (n | 1) doubles + n label bytes fit kLdsBlock up to here

struct Spline3 {
  double z;     // the pole sqrt(3) - 2
  double gain;  // (1 - z) (1 - 1 / z) = 6; 1 for a line of one sample, which ndimage leaves alone
  double zn1;   // z^(n - 1)
  double den0;  // 1 - zn1 * zn1
  double den1;  // z * z - 1
};

inline Spline3 spline3_consts(int n) {
  Spline3 k;
  k.z = sqrt(3.0) - 2.0;
  k.gain = n > 1 ? (1.0 - k.z) * (1.0 - 1.0 / k.z) : 1.0;
  k.zn1 = pow(k.z, (double)(n - 1));
  k.den0 = 1.0 - k.zn1 * k.zn1;
  k.den1 = k.z * k.z - 1.0;
  return k;
}

// c[i * s], i < n: the samples times the gain on entry, the B-spline coefficients on return.  The causal pass starts
// from the exact sum over the mirrored line, not from a truncated horizon.
__device__ __forceinline__ void bspline3_line(double* __restrict__ c, const int s, const int n, const Spline3& k) {
  if (n < 2) return;
  const double z = k.z;
  double v = c[0] + k.zn1 * c[(n - 1) * s];
  double zi = z;
  for (int i = 1; i < n - 1; ++i) {
    v = v + zi * (c[i * s] + k.zn1 * c[(n - 1 - i) * s]);
    zi = zi * z;
  }
  v = v / k.den0;
  c[0] = v;
  for (int i = 1; i < n; ++i) {
    v = c[i * s] + z * v;
    c[i * s] = v;
  }
  v = ((z * c[(n - 2) * s] + v) * z) / k.den1;
  c[(n - 1) * s] = v;
  for (int i = n - 2; i >= 0; --i) {
    v = z * (v - c[i * s]);
    c[i * s] = v;
  }
}

// lines per block: a multiple of 64 (whole waves in the recursion, 16-byte aligned regions), as many as kLdsTarget
// holds, at least 64 (n <= kMaxN makes those fit kLdsBlock)
inline int lines_per_block(int n, int C) {
  const int per_line = (n | 1) * 8 + (C == 2 ? n : 0);
  int lb = (kLdsTarget / per_line) / 64 * 64;
  return lb < 64 ? 64 : (lb > kThreads ? kThreads : lb);
}

// EVAL: the zoom (img / label out).  !EVAL: the coefficients themselves go back out (C == 1, the last-axis prefilter).
template <int C, bool EVAL>
__global__ __launch_bounds__(kThreads) void zoom_depth_kernel(
    const float* __restrict__ vol, const int64_t lines, const int n, const int32_t* __restrict__ idx,
    const double* __restrict__ w, const int32_t* __restrict__ nn, const int Z, float* __restrict__ img,
    uint8_t* __restrict__ label, const int LB, const Spline3 k, const bool vec_in, const bool vec_out) {
  extern __shared__ double s_c[];
  const int ns = n | 1;
  uint8_t* s_lab = reinterpret_cast<uint8_t*>(s_c + (size_t)LB * ns);
  const int64_t line0 = (int64_t)blockIdx.x * LB;
  const int nl = (int)(lines - line0 < LB ? lines - line0 : LB);
  const int tid = threadIdx.x;
  // the block's samples: one contiguous run of nl * n * C floats
  {
    const float* src = vol + line0 * n * C;
    const int count = nl * n * C;
    for (int f = tid * 4; f < count; f += kThreads * 4) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (vec_in && f + 3 < count) {
        v = *reinterpret_cast<const f32x4*>(src + f);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (f + e < count) v[e] = src[f + e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int g = f + e;
        if (g >= count) break;
        const int smp = g / C;
        const int line = smp / n;
        const int i = smp - line * n;
        if (C == 1 || (g & 1) == 0)
          s_c[line * ns + i] = (double)v[e] * k.gain;
        else
          s_lab[line * n + i] = (uint8_t)(int32_t)v[e];
      }
    }
  }
  __syncthreads();
  for (int l = tid; l < nl; l += kThreads) bspline3_line(s_c + l * ns, 1, n, k);
  __syncthreads();
  if (EVAL) {
    const int count = nl * Z;
    float* dst = img + line0 * Z;
    uint8_t* ldst = C == 2 ? label + line0 * Z : nullptr;
    for (int f = tid * 4; f < count; f += kThreads * 4) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      uint32_t lab4 = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int g = f + e;
        if (g >= count) break;
        const int line = g / Z;
        const int j = g - line * Z;
        const double* cl = s_c + line * ns;
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ix = min(max(idx[4 * j + q], 0), n - 1);
          t = t + cl[ix] * w[4 * j + q];
        }
        v[e] = (float)t;
        if (C == 2) {
          const int r = nn[j];
          if (r >= 0) lab4 |= (uint32_t)s_lab[line * n + min(r, n - 1)] << (8 * e);
        }
      }
      if (vec_out && f + 3 < count) {
        *reinterpret_cast<f32x4*>(dst + f) = v;
        if (C == 2) *reinterpret_cast<uint32_t*>(ldst + f) = lab4;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (f + e < count) {
            dst[f + e] = v[e];
            if (C == 2) ldst[f + e] = (uint8_t)(lab4 >> (8 * e));
          }
      }
    }
  } else {
    const int count = nl * n;
    float* dst = img + line0 * n;
    for (int f = tid * 4; f < count; f += kThreads * 4) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int g = f + e;
        if (g >= count) break;
        const int line = g / n;
        v[e] = (float)s_c[line * ns + (g - line * n)];
      }
      if (vec_out && f + 3 < count) {
        *reinterpret_cast<f32x4*>(dst + f) = v;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (f + e < count) dst[f + e] = v[e];
      }
    }
  }
}

// inner > 1: consecutive lines are consecutive in memory, one lane per line, its coefficients in column tid of an
// [n][T] fp64 LDS array (lanes on consecutive bank pairs)
__global__ __launch_bounds__(kThreads) void prefilter_strided_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                      const int64_t lines, const int n,
                                                                      const int64_t inner, const Spline3 k) {
  extern __shared__ double s_c[];
  const int T = blockDim.x;
  const int64_t line = (int64_t)blockIdx.x * T + threadIdx.x;
  if (line >= lines) return;
  const int64_t base = (line / inner) * n * inner + line % inner;
  double* c = s_c + threadIdx.x;
  for (int i = 0; i < n; ++i) c[i * T] = (double)x[base + i * inner] * k.gain;
  bspline3_line(c, T, n, k);
  for (int i = 0; i < n; ++i) y[base + i * inner] = (float)c[i * T];
}

// out[z][a][b] = sum_t taps[t] * img[(a + t - left) * sa + b * sb + z].  Block: 8 waves, a 32 (b) x 64 (z) tile and a
// chunk of a.  Loading, lane = z (coalesced) and every thread slides a register window of its 4 rows of b along a; the
// sums cross a padded LDS tile to leave along b, 8 lanes x 16 bytes per slice.
constexpr int kBlurThreads = 512, kTB = 32, kTZ = 64;

template <int LMAX>
__global__ __launch_bounds__(kBlurThreads) void blur_to_slices_kernel(const float* __restrict__ img,
                                                                      const float* __restrict__ taps, const int L,
                                                                      float* __restrict__ out, const int A, const int B,
                                                                      const int Z, const int64_t sa, const int64_t sb,
                                                                      const int chunk, const bool vec) {
  __shared__ float tile[kTB][kTZ + 1];
  const int b0 = blockIdx.x * kTB, z0 = blockIdx.z * kTZ;
  const int a0 = blockIdx.y * chunk;
  const int a1 = min(A, a0 + chunk);
  const int left = (L - 1) / 2;
  const int j = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int z = z0 + j;
  float k[LMAX];
#pragma unroll
  for (int t = 0; t < LMAX; ++t) k[t] = t < L ? taps[t] : 0.f;
  auto fetch = [&](int a) -> f32x4 {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (a < 0 || a >= A || z >= Z) return v;
    const float* p = img + (int64_t)a * sa + z;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int b = b0 + r + 8 * e;
      if (b < B) v[e] = p[(int64_t)b * sb];
    }
    return v;
  };
  // win[t]: the rows a + t - left (zero outside the axis and for t >= L)
  f32x4 win[LMAX];
#pragma unroll
  for (int t = 0; t < LMAX; ++t) win[t] = (t >= 1 && t < L) ? fetch(a0 + t - 1 - left) : f32x4{0.f, 0.f, 0.f, 0.f};
  const int lb = (threadIdx.x & 7) * 4, lz = threadIdx.x >> 3;
  for (int a = a0; a < a1; ++a) {
#pragma unroll
    for (int t = 0; t + 1 < LMAX; ++t) win[t] = win[t + 1];
    const f32x4 in = fetch(a + L - 1 - left);
#pragma unroll
    for (int t = 0; t < LMAX; ++t)
      if (t == L - 1) win[t] = in;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < LMAX; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(k[t], win[t][e], acc[e]);
    __syncthreads();  // the previous slice row has been read out of the tile
#pragma unroll
    for (int e = 0; e < 4; ++e) tile[r + 8 * e][j] = acc[e];
    __syncthreads();
    const int zz = z0 + lz, b = b0 + lb;
    if (zz < Z && b < B) {
      float* q = out + ((int64_t)zz * A + a) * B + b;
      if (vec) {  // B % 4 == 0: b + 3 < B
        *reinterpret_cast<f32x4*>(q) = f32x4{tile[lb][lz], tile[lb + 1][lz], tile[lb + 2][lz], tile[lb + 3][lz]};
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (b + e < B) q[e] = tile[lb + e][lz];
      }
    }
  }
}

template <int C, bool EVAL>
int launch_zoom(const float* vol, int64_t lines, int n, const int32_t* idx, const double* w, const int32_t* nn, int Z,
                float* img, uint8_t* label, hipStream_t stream) {
  const int LB = lines_per_block(n, C);
  const int lds = LB * ((n | 1) * 8 + (C == 2 ? n : 0));
  if (lds > kLdsBlock) return REHR_ENOSUP;
  const int64_t blocks = (lines + LB - 1) / LB;
  if (blocks > 0x7fffffff) return REHR_ENOSUP;
  if (set_dyn_lds_once<zoom_depth_kernel<C, EVAL>>(kLdsBlock) != REHR_OK) return REHR_EHIP;
  // LB % 4 == 0: every block's regions start on a multiple of 4 elements
  const bool vec_in = !misaligned(16, vol);
  const bool vec_out = !misaligned(16, img) && !misaligned(4, label);
  hipLaunchKernelGGL((zoom_depth_kernel<C, EVAL>), dim3((unsigned)blocks), dim3(kThreads), (size_t)lds, stream, vol,
                     lines, n, idx, w, nn, Z, img, label, LB, spline3_consts(n), vec_in, vec_out);
  return REHR_OK;
}

}  // namespace

extern "C" int rehr_zoom_depth_f32(const float* vol, int64_t lines, int32_t n, int32_t C, const int32_t* idx,
                                   const double* w, const int32_t* nn, int32_t Z, float* img, uint8_t* label,
                                   void* stream) {
  if (vol == nullptr || idx == nullptr || w == nullptr || img == nullptr) return REHR_EINVAL;
  if (lines < 1 || n < 1 || Z < 1 || (C != 1 && C != 2)) return REHR_EINVAL;
  if (C == 2 && (nn == nullptr || label == nullptr)) return REHR_EINVAL;
  if (misaligned(4, vol, img, idx, nn) || misaligned(8, w)) return REHR_EINVAL;
  if (lines * n * C >= ((int64_t)1 << 40) || lines * Z >= ((int64_t)1 << 40)) return REHR_EINVAL;
  if (n > kMaxN) return REHR_ENOSUP;
  if ((int64_t)Z * kThreads >= ((int64_t)1 << 30)) return REHR_ENOSUP;  // a block's output run is indexed in 32 bits
  int rc;
  if (C == 1)
    rc = launch_zoom<1, true>(vol, lines, n, idx, w, nullptr, Z, img, nullptr, (hipStream_t)stream);
  else
    rc = launch_zoom<2, true>(vol, lines, n, idx, w, nn, Z, img, label, (hipStream_t)stream);
  if (rc != REHR_OK) return rc;
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_bspline_prefilter_axis_f64acc_f32(const float* x, float* y, int64_t outer, int32_t n, int64_t inner,
                                                      void* stream) {
  if (x == nullptr || y == nullptr || x == y) return REHR_EINVAL;
  if (outer < 1 || n < 1 || inner < 1 || misaligned(4, x, y)) return REHR_EINVAL;
  if (outer >= ((int64_t)1 << 40) || inner >= ((int64_t)1 << 40) || outer * inner >= ((int64_t)1 << 40) ||
      outer * inner * n >= ((int64_t)1 << 40))
    return REHR_EINVAL;
  if (n > kMaxN) return REHR_ENOSUP;
  if (inner == 1) {
    const int rc = launch_zoom<1, false>(x, outer, n, nullptr, nullptr, nullptr, 1, y, nullptr, (hipStream_t)stream);
    if (rc != REHR_OK) return rc;
  } else {
    const int64_t lines = outer * inner;
    int T = kThreads;
    while (T > 64 && n * T * 8 > kLdsTarget) T >>= 1;
    const int lds = n * T * 8;  // <= kMaxN * 64 * 8 < kLdsBlock
    const int64_t blocks = (lines + T - 1) / T;
    if (blocks > 0x7fffffff) return REHR_ENOSUP;
    if (set_dyn_lds_once<prefilter_strided_kernel>(kLdsBlock) != REHR_OK) return REHR_EHIP;
    hipLaunchKernelGGL(prefilter_strided_kernel, dim3((unsigned)blocks), dim3(T), (size_t)lds, (hipStream_t)stream, x, y,
                       lines, n, inner, spline3_consts(n));
  }
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_blur_to_slices_f32(const float* img, const float* taps, int32_t L, float* out, int32_t X, int32_t Y,
                                       int32_t Z, int32_t axis, void* stream) {
  if (img == nullptr || taps == nullptr || out == nullptr || img == out) return REHR_EINVAL;
  if (L < 1 || X < 1 || Y < 1 || Z < 1 || (axis != 0 && axis != 1)) return REHR_EINVAL;
  if ((int64_t)X * Y * Z >= ((int64_t)1 << 40)) return REHR_EINVAL;
  if (misaligned(4, img, out, taps)) return REHR_EINVAL;
  if (L > 32) return REHR_ENOSUP;
  // a: the blurred axis, b: the other in-plane axis (the output's fastest)
  const int A = axis == 0 ? X : Y, B = axis == 0 ? Y : X;
  const int64_t sa = axis == 0 ? (int64_t)Y * Z : Z, sb = axis == 0 ? Z : (int64_t)Y * Z;
  const int tb = (B + kTB - 1) / kTB, tz = (Z + kTZ - 1) / kTZ;
  // every chunk re-reads L - 1 rows of its neighbours: long chunks, unless that leaves the device short of blocks
  int chunk = 64;
  while (chunk > 8 && (int64_t)tb * tz * ((A + chunk - 1) / chunk) < 512) chunk >>= 1;
  const dim3 grid((unsigned)tb, (unsigned)((A + chunk - 1) / chunk), (unsigned)tz);
  if (grid.y > 65535 || grid.z > 65535) return REHR_ENOSUP;
  const bool vec = B % 4 == 0 && !misaligned(16, out);
#define REHR_BLUR(LMAX)                                                                                             \
  hipLaunchKernelGGL((blur_to_slices_kernel<LMAX>), grid, dim3(kBlurThreads), 0, (hipStream_t)stream, img, taps, L, \
                     out, A, B, Z, sa, sb, chunk, vec)
  if (L <= 8)
    REHR_BLUR(8);
  else if (L <= 16)
    REHR_BLUR(16);
  else
    REHR_BLUR(32);
#undef REHR_BLUR
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}
