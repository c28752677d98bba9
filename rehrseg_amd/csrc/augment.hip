// nnU-Net training augmentation on the device (utils/seg_utils.py:632-728 get_training_transforms as REHRSeg calls it,
// utils/train_set.py:64-84 / :259-280), after the patch gather and before the step.
//
//   rehr_aug_warp2d_f32     the in-plane affine of MySpatialTransform with the dummy-2D conversion (every depth slice
//                           and every key shares one coordinate map per item): order-3 B-spline taps over coefficients
//                           prefiltered on the host-built tap tables of rehr_axis_resample_f32 (scipy map_coordinates,
//                           mode 'constant': a point outside [0, n-1] on either axis reads cval, interior taps mirror),
//                           or the batchgenerators label vote (order-1 indicator per label, >= 0.5 wins, the larger
//                           label last), its bilinear weights in fp64.
//   rehr_aug_stats_f32      sum, sum of squares, min, max of each item (fp64), per-block partials reduced in a fixed
//                           order (bitwise reproducible).
//   rehr_aug_pointwise_f32  one intensity step over every item, parameters and statistics read from device memory, so
//                           that the host never waits: noise (counter-based normal), brightness, contrast with its
//                           clip, the clip of the low-resolution simulation, gamma power, the retain-stats affine.
#include "common.h"

namespace {

constexpr int kStatThreads = 256;

__device__ __forceinline__ int mirror_index(int k, int n) {
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  k = k < 0 ? -k : k;
  k %= period;
  return k >= n ? period - k : k;
}

__device__ __forceinline__ double bspline3(double t) {
  t = t < 0.0 ? -t : t;
  if (t < 1.0) return 2.0 / 3.0 - t * t + 0.5 * t * t * t;
  if (t < 2.0) {
    const double u = 2.0 - t;
    return u * u * u / 6.0;
  }
  return 0.0;
}

// one thread per output pixel; grid (tiles, C, B)
__global__ __launch_bounds__(256) void warp2d_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                     const double* __restrict__ params, const int C, const int Hi,
                                                     const int Wi, const int Ho, const int Wo, const int mode) {
  const int b = blockIdx.z, c = blockIdx.y;
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= Ho * Wo) return;
  const int i = pix / Wo, j = pix % Wo;
  const double* p = params + (size_t)b * REHR_AUG_WARP_PARAMS;
  // coordinates as augment_spatial builds them: zero-centred mesh, (mesh^T R)^T, * scale, + centre; no contraction
  const double p0 = (double)i - (double)(Ho - 1) * 0.5, p1 = (double)j - (double)(Wo - 1) * 0.5;
  const double r0 = __dadd_rn(__dmul_rn(p0, p[0]), __dmul_rn(p1, p[2]));
  const double r1 = __dadd_rn(__dmul_rn(p0, p[1]), __dmul_rn(p1, p[3]));
  const double y = __dadd_rn(__dmul_rn(r0, p[4]), p[5]);
  const double x = __dadd_rn(__dmul_rn(r1, p[4]), p[6]);
  const float* s = src + ((size_t)b * C + c) * (size_t)Hi * Wi;
  float* d = dst + ((size_t)b * C + c) * (size_t)Ho * Wo;
  const bool inside = y >= 0.0 && y <= (double)(Hi - 1) && x >= 0.0 && x <= (double)(Wi - 1);
  if (!inside) {
    d[pix] = 0.f;  // data / uncertainty: cval 0; labels: every indicator reads -1, nothing is written over 0
    return;
  }
  const double fy = floor(y), fx = floor(x);
  const int iy = (int)fy, ix = (int)fx;
  if (mode == REHR_AUG_WARP_SPLINE3) {
    double wy[4], wx[4];
    int ry[4], rx[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      wy[t] = bspline3(y - (fy + (t - 1)));
      wx[t] = bspline3(x - (fx + (t - 1)));
      ry[t] = mirror_index(iy + t - 1, Hi);
      rx[t] = mirror_index(ix + t - 1, Wi);
    }
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const float* row = s + (size_t)ry[a] * Wi;
      double r = 0.0;
#pragma unroll
      for (int e = 0; e < 4; ++e) r += wx[e] * (double)row[rx[e]];
      acc += wy[a] * r;
    }
    d[pix] = (float)acc;
    return;
  }
  // label vote: indicator of each label interpolated bilinearly; the largest label whose indicator reaches 0.5 wins
  const double ty = y - fy, tx = x - fx;
  const double wy[2] = {1.0 - ty, ty}, wx[2] = {1.0 - tx, tx};
  float lab[4];
  double w[4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      lab[a * 2 + e] = s[(size_t)mirror_index(iy + a, Hi) * Wi + mirror_index(ix + e, Wi)];
      w[a * 2 + e] = wy[a] * wx[e];
    }
  float out = 0.f;
  bool any = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double ind = 0.0;
#pragma unroll
    for (int m = 0; m < 4; ++m) ind += lab[m] == lab[k] ? w[m] : 0.0;
    if (ind >= 0.5 && (!any || lab[k] > out)) {
      out = lab[k];
      any = true;
    }
  }
  d[pix] = out;
}

// grid (parts, B): partial {sum, sumsq, min, max} of a contiguous chunk
__global__ __launch_bounds__(kStatThreads) void stats_partial_kernel(const float* __restrict__ x, const int64_t S,
                                                                     const int parts, double* __restrict__ partial) {
  const int b = blockIdx.y, part = blockIdx.x;
  const int64_t chunk = (S + parts - 1) / parts;
  const int64_t lo = (int64_t)part * chunk, hi = lo + chunk < S ? lo + chunk : S;
  const float* xb = x + (size_t)b * S;
  double s = 0.0, q = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kStatThreads) {
    const float v = xb[i];
    s += (double)v;
    q += (double)v * (double)v;
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  __shared__ double red[4][kStatThreads / 64];
  s = wave_sum_d(s);
  q = wave_sum_d(q);
  mn = wave_min(mn);
  mx = wave_max(mx);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][wv] = s;
    red[1][wv] = q;
    red[2][wv] = mn;
    red[3][wv] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a[4] = {red[0][0], red[1][0], red[2][0], red[3][0]};
    for (int k = 1; k < kStatThreads / 64; ++k) {
      a[0] += red[0][k];
      a[1] += red[1][k];
      a[2] = fmin(a[2], red[2][k]);
      a[3] = fmax(a[3], red[3][k]);
    }
    double* o = partial + ((size_t)b * parts + part) * 4;
    for (int k = 0; k < 4; ++k) o[k] = a[k];
  }
}

__global__ __launch_bounds__(64) void stats_final_kernel(const double* __restrict__ partial, const int parts,
                                                         double* __restrict__ stats) {
  const int b = blockIdx.x;
  if (threadIdx.x != 0) return;
  const double* p = partial + (size_t)b * parts * 4;
  double a[4] = {p[0], p[1], p[2], p[3]};
  for (int k = 1; k < parts; ++k) {
    a[0] += p[k * 4 + 0];
    a[1] += p[k * 4 + 1];
    a[2] = fmin(a[2], p[k * 4 + 2]);
    a[3] = fmax(a[3], p[k * 4 + 3]);
  }
  for (int k = 0; k < 4; ++k) stats[b * 4 + k] = a[k];
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// standard normal of (seed, i): two 32-bit uniforms from a splitmix64 hash of the counter, Box-Muller
__device__ __forceinline__ float counter_normal(uint64_t seed, uint64_t i) {
  const uint64_t h = mix64(seed * 0x9e3779b97f4a7c15ull + mix64(i + 0x632be59bd9b4e019ull));
  const float u1 = ((float)(uint32_t)(h >> 32) + 1.0f) * 2.3283064e-10f;  // (0, 1]
  const float u2 = (float)(uint32_t)h * 2.3283064e-10f;                  // [0, 1)
  return sqrtf(-2.0f * __logf(u1)) * __cosf(6.2831853f * u2);
}

__device__ __forceinline__ void mean_std(const double* st, const int64_t S, double& mean, double& sd) {
  mean = st[0] / (double)S;
  const double var = st[1] / (double)S - mean * mean;
  sd = sqrt(var > 0.0 ? var : 0.0);
}

// grid (tiles, B); parameter record of the item in params[b * REHR_AUG_PW_PARAMS], [0] != 0: the step fires
__global__ __launch_bounds__(256) void pointwise_kernel(float* __restrict__ x, const int64_t S, const int op,
                                                        const double* __restrict__ params,
                                                        const double* __restrict__ st0,
                                                        const double* __restrict__ st1) {
  const int b = blockIdx.y;
  const double* p = params + (size_t)b * REHR_AUG_PW_PARAMS;
  if (p[0] == 0.0) return;
  float* xb = x + (size_t)b * S;
  // the per-item scalars, in the precision the reference's numpy arithmetic has them (float32 arrays, float32 stats)
  float a = 0.f, f = 1.f, lo = 0.f, hi = 0.f, g = 1.f, sgn = 1.f, m1 = 0.f, d1 = 1.f, s0 = 1.f, m0 = 0.f;
  uint64_t seed = 0;
  if (op == REHR_AUG_NOISE) {
    f = (float)p[1];
    seed = (uint64_t)p[2];
  } else if (op == REHR_AUG_SCALE) {
    f = (float)p[1];
  } else if (op == REHR_AUG_CONTRAST || op == REHR_AUG_CLIP) {
    double mean, sd;
    mean_std(st0 + b * 4, S, mean, sd);
    a = (float)mean;
    f = (float)p[1];
    lo = (float)st0[b * 4 + 2];
    hi = (float)st0[b * 4 + 3];
  } else if (op == REHR_AUG_GAMMA) {
    // x' = sgn * x; minm / rnge of x' from the statistics of x
    sgn = (float)p[2];
    g = (float)p[1];
    const float mnx = (float)st0[b * 4 + 2], mxx = (float)st0[b * 4 + 3];
    lo = sgn > 0.f ? mnx : -mxx;
    hi = (sgn > 0.f ? mxx : -mnx) - lo + 1e-7f;  // rnge + epsilon
  } else if (op == REHR_AUG_RETAIN) {
    sgn = (float)p[2];
    double mean0, sd0, mean1, sd1;
    mean_std(st0 + b * 4, S, mean0, sd0);
    mean_std(st1 + b * 4, S, mean1, sd1);
    m0 = sgn * (float)mean0;         // mean of x' = sgn * x
    m1 = (float)mean1;
    d1 = (float)sd1 + 1e-8f;
    s0 = (float)sd0;
  }
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = i0; i < S; i += step) {
    float v = xb[i];
    switch (op) {
      case REHR_AUG_NOISE: v = v + f * counter_normal(seed, (uint64_t)i); break;
      case REHR_AUG_SCALE: v = v * f; break;
      case REHR_AUG_CONTRAST:  // preserve_range: clipped to the item's range before the step
        v = (v - a) * f + a;
        v = v < lo ? lo : (v > hi ? hi : v);
        break;
      case REHR_AUG_CLIP: v = v < lo ? lo : (v > hi ? hi : v); break;
      case REHR_AUG_GAMMA: v = powf((sgn * v - lo) / hi, g) * hi + lo; break;
      case REHR_AUG_RETAIN: v = sgn * ((v - m1) / d1 * s0 + m0); break;
      default: break;
    }
    xb[i] = v;
  }
}

}  // namespace

extern "C" int rehr_aug_warp2d_f32(const float* src, float* dst, const double* params, int32_t B, int32_t C,
                                   int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t mode, void* stream) {
  if (src == nullptr || dst == nullptr || params == nullptr) return REHR_EINVAL;
  if (B < 1 || C < 1 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1 || C > 65535 || B > 65535) return REHR_EINVAL;
  if (mode != REHR_AUG_WARP_SPLINE3 && mode != REHR_AUG_WARP_LABEL) return REHR_EINVAL;
  if ((int64_t)Ho * Wo >= ((int64_t)1 << 31) || (int64_t)Hi * Wi >= ((int64_t)1 << 31)) return REHR_EINVAL;
  const int tiles = (int)(((int64_t)Ho * Wo + 255) / 256);
  hipLaunchKernelGGL(warp2d_kernel, dim3(tiles, C, B), dim3(256), 0, (hipStream_t)stream, src, dst, params, C, Hi, Wi,
                     Ho, Wo, mode);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_aug_stats_f32(const float* x, int32_t B, int64_t S, double* work, double* stats, void* stream) {
  if (x == nullptr || work == nullptr || stats == nullptr || B < 1 || B > 65535 || S < 1) return REHR_EINVAL;
  int64_t parts = (S + 8191) / 8192;
  parts = parts < REHR_AUG_STAT_PARTS ? parts : REHR_AUG_STAT_PARTS;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(stats_partial_kernel, dim3((unsigned)parts, B), dim3(kStatThreads), 0, st, x, S, (int)parts, work);
  hipLaunchKernelGGL(stats_final_kernel, dim3(B), dim3(64), 0, st, work, (int)parts, stats);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_aug_pointwise_f32(float* x, int32_t B, int64_t S, int32_t op, const double* params,
                                      const double* stats0, const double* stats1, void* stream) {
  if (x == nullptr || params == nullptr || B < 1 || B > 65535 || S < 1) return REHR_EINVAL;
  if (op < REHR_AUG_NOISE || op > REHR_AUG_RETAIN) return REHR_EINVAL;
  if ((op == REHR_AUG_CONTRAST || op == REHR_AUG_CLIP || op == REHR_AUG_GAMMA || op == REHR_AUG_RETAIN) &&
      stats0 == nullptr)
    return REHR_EINVAL;
  if (op == REHR_AUG_RETAIN && stats1 == nullptr) return REHR_EINVAL;
  int64_t blocks = (S + 255) / 256;
  blocks = blocks < 2048 ? blocks : 2048;
  hipLaunchKernelGGL(pointwise_kernel, dim3((unsigned)blocks, B), dim3(256), 0, (hipStream_t)stream, x, S, op, params,
                     stats0, stats1);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}
