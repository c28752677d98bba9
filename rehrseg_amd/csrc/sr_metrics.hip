// Stage-1 validation on the device: L1, MSE, SSIM and the Dice counts of a predicted / target image pair in one pass.
//
//   rehr_sr_metrics_f32 / _bf16   seven fp64 numbers per sample of a logical (N, D, H, W) pair addressed through element
//                                 strides (the network's channels-last channel 0 next to a plane of an NCDHW target):
//                                 sum |p - t|, sum (p - t)^2, the sum of the SSIM index over the valid window positions
//                                 of every (H, W) slice, their number, and -- with the segmentation pair -- the exact
//                                 counts #(logit > 0 and target > 0.5), #(logit > 0), #(target > 0.5).
//
// SSIM is Wang et al. 2004 per slice: an 11x11 Gaussian window (sigma 1.5, unit sum, separable), the biased
// window-weighted variances E[x^2] - mu_x^2 and covariance, C1 = (0.01 R)^2, C2 = (0.03 R)^2, and only the positions
// whose window lies inside the slice.
//
// One block per 32x32 tile of one slice.  Both images are staged in LDS with a 5-pixel halo (42x42, read once from
// HBM apart from the halo), a horizontal 11-tap pass writes the five fields x, y, x^2, y^2, xy to LDS, a vertical pass
// forms the window moments and the index.  L1, MSE and the counts come from the tile's own 32x32 interior while it is
// staged, so every voxel counts once.  Per-voxel terms and window moments are fp32, every sum across voxels, positions
// or blocks is fp64: the block's sums go to its own slot of the workspace and a second kernel adds the slots of a
// sample in a fixed order -- no floating-point atomics, the same bits on every run.  x^2, y^2 and xy go through the
// same operations, and nothing below is contracted behind the source's back, so p == t gives an index of exactly 1.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;             // interior edge
constexpr int kHalo = 5;
constexpr int kRows = kTile + 2 * kHalo;   // 42 staged rows
constexpr int kPitch = 44;            // staged row pitch in floats: 16-byte rows, columns 42 / 43 are zero padding
constexpr int kSlots = 6;             // doubles per block in the workspace

struct GaussTaps {
  float w[11];
};

__device__ __forceinline__ float ld(const float* p) { return *p; }
__device__ __forceinline__ float ld(const __bf16* p) { return (float)*p; }

// thread t < kSlots adds the four waves' sums of value t in wave order and returns the total
__device__ __forceinline__ void block_sums(double (&v)[kSlots], double (*red)[kSlots], double* out) {
#pragma unroll
  for (int k = 0; k < kSlots; ++k) v[k] = wave_sum_d(v[k]);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < kSlots; ++k) red[wave][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < kSlots) {
    const int k = threadIdx.x;
    out[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

template <typename P>
__global__ __launch_bounds__(kThreads) void sr_metrics_tile_kernel(
    const P* __restrict__ pred, const int64_t pn, const int64_t pd, const int64_t ph, const int64_t pw,
    const float* __restrict__ tgt, const int64_t tn, const int64_t td, const int64_t th, const int64_t tw,
    const P* __restrict__ slog, const int64_t ln, const int64_t ldd, const int64_t lh, const int64_t lw,
    const float* __restrict__ stgt, const int64_t gn, const int64_t gd, const int64_t gh, const int64_t gw, const int D,
    const int H, const int W, const int tiles_x, const int tiles_y, const float C1, const float C2, const GaussTaps g,
    double* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float sP[kRows * kPitch];
  __shared__ __attribute__((aligned(16))) float sT[kRows * kPitch];
  __shared__ __attribute__((aligned(16))) float sF[5][kRows * kTile];
  __shared__ double sRed[kThreads / 64][kSlots];

  int b = blockIdx.x;
  const int tx = b % tiles_x;
  b /= tiles_x;
  const int ty = b % tiles_y;
  b /= tiles_y;
  const int d = b % D;
  const int n = b / D;
  const int x0 = tx * kTile, y0 = ty * kTile;
  const P* p0 = pred + n * pn + d * pd;
  const float* t0 = tgt + n * tn + d * td;

  double s_abs = 0.0, s_sq = 0.0, s_ssim = 0.0;
  unsigned c_inter = 0, c_pred = 0, c_tgt = 0;

  // stage both tiles with their halo; a position outside the slice holds 0 and reaches no valid window
  for (int i = threadIdx.x; i < kRows * kPitch; i += kThreads) {
    const int r = i / kPitch, c = i - r * kPitch;
    const int y = y0 - kHalo + r, x = x0 - kHalo + c;
    float p = 0.f, t = 0.f;
    if (c < kRows && y >= 0 && y < H && x >= 0 && x < W) {
      p = ld(p0 + y * ph + x * pw);
      t = t0[y * th + x * tw];
      if (r >= kHalo && r < kHalo + kTile && c >= kHalo && c < kHalo + kTile) {   // the tile's own voxels
        const float e = p - t;
        s_abs += (double)fabsf(e);
        s_sq += (double)(e * e);
        if (slog != nullptr) {
          const bool fp = ld(slog + n * ln + d * ldd + y * lh + x * lw) > 0.f;
          const bool ft = stgt[n * gn + d * gd + y * gh + x * gw] > 0.5f;
          c_inter += fp && ft;
          c_pred += fp;
          c_tgt += ft;
        }
      }
    }
    sP[i] = p;
    sT[i] = t;
  }
  __syncthreads();

  // horizontal pass: 4 neighbouring outputs per item from 16 staged columns (four 16-byte LDS reads per image)
  for (int i = threadIdx.x; i < kRows * (kTile / 4); i += kThreads) {
    const int r = i >> 3, q = (i & 7) * 4;
    float xs[16], ys[16];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(&sP[r * kPitch + q + 4 * v]);
      const f32x4 c = *reinterpret_cast<const f32x4*>(&sT[r * kPitch + q + 4 * v]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xs[4 * v + e] = a[e];
        ys[4 * v + e] = c[e];
      }
    }
    f32x4 f[5];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      float ax = 0.f, ay = 0.f, axx = 0.f, ayy = 0.f, axy = 0.f;
#pragma unroll
      for (int k = 0; k < 11; ++k) {
        const float x = xs[o + k], y = ys[o + k];
        ax = fmaf(g.w[k], x, ax);
        ay = fmaf(g.w[k], y, ay);
        axx = fmaf(g.w[k], x * x, axx);
        ayy = fmaf(g.w[k], y * y, ayy);
        axy = fmaf(g.w[k], x * y, axy);
      }
      f[0][o] = ax;
      f[1][o] = ay;
      f[2][o] = axx;
      f[3][o] = ayy;
      f[4][o] = axy;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) *reinterpret_cast<f32x4*>(&sF[k][r * kTile + q]) = f[k];
  }
  __syncthreads();

  // vertical pass: column c, 4 neighbouring rows per thread from 14 rows of every field
  {
    const int c = threadIdx.x & 31, r0 = (threadIdx.x >> 5) * 4;
    float m[5][4];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      float col[14];
#pragma unroll
      for (int j = 0; j < 14; ++j) col[j] = sF[k][(r0 + j) * kTile + c];
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 11; ++j) a = fmaf(g.w[j], col[o + j], a);
        m[k][o] = a;
      }
    }
    const int x = x0 + c;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int y = y0 + r0 + o;
      if (y >= kHalo && y < H - kHalo && x >= kHalo && x < W - kHalo) {
        const float mx = m[0][o], my = m[1][o];
        const float mxx = mx * mx, myy = my * my, mxy = mx * my;
        const float sxx = m[2][o] - mxx, syy = m[3][o] - myy, sxy = m[4][o] - mxy;
        const float num = (2.f * mxy + C1) * (2.f * sxy + C2);
        const float den = ((mxx + myy) + C1) * ((sxx + syy) + C2);
        s_ssim += (double)(num / den);
      }
    }
  }

  double v[kSlots] = {s_abs, s_sq, s_ssim, (double)c_inter, (double)c_pred, (double)c_tgt};
  block_sums(v, sRed, ws + (int64_t)blockIdx.x * kSlots);
}

// one block per sample: the slots of its `per` tiles in a fixed order
__global__ __launch_bounds__(kThreads) void sr_metrics_finish_kernel(const double* __restrict__ ws, const int per,
                                                                     const double ssim_cnt,
                                                                     double* __restrict__ stats) {
  __shared__ double sRed[kThreads / 64][kSlots];
  __shared__ double sOut[kSlots];
  const double* w = ws + (int64_t)blockIdx.x * per * kSlots;
  double v[kSlots] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < per; i += kThreads) {
#pragma unroll
    for (int k = 0; k < kSlots; ++k) v[k] += w[(int64_t)i * kSlots + k];
  }
  block_sums(v, sRed, sOut);
  __syncthreads();
  if (threadIdx.x < 7) {
    const int k = threadIdx.x;
    stats[blockIdx.x * 7 + k] = k < 3 ? sOut[k] : (k == 3 ? ssim_cnt : sOut[k - 1]);
  }
}

struct Geometry {
  int tiles_x, tiles_y;
  int64_t per, blocks;
};

int geometry(int32_t N, int32_t D, int32_t H, int32_t W, Geometry* g) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0) return REHR_EINVAL;
  if (H < 11 || W < 11) return REHR_ENOSUP;
  g->tiles_x = (W + kTile - 1) / kTile;
  g->tiles_y = (H + kTile - 1) / kTile;
  g->per = (int64_t)D * g->tiles_y * g->tiles_x;
  if (g->per > INT32_MAX / N) return REHR_ENOSUP;   // one 1-D grid
  g->blocks = g->per * N;
  return REHR_OK;
}

template <typename P>
int sr_metrics(const P* pred, const int64_t* ps, const float* tgt, const int64_t* ts, const P* slog, const int64_t* ls,
               const float* stgt, const int64_t* gs, int32_t N, int32_t D, int32_t H, int32_t W, float data_range,
               double* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  if (pred == nullptr || ps == nullptr || tgt == nullptr || ts == nullptr || stats == nullptr || workspace == nullptr)
    return REHR_EINVAL;
  if ((slog == nullptr) != (stgt == nullptr)) return REHR_EINVAL;
  if (slog != nullptr && (ls == nullptr || gs == nullptr)) return REHR_EINVAL;
  if (!(data_range > 0.f)) return REHR_EINVAL;
  Geometry g;
  const int rc = geometry(N, D, H, W, &g);
  if (rc != REHR_OK) return rc;
  if (workspace_bytes < g.blocks * kSlots * (int64_t)sizeof(double)) return REHR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(stats)) & 7) return REHR_EINVAL;
  static const int64_t zero[4] = {0, 0, 0, 0};
  if (slog == nullptr) ls = gs = zero;
  for (int a = 0; a < 4; ++a)
    if (ps[a] < 0 || ts[a] < 0 || ls[a] < 0 || gs[a] < 0) return REHR_EINVAL;
  GaussTaps taps;
  double e[11], sum = 0.0;
  for (int k = 0; k < 11; ++k) {
    e[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
    sum += e[k];
  }
  for (int k = 0; k < 11; ++k) taps.w[k] = (float)(e[k] / sum);
  const float c1 = 0.01f * data_range, c2 = 0.03f * data_range;
  hipLaunchKernelGGL(sr_metrics_tile_kernel<P>, dim3((unsigned)g.blocks), dim3(kThreads), 0, (hipStream_t)stream, pred,
                     ps[0], ps[1], ps[2], ps[3], tgt, ts[0], ts[1], ts[2], ts[3], slog, ls[0], ls[1], ls[2], ls[3], stgt,
                     gs[0], gs[1], gs[2], gs[3], D, H, W, g.tiles_x, g.tiles_y, c1 * c1, c2 * c2, taps,
                     (double*)workspace);
  hipLaunchKernelGGL(sr_metrics_finish_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream,
                     (const double*)workspace, (int)g.per, (double)D * (double)(H - 10) * (double)(W - 10), stats);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

}  // namespace

extern "C" int64_t rehr_sr_metrics_workspace_bytes(int32_t N, int32_t D, int32_t H, int32_t W) {
  Geometry g;
  const int rc = geometry(N, D, H, W, &g);
  return rc != REHR_OK ? rc : g.blocks * kSlots * (int64_t)sizeof(double);
}

extern "C" int rehr_sr_metrics_f32(const float* pred, const int64_t* pred_strides, const float* target,
                                   const int64_t* target_strides, const float* seg_logits,
                                   const int64_t* seg_logits_strides, const float* seg_target,
                                   const int64_t* seg_target_strides, int32_t N, int32_t D, int32_t H, int32_t W,
                                   float data_range, double* stats, void* workspace, int64_t workspace_bytes,
                                   void* stream) {
  return sr_metrics<float>(pred, pred_strides, target, target_strides, seg_logits, seg_logits_strides, seg_target,
                           seg_target_strides, N, D, H, W, data_range, stats, workspace, workspace_bytes, stream);
}

extern "C" int rehr_sr_metrics_bf16(const void* pred, const int64_t* pred_strides, const float* target,
                                    const int64_t* target_strides, const void* seg_logits,
                                    const int64_t* seg_logits_strides, const float* seg_target,
                                    const int64_t* seg_target_strides, int32_t N, int32_t D, int32_t H, int32_t W,
                                    float data_range, double* stats, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
  if ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(seg_logits)) & 1) return REHR_EINVAL;
  return sr_metrics<__bf16>((const __bf16*)pred, pred_strides, target, target_strides, (const __bf16*)seg_logits,
                            seg_logits_strides, seg_target, seg_target_strides, N, D, H, W, data_range, stats, workspace,
                            workspace_bytes, stream);
}
