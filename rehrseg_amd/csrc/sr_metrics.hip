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
// HBM apart from the halo); the horizontal 11-tap pass over the five fields x, y, x^2, y^2, xy, the vertical pass that
// forms the window moments and the index itself are csrc/ssim_tile.h, the code the structure loss runs as well.  L1,
// MSE and the counts come from the tile's own 32x32 interior while it is staged, so every voxel counts once.
// Per-voxel terms and window moments are fp32, every sum across voxels, positions or blocks is fp64: the block's sums
// go to its own slot of the workspace and a second kernel adds the slots of a sample in a fixed order -- no
// floating-point atomics, the same bits on every run.
#include "ssim_tile.h"

#pragma clang fp contract(off)

namespace {

constexpr int kSlots = 6;             // doubles per block in the workspace

__device__ __forceinline__ float ld(const float* p) { return *p; }
__device__ __forceinline__ float ld(const __bf16* p) { return (float)*p; }

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

  // the window moments of x, y, x^2, y^2, xy: horizontal pass, barrier, vertical pass (ssim_tile.h)
  ssim_hpass_pair(g, sP, sT, sF);
  __syncthreads();

  {
    float m[5][4];
    ssim_vpass<5>(g, sF, m);
    const int x = x0 + ssim_column();
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      ssim_if_valid(y0 + ssim_row0() + o, x, H, W, [&] {
        s_ssim += (double)ssim_index(m[0][o], m[1][o], m[2][o], m[3][o], m[4][o], C1, C2).S;
      });
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
  block_sums_of_tiles(ws + (int64_t)blockIdx.x * per * kSlots, per, sRed, sOut);
  __syncthreads();
  if (threadIdx.x < 7) {
    const int k = threadIdx.x;
    stats[blockIdx.x * 7 + k] = k < 3 ? sOut[k] : (k == 3 ? ssim_cnt : sOut[k - 1]);
  }
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
  const int rc = tile_geometry(N, 1, D, H, W, true, &g);
  if (rc != REHR_OK) return rc;
  const auto [slots, need] = tile_sums_layout<kSlots>(workspace, g);
  if (workspace_bytes < need || misaligned(8, workspace, stats)) return REHR_EINVAL;
  static const int64_t zero[4] = {0, 0, 0, 0};
  if (slog == nullptr) ls = gs = zero;
  for (int a = 0; a < 4; ++a)
    if (ps[a] < 0 || ts[a] < 0 || ls[a] < 0 || gs[a] < 0) return REHR_EINVAL;
  const float c1 = 0.01f * data_range, c2 = 0.03f * data_range;
  hipLaunchKernelGGL(sr_metrics_tile_kernel<P>, dim3((unsigned)g.blocks), dim3(kThreads), 0, (hipStream_t)stream, pred,
                     ps[0], ps[1], ps[2], ps[3], tgt, ts[0], ts[1], ts[2], ts[3], slog, ls[0], ls[1], ls[2], ls[3], stgt,
                     gs[0], gs[1], gs[2], gs[3], D, H, W, g.tiles_x, g.tiles_y, c1 * c1, c2 * c2, gauss_taps(), slots);
  hipLaunchKernelGGL(sr_metrics_finish_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream,
                     (const double*)slots, (int)g.per, (double)D * (double)(H - 10) * (double)(W - 10), stats);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

}  // namespace

extern "C" int64_t rehr_sr_metrics_workspace_bytes(int32_t N, int32_t D, int32_t H, int32_t W) {
  Geometry g;
  const int rc = tile_geometry(N, 1, D, H, W, true, &g);
  return rc != REHR_OK ? rc : tile_sums_layout<kSlots>(nullptr, g).bytes;
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
  if (misaligned(2, pred, seg_logits)) return REHR_EINVAL;
  return sr_metrics<__bf16>((const __bf16*)pred, pred_strides, target, target_strides, (const __bf16*)seg_logits,
                            seg_logits_strides, seg_target, seg_target_strides, N, D, H, W, data_range, stats, workspace,
                            workspace_bytes, stream);
}
