// Stage-1 structure losses: L1, L2, 1 - SSIM and a Sobel edge term of a predicted / target image pair, fused.
//
//   rehr_structure_loss_fwd_f32   one pass over both images: per-sample fp64 sums of |p - t|, (p - t)^2, the SSIM index
//                                 over the valid window positions and |G(p) - G(t)|, the weighted loss as one fp32
//                                 scalar on the device and (for the backward pass) the three SSIM coefficient fields.
//   rehr_structure_loss_bwd_f32   d loss / d input in gather form: every pixel is owned by one thread.
//
// Operands are logical (N, C, D, H, W) images addressed through five element strides; every (H, W) slice is an image.
// SSIM is the index of csrc/sr_metrics.hip by construction: both kernels run the taps, the two 11-tap passes and the
// index of csrc/ssim_tile.h on tiles staged the same way, so 1 - the SSIM term is the mean index rehr_sr_metrics_f32
// reports, bit for bit.  G is the Sobel magnitude sqrt(gx^2 + gy^2 + 1e-6) with the 3x3 kernels / 8 and
// replicate padding.  The tiles are staged with CLAMPED coordinates: that is the replicate padding the Sobel term
// needs, and the SSIM term never looks at a staged position outside the slice from a valid window.
//
// Forward: one block per 32x32 tile of one slice, staged with a 5-pixel halo as sr_metrics does.  Backward: the forward
// stored, per valid window position i, a_i = dS/dmu_x, b_i = dS/dE[x^2], c_i = dS/dE[xy]; the gradient of the SSIM
// term at pixel j is -(ssim / M) ((w * a)_j + 2 x_j (w * b)_j + y_j (w * c)_j), two 11-tap passes over the three
// fields staged with a 5-pixel halo (zero outside the valid positions).  The Sobel term needs u = sign(G(p) - G(t))
// (gx, gy) / G(p) on tile + 1, from the images on tile + 2, and gathers the 3x3 neighbours with the adjoint of the
// replicate padding.  A weight of 0 skips its term's arithmetic, its staging included.
#include "ssim_tile.h"

#pragma clang fp contract(off)

namespace {

constexpr int kSlots = 4;             // doubles per block in the workspace
constexpr int kImg = kTile + 4;       // backward: images with a 2-pixel halo
constexpr int kImgPitch = kImg + 1;
constexpr int kU = kTile + 2;         // backward: the Sobel fields with a 1-pixel halo
constexpr int kUPitch = kU + 1;
enum { kL1 = 1, kL2 = 2, kSsim = 4, kSobel = 8 };

struct View {        // a logical (N, C, D, H, W) fp32 image in element strides
  float* p;
  int64_t n, c, d, h, w;
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the Sobel responses / 8 and the magnitude at the staged position i of an image of row pitch `pitch`
__device__ __forceinline__ float sobel(const float* s, const int pitch, const int i, float& gx, float& gy) {
  const float a = s[i - pitch - 1], b = s[i - pitch], c = s[i - pitch + 1];
  const float d = s[i - 1], f = s[i + 1];
  const float g = s[i + pitch - 1], h = s[i + pitch], k = s[i + pitch + 1];
  gx = (((c - a) + 2.f * (f - d)) + (k - g)) * 0.125f;
  gy = (((g - a) + 2.f * (h - b)) + (k - c)) * 0.125f;
  return sqrtf((gx * gx + gy * gy) + 1e-6f);
}

// blockIdx.x -> tile origin and the slice's index (n * C + c) * D + d
__device__ __forceinline__ void locate(const int tiles_x, const int tiles_y, const int C, const int D, int& x0, int& y0,
                                       int& n, int& c, int& d, int64_t& img) {
  int b = blockIdx.x;
  x0 = (b % tiles_x) * kTile;
  b /= tiles_x;
  y0 = (b % tiles_y) * kTile;
  b /= tiles_y;
  img = b;
  d = b % D;
  b /= D;
  c = b % C;
  n = b / C;
}

__global__ __launch_bounds__(kThreads) void structure_loss_fwd_kernel(const View in, const View tg, const int C,
                                                                      const int D, const int H, const int W,
                                                                      const int tiles_x, const int tiles_y,
                                                                      const int flags, const float C1, const float C2,
                                                                      const GaussTaps g, float* __restrict__ fields,
                                                                      double* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float sP[kRows * kPitch];
  __shared__ __attribute__((aligned(16))) float sT[kRows * kPitch];
  __shared__ __attribute__((aligned(16))) float sF[5][kRows * kTile];
  __shared__ double sRed[kThreads / 64][kSlots];

  int x0, y0, n, ch, d;
  int64_t img;
  locate(tiles_x, tiles_y, C, D, x0, y0, n, ch, d, img);
  const float* p0 = in.p + n * in.n + ch * in.c + d * in.d;
  const float* t0 = tg.p + n * tg.n + ch * tg.c + d * tg.d;

  double s_abs = 0.0, s_sq = 0.0, s_ssim = 0.0, s_sob = 0.0;

  // stage both tiles with their halo at clamped coordinates (replicate padding)
  for (int i = threadIdx.x; i < kRows * kPitch; i += kThreads) {
    const int r = i / kPitch, c = i - r * kPitch;
    const int y = y0 - kHalo + r, x = x0 - kHalo + c;
    float p = 0.f, t = 0.f;
    if (c < kRows) {
      const int yc = clampi(y, H - 1), xc = clampi(x, W - 1);
      p = p0[yc * in.h + xc * in.w];
      t = t0[yc * tg.h + xc * tg.w];
      if (r >= kHalo && r < kHalo + kTile && c >= kHalo && c < kHalo + kTile && y < H && x < W) {   // the tile's own
        const float e = p - t;
        if (flags & kL1) s_abs += (double)fabsf(e);
        if (flags & kL2) s_sq += (double)(e * e);
      }
    }
    sP[i] = p;
    sT[i] = t;
  }
  __syncthreads();

  if (flags & kSobel) {
    const int c = threadIdx.x & 31, r0 = (threadIdx.x >> 5) * 4;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      if (y0 + r0 + o < H && x0 + c < W) {
        const int i = (r0 + o + kHalo) * kPitch + c + kHalo;
        float gx, gy;
        const float gp = sobel(sP, kPitch, i, gx, gy);
        const float gt = sobel(sT, kPitch, i, gx, gy);
        s_sob += (double)fabsf(gp - gt);
      }
    }
  }

  if (flags & kSsim) {
    // the window moments of x, y, x^2, y^2, xy: horizontal pass, barrier, vertical pass (ssim_tile.h)
    ssim_hpass_pair(g, sP, sT, sF);
    __syncthreads();

    float m[5][4];
    ssim_vpass<5>(g, sF, m);
    const int x = x0 + ssim_column();
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int y = y0 + ssim_row0() + o;
      ssim_if_valid(y, x, H, W, [&] {
        const float mx = m[0][o], my = m[1][o];
        const SsimIndex ix = ssim_index(mx, my, m[2][o], m[3][o], m[4][o], C1, C2);
        const float A1 = ix.A1, A2 = ix.A2, B1 = ix.B1, B2 = ix.B2, S = ix.S;
        s_ssim += (double)S;
        if (fields != nullptr) {
          const float inv = 1.f / (B1 * B2);
          float* f = fields + ((img * 3) * H + y) * (int64_t)W + x;
          const int64_t plane = (int64_t)H * W;
          f[0] = (2.f * my) * (A2 - A1) * inv - (2.f * mx) * S * (1.f / B1 - 1.f / B2);
          f[plane] = -S / B2;
          f[2 * plane] = (2.f * A1) * inv;
        }
      });
    }
  }

  double v[kSlots] = {s_abs, s_sq, s_ssim, s_sob};
  block_sums(v, sRed, ws + (int64_t)blockIdx.x * kSlots);
}

// one block per sample: the slots of its `per` tiles in a fixed order
__global__ __launch_bounds__(kThreads) void structure_loss_finish_kernel(const double* __restrict__ ws, const int per,
                                                                         double* __restrict__ stats) {
  __shared__ double sRed[kThreads / 64][kSlots];
  block_sums_of_tiles(ws + (int64_t)blockIdx.x * per * kSlots, per, sRed, stats + (int64_t)blockIdx.x * kSlots);
}

// the weighted loss from the samples' sums, in sample order
__global__ void structure_loss_value_kernel(const double* __restrict__ stats, const int N, const int flags,
                                            const double k_l1, const double k_l2, const double w_ssim, const double M,
                                            const double k_sobel, float* __restrict__ loss) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s[kSlots] = {0.0, 0.0, 0.0, 0.0};
  for (int n = 0; n < N; ++n) {
#pragma unroll
    for (int k = 0; k < kSlots; ++k) s[k] += stats[n * kSlots + k];
  }
  double l = 0.0;
  if (flags & kL1) l += k_l1 * s[0];
  if (flags & kL2) l += k_l2 * s[1];
  if (flags & kSsim) l += w_ssim * (1.0 - s[2] / M);
  if (flags & kSobel) l += k_sobel * s[3];
  *loss = (float)l;
}

// the coefficients with which the position v + o (o = -1, 0, 1) of an axis of n samples reaches v through the taps
// k[-1..1] of a 3-tap correlation under replicate padding: smoothing taps (1, 2, 1) -> rs, difference taps (-1, 0, 1) -> rd
__device__ __forceinline__ void adjoint_taps(const int v, const int n, float (&rs)[3], float (&rd)[3]) {
#pragma unroll
  for (int o = -1; o <= 1; ++o) {
    const int q = v + o;
    float a = 0.f, b = 0.f;
    if (q >= 0 && q < n) {
#pragma unroll
      for (int t = -1; t <= 1; ++t) {
        if (clampi(q + t, n - 1) == v) {
          a += t == 0 ? 2.f : 1.f;
          b += (float)t;
        }
      }
    }
    rs[o + 1] = a;
    rd[o + 1] = b;
  }
}

__global__ __launch_bounds__(kThreads) void structure_loss_bwd_kernel(const View in, const View tg, const View out,
                                                                      const int C, const int D, const int H, const int W,
                                                                      const int tiles_x, const int tiles_y,
                                                                      const int flags, const float k_l1, const float k_l2,
                                                                      const float k_ssim, const float k_sobel,
                                                                      const GaussTaps g,
                                                                      const float* __restrict__ fields,
                                                                      const float* __restrict__ grad_out) {
  __shared__ __attribute__((aligned(16))) float sA[3][kRows * kPitch];
  __shared__ __attribute__((aligned(16))) float sH[3][kRows * kTile];
  __shared__ float sP[kImg * kImgPitch];
  __shared__ float sT[kImg * kImgPitch];
  __shared__ float sU[2][kU * kUPitch];

  int x0, y0, n, ch, d;
  int64_t img;
  locate(tiles_x, tiles_y, C, D, x0, y0, n, ch, d, img);
  const float* p0 = in.p + n * in.n + ch * in.c + d * in.d;
  const float* t0 = tg.p + n * tg.n + ch * tg.c + d * tg.d;
  float* o0 = out.p + n * out.n + ch * out.c + d * out.d;

  // both images with a 2-pixel halo at clamped coordinates
  for (int i = threadIdx.x; i < kImg * kImg; i += kThreads) {
    const int r = i / kImg, c = i - r * kImg;
    const int yc = clampi(y0 - 2 + r, H - 1), xc = clampi(x0 - 2 + c, W - 1);
    sP[r * kImgPitch + c] = p0[yc * in.h + xc * in.w];
    sT[r * kImgPitch + c] = t0[yc * tg.h + xc * tg.w];
  }
  if (flags & kSsim) {   // the three coefficient fields with a 5-pixel halo, zero outside the valid positions
    const int64_t plane = (int64_t)H * W;
    for (int i = threadIdx.x; i < 3 * kRows * kPitch; i += kThreads) {
      const int k = i / (kRows * kPitch), j = i - k * (kRows * kPitch);
      const int r = j / kPitch, c = j - r * kPitch;
      const int y = y0 - kHalo + r, x = x0 - kHalo + c;
      float v = 0.f;
      if (c < kRows) ssim_if_valid(y, x, H, W, [&] { v = fields[(img * 3 + k) * plane + (int64_t)y * W + x]; });
      sA[k][j] = v;
    }
  }
  __syncthreads();

  if (flags & kSobel) {   // u = sign(G(p) - G(t)) (gx, gy) / G(p) on the tile and one pixel around it; 0 outside the slice
    for (int i = threadIdx.x; i < kU * kU; i += kThreads) {
      const int r = i / kU, c = i - r * kU;
      const int y = y0 - 1 + r, x = x0 - 1 + c;
      float ux = 0.f, uy = 0.f;
      if (y >= 0 && y < H && x >= 0 && x < W) {
        const int j = (r + 1) * kImgPitch + c + 1;
        float gx, gy, tx, ty;
        const float gp = sobel(sP, kImgPitch, j, gx, gy);
        const float gt = sobel(sT, kImgPitch, j, tx, ty);
        const float e = gp - gt;
        const float s = e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);
        ux = s * gx / gp;
        uy = s * gy / gp;
      }
      sU[0][r * kUPitch + c] = ux;
      sU[1][r * kUPitch + c] = uy;
    }
  }
  if (flags & kSsim) {   // horizontal pass over the three fields, the forward's
    ssim_hpass_plain<3>(g, sA, sH);
  }
  __syncthreads();

  const int c = ssim_column(), r0 = ssim_row0();
  const int x = x0 + c;
  float m[3][4];
  if (flags & kSsim) ssim_vpass<3>(g, sH, m);
  const float go = *grad_out;
  float xs_[3], xd_[3];
  if (flags & kSobel) adjoint_taps(x, W, xs_, xd_);
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int y = y0 + r0 + o;
    if (y >= H || x >= W) continue;
    const float p = sP[(r0 + o + 2) * kImgPitch + c + 2], t = sT[(r0 + o + 2) * kImgPitch + c + 2];
    const float e = p - t;
    float gr = 0.f;
    if (flags & kL1) gr += k_l1 * (e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f));
    if (flags & kL2) gr += k_l2 * e;
    if (flags & kSsim) gr += k_ssim * ((m[0][o] + (2.f * p) * m[1][o]) + t * m[2][o]);
    if (flags & kSobel) {
      float ys_[3], yd_[3];
      adjoint_taps(y, H, ys_, yd_);
      float acc = 0.f;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const int j = (r0 + o + a) * kUPitch + c + b;   // the neighbour (y + a - 1, x + b - 1) in u coordinates
          acc += sU[0][j] * (ys_[a] * xd_[b]) + sU[1][j] * (yd_[a] * xs_[b]);
        }
      }
      gr += k_sobel * (acc * 0.125f);
    }
    o0[y * out.h + x * out.w] = go * gr;
  }
}

// the terms with a weight other than 0; < 0: a weight that is no finite number
int term_flags(float l1, float l2, float ssim, float sobel) {
  if (!isfinite(l1) || !isfinite(l2) || !isfinite(ssim) || !isfinite(sobel)) return -1;
  return (l1 != 0.f ? kL1 : 0) | (l2 != 0.f ? kL2 : 0) | (ssim != 0.f ? kSsim : 0) | (sobel != 0.f ? kSobel : 0);
}

int view(const float* p, const int64_t* s, View* v) {
  if (p == nullptr || s == nullptr) return REHR_EINVAL;
  for (int a = 0; a < 5; ++a)
    if (s[a] < 0) return REHR_EINVAL;
  *v = View{const_cast<float*>(p), s[0], s[1], s[2], s[3], s[4]};
  return REHR_OK;
}

}  // namespace

extern "C" int64_t rehr_structure_loss_workspace_bytes(int32_t N, int32_t C, int32_t D, int32_t H, int32_t W) {
  Geometry g;
  const int rc = tile_geometry(N, C, D, H, W, false, &g);
  return rc != REHR_OK ? rc : tile_sums_layout<kSlots>(nullptr, g).bytes;
}

extern "C" int rehr_structure_loss_fwd_f32(const float* input, const int64_t* input_strides, const float* target,
                                           const int64_t* target_strides, int32_t N, int32_t C, int32_t D, int32_t H,
                                           int32_t W, float l1, float l2, float ssim, float sobel, float data_range,
                                           double* stats, float* loss, float* fields, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
  View in, tg;
  if (view(input, input_strides, &in) != REHR_OK || view(target, target_strides, &tg) != REHR_OK) return REHR_EINVAL;
  if (stats == nullptr || loss == nullptr || workspace == nullptr) return REHR_EINVAL;
  if (!(data_range > 0.f) || !isfinite(data_range)) return REHR_EINVAL;
  const int flags = term_flags(l1, l2, ssim, sobel);
  if (flags < 0) return REHR_EINVAL;
  Geometry g;
  const int rc = tile_geometry(N, C, D, H, W, (flags & kSsim) != 0, &g);
  if (rc != REHR_OK) return rc;
  const auto [slots, need] = tile_sums_layout<kSlots>(workspace, g);
  if (workspace_bytes < need || misaligned(8, workspace, stats) || misaligned(4, loss, fields)) return REHR_EINVAL;
  const double V = (double)N * C * D * H * W;
  const double M = (double)N * C * D * ((double)H - 10.0) * ((double)W - 10.0);
  const float c1 = 0.01f * data_range, c2 = 0.03f * data_range;
  hipLaunchKernelGGL(structure_loss_fwd_kernel, dim3((unsigned)g.blocks), dim3(kThreads), 0, (hipStream_t)stream, in, tg,
                     C, D, H, W, g.tiles_x, g.tiles_y, flags, c1 * c1, c2 * c2, gauss_taps(),
                     (flags & kSsim) ? fields : nullptr, slots);
  hipLaunchKernelGGL(structure_loss_finish_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream,
                     (const double*)slots, (int)g.per, stats);
  hipLaunchKernelGGL(structure_loss_value_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)stats, N,
                     flags, (double)l1 / V, (double)l2 / V, (double)ssim, M, (double)sobel / V, loss);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_structure_loss_bwd_f32(const float* input, const int64_t* input_strides, const float* target,
                                           const int64_t* target_strides, int32_t N, int32_t C, int32_t D, int32_t H,
                                           int32_t W, float l1, float l2, float ssim, float sobel, const float* fields,
                                           const float* grad_output, float* dinput, const int64_t* dinput_strides,
                                           void* stream) {
  View in, tg, out;
  if (view(input, input_strides, &in) != REHR_OK || view(target, target_strides, &tg) != REHR_OK ||
      view(dinput, dinput_strides, &out) != REHR_OK)
    return REHR_EINVAL;
  if (grad_output == nullptr) return REHR_EINVAL;
  const int flags = term_flags(l1, l2, ssim, sobel);
  if (flags < 0) return REHR_EINVAL;
  Geometry g;
  const int rc = tile_geometry(N, C, D, H, W, (flags & kSsim) != 0, &g);
  if (rc != REHR_OK) return rc;
  if ((flags & kSsim) && fields == nullptr) return REHR_EINVAL;
  if (misaligned(4, fields, grad_output)) return REHR_EINVAL;
  // every pixel of d input is written by one thread: its strides must address N * C * D * H * W distinct elements
  const int64_t ext[5] = {N, C, D, H, W};
  for (int a = 0; a < 5; ++a)
    if (ext[a] > 1 && dinput_strides[a] == 0) return REHR_EINVAL;
  const double V = (double)N * C * D * H * W;
  const double M = (double)N * C * D * ((double)H - 10.0) * ((double)W - 10.0);
  hipLaunchKernelGGL(structure_loss_bwd_kernel, dim3((unsigned)g.blocks), dim3(kThreads), 0, (hipStream_t)stream, in, tg,
                     out, C, D, H, W, g.tiles_x, g.tiles_y, flags, (float)((double)l1 / V), (float)(2.0 * (double)l2 / V),
                     (flags & kSsim) ? (float)(-(double)ssim / M) : 0.f, (float)((double)sobel / V), gauss_taps(), fields,
                     grad_output);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}
