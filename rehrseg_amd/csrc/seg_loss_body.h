// Per-block bodies of the fused segmentation loss (softmax + cross-entropy + soft Dice), shared by the single-level
// kernels of seg_loss.hip and the deep-supervision kernels of seg_loss_ds.hip.  A body is handed its place in the
// level's own grid (block `bx` of `nbx` along the voxels, first sample `b0` of its chunk), so a kernel that serves
// several levels in one launch runs exactly the arithmetic of a launch per level.
#pragma once
#include "common.h"

constexpr int SL_MAXN = 4;

static inline int sl_grid_for(int64_t S) {
  int64_t b = (S + 255) / 256;
  return (int)(b > 2048 ? 2048 : b);
}

template <int C>
__device__ __forceinline__ void softmax_ce(const float* __restrict__ lp, int t, float (&p)[C], float& ce) {
  float l[C];
#pragma unroll
  for (int c = 0; c < C; ++c) l[c] = lp[c];
  float m = l[0];
#pragma unroll
  for (int c = 1; c < C; ++c) m = fmaxf(m, l[c]);
  float s = 0.f, lt = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    p[c] = __expf(l[c] - m);
    s += p[c];
    lt = (c == t) ? l[c] : lt;
  }
  const float inv = 1.f / s;
#pragma unroll
  for (int c = 0; c < C; ++c) p[c] *= inv;
  ce = __logf(s) - (lt - m);
}

// A zero of either sign as +0: the top-k select orders bit patterns, the loss compares values
__device__ __forceinline__ float plus_zero(float v) { return v == 0.f ? 0.f : v; }

// weight of a selection-map element in the top-k mean: 1 above the threshold, the tie weight on it, 0 below
__device__ __forceinline__ float topk_weight(float m, float thr, float wtie) {
  return m > thr ? 1.f : (m == thr ? wtie : 0.f);
}

// stats[N][C][3] = {I, P, G}, stats[N*C*3] = sum_v (sum_b ce)(sum_a u); 256 threads
// MAP (seg_loss_topk.hip): the same pass also writes the per-voxel loss map the reference forms before its mean,
// map[b][v] = ce, or with an uncertainty the broadcast product map[a][b][v] = ce[b][v] * u[a][v]
template <int C, bool MAP = false>
__device__ __forceinline__ void seg_loss_fwd_body(const float* __restrict__ logits, int ld,
                                                  const float* __restrict__ target, const float* __restrict__ unc,
                                                  int N, int64_t S, double* __restrict__ stats, int bx, int nbx, int b0,
                                                  float* __restrict__ map = nullptr) {
  float aI[SL_MAXN][C], aP[SL_MAXN][C], aG[SL_MAXN][C];
#pragma unroll
  for (int b = 0; b < SL_MAXN; ++b)
#pragma unroll
    for (int c = 0; c < C; ++c) aI[b][c] = aP[b][c] = aG[b][c] = 0.f;
  float ace = 0.f;
  // samples are taken SL_MAXN at a time (b0): the cross-sample term sum_v (sum_b ce_b)(sum_a u_a) splits over
  // chunks of b, every chunk pairing its ce with the uncertainty sum over ALL samples
  const int nb = (N - b0 < SL_MAXN) ? N - b0 : SL_MAXN;
  for (int64_t v = (int64_t)bx * blockDim.x + threadIdx.x; v < S; v += (int64_t)nbx * blockDim.x) {
    float sce = 0.f, su = 0.f;
    if (unc != nullptr)
      for (int a = 0; a < N; ++a) su += unc[(int64_t)a * S + v];
#pragma unroll
    for (int b = 0; b < SL_MAXN; ++b) {
      if (b < nb) {
        const int64_t i = (int64_t)(b0 + b) * S + v;
        const int t = (int)target[i];
        float p[C], ce;
        softmax_ce<C>(logits + i * ld, t, p, ce);
        sce += ce;
        if constexpr (MAP) {
          if (unc == nullptr) {
            map[i] = plus_zero(ce);
          } else {
            for (int a = 0; a < N; ++a)
              map[((int64_t)a * N + (b0 + b)) * S + v] = plus_zero(ce * unc[(int64_t)a * S + v]);
          }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float y = (c == t) ? 1.f : 0.f;
          aI[b][c] += p[c] * y;
          aP[b][c] += p[c];
          aG[b][c] += y;
        }
      }
    }
    ace += (unc != nullptr) ? sce * su : sce;
  }
  // block reduction, then one double atomic per statistic and block
  __shared__ float red[4][SL_MAXN * C * 3 + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int b = 0; b < SL_MAXN; ++b)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float i_ = wave_sum(aI[b][c]), p_ = wave_sum(aP[b][c]), g_ = wave_sum(aG[b][c]);
      if (lane == 0) {
        red[w][(b * C + c) * 3 + 0] = i_;
        red[w][(b * C + c) * 3 + 1] = p_;
        red[w][(b * C + c) * 3 + 2] = g_;
      }
    }
  const float ce_ = wave_sum(ace);
  if (lane == 0) red[w][SL_MAXN * C * 3] = ce_;
  __syncthreads();
  const int nstat = nb * C * 3;
  for (int k = threadIdx.x; k <= nstat; k += blockDim.x) {
    const int src = (k == nstat) ? SL_MAXN * C * 3 : k;
    const float s = red[0][src] + red[1][src] + red[2][src] + red[3][src];
    atomicAdd(stats + ((k == nstat) ? N * C * 3 : b0 * C * 3 + k), (double)s);
  }
}

// dlogits[N][S][ldd] = go * d(loss)/d(logits); 256 threads
// TOPK (seg_loss_topk.hip): the CE term is the top-k mean over the forward's map; w_ce arrives divided by K, and
// tk = {n_gt, n_eq, sum above, threshold} of the forward, from which every block forms the tie weight
// (K - n_gt) / n_eq.  d(loss)/d(ce[b][v]) = w_ce / K * sum_a weight(map[a][b][v]) * u[a][v].
template <int C, bool TOPK = false>
__device__ __forceinline__ void seg_loss_bwd_body(const float* __restrict__ logits, int ld,
                                                  const float* __restrict__ target, const float* __restrict__ unc,
                                                  int N, int64_t S, const double* __restrict__ stats, float w_ce,
                                                  float w_dice, float smooth, int do_bg, float go,
                                                  float* __restrict__ dlogits, int ldd, int bx, int nbx, int b0,
                                                  const float* __restrict__ map = nullptr,
                                                  const double* __restrict__ tk = nullptr, double K = 0.0) {
  // per (sample, class) Dice constants: d(-dc)/dp = -(2 y den - num) / den^2 = y*A + B
  __shared__ float cA[SL_MAXN * C], cB[SL_MAXN * C];
  const int nb = (N - b0 < SL_MAXN) ? N - b0 : SL_MAXN;
  if (threadIdx.x < nb * C) {
    const int c = threadIdx.x % C;
    const double* sp = stats + (size_t)(b0 * C + threadIdx.x) * 3;
    const double I = sp[0], P = sp[1], G = sp[2];
    const double num = 2.0 * I + smooth;
    const double raw = G + P + smooth;
    const double den = raw < 1e-8 ? 1e-8 : raw;
    const int ncls = do_bg ? C : C - 1;
    const double k = (double)w_dice / ((double)N * ncls);
    const bool on = do_bg || c > 0;
    // clipped denominator: its derivative vanishes, only the numerator's 2*y term remains
    cA[threadIdx.x] = on ? (float)(-k * 2.0 / den) : 0.f;
    cB[threadIdx.x] = (on && raw >= 1e-8) ? (float)(k * num / (den * den)) : 0.f;
  }
  __syncthreads();
  const float kce = TOPK ? (float)((double)w_ce / K)
                         : w_ce / ((unc != nullptr) ? (float)((double)N * N * S) : (float)((double)N * S));
  float thr = 0.f, wtie = 0.f;
  if constexpr (TOPK) {
    thr = (float)tk[3];
    wtie = tk[1] > 0.0 ? (float)((K - tk[0]) / tk[1]) : 0.f;
  }
  for (int64_t v = (int64_t)bx * blockDim.x + threadIdx.x; v < S; v += (int64_t)nbx * blockDim.x) {
    float su = 1.f;
    if (!TOPK && unc != nullptr) {
      su = 0.f;
      for (int a = 0; a < N; ++a) su += unc[(int64_t)a * S + v];
    }
    float cw = kce * su;
#pragma unroll
    for (int b = 0; b < SL_MAXN; ++b) {
      if (b < nb) {
        const int64_t i = (int64_t)(b0 + b) * S + v;
        const int t = (int)target[i];
        float p[C], ce;
        softmax_ce<C>(logits + i * ld, t, p, ce);
        if constexpr (TOPK) {
          if (unc == nullptr) {
            cw = kce * topk_weight(map[i], thr, wtie);
          } else {
            float acc = 0.f;
            for (int a = 0; a < N; ++a)
              acc += topk_weight(map[((int64_t)a * N + (b0 + b)) * S + v], thr, wtie) * unc[(int64_t)a * S + v];
            cw = kce * acc;
          }
        }
        float g[C], dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float y = (c == t) ? 1.f : 0.f;
          g[c] = y * cA[b * C + c] + cB[b * C + c];
          dot += g[c] * p[c];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float y = (c == t) ? 1.f : 0.f;
          dlogits[i * ldd + c] = go * (cw * (p[c] - y) + p[c] * (g[c] - dot));
        }
      }
    }
  }
}
