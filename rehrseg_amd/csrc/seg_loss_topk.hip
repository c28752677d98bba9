// Top-k cross-entropy + soft Dice (nnU-Net's DC_and_topk_loss / TopKLoss, k percent of the voxels).
//
//   m         = the per-voxel loss map of RobustCrossEntropyLoss before its mean: ce[b][v], or with an uncertainty
//               the reference's broadcast product m[a][b][v] = ce[b][v] * u[a][v]; M elements
//   CE term   = mean of the K = int(M k / 100) largest elements of m
//   t = the K-th largest value, n_gt = #{m > t}, n_eq = #{m == t}:
//     value   = (sum_{m > t} m + (K - n_gt) t) / K               (torch.topk's value under any tie-break)
//     d/dm    = 1 / K above t, (K - n_gt) / n_eq / K on t, 0 below (deterministic, no scan)
//
// Forward: the pass of seg_loss.hip over the logits (seg_loss_fwd_body, which also leaves the Dice statistics and
// the plain CE sum) writes m into the workspace; rehr_order_stats_f32 (intensity_norm.hip: exact radix select, nine
// launches, nothing read back) picks rank M - K; one pass over m counts n_gt and n_eq and sums what lies above t.
// Backward: the pass of seg_loss.hip with the CE coefficient of every voxel taken from m and the threshold.
// Zeros enter m as +0 (a saturated fp32 CE is exactly 0, times a negative uncertainty -0): the select orders bit
// patterns, the counts compare values, and both must see one value.
#include "seg_loss_body.h"
#include "host_util.h"

namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxM = (int64_t)1 << 30;   // rehr_order_stats_f32's limit
constexpr int kTk = 4;                        // {n_gt, n_eq, sum above, t} behind the Dice statistics and the CE sum

template <int C>
__global__ __launch_bounds__(kThreads) void seg_topk_fwd_kernel(const float* __restrict__ logits, int ld,
                                                                const float* __restrict__ target,
                                                                const float* __restrict__ unc, int N, int64_t S,
                                                                double* __restrict__ stats, float* __restrict__ map) {
  seg_loss_fwd_body<C, true>(logits, ld, target, unc, N, S, stats, blockIdx.x, gridDim.x, 0, map);
}

// tk[0..2] += {#(m > t), #(m == t), sum of m > t}, tk[3] = t.  The map is a workspace segment, so it starts on a
// multiple of 16 bytes: 16-byte loads and a scalar tail of at most 3 elements.  The counts are integers below 2^30
// carried in doubles: their atomic sums are exact, the same bits on every run.
__global__ __launch_bounds__(kThreads) void seg_topk_count_kernel(const float* __restrict__ map, const int64_t M,
                                                                  const float* __restrict__ tsel,
                                                                  double* __restrict__ tk) {
  const float t = tsel[0];
  uint32_t ngt = 0, neq = 0;
  double sum = 0.0;
  const int64_t nvec = M / 4, step = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < nvec; i += step) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(map + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool gt = v[e] > t;
      ngt += gt ? 1u : 0u;
      neq += v[e] == t ? 1u : 0u;
      sum += gt ? (double)v[e] : 0.0;
    }
  }
  if (blockIdx.x == 0 && nvec * 4 + threadIdx.x < M) {
    const float m = map[nvec * 4 + threadIdx.x];
    const bool gt = m > t;
    ngt += gt ? 1u : 0u;
    neq += m == t ? 1u : 0u;
    sum += gt ? (double)m : 0.0;
  }
  __shared__ double red[4][3];
  double v[3] = {(double)wave_sum(ngt), (double)wave_sum(neq), sum};
  v[2] = wave_sum_d(v[2]);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    red[w][0] = v[0];
    red[w][1] = v[1];
    red[w][2] = v[2];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const double s = wave_order_sum(red, threadIdx.x);
    if (s != 0.0) atomicAdd(tk + threadIdx.x, s);
  }
  if (blockIdx.x == 0 && threadIdx.x == 3) tk[3] = (double)t;
}

template <int C>
__global__ __launch_bounds__(kThreads) void seg_topk_bwd_kernel(const float* __restrict__ logits, int ld,
                                                                const float* __restrict__ target,
                                                                const float* __restrict__ unc, int N, int64_t S,
                                                                const double* __restrict__ stats, float w_ce,
                                                                float w_dice, float smooth, int do_bg,
                                                                const float* __restrict__ grad_out,
                                                                float* __restrict__ dlogits, int ldd,
                                                                const float* __restrict__ map, double K) {
  seg_loss_bwd_body<C, true>(logits, ld, target, unc, N, S, stats, w_ce, w_dice, smooth, do_bg, grad_out[0], dlogits,
                             ldd, blockIdx.x, gridDim.x, 0, map, stats + N * C * 3 + 1, K);
}

// ENOSUP outside what the kernels cover, else M = the elements of the selection map
int64_t map_elements(int32_t N, int32_t C, int64_t S, bool with_unc) {
  if (N < 1 || S < 1) return REHR_EINVAL;
  if (C < 2 || C > 4 || N > SL_MAXN || S > kMaxM) return REHR_ENOSUP;
  const int64_t M = (with_unc ? (int64_t)N * N : (int64_t)N) * S;
  return M > kMaxM ? REHR_ENOSUP : M;
}

// workspace: [map: M floats][the selected threshold: one float][rehr_order_stats_f32's workspace for one rank]
struct Layout {
  float *map, *tsel;
  char* select;
  int64_t select_bytes, bytes;
};
Layout layout(void* base, int64_t M) {
  Carver c(base);   // a braced list is evaluated left to right
  const int64_t sel = rehr_order_stats_workspace_bytes(1, 1);
  return {c.take<float>(M), c.take<float>(1), c.take<char>(sel), sel, c.bytes()};
}

}  // namespace

extern "C" int64_t rehr_seg_topk_workspace_bytes(int32_t N, int32_t C, int64_t S, int32_t with_unc) {
  const int64_t M = map_elements(N, C, S, with_unc != 0);
  if (M < 0) return M;
  return layout(nullptr, M).bytes;
}

extern "C" int rehr_seg_topk_fwd_f32(const float* logits, int32_t ld, const float* target, const float* unc,
                                     int32_t N, int32_t C, int64_t S, int64_t K, double* stats, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
  if (!logits || !target || !stats || !workspace) return REHR_EINVAL;
  const int64_t M = map_elements(N, C, S, unc != nullptr);
  if (M < 0) return (int)M;
  if (K < 1 || K > M || ld < C) return REHR_EINVAL;
  const Layout L = layout(workspace, M);
  if (workspace_bytes < L.bytes || misaligned(16, workspace) || misaligned(4, logits, target, unc) ||
      misaligned(8, stats))
    return REHR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(stats, 0, sizeof(double) * ((size_t)N * C * 3 + 1 + kTk), st) != hipSuccess) return REHR_EHIP;
  const dim3 g(sl_grid_for(S)), t(kThreads);
  if (C == 2) hipLaunchKernelGGL(seg_topk_fwd_kernel<2>, g, t, 0, st, logits, ld, target, unc, N, S, stats, L.map);
  else if (C == 3) hipLaunchKernelGGL(seg_topk_fwd_kernel<3>, g, t, 0, st, logits, ld, target, unc, N, S, stats, L.map);
  else hipLaunchKernelGGL(seg_topk_fwd_kernel<4>, g, t, 0, st, logits, ld, target, unc, N, S, stats, L.map);
  REHR_LAUNCH_CHECK();
  const int64_t rank = M - K;   // ascending
  const int rc = rehr_order_stats_f32(L.map, 1, M, M, &rank, 1, L.tsel, L.select, L.select_bytes, stream);
  if (rc != REHR_OK) return rc;
  hipLaunchKernelGGL(seg_topk_count_kernel, dim3(grid_for(M / 4, kThreads * 4, 2048)), t, 0, st,
                     (const float*)L.map, M, (const float*)L.tsel, stats + (size_t)N * C * 3 + 1);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_seg_topk_bwd_f32(const float* logits, int32_t ld, const float* target, const float* unc,
                                     int32_t N, int32_t C, int64_t S, int64_t K, const double* stats,
                                     const void* workspace, int64_t workspace_bytes, float w_ce, float w_dice,
                                     float smooth, int32_t do_bg, const float* grad_out, float* dlogits, int32_t ldd,
                                     void* stream) {
  if (!logits || !target || !stats || !workspace || !grad_out || !dlogits) return REHR_EINVAL;
  const int64_t M = map_elements(N, C, S, unc != nullptr);
  if (M < 0) return (int)M;
  if (K < 1 || K > M || ld < C || ldd < C) return REHR_EINVAL;
  const Layout L = layout(const_cast<void*>(workspace), M);
  if (workspace_bytes < L.bytes || misaligned(16, workspace) || misaligned(4, logits, target, unc, grad_out, dlogits) ||
      misaligned(8, stats))
    return REHR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 g(sl_grid_for(S)), t(kThreads);
#define TK_BWD(C_)                                                                                             \
  hipLaunchKernelGGL(seg_topk_bwd_kernel<C_>, g, t, 0, st, logits, ld, target, unc, N, S, stats, w_ce, w_dice, \
                     smooth, do_bg, grad_out, dlogits, ldd, (const float*)L.map, (double)K)
  if (C == 2) TK_BWD(2);
  else if (C == 3) TK_BWD(3);
  else TK_BWD(4);
#undef TK_BWD
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}
