// Deep supervision of the stage-2 segmentation network (nnU-Net's DeepSupervisionWrapper over DC_and_weighted_CE_loss,
// utils/seg_utils.py:363-371, and DownsampleSegForDSTransform2 in front of it, :723-725).
//
// The network returns one logits tensor per decoder stage; the coarse ones together hold about a third of the
// voxels of the finest, so a launch (and a memset) per level costs more in launches than in bytes.  Here every level
// of one pass is served by ONE launch: the blocks of the grid are dealt out to the levels by a prefix table in the
// kernel arguments, and a block then runs the single-level body of seg_loss_body.h on its level, with the block
// count the single-level entry point would have given that level.  The label pyramid is built the same way: one
// launch gathers every level of the order-0 resize through per-axis index tables.
#include "seg_loss_body.h"

namespace {

struct DsLevelK {
  const float* logits;
  const float* target;
  const float* unc;
  float* dlogits;
  int64_t S;
  int ld, ldd;
  float weight;
  int blk0, nblk;  // this level's blocks are [blk0, blk0 + nblk) of grid.x; nblk == 0: skipped
};
struct DsArgs {
  DsLevelK lv[REHR_DS_MAX_LEVELS];
  int n;
};

struct PyrLevelK {
  float* dst;
  const int32_t *iz, *iy, *ix;
  int d, h, w;
  int blk0, nblk;
};
struct PyrArgs {
  PyrLevelK lv[REHR_DS_MAX_LEVELS];
  int n;
};

// the level that owns block bx (wave-uniform: every block belongs to exactly one level)
template <typename A>
__device__ __forceinline__ int level_of(const A& a, int bx) {
  int l = 0;
  for (int k = 1; k < a.n; ++k)
    if (bx >= a.lv[k].blk0 && bx < a.lv[k].blk0 + a.lv[k].nblk) l = k;
  return l;
}

template <int C>
__global__ __launch_bounds__(256) void seg_loss_ds_fwd_kernel(const DsArgs a, int N, double* __restrict__ stats) {
  const DsLevelK& L = a.lv[level_of(a, blockIdx.x)];
  seg_loss_fwd_body<C>(L.logits, L.ld, L.target, L.unc, N, L.S, stats + (size_t)(&L - a.lv) * ((size_t)N * C * 3 + 1),
                       blockIdx.x - L.blk0, L.nblk, blockIdx.y * SL_MAXN);
}

template <int C>
__global__ __launch_bounds__(256) void seg_loss_ds_bwd_kernel(const DsArgs a, int N, const double* __restrict__ stats,
                                                              float w_ce, float w_dice, float smooth, int do_bg,
                                                              const float* __restrict__ grad_out) {
  const DsLevelK& L = a.lv[level_of(a, blockIdx.x)];
  seg_loss_bwd_body<C>(L.logits, L.ld, L.target, L.unc, N, L.S, stats + (size_t)(&L - a.lv) * ((size_t)N * C * 3 + 1),
                       w_ce, w_dice, smooth, do_bg, grad_out[0] * L.weight, L.dlogits, L.ldd, blockIdx.x - L.blk0,
                       L.nblk, blockIdx.y * SL_MAXN);
}

// dst_l[b][k][j][i] = src[b][iz[k]][iy[j]][ix[i]]: consecutive threads write consecutive i (coalesced stores; the loads
// of one wave fall into one or two source rows)
__global__ __launch_bounds__(256) void label_pyramid_kernel(const float* __restrict__ src, int B, int z, int y, int x,
                                                            const PyrArgs a) {
  const PyrLevelK& L = a.lv[level_of(a, blockIdx.x)];
  const int64_t total = (int64_t)B * L.d * L.h * L.w;
  for (int64_t o = (int64_t)(blockIdx.x - L.blk0) * blockDim.x + threadIdx.x; o < total;
       o += (int64_t)L.nblk * blockDim.x) {
    const int i = (int)(o % L.w);
    int64_t t = o / L.w;
    const int j = (int)(t % L.h);
    t /= L.h;
    const int k = (int)(t % L.d);
    const int64_t b = t / L.d;
    L.dst[o] = src[((b * z + L.iz[k]) * y + L.iy[j]) * (int64_t)x + L.ix[i]];
  }
}

// Validates the levels and deals out the blocks; returns the grid's x extent (or a negative REHR_E*).
int plan_ds(const rehr_seg_ds_level* levels, int n_levels, int N, int C, bool bwd, DsArgs& a) {
  if (!levels || n_levels < 1 || n_levels > REHR_DS_MAX_LEVELS || N < 1) return REHR_EINVAL;
  if (C < 2 || C > 4 || N > 65535 * SL_MAXN) return REHR_ENOSUP;
  int blocks = 0;
  a.n = n_levels;
  for (int l = 0; l < n_levels; ++l) {
    const rehr_seg_ds_level& s = levels[l];
    DsLevelK& k = a.lv[l];
    k = DsLevelK{s.logits, s.target, s.unc, s.dlogits, s.S, s.ld, s.ldd, s.weight, blocks, 0};
    if (s.weight == 0.f) continue;
    if (!s.logits || !s.target || (bwd && !s.dlogits) || s.d < 1 || s.h < 1 || s.w < 1 ||
        s.S != (int64_t)s.d * s.h * s.w || s.ld < C || (bwd && s.ldd < C))
      return REHR_EINVAL;
    k.nblk = sl_grid_for(s.S);
    blocks += k.nblk;
  }
  return blocks > 0 ? blocks : REHR_EINVAL;
}

}  // namespace

extern "C" int rehr_seg_loss_ds_fwd_f32(const rehr_seg_ds_level* levels, int32_t n_levels, int32_t N, int32_t C,
                                        double* stats, void* stream) {
  DsArgs a;
  const int blocks = plan_ds(levels, n_levels, N, C, false, a);
  if (blocks < 0) return blocks;
  if (!stats) return REHR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(stats, 0, sizeof(double) * ((size_t)N * C * 3 + 1) * n_levels, st) != hipSuccess) return REHR_EHIP;
  const dim3 g(blocks, (N + SL_MAXN - 1) / SL_MAXN), t(256);
  if (C == 2) hipLaunchKernelGGL(seg_loss_ds_fwd_kernel<2>, g, t, 0, st, a, N, stats);
  else if (C == 3) hipLaunchKernelGGL(seg_loss_ds_fwd_kernel<3>, g, t, 0, st, a, N, stats);
  else hipLaunchKernelGGL(seg_loss_ds_fwd_kernel<4>, g, t, 0, st, a, N, stats);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_seg_loss_ds_bwd_f32(const rehr_seg_ds_level* levels, int32_t n_levels, int32_t N, int32_t C,
                                        const double* stats, float w_ce, float w_dice, float smooth, int32_t do_bg,
                                        const float* grad_out, void* stream) {
  DsArgs a;
  const int blocks = plan_ds(levels, n_levels, N, C, true, a);
  if (blocks < 0) return blocks;
  if (!stats || !grad_out) return REHR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 g(blocks, (N + SL_MAXN - 1) / SL_MAXN), t(256);
#define SL_DS_BWD(C_) \
  hipLaunchKernelGGL(seg_loss_ds_bwd_kernel<C_>, g, t, 0, st, a, N, stats, w_ce, w_dice, smooth, do_bg, grad_out)
  if (C == 2) SL_DS_BWD(2);
  else if (C == 3) SL_DS_BWD(3);
  else SL_DS_BWD(4);
#undef SL_DS_BWD
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_label_pyramid_f32(const float* src, int32_t B, int32_t z, int32_t y, int32_t x,
                                      const rehr_pyramid_level* levels, int32_t n_levels, void* stream) {
  if (!src || !levels || B < 1 || z < 1 || y < 1 || x < 1 || n_levels < 1 || n_levels > REHR_DS_MAX_LEVELS)
    return REHR_EINVAL;
  PyrArgs a;
  a.n = n_levels;
  int blocks = 0;
  for (int l = 0; l < n_levels; ++l) {
    const rehr_pyramid_level& s = levels[l];
    if (!s.dst || !s.iz || !s.iy || !s.ix || s.d < 1 || s.h < 1 || s.w < 1) return REHR_EINVAL;
    const int nblk = sl_grid_for((int64_t)B * s.d * s.h * s.w);
    a.lv[l] = PyrLevelK{s.dst, s.iz, s.iy, s.ix, s.d, s.h, s.w, blocks, nblk};
    blocks += nblk;
  }
  hipLaunchKernelGGL(label_pyramid_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, B, z, y, x, a);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}
