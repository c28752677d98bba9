// Host code shared by every kernel file that consumes rehr_gather_gemm_desc (gather_gemm.hip, gather_gemm_bf16.hip,
// halo_conv*.hip, wino*_conv.hip): validation, planning, the range checks of the buffer-addressed operands and the
// single / multi-phase launcher of the generic kernels, written once and parameterised by the element size `es`
// (4 = fp32, 2 = bf16).  A wrong range check here is an out-of-bounds access on the device: fix it in this file only.
#pragma once
#include "common.h"
#include "taps.h"   // span(), three_taps(), BUF_LIMIT

// ---- plan of one launch / of the phases that share one grid (kernel arguments: the layout is part of the kernels) ----
struct GGParams {
  rehr_gather_gemm_desc d;
  int tiles_d, tiles_h, tiles_w, m_tiles, n_tiles;
  int kchunks;  // K steps per tap: Cin / chunk width, rounded up
  int64_t wp_bytes;
};

constexpr int MAX_PHASES = 8;
// Several launches that differ only in lattice / taps / destination offset (the stride phases of one transposed conv or
// strided input gradient) share ONE grid: blockIdx.z picks the phase, so four quarter-size launches fill the chip like
// one full-size launch.
// interleave != 0 (REHR_DBG_GG_INTERLEAVE; all phases have the same tile counts -- kernel = stride transposed
// convolutions, input gradients of strided convolutions on even extents): a 1-D grid in which the `count` phases of one
// lattice tile are CONSECUTIVE blocks of ONE XCD, so that the tile's source rows come from HBM once and from that XCD's L2
// for the other phases (with blockIdx.z = phase the source tensor is streamed once per phase).  Tried in round 3 and
// measured SLOWER in the step (cfg-3 +1.4 ms, cfg-5 +0.25 ms, profiles/r03_ab_phase_interleave.txt): these launches are
// bound by block turnover (K = C_in only: two k-steps per block), not by the source re-reads, and eight blocks storing
// into the same 2x2x2 output neighbourhood at once serialise at the memory side.  Off by default; tests keep it alive.
struct GGMulti {
  GGParams ph[MAX_PHASES];
  int interleave, count, no_interleave;
};

// block b of the interleaved grid -> (phase, logical tile); false: padding block
__device__ __forceinline__ bool interleaved_block(int b, int m_tiles, int n_tiles, int count, int& phase, int& logical) {
  const int xcd = b & 7, j = b >> 3, per = count * n_tiles;
  const int mt = (j / per) * 8 + xcd, rem = j % per;
  phase = rem / n_tiles;
  logical = mt * n_tiles + (rem - phase * n_tiles);
  return mt < m_tiles;
}

// ---- range checks: raw buffer loads take 32-bit byte offsets (the limit itself: taps.h) ----
constexpr int64_t GG_BUF_LIMIT = BUF_LIMIT;

// bytes of the weight panel wp[tap][Npad][Cin] up to the last tap the descriptor can reach
inline int64_t gg_wp_bytes(const rehr_gather_gemm_desc& d, int es) {
  const int64_t kd_max = d.td.k0 + (int64_t)d.td.ks * (d.td.count - 1);
  const int64_t kh_max = d.th.k0 + (int64_t)d.th.ks * (d.th.count - 1);
  const int64_t kw_max = d.tw.k0 + (int64_t)d.tw.ks * (d.tw.count - 1);
  return (((kd_max * d.KH) + kh_max) * d.KW + kw_max + 1) * d.Npad * d.Cin * es;
}

// do `vox` voxels of x1 (and of x2, when given) fit one buffer?  vox: one sample for the kernels that make a buffer per
// sample, the whole batch for the flattened-tile planners
inline bool gg_src_fits(const rehr_gather_gemm_desc& d, int64_t vox, int es) {
  const int64_t b = vox * es;
  return b * d.ldx1 < GG_BUF_LIMIT && (!d.x2 || b * d.ldx2 < GG_BUF_LIMIT);
}

// ---- validation: everything a kernel of the family relies on without checking it again ----
inline int gg_validate(const rehr_gather_gemm_desc& d, int es) {
  const int row = 16 / es;  // channels of one 16-byte load: every source row is a whole number of them
  if (!d.x1 || !d.wp || !d.y) return REHR_EINVAL;
  if (d.N < 1 || d.Cin < 16 || d.Cin % 16 || d.c1 < 1 || d.c1 > d.Cin) return REHR_EINVAL;
  if (d.c1 < d.Cin && (d.c1 % 32 || !d.x2)) return REHR_EINVAL;  // a virtual concat splits on a chunk boundary
  if (d.ldx1 % row || (d.x2 && d.ldx2 % row)) return REHR_EINVAL;
  if (((uintptr_t)d.x1 | (uintptr_t)d.wp | (uintptr_t)(d.x2 ? d.x2 : d.x1)) & 15) return REHR_EINVAL;
  if (d.Npad % 32 || d.Npad < d.Cout || d.Cout < 1) return REHR_EINVAL;
  if (d.Ld < 1 || d.Lh < 1 || d.Lw < 1) return REHR_EINVAL;
  if (d.td.count < 1 || d.th.count < 1 || d.tw.count < 1) return REHR_EINVAL;
  if (d.tile_d != 0 && (d.tile_d < 1 || d.tile_h < 1 || d.tile_w < 1 || d.tile_d * d.tile_h * d.tile_w != 128))
    return REHR_EINVAL;
  if (d.stats_mode != 0 && !d.stats) return REHR_EINVAL;
  if (d.N > 65535) return REHR_EINVAL;
  // destination extent check: the last lattice point must land inside y
  const int64_t yd = (int64_t)(d.Ld - 1) * d.osd + d.obd, yh = (int64_t)(d.Lh - 1) * d.osh + d.obh,
                yw = (int64_t)(d.Lw - 1) * d.osw + d.obw;
  if (d.obd < 0 || d.obh < 0 || d.obw < 0 || yd >= d.Dy || yh >= d.Hy || yw >= d.Wy) return REHR_EINVAL;
  if (d.ldy < d.Cout) return REHR_EINVAL;
  if ((int64_t)d.N * d.Dy * d.Hy * d.Wy >= (1ll << 31)) return REHR_EINVAL;
  return REHR_OK;
}

// ---- planning of the generic kernels: 128-voxel lattice tiles, `bk`-channel K steps ----
inline int gg_plan(const rehr_gather_gemm_desc& d, GGParams& p, int es, int bk) {
  p.d = d;
  if (d.tile_d == 0) {
    p.tiles_d = p.tiles_h = 1;
    p.tiles_w = (int)(((int64_t)d.Ld * d.Lh * d.Lw + 127) / 128);
    p.m_tiles = p.tiles_w;
  } else {
    p.tiles_d = (d.Ld + d.tile_d - 1) / d.tile_d;
    p.tiles_h = (d.Lh + d.tile_h - 1) / d.tile_h;
    p.tiles_w = (d.Lw + d.tile_w - 1) / d.tile_w;
    p.m_tiles = p.tiles_d * p.tiles_h * p.tiles_w;
  }
  p.kchunks = (d.Cin + bk - 1) / bk;
  p.wp_bytes = gg_wp_bytes(d, es);
  if (p.wp_bytes >= GG_BUF_LIMIT || !gg_src_fits(d, (int64_t)d.Di * d.Hi * d.Wi, es)) return REHR_ENOSUP;
  p.n_tiles = d.Npad / (d.Npad % 128 == 0 ? 128 : (d.Npad % 64 == 0 ? 64 : 32));
  return REHR_OK;
}

// bf16: 64-channel K steps when neither Cin nor the concat split leaves a half chunk (else 32, as in fp32)
inline bool gg_chunk64(const rehr_gather_gemm_desc& d) { return d.Cin % 64 == 0 && (d.c1 == d.Cin || d.c1 % 64 == 0); }

// ---- launch of `count` planned phases: the single-launch kernel for one, one shared grid for several ----
// (the dynamic-LDS attribute is set once per instantiation, i.e. once per kernel pair)
template <void (*KERN1)(GGParams), void (*KERNM)(GGMulti), int NT, size_t SMEM>
int gg_launch(const GGMulti& pm, int count, hipStream_t stream) {
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(KERN1), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)SMEM) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(KERNM), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)SMEM) != hipSuccess)
      return REHR_EHIP;
    attr_set = true;
  }
  if (count == 1) {
    const GGParams& p = pm.ph[0];
    hipLaunchKernelGGL(KERN1, dim3(p.m_tiles * p.n_tiles, p.d.N, 1), dim3(NT), SMEM, stream, p);
  } else {
    int nb = 0;
    bool uniform = true;
    for (int i = 0; i < count; ++i) {
      const int n = pm.ph[i].m_tiles * pm.ph[i].n_tiles;
      nb = n > nb ? n : nb;
      uniform = uniform && pm.ph[i].m_tiles == pm.ph[0].m_tiles && pm.ph[i].n_tiles == pm.ph[0].n_tiles;
    }
    GGMulti pmi = pm;
    pmi.count = count;
    const int64_t gx = (int64_t)((pm.ph[0].m_tiles + 7) / 8) * 8 * count * pm.ph[0].n_tiles;
    pmi.interleave = (uniform && !pm.no_interleave && gx < (1ll << 31)) ? 1 : 0;
    if (pmi.interleave) hipLaunchKernelGGL(KERNM, dim3((unsigned)gx, pm.ph[0].d.N, 1), dim3(NT), SMEM, stream, pmi);
    else hipLaunchKernelGGL(KERNM, dim3(nb, pm.ph[0].d.N, count), dim3(NT), SMEM, stream, pmi);
  }
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}
