// Host code of the direct gather-GEMM kernels -- the halo kernels (halo_conv.hip, halo_conv_bf16.hip), tconv_ks.hip and
// the generic kernels of gather_gemm.hip / gather_gemm_bf16.hip: the brick planner both halo files share and the ONE
// decision which of these kernels takes each part of a call (direct_route).  The entry points execute that decision and
// rehr_gather_gemm_direct_route reports it; nothing here launches or reads operand memory.
#pragma once
#include "gg_shared.h"

// ---- halo kernels: plan of one launch (a kernel argument of both: the layout is part of the kernels) ----
struct HaloParams {
  rehr_gather_gemm_desc d;
  int HD, HH, HW, hvox;   // brick + tap span per axis, and their product: the rows a block stages per chunk
  int mind, minh, minw;   // smallest tap offset per axis: halo origin relative to the brick origin
  int nb_d, nb_h, nb_w, tiles_per_img;
  int64_t ntiles;         // N * tiles_per_img
  int tiles_per_block;    // persistent blocks: consecutive tiles each one walks
  int kchunks;            // 32-channel chunks of Cin
  uint32_t wp_bytes;
};

// What differs between the kernel variants.  The tables stand next to the kernels they describe.
struct HaloBrickSpec {
  int BD, BH, BW;        // lattice brick of one block
  int BN;                // output channels of one block
  int threads;
  int min_ld;            // smallest lattice depth taken (height and width: a whole brick)
  int es;                // bytes per element
  int max_hvox;          // staged rows a block can hold in registers on the way to LDS; 0: bounded by max_grow
  int max_grow;          // halo <= brick + max_grow per axis; < 0: bounded by max_hvox
  int lds_rows;          // staged rows the LDS is sized for; 0: hvox
  int lds_row;           // bytes of one staged row
  int lds_fixed;         // LDS bytes besides the staged rows
  int lds_max, lds_attr; // largest launch taken / the dynamic-LDS attribute of the kernel
  int want_blocks;       // persistent blocks wanted over all output-channel tiles
  int64_t max_y_bytes;   // y addressed through one buffer: its bytes stay below this; 0: plain stores
  int64_t max_ntiles;    // 32-bit tile counters in the kernel; 0: 64-bit
};

struct HaloPlan {
  HaloParams p;
  size_t smem;
  int variant;   // 1.. in the order of preference of halo_f32_plan / halo_bf16_plan
};

constexpr int HALO_MAX_EXT = 1023;   // both kernels pack a halo row's (d, h, w) into 10-bit fields

// Does the variant `s` take `d`?  Fills p and the launch's LDS bytes.  A brick that does not fit the lattice or pads
// it by more than 1.3x declines; so does a halo the block cannot stage and every operand a 32-bit offset cannot reach.
inline bool halo_brick_plan(const rehr_gather_gemm_desc& d, const HaloBrickSpec& s, HaloParams& p, size_t& smem) {
  if (d.Ld < s.min_ld || d.Lh < s.BH || d.Lw < s.BW) return false;
  const int64_t nb_d = (d.Ld + s.BD - 1) / s.BD, nb_h = (d.Lh + s.BH - 1) / s.BH, nb_w = (d.Lw + s.BW - 1) / s.BW;
  if (nb_d * s.BD * nb_h * s.BH * nb_w * s.BW * 10 > (int64_t)d.Ld * d.Lh * d.Lw * 13) return false;
  int mn[3], mx[3];
  span(d.td, d.bd, &mn[0], &mx[0]);
  span(d.th, d.bh, &mn[1], &mx[1]);
  span(d.tw, d.bw, &mn[2], &mx[2]);
  p.d = d;
  p.HD = s.BD + mx[0] - mn[0]; p.HH = s.BH + mx[1] - mn[1]; p.HW = s.BW + mx[2] - mn[2];
  p.hvox = p.HD * p.HH * p.HW;
  if (s.max_hvox && p.hvox > s.max_hvox) return false;
  if (s.max_grow >= 0 && (p.HD > s.BD + s.max_grow || p.HH > s.BH + s.max_grow || p.HW > s.BW + s.max_grow)) return false;
  if (p.HH > HALO_MAX_EXT || p.HW > HALO_MAX_EXT) return false;
  smem = (size_t)(s.lds_rows ? s.lds_rows : p.hvox) * s.lds_row + s.lds_fixed;
  if (smem > (size_t)s.lds_max) return false;
  if (!gg_src_fits(d, (int64_t)d.Di * d.Hi * d.Wi, s.es)) return false;
  const int64_t yvox = (int64_t)d.N * d.Dy * d.Hy * d.Wy;   // row offsets into y are ints
  if (yvox >= (1ll << 31) || (s.max_y_bytes && yvox * d.ldy * s.es >= s.max_y_bytes)) return false;
  p.mind = mn[0]; p.minh = mn[1]; p.minw = mn[2];
  p.nb_d = (int)nb_d; p.nb_h = (int)nb_h; p.nb_w = (int)nb_w;
  p.tiles_per_img = (int)(nb_d * nb_h * nb_w);
  p.ntiles = (int64_t)d.N * p.tiles_per_img;
  if (s.max_ntiles && p.ntiles >= s.max_ntiles) return false;
  p.kchunks = (d.Cin + 31) / 32;
  const int64_t wb = gg_wp_bytes(d, s.es);
  if (wb >= GG_BUF_LIMIT) return false;
  p.wp_bytes = (uint32_t)wb;
  // persistent blocks: whole rounds of want_blocks over the output-channel tiles, no more blocks than tiles
  int64_t want = s.want_blocks / (d.Npad / s.BN);
  if (want < 1) want = 1;
  if (want > p.ntiles) want = p.ntiles;
  p.tiles_per_block = (int)((p.ntiles + want - 1) / want);
  return true;
}

// "set the dynamic-LDS attribute once, then launch", once per kernel instantiation
template <void (*KERN)(HaloParams)>
int halo_launch(const HaloPlan& pl, const HaloBrickSpec& s, hipStream_t stream) {
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize,
                            s.lds_attr) != hipSuccess)
      return REHR_EHIP;
    attr_set = true;
  }
  const int64_t blocks_x = (pl.p.ntiles + pl.p.tiles_per_block - 1) / pl.p.tiles_per_block;
  hipLaunchKernelGGL(KERN, dim3((unsigned)blocks_x, pl.p.d.Npad / s.BN, 1), dim3(s.threads), pl.smem, stream, pl.p);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

// The per-precision entry conditions, then the first variant in the order of preference whose brick plan holds
// (halo_conv.hip, halo_conv_bf16.hip).  false: not a halo shape.  The launchers take what the planners filled.
bool halo_f32_plan(const rehr_gather_gemm_desc& d, HaloPlan& plan);
bool halo_bf16_plan(const rehr_gather_gemm_desc& d, HaloPlan& plan);
int halo_f32_launch(const HaloPlan& plan, hipStream_t stream);
int halo_bf16_launch(const HaloPlan& plan, hipStream_t stream);

// kernel == stride transposed convolution, fp32 and bf16: all stride phases of a 128-voxel input tile in one block
// (tconv_ks.hip).  tconv_ks_takes: the `count` validated parts are such phases and tconv_ks_launch will launch them.
bool tconv_ks_takes(const rehr_gather_gemm_desc* ds, int count, bool bf16);
int tconv_ks_launch(const rehr_gather_gemm_desc* ds, int count, bool bf16, hipStream_t stream);

// ---- the route of one call ----
// (the values are REHR_GG_DIRECT_* of the public header)
enum DirectKind { DIRECT_NONE = 0, DIRECT_GENERIC = 1, DIRECT_HALO = 2, DIRECT_TCONV_KS = 3 };
struct DirectRoute {
  int kind;       // DIRECT_NONE: no direct kernel reaches the operands (REHR_ENOSUP unless a Winograd kernel takes the part)
  int variant;    // DIRECT_HALO: HaloPlan::variant; else 0
  HaloPlan halo;  // DIRECT_HALO
  GGParams gg;    // DIRECT_GENERIC: the part's phase of the shared generic grid
};

// Which direct kernel takes each of the `count` parts of one call (es: 4 = fp32, 2 = bf16) when no Winograd kernel does.
// Every part is validated before anything is decided, so the entry points launch nothing for a call with an invalid
// part.  In this order:
//   1. count > 1 and the parts are the stride phases of a kernel == stride transposed convolution: tconv_ks takes
//      all of them in one launch (REHR_DBG_GG_NO_TCONV_KS: never);
//   2. per part, the halo kernel of the precision (bf16: not with REHR_DBG_GG_NO_HALO, and not for the tap-range parts
//      of a split-K call -- they differ in y -- which stay together in ONE generic grid: a halo launch per part would
//      run them one after the other on a few CUs each);
//   3. the generic kernel: the parts left share one grid.
inline int direct_route(const rehr_gather_gemm_desc* ds, int count, int es, DirectRoute out[MAX_PHASES]) {
  if (ds == nullptr || count < 1 || count > MAX_PHASES) return REHR_EINVAL;
  const bool bf16 = es == 2;
  for (int i = 0; i < count; ++i) {
    const int rc = gg_validate(ds[i], es);
    if (rc != REHR_OK) return rc;
    // parts of one layer: same operands and channel geometry (y may differ: split-K partials go to separate slabs)
    if (ds[i].Npad != ds[0].Npad || ds[i].N != ds[0].N || ds[i].wp != ds[0].wp || ds[i].x1 != ds[0].x1) return REHR_EINVAL;
    // bf16: Cin and c1 as well -- the generic launch takes gg_chunk64() from part 0 (fp32: 32 channels for every part)
    if (bf16 && (ds[i].Cin != ds[0].Cin || ds[i].c1 != ds[0].c1)) return REHR_EINVAL;
  }
  if (count > 1 && tconv_ks_takes(ds, count, bf16)) {
    for (int i = 0; i < count; ++i) out[i].kind = DIRECT_TCONV_KS, out[i].variant = 0;
    return REHR_OK;
  }
  for (int i = 0; i < count; ++i) {
    DirectRoute& r = out[i];
    r.variant = 0;
    const bool split_part = count > 1 && ds[i].y != ds[(i + 1) % count].y;
    const bool halo = bf16 ? !(ds[i].debug_flags & REHR_DBG_GG_NO_HALO) && !split_part && halo_bf16_plan(ds[i], r.halo)
                           : halo_f32_plan(ds[i], r.halo);
    if (halo) {
      r.kind = DIRECT_HALO;
      r.variant = r.halo.variant;
    } else {
      const int bk = bf16 && gg_chunk64(ds[i]) ? 64 : 32;
      r.kind = gg_plan(ds[i], r.gg, es, bk) == REHR_OK ? DIRECT_GENERIC : DIRECT_NONE;
    }
  }
  return REHR_OK;
}
