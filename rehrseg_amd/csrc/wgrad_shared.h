// Types and host helpers shared by the weight-gradient family: the slab kernels and the reduction (wgrad.hip), the LDS
// brick kernels (wgrad_brick.hip, wgrad_brick_bf16.hip) and the transform-domain kernels (wino_wgrad.hip,
// wino22_wgrad.hip).  wgrad.hip decides the route; the other files expose a planner and a launcher each.
#pragma once
#include "common.h"
#include "taps.h"

struct Magic {  // q = n / d for 0 <= n < 2^31
  uint32_t m;
  uint32_t sh;  // 255: d == 1
};

struct WGParams {
  rehr_wgrad_desc d;
  int a_tiles, c_tiles, T;
  int64_t kv_total;   // N * Ld*Lh*Lw
  int64_t kv_per_split;
  int splits;
  int Capad, Cgpad;   // tile-padded channel counts of the slab
  float* slab_bias;   // [splits][Ca] or null
  Magic mg_vox, mg_hw, mg_w;
  uint32_t g_bytes;
};

// tile-padded slab geometry for square `tile` x `tile` channel tiles
inline void set_slab_geometry(WGParams& p, int Ca, int Cg, int tile) {
  p.a_tiles = (Ca + tile - 1) / tile;
  p.c_tiles = (Cg + tile - 1) / tile;
  p.Capad = p.a_tiles * tile;
  p.Cgpad = p.c_tiles * tile;
}

// ---- split-count searches.  The chosen split fixes the summation order and so the bits of the result: the double
// arithmetic and the thresholds below are part of the plan. ----
// All blocks take the same time and 512 are resident at once (256 CUs x 2): the split count near `want` (at most
// max_by_k) whose last round of blocks is fullest (tail effect).
inline int64_t splits_fullest_last_round(int64_t want, int64_t max_by_k, int64_t tiles) {
  int64_t best = want;
  double best_eff = 0.0;
  const int64_t lo = want > 2 ? want - want / 3 : 1;
  int64_t hi = want + want / 2 + 1;
  if (hi > max_by_k) hi = max_by_k > want ? max_by_k : want;
  for (int64_t s = lo; s <= hi; ++s) {
    const double rounds = (double)(tiles * s) / 512.0;
    const double eff = rounds / (double)(int64_t)(rounds + 0.999999);
    if (eff > best_eff + 1e-9) { best_eff = eff; best = s; }
  }
  return best;
}
// Whole rounds of `slots` resident blocks with at least 16 of the `items` stages per block: the first of 1..4 rounds
// that fills the chip 3 % better than the ones before it.
inline int splits_whole_rounds(int tiles, int slots, int64_t items) {
  int best_s = 1;
  double best_eff = 0.0;
  for (int k = 1; k <= 4; ++k) {
    int s = (slots * k) / tiles;
    if (s < 1) s = 1;
    if ((int64_t)s * 16 > items) s = (int)(items / 16);
    if (s < 1) s = 1;
    const int64_t blocks = (int64_t)s * tiles;
    const int64_t rounds = (blocks + slots - 1) / slots;
    const double eff = (double)blocks / (double)(rounds * slots);
    if (eff > best_eff + 0.03) { best_eff = eff; best_s = s; }
  }
  return best_s;
}

// brick plan of the fp32 weight gradient (wgrad_brick.hip): the tail of the kernel argument, read in this order
struct BrickPlanOut {
  int HD, HH, HW;        // halo extents
  int mind, minh, minw;  // smallest tap offset per axis (incl. the lattice->source offset b)
  int nb_d, nb_h, nb_w;  // bricks per sample along each axis
  int64_t nbricks;
  int bricks_per_split;
};

// brick plan of the mixed-precision weight gradient (wgrad_brick_bf16.hip)
struct BrickBf16 {
  int mind, minh, minw;      // halo origin relative to the lattice brick origin
  int nb_d, nb_h, nb_w, tiles_per_img, ntiles, tiles_per_block;
};
bool wgrad_brick_bf16_plan(const rehr_wgrad_desc& d, WGParams& w, BrickBf16& out);
int wgrad_brick_bf16_launch(const WGParams& w, const BrickBf16& o, hipStream_t stream);

bool wgrad_brick_plan(const rehr_wgrad_desc& d, WGParams& w, BrickPlanOut& out);
int wgrad_brick_launch(const WGParams& w, const BrickPlanOut& o, hipStream_t stream);

// Winograd weight gradient (wino_wgrad.hip): tried first for unit-stride 3x3 (H, W) taps
int64_t wino_wgrad_workspace_bytes(const rehr_wgrad_desc& d);  // 0 = not applicable
int wino_wgrad_try(const rehr_wgrad_desc& d, hipStream_t stream);
// F(2x2,2x2) weight gradient of stride-2 4-tap transposed convolutions (wino22_wgrad.hip)
int64_t wino22_wgrad_workspace_bytes(const rehr_wgrad_desc& d);  // 0 = not applicable
int wino22_wgrad_try(const rehr_wgrad_desc& d, hipStream_t stream);
