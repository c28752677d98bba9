// Types and host helpers shared by the fp32 transform-domain forward / input-gradient family: the F(2x2,3x3) region
// kernels (wino_conv.hip), the flattened-tile F(2x2,3x3) kernel (wino_flat8_conv.hip) and the F(2x2,2x2) kernels
// (wino22_conv.hip).  gather_gemm.hip decides the route (wino_route); the kernel files expose planners (pure: they read
// no pointer) and launchers (they take the plan).  The size query, the route query and the launch read the same plan.
#pragma once
#include "common.h"
#include "gg_shared.h"
#include "wino22_shared.h"

// route of one descriptor, in the order in which wino_route() tries them (values = REHR_GG_ROUTE_*)
enum WinoRoute {
  WINO_NONE = REHR_GG_ROUTE_NONE,
  WINO_FLAT8 = REHR_GG_ROUTE_FLAT8,        // F(2x2,3x3), flattened tiles (wino_flat8_conv.hip)
  WINO_W32P = REHR_GG_ROUTE_W32P,          // F(2x2,3x3), 32-channel pipelined tile (wino_conv.hip)
  WINO_BIG8 = REHR_GG_ROUTE_BIG8,          // F(2x2,3x3), 16 x 16 regions x 64 channels (wino_conv.hip)
  WINO_SMALL = REHR_GG_ROUTE_SMALL,        // F(2x2,3x3), 8 x 16 regions x 32 channels (wino_conv.hip)
  WINO_FLAT22 = REHR_GG_ROUTE_FLAT22,      // F(2x2,2x2), flattened tiles (wino22_conv.hip)
  WINO_REGION22 = REHR_GG_ROUTE_REGION22,  // F(2x2,2x2), 16 x 16 regions (wino22_conv.hip)
};

constexpr int WINO_LDX = 36;    // floats per voxel slot in LDS (32 channels + 4), every kernel of the family but w32p
constexpr int WINO_MAXPH = 4;   // source phases of one F(2x2,2x2) launch / output phases of one flattened-tile grid

struct Phase {     // one source phase of the F(2x2,2x2) kernels
  int sh, sw;      // source stride of the sub-lattice (1 or 2)
  int ph, pw;      // parity offset inside the source
  int dh0, dw0;    // sub-lattice position of patch row/col 0 relative to the region origin
};

// geometry of a flattened-tile launch: the 2 x 2 tiles of all slices numbered consecutively, a block stages the
// contiguous range of padded rows its tiles read (the kernels' argument structs are filled from this)
struct FlatGeom {
  int nth, ntw, tps;   // tiles per slice
  int ntiles;          // N * Ld * tps
  int PH;              // padded rows per slice
  int PWs, nev;        // column slots per row; even columns first (nev of them)
  int RP, rowpad;      // row pitch in floats = PWs * WINO_LDX + rowpad
  int rows;            // rows a block stages at most
  int rowmagic;        // v / PWs == (v * rowmagic) >> 16 for every staged v
  int tab_off;         // float offset of the per-tile tables behind the exchange buffer
};
// what the two flattened-tile kernels differ in
struct FlatConsts {
  int border;          // zero rows / columns around a slice: 2 (3 taps), 1 (2 taps)
  int tiles;           // tiles per block
  int pieces;          // 16-byte pieces a block can stage: pieces per thread x threads
  int fill_min;        // 64 x 64 units below which another path fills the chip better
  int64_t efl, rfl;    // floats of the exchange and of the statistics buffer (they share the staging buffer's LDS)
  int lds_cap;         // bytes
};
constexpr int FLAT_MAXSLOT = 8;   // slices a block may touch (statistics slots)

struct WinoPlan {
  int64_t bytes;       // scratch for the transformed weights of this descriptor
  int variant;         // FLAT8: tile groups NFM (1 = 32, 2 = 64 tiles per block); W32P: G (1 | 2); else 0
  int kchunks;         // 32-channel chunks
  int nb_h, nb_w;      // regions per slice (region kernels)
  FlatGeom flat;       // flattened-tile kernels
  int nphase;          // F(2x2,2x2): source phases; the parts of a multi-part flat22 plan have one each, phase[part]
  Phase phase[WINO_MAXPH];
};

// bytes of `xforms` transformed taps per (depth tap, output channel, 32-padded input channel); 0: beyond a 32-bit offset
inline int64_t wino_scratch_bytes(const rehr_gather_gemm_desc& d, int xforms) {
  const int64_t need = (int64_t)xforms * d.td.count * d.Npad * ((d.Cin + 31) / 32) * 32 * (int64_t)sizeof(float);
  return need >= (1ll << 32) - 64 ? 0 : need;
}
// the scratch admission: given, large enough, 16-byte aligned
inline bool wino_ws_ok(const rehr_gather_gemm_desc& d, int64_t need) {
  return d.wino_ws && d.wino_ws_bytes >= need && !((uintptr_t)d.wino_ws & 15);
}

// LDS bank-group spread of one 16-lane phase of a fragment read: lanes = 16 consecutive tiles at one column parity,
// 16-byte units (tw * 9 + (row pitch / 2) * tile row) mod 16; returns the worst multiplicity over the alignments
inline int flat_conflicts(int ntw, int RP) {
  int worst = 0;
  for (int a = 0; a < ntw; ++a) {
    int cnt[16] = {0};
    for (int l = 0; l < 16; ++l) {
      const int t = a + l, th = t / ntw, tw = t - th * ntw;
      const int unit = ((tw * WINO_LDX + th * 2 * RP) / 4) & 15;
      if (++cnt[unit] > worst) worst = cnt[unit];
    }
  }
  return worst;
}

// Everything the flattened-tile planners share, behind their own tap checks: plane limits, padding rule, fill threshold,
// staging geometry, index bounds and LDS size.  `parts`: descriptors that share the grid (fill threshold only).
inline bool plan_flat_geom(const rehr_gather_gemm_desc& d, const FlatConsts& c, int parts, FlatGeom& g) {
  if (d.td.count < 1 || d.td.count > 3) return false;
  if (d.Npad % 64 || d.Lh < 6 || d.Lw < 6 || d.Lw > 64) return false;
  if (d.Lh % 16 == 0 && d.Lw % 16 == 0) return false;      // whole 16 x 16 regions: the region kernels stage less halo
  g.nth = (d.Lh + 1) / 2;
  g.ntw = (d.Lw + 1) / 2;
  g.tps = g.nth * g.ntw;
  if ((int64_t)g.nth * 2 * g.ntw * 2 * 10 > (int64_t)d.Lh * d.Lw * 13) return false;  // odd extents pad a half tile
  const int64_t ntiles = (int64_t)d.N * d.Ld * g.tps;
  if (ntiles >= (1ll << 30) || ntiles < c.tiles) return false;
  g.ntiles = (int)ntiles;
  if ((ntiles + 63) / 64 * (d.Npad / 64) * parts < c.fill_min) return false;
  if ((c.tiles - 2) / g.tps + 2 > FLAT_MAXSLOT) return false;
  g.PH = 2 * g.nth + c.border;
  g.nev = g.ntw + 1;
  g.PWs = 2 * g.ntw + c.border;
  const int trr = (c.tiles - 2) / g.ntw + 2, sdiff = (c.tiles - 2) / g.tps + 1;
  g.rows = 2 * (trr - 1) + c.border * (sdiff + 1) + 2;
  if ((int64_t)g.rows * g.PWs * 8 > c.pieces) return false;
  g.rowmagic = 65536 / g.PWs + 1;
  for (int v = 0; v <= g.rows * g.PWs; ++v)
    if (((v * g.rowmagic) >> 16) != v / g.PWs) return false;
  int best = 1 << 30;
  for (int pad = 4; pad <= 64; pad += 4) {
    const int cf = flat_conflicts(g.ntw, g.PWs * WINO_LDX + pad);
    if (cf < best) { best = cf; g.rowpad = pad; }
  }
  g.RP = g.PWs * WINO_LDX + g.rowpad;
  if (!gg_src_fits(d, (int64_t)d.N * d.Di * d.Hi * d.Wi, 4)) return false;   // one buffer over the whole batch
  if ((int64_t)d.N * d.Dy * d.Hy * d.Wy >= (1ll << 31) || d.Npad / 64 > 65535) return false;
  int64_t fl = (int64_t)2 * (g.rows * g.RP + WINO_LDX + 4);
  if (c.efl > fl) fl = c.efl;
  if (c.rfl > fl) fl = c.rfl;
  g.tab_off = (int)fl;
  return (fl + 3 * c.tiles) * 4 <= c.lds_cap;
}
// the kernels' argument structs keep their own field order (Flat8Params, F22Params): filled from the geometry by name
template <typename P>
inline void flat_fill(P& p, const FlatGeom& g) {
  p.nth = g.nth; p.ntw = g.ntw; p.tps = g.tps; p.ntiles = g.ntiles;
  p.PH = g.PH; p.PWs = g.PWs; p.nev = g.nev; p.RP = g.RP; p.rowpad = g.rowpad;
  p.rows = g.rows; p.rowmagic = g.rowmagic; p.tab_off = g.tab_off;
}
inline size_t flat_lds_bytes(const FlatGeom& g, int tiles) { return (size_t)(g.tab_off + 3 * tiles) * sizeof(float); }

// the source phases of an F(2x2,2x2) plan from its two axis plans; returns their number
inline int fill_phases(const AxisPlan& ah, const AxisPlan& aw, Phase* phase) {
  for (int i = 0; i < ah.nph; ++i)
    for (int j = 0; j < aw.nph; ++j) {
      Phase& P = phase[i * aw.nph + j];
      P.sh = ah.stride; P.sw = aw.stride;
      P.ph = ah.par[i]; P.pw = aw.par[j];
      P.dh0 = ah.dmin[i]; P.dw0 = aw.dmin[j];
    }
  return ah.nph * aw.nph;
}

// "The same layer as part 0" for the two multi-part entries.  Always compared: the source (x2, channel split, row
// pitches), the channel geometry and the lattice with its depth origin.  (x1, wp, N and Npad: the dispatcher has compared
// them for every multi-descriptor call.)  The field sets of the two entries really differ:
//  * split-K parts (wino_split_plan) differ in their DEPTH taps and write one slab each: the (H, W) taps must agree
//    (SAME_HW_TAPS); y, td and the scratch are per part.  Dy/Hy/Wy and the output stride / offset are not compared:
//    the planner of every part already requires the lattice to be the whole destination.
//  * output phases of a transposed convolution (wino22_flat_multi_plan) differ in their (H, W) taps and (H, W) output
//    offsets and interleave into ONE destination: the depth taps' geometry and the destination with its epilogue must
//    agree (SAME_DEPTH_TAPS | SAME_DEST).  td.k0 / td.ks are not compared: each part transforms its own weights.
enum { SAME_HW_TAPS = 1, SAME_DEPTH_TAPS = 2, SAME_DEST = 4 };
inline bool gg_same_layer(const rehr_gather_gemm_desc& d, const rehr_gather_gemm_desc& d0, unsigned groups) {
  if (d.x2 != d0.x2 || d.Cin != d0.Cin || d.c1 != d0.c1 || d.ldx1 != d0.ldx1 || d.ldx2 != d0.ldx2 || d.Cout != d0.Cout ||
      d.ldy != d0.ldy || d.Ld != d0.Ld || d.Lh != d0.Lh || d.Lw != d0.Lw || d.Di != d0.Di || d.Hi != d0.Hi ||
      d.Wi != d0.Wi || d.bd != d0.bd)
    return false;
  auto same_axis = [](const rehr_axis_taps& a, const rehr_axis_taps& b) {
    return a.count == b.count && a.off0 == b.off0 && a.offs == b.offs && a.k0 == b.k0 && a.ks == b.ks;
  };
  if ((groups & SAME_HW_TAPS) && (d.bh != d0.bh || d.bw != d0.bw || d.KH != d0.KH || d.KW != d0.KW ||
                                  !same_axis(d.th, d0.th) || !same_axis(d.tw, d0.tw)))
    return false;
  if ((groups & SAME_DEPTH_TAPS) && (d.td.count != d0.td.count || d.td.off0 != d0.td.off0 || d.td.offs != d0.td.offs))
    return false;
  if ((groups & SAME_DEST) &&
      (d.y != d0.y || d.Dy != d0.Dy || d.Hy != d0.Hy || d.Wy != d0.Wy || d.osd != d0.osd || d.osh != d0.osh ||
       d.osw != d0.osw || d.obd != d0.obd || d.bias != d0.bias || d.act != d0.act || d.slope != d0.slope ||
       d.stats != d0.stats || d.stats_mode != d0.stats_mode))
    return false;
  return true;
}

// The transform arithmetic of the weight forms, one copy: the panel transforms (wino_weights*_kernel, w22_weights_kernel)
// and the one-pass form kernel (wino_forms.hip) call these, so both write the same bits.
// F(2x2,3x3): u[r*4 + c] = (G g G^T)[r][c]
__device__ __forceinline__ void wino_u33(const float (&g)[3][3], float (&u)[16]) {
  const float G[4][3] = {{1.f, 0.f, 0.f}, {.5f, .5f, .5f}, {.5f, -.5f, .5f}, {0.f, 0.f, 1.f}};
  float t[4][3];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int b = 0; b < 3; ++b) t[r][b] = G[r][0] * g[0][b] + G[r][1] * g[1][b] + G[r][2] * g[2][b];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) u[r * 4 + c] = t[r][0] * G[c][0] + t[r][1] * G[c][1] + t[r][2] * G[c][2];
}
// F(2x2,2x2): G = [[1,0],[1,1],[0,1]]
__device__ __forceinline__ void wino_u22(const float (&g)[2][2], float (&u)[9]) {
  u[0] = g[0][0];              u[1] = g[0][0] + g[0][1];                     u[2] = g[0][1];
  u[3] = g[0][0] + g[1][0];    u[4] = g[0][0] + g[0][1] + g[1][0] + g[1][1]; u[5] = g[0][1] + g[1][1];
  u[6] = g[1][0];              u[7] = g[1][0] + g[1][1];                     u[8] = g[1][1];
}

// One weight-transform launch: `total` items on blocks of 256 threads, at most `cap` blocks (grid-stride kernels);
// skipped when the caller kept the transformed weights of an earlier call (REHR_GG_WS_READY).  The REHR_GG_WS_ONLY
// return is the dispatcher's, right behind this.  (static: rehr_launch_failed is per translation unit)
template <auto KERN, typename... Args>
static int wino_transform_launch(const rehr_gather_gemm_desc& d, int64_t total, int cap, hipStream_t stream, Args... args) {
  if (d.flags & REHR_GG_WS_READY) return REHR_OK;
  int64_t blocks = (total + 255) / 256;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(KERN, dim3((unsigned)blocks), dim3(256), 0, stream, d, d.wino_ws, args...);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

// ---- planners and launchers of the kernel files.  `ds` / `count`: the parts of a multi-part plan (count == 1: plain).
// wino_conv.hip: W32P before BIG8 before SMALL, or WINO_NONE
WinoRoute wino_region_plan(const rehr_gather_gemm_desc& d, WinoPlan& plan);
// split-K parts (depth-tap ranges of one layer, one slab each) in one grid of the big-tile kernel: all parts or none
bool wino_split_plan(const rehr_gather_gemm_desc* ds, int count, WinoPlan& plan);
int wino_weights_launch(WinoRoute r, const rehr_gather_gemm_desc& d, const WinoPlan& plan, hipStream_t stream);
int wino_region_launch(WinoRoute r, const rehr_gather_gemm_desc* ds, int count, const WinoPlan& plan, hipStream_t stream);
// wino_flat8_conv.hip (its weight transform is wino_weights_launch)
bool wino_flat8_plan(const rehr_gather_gemm_desc& d, WinoPlan& plan);
int wino_flat8_launch(const rehr_gather_gemm_desc& d, const WinoPlan& plan, hipStream_t stream);
// wino22_conv.hip; `parts`: descriptors that will share the flattened-tile grid
bool wino22_flat_plan(const rehr_gather_gemm_desc& d, WinoPlan& plan, int parts);
bool wino22_region_plan(const rehr_gather_gemm_desc& d, WinoPlan& plan);
// the output phases of one transposed convolution in one grid of the flattened-tile kernel: all parts or none
bool wino22_flat_multi_plan(const rehr_gather_gemm_desc* ds, int count, WinoPlan& plan);
int wino22_weights_launch(const rehr_gather_gemm_desc& d, const WinoPlan& plan, hipStream_t stream);
int wino22_launch(WinoRoute r, const rehr_gather_gemm_desc* ds, int count, const WinoPlan& plan, hipStream_t stream);

// wino_forms.hip: the transform-domain weights of `count` parts (route r[i], scratch attached and admitted) straight
// from the fp32 parameter in torch layout -- no panel.  Element (tap t, destination row n, source channel ci) of the
// parameter is w[n * sn + ci * sc + t]; rows >= d.Cout and channels >= d.Cin are zero, as in a panel.
struct WinoWeightSrc {
  const float* w;
  int64_t sn, sc;
};
int wino_forms_launch(const WinoRoute* r, const rehr_gather_gemm_desc* ds, int count, const WinoWeightSrc& src,
                      hipStream_t stream);
