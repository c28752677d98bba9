/*
 * rehrseg_hip.h -- C-ABI of librehrseg_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the 3D-convolutional hot path of zhiyuns/REHRSeg.  The
 * reference has no FFI of its own: its operator layer is torch.nn
 * (Conv3d / ConvTranspose3d / InstanceNorm3d / LeakyReLU / F.interpolate, see
 * the citations on every entry point).  These entry points are what a
 * maintainer would bind with ctypes in place of those torch.nn calls
 * (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (no allocation
 *     happens behind the ABI; scratch comes from a caller-provided workspace);
 *   - activations are fp32, channel-innermost ("NDHWC"): element (n,d,h,w,c) of
 *     a tensor with voxel stride `ld` lives at ((n*D+d)*H+h)*W+w)*ld + c, so a
 *     channel slice of a wider buffer is addressed by offsetting the pointer
 *     and keeping `ld` (this is how skip concatenation costs nothing);
 *   - `stream` is a hipStream_t passed as void*; launches are stream ordered,
 *     re-entrant, and never synchronise;
 *   - return value 0 = launched; <0 = rejected argument (REHR_E*), nothing was
 *     launched.  No exceptions, no global state.
 */
#ifndef REHRSEG_HIP_H
#define REHRSEG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REHR_OK 0
#define REHR_EINVAL -1   /* malformed descriptor (sizes, alignment, null) */
#define REHR_ENOSUP -2   /* valid but not supported by this build */
#define REHR_EHIP -3     /* hip launch error */

/* activation codes used by the fused epilogues */
#define REHR_ACT_NONE 0
#define REHR_ACT_RELU 1
#define REHR_ACT_LRELU 2 /* slope given separately */

/* Taps of one spatial axis, described arithmetically (no device tables):
 * tap j (0 <= j < count) reads the source at  base + off0 + offs*j  and uses
 * weight index  k0 + ks*j  along this axis.                                   */
typedef struct {
  int32_t count, off0, offs, k0, ks;
} rehr_axis_taps;

/* ------------------------------------------------------------------------- *
 * Gather-GEMM: the one contraction behind Conv3d forward, Conv3d input
 * gradient (one launch per stride phase), ConvTranspose3d forward (one launch
 * per stride phase), ConvTranspose3d input gradient, and Conv2d (D = 1).
 *
 *   for every lattice point o=(od,oh,ow), sample n, output channel co:
 *     y[n, o*os+ob, co] = act( bias[co] + sum_{taps j} sum_{ci}
 *           x[n, o*s+b+off(j), ci] * wp[tap(j)][co][ci] )
 *   (source positions outside [0,Di)x[0,Hi)x[0,Wi) read as zero)
 *
 * Replaces: torch.nn.Conv3d.forward as used at models/FLAVR/resnet_3D.py:19-33,
 * 42-50, 196-200; models/FLAVR/FLAVR_arch.py:50,77,145,153-156;
 * models/seg_model.py:197-199 and the PlainConvUNet blocks behind
 * models/seg_model.py:174-191, plus the autograd input-gradient of each.
 * ------------------------------------------------------------------------- */
typedef struct {
  /* source tensor(s): channels [0,c1) come from x1, [c1,Cin) from x2 (virtual
   * concat, models/FLAVR/FLAVR_arch.py:14-21); x2 may be NULL when c1 == Cin. */
  const float* x1;
  const float* x2;
  int32_t c1, ldx1, ldx2;
  int32_t N, Di, Hi, Wi, Cin;      /* Cin % 16 == 0; c1 % 32 == 0 when x2 is used */
  /* lattice and its map into the source */
  int32_t Ld, Lh, Lw;
  int32_t sd, sh, sw, bd, bh, bw;
  rehr_axis_taps td, th, tw;
  int32_t KH, KW;                  /* weight tap index = (kd*KH+kh)*KW+kw */
  /* packed weights wp[tap][Npad][Cin] (ci innermost), Npad % 32 == 0 */
  const float* wp;
  int32_t Npad;
  /* destination tensor and the lattice's map into it */
  float* y;
  int32_t Dy, Hy, Wy, Cout, ldy;
  int32_t osd, osh, osw, obd, obh, obw;
  /* fused epilogue */
  const float* bias;               /* NULL or [Cout] */
  int32_t act;
  float slope;
  /* optional per-(n,co) statistics of the stored value, accumulated with
   * double atomics into stats[n][co][2] = {sum, sum of squares}; 0 = off,
   * 1 = sum only (SEGating pool), 2 = sum and squares (InstanceNorm3d).       */
  double* stats;
  int32_t stats_mode;
  /* lattice tile: a td x th x tw brick with td*th*tw == 128, or tile_d == 0
   * for runs of 128 consecutive flattened lattice points (odd extents)         */
  int32_t tile_d, tile_h, tile_w;
  /* optional scratch for the Winograd F(2x2,3x3)-over-(H,W) kernel (NULL = never use
   * it).  When given, >= rehr_gather_gemm_wino_bytes(d) bytes, 16-byte aligned, and
   * the contraction is a unit-stride one with taps {-1,0,+1} along H and W, the
   * library transforms wp into it and runs the 2.25x-fewer-multiplications path
   * (same fp32 results up to the transform's rounding, ~1e-6 relative).          */
  float* wino_ws;
  int64_t wino_ws_bytes;
  int32_t flags;                   /* REHR_GG_* bits; 0 = the library picks the measured-best kernel */
  int32_t debug_flags;             /* REHR_DBG_GG_* bits (below): kernel-selection overrides for tests and A/B
                                    * runs.  NOT part of the stable interface -- integrators leave it 0.        */
} rehr_gather_gemm_desc;

/* bf16 entry points: store y as fp32 instead of bf16 (logits, features handed to fp32 losses) */
#define REHR_GG_Y_F32 1
/* fp32 entry points, wino_ws given.  The Winograd-domain weights in wino_ws depend on wp and on the descriptor's
 * geometry only, so a caller whose weights have not changed since an earlier call with the same geometry may keep the
 * scratch and skip the transform launch:
 *   REHR_GG_WS_ONLY   run ONLY the weight transform(s) this descriptor (or this multi-call) would run: wino_ws is
 *                     filled, nothing else is launched, x1 / x2 / y / bias / stats are not dereferenced (REHR_OK also
 *                     when no Winograd kernel takes the descriptor: nothing to prepare);
 *   REHR_GG_WS_READY  wino_ws already holds what REHR_GG_WS_ONLY (or a full call) with the same geometry, the same wp
 *                     contents and the same debug_flags wrote: skip the transform.
 * In a multi-call every descriptor carries the same two bits. */
#define REHR_GG_WS_READY 2
#define REHR_GG_WS_ONLY 4

/* debug_flags (unstable; the parity tests compare kernel organisations with each other through them):
 * bf16: never take the LDS halo-brick kernel (per-tap gather kernel instead) */
#define REHR_DBG_GG_NO_HALO 1
/* fp32: the flattened-tile Winograd kernels (wino_flat8_conv.hip, wino22_flat) off / forced to 32 or 64 tiles per block */
#define REHR_DBG_GG_NO_FLAT8 2
#define REHR_DBG_GG_FLAT8_HALF 4
#define REHR_DBG_GG_FLAT8_FULL 8
/* fp32: the 32-channel-tile Winograd kernel forced to two 256-thread blocks per CU / one 512-thread block */
#define REHR_DBG_GG_W32P_TWO_PER_CU 16
#define REHR_DBG_GG_W32P_ONE_PER_CU 32
/* multi-phase launches with equal tile counts: the phases of a lattice tile as consecutive blocks of one XCD instead of
 * blockIdx.z = phase.  Measured SLOWER (profiles/r03_ab_phase_interleave.txt: +1.4 ms per cfg-3 step, +0.25 ms cfg-5),
 * kept as a test-selectable organisation only. */
#define REHR_DBG_GG_INTERLEAVE 64
/* kernel == stride transposed convolutions: the generic one-block-per-(tile, phase) grid instead of the fused kernel
 * that stages a tile once for all phases (tconv_ks.hip) */
#define REHR_DBG_GG_NO_TCONV_KS 128
/* fp32 Winograd kernels: tiles in slice-major order (bw, bh, od) instead of the band-major order (bw, od, bh) that keeps
 * the depth neighbours of a tile on one XCD */
#define REHR_DBG_GG_SLICE_MAJOR 256

/* scratch bytes the Winograd path needs for this descriptor; 0 = not applicable */
int64_t rehr_gather_gemm_wino_bytes(const rehr_gather_gemm_desc* d);
/* Which fp32 Winograd kernel a launch of this descriptor with that scratch takes: the route in the low byte
 * (0 exactly when rehr_gather_gemm_wino_bytes is 0), the variant in bits 8..15 -- FLAT8: 1 / 2 for 32 / 64 tiles per
 * block, W32P: 1 / 2 for 256- / 512-thread blocks, else 0.  Reads no pointer of the descriptor. */
#define REHR_GG_ROUTE_NONE 0
#define REHR_GG_ROUTE_FLAT8 1    /* F(2x2,3x3), flattened tiles (small planes) */
#define REHR_GG_ROUTE_W32P 2     /* F(2x2,3x3), 32-channel pipelined tile */
#define REHR_GG_ROUTE_BIG8 3     /* F(2x2,3x3), 16 x 16 regions x 64 channels */
#define REHR_GG_ROUTE_SMALL 4    /* F(2x2,3x3), 8 x 16 regions x 32 channels */
#define REHR_GG_ROUTE_FLAT22 5   /* F(2x2,2x2), flattened tiles */
#define REHR_GG_ROUTE_REGION22 6 /* F(2x2,2x2), 16 x 16 regions */
int rehr_gather_gemm_wino_route(const rehr_gather_gemm_desc* d);
/* Which direct kernel a call of rehr_gather_gemm_multi_f32 (bf16 = 0) or rehr_gather_gemm_multi_bf16 (bf16 != 0) with
 * these `count` descriptors runs for each part that no Winograd kernel takes: routes[i] = kind | variant << 8.
 * HALO variants, in the order of preference -- fp32: 1 / 2 for the 64- / 32-channel tile; bf16: 1 / 2 / 3 for the
 * bricks 4x8x16 / 8x8x8 / 2x16x16; else 0.  TCONV_KS: every part carries it (one launch runs them all).  NONE: no direct
 * kernel reaches the operands, the call returns REHR_ENOSUP unless a Winograd kernel takes the part.
 * Returns REHR_OK, or REHR_EINVAL exactly when the launch would (routes is then not written).  The same decision
 * drives the launch.  Reads no operand memory. */
#define REHR_GG_DIRECT_NONE 0
#define REHR_GG_DIRECT_GENERIC 1   /* the per-tap gather kernels; the generic parts of a call share one grid */
#define REHR_GG_DIRECT_HALO 2      /* input brick with its halo staged in LDS (halo_conv.hip, halo_conv_bf16.hip) */
#define REHR_GG_DIRECT_TCONV_KS 3  /* kernel == stride transposed convolution, all stride phases in one block */
int rehr_gather_gemm_direct_route(const rehr_gather_gemm_desc* descs, int32_t count, int32_t bf16, int32_t* routes);
int rehr_gather_gemm_f32(const rehr_gather_gemm_desc* d, void* stream);
/* The stride phases of ONE layer (same x1/x2, wp, y, N, Npad; count <= 8), differing
 * only in lattice, taps and destination offset, in a single grid.                   */
int rehr_gather_gemm_multi_f32(const rehr_gather_gemm_desc* descs, int32_t count,
                               void* stream);
/* The Winograd-domain weights of one call (the `count` <= 8 descriptors that rehr_gather_gemm_multi_f32 would get, scratch
 * attached) straight from the fp32 parameter, without a panel: fills every descriptor's wino_ws with exactly what the
 * call -- or REHR_GG_WS_ONLY -- writes there from the panel of that parameter, bit for bit; the convolution is then
 * launched with REHR_GG_WS_READY.  No Winograd kernel dereferences wp under REHR_GG_WS_READY: it only has to pass the
 * validation (non-null, 16-byte aligned, the same in every part).
 *   w        the parameter in torch layout, (D0, D1, T) contiguous with T = KD * KH * KW taps: (Cout, Cin, ...) of a
 *            Conv3d, (Cin, Cout, ...) of a ConvTranspose3d
 *   dest_dim which of the two dimensions feeds the descriptor's destination rows (0 | 1): forward or input gradient
 *   dest_lo, src_lo   first channel of the destination / source dimension (the halves of a virtual concat are
 *            sub-ranges, read in place); the ranges are [dest_lo, dest_lo + Cout) and [src_lo, src_lo + Cin)
 * The descriptor's taps select what is read, as in a launch (k0, ks, count per axis; mirrored taps, depth-tap ranges,
 * the 2-tap phases and the 4-tap stride-2 gather of the transposed convolutions).
 * REHR_EINVAL: what rehr_gather_gemm_multi_f32 rejects, a null or misaligned w, a range or a tap outside the parameter.
 * REHR_ENOSUP: the launch would not run a Winograd kernel for every part (no route, no or too small a scratch, the
 * fused kernel == stride transposed convolution): nothing is launched, the caller needs the panel. */
int rehr_gather_gemm_wino_forms_f32(const rehr_gather_gemm_desc* descs, int32_t count, const float* w, int32_t D0,
                                    int32_t D1, int32_t T, int32_t dest_dim, int32_t dest_lo, int32_t src_lo,
                                    void* stream);
/* Mixed-precision variants (BASELINE.json configs[4]: bf16 conv inputs / weights, fp32 accumulation on
 * v_mfma_f32_32x32x16_bf16, fp32 bias / fp64 statistics formed from the fp32 accumulators): the SAME descriptor
 * with x1, x2, wp and y pointing at bf16 elements (ld* and channel counts stay in ELEMENTS; rows must be
 * 16-byte aligned: ldx % 8 == 0; c1 % 32 == 0 when x2 is used), y fp32 with REHR_GG_Y_F32; wino_ws is
 * ignored (the bf16 pipe is 16x the fp32 one: the direct contraction is operand-bandwidth bound already).
 * rehr_pack_weights_bf16: the torch parameter layout in[a][b][t] (transpose_ab: in[b][a][t]) fp32 ->
 * out[t][Apad][B] bf16 -- master weights stay fp32.
 * Replaces the same torch.nn.Conv3d / ConvTranspose3d call sites under bf16 autocast.                */
int rehr_gather_gemm_bf16(const rehr_gather_gemm_desc* d, void* stream);
int rehr_gather_gemm_multi_bf16(const rehr_gather_gemm_desc* descs, int32_t count, void* stream);
int rehr_pack_weights_bf16(const float* in, void* out, int32_t A, int32_t Apad, int32_t B, int32_t T,
                           int32_t transpose_ab, void* stream);

/* Split-K combine: y[row][c] = act(bias[c] + sum_s slabs[s*slab_stride + row*C + c]).
 * A contraction with few lattice tiles and very many taps (feature_fuse:
 * models/FLAVR/FLAVR_arch.py:145, 16384 voxels x 1152 taps) is launched as S
 * tap ranges writing S dense slabs through rehr_gather_gemm_multi_f32 (descs that
 * differ in y), then combined here in a fixed order.                            */
int rehr_sum_slabs_bias_act_f32(const float* slabs, int32_t S, int64_t slab_stride,
                                const float* bias, float* y, int64_t rows, int32_t C,
                                int32_t act, float slope, void* stream);

/* The same combine with the statistics epilogue of the gather-GEMM: stats[N][C][2] += {sum, sum of
 * squares} of the stored value per sample and channel (y is dense [N][SV][C]; stats pre-zeroed by
 * the caller).  Lets the low-resolution nnU-Net stages (<= 8^3 voxels, 320 channels: 40 tiles on
 * 256 CUs) run split over their taps.                                                       */
int rehr_sum_slabs_stats_f32(const float* slabs, int32_t S, int64_t slab_stride, const float* bias,
                             float* y, int32_t N, int64_t SV, int32_t C, int32_t act, float slope,
                             double* stats, void* stream);

/* Mixed precision: the same two combines with fp32 slabs (the bf16 gather-GEMM writes them with REHR_GG_Y_F32) and a
 * bf16 result; statistics are formed from the fp32 sums, like the conv epilogues.                  */
int rehr_sum_slabs_bias_act_bf16(const float* slabs, int32_t S, int64_t slab_stride, const float* bias, void* y,
                                 int64_t rows, int32_t C, int32_t act, float slope, void* stream);
int rehr_sum_slabs_stats_bf16(const float* slabs, int32_t S, int64_t slab_stride, const float* bias, void* y,
                              int32_t N, int64_t SV, int32_t C, int32_t act, float slope, double* stats,
                              void* stream);

/* ------------------------------------------------------------------------- *
 * Weight gradient (Conv3d.weight.grad / ConvTranspose3d.weight.grad):
 *
 *   dst[a*dst_sa + c*dst_sc + tap*dst_st] = sum_{n, lattice o}
 *         l[n, o, a] * g[n, o*s+b+off(tap), c]
 *
 * l = the tensor living ON the lattice (dY for Conv3d, the input for
 * ConvTranspose3d), g = the gathered tensor (X for Conv3d, dY for
 * ConvTranspose3d).  Deterministic: partial sums go to `workspace` slabs
 * and are reduced in a fixed order.
 * Replaces autograd's conv weight gradient for the call sites listed above.
 * ------------------------------------------------------------------------- */
typedef struct {
  const float* l;
  int32_t ldl, Ca;                 /* Ca % 4 == 0 */
  const float* g;
  int32_t ldg, Cg;                 /* Cg % 4 == 0 */
  int32_t N, Ld, Lh, Lw;           /* lattice (= spatial dims of l) */
  int32_t Dg, Hg, Wg;              /* spatial dims of g */
  int32_t sd, sh, sw, bd, bh, bw;
  rehr_axis_taps td, th, tw;
  int32_t KH, KW;
  float* dst;
  int64_t dst_sa, dst_sc, dst_st;
  int32_t accumulate;              /* 0: dst = sum, 1: dst += sum */
  float* workspace;                /* >= rehr_wgrad_workspace_bytes() */
  int64_t workspace_bytes;
  float* dbias;                    /* NULL or [Ca]: dbias[a] (+)= sum l[...,a] */
  int32_t flags;                   /* reserved, 0 */
  int32_t debug_flags;             /* REHR_DBG_WGRAD_* bits: kernel-selection overrides for tests and A/B runs;
                                    * NOT part of the stable interface -- integrators leave it 0.  Everything that
                                    * selects a kernel travels in the descriptors: the library reads no environment
                                    * variables and keeps no mutable state between calls.                        */
} rehr_wgrad_desc;

/* debug_flags: force the direct (slab / brick) kernels even where a transform-domain (Winograd) kernel applies */
#define REHR_DBG_WGRAD_DIRECT 1
/* Winograd weight gradient: walk every output slice for every depth tap (default: a tap skips the slices whose source
 * slice lies outside the volume; tests compare both) */
#define REHR_DBG_WGRAD_NO_TAP_SKIP 2
/* Winograd weight gradient: blockIdx.z = depth tap instead of the taps of a split as consecutive blocks of one XCD */
#define REHR_DBG_WGRAD_NO_TAP_COLOCATE 4

/* Mixed-precision weight gradient: l and g point at bf16 elements (ld* in elements, % 8 == 0; Ca, Cg % 8 == 0),
 * fp32 accumulation on v_mfma_f32_32x32x16_bf16, fp32 slabs and fp32 dst (the master-weight gradient).  dbias must
 * be NULL (the bias gradient is a column sum of dY: rehr_channel_sum).  Own workspace query.                  */
int64_t rehr_wgrad_bf16_workspace_bytes(const rehr_wgrad_desc* d);
int rehr_wgrad_bf16(const rehr_wgrad_desc* d, void* stream);
int64_t rehr_wgrad_workspace_bytes(const rehr_wgrad_desc* d);
/* 1 when rehr_wgrad_f32 will take a transform-domain path for this descriptor: F(2x2,3x3)
 * (unit stride, taps {-1,0,+1} over H and W, >= 16 channels on both sides: 16 products per
 * 2x2 output tile and depth tap instead of 36) or F(2x2,2x2) (stride-2 four-tap transposed
 * taps over H and W, >= 64 channels, no dbias: 9 instead of 16).  The same route decision
 * sizes rehr_wgrad_workspace_bytes and drives the launch.                              */
int rehr_wgrad_uses_winograd(const rehr_wgrad_desc* d);
int rehr_wgrad_f32(const rehr_wgrad_desc* d, void* stream);

/* out[t][a][b] = in[a][b][t] (transpose_ab = 0) or in[b][a][t] (1); rows
 * a >= A are written as zero up to Apad.  Turns the (Cout,Cin,kD,kH,kW)
 * parameter layout of torch.nn.Conv3d / the (Cin,Cout,...) layout of
 * ConvTranspose3d into wp[tap][Npad][Cin].                                   */
int rehr_pack_weights_f32(const float* in, float* out, int32_t A, int32_t Apad,
                          int32_t B, int32_t T, int32_t transpose_ab,
                          void* stream);

/* ------------------------------------------------------------------------- *
 * Direct convolution for Cin in {1,2} -> Cout in {16,32,64} (HBM bound, no
 * MFMA): the stem Conv3d (3,7,7)/(1,2,2) of models/FLAVR/resnet_3D.py:47-48
 * and the first nnU-Net conv.  Weights stay in the torch parameter layout
 * (Cout,Cin,kD,kH,kW); x/y are NDHWC.  The input of these layers is the
 * network input, so no input gradient exists.
 * ------------------------------------------------------------------------- */
typedef struct {
  const float* x;
  int32_t ldx, N, Di, Hi, Wi, Cin;
  const float* w;                  /* (Cout,Cin,KD,KH,KW) */
  const float* bias;               /* NULL or [Cout] */
  float* y;                        /* forward: output; wgrad: dY (read) */
  int32_t ldy, Do, Ho, Wo, Cout;
  int32_t KD, KH, KW, sd, sh, sw, pd, ph, pw;
  int32_t act;
  float slope;
  double* stats;
  int32_t stats_mode;
} rehr_direct_conv_desc;

int rehr_conv_small_cin_fwd_f32(const rehr_direct_conv_desc* d, void* stream);
/* out[n,o][k], k = ci*T + tap (order of the (Cin,kD,kH,kW) weight), zero for
 * k >= Cin*T and in the padding; Kpad % 32 == 0.  The weight gradient of the thin
 * conv is then rehr_wgrad_f32 with l = dY, g = out (1x1x1 taps) on the MFMA path. */
int rehr_im2col_f32(const rehr_direct_conv_desc* d, float* out, int32_t Kpad,
                    void* stream);
int64_t rehr_conv_small_cin_wgrad_workspace_bytes(const rehr_direct_conv_desc* d);
/* 1 when rehr_conv_small_cin_wgrad_f32 takes this shape on the matrix cores (thin_cin_conv.hip: C_out 32 / 64,
 * 1x3x3 / 3x3x3 / (3,7,7) taps, stride_w <= 2) -- dY and x are then each read once, no im2col columns */
int rehr_conv_small_cin_wgrad_on_mfma(const rehr_direct_conv_desc* d);
/* 1 when rehr_conv_small_cin_fwd_f32 takes this shape on the matrix cores, which is when rehr_conv_small_cin_fwd_ybf16
 * takes it at all (C_out 32 / 64, kW <= 8, stride_w <= 2, weights and patch within 150 KB of LDS).  A question about
 * the shape, to be asked before y is allocated: x, w and y may be null; a y that is given is held to the alignment of
 * bf16 elements (8 bytes).  (ABI 6) */
int rehr_conv_small_cin_fwd_on_mfma(const rehr_direct_conv_desc* d);
/* Mixed precision: the same layers with y (forward) / dY (weight gradient) pointing at bf16 elements -- the thin-input
 * layers compute in fp32 on the fp32 image, the layer behind takes bf16.  Matrix-core shapes only
 * (rehr_conv_small_cin_wgrad_on_mfma; C_out 32 / 64, kW <= 8, stride_w <= 2 for the forward), else REHR_ENOSUP.
 * Same workspace query as the fp32 entry. */
int rehr_conv_small_cin_fwd_ybf16(const rehr_direct_conv_desc* d, void* stream);
int rehr_conv_small_cin_wgrad_dybf16(const rehr_direct_conv_desc* d, float* dw, float* dbias, float* workspace,
                                     int64_t workspace_bytes, void* stream);
/* dw (Cout,Cin,KD,KH,KW) = sum_{n,o} dY[n,o,co] * x[n,o*s-p+k,ci]; dbias optional */
int rehr_conv_small_cin_wgrad_f32(const rehr_direct_conv_desc* d, float* dw,
                                  float* dbias, float* workspace,
                                  int64_t workspace_bytes, void* stream);

/* Direct convolution for Cout <= 4, Cin % 16 == 0, stride 1, kW <= 7 (HBM/VALU
 * bound): the 1x1x1 segmentation layer (models/seg_model.py:42-44) and sr_head's
 * 5x5x5 16->num_classes conv (models/seg_model.py:199), with both gradients.
 * Same descriptor; `y` is the output (forward) or dY (gradients).              */
int rehr_conv_small_cout_fwd_f32(const rehr_direct_conv_desc* d, void* stream);
int rehr_conv_small_cout_dgrad_f32(const rehr_direct_conv_desc* d, float* dx,
                                   void* stream);
int64_t rehr_conv_small_cout_wgrad_workspace_bytes(const rehr_direct_conv_desc* d);
int rehr_conv_small_cout_wgrad_f32(const rehr_direct_conv_desc* d, float* dw,
                                   float* dbias, float* workspace,
                                   int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * SEGating (models/FLAVR/resnet_3D.py:100-116) and its fused neighbours.
 *   gate[n][c] = sigmoid( b[c] + sum_k W[c][k] * stats[n][k][0] / S )
 *   y = act( x * gate[n][c] + res )      (res optional: BasicBlock :144-149;
 *                                         act lrelu(0.2): FLAVR_arch.py:188-200)
 * ------------------------------------------------------------------------- */
int rehr_se_gate_fwd_f32(const double* stats, const float* w, const float* b,
                         float* gate, float* mean, int32_t N, int32_t C,
                         int64_t S, void* stream);
int rehr_scale_res_act_fwd_f32(const float* x, int32_t ldx, const float* gate,
                               const float* res, int32_t ldr, float* y,
                               int32_t ldy, int32_t N, int64_t S, int32_t C,
                               int32_t act, float slope, void* stream);
/* dz = dy * act'(y); dres = dz (optional); dx = dz * gate;
 * dgate_acc[n][c] += sum_s dz * x   (double)                                 */
int rehr_scale_res_act_bwd_f32(const float* dy, int32_t lddy, const float* y,
                               int32_t ldy, const float* x, int32_t ldx,
                               const float* gate, float* dx, int32_t lddx,
                               float* dres, int32_t lddr, double* dgate_acc,
                               int32_t N, int64_t S, int32_t C, int32_t act,
                               float slope, void* stream);
/* From dgate_acc: ds = dgate*g*(1-g); dW += ds (x) mean; db += ds;
 * kconst[n][c] = (W^T ds)[c] / S.                                             */
int rehr_se_gate_bwd_f32(const double* dgate_acc, const float* gate,
                         const float* mean, const float* w, float* dw,
                         float* db, float* kconst, int32_t N, int32_t C,
                         int64_t S, void* stream);
/* x[n,s,c] += k[n][c] in place */
int rehr_add_channel_const_f32(float* x, int32_t ldx, const float* k, int32_t N,
                               int64_t S, int32_t C, void* stream);

/* ------------------------------------------------------------------------- *
 * InstanceNorm3d(affine, eps) + LeakyReLU applied to a conv output whose
 * {sum, sum of squares} were accumulated by the conv epilogue
 * (nnU-Net ConvDropoutNormReLU: dynamic_network_architectures==0.3.1, call
 * sites models/seg_model.py:174-191).
 *   mean = s1/S; var = s2/S - mean^2 (biased); rstd = 1/sqrt(var+eps)
 *   y = lrelu( (x-mean)*rstd*gamma + beta )
 * ------------------------------------------------------------------------- */
int rehr_instnorm_act_fwd_f32(const float* x, int32_t ldx, const double* stats,
                              const float* gamma, const float* beta, float* y,
                              int32_t ldy, float* mean_rstd /* [N][C][2] */,
                              int32_t N, int64_t S, int32_t C, float eps,
                              int32_t act, float slope, void* stream);
/* dz = dy*act'(xhat*gamma+beta); dgamma = sum dz*xhat; dbeta = sum dz;
 * dx = rstd*gamma*(dz - mean_s(dz) - xhat*mean_s(dz*xhat)).  `red` is a
 * caller-zeroed [N][C][2] double scratch.                                     */
int rehr_instnorm_act_bwd_f32(const float* dy, int32_t lddy, const float* x,
                              int32_t ldx, const float* mean_rstd,
                              const float* gamma, const float* beta, float* dx,
                              int32_t lddx, float* dgamma, float* dbeta,
                              double* red, int32_t N, int64_t S, int32_t C,
                              int32_t act, float slope, void* stream);

/* ------------------------------------------------------------------------- *
 * Depth-only linear upsample, align_corners=True
 * (F.interpolate(scale_factor=(upscale,1,1), mode='trilinear'),
 * models/seg_model.py:204).  Do = floor(Di*upscale).
 * ------------------------------------------------------------------------- */
int rehr_upsample_depth_fwd_f32(const float* x, float* y, int32_t N, int32_t Di,
                                int32_t Do, int64_t HW, int32_t C, void* stream);
int rehr_upsample_depth_bwd_f32(const float* dy, float* dx, int32_t N,
                                int32_t Di, int32_t Do, int64_t HW, int32_t C,
                                void* stream);

/* Depth upsample fused with the depth-tap sum of the convolution that follows it
 * (models/seg_model.py:204-205: F.interpolate(features, (upscale,1,1), trilinear, align_corners) ->
 * sr_head[0] = Conv3d(32, 16, 3, padding=1) -> ReLU).  Both are linear, so the (kH,kW) part of every
 * depth tap kd is taken on the low-resolution slices first -- g[n][j][hw][kd*C + co], a (1,kH,kW)
 * convolution with KD*C output channels on the ordinary conv path -- and
 *   y[n][d][hw][co] = act(bias[co] + sum_kd [0 <= u < Do] ((1-t) g[n][i0][hw][kd*C+co] + t g[n][i1][..])),
 *   u = d + kd - pd, (i0, i1, t) = align_corners source of upsampled slice u.
 * bwd: dg from dz = dy * act'(y), formed on the fly from dy and the saved output y.  C % 4 == 0.    */
int rehr_upmix_depth_fwd_f32(const float* g, const float* bias, float* y, int32_t N,
                             int32_t Di, int32_t Do, int64_t HW, int32_t C, int32_t KD,
                             int32_t pd, int32_t act, float slope, void* stream);
int rehr_upmix_depth_bwd_f32(const float* dy, const float* y, float* dg, int32_t N,
                             int32_t Di, int32_t Do, int64_t HW, int32_t C, int32_t KD,
                             int32_t pd, int32_t act, float slope, void* stream);
/* out[c] = sum over rows of dy[row][c] * act'(y[row][c]): the bias gradient behind a fused activation */
int rehr_channel_sum_actgrad_f32(const float* dy, const float* y, int32_t ld, int64_t rows,
                                 int32_t C, int32_t act, float slope, float* out,
                                 double* scratch, void* stream);

/* cosine_distance_loss (models/seg_model.py:60-78) on two (N, 64, D, H, W) NDHWC tensors, S = D*H*W:
 * stats[n][c] = (S12, S11, S22) of the per-voxel channel-normalised tensors (fp64, zeroed by the call);
 * loss = mean_{n,c}(1 - S12 / (max(sqrt(S11), 1e-8) * max(sqrt(S22), 1e-8))) is three lines of host code.
 * bwd: gradient w.r.t. x1 only (x2 = the frozen teacher), scale = -dloss / (N*C).                   */
int rehr_cosdist_stats_f32(const float* x1, const float* x2, double* stats, int32_t N,
                           int64_t S, int32_t C, void* stream);
int rehr_cosdist_bwd_f32(const float* x1, const float* x2, const double* stats, float* dx1,
                         int32_t N, int64_t S, int32_t C, float scale, void* stream);

/* UASR head of UNet_3D_3D(use_uncertainty=True) (reference models/FLAVR/FLAVR_arch.py:203-246): per output voxel the
 * K candidate (image, segmentation) pairs are blended with softmax weights, and the weights give the uncertainty:
 *   s = softmax_i ue_i;  out0 = sum_i s_i (tanh(om_2i) + 1)/2;  out1 = sum_i s_i om_{2i+1};
 *   unc = sigmoid(bu + sum_i s_i wu_i)                      (uncertainty_out = Conv3d(K, 1, 1), :151,245)
 * om [n][hw][d*2K + c], ue [n][hw][d*K + i]: the NDHWC outputs of feature_fuse1 / uncertainty_early on the fused
 * slice (the split(dim=1) + stack(dim=2) of :205-211 is this indexing); out (N,2,D,H,W) and unc (N,1,D,H,W) NCDHW.
 * K in {4, 8, 16, 32}; om, ue (dom, due) 16-byte aligned.
 * bwd: dom, due from (gout, gunc) with the softmax recomputed; partial[blocks][K+1] (double) holds per-block sums of
 * (dwu[0..K), dbu) -- blocks = rehr_uasr_mix_blocks(N, D, HW); the host adds them.                       */
int32_t rehr_uasr_mix_blocks(int32_t N, int32_t D, int64_t HW);
int rehr_uasr_mix_fwd_f32(const float* om, const float* ue, const float* wu, const float* bu, float* out,
                          float* unc, int32_t N, int32_t K, int32_t D, int64_t HW, void* stream);
int rehr_uasr_mix_bwd_f32(const float* om, const float* ue, const float* wu, const float* bu,
                          const float* gout, const float* gunc, float* dom, float* due, double* partial,
                          int32_t N, int32_t K, int32_t D, int64_t HW, void* stream);

/* Max-pool of every (sample, depth) slice with a (H/2, W/2) window and stride: the 2x2 summary per slice and
 * channel that Distiller's structure loss compares (CriterionPairWiseforWholeFeatAfterPool,
 * models/seg_model.py:95-113; MaxPool2d(ceil_mode=True) with even H, W).  x [slices][H][W][C] (NDHWC slices),
 * y [slices][2][2][C], idx = row-major position of the first maximum inside its slice (for the backward).
 * A NaN in a window is its result (the last one, as in ATen's scan), and idx points at it.  Any C >= 1.
 * bwd: dx is zero-filled, then dx[slice][idx][c] = dy[slice][q][c].                                          */
int rehr_quad_maxpool_fwd_f32(const float* x, float* y, int32_t* idx, int64_t slices,
                              int32_t H, int32_t W, int32_t C, void* stream);
int rehr_quad_maxpool_bwd_f32(const float* dy, const int32_t* idx, float* dx, int64_t slices,
                              int32_t H, int32_t W, int32_t C, void* stream);

/* Stem of the distillation teacher's overlapping 4-slice windows (get_intermediate_features,
 * train_all.py:85-112 -> UNet_3D_3D.forward's mean subtraction FLAVR_arch.py:181 -> BasicStem
 * resnet_3D.py:42-50).  g0..g2 = the (1,kH,kW) part of the stem's three depth taps on every slice of the
 * depth-padded volume (B*nslices slices, NHWC) followed by one more "slice": the response to a
 * constant 1 in channel 0.  y[b*nwin + w][k][hw][c] = act(bias[c] + sum over the taps kd that stay inside
 * the window (0 <= k+kd-1 <= 3) of g[kd][b*nslices + w + k+kd-1] - mean[b*nwin + w] * g[kd][B*nslices]).
 * nslices = nwin + 3.  No gradient (the teacher is frozen).                                           */
int rehr_window_stem_assemble_f32(const float* g0, const float* g1, const float* g2,
                                  const float* mean, const float* bias, float* y, int32_t B,
                                  int32_t nwin, int32_t nslices, int64_t HW, int32_t C,
                                  int32_t act, float slope, void* stream);
/* the same with a bf16 result (mixed precision: the teacher's first block takes bf16); fp32 responses in */
int rehr_window_stem_assemble_bf16(const float* g0, const float* g1, const float* g2,
                                   const float* mean, const float* bias, void* y, int32_t B,
                                   int32_t nwin, int32_t nslices, int64_t HW, int32_t C,
                                   int32_t act, float slope, void* stream);

/* ------------------------------------------------------------------------- *
 * Fused segmentation loss: softmax + cross-entropy, optionally
 * weighted by the uncertainty map with the reference's (B,D,H,W)*(B,1,D,H,W)
 * broadcast, + nnU-Net soft Dice, one pass over the logits each way.
 * Replaces utils/seg_utils.py:289-304 (RobustCrossEntropyLoss), :306-351
 * (DC_and_weighted_CE_loss) and nnunetv2 MemoryEfficientSoftDiceLoss behind them.
 *   logits [N][S][ld] (NDHWC, C <= ld, 2 <= C <= 4, N <= 4), target [N][S] float class
 *   ids, unc NULL or [N][S].  fwd fills stats[N*C*3 + 1] = {I,P,G per (n,c); sum of
 *   (sum_b ce)*(sum_a unc) or sum of ce}; the caller forms the scalar
 *     w_ce * stats[last] / (unc ? N*N*S : N*S)
 *       - w_dice * mean_{n, c >= !do_bg} (2I+smooth)/max(G+P+smooth, 1e-8).
 *   bwd writes dlogits[N][S][ldd] = *grad_out * d(loss)/d(logits).
 * ------------------------------------------------------------------------- */
int rehr_seg_loss_fwd_f32(const float* logits, int32_t ld, const float* target, const float* unc,
                          int32_t N, int32_t C, int64_t S, double* stats, void* stream);
int rehr_seg_loss_bwd_f32(const float* logits, int32_t ld, const float* target, const float* unc,
                          int32_t N, int32_t C, int64_t S, const double* stats, float w_ce,
                          float w_dice, float smooth, int32_t do_bg, const float* grad_out,
                          float* dlogits, int32_t ldd, void* stream);

/* ------------------------------------------------------------------------- *
 * Top-k cross-entropy + soft Dice (nnU-Net's DC_and_topk_loss): the CE
 * term of the loss above replaced by the mean of the K largest elements of the loss map
 * m that RobustCrossEntropyLoss forms before its mean: m[b][v] = ce, M = N*S elements,
 * or with unc m[a][b][v] = ce[b][v]*unc[a][v], M = N*N*S.  Operands as
 * rehr_seg_loss_*_f32 with N <= 4 and M <= 2^30; K is a host integer in [1, M].
 *   fwd: one pass over the logits writes m into the workspace next to the Dice
 *        statistics, rehr_order_stats_f32 selects t = the K-th largest element, one pass
 *        over m counts.  stats[N*C*3 + 5] = {I,P,G per (n,c); the plain CE sum as above;
 *        n_gt = #(m > t); n_eq = #(m == t); sum of m > t; t}.  t, n_gt and n_eq are the
 *        same bits on every run; a NaN in m makes t NaN.  The caller forms
 *          w_ce * (sum + (K - n_gt) * t) / K - w_dice * (the Dice mean as above).
 *        Eleven launches and one memset, nothing read back.
 *   bwd: one pass; an element of m carries weight 1 above t, (K - n_gt)/n_eq on t (zeros
 *        of either sign are one value), 0 below, and
 *          dlogits[b][v][c] = *grad_out * (w_ce/K * (sum_a weight(m[a][b][v]) * unc[a][v])
 *                             * (softmax_c - onehot_c) + the Dice part as above).
 *        `workspace` and `stats` are the forward's, unchanged.
 * EINVAL: a null pointer (unc may be null), N or S < 1, K outside [1, M], ld / ldd < C,
 * a workspace that is no multiple of 16 bytes off or smaller than the query's answer;
 * ENOSUP: C outside 2..4, N > 4, M > 2^30.  All of them before any launch.
 * ------------------------------------------------------------------------- */
int64_t rehr_seg_topk_workspace_bytes(int32_t N, int32_t C, int64_t S, int32_t with_unc);
int rehr_seg_topk_fwd_f32(const float* logits, int32_t ld, const float* target, const float* unc,
                          int32_t N, int32_t C, int64_t S, int64_t K, double* stats, void* workspace,
                          int64_t workspace_bytes, void* stream);
int rehr_seg_topk_bwd_f32(const float* logits, int32_t ld, const float* target, const float* unc,
                          int32_t N, int32_t C, int64_t S, int64_t K, const double* stats,
                          const void* workspace, int64_t workspace_bytes, float w_ce, float w_dice,
                          float smooth, int32_t do_bg, const float* grad_out, float* dlogits,
                          int32_t ldd, void* stream);

/* ------------------------------------------------------------------------- *
 * Deep supervision (nnU-Net's DeepSupervisionWrapper over the loss above, and
 * DownsampleSegForDSTransform2 in front of it; utils/seg_utils.py:363-371, :723-725).
 *
 * rehr_seg_loss_ds_{fwd,bwd}_f32: the arithmetic of rehr_seg_loss_{fwd,bwd}_f32 over up
 * to REHR_DS_MAX_LEVELS output levels of one network in ONE launch each way.  `levels`
 * is a HOST array (copied into the kernel arguments; the library assigns every level
 * its own range of blocks).  All levels share N and C.  A level with weight == 0 is
 * skipped: it gets no blocks, its pointers are not read and nothing is written for it.
 *   fwd: stats[n_levels][N*C*3 + 1], zeroed inside by one memset, one row per level laid
 *        out as the single-level stats; the caller forms sum_l weight_l * loss_l.
 *   bwd: dlogits_l[N][S][ldd] = *grad_out * weight_l * d(loss_l)/d(logits_l).
 * EINVAL: n_levels outside 1..8, a null pointer of a non-skipped level, S != d*h*w,
 * ld / ldd < C, no level with a weight; ENOSUP: C outside 2..4.
 *
 * rehr_label_pyramid_f32: every level of the label pyramid of one source volume
 * src[B][z][y][x] in ONE launch: dst_l[b][k][j][i] = src[b][iz_l[k]][iy_l[j]][ix_l[i]]
 * (order-0 resize per axis; a pure gather, the same entry point serves the labels and
 * the uncertainty map).  iz / iy / ix are DEVICE int32 tables of d / h / w entries whose
 * values the caller guarantees to lie inside the source axis.
 * ------------------------------------------------------------------------- */
#define REHR_DS_MAX_LEVELS 8
typedef struct {
  const float* logits;   /* [N][S][ld] (NDHWC) */
  const float* target;   /* [N][S] float class ids */
  const float* unc;      /* NULL or [N][S] */
  float* dlogits;        /* bwd only: [N][S][ldd] */
  int64_t S;             /* d * h * w */
  int32_t d, h, w;
  int32_t ld, ldd;
  float weight;          /* 0: the level is skipped */
} rehr_seg_ds_level;
int rehr_seg_loss_ds_fwd_f32(const rehr_seg_ds_level* levels, int32_t n_levels, int32_t N, int32_t C,
                             double* stats, void* stream);
int rehr_seg_loss_ds_bwd_f32(const rehr_seg_ds_level* levels, int32_t n_levels, int32_t N, int32_t C,
                             const double* stats, float w_ce, float w_dice, float smooth, int32_t do_bg,
                             const float* grad_out, void* stream);
typedef struct {
  float* dst;                     /* [B][d][h][w] */
  int32_t d, h, w;
  const int32_t *iz, *iy, *ix;    /* device tables: source index of every output index, per axis */
} rehr_pyramid_level;
int rehr_label_pyramid_f32(const float* src, int32_t B, int32_t z, int32_t y, int32_t x,
                           const rehr_pyramid_level* levels, int32_t n_levels, void* stream);

/* Elementwise helpers used by the blocks above. */
int rehr_act_fwd_f32(const float* x, float* y, int64_t n, int32_t act,
                     float slope, void* stream);
int rehr_act_bwd_f32(const float* dy, const float* y, float* dx, int64_t n,
                     int32_t act, float slope, void* stream);
/* out[c] (+)= sum over rows of x[row*ld + c], rows = N*S (bias gradient).     */
int rehr_channel_sum_f32(const float* x, int32_t ldx, int64_t rows, int32_t C,
                         float* out, int32_t accumulate, double* scratch,
                         void* stream);
/* strided channel-slice copy: y[row*ldy + c] = x[row*ldx + c], c < C          */
int rehr_copy_channels_f32(const float* x, int32_t ldx, float* y, int32_t ldy,
                           int64_t rows, int32_t C, void* stream);
/* NCDHW <-> NDHWC for API-edge tensors                                        */
int rehr_nchw_to_nhwc_f32(const float* x, float* y, int32_t N, int32_t C,
                          int64_t S, void* stream);
int rehr_nhwc_to_nchw_f32(const float* x, float* y, int32_t N, int32_t C,
                          int64_t S, void* stream);

/* BCE-with-logits + Dice of the SR stage's segmentation channel in one pass each way: utils/seg_utils.py:786-885
 * (BCEDiceLoss: alpha * BCEWithLogitsLoss + beta * (1 - mean_c 2 sum(p t) / clamp(sum p^2 + sum t^2, 1e-6)), p = sigmoid(x),
 * sums per channel over batch and space; called from train_sr, train_all.py:134).  x, t dense [N][C][S] fp32;
 * stats[C][4] double = {sum bce, sum p t, sum p^2, sum t^2} (zeroed inside); loss = alpha * sum_c bce / (N C S) +
 * beta * (1 - mean_c dice_c) is formed by the caller; grad_out = device scalar. */
int rehr_bce_dice_fwd_f32(const float* x, const float* t, int32_t N, int32_t C, int64_t S, double* stats, void* stream);
int rehr_bce_dice_bwd_f32(const float* x, const float* t, int32_t N, int32_t C, int64_t S, const double* stats,
                          float alpha, float beta, const float* grad_out, float* dx, void* stream);

/* ------------------------------------------------------------------------- *
 * sr_head.2 of the segmentation model -- Conv3d(16 -> 2, 5x5x5, stride 1, pad 2) on the depth-upsampled features,
 * models/seg_model.py:199, :205 -- on the bf16 matrix cores (mixed-precision path, BASELINE.json configs[4]).
 * Same descriptor as the rehr_conv_small_cout_* entry points with `x` addressing bf16 elements (ldx % 8 == 0),
 * weights / bias fp32 in the torch layout, y (forward output, or dY for the gradients) fp32 NDHWC.
 * Supported: Cin 16, Cout 2, 5x5x5, stride 1, pad 2, Wi % 32 == 0, 32 <= Wi <= 160 (rehr_conv5_thin_supported);
 * anything else returns REHR_ENOSUP.  `workspace`: rehr_conv5_thin_workspace_bytes(d) bytes of device scratch
 * (repacked weights; the weight-gradient partial sums).
 * ------------------------------------------------------------------------- */
int64_t rehr_conv5_thin_workspace_bytes(const rehr_direct_conv_desc* d);  /* < 0: REHR_E* */
int rehr_conv5_thin_supported(const rehr_direct_conv_desc* d);
int rehr_conv5_thin_fwd_bf16(const rehr_direct_conv_desc* d, void* workspace, int64_t workspace_bytes, void* stream);
/* dx (bf16 NDHWC, lddx % 4 == 0) = input gradient of the layer from dY = d->y (fp32) */
int rehr_conv5_thin_dgrad_bf16(const rehr_direct_conv_desc* d, void* dx, int32_t lddx, void* workspace,
                               int64_t workspace_bytes, void* stream);
/* dw (2,16,5,5,5) fp32 = weight gradient from x = d->x (bf16) and dY = d->y (fp32), dbias (NULL or [2]) = column sums
 * of dY; partial sums per block in the workspace, combined in a fixed order (bitwise reproducible). */
int rehr_conv5_thin_wgrad_bf16(const rehr_direct_conv_desc* d, float* dw, float* dbias, void* workspace,
                               int64_t workspace_bytes, void* stream);

/* The same layer on the fp32 matrix cores (v_mfma_f32_16x16x4_f32) for the fp32 path: x, dx fp32 (ldx, lddx % 4 == 0),
 * Wi % 32 == 0, 32 <= Wi <= 128; same descriptor, same workspace protocol (rehr_conv5_thin_f32_workspace_bytes).
 * Replaces rehr_conv_small_cout_{fwd,dgrad,wgrad}_f32 for sr_head.2 where the shape qualifies. */
int64_t rehr_conv5_thin_f32_workspace_bytes(const rehr_direct_conv_desc* d);
int rehr_conv5_thin_f32_supported(const rehr_direct_conv_desc* d);
int rehr_conv5_thin_fwd_f32(const rehr_direct_conv_desc* d, void* workspace, int64_t workspace_bytes, void* stream);
int rehr_conv5_thin_dgrad_f32(const rehr_direct_conv_desc* d, float* dx, int32_t lddx, void* workspace,
                              int64_t workspace_bytes, void* stream);
int rehr_conv5_thin_wgrad_f32(const rehr_direct_conv_desc* d, float* dw, float* dbias, void* workspace,
                              int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Training-patch feed from HBM-resident volumes.
 * Replaces the host-side numpy chain of utils/train_set.py:100-160 (TrainSetMultipleSegSREfficient.__getitem__),
 * :205-224 (TrainSetMultipleSegSR.__getitem__) and :330-434 (TrainSetMultiple.__getitem__): transposition, crop,
 * constant pad (utils/pad.py:14-21), flips, every-k-th slice, astype(float32), transpose / permute.
 *   out[item][o0][o1][o2][o3] = ((lo[k] <= o_k < hi[k] for every k) ? src[base + sum_k o_k * stride[k]] : 0) * scale + bias
 * `items` is a HOST array of n_items descriptors (copied into the kernel arguments, REHR_PATCH_MAX_ITEMS per launch);
 * src / dst are device pointers; strides and base count source elements and may be negative (flips).
 * ------------------------------------------------------------------------- */
#define REHR_PATCH_F32 0
#define REHR_PATCH_U8 1
#define REHR_PATCH_MAX_ITEMS 16
typedef struct {
  const void* src;      /* volume (device), fp32 or uint8 elements */
  int64_t base;         /* element offset of output index (0,0,0,0) */
  int64_t stride[4];    /* source elements per step of each output axis */
  int32_t lo[4], hi[4]; /* output indices outside [lo, hi) read as 0 (the constant pad) */
} rehr_patch_item;
typedef struct {
  int32_t n_items;
  int32_t dims[4];         /* output extent of one item */
  int32_t src_dtype;       /* REHR_PATCH_F32 / REHR_PATCH_U8 */
  float scale, bias;       /* applied after the pad (uncertainty maps: utils/train_set.py:147) */
  float* dst;              /* [n_items][dst_item_stride], fp32 */
  int64_t dst_item_stride; /* >= prod(dims) */
} rehr_patch_gather_desc;
int rehr_patch_gather(const rehr_patch_gather_desc* d, const rehr_patch_item* items, void* stream);

/* 1-D weighted gather along one axis: dst[o][j][i] = sum_t w[j][t] * src[o][idx[j][t]][i] (idx < 0: term dropped).
 * Serves the slice-profile blur (utils/train_set.py:306-318: F.conv2d with the (L,1) kernel of
 * utils/blur_kernel_ops.py:7-18, padding="same") and the 1-D down-sampling of the LR simulation (:403-404).
 * src [outer][n_in][inner], dst [outer][n_out][inner] dense fp32; idx / w [n_out][taps] on the device. */
int rehr_axis_resample_f32(const float* src, float* dst, const int32_t* idx, const float* w, int64_t outer,
                           int32_t n_in, int32_t n_out, int64_t inner, int32_t taps, void* stream);

/* ------------------------------------------------------------------------- *
 * nnU-Net training augmentation on the device (utils/seg_utils.py:632-728 get_training_transforms as REHRSeg calls
 * it; rehrseg_amd/utils/augment.py builds the chain).  Batches are dense fp32 [B][...]; per-item parameter records
 * (fp64) and statistics live in device memory, drawn and uploaded by the host once per batch.
 * ------------------------------------------------------------------------- */
#define REHR_AUG_WARP_SPLINE3 0 /* order-3 B-spline over prefiltered coefficients, cval 0 (data, uncertainty) */
#define REHR_AUG_WARP_LABEL 1   /* batchgenerators interpolate_img(is_seg=True, order=1, cval=-1): label vote */
#define REHR_AUG_WARP_PARAMS 8  /* doubles per item: R00 R01 R10 R11 scale ctr0 ctr1 (unused) */
/* dst[b][c][i][j] = sample of src[b][c] (Hi x Wi) at ((p R) * scale + ctr) with p = (i - (Ho-1)/2, j - (Wo-1)/2):
 * MySpatialTransform (dim 2, no elastic deformation) of every depth slice c with the coordinates of item b. */
int rehr_aug_warp2d_f32(const float* src, float* dst, const double* params, int32_t B, int32_t C, int32_t Hi,
                        int32_t Wi, int32_t Ho, int32_t Wo, int32_t mode, void* stream);
/* stats[b] = {sum, sum of squares, min, max} of x[b][0..S) (fp64); work holds B * REHR_AUG_STAT_PARTS * 4 doubles. */
#define REHR_AUG_STAT_PARTS 256
int rehr_aug_stats_f32(const float* x, int32_t B, int64_t S, double* work, double* stats, void* stream);
/* One intensity step in place over x[b][0..S); params[b][REHR_AUG_PW_PARAMS] = {fires (0: item untouched), a, b, c}:
 *   NOISE     {1, std, seed}: x += std * N(0, 1) from a counter-based generator of (seed, index)
 *   SCALE     {1, m}: x *= m
 *   CONTRAST  {1, f}, stats0 of x: x = clip((x - mean) * f + mean, min, max)
 *   CLIP      {1}, stats0: x = clip(x, min, max)
 *   GAMMA     {1, g, s}, stats0 of x: x' = s x, x = ((x' - min') / (rng' + 1e-7))^g * (rng' + 1e-7) + min'
 *   RETAIN    {1, -, s}, stats0 of x before GAMMA, stats1 of x after it: x = s ((x - mean1) / (sd1 + 1e-8) * sd0' + mean0') */
#define REHR_AUG_PW_PARAMS 4
#define REHR_AUG_NOISE 0
#define REHR_AUG_SCALE 1
#define REHR_AUG_CONTRAST 2
#define REHR_AUG_CLIP 3
#define REHR_AUG_GAMMA 4
#define REHR_AUG_RETAIN 5
int rehr_aug_pointwise_f32(float* x, int32_t B, int64_t S, int32_t op, const double* params, const double* stats0,
                           const double* stats1, void* stream);

/* ------------------------------------------------------------------------- *
 * Stage-2 validation on the device (utils/seg_utils.py:240-287 tiled predictor with mirror TTA, :736-784
 * evaluate_case; rehrseg_amd/utils/seg_utils.py drives them).  fp16 accumulators as the reference's; every rounding
 * equals torch's on the same operands (csrc/seg_eval.hip).
 * ------------------------------------------------------------------------- */
/* out (8, 1, d, h, w) fp32 = the tile at (start_d, start_h, start_w) of the volume vol (D, H, W) constant-padded by
 * (pad_d, pad_h, pad_w) voxels below (zeros outside vol), as the identity then the mirrorings of the axes
 * (d), (h), (w), (d,h), (d,w), (h,w), (d,h,w). */
int rehr_tta_gather_f32(const float* vol, float* out, int32_t D, int32_t H, int32_t W, int32_t pad_d, int32_t pad_h,
                        int32_t pad_w, int32_t start_d, int32_t start_h, int32_t start_w, int32_t d, int32_t h,
                        int32_t w, void* stream);
/* pred: fp32 (8, C, d, h, w) with element strides[5] (any layout, >= 0).  For every voxel of the tile and every c:
 * p = ((pred[0] + unflip(pred[1])) + ...) + unflip(pred[7]), p = p / 8, logits[c][od+i][oh+j][ow+k] += p * g and
 * counts[od+i][oh+j][ow+k] += g in fp32, each rounded once to fp16; g = gaussian[i][j][k] (fp16 (d, h, w)), or 1 when
 * gaussian is NULL.  logits: fp16 [C][Do][Ho][Wo], counts: fp16 [Do][Ho][Wo]. */
int rehr_tta_blend_f16acc(const float* pred, const int64_t* strides, int32_t C, int32_t d, int32_t h, int32_t w,
                          const void* gaussian, void* logits, void* counts, int32_t Do, int32_t Ho, int32_t Wo,
                          int32_t od, int32_t oh, int32_t ow, void* stream);
/* logits fp16 [2][D][H][W] /= counts fp16 [D][H][W] in place (fp32 quotient rounded to fp16); stats[0] is set to 1 if
 * any quotient is +-inf.  labels (NULL: skipped) [CD][CH][CW] uint8 = argmax over the 2 classes (ties: class 0) inside
 * the crop at (crop_d, crop_h, crop_w); with gt (uint8, the crop's shape) stats[1..3] += sum(p * gt), sum(p), sum(gt).
 * stats: 4 uint64, zeroed by the caller. */
int rehr_seg_eval_finalize_f16(void* logits, const void* counts, int32_t D, int32_t H, int32_t W, int32_t crop_d,
                               int32_t crop_h, int32_t crop_w, int32_t CD, int32_t CH, int32_t CW, uint8_t* labels,
                               const uint8_t* gt, uint64_t* stats, void* stream);

/* ------------------------------------------------------------------------- *
 * Stage-2 validation, boundary metrics in physical units (csrc/seg_surface.hip): the Hausdorff distance,
 * its 95th percentile and the average symmetric surface distance of two label maps (D, H, W), non-zero = foreground.
 * A surface voxel is a foreground voxel with a background face neighbour (outside the volume is background); the
 * distance of two voxels is sqrt(((dz) sd)^2 + ((dy) sh)^2 + ((dx) sw)^2), each term fl(fl((float)d * s)^2), summed
 * w + h first, then + d, in fp32, then sqrtf.  Every axis <= REHR_SEG_SURFACE_MAX_AXIS and D * H * W <= 2^30
 * (REHR_ENOSUP above); extents < 1, a null pointer, a spacing that is not finite and positive, a misaligned or too
 * small workspace: REHR_EINVAL, before any launch.
 * ------------------------------------------------------------------------- */
#define REHR_SEG_SURFACE_MAX_AXIS 2048
/* Bytes of the workspace of rehr_seg_surface_dist_f32 (rehr_seg_surface_reduce_f64 needs no more), or the error code. */
int64_t rehr_seg_surface_workspace_bytes(int32_t D, int32_t H, int32_t W);
/* dist: fp32 [2][D * H * W]; dist[0][v] = the distance of voxel v to the nearest surface voxel of gt where v is a
 * surface voxel of pred, dist[1][v] = to the nearest surface voxel of pred where v is one of gt, +inf at every other
 * voxel (and everywhere in a row whose target surface is empty).  counts[0] += the surface voxels of pred,
 * counts[1] += of gt: 2 uint64, zeroed by the caller.  workspace: 16-byte aligned. */
int rehr_seg_surface_dist_f32(const uint8_t* pred, const uint8_t* gt, int32_t D, int32_t H, int32_t W, float sd,
                              float sh, float sw, float* dist, uint64_t* counts, void* workspace,
                              int64_t workspace_bytes, void* stream);
/* out[3] = {hd, hd95, assd} (fp64) from dist (as written above, N = D * H * W), `sorted` = the 2 N values of dist in
 * ascending order and the two counts, all read on the device: with n = counts[0] + counts[1], hd = sorted[n - 1],
 * hd95 = numpy.percentile(sorted[0..n), 95) (linear: h = 0.95 (n - 1), numpy's lerp of sorted[floor h] and the next),
 * assd = (sum dist[0] / counts[0] + sum dist[1] / counts[1]) / 2 over the finite entries, summed in fp64 in a fixed
 * order.  All three are NaN when a count is 0.  workspace: 8-byte aligned, at least 4096 bytes. */
int rehr_seg_surface_reduce_f64(const float* dist, const float* sorted, const uint64_t* counts, int64_t N, double* out,
                                void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Stage-2 validation, connected components and lesion-wise scores (csrc/seg_components.hip).  A mask is
 * uint8 (D, H, W), contiguous, non-zero = foreground; connectivity 6, 18 or 26 = face, + edge, + corner neighbours
 * (scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3)); outside the volume is background and nothing wraps around
 * a row or a slice.  Every axis >= 1 and D * H * W <= 2^30, anything else REHR_ENOSUP; a null pointer, another
 * connectivity, a misaligned or too small workspace: REHR_EINVAL; all before any launch.  Every call is a fixed number
 * of launches and reads nothing back.
 * ------------------------------------------------------------------------- */
/* Bytes of the workspace of the two calls below (64 + 16 per voxel), or the error code. */
int64_t rehr_seg_cc_workspace_bytes(int32_t D, int32_t H, int32_t W);
/* roots[v] = the smallest linear index (d * H + h) * W + w of any voxel of v's component, -1 at a background voxel:
 * a function of the mask alone, the same bits on every run.  The workspace is checked and not written. */
int rehr_seg_cc_roots_i32(const uint8_t* mask, int32_t D, int32_t H, int32_t W, int32_t connectivity, int32_t* roots,
                          void* workspace, int64_t workspace_bytes, void* stream);
/* out: int64[8], zeroed by the caller, each slot added to: [0] n_pred and [1] n_gt, the numbers of components;
 * [2] tp_pred, predicted components with at least one foreground voxel of gt; [3] tp_gt, the reverse; [4], [5] the
 * voxels of the largest component of pred / gt (among equal sizes the one with the smaller root); [6] the foreground
 * voxels of gt inside that largest component of pred; [7] the foreground voxels of gt.  roots_*: as written above, N
 * words each (a word outside [0, N) counts as background).  workspace: 16-byte aligned, at least 64 + 16 N bytes,
 * overwritten; on return its first two uint64 are the keys (size << 32) | (0xffffffff - root) of the largest
 * component of pred and of gt, 0 for an empty map. */
int rehr_seg_cc_lesion_i64(const int32_t* roots_pred, const int32_t* roots_gt, int64_t N, int64_t* out,
                           void* workspace, int64_t workspace_bytes, void* stream);
/* labels[v] = rank[roots[v]], 0 at background, where rank is the inclusive prefix sum over v of (roots[v] == v) as
 * int32 (the caller's scan): 1..n in the order of the roots.  count: int64[1], zeroed by the caller, += n. */
int rehr_seg_cc_compact_i32(const int32_t* roots, int64_t N, const int32_t* rank, int32_t* labels, int64_t* count,
                            void* stream);

/* ------------------------------------------------------------------------- *
 * Intensity normalisation on the device (utils/seg_utils.py:74-135 percentile_normalization, zeroone_normalization;
 * rehrseg_amd/utils/seg_utils.py drives them, csrc/intensity_norm.hip).  Items are dense runs of S fp32
 * values, item b starting `stride` elements after item b - 1 (4-byte aligned; 16-byte loads where an item start is
 * 16-byte aligned, a scalar head and tail otherwise).  S <= 2^30, B <= 65535, R <= REHR_ORDER_STATS_MAX_RANKS,
 * Q <= REHR_PERCENTILE_MAX_Q: REHR_ENOSUP above; a null pointer, a size < 1, a rank outside [0, S), a misaligned
 * pointer or too small a workspace: REHR_EINVAL; all before any launch.  Every call is a fixed number of launches and
 * reads nothing back.
 * ------------------------------------------------------------------------- */
#define REHR_ORDER_STATS_MAX_RANKS 8
#define REHR_PERCENTILE_MAX_Q 4
/* Bytes of the workspace of rehr_order_stats_f32 (16 per (item, rank), 4 per item, 1024 per (item, rank), each part
 * rounded up to 16), or the error code. */
int64_t rehr_order_stats_workspace_bytes(int32_t B, int32_t R);
/* out[b][r] = sort(x[b][0..S))[ranks[r]]: the exact float, bit for bit the value an ascending sort puts at that index
 * (-0 and +0 are distinct keys here, -0 first; a sort that treats them as equal may leave either).  An item that holds
 * a NaN gets the quiet NaN 0x7fc00000 in every rank; +-inf are ordinary values.  `ranks`: R host integers, read during
 * the call, the same for every item.  MSD radix select on the order-preserving 32-bit key, four digits of 8 bits,
 * integer counts only: the same bits on every run.  workspace: 16-byte aligned, overwritten. */
int rehr_order_stats_f32(const float* x, int32_t B, int64_t S, int64_t item_stride, const int64_t* ranks, int32_t R,
                         float* out, void* workspace, int64_t workspace_bytes, void* stream);
/* out[b][j] (fp64) = numpy.percentile's 'linear' value from stats[b][2 j] = sorted[floor h_j] and stats[b][2 j + 1] =
 * sorted[min(floor h_j + 1, S - 1)] (fp32 [B][2 Q], rehr_order_stats_f32's output) and t[j] = h_j - floor h_j (Q host
 * doubles in [0, 1), h_j = q_j / 100 * (S - 1) formed by the caller): with a, b widened to fp64 and d = b - a,
 * t >= 0.5 ? b - d * (1 - t) : a + d * t, every operation rounded on its own.  With strictly_positive != 0 a negative
 * out[b][0] becomes 0 (_percentile_norm's v_min). */
int rehr_percentile_f64(const float* stats, int32_t B, int32_t Q, const double* t, int32_t strictly_positive,
                        double* out, void* stream);
#define REHR_INTENSITY_PERCENTILE 0 /* y = (min(max(x, lo), hi) - lo) / (hi - lo); a NaN stays a NaN */
#define REHR_INTENSITY_ZEROONE 1    /* y = (x - lo) / (hi - lo) */
/* One streaming pass over x[b][0..S) into y[b][0..S) (strides in elements; y may be x) with lo = (float)bounds[b *
 * bounds_stride], hi = (float)bounds[b * bounds_stride + 1] read on the device (fp64: rehr_percentile_f64's output
 * with stride 2, or the {min, max} of rehr_aug_stats_f32 with stride 4).  IEEE fp32 subtractions and a correctly
 * rounded fp32 division, no reciprocal and no FMA: the bits of the same numpy float32 expression.  hi == lo gives
 * 0 / 0 = NaN, NaN bounds give NaN everywhere. */
int rehr_intensity_apply_f32(const float* x, float* y, int32_t B, int64_t S, int64_t x_stride, int64_t y_stride,
                             int32_t mode, const double* bounds, int64_t bounds_stride, void* stream);

/* ------------------------------------------------------------------------- *
 * Class locations on the device: the voxels a foreground-oversampling patch feed centres its crops on
 * (rehrseg_amd/utils/seg_utils.py sample_class_locations drives it, csrc/class_locations.hip).
 * label: a dense run of N uint8 voxels, 16-byte aligned, only read.  A voxel matches when label == value; value -1:
 * when label != 0.  N <= 2^31 - 1 and R <= 2^20: REHR_ENOSUP above; a null pointer, N < 1, R < 1, a value outside
 * [-1, 255], a misaligned pointer or too small a workspace: REHR_EINVAL; all before any launch.  Three launches,
 * nothing read back, no atomics: the same bits on every run.
 * ------------------------------------------------------------------------- */
/* Bytes of the workspace of rehr_class_locations_u8 (one uint32 per chunk of 4096 voxels, rounded up to 16), or the
 * error code. */
int64_t rehr_class_locations_workspace_bytes(int64_t N);
/* count[0] (int64, 8-byte aligned) = the number of matching voxels.  With rank_j = ((uint64)u[j] * count) >> 32 (u: R
 * device words, 32-bit fractions of the count, 4-byte aligned), index[j] (int32, 4-byte aligned) = the linear index of
 * the rank_j-th matching voxel in ascending order: numpy.flatnonzero(match)[(u.astype(uint64) * count) >> 32].  Every
 * index[j] is -1 when count is 0.  The ranks are formed on the device, so the caller needs no count to draw them.
 * workspace: 16-byte aligned, overwritten. */
int rehr_class_locations_u8(const uint8_t* label, int64_t N, int32_t value, const uint32_t* u, int32_t R,
                            int64_t* count, int32_t* index, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Stage-1 -> stage-2 volume handoff on the device (utils/sr_utils.py:137-242 inference_flavr, :279-304 zeroonenorm /
 * postprocess_flavr; rehrseg_amd/utils/sr_utils.py drives them, csrc/sr_volume.hip).
 * A "minmax" buffer is two uint32 codes {min, max} that order like the floats they stand for:
 * code(f) = bits(f) ^ 0x80000000 for f >= +0, ~bits(f) below; the caller initialises it to {0xffffffff, 0} and the
 * kernels fold values in with atomicMin / atomicMax (order-independent, deterministic).
 * ------------------------------------------------------------------------- */
/* minmax <- min / max of x[0..n) folded into its current content (no NaN). */
int rehr_minmax_f32(const float* x, int64_t n, uint32_t* minmax, void* stream);
/* vol: the stored (X, Y, Z, C) fp32 volume, C in {1, 2}.  out: the network input of the windows [w0, w0 + b) of
 * apply_to_vol_flavr (window w reads the slices w-1 .. w+2; a slice outside the volume is zero; Z == 2: -2 .. 1),
 * logical (b, C, 4, Xp, Yp) in NDHWC memory: out[bi][s][x][y][c] = vol[x][y][z][c], zero for x >= X or y >= Y.
 * Xp, Yp: multiples of 16; out 16-byte aligned. */
int rehr_sr_window_gather_f32(const float* vol, float* out, int32_t X, int32_t Y, int32_t Z, int32_t C, int32_t w0,
                              int32_t b, int32_t Xp, int32_t Yp, void* stream);
/* net: the network's fp32 (b, C, n_out, >= X, >= Y) output for the windows [w0, w0 + b) of n_windows, element
 * strides[5] (any layout, >= 0).  With v(c) = net[bi][c][s][x][y] * (max - min) + min (two roundings; min / max
 * decoded from in_minmax): img[(w0 + bi) * n_out + s][y][x] = v(0); seg (NULL: skipped; needs C >= 2) = v(1) > 0;
 * out_minmax folds in the written img values.  img / seg: (n_windows * n_out, Y, X); with X % 4 == 0 img must be
 * 16-byte and seg 4-byte aligned. */
int rehr_sr_volume_scatter_f32(const float* net, const int64_t* strides, int32_t b, int32_t C, int32_t n_out, int32_t X,
                               int32_t Y, int32_t w0, int32_t n_windows, const uint32_t* in_minmax, float* img,
                               uint8_t* seg, uint32_t* out_minmax, void* stream);
/* out[x][p] = sum_t taps[t] * n(img[x + t - (L - 1) / 2][p]) over the terms inside [0, X), with
 * n(v) = ((v - min) / (max - min)) * 255 (three roundings): zeroonenorm and the slice-profile blur along the first
 * axis of postprocess_flavr.  img, out: (X, P) fp32, distinct; taps: L <= 32 device floats (REHR_ENOSUP above). */
int rehr_stage2_prep_f32(const float* img, const uint32_t* minmax, const float* taps, int32_t L, float* out, int32_t X,
                         int64_t P, void* stream);
/* out[i] = low 8 bits of (int32)(n(u[i]) * 255), truncated toward zero: (zeroonenorm(u) * 255).astype('uint8'). */
int rehr_stage2_unc_u8_f32(const float* u, const uint32_t* minmax, uint8_t* out, int64_t n, void* stream);

/* ------------------------------------------------------------------------- *
 * Stage-1 volume preparation on the device (utils/sr_utils.py:244-277 postprocess_smore; rehrseg_amd/utils/sr_utils.py
 * drives it, csrc/stage1_volume.hip).  The cubic B-spline prefilter is ndimage's spline_filter1d(mode='mirror'): gain 6,
 * pole sqrt(3) - 2, the causal pass started from the exact sum over the mirrored line, carried in fp64 in ndimage's
 * order of operations; a line of one sample is left as it is.  Lines of up to 283 samples (REHR_ENOSUP above).
 * ------------------------------------------------------------------------- */
/* scipy.ndimage.zoom along the slice axis of the stored (lines, n, C) fp32 volume (lines = X * Y), C in {1, 2}:
 * img[l][j] = fp32(sum_q coeff[l][idx[j][q]] * w[j][q]), q = 0..3 in this order in fp64, coeff = the prefiltered
 * channel 0; with C == 2 label[l][j] = (uint8)(int32) vol[l][nn[j]][1], 0 where nn[j] < 0.  idx: int32 [Z][4], w: double
 * [Z][4], nn: int32 [Z] on the device (nn, label: NULL with C == 1); indices are clamped into [0, n).  img: (lines, Z)
 * fp32, label: (lines, Z) uint8. */
int rehr_zoom_depth_f32(const float* vol, int64_t lines, int32_t n, int32_t C, const int32_t* idx, const double* w,
                        const int32_t* nn, int32_t Z, float* img, uint8_t* label, void* stream);
/* y = the B-spline coefficients of x along the middle axis of its (outer, n, inner) view, rounded to fp32 once; x, y
 * distinct. */
int rehr_bspline_prefilter_axis_f64acc_f32(const float* x, float* y, int64_t outer, int32_t n, int64_t inner,
                                           void* stream);
/* img: (X, Y, Z) fp32.  axis 0: out (Z, X, Y), out[z][x][y] = sum_t taps[t] * img[x + t - (L - 1) / 2][y][z];
 * axis 1: out (Z, Y, X), out[z][y][x] = sum_t taps[t] * img[x][y + t - (L - 1) / 2][z]; terms outside the axis are
 * dropped; one fmaf per tap in tap order from 0 (the bits of rehr_axis_resample_f32 over the blur's tap table).
 * taps: L <= 32 device floats (REHR_ENOSUP above). */
int rehr_blur_to_slices_f32(const float* img, const float* taps, int32_t L, float* out, int32_t X, int32_t Y, int32_t Z,
                            int32_t axis, void* stream);

/* ------------------------------------------------------------------------- *
 * Stage-1 validation on the device (rehrseg_amd/train_steps.py validate_sr, csrc/sr_metrics.hip): the quality of a
 * predicted image against its target, and of a predicted foreground against its label, in one pass.
 * pred / target (and, both or neither, seg_logits / seg_target) are logical (N, D, H, W) images, each addressed by
 * a base pointer and four element strides (>= 0; any layout, nothing is copied).  pred and seg_logits are fp32
 * (_f32) or bf16 widened at the load (_bf16); the targets are fp32.  stats[n][7] double, written (not accumulated):
 *   [0] sum |p - t|   [1] sum (p - t)^2   over the sample's D * H * W voxels
 *   [2] the sum of the SSIM index (Wang et al. 2004) over all valid window positions of the D slices: per (H, W)
 *       slice, 11x11 Gaussian window, sigma 1.5, unit sum, separable; the biased window-weighted variances
 *       E[x^2] - mu_x^2 and covariance; C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2;
 *       S = (2 mu_x mu_y + C1)(2 s_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(s_xx + s_yy + C2)); a position is valid when its
 *       window lies inside the slice
 *   [3] their number D * (H - 10) * (W - 10)
 *   [4] #(logit > 0 and target > 0.5)   [5] #(logit > 0)   [6] #(target > 0.5)   (exact; zeros without the pair)
 * Per-voxel terms and window moments are fp32, every sum over voxels, positions and blocks fp64 in a fixed order:
 * the same bits on every run; identical pred and target give an index of exactly 1.
 * H, W >= 11 (REHR_ENOSUP below).  workspace: rehr_sr_metrics_workspace_bytes(N, D, H, W) bytes of device scratch,
 * 8-byte aligned (< 0: REHR_E*).
 * ------------------------------------------------------------------------- */
int64_t rehr_sr_metrics_workspace_bytes(int32_t N, int32_t D, int32_t H, int32_t W);
int rehr_sr_metrics_f32(const float* pred, const int64_t* pred_strides, const float* target,
                        const int64_t* target_strides, const float* seg_logits, const int64_t* seg_logits_strides,
                        const float* seg_target, const int64_t* seg_target_strides, int32_t N, int32_t D, int32_t H,
                        int32_t W, float data_range, double* stats, void* workspace, int64_t workspace_bytes,
                        void* stream);
int rehr_sr_metrics_bf16(const void* pred, const int64_t* pred_strides, const float* target,
                         const int64_t* target_strides, const void* seg_logits, const int64_t* seg_logits_strides,
                         const float* seg_target, const int64_t* seg_target_strides, int32_t N, int32_t D, int32_t H,
                         int32_t W, float data_range, double* stats, void* workspace, int64_t workspace_bytes,
                         void* stream);

/* ------------------------------------------------------------------------- *
 * Stage-1 structure losses (rehrseg_amd/models/losses.py StructureLoss, csrc/sr_losses.hip): a differentiable
 *   loss = l1 mean|p - t| + l2 mean (p - t)^2 + ssim (1 - mean S) + sobel mean|G(p) - G(t)|
 * of input p against target t, logical (N, C, D, H, W) fp32 images each addressed by a base pointer and five element
 * strides (>= 0; any layout, nothing is copied); every (H, W) slice is an image, V = N C D H W.
 *   S  the SSIM index of rehr_sr_metrics_f32 (same window, constants, arithmetic and order of operations) over the
 *      M = N C D (H - 10)(W - 10) valid window positions: 1 - the term is the mean index that entry point reports;
 *   G  the Sobel magnitude sqrt(gx^2 + gy^2 + 1e-6) per slice, gx = [[-1,0,1],[-2,0,2],[-1,0,1]] / 8, gy its
 *      transpose, replicate padding.
 * A weight of 0 skips its term.  ssim != 0 needs H, W >= 11 (REHR_ENOSUP below); weights finite, data_range > 0.
 * fwd: stats[n][4] double (written) = sum |p - t|, sum (p - t)^2, sum of S over the valid positions, sum |G(p) - G(t)|
 *   of sample n (0 for a skipped term); *loss = the fp32 value; fields: NULL, or 3 V floats that receive the SSIM
 *   coefficient fields the backward pass reads (only with ssim != 0).  Per-pixel terms fp32, every sum fp64 in a
 *   fixed order: the same bits on every run; p == t gives exactly 0.  workspace:
 *   rehr_structure_loss_workspace_bytes(N, C, D, H, W) bytes of device scratch, 8-byte aligned (< 0: REHR_E*).
 * bwd: dinput (its own five strides, none 0 along an axis longer than 1) = *grad_output * d loss / d input, every
 *   element written by one thread; |.| has derivative 0 at 0.  fields: what fwd wrote for the same operands and
 *   weights (required with ssim != 0).  grad_output: one device float.
 * ------------------------------------------------------------------------- */
int64_t rehr_structure_loss_workspace_bytes(int32_t N, int32_t C, int32_t D, int32_t H, int32_t W);
int rehr_structure_loss_fwd_f32(const float* input, const int64_t* input_strides, const float* target,
                                const int64_t* target_strides, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                                float l1, float l2, float ssim, float sobel, float data_range, double* stats,
                                float* loss, float* fields, void* workspace, int64_t workspace_bytes, void* stream);
int rehr_structure_loss_bwd_f32(const float* input, const int64_t* input_strides, const float* target,
                                const int64_t* target_strides, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                                float l1, float l2, float ssim, float sobel, const float* fields,
                                const float* grad_output, float* dinput, const int64_t* dinput_strides, void* stream);

/* ------------------------------------------------------------------------- *
 * Mixed-precision (*_bf16) variants of the HBM-bound fused-block kernels: the SAME arguments as the *_f32 entry
 * points above with every ACTIVATION pointer (x, y, res, dy, dx, dres) addressing bf16 elements (ld* in elements,
 * % 8 == 0, C % 8 == 0); gates, gamma / beta, mean_rstd stay fp32, statistics and reduction buffers fp64, the
 * arithmetic is fp32 in registers.  BASELINE.json configs[4] (bf16 autocast of the same torch.nn call sites).
 * ------------------------------------------------------------------------- */
int rehr_scale_res_act_fwd_bf16(const void* x, int32_t ldx, const float* gate, const void* res, int32_t ldr, void* y,
                                int32_t ldy, int32_t N, int64_t S, int32_t C, int32_t act, float slope, void* stream);
int rehr_scale_res_act_bwd_bf16(const void* dy, int32_t lddy, const void* y, int32_t ldy, const void* x, int32_t ldx,
                                const float* gate, void* dx, int32_t lddx, void* dres, int32_t lddr,
                                double* dgate_acc, int32_t N, int64_t S, int32_t C, int32_t act, float slope,
                                void* stream);
int rehr_upmix_depth_fwd_bf16(const void* g, const float* bias, void* y, int32_t N, int32_t Di, int32_t Do, int64_t HW,
                              int32_t C, int32_t KD, int32_t pd, int32_t act, float slope, void* stream);
int rehr_upmix_depth_bwd_bf16(const void* dz, const void* y, void* dg, int32_t N, int32_t Di, int32_t Do, int64_t HW,
                              int32_t C, int32_t KD, int32_t pd, int32_t act, float slope, void* stream);
int rehr_channel_sum_actgrad_bf16(const void* dy, const void* y, int32_t ld, int64_t rows, int32_t C, int32_t act,
                                  float slope, float* out, double* scratch, void* stream);
int rehr_add_channel_const_bf16(void* x, int32_t ldx, const float* k, int32_t N, int64_t S, int32_t C, void* stream);
int rehr_instnorm_act_fwd_bf16(const void* x, int32_t ldx, const double* stats, const float* gamma, const float* beta,
                               void* y, int32_t ldy, float* mean_rstd, int32_t N, int64_t S, int32_t C, float eps,
                               int32_t act, float slope, void* stream);
int rehr_instnorm_act_bwd_bf16(const void* dy, int32_t lddy, const void* x, int32_t ldx, const float* mean_rstd,
                               const float* gamma, const float* beta, void* dx, int32_t lddx, float* dgamma,
                               float* dbeta, double* red, int32_t N, int64_t S, int32_t C, int32_t act, float slope,
                               void* stream);
/* the same, and dconv_bias[c] = sum over all samples and voxels of the dx it writes: the gradient of the bias of the
 * convolution in front of the normalisation (the mixed-precision weight-gradient kernels carry no bias column; this
 * replaces a separate rehr_channel_sum_bf16 pass over dx).  dsum: [C] doubles of scratch. */
int rehr_instnorm_act_bwd_dbias_bf16(const void* dy, int32_t lddy, const void* x, int32_t ldx, const float* mean_rstd,
                                     const float* gamma, const float* beta, void* dx, int32_t lddx, float* dgamma,
                                     float* dbeta, double* red, int32_t N, int64_t S, int32_t C, int32_t act,
                                     float slope, double* dsum, float* dconv_bias, void* stream);
int rehr_channel_sum_bf16(const void* x, int32_t ldx, int64_t rows, int32_t C, float* out, int32_t accumulate,
                          double* scratch, void* stream);
int rehr_act_bwd_bf16(const void* dy, const void* y, void* dx, int64_t n, int32_t act, float slope, void* stream);

/* ABI version, bumped on any signature change. */
int rehr_abi_version(void);
/* Text of the last HIP launch error seen on the calling thread (diagnostics). */
const char* rehr_last_hip_error(void);

#ifdef __cplusplus
}
#endif
#endif /* REHRSEG_HIP_H */
