// Types and host helpers shared by the thin-convolution family, everything driven by rehr_direct_conv_desc: the vector
// kernels (direct_conv.hip), the thin-input matrix-core kernels (thin_cin_conv.hip) and sr_head.2 on the matrix cores
// (thin_conv_bf16.hip, thin_conv_f32.hip).  direct_conv.hip decides the route of the thin-input layers; the route
// predicates exist here and nowhere else -- the Python side asks through the queries of rehrseg_hip.h.
#pragma once
#include "common.h"
#include <type_traits>

// the output extent follows from the input extent
inline bool conv_out_extent_ok(const rehr_direct_conv_desc& d) {
  return d.sd >= 1 && d.sh >= 1 && d.sw >= 1 && (d.Di + 2 * d.pd - d.KD) / d.sd + 1 == d.Do &&
         (d.Hi + 2 * d.ph - d.KH) / d.sh + 1 == d.Ho && (d.Wi + 2 * d.pw - d.KW) / d.sw + 1 == d.Wo;
}

// ---- thin input on the fp32 matrix cores (thin_cin_conv.hip).  REHR_ENOSUP = not a shape for it: the caller goes on
// to the vector kernel.
bool thin_cin_fwd_has_plan(const rehr_direct_conv_desc& d);   // reads no pointer
int thin_cin_fwd_launch(const rehr_direct_conv_desc& d, hipStream_t stream, bool y_bf16);
int64_t thin_cin_wgrad_workspace_bytes(const rehr_direct_conv_desc& d);   // 0 = not applicable
int thin_cin_wgrad_try(const rehr_direct_conv_desc& d, float* dw, float* dbias, float* workspace, int64_t workspace_bytes,
                       hipStream_t stream, bool dy_bf16);

// ---- sr_head.2, Conv3d(16 -> 2, 5x5x5, stride 1, pad 2), in both precisions
constexpr int T5_CIN = 16, T5_K = 5, T5_BH = 4;   // channels, kernel extent, output rows per block
constexpr int T5_ROWS = T5_BH + T5_K - 1;          // staged rows per plane
constexpr int T5_PP = 11;                          // floats per voxel in the P row (10 used + 1: odd pitch, conflict-free reads)
constexpr int T5_RING = 6;                         // dY planes in LDS
constexpr int T5_PADW = 8;                         // dY row of the input gradient: 2 zero voxels in front, 6 behind
constexpr int T5_SLAB = 25 * 16 * 16;              // weight-gradient partial sums per block: [kd*5 + kw][ci][kh*2 + co]
constexpr int T5_SLABF = T5_SLAB + 16;             // + the block's column sums of dY (bias gradient) in the first two extra slots

struct Thin5Prec {
  int elem_bytes, ldx_multiple, w_max;
  int64_t pack_bytes;   // the largest packed weight panel
};

inline bool thin5_shape_ok(const rehr_direct_conv_desc& d, const Thin5Prec& k) {
  return d.Cin == T5_CIN && d.Cout == 2 && d.KD == T5_K && d.KH == T5_K && d.KW == T5_K && d.sd == 1 && d.sh == 1 &&
         d.sw == 1 && d.pd == 2 && d.ph == 2 && d.pw == 2 && d.Do == d.Di && d.Ho == d.Hi && d.Wo == d.Wi &&
         d.Wi % 32 == 0 && d.Wi >= 32 && d.Wi <= k.w_max && d.ldx % k.ldx_multiple == 0 && d.ldx >= T5_CIN && d.ldy >= 2 &&
         (int64_t)d.Di * d.Hi * d.Wi * d.ldx * k.elem_bytes < ((int64_t)1 << 32);   // buffer resource of one image
}

// strips of T5_BH rows x depth segments: enough blocks for the chip, each long enough to amortise the halo planes.
// Returns the number of blocks.
inline int64_t thin5_segments(const rehr_direct_conv_desc& d, int& nstrip, int& dseg, int& nseg) {
  nstrip = (d.Hi + T5_BH - 1) / T5_BH;
  int ns = 1;
  while ((int64_t)d.N * nstrip * ns < 512 && d.Di / (ns * 2) >= 16) ns *= 2;
  dseg = (d.Di + ns - 1) / ns;
  nseg = (d.Di + dseg - 1) / dseg;
  return (int64_t)d.N * nstrip * nseg;
}

// one workspace for all three passes: the weight gradient's slabs or the packed weights
inline int64_t thin5_workspace_bytes(const rehr_direct_conv_desc& d, const Thin5Prec& k) {
  if (!thin5_shape_ok(d, k)) return REHR_ENOSUP;
  int nstrip, dseg, nseg;
  const int64_t slabs = thin5_segments(d, nstrip, dseg, nseg) * T5_SLABF * 4;
  return slabs > k.pack_bytes ? slabs : k.pack_bytes;
}

// what every entry point asks after its own pointers: REHR_OK or the code to return
inline int thin5_admit(const rehr_direct_conv_desc& d, const void* workspace, int64_t workspace_bytes, const Thin5Prec& k) {
  if (workspace == nullptr) return REHR_EINVAL;
  if (!thin5_shape_ok(d, k)) return REHR_ENOSUP;
  return workspace_bytes < thin5_workspace_bytes(d, k) ? REHR_EINVAL : REHR_OK;
}

// f(std::integral_constant<int, n>) for n = tiles <= NMAX: the kernels are instantiated per row width (W = 32 n)
template <int NMAX, typename F>
static int thin5_for_width(int n, F&& f) {
  switch (n) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5:
      if constexpr (NMAX >= 5) return f(std::integral_constant<int, 5>{});
  }
  return REHR_ENOSUP;
}
// The LDS limit is raised at every launch: set_dyn_lds_once() remembers per process, and nothing pins this family to
// one device.  (static: rehr_launch_failed is per translation unit)
template <typename P>
static int thin5_launch(void (*kernel)(P), int64_t blocks, int threads, size_t smem, hipStream_t st, const P& p) {
  REHR_LAUNCH_CHECK();   // the weight pack launched before
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) !=
      hipSuccess)
    return REHR_EHIP;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(threads), smem, st, p);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}
// dw (2,16,5,5,5) and db = the block slabs summed in a fixed order (direct_conv.hip)
int thin5_wgrad_reduce(const float* slabs, int nblocks, float* dw, float* dbias, hipStream_t st);
