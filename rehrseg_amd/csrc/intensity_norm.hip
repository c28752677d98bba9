// Intensity normalisation on the device: exact order statistics by radix select, numpy's percentile
// from them, and the clip / scale pass of percentile_normalization and zeroone_normalization.
//
//   rehr_order_stats_f32       out[b][r] = sort(x[b][0..S))[ranks[r]], the exact float; NaN in every rank of an item
//                              that holds a NaN.  Nine launches, none depending on anything read back.
//   rehr_percentile_f64        numpy.percentile (method 'linear') from pairs of order statistics, in fp64.
//   rehr_intensity_apply_f32   y = (clip(x, lo, hi) - lo) / (hi - lo) or y = (x - lo) / (hi - lo), bounds read on the
//                              device, plain IEEE fp32 subtraction and a correctly rounded division.
//
// Select: MSD radix select over the order-preserving key of a float (all bits of a negative flipped, the sign bit of
// the rest), four digits of 8 bits.  Pass p counts the digit p of every element whose digits 0..p-1 equal the prefix a
// rank has chosen so far: per-block histograms in LDS with integer atomics, flushed into global uint32 counts (exact
// and order-free: the same bits on every run).  Pass 0 has no prefix and is shared by all ranks; in the later passes
// ranks whose prefixes are equal share one histogram (the k0 / k0 + 1 pair of a percentile nearly always does).
// Between the passes one block per item scans the 256 counts of every rank, picks the bin that holds the rank and the
// rank's position inside it, and clears the counts for the next pass.  After pass 3 the key is complete.
//
// A wave whose lanes hit one bin (an MRI volume is often more than half exact zeros; the first digit is the sign and
// seven exponent bits, so any smooth distribution puts most of a wave into two or three bins as well) sends 64 atomics
// to one LDS word, whose cost on this chip is unmeasured: up to kPeel times the lanes that share the first pending
// lane's bin are folded by a ballot into one add of their number, and only what is left goes out lane by lane.
#include "common.h"
#include "host_util.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBins = 256;
constexpr int kMaxRanks = REHR_ORDER_STATS_MAX_RANKS;
constexpr int kMaxBlocks = 1024;              // per item
constexpr int kVecPerBlock = 2048;            // 16-byte vectors a block takes at least (where there are that many)
constexpr int kPeel = 4;
constexpr int64_t kMaxS = (int64_t)1 << 30;

typedef unsigned long long u64;

struct Ranks {
  uint32_t k[kMaxRanks];
};

// per (item, rank): the digits chosen so far, the rank inside the elements that share them, and the first rank of the
// item with the same prefix (the one whose histogram is counted)
struct RankState {
  uint32_t prefix, krem, rep, pad;
};

// h[bin] += 1 for every lane with `on`; called by whole waves
__device__ __forceinline__ void wave_count(unsigned* h, const bool on, const uint32_t bin, const int lane) {
  u64 todo = __ballot(on);
  bool mine = on;
#pragma unroll
  for (int round = 0; round < kPeel; ++round) {
    if (!todo) return;
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
    const u64 m = __ballot(mine && bin == b0);
    if (lane == leader) atomicAdd(h + b0, (unsigned)__popcll(m));
    mine = mine && bin != b0;
    todo &= ~m;
  }
  if (mine) atomicAdd(h + bin, 1u);
}

template <int PASS>
__device__ __forceinline__ void count_element(unsigned* h, const bool valid, const uint32_t bits, const int R,
                                              const uint32_t* pre, const uint32_t live, const int lane, bool& nan) {
  const uint32_t key = ord_of_bits(bits);
  if (PASS == 0) {
    nan = nan || (valid && (bits & 0x7fffffffu) > 0x7f800000u);
    wave_count(h, valid, key >> 24, lane);
  } else {
    const uint32_t head = key >> (32 - 8 * PASS), digit = (key >> (24 - 8 * PASS)) & 0xffu;
    for (int r = 0; r < R; ++r) {
      if (!((live >> r) & 1u)) continue;                          // wave-uniform
      wave_count(h + r * kBins, valid && head == pre[r], digit, lane);
    }
  }
}

// grid (blocks, B).  Item b starts at x + b * stride: a scalar head up to the first 16-byte boundary, 16-byte loads,
// a scalar tail.  Every loop runs the same number of steps in all lanes of a wave (the ballots need whole waves).
template <int PASS>
__global__ __launch_bounds__(kThreads) void select_hist_kernel(const float* __restrict__ x, const int64_t S,
                                                               const int64_t stride, const int R,
                                                               const RankState* __restrict__ state,
                                                               unsigned* __restrict__ hist,
                                                               unsigned* __restrict__ nanflag) {
  __shared__ unsigned h[PASS == 0 ? kBins : kMaxRanks * kBins];
  __shared__ uint32_t pre[kMaxRanks];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int nh = PASS == 0 ? kBins : R * kBins;
  for (int i = tid; i < nh; i += kThreads) h[i] = 0;
  uint32_t live = 0;
  if (PASS != 0) {
    if (tid < R) pre[tid] = state[b * R + tid].prefix;
    for (int r = 0; r < R; ++r) live |= (state[b * R + r].rep == (uint32_t)r ? 1u : 0u) << r;
  }
  __syncthreads();

  const uint32_t* xb = reinterpret_cast<const uint32_t*>(x + (size_t)b * stride);
  const int64_t mis = (int64_t)((16 - (reinterpret_cast<uintptr_t>(xb) & 15)) & 15) / 4;
  const int64_t head = mis < S ? mis : S;
  const int64_t nvec = (S - head) / 4, tail0 = head + nvec * 4;
  bool nan = false;
  if (blockIdx.x == 0 && tid < 64) {                             // one wave: at most 3 + 3 elements
    const bool vh = tid < head, vt = tail0 + tid < S;
    count_element<PASS>(h, vh, vh ? xb[tid] : 0u, R, pre, live, lane, nan);
    count_element<PASS>(h, vt, vt ? xb[tail0 + tid] : 0u, R, pre, live, lane, nan);
  }
  const uint4* xv = reinterpret_cast<const uint4*>(xb + head);
  const int64_t per = (nvec + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < nvec ? lo + per : nvec;
  for (int64_t base = lo; base < hi; base += kThreads) {
    const int64_t i = base + tid;
    const bool valid = i < hi;
    const uint4 v = valid ? xv[i] : make_uint4(0, 0, 0, 0);
    count_element<PASS>(h, valid, v.x, R, pre, live, lane, nan);
    count_element<PASS>(h, valid, v.y, R, pre, live, lane, nan);
    count_element<PASS>(h, valid, v.z, R, pre, live, lane, nan);
    count_element<PASS>(h, valid, v.w, R, pre, live, lane, nan);
  }
  if (PASS == 0 && __ballot(nan) && lane == 0) atomicOr(nanflag + b, 1u);
  __syncthreads();
  unsigned* hb = hist + (size_t)b * R * kBins;
  for (int i = tid; i < nh; i += kThreads) {
    const unsigned c = h[i];
    if (c) atomicAdd(hb + i, c);
  }
}

// one block of 256 threads per item: for every rank the bin that holds it, from an inclusive scan of the counts of
// the rank's histogram (pass 0: the shared one); then the counts are cleared.  After pass 3 the key is complete and goes out.
__global__ __launch_bounds__(kBins) void select_scan_kernel(unsigned* __restrict__ hist, RankState* __restrict__ state,
                                                            const int R, const int pass, const Ranks ranks,
                                                            const unsigned* __restrict__ nanflag,
                                                            float* __restrict__ out) {
  __shared__ unsigned inc[2][kBins];
  __shared__ RankState next[kMaxRanks];
  const int b = blockIdx.x, t = threadIdx.x;
  unsigned* hb = hist + (size_t)b * R * kBins;
  RankState* sb = state + (size_t)b * R;
  for (int r = 0; r < R; ++r) {
    const RankState cur = pass == 0 ? RankState{0u, ranks.k[r], 0u, 0u} : sb[r];
    const unsigned c = hb[cur.rep * kBins + t];
    int w = 0;
    inc[0][t] = c;
    __syncthreads();
#pragma unroll
    for (int o = 1; o < kBins; o <<= 1) {
      inc[w ^ 1][t] = inc[w][t] + (t >= o ? inc[w][t - o] : 0u);
      w ^= 1;
      __syncthreads();
    }
    const unsigned incl = inc[w][t], excl = incl - c;
    if (excl <= cur.krem && cur.krem < incl) {                   // one thread: the counts sum to more than krem
      next[r].prefix = (cur.prefix << 8) | (uint32_t)t;
      next[r].krem = cur.krem - excl;
    }
    __syncthreads();
  }
  if (t < R) {
    uint32_t rep = (uint32_t)t;
    for (int r = t - 1; r >= 0; --r)
      if (next[r].prefix == next[t].prefix) rep = (uint32_t)r;
    sb[t] = RankState{next[t].prefix, next[t].krem, rep, 0u};
    if (pass == 3) {
      const uint32_t bits = nanflag[b] ? 0x7fc00000u : bits_of_ord(next[t].prefix);
      out[(size_t)b * R + t] = __uint_as_float(bits);
    }
  }
  __syncthreads();
  for (int i = t; i < R * kBins; i += kBins) hb[i] = 0;
}

__global__ __launch_bounds__(kThreads) void select_zero_kernel(uint4* __restrict__ p, const int64_t n16) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n16; i += (int64_t)gridDim.x * kThreads)
    p[i] = make_uint4(0, 0, 0, 0);
}

struct Lerp {
  double t[REHR_PERCENTILE_MAX_Q];
};

// one thread per item: numpy's two-sided lerp of the order statistics 2 j and 2 j + 1 (the formula of
// seg_surface.hip's hd95), in fp64 without contraction
#pragma clang fp contract(off)
__global__ __launch_bounds__(kThreads) void percentile_kernel(const float* __restrict__ stats, const int B, const int Q,
                                                              const Lerp lerp, const int strictly_positive,
                                                              double* __restrict__ out) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= B) return;
  for (int j = 0; j < Q; ++j) {
    const double lo = (double)stats[(size_t)b * 2 * Q + 2 * j], hi = (double)stats[(size_t)b * 2 * Q + 2 * j + 1];
    const double t = lerp.t[j], diff = hi - lo;
    double v = t >= 0.5 ? hi - diff * (1.0 - t) : lo + diff * t;
    if (j == 0 && strictly_positive && v < 0.0) v = 0.0;
    out[(size_t)b * Q + j] = v;
  }
}

__device__ __forceinline__ float norm_one(const float x, const float lo, const float hi, const float range,
                                          const bool clip) {
  float v = x;
  if (clip) {                       // numpy.clip: a NaN stays a NaN
    v = v < lo ? lo : v;
    v = v > hi ? hi : v;
  }
  return __fdiv_rn(__fsub_rn(v, lo), range);
}

// grid (blocks, B); x and y may be the same buffer (every element is read once, by the thread that writes it)
__global__ __launch_bounds__(kThreads) void intensity_apply_kernel(const float* x, float* y, const int64_t S,
                                                                   const int64_t x_stride, const int64_t y_stride,
                                                                   const bool clip, const double* __restrict__ bounds,
                                                                   const int64_t bounds_stride) {
  const int b = blockIdx.y;
  const float lo = (float)bounds[(size_t)b * bounds_stride], hi = (float)bounds[(size_t)b * bounds_stride + 1];
  const float range = __fsub_rn(hi, lo);
  const float* xb = x + (size_t)b * x_stride;
  float* yb = y + (size_t)b * y_stride;
  const int64_t step = (int64_t)gridDim.x * kThreads, first = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (((reinterpret_cast<uintptr_t>(xb) | reinterpret_cast<uintptr_t>(yb)) & 15) == 0) {
    const int64_t nvec = S / 4;
    for (int64_t i = first; i < nvec; i += step) {
      f32x4 v = *reinterpret_cast<const f32x4*>(xb + i * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = norm_one(v[e], lo, hi, range, clip);
      *reinterpret_cast<f32x4*>(yb + i * 4) = v;
    }
    for (int64_t i = nvec * 4 + first; i < S; i += step) yb[i] = norm_one(xb[i], lo, hi, range, clip);
  } else {
    for (int64_t i = first; i < S; i += step) yb[i] = norm_one(xb[i], lo, hi, range, clip);
  }
}

int check_select(int32_t B, int32_t R) {
  if (B < 1 || R < 1) return REHR_EINVAL;
  if (B > 65535 || R > kMaxRanks) return REHR_ENOSUP;
  return REHR_OK;
}

// workspace: [RankState per (item, rank)][NaN flag per item][counts: B * R * 256 uint32]
struct Layout {
  RankState* state;
  unsigned *nanflag, *hist;
  int64_t bytes;
};
Layout layout(void* base, int64_t B, int64_t R) {
  Carver c(base);   // a braced list is evaluated left to right
  return {c.take<RankState>(B * R), c.take<unsigned>(B), c.take<unsigned>(B * R * kBins), c.bytes()};
}

}  // namespace

extern "C" int64_t rehr_order_stats_workspace_bytes(int32_t B, int32_t R) {
  const int rc = check_select(B, R);
  if (rc != REHR_OK) return rc;
  return layout(nullptr, B, R).bytes;
}

extern "C" int rehr_order_stats_f32(const float* x, int32_t B, int64_t S, int64_t item_stride, const int64_t* ranks,
                                    int32_t R, float* out, void* workspace, int64_t workspace_bytes, void* stream) {
  if (x == nullptr || ranks == nullptr || out == nullptr || workspace == nullptr) return REHR_EINVAL;
  if (S < 1 || (B > 1 && item_stride < S)) return REHR_EINVAL;
  const int rc = check_select(B, R);
  if (rc != REHR_OK) return rc;
  if (S > kMaxS) return REHR_ENOSUP;
  Ranks rk = {};
  for (int r = 0; r < R; ++r) {
    if (ranks[r] < 0 || ranks[r] >= S) return REHR_EINVAL;
    rk.k[r] = (uint32_t)ranks[r];
  }
  const auto [state, nanflag, hist, need] = layout(workspace, B, R);
  if (workspace_bytes < need || misaligned(16, workspace) || misaligned(4, x, out)) return REHR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n16 = need / 16;
  hipLaunchKernelGGL(select_zero_kernel, dim3(grid_for(n16, kThreads, 4096)), dim3(kThreads), 0, st,
                     static_cast<uint4*>(workspace), n16);
  const dim3 grid(grid_for(S / 4, kVecPerBlock, kMaxBlocks), (unsigned)B), scan((unsigned)B);
  hipLaunchKernelGGL(select_hist_kernel<0>, grid, dim3(kThreads), 0, st, x, S, item_stride, R,
                     (const RankState*)state, hist, nanflag);
  hipLaunchKernelGGL(select_scan_kernel, scan, dim3(kBins), 0, st, hist, state, R, 0, rk, (const unsigned*)nanflag, out);
  hipLaunchKernelGGL(select_hist_kernel<1>, grid, dim3(kThreads), 0, st, x, S, item_stride, R,
                     (const RankState*)state, hist, nanflag);
  hipLaunchKernelGGL(select_scan_kernel, scan, dim3(kBins), 0, st, hist, state, R, 1, rk, (const unsigned*)nanflag, out);
  hipLaunchKernelGGL(select_hist_kernel<2>, grid, dim3(kThreads), 0, st, x, S, item_stride, R,
                     (const RankState*)state, hist, nanflag);
  hipLaunchKernelGGL(select_scan_kernel, scan, dim3(kBins), 0, st, hist, state, R, 2, rk, (const unsigned*)nanflag, out);
  hipLaunchKernelGGL(select_hist_kernel<3>, grid, dim3(kThreads), 0, st, x, S, item_stride, R,
                     (const RankState*)state, hist, nanflag);
  hipLaunchKernelGGL(select_scan_kernel, scan, dim3(kBins), 0, st, hist, state, R, 3, rk, (const unsigned*)nanflag, out);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_percentile_f64(const float* stats, int32_t B, int32_t Q, const double* t, int32_t strictly_positive,
                                   double* out, void* stream) {
  if (stats == nullptr || t == nullptr || out == nullptr || B < 1 || Q < 1) return REHR_EINVAL;
  if (Q > REHR_PERCENTILE_MAX_Q) return REHR_ENOSUP;
  if (misaligned(4, stats) || misaligned(8, out)) return REHR_EINVAL;
  Lerp lerp = {};
  for (int j = 0; j < Q; ++j) {
    if (!(t[j] >= 0.0 && t[j] < 1.0)) return REHR_EINVAL;
    lerp.t[j] = t[j];
  }
  hipLaunchKernelGGL(percentile_kernel, dim3((unsigned)((B + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, stats, B, Q, lerp, strictly_positive, out);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_intensity_apply_f32(const float* x, float* y, int32_t B, int64_t S, int64_t x_stride,
                                        int64_t y_stride, int32_t mode, const double* bounds, int64_t bounds_stride,
                                        void* stream) {
  if (x == nullptr || y == nullptr || bounds == nullptr || B < 1 || S < 1) return REHR_EINVAL;
  if (mode != REHR_INTENSITY_PERCENTILE && mode != REHR_INTENSITY_ZEROONE) return REHR_EINVAL;
  if (bounds_stride < 2 || (B > 1 && (x_stride < S || y_stride < S))) return REHR_EINVAL;
  if (B > 65535 || S > kMaxS) return REHR_ENOSUP;
  if (misaligned(4, x, y) || misaligned(8, bounds)) return REHR_EINVAL;
  hipLaunchKernelGGL(intensity_apply_kernel, dim3(grid_for(S / 4, kThreads * 4, 2048), (unsigned)B), dim3(kThreads), 0,
                     (hipStream_t)stream, x, y, S, x_stride, y_stride, mode == REHR_INTENSITY_PERCENTILE, bounds,
                     bounds_stride);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}
