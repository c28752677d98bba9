// Tap geometry of one axis and the range limit of buffer-addressed operands: what the gather-GEMM family (gg_shared.h)
// and the weight-gradient family (wgrad_shared.h) both need on the host.
#pragma once
#include "common.h"

// ---- range checks: raw buffer loads take 32-bit byte offsets ----
// A tensor (or slice) a kernel addresses through one buffer resource must be smaller than this; a planner that lets a
// larger one through is an out-of-bounds access on the device.
constexpr int64_t BUF_LIMIT = (1ll << 32) - 64;
inline bool fits_buffer(int64_t bytes) { return bytes < BUF_LIMIT; }

// ---- tap geometry ----
// smallest / largest source offset of an axis' taps relative to the lattice point
inline void span(const rehr_axis_taps& t, int b, int* mn, int* mx) {
  int lo = b + t.off0, hi = lo;
  for (int j = 1; j < t.count; ++j) {
    const int o = b + t.off0 + t.offs * j;
    if (o < lo) lo = o;
    if (o > hi) hi = o;
  }
  *mn = lo;
  *mx = hi;
}

// the taps of a unit-stride "same" 3-tap axis: offsets -1, 0, +1 in either order (what the F(2x2,3x3) kernels transform)
inline bool three_taps(const rehr_axis_taps& t, int b) {
  if (t.count != 3) return false;
  const int o0 = b + t.off0, o1 = b + t.off0 + t.offs, o2 = b + t.off0 + 2 * t.offs;
  return (o1 == 0) && ((o0 == -1 && o2 == 1) || (o0 == 1 && o2 == -1));
}
