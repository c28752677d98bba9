// The SSIM window arithmetic of sr_metrics.hip and sr_losses.hip: one copy, so that the index the validation reports
// and the index the loss differentiates are the same code and therefore the same bits.
//
// A block of kThreads owns a 32x32 tile of one (H, W) slice.  The kernel stages its images (or, in the loss's backward
// pass, its coefficient fields) in LDS with a 5-pixel halo at a row pitch of kPitch floats; staging differs per kernel
// and stays there.  From the staged rows: ssim_hpass_pair or ssim_hpass_plain, the horizontal 11-tap pass of NF fields into LDS, a barrier of
// the kernel's, ssim_vpass, the vertical pass (14 rows feed the 4 outputs of a thread), and ssim_index.  Every tap is
// one fmaf in ascending tap order and nothing else is contracted: the pragma below governs this header wherever it is
// included, and x^2, y^2 and xy go through the same operations, so p == t gives an index of exactly 1.
#pragma once
#include <math.h>

#include "common.h"
#include "host_util.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;             // interior edge
constexpr int kHalo = 5;
constexpr int kRows = kTile + 2 * kHalo;   // 42 staged rows
constexpr int kPitch = 44;            // staged row pitch in floats: 16-byte rows, columns 42 / 43 are padding

struct GaussTaps {
  float w[11];
};

// the 11 taps of a Gaussian of sigma 1.5 with unit sum
inline GaussTaps gauss_taps() {
  GaussTaps taps;
  double e[11], sum = 0.0;
  for (int k = 0; k < 11; ++k) {
    e[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
    sum += e[k];
  }
  for (int k = 0; k < 11; ++k) taps.w[k] = (float)(e[k] / sum);
  return taps;
}

struct Geometry {
  int tiles_x, tiles_y;
  int64_t per, blocks;   // tiles per sample, tiles in all
};

// one block per tile of every slice of an (N, C, D, H, W) image in one 1-D grid; `window`: an 11x11 window must fit
inline int tile_geometry(int32_t N, int32_t C, int32_t D, int32_t H, int32_t W, bool window, Geometry* g) {
  if (N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return REHR_EINVAL;
  if (window && (H < 2 * kHalo + 1 || W < 2 * kHalo + 1)) return REHR_ENOSUP;
  g->tiles_x = (W + kTile - 1) / kTile;
  g->tiles_y = (H + kTile - 1) / kTile;
  g->per = (int64_t)g->tiles_y * g->tiles_x;
  if (g->per > INT32_MAX / D || g->per * D > INT32_MAX / C) return REHR_ENOSUP;
  g->per *= (int64_t)D * C;
  if (g->per > INT32_MAX / N) return REHR_ENOSUP;
  g->blocks = g->per * N;
  return REHR_OK;
}

// workspace of a tile kernel: [SLOTS doubles per block: its partial sums, which the finish pass adds up per sample]
struct TileSums {
  double* slots;
  int64_t bytes;
};
template <int SLOTS>
inline TileSums tile_sums_layout(void* base, const Geometry& g) {
  static_assert(SLOTS % 2 == 0, "the size is blocks * SLOTS doubles exactly: no padding to 16 bytes");
  Carver c(base);   // a braced list is evaluated left to right
  return {c.take<double>(g.blocks * SLOTS), c.bytes()};
}

// runs body() at the positions whose window lies inside the slice.  The test stands in an `if` of its own rather than
// in a function that returns it: returned as a value, the four comparisons merge into one branch and the compiler lays
// the vertical pass out differently (profiles/ssim_tile_bench.txt)
template <typename Body>
__device__ __forceinline__ void ssim_if_valid(const int y, const int x, const int H, const int W, const Body& body) {
  if (y >= kHalo && y < H - kHalo && x >= kHalo && x < W - kHalo) body();
}

// Horizontal pass over the kRows staged rows.  An item is 4 neighbouring outputs of one row, from 16 staged columns
// of NS staged arrays: load(j, s) fills s[a][0..16) from the staged offsets j .. j + 15, and fields(s, e, v) gives the
// NF field values v[n] at the column e of them.
template <typename Item>
__device__ __forceinline__ void ssim_hitems(const Item& item) {
#pragma unroll   // two items per thread at the most
  for (int i = threadIdx.x; i < kRows * (kTile / 4); i += kThreads) item(i >> 3, (i & 7) * 4);
}
template <int NF, int NS, typename Load, typename Fields>
__device__ __forceinline__ void ssim_hitem(const GaussTaps& g, const int r, const int q, float (*out)[kRows * kTile],
                                           const Load& load, const Fields& fields) {
  float s[NS][16];
  load(r * kPitch + q, s);
  f32x4 f[NF];
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    float a[NF];
#pragma unroll
    for (int n = 0; n < NF; ++n) a[n] = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      float v[NF];
      fields(s, o + k, v);
#pragma unroll
      for (int n = 0; n < NF; ++n) a[n] = fmaf(g.w[k], v[n], a[n]);
    }
#pragma unroll
    for (int n = 0; n < NF; ++n) f[n][o] = a[n];
  }
#pragma unroll
  for (int n = 0; n < NF; ++n) *reinterpret_cast<f32x4*>(&out[n][r * kTile + q]) = f[n];
}
// the five fields x, y, x^2, y^2, xy of an image pair staged at sP and sT
__device__ __forceinline__ void ssim_hpass_pair(const GaussTaps& g, const float* sP, const float* sT,
                                                float (*out)[kRows * kTile]) {
  ssim_hitems([&](const int r, const int q) {
    ssim_hitem<5, 2>(
        g, r, q, out,
        [&](const int j, float (&s)[2][16]) {
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(sP + j + 4 * v);
            const f32x4 c = *reinterpret_cast<const f32x4*>(sT + j + 4 * v);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              s[0][4 * v + e] = a[e];
              s[1][4 * v + e] = c[e];
            }
          }
        },
        [](const float (&s)[2][16], const int e, float (&v)[5]) {
          const float x = s[0][e], y = s[1][e];
          v[0] = x;
          v[1] = y;
          v[2] = x * x;
          v[3] = y * y;
          v[4] = x * y;
        });
  });
}
// NF staged fields as they are, one after the other
template <int NF>
__device__ __forceinline__ void ssim_hpass_plain(const GaussTaps& g, const float (*in)[kRows * kPitch],
                                                 float (*out)[kRows * kTile]) {
  ssim_hitems([&](const int r, const int q) {
#pragma unroll
    for (int n = 0; n < NF; ++n) {
      ssim_hitem<1, 1>(
          g, r, q, out + n,
          [&](const int j, float (&s)[1][16]) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const f32x4 a = *reinterpret_cast<const f32x4*>(&in[n][j + 4 * v]);
#pragma unroll
              for (int e = 0; e < 4; ++e) s[0][4 * v + e] = a[e];
            }
          },
          [](const float (&s)[1][16], const int e, float (&v)[1]) { v[0] = s[0][e]; });
    }
  });
}

// Vertical pass: m[n][o] = field n at column c, row r0 + o of the tile, from 14 rows of the horizontal pass's output.
// The thread's (c, r0) are ssim_column() / ssim_row0().
__device__ __forceinline__ int ssim_column() { return threadIdx.x & 31; }
__device__ __forceinline__ int ssim_row0() { return (threadIdx.x >> 5) * 4; }
template <int NF>
__device__ __forceinline__ void ssim_vpass(const GaussTaps& g, const float (*in)[kRows * kTile], float (&m)[NF][4]) {
  const int c = ssim_column(), r0 = ssim_row0();
#pragma unroll
  for (int n = 0; n < NF; ++n) {
    float col[14];
#pragma unroll
    for (int j = 0; j < 14; ++j) col[j] = in[n][(r0 + j) * kTile + c];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      float a = 0.f;
#pragma unroll
      for (int j = 0; j < 11; ++j) a = fmaf(g.w[j], col[o + j], a);
      m[n][o] = a;
    }
  }
}

// The index S = (A1 A2) / (B1 B2) of one window from its moments mu_x, mu_y, E[x^2], E[y^2], E[xy]
struct SsimIndex {
  float A1, A2, B1, B2, S;
};
__device__ __forceinline__ SsimIndex ssim_index(const float mx, const float my, const float exx, const float eyy,
                                                const float exy, const float C1, const float C2) {
  const float mxx = mx * mx, myy = my * my, mxy = mx * my;
  const float sxx = exx - mxx, syy = eyy - myy, sxy = exy - mxy;
  SsimIndex s;
  s.A1 = 2.f * mxy + C1;
  s.A2 = 2.f * sxy + C2;
  s.B1 = (mxx + myy) + C1;
  s.B2 = (sxx + syy) + C2;
  s.S = (s.A1 * s.A2) / (s.B1 * s.B2);
  return s;
}

}  // namespace
