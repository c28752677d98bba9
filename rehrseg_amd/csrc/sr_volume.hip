// Stage-1 -> stage-2 volume handoff on the device (utils/sr_utils.py:137-242 inference_flavr, :279-304 zeroonenorm /
// postprocess_flavr; rehrseg_amd/utils/sr_utils.py drives them).  All of it is streaming, HBM-bound work.
//
//   rehr_minmax_f32             min / max of an fp32 array into two order-preserving uint32 codes (atomicMin / atomicMax).
//   rehr_sr_window_gather_f32   the stored (x, y, z, C) volume -> the network input of the windows [w0, w0 + b):
//                               (b, C, 4, Xp, Yp) in NDHWC memory, zero slices at the volume's ends, zero padding
//                               in-plane.  16-byte stores along (y, c).
//   rehr_sr_volume_scatter_f32  the network's (b, C, n_out, Xp, Yp) output (any strides) -> the voxels these windows own
//                               of the (Zo, Y, X) volumes: the image after inv_normalize (fp32), the thresholded label
//                               (uint8), and the running min / max of the written image.  The x <-> y transposition goes
//                               through a 64 x 64 LDS tile, so both the loads (along y) and the stores (along x, 16 bytes
//                               per lane) are coalesced.
//   rehr_stage2_prep_f32        zeroonenorm and the slice-profile blur along x of an (X, Y * Z) image in one pass: every
//                               lane owns 4 consecutive (y, z) voxels and slides a register window of the normalised
//                               values over a chunk of x.
//   rehr_stage2_unc_u8_f32      (zeroonenorm(u) * 255).astype(uint8): truncation to int32, low 8 bits.
//
// Rounding contract: the fp32 operations numpy performs, one rounding each, nothing contracted: inv_normalize is
// x * (max - min) then + min; zeroonenorm is ((v - min) / (max - min)) * 255.  The arithmetic is written with plain
// operators: contract(off) governs those, while the __f*_rn helpers are inlined from a header compiled with
// contraction allowed and would be fused into v_fma.
#include "common.h"
#include "host_util.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;

// wave reduction, then the block's 4 partials through LDS, then one atomic pair per block
__device__ __forceinline__ void block_minmax_commit(float lo, float hi, uint32_t* __restrict__ mm) {
  __shared__ float s_lo[kThreads / 64], s_hi[kThreads / 64];
  lo = wave_min(lo);
  hi = wave_max(hi);
  if ((threadIdx.x & 63) == 0) {
    s_lo[threadIdx.x >> 6] = lo;
    s_hi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) {
      lo = fminf(lo, s_lo[w]);
      hi = fmaxf(hi, s_hi[w]);
    }
    if (lo <= hi) {  // false only when the block saw no element
      atomicMin(mm, f2ord(lo));
      atomicMax(mm + 1, f2ord(hi));
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void minmax_kernel(const float* __restrict__ x, const int64_t n,
                                                          uint32_t* __restrict__ mm) {
  float lo = INFINITY, hi = -INFINITY;
  const int64_t step = (int64_t)gridDim.x * kThreads;
  if (VEC) {
    const int64_t n4 = n >> 2;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < n4; t += step) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + t * 4);
      lo = fminf(fminf(lo, v[0]), fminf(v[1], fminf(v[2], v[3])));
      hi = fmaxf(fmaxf(hi, v[0]), fmaxf(v[1], fmaxf(v[2], v[3])));
    }
    for (int64_t t = n4 * 4 + (int64_t)blockIdx.x * kThreads + threadIdx.x; t < n; t += step) {
      lo = fminf(lo, x[t]);
      hi = fmaxf(hi, x[t]);
    }
  } else {
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < n; t += step) {
      lo = fminf(lo, x[t]);
      hi = fmaxf(hi, x[t]);
    }
  }
  block_minmax_commit(lo, hi, mm);
}

// one thread per 4 consecutive floats of an output row (Yp * C floats, Yp % 16 == 0): 4 / C voxels along y
template <int C>
__global__ __launch_bounds__(kThreads) void window_gather_kernel(const float* __restrict__ vol, float* __restrict__ out,
                                                                 const int X, const int Y, const int Z, const int w0,
                                                                 const int zoff, const int b, const int Xp,
                                                                 const int Yp) {
  constexpr int V = 4 / C;  // voxels per thread
  const int gy = Yp / V;
  const int64_t n = (int64_t)b * 4 * Xp * gy;
  for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < n; t += (int64_t)gridDim.x * kThreads) {
    const int y0 = (int)(t % gy) * V;
    const int x = (int)((t / gy) % Xp);
    const int s = (int)((t / ((int64_t)gy * Xp)) % 4);
    const int bi = (int)(t / ((int64_t)gy * Xp * 4));
    const int z = w0 + bi + zoff + s;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (z >= 0 && z < Z && x < X) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int y = y0 + e;
        if (y < Y) {
          const float* p = vol + (((int64_t)x * Y + y) * Z + z) * C;
#pragma unroll
          for (int c = 0; c < C; ++c) o[e * C + c] = p[c];
        }
      }
    }
    *reinterpret_cast<f32x4*>(out + t * 4) = o;
  }
}

// one block per (window, output slice, 64 x 64 tile of (x, y))
__global__ __launch_bounds__(kThreads) void volume_scatter_kernel(
    const float* __restrict__ net, const int64_t sb, const int64_t sc, const int64_t st, const int64_t sx,
    const int64_t sy, const int n_out, const int X, const int Y, const int w0, const uint32_t* __restrict__ in_mm,
    float* __restrict__ img, uint8_t* __restrict__ seg, uint32_t* __restrict__ out_mm, const int tiles_x,
    const int tiles_y) {
  __shared__ float tile[2][kTile][kTile + 1];
  int blk = blockIdx.x;
  const int ty = blk % tiles_y;
  blk /= tiles_y;
  const int tx = blk % tiles_x;
  blk /= tiles_x;
  const int s = blk % n_out;
  const int bi = blk / n_out;
  const int x0 = tx * kTile, y0 = ty * kTile;
  const bool has_seg = seg != nullptr;
  const float vmin = ord2f(in_mm[0]);
  const float scale = (ord2f(in_mm[1]) - vmin);
  const float* src = net + bi * sb + s * st;
  // load: lanes along y (the source's fast spatial axis)
  {
    const int j = threadIdx.x & 63;
    const int y = y0 + j;
    for (int i = threadIdx.x >> 6; i < kTile; i += kThreads / 64) {
      const int x = x0 + i;
      if (x < X && y < Y) {
        const float* p = src + x * sx + y * sy;
        tile[0][i][j] = p[0];
        if (has_seg) tile[1][i][j] = p[sc];
      }
    }
  }
  __syncthreads();
  // store: 16 lanes x 4 voxels along x per row of y
  const int64_t zo = (int64_t)(w0 + bi) * n_out + s;
  float lo = INFINITY, hi = -INFINITY;
  const int i4 = (threadIdx.x & 15) * 4;
  const bool vec = (X & 3) == 0;
  for (int j = threadIdx.x >> 4; j < kTile; j += kThreads / 16) {
    const int y = y0 + j, x = x0 + i4;
    if (y >= Y || x >= X) continue;
    const int64_t o = (zo * Y + y) * X + x;
    f32x4 v;
    uint8_t l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = x + e < X;
      v[e] = in ? ((tile[0][i4 + e][j] * scale) + vmin) : 0.f;
      if (in) {
        lo = fminf(lo, v[e]);
        hi = fmaxf(hi, v[e]);
      }
      l[e] = (has_seg && in && ((tile[1][i4 + e][j] * scale) + vmin) > 0.f) ? 1 : 0;
    }
    if (vec) {  // X % 4 == 0: x + 3 < X, and both rows are 16- / 4-byte aligned
      *reinterpret_cast<f32x4*>(img + o) = v;
      if (has_seg) *reinterpret_cast<uint32_t*>(seg + o) = l[0] | (l[1] << 8) | (l[2] << 16) | ((uint32_t)l[3] << 24);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (x + e < X) {
          img[o + e] = v[e];
          if (has_seg) seg[o + e] = l[e];
        }
    }
  }
  block_minmax_commit(lo, hi, out_mm);
}

// P = Y * Z voxels per x; thread = 4 consecutive voxels of the plane (VEC: one 16-byte access) and one chunk of x
template <int LMAX, bool VEC>
__global__ __launch_bounds__(kThreads) void stage2_prep_kernel(const float* __restrict__ img,
                                                               const uint32_t* __restrict__ mm,
                                                               const float* __restrict__ taps, const int L,
                                                               float* __restrict__ out, const int X, const int64_t P,
                                                               const int chunk) {
  const int64_t groups = (P + 3) >> 2;
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= groups) return;
  const int64_t p0 = g * 4;
  const int xa = blockIdx.y * chunk;
  const int xb = min(X, xa + chunk);
  const int left = (L - 1) / 2;
  const float vmin = ord2f(mm[0]);
  const float range = (ord2f(mm[1]) - vmin);
  float k[LMAX];
#pragma unroll
  for (int t = 0; t < LMAX; ++t) k[t] = t < L ? taps[t] : 0.f;
  // win[t] holds the normalised voxels of x + t - left (zero outside the axis and for t >= L)
  f32x4 win[LMAX];
  auto fetch = [&](int xs) -> f32x4 {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (xs < 0 || xs >= X) return v;
    const float* p = img + (int64_t)xs * P + p0;
    if (VEC) {
      v = *reinterpret_cast<const f32x4*>(p);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (p0 + e < P) v[e] = p[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ((v[e] - vmin) / range) * 255.0f;
    return v;
  };
#pragma unroll
  for (int t = 0; t < LMAX; ++t) win[t] = (t >= 1 && t < L) ? fetch(xa + t - 1 - left) : f32x4{0.f, 0.f, 0.f, 0.f};
  for (int x = xa; x < xb; ++x) {
    // slide by one: drop x - 1 - left, take in x + L - 1 - left
#pragma unroll
    for (int t = 0; t + 1 < LMAX; ++t) win[t] = win[t + 1];
    const f32x4 in = fetch(x + L - 1 - left);
#pragma unroll
    for (int t = 0; t < LMAX; ++t)
      if (t == L - 1) win[t] = in;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < LMAX; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = (acc[e] + (k[t] * win[t][e]));
    float* q = out + (int64_t)x * P + p0;
    if (VEC) {
      *reinterpret_cast<f32x4*>(q) = acc;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (p0 + e < P) q[e] = acc[e];
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void unc_u8_kernel(const float* __restrict__ u, const uint32_t* __restrict__ mm,
                                                          uint8_t* __restrict__ out, const int64_t n) {
  const float vmin = ord2f(mm[0]);
  const float range = (ord2f(mm[1]) - vmin);
  auto cast = [&](float v) -> uint32_t {
    const float q = (((v - vmin) / range) * 255.0f) * 255.0f;
    return (uint32_t)(int32_t)q & 0xffu;
  };
  const int64_t step = (int64_t)gridDim.x * kThreads;
  if (VEC) {
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < (n >> 2); t += step) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(u + t * 4);
      *reinterpret_cast<uint32_t*>(out + t * 4) = cast(v[0]) | (cast(v[1]) << 8) | (cast(v[2]) << 16) | (cast(v[3]) << 24);
    }
    for (int64_t t = (n >> 2) * 4 + (int64_t)blockIdx.x * kThreads + threadIdx.x; t < n; t += step)
      out[t] = (uint8_t)cast(u[t]);
  } else {
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < n; t += step) out[t] = (uint8_t)cast(u[t]);
  }
}

}  // namespace

extern "C" int rehr_minmax_f32(const float* x, int64_t n, uint32_t* minmax, void* stream) {
  if (x == nullptr || minmax == nullptr || n < 1 || misaligned(4, x)) return REHR_EINVAL;
  if (!misaligned(16, x))
    hipLaunchKernelGGL(minmax_kernel<true>, dim3(grid_for(n / 4 + 1, kThreads, 2048)), dim3(kThreads), 0,
                       (hipStream_t)stream, x, n, minmax);
  else
    hipLaunchKernelGGL(minmax_kernel<false>, dim3(grid_for(n, kThreads, 2048)), dim3(kThreads), 0, (hipStream_t)stream,
                       x, n, minmax);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_sr_window_gather_f32(const float* vol, float* out, int32_t X, int32_t Y, int32_t Z, int32_t C,
                                         int32_t w0, int32_t b, int32_t Xp, int32_t Yp, void* stream) {
  if (vol == nullptr || out == nullptr) return REHR_EINVAL;
  if (X < 1 || Y < 1 || Z < 2 || (C != 1 && C != 2)) return REHR_EINVAL;
  if (w0 < 0 || b < 1 || (int64_t)w0 + b > Z - 1) return REHR_EINVAL;
  if (Xp < X || Yp < Y || Xp % 16 || Yp % 16) return REHR_EINVAL;
  if (misaligned(16, out) || misaligned(4, vol)) return REHR_EINVAL;
  if ((int64_t)X * Y * Z * C >= ((int64_t)1 << 40) || (int64_t)b * 4 * Xp * Yp * C >= ((int64_t)1 << 40))
    return REHR_EINVAL;
  const int zoff = Z == 2 ? -2 : -1;  // the two-slice volume's single window is padded in front (:116-118)
  const int64_t n = (int64_t)b * 4 * Xp * Yp * C / 4;
  if (C == 1)
    hipLaunchKernelGGL(window_gather_kernel<1>, dim3(grid_for(n, kThreads, 16384)), dim3(kThreads), 0,
                       (hipStream_t)stream, vol, out, X, Y, Z, w0, zoff, b, Xp, Yp);
  else
    hipLaunchKernelGGL(window_gather_kernel<2>, dim3(grid_for(n, kThreads, 16384)), dim3(kThreads), 0,
                       (hipStream_t)stream, vol, out, X, Y, Z, w0, zoff, b, Xp, Yp);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_sr_volume_scatter_f32(const float* net, const int64_t* strides, int32_t b, int32_t C, int32_t n_out,
                                          int32_t X, int32_t Y, int32_t w0, int32_t n_windows,
                                          const uint32_t* in_minmax, float* img, uint8_t* seg, uint32_t* out_minmax,
                                          void* stream) {
  if (net == nullptr || strides == nullptr || in_minmax == nullptr || img == nullptr || out_minmax == nullptr)
    return REHR_EINVAL;
  if (b < 1 || C < 1 || n_out < 1 || X < 1 || Y < 1 || w0 < 0 || (int64_t)w0 + b > n_windows) return REHR_EINVAL;
  if (seg != nullptr && C < 2) return REHR_EINVAL;
  for (int a = 0; a < 5; ++a)
    if (strides[a] < 0) return REHR_EINVAL;
  if (misaligned(4, net, img)) return REHR_EINVAL;
  if ((int64_t)n_windows * n_out * X * Y >= ((int64_t)1 << 40)) return REHR_EINVAL;
  const int tiles_x = (X + kTile - 1) / kTile, tiles_y = (Y + kTile - 1) / kTile;
  const int64_t blocks = (int64_t)b * n_out * tiles_x * tiles_y;
  if (blocks > 0x7fffffff) return REHR_EINVAL;
  // the vector stores need 16-byte rows: X % 4 == 0 and an aligned base; otherwise the kernel's scalar path runs, which
  // it selects by X % 4 alone, so a misaligned base with X % 4 == 0 is refused here
  if (X % 4 == 0 && (misaligned(16, img) || misaligned(4, seg))) return REHR_EINVAL;
  hipLaunchKernelGGL(volume_scatter_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, net,
                     strides[0], strides[1], strides[2], strides[3], strides[4], n_out, X, Y, w0, in_minmax, img, seg,
                     out_minmax, tiles_x, tiles_y);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_stage2_prep_f32(const float* img, const uint32_t* minmax, const float* taps, int32_t L, float* out,
                                    int32_t X, int64_t P, void* stream) {
  if (img == nullptr || minmax == nullptr || taps == nullptr || out == nullptr) return REHR_EINVAL;
  if (L < 1 || X < 1 || P < 1 || X * P >= ((int64_t)1 << 40)) return REHR_EINVAL;
  if (L > 32) return REHR_ENOSUP;
  if (img == out || misaligned(4, img, out)) return REHR_EINVAL;
  const bool vec = P % 4 == 0 && !misaligned(16, img, out);
  const int chunk = X < 64 ? X : 64;  // every chunk re-reads L - 1 rows of its neighbours
  const dim3 grid((unsigned)(((P + 3) / 4 + kThreads - 1) / kThreads), (unsigned)((X + chunk - 1) / chunk));
  if (grid.y > 65535) return REHR_ENOSUP;
#define REHR_PREP(LMAX)                                                                                             \
  do {                                                                                                              \
    if (vec)                                                                                                        \
      hipLaunchKernelGGL((stage2_prep_kernel<LMAX, true>), grid, dim3(kThreads), 0, (hipStream_t)stream, img, minmax, \
                         taps, L, out, X, P, chunk);                                                                \
    else                                                                                                            \
      hipLaunchKernelGGL((stage2_prep_kernel<LMAX, false>), grid, dim3(kThreads), 0, (hipStream_t)stream, img,      \
                         minmax, taps, L, out, X, P, chunk);                                                        \
  } while (0)
  if (L <= 8)
    REHR_PREP(8);
  else if (L <= 16)
    REHR_PREP(16);
  else
    REHR_PREP(32);
#undef REHR_PREP
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_stage2_unc_u8_f32(const float* u, const uint32_t* minmax, uint8_t* out, int64_t n, void* stream) {
  if (u == nullptr || minmax == nullptr || out == nullptr || n < 1 || misaligned(4, u)) return REHR_EINVAL;
  if (!misaligned(16, u) && !misaligned(4, out))
    hipLaunchKernelGGL(unc_u8_kernel<true>, dim3(grid_for(n / 4 + 1, kThreads, 4096)), dim3(kThreads), 0,
                       (hipStream_t)stream, u, minmax, out, n);
  else
    hipLaunchKernelGGL(unc_u8_kernel<false>, dim3(grid_for(n, kThreads, 4096)), dim3(kThreads), 0, (hipStream_t)stream,
                       u, minmax, out, n);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}
