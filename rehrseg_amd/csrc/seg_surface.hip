// Stage-2 validation on the device, boundary metrics: the Hausdorff distance, its 95th percentile and the average
// symmetric surface distance of two label maps, in the physical units of a per-axis voxel spacing.
//
//   rehr_seg_surface_dist_f32    the surface voxels of both maps (a foreground voxel with a background face neighbour;
//                                outside the volume is background), their exact counts, the exact squared Euclidean
//                                distance transform to either surface, and the distance of every surface voxel of one
//                                map to the surface of the other in a 2 x D*H*W buffer (+inf at the other voxels).
//   rehr_seg_surface_reduce_f64  hd, hd95 and assd in fp64 from that buffer, its ascending sort and the two counts, all
//                                read from device memory.
//
// The distance transform is three separable min-plus passes over fp32 fields, W then H then D:
// out[i] = min_j (in[j] + ((i - j) * s)^2), the field holding +inf where no surface voxel has been seen yet.  The term
// is formed from the integer offset, t = (float)(i - j) * s, t * t, and added in fp32; rounding is monotone, so the
// minimum over j of the rounded sums is the rounded sum at the nearest surface voxel: every result is
// fl(fl(tw^2 + th^2) + td^2) of one surface voxel, the minimum of that expression over all of them, with no branch and
// no intersection point that could pick the wrong parabola at a near-tie.  Nothing is contracted to an FMA.
//
// W pass: a block owns 64 outputs along x (one per lane) of 16 rows (4 per wave) and walks the row in steps of 64
// source positions staged in LDS from the surface bits as 0 / +inf, both fields at once (8 KiB); the term is shared by
// the 8 minima of a thread.  H and D pass: a block owns 64 adjacent columns (one per lane, so every global access is
// one contiguous 256-byte row) and 32 outputs along the line (8 per wave) and walks the line in steps of 64 source
// positions staged in LDS (16 KiB).  The D pass takes the square root and writes the distance buffer directly.
// No pass holds a whole line, so an axis may have any length up to REHR_SEG_SURFACE_MAX_AXIS.
//
// The sums of the reduction are fp64 over a fixed partition (256 blocks, a butterfly per wave, the waves in order, then
// the 256 slots the same way): the same bits on every run.  The counts are integer atomics, whose sum is order-free.
#include <math.h>

#include "common.h"
#include "host_util.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kStep = 64;       // source positions staged per step
constexpr int kLanes = 64;      // outputs along x (W pass) / adjacent columns (line pass) per block
constexpr int kRowsW = 16;      // W pass: rows per block, 4 per wave
constexpr int kOutLine = 32;    // line pass: outputs along the line per block, 8 per wave
constexpr int kParts = 256;     // blocks (and slots) of the fixed-order sum
constexpr int64_t kMaxVoxels = (int64_t)1 << 30;
constexpr int64_t kPartsBytes = kParts * 2 * (int64_t)sizeof(double);

__device__ __forceinline__ bool fg(const uint8_t* __restrict__ m, int64_t i) { return m[i] != 0; }

// bit 0: surface voxel of pred, bit 1: of gt; grid-stride, one voxel per thread and step
__global__ __launch_bounds__(kThreads) void surface_kernel(const uint8_t* __restrict__ pred,
                                                           const uint8_t* __restrict__ gt, const int D, const int H,
                                                           const int W, uint8_t* __restrict__ surf,
                                                           unsigned long long* __restrict__ counts) {
  const int64_t HW = (int64_t)H * W, N = (int64_t)D * HW;
  unsigned np = 0, ng = 0;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < N; v += (int64_t)gridDim.x * kThreads) {
    const int x = (int)(v % W), y = (int)((v / W) % H), z = (int)(v / HW);
    const bool inner = x > 0 && x < W - 1 && y > 0 && y < H - 1 && z > 0 && z < D - 1;
    uint8_t bits = 0;
    if (fg(pred, v)) {
      const bool covered = inner && fg(pred, v - 1) && fg(pred, v + 1) && fg(pred, v - W) && fg(pred, v + W) &&
                           fg(pred, v - HW) && fg(pred, v + HW);
      if (!covered) bits |= 1;
    }
    if (fg(gt, v)) {
      const bool covered = inner && fg(gt, v - 1) && fg(gt, v + 1) && fg(gt, v - W) && fg(gt, v + W) &&
                           fg(gt, v - HW) && fg(gt, v + HW);
      if (!covered) bits |= 2;
    }
    surf[v] = bits;
    np += bits & 1;
    ng += bits >> 1;
  }
  np = wave_sum(np);
  ng = wave_sum(ng);
  if ((threadIdx.x & 63) == 0) {
    if (np) atomicAdd(counts, (unsigned long long)np);
    if (ng) atomicAdd(counts + 1, (unsigned long long)ng);
  }
}

// rows = D * H lines of W surface bytes -> fp[row][x], fg_[row][x] = min over the surface voxels j of the row of
// ((x - j) * sw)^2, +inf for a row without one
__global__ __launch_bounds__(kThreads) void edt_w_kernel(const uint8_t* __restrict__ surf, float* __restrict__ fp,
                                                         float* __restrict__ fg_, const int64_t rows, const int W,
                                                         const float sw, const int xtiles) {
  __shared__ __attribute__((aligned(16))) float sIn[2][kRowsW][kStep];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int xt = (int)(blockIdx.x % (unsigned)xtiles);
  const int64_t row0 = (int64_t)(blockIdx.x / (unsigned)xtiles) * kRowsW;
  const int x = xt * kLanes + lane;
  float acc[2][4];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[f][r] = INFINITY;

  for (int j0 = 0; j0 < W; j0 += kStep) {
    __syncthreads();
    {
      const int r = threadIdx.x >> 4, jj = (threadIdx.x & 15) * 4;
      const int64_t row = row0 + r;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = j0 + jj + e;
        const uint8_t b = (row < rows && j < W) ? surf[row * W + j] : (uint8_t)0;
        sIn[0][r][jj + e] = (b & 1) ? 0.f : INFINITY;
        sIn[1][r][jj + e] = (b & 2) ? 0.f : INFINITY;
      }
    }
    __syncthreads();
    const float d0 = (float)(x - j0);
    for (int jj = 0; jj < kStep; jj += 4) {
      float t2[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t = (d0 - (float)(jj + e)) * sw;   // (float)(x - j): small integers, exact
        t2[e] = t * t;
      }
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(&sIn[f][wave * 4 + r][jj]);   // one address per wave
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[f][r] = fminf(acc[f][r], v[e] + t2[e]);
        }
    }
  }
  if (x < W) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = row0 + wave * 4 + r;
      if (row < rows) {
        fp[row * W + x] = acc[0][r];
        fg_[row * W + x] = acc[1][r];
      }
    }
  }
}

// in, out: [O][L][C]; out[o][i][c] = min_j (in[o][j][c] + ((i - j) * sp)^2).  GATHER (the last pass: O = 2 fields,
// L = D, C = H * W = N / D): instead, dist[(1 - o) * N + i * C + c] = sqrt of that where the voxel is a surface voxel
// of the other map (field 0 is the distance to pred's surface and is read at gt's surface voxels), +inf elsewhere.
template <bool GATHER>
__global__ __launch_bounds__(kThreads) void edt_line_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            const int L, const int64_t C, const float sp,
                                                            const int64_t ctiles, const int itiles,
                                                            const uint8_t* __restrict__ surf) {
  __shared__ float sIn[kStep][kLanes];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = blockIdx.x;
  const int64_t c = (b % ctiles) * kLanes + lane;
  const int i0 = (int)((b / ctiles) % itiles) * kOutLine + wave * 8;
  const int64_t o = b / (ctiles * itiles);
  const float* src = in + o * L * C;
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = INFINITY;

  for (int j0 = 0; j0 < L; j0 += kStep) {
    __syncthreads();
    for (int k = wave; k < kStep; k += 4) {
      const int j = j0 + k;
      sIn[k][lane] = (j < L && c < C) ? src[(int64_t)j * C + c] : INFINITY;
    }
    __syncthreads();
    const float d0 = (float)(i0 - j0);
#pragma unroll 4
    for (int jj = 0; jj < kStep; ++jj) {
      const float v = sIn[jj][lane];
      const float dj = d0 - (float)jj;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float t = (dj + (float)k) * sp;   // (float)(i - j): small integers, exact
        acc[k] = fminf(acc[k], v + t * t);
      }
    }
  }
  if (c < C) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = i0 + k;
      if (i >= L) continue;
      const int64_t v = (int64_t)i * C + c;
      if (GATHER) {
        const int64_t N = (int64_t)L * C;
        const bool on = surf[v] & (o == 0 ? 2 : 1);
        out[(1 - o) * N + v] = on ? sqrtf(acc[k]) : INFINITY;
      } else {
        out[o * L * C + v] = acc[k];
      }
    }
  }
}

// every thread returns the block's sum, in the order of common.h's block sums; the leading barrier lets `red` be
// used again right after a call
__device__ __forceinline__ double block_sum(double v, double (*red)[1]) {
  double a[1] = {v};
  __syncthreads();
  block_partials(a, red);
  return wave_order_sum(red, 0);
}

// parts[b][f] = the sum of the finite entries of dist[f][b * 256 + t + k * kParts * 256], a fixed partition
__global__ __launch_bounds__(kThreads) void surface_sum_kernel(const float* __restrict__ dist, const int64_t N,
                                                               double* __restrict__ parts) {
  __shared__ double red[kThreads / 64][1];
  double s0 = 0.0, s1 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (int64_t)kParts * kThreads) {
    const float a = dist[i], b = dist[N + i];
    if (a < INFINITY) s0 += (double)a;
    if (b < INFINITY) s1 += (double)b;
  }
  s0 = block_sum(s0, red);
  s1 = block_sum(s1, red);
  if (threadIdx.x == 0) {
    parts[blockIdx.x * 2] = s0;
    parts[blockIdx.x * 2 + 1] = s1;
  }
}

// one block: out = {hd, hd95, assd}; NaN when either surface is empty
__global__ __launch_bounds__(kThreads) void surface_finish_kernel(const double* __restrict__ parts,
                                                                  const float* __restrict__ sorted,
                                                                  const unsigned long long* __restrict__ counts,
                                                                  const int64_t N, double* __restrict__ out) {
  __shared__ double red[kThreads / 64][1];
  const double s0 = block_sum(parts[threadIdx.x * 2], red);
  const double s1 = block_sum(parts[threadIdx.x * 2 + 1], red);
  if (threadIdx.x != 0) return;
  const unsigned long long np = counts[0], ng = counts[1];
  if (np == 0 || ng == 0 || np > (unsigned long long)N || ng > (unsigned long long)N) {
    out[0] = out[1] = out[2] = (double)NAN;
    return;
  }
  const int64_t n = (int64_t)(np + ng);
  // numpy.percentile(v, 95), method 'linear': the index 0.95 * (n - 1) and numpy's two-sided lerp
  const double h = 0.95 * (double)(n - 1);
  const double lo = floor(h), t = h - lo;
  const int64_t k0 = (int64_t)lo, k1 = k0 + 1 < n ? k0 + 1 : n - 1;
  const double a = (double)sorted[k0], b = (double)sorted[k1], diff = b - a;
  out[0] = (double)sorted[n - 1];
  out[1] = t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
  out[2] = (s0 / (double)np + s1 / (double)ng) / 2.0;
}

int check_extent(int32_t D, int32_t H, int32_t W) {
  if (D < 1 || H < 1 || W < 1) return REHR_EINVAL;
  if (D > REHR_SEG_SURFACE_MAX_AXIS || H > REHR_SEG_SURFACE_MAX_AXIS || W > REHR_SEG_SURFACE_MAX_AXIS)
    return REHR_ENOSUP;
  if ((int64_t)D * H * W > kMaxVoxels) return REHR_ENOSUP;
  return REHR_OK;
}

inline bool good_spacing(float s) { return s > 0.f && s < INFINITY; }   // false for NaN

// workspace: [256 x 2 doubles of the sum][field pair A: 2N floats][field pair B: 2N floats][surface bits: N bytes]
struct Layout {
  double* parts;
  float *A, *B;
  uint8_t* surf;
  int64_t bytes;
};
Layout layout(void* base, int64_t N) {
  Carver c(base);   // a braced list is evaluated left to right
  return {c.take<double>(kParts * 2), c.take<float>(2 * N), c.take<float>(2 * N), c.take<uint8_t>(N), c.bytes()};
}

}  // namespace

extern "C" int64_t rehr_seg_surface_workspace_bytes(int32_t D, int32_t H, int32_t W) {
  const int rc = check_extent(D, H, W);
  if (rc != REHR_OK) return rc;
  return layout(nullptr, (int64_t)D * H * W).bytes;
}

extern "C" int rehr_seg_surface_dist_f32(const uint8_t* pred, const uint8_t* gt, int32_t D, int32_t H, int32_t W,
                                         float sd, float sh, float sw, float* dist, uint64_t* counts, void* workspace,
                                         int64_t workspace_bytes, void* stream) {
  if (pred == nullptr || gt == nullptr || dist == nullptr || counts == nullptr || workspace == nullptr)
    return REHR_EINVAL;
  const int rc = check_extent(D, H, W);
  if (rc != REHR_OK) return rc;
  if (!good_spacing(sd) || !good_spacing(sh) || !good_spacing(sw)) return REHR_EINVAL;
  const int64_t N = (int64_t)D * H * W, HW = (int64_t)H * W;
  const auto [parts, A, B, surf, need] = layout(workspace, N);
  if (workspace_bytes < need) return REHR_EINVAL;
  if (misaligned(16, workspace) || misaligned(4, dist) || misaligned(8, counts)) return REHR_EINVAL;
  hipStream_t st = (hipStream_t)stream;

  hipLaunchKernelGGL(surface_kernel, dim3(grid_for(N, kThreads, 4096)), dim3(kThreads), 0, st, pred, gt, D, H, W, surf,
                     reinterpret_cast<unsigned long long*>(counts));
  // every grid below is at most 2^23 blocks: axes <= 2048 and N <= 2^30
  const int64_t rows = (int64_t)D * H;
  const int xtiles = (W + kLanes - 1) / kLanes;
  hipLaunchKernelGGL(edt_w_kernel, dim3((unsigned)(xtiles * ((rows + kRowsW - 1) / kRowsW))), dim3(kThreads), 0, st,
                     surf, A, A + N, rows, W, sw, xtiles);
  {
    const int64_t ctiles = (W + kLanes - 1) / kLanes;   // [2 * D][H][W]
    const int itiles = (H + kOutLine - 1) / kOutLine;
    hipLaunchKernelGGL(edt_line_kernel<false>, dim3((unsigned)(ctiles * itiles * 2 * D)), dim3(kThreads), 0, st, A, B,
                       H, (int64_t)W, sh, ctiles, itiles, (const uint8_t*)nullptr);
  }
  {
    const int64_t ctiles = (HW + kLanes - 1) / kLanes;  // [2][D][H * W]
    const int itiles = (D + kOutLine - 1) / kOutLine;
    hipLaunchKernelGGL(edt_line_kernel<true>, dim3((unsigned)(ctiles * itiles * 2)), dim3(kThreads), 0, st, B, dist, D,
                       HW, sd, ctiles, itiles, (const uint8_t*)surf);
  }
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_seg_surface_reduce_f64(const float* dist, const float* sorted, const uint64_t* counts, int64_t N,
                                           double* out, void* workspace, int64_t workspace_bytes, void* stream) {
  if (dist == nullptr || sorted == nullptr || counts == nullptr || out == nullptr || workspace == nullptr)
    return REHR_EINVAL;
  if (N < 1) return REHR_EINVAL;
  if (N > kMaxVoxels) return REHR_ENOSUP;
  if (workspace_bytes < kPartsBytes) return REHR_EINVAL;
  if (misaligned(8, workspace, out, counts) || misaligned(4, dist, sorted)) return REHR_EINVAL;
  double* parts = static_cast<double*>(workspace);   // a buffer of its own will do: kPartsBytes on a multiple of 8
  hipLaunchKernelGGL(surface_sum_kernel, dim3(kParts), dim3(kThreads), 0, (hipStream_t)stream, dist, N, parts);
  hipLaunchKernelGGL(surface_finish_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (const double*)parts,
                     sorted, reinterpret_cast<const unsigned long long*>(counts), N, out);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}
