// Stage-2 validation on the device, connected components and lesion-wise scores.
//
//   rehr_seg_cc_roots_i32    roots[v] = the smallest linear index of v's component (6-, 18- or 26-connectivity),
//                            -1 at background voxels; four launches, none depending on anything read back.
//   rehr_seg_cc_lesion_i64   the eight lesion-wise integers of two root maps; four launches.
//   rehr_seg_cc_compact_i32  labels 1..n in the order of the roots from an inclusive prefix sum of (roots[v] == v).
//
// Labelling: union-find over voxel indices, the parent array is `roots`, a parent is never larger than its child.
//   init      a wave walks a row in steps of 64 voxels; a ballot gives every foreground voxel the first voxel of its
//             run along W (the run start of the previous step is carried over).  Background: -1.
//   merge     every foreground voxel unites itself with the foreground neighbours in the rows in front of it (the row
//             above in its slice and the rows of the slice above), per-axis bounds checks, no wrap-around.  A union is
//             left out when the voxel to the left, or the neighbour's left voxel, already stands for it (same run).
//             unite() follows parent words to two candidates and hooks the larger under the smaller with atomicMin.
//             The loads on the way are relaxed agent-scope loads and only hints: a stale word is a value the parent
//             held earlier, i.e. a voxel of the same component with a larger index.  What decides is the value the
//             atomic returns: `old == a` means a was a root and now hangs under b; anything else is a's true parent
//             at that instant, and the pair (old, b) is united instead.  max(a, b) falls with every round, so the loop
//             ends without waiting for any other workgroup.  Only run starts and roots are ever hooked.
//   compress  (its own launch) every run start walks to its root and stores it, relaxed agent-scope loads and stores:
//             a word holds either its value after the merge launch or its final root, and both lead to the root.
//   spread    (its own launch) every other voxel takes the root of its run start: reads run-start words only, writes
//             the other words only.
// The root of a tree is its smallest index and a tree is a component once every adjacent pair has been united, so the
// result is a function of the mask alone.
//
// Lesion statistics: sizes, overlaps and hit flags live in workspace arrays indexed by root.  A wave first sums over
// the lanes that share a root with ballots and keeps the heaviest root of its chunk in registers, then issues one
// atomic per root and step (one per chunk for the cached root); the counts per wave go to `out` with one atomic per
// wave; the largest component is an atomicMax of (size << 32) | (0xffffffff - root), which prefers the smaller root
// among equal sizes.
#include "common.h"
#include "host_util.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 4096;
constexpr int64_t kMaxVoxels = (int64_t)1 << 30;
constexpr int64_t kHeaderBytes = 64;     // keys[0]: largest predicted component, keys[1]: largest of the label

typedef unsigned long long u64;

__device__ __forceinline__ int ld_hint(const int* p, int i) {
  return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// some voxel of i's component that is no larger than i: the root if no word on the way is stale
__device__ __forceinline__ int find_hint(const int* p, int i) {
  int q;
  while ((q = ld_hint(p, i)) < i && q >= 0) i = q;
  return i;
}

__device__ __forceinline__ void unite(int* p, int a, int b) {
  a = find_hint(p, a);
  b = find_hint(p, b);
  while (a != b) {
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(p + a, b);
    if (old == a) break;          // a was a root; it hangs under b now
    a = find_hint(p, old);        // a's parent at that instant (the word is min(old, b) now): go on with (old, b)
    b = find_hint(p, b);
  }
}

// one wave per row of W voxels, grid-stride over the D * H rows
__global__ __launch_bounds__(kThreads) void cc_init_kernel(const uint8_t* __restrict__ mask, const int64_t rows,
                                                           const int W, int* __restrict__ roots) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  for (int64_t row = wave0; row < rows; row += (int64_t)gridDim.x * kWaves) {
    const int64_t base = row * W;
    int carry = -1;                                  // start of the run that reaches the end of the previous step
    for (int x0 = 0; x0 < W; x0 += 64) {
      const int x = x0 + lane;
      const bool f = x < W && mask[base + x] != 0;
      const u64 ball = __ballot(f);
      const u64 gaps = ~ball;
      const u64 below = gaps & ((1ull << lane) - 1);   // background lanes in front of this one
      const int first = carry >= 0 ? carry : x0;
      const int start = below ? x0 + 64 - __clzll((long long)below) : first;
      if (x < W) roots[base + x] = f ? (int)(base + start) : -1;
      if (ball >> 63)
        carry = gaps ? x0 + 64 - __clzll((long long)gaps) : first;
      else
        carry = -1;
    }
  }
}

// MAXNZ: how many axes of a neighbour offset may be non-zero (1: faces, 2: + edges, 3: + corners)
template <int MAXNZ>
__global__ __launch_bounds__(kThreads) void cc_merge_kernel(const uint8_t* __restrict__ mask, const int D, const int H,
                                                            const int W, int* __restrict__ roots) {
  const int N = D * H * W;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kThreads) {
    const int v = (int)i;
    if (mask[v] == 0) continue;
    const int x = v % W, y = (v / W) % H, z = v / (W * H);
    const bool left = x > 0 && mask[v - 1] != 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int dz = k == 0 ? 0 : -1, dy = k == 0 ? -1 : k - 2;       // (0,-1) (-1,-1) (-1,0) (-1,1)
      const int nz = (dz != 0) + (dy != 0);
      if (nz > MAXNZ) continue;
      const bool wide = nz + 1 <= MAXNZ;                              // dx = -1, 0, 1; else dx = 0 only
      const int zz = z + dz, yy = y + dy;
      if (zz < 0 || yy < 0 || yy >= H) continue;
      const int rb = (zz * H + yy) * W;
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if (!wide && dx != 0) continue;
        const int xx = x + dx;
        if (xx < 0 || xx >= W) continue;
        if (mask[rb + xx] == 0) continue;
        // (v - 1) is in v's run and touches this neighbour itself: it unites the two
        if (left && wide && dx <= 0) continue;
        // the neighbour's left voxel is in its run and touches (v - 1), or v itself at an earlier dx
        if (xx > 0 && mask[rb + xx - 1] != 0 && (left || (wide && dx > -1))) continue;
        unite(roots, v, rb + xx);
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void cc_compress_kernel(const uint8_t* __restrict__ mask, const int N,
                                                               const int W, int* __restrict__ roots) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kThreads) {
    const int v = (int)i;
    if (mask[v] == 0 || (v % W != 0 && mask[v - 1] != 0)) continue;   // run starts only
    const int r = find_hint(roots, v);
    if (r != v) __hip_atomic_store(roots + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(kThreads) void cc_spread_kernel(const int N, int* __restrict__ roots) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kThreads) {
    const int q = roots[i];
    if (q < 0) continue;
    const int r = roots[q];      // q is a run start (or a root): final since the previous launch, not written here
    if (r != q) roots[i] = r;    // only a voxel that is no run start gets here
  }
}

__global__ __launch_bounds__(kThreads) void cc_zero_kernel(uint4* __restrict__ p, const int64_t n16) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n16; i += (int64_t)gridDim.x * kThreads)
    p[i] = make_uint4(0, 0, 0, 0);
}

// The lanes of a wave that hold the same root form a group.  A wave walks a contiguous chunk of the volume in steps
// of 64 voxels and keeps the counts of one root in registers (the heaviest root of the last step that changed it: a
// large component stays there for the whole chunk); every other group costs one atomic per step.  All of it is
// wave-uniform: ballots, a readlane and scalar counts.
struct RootCache {
  int r;
  unsigned n, ov;
};

template <bool FLAG>   // FLAG: the overlap is kept as a hit flag (atomicOr), else as a count (atomicAdd)
__device__ __forceinline__ void cache_flush(const RootCache& c, unsigned* __restrict__ size,
                                            unsigned* __restrict__ ov, const int lane) {
  if (c.r < 0 || lane != 0) return;
  if (c.n) atomicAdd(size + c.r, c.n);
  if (c.ov) {
    if (FLAG)
      atomicOr(ov + c.r, 1u);
    else
      atomicAdd(ov + c.r, c.ov);
  }
}

template <bool FLAG>
__device__ __forceinline__ void count_step(const int r, const u64 both, const int lane, RootCache& c,
                                           unsigned* __restrict__ size, unsigned* __restrict__ ov) {
  u64 todo = __ballot(r >= 0);
  int heavy = -1;
  unsigned heavy_n = 0, cached_n = 0;
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int r0 = __builtin_amdgcn_readlane(r, leader);
    const u64 m = __ballot(r == r0);
    const unsigned n = __popcll(m), o = __popcll(m & both);
    if (r0 == c.r) {
      c.n += n;
      c.ov += o;
      cached_n = n;
    } else {
      if (lane == leader) {
        atomicAdd(size + r0, n);
        if (o) {
          if (FLAG)
            atomicOr(ov + r0, 1u);
          else
            atomicAdd(ov + r0, o);
        }
      }
      if (n > heavy_n) {
        heavy_n = n;
        heavy = r0;
      }
    }
    todo &= ~m;
  }
  if (heavy_n > cached_n) {        // this step's share of `heavy` has gone out already: the cache starts at zero
    cache_flush<FLAG>(c, size, ov, lane);
    c.r = heavy;
    c.n = c.ov = 0;
  }
}

// steps of 64 voxels [first, last) of this wave: `per_wave` consecutive steps each
__device__ __forceinline__ void wave_chunk(const int N, const int per_wave, int64_t* first, int64_t* last) {
  const int64_t steps = ((int64_t)N + 63) / 64;
  const int64_t wave = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  *first = wave * per_wave;
  const int64_t end = *first + per_wave;
  *last = end < steps ? end : steps;
}

__global__ __launch_bounds__(kThreads) void cc_stats_kernel(const int* __restrict__ rp_, const int* __restrict__ rg_,
                                                            const int N, const int per_wave,
                                                            unsigned* __restrict__ sizeP, unsigned* __restrict__ ovP,
                                                            unsigned* __restrict__ sizeG, unsigned* __restrict__ hitG,
                                                            u64* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  int64_t first, last;
  wave_chunk(N, per_wave, &first, &last);
  RootCache cp = {-1, 0, 0}, cg = {-1, 0, 0};
  unsigned n_gt = 0;
  for (int64_t s = first; s < last; ++s) {
    const int64_t i = s * 64 + lane;
    int rp = i < N ? rp_[i] : -1, rg = i < N ? rg_[i] : -1;
    if ((unsigned)rp >= (unsigned)N) rp = -1;       // a word that is no index counts as background: nothing is
    if ((unsigned)rg >= (unsigned)N) rg = -1;       // written outside the arrays whatever the caller passed
    const u64 both = __ballot(rp >= 0 && rg >= 0);
    n_gt += __popcll(__ballot(rg >= 0));
    count_step<false>(rp, both, lane, cp, sizeP, ovP);
    count_step<true>(rg, both, lane, cg, sizeG, hitG);
  }
  cache_flush<false>(cp, sizeP, ovP, lane);
  cache_flush<true>(cg, sizeG, hitG, lane);
  if (lane == 0 && n_gt) atomicAdd(out + 7, (u64)n_gt);
}

__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

__global__ __launch_bounds__(kThreads) void cc_count_kernel(const int* __restrict__ rp_, const int* __restrict__ rg_,
                                                            const int N, const int per_wave,
                                                            const unsigned* __restrict__ sizeP,
                                                            const unsigned* __restrict__ ovP,
                                                            const unsigned* __restrict__ sizeG,
                                                            const unsigned* __restrict__ hitG, u64* __restrict__ keys,
                                                            u64* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  unsigned n_p = 0, n_g = 0, tp_p = 0, tp_g = 0;       // the same in every lane of a wave
  u64 kp = 0, kg = 0;
  int64_t first, last;
  wave_chunk(N, per_wave, &first, &last);
  for (int64_t s = first; s < last; ++s) {
    const int64_t i = s * 64 + lane;
    const bool isp = i < N && rp_[i] == (int)i, isg = i < N && rg_[i] == (int)i;
    n_p += __popcll(__ballot(isp));
    n_g += __popcll(__ballot(isg));
    tp_p += __popcll(__ballot(isp && ovP[i] != 0));
    tp_g += __popcll(__ballot(isg && hitG[i] != 0));
    if (isp) {
      const u64 k = ((u64)sizeP[i] << 32) | (u64)(0xffffffffu - (unsigned)i);
      kp = k > kp ? k : kp;
    }
    if (isg) {
      const u64 k = ((u64)sizeG[i] << 32) | (u64)(0xffffffffu - (unsigned)i);
      kg = k > kg ? k : kg;
    }
  }
  kp = wave_max(kp);
  kg = wave_max(kg);
  if (lane == 0) {
    if (n_p) atomicAdd(out + 0, (u64)n_p);
    if (n_g) atomicAdd(out + 1, (u64)n_g);
    if (tp_p) atomicAdd(out + 2, (u64)tp_p);
    if (tp_g) atomicAdd(out + 3, (u64)tp_g);
    if (kp) atomicMax(keys + 0, kp);
    if (kg) atomicMax(keys + 1, kg);
  }
}

// one thread: the keys are final since the previous launch
__global__ void cc_largest_kernel(const u64* __restrict__ keys, const unsigned* __restrict__ ovP,
                                  u64* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const u64 kp = keys[0], kg = keys[1];
  if (kp) {
    out[4] += kp >> 32;
    out[6] += ovP[0xffffffffu - (unsigned)(kp & 0xffffffffu)];
  }
  if (kg) out[5] += kg >> 32;
}

__global__ __launch_bounds__(kThreads) void cc_compact_kernel(const int* __restrict__ roots, const int N,
                                                              const int* __restrict__ rank, int* __restrict__ labels,
                                                              u64* __restrict__ count) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kThreads) {
    const int r = roots[i];
    labels[i] = (unsigned)r < (unsigned)N ? rank[r] : 0;
    if (i == N - 1) count[0] += (u64)rank[i];
  }
}

int check_extent(int32_t D, int32_t H, int32_t W) {
  if (D < 1 || H < 1 || W < 1) return REHR_ENOSUP;
  if ((int64_t)D * H > kMaxVoxels || (int64_t)D * H * W > kMaxVoxels) return REHR_ENOSUP;
  return REHR_OK;
}

// workspace: [64 bytes: the two packed keys][sizes of pred's components: N uint32][gt voxels inside them: N]
//            [sizes of gt's components: N][their hit flags: N], every array indexed by root
struct Layout {
  u64* keys;
  unsigned *sizeP, *ovP, *sizeG, *hitG;
  int64_t bytes;
};
Layout layout(void* base, int64_t N) {
  Carver c(base);   // a braced list is evaluated left to right
  return {c.take<u64>(kHeaderBytes / 8), c.take<unsigned>(N), c.take<unsigned>(N), c.take<unsigned>(N),
          c.take<unsigned>(N), c.bytes()};
}

}  // namespace

extern "C" int64_t rehr_seg_cc_workspace_bytes(int32_t D, int32_t H, int32_t W) {
  const int rc = check_extent(D, H, W);
  if (rc != REHR_OK) return rc;
  return layout(nullptr, (int64_t)D * H * W).bytes;
}

extern "C" int rehr_seg_cc_roots_i32(const uint8_t* mask, int32_t D, int32_t H, int32_t W, int32_t connectivity,
                                     int32_t* roots, void* workspace, int64_t workspace_bytes, void* stream) {
  if (mask == nullptr || roots == nullptr || workspace == nullptr) return REHR_EINVAL;
  if (connectivity != 6 && connectivity != 18 && connectivity != 26) return REHR_EINVAL;
  const int rc = check_extent(D, H, W);
  if (rc != REHR_OK) return rc;
  const int64_t rows = (int64_t)D * H;
  if (workspace_bytes < layout(workspace, rows * W).bytes || misaligned(4, roots)) return REHR_EINVAL;
  const int N = (int)(rows * W);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_init_kernel, dim3(grid_for(rows, kWaves, kMaxBlocks)), dim3(kThreads), 0, st, mask, rows, W,
                     roots);
  const dim3 grid(grid_for(N, kThreads, kMaxBlocks));
  if (connectivity == 6)
    hipLaunchKernelGGL(cc_merge_kernel<1>, grid, dim3(kThreads), 0, st, mask, D, H, W, roots);
  else if (connectivity == 18)
    hipLaunchKernelGGL(cc_merge_kernel<2>, grid, dim3(kThreads), 0, st, mask, D, H, W, roots);
  else
    hipLaunchKernelGGL(cc_merge_kernel<3>, grid, dim3(kThreads), 0, st, mask, D, H, W, roots);
  hipLaunchKernelGGL(cc_compress_kernel, grid, dim3(kThreads), 0, st, mask, N, W, roots);
  hipLaunchKernelGGL(cc_spread_kernel, grid, dim3(kThreads), 0, st, N, roots);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_seg_cc_lesion_i64(const int32_t* roots_pred, const int32_t* roots_gt, int64_t N, int64_t* out,
                                      void* workspace, int64_t workspace_bytes, void* stream) {
  if (roots_pred == nullptr || roots_gt == nullptr || out == nullptr || workspace == nullptr) return REHR_EINVAL;
  if (N < 1 || N > kMaxVoxels) return REHR_ENOSUP;
  const auto [keys, sizeP, ovP, sizeG, hitG, need] = layout(workspace, N);
  if (workspace_bytes < need) return REHR_EINVAL;
  if (misaligned(16, workspace) || misaligned(8, out) || misaligned(4, roots_pred, roots_gt)) return REHR_EINVAL;
  u64* o = reinterpret_cast<u64*>(out);
  hipStream_t st = (hipStream_t)stream;
  const int n = (int)N;
  hipLaunchKernelGGL(cc_zero_kernel, dim3(grid_for(need / 16, kThreads, kMaxBlocks)), dim3(kThreads), 0, st,
                     static_cast<uint4*>(workspace), need / 16);
  // a wave takes at least 8 consecutive steps of 64 voxels where there are that many; at most 1024 blocks
  const int64_t steps = (N + 63) / 64;
  const unsigned blocks = grid_for(steps, kWaves * 8, 1024);
  const int per_wave = (int)((steps + (int64_t)blocks * kWaves - 1) / ((int64_t)blocks * kWaves));
  hipLaunchKernelGGL(cc_stats_kernel, dim3(blocks), dim3(kThreads), 0, st, roots_pred, roots_gt, n, per_wave, sizeP, ovP,
                     sizeG, hitG, o);
  hipLaunchKernelGGL(cc_count_kernel, dim3(blocks), dim3(kThreads), 0, st, roots_pred, roots_gt, n, per_wave,
                     (const unsigned*)sizeP, (const unsigned*)ovP, (const unsigned*)sizeG, (const unsigned*)hitG, keys,
                     o);
  hipLaunchKernelGGL(cc_largest_kernel, dim3(1), dim3(64), 0, st, (const u64*)keys, (const unsigned*)ovP, o);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}

extern "C" int rehr_seg_cc_compact_i32(const int32_t* roots, int64_t N, const int32_t* rank, int32_t* labels,
                                       int64_t* count, void* stream) {
  if (roots == nullptr || rank == nullptr || labels == nullptr || count == nullptr) return REHR_EINVAL;
  if (N < 1 || N > kMaxVoxels) return REHR_ENOSUP;
  if (misaligned(4, roots, rank, labels) || misaligned(8, count)) return REHR_EINVAL;
  hipLaunchKernelGGL(cc_compact_kernel, dim3(grid_for(N, kThreads, kMaxBlocks)), dim3(kThreads), 0, (hipStream_t)stream,
                     roots, (int)N, rank, labels, reinterpret_cast<u64*>(count));
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}
