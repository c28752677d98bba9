// Class locations on the device: the r-th voxel of a class in linear order, exactly, for R ranks that
// are formed on the device from the class's voxel count -- nothing is read back between the passes.
//
//   rehr_class_locations_u8   count = #{i : label[i] matches value}   (value -1: any non-zero label)
//                             rank_j = (uint64(u[j]) * count) >> 32   (integers only: numpy's uint64 gives the same)
//                             index[j] = the rank_j-th matching i in ascending order, -1 for every j when count == 0
//
// Sizes (the tests derive their shapes from these):
//   vector   16 bytes: one load of one lane
//   kWave    64 lanes * 16 = 1024 voxels: what a wave takes in one step of the select pass
//   kChunk   256 lanes * 16 = 4096 voxels: what a block takes in one step of the count pass, one uint32 per chunk
// A run of N voxels has ceil(N / 4096) chunks (at most 2^19 for N < 2^31).  The N % 16 bytes behind the last whole
// vector are read one by one by the lane whose vector they would be, into a vector filled up with a byte that does
// not match, so the count and the select pass see the same 16-byte words.
//
// Passes, three launches on the caller's stream:
//   count    grid-strided over chunks.  Per lane a SWAR compare of its 16 bytes (0x80 in every matching byte, exact)
//            and a popcount; a wave64 butterfly and four LDS words give the chunk's uint32.
//   scan     one block: the exclusive prefix of the chunk counts in place, tiles of 2048, and count as int64.
//   select   one wave per u[j].  Upper-bound binary search of the prefix: the LAST chunk whose prefix is <= rank, so
//            of a run of equal prefixes (empty chunks) the one that holds matches.  Inside the chunk up to four wave
//            steps: an inclusive scan of the lanes' popcounts across the wave finds the lane that holds the k-th match,
//            and that lane walks its 16 mask bits.
// No atomics and no floating point: the same bits on every run.  The label run is only read.
#include "common.h"
#include "host_util.h"

namespace {

constexpr int kThreads = 256;
constexpr int kVec = 16;                      // bytes per lane and load
constexpr int kWave = 64 * kVec;              // 1024
constexpr int kChunk = kThreads * kVec;       // 4096
constexpr int kScanPer = 8;                   // chunk counts per thread and scan tile
constexpr int kScanTile = kThreads * kScanPer;
constexpr int kMaxCountBlocks = 2048;
constexpr int64_t kMaxN = ((int64_t)1 << 31) - 1;
constexpr int32_t kMaxR = 1 << 20;

inline int64_t chunks_of(int64_t N) { return (N + kChunk - 1) / kChunk; }

// 0x80 in every non-zero byte of x, 0 in the others (the low seven bits cannot carry into the next byte)
__device__ __forceinline__ uint32_t nonzero_bytes(const uint32_t x) {
  return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
}

// 0x80 in every byte of w that matches: pattern = value in all four bytes; any: non-zero bytes match
__device__ __forceinline__ uint32_t match_bytes(const uint32_t w, const uint32_t pattern, const bool any) {
  return any ? nonzero_bytes(w) : (~nonzero_bytes(w ^ pattern) & 0x80808080u);
}

// vector v of the run: a 16-byte load below nvec; the vector behind the last whole one holds the tail bytes, read
// one by one, and `filler` (a byte that does not match) behind them; all filler past that
__device__ __forceinline__ uint4 load_vec(const uint8_t* __restrict__ label, const int64_t v, const int64_t nvec,
                                          const int tail, const uint32_t filler) {
  if (v < nvec) return reinterpret_cast<const uint4*>(label)[v];
  const uint32_t f4 = filler * 0x01010101u;
  uint32_t w[4] = {f4, f4, f4, f4};
  if (v == nvec) {
    const uint8_t* t = label + nvec * kVec;
#pragma unroll
    for (int i = 0; i < kVec - 1; ++i) {
      if (i < tail) w[i >> 2] = (w[i >> 2] & ~(0xffu << (8 * (i & 3)))) | ((uint32_t)t[i] << (8 * (i & 3)));
    }
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

struct Match {
  uint32_t m[4];
  __device__ __forceinline__ uint32_t count() const {
    return (uint32_t)(__popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]));
  }
};

__device__ __forceinline__ Match match_vec(const uint4 w, const uint32_t pattern, const bool any) {
  return {{match_bytes(w.x, pattern, any), match_bytes(w.y, pattern, any), match_bytes(w.z, pattern, any),
           match_bytes(w.w, pattern, any)}};
}

struct Run {
  const uint8_t* label;
  int64_t nvec;         // whole 16-byte vectors
  int32_t tail;         // bytes behind them, 0..15
  int32_t nchunks;
  uint32_t pattern, filler;
  int32_t any;
};

// chunk_count[c] = matches in chunk c.  Every thread of a block runs the same number of steps (the barriers).
__global__ __launch_bounds__(kThreads) void class_count_kernel(const Run run, uint32_t* __restrict__ chunk_count) {
  __shared__ uint32_t part[kThreads / 64];
  const int tid = threadIdx.x;
  for (int32_t c = (int32_t)blockIdx.x; c < run.nchunks; c += (int32_t)gridDim.x) {
    const int64_t v = (int64_t)c * kThreads + tid;
    const Match m = match_vec(load_vec(run.label, v, run.nvec, run.tail, run.filler), run.pattern, run.any != 0);
    const uint32_t s = wave_sum(m.count());
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) chunk_count[c] = ((part[0] + part[1]) + part[2]) + part[3];
    __syncthreads();
  }
}

// inclusive scan across the 64 lanes of a wave
__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v, const int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  return v;
}

// one block: counts[c] becomes the number of matches before chunk c; *count = all matches
__global__ __launch_bounds__(kThreads) void class_scan_kernel(uint32_t* __restrict__ counts, const int32_t nchunks,
                                                              int64_t* __restrict__ count) {
  __shared__ uint32_t wtot[kThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t carry = 0;
  for (int32_t base = 0; base < nchunks; base += kScanTile) {
    const int32_t first = base + tid * kScanPer;
    uint32_t c[kScanPer], s = 0;
#pragma unroll
    for (int e = 0; e < kScanPer; ++e) {
      c[e] = first + e < nchunks ? counts[first + e] : 0u;
      s += c[e];
    }
    const uint32_t incl = wave_inclusive(s, lane);
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t before = carry, total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
      if (w < wave) before += wtot[w];
      total += wtot[w];
    }
    uint32_t run = before + incl - s;
#pragma unroll
    for (int e = 0; e < kScanPer; ++e) {
      if (first + e < nchunks) counts[first + e] = run;
      run += c[e];
    }
    carry += total;
    __syncthreads();
  }
  if (tid == 0) *count = (int64_t)carry;
}

// one wave per fraction; prefix: class_scan_kernel's, count: its total
__global__ __launch_bounds__(kThreads) void class_select_kernel(const Run run, const uint32_t* __restrict__ prefix,
                                                                const int64_t* __restrict__ count,
                                                                const uint32_t* __restrict__ u, const int32_t R,
                                                                int32_t* __restrict__ index) {
  const int lane = threadIdx.x & 63;
  const int32_t j = (int32_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (j >= R) return;                                            // whole waves
  const uint32_t total = (uint32_t)*count;
  if (total == 0) {
    if (lane == 0) index[j] = -1;
    return;
  }
  const uint32_t rank = (uint32_t)(((uint64_t)u[j] * (uint64_t)total) >> 32);      // < total
  // the last chunk with prefix <= rank (prefix[0] = 0 <= rank): lo stays such a chunk, every chunk from hi on is past
  int32_t lo = 0, hi = run.nchunks;
  while (hi - lo > 1) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (prefix[mid] <= rank) lo = mid; else hi = mid;
  }
  uint32_t k = rank - prefix[lo];                                // the k-th match of chunk lo; wave-uniform
  int32_t found = -1;
  for (int step = 0; step < kChunk / kWave; ++step) {
    const int64_t v = (int64_t)lo * kThreads + step * 64 + lane;
    const Match m = match_vec(load_vec(run.label, v, run.nvec, run.tail, run.filler), run.pattern, run.any != 0);
    const uint32_t mine = m.count();
    const uint32_t incl = wave_inclusive(mine, lane);
    const uint32_t in_step = __shfl(incl, 63, 64);
    if (k < in_step) {
      if (incl - mine <= k && k < incl) {                        // one lane
        const uint32_t kk = k - (incl - mine);
        uint32_t seen = 0;
        int at = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            if ((m.m[q] >> (8 * b + 7)) & 1u) {
              if (seen == kk) at = q * 4 + b;
              ++seen;
            }
          }
        }
        found = (int32_t)(v * kVec + at);
      }
      break;                                                     // wave-uniform: k and in_step are
    }
    k -= in_step;
  }
  // exactly one lane holds the index when count and prefix describe this label run; -1 if they do not
  const unsigned long long who = __ballot(found >= 0);
  if (who == 0) {
    if (lane == 0) index[j] = -1;
  } else if (found >= 0) {
    index[j] = found;
  }
}

int check_run(int64_t N) {
  if (N < 1) return REHR_EINVAL;
  if (N > kMaxN) return REHR_ENOSUP;
  return REHR_OK;
}

// workspace: [one uint32 per chunk: its count, then its exclusive prefix]
struct Layout {
  uint32_t* chunks;
  int64_t bytes;
};
Layout layout(void* base, int64_t N) {
  Carver c(base);   // a braced list is evaluated left to right
  return {c.take<uint32_t>(chunks_of(N)), c.bytes()};
}

}  // namespace

extern "C" int64_t rehr_class_locations_workspace_bytes(int64_t N) {
  const int rc = check_run(N);
  if (rc != REHR_OK) return rc;
  return layout(nullptr, N).bytes;
}

extern "C" int rehr_class_locations_u8(const uint8_t* label, int64_t N, int32_t value, const uint32_t* u, int32_t R,
                                       int64_t* count, int32_t* index, void* workspace, int64_t workspace_bytes,
                                       void* stream) {
  if (label == nullptr || u == nullptr || count == nullptr || index == nullptr || workspace == nullptr)
    return REHR_EINVAL;
  if (R < 1 || value < -1 || value > 255) return REHR_EINVAL;
  const int rc = check_run(N);
  if (rc != REHR_OK) return rc;
  if (R > kMaxR) return REHR_ENOSUP;
  const auto [chunks, need] = layout(workspace, N);
  if (workspace_bytes < need || misaligned(16, workspace, label) || misaligned(4, u, index) || misaligned(8, count))
    return REHR_EINVAL;
  const bool any = value < 0;
  Run run = {};
  run.label = label;
  run.nvec = N / kVec;
  run.tail = (int32_t)(N % kVec);
  run.nchunks = (int32_t)chunks_of(N);
  run.pattern = any ? 0u : (uint32_t)value * 0x01010101u;
  run.filler = value == 0 ? 1u : 0u;
  run.any = any ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(class_count_kernel, dim3(grid_for(run.nchunks, 1, kMaxCountBlocks)), dim3(kThreads), 0, st, run,
                     chunks);
  hipLaunchKernelGGL(class_scan_kernel, dim3(1), dim3(kThreads), 0, st, chunks, run.nchunks, count);
  hipLaunchKernelGGL(class_select_kernel, dim3(grid_for(R, kThreads / 64, (int64_t)kMaxR)), dim3(kThreads), 0, st, run,
                     (const uint32_t*)chunks, (const int64_t*)count, u, R, index);
  REHR_LAUNCH_CHECK();
  return REHR_OK;
}
