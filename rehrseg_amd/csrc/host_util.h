// Host-side helpers of the pipeline kernels' entry points (host code only: nothing here reaches a kernel).
#pragma once
#include <stdint.h>

inline int64_t align16(int64_t n) { return (n + 15) & ~(int64_t)15; }

// true when an address is no multiple of `bytes` (a power of two); null counts as aligned, so optional operands pass
template <typename... P>
inline bool misaligned(uintptr_t bytes, const P*... p) {
  return ((reinterpret_cast<uintptr_t>(p) | ...) & (bytes - 1)) != 0;
}

// blocks of a 1-D grid: ceil(items / per_block), at least 1 and at most cap
inline unsigned grid_for(int64_t items, int64_t per_block, int64_t cap) {
  const int64_t b = (items + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : (b < cap ? b : cap));
}

// Carves a workspace into segments that each start on a multiple of 16 bytes from the base.  Every workspace has ONE
// layout function that takes its segments from a Carver and returns their pointers next to bytes(): the size query
// calls it on a null base (null segments, the same size), the launchers on the caller's buffer.
class Carver {
 public:
  explicit Carver(void* base) : base_(static_cast<char*>(base)) {}
  template <typename T>
  T* take(int64_t count) {
    T* p = base_ != nullptr ? reinterpret_cast<T*>(base_ + bytes_) : nullptr;
    bytes_ += align16(count * (int64_t)sizeof(T));
    return p;
  }
  int64_t bytes() const { return bytes_; }

 private:
  char* base_;
  int64_t bytes_ = 0;
};
