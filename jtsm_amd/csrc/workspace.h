// One arena for the caller-owned workspaces: an entry point's `carve(Arena&, dims...)` names every buffer once, with its
// element type and count, and is run twice — over a null base by `*_workspace_bytes` (measure: `off` is the answer) and
// over the caller's buffer by the call itself.  Buffers start on multiples of `granule` bytes: 256 everywhere but in
// the layouts whose published byte counts are sums of 16-byte pieces (the MIL and PCL workspaces, the DeepLab loss, the
// Panoptic-DeepLab centres and merge).  Host code only.
#pragma once
#include <cstddef>

namespace jtsm {

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t a16(size_t b) { return (b + 15) & ~(size_t)15; }

struct Arena {
  char* base;               // nullptr: measure only
  bool pad_empty = false;   // an empty buffer still takes a granule (the evaluators) instead of none (NMS, the miners)
  size_t granule = 256;     // a power of two
  size_t off = 0;

  template <class T>
  T* take(size_t count) {
    const size_t at = off, bytes = count * sizeof(T);
    off += ((bytes || !pad_empty ? bytes : 1) + granule - 1) & ~(granule - 1);
    return base ? reinterpret_cast<T*>(base + at) : nullptr;
  }
  size_t mark() const { return off; }   // the ends of a contiguous region that one memset clears
};

}  // namespace jtsm
