// One arena for the caller-owned, 256-byte aligned workspaces: an entry point's `carve(Arena&, dims...)` names every
// buffer once, with its element type and count, and is run twice — over a null base by `*_workspace_bytes` (measure:
// `off` is the answer) and over the caller's buffer by the call itself.  Host code only.
#pragma once
#include <cstddef>

namespace jtsm {

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct Arena {
  char* base;               // nullptr: measure only
  bool pad_empty = false;   // an empty buffer still takes 256 bytes (the evaluators) instead of none (NMS, the miners)
  size_t off = 0;

  template <class T>
  T* take(size_t count) {
    const size_t at = off, bytes = count * sizeof(T);
    off += align256(bytes || !pad_empty ? bytes : 1);
    return base ? reinterpret_cast<T*>(base + at) : nullptr;
  }
  size_t mark() const { return off; }   // the ends of a contiguous region that one memset clears
};

}  // namespace jtsm
