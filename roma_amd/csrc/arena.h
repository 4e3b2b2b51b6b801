// Bump arena over one device allocation, planned by a dry run (roma_finalize): no allocation inside roma_match.
// Host-only C++, no HIP in it.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace roma {

// x rounded up to the 256-byte alignment of every workspace region
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

class Arena {
 public:
  char* base = nullptr;
  size_t cap = 0, off = 0, peak = 0;
  bool dry = true;
  // set when a live allocation did not fit the planned capacity (an option changed between roma_finalize's dry run and the
  // call): the request is then served from the START of the arena - aliased, so no kernel could write outside the
  // hipMalloc'd workspace - and the schedule returns the error before the launches of that stage (Model::fits, model.hip)
  bool overflow = false;
  void reset() { off = 0; }
  void* alloc(size_t bytes) {
    off = align256(off);
    if (!dry && off + bytes > cap) {
      overflow = true;
      if (off > peak) peak = off;
      return bytes <= cap ? (void*)base : nullptr;
    }
    void* p = dry ? reinterpret_cast<void*>((uintptr_t)0x1000 + off) : (void*)(base + off);
    off += bytes;
    if (off > peak) peak = off;
    return p;
  }
  size_t mark() const { return off; }
  void release(size_t m) { off = m; }
};

}  // namespace roma
