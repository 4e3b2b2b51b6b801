// Carver of an operator's caller-provided workspace: the operator names its regions once, as a sequence of take<T>(count), and
// runs that sequence twice - over nothing, for the bytes its *_workspace_bytes reports, and over the caller's pointer, for
// the pointers its kernels get.  Host-only C++, no HIP in it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "arena.h"

namespace roma {

// Regions are rounded up to ALIGN bytes.  SLACK: the base is rounded up to ALIGN inside what the caller gives, and bytes()
// includes the ALIGN bytes that can cost; without it the base is used as given (the operator refuses a misaligned one).
template <size_t ALIGN, bool SLACK>
class Workspace {
 public:
  Workspace() = default;  // a sizing run: every take returns nullptr, and no pointer arithmetic happens
  explicit Workspace(void* ws) : base_(reinterpret_cast<uintptr_t>(ws)) {
    if (SLACK && ws) base_ = (base_ + (ALIGN - 1)) & ~(uintptr_t)(ALIGN - 1);
  }

  template <typename T>
  T* take(size_t count) {
    T* p = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
    off_ += (count * sizeof(T) + (ALIGN - 1)) & ~(ALIGN - 1);
    return p;
  }
  size_t bytes() const { return off_ + (SLACK ? ALIGN : 0); }

 private:
  uintptr_t base_ = 0;
  size_t off_ = 0;
};

using Workspace256 = Workspace<256, true>;   // the geometry operators
using Workspace16 = Workspace<16, false>;    // sample_matches, match_keypoints

// the `long workspace_bytes` of an entry point as a size: a negative count is an empty workspace, which the operator refuses
inline size_t workspace_size(long workspace_bytes) { return workspace_bytes > 0 ? (size_t)workspace_bytes : 0; }

}  // namespace roma
