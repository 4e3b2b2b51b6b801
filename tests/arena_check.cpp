// Stand-alone host check of the workspace arena (roma_amd/csrc/arena.h): compiled and run by tests/test_cpu_arena.py.
// Exit status 0 and "arena ok" on stdout when every property holds.
#include <stdio.h>

#include <vector>

#include "arena.h"

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("arena_check.cpp:%d: CHECK failed: %s\n", __LINE__, #cond); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

int main() {
  using roma::Arena;
  // planning run: no memory behind it, fake non-null pointers, the peak is what a live arena needs
  Arena plan;
  CHECK(plan.dry && !plan.overflow);
  void* a0 = plan.alloc(1000);
  const size_t m = plan.mark();
  void* a1 = plan.alloc(300);
  CHECK(a0 && a1 && a0 != a1);
  CHECK(plan.off == 1024 + 300 && plan.peak == plan.off);  // 256-byte alignment of every request
  plan.release(m);
  (void)plan.alloc(100);
  CHECK(plan.off == 1024 + 100 && plan.peak == 1024 + 300 && !plan.overflow);  // released scratch is reused, the peak stays

  // a live arena of exactly the planned size serves the same sequence inside its buffer
  std::vector<char> buf(plan.peak);
  Arena live;
  live.base = buf.data();
  live.cap = buf.size();
  live.dry = false;
  char* p0 = (char*)live.alloc(1000);
  const size_t lm = live.mark();
  char* p1 = (char*)live.alloc(300);
  CHECK(p0 == buf.data() && p1 == buf.data() + 1024 && !live.overflow);
  p1[299] = 1;  // the last planned byte is inside the buffer (the sanitizer build checks the write)
  live.release(lm);
  CHECK(live.alloc(100) == buf.data() + 1024 && !live.overflow);

  // a request that does not fit but is no larger than the arena: flagged, served from the START (aliased, inside the buffer)
  const size_t off_before = live.off;
  char* q = (char*)live.alloc(buf.size() - 512);
  CHECK(live.overflow && q == buf.data());
  CHECK(live.off == ((off_before + 255) & ~(size_t)255));  // nothing was reserved for it
  q[buf.size() - 513] = 2;
  // the flag is sticky until the schedule clears it: a later request that fits is served as usual
  char* r = (char*)live.alloc(16);
  CHECK(live.overflow && r >= buf.data() && r + 16 <= buf.data() + buf.size());
  live.overflow = false;

  // a request larger than the whole arena: flagged, nullptr
  CHECK(live.alloc(buf.size() + 1) == nullptr && live.overflow);
  live.reset();
  CHECK(live.off == 0 && live.alloc(buf.size()) == buf.data());  // exactly the capacity fits
  printf("arena ok\n");
  return 0;
}
