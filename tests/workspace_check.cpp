// Stand-alone host check of the operators' workspace carver (roma_amd/csrc/workspace.h): compiled and run by
// tests/test_cpu_workspace.py.  Exit status 0 and "workspace ok" on stdout when every property holds.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "workspace.h"

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      printf("workspace_check.cpp:%d: CHECK failed: %s\n", __LINE__, #cond); \
      return 1;                                                           \
    }                                                                     \
  } while (0)

namespace {

struct Odd {  // 24 bytes: no multiple of it is a multiple of 256 below 32 elements
  double a, b, c;
};

constexpr int REGIONS = 5;

// one take sequence for every run: the pointers, and the offset each region must have from the aligned base
template <class W>
size_t carve(W ws, char* (&p)[REGIONS], size_t (&want)[REGIONS], size_t align) {
  const size_t counts[REGIONS] = {7, 0, 1000, 3, 1};
  const size_t sizes[REGIONS] = {sizeof(Odd), sizeof(int), sizeof(char), sizeof(double), sizeof(short)};
  size_t off = 0;
  for (int r = 0; r < REGIONS; ++r) {
    want[r] = off;
    off += (counts[r] * sizes[r] + align - 1) / align * align;
  }
  p[0] = reinterpret_cast<char*>(ws.template take<Odd>(7));
  p[1] = reinterpret_cast<char*>(ws.template take<int>(0));
  p[2] = ws.template take<char>(1000);
  p[3] = reinterpret_cast<char*>(ws.template take<double>(3));
  p[4] = reinterpret_cast<char*>(ws.template take<short>(1));
  return ws.bytes();
}

}  // namespace

int main() {
  using roma::Workspace16;
  using roma::Workspace256;
  char* p[REGIONS];
  size_t want[REGIONS];

  // a sizing run: null pointers only, bytes() = the regions rounded up to 256 and 256 bytes of slack
  const size_t need = carve(Workspace256(), p, want, 256);
  for (int r = 0; r < REGIONS; ++r) CHECK(p[r] == nullptr);
  CHECK(need == 256 + 0 + 1024 + 256 + 256 + 256);
  CHECK(want[1] == 256 && want[2] == 256);  // a region of zero elements is legal and consumes nothing
  CHECK(Workspace256().bytes() == 256 && Workspace16().bytes() == 0);

  // live runs over a buffer of exactly bytes(), its start aligned, off by 8 and off by 255: the same bytes(), every region
  // at its predicted offset from the aligned base and inside [ws, ws + bytes())
  std::vector<char> buf(need + 512);
  char* aligned = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(buf.data()) + 255) & ~(uintptr_t)255);
  const size_t counts_bytes[REGIONS] = {7 * sizeof(Odd), 0, 1000, 3 * sizeof(double), sizeof(short)};
  for (size_t shift : {(size_t)0, (size_t)8, (size_t)255}) {
    char* ws = aligned + shift;
    CHECK(carve(Workspace256(ws), p, want, 256) == need);
    char* base = shift ? aligned + 256 : aligned;
    for (int r = 0; r < REGIONS; ++r) {
      CHECK(p[r] == base + want[r]);
      CHECK((reinterpret_cast<uintptr_t>(p[r]) & 255) == 0);
      CHECK(p[r] >= ws && p[r] + counts_bytes[r] <= ws + need);
      memset(p[r], r, counts_bytes[r]);  // the sanitizer build checks the writes
    }
  }

  // the 16-byte policy: the base as given, no slack, the last region padded like every other
  CHECK(carve(Workspace16(), p, want, 16) == 176 + 0 + 1008 + 32 + 16);
  for (int r = 0; r < REGIONS; ++r) CHECK(p[r] == nullptr);
  const size_t need16 = carve(Workspace16(aligned + 16), p, want, 16);
  CHECK(need16 == 176 + 1008 + 32 + 16);
  for (int r = 0; r < REGIONS; ++r) {
    CHECK(p[r] == aligned + 16 + want[r]);
    CHECK(p[r] + counts_bytes[r] <= aligned + 16 + need16);
    memset(p[r], r, counts_bytes[r]);
  }
  CHECK(want[4] + 16 == need16);  // 2 bytes asked, 16 consumed
  printf("workspace ok\n");
  return 0;
}
