// dev_mem_check.cpp -- the failure paths of csrc/dev_mem.h, on the CPU.
//
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I audio-modem-radio_amd/csrc \
//       tests/host/dev_mem_check.cpp -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -o dev_mem_check
//
// Every request is for 2^60 bytes, which no machine grants (without a GPU
// every HIP call fails anyway), so the program needs no device.  A buffer
// that "already holds a block" holds one in its bookkeeping only
// (DevBuf::adopt of an address that is never dereferenced or freed: it is
// detached again before the buffer dies).  Exit status 0 and "dev_mem ok" on
// success; the first failed check prints its line and exits 1.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "dev_mem.h"

using amr::DevBuf;

#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);         \
      std::exit(1);                                              \
    }                                                            \
  } while (0)

static const int64_t kNever = (int64_t)1 << 60;
static char g_block_a[64], g_block_b[64];        // addresses for the bookkeeping, never device memory

int main() {
  {  // a failed reserve leaves the buffer empty; destroying it frees nothing
    DevBuf b;
    CHECK(b.reserve(kNever, nullptr) != hipSuccess);
    CHECK(!b && b.get() == nullptr && b.bytes() == 0);
    CHECK(b.reserve(kNever, nullptr) != hipSuccess);   // and again, from the empty state
    CHECK(!b && b.bytes() == 0);
  }
  {  // a held block that is large enough is kept: reserve does nothing
    DevBuf b = DevBuf::adopt(g_block_a, 64);
    CHECK(b.reserve(64, nullptr) == hipSuccess && b.reserve(1, nullptr) == hipSuccess);
    CHECK(b.get() == g_block_a && b.bytes() == 64 && b.as<char>() == g_block_a);
    CHECK(b.detach() == g_block_a);
    CHECK(!b && b.bytes() == 0);
  }
  {  // moved-from buffers are empty; the block has one owner at a time
    DevBuf a = DevBuf::adopt(g_block_a, 64);
    DevBuf b(std::move(a));
    CHECK(!a && a.bytes() == 0 && b.get() == g_block_a && b.bytes() == 64);
    DevBuf c;
    c = std::move(b);
    CHECK(!b && b.bytes() == 0 && c.get() == g_block_a && c.bytes() == 64);
    c.swap(a);
    CHECK(!c && c.bytes() == 0 && a.get() == g_block_a && a.bytes() == 64);
    CHECK(a.detach() == g_block_a);
  }
  {  // a failed group reserve (the last member cannot be had) leaves every member as it was
    DevBuf held_a = DevBuf::adopt(g_block_a, 16), empty, held_b = DevBuf::adopt(g_block_b, 32), last;
    const hipError_t e = amr::reserve_all({{held_a, 64}, {empty, 64}, {held_b, 64}, {last, kNever}}, nullptr);
    CHECK(e != hipSuccess);
    CHECK(held_a.get() == g_block_a && held_a.bytes() == 16);
    CHECK(!empty && empty.bytes() == 0);
    CHECK(held_b.get() == g_block_b && held_b.bytes() == 32);
    CHECK(!last && last.bytes() == 0);
    // a group that already holds what is asked is left alone
    CHECK(amr::reserve_all({{held_a, 16}, {held_b, 32}}, nullptr) == hipSuccess);
    CHECK(held_a.get() == g_block_a && held_b.get() == g_block_b);
    CHECK(held_a.detach() == g_block_a && held_b.detach() == g_block_b);
  }
  {  // all members empty, all fail: still empty, and their destructors free nothing
    DevBuf a, b;
    CHECK(amr::reserve_all({{a, kNever}, {b, kNever}}, nullptr) != hipSuccess);
    CHECK(!a && !b && a.bytes() == 0 && b.bytes() == 0);
  }
  {  // a stream scope that was never created destroys nothing
    amr::StreamScope st;
    CHECK(st.get() == nullptr);
  }
  std::printf("dev_mem ok\n");
  return 0;
}
