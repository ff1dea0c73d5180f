// Stand-alone test of the RAII owners in csrc/hip/hip_util.h.  Free device
// memory (hipMemGetInfo) is always compared with an earlier reading of the
// same run, never with a fixed number.  Without a device: skip.
#include "hip/hip_util.h"

#include <cstdio>
#include <stdexcept>
#include <utility>

using namespace pumitally;

static int g_fail = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) {                                                             \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);              \
      ++g_fail;                                                                \
    }                                                                          \
  } while (0)

static constexpr int64_t kMiB = 1 << 20;
static constexpr int64_t kBig = 64 * kMiB; // the watched allocation
static constexpr int64_t kSlack = 4 * kMiB; // "back to where it was"

static int64_t free_bytes() {
  size_t f = 0, t = 0;
  PT_HIP_CHECK(hipMemGetInfo(&f, &t));
  return (int64_t)f;
}

// Two buffer members; the constructor fails after the first allocation.
struct ThrowsHalfway {
  DeviceBuffer<char> a, b;
  explicit ThrowsHalfway(bool fail) : a(kBig) {
    if (fail)
      throw std::runtime_error("constructor failed between two allocations");
    b.allocate(kBig);
  }
};

static void test_scope_and_move() {
  const int64_t before = free_bytes();
  {
    DeviceBuffer<char> b(kBig);
    CHECK(b.get() != nullptr && b.size() == kBig);
    CHECK(free_bytes() <= before - kBig + kSlack);
    char *const p = b.get();
    DeviceBuffer<char> c(std::move(b));
    CHECK(b.get() == nullptr && b.size() == 0 && !b);
    CHECK(c.get() == p && c.size() == kBig);
    CHECK(free_bytes() <= before - kBig + kSlack); // moved, not copied/freed
  }
  CHECK(free_bytes() >= before - kSlack);
}

static void test_reserve() {
  DeviceBuffer<double> b;
  b.reserve(1000);
  CHECK(b.size() == 1250);
  double *const p = b.get();
  b.reserve(1250);
  b.reserve(10);
  b.reserve(0);
  CHECK(b.get() == p && b.size() == 1250);
  b.reserve(1251);
  CHECK(b.size() == 1251 + 1251 / 4 && b.get() != nullptr);
}

static void test_zero_count() {
  DeviceBuffer<double> a(0), b;
  b.allocate(0);
  b.reserve(0);
  CHECK(a.get() == nullptr && a.size() == 0);
  CHECK(b.get() == nullptr && b.size() == 0);
  PinnedBuffer<int32_t> h(0);
  CHECK(h.get() == nullptr && h.size() == 0);
  b.allocate(8);
  b.allocate(0); // drops the block
  CHECK(b.get() == nullptr && b.size() == 0);
}

static void test_throwing_constructor() {
  const int64_t before = free_bytes();
  bool thrown = false;
  try {
    ThrowsHalfway t(/*fail=*/true);
  } catch (const std::runtime_error &) {
    thrown = true;
  }
  CHECK(thrown);
  CHECK(free_bytes() >= before - kSlack);
}

int main() {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
    std::printf("test_hip_util: SKIP (no HIP device)\n");
    return 0;
  }
  PT_HIP_CHECK(hipSetDevice(0));
  { // runtime warm-up, so one-off setup is not charged to a test
    DeviceBuffer<char> warm(kMiB);
    PinnedBuffer<char> hwarm(kMiB);
    Stream s;
    s.create();
    Event e;
    e.create();
    PT_HIP_CHECK(hipEventRecord(e, s));
    PT_HIP_CHECK(hipStreamSynchronize(s));
  }
  test_scope_and_move();
  test_reserve();
  test_zero_count();
  test_throwing_constructor();
  if (g_fail) {
    std::printf("test_hip_util: %d check(s) FAILED\n", g_fail);
    return 1;
  }
  std::printf("test_hip_util: OK\n");
  return 0;
}
