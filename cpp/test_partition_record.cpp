// Host-only test of the handoff record layout
// (csrc/core/partition_record.h): every field written is read back, for
// every shape the record takes.
#include "core/partition_record.h"

#include <cstdio>
#include <vector>

using namespace pumitally;

static int g_fail = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) {                                                             \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);              \
      ++g_fail;                                                                \
    }                                                                          \
  } while (0)

static void roundtrip(bool carry_grp, int nscores) {
  const HandoffLayout L{nscores, carry_grp};
  CHECK(L.width() == 11 + (carry_grp ? 1 : 0) + nscores);
  CHECK(L.dep_width() == L.width() + 1);

  // distinct values everywhere, poison around the entry
  const double poison = -777.0;
  std::vector<double> buf(L.dep_width() + 2, poison);
  double *e = buf.data() + 1;
  const double resp[3] = {1.25, 2.5, 3.75};
  L.write(e, 123456, Vec3{0.1, 0.2, 0.3}, 654321, Vec3{0.4, 0.5, 0.6}, 0.7,
          0.8, 4242, 9, resp, 5);
  CHECK(buf.front() == poison && buf.back() == poison);
  for (int k = 0; k < L.dep_width(); ++k) CHECK(e[k] != poison);

  CHECK(L.gid(e) == 123456);
  CHECK(L.pos(e).x == 0.1 && L.pos(e).y == 0.2 && L.pos(e).z == 0.3);
  CHECK(L.target_gid(e) == 654321);
  CHECK(L.dest(e).x == 0.4 && L.dest(e).y == 0.5 && L.dest(e).z == 0.6);
  CHECK(L.weight(e) == 0.7);
  CHECK(L.t(e) == 0.8);
  CHECK(L.prev_gid(e) == 4242);
  CHECK(L.group(e) == (carry_grp ? 9 : 0));
  for (int k = 0; k < nscores; ++k) CHECK(L.responses(e)[k] == resp[k]);
  CHECK(L.owner(e) == 5);

  // a fresh entry: no exited-from element, no responses given
  L.write(e, 1, Vec3{0, 0, 0}, 2, Vec3{1, 1, 1}, 1.0, 0.0, -1, 0, nullptr, 0);
  CHECK(L.prev_gid(e) == -1);
  CHECK(L.t(e) == 0.0);
  for (int k = 0; k < nscores; ++k) CHECK(L.responses(e)[k] == 1.0);
  CHECK(buf.front() == poison && buf.back() == poison);
}

int main() {
  roundtrip(false, 1);
  roundtrip(true, 1);
  roundtrip(false, 2);
  roundtrip(true, 3);
  std::printf("test_partition_record: %s\n", g_fail ? "FAIL" : "PASS");
  return g_fail ? 1 : 0;
}
