// Collision-estimator tallies on the CPU engine (core/engine.h):
// score_collisions and score_points with ngroups=3, nscores=2, end_batch and
// misses.  Weights and responses are small integers, so every expected sum
// is exact in fp64 and compared with ==.  No GPU: passes in a build
// configured with a plain host compiler.
#include "core/engine.h"

#include <cstdio>
#include <random>
#include <vector>

using namespace pumitally;

namespace {

int g_fail = 0;

#define CHECK(cond)                                                           \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      ++g_fail;                                                               \
    }                                                                         \
  } while (0)

constexpr int G = 3, S = 2;

// A point strictly inside tet t: barycentric weights 0.8*u + 0.05 with u on
// the simplex.  Its element is t by construction.
Vec3 point_in(const Mesh &m, int32_t t, std::mt19937_64 &rng) {
  std::exponential_distribution<double> ex(1.0);
  double lam[4], sum = 0;
  for (double &l : lam) sum += (l = ex(rng));
  Vec3 p{0, 0, 0};
  for (int k = 0; k < 4; ++k)
    p = p + (0.8 * lam[k] / sum + 0.05) * m.vert(m.tet2vert[t * 4 + k]);
  return p;
}

struct Case {
  std::vector<int32_t> tet;
  std::vector<double> xyz, w, resp;
  std::vector<uint16_t> grp;
  std::vector<int8_t> active;
};

Case make_case(const Mesh &m, int64_t n, uint64_t seed) {
  std::mt19937_64 rng(seed);
  Case c;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t t = (int32_t)(rng() % (uint64_t)m.nelems);
    const Vec3 p = point_in(m, t, rng);
    c.tet.push_back(t);
    c.xyz.insert(c.xyz.end(), {p.x, p.y, p.z});
    c.w.push_back((double)(1 + rng() % 4));
    c.grp.push_back((uint16_t)(rng() % 7)); // wraps: % ngroups
    for (int k = 0; k < S; ++k) c.resp.push_back((double)(1 + rng() % 4));
    c.active.push_back((int8_t)(rng() % 2));
  }
  return c;
}

// Expected tally of the rows with use[i] != 0 (all rows for use == nullptr).
std::vector<double> expect(const Mesh &m, const Case &c, const int8_t *use,
                           bool with_resp) {
  std::vector<double> out((size_t)S * G * m.nelems, 0.0);
  for (size_t i = 0; i < c.tet.size(); ++i) {
    if (use && !use[i]) continue;
    for (int k = 0; k < (with_resp ? S : 1); ++k)
      out[((int64_t)k * G + c.grp[i] % G) * m.nelems + c.tet[i]] +=
          c.w[i] * (with_resp ? c.resp[i * S + k] : 1.0);
  }
  return out;
}

void test_off() {
  auto eng = make_cpu_engine(build_box(1, 1, 1, 1.0, 1.0, 1.0), 2);
  CHECK(!eng->collision_tallies);
  const int8_t a[2] = {1, 1};
  const double w[2] = {1, 1}, p[6] = {.5, .5, .5, .5, .5, .5};
  int thrown = 0;
  auto off = [&](auto call) {
    try {
      call();
    } catch (const std::runtime_error &e) {
      thrown += std::string(e.what()) ==
                "collision tallies are off: create the engine with "
                "collisions=true";
    }
  };
  off([&] { eng->score_collisions(a, w, 2); });
  off([&] { eng->score_points(2, p, w); });
  off([&] { eng->score_collisions_device(a, w, 2); });
  off([&] { eng->score_points_device(2, p, w); });
  off([&] { (void)eng->collisions(); });
  off([&] { (void)eng->collision_sum(); });
  off([&] { (void)eng->collision_sum_sq(); });
  off([&] { eng->set_collisions(w, 2); });
  CHECK(thrown == 8);
}

void test_scoring_and_batches() {
  const Mesh mesh = build_box(3, 3, 3, 1.0, 1.0, 1.0);
  const int64_t n = 2000;
  const Case c = make_case(mesh, n, 7);
  auto eng = make_cpu_engine(mesh, n, G, S, false, false, true);
  CHECK(eng->collision_tallies);
  eng->copy_initial_position(c.xyz.data(), n);
  CHECK(eng->elem_ids() == c.tet); // the oracle's precondition

  const std::vector<double> flux0 = eng->flux();
  const std::vector<int8_t> active0 = c.active;
  eng->score_collisions(c.active.data(), c.w.data(), n, c.grp.data(),
                        c.resp.data());
  const auto b1 = expect(mesh, c, c.active.data(), true);
  CHECK(eng->collisions() == b1);
  CHECK(c.active == active0);
  CHECK(eng->elem_ids() == c.tet);
  CHECK(eng->flux() == flux0);
  int64_t on = 0;
  for (int8_t a : c.active) on += a != 0;
  CHECK(eng->stats().collisions_scored == on);
  CHECK(eng->stats().collision_misses == 0);
  eng->end_batch();
  for (double v : eng->collisions()) CHECK(v == 0.0);

  // batch 2: free points (any n), null responses -> score 0 only
  const Case d = make_case(mesh, 777, 8);
  eng->score_points(777, d.xyz.data(), d.w.data(), d.grp.data());
  eng->score_points(0, nullptr, nullptr);
  const auto b2 = expect(mesh, d, nullptr, false);
  CHECK(eng->collisions() == b2);
  for (int64_t e = (int64_t)G * mesh.nelems; e < (int64_t)b2.size(); ++e)
    CHECK(b2[e] == 0.0);
  CHECK(eng->stats().collisions_scored == on + 777);
  eng->end_batch();

  const auto sum = eng->collision_sum(), sq = eng->collision_sum_sq();
  for (size_t e = 0; e < b1.size(); ++e) {
    CHECK(sum[e] == b1[e] + b2[e]);
    CHECK(sq[e] == b1[e] * b1[e] + b2[e] * b2[e]);
  }
  CHECK(eng->num_batches() == 2);

  eng->set_collisions(b1.data(), (int64_t)b1.size());
  CHECK(eng->collisions() == b1);
  bool threw = false;
  try {
    eng->set_collisions(b1.data(), 3);
  } catch (const std::runtime_error &) {
    threw = true;
  }
  CHECK(threw);
}

void test_misses() {
  const Mesh mesh = build_box(1, 1, 1, 1.0, 1.0, 1.0);
  const int64_t n = 5;
  auto eng = make_cpu_engine(mesh, n, 1, 1, false, false, true);
  std::vector<double> o, d;
  for (int64_t i = 0; i < n; ++i) {
    o.insert(o.end(), {0.1, 0.4, 0.5});
    d.insert(d.end(), {1.2, 0.4, 0.5});
  }
  const std::vector<int8_t> fly(n, 1);
  const std::vector<double> w{1, 2, 3, 4, 1};
  eng->copy_initial_position(o.data(), n);
  eng->score_collisions(fly.data(), w.data(), n);
  std::vector<double> want(mesh.nelems, 0.0);
  want[2] = 11.0;
  CHECK(eng->collisions() == want);
  // through the vacuum face: escaped, no longer in the mesh
  eng->move(o.data(), d.data(), fly.data(), w.data(), n);
  eng->score_collisions(fly.data(), w.data(), n);
  CHECK(eng->collisions() == want);
  CHECK(eng->stats().collisions_scored == n);
  CHECK(eng->stats().collision_misses == n);
  // points outside the mesh miss too
  eng->score_points(n, d.data(), w.data());
  CHECK(eng->collisions() == want);
  CHECK(eng->stats().collision_misses == 2 * n);
  // inactive particles neither score nor miss
  const std::vector<int8_t> none(n, 0);
  eng->score_collisions(none.data(), w.data(), n);
  CHECK(eng->stats().collision_misses == 2 * n);
  bool threw = false;
  try {
    eng->score_collisions(fly.data(), w.data(), n - 1);
  } catch (const std::runtime_error &) {
    threw = true;
  }
  CHECK(threw);
}

} // namespace

int main() {
  test_off();
  test_scoring_and_batches();
  test_misses();
  std::printf("test_collisions: %s\n", g_fail ? "FAIL" : "PASS");
  return g_fail ? 1 : 0;
}
