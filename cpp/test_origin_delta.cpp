// Stand-alone test of the host delta pass behind origin elision
// (csrc/core/origin_delta.h).  No GPU, no engine: plain memory in, patch
// list out.
#include "core/origin_delta.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <set>
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

static bool same_bits(const double *a, const double *b, int64_t count) {
  return std::memcmp(a, b, count * sizeof(double)) == 0;
}

struct Case {
  int64_t n, lo, hi;
  std::vector<double> origin, dest, shadow;
  std::set<int64_t> changed; // expected, absolute indices in [lo, hi)
};

static Case make_case(int64_t n, int64_t lo, int64_t hi, unsigned seed) {
  Case c;
  c.n = n;
  c.lo = lo;
  c.hi = hi;
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> u(-1.0, 2.0);
  c.origin.resize(n * 3);
  c.dest.resize(n * 3);
  for (auto &v : c.dest) v = u(rng);
  for (auto &v : c.origin) v = u(rng);
  c.shadow = c.origin; // nothing changed until a test says so
  return c;
}

// Runs the pass and checks every structural property against c.changed.
static void run_and_check(Case &c, int nthreads, bool nontemporal) {
  OriginDeltaPool pool(nthreads);
  const int64_t len = c.hi - c.lo;
  const int64_t cap = origin_delta_patch_capacity(len, nthreads);
  std::vector<int32_t> pidx(cap, -7);
  std::vector<double> pxyz(cap * 3, -7.0);
  std::vector<double> shadow_before = c.shadow;
  OriginDeltaResult r =
      origin_delta_pass(pool, c.origin.data(), c.dest.data(), c.shadow.data(),
                        c.lo, c.hi, pidx.data(), pxyz.data(), nontemporal);

  CHECK(r.changed == (int64_t)c.changed.size());
  CHECK(r.block == origin_delta_block(len, nthreads));
  CHECK(r.nsegs == (len + r.block - 1) / r.block);
  CHECK((int64_t)r.seg_count.size() == r.nsegs);
  // shadow == dest inside the range, untouched outside
  CHECK(same_bits(c.shadow.data() + c.lo * 3, c.dest.data() + c.lo * 3,
                  len * 3));
  CHECK(same_bits(c.shadow.data(), shadow_before.data(), c.lo * 3));
  CHECK(same_bits(c.shadow.data() + c.hi * 3, shadow_before.data() + c.hi * 3,
                  (c.n - c.hi) * 3));
  // segments: disjoint, inside the region, strictly increasing indices that
  // stay inside the segment's own block
  int64_t sum = 0, prev_end = 0;
  bool any_over = false;
  for (int64_t b = 0; b < r.nsegs; ++b) {
    CHECK(r.seg_off[b] >= prev_end);
    CHECK(r.seg_off[b] + r.seg_cap[b] <= cap);
    prev_end = r.seg_off[b] + r.seg_cap[b];
    sum += r.seg_count[b];
    if (r.seg_count[b] > r.seg_cap[b]) any_over = true;
    const int64_t stored = std::min(r.seg_count[b], r.seg_cap[b]);
    const int64_t blo = c.lo + b * r.block;
    const int64_t bhi = std::min(c.hi, blo + r.block);
    for (int64_t k = 0; k < stored; ++k) {
      CHECK(pidx[r.seg_off[b] + k] >= blo && pidx[r.seg_off[b] + k] < bhi);
      if (k) CHECK(pidx[r.seg_off[b] + k - 1] < pidx[r.seg_off[b] + k]);
    }
  }
  CHECK(sum == r.changed);
  CHECK(any_over == r.overflow);
  if (r.overflow) return;

  origin_delta_compact(r, pidx.data(), pxyz.data());
  std::set<int64_t> got;
  for (int64_t k = 0; k < r.changed; ++k) {
    const int64_t i = pidx[k];
    CHECK(i >= c.lo && i < c.hi);
    if (k) CHECK(pidx[k - 1] < pidx[k]);
    got.insert(i);
    if (i >= c.lo && i < c.hi)
      CHECK(same_bits(&pxyz[k * 3], &c.origin[i * 3], 3));
  }
  CHECK(got == c.changed);
}

static void perturb(Case &c, int64_t i, int comp = 0) {
  c.origin[i * 3 + comp] += 0.25;
  c.changed.insert(i);
}

int main() {
  const int64_t sizes[] = {1, 2, 5, 17, 257, 1000, 4099};
  for (int nt = 1; nt <= kOriginDeltaMaxThreads; ++nt) {
    for (int64_t n : sizes) {
      for (int ntmp = 0; ntmp < 2; ++ntmp) {
        const bool nontemporal = ntmp != 0;
        { // zero changed
          Case c = make_case(n, 0, n, 1);
          run_and_check(c, nt, nontemporal);
        }
        { // first only, last only (each of x, y, z decides on its own)
          for (int comp = 0; comp < 3; ++comp) {
            Case c = make_case(n, 0, n, 2);
            perturb(c, 0, comp);
            run_and_check(c, nt, nontemporal);
            Case d = make_case(n, 0, n, 3);
            perturb(d, n - 1, comp);
            run_and_check(d, nt, nontemporal);
          }
        }
        { // all changed
          Case c = make_case(n, 0, n, 4);
          for (int64_t i = 0; i < n; ++i) perturb(c, i, (int)(i % 3));
          run_and_check(c, nt, nontemporal);
        }
        { // ~10 % random, on a sub-range with both ends off the array ends
          const int64_t lo = n / 5, hi = n - n / 7;
          Case c = make_case(n, lo, hi, 5);
          std::mt19937_64 rng(6);
          for (int64_t i = lo; i < hi; ++i)
            if (rng() % 10 == 0) perturb(c, i, (int)(rng() % 3));
          // a difference outside [lo, hi) must not be reported
          if (lo > 0) c.origin[0] += 1.0;
          if (lo < hi) run_and_check(c, nt, nontemporal);
        }
      }
    }
  }

  { // blocks long enough for half-sized segments: all changed overflows
    // them (counts stay exact), just under half does not
    const int64_t n = 40000;
    for (int nt : {1, 3, 8}) {
      Case c = make_case(n, 0, n, 9);
      for (int64_t i = 0; i < n; ++i) perturb(c, i, (int)(i % 3));
      run_and_check(c, nt, false);
      Case d = make_case(n, 0, n, 10);
      for (int64_t i = 0; i < n; i += 2) perturb(d, i + (i % 4 == 0), 1);
      run_and_check(d, nt, false);
    }
  }

  { // -0.0 vs 0.0 is changed; identical NaN bits are unchanged
    const int64_t n = 64;
    Case c = make_case(n, 0, n, 7);
    c.origin[3 * 5 + 1] = 0.0;
    c.shadow[3 * 5 + 1] = -0.0;
    CHECK(c.origin[3 * 5 + 1] == c.shadow[3 * 5 + 1]); // fp == cannot see it
    c.changed.insert(5);
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    c.origin[3 * 9] = qnan;
    c.shadow[3 * 9] = qnan;
    CHECK(!(c.origin[3 * 9] == c.shadow[3 * 9])); // fp == would call it changed
    // NaN with a different payload is changed
    uint64_t bits;
    std::memcpy(&bits, &qnan, 8);
    bits ^= 1;
    double nan2;
    std::memcpy(&nan2, &bits, 8);
    c.origin[3 * 11 + 2] = qnan;
    c.shadow[3 * 11 + 2] = nan2;
    c.changed.insert(11);
    run_and_check(c, 4, true);
  }

  { // seeding copies dest to shadow on the range only
    const int64_t n = 1001;
    Case c = make_case(n, 10, 990, 8);
    std::vector<double> before = c.shadow;
    OriginDeltaPool pool(7);
    origin_delta_seed(pool, c.dest.data(), c.shadow.data(), c.lo, c.hi);
    CHECK(same_bits(c.shadow.data() + 30, c.dest.data() + 30, 980 * 3));
    CHECK(same_bits(c.shadow.data(), before.data(), 30));
    CHECK(same_bits(c.shadow.data() + 990 * 3, before.data() + 990 * 3, 33));
  }

  { // thread count is capped whatever is asked for
    CHECK(origin_delta_clamp_threads(0) == 1);
    CHECK(origin_delta_clamp_threads(1000) == kOriginDeltaMaxThreads);
    OriginDeltaPool pool(1000);
    CHECK(pool.nthreads() == kOriginDeltaMaxThreads);
  }

  if (g_fail) {
    std::printf("test_origin_delta: %d check(s) FAILED\n", g_fail);
    return 1;
  }
  std::printf("test_origin_delta: OK\n");
  return 0;
}
