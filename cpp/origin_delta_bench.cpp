// Stand-alone timing of the origin-elision host pass
// (csrc/core/origin_delta.h) on pinned buffers allocated the way
// pumiumtally_amd.pinned_array allocates them (hipHostMalloc, default flags).
//
//   origin_delta_bench [n_particles=10000000] [reps=10]
//
// Sweeps worker threads {1, 4, 8, 16} x shadow stores {streaming, ordinary}
// x changed origins {none, 10 % on every other pass}, ping-ponging two
// end-point arrays exactly as the headline benchmark does.  Prints ms per
// pass (min / median).
#include "core/origin_delta.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

using namespace pumitally;

static double *pinned_doubles(int64_t count) {
  void *p = nullptr;
  if (hipHostMalloc(&p, count * sizeof(double), hipHostMallocDefault) !=
      hipSuccess) {
    std::fprintf(stderr, "hipHostMalloc failed\n");
    std::exit(2);
  }
  return (double *)p;
}

int main(int argc, char **argv) {
  const int64_t n = argc > 1 ? atoll(argv[1]) : 10000000;
  const int reps = argc > 2 ? atoi(argv[2]) : 10;
  double *ends[2] = {pinned_doubles(n * 3), pinned_doubles(n * 3)};
  double *alt = pinned_doubles(n * 3); // ends[0] with 10 % resampled
  std::mt19937_64 rng(1);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  for (int64_t k = 0; k < n * 3; ++k) {
    ends[0][k] = u(rng);
    ends[1][k] = u(rng);
  }
  std::memcpy(alt, ends[0], n * 3 * sizeof(double));
  for (int64_t i = 0; i < n; ++i)
    if (rng() % 10 == 0) alt[i * 3 + 1] = u(rng);
  std::unique_ptr<double[]> shadow(new double[n * 3]);
  int64_t cap = 0; // the block layout, hence the capacity, depends on threads
  for (int nt : {1, 4, 8, 16})
    cap = std::max(cap, origin_delta_patch_capacity(n, nt));
  void *pi = nullptr, *px = nullptr;
  if (hipHostMalloc(&pi, cap * sizeof(int32_t), hipHostMallocDefault) !=
          hipSuccess ||
      hipHostMalloc(&px, cap * 3 * sizeof(double), hipHostMallocDefault) !=
          hipSuccess) {
    std::fprintf(stderr, "hipHostMalloc failed\n");
    return 2;
  }
  std::printf("n=%lld reps=%d (96 B/particle streamed, 120 B ordinary)\n",
              (long long)n, reps);
  for (int nt : {1, 4, 8, 16}) {
    OriginDeltaPool pool(nt);
    for (int nontemporal = 1; nontemporal >= 0; --nontemporal) {
      for (int frac10 = 0; frac10 < 2; ++frac10) {
        // shadow := ends[0], as left by a move whose dest was ends[0]
        origin_delta_seed(pool, ends[0], shadow.get(), 0, n, nontemporal != 0);
        std::vector<double> ms;
        int64_t changed = 0;
        for (int r = 0; r < reps; ++r) {
          // move r: origin = previous dest (ends[r&1], or its 10 % resampled
          // twin on even moves), dest = the other end
          const double *origin =
              (frac10 && (r & 1) == 0) ? alt : ends[r & 1];
          const auto t0 = std::chrono::steady_clock::now();
          OriginDeltaResult res = origin_delta_pass(
              pool, origin, ends[(r + 1) & 1], shadow.get(), 0, n,
              (int32_t *)pi, (double *)px, nontemporal != 0);
          if (!res.overflow)
            origin_delta_compact(res, (int32_t *)pi, (double *)px);
          const auto t1 = std::chrono::steady_clock::now();
          ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0)
                           .count());
          changed += res.changed;
        }
        std::sort(ms.begin(), ms.end());
        std::printf("threads=%2d stores=%-9s changed=%-4s  min %7.2f ms  "
                    "median %7.2f ms  (%.1f GB/s at median; changed/pass "
                    "%lld)\n",
                    nt, nontemporal ? "streaming" : "ordinary",
                    frac10 ? "~5%" : "0", ms.front(), ms[ms.size() / 2],
                    (nontemporal ? 96.0 : 120.0) * n / ms[ms.size() / 2] / 1e6,
                    (long long)(changed / reps));
      }
    }
  }
  return 0;
}
