// World-1 scenario for the CPU stateful partitioned engine, shared by
// cpp/test_partition_engine_cpu.cpp and the sanitizer harness
// (tools/asan_check.cpp): 100 particles on build_box(3,3,3), 3 steps with
// ~10 % of origins resampled (some outside the mesh), 2 energy groups.
// flux_global() must equal the replicated CPU engine at 1e-12, driven once
// through step() and once through resident_list()/step_local().
#pragma once

#include "../csrc/core/engine.h"
#include "../csrc/core/partition_engine.h"

#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

namespace pumitally {

// returns the number of failed checks
inline int partition_cpu_scenario() {
  const int64_t n = 100;
  const int steps = 3, ngroups = 2;
  const Mesh mesh = build_box(3, 3, 3, 1.0, 1.0, 1.0);
  std::mt19937_64 rng(2024);
  std::uniform_real_distribution<double> inside(0.05, 0.95);
  std::uniform_real_distribution<double> around(-0.05, 1.05);
  std::uniform_real_distribution<double> u01(0.0, 1.0);
  std::normal_distribution<double> hop(0.0, 0.3);

  struct Step {
    std::vector<double> origin, dest, w;
    std::vector<int8_t> fly;
  };
  std::vector<double> p0(n * 3);
  for (double &v : p0) v = inside(rng);
  std::vector<uint16_t> grp(n);
  for (uint16_t &g : grp) g = (uint16_t)(rng() % ngroups);

  // the replicated oracle also supplies each step's committed positions,
  // so an origin differs from them exactly where it was resampled
  auto oracle = make_cpu_engine(mesh, n, ngroups);
  oracle->copy_initial_position(p0.data(), n);
  std::vector<Step> hist(steps);
  for (Step &s : hist) {
    s.origin = oracle->positions();
    s.dest.resize(n * 3);
    s.w.resize(n);
    s.fly.resize(n);
    for (int64_t i = 0; i < n; ++i) {
      if (u01(rng) < 0.10)
        for (int k = 0; k < 3; ++k) s.origin[i * 3 + k] = around(rng);
      for (int k = 0; k < 3; ++k) {
        const double d = s.origin[i * 3 + k] + hop(rng);
        s.dest[i * 3 + k] = d < -0.1 ? -0.1 : (d > 1.1 ? 1.1 : d);
      }
      s.w[i] = 0.1 + 0.9 * u01(rng);
      s.fly[i] = u01(rng) > 0.1 ? 1 : 0;
    }
    oracle->move(s.origin.data(), s.dest.data(), s.fly.data(), s.w.data(), n,
                 grp.data());
  }
  const std::vector<double> want = oracle->flux();

  int fail = 0;
  for (int local = 0; local < 2; ++local) {
    auto pe = make_partitioned_engine(mesh, n, nullptr, 0, 1, "cpu", ngroups);
    pe->localize(p0.data(), n);
    for (const Step &s : hist) {
      if (!local) {
        pe->step(s.dest.data(), s.fly.data(), s.w.data(), n, s.origin.data(),
                 grp.data());
        continue;
      }
      const std::vector<int64_t> gids = pe->resident_list();
      const int64_t m = (int64_t)gids.size();
      std::vector<double> o(m * 3), d(m * 3), w(m);
      std::vector<int8_t> f(m);
      std::vector<uint16_t> g(m);
      for (int64_t j = 0; j < m; ++j) {
        for (int k = 0; k < 3; ++k) {
          o[j * 3 + k] = s.origin[gids[j] * 3 + k];
          d[j * 3 + k] = s.dest[gids[j] * 3 + k];
        }
        w[j] = s.w[gids[j]];
        f[j] = s.fly[gids[j]];
        g[j] = grp[gids[j]];
      }
      pe->step_local(d.data(), f.data(), w.data(), m, o.data(), g.data());
    }
    const std::vector<double> got = pe->flux_global();
    double worst = 0.0, total = 0.0;
    for (size_t i = 0; i < want.size(); ++i) {
      worst = std::fmax(worst, std::fabs(got[i] - want[i]));
      total += want[i];
    }
    const bool ok = got.size() == want.size() && worst <= 1e-12 &&
                    total > 0.0 && pe->resident() == n &&
                    pe->stats().relocated > 0;
    std::printf("partition_cpu_scenario[%s]: max |dflux| %.3e, relocated "
                "%lld: %s\n",
                local ? "step_local" : "step", worst,
                (long long)pe->stats().relocated, ok ? "ok" : "FAIL");
    if (!ok) ++fail;
  }
  return fail;
}

} // namespace pumitally
