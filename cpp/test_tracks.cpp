// Stateless track tallies on the CPU engine (core/track.h, core/engine.h):
//   * ray_enter through the boundary-face grid against a brute-force loop over
//     every vacuum boundary face -- the same face and a bitwise-identical t --
//     for random, axis-parallel and cell-wall-hugging segments on a jittered
//     and an unjittered shell with a cavity;
//   * the golden cube numbers through Engine::tally_tracks.
// No GPU: passes in a build configured with a plain host compiler.
#include "core/engine.h"
#include "core/track.h"

#include <cstdio>
#include <cstring>
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

// The 156-tet shell: the tets of build_box(5,5,5,5,5,5) whose (unjittered)
// centroid cell is in [1,3]^3, minus the centre cell; interior vertices
// optionally moved by up to 0.15 per axis.
Mesh make_shell(bool jitter) {
  const Mesh box = build_box(5, 5, 5, 5.0, 5.0, 5.0);
  std::vector<double> coords = box.coords;
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> jit(-0.15, 0.15);
  if (jitter)
    for (int64_t v = 0; v < box.nverts; ++v) {
      bool inner = true;
      for (int k = 0; k < 3; ++k)
        inner &= coords[v * 3 + k] > 1e-9 && coords[v * 3 + k] < 5.0 - 1e-9;
      if (inner)
        for (int k = 0; k < 3; ++k) coords[v * 3 + k] += jit(rng);
    }
  std::vector<int32_t> remap(box.nverts, -1), tets;
  std::vector<char> used(box.nverts, 0);
  std::vector<int32_t> kept;
  for (int32_t t = 0; t < box.nelems; ++t) {
    const Vec3 c = box.centroid(t);
    const int cx = (int)c.x, cy = (int)c.y, cz = (int)c.z;
    const bool in = cx >= 1 && cx <= 3 && cy >= 1 && cy <= 3 && cz >= 1 &&
                    cz <= 3 && !(cx == 2 && cy == 2 && cz == 2);
    if (!in) continue;
    kept.push_back(t);
    for (int k = 0; k < 4; ++k) used[box.tet2vert[t * 4 + k]] = 1;
  }
  std::vector<double> sub_coords;
  int32_t next = 0;
  for (int64_t v = 0; v < box.nverts; ++v)
    if (used[v]) {
      remap[v] = next++;
      for (int k = 0; k < 3; ++k) sub_coords.push_back(coords[v * 3 + k]);
    }
  for (int32_t t : kept)
    for (int k = 0; k < 4; ++k) tets.push_back(remap[box.tet2vert[t * 4 + k]]);
  return mesh_from_arrays(next, sub_coords.data(), (int64_t)kept.size(),
                          tets.data());
}

int32_t brute_enter(const Mesh &m, Vec3 o, Vec3 d, double t_min, double tol,
                    double *t_out) {
  int32_t best = -1;
  double best_t = 2.0;
  for (int64_t f = m.nelems * 4 - 1; f >= 0; --f) // descending on purpose
    if (m.nbr[f] == -1)
      ray_consider(m.planes.data(), (int32_t)f, o, d, t_min, tol, best, best_t);
  if (best >= 0) *t_out = best_t;
  return best;
}

void grid_against_brute(bool jitter) {
  Mesh m = make_shell(jitter);
  CHECK(m.nelems == 156);
  m.build_face_grid();
  int64_t nb = 0;
  for (int32_t v : m.nbr) nb += v == -1;
  CHECK(nb == 120);
  CHECK((int64_t)m.face_cell_start.size() ==
        (int64_t)m.grid.nx * m.grid.ny * m.grid.nz + 1);
  const FaceGridView g{m.grid.nx,
                       m.grid.ny,
                       m.grid.nz,
                       m.grid.lo,
                       m.grid.inv_h,
                       m.face_cell_start.data(),
                       m.face_cell_faces.data()};
  const double tol = 1e-10 * norm(m.bbox_hi - m.bbox_lo);
  std::mt19937_64 rng(jitter ? 21 : 22);
  std::uniform_real_distribution<double> pos(-1.0, 6.0), unit(0.0, 1.0);
  // coordinates that sit on grid-cell walls, mesh planes and the cavity wall
  const double special[] = {0.0, 1.0, 2.0, 2.5, 3.0, 4.0, 5.0};
  int64_t hits = 0, later = 0;
  for (int i = 0; i < 20000; ++i) {
    Vec3 o{pos(rng), pos(rng), pos(rng)}, d{pos(rng), pos(rng), pos(rng)};
    const int kind = i % 5;
    double *oc[3] = {&o.x, &o.y, &o.z}, *dc[3] = {&d.x, &d.y, &d.z};
    if (kind == 1 || kind == 2) { // axis-parallel: two coordinates frozen
      const int a = (int)(rng() % 3);
      for (int k = 0; k < 3; ++k)
        if (k != a) {
          if (kind == 2) *oc[k] = special[rng() % 7]; // ... on a wall
          *dc[k] = *oc[k];
        }
    } else if (kind == 3) { // lying in a cell-boundary plane, e.g. y = 2.0
      const int a = (int)(rng() % 3);
      *oc[a] = *dc[a] = special[rng() % 7];
    }
    const double t_min = kind == 4 ? unit(rng) : 0.0;
    double tg = -1.0, tb = -1.0;
    const int32_t fg = ray_enter(g, m.planes.data(), o, d, t_min, tol, &tg);
    const int32_t fb = brute_enter(m, o, d, t_min, tol, &tb);
    if (fg != fb || std::memcmp(&tg, &tb, sizeof tg) != 0) {
      if (g_fail < 10)
        std::printf("  case %d kind %d: grid (%d, %.17g) brute (%d, %.17g)\n", i,
                    kind, fg, tg, fb, tb);
      ++g_fail;
    }
    hits += fg >= 0;
    later += fg >= 0 && t_min > 0.0;
  }
  std::printf("  %s shell: %lld of 20000 searches hit, %lld with t_min > 0\n",
              jitter ? "jittered" : "plain", (long long)hits, (long long)later);
  // both outcomes are well exercised (wall-hugging segments mostly miss)
  CHECK(hits > 3000 && hits < 17000 && later > 300);
}

void golden_cube() {
  auto eng = make_cpu_engine(build_box(1, 1, 1, 1.0, 1.0, 1.0), 2);
  const std::vector<double> pos0 = eng->positions();
  const double o[] = {-0.5, 0.4, 0.5, -1e3, 0.4, 0.5, -0.5, 2.0, 2.0,
                      0.3,  0.4, 0.5, -0.5, 0.4, 0.5};
  const double d[] = {1.2, 0.4, 0.5, 1e3, 0.4, 0.5, 1.5, 2.0, 2.0,
                      0.3, 0.4, 0.5, 1.2, 0.4, 0.5};
  const double w[] = {1.0, 1.0, 1.0, 1.0, 0.0};
  eng->tally_tracks(1, o, d, w);
  std::vector<double> f = eng->flux();
  const double want[6] = {0, 0, 0.4, 0.1, 0.5, 0};
  for (int e = 0; e < 6; ++e) CHECK(std::fabs(f[e] - want[e]) <= 1e-15);
  CHECK(eng->stats().tracks == 1 && eng->stats().track_entries == 1 &&
        eng->stats().track_misses == 0);
  eng->tally_tracks(4, o + 3, d + 3, w + 1); // far chord, miss, two skipped
  f = eng->flux();
  for (int e = 0; e < 6; ++e) CHECK(std::fabs(f[e] - 2 * want[e]) <= 1e-12);
  CHECK(eng->stats().tracks == 5 && eng->stats().track_entries == 2 &&
        eng->stats().track_misses == 1 && eng->stats().lost_particles == 0);
  eng->tally_tracks(0, nullptr, nullptr, nullptr);
  CHECK(eng->stats().tracks == 5);
  CHECK(eng->positions() == pos0);
  bool threw = false;
  try {
    eng->tally_tracks_device(1, o, d, w);
  } catch (const std::runtime_error &) {
    threw = true;
  }
  CHECK(threw);
}

void cut_mesh_is_refused() {
  const Mesh m = build_box(3, 3, 3, 1.0, 1.0, 1.0);
  const SubMesh part = extract_submesh(m, partition_morton(m, 2), 0);
  auto eng = make_cpu_engine(part.local, 1);
  const double o[] = {0.1, 0.1, 0.1}, d[] = {0.9, 0.9, 0.9}, w[] = {1.0};
  for (int k = 0; k < 2; ++k) {
    bool threw = false;
    try {
      eng->tally_tracks(1, o, d, w);
    } catch (const std::invalid_argument &) {
      threw = true;
    }
    CHECK(threw);
  }
}

} // namespace

int main() {
  std::printf("test_tracks\n");
  grid_against_brute(true);
  grid_against_brute(false);
  golden_cube();
  cut_mesh_is_refused();
  std::printf(g_fail ? "FAILED (%d)\n" : "OK\n", g_fail);
  return g_fail ? 1 : 0;
}
