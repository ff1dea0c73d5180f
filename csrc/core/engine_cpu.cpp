// Serial CPU engine: the correctness oracle for the HIP engine and the
// no-GPU plumbing path (BASELINE config 1).
#include "engine.h"
#include "tally_sink.h"
#include "track.h"
#include "walk.h"

#include <atomic>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <thread>
#include <type_traits>

namespace pumitally {

int default_max_steps(const Mesh &m) {
  const int c = (int)std::ceil(std::cbrt((double)m.nelems));
  return std::max(1000, 32 * c + 64);
}

std::vector<double> normalize_flux(const Mesh &m, const std::vector<double> &flux) {
  if ((int64_t)flux.size() != m.nelems)
    throw std::runtime_error(
        "normalize_flux: flux size != nelems (for grouped tallies normalize "
        "each group slice)");
  std::vector<double> out(m.nelems);
  for (int64_t e = 0; e < m.nelems; ++e) out[e] = flux[e] / m.volumes[e];
  return out;
}

namespace {

class CpuEngine final : public Engine {
  // Where one thread's contributions land: the engine's arrays on the
  // serial path, that thread's partials on the threaded one.
  struct Tallies {
    double *flux, *moments, *currents;
  };
  struct Counts {
    int64_t lost = 0, reloc = 0;
    int64_t entries = 0, misses = 0; // tally_tracks only
  };

public:
  CpuEngine(Mesh mesh, int64_t n, int groups, int scores, bool lin, bool cur,
            bool coll)
      : mesh_(std::move(mesh)), n_(n) {
    ngroups = groups < 1 ? 1 : groups;
    nscores = scores < 1 ? 1 : scores;
    linear = lin;
    face_currents = cur;
    collision_tallies = coll;
    flux_.assign(mesh_.nelems * ngroups * nscores, 0.0);
    if (linear) {
      mesh_.build_inv_heights();
      moments_.assign(flux_.size() * 4, 0.0);
    }
    if (face_currents) currents_.assign(flux_.size() * 4, 0.0);
    if (collision_tallies) collisions_.assign(flux_.size(), 0.0);
    pos_.resize(n_ * 3);
    elem_.assign(n_, 0);
    escaped_.assign(n_, 0);
    const Vec3 c0 = mesh_.nelems > 0 ? mesh_.centroid(0) : Vec3{0, 0, 0};
    for (int64_t i = 0; i < n_; ++i) {
      pos_[i * 3] = c0.x;
      pos_[i * 3 + 1] = c0.y;
      pos_[i * 3 + 2] = c0.z;
    }
    loc_tol_ = loc_tol_rel() * norm(mesh_.bbox_hi - mesh_.bbox_lo);
    walk_fp32 = default_walk_fp32();
    reflective = default_reflective();
  }

  int64_t num_particles() const override { return n_; }
  const Mesh &mesh() const override { return mesh_; }

  void copy_initial_position(const double *p, int64_t n) override {
    check_n(n);
    auto locate_range = [&](int64_t lo, int64_t hi) {
      int64_t my_loose = 0;
      for (int64_t i = lo; i < hi; ++i) {
        const Vec3 q{p[i * 3], p[i * 3 + 1], p[i * 3 + 2]};
        bool loose = false;
        elem_[i] = mesh_.locate(q, loc_tol_, &loose);
        my_loose += loose;
        pos_[i * 3] = q.x;
        pos_[i * 3 + 1] = q.y;
        pos_[i * 3 + 2] = q.z;
        escaped_[i] = 0;
      }
      loose_ += my_loose;
    };
    const unsigned hw = std::thread::hardware_concurrency();
    if (n >= 65536 && hw > 1) {
      const int nthreads = (int)std::min<unsigned>(hw, 64);
      const int64_t per = (n + nthreads - 1) / nthreads;
      std::vector<std::thread> workers;
      for (int t = 0; t < nthreads; ++t)
        workers.emplace_back([&, t] {
          locate_range(t * per, std::min<int64_t>(n, (t + 1) * per));
        });
      for (auto &w : workers) w.join();
      return;
    }
    locate_range(0, n);
  }

  void move(const double *origin, const double *dest, const int8_t *flying,
            const double *weights, int64_t n, const uint16_t *groups = nullptr,
            const double *responses = nullptr) override {
    check_n(n);
    const int steps = max_steps > 0 ? max_steps : default_max_steps(mesh_);
    unsigned hw = std::thread::hardware_concurrency();
    if (const char *env = getenv("PUMITALLY_CPU_THREADS")) {
      const int v = atoi(env);
      hw = v > 0 ? (unsigned)v : 1;
    }
    const Counts c =
        for_each_particle(n, hw, [&](int64_t i, const Tallies &out, Counts &k) {
          move_one(origin, dest, flying, weights, groups, responses, i, steps,
                   out, k);
        });
    stats_.lost_particles += c.lost;
    stats_.relocated += c.reloc;
    stats_.moves++;
  }

  // One particle of a move(): phase A (relocation, skipped for escaped
  // particles -- behavioral pin, see engine.h) + phase B tallied walk.
  void move_one(const double *origin, const double *dest,
                const int8_t *flying, const double *weights,
                const uint16_t *groups, const double *responses, int64_t i,
                int steps, const Tallies &out, Counts &counts) {
    if (!flying[i]) return;
    Vec3 o{pos_[i * 3], pos_[i * 3 + 1], pos_[i * 3 + 2]};
    if (origin && !escaped_[i]) {
      const Vec3 q{origin[i * 3], origin[i * 3 + 1], origin[i * 3 + 2]};
      if (q.x != o.x || q.y != o.y || q.z != o.z) {
        bool loose = false;
        elem_[i] = mesh_.locate(q, loc_tol_, &loose);
        if (loose) loose_++; // rare; atomic is fine in the threaded path
        o = q;
        counts.reloc++;
      }
    }
    if (elem_[i] < 0) {
      // outside the mesh: nothing to tally; remember requested position
      pos_[i * 3] = o.x;
      pos_[i * 3 + 1] = o.y;
      pos_[i * 3 + 2] = o.z;
      return;
    }
    const Vec3 d{dest[i * 3], dest[i * 3 + 1], dest[i * 3 + 2]};
    int32_t out_elem;
    Vec3 out_pos;
    bool out_esc;
    const TallyMesh tm = tally_mesh();
    // an escaped particle leaving again where it sits is one departure
    // (walk.h walk_current_face)
    tally_walk</*ReexitRule=*/true>(
        out, groups, responses, i, tm, escaped_[i] != 0, [&](auto &sink) {
          if (walk_fp32)
            walk_segment32<true>(tm.planes, mesh_.planes32.data(), tm.nbr,
                                 elem_[i], o, d, weights[i], steps, sink,
                                 &out_elem, &out_pos, &out_esc, reflective,
                                 tm.face_bc, tm.pidx,
                                 mesh_.periodic_elem.data(),
                                 mesh_.periodic_shift.data());
          else
            walk_segment<true>(tm.planes, tm.nbr, elem_[i], o, d, weights[i],
                               steps, sink, &out_elem, &out_pos, &out_esc,
                               reflective, tm.face_bc, tm.pidx,
                               mesh_.periodic_elem.data(),
                               mesh_.periodic_shift.data());
        });
    if (out_elem == kWalkLost) {
      counts.lost++;
      record_lost(i, out_pos);
      out_elem = elem_[i];
    }
    elem_[i] = out_elem;
    pos_[i * 3] = out_pos.x;
    pos_[i * 3 + 1] = out_pos.y;
    pos_[i * 3 + 2] = out_pos.z;
    escaped_[i] = out_esc ? 1 : 0;
  }

  void walk_raw(int64_t n, const double *pos, const double *dest,
                const int32_t *elem, const double *weights, double *out_pos,
                int32_t *out_elem, int8_t *out_status,
                const uint16_t *groups = nullptr,
                const double *responses = nullptr,
                double *out_dest = nullptr,
                const double *in_t = nullptr,
                const int32_t *in_prev = nullptr, double *out_o = nullptr,
                double *out_t = nullptr,
                int32_t *out_prev = nullptr) override {
    const int steps = max_steps > 0 ? max_steps : default_max_steps(mesh_);
    // PUMITALLY_CPU_THREADS is move()'s switch; walk_raw threads on the
    // hardware count alone
    const Counts c = for_each_particle(
        n, std::thread::hardware_concurrency(),
        [&](int64_t i, const Tallies &out, Counts &k) {
          walk_raw_one(pos, dest, elem, weights, groups, responses, out_pos,
                       out_elem, out_status, out_dest, in_t, in_prev, out_o,
                       out_t, out_prev, i, steps, out, k);
        });
    stats_.lost_particles += c.lost;
  }

  void walk_raw_one(const double *pos, const double *dest,
                    const int32_t *elem, const double *weights,
                    const uint16_t *groups, const double *responses,
                    double *out_pos, int32_t *out_elem, int8_t *out_status,
                    double *out_dest, const double *in_t,
                    const int32_t *in_prev, double *out_o, double *out_t,
                    int32_t *out_prev, int64_t i, int steps,
                    const Tallies &out, Counts &counts) {
    {
      const Vec3 o{pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2]};
      const Vec3 d{dest[i * 3], dest[i * 3 + 1], dest[i * 3 + 2]};
      int32_t oe;
      Vec3 op;
      bool esc;
      const TallyMesh tm = tally_mesh();
      Vec3 od{d.x, d.y, d.z};
      const double rt = in_t ? in_t[i] : 0.0;
      const int32_t rp = in_prev ? in_prev[i] : -1;
      Vec3 oo{o.x, o.y, o.z};
      double ot = 0.0;
      int32_t opv = -1;
      // Resumed walks (in_t / in_prev) need nothing extra for the moments:
      // in_t only seeds t_cur, pos is the wrap-segment origin the sender
      // exported, so (o, d, seg_len) -- all tet_moments reads besides
      // [t0, t1] -- are the uncut walk's.  For the currents, a resumed walk
      // starts inside its element, so the crossing its sender counted is not
      // counted again; there is no particle state and no re-exit rule.
      tally_walk</*ReexitRule=*/false>(
          out, groups, responses, i, tm, false, [&](auto &sink) {
            if (walk_fp32)
              walk_segment32<true>(tm.planes, mesh_.planes32.data(), tm.nbr,
                                   elem[i], o, d, weights[i], steps, sink, &oe,
                                   &op, &esc, reflective, tm.face_bc, tm.pidx,
                                   mesh_.periodic_elem.data(),
                                   mesh_.periodic_shift.data(), &od, rt, rp,
                                   &oo, &ot, &opv);
            else
              walk_segment<true>(tm.planes, tm.nbr, elem[i], o, d, weights[i],
                                 steps, sink, &oe, &op, &esc, reflective,
                                 tm.face_bc, tm.pidx,
                                 mesh_.periodic_elem.data(),
                                 mesh_.periodic_shift.data(), &od, rt, rp, &oo,
                                 &ot, &opv);
          });
      int8_t st = 0;
      if (oe == kWalkLost) {
        st = 3;
        oe = elem[i];
        counts.lost++;
        record_lost(i, op);
      } else if (esc) {
        st = 1;
      } else if (oe < -1) {
        st = 2;
      }
      out_elem[i] = oe;
      out_pos[i * 3] = op.x;
      out_pos[i * 3 + 1] = op.y;
      out_pos[i * 3 + 2] = op.z;
      out_status[i] = st;
      if (out_dest) {
        out_dest[i * 3] = od.x;
        out_dest[i * 3 + 1] = od.y;
        out_dest[i * 3 + 2] = od.z;
      }
      if (out_o) {
        out_o[i * 3] = oo.x;
        out_o[i * 3 + 1] = oo.y;
        out_o[i * 3 + 2] = oo.z;
      }
      if (out_t) out_t[i] = ot;
      if (out_prev) out_prev[i] = opv;
    }
  }

  // Stateless track tallies (engine.h, track.h).  Threads like walk_raw;
  // particle state is never looked at.
  void tally_tracks(int64_t n, const double *origin, const double *dest,
                    const double *weights, const uint16_t *groups = nullptr,
                    const double *responses = nullptr) override {
    if (n <= 0) return;
    if (tracks_refused_)
      throw std::invalid_argument(
          "track tallies do not support a mesh with partition-cut faces");
    if (mesh_.face_cell_start.empty()) {
      try {
        mesh_.build_face_grid();
      } catch (const std::invalid_argument &) {
        tracks_refused_ = true; // checked once, the answer is kept
        throw;
      }
    }
    const LocGrid &g = mesh_.grid;
    const TallyMesh tm = tally_mesh();
    const TrackMesh trk{
        tm.planes,
        mesh_.planes32.data(),
        tm.nbr,
        GridView{g.nx, g.ny, g.nz, g.lo, g.inv_h, g.cell_start.data(),
                 g.cell_tets.data()},
        FaceGridView{g.nx, g.ny, g.nz, g.lo, g.inv_h,
                     mesh_.face_cell_start.data(),
                     mesh_.face_cell_faces.data()},
        tm.face_bc,
        tm.pidx,
        mesh_.periodic_elem.data(),
        mesh_.periodic_shift.data(),
        reflective,
        loc_tol_,
        max_steps > 0 ? max_steps : default_max_steps(mesh_)};
    const Counts c = for_each_particle(
        n, std::thread::hardware_concurrency(),
        [&](int64_t i, const Tallies &out, Counts &k) {
          const Vec3 o{origin[i * 3], origin[i * 3 + 1], origin[i * 3 + 2]};
          const Vec3 d{dest[i * 3], dest[i * 3 + 1], dest[i * 3 + 2]};
          TrackResult r;
          tally_walk</*ReexitRule=*/false>(
              out, groups, responses, i, tm, false, [&](auto &sink) {
                if (walk_fp32)
                  track_tally<true>(trk, o, d, weights[i], sink, r);
                else
                  track_tally<false>(trk, o, d, weights[i], sink, r);
              });
          k.entries += r.entries;
          k.misses += r.miss;
          if (r.loose) loose_++;
          if (r.lost) {
            k.lost++;
            record_lost(i, r.lost_pos);
          }
        });
    stats_.tracks += n;
    stats_.track_entries += c.entries;
    stats_.track_misses += c.misses;
    stats_.lost_particles += c.lost;
  }

  // Collision-estimator scoring (engine.h).  One gather and one add per
  // particle; a serial loop, so the sums are in caller order.
  void score_collisions(const int8_t *active, const double *weights,
                        int64_t n, const uint16_t *groups = nullptr,
                        const double *responses = nullptr) override {
    if (!collision_tallies) throw_not_collisions();
    check_n(n);
    for (int64_t i = 0; i < n; ++i)
      if (active[i])
        score_one(escaped_[i] ? -1 : elem_[i], weights, groups, responses, i);
  }

  void score_points(int64_t n, const double *xyz, const double *weights,
                    const uint16_t *groups = nullptr,
                    const double *responses = nullptr) override {
    if (!collision_tallies) throw_not_collisions();
    for (int64_t i = 0; i < n; ++i) {
      bool loose = false;
      const int32_t e = mesh_.locate(
          Vec3{xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2]}, loc_tol_, &loose);
      if (loose) loose_++;
      score_one(e, weights, groups, responses, i);
    }
  }

  // Row i of the caller's arrays scores in element e, or misses (e < 0).
  void score_one(int32_t e, const double *weights, const uint16_t *groups,
                 const double *responses, int64_t i) {
    if (e < 0) {
      stats_.collision_misses++;
      return;
    }
    score_contribute(PlainAdder<HostPlus>{}, collisions_.data(),
                     tally_group_offset(groups, i, ngroups, mesh_.nelems),
                     (int64_t)ngroups * mesh_.nelems, e, weights[i], responses,
                     i, nscores);
    stats_.collisions_scored++;
  }

  void end_batch() override {
    if (batch_sum_.empty()) {
      batch_sum_.assign(flux_.size(), 0.0);
      batch_sq_.assign(flux_.size(), 0.0);
    }
    for (size_t e = 0; e < flux_.size(); ++e) {
      batch_sum_[e] += flux_[e];
      batch_sq_[e] += flux_[e] * flux_[e];
      flux_[e] = 0.0;
    }
    if (linear) {
      if (moment_sum_.empty()) moment_sum_.assign(moments_.size(), 0.0);
      for (size_t e = 0; e < moments_.size(); ++e) {
        moment_sum_[e] += moments_[e];
        moments_[e] = 0.0;
      }
    }
    if (face_currents) {
      if (current_sum_.empty()) {
        current_sum_.assign(currents_.size(), 0.0);
        current_sq_.assign(currents_.size(), 0.0);
      }
      for (size_t e = 0; e < currents_.size(); ++e) {
        current_sum_[e] += currents_[e];
        current_sq_[e] += currents_[e] * currents_[e];
        currents_[e] = 0.0;
      }
    }
    if (collision_tallies) {
      if (collision_sum_.empty()) {
        collision_sum_.assign(collisions_.size(), 0.0);
        collision_sq_.assign(collisions_.size(), 0.0);
      }
      for (size_t e = 0; e < collisions_.size(); ++e) {
        collision_sum_[e] += collisions_[e];
        collision_sq_[e] += collisions_[e] * collisions_[e];
        collisions_[e] = 0.0;
      }
    }
    nbatches_++;
  }
  std::vector<double> batch_sum() const override {
    return batch_sum_.empty() ? std::vector<double>(flux_.size(), 0.0) : batch_sum_;
  }
  std::vector<double> batch_sum_sq() const override {
    return batch_sq_.empty() ? std::vector<double>(flux_.size(), 0.0) : batch_sq_;
  }
  int64_t num_batches() const override { return nbatches_; }

  std::vector<double> flux() const override { return flux_; }
  std::vector<int32_t> elem_ids() const override { return elem_; }
  std::vector<double> positions() const override { return pos_; }
  std::vector<uint8_t> escaped() const override { return escaped_; }
  const EngineStats &stats() const override {
    stats_.loose_localizations = loose_.load();
    return stats_;
  }

  std::vector<double> lost_records() const override {
    const int64_t k =
        std::min<int64_t>(lost_rec_n_.load(), kMaxLostRecords);
    return {lost_rec_.begin(), lost_rec_.begin() + k * 4};
  }

  void set_flux(const double *f, int64_t ne) override {
    if (ne != (int64_t)flux_.size()) throw std::runtime_error("set_flux size mismatch");
    std::memcpy(flux_.data(), f, ne * sizeof(double));
  }

  std::vector<double> moments() const override {
    if (!linear) throw_not_linear();
    return moments_;
  }
  std::vector<double> moment_sum() const override {
    if (!linear) throw_not_linear();
    return moment_sum_.empty() ? std::vector<double>(moments_.size(), 0.0)
                               : moment_sum_;
  }
  void set_moments(const double *m, int64_t n) override {
    if (!linear) throw_not_linear();
    if (n != (int64_t)moments_.size())
      throw std::runtime_error("set_moments size mismatch");
    std::memcpy(moments_.data(), m, n * sizeof(double));
  }

  std::vector<double> currents() const override {
    if (!face_currents) throw_not_currents();
    return currents_;
  }
  std::vector<double> current_sum() const override {
    if (!face_currents) throw_not_currents();
    return current_sum_.empty() ? std::vector<double>(currents_.size(), 0.0)
                                : current_sum_;
  }
  std::vector<double> current_sum_sq() const override {
    if (!face_currents) throw_not_currents();
    return current_sq_.empty() ? std::vector<double>(currents_.size(), 0.0)
                               : current_sq_;
  }
  void set_currents(const double *j, int64_t n) override {
    if (!face_currents) throw_not_currents();
    if (n != (int64_t)currents_.size())
      throw std::runtime_error("set_currents size mismatch");
    std::memcpy(currents_.data(), j, n * sizeof(double));
  }

  std::vector<double> collisions() const override {
    if (!collision_tallies) throw_not_collisions();
    return collisions_;
  }
  std::vector<double> collision_sum() const override {
    if (!collision_tallies) throw_not_collisions();
    return collision_sum_.empty()
               ? std::vector<double>(collisions_.size(), 0.0)
               : collision_sum_;
  }
  std::vector<double> collision_sum_sq() const override {
    if (!collision_tallies) throw_not_collisions();
    return collision_sq_.empty()
               ? std::vector<double>(collisions_.size(), 0.0)
               : collision_sq_;
  }
  void set_collisions(const double *c, int64_t n) override {
    if (!collision_tallies) throw_not_collisions();
    if (n != (int64_t)collisions_.size())
      throw std::runtime_error("set_collisions size mismatch");
    std::memcpy(collisions_.data(), c, n * sizeof(double));
  }

  void set_particle_state(const double *pos, const int32_t *elem,
                          const uint8_t *escaped, int64_t n) override {
    check_n(n);
    std::memcpy(pos_.data(), pos, n * 3 * sizeof(double));
    std::memcpy(elem_.data(), elem, n * sizeof(int32_t));
    std::memcpy(escaped_.data(), escaped, n);
  }

private:
  void check_n(int64_t n) const {
    if (n != n_) throw std::runtime_error("particle count mismatch");
  }

  // Runs one(i, tallies, counts) for every particle i in [0, n).
  // Thread-parallel over particles for large batches (the reference's CPU
  // path is Kokkos OpenMP), on up to `hw` threads.  Each thread tallies into
  // private partials; they are summed in thread-index order, so results are
  // DETERMINISTIC for a fixed thread count (and exactly serial-order for one
  // thread).  Small batches stay serial for bitwise stability of the golden
  // tests.
  template <class One>
  Counts for_each_particle(int64_t n, unsigned hw, One one) {
    Counts total;
    const int nthreads =
        (n >= 65536 && hw > 1) ? (int)std::min<unsigned>(hw, 64) : 1;
    if (nthreads == 1) {
      const Tallies out{flux_.data(), moments_.data(), currents_.data()};
      for (int64_t i = 0; i < n; ++i) one(i, out, total);
      return total;
    }
    // Every partial has its array's FULL shape, score dimension included:
    // the scored add writes k*ngroups*nelems + group*nelems + elem for
    // k < nscores (an nelems*ngroups-sized partial overflows the heap --
    // found by tools/part_world2_soak at 400k particles with nscores=2).
    // Moments and currents are 4x the flux shape, or empty (and never
    // written) when the engine does not tally them.
    std::vector<double> *const arrays[3] = {&flux_, &moments_, &currents_};
    std::vector<std::vector<double>> partial[3];
    for (int a = 0; a < 3; ++a)
      partial[a].assign(nthreads, std::vector<double>(arrays[a]->size(), 0.0));
    std::vector<Counts> counts(nthreads);
    std::vector<std::thread> workers;
    const int64_t per = (n + nthreads - 1) / nthreads;
    for (int t = 0; t < nthreads; ++t) {
      workers.emplace_back([&, t] {
        const int64_t lo = t * per, hi = std::min<int64_t>(n, lo + per);
        const Tallies out{partial[0][t].data(), partial[1][t].data(),
                          partial[2][t].data()};
        Counts mine;
        for (int64_t i = lo; i < hi; ++i) one(i, out, mine);
        counts[t] = mine;
      });
    }
    for (auto &w : workers) w.join();
    for (int a = 0; a < 3; ++a)
      for (int t = 0; t < nthreads; ++t)
        for (size_t e = 0; e < arrays[a]->size(); ++e)
          (*arrays[a])[e] += partial[a][t][e];
    for (const Counts &c : counts) {
      total.lost += c.lost;
      total.reloc += c.reloc;
      total.entries += c.entries;
      total.misses += c.misses;
    }
    return total;
  }

  TallyMesh tally_mesh() const {
    return {mesh_.planes.data(),
            mesh_.inv_heights.data(),
            mesh_.nbr.data(),
            mesh_.face_bc_bits.empty() ? nullptr : mesh_.face_bc_bits.data(),
            mesh_.periodic_idx.empty() ? nullptr : mesh_.periodic_idx.data(),
            reflective};
  }

  // Builds particle i's tally sink (tally_sink.h) for the engine's mode, with
  // plain += into `out`, and hands it to walk(sink).
  template <bool ReexitRule, class Walk>
  void tally_walk(const Tallies &out, const uint16_t *groups,
                  const double *responses, int64_t i, const TallyMesh &tm,
                  bool reexit, Walk walk) const {
    auto go = [&](auto mode, double *companion) {
      TallySink<decltype(mode)::value, /*Scored=*/true, PlainAdder<HostPlus>,
                ReexitRule, /*Periodic=*/true>
          sink{{},
               out.flux,
               companion,
               tally_group_offset(groups, i, ngroups, mesh_.nelems),
               (int64_t)ngroups * mesh_.nelems,
               responses,
               i,
               nscores,
               tm,
               reexit};
      walk(sink);
    };
    using M = TallyMode;
    if (linear)
      go(std::integral_constant<M, M::Linear>{}, out.moments);
    else if (face_currents)
      go(std::integral_constant<M, M::Currents>{}, out.currents);
    else
      go(std::integral_constant<M, M::Flux>{}, nullptr);
  }

  void record_lost(int64_t i, Vec3 p) {
    const int64_t k = lost_rec_n_.fetch_add(1);
    if (k < kMaxLostRecords) {
      lost_rec_[k * 4] = (double)i;
      lost_rec_[k * 4 + 1] = p.x;
      lost_rec_[k * 4 + 2] = p.y;
      lost_rec_[k * 4 + 3] = p.z;
    }
  }

  Mesh mesh_;
  int64_t n_;
  double loc_tol_;
  std::vector<double> flux_, pos_, batch_sum_, batch_sq_;
  std::vector<double> moments_, moment_sum_; // linear mode only, else empty
  // face currents only, else empty
  std::vector<double> currents_, current_sum_, current_sq_;
  // collision tallies only, else empty; never a for_each_particle target
  std::vector<double> collisions_, collision_sum_, collision_sq_;
  int64_t nbatches_ = 0;
  bool tracks_refused_ = false; // tally_tracks: the mesh has cut faces
  std::vector<int32_t> elem_;
  std::vector<uint8_t> escaped_;
  mutable EngineStats stats_;
  std::atomic<int64_t> loose_{0};
  std::vector<double> lost_rec_ =
      std::vector<double>((size_t)kMaxLostRecords * 4, 0.0);
  std::atomic<int64_t> lost_rec_n_{0};
};

} // namespace

std::unique_ptr<Engine> make_cpu_engine(Mesh mesh, int64_t num_particles,
                                        int ngroups, int nscores,
                                        bool linear, bool currents,
                                        bool collisions) {
  check_tally_options(linear, currents);
  return std::make_unique<CpuEngine>(std::move(mesh), num_particles, ngroups,
                                     nscores, linear, currents, collisions);
}

} // namespace pumitally
