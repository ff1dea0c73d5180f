// CPU stateful partitioned engine: the same algorithm as the GPU engine
// (csrc/hip/partition_engine.hip) with host loops.  It is the differential
// oracle for the GPU engine and the no-GPU fallback.  Plain C++17, no HIP.
#include "partition_engine_common.h"

#include "../comm/comm.h"

#include <utility>

namespace pumitally {

namespace {

class CpuPartitionedEngine final : public PartitionedEngineBase {
public:
  explicit CpuPartitionedEngine(const PartitionedEngineArgs &a)
      : PartitionedEngineBase(a) {
    eng_ = make_cpu_engine(dec_.sub.local, 1, ngroups_, nscores_);
    pos_.assign(n_ * 3, 0.0);
    elem_.assign(n_, -1);
    res_.assign(n_, 0);
    esc_.assign(n_, 0);
  }

  void localize(const double *origins, int64_t n) override {
    check_n(n);
    const Mesh &lm = dec_.sub.local;
    std::vector<int64_t> claim((n_ + 63) / 64, 0);
    for (int64_t g = 0; g < n_; ++g) {
      res_[g] = 0;
      const Vec3 q{origins[g * 3], origins[g * 3 + 1], origins[g * 3 + 2]};
      bool lo = false;
      const int32_t le = lm.locate(q, loc_tol_, &lo);
      // strict hits only -- loose submesh hits can steal points whose
      // true element is absent from the ghost ring (GPU k_part_localize
      // comment); the full-mesh pass below resolves them
      if (le >= 0 && !lo && dec_.lowner[le] == rank_) {
        place(g, le, q);
        claim[g >> 6] |= (int64_t)(1ull << (g & 63));
      }
    }
    std::vector<int32_t> cg, cl;
    resolve_unclaimed(origins, claim, cg, cl);
    for (size_t i = 0; i < cg.size(); ++i) {
      const int64_t g = cg[i];
      place(g, cl[i],
            Vec3{origins[g * 3], origins[g * 3 + 1], origins[g * 3 + 2]});
    }
    if (rank_ == 0) {
      // rank 0 claims globally-unfound particles (outside the mesh)
      for (int64_t g = 0; g < n_; ++g)
        if (!((claim[g >> 6] >> (g & 63)) & 1))
          place(g, -1,
                Vec3{origins[g * 3], origins[g * 3 + 1], origins[g * 3 + 2]});
    }
  }

  // A resolved unit of walk work: every input the particle needs travels
  // with it, so global-array steps, coupled-host steps and exchanged
  // arrivals all feed the same loop (the CPU mirror of the GPU wire
  // format).
  struct Item {
    int64_t gid;
    Vec3 pos, dest;
    double w;
    uint16_t grp;
    std::vector<double> resp; // nscores entries when used, else empty
    int32_t lelem;
    // bitwise handoff resume (walk.h walk_segment doc): pos carries the
    // wrap-segment origin for exchanged arrivals; t0/prev seed the walk
    double t0 = 0.0;
    int32_t prev = -1;
  };

  void step(const double *dest, const int8_t *flying, const double *weights,
            int64_t n, const double *origin, const uint16_t *groups,
            const double *responses) override {
    check_n(n);
    check_groups(groups, ngroups_);
    std::vector<Item> items;
    std::vector<double> dep;
    for (int64_t g = 0; g < n_; ++g) {
      if (!res_[g] || !flying[g]) continue;
      enter_particle(g, origin ? origin + g * 3 : nullptr, dest + g * 3,
                     weights[g], groups ? groups[g] : (uint16_t)0,
                     responses ? responses + g * nscores_ : nullptr, items,
                     dep);
    }
    run_items(std::move(items), std::move(dep), responses != nullptr);
    stats_.moves++;
  }

  std::vector<int64_t> resident_list() override {
    frame_.clear();
    for (int64_t g = 0; g < n_; ++g)
      if (res_[g]) frame_.push_back(g);
    have_frame_ = true;
    return frame_;
  }

  void step_local(const double *dest, const int8_t *flying,
                  const double *weights, int64_t n_local,
                  const double *origin, const uint16_t *groups,
                  const double *responses) override {
    check_step_local(n_local, have_frame_ ? (int64_t)frame_.size() : -1,
                     groups);
    std::vector<Item> items;
    std::vector<double> dep;
    for (int64_t j = 0; j < n_local; ++j) {
      const int64_t g = frame_[j];
      if (!res_[g] || !flying[j]) continue;
      enter_particle(g, origin ? origin + j * 3 : nullptr, dest + j * 3,
                     weights[j], groups ? groups[j] : (uint16_t)0,
                     responses ? responses + j * nscores_ : nullptr, items,
                     dep);
    }
    have_frame_ = false; // residency changes below
    run_items(std::move(items), std::move(dep), responses != nullptr);
    stats_.moves++;
  }

  int64_t resident() const override {
    int64_t c = 0;
    for (uint8_t v : res_) c += v;
    return c;
  }

  std::vector<uint8_t> resident_mask() const override { return res_; }
  std::vector<double> positions() const override { return pos_; }
  std::vector<int32_t> elem_ids() const override { return elem_; }

  std::vector<int32_t> elem_ids_global() const override {
    std::vector<int32_t> out(n_, -1);
    for (int64_t g = 0; g < n_; ++g)
      if (res_[g] && elem_[g] >= 0) out[g] = dec_.l2g32[elem_[g]];
    return out;
  }

  std::vector<uint8_t> escaped_mask() const override { return esc_; }

  void set_state(const double *pos, const int32_t *gelem,
                 const uint8_t *escaped, int64_t n) override {
    check_n(n);
    claim_state(gelem, res_, elem_);
    pos_.assign(pos, pos + n_ * 3);
    esc_.assign(escaped, escaped + n_);
    have_frame_ = false;
  }

private:
  void set_pos(int64_t g, Vec3 q) {
    pos_[g * 3] = q.x;
    pos_[g * 3 + 1] = q.y;
    pos_[g * 3 + 2] = q.z;
  }

  // particle g becomes resident here, unescaped, in local element le at q
  void place(int64_t g, int32_t le, Vec3 q) {
    res_[g] = 1;
    esc_[g] = 0;
    elem_[g] = le;
    set_pos(g, q);
  }

  // Phase A + admission for one flying resident particle: relocation /
  // reroute / eject resolution, then either queue a walk Item or emit a
  // departure record.  resp == nullptr: no responses this step.
  void enter_particle(int64_t g, const double *origin3, const double *dest3,
                      double w, uint16_t grp, const double *resp,
                      std::vector<Item> &items, std::vector<double> &dep) {
    const Mesh &lm = dec_.sub.local;
    const Vec3 d{dest3[0], dest3[1], dest3[2]};
    if (origin3 && !esc_[g]) {
      const Vec3 q{origin3[0], origin3[1], origin3[2]};
      if (q.x != pos_[g * 3] || q.y != pos_[g * 3 + 1] ||
          q.z != pos_[g * 3 + 2]) {
        stats_.relocated++;
        bool lo = false;
        int32_t le = lm.locate(q, loc_tol_, &lo);
        if (lo) le = -1; // loose submesh hit: resolve on the full mesh
        int64_t tgid = -1;
        int towner = -1;
        if (le >= 0 && dec_.lowner[le] != rank_) {
          tgid = dec_.l2g32[le];
          towner = dec_.lowner[le];
        } else if (le < 0) {
          const int32_t ge = locate_full(q);
          if (ge >= 0) {
            tgid = ge;
            towner = dec_.owners[ge];
          } else {
            elem_[g] = -1; // outside the mesh: park at the origin
            set_pos(g, q);
            return;
          }
        }
        if (towner >= 0) {
          // fresh walk on the owner: no resume state
          emit_dep(dep, g, q, tgid, d, w, 0.0, -1, grp, resp, towner);
          res_[g] = 0;
          return;
        }
        elem_[g] = le;
        set_pos(g, q);
      }
    }
    if (elem_[g] < 0) return; // outside mesh
    Item it;
    it.gid = g;
    it.pos = Vec3{pos_[g * 3], pos_[g * 3 + 1], pos_[g * 3 + 2]};
    it.dest = d;
    it.w = w;
    it.grp = grp;
    if (resp) it.resp.assign(resp, resp + nscores_);
    it.lelem = elem_[g];
    items.push_back(std::move(it));
  }

  void emit_dep(std::vector<double> &dep, int64_t g, Vec3 p, int64_t tgid,
                Vec3 d, double w, double t, int64_t prev_gid, uint16_t grp,
                const double *resp, int owner) {
    const size_t base = dep.size();
    dep.resize(base + rec_.dep_width(), 0.0);
    rec_.write(dep.data() + base, g, p, tgid, d, w, t, prev_gid, grp, resp,
               owner);
  }

  void run_items(std::vector<Item> items, std::vector<double> dep,
                 bool resp_used) {
    const bool groups_used = rec_.carry_grp;
    const int rw = rec_.width(), dw = rec_.dep_width();
    for (int round = 0; round <= max_rounds(); ++round) {
      if (!items.empty()) {
        const int64_t m = (int64_t)items.size();
        std::vector<double> wpos(m * 3), wdest(m * 3), ww(m),
            wout_pos(m * 3), wout_dest(m * 3);
        std::vector<int32_t> welem(m), wout_elem(m);
        std::vector<int8_t> wstatus(m);
        std::vector<uint16_t> wgrp(groups_used ? m : 0);
        std::vector<double> wresp(resp_used ? m * nscores_ : 0);
        std::vector<double> wt0(m), wout_o(m * 3), wout_t(m);
        std::vector<int32_t> wprev(m), wout_prev(m);
        for (int64_t j = 0; j < m; ++j) {
          const Item &it = items[j];
          wpos[j * 3] = it.pos.x;
          wpos[j * 3 + 1] = it.pos.y;
          wpos[j * 3 + 2] = it.pos.z;
          wdest[j * 3] = it.dest.x;
          wdest[j * 3 + 1] = it.dest.y;
          wdest[j * 3 + 2] = it.dest.z;
          welem[j] = it.lelem;
          ww[j] = it.w;
          wt0[j] = it.t0;
          wprev[j] = it.prev;
          if (groups_used) wgrp[j] = it.grp;
          if (resp_used)
            for (int k = 0; k < nscores_; ++k)
              wresp[j * nscores_ + k] = it.resp[k];
        }
        eng_->walk_raw(m, wpos.data(), wdest.data(), welem.data(), ww.data(),
                       wout_pos.data(), wout_elem.data(), wstatus.data(),
                       groups_used ? wgrp.data() : nullptr,
                       resp_used ? wresp.data() : nullptr,
                       wout_dest.data(), wt0.data(), wprev.data(),
                       wout_o.data(), wout_t.data(), wout_prev.data());
        for (int64_t j = 0; j < m; ++j) {
          const int64_t g = items[j].gid;
          if (wstatus[j] == 2) {
            const int32_t k = -(wout_elem[j] + 2);
            emit_dep(dep, g,
                     Vec3{wout_o[j * 3], wout_o[j * 3 + 1],
                          wout_o[j * 3 + 2]},
                     dec_.sub.foreign_gid[k],
                     Vec3{wout_dest[j * 3], wout_dest[j * 3 + 1],
                          wout_dest[j * 3 + 2]},
                     ww[j], wout_t[j],
                     wout_prev[j] >= 0 ? (int64_t)dec_.l2g32[wout_prev[j]]
                                       : (int64_t)-1,
                     groups_used ? wgrp[j] : (uint16_t)0,
                     resp_used ? &wresp[j * nscores_] : nullptr,
                     dec_.sub.foreign_owner[k]);
            res_[g] = 0;
          } else {
            set_pos(g, Vec3{wout_pos[j * 3], wout_pos[j * 3 + 1],
                            wout_pos[j * 3 + 2]});
            elem_[g] = wout_elem[j];
            esc_[g] = (wstatus[j] == 1) ? 1 : 0;
          }
        }
      }
      items.clear();

      // bucket by owner, exchange, unpack into next-round items
      const int64_t m = (int64_t)dep.size() / dw;
      std::vector<int64_t> scounts(world_, 0), rcounts;
      std::vector<double> send(m * rw);
      {
        std::vector<int64_t> offs(world_, 0), cur(world_, 0);
        for (int64_t i = 0; i < m; ++i) scounts[rec_.owner(&dep[i * dw])]++;
        int64_t acc = 0;
        for (int r = 0; r < world_; ++r) {
          offs[r] = acc;
          acc += scounts[r];
        }
        for (int64_t i = 0; i < m; ++i) {
          const int o = rec_.owner(&dep[i * dw]);
          const int64_t sl = offs[o] + cur[o]++;
          for (int k = 0; k < rw; ++k) send[sl * rw + k] = dep[i * dw + k];
        }
      }
      dep.clear();

      if (!exchange_counts(scounts, rcounts)) break;
      std::vector<double> recv;
      if (world_ == 1) {
        recv = std::move(send);
      } else {
        std::vector<int64_t> sc(world_);
        for (int r = 0; r < world_; ++r) sc[r] = scounts[r] * rw;
        recv = comm_->alltoallv(send.data(), sc);
      }
      const int64_t nr = (int64_t)recv.size() / rw;
      for (int64_t i = 0; i < nr; ++i) {
        const double *e = recv.data() + i * rw;
        Item it;
        it.gid = rec_.gid(e);
        it.pos = rec_.pos(e);
        it.dest = rec_.dest(e);
        it.w = rec_.weight(e);
        it.t0 = rec_.t(e);
        const int64_t pg = rec_.prev_gid(e);
        it.prev = pg >= 0 ? dec_.g2l[pg] : -1;
        it.grp = rec_.group(e);
        if (resp_used)
          it.resp.assign(rec_.responses(e), rec_.responses(e) + nscores_);
        it.lelem = dec_.g2l[rec_.target_gid(e)];
        place(it.gid, it.lelem, it.pos);
        items.push_back(std::move(it));
      }
      if (round == max_rounds()) throw_not_converged();
    }
  }

  std::vector<double> pos_;
  std::vector<int32_t> elem_;
  std::vector<uint8_t> res_, esc_;
  std::vector<int64_t> frame_;
  bool have_frame_ = false;
};

} // namespace

std::unique_ptr<PartitionedEngine>
make_cpu_partitioned_engine(const PartitionedEngineArgs &a) {
  return std::make_unique<CpuPartitionedEngine>(a);
}

} // namespace pumitally
