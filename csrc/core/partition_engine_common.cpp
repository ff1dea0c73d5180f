// Device-independent half of the stateful partitioned engine (see
// partition_engine_common.h) and the factory.
#include "partition_engine_common.h"

#include "../comm/comm.h"

#include <cstdlib>
#include <stdexcept>

namespace pumitally {

Decomp build_decomp(const Mesh &full, int rank, int world,
                    const int32_t *owners_in, int ghost_rings) {
  if (full.has_periodic() && world > 1)
    throw std::runtime_error(
        "PartitionedEngine: periodic BCs with world > 1 are unsupported in "
        "the stateful engine (a cross-rank wrap would need a translated "
        "destination, but destinations are gathered by gid from the "
        "untranslated global arrays); use the stateless "
        "pumiumtally_amd.parallel.PartitionedTally driver, which ships the "
        "translated destination in its exchange records");
  Decomp d;
  d.owners = owners_in
                 ? std::vector<int32_t>(owners_in, owners_in + full.nelems)
                 : partition_morton(full, world);
  d.sub = extract_submesh(full, d.owners, rank, ghost_rings);
  const int64_t nl = d.sub.local.nelems;
  d.l2g32.resize(nl);
  d.lowner.resize(nl);
  for (int64_t t = 0; t < nl; ++t) {
    d.l2g32[t] = (int32_t)d.sub.elem_l2g[t];
    d.lowner[t] = d.owners[d.sub.elem_l2g[t]];
  }
  d.g2l.assign(full.nelems, -1);
  for (int64_t t = 0; t < nl; ++t) d.g2l[d.sub.elem_l2g[t]] = (int32_t)t;
  return d;
}

PartitionedEngineBase::PartitionedEngineBase(const PartitionedEngineArgs &a)
    : n_(a.n), comm_(a.comm), rank_(a.rank), world_(a.world),
      ngroups_(a.ngroups < 1 ? 1 : a.ngroups),
      nscores_(a.nscores < 1 ? 1 : a.nscores),
      rec_{nscores_, ngroups_ > 1}, nelems_global_(a.full.nelems),
      dec_(build_decomp(a.full, a.rank, a.world, a.owners, a.ghost_rings)),
      loc_tol_(loc_tol_rel() * norm(a.full.bbox_hi - a.full.bbox_lo)),
      full_locate_(a.full_locate), max_rounds_(a.max_rounds) {
  if (world_ > 1 && !comm_)
    throw std::runtime_error("PartitionedEngine: world > 1 needs a comm");
}

void PartitionedEngineBase::check_n(int64_t n) const {
  if (n != n_) throw std::runtime_error("global particle count mismatch");
}

void PartitionedEngineBase::check_groups(const uint16_t *groups,
                                         int ngroups) {
  if (groups && ngroups <= 1)
    throw std::runtime_error("groups passed but ngroups == 1");
}

void PartitionedEngineBase::check_step_local(int64_t n_local,
                                             int64_t n_frame,
                                             const uint16_t *groups) const {
  if (n_frame < 0)
    throw std::runtime_error(
        "step_local: call resident_list() first (it defines the input "
        "order this call consumes)");
  if (n_local != n_frame)
    throw std::runtime_error("step_local: n_local " +
                             std::to_string(n_local) +
                             " != resident_list size " +
                             std::to_string(n_frame));
  check_groups(groups, ngroups_);
}

std::vector<double> PartitionedEngineBase::flux_global() {
  eng_->synchronize();
  const std::vector<double> local = eng_->flux(); // nscores*ngroups*nlocal
  const int64_t nl = dec_.sub.local.nelems;
  const int64_t slabs = (int64_t)nscores_ * ngroups_;
  std::vector<double> out(slabs * nelems_global_, 0.0);
  for (int64_t s = 0; s < slabs; ++s)
    for (int64_t t = 0; t < nl; ++t)
      out[s * nelems_global_ + dec_.sub.elem_l2g[t]] += local[s * nl + t];
  if (world_ > 1) comm_->allreduce_sum(out.data(), (int64_t)out.size());
  return out;
}

const EngineStats &PartitionedEngineBase::stats() const {
  stats_.lost_particles = eng_->stats().lost_particles;
  return stats_;
}

void PartitionedEngineBase::claim_state(const int32_t *gelem,
                                        std::vector<uint8_t> &res,
                                        std::vector<int32_t> &lel) const {
  res.assign(n_, 0);
  lel.assign(n_, -1);
  for (int64_t g = 0; g < n_; ++g) {
    const int32_t ge = gelem[g];
    if (ge >= 0) {
      if (dec_.owners[ge] == rank_) {
        res[g] = 1;
        lel[g] = dec_.g2l[ge];
        if (lel[g] < 0)
          throw std::runtime_error(
              "set_state: owned element missing from this submesh");
      }
    } else if (rank_ == 0) {
      res[g] = 1; // out-of-mesh particles live on rank 0
    }
  }
}

void PartitionedEngineBase::resolve_unclaimed(const double *origins,
                                              std::vector<int64_t> &words,
                                              std::vector<int32_t> &gids,
                                              std::vector<int32_t> &lels) {
  // claims are disjoint (only the owner claims), so bitwise OR of the
  // claim masks == integer sum of the words
  if (world_ > 1) comm_->allreduce_sum(words.data(), (int64_t)words.size());
  if (!full_locate_) return;
  // Unclaimed = outside the mesh OR only loosely localizable on a submesh
  // (true element absent from the ghost ring, or the point is within
  // tolerance of a cut face).
  for (int64_t g = 0; g < n_; ++g) {
    if ((words[g >> 6] >> (g & 63)) & 1) continue;
    const Vec3 q{origins[g * 3], origins[g * 3 + 1], origins[g * 3 + 2]};
    bool lo = false;
    const int32_t ge = full_locate_(q, loc_tol_, &lo);
    if (ge < 0) continue; // truly outside: rank 0 parks it
    if (lo) stats_.loose_localizations++;
    words[g >> 6] |= (int64_t)(1ull << (g & 63));
    if (dec_.owners[ge] == rank_) {
      gids.push_back((int32_t)g);
      lels.push_back(dec_.g2l[ge]);
    }
  }
}

int32_t PartitionedEngineBase::locate_full(Vec3 q) {
  bool lo = false;
  const int32_t ge = full_locate_ ? full_locate_(q, loc_tol_, &lo) : -1;
  if (lo) stats_.loose_localizations++;
  return ge;
}

bool PartitionedEngineBase::exchange_counts(
    const std::vector<int64_t> &scounts, std::vector<int64_t> &rcounts) {
  if (world_ == 1) {
    rcounts = scounts;
    return scounts[0] != 0;
  }
  std::vector<int64_t> flat((int64_t)world_ * world_, 0);
  for (int r = 0; r < world_; ++r)
    flat[(int64_t)rank_ * world_ + r] = scounts[r];
  comm_->allreduce_sum(flat.data(), (int64_t)world_ * world_);
  int64_t total = 0;
  for (int64_t c : flat) total += c;
  if (total == 0) return false;
  rcounts.resize(world_);
  for (int s = 0; s < world_; ++s)
    rcounts[s] = flat[(int64_t)s * world_ + rank_];
  return true;
}

void PartitionedEngineBase::throw_not_converged() const {
  throw std::runtime_error("partitioned step did not converge in " +
                           std::to_string(max_rounds_) + " handoff rounds");
}

std::unique_ptr<PartitionedEngine> make_partitioned_engine(
    const Mesh &full, int64_t n_global, Comm *comm, int rank, int world,
    const std::string &device, int ngroups, int nscores,
    const int32_t *owners, int ghost_rings) {
  // the rare global-resolve path keeps a host copy of the full mesh
  auto full_copy = std::make_shared<Mesh>(full);
  const PartitionedEngineArgs args{
      full, n_global, comm, rank, world, ngroups, nscores, owners,
      ghost_rings, [full_copy](Vec3 q, double tol, bool *lo) {
        return full_copy->locate(q, tol, lo);
      }};
  if (device != "cpu") {
    int ordinal = 0;
    if (device.rfind("cuda:", 0) == 0) ordinal = atoi(device.c_str() + 5);
    else if (!device.empty() && device != "auto") ordinal = atoi(device.c_str());
    if (auto e = make_gpu_partitioned_engine(args, ordinal)) return e;
    if (device != "auto")
      throw std::runtime_error("PartitionedEngine: HIP device unavailable");
  }
  return make_cpu_partitioned_engine(args);
}

} // namespace pumitally
