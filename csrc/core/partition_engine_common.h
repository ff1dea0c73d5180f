// What the CPU and GPU stateful partitioned engines share: the host-side
// decomposition tables and every piece of a step that has nothing
// device-specific in it (internal header; the public surface is
// partition_engine.h).
#pragma once

#include "engine.h"
#include "partition_engine.h"
#include "partition_record.h"

#include <functional>
#include <memory>
#include <string>
#include <vector>

namespace pumitally {

struct Decomp {
  SubMesh sub;
  std::vector<int32_t> owners; // global elem -> rank
  std::vector<int32_t> l2g32;  // local elem -> global (int32)
  std::vector<int32_t> lowner; // local elem -> owner rank
  std::vector<int32_t> g2l;    // global elem -> local (-1 if absent)
};

Decomp build_decomp(const Mesh &full, int rank, int world,
                    const int32_t *owners_in, int ghost_rings);

// Locate over the FULL mesh on the host: (point, tol, &loose) -> global
// element or -1.
using FullLocate = std::function<int32_t(Vec3, double, bool *)>;

// Everything a partitioned engine needs apart from its device.
struct PartitionedEngineArgs {
  const Mesh &full;
  int64_t n;
  Comm *comm;
  int rank, world;
  int ngroups, nscores;
  const int32_t *owners;
  int ghost_rings;
  FullLocate full_locate;
  int max_rounds = 64; // handoff rounds before a step is declared stuck
};

class PartitionedEngineBase : public PartitionedEngine {
public:
  int rank() const override { return rank_; }
  int world() const override { return world_; }
  int64_t num_particles() const override { return n_; }
  std::vector<double> flux_global() override;
  const EngineStats &stats() const override;
  void synchronize() override { eng_->synchronize(); }

protected:
  explicit PartitionedEngineBase(const PartitionedEngineArgs &a);

  void check_n(int64_t n) const;
  static void check_groups(const uint16_t *groups, int ngroups);
  // step_local preconditions; n_frame < 0 means no snapshot was taken
  void check_step_local(int64_t n_local, int64_t n_frame,
                        const uint16_t *groups) const;

  // set_state: which particles this rank claims under ITS decomposition
  // (res) and their local element (lel, -1 for out-of-mesh)
  void claim_state(const int32_t *gelem, std::vector<uint8_t> &res,
                   std::vector<int32_t> &lel) const;

  // Host half of localize().  words: this rank's strict-hit claim mask, one
  // bit per gid.  Sums it over ranks, then resolves every unclaimed gid on
  // the full mesh -- every rank computes the same answer, so the owner
  // claims without extra communication and the element matches the
  // replicated oracle's bitwise.  Appends what THIS rank claims to
  // gids/lels; on return a clear bit means "outside the mesh".
  void resolve_unclaimed(const double *origins, std::vector<int64_t> &words,
                         std::vector<int32_t> &gids,
                         std::vector<int32_t> &lels);

  // Full-mesh locate of a resampled origin that missed the local submesh;
  // counts loose hits.  -1: outside the mesh.
  int32_t locate_full(Vec3 q);

  // One exchange round's count bookkeeping.  scounts[r] = records this rank
  // sends to r.  Returns false when no rank has anything left to send (the
  // step is over); otherwise rcounts[s] = records arriving from s.  World 1
  // exchanges with itself.
  bool exchange_counts(const std::vector<int64_t> &scounts,
                       std::vector<int64_t> &rcounts);

  int max_rounds() const { return max_rounds_; }
  [[noreturn]] void throw_not_converged() const;

  const int64_t n_;
  Comm *const comm_;
  const int rank_, world_;
  const int ngroups_, nscores_;
  const HandoffLayout rec_;
  const int64_t nelems_global_;
  const Decomp dec_;
  const double loc_tol_;
  std::unique_ptr<Engine> eng_; // the derived class creates it
  mutable EngineStats stats_;

private:
  FullLocate full_locate_;
  int max_rounds_;
};

// Returns nullptr when no HIP device `ordinal` is available.
std::unique_ptr<PartitionedEngine>
make_gpu_partitioned_engine(const PartitionedEngineArgs &a, int ordinal);

std::unique_ptr<PartitionedEngine>
make_cpu_partitioned_engine(const PartitionedEngineArgs &a);

} // namespace pumitally
