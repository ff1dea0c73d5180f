// Stateful domain-decomposed tally engine (native C++/HIP/RCCL).
//
// Round-1's partitioned mode (pumiumtally_amd/parallel/partition.py)
// was stateless: every step re-localized and re-uploaded the whole
// global batch from the host, landing 27x off the replicated engine's
// step time.  This engine keeps particles RESIDENT on their owner rank
// between steps -- the design the reference gets from pumipic's
// migrate-inside-search (/root/reference/src/pumitally/
// PumiTallyImpl.cpp:111-145,433-459), rebuilt MI355X-first:
//
//   * State is indexed by GLOBAL particle id in per-rank device arrays
//     (committed position, local element, resident/escaped masks) --
//     ~30 B per global particle per rank, trivial against 288 GB HBM3E,
//     and it makes arrival/departure a mask flip instead of a
//     compaction problem.
//   * One step uploads only the step inputs (dest/flying/weights, plus
//     origin when resampling happened); walk lists are compacted on
//     device; the walk itself is the same fused k_walk kernel as the
//     replicated engine (walk_raw_device).
//   * Cut-crossing particles ship as handoff records (layout:
//     partition_record.h) over Comm::alltoallv_device (RCCL grouped
//     send/recv pairs over xGMI).
//   * Resampled particles (origin != committed) relocate via the LOCAL
//     submesh grid first (covers the owned region + ghost ring); only
//     the rare local-miss falls back to a host-side global locate.
//
// Semantics match Engine::move() (engine.h): non-flying particles do
// not move; escaped particles keep their clipped position/element and
// phase A does not relocate them; particles outside the mesh tally
// nothing and remember their requested position.
#pragma once

#include "engine.h"
#include "mesh.h"

#include <cstdint>
#include <memory>
#include <vector>

namespace pumitally {

class Comm;

class PartitionedEngine {
public:
  virtual ~PartitionedEngine() = default;

  virtual int rank() const = 0;
  virtual int world() const = 0;
  virtual int64_t num_particles() const = 0; // global batch size

  // One-time (or per-resample-wave) localization of the global batch:
  // every rank passes the SAME global origins array; each rank claims
  // the particles whose position lies in its owned elements.
  virtual void localize(const double *origins, int64_t n_global) = 0;

  // One transport step over the global batch.  Every rank passes the
  // same global arrays.  origin == nullptr means no particle was
  // resampled (continue from committed positions).  groups optional
  // (requires ngroups > 1 at construction); responses optional
  // (n_global * nscores score multipliers, engine.h semantics).
  virtual void step(const double *dest, const int8_t *flying,
                    const double *weights, int64_t n_global,
                    const double *origin = nullptr,
                    const uint16_t *groups = nullptr,
                    const double *responses = nullptr) = 0;

  // ------ coupled-host path (rank-parallel transport codes) ---------
  // When the host app is decomposed the same way (the config-5 multi-
  // GPU coupling), it produces step inputs only for the particles IT
  // owns.  resident_list() snapshots this rank's resident particles and
  // returns their global ids; the NEXT step_local call passes arrays in
  // exactly that order (n_local entries).  Unlike step(), nothing
  // global-sized crosses PCIe, so the upload cost scales with the local
  // batch -- the weak-scaling-correct form.  Handoff records carry
  // weight/group/responses along with the destination (the receiver
  // cannot gather them from arrays it never saw).
  virtual std::vector<int64_t> resident_list() = 0;
  virtual void step_local(const double *dest, const int8_t *flying,
                          const double *weights, int64_t n_local,
                          const double *origin = nullptr,
                          const uint16_t *groups = nullptr,
                          const double *responses = nullptr) = 0;

  // Local tally scattered to global element ids and summed over ranks
  // (nscores * ngroups * nelems doubles).
  virtual std::vector<double> flux_global() = 0;

  // Residency / diagnostics.
  virtual int64_t resident() const = 0;     // particles on this rank
  virtual const EngineStats &stats() const = 0;
  virtual void synchronize() = 0;

  // Per-particle readback (global index space; only entries resident on
  // this rank are meaningful -- use resident_mask to select).
  virtual std::vector<uint8_t> resident_mask() const = 0;
  virtual std::vector<double> positions() const = 0;  // n_global*3
  virtual std::vector<int32_t> elem_ids() const = 0;  // LOCAL elem ids

  // Decomposition-independent state transfer (checkpoint/resume and
  // dynamic repartitioning).  elem_ids_global() maps this rank's
  // resident entries to GLOBAL element ids (-1 for out-of-mesh).
  // set_state() installs a full global snapshot: every rank passes the
  // SAME arrays and claims the particles whose element it owns under
  // THIS engine's decomposition (out-of-mesh particles go to rank 0),
  // so a snapshot taken under one decomposition restores under any
  // other -- repartitioning is "build a new engine with new owners,
  // set_state(old snapshot)".  The flux tally is NOT transferred: drain
  // it with flux_global() first and sum host-side.
  virtual std::vector<int32_t> elem_ids_global() const = 0;
  virtual std::vector<uint8_t> escaped_mask() const = 0;
  virtual void set_state(const double *pos, const int32_t *gelem,
                         const uint8_t *escaped, int64_t n_global) = 0;
};

// comm may be null only when world == 1.  device: "cpu" or a HIP
// ordinal.  owners: optional explicit element->rank map (size nelems);
// default Morton partition into `world` parts.  ghost_rings as in
// extract_submesh.
std::unique_ptr<PartitionedEngine> make_partitioned_engine(
    const Mesh &full, int64_t n_global, Comm *comm, int rank, int world,
    const std::string &device, int ngroups = 1, int nscores = 1,
    const int32_t *owners = nullptr, int ghost_rings = 1);

} // namespace pumitally
