// Tally engine interface: the device-agnostic contract behind the public
// PumiTally API.  Two implementations:
//   * CpuEngine  (engine_cpu.cpp)  - serial oracle, runs everywhere
//   * GpuEngine  (../hip/engine_gpu.hip) - MI355X HIP engine
//
// Semantics mirror the reference's 4-call flow
// (/root/reference/src/pumitally/PumiTally.h:50-103):
//   ctor                 -> all particles at the centroid of element 0
//                           (PumiTallyImpl.cpp:492-528)
//   copy_initial_position-> localize each particle at its given position;
//                           no tallying (PumiTallyImpl.cpp:54-64,195-221)
//   move                 -> phase A: relocate flying particles to the given
//                           origin WITHOUT tallying; phase B: walk them to
//                           the destination, tallying track_length*weight
//                           per element crossed (PumiTallyImpl.cpp:66-149)
//   write_tally_results  -> normalize flux by element volume, write VTK
//                           (PumiTallyImpl.cpp:151-157,382-416)
//
// Behavioral pins taken from the reference tests
// (test/test_pumi_tally_impl_methods.cpp):
//   * a particle that exited through the vacuum boundary keeps its clipped
//     position and element id; phase A does NOT relocate it (the 2nd-move
//     flux expectations at :361-389 are only satisfiable this way)
//   * non-flying particles do not move and do not tally
//   * flux accumulates across move calls until write
//
// Design deviation (MI355X-first): phase A is a direct grid localization of
// the particles whose origin actually changed, not a zero-weight walk
// through the mesh as in the reference -- same observable state, a fraction
// of the work.
#pragma once

#include "mesh.h"
#include "walk.h"

#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <memory>
#include <string>
#include <vector>

namespace pumitally {

struct EngineStats {
  int64_t lost_particles = 0;   // walks that hit max_steps
  int64_t moves = 0;            // move() calls
  int64_t relocated = 0;        // phase-A relocations performed
  // Localizations that only succeeded at the loosened tolerance (tol*1e4
  // retry in grid_locate / Mesh::locate).  A nonzero count near partition
  // cuts can mean mis-assigned particles; surfaced so it is never silent.
  int64_t loose_localizations = 0;
  // Origin elision (GPU engine, Engine::origin_elide): particles whose
  // origin was taken from the previous move's destinations already in
  // device memory instead of being uploaded, and the origin bytes that did
  // cross the link (24 per uploaded particle).  Cumulative; the CPU engine
  // stages nothing and reports 0 for both.
  int64_t origins_elided = 0;
  int64_t origin_bytes_uploaded = 0;
  // Host time spent in the elision compare pass (seeding copies included),
  // cumulative seconds: what the feature costs the calling thread.
  double origin_pass_seconds = 0.0;
  // Collision-estimator tallies (Engine::score_collisions / score_points):
  // particles or points that scored, and those that did not because they
  // are not in the mesh (unlocated or escaped).  Cumulative.
  int64_t collisions_scored = 0;
  int64_t collision_misses = 0;
  // Stateless track tallies (Engine::tally_tracks): tracks handed over (the
  // sum of n over calls), times a track entered the mesh from outside
  // through a boundary face (a start inside the mesh is not an entry), and
  // tallied tracks that were never inside the mesh.  Cumulative.
  int64_t tracks = 0;
  int64_t track_entries = 0;
  int64_t track_misses = 0;
};

// First-K lost-particle capture (walks that hit max_steps): enough to find
// and reproduce the offending histories the day a real mesh produces a
// nonzero lost count, without any steady-state cost.
constexpr int kMaxLostRecords = 16;

class Engine {
public:
  virtual ~Engine() = default;

  virtual int64_t num_particles() const = 0;
  virtual const Mesh &mesh() const = 0;

  // positions: n*3 doubles (x,y,z interleaved).
  virtual void copy_initial_position(const double *positions, int64_t n) = 0;

  // origin/dest: n*3 doubles; flying: n int8; weights: n doubles.
  // groups (optional, nullable): per-particle energy-group index in
  // [0, ngroups); contributions land in flux[group*nelems + elem].  The
  // reference has a single scalar tally; ngroups=1 (the default) matches
  // it exactly.
  // responses (optional, nullable): n*nscores per-particle response
  // multipliers for simultaneous tally SCORES (e.g. flux + heating +
  // fission from one walk).  With responses given, score k of a crossing
  // tallies seg * weight * responses[i*nscores+k] into
  // flux[(k*ngroups + group)*nelems + elem].  With responses == nullptr
  // only score 0 is tallied (plain seg * weight); scores 1..nscores-1
  // stay zero (see test_scored_null_responses_is_plain_flux).  nscores=1
  // with null responses (the default) is exactly the reference's single
  // tally.
  virtual void move(const double *origin, const double *dest,
                    const int8_t *flying, const double *weights, int64_t n,
                    const uint16_t *groups = nullptr,
                    const double *responses = nullptr) = 0;

  // Fast path for callers that know no particle was resampled this step
  // (origin == committed position for every particle): skips the origin
  // upload and phase A entirely.  origin=nullptr in move() semantics.
  virtual void move_continue(const double *dest, const int8_t *flying,
                             const double *weights, int64_t n,
                             const uint16_t *groups = nullptr,
                             const double *responses = nullptr) {
    move(nullptr, dest, flying, weights, n, groups, responses);
  }

  // Device-resident move: all arrays already live in this engine's device
  // memory (for GPU-side transport codes; no host staging at all).
  // origin may be nullptr (continue semantics).  Throws on the CPU engine.
  virtual void move_device(const double *d_origin, const double *d_dest,
                           const int8_t *d_flying, const double *d_weights,
                           int64_t n, const uint16_t *d_groups = nullptr,
                           const double *d_responses = nullptr) {
    (void)d_origin; (void)d_dest; (void)d_flying; (void)d_weights; (void)n;
    (void)d_groups; (void)d_responses;
    throw std::runtime_error("move_device requires the GPU engine");
  }

  // Raw batched walk for the partitioned driver: walks n independent
  // segments (pos->dest) starting in the given elements, tallying into
  // this engine's flux.  status: 0=reached dest, 1=escaped (vacuum),
  // 2=handoff (out_elem = encoded foreign ref -(2+k)), 3=lost.
  // groups (nullable): per-segment energy-group index, same semantics as
  // move(); a handed-off particle keeps its group (the partitioned driver
  // carries it in the exchange record).  responses (nullable): n*nscores
  // per-segment score multipliers, same semantics as move().
  // Synchronous; host memory.
  // out_dest (optional, n*3): the walk's CURRENT destination at
  // termination -- reflective restarts mirror it, periodic restarts
  // translate it, so a handoff (status 2) must resume toward out_dest,
  // not the original dest.
  // Bitwise-exact handoff resume (walk.h walk_segment doc): in_t/in_prev
  // (optional, n) seed the walk's segment progress and entry-exclusion
  // element for resumed particles; out_o (n*3) / out_t (n) / out_prev
  // (n) export the wrap-segment origin, the progress t at termination,
  // and the element a handoff exited from.  A handoff record carrying
  // (out_o, out_dest, out_t, out_prev) lets the receiving rank replay
  // the remaining crossings with fp decisions identical to an uncut
  // walk, so partitioned flux attribution matches the replicated
  // engine elementwise.
  virtual void walk_raw(int64_t n, const double *pos, const double *dest,
                        const int32_t *elem, const double *weights,
                        double *out_pos, int32_t *out_elem,
                        int8_t *out_status,
                        const uint16_t *groups = nullptr,
                        const double *responses = nullptr,
                        double *out_dest = nullptr,
                        const double *in_t = nullptr,
                        const int32_t *in_prev = nullptr,
                        double *out_o = nullptr, double *out_t = nullptr,
                        int32_t *out_prev = nullptr) = 0;

  // Device-resident walk_raw: every array already lives in this engine's
  // device memory (no staging at all -- the partitioned driver keeps its
  // round loop on device and exchanges records over RCCL directly).
  // Synchronous like walk_raw.  Throws on the CPU engine.
  virtual void walk_raw_device(int64_t n, const double *d_pos,
                               const double *d_dest, const int32_t *d_elem,
                               const double *d_weights, double *d_out_pos,
                               int32_t *d_out_elem, int8_t *d_out_status,
                               const uint16_t *d_groups = nullptr,
                               const double *d_responses = nullptr,
                               double *d_out_dest = nullptr,
                               const double *d_in_t = nullptr,
                               const int32_t *d_in_prev = nullptr,
                               double *d_out_o = nullptr,
                               double *d_out_t = nullptr,
                               int32_t *d_out_prev = nullptr) {
    (void)n; (void)d_pos; (void)d_dest; (void)d_elem; (void)d_weights;
    (void)d_out_pos; (void)d_out_elem; (void)d_out_status; (void)d_groups;
    (void)d_responses; (void)d_out_dest; (void)d_in_t; (void)d_in_prev;
    (void)d_out_o; (void)d_out_t; (void)d_out_prev;
    throw std::runtime_error("walk_raw_device requires the GPU engine");
  }

  // Stateless track tallies: n free segments origin -> dest with weights
  // (any n, independent of num_particles; n == 0 is a no-op) that may start
  // or end anywhere, pass through the mesh from outside, leave through a
  // hole and come back, or miss it (track.h has the rules of one track).
  // Each track is independent; the call never reads or writes particle
  // state (positions, elements, escaped flags, the origin-elision cache).
  // Contributions go where move()'s go: the flux, on linear engines the
  // moments too, on currents engines the currents too (no re-exit rule, as
  // in walk_raw); groups and responses as in move().  The collision tally is
  // not touched.  A zero-length or zero-weight track is skipped before any
  // geometry.  Counted in EngineStats::tracks / track_entries /
  // track_misses; a track that runs out of steps or entries counts into
  // lost_particles, its lost_records row carrying the track index.
  // Synchronous; host memory.  Throws std::invalid_argument on a mesh with
  // partition-cut faces (nbr < -1).
  virtual void tally_tracks(int64_t n, const double *origin,
                            const double *dest, const double *weights,
                            const uint16_t *groups = nullptr,
                            const double *responses = nullptr) = 0;
  // Device-resident twin: every array already lives in this engine's device
  // memory; queued on the engine's compute stream, nothing is staged.
  // Throws on the CPU engine.
  virtual void tally_tracks_device(int64_t n, const double *d_origin,
                                   const double *d_dest,
                                   const double *d_weights,
                                   const uint16_t *d_groups = nullptr,
                                   const double *d_responses = nullptr) {
    (void)n; (void)d_origin; (void)d_dest; (void)d_weights; (void)d_groups;
    (void)d_responses;
    throw std::runtime_error("tally_tracks_device requires the GPU engine");
  }

  // Read back state (host copies).
  virtual std::vector<double> flux() const = 0;           // nelems*ngroups*nscores, raw tally
  virtual std::vector<int32_t> elem_ids() const = 0;      // n
  virtual std::vector<double> positions() const = 0;      // n*3
  virtual std::vector<uint8_t> escaped() const = 0;       // n

  virtual const EngineStats &stats() const = 0;

  // First min(lost_particles, kMaxLostRecords) lost-walk records, 4 doubles
  // each: (caller particle index -- or segment index for walk_raw --,
  // drop x, drop y, drop z).  Empty when nothing was lost.
  virtual std::vector<double> lost_records() const { return {}; }

  // Batch statistics (standard MC uncertainty accounting; the reference
  // has a single accumulating tally with no variance).  end_batch()
  // accumulates the current flux into running sum / sum-of-squares and
  // zeroes the per-batch tally; batch_sum/batch_sum_sq read the
  // accumulators (size nelems*ngroups); num_batches counts end_batch calls.
  virtual void end_batch() = 0;
  virtual std::vector<double> batch_sum() const = 0;
  virtual std::vector<double> batch_sum_sq() const = 0;
  virtual int64_t num_batches() const = 0;

  // Overwrite the flux tally (used by the distributed driver to install the
  // all-reduced global tally on rank 0 before writing).
  virtual void set_flux(const double *flux, int64_t nelems) = 0;

  // Linear (per-vertex) track-length moments -- only on engines created
  // with linear=true; every call below throws otherwise.  For each tallied
  // crossing the walk adds, next to the flux contribution, the 4 first
  // barycentric moments  m_f = integral of weight * lambda_f dl  over the
  // chord (walk.h tet_moments), with groups and scores applied exactly as
  // for flux.  Layout: [nscores x ngroups x nelems x 4], local vertex
  // fastest (a crossing's four adds are one 32-byte span).  sum_f m_f equals
  // the flux entry up to rounding.  The flux tally itself is produced
  // exactly as without linear mode.
  // end_batch() adds the per-batch moments into a running sum
  // (moment_sum) and zeroes them.  Moments get NO sum of squares: their
  // consumers reconstruct a field from the batch-summed moments, and a
  // variance of the derived nodal values is not a per-entry quantity.
  virtual std::vector<double> moments() const { throw_not_linear(); }
  virtual std::vector<double> moment_sum() const { throw_not_linear(); }
  // Overwrite the per-batch moments (checkpoint restore); n must be the
  // full moments size.
  virtual void set_moments(const double *m, int64_t n) {
    (void)m; (void)n;
    throw_not_linear();
  }

  // Face-current tallies -- only on engines created with currents=true;
  // every call below throws otherwise.  For every tallied crossing where the
  // walk leaves element e through local face f (the face opposite local
  // vertex f; flat face index e*4+f as in the boundary-face tables) the
  // particle's weight is added to J[e, f]: the outward partial current J+
  // integrated over the face.  No track length and no cosine enter.  Groups
  // and scores apply exactly as for flux (group offset, weight *
  // responses[i,k] per score; null responses: score 0 only).  Layout:
  // [nscores x ngroups x nelems x 4], local face fastest, index = (flux
  // index)*4 + f.  A crossing is every exit-face selection of walk_advance
  // with t_exit < 1 on a tallied walk (neighbor step, vacuum clip, handoff,
  // reflective or periodic restart, zero-length slivers included); the
  // final partial segment, untallied walks and phase-A relocation count
  // nothing.  The flux tally itself is produced exactly as without the
  // option.  end_batch() adds the per-batch currents into current_sum and
  // their squares into current_sum_sq (a per-entry variance is meaningful
  // here, unlike for the moments) and zeroes them.
  virtual std::vector<double> currents() const { throw_not_currents(); }
  virtual std::vector<double> current_sum() const { throw_not_currents(); }
  virtual std::vector<double> current_sum_sq() const { throw_not_currents(); }
  // Overwrite the per-batch currents (checkpoint restore); n must be the
  // full currents size.
  virtual void set_currents(const double *j, int64_t n) {
    (void)j; (void)n;
    throw_not_currents();
  }

  // Collision-estimator tallies -- only on engines created with
  // collisions=true; every call below throws otherwise.  A second tally
  // array laid out exactly like flux ([nscores x ngroups x nelems], flat
  // index (k*ngroups + g)*nelems + e), filled ONLY by the explicit scoring
  // calls below, never by move(): a point estimator (w/Sigma_t at each
  // collision, scattering into a group, analog counts ...) needs no track
  // and no geometry, just the element the engine already holds.  The scoring
  // calls never modify `active`, particle state (position, element, escaped),
  // flux, moments or currents; move() never touches the collisions.
  // Combines freely with linear and with currents.
  //
  // score_collisions (n == num_particles): every particle i with
  // active[i] != 0 whose held element e is >= 0 and which is not flagged
  // escaped SCORES: with responses given, weights[i] * responses[i*nscores+k]
  // is added to score k for every k; with responses == nullptr, weights[i]
  // to score 0 only (move()'s rule); in group groups[i] % ngroups (group 0
  // without groups), at element e.  Any other active particle is unlocated
  // or escaped -- it sits on the vacuum face it left through, no longer in
  // the mesh -- adds nothing and counts as a MISS.  A particle whose last
  // walk was lost (hit max_steps) scores in the element the engine kept for
  // it, the one the walk started from.
  //
  // score_points: n free points (any n, independent of num_particles;
  // n == 0 is a no-op), xyz n*3 doubles.  Each is localized with the
  // engine's grid and localization tolerance -- grid_locate on the device,
  // Mesh::locate on the CPU, the calls and first-hit rule of
  // copy_initial_position -- and a located point scores as above (its own
  // weights / groups / responses row); a point outside the mesh is a miss.
  // Loose hits count into loose_localizations.  Synchronous.
  //
  // EngineStats::collisions_scored / collision_misses count both calls.
  // end_batch() adds the per-batch collisions into collision_sum and their
  // squares into collision_sum_sq (a per-entry variance is meaningful, as for
  // the currents) and zeroes them.
  virtual void score_collisions(const int8_t *active, const double *weights,
                                int64_t n, const uint16_t *groups = nullptr,
                                const double *responses = nullptr) {
    (void)active; (void)weights; (void)n; (void)groups; (void)responses;
    throw_not_collisions();
  }
  virtual void score_points(int64_t n, const double *xyz,
                            const double *weights,
                            const uint16_t *groups = nullptr,
                            const double *responses = nullptr) {
    (void)n; (void)xyz; (void)weights; (void)groups; (void)responses;
    throw_not_collisions();
  }
  // Device-resident twins, move_device's contract: every array already
  // lives in this engine's device memory, nothing is staged, the kernel runs
  // on the engine's compute stream.  Throw on the CPU engine.
  virtual void score_collisions_device(const int8_t *d_active,
                                       const double *d_weights, int64_t n,
                                       const uint16_t *d_groups = nullptr,
                                       const double *d_responses = nullptr) {
    (void)d_active; (void)d_weights; (void)n; (void)d_groups;
    (void)d_responses;
    if (!collision_tallies) throw_not_collisions();
    throw std::runtime_error("score_collisions_device requires the GPU engine");
  }
  virtual void score_points_device(int64_t n, const double *d_xyz,
                                   const double *d_weights,
                                   const uint16_t *d_groups = nullptr,
                                   const double *d_responses = nullptr) {
    (void)n; (void)d_xyz; (void)d_weights; (void)d_groups; (void)d_responses;
    if (!collision_tallies) throw_not_collisions();
    throw std::runtime_error("score_points_device requires the GPU engine");
  }
  virtual std::vector<double> collisions() const { throw_not_collisions(); }
  virtual std::vector<double> collision_sum() const { throw_not_collisions(); }
  virtual std::vector<double> collision_sum_sq() const {
    throw_not_collisions();
  }
  // Overwrite the per-batch collisions (checkpoint restore); n must be the
  // full flux size.
  virtual void set_collisions(const double *c, int64_t n) {
    (void)c; (void)n;
    throw_not_collisions();
  }

  // Restore particle state (checkpoint/resume support -- the reference has
  // none; a crash there loses the whole batch).
  virtual void set_particle_state(const double *pos, const int32_t *elem,
                                  const uint8_t *escaped, int64_t n) = 0;

  // Block until all queued device work is done (no-op on CPU).
  virtual void synchronize() {}

  // Device-resident mesh views (GPU engines only): lets sibling device
  // code (the partitioned engine's localization kernels) reuse the
  // engine's uploaded planes/grid instead of duplicating them in HBM.
  struct DeviceMeshView {
    const Plane *planes = nullptr; // nelems*4
    const int32_t *nbr = nullptr;  // nelems*4
    GridView grid{};
    // the engine's compute stream (hipStream_t; void* keeps this header
    // HIP-free): sibling kernels launched here order naturally against
    // walk_raw_device without device-wide fences
    void *stream = nullptr;
  };
  virtual bool device_mesh(DeviceMeshView *out) const {
    (void)out;
    return false;
  }

  int max_steps = 0; // 0 = auto (set by implementations from mesh size)
  int ngroups = 1;   // energy groups
  int nscores = 1;   // tally scores (flux is [nscores x ngroups x nelems])

  bool reflective = false; // specular-reflect at boundaries (else vacuum)

  // Linear moment tallies enabled (see moments()).  Fixed at construction
  // (make_*_engine's trailing argument); read-only afterwards.
  bool linear = false;

  // Face-current tallies enabled (see currents()).  Fixed at construction
  // (make_*_engine's trailing argument); read-only afterwards.  Cannot be
  // combined with linear.  (Named face_currents because currents() is the
  // accessor.)
  bool face_currents = false;

  // Collision-estimator tallies enabled (see score_collisions()).  Fixed at
  // construction (make_*_engine's trailing argument); read-only afterwards.
  // (Named collision_tallies because collisions() is the accessor.)
  bool collision_tallies = false;

  // fp32-traversal fast path (walk.h walk_advance32): candidate exit-face
  // decisions in fp32, crossings/tallies in fp64.  Controlled by
  // PUMITALLY_WALK=fp32|fp64; both engines honor it so CPU remains the
  // bitwise oracle for the GPU in either mode.
  bool walk_fp32 = false;

  // Origin elision (GPU engine's move(); see engine_gpu.hip): skip the
  // upload of every origin that is bit-identical to the destination the
  // previous move() staged, rebuilding it on device instead.  Results are
  // unchanged; origin_elide=false restores the plain full upload.
  // Env defaults: PUMITALLY_ORIGIN_ELIDE (0|1), PUMITALLY_ORIGIN_THREADS
  // (host compare workers, capped at 16), PUMITALLY_ORIGIN_CHUNK (particles
  // per host chunk; 0 = auto).  Per engine, so two engines in one process
  // can differ.  The CPU engine ignores all three.
  bool origin_elide = true;
  int origin_threads = 8;
  int64_t origin_chunk = 0;

protected:
  [[noreturn]] static void throw_not_linear() {
    throw std::runtime_error(
        "linear moment tallies are off: create the engine with linear=true");
  }
  [[noreturn]] static void throw_not_currents() {
    throw std::runtime_error(
        "face-current tallies are off: create the engine with currents=true");
  }
  [[noreturn]] static void throw_not_collisions() {
    throw std::runtime_error(
        "collision tallies are off: create the engine with collisions=true");
  }
};

inline bool default_walk_fp32() {
  const char *s = getenv("PUMITALLY_WALK");
  return s && std::string(s) == "fp32";
}

inline bool default_origin_elide() {
  const char *s = getenv("PUMITALLY_ORIGIN_ELIDE");
  return !s || atoi(s) != 0;
}

inline int default_origin_threads() {
  const char *s = getenv("PUMITALLY_ORIGIN_THREADS");
  const int k = s ? atoi(s) : 8;
  return k < 1 ? 1 : (k > 16 ? 16 : k);
}

inline int64_t default_origin_chunk() {
  const char *s = getenv("PUMITALLY_ORIGIN_CHUNK");
  const int64_t c = s ? (int64_t)atoll(s) : 0;
  return c < 0 ? 0 : c;
}

// Localization tolerance (accepted signed distance below a face plane),
// relative to the mesh bounding-box diagonal.  The reference hardcodes its
// geometric tolerance (1e-8 at PumiTallyImpl.cpp:51); here it is runtime
// configurable (SURVEY.md section 5 flags the hardcoding).
// Boundary condition: vacuum (reference parity, default) or specular
// reflective on every boundary face (symmetry-plane models).  Env:
// PUMITALLY_BC=vacuum|reflective.
inline bool default_reflective() {
  const char *s = getenv("PUMITALLY_BC");
  return s && std::string(s) == "reflective";
}

inline double loc_tol_rel() {
  const char *s = getenv("PUMITALLY_LOC_TOL");
  return s ? atof(s) : 1e-10;
}

std::unique_ptr<Engine> make_cpu_engine(Mesh mesh, int64_t num_particles,
                                        int ngroups = 1, int nscores = 1,
                                        bool linear = false,
                                        bool currents = false,
                                        bool collisions = false);

// Returns nullptr when no HIP device is available.
std::unique_ptr<Engine> make_gpu_engine(Mesh mesh, int64_t num_particles,
                                        int device, int ngroups = 1,
                                        int nscores = 1, bool linear = false,
                                        bool currents = false,
                                        bool collisions = false);

// make_*_engine reject the one unsupported option pair up front.
inline void check_tally_options(bool linear, bool currents) {
  if (linear && currents)
    throw std::invalid_argument(
        "currents=true cannot be combined with linear=true (not implemented)");
}

// Normalized flux = flux / element volume (volume-only, matching the
// reference implementation rather than its docstring:
// PumiTallyImpl.cpp:382-409, TODO at :372 never implemented).
std::vector<double> normalize_flux(const Mesh &m, const std::vector<double> &flux);

void write_tally_vtk(const std::string &filename, const Mesh &m,
                     const std::vector<double> &flux);

int default_max_steps(const Mesh &m);

} // namespace pumitally
