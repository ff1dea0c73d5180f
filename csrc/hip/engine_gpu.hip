// MI355X (gfx950) tally engine.
//
// Design (MI355X-first, not a port of the reference's Kokkos structure):
//   * The whole per-step pipeline of the reference -- H2D staging (M1-M3),
//     buffer->particle copies (K1-K4), the external ParticleTracer search
//     loop and the per-boundary handler kernels (K5-K9)
//     (/root/reference/src/pumitally/PumiTallyImpl.cpp:66-149,243-380) --
//     collapses into ONE fused kernel (k_move) that walks each particle's
//     whole segment in registers and atomicAdds per-element contributions.
//   * Mesh data is flat HBM arrays consumed by the walk: 4 face planes
//     (double4, inward-positive unit normals) + 4 neighbor ids per tet --
//     144 B/tet, contiguous, no indirection to vertex coords in the hot
//     loop.  A 1M-tet mesh (~150 MB) is resident in the 256 MiB
//     Infinity Cache.
//   * Particle state lives in SPATIAL (Morton) order: a device radix sort
//     (hipCUB) orders particle slots by position at localization and
//     periodically thereafter, so neighboring lanes walk neighboring
//     tets and each XCD's private L2 sees one compact mesh region
//     (measured 2.2x on the walk).  A slot->caller index map keeps the
//     public API's particle indices unchanged; the caller's arrays are
//     gathered through it on device.
//   * Host input staging is parity double-buffered: step k+1's H2D
//     copies (origin/dest/flying/weights, plus groups/responses when
//     used; on the copy stream) overlap step k's walk kernels (on the
//     compute stream); buffer reuse is fenced with per-parity events.
//     Pinned sources (pumiumtally_amd.pinned_array or app-registered
//     buffers) run at full link rate.
//   * That link is what bounds the host-staged step, so move() does not
//     send what the device already has: origins that are bit for bit the
//     previous move's destinations are rebuilt from the copy still in HBM
//     (origin elision, see stage_elided below) -- 42 % fewer bytes per
//     steady-state step, results unchanged.
#include "../core/engine.h"
#include "../core/origin_delta.h"
#include "../core/tally_sink.h"
#include "../core/track.h"
#include "../core/walk.h"
#include "hip_util.h"

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <type_traits>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace pumitally {

namespace {

// Block size for all particle kernels; swept via PUMITALLY_BLOCK.
inline int block_size() {
  static int v = [] {
    const char *s = getenv("PUMITALLY_BLOCK");
    int k = s ? atoi(s) : 256;
    if (k < 64) k = 64;
    if (k > 1024) k = 1024;
    return (k / 64) * 64; // multiple of the 64-wide wavefront
  }();
  return v;
}
#define kBlock block_size()

__global__ void k_init_particles(double *__restrict__ pos,
                                 int32_t *__restrict__ elem,
                                 uint8_t *__restrict__ escaped,
                                 int32_t *__restrict__ s2c, int64_t n,
                                 double cx, double cy, double cz) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    pos[i * 3] = cx;
    pos[i * 3 + 1] = cy;
    pos[i * 3 + 2] = cz;
    elem[i] = 0;
    escaped[i] = 0;
    s2c[i] = (int32_t)i;
  }
}

__global__ void k_iota(int32_t *__restrict__ a, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    a[i] = (int32_t)i;
}

// Origin elision, step 1: d_origin_[p] := the previous move's staged
// destinations.  Plain streaming copy, 16 B per lane; `count` doubles.
// Both buffers come straight from hipMalloc (256 B aligned).
__global__ void k_copy_doubles(const double *__restrict__ src,
                               double *__restrict__ dst, int64_t count) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t pairs = count / 2;
  const double2 *__restrict__ s2 = reinterpret_cast<const double2 *>(src);
  double2 *__restrict__ d2 = reinterpret_cast<double2 *>(dst);
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < pairs;
       i += stride)
    d2[i] = s2[i];
  if ((count & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    dst[count - 1] = src[count - 1];
}

// Origin elision, step 2: overwrite the origins the host found changed.
// idx holds caller particle indices in [0, n), strictly increasing, so no
// two entries touch the same origin.
__global__ void k_scatter_origins(const int32_t *__restrict__ idx,
                                  const double *__restrict__ xyz,
                                  double *__restrict__ origin, int64_t count) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = blockIdx.x * blockDim.x + threadIdx.x; j < count;
       j += stride) {
    const int64_t i = idx[j];
    origin[i * 3] = xyz[j * 3];
    origin[i * 3 + 1] = xyz[j * 3 + 1];
    origin[i * 3 + 2] = xyz[j * 3 + 2];
  }
}

__global__ void k_locate(const Plane *__restrict__ planes, GridView grid,
                         const double *__restrict__ q,
                         double *__restrict__ pos, int32_t *__restrict__ elem,
                         uint8_t *__restrict__ escaped,
                         unsigned long long *__restrict__ loose, int64_t n,
                         double tol) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const Vec3 p{q[i * 3], q[i * 3 + 1], q[i * 3 + 2]};
    bool used_loose = false;
    elem[i] = grid_locate(grid, planes, p, tol, &used_loose);
    if (used_loose) atomicAdd(loose, 1ull); // rare by construction
    pos[i * 3] = p.x;
    pos[i * 3 + 1] = p.y;
    pos[i * 3 + 2] = p.z;
    escaped[i] = 0;
  }
}

__device__ __forceinline__ uint64_t morton_spread(uint64_t v) {
  v &= 0x1fffff;
  v = (v | v << 32) & 0x1f00000000ffffull;
  v = (v | v << 16) & 0x1f0000ff0000ffull;
  v = (v | v << 8) & 0x100f00f00f00f00full;
  v = (v | v << 4) & 0x10c30c30c30c30c3ull;
  v = (v | v << 2) & 0x1249249249249249ull;
  return v;
}

__global__ void k_morton_keys(const double *__restrict__ pos,
                              uint64_t *__restrict__ keys,
                              int32_t *__restrict__ vals, int64_t n, Vec3 lo,
                              Vec3 scale) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    double x = (pos[i * 3] - lo.x) * scale.x;
    double y = (pos[i * 3 + 1] - lo.y) * scale.y;
    double z = (pos[i * 3 + 2] - lo.z) * scale.z;
    x = x < 0 ? 0 : (x > 2097151.0 ? 2097151.0 : x);
    y = y < 0 ? 0 : (y > 2097151.0 ? 2097151.0 : y);
    z = z < 0 ? 0 : (z > 2097151.0 ? 2097151.0 : z);
    keys[i] = morton_spread((uint64_t)x) | (morton_spread((uint64_t)y) << 1) |
              (morton_spread((uint64_t)z) << 2);
    vals[i] = (int32_t)i;
  }
}

__global__ void k_permute_state(const int32_t *__restrict__ order,
                                const double *__restrict__ pos_in,
                                const int32_t *__restrict__ elem_in,
                                const uint8_t *__restrict__ esc_in,
                                const int32_t *__restrict__ s2c_in,
                                double *__restrict__ pos_out,
                                int32_t *__restrict__ elem_out,
                                uint8_t *__restrict__ esc_out,
                                int32_t *__restrict__ s2c_out, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
    const int32_t i = order[j];
    pos_out[j * 3] = pos_in[(int64_t)i * 3];
    pos_out[j * 3 + 1] = pos_in[(int64_t)i * 3 + 1];
    pos_out[j * 3 + 2] = pos_in[(int64_t)i * 3 + 2];
    elem_out[j] = elem_in[i];
    esc_out[j] = esc_in[i];
    s2c_out[j] = s2c_in[i];
  }
}

__global__ void k_accumulate_batch(double *__restrict__ flux,
                                   double *__restrict__ bsum,
                                   double *__restrict__ bsq, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double f = flux[i];
    bsum[i] += f;
    bsq[i] += f * f;
    flux[i] = 0.0;
  }
}

// end_batch() pass over the linear moments: running sum, then zero.
__global__ void k_accumulate_moments(double *__restrict__ mom,
                                     double *__restrict__ msum, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    msum[i] += mom[i];
    mom[i] = 0.0;
  }
}

__global__ void k_reduce_slices(double *__restrict__ flux, int64_t nelems,
                                int slices) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nelems;
       i += stride) {
    double s = flux[i];
    for (int k = 1; k < slices; ++k) {
      s += flux[(int64_t)k * nelems + i];
      flux[(int64_t)k * nelems + i] = 0.0;
    }
    flux[i] = s;
  }
}

// Wave-level tally aggregation: Morton-sorted slots put neighboring lanes
// in neighboring tets, so at a given walk iteration many of a wave's 64
// lanes tally into the SAME element.  The fp64-atomic pipe is the measured
// ceiling of the walk (profiles/README.md: chase probe 19.1 G atomics/s;
// walk at 84% of it), while VALU sits ~12% busy -- so spend idle VALU on a
// segmented wave reduction over runs of equal element id and issue ONE
// atomicAdd per run (the run tail carries the total).  Runs are maximal
// CONTIGUOUS ACTIVE lane spans with equal el: a gap in the active mask
// starts a new run, so shuffles never read across inactive lanes.
//
// wave_run_sum does the reduction over any number of values that share one
// key (one for the flux or a keyed current, five for the flux plus the four
// moments of a Linear crossing): the run structure (heads, tails) depends
// only on the key and the active mask, so it is computed ONCE however many
// values ride on it.  The run's tail lane then calls tail(totals...).
__device__ __forceinline__ void wave_run_step(double &acc, int off, int lane,
                                              int head_lane) {
  const double up = __shfl_up(acc, off);
  if (lane - off >= head_lane) acc += up;
}

template <class Tail, class... Acc>
__device__ __forceinline__ void wave_run_sum(int32_t key, Tail tail,
                                             Acc... acc) {
  const unsigned long long mask = __ballot(1);
  const int lane = (int)(threadIdx.x & 63u);
  const int32_t prev_key = __shfl_up(key, 1);
  const bool prev_active = lane > 0 && ((mask >> (lane - 1)) & 1ull);
  const bool head = !prev_active || prev_key != key;
  // inclusive max-scan of head lane indices: every lane learns its run head
  int head_lane = head ? lane : 0;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(head_lane, off);
    if (lane >= off && ((mask >> (lane - off)) & 1ull) && up > head_lane)
      head_lane = up;
  }
  // inclusive segmented sum over the run (all source lanes inside the run
  // are active and contiguous by construction)
#pragma unroll
  for (int off = 1; off < 64; off <<= 1)
    (wave_run_step(acc, off, lane, head_lane), ...);
  const int32_t next_key = __shfl_down(key, 1);
  const bool next_active = lane < 63 && ((mask >> (lane + 1)) & 1ull);
  if (!next_active || next_key != key) tail(acc...);
}

// The adder policies of the tally sink (core/tally_sink.h) on the device:
// one atomicAdd per value ...
struct AtomicPlus {
  __device__ __forceinline__ void operator()(double *p, double v) const {
    atomicAdd(p, v);
  }
};
using AtomicAdder = PlainAdder<AtomicPlus>;

// ... or, for unscored, ungrouped moves under wave aggregation (the flux
// index is then the element id, an int32 key), one atomicAdd per run: the
// flux through wave_run_sum; a Linear crossing's flux and four moments
// through ONE five-value reduction, the tail issuing flux[el] and the
// 32-byte span moments[4*el .. 4*el+3] (how the memory side treats a
// 32-byte atomic span is unmeasured; nothing here relies on it); a current
// as one plain atomicAdd per crossing (default), or with `cur_keyed` the
// same run aggregation keyed on the flat face index el*4+f, which the engine
// enables only while nelems*4 fits an int32.
struct WaveAdder {
  static constexpr bool kFusedMoments = true;
  bool cur_keyed;
  __device__ __forceinline__ void flux(double *__restrict__ flux, int64_t at,
                                       double v) const {
    const int32_t el = (int32_t)at;
    wave_run_sum(el, [&](double sum) { atomicAdd(&flux[el], sum); }, v);
  }
  __device__ __forceinline__ void moments(double *__restrict__ flux,
                                          double *__restrict__ mom, int64_t at,
                                          double v,
                                          const double (&m)[4]) const {
    const int32_t el = (int32_t)at;
    wave_run_sum(
        el,
        [&](double sum, double m0, double m1, double m2, double m3) {
          atomicAdd(&flux[el], sum);
          double *mo = mom + (int64_t)el * 4;
          atomicAdd(&mo[0], m0);
          atomicAdd(&mo[1], m1);
          atomicAdd(&mo[2], m2);
          atomicAdd(&mo[3], m3);
        },
        v, m[0], m[1], m[2], m[3]);
  }
  // a current, at4 = el*4 + face
  __device__ __forceinline__ void companion(double *__restrict__ cur,
                                            int64_t at4, double w) const {
    if (cur_keyed) {
      const int32_t key = (int32_t)at4;
      wave_run_sum(key, [&](double sum) { atomicAdd(&cur[key], sum); }, w);
    } else {
      atomicAdd(&cur[at4], w);
    }
  }
};

// The kernels' <Linear, Currents> switches as a sink mode.
template <bool Linear, bool Currents>
constexpr TallyMode kernel_tally_mode =
    Linear ? TallyMode::Linear
           : (Currents ? TallyMode::Currents : TallyMode::Flux);

template <bool Wave>
__device__ __forceinline__ auto make_adder(bool cur_keyed) {
  if constexpr (Wave)
    return WaveAdder{cur_keyed};
  else
    return AtomicAdder{};
}

// Face currents under the aggregated dispatch: plain atomics (default) or
// the same run aggregation keyed on the flat face index el*4+f
// (PUMITALLY_CURRENTS_AGG=1).  Read per engine, at construction, so one
// process can compare the two (benchmarks/currents_cost.py; figures in
// profiles/README.md).
inline bool currents_keyed_agg() {
  const char *s = getenv("PUMITALLY_CURRENTS_AGG");
  return s ? atoi(s) != 0 : false;
}

inline bool wave_agg() {
  static bool v = [] {
    const char *s = getenv("PUMITALLY_WAVE_AGG");
    // measured on MI355X: device-resident walk 1776 -> 1831M ps/s
    // (chord 8, sorted slots), flux bit-identical; default on
    return s ? atoi(s) != 0 : true;
  }();
  return v;
}

// Collision scoring under run aggregation: PUMITALLY_WAVE_AGG as for the
// walk, but read per engine, at construction, so one process can time both
// arms (benchmarks/collision_cost.py).  Default on: measured on MI355X at
// 10M particles, 0.220 ms aggregated against 0.337 ms plain per step for a
// spread source, 3.53 against 93.0 ms for the 2 % point source
// (profiles/README.md).
inline bool collisions_run_agg() {
  const char *s = getenv("PUMITALLY_WAVE_AGG");
  return s ? atoi(s) != 0 : true;
}

// What a wave's lanes did in one pass of a scoring loop, counted once per
// wave: every lane of the wave executes this (the loops below keep their
// trip count wave-uniform), so the two popcounts are the same value in all
// of them and each lane's running totals are the wave's.
__device__ __forceinline__ void score_count(bool active, bool hit,
                                            unsigned long long &scored,
                                            unsigned long long &missed) {
  const unsigned long long am = __ballot(active), hm = __ballot(hit);
  scored += (unsigned long long)__popcll(hm);
  missed += (unsigned long long)__popcll(am & ~hm);
}

__device__ __forceinline__ void
score_count_flush(unsigned long long scored, unsigned long long missed,
                  unsigned long long *__restrict__ counts) {
  if ((threadIdx.x & 63u) == 0) {
    if (scored) atomicAdd(&counts[0], scored);
    if (missed) atomicAdd(&counts[1], missed);
  }
}

// Engine::score_collisions on the device: one gather and one add per active
// particle, no geometry.  Iterates particle SLOTS (Morton order) with
// k_move's XCD-aware block->range mapping, so a wave's 64 lanes are
// neighbouring slots -- hence mostly the same few elements; the caller's
// arrays are gathered through s2c.  Reads elem/escaped, writes neither.
// Wave=true (host: no groups, no responses) keys the add on the int32
// element id and issues one atomicAdd per run of equal elements
// (wave_run_sum); Wave=false adds every value with a plain atomicAdd.
// counts[0] += particles that scored, counts[1] += misses.
template <bool Wave>
__global__ void k_score_slots(const int32_t *__restrict__ s2c,
                              const int32_t *__restrict__ elem,
                              const uint8_t *__restrict__ escaped,
                              const int8_t *__restrict__ active,
                              const double *__restrict__ weights,
                              const uint16_t *__restrict__ groups,
                              const double *__restrict__ resp, int ngroups,
                              int nscores, int64_t nelems,
                              double *__restrict__ coll,
                              unsigned long long *__restrict__ counts,
                              int64_t n) {
  const unsigned bpx = gridDim.x / 8u;
  const unsigned vb = bpx ? (blockIdx.x % 8u) * bpx + blockIdx.x / 8u
                          : blockIdx.x;
  const int64_t per_blk = (n + gridDim.x - 1) / gridDim.x;
  const int64_t base = (int64_t)vb * per_blk;
  const int64_t end = base + per_blk < n ? base + per_blk : n;
  const int lane = (int)(threadIdx.x & 63u);
  unsigned long long scored = 0, missed = 0;
  // i0 is the wave's first slot of the pass: the same in all 64 lanes
  for (int64_t i0 = base + (threadIdx.x - lane); i0 < end; i0 += blockDim.x) {
    const int64_t i = i0 + lane;
    int64_t c = 0;
    int32_t e = -1;
    bool act = false;
    if (i < end) {
      c = s2c[i];
      act = active[c] != 0;
    }
    if (act && !escaped[i]) e = elem[i];
    score_count(act, e >= 0, scored, missed);
    if (e < 0) continue;
    const int64_t goff =
        Wave ? 0 : tally_group_offset(groups, c, ngroups, nelems);
    score_contribute(make_adder<Wave>(false), coll, goff,
                     (int64_t)ngroups * nelems, e, weights[c],
                     Wave ? nullptr : resp, c, nscores);
  }
  score_count_flush(scored, missed, counts);
}

// Engine::score_points on the device: n free points in caller order,
// grid-stride, each localized with grid_locate (copy_initial_position's
// call) and scored like a particle.  Runs of equal elements only form when
// the caller sorted the points; the result does not depend on it.
template <bool Wave>
__global__ void k_score_points(const Plane *__restrict__ planes, GridView grid,
                               const double *__restrict__ xyz,
                               const double *__restrict__ weights,
                               const uint16_t *__restrict__ groups,
                               const double *__restrict__ resp, int ngroups,
                               int nscores, int64_t nelems, double tol,
                               double *__restrict__ coll,
                               unsigned long long *__restrict__ counts,
                               unsigned long long *__restrict__ loose,
                               int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int lane = (int)(threadIdx.x & 63u);
  unsigned long long scored = 0, missed = 0;
  for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane);
       i0 < n; i0 += stride) {
    const int64_t i = i0 + lane;
    int32_t e = -1;
    if (i < n) {
      bool used_loose = false;
      e = grid_locate(grid, planes,
                      Vec3{xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2]}, tol,
                      &used_loose);
      if (used_loose) atomicAdd(loose, 1ull); // rare by construction
    }
    score_count(i < n, e >= 0, scored, missed);
    if (e < 0) continue;
    const int64_t goff =
        Wave ? 0 : tally_group_offset(groups, i, ngroups, nelems);
    score_contribute(make_adder<Wave>(false), coll, goff,
                     (int64_t)ngroups * nelems, e, weights[i],
                     Wave ? nullptr : resp, i, nscores);
  }
  score_count_flush(scored, missed, counts);
}

// The fused move kernel: phase A (relocation of flying, non-escaped
// particles whose origin changed) + phase B (tallied walk to destination).
//
// Iteration is over particle SLOTS (spatial order); the caller's arrays
// are gathered through s2c.  Block->slot mapping is XCD-aware: MI355X
// dispatches block b to XCD b%8 and each XCD has a private 4 MiB L2; we
// remap blocks so each XCD owns one contiguous (hence spatially compact)
// slot range.  Purely a speed lever: any placement is correct.
//
// Linear=true additionally tallies the crossing's four barycentric moments
// (walk.h tet_moments) into `moments` -- ONE un-sliced array, see
// flux_slices -- reading `inv_h`.  Linear=false instantiations never read
// either trailing argument.
//
// Currents=true (never together with Linear) additionally adds the weight
// of every crossing to `cur` at (flux index)*4 + exit face -- ONE un-sliced
// array like the moments.  Under Agg the flux still goes through the run
// aggregation first thing in the callback, i.e. with the active set the
// non-currents kernel has there; the current follows (WaveAdder::current).
// Currents=false instantiations never read cur / cur_keyed.
//
// What a crossing contributes, and where, is the tally sink's business
// (core/tally_sink.h); the kernel only picks its mode and adder.
template <bool F32, bool Scored = false, bool Periodic = false,
          bool Agg = false, bool Linear = false, bool Currents = false>
__global__ void k_move(const Plane *__restrict__ planes,
                       const Plane32 *__restrict__ planes32,
                       const int32_t *__restrict__ nbr, GridView grid,
                       const int32_t *__restrict__ s2c,
                       const double *__restrict__ origin,
                       const double *__restrict__ dest,
                       const int8_t *__restrict__ flying,
                       const double *__restrict__ weights,
                       const uint16_t *__restrict__ groups, int ngroups,
                       double *__restrict__ pos, int32_t *__restrict__ elem,
                       uint8_t *__restrict__ escaped,
                       double *__restrict__ flux,
                       unsigned long long *__restrict__ lost,
                       double *__restrict__ lostrec,
                       unsigned long long *__restrict__ loose, int64_t lo,
                       int64_t hi, double loc_tol, int max_steps,
                       int64_t nelems, int slice_mask, bool reflective,
                       const uint32_t *__restrict__ face_bc,
                       const double *__restrict__ resp = nullptr,
                       int nscores = 1,
                       const int32_t *__restrict__ pidx = nullptr,
                       const int32_t *__restrict__ pelem = nullptr,
                       const double *__restrict__ pshift = nullptr,
                       const double *__restrict__ inv_h = nullptr,
                       double *__restrict__ moments = nullptr,
                       double *__restrict__ cur = nullptr,
                       bool cur_keyed = false) {
  static_assert(!(Linear && Currents), "linear + currents is not built");
  // Scored=false, Periodic=false is the headline instantiation:
  // resp/pidx are unused and the walk compiles without the score loop or
  // the periodic branch.  The slice stride is the allocated one in every
  // instantiation -- nelems*ngroups*nscores, the host's fsz_, which
  // k_reduce_slices reduces with: an engine built with nscores > 1 runs the
  // unscored kernels whenever a move passes no responses, and its slices
  // are still nscores scores apart.
  flux += (int64_t)(blockIdx.x & (unsigned)slice_mask) * nelems * ngroups *
          nscores;
  constexpr TallyMode Mode = kernel_tally_mode<Linear, Currents>;
  const TallyMesh tmesh{planes, inv_h, nbr, face_bc, pidx, reflective};
  const unsigned bpx = gridDim.x / 8u;
  const unsigned vb = (blockIdx.x % 8u) * bpx + blockIdx.x / 8u;
  const int64_t m = hi - lo;
  const int64_t per_blk = (m + gridDim.x - 1) / gridDim.x;
  const int64_t base = lo + (int64_t)vb * per_blk;
  const int64_t end = base + per_blk < hi ? base + per_blk : hi;

  for (int64_t i = base + threadIdx.x; i < end; i += blockDim.x) {
    const int64_t c = s2c[i];
    if (!flying[c]) continue;
    Vec3 o{pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2]};
    int32_t e = elem[i];
    if (origin != nullptr && !escaped[i]) {
      const Vec3 q{origin[c * 3], origin[c * 3 + 1], origin[c * 3 + 2]};
      if (q.x != o.x || q.y != o.y || q.z != o.z) {
        bool used_loose = false;
        e = grid_locate(grid, planes, q, loc_tol, &used_loose);
        if (used_loose) atomicAdd(loose, 1ull);
        o = q;
      }
    }
    if (e < 0) {
      pos[i * 3] = o.x;
      pos[i * 3 + 1] = o.y;
      pos[i * 3 + 2] = o.z;
      elem[i] = e;
      continue;
    }
    const Vec3 d{dest[c * 3], dest[c * 3 + 1], dest[c * 3 + 2]};
    int32_t out_elem;
    Vec3 out_pos;
    bool out_esc;
    // Wave aggregation is dispatched only when groups==nullptr, so the group
    // offset is 0 for every lane and the element id alone is the key.
    constexpr bool Wave = Agg && !Scored;
    const int64_t goff =
        Wave ? 0 : tally_group_offset(groups, c, ngroups, nelems);
    // An escaped particle leaving again where it sits is one departure
    // (walk.h walk_current_face); the flag is read only by Currents
    // instantiations.
    bool reexit = false;
    if constexpr (Currents) reexit = escaped[i] != 0;
    TallySink<Mode, Scored, decltype(make_adder<Wave>(cur_keyed)),
              /*ReexitRule=*/true, Periodic>
        sink{make_adder<Wave>(cur_keyed), flux, Linear ? moments : cur, goff,
             (int64_t)ngroups * nelems, resp, c, nscores, tmesh, reexit};
    auto walk = [&](auto &tally) {
      if constexpr (F32)
        walk_segment32<Periodic>(planes, planes32, nbr, e, o, d, weights[c],
                                 max_steps, tally, &out_elem, &out_pos,
                                 &out_esc, reflective, face_bc, pidx, pelem,
                                 pshift);
      else
        walk_segment<Periodic>(planes, nbr, e, o, d, weights[c], max_steps,
                               tally, &out_elem, &out_pos, &out_esc,
                               reflective, face_bc, pidx, pelem, pshift);
    };
    walk(sink);
    if (out_elem == kWalkLost) {
      const unsigned long long k = atomicAdd(lost, 1ull);
      if (k < (unsigned long long)kMaxLostRecords) {
        lostrec[k * 4] = (double)c;
        lostrec[k * 4 + 1] = out_pos.x;
        lostrec[k * 4 + 2] = out_pos.y;
        lostrec[k * 4 + 3] = out_pos.z;
      }
      out_elem = e;
    }
    elem[i] = out_elem;
    pos[i * 3] = out_pos.x;
    pos[i * 3 + 1] = out_pos.y;
    pos[i * 3 + 2] = out_pos.z;
    escaped[i] = out_esc ? 1 : 0;
  }
}

template <bool F32, bool Linear = false, bool Currents = false>
__global__ void k_walk_raw(const Plane *__restrict__ planes,
                           const Plane32 *__restrict__ planes32,
                           const int32_t *__restrict__ nbr,
                           const double *__restrict__ pos,
                           const double *__restrict__ dest,
                           const int32_t *__restrict__ elem,
                           const double *__restrict__ weights,
                           const uint16_t *__restrict__ groups,
                           const double *__restrict__ resp,
                           double *__restrict__ out_pos,
                           int32_t *__restrict__ out_elem,
                           int8_t *__restrict__ out_status,
                           double *__restrict__ out_dest,
                           double *__restrict__ flux,
                           unsigned long long *__restrict__ lost,
                           double *__restrict__ lostrec, int64_t n,
                           int max_steps, bool reflective,
                           const uint32_t *__restrict__ face_bc, int ngroups,
                           int64_t nelems, int nscores,
                           const int32_t *__restrict__ pidx = nullptr,
                           const int32_t *__restrict__ pelem = nullptr,
                           const double *__restrict__ pshift = nullptr,
                           const double *__restrict__ in_t = nullptr,
                           const int32_t *__restrict__ in_prev = nullptr,
                           double *__restrict__ out_o = nullptr,
                           double *__restrict__ out_t = nullptr,
                           int32_t *__restrict__ out_prev = nullptr,
                           const double *__restrict__ inv_h = nullptr,
                           double *__restrict__ moments = nullptr,
                           double *__restrict__ cur = nullptr) {
  static_assert(!(Linear && Currents), "linear + currents is not built");
  // XCD-aware block->range remap, same as k_move: MI355X dispatches
  // block b to XCD b%8; giving each XCD one contiguous (spatially
  // compact, since callers keep lists near-Morton-ordered) index range
  // keeps its private L2 on one mesh region.
  constexpr TallyMode Mode = kernel_tally_mode<Linear, Currents>;
  const TallyMesh tmesh{planes, inv_h, nbr, face_bc, pidx, reflective};
  const unsigned bpx = gridDim.x / 8u;
  const unsigned vb = bpx ? (blockIdx.x % 8u) * bpx + blockIdx.x / 8u
                          : blockIdx.x;
  const int64_t per_blk = (n + gridDim.x - 1) / gridDim.x;
  const int64_t base = (int64_t)vb * per_blk;
  const int64_t end = base + per_blk < n ? base + per_blk : n;
  for (int64_t i = base + threadIdx.x; i < end; i += blockDim.x) {
    const Vec3 o{pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2]};
    const Vec3 d{dest[i * 3], dest[i * 3 + 1], dest[i * 3 + 2]};
    int32_t oe;
    Vec3 op;
    bool esc;
    // Plain atomics; responses are a run-time choice here.  Resumed walks
    // need nothing extra for the moments (in_t only seeds t_cur), and a
    // resumed walk starts inside its element, so the crossing its sender
    // counted is not counted again -- there is no re-exit rule.
    TallySink<Mode, /*Scored=*/true, AtomicAdder> sink{
        AtomicAdder{}, flux, Linear ? moments : cur,
        tally_group_offset(groups, i, ngroups, nelems),
        (int64_t)ngroups * nelems, resp, i, nscores, tmesh, false};
    Vec3 od{d.x, d.y, d.z};
    const double rt = in_t ? in_t[i] : 0.0;
    const int32_t rp = in_prev ? in_prev[i] : -1;
    Vec3 oo{o.x, o.y, o.z};
    double ot = 0.0;
    int32_t opv = -1;
    auto walk = [&](auto &tally) {
      if constexpr (F32)
        walk_segment32<true>(planes, planes32, nbr, elem[i], o, d, weights[i],
                             max_steps, tally, &oe, &op, &esc, reflective,
                             face_bc, pidx, pelem, pshift, &od, rt, rp, &oo,
                             &ot, &opv);
      else
        walk_segment<true>(planes, nbr, elem[i], o, d, weights[i], max_steps,
                           tally, &oe, &op, &esc, reflective, face_bc, pidx,
                           pelem, pshift, &od, rt, rp, &oo, &ot, &opv);
    };
    walk(sink);
    int8_t st = 0;
    if (oe == kWalkLost) {
      st = 3;
      oe = elem[i];
      const unsigned long long k = atomicAdd(lost, 1ull);
      if (k < (unsigned long long)kMaxLostRecords) {
        lostrec[k * 4] = (double)i;
        lostrec[k * 4 + 1] = op.x;
        lostrec[k * 4 + 2] = op.y;
        lostrec[k * 4 + 3] = op.z;
      }
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

// Sum over the wave's lanes of a small non-negative per-lane count, by bit
// planes: one ballot and one popcount per bit any lane has set.  Executed by
// all 64 lanes; every lane gets the sum.
__device__ __forceinline__ unsigned long long wave_count_sum(unsigned v) {
  unsigned long long sum = 0;
  for (int b = 0; __ballot(v >> b) != 0ull; ++b)
    sum += (unsigned long long)__popcll(__ballot((v >> b) & 1u)) << b;
  return sum;
}

// Engine::tally_tracks on the device: one lane per free track, in caller
// order, k_walk_raw's XCD-aware block->range remap.  Each track is
// core/track.h track_tally -- localize the origin, walk, and on every vacuum
// clip search the boundary-face grid for the next entry -- through the tally
// sink with plain atomics into flux slice 0 (responses a run-time choice, no
// re-exit rule), as k_walk_raw.  Reads no particle state.  The loop's trip
// count is wave-uniform, so entries and misses are summed per wave and
// flushed with one atomicAdd each: counts[0] += entries, counts[1] += misses.
template <bool F32, TallyMode Mode>
__global__ void k_tally_tracks(TrackMesh trk, const double *__restrict__ origin,
                               const double *__restrict__ dest,
                               const double *__restrict__ weights,
                               const uint16_t *__restrict__ groups,
                               const double *__restrict__ resp,
                               double *__restrict__ flux,
                               double *__restrict__ companion,
                               const double *__restrict__ inv_h,
                               unsigned long long *__restrict__ counts,
                               unsigned long long *__restrict__ lost,
                               double *__restrict__ lostrec,
                               unsigned long long *__restrict__ loose,
                               int64_t n, int ngroups, int64_t nelems,
                               int nscores) {
  const TallyMesh tmesh{trk.planes, inv_h,    trk.nbr,
                        trk.face_bc, trk.pidx, trk.reflective};
  const unsigned bpx = gridDim.x / 8u;
  const unsigned vb = bpx ? (blockIdx.x % 8u) * bpx + blockIdx.x / 8u
                          : blockIdx.x;
  const int64_t per_blk = (n + gridDim.x - 1) / gridDim.x;
  const int64_t base = (int64_t)vb * per_blk;
  const int64_t end = base + per_blk < n ? base + per_blk : n;
  const int lane = (int)(threadIdx.x & 63u);
  unsigned long long entries = 0, misses = 0;
  // i0 is the wave's first track of the pass: the same in all 64 lanes
  for (int64_t i0 = base + (threadIdx.x - lane); i0 < end; i0 += blockDim.x) {
    const int64_t i = i0 + lane;
    TrackResult r;
    if (i < end) {
      const Vec3 o{origin[i * 3], origin[i * 3 + 1], origin[i * 3 + 2]};
      const Vec3 d{dest[i * 3], dest[i * 3 + 1], dest[i * 3 + 2]};
      TallySink<Mode, /*Scored=*/true, AtomicAdder> sink{
          AtomicAdder{}, flux, companion,
          tally_group_offset(groups, i, ngroups, nelems),
          (int64_t)ngroups * nelems, resp, i, nscores, tmesh, false};
      track_tally<F32>(trk, o, d, weights[i], sink, r);
      if (r.loose) atomicAdd(loose, 1ull); // rare by construction
      if (r.lost) {
        const unsigned long long k = atomicAdd(lost, 1ull);
        if (k < (unsigned long long)kMaxLostRecords) {
          lostrec[k * 4] = (double)i;
          lostrec[k * 4 + 1] = r.lost_pos.x;
          lostrec[k * 4 + 2] = r.lost_pos.y;
          lostrec[k * 4 + 3] = r.lost_pos.z;
        }
      }
    }
    entries += wave_count_sum((unsigned)r.entries);
    misses += (unsigned long long)__popcll(__ballot(r.miss));
  }
  if (lane == 0) {
    if (entries) atomicAdd(&counts[0], entries);
    if (misses) atomicAdd(&counts[1], misses);
  }
}

// Tally slices: S independent copies of the flux array, selected by
// blockIdx & (S-1), reduced at readout.  The hot-element (point-source)
// mitigation: measured on MI355X (profiles/README.md round 2), the
// config-4 contention stress at 10M particles through a 2%-cube source
// runs 74.2 ms/step with 1 slice, 7.8 ms with 64 and 6.48 ms with 256
// (11.4x, within 18% of the uncontended walk), while spread sources and
// the headline are unchanged to the noise floor at any slice count.
// Default is adaptive: 256 slices when the copies fit a 2 GiB HBM
// budget (trivial against 288 GB for 1M-tet meshes), halved until they
// do.
// The linear moments (Engine::moments) are NOT sliced: one device copy,
// 4x the size of one flux slice, so slicing them too would quadruple the
// footprint.  Only the flux stays privatized.
int flux_slices(int64_t flux_doubles) {
  const char *s = getenv("PUMITALLY_FLUX_SLICES");
  int k = s ? atoi(s) : 256;
  if (k < 1) k = 1;
  if (k > 256) k = 256;
  while (k & (k - 1)) k--; // power of two for the cheap in-kernel mask
  if (!s) {
    // adaptive: keep the slice copies under ~2 GiB
    const int64_t budget = (int64_t)2 << 30;
    while (k > 1 && flux_doubles * k * 8 > budget) k >>= 1;
  }
  return k;
}

int grid_cap() {
  static int cap = [] {
    const char *s = getenv("PUMITALLY_GRID_CAP");
    return s ? atoi(s) : 1024; // swept on MI355X: 1024 > 2048 > 4096
  }();
  return cap;
}

int sort_every() {
  static int v = [] {
    const char *s = getenv("PUMITALLY_SORT");
    return s ? atoi(s) : 16; // re-sort cadence in moves; 0 disables
  }();
  return v;
}

int64_t chunk_particles(int64_t n) {
  static int64_t c = [] {
    const char *s = getenv("PUMITALLY_CHUNK");
    return s ? (int64_t)atoll(s) : (int64_t)0;
  }();
  if (c > 0) return c;
  // swept on MI355X: ~2.6M-particle chunks beat 1.25M and whole-batch
  return std::max<int64_t>((int64_t)2621440, (n + 7) / 8);
}

int grid_blocks(int64_t work) {
  int64_t blocks = (work + kBlock - 1) / kBlock;
  if (blocks > grid_cap()) blocks = grid_cap();
  // round up to a multiple of 8 for the XCD-aware remap in k_move
  return (int)((blocks + 7) / 8 * 8);
}

class GpuEngine final : public Engine {
public:
  GpuEngine(Mesh mesh, int64_t n, int device, int groups, int scores,
            bool lin, bool cur, bool coll)
      : mesh_(std::move(mesh)), n_(n) {
    ngroups = groups < 1 ? 1 : groups;
    nscores = scores < 1 ? 1 : scores;
    linear = lin;
    face_currents = cur;
    collision_tallies = coll;
    PT_HIP_CHECK(hipSetDevice(device));
    device_ = device;
    s_copy_.create();
    s_comp_.create();
    for (auto &ev : copy_ev_) ev.create();
    for (auto &ev : kernels_done_) ev.create();
    if (collision_tallies) {
      s_score_.create();
      score_copied_.create();
      score_done_.create();
    }

    // Mesh upload (once).
    d_planes_ = upload(mesh_.planes);
    d_planes32_ = upload(mesh_.planes32);
    d_nbr_ = upload(mesh_.nbr);
    d_cell_start_ = upload(mesh_.grid.cell_start);
    d_cell_tets_.allocate(mesh_.grid.cell_tets.size() + 1);
    PT_HIP_CHECK(hipMemcpy(d_cell_tets_, mesh_.grid.cell_tets.data(),
                           mesh_.grid.cell_tets.size() * sizeof(int32_t),
                           hipMemcpyHostToDevice));
    d_face_bc_ = upload(mesh_.face_bc_bits); // empty: stays null
    if (mesh_.has_periodic()) {
      d_pidx_ = upload(mesh_.periodic_idx);
      d_pelem_ = upload(mesh_.periodic_elem);
      d_pshift_ = upload(mesh_.periodic_shift);
    }
    grid_view_ = GridView{mesh_.grid.nx, mesh_.grid.ny, mesh_.grid.nz,
                          mesh_.grid.lo,  mesh_.grid.inv_h,
                          d_cell_start_,  d_cell_tets_};

    // Particle state (slot order) + slot->caller map.
    d_pos_.allocate(n_ * 3);
    d_elem_.allocate(n_);
    d_escaped_.allocate(n_);
    d_s2c_.allocate(n_);
    fsz_ = mesh_.nelems * ngroups * nscores;
    slices_ = flux_slices(fsz_);
    d_flux_.allocate(fsz_ * slices_);
    d_lost_.allocate(1);
    d_loose_.allocate(1);
    d_lostrec_.allocate((int64_t)kMaxLostRecords * 4);
    PT_HIP_CHECK(hipMemset(d_flux_, 0, fsz_ * slices_ * sizeof(double)));
    if (linear) {
      mesh_.build_inv_heights();
      d_inv_h_ = upload(mesh_.inv_heights);
      d_moments_.allocate(fsz_ * 4);
      PT_HIP_CHECK(hipMemset(d_moments_, 0, fsz_ * 4 * sizeof(double)));
    }
    if (face_currents) {
      d_cur_.allocate(fsz_ * 4);
      PT_HIP_CHECK(hipMemset(d_cur_, 0, fsz_ * 4 * sizeof(double)));
      // the keyed aggregation carries el*4+f in an int32 lane value
      cur_keyed_ = currents_keyed_agg() && mesh_.nelems < ((int64_t)1 << 29);
    }
    if (collision_tallies) {
      d_coll_.allocate(fsz_);
      PT_HIP_CHECK(hipMemset(d_coll_, 0, fsz_ * sizeof(double)));
      d_coll_counts_.allocate(2);
      PT_HIP_CHECK(
          hipMemset(d_coll_counts_, 0, 2 * sizeof(unsigned long long)));
      coll_agg_ = collisions_run_agg();
    }
    PT_HIP_CHECK(hipMemset(d_lost_, 0, sizeof(unsigned long long)));
    PT_HIP_CHECK(hipMemset(d_loose_, 0, sizeof(unsigned long long)));
    PT_HIP_CHECK(
        hipMemset(d_lostrec_, 0, kMaxLostRecords * 4 * sizeof(double)));

    // Parity double-buffered input staging.
    for (int p = 0; p < 2; ++p) {
      d_origin_[p].allocate(n_ * 3);
      d_dest_[p].allocate(n_ * 3);
      d_flying_[p].allocate(n_);
      d_weights_[p].allocate(n_);
      if (ngroups > 1) d_groups_[p].allocate(n_);
      // d_resp_ is lazy-allocated on the first move() that passes
      // responses (valid even with nscores==1: a single per-particle
      // response multiplier).
    }

    // Spatial-sort scratch.
    sort_every_ = sort_every();
    if (sort_every_ > 0) {
      d_keys_.allocate(n_);
      d_keys2_.allocate(n_);
      d_vals_.allocate(n_);
      d_order_.allocate(n_);
      d_pos2_.allocate(n_ * 3);
      d_elem2_.allocate(n_);
      d_esc2_.allocate(n_);
      d_s2c2_.allocate(n_);
      size_t bytes = 0;
      PT_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(
          nullptr, bytes, d_keys_.get(), d_keys2_.get(), d_vals_.get(),
          d_order_.get(), (int)n_, 0, 64, s_comp_));
      sorttmp_bytes_ = bytes;
      d_sorttmp_.allocate(bytes ? bytes : 1);
      const Vec3 ext = mesh_.bbox_hi - mesh_.bbox_lo;
      sort_scale_ = Vec3{ext.x > 0 ? 2097151.0 / ext.x : 0.0,
                         ext.y > 0 ? 2097151.0 / ext.y : 0.0,
                         ext.z > 0 ? 2097151.0 / ext.z : 0.0};
    }

    loc_tol_ = loc_tol_rel() * norm(mesh_.bbox_hi - mesh_.bbox_lo);
    walk_fp32 = default_walk_fp32();
    reflective = default_reflective();
    origin_elide = default_origin_elide();
    origin_threads = default_origin_threads();
    origin_chunk = default_origin_chunk();
    const Vec3 c0 = mesh_.nelems > 0 ? mesh_.centroid(0) : Vec3{0, 0, 0};
    k_init_particles<<<grid_blocks(n_), kBlock, 0, s_comp_>>>(
        d_pos_, d_elem_, d_escaped_, d_s2c_, n_, c0.x, c0.y, c0.z);
    PT_HIP_CHECK(hipGetLastError());
    PT_HIP_CHECK(hipStreamSynchronize(s_comp_));
  }

  ~GpuEngine() override {
    (void)hipSetDevice(device_);
    (void)hipDeviceSynchronize();
    // members release themselves: buffers first, then events and streams
  }

  int64_t num_particles() const override { return n_; }
  const Mesh &mesh() const override { return mesh_; }

  void copy_initial_position(const double *p, int64_t n) override {
    check_n(n);
    PT_HIP_CHECK(hipSetDevice(device_));
    sync(); // staging buffers and state may be read by in-flight kernels
    stage(p, n * 3 * sizeof(double), d_origin_[0], s_copy_);
    PT_HIP_CHECK(hipStreamSynchronize(s_copy_));
    k_iota<<<grid_blocks(n_), kBlock, 0, s_comp_>>>(d_s2c_, n_);
    k_locate<<<grid_blocks(n_), kBlock, 0, s_comp_>>>(
        d_planes_, grid_view_, d_origin_[0], d_pos_, d_elem_, d_escaped_,
        d_loose_, n_, loc_tol_);
    PT_HIP_CHECK(hipGetLastError());
    if (sort_every_ > 0) spatial_sort();
    moves_since_sort_ = 0;
    // k_locate reads the staging buffer d_origin_[0]; an immediately
    // following move() would re-stage into it with no recorded fence
    // (kernels_done_[0] has never been recorded at that point).  This is
    // a once-per-batch call: block until localization/sort finish.
    PT_HIP_CHECK(hipStreamSynchronize(s_comp_));
  }

  void move(const double *origin, const double *dest, const int8_t *flying,
            const double *weights, int64_t n,
            const uint16_t *groups = nullptr,
            const double *responses = nullptr) override {
    check_n(n);
    PT_HIP_CHECK(hipSetDevice(device_));
    const int steps = max_steps > 0 ? max_steps : default_max_steps(mesh_);
    const int p = (int)(parity_++ & 1);
    // WAR fence: buffer set p was last read by the kernels of the move
    // two calls ago; its copies must wait for them.
    PT_HIP_CHECK(hipStreamWaitEvent(s_copy_, kernels_done_[p], 0));
    if (responses && !d_resp_[p]) d_resp_[p].allocate(n_ * nscores);
    // Origin elision applies when the host shadow holds exactly what the
    // previous call staged into d_dest_[p^1]; every other case (continue
    // semantics, switch off, back-off, first move) takes the plain upload.
    const bool probe = origin && origin_elide && n > 0 && elide_skip_ == 0;
    if (probe && shadow_valid_) {
      stage_elided(p, origin, dest, flying, weights, groups, responses, n);
    } else {
      if (origin) {
        stage(origin, n * 3 * sizeof(double), d_origin_[p], s_copy_);
        stats_.origin_bytes_uploaded += n * 3 * (int64_t)sizeof(double);
      }
      stage_inputs(p, dest, flying, weights, groups, responses, n);
      // d_dest_[p] no longer matches the shadow (move_continue marks it
      // invalid rather than paying for an update it may never use) ...
      shadow_valid_ = false;
      if (probe) {
        // ... unless this is a full upload that seeds it: copy the
        // caller's dest while the DMA engine is busy with the copies above.
        ensure_elide_host(n);
        const auto t0 = std::chrono::steady_clock::now();
        origin_delta_seed(*delta_pool_, dest, shadow_.get(), 0, n,
                          /*nontemporal=*/false);
        stats_.origin_pass_seconds += seconds_since(t0);
        shadow_valid_ = true;
      } else if (origin && origin_elide && elide_skip_ > 0) {
        --elide_skip_;
      }
    }
    PT_HIP_CHECK(hipEventRecord(copy_ev_[p], s_copy_));
    PT_HIP_CHECK(hipStreamWaitEvent(s_comp_, copy_ev_[p], 0));
    launch_move_chunks(origin ? d_origin_[p] : nullptr, d_dest_[p],
                       d_flying_[p], d_weights_[p],
                       groups ? d_groups_[p] : nullptr,
                       responses ? d_resp_[p] : nullptr, n, steps);
    PT_HIP_CHECK(hipEventRecord(kernels_done_[p], s_comp_));
    maybe_resort();
    // The caller may mutate or free its buffers as soon as move() returns
    // (the facade zeroes the flying array; transients die).  Block until
    // every H2D copy has consumed them; the walk keeps running async.
    PT_HIP_CHECK(hipStreamSynchronize(s_copy_));
    stats_.moves++;
  }

  void move_device(const double *d_origin, const double *d_dest,
                   const int8_t *d_flying, const double *d_weights, int64_t n,
                   const uint16_t *d_groups = nullptr,
                   const double *d_responses = nullptr) override {
    check_n(n);
    PT_HIP_CHECK(hipSetDevice(device_));
    const int steps = max_steps > 0 ? max_steps : default_max_steps(mesh_);
    launch_move_chunks(d_origin, d_dest, d_flying, d_weights, d_groups,
                       d_responses, n, steps);
    maybe_resort();
    stats_.moves++;
  }

  // ---- collision-estimator scoring (engine.h) ---------------------------
  //
  // score_collisions stages the caller's arrays into buffers of its own
  // (sc_*, allocated on first use: 11 + 8*nscores B per particle with groups
  // and responses) on a stream of its own, so it neither uses nor advances
  // anything move() owns: not the parity buffers d_*_[p], not parity_, not
  // the elision shadow, not moves_since_sort_.  Ordering:
  //   * uploads (s_score_) wait for score_done_, the previous score kernel,
  //     the only other reader or writer of sc_*;
  //   * the kernel goes on s_comp_ after score_copied_, i.e. behind every
  //     queued move and re-sort, and sees the state they leave;
  //   * the call returns once s_score_ has drained, i.e. the copies have
  //     consumed the caller's arrays (move()'s contract); the kernel keeps
  //     running async, and every readback syncs s_comp_.
  void score_collisions(const int8_t *active, const double *weights,
                        int64_t n, const uint16_t *groups = nullptr,
                        const double *responses = nullptr) override {
    if (!collision_tallies) throw_not_collisions();
    check_n(n);
    if (n == 0) return;
    PT_HIP_CHECK(hipSetDevice(device_));
    if (!sc_active_) {
      sc_active_.allocate(n_);
      sc_weights_.allocate(n_);
    }
    if (groups && !sc_groups_) sc_groups_.allocate(n_);
    if (responses && !sc_resp_) sc_resp_.allocate(n_ * nscores);
    if (score_queued_)
      PT_HIP_CHECK(hipStreamWaitEvent(s_score_, score_done_, 0));
    stage(active, n * sizeof(int8_t), sc_active_, s_score_);
    stage(weights, n * sizeof(double), sc_weights_, s_score_);
    if (groups) stage(groups, n * sizeof(uint16_t), sc_groups_, s_score_);
    if (responses)
      stage(responses, n * nscores * sizeof(double), sc_resp_, s_score_);
    PT_HIP_CHECK(hipEventRecord(score_copied_, s_score_));
    PT_HIP_CHECK(hipStreamWaitEvent(s_comp_, score_copied_, 0));
    launch_score_slots(sc_active_, sc_weights_, groups ? sc_groups_ : nullptr,
                       responses ? sc_resp_ : nullptr);
    PT_HIP_CHECK(hipEventRecord(score_done_, s_comp_));
    score_queued_ = true;
    PT_HIP_CHECK(hipStreamSynchronize(s_score_));
  }

  void score_collisions_device(const int8_t *d_active, const double *d_weights,
                               int64_t n, const uint16_t *d_groups = nullptr,
                               const double *d_responses = nullptr) override {
    if (!collision_tallies) throw_not_collisions();
    check_n(n);
    if (n == 0) return;
    PT_HIP_CHECK(hipSetDevice(device_));
    launch_score_slots(d_active, d_weights, d_groups, d_responses);
  }

  void launch_score_slots(const int8_t *active, const double *weights,
                          const uint16_t *groups, const double *resp) {
    const auto kernel = coll_agg_ && !groups && !resp ? k_score_slots<true>
                                                      : k_score_slots<false>;
    kernel<<<grid_blocks(n_), kBlock, 0, s_comp_>>>(
        d_s2c_, d_elem_, d_escaped_, active, weights, groups, resp, ngroups,
        nscores, mesh_.nelems, d_coll_, d_coll_counts_, n_);
    PT_HIP_CHECK(hipGetLastError());
  }

  // Grow-once scratch of score_points, like WalkRawScratch.
  struct ScorePointsScratch {
    DeviceBuffer<double> xyz, w, resp;
    DeviceBuffer<uint16_t> groups;
  };

  void score_points(int64_t n, const double *xyz, const double *weights,
                    const uint16_t *groups = nullptr,
                    const double *responses = nullptr) override {
    if (!collision_tallies) throw_not_collisions();
    if (n <= 0) return;
    PT_HIP_CHECK(hipSetDevice(device_));
    // the previous call synchronized s_comp_ before returning, so the
    // scratch is free for reuse here
    sp_.xyz.reserve(n * 3);
    sp_.w.reserve(n);
    if (groups) sp_.groups.reserve(n);
    if (responses) sp_.resp.reserve(n * nscores);
    PT_HIP_CHECK(hipMemcpy(sp_.xyz, xyz, n * 3 * 8, hipMemcpyHostToDevice));
    PT_HIP_CHECK(hipMemcpy(sp_.w, weights, n * 8, hipMemcpyHostToDevice));
    if (groups)
      PT_HIP_CHECK(hipMemcpy(sp_.groups, groups, n * 2, hipMemcpyHostToDevice));
    if (responses)
      PT_HIP_CHECK(hipMemcpy(sp_.resp, responses, n * nscores * 8,
                             hipMemcpyHostToDevice));
    launch_score_points(n, sp_.xyz, sp_.w, groups ? sp_.groups.get() : nullptr,
                        responses ? sp_.resp.get() : nullptr);
    PT_HIP_CHECK(hipStreamSynchronize(s_comp_));
  }

  void score_points_device(int64_t n, const double *d_xyz,
                           const double *d_weights,
                           const uint16_t *d_groups = nullptr,
                           const double *d_responses = nullptr) override {
    if (!collision_tallies) throw_not_collisions();
    if (n <= 0) return;
    PT_HIP_CHECK(hipSetDevice(device_));
    launch_score_points(n, d_xyz, d_weights, d_groups, d_responses);
  }

  void launch_score_points(int64_t n, const double *xyz, const double *weights,
                           const uint16_t *groups, const double *resp) {
    const auto kernel = coll_agg_ && !groups && !resp ? k_score_points<true>
                                                      : k_score_points<false>;
    kernel<<<grid_blocks(n), kBlock, 0, s_comp_>>>(
        d_planes_, grid_view_, xyz, weights, groups, resp, ngroups, nscores,
        mesh_.nelems, loc_tol_, d_coll_, d_coll_counts_, d_loose_, n);
    PT_HIP_CHECK(hipGetLastError());
  }

  // Grow-once scratch of tally_tracks, like ScorePointsScratch.
  // Every array has a pinned host twin the caller's rows are copied into
  // first, so the uploads run async at the full link rate whatever memory
  // the caller passed.
  struct TrackScratch {
    DeviceBuffer<double> origin, dest, w, resp;
    DeviceBuffer<uint16_t> groups;
    PinnedBuffer<double> h_origin, h_dest, h_w, h_resp;
    PinnedBuffer<uint16_t> h_groups;
  };

  // Upload `count` elements of src through the pinned twin, on s_comp_.
  template <class T>
  void stage_pinned(const T *src, int64_t count, PinnedBuffer<T> &pin,
                    DeviceBuffer<T> &dev) {
    if (pin.size() < count) pin.allocate(count + count / 4);
    dev.reserve(count);
    std::memcpy(pin.get(), src, (size_t)count * sizeof(T));
    stage(pin.get(), (size_t)count * sizeof(T), dev, s_comp_);
  }

  // Stateless track tallies (engine.h, core/track.h).  The uploads and the
  // kernel are queued on the compute stream, behind every queued move, and
  // the call returns once they have drained, so the scratch is free for the
  // next call.
  void tally_tracks(int64_t n, const double *origin, const double *dest,
                    const double *weights, const uint16_t *groups = nullptr,
                    const double *responses = nullptr) override {
    if (n <= 0) return;
    PT_HIP_CHECK(hipSetDevice(device_));
    ensure_face_grid();
    stage_pinned(origin, n * 3, tt_.h_origin, tt_.origin);
    stage_pinned(dest, n * 3, tt_.h_dest, tt_.dest);
    stage_pinned(weights, n, tt_.h_w, tt_.w);
    if (groups) stage_pinned(groups, n, tt_.h_groups, tt_.groups);
    if (responses)
      stage_pinned(responses, n * nscores, tt_.h_resp, tt_.resp);
    launch_tally_tracks(n, tt_.origin, tt_.dest, tt_.w,
                        groups ? tt_.groups.get() : nullptr,
                        responses ? tt_.resp.get() : nullptr);
    PT_HIP_CHECK(hipStreamSynchronize(s_comp_));
  }

  void tally_tracks_device(int64_t n, const double *d_origin,
                           const double *d_dest, const double *d_weights,
                           const uint16_t *d_groups = nullptr,
                           const double *d_responses = nullptr) override {
    if (n <= 0) return;
    PT_HIP_CHECK(hipSetDevice(device_));
    ensure_face_grid();
    launch_tally_tracks(n, d_origin, d_dest, d_weights, d_groups, d_responses);
  }

  // First tally_tracks call: build the boundary-face grid on the engine's
  // mesh copy (throws on a mesh with partition-cut faces, every time: a
  // refused mesh is remembered) and upload it, once.
  void ensure_face_grid() {
    if (d_track_counts_) return;
    if (tracks_refused_)
      throw std::invalid_argument(
          "track tallies do not support a mesh with partition-cut faces");
    try {
      mesh_.build_face_grid();
    } catch (const std::invalid_argument &) {
      tracks_refused_ = true; // checked once, the answer is kept
      throw;
    }
    d_face_start_ = upload(mesh_.face_cell_start);
    d_face_list_.allocate((int64_t)mesh_.face_cell_faces.size() + 1);
    PT_HIP_CHECK(hipMemcpy(d_face_list_, mesh_.face_cell_faces.data(),
                           mesh_.face_cell_faces.size() * sizeof(int32_t),
                           hipMemcpyHostToDevice));
    d_track_counts_.allocate(2);
    PT_HIP_CHECK(
        hipMemset(d_track_counts_, 0, 2 * sizeof(unsigned long long)));
  }

  void launch_tally_tracks(int64_t n, const double *origin, const double *dest,
                           const double *weights, const uint16_t *groups,
                           const double *resp) {
    const TrackMesh trk{
        d_planes_,
        d_planes32_,
        d_nbr_,
        grid_view_,
        FaceGridView{grid_view_.nx, grid_view_.ny, grid_view_.nz,
                     grid_view_.lo, grid_view_.inv_h, d_face_start_,
                     d_face_list_},
        d_face_bc_,
        d_pidx_,
        d_pelem_,
        d_pshift_,
        reflective,
        loc_tol_,
        max_steps > 0 ? max_steps : default_max_steps(mesh_)};
    using M = TallyMode;
    const auto kernel =
        linear ? (walk_fp32 ? k_tally_tracks<true, M::Linear>
                            : k_tally_tracks<false, M::Linear>)
        : face_currents
            ? (walk_fp32 ? k_tally_tracks<true, M::Currents>
                         : k_tally_tracks<false, M::Currents>)
            : (walk_fp32 ? k_tally_tracks<true, M::Flux>
                         : k_tally_tracks<false, M::Flux>);
    kernel<<<grid_blocks(n), kBlock, 0, s_comp_>>>(
        trk, origin, dest, weights, groups, resp, d_flux_,
        linear ? d_moments_.get() : d_cur_.get(), d_inv_h_, d_track_counts_,
        d_lost_, d_lostrec_, d_loose_, n, ngroups, mesh_.nelems, nscores);
    PT_HIP_CHECK(hipGetLastError());
    stats_.tracks += n;
  }

  // Persistent scratch for walk_raw.  The partitioned driver calls
  // walk_raw once per exchange round; per-call hipMalloc/hipFree pairs
  // would device-sync every round, so the buffers are grown once and
  // reused (released with the engine).
  struct WalkRawScratch {
    int64_t cap = 0;
    DeviceBuffer<double> pos, dest, w, out_pos, resp, out_dest;
    DeviceBuffer<int32_t> elem, out_elem;
    DeviceBuffer<int8_t> status;
    DeviceBuffer<uint16_t> groups;
    DeviceBuffer<double> in_t, out_o, out_t;
    DeviceBuffer<int32_t> in_prev, out_prev;
  };

  void ensure_wr_cap(int64_t n, bool need_groups, bool need_resp) {
    if (n > wr_.cap) {
      wr_ = WalkRawScratch{}; // drops the optional buffers too
      const int64_t cap = n + n / 4; // headroom against round-to-round growth
      wr_.pos.allocate(cap * 3);
      wr_.dest.allocate(cap * 3);
      wr_.w.allocate(cap);
      wr_.out_pos.allocate(cap * 3);
      wr_.elem.allocate(cap);
      wr_.out_elem.allocate(cap);
      wr_.status.allocate(cap);
      wr_.cap = cap;
    }
    if (need_groups && !wr_.groups) wr_.groups.allocate(wr_.cap);
    if (need_resp && !wr_.resp) wr_.resp.allocate(wr_.cap * nscores);
  }

  void walk_raw(int64_t n, const double *pos, const double *dest,
                const int32_t *elem, const double *weights, double *out_pos,
                int32_t *out_elem, int8_t *out_status,
                const uint16_t *groups = nullptr,
                const double *responses = nullptr,
                double *out_dest = nullptr, const double *in_t = nullptr,
                const int32_t *in_prev = nullptr, double *out_o = nullptr,
                double *out_t = nullptr,
                int32_t *out_prev = nullptr) override {
    if (n == 0) return;
    PT_HIP_CHECK(hipSetDevice(device_));
    ensure_wr_cap(n, groups != nullptr, responses != nullptr);
    const bool resume = in_t || in_prev || out_o || out_t || out_prev;
    if (resume && !wr_.in_t) {
      wr_.in_t.allocate(wr_.cap);
      wr_.in_prev.allocate(wr_.cap);
      wr_.out_o.allocate(wr_.cap * 3);
      wr_.out_t.allocate(wr_.cap);
      wr_.out_prev.allocate(wr_.cap);
    }
    if (in_t)
      PT_HIP_CHECK(hipMemcpy(wr_.in_t, in_t, n * 8, hipMemcpyHostToDevice));
    if (in_prev)
      PT_HIP_CHECK(hipMemcpy(wr_.in_prev, in_prev, n * 4,
                             hipMemcpyHostToDevice));
    // Previous round's kernel has been synchronized below before this
    // call returns, so the scratch is free for reuse here.
    PT_HIP_CHECK(hipMemcpy(wr_.pos, pos, n * 3 * 8, hipMemcpyHostToDevice));
    PT_HIP_CHECK(hipMemcpy(wr_.dest, dest, n * 3 * 8, hipMemcpyHostToDevice));
    PT_HIP_CHECK(hipMemcpy(wr_.w, weights, n * 8, hipMemcpyHostToDevice));
    PT_HIP_CHECK(hipMemcpy(wr_.elem, elem, n * 4, hipMemcpyHostToDevice));
    const uint16_t *dg = groups ? wr_.groups : nullptr;
    const double *dr = responses ? wr_.resp : nullptr;
    if (groups)
      PT_HIP_CHECK(hipMemcpy(wr_.groups, groups, n * 2, hipMemcpyHostToDevice));
    if (responses)
      PT_HIP_CHECK(hipMemcpy(wr_.resp, responses, n * nscores * 8,
                             hipMemcpyHostToDevice));
    if (out_dest && !wr_.out_dest) wr_.out_dest.allocate(wr_.cap * 3);
    launch_walk_raw(n, wr_.pos, wr_.dest, wr_.elem, wr_.w, wr_.out_pos,
                    wr_.out_elem, wr_.status, dg, dr,
                    out_dest ? wr_.out_dest : nullptr,
                    in_t ? wr_.in_t : nullptr,
                    in_prev ? wr_.in_prev : nullptr,
                    out_o ? wr_.out_o : nullptr, out_t ? wr_.out_t : nullptr,
                    out_prev ? wr_.out_prev : nullptr);
    PT_HIP_CHECK(hipStreamSynchronize(s_comp_));
    PT_HIP_CHECK(hipMemcpy(out_pos, wr_.out_pos, n * 3 * 8,
                           hipMemcpyDeviceToHost));
    PT_HIP_CHECK(hipMemcpy(out_elem, wr_.out_elem, n * 4,
                           hipMemcpyDeviceToHost));
    PT_HIP_CHECK(hipMemcpy(out_status, wr_.status, n, hipMemcpyDeviceToHost));
    if (out_dest)
      PT_HIP_CHECK(hipMemcpy(out_dest, wr_.out_dest, n * 3 * 8,
                             hipMemcpyDeviceToHost));
    if (out_o)
      PT_HIP_CHECK(hipMemcpy(out_o, wr_.out_o, n * 3 * 8,
                             hipMemcpyDeviceToHost));
    if (out_t)
      PT_HIP_CHECK(hipMemcpy(out_t, wr_.out_t, n * 8,
                             hipMemcpyDeviceToHost));
    if (out_prev)
      PT_HIP_CHECK(hipMemcpy(out_prev, wr_.out_prev, n * 4,
                             hipMemcpyDeviceToHost));
  }

  void walk_raw_device(int64_t n, const double *d_pos, const double *d_dest,
                       const int32_t *d_elem, const double *d_weights,
                       double *d_out_pos, int32_t *d_out_elem,
                       int8_t *d_out_status,
                       const uint16_t *d_groups = nullptr,
                       const double *d_responses = nullptr,
                       double *d_out_dest = nullptr,
                       const double *d_in_t = nullptr,
                       const int32_t *d_in_prev = nullptr,
                       double *d_out_o = nullptr, double *d_out_t = nullptr,
                       int32_t *d_out_prev = nullptr) override {
    if (n == 0) return;
    PT_HIP_CHECK(hipSetDevice(device_));
    launch_walk_raw(n, d_pos, d_dest, d_elem, d_weights, d_out_pos, d_out_elem,
                    d_out_status, d_groups, d_responses, d_out_dest, d_in_t,
                    d_in_prev, d_out_o, d_out_t, d_out_prev);
    PT_HIP_CHECK(hipStreamSynchronize(s_comp_));
  }

  void end_batch() override {
    PT_HIP_CHECK(hipSetDevice(device_));
    sync();
    const int64_t fsz = fsz_;
    if (slices_ > 1) {
      k_reduce_slices<<<grid_blocks(fsz), kBlock, 0, s_comp_>>>(d_flux_, fsz,
                                                               slices_);
      PT_HIP_CHECK(hipGetLastError());
    }
    close_batch(d_flux_, d_bsum_, &d_bsq_, fsz);
    // there is no sum of squares for the moments
    if (linear) close_batch(d_moments_, d_msum_, nullptr, fsz * 4);
    if (face_currents) close_batch(d_cur_, d_csum_, &d_csq_, fsz * 4);
    if (collision_tallies) close_batch(d_coll_, d_collsum_, &d_collsq_, fsz);
    PT_HIP_CHECK(hipStreamSynchronize(s_comp_));
    nbatches_++;
  }

  // end_batch() for one tally array: add it into its running sum (and sum of
  // squares, when it keeps one), then zero it.  The sums are allocated on
  // first use.
  void close_batch(double *tally, DeviceBuffer<double> &sum,
                   DeviceBuffer<double> *sq, int64_t count) {
    for (DeviceBuffer<double> *acc : {&sum, sq})
      if (acc && !*acc) {
        acc->allocate(count);
        PT_HIP_CHECK(hipMemset(*acc, 0, count * sizeof(double)));
      }
    if (sq)
      k_accumulate_batch<<<grid_blocks(count), kBlock, 0, s_comp_>>>(
          tally, sum, *sq, count);
    else
      k_accumulate_moments<<<grid_blocks(count), kBlock, 0, s_comp_>>>(
          tally, sum, count);
    PT_HIP_CHECK(hipGetLastError());
  }
  std::vector<double> batch_sum() const override {
    return fetch_tally(d_bsum_, fsz_);
  }
  std::vector<double> batch_sum_sq() const override {
    return fetch_tally(d_bsq_, fsz_);
  }
  int64_t num_batches() const override { return nbatches_; }

  // Readback of an un-sliced tally array: the batch sums [fsz_], the
  // moments, the currents and their batch sums [fsz_*4].  A null array (not
  // allocated before the first end_batch) reads as zeros.
  std::vector<double> fetch_tally(const double *p, int64_t count) const {
    std::vector<double> out(count, 0.0);
    if (p) {
      sync();
      PT_HIP_CHECK(hipMemcpy(out.data(), p, count * sizeof(double),
                             hipMemcpyDeviceToHost));
    }
    return out;
  }
  // Upload of a whole [fsz_*4] array (moments or currents).
  void set_tally4(double *dst, const double *src, int64_t n,
                  const char *mismatch) {
    if (n != fsz_ * 4) throw std::runtime_error(mismatch);
    sync();
    PT_HIP_CHECK(hipMemcpy(dst, src, n * sizeof(double),
                           hipMemcpyHostToDevice));
  }

  std::vector<double> flux() const override {
    sync();
    const int64_t fsz = fsz_;
    if (slices_ > 1) {
      k_reduce_slices<<<grid_blocks(fsz), kBlock, 0, s_comp_>>>(d_flux_, fsz,
                                                               slices_);
      PT_HIP_CHECK(hipGetLastError());
      PT_HIP_CHECK(hipStreamSynchronize(s_comp_));
    }
    std::vector<double> out(fsz);
    PT_HIP_CHECK(hipMemcpy(out.data(), d_flux_, fsz * sizeof(double),
                           hipMemcpyDeviceToHost));
    return out;
  }

  std::vector<double> moments() const override {
    if (!linear) throw_not_linear();
    return fetch_tally(d_moments_, fsz_ * 4);
  }
  std::vector<double> moment_sum() const override {
    if (!linear) throw_not_linear();
    return fetch_tally(d_msum_, fsz_ * 4);
  }
  void set_moments(const double *m, int64_t n) override {
    if (!linear) throw_not_linear();
    set_tally4(d_moments_, m, n, "set_moments size mismatch");
  }

  std::vector<double> currents() const override {
    if (!face_currents) throw_not_currents();
    return fetch_tally(d_cur_, fsz_ * 4);
  }
  std::vector<double> current_sum() const override {
    if (!face_currents) throw_not_currents();
    return fetch_tally(d_csum_, fsz_ * 4);
  }
  std::vector<double> current_sum_sq() const override {
    if (!face_currents) throw_not_currents();
    return fetch_tally(d_csq_, fsz_ * 4);
  }
  void set_currents(const double *j, int64_t n) override {
    if (!face_currents) throw_not_currents();
    set_tally4(d_cur_, j, n, "set_currents size mismatch");
  }

  std::vector<double> collisions() const override {
    if (!collision_tallies) throw_not_collisions();
    return fetch_tally(d_coll_, fsz_);
  }
  std::vector<double> collision_sum() const override {
    if (!collision_tallies) throw_not_collisions();
    return fetch_tally(d_collsum_, fsz_);
  }
  std::vector<double> collision_sum_sq() const override {
    if (!collision_tallies) throw_not_collisions();
    return fetch_tally(d_collsq_, fsz_);
  }
  void set_collisions(const double *c, int64_t n) override {
    if (!collision_tallies) throw_not_collisions();
    if (n != fsz_) throw std::runtime_error("set_collisions size mismatch");
    sync();
    PT_HIP_CHECK(hipMemcpy(d_coll_, c, n * sizeof(double),
                           hipMemcpyHostToDevice));
  }

  std::vector<int32_t> elem_ids() const override {
    auto [s2c, elem] = fetch<int32_t>(d_elem_, 1);
    std::vector<int32_t> out(n_);
    for (int64_t i = 0; i < n_; ++i) out[s2c[i]] = elem[i];
    return out;
  }
  std::vector<double> positions() const override {
    auto [s2c, pos] = fetch<double>(d_pos_, 3);
    std::vector<double> out(n_ * 3);
    for (int64_t i = 0; i < n_; ++i)
      for (int k = 0; k < 3; ++k) out[(int64_t)s2c[i] * 3 + k] = pos[i * 3 + k];
    return out;
  }
  std::vector<uint8_t> escaped() const override {
    auto [s2c, esc] = fetch<uint8_t>(d_escaped_, 1);
    std::vector<uint8_t> out(n_);
    for (int64_t i = 0; i < n_; ++i) out[s2c[i]] = esc[i];
    return out;
  }

  const EngineStats &stats() const override {
    sync();
    unsigned long long lost = 0, loose = 0;
    PT_HIP_CHECK(hipMemcpy(&lost, d_lost_, sizeof lost, hipMemcpyDeviceToHost));
    PT_HIP_CHECK(
        hipMemcpy(&loose, d_loose_, sizeof loose, hipMemcpyDeviceToHost));
    stats_.lost_particles = (int64_t)lost;
    stats_.loose_localizations = (int64_t)loose;
    if (collision_tallies) {
      unsigned long long c[2] = {0, 0};
      PT_HIP_CHECK(
          hipMemcpy(c, d_coll_counts_, sizeof c, hipMemcpyDeviceToHost));
      stats_.collisions_scored = (int64_t)c[0];
      stats_.collision_misses = (int64_t)c[1];
    }
    if (d_track_counts_) {
      unsigned long long c[2] = {0, 0};
      PT_HIP_CHECK(
          hipMemcpy(c, d_track_counts_, sizeof c, hipMemcpyDeviceToHost));
      stats_.track_entries = (int64_t)c[0];
      stats_.track_misses = (int64_t)c[1];
    }
    return stats_;
  }

  std::vector<double> lost_records() const override {
    sync();
    unsigned long long lost = 0;
    PT_HIP_CHECK(hipMemcpy(&lost, d_lost_, sizeof lost, hipMemcpyDeviceToHost));
    const int64_t k = std::min<int64_t>((int64_t)lost, kMaxLostRecords);
    std::vector<double> out((size_t)k * 4);
    if (k)
      PT_HIP_CHECK(hipMemcpy(out.data(), d_lostrec_, k * 4 * sizeof(double),
                             hipMemcpyDeviceToHost));
    return out;
  }

  void set_flux(const double *f, int64_t ne) override {
    if (ne != fsz_)
      throw std::runtime_error("set_flux size mismatch");
    sync();
    PT_HIP_CHECK(hipMemset(d_flux_, 0, ne * slices_ * sizeof(double)));
    PT_HIP_CHECK(hipMemcpy(d_flux_, f, ne * sizeof(double), hipMemcpyHostToDevice));
  }

  void set_particle_state(const double *pos, const int32_t *elem,
                          const uint8_t *escaped, int64_t n) override {
    check_n(n);
    PT_HIP_CHECK(hipSetDevice(device_));
    sync();
    // caller order -> identity map; next move's cadence re-sorts
    k_iota<<<grid_blocks(n_), kBlock, 0, s_comp_>>>(d_s2c_, n_);
    PT_HIP_CHECK(hipGetLastError());
    PT_HIP_CHECK(hipStreamSynchronize(s_comp_));
    PT_HIP_CHECK(hipMemcpy(d_pos_, pos, n * 3 * sizeof(double), hipMemcpyHostToDevice));
    PT_HIP_CHECK(hipMemcpy(d_elem_, elem, n * sizeof(int32_t), hipMemcpyHostToDevice));
    PT_HIP_CHECK(hipMemcpy(d_escaped_, escaped, n, hipMemcpyHostToDevice));
    moves_since_sort_ = sort_every_; // re-sort on the next move
  }

  void synchronize() override { sync(); }

  bool device_mesh(DeviceMeshView *out) const override {
    out->planes = d_planes_;
    out->nbr = d_nbr_;
    out->grid = grid_view_;
    out->stream = (void *)s_comp_;
    return true;
  }

private:
  void check_n(int64_t n) const {
    if (n != n_) throw std::runtime_error("particle count mismatch");
  }

  void sync() const {
    PT_HIP_CHECK(hipStreamSynchronize(s_copy_));
    PT_HIP_CHECK(hipStreamSynchronize(s_comp_));
  }

  // Async H2D from caller memory.  No implicit hipHostRegister: a
  // registration cache outliving freed caller buffers poisons the
  // runtime's pinning table for unrelated later copies.  Pinned sources
  // copy at full link rate; pageable sources take the runtime's internal
  // staging path -- always correct, just slower.
  void stage(const void *src, size_t bytes, void *dst, hipStream_t s) {
    PT_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
  }

  // Everything a move stages besides the origins, into buffer set p.
  void stage_inputs(int p, const double *dest, const int8_t *flying,
                    const double *weights, const uint16_t *groups,
                    const double *responses, int64_t n) {
    stage(dest, n * 3 * sizeof(double), d_dest_[p], s_copy_);
    stage(flying, n * sizeof(int8_t), d_flying_[p], s_copy_);
    stage(weights, n * sizeof(double), d_weights_[p], s_copy_);
    if (groups && d_groups_[p])
      stage(groups, n * sizeof(uint16_t), d_groups_[p], s_copy_);
    if (responses)
      stage(responses, n * nscores * sizeof(double), d_resp_[p], s_copy_);
  }

  // ---- origin elision ---------------------------------------------------
  //
  // The headline move() is bound by the host-to-device link, and 240 of its
  // 570 MB are origins that, in steady state, are bit for bit the
  // destinations the previous move() staged -- still in d_dest_[p^1].
  // stage_elided() builds d_origin_[p] on device instead:
  //   1. k_copy_doubles: d_origin_[p] := d_dest_[p^1]       (HBM only)
  //   2. per host chunk, the origins the host delta pass found NOT
  //      bit-identical to its shadow of the previous dest are uploaded as a
  //      patch list and scattered over the copy (or, when more than half
  //      of the chunk changed, the chunk's origins are uploaded whole).
  // Every particle's 24 origin bytes in d_origin_[p] are therefore exactly
  // the caller's: from the patch/whole upload, or from a device copy of a
  // value the host proved bit-identical.  k_move is untouched and no
  // particle state is consulted, so results cannot change.
  //
  // Ordering (everything below is enqueued on s_copy_, in this order,
  // after move()'s wait on kernels_done_[p]):
  //   * d_origin_[p] writers (copy kernel, scatters, whole-chunk uploads):
  //     its last readers are the k_move launches of the move two calls
  //     ago, which kernels_done_[p] covers -- the same fence the plain
  //     origin upload relies on.  Scatter / whole-chunk upload follow the
  //     copy kernel in stream order, so they overwrite it, never the
  //     reverse; a scatter follows its own patch upload in stream order.
  //   * d_dest_[p^1] reader (copy kernel): its writer is the previous
  //     move's dest upload, earlier on s_copy_ (and complete: move() only
  //     returns after hipStreamSynchronize(s_copy_)).  Its next writer is
  //     the NEXT move's dest upload, later on s_copy_.  So the copy kernel
  //     sees exactly the previous destinations.  This is why the copy runs
  //     here and k_move never reads d_dest_[p^1] itself: the next move's
  //     copies wait only for the kernels of two moves ago and would
  //     overwrite the buffer under a k_move still reading it.
  //   * patch buffers (d_patch_idx_/d_patch_xyz_, single set): written by
  //     uploads and read by scatters on s_copy_ only, so stream order
  //     serializes reuse across chunks and across moves.  The pinned host
  //     side gives every chunk its own region, so workers filling chunk
  //     c+1's patch never touch memory the DMA engine is still reading for
  //     chunk c.
  //   * s_comp_ waits on copy_ev_[p], recorded after all of the above.
  //   * caller memory: the pass reads origin/dest synchronously; the
  //     async copies that read caller memory are all on s_copy_, which
  //     move() synchronizes before returning, as before.  The shadow is a
  //     real copy, so the caller may scribble over dest right after.
  // Validity: shadow_valid_ is only ever set by a move() that staged the
  // shadow's contents into d_dest_[parity of that move]; the next move()
  // has the opposite parity, so d_dest_[p^1] is that buffer.  The only
  // writers of d_dest_ are move()/move_continue() (one code path); the
  // plain path clears shadow_valid_.  move_device, copy_initial_position
  // (stages into d_origin_[0] after a full sync), set_particle_state and
  // the re-sort never touch d_dest_, and d_origin_[p] is rebuilt in full
  // by every move that reads it.
  static constexpr int kElideBackoffFirst = 16;
  static constexpr int kElideBackoffMax = 256;

  static double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() -
                                         t0)
        .count();
  }

  int64_t elide_chunk(int64_t n) const {
    if (origin_chunk > 0) return std::max<int64_t>(origin_chunk, 64);
    // Two chunks: the first half's patches upload while the second half is
    // compared, and the whole-upload fallback is decided per half.  Every
    // chunk costs one wake-up of the worker pool, bounded by its slowest
    // thread; swept on MI355X, n/2 beat n/8 and n/32 (profiles/README.md).
    return std::max<int64_t>((int64_t)262144, (n + 1) / 2);
  }

  void ensure_elide_host(int64_t n) {
    const int want = origin_delta_clamp_threads(origin_threads);
    if (!delta_pool_ || delta_pool_->nthreads() != want)
      delta_pool_ = std::make_unique<OriginDeltaPool>(want);
    if (!shadow_) shadow_.reset(new double[n * 3]);
  }

  void ensure_patch(int64_t need) {
    if (need <= patch_cap_) return;
    PT_HIP_CHECK(hipStreamSynchronize(s_copy_)); // scatters may still read
    patch_cap_ = 0;
    h_patch_idx_.reset();
    h_patch_xyz_.reset();
    d_patch_idx_.reset();
    d_patch_xyz_.reset();
    h_patch_idx_.allocate(need);
    h_patch_xyz_.allocate(need * 3);
    d_patch_idx_.allocate(need);
    d_patch_xyz_.allocate(need * 3);
    patch_cap_ = need;
  }

  void stage_elided(int p, const double *origin, const double *dest,
                    const int8_t *flying, const double *weights,
                    const uint16_t *groups, const double *responses,
                    int64_t n) {
    ensure_elide_host(n);
    const int nthreads = delta_pool_->nthreads();
    const int64_t chunk = elide_chunk(n);
    int64_t need = 0;
    for (int64_t lo = 0; lo < n; lo += chunk)
      need += origin_delta_patch_capacity(std::min(chunk, n - lo), nthreads);
    ensure_patch(need);
    shadow_valid_ = false; // until every chunk's shadow has been refreshed
    k_copy_doubles<<<grid_blocks(n * 3 / 2), kBlock, 0, s_copy_>>>(
        d_dest_[p ^ 1], d_origin_[p], n * 3);
    PT_HIP_CHECK(hipGetLastError());
    // None of these depends on the host pass, so they go first and whole:
    // the DMA engine has its ~330 MB queued before the first compare
    // starts and the entire pass, first chunk included, runs in its shadow.
    // (Measured on MI355X: interleaving per-chunk slices of these copies
    // with the pass averaged 8.05 ms/step over a thread x chunk sweep,
    // this order 7.05; profiles/README.md.)
    stage_inputs(p, dest, flying, weights, groups, responses, n);
    int64_t region = 0, uploaded = 0;
    for (int64_t lo = 0; lo < n; lo += chunk) {
      const int64_t hi = std::min(n, lo + chunk);
      const int64_t len = hi - lo;
      const int64_t cap = origin_delta_patch_capacity(len, nthreads);
      if (region + cap > patch_cap_)
        throw std::runtime_error("origin elision: patch region overflow");
      int32_t *hidx = h_patch_idx_ + region;
      double *hxyz = h_patch_xyz_ + region * 3;
      // Synchronous on the host; the copies enqueued above (and the
      // patches of earlier chunks) keep the DMA engine busy meanwhile.
      const auto t0 = std::chrono::steady_clock::now();
      const OriginDeltaResult r = origin_delta_pass(
          *delta_pool_, origin, dest, shadow_.get(), lo, hi, hidx, hxyz,
          /*nontemporal=*/false);
      stats_.origin_pass_seconds += seconds_since(t0);
      if (r.overflow || r.changed * 2 > len) {
        // a patch entry (28 B) costs more than the origin it replaces
        stage(origin + lo * 3, len * 3 * sizeof(double),
              d_origin_[p] + lo * 3, s_copy_);
        uploaded += len;
      } else if (r.changed > 0) {
        origin_delta_compact(r, hidx, hxyz);
        stage(hidx, r.changed * sizeof(int32_t), d_patch_idx_ + region,
              s_copy_);
        stage(hxyz, r.changed * 3 * sizeof(double),
              d_patch_xyz_ + region * 3, s_copy_);
        k_scatter_origins<<<grid_blocks(r.changed), kBlock, 0, s_copy_>>>(
            d_patch_idx_ + region, d_patch_xyz_ + region * 3, d_origin_[p],
            r.changed);
        PT_HIP_CHECK(hipGetLastError());
        uploaded += r.changed;
      }
      region += cap;
    }
    stats_.origins_elided += n - uploaded;
    stats_.origin_bytes_uploaded += uploaded * 3 * (int64_t)sizeof(double);
    shadow_valid_ = true;
    // Adaptive back-off: a workload that resamples (nearly) everything
    // gains nothing from the host pass.  Skip it for the next few moves
    // (plain uploads, shadow left invalid), then seed and probe again,
    // doubling the pause each time the probe fails.
    if (uploaded * 2 > n) {
      elide_skip_ = elide_backoff_;
      elide_backoff_ = std::min(elide_backoff_ * 2, kElideBackoffMax);
    } else {
      elide_backoff_ = kElideBackoffFirst;
    }
  }

  // The k_walk_raw launch of walk_raw and walk_raw_device (device pointers,
  // argument order of walk_raw_device).
  void launch_walk_raw(int64_t n, const double *pos, const double *dest,
                       const int32_t *elem, const double *weights,
                       double *out_pos, int32_t *out_elem, int8_t *out_status,
                       const uint16_t *groups, const double *resp,
                       double *out_dest, const double *in_t,
                       const int32_t *in_prev, double *out_o, double *out_t,
                       int32_t *out_prev) {
    const int steps = max_steps > 0 ? max_steps : default_max_steps(mesh_);
    const auto kernel =
        linear ? (walk_fp32 ? k_walk_raw<true, true> : k_walk_raw<false, true>)
        : face_currents
            ? (walk_fp32 ? k_walk_raw<true, false, true>
                         : k_walk_raw<false, false, true>)
            : (walk_fp32 ? k_walk_raw<true> : k_walk_raw<false>);
    kernel<<<grid_blocks(n), kBlock, 0, s_comp_>>>(
        d_planes_, d_planes32_, d_nbr_, pos, dest, elem, weights, groups, resp,
        out_pos, out_elem, out_status, out_dest, d_flux_, d_lost_, d_lostrec_,
        n, steps, reflective, d_face_bc_, ngroups, mesh_.nelems, nscores,
        d_pidx_, d_pelem_, d_pshift_, in_t, in_prev, out_o, out_t, out_prev,
        d_inv_h_, d_moments_, d_cur_);
    PT_HIP_CHECK(hipGetLastError());
  }

  // The k_move instantiation of a move.  Scored / periodic / wave-aggregated
  // / linear / currents moves take dedicated instantiations; the plain
  // (headline) one compiles without any of those features.  The tally arm
  // is scored when responses are passed, else wave-aggregated when `agg`,
  // else plain atomics; linear and face-current engines take their mode's
  // instantiation of whichever arm and traversal the move would otherwise
  // get.  All instantiations share one signature, so they fit one table.
  using MoveKernel = decltype(&k_move<false>);
  enum MoveArm { kArmPlain, kArmWave, kArmScored };
  template <bool Linear, bool Currents>
  static MoveKernel move_kernel(bool f32, bool per, MoveArm arm) {
#define PT_MOVE_ARMS(F32, PER)                                               \
  {                                                                          \
    k_move<F32, false, PER, false, Linear, Currents>,                        \
        k_move<F32, false, PER, true, Linear, Currents>,                     \
        k_move<F32, true, PER, false, Linear, Currents>                      \
  }
    static constexpr MoveKernel table[2][2][3] = {
        {PT_MOVE_ARMS(false, false), PT_MOVE_ARMS(false, true)},
        {PT_MOVE_ARMS(true, false), PT_MOVE_ARMS(true, true)}};
#undef PT_MOVE_ARMS
    return table[f32][per][arm];
  }

  void launch_move_chunks(const double *origin, const double *dest,
                          const int8_t *flying, const double *weights,
                          const uint16_t *groups, const double *resp,
                          int64_t n, int steps) {
    const bool per = d_pidx_ != nullptr;
    // wave aggregation needs a single flat tally key per lane: plain
    // (unscored, ungrouped) moves only
    const bool agg = wave_agg() && !resp && !groups;
    const MoveArm arm = resp ? kArmScored : (agg ? kArmWave : kArmPlain);
    const MoveKernel kernel =
        linear          ? move_kernel<true, false>(walk_fp32, per, arm)
        : face_currents ? move_kernel<false, true>(walk_fp32, per, arm)
                        : move_kernel<false, false>(walk_fp32, per, arm);
    // Chunked launches: a ~2.6M-slot launch keeps each XCD's Morton-
    // contiguous slot range's mesh working set inside its private L2.
    const int64_t chunk = chunk_particles(n);
    for (int64_t lo = 0; lo < n; lo += chunk) {
      const int64_t hi = std::min(n, lo + chunk);
      kernel<<<grid_blocks(hi - lo), kBlock, 0, s_comp_>>>(
          d_planes_, d_planes32_, d_nbr_, grid_view_, d_s2c_, origin, dest,
          flying, weights, groups, ngroups, d_pos_, d_elem_, d_escaped_,
          d_flux_, d_lost_, d_lostrec_, d_loose_, lo, hi, loc_tol_, steps,
          mesh_.nelems, slices_ - 1, reflective, d_face_bc_, resp, nscores,
          d_pidx_, d_pelem_, d_pshift_, d_inv_h_, d_moments_, d_cur_,
          cur_keyed_);
      PT_HIP_CHECK(hipGetLastError());
    }
  }

  // Device Morton sort of particle slots by current position (hipCUB radix
  // sort); measured 2.2x on the walk for spatially random particle order.
  void spatial_sort() {
    k_morton_keys<<<grid_blocks(n_), kBlock, 0, s_comp_>>>(
        d_pos_, d_keys_, d_vals_, n_, mesh_.bbox_lo, sort_scale_);
    PT_HIP_CHECK(hipGetLastError());
    size_t bytes = sorttmp_bytes_;
    PT_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(
        d_sorttmp_, bytes, d_keys_.get(), d_keys2_.get(), d_vals_.get(),
        d_order_.get(), (int)n_, 0, 64, s_comp_));
    k_permute_state<<<grid_blocks(n_), kBlock, 0, s_comp_>>>(
        d_order_, d_pos_, d_elem_, d_escaped_, d_s2c_, d_pos2_, d_elem2_,
        d_esc2_, d_s2c2_, n_);
    PT_HIP_CHECK(hipGetLastError());
    std::swap(d_pos_, d_pos2_);
    std::swap(d_elem_, d_elem2_);
    std::swap(d_escaped_, d_esc2_);
    std::swap(d_s2c_, d_s2c2_);
  }

  void maybe_resort() {
    if (sort_every_ > 0 && ++moves_since_sort_ >= sort_every_) {
      spatial_sort();
      moves_since_sort_ = 0;
    }
  }

  // D2H of (s2c, state-array) for caller-order readback.
  template <class T>
  std::pair<std::vector<int32_t>, std::vector<T>> fetch(const T *dev,
                                                        int comps) const {
    sync();
    std::vector<int32_t> s2c(n_);
    std::vector<T> v(n_ * comps);
    PT_HIP_CHECK(hipMemcpy(s2c.data(), d_s2c_, n_ * sizeof(int32_t),
                           hipMemcpyDeviceToHost));
    PT_HIP_CHECK(hipMemcpy(v.data(), dev, n_ * comps * sizeof(T),
                           hipMemcpyDeviceToHost));
    return {std::move(s2c), std::move(v)};
  }

  Mesh mesh_;
  int64_t n_;
  int64_t fsz_ = 0; // nelems * ngroups * nscores
  int device_ = 0;
  double loc_tol_ = 1e-12;
  int slices_ = 1;
  int sort_every_ = 0;
  int64_t moves_since_sort_ = 0;
  uint64_t parity_ = 0;
  Vec3 sort_scale_{0, 0, 0};

  // Origin elision (stage_elided): host shadow of the dest staged by the
  // previous move() (3*n doubles, plain memory), compare workers, and the
  // patch list (pinned host + device, patch_cap_ entries of int32 + 3
  // doubles).  All allocated on first use.
  std::unique_ptr<double[]> shadow_;
  bool shadow_valid_ = false;
  std::unique_ptr<OriginDeltaPool> delta_pool_;
  int64_t patch_cap_ = 0;
  int elide_skip_ = 0;                     // plain moves left in a back-off
  int elide_backoff_ = kElideBackoffFirst; // length of the next back-off

  // Streams and events come before every buffer, so they are destroyed
  // after all of them.
  Stream s_copy_, s_comp_;
  std::array<Event, 2> copy_ev_;
  std::array<Event, 2> kernels_done_;
  // collision tallies only: score_collisions' upload stream and its fences
  Stream s_score_;
  Event score_copied_, score_done_;
  bool score_queued_ = false;

  PinnedBuffer<int32_t> h_patch_idx_;
  PinnedBuffer<double> h_patch_xyz_;
  DeviceBuffer<int32_t> d_patch_idx_;
  DeviceBuffer<double> d_patch_xyz_;

  DeviceBuffer<Plane> d_planes_;
  DeviceBuffer<Plane32> d_planes32_;
  DeviceBuffer<int32_t> d_nbr_, d_cell_start_, d_cell_tets_;
  GridView grid_view_{};

  DeviceBuffer<double> d_pos_;
  DeviceBuffer<int32_t> d_elem_;
  DeviceBuffer<uint8_t> d_escaped_;
  DeviceBuffer<int32_t> d_s2c_;
  DeviceBuffer<double> d_flux_;
  DeviceBuffer<unsigned long long> d_lost_, d_loose_;
  DeviceBuffer<double> d_lostrec_;
  DeviceBuffer<double> d_origin_[2], d_dest_[2], d_weights_[2], d_resp_[2];
  DeviceBuffer<int8_t> d_flying_[2];
  DeviceBuffer<uint16_t> d_groups_[2];
  DeviceBuffer<double> d_bsum_, d_bsq_;
  // Linear mode only (null otherwise): 1/heights, the un-sliced moments
  // [fsz_*4] and their end_batch running sum (allocated on first use).
  DeviceBuffer<double> d_inv_h_, d_moments_, d_msum_;
  // Face currents only (null otherwise): the un-sliced currents [fsz_*4]
  // and their end_batch sum / sum of squares (allocated on first use).
  DeviceBuffer<double> d_cur_, d_csum_, d_csq_;
  bool cur_keyed_ = false;
  // Collision tallies only (null otherwise): the un-sliced collisions
  // [fsz_], their end_batch sum / sum of squares (allocated on first use),
  // the {scored, missed} counters, score_collisions' staging buffers and
  // score_points' scratch (both allocated on first use).
  DeviceBuffer<double> d_coll_, d_collsum_, d_collsq_;
  DeviceBuffer<unsigned long long> d_coll_counts_;
  bool coll_agg_ = true;
  DeviceBuffer<int8_t> sc_active_;
  DeviceBuffer<double> sc_weights_, sc_resp_;
  DeviceBuffer<uint16_t> sc_groups_;
  ScorePointsScratch sp_;
  DeviceBuffer<uint32_t> d_face_bc_;
  DeviceBuffer<int32_t> d_pidx_, d_pelem_;
  DeviceBuffer<double> d_pshift_;
  WalkRawScratch wr_;
  // Track tallies only, all from the first tally_tracks call: the
  // boundary-face grid (CSR over grid_view_'s cells), the {entries, misses}
  // counters and the host path's scratch.
  DeviceBuffer<int32_t> d_face_start_, d_face_list_;
  DeviceBuffer<unsigned long long> d_track_counts_;
  bool tracks_refused_ = false;
  TrackScratch tt_;
  int64_t nbatches_ = 0;

  DeviceBuffer<uint64_t> d_keys_, d_keys2_;
  DeviceBuffer<int32_t> d_vals_, d_order_;
  DeviceBuffer<double> d_pos2_;
  DeviceBuffer<int32_t> d_elem2_;
  DeviceBuffer<uint8_t> d_esc2_;
  DeviceBuffer<int32_t> d_s2c2_;
  DeviceBuffer<unsigned char> d_sorttmp_;
  size_t sorttmp_bytes_ = 0;

  mutable EngineStats stats_;
};

} // namespace

std::unique_ptr<Engine> make_gpu_engine(Mesh mesh, int64_t num_particles,
                                        int device, int ngroups, int nscores,
                                        bool linear, bool currents,
                                        bool collisions) {
  check_tally_options(linear, currents);
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= device) {
    (void)hipGetLastError();
    return nullptr;
  }
  return std::make_unique<GpuEngine>(std::move(mesh), num_particles, device,
                                     ngroups, nscores, linear, currents,
                                     collisions);
}

} // namespace pumitally
