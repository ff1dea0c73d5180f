// The tally sink: what one crossing of the walk contributes, written once
// for both engines.  The CPU engine is the oracle of the HIP kernels, so its
// contribution code is this very text, not a hand-kept copy.
//
// A TallySink is the "face" form walk_contribute accepts (walk.h).  Per
// crossing it computes the flux value, in Linear mode the four barycentric
// moments, in Currents mode the face to book, and hands them -- once, or
// once per score -- to an ADDER POLICY that knows how a value reaches memory:
//   PlainAdder<HostPlus>   plain += (CPU engine)
//   PlainAdder<Plus>       any other per-value add; the HIP engine plugs in
//                          atomicAdd
//   a wave-aggregating adder, device-only, lives with the HIP engine
// An adder books one value at a time,
//   flux(flux, at, v)              flux[at] (+)= v
//   companion(array, at4, v)       array[at4] (+)= v
// and, when it declares kFusedMoments, a Linear crossing in one call,
//   moments(flux, mom, at, v, m)   flux[at], then mom[at*4 + 0..3]
// The flux always goes first, its `*4` companion (moments or currents) after
// it.  `at` is the flat flux index [score][group][element]; the index
// formula is here and nowhere else.
#pragma once

#include "walk.h"

namespace pumitally {

enum class TallyMode { Flux, Linear, Currents };

struct HostPlus {
  PT_HD void operator()(double *p, double v) const { *p += v; }
};

template <class Plus> struct PlainAdder {
  static constexpr bool kFusedMoments = false;
  Plus plus;
  PT_HD void flux(double *flux, int64_t at, double v) const {
    plus(&flux[at], v);
  }
  PT_HD void companion(double *array, int64_t at4, double v) const {
    plus(&array[at4], v);
  }
};

// Offset of a particle's energy group in the flux index (0 without groups).
PT_HD int64_t tally_group_offset(const uint16_t *__restrict__ groups,
                                 int64_t particle, int ngroups,
                                 int64_t nelems) {
  return groups ? (int64_t)(groups[particle] % ngroups) * nelems : 0;
}

// A point score (Engine::score_collisions / score_points): what one scoring
// particle or free point, sitting in element `el` with weight `w`, adds to
// the flux-shaped `array`.  No track and no mesh data enter.  Scores and
// groups apply as in the walk sink: with `resp`, score k gets
// w * resp[particle*nscores + k] at k*gsz + goff + el; without, score 0 alone
// gets w.  `goff` is tally_group_offset of the particle, `gsz` the score
// stride ngroups*nelems.  Values go through Adder::flux, so any adder of the
// walk sink serves.
template <class Adder>
PT_HD void score_contribute(const Adder &add, double *array, int64_t goff,
                            int64_t gsz, int32_t el, double w,
                            const double *__restrict__ resp, int64_t particle,
                            int nscores) {
  if (resp) {
    for (int k = 0; k < nscores; ++k)
      add.flux(array, k * gsz + goff + el, w * resp[particle * nscores + k]);
    return;
  }
  add.flux(array, goff + el, w);
}

// The mesh arrays the Linear and Currents modes read; Flux reads none.
struct TallyMesh {
  const Plane *planes;     // Linear
  const double *inv_h;     // Linear: Mesh::inv_heights
  const int32_t *nbr;      // Currents with the re-exit rule, as are:
  const uint32_t *face_bc;
  const int32_t *pidx;
  bool reflective;
};

// One particle's sink.  Compile-time switches:
//   Scored      false: `resp` is never looked at and no score loop is
//               compiled; true: a non-null `resp` scores every contribution
//               nscores times, value * resp[particle*nscores + k], scores
//               the OUTER loop (per score: flux, then its companion).
//   ReexitRule  Currents only: apply walk_current_face (an escaped particle
//               leaving again where it sits is one departure).  move() does;
//               walk_raw has no particle state and does not.
//   Periodic    forwarded to walk_current_face.
// The flux value is (t1 - t0) * seg_len * weight -- the expression the
// legacy callback form receives -- in every mode, so flux is bit-identical
// whatever else is tallied.
template <TallyMode Mode, bool Scored, class Adder, bool ReexitRule = false,
          bool Periodic = false>
struct TallySink {
  Adder add;
  double *flux;
  double *companion; // moments (Linear) or currents (Currents), [flux size*4]
  int64_t goff;      // tally_group_offset of this particle
  int64_t gsz;       // ngroups * nelems, the score stride
  const double *resp;
  int64_t particle; // row of `resp`
  int nscores;
  TallyMesh mesh;
  bool reexit; // ReexitRule: the particle entered this move flagged escaped

  PT_HD void operator()(int32_t el, double t0, double t1, const WalkState &s,
                        int exit_face) {
    if constexpr (Mode == TallyMode::Currents && ReexitRule)
      exit_face =
          walk_current_face<Periodic>(reexit, mesh.nbr, el, exit_face, t1,
                                      mesh.reflective, mesh.face_bc, mesh.pidx);
    const double v = (t1 - t0) * s.seg_len * s.weight;
    double m[4];
    if constexpr (Mode == TallyMode::Linear)
      tet_moments(mesh.planes + (int64_t)el * 4, mesh.inv_h + (int64_t)el * 4,
                  s, t0, t1, v, m);
    if constexpr (Scored) {
      if (resp) {
        for (int k = 0; k < nscores; ++k)
          book<true>(k * gsz + goff + el, resp[particle * nscores + k], v, m,
                     exit_face, s.weight);
        return;
      }
    }
    book<false>(goff + el, 1.0, v, m, exit_face, s.weight);
  }

private:
  // One score's adds at flux index `at`; Scaled: every value times r.
  template <bool Scaled>
  PT_HD void book(int64_t at, double r, double v, const double (&m)[4],
                  int face, double w) {
    if constexpr (Mode == TallyMode::Linear && Adder::kFusedMoments &&
                  !Scaled) {
      add.moments(flux, companion, at, v, m);
      return;
    }
    add.flux(flux, at, Scaled ? v * r : v);
    if constexpr (Mode == TallyMode::Linear) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int f = 0; f < 4; ++f)
        add.companion(companion, at * 4 + f, Scaled ? m[f] * r : m[f]);
    }
    if constexpr (Mode == TallyMode::Currents)
      if (face >= 0) add.companion(companion, at * 4 + face, Scaled ? w * r : w);
  }
};

} // namespace pumitally
