// The handoff record of the stateful partitioned engine: the ONE place
// its layout is defined.  Every writer and reader, on host and device,
// goes through HandoffLayout.
//
// A record is width() = 11 + carry_grp + nscores doubles:
//
//   [0]      gid         global particle id
//   [1..3]   pos         where the receiver starts from: the walk's current
//                        wrap-segment origin for a cut crossing, the
//                        resampled origin for a reroute
//   [4]      target gid  global id of the element to enter
//   [5..7]   dest        reflective/periodic restarts inside the walk
//                        mutate the destination, so it travels
//   [8]      w           weight
//   [9]      t           walk progress at the cut crossing (0: fresh walk)
//   [10]     prev gid    global id of the element exited from (-1: fresh)
//   [11]     group       only when carry_grp (ngroups > 1)
//   [..]     responses   nscores score multipliers (1.0 when none given)
//
// Carrying (pos, t, prev) instead of the crossing point lets the receiver
// resume with the sender's exact fp state, so partitioned flux attribution
// is elementwise identical to the replicated engine (walk.h walk_segment).
// Weight, group and responses travel because in the coupled-host mode
// (step_local) the receiver never saw the sender's input arrays; in the
// global-array mode the receiver scatters the (identical) carried values,
// so both modes share one code path.
//
// A departure-list entry is one record plus the destination OWNER rank in
// column [width()]: dep_width() doubles.  The owner column is dropped when
// entries are packed for the exchange.
#pragma once

#include "geom.h"

#include <cstdint>

namespace pumitally {

struct HandoffLayout {
  int nscores;
  bool carry_grp;

  enum : int { kGid = 0, kPos = 1, kTarget = 4, kDest = 5, kWeight = 8,
               kT = 9, kPrev = 10, kGroup = 11 };

  PT_HD int resp_at() const { return kGroup + (carry_grp ? 1 : 0); }
  PT_HD int width() const { return resp_at() + nscores; }
  PT_HD int dep_width() const { return width() + 1; }

  // Fills one departure entry.  resp == nullptr writes 1.0 multipliers.
  PT_HD void write(double *e, int64_t gid, Vec3 pos, int64_t target_gid,
                   Vec3 dest, double w, double t, int64_t prev_gid,
                   uint16_t grp, const double *resp, int owner) const {
    e[kGid] = (double)gid;
    e[kPos] = pos.x;
    e[kPos + 1] = pos.y;
    e[kPos + 2] = pos.z;
    e[kTarget] = (double)target_gid;
    e[kDest] = dest.x;
    e[kDest + 1] = dest.y;
    e[kDest + 2] = dest.z;
    e[kWeight] = w;
    e[kT] = t;
    e[kPrev] = (double)prev_gid;
    if (carry_grp) e[kGroup] = (double)grp;
    double *r = e + resp_at();
    for (int k = 0; k < nscores; ++k) r[k] = resp ? resp[k] : 1.0;
    e[width()] = (double)owner;
  }

  PT_HD int64_t gid(const double *e) const { return (int64_t)e[kGid]; }
  PT_HD Vec3 pos(const double *e) const {
    return Vec3{e[kPos], e[kPos + 1], e[kPos + 2]};
  }
  PT_HD int64_t target_gid(const double *e) const {
    return (int64_t)e[kTarget];
  }
  PT_HD Vec3 dest(const double *e) const {
    return Vec3{e[kDest], e[kDest + 1], e[kDest + 2]};
  }
  PT_HD double weight(const double *e) const { return e[kWeight]; }
  PT_HD double t(const double *e) const { return e[kT]; }
  PT_HD int64_t prev_gid(const double *e) const { return (int64_t)e[kPrev]; }
  PT_HD uint16_t group(const double *e) const {
    return carry_grp ? (uint16_t)e[kGroup] : (uint16_t)0;
  }
  PT_HD const double *responses(const double *e) const {
    return e + resp_at();
  }
  PT_HD int owner(const double *dep_entry) const {
    return (int)dep_entry[width()];
  }
};

} // namespace pumitally
