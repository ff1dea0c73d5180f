// Stateless track tallies: one free segment (o -> d, weight w) against a
// mesh that need not contain its end points.  The track may start outside,
// enter through a vacuum boundary face, leave through a hole or a notch and
// come back, or miss the mesh altogether (Engine::tally_tracks).
//
// Inside the mesh the track is the ordinary walk (walk.h walk_advance /
// walk_advance32, Periodic=true); what is new is the ENTRY SEARCH ray_enter:
// the first vacuum boundary face the segment crosses inwards at or after a
// given parameter.  The segment keeps ONE parametrization over the caller's
// (o, d) for its whole life -- a found entry only sets the walk's element and
// t_cur, nothing is rebased -- so every in-mesh crossing has the very t0, t1
// a walk through a mesh that also filled the voids would compute (shared
// planes are bitwise-consistent and t = vo / (vo - vd) is the expression
// walk_advance evaluates on the twin face).  Only reflective and periodic
// restarts rebase (s.o, s.d), as they always did; the search then runs on the
// rebased pair.
//
// Header-only, host+device: the CPU engine is the oracle of the HIP kernel.
#pragma once

#include "walk.h"

namespace pumitally {

// Entries per track before it is dropped as lost (a numerically stuck
// enter/leave cycle must terminate).
constexpr int kMaxEntries = 1024;

// Inflation of a boundary triangle's AABB when it is binned, in units of one
// grid cell.  The traversal below decides which cells a segment visits in
// floating point: at a cell corner or edge it may step A -> C and skip a cell
// B whose true share of the segment is only rounding-error long (~1e-16 of a
// cell per unit of |u|, far below this pad), and it may place a point that
// lies on a cell wall on either side.  A face hit inside such a sliver lies
// within that rounding distance of a cell the traversal DOES visit, so the
// padded box of the face overlaps the visited cell and the face is listed
// there.  Hence a skipped corner cell cannot lose a hit.
constexpr double kFaceGridPad = 1e-6;

// CSR lists, over the cells of the localization grid (LocGrid: same nx, ny,
// nz, lo, inv_h), of the vacuum boundary faces (flat index elem*4+f) whose
// padded triangle AABB overlaps the cell.  Built by Mesh::build_face_grid.
struct FaceGridView {
  int nx, ny, nz;
  Vec3 lo, inv_h;
  const int32_t *cell_start;
  const int32_t *cell_faces;
};

// Everything one track reads besides its own row.
struct TrackMesh {
  const Plane *planes;
  const Plane32 *planes32; // fp32 traversal only
  const int32_t *nbr;
  GridView grid;
  FaceGridView faces;
  const uint32_t *face_bc;
  const int32_t *pidx, *pelem;
  const double *pshift;
  bool reflective; // global BC: nothing ever enters
  double tol;      // absolute localization tolerance
  int max_steps;   // per in-mesh piece
};

// Entry test of one vacuum boundary face for the segment o -> d.  With
// V(t) the face plane along the segment (inward-positive), the face admits
// the track iff V rises (vd - vo > 0) to a positive end value (vd > 0), the
// crossing t = vo / (vo - vd) is not before t_min, the hit point lies in the
// face's triangle (the tet's other three planes >= -tol there) and the track
// does not leave the tet at once through another plane it sits on
// (V_g <= tol and falling).  The last rule rejects edge- and vertex-grazing
// entries, which would be followed by a zero-length exit and the same entry
// again; it loses at most tol * w of track length.
PT_HD bool face_entry(const Plane *__restrict__ planes, int32_t fidx, Vec3 o,
                      Vec3 d, double t_min, double tol, double *t_out) {
  const int f = fidx & 3;
  const Plane *pl = planes + (int64_t)(fidx >> 2) * 4;
  const double vo = plane_eval(pl[f], o);
  const double vd = plane_eval(pl[f], d);
  if (!(vd - vo > 0.0) || !(vd > 0.0)) return false;
  const double t = vo / (vo - vd);
  if (!(t >= t_min - kWalkTEps)) return false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int g = 0; g < 4; ++g) {
    if (g == f) continue;
    const double vog = plane_eval(pl[g], o);
    const double slope = plane_eval(pl[g], d) - vog;
    const double vp = vog + t * slope;
    if (!(vp >= -tol)) return false;
    if (vp <= tol && slope < 0.0) return false;
  }
  *t_out = t;
  return true;
}

// Keeps the better of (best_face, best_t) and face fidx: smallest t, ties to
// the smallest flat face index -- independent of the order faces are visited
// in, so the CPU engine, the HIP kernel and a brute-force loop agree.
PT_HD void ray_consider(const Plane *__restrict__ planes, int32_t fidx, Vec3 o,
                        Vec3 d, double t_min, double tol, int32_t &best_face,
                        double &best_t) {
  double t;
  if (!face_entry(planes, fidx, o, d, t_min, tol, &t)) return;
  if (best_face < 0 || t < best_t || (t == best_t && fidx < best_face)) {
    best_t = t;
    best_face = fidx;
  }
}

// One axis of the slab clip, in cell units (the grid box is [0, n], padded by
// kFaceGridPad).  An axis the segment does not move along (|du| below any
// meaningful slope) only checks that the segment lies inside the slab.
constexpr double kRayStill = 1e-280;
constexpr double kRayHuge = 1e300;

PT_HD void ray_slab(double uo, double du, double n, double &t_lo, double &t_hi,
                    bool &ok) {
  if (fabs(du) >= kRayStill) {
    const double inv = 1.0 / du;
    double ta = (-kFaceGridPad - uo) * inv;
    double tb = (n + kFaceGridPad - uo) * inv;
    if (ta > tb) {
      const double x = ta;
      ta = tb;
      tb = x;
    }
    if (ta > t_lo) t_lo = ta;
    if (tb < t_hi) t_hi = tb;
  } else if (!(uo >= -kFaceGridPad && uo <= n + kFaceGridPad)) {
    ok = false;
  }
}

// Cell index of coordinate u (cell units) clamped into [0, n); NaN gives 0.
PT_HD int ray_cell(double u, int n) {
  return u >= (double)n ? n - 1 : (u > 0.0 ? (int)u : 0);
}

// Entry search: the first vacuum boundary face the segment o -> d enters the
// mesh through at t >= t_min - kWalkTEps.  Returns its flat index (t in
// *t_out) or -1.  The parameter range is clipped to the padded grid box, the
// cells along it are visited by a 3D-DDA (scalar per-axis state, no indexed
// arrays), every face listed in a visited cell is tested, and the search
// stops once the best hit is not beyond the current cell's exit parameter:
// any face hit at or before that parameter lies in a cell already visited.
// Bounded: at most nx + ny + nz + 3 cells, finite face lists.
PT_HD int32_t ray_enter(const FaceGridView &g,
                        const Plane *__restrict__ planes, Vec3 o, Vec3 d,
                        double t_min, double tol, double *t_out) {
  const double uox = (o.x - g.lo.x) * g.inv_h.x;
  const double uoy = (o.y - g.lo.y) * g.inv_h.y;
  const double uoz = (o.z - g.lo.z) * g.inv_h.z;
  const double dux = (d.x - g.lo.x) * g.inv_h.x - uox;
  const double duy = (d.y - g.lo.y) * g.inv_h.y - uoy;
  const double duz = (d.z - g.lo.z) * g.inv_h.z - uoz;
  double t_lo = t_min - kWalkTEps;
  if (!(t_lo > 0.0)) t_lo = 0.0;
  double t_hi = 1.0;
  bool ok = true;
  ray_slab(uox, dux, (double)g.nx, t_lo, t_hi, ok);
  ray_slab(uoy, duy, (double)g.ny, t_lo, t_hi, ok);
  ray_slab(uoz, duz, (double)g.nz, t_lo, t_hi, ok);
  if (!ok || !(t_lo <= t_hi)) return -1;

  int cx = ray_cell(uox + t_lo * dux, g.nx);
  int cy = ray_cell(uoy + t_lo * duy, g.ny);
  int cz = ray_cell(uoz + t_lo * duz, g.nz);
  // an axis the segment does not move along never steps: its wall is
  // "reached" at a huge finite parameter instead of a division by zero
  const bool mx = fabs(dux) >= kRayStill, my = fabs(duy) >= kRayStill,
             mz = fabs(duz) >= kRayStill;
  const double ix = mx ? 1.0 / dux : 0.0, iy = my ? 1.0 / duy : 0.0,
               iz = mz ? 1.0 / duz : 0.0;
  const int sx = dux > 0.0 ? 1 : -1, sy = duy > 0.0 ? 1 : -1,
            sz = duz > 0.0 ? 1 : -1;
  int32_t best_face = -1;
  double best_t = 2.0;
  const int max_cells = g.nx + g.ny + g.nz + 3;
  for (int it = 0; it < max_cells; ++it) {
    // parameter at which the segment leaves the current cell, per axis
    const double tx =
        mx ? ((double)(cx + (sx > 0 ? 1 : 0)) - uox) * ix : kRayHuge;
    const double ty =
        my ? ((double)(cy + (sy > 0 ? 1 : 0)) - uoy) * iy : kRayHuge;
    const double tz =
        mz ? ((double)(cz + (sz > 0 ? 1 : 0)) - uoz) * iz : kRayHuge;
    const double txy = tx < ty ? tx : ty;
    const double t_leave = txy < tz ? txy : tz;
    const int64_t c = ((int64_t)cz * g.ny + cy) * g.nx + cx;
    const int32_t b = g.cell_start[c], e = g.cell_start[c + 1];
    for (int32_t i = b; i < e; ++i)
      ray_consider(planes, g.cell_faces[i], o, d, t_min, tol, best_face,
                   best_t);
    if (best_face >= 0 && best_t <= t_leave) break;
    if (t_leave > t_hi) break;
    if (tx <= ty && tx <= tz) {
      cx += sx;
      if (cx < 0 || cx >= g.nx) break;
    } else if (ty <= tz) {
      cy += sy;
      if (cy < 0 || cy >= g.ny) break;
    } else {
      cz += sz;
      if (cz < 0 || cz >= g.nz) break;
    }
  }
  if (best_face >= 0) *t_out = best_t;
  return best_face;
}

// Forwards every contribution to the real sink and remembers its end
// parameter.  walk_advance does not store the clamped exit parameter into
// the state on a vacuum clip (walk_raw exports s.t_cur, so that stays); the
// clipped crossing's contribution carries it as t1, and every piece of a
// tallied track contributes before it clips.
template <class Sink> struct ExitRecorder {
  Sink &sink;
  double t_exit;
  PT_HD void operator()(int32_t el, double t0, double t1, const WalkState &s,
                        int exit_face) {
    t_exit = t1;
    sink(el, t0, t1, s, exit_face);
  }
};

struct TrackResult {
  int entries = 0;      // times the track entered through a boundary face
  bool tallied = false; // false: zero length or zero weight, nothing done
  bool miss = false;    // tallied, but never inside the mesh
  bool loose = false;   // origin localized at the loosened tolerance only
  bool lost = false;    // ran out of steps or entries; lost_pos is the drop
  Vec3 lost_pos{0, 0, 0};
};

// One track through sink (a TallySink; re-exit rule off).
template <bool F32, class Sink>
PT_HD void track_tally(const TrackMesh &m, Vec3 o, Vec3 d, double w,
                       Sink &sink, TrackResult &r) {
  WalkState s;
  walk_init(s, -1, o, d, w);
  if (!s.tally) return;
  r.tallied = true;
  int32_t e = grid_locate(m.grid, m.planes, o, m.tol, &r.loose);
  const bool started_inside = e >= 0;
  s.elem = e;
  double t_from = 0.0;
  ExitRecorder<Sink> rec{sink, 0.0};
  for (;;) {
    if (e < 0) {
      if (m.reflective) break;
      if (r.entries >= kMaxEntries) {
        r.lost = true;
        r.lost_pos = s.o + t_from * (s.d - s.o);
        break;
      }
      double t_in = 0.0;
      const int32_t face =
          ray_enter(m.faces, m.planes, s.o, s.d, t_from, m.tol, &t_in);
      if (face < 0) break;
      e = face >> 2;
      s.elem = e;
      s.prev_elem = -1;
      s.t_cur = t_in > t_from ? t_in : t_from;
      s.step = 0;
      r.entries++;
    }
    int32_t oe;
    Vec3 op;
    bool esc;
    for (;;) {
      bool done;
      if constexpr (F32)
        done = walk_advance32<true>(m.planes, m.planes32, m.nbr, s,
                                    m.max_steps, rec, &oe, &op, &esc,
                                    m.reflective, m.face_bc, m.pidx, m.pelem,
                                    m.pshift);
      else
        done = walk_advance<true>(m.planes, m.nbr, s, m.max_steps, rec, &oe,
                                  &op, &esc, m.reflective, m.face_bc, m.pidx,
                                  m.pelem, m.pshift);
      if (done) break;
    }
    if (oe == kWalkLost) {
      r.lost = true;
      r.lost_pos = op;
      break;
    }
    if (!esc) break; // reached the destination inside the mesh
    // vacuum clip: look for the next entry from the exit parameter, on the
    // walk's current (s.o, s.d)
    t_from = rec.t_exit;
    e = -1;
  }
  r.miss = !started_inside && r.entries == 0;
}

} // namespace pumitally
