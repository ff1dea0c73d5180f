"""One battery of engine calls, run by both engines.

run_battery(device) drives every entry point of the engine that launches a
particle kernel -- move / move_continue (flux, linear, currents, keyed
currents, periodic, scored), end_batch, score_collisions, score_points,
tally_tracks, walk_raw -- over fixed inputs and returns what they computed,
keyed "case.name".  tests/test_launch_geometry.py imports it for the CPU
reference and starts it as a child process for the GPU:

    python tests/launch_battery.py --device cuda:0 --out result.npz

The launch geometry of the HIP engine (PUMITALLY_CHUNK, PUMITALLY_GRID_CAP,
PUMITALLY_BLOCK, PUMITALLY_WAVE_AGG, PUMITALLY_SORT) is read once per
process, so a configuration is the environment of one child.

Shapes: build_box(4, 4, 4) (384 tets); n = 5000 = 78 * 64 + 8, so the last
wave is partial.  Weights and responses are small integers stored as
float64: currents, collisions and counters are exact in any order of adds.
"""
import argparse
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pumiumtally_amd as pt  # noqa: E402

N = 5000
N_FREE = 3000  # free points, tracks and raw walks
CELLS = 4
SOURCE = (0.37, 0.41, 0.53)  # interior of one tet, on no face plane


@functools.lru_cache(maxsize=None)
def mesh(periodic=False):
    m = pt.build_box(CELLS, CELLS, CELLS)
    if periodic:
        fid, cen, _ = m.boundary_faces()
        hi = fid[np.abs(cen[:, 0] - 1.0) < 1e-12]
        lo = fid[np.abs(cen[:, 0] - 0.0) < 1e-12]
        m.set_periodic_faces(hi, lo, np.array([-1.0, 0.0, 0.0]))
    return m


def _outside(rng, k):
    """k points of [-0.5, 1.5]^3 outside the unit box."""
    p = rng.uniform(-0.5, 1.5, size=(k, 3))
    ax = rng.integers(0, 3, k)
    side = rng.integers(0, 2, k)
    p[np.arange(k), ax] = np.where(side == 1, rng.uniform(1.05, 1.5, k),
                                   rng.uniform(-0.5, -0.05, k))
    return p


@functools.lru_cache(maxsize=None)
def inputs():
    """Shared by every case and both engines; read-only."""
    rng = np.random.default_rng(20260)
    x = {}
    # the three particle moves
    o1 = rng.uniform(0.02, 0.98, size=(N, 3))
    d1 = rng.uniform(0.02, 0.98, size=(N, 3))
    d1[::9] = o1[::9] + rng.normal(0, 1.0, size=(len(d1[::9]), 3))
    o2 = d1.copy()  # call 2 starts where call 1 ended ...
    o2[::5] = rng.uniform(0.02, 0.98, size=(len(o2[::5]), 3))  # ... mostly
    d2 = rng.uniform(0.02, 0.98, size=(N, 3))
    d3 = rng.uniform(0.02, 0.98, size=(N, 3))
    # an escaped particle re-enters on its next flight, so the last flights
    # throw some out again: the recorded state has escaped particles in it
    d2[::11] = _outside(rng, len(d2[::11]))
    d3[::7] = _outside(rng, len(d3[::7]))
    d4 =rng.uniform(0.02, 0.98, size=(N, 3))
    fly_all = np.ones(N, np.int8)
    fly2 = np.ones(N, np.int8)
    fly2[::3] = 0
    x.update(o1=o1, d1=d1, o2=o2, d2=d2, d3=d3, d4=d4, fly_all=fly_all,
             fly2=fly2)
    x["w"] = rng.integers(1, 5, N).astype(np.float64)
    x["w2"] = rng.integers(1, 5, N).astype(np.float64)
    x["grp"] = rng.integers(0, 2, N).astype(np.uint16)
    x["resp"] = rng.integers(1, 4, size=(N, 2)).astype(np.float64)
    # point source: one origin, isotropic destinations, every 4th at rest
    u = rng.normal(size=(N, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    x["ps_o"] = np.tile(np.array(SOURCE), (N, 1))
    x["ps_d"] = x["ps_o"] + u * rng.uniform(0.05, 0.7, size=(N, 1))
    fly4 = np.ones(N, np.int8)
    fly4[::4] = 0
    x["fly4"] = fly4
    # free points: a fifth outside the mesh
    pts = rng.uniform(0.02, 0.98, size=(N_FREE, 3))
    pts[::5] = _outside(rng, len(pts[::5]))
    x["pts"] = pts
    x["pts_w"] = rng.integers(1, 5, N_FREE).astype(np.float64)
    x["pts_grp"] = rng.integers(0, 2, N_FREE).astype(np.uint16)
    x["pts_resp"] = rng.integers(1, 4, size=(N_FREE, 2)).astype(np.float64)
    # tracks: a third start outside the box; every 12th stays outside it
    to = rng.uniform(0.02, 0.98, size=(N_FREE, 3))
    td = rng.uniform(-0.3, 1.3, size=(N_FREE, 3))
    to[::3] = _outside(rng, len(to[::3]))
    td[::12] = to[::12] + rng.uniform(-0.02, 0.02, size=(len(td[::12]), 3))
    x.update(trk_o=to, trk_d=td)
    # raw walks: start inside, every 9th leaves
    ro = rng.uniform(0.02, 0.98, size=(N_FREE, 3))
    rd = rng.uniform(0.02, 0.98, size=(N_FREE, 3))
    rd[::9] = ro[::9] + rng.normal(0, 1.0, size=(len(rd[::9]), 3))
    x.update(raw_o=ro, raw_d=rd)
    for a in x.values():
        a.setflags(write=False)
    return x


def _put(out, case, **arrays):
    for name, a in arrays.items():
        out[f"{case}.{name}"] = np.array(a)  # a copy, 0-d for counters


def _state(out, case, eng):
    eng.synchronize()
    _put(out, case, flux=eng.flux(), positions=eng.positions(),
         elem_ids=eng.elem_ids(), escaped=eng.escaped(),
         lost_particles=np.int64(eng.stats()["lost_particles"]))
    if eng.linear:
        _put(out, case, moments=eng.moments())
    if eng.face_currents:
        _put(out, case, currents=eng.currents())


def _three_calls(out, case, eng, calls=3):
    """Call 1: everything flies, every 9th destination outside the box.
    Call 2: every 3rd particle rests, every 5th origin is re-sampled, the
    escaped carry over.  Call 3: move_continue."""
    x = inputs()
    eng.copy_initial_position(x["o1"].ravel())
    eng.move(x["o1"].ravel(), x["d1"].ravel(), x["fly_all"], x["w"])
    _put(out, case, flux_call1=eng.flux())
    eng.move(x["o2"].ravel(), x["d2"].ravel(), x["fly2"], x["w2"])
    if calls > 2:
        eng.move_continue(x["d3"].ravel(), x["fly_all"], x["w"])
    _state(out, case, eng)


def _batches(out, case, eng):
    x = inputs()
    eng.end_batch()
    eng.move_continue(x["d4"].ravel(), x["fly2"], x["w2"])
    eng.end_batch()
    _put(out, case, batch_sum=eng._eng.batch_sum(),
         batch_sum_sq=eng._eng.batch_sum_sq())


def run_battery(device):
    """Every case on a fresh engine of `device`; dict of arrays."""
    x = inputs()
    box = mesh(False)
    out = {}

    eng = pt.TallyEngine(box, N, device=device)
    _three_calls(out, "plain", eng)
    _batches(out, "plain", eng)

    eng = pt.TallyEngine(box, N, device=device, linear=True)
    _three_calls(out, "linear", eng)

    eng = pt.TallyEngine(box, N, device=device, currents=True)
    _three_calls(out, "currents", eng)

    saved = os.environ.get("PUMITALLY_CURRENTS_AGG")
    os.environ["PUMITALLY_CURRENTS_AGG"] = "1"
    try:
        eng = pt.TallyEngine(box, N, device=device, currents=True)
    finally:
        if saved is None:
            del os.environ["PUMITALLY_CURRENTS_AGG"]
        else:
            os.environ["PUMITALLY_CURRENTS_AGG"] = saved
    _three_calls(out, "currents_keyed", eng)

    eng = pt.TallyEngine(mesh(True), N, device=device)
    _three_calls(out, "periodic_plain", eng, calls=2)

    eng = pt.TallyEngine(box, N, device=device, ngroups=2, nscores=2)
    eng.copy_initial_position(x["o1"].ravel())
    eng.move(x["o1"].ravel(), x["d1"].ravel(), x["fly_all"], x["w"],
             groups=x["grp"], responses=x["resp"])
    eng.move(x["o2"].ravel(), x["d2"].ravel(), x["fly2"], x["w2"])
    eng.synchronize()
    _put(out, "scored_mixed", flux=eng.flux(),
         lost_particles=np.int64(eng.stats()["lost_particles"]))

    eng = pt.TallyEngine(box, N, device=device, nscores=2)
    eng.copy_initial_position(x["o1"].ravel())
    eng.move(x["o1"].ravel(), x["d1"].ravel(), x["fly_all"], x["w"])
    eng.synchronize()
    _put(out, "null_responses", flux=eng.flux(),
         lost_particles=np.int64(eng.stats()["lost_particles"]))

    for case, kw in (("point_source", {}),
                     ("point_source_linear", dict(linear=True))):
        eng = pt.TallyEngine(box, N, device=device, **kw)
        eng.copy_initial_position(x["ps_o"].ravel())
        eng.move(x["ps_o"].ravel(), x["ps_d"].ravel(), x["fly4"], x["w"])
        _state(out, case, eng)

    eng = pt.TallyEngine(box, N, device=device, ngroups=2, nscores=2,
                         collisions=True)
    eng.copy_initial_position(x["o1"].ravel())
    eng.move(x["o1"].ravel(), x["d1"].ravel(), x["fly_all"], x["w"],
             groups=x["grp"], responses=x["resp"])
    eng.score_collisions(x["fly2"], x["w"])
    eng.score_collisions(x["fly4"], x["w2"], groups=x["grp"],
                         responses=x["resp"])
    eng.score_points(x["pts"], x["pts_w"])
    eng.score_points(x["pts"], x["pts_w"], groups=x["pts_grp"],
                     responses=x["pts_resp"])
    eng.synchronize()
    st = eng.stats()
    _put(out, "collisions", collisions=eng.collisions(),
         collisions_scored=np.int64(st["collisions_scored"]),
         collision_misses=np.int64(st["collision_misses"]),
         lost_particles=np.int64(st["lost_particles"]))

    eng = pt.TallyEngine(box, 1, device=device, ngroups=2)
    eng.tally_tracks(x["trk_o"], x["trk_d"], x["pts_w"], groups=x["pts_grp"])
    eng.synchronize()
    st = eng.stats()
    _put(out, "tracks", flux=eng.flux(),
         track_entries=np.int64(st["track_entries"]),
         track_misses=np.int64(st["track_misses"]),
         lost_particles=np.int64(st["lost_particles"]))

    eng = pt.TallyEngine(box, 1, device=device, ngroups=2)
    raw = eng.walk_raw(x["raw_o"].ravel(), x["raw_d"].ravel(),
                       box.locate(x["raw_o"]).astype(np.int32), x["pts_w"],
                       groups=x["pts_grp"])
    eng.synchronize()
    _put(out, "walk_raw", flux=eng.flux(), out_pos=raw[0], out_elem=raw[1],
         status=raw[2], out_dest=raw[3],
         lost_particles=np.int64(eng.stats()["lost_particles"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    np.savez(args.out, **run_battery(args.device))
    print("BATTERY_OK")


if __name__ == "__main__":
    main()
