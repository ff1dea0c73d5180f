"""Cost of stateless track tallies (TallyEngine.tally_tracks_from_device) on
one GPU, at the headline shape: the 1M-tet box, 10M chord-8 tracks from the
synthetic generator, Morton-sorted, already in HBM.  Three cases, the SAME
tracks in each:

  inside  the full box: every track lies wholly inside.  Compared with
          walk_raw_device fed the elements mesh.locate gives -- the walk that
          needs its origins localized by the caller.  Alternating windows.
  half    a mesh made of the inner half of the box (the middle half of the
          cells per axis): most tracks start outside, many miss
  hole    the full box with the central quarter of the cells per axis
          removed: tracks cross the void and re-enter

Each timed window is `--steps` calls ending in a device synchronise.  Prints
one line per window to stderr, then one JSON line with, per case, the median
ns per track, min, max, the run-to-run spread ((max-min)/median) and the
entry and miss counts of one call.  bench.py is the project's headline
benchmark and is not involved.

    python benchmarks/tracks_cost.py [--tracks N] [--mesh-tets T] [--steps K]
                                     [--warmup W] [--repeats R]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def cut_mesh(pt, box, cells, keep_cell):
    """The submesh of `box` (cells^3 unit-extent cells, 6 tets each) whose
    tets lie in a cell (ix, iy, iz) with keep_cell(ix, iy, iz) true."""
    coords = np.asarray(box.coords, dtype=np.float64).reshape(-1, 3)
    t2v = np.asarray(box.tet2vert, dtype=np.int32).reshape(-1, 4)
    cell = np.floor(coords[t2v].mean(axis=1) * cells).astype(np.int64)
    keep = keep_cell(cell[:, 0], cell[:, 1], cell[:, 2])
    used = np.unique(t2v[keep])
    remap = np.full(len(coords), -1, dtype=np.int32)
    remap[used] = np.arange(len(used), dtype=np.int32)
    return pt.mesh_from_arrays(coords[used].ravel(), remap[t2v[keep]].ravel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=10_000_000)
    ap.add_argument("--mesh-tets", type=int, default=1_000_000)
    ap.add_argument("--mean-chord", type=float, default=8.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import torch

    import pumiumtally_amd as pt
    from pumiumtally_amd.mesh import box_mesh_with_tets
    from pumiumtally_amd.utils import make_box_histories

    if not pt.have_gpu():
        raise SystemExit("tracks_cost.py needs a GPU")
    box, cells = box_mesh_with_tets(args.mesh_tets, extent=1.0)
    n = args.tracks
    q, h = cells // 4, cells // 8

    def mid(i, half_width):
        return (i >= cells // 2 - half_width) & (i < cells - cells // 2 + half_width)

    meshes = {
        "inside": box,
        "half": cut_mesh(pt, box, cells, lambda x, y, z:
                         mid(x, q) & mid(y, q) & mid(z, q)),
        "hole": cut_mesh(pt, box, cells, lambda x, y, z:
                         ~(mid(x, h) & mid(y, h) & mid(z, h))),
    }
    p0, p1, _, weights = make_box_histories(
        (1.0, 1.0, 1.0), n, args.mean_chord, cells, seed=0, pinned=False)
    dev = torch.device("cuda:0")
    t_o = torch.from_numpy(p0.reshape(-1).copy()).to(dev)
    t_d = torch.from_numpy(p1.reshape(-1).copy()).to(dev)
    t_w = torch.from_numpy(np.asarray(weights).copy()).to(dev)
    elem = np.asarray(box.locate(p0.reshape(-1)), dtype=np.int32)
    assert (elem >= 0).all()
    t_e = torch.from_numpy(elem).to(dev)
    t_op = torch.empty(n * 3, dtype=torch.float64, device=dev)
    t_oe = torch.empty(n, dtype=torch.int32, device=dev)
    t_st = torch.empty(n, dtype=torch.int8, device=dev)
    torch.cuda.synchronize()

    out = {"tracks": n, "mesh_tets": {k: int(m.nelems) for k, m in meshes.items()},
           "mean_chord": args.mean_chord, "steps": args.steps,
           "repeats": args.repeats, "unit": "ns per track"}
    engines = {k: pt.TallyEngine(m, 1, device="cuda:0")
               for k, m in meshes.items()}
    engines["walk_raw"] = pt.TallyEngine(box, 1, device="cuda:0")

    def tracks(case):
        return lambda: engines[case].tally_tracks_from_device(
            t_o, t_d, t_w, sync_torch=False)

    def walk_raw():
        engines["walk_raw"]._eng.walk_raw_device(
            n, t_o.data_ptr(), t_d.data_ptr(), t_e.data_ptr(), t_w.data_ptr(),
            t_op.data_ptr(), t_oe.data_ptr(), t_st.data_ptr())

    calls = {"inside": tracks("inside"), "walk_raw": walk_raw,
             "half": tracks("half"), "hole": tracks("hole")}

    def window(call, eng):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            call()
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e9 / (args.steps * n)

    # one call each first: the counts of a single call, and the check that
    # tally_tracks and walk_raw tally the same flux for tracks wholly inside
    for name, call in calls.items():
        call()
        engines[name].synchronize()
        st = engines[name].stats()
        assert st["lost_particles"] == 0
        if name != "walk_raw":
            out[f"{name}_entries"] = st["track_entries"]
            out[f"{name}_misses"] = st["track_misses"]
    a, b = engines["inside"].flux(), engines["walk_raw"].flux()
    assert np.abs(a - b).max() <= 1e-9 * np.abs(b).max()
    assert out["inside_entries"] == 0 and out["inside_misses"] == 0
    for name, call in calls.items():
        for _ in range(args.warmup):
            call()
        engines[name].synchronize()
    runs = {name: [] for name in calls}
    for r in range(args.repeats):
        for name, call in calls.items():
            ns = window(call, engines[name])
            runs[name].append(ns)
            print(f"repeat {r} {name:<9} {ns:8.3f} ns/track",
                  file=sys.stderr, flush=True)
    for name, x in runs.items():
        med = float(np.median(x))
        out[f"{name}_ns"] = med
        out[f"{name}_min_ns"] = float(min(x))
        out[f"{name}_max_ns"] = float(max(x))
        out[f"{name}_spread"] = float((max(x) - min(x)) / med)
    out["inside_over_walk_raw"] = out["inside_ns"] / out["walk_raw_ns"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
