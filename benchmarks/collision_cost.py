"""Cost of one collision-scoring step beside one move step, on one GPU, at
the headline shape (1M-tet box, 10M particles), for two sources:

  spread  origins uniform in the box (the steady-state load)
  point   the config-4 point source: every origin in the central 2 % cube,
          so all particles score into the same few elements

and both ways score_collisions can add (PUMITALLY_WAVE_AGG, read per engine
at construction for this tally):

  agg     one atomicAdd per run of equal elements in a wave (wave_run_sum)
  plain   one atomicAdd per particle

Device-resident calls (score_collisions_from_device / move_from_device,
inputs already in HBM), so the figures are the kernels, not the host link.
The particles are scored where copy_initial_position and two ping-pong moves
left them: back at their origins, in the slot order of the initial sort.
Each timed window is `--steps` calls ending in a device synchronise; the two
arms and the move alternate inside every repeat so drift hits all alike.
Prints one line per window to stderr, then one JSON line with, per source
and arm, the median ms per step, min, max and the run-to-run spread
((max-min)/median).  bench.py is the project's headline benchmark and is not
involved.

    python benchmarks/collision_cost.py [--particles N] [--mesh-tets T]
                                        [--steps K] [--warmup W] [--repeats R]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=10_000_000)
    ap.add_argument("--mesh-tets", type=int, default=1_000_000)
    ap.add_argument("--mean-chord", type=float, default=8.0)
    ap.add_argument("--point-frac", type=float, default=0.02)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import torch

    import pumiumtally_amd as pt
    from pumiumtally_amd.mesh import box_mesh_with_tets
    from pumiumtally_amd.utils import make_box_histories

    if not pt.have_gpu():
        raise SystemExit("collision_cost.py needs a GPU")
    mesh, cells = box_mesh_with_tets(args.mesh_tets, extent=1.0)
    n = args.particles
    dev = torch.device("cuda:0")
    out = {"particles": n, "mesh_tets": int(mesh.nelems),
           "mean_chord": args.mean_chord, "steps": args.steps,
           "repeats": args.repeats, "unit": "ms per step"}

    def window(call):
        """ms per call over one timed window of args.steps calls."""
        t0 = time.perf_counter()
        for k in range(args.steps):
            call(k)
        eng_sync()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    for source, frac in (("spread", 1.0), ("point", args.point_frac)):
        p0, p1, flying, weights = make_box_histories(
            (1.0, 1.0, 1.0), n, args.mean_chord, cells, seed=0, pinned=False,
            source_frac=frac)
        ends = [torch.from_numpy(p.reshape(-1).copy()).to(dev)
                for p in (p0, p1)]
        t_on = torch.from_numpy(np.asarray(flying).copy()).to(dev)
        t_w = torch.from_numpy(np.asarray(weights).copy()).to(dev)
        torch.cuda.synchronize()

        engines = {}
        for arm in ("mover", "agg", "plain"):
            # The scoring kernels' switch is read per engine, at
            # construction.  The move kernels latch theirs once per process,
            # at the first move: that happens below on the first engine,
            # built with the switch unset, so every move here is the default.
            # The timed moves run on an engine of their own, so both scoring
            # arms stay in the same state (re-sorts follow moves).
            if arm != "mover":
                os.environ["PUMITALLY_WAVE_AGG"] = "1" if arm == "agg" else "0"
            eng = pt.TallyEngine(mesh, n, device="cuda:0",
                                 collisions=arm != "mover")
            eng.copy_initial_position(p0.reshape(-1))
            for k in range(2):           # out and back: particles at p0
                eng.move_from_device(ends[(k + 1) % 2], t_on, t_w,
                                     sync_torch=False)
            eng.synchronize()
            engines[arm] = eng
        os.environ.pop("PUMITALLY_WAVE_AGG")
        scorers = {a: engines[a] for a in ("agg", "plain")}

        def eng_sync():
            for e in engines.values():
                e.synchronize()

        def score(arm):
            return lambda k: engines[arm].score_collisions_from_device(
                t_on, t_w, sync_torch=False)

        def move(k):
            # two moves per pair of calls return the particles to p0
            engines["mover"].move_from_device(ends[(k + 1) % 2], t_on, t_w,
                                              sync_torch=False)

        calls = {"score_agg": score("agg"), "score_plain": score("plain"),
                 "move": move}
        assert args.steps % 2 == 0, "--steps must be even (ping-pong moves)"
        for name, call in calls.items():
            for k in range(args.warmup + args.warmup % 2):
                call(k)
        eng_sync()
        before = {a: e.stats()["collisions_scored"]
                  for a, e in scorers.items()}
        runs = {name: [] for name in calls}
        for r in range(args.repeats):
            for name, call in calls.items():
                ms = window(call)
                runs[name].append(ms)
                print(f"{source:>6} repeat {r} {name:<11} {ms:9.4f} ms/step",
                      file=sys.stderr, flush=True)

        # both arms scored every particle every call, into the same tally
        a, b = (scorers[x].collisions() for x in ("agg", "plain"))
        calls_made = args.repeats * args.steps
        for arm, e in scorers.items():
            st = e.stats()
            assert st["collisions_scored"] - before[arm] == calls_made * n
            assert st["collision_misses"] == 0 and st["lost_particles"] == 0
        assert np.allclose(a, b, rtol=1e-9, atol=0)
        for name, x in runs.items():
            med = float(np.median(x))
            out[f"{source}_{name}_ms"] = med
            out[f"{source}_{name}_min_ms"] = float(min(x))
            out[f"{source}_{name}_max_ms"] = float(max(x))
            out[f"{source}_{name}_spread"] = float((max(x) - min(x)) / med)
        out[f"{source}_agg_over_plain"] = \
            out[f"{source}_score_agg_ms"] / out[f"{source}_score_plain_ms"]
        out[f"{source}_score_agg_over_move"] = \
            out[f"{source}_score_agg_ms"] / out[f"{source}_move_ms"]
        out[f"{source}_hottest_element_share"] = float(a.max() / a.sum())
        del engines, scorers, ends, t_on, t_w
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
