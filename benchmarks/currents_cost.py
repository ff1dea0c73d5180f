"""Cost of the face-current tallies: the same synthetic batch on one GPU,
engine built with currents off and on, in two configurations:

  aggregated  plain move (no groups, no responses): the wave-aggregated
              kernels.  The flux goes through the run aggregation either
              way; the current is booked with one plain atomic per crossing
              ("plain"), or through the same run aggregation keyed on the
              flat face index ("keyed", PUMITALLY_CURRENTS_AGG=1)
  grouped     groups + responses: the plain-atomic kernels

Device-resident moves (inputs already in HBM), so the figure is the walk
kernel and its atomics, not the host link.  Prints segments/s (element
crossings per second, counted from the mean chord) per variant and repeat,
then one JSON line with the medians, the run-to-run spread of each variant,
the on/off ratios and the keyed-over-plain ratio.  bench.py is the project's
headline benchmark and is not involved.

    python benchmarks/currents_cost.py [--particles N] [--mesh-tets T]
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
    ap.add_argument("--particles", type=int, default=4_000_000)
    ap.add_argument("--mesh-tets", type=int, default=1_000_000)
    ap.add_argument("--mean-chord", type=float, default=8.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import torch

    import pumiumtally_amd as pt
    from pumiumtally_amd.mesh import box_mesh_with_tets
    from pumiumtally_amd.utils import make_box_histories

    if not pt.have_gpu():
        raise SystemExit("currents_cost.py needs a GPU")
    mesh, cells = box_mesh_with_tets(args.mesh_tets, extent=1.0)
    n, G, S = args.particles, 2, 2
    p0, p1, flying, weights = make_box_histories(
        (1.0, 1.0, 1.0), n, args.mean_chord, cells, seed=0, pinned=False)
    rng = np.random.default_rng(1)
    dev = torch.device("cuda:0")
    ends = [torch.from_numpy(p.reshape(-1).copy()).to(dev) for p in (p0, p1)]
    t_fly = torch.from_numpy(np.asarray(flying).copy()).to(dev)
    t_w = torch.from_numpy(np.asarray(weights).copy()).to(dev)
    t_grp = torch.from_numpy(
        rng.integers(0, G, n).astype(np.uint16).view(np.int16)).to(dev)
    t_rsp = torch.from_numpy(rng.uniform(0.5, 2.0, size=(n, S))).to(dev)
    torch.cuda.synchronize()

    class U16View:
        """int16 torch storage presented as the uint16 array it holds."""
        def __init__(self, t):
            self.t = t
            self.__cuda_array_interface__ = dict(
                t.__cuda_array_interface__, typestr="<u2")

    grp = U16View(t_grp)

    def rate(grouped, mode):
        kw = dict(ngroups=G, nscores=S) if grouped else {}
        # the engine reads the switch once, at construction
        os.environ["PUMITALLY_CURRENTS_AGG"] = "1" if mode == "keyed" else "0"
        eng = pt.TallyEngine(mesh, n, device="cuda:0",
                             currents=mode != "off", **kw)
        eng.copy_initial_position(p0.reshape(-1))

        def step(k):
            eng.move_from_device(
                ends[(k + 1) % 2], t_fly, t_w, sync_torch=False,
                groups=grp if grouped else None,
                responses=t_rsp if grouped else None)

        for k in range(args.warmup):
            step(k)
        eng.synchronize()
        t0 = time.perf_counter()
        for k in range(args.warmup, args.warmup + args.steps):
            step(k)
        eng.synchronize()
        dt = time.perf_counter() - t0
        assert eng.stats()["lost_particles"] == 0
        return args.mean_chord * n * args.steps / dt

    variants = [("aggregated", "off"), ("aggregated", "plain"),
                ("aggregated", "keyed"), ("grouped", "off"),
                ("grouped", "plain")]
    runs = {v: [] for v in variants}
    for r in range(args.repeats):         # interleaved: drift hits all alike
        for v in variants:
            x = rate(v[0] == "grouped", v[1])
            runs[v].append(x)
            print(f"repeat {r} {v[0]:>10} currents={v[1]:<5} "
                  f"{x / 1e9:8.3f} G segments/s", file=sys.stderr, flush=True)

    med = {v: float(np.median(x)) for v, x in runs.items()}
    out = {"particles": n, "mesh_tets": int(mesh.nelems),
           "mean_chord": args.mean_chord, "steps": args.steps,
           "repeats": args.repeats, "unit": "segments/s (nominal chord)"}
    for v in variants:
        key = f"{v[0]}_currents_{v[1]}"
        out[key] = med[v]
        out[key + "_spread"] = float((max(runs[v]) - min(runs[v])) / med[v])
        out[key + "_particle_steps_per_s"] = med[v] / args.mean_chord
    out["aggregated_on_over_off"] = \
        med[("aggregated", "plain")] / med[("aggregated", "off")]
    out["aggregated_keyed_on_over_off"] = \
        med[("aggregated", "keyed")] / med[("aggregated", "off")]
    out["aggregated_keyed_over_plain"] = \
        med[("aggregated", "keyed")] / med[("aggregated", "plain")]
    out["grouped_on_over_off"] = \
        med[("grouped", "plain")] / med[("grouped", "off")]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
