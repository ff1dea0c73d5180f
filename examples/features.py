"""Extended tally features in one tour: energy groups, multi-score
responses, periodic boundaries, batch statistics, .vtu output.

Everything runs on CPU anywhere; add device="cuda:0" on an MI355X.
    python examples/features.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pumiumtally_amd as pt  # noqa: E402

rng = np.random.default_rng(1)
mesh = pt.build_box(8, 8, 8)

# -- periodic boundaries: pair the x=1 faces with the x=0 faces ----------
fid, cen, nor = mesh.boundary_faces()
x_hi = fid[np.abs(cen[:, 0] - 1.0) < 1e-12]
x_lo = fid[np.abs(cen[:, 0] - 0.0) < 1e-12]
mesh.set_periodic_faces(x_hi, x_lo, np.array([-1.0, 0.0, 0.0]))
print(f"mesh: {mesh.nelems} tets, x-periodic")

# -- engine with 3 energy groups and 2 simultaneous scores ---------------
# score 0 = flux (response 1), score 1 = "heating" with a per-particle
# response (e.g. energy-dependent KERMA factor looked up by the caller)
n = 20000
G, S = 3, 2
eng = pt.TallyEngine(mesh, n, device="auto", ngroups=G, nscores=S)

pos = rng.uniform(0.05, 0.95, size=(n, 3))
eng.copy_initial_position(pos.ravel())
groups = rng.integers(0, G, n).astype(np.uint16)
heating = rng.uniform(0.2, 5.0, n)            # per-particle response
responses = np.column_stack([np.ones(n), heating])
weights = rng.uniform(0.5, 1.0, n)

for batch in range(3):
    alive = np.ones(n, np.int8)
    for step in range(10):
        # long x-flights exercise the periodic wrap
        d = pos + np.column_stack([rng.normal(0, 0.3, n),
                                   rng.normal(0, 0.05, n),
                                   rng.normal(0, 0.05, n)])
        d[:, 1:] = np.clip(d[:, 1:], 0.0, 1.0)
        eng.move(pos.ravel(), d.ravel(), alive.copy(), weights,
                 groups=groups, responses=responses)
        alive[eng.escaped().astype(bool)] = 0
        pos = eng.positions()
    f = eng.flux()                     # (S, G, nelems)
    print(f"batch {batch}: flux total {f[0].sum():.2f}, "
          f"heating total {f[1].sum():.2f}, "
          f"per-group {np.round(f[0].sum(axis=1), 1)}")
    eng.end_batch()                    # fold into batch statistics

mean, rel_err = eng.batch_statistics() # shaped (S, G, nelems)
print(f"flux mean total {mean[0].sum():.2f}, "
      f"median rel. std. error {np.median(rel_err[rel_err > 0]):.3f}")

# -- modern .vtu output (per-score and per-group fields) -----------------
# restore the last batch's tally for the writer
eng.set_flux(mean.reshape(-1) * eng._eng.num_batches)
eng.write_tally_results("features_flux.vtu")
print("wrote features_flux.vtu (fields: flux, flux_g*, score1, score1_g*)")

# -- stateless track tallies: a tally mesh that covers part of the geometry
# The host owns the particles; the engine gets free segments.  The tally mesh
# is a detector block [0.25, 0.75]^3 with a duct drilled through it along x,
# and a point source sits outside it: tracks enter from outside, cross the
# duct, come back, or miss.
box = pt.build_box(8, 8, 8)
xyz = np.asarray(box.coords).reshape(-1, 3)
t2v = np.asarray(box.tet2vert).reshape(-1, 4)
cell = np.floor(xyz[t2v].mean(axis=1) * 8).astype(int)
keep = np.all((cell >= 2) & (cell <= 5), axis=1) \
    & ~np.all((cell[:, 1:] >= 3) & (cell[:, 1:] <= 4), axis=1)
used = np.unique(t2v[keep])
remap = np.full(len(xyz), -1, np.int32)
remap[used] = np.arange(len(used), dtype=np.int32)
block = pt.mesh_from_arrays(xyz[used].ravel(), remap[t2v[keep]].ravel())
det = pt.TallyEngine(block, 1, device="auto")
m = 20000
src = np.tile([0.05, 0.5, 0.5], (m, 1))
aim = rng.uniform(0.0, 1.0, size=(m, 3))
aim[:, 0] = 1.0
det.tally_tracks(src, aim, np.full(m, 1.0 / m))
st = det.stats()
print(f"detector block ({block.nelems} tets): uncollided track length "
      f"{det.flux().sum():.4f} per source particle, "
      f"{st['track_entries']} entries, {st['track_misses']} misses "
      f"of {st['tracks']} tracks")

# -- failure-path observability ------------------------------------------
# loose-tolerance localizations and lost walks are counted and the first
# lost walks are captured with drop positions (the reference only
# printfs "Not all particles are found")
stats = eng.stats()
print(f"stats: {stats}; lost records shape {eng.lost_records().shape}")
