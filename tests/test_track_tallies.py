"""Stateless track tallies: TallyEngine.tally_tracks (docs/DESIGN.md,
"Stateless track tallies").

Free segments (o, d, w) that may start outside the mesh, enter through vacuum
boundary faces, cross a cavity and come back, or miss.

Oracle for the shell fixtures: the walk_raw that predates this feature, on the
FULL 5x5x5 box the shell was cut from, started at full.locate(o), its tallies
restricted to the kept elements.  It walks the voids as ordinary elements, so
every in-mesh crossing has the same end parameters over the same (o, d) and
the same planes; only the order of the sums differs.  Gate, elementwise:
|got - oracle| <= 1e-12 * max|oracle| (the project's parity gate).

Entry and miss counts on the unjittered shell are integers from an analytic
slab clip against [1,4]^3 minus (2,3)^3, written here in numpy.
"""
import functools

import numpy as np
import pytest

import pumiumtally_amd as pt

GATE = 1e-12
N = 4000


# --------------------------------------------------------------- fixtures ---

@functools.lru_cache(maxsize=None)
def shell(jitter):
    """(full 750-tet mesh, 156-tet shell submesh, keep mask, o, d, w, rng
    state continues in the returned generator)."""
    rng = np.random.default_rng(11)
    box = pt.build_box(5, 5, 5, 5.0, 5.0, 5.0)
    coords = np.asarray(box.coords, dtype=np.float64).reshape(-1, 3).copy()
    t2v = np.asarray(box.tet2vert, dtype=np.int32).reshape(-1, 4).copy()
    cell = np.floor(coords[t2v].mean(axis=1)).astype(int)   # unjittered
    if jitter:
        inner = np.all((coords > 1e-9) & (coords < 5.0 - 1e-9), axis=1)
        coords[inner] += rng.uniform(-0.15, 0.15, size=(int(inner.sum()), 3))
    full = pt.mesh_from_arrays(coords.ravel(), t2v.ravel())
    keep = np.all((cell >= 1) & (cell <= 3), axis=1) & ~np.all(cell == 2, axis=1)
    used = np.unique(t2v[keep])
    remap = np.full(len(coords), -1, dtype=np.int32)
    remap[used] = np.arange(len(used), dtype=np.int32)
    sub = pt.mesh_from_arrays(coords[used].ravel(), remap[t2v[keep]].ravel())
    assert full.nelems == 750 and sub.nelems == 156
    assert len(sub.boundary_faces()[0]) == 120
    # tet order (and orientation fix-ups) survive: flux maps through keep
    assert np.array_equal(np.asarray(sub.volumes),
                          np.asarray(full.volumes)[keep])
    assert np.array_equal(used[np.asarray(sub.tet2vert).reshape(-1, 4)],
                          np.asarray(full.tet2vert).reshape(-1, 4)[keep])
    o = rng.uniform(0.013, 4.987, size=(N, 3))
    d = rng.uniform(0.013, 4.987, size=(N, 3))
    w = rng.uniform(0.5, 1.5, size=N)
    grp = rng.integers(0, 2, N).astype(np.uint16)
    resp = rng.uniform(0.5, 2.0, size=(N, 2))
    return full, sub, keep, o, d, w, grp, resp


def oracle(jitter, n=N, grouped=False, **kw):
    """The pre-existing walk_raw on the full mesh: (engine, all reached)."""
    full, _, _, o, d, w, grp, resp = shell(jitter)
    if grouped:
        kw.update(ngroups=2, nscores=2)
    eng = pt.TallyEngine(full, 1, device="cpu", **kw)
    el = np.asarray(full.locate(o[:n].ravel()), dtype=np.int32)
    assert (el >= 0).all()                       # nothing unlocated
    out = eng.walk_raw(o[:n].ravel(), d[:n].ravel(), el, w[:n],
                       grp[:n] if grouped else None,
                       resp[:n] if grouped else None)
    assert not np.asarray(out[2]).any()          # every status is 0
    return eng


def tracked(jitter, n=N, device="cpu", grouped=False, mesh=None, **kw):
    _, sub, _, o, d, w, grp, resp = shell(jitter)
    if grouped:
        kw.update(ngroups=2, nscores=2)
    eng = pt.TallyEngine(sub if mesh is None else mesh, 3, device=device, **kw)
    eng.tally_tracks(o[:n], d[:n], w[:n], grp[:n] if grouped else None,
                     resp[:n] if grouped else None)
    return eng


def close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    scale = np.abs(want).max()
    assert scale > 0
    err = np.abs(got - want).max()
    print(f"max |got - want| = {err:.3e}, gate {GATE * scale:.3e}")
    assert err <= GATE * scale


def analytic_counts(o, d):
    """Per track on the unjittered shell: (entries, exits before the end,
    in-mesh fraction of the length), by slab clips."""
    def clip(lo, hi):
        with np.errstate(divide="ignore", invalid="ignore"):
            ta = (lo - o) / (d - o)
            tb = (hi - o) / (d - o)
        t0 = np.minimum(ta, tb).max(axis=1).clip(min=0.0)
        t1 = np.maximum(ta, tb).min(axis=1).clip(max=1.0)
        return t0, t1
    a, b = clip(1.0, 4.0)
    c, e = clip(2.0, 3.0)
    entries = np.zeros(len(o), dtype=np.int64)
    exits = np.zeros(len(o), dtype=np.int64)
    frac = np.zeros(len(o))
    for i in range(len(o)):
        if not b[i] > a[i]:
            continue
        pieces = [(a[i], b[i])]
        if e[i] > c[i]:
            pieces = [p for p in ((a[i], c[i]), (e[i], b[i])) if p[1] > p[0]]
        for t0, t1 in pieces:
            entries[i] += t0 > 0.0
            exits[i] += t1 < 1.0
            frac[i] += t1 - t0
    return entries, exits, frac


# ---------------------------------------------------- fixture A: golden cube

def golden(device):
    m = pt.build_box(1, 1, 1)
    eng = pt.TallyEngine(m, 4, device=device)
    before = (eng.positions().copy(), eng.elem_ids().copy(),
              eng.escaped().copy())
    want = np.zeros(6)
    want[[2, 3, 4]] = [0.4, 0.1, 0.5]
    eng.tally_tracks(np.array([[-0.5, 0.4, 0.5]]), np.array([[1.2, 0.4, 0.5]]),
                     np.ones(1))
    f = eng.flux()
    assert np.abs(f - want).max() <= 1e-15
    assert np.count_nonzero(f) == 3
    s = eng.stats()
    assert (s["tracks"], s["track_entries"], s["track_misses"]) == (1, 1, 0)
    # clipping to the grid box: the same chord from far outside
    eng.tally_tracks(np.array([[-1e3, 0.4, 0.5]]), np.array([[1e3, 0.4, 0.5]]),
                     np.ones(1))
    assert np.abs(eng.flux() - 2 * want).max() <= 1e-12
    # a miss, a zero-length and a zero-weight track
    eng.tally_tracks(np.array([[-0.5, 2.0, 2.0]]), np.array([[1.5, 2.0, 2.0]]),
                     np.ones(1))
    eng.tally_tracks(np.array([[0.3, 0.4, 0.5], [-0.5, 0.4, 0.5]]),
                     np.array([[0.3, 0.4, 0.5], [1.2, 0.4, 0.5]]),
                     np.array([1.0, 0.0]))
    assert np.abs(eng.flux() - 2 * want).max() <= 1e-12
    s = eng.stats()
    assert (s["tracks"], s["track_entries"], s["track_misses"]) == (5, 2, 1)
    assert s["lost_particles"] == 0 and s["moves"] == 0
    # n == 0 is a no-op
    eng.tally_tracks(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0))
    assert eng.stats()["tracks"] == 5
    # particle state untouched
    assert np.array_equal(eng.positions(), before[0])
    assert np.array_equal(eng.elem_ids(), before[1])
    assert np.array_equal(eng.escaped(), before[2])


def test_golden_cube():
    golden("cpu")


def test_exact_dtypes_and_shapes():
    eng = pt.TallyEngine(pt.build_box(1, 1, 1), 1, device="cpu")
    with pytest.raises(TypeError):
        eng.tally_tracks(np.zeros((1, 3), np.float32), np.ones((1, 3)),
                         np.ones(1))
    with pytest.raises(RuntimeError):
        eng.tally_tracks(np.zeros((2, 3)), np.ones((1, 3)), np.ones(1))
    with pytest.raises(TypeError):               # not CUDA arrays
        eng.tally_tracks_from_device(np.zeros((1, 3)), np.ones((1, 3)),
                                     np.ones(1))
    with pytest.raises(RuntimeError):            # the CPU engine has no twin
        eng._eng.tally_tracks_device(1, 0, 0, 0)


# ------------------------------------------- fixture B / B': cavity in shell

@pytest.mark.parametrize("jitter", [False, True])
def test_shell_flux_matches_full_mesh_walk(jitter):
    _, _, keep, o, d, w, _, _ = shell(jitter)
    ref = oracle(jitter)
    # the oracle conserves total length: no track is left out
    total = (np.linalg.norm(d - o, axis=1) * w).sum()
    assert abs(ref.flux().sum() - total) <= 1e-13 * total
    eng = tracked(jitter)
    close(eng.flux(), ref.flux()[keep])
    s = eng.stats()
    assert s["lost_particles"] == 0 and s["tracks"] == N
    assert len(eng.lost_records()) == 0


def test_shell_counters_match_slab_clip():
    _, _, _, o, d, w, _, _ = shell(False)
    entries, exits, frac = analytic_counts(o, d)
    eng = tracked(False, currents=True)
    s = eng.stats()
    print(f"entries {entries.sum()}, two-piece tracks "
          f"{int((entries + (frac > 0) >= 2).sum())}, misses "
          f"{int((frac == 0).sum())}")
    assert (entries == 2).sum() > 100 and (frac == 0).sum() > 300
    assert s["track_entries"] == entries.sum()
    assert s["track_misses"] == (frac == 0).sum()
    length = np.linalg.norm(d - o, axis=1)
    want = (w * length * frac).sum()
    assert abs(eng.flux().sum() - want) <= 1e-12 * want
    # vacuum-face currents: w times the exits before the track's end
    want_leak = (w * exits).sum()
    assert abs(eng.leakage() - want_leak) <= 1e-12 * want_leak


def test_hand_checked_track_through_the_cavity():
    _, sub, _, _, _, _, _, _ = shell(False)
    o = np.array([[0.2, 2.37, 2.61]])
    d = np.array([[4.9, 2.41, 2.58]])
    w = np.array([1.25])
    eng = pt.TallyEngine(sub, 1, device="cpu", currents=True)
    eng.tally_tracks(o, d, w)
    want = 2.0 * np.linalg.norm(d - o) / 4.7
    assert abs(want - 2.0001131701797483) < 1e-15
    assert abs(eng.flux().sum() - want * 1.25) <= 1e-12 * want
    s = eng.stats()
    assert (s["track_entries"], s["track_misses"]) == (2, 0)
    assert abs(eng.leakage() - 2 * 1.25) <= 1e-15


def test_grouped_and_scored():
    _, _, keep, _, _, _, _, _ = shell(True)
    ref = oracle(True, grouped=True)
    eng = tracked(True, grouped=True)
    assert eng.flux().shape == (2, 2, 156)
    close(eng.flux(), ref.flux()[..., keep])
    # null responses: score 0 only
    _, sub, _, o, d, w, grp, _ = shell(True)
    e2 = pt.TallyEngine(sub, 1, device="cpu", ngroups=2, nscores=2)
    e2.tally_tracks(o, d, w, grp)
    close(e2.flux()[0].sum(axis=0), oracle(True).flux()[keep])
    assert not e2.flux()[1].any()


def test_linear_moments():
    _, _, keep, _, _, _, _, _ = shell(True)
    ref = oracle(True, linear=True)
    eng = tracked(True, linear=True)
    close(eng.moments().sum(axis=-1), eng.flux())
    close(eng.moments(), ref.moments()[keep])
    close(eng.flux(), ref.flux()[keep])


def test_currents():
    _, sub, keep, _, _, _, _, _ = shell(True)
    ref = oracle(True, currents=True)
    eng = tracked(True, currents=True)
    J, Jref = eng.currents(), ref.currents()[keep]
    interior = np.asarray(sub.neighbors).reshape(-1, 4) >= 0
    close(J[interior], Jref[interior])
    # a kept element's face towards a void is a vacuum face of the shell;
    # the oracle books the same departures there
    close(J[~interior], Jref[~interior])
    assert abs(eng.leakage() - Jref[~interior].sum()) <= GATE * eng.leakage()
    close(eng.flux(), ref.flux()[keep])


def test_fp32_traversal(monkeypatch):
    monkeypatch.setenv("PUMITALLY_WALK", "fp32")
    _, _, keep, _, _, _, _, _ = shell(True)
    ref = oracle(True)
    eng = tracked(True)
    close(eng.flux(), ref.flux()[keep])
    assert eng.stats()["lost_particles"] == 0


def _reflective_cavity_shell():
    _, sub, _, _, _, _, _, _ = shell(False)
    m = pt.mesh_from_arrays(np.asarray(sub.coords).ravel(),
                            np.asarray(sub.tet2vert).ravel())
    fid, cen, _ = m.boundary_faces()
    wall = np.all((cen > 1.5) & (cen < 3.5), axis=1)
    assert wall.sum() == 12                      # 6 sides x 2 triangles
    m.set_reflective_faces(fid[wall])
    return m


def test_reflective_cavity_wall():
    m = _reflective_cavity_shell()
    rng = np.random.default_rng(5)
    # from inside the cavity nothing gets in: the wall reflects
    o = rng.uniform(2.05, 2.95, size=(200, 3))
    d = rng.uniform(0.1, 4.9, size=(200, 3))
    eng = pt.TallyEngine(m, 1, device="cpu")
    eng.tally_tracks(o, d, np.ones(200))
    s = eng.stats()
    assert (s["track_entries"], s["track_misses"]) == (0, 200)
    assert not eng.flux().any()
    # tracks that start in the shell within 0.5 of the cavity and are shorter
    # than 0.45 cannot reach the outer (vacuum) boundary: whatever the wall
    # reflects, their whole length is tallied
    o = rng.uniform(1.55, 3.45, size=(3000, 3))
    o = o[~np.all((o > 2.0) & (o < 3.0), axis=1)][:1500]
    v = rng.normal(size=o.shape)
    v *= (rng.uniform(0.2, 0.45, len(o)) / np.linalg.norm(v, axis=1))[:, None]
    w = rng.uniform(0.5, 1.5, len(o))
    d = o + v
    hits = int(np.all((d > 2.0) & (d < 3.0), axis=1).sum())
    assert hits > 50                             # the wall is exercised
    eng = pt.TallyEngine(m, 1, device="cpu")
    eng.tally_tracks(o, d, w)
    want = (w * np.linalg.norm(v, axis=1)).sum()
    assert abs(eng.flux().sum() - want) <= 1e-12 * want
    s = eng.stats()
    assert (s["track_entries"], s["track_misses"], s["lost_particles"]) == \
        (0, 0, 0)
    # with a vacuum wall the same tracks lose what lies in the cavity
    _, sub, _, _, _, _, _, _ = shell(False)
    vac = pt.TallyEngine(sub, 1, device="cpu")
    vac.tally_tracks(o, d, w)
    assert vac.flux().sum() < want * (1 - 1e-3)


def test_global_reflective_admits_nothing(monkeypatch):
    monkeypatch.setenv("PUMITALLY_BC", "reflective")
    eng = pt.TallyEngine(pt.build_box(1, 1, 1), 1, device="cpu")
    eng.tally_tracks(np.array([[-0.5, 0.4, 0.5]]), np.array([[1.2, 0.4, 0.5]]),
                     np.ones(1))
    s = eng.stats()
    assert (s["track_entries"], s["track_misses"]) == (0, 1)
    assert not eng.flux().any()


def test_end_batch_and_checkpoint(tmp_path):
    _, sub, _, _, _, _, _, _ = shell(True)
    eng = tracked(True, linear=True)
    f, mom = eng.flux().copy(), eng.moments().copy()
    path = str(tmp_path / "ck.npz")
    eng.save_checkpoint(path)
    back = pt.TallyEngine(sub, 3, device="cpu", linear=True)
    back.load_checkpoint(path)
    assert np.array_equal(back.flux(), f)
    assert np.array_equal(back.moments(), mom)
    eng.end_batch()
    assert not eng.flux().any() and not eng.moments().any()
    assert np.array_equal(eng._eng.batch_sum(), f.ravel())
    assert np.array_equal(eng.moment_sum(), mom)
    eng.write_tally_results(str(tmp_path / "out.vtk"))


def move_interleaved(device, with_tracks):
    """move, [tally_tracks,] move on one engine: (state, flux increments)."""
    _, sub, _, o, d, w, _, _ = shell(True)
    n = 500
    rng = np.random.default_rng(3)
    p0 = rng.uniform(1.05, 1.95, size=(n, 3))
    p1 = rng.uniform(0.5, 4.5, size=(n, 3))
    p2 = rng.uniform(0.5, 4.5, size=(n, 3))
    fly, pw = np.ones(n, np.int8), np.ones(n)
    eng = pt.TallyEngine(sub, n, device=device)
    eng.copy_initial_position(p0.ravel())
    eng.move(p0.ravel(), p1.ravel(), fly, pw)
    f1 = eng.flux().copy()
    if with_tracks:
        eng.tally_tracks(o, d, w)
    f2 = eng.flux().copy()
    eng.move(p1.ravel(), p2.ravel(), fly, pw)
    f3 = eng.flux().copy()
    state = (eng.positions().copy(), eng.elem_ids().copy(),
             eng.escaped().copy())
    return state, f1, f2 - f1, f3 - f2, eng.stats()


def test_move_is_unaffected():
    sa, fa1, tr, fa3, stats = move_interleaved("cpu", True)
    sb, fb1, zero, fb3, _ = move_interleaved("cpu", False)
    for x, y in zip(sa, sb):
        assert np.array_equal(x, y)
    assert np.array_equal(fa1, fb1) and not zero.any()
    close(fa3, fb3)
    close(tr, tracked(True).flux())
    assert stats["moves"] == 2 and stats["tracks"] == N


def test_partition_cut_mesh_is_refused():
    mesh = pt.build_box(3, 3, 3)
    owners = pt._core.partition_morton(mesh, 2)
    part = pt._core.extract_submesh(mesh, owners, 0)
    eng = pt.TallyEngine(part.local, 1, device="cpu")
    for _ in range(2):                           # the answer is cached
        with pytest.raises(ValueError):
            eng.tally_tracks(np.zeros((1, 3)), np.ones((1, 3)), np.ones(1))
    assert eng.stats()["tracks"] == 0


def test_lost_track_is_counted_and_recorded():
    _, sub, _, o, d, w, _, _ = shell(True)
    eng = pt.TallyEngine(sub, 1, device="cpu")
    eng.max_steps = 1
    eng.tally_tracks(o[:50], d[:50], w[:50])
    s = eng.stats()
    rec = eng.lost_records()
    assert s["lost_particles"] > 0
    assert len(rec) == min(s["lost_particles"], 16)
    assert set(rec[:, 0].astype(int)) <= set(range(50))


# --------------------------------------------------------------------- GPU

class _U16View:
    """int16 torch storage presented as the uint16 array it holds."""

    def __init__(self, t):
        self.t = t
        self.__cuda_array_interface__ = dict(t.__cuda_array_interface__,
                                             typestr="<u2")


def same_counters(a, b):
    for k in ("tracks", "track_entries", "track_misses", "lost_particles",
              "loose_localizations"):
        assert a[k] == b[k], k


@pytest.mark.gpu
def test_gpu_golden_cube():
    golden("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 65, N])
def test_gpu_shell_matches_cpu(n):
    _, sub, _, o, d, w, _, _ = shell(True)
    gpu = tracked(True, n=n, device="cuda")
    cpu = tracked(True, n=n)
    if n == 0:
        assert not gpu.flux().any()
    else:
        close(gpu.flux(), cpu.flux())
    same_counters(gpu.stats(), cpu.stats())
    # the device-resident twin, torch tensors
    import torch
    dev = pt.TallyEngine(sub, 3, device="cuda")
    dev.tally_tracks_from_device(torch.from_numpy(o[:n].copy()).cuda(),
                                 torch.from_numpy(d[:n].copy()).cuda(),
                                 torch.from_numpy(w[:n].copy()).cuda())
    dev.synchronize()
    if n:
        close(dev.flux(), cpu.flux())
    same_counters(dev.stats(), cpu.stats())


@pytest.mark.gpu
def test_gpu_unjittered_shell_counters():
    gpu, cpu = tracked(False, device="cuda"), tracked(False)
    close(gpu.flux(), cpu.flux())
    same_counters(gpu.stats(), cpu.stats())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["grouped", "linear", "currents", "fp32"])
def test_gpu_options(mode, monkeypatch):
    kw = {}
    if mode == "fp32":
        monkeypatch.setenv("PUMITALLY_WALK", "fp32")
    elif mode == "grouped":
        kw["grouped"] = True
    else:
        kw[mode] = True
    gpu, cpu = tracked(True, device="cuda", **kw), tracked(True, **kw)
    close(gpu.flux(), cpu.flux())
    if mode == "linear":
        close(gpu.moments(), cpu.moments())
    if mode == "currents":
        close(gpu.currents(), cpu.currents())
    same_counters(gpu.stats(), cpu.stats())
    if mode == "grouped":
        import torch
        _, sub, _, o, d, w, grp, resp = shell(True)
        dev = pt.TallyEngine(sub, 3, device="cuda", ngroups=2, nscores=2)
        dev.tally_tracks_from_device(
            torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(),
            torch.from_numpy(w).cuda(),
            groups=_U16View(torch.from_numpy(grp.view(np.int16)).cuda()),
            responses=torch.from_numpy(resp).cuda())
        dev.synchronize()
        close(dev.flux(), cpu.flux())


@pytest.mark.gpu
def test_gpu_reflective_cavity_wall():
    m = _reflective_cavity_shell()
    rng = np.random.default_rng(6)
    o = rng.uniform(1.2, 3.8, size=(1000, 3))
    d = rng.uniform(0.1, 4.9, size=(1000, 3))
    w = rng.uniform(0.5, 1.5, 1000)
    gpu = pt.TallyEngine(m, 1, device="cuda")
    cpu = pt.TallyEngine(m, 1, device="cpu")
    for e in (gpu, cpu):
        e.tally_tracks(o, d, w)
    close(gpu.flux(), cpu.flux())
    same_counters(gpu.stats(), cpu.stats())


@pytest.mark.gpu
def test_gpu_interleaved_with_move():
    sg, g1, gt, g3, gs = move_interleaved("cuda", True)
    sc, c1, ct, c3, cs = move_interleaved("cpu", True)
    for x, y in zip(sg, sc):
        assert np.array_equal(x, y)
    close(g1, c1)
    close(gt, ct)
    close(g3, c3)
    same_counters(gs, cs)
    assert gs["moves"] == 2
