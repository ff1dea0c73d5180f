"""Collision-estimator tallies: TallyEngine(collisions=True).

A second, flux-shaped tally filled only by the explicit scoring calls
(docs/DESIGN.md, "Collision-estimator tallies"): score_collisions() scores
every active particle at the element the engine holds for it,
score_points() localizes free points and scores them.  A particle or point
that is not in the mesh adds nothing and counts as a miss.

Weights (and responses) are small integers (1..4) wherever exact equality is
asked for, so every sum is exact in fp64 whatever the order of the adds, and
"equal" means np.array_equal.

Oracle: no planes and no localization.  A point is BUILT inside a chosen tet
t from barycentric weights 0.8*Dirichlet(1,1,1,1) + 0.05, so its containing
element is t by construction and the expected tally is np.bincount(t, w).
Every test asserts the precondition elem_ids() == t before the tally.
"""
import functools

import numpy as np
import pytest

import pumiumtally_amd as pt

OFF = "collision tallies are off: create the engine with collisions=true"
MESHES = [(3, 3, 3), (4, 3, 2)]


# ---------------------------------------------------------------- helpers ---

@functools.lru_cache(maxsize=None)
def _mesh(dims):
    return pt.build_box(*dims)


def _built_points(mesh, n, seed, tets=None):
    """(t, p): n tets and one point strictly inside each."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, mesh.nelems, n) if tets is None else \
        np.asarray(tets)
    lam = 0.8 * rng.dirichlet(np.ones(4), n) + 0.05
    X = np.asarray(mesh.coords)[np.asarray(mesh.tet2vert)[t]]    # (n, 4, 3)
    return t.astype(np.int64), (lam[:, :, None] * X).sum(axis=1)


def _int_weights(n, seed):
    return np.random.default_rng(seed).integers(1, 5, n).astype(np.float64)


def _bincount(mesh, t, w, ngroups=1, nscores=1, groups=None, responses=None):
    """Expected tally, flat [nscores x ngroups x nelems]."""
    ne = mesh.nelems
    g = np.zeros(len(t), np.int64) if groups is None else \
        groups.astype(np.int64) % ngroups
    out = np.zeros(nscores * ngroups * ne)
    for k in range(nscores):
        wk = w if responses is None else w * responses[:, k]
        if responses is None and k > 0:
            break
        out += np.bincount((k * ngroups + g) * ne + t, weights=wk,
                           minlength=out.size)
    return out


def _engine(mesh, n, device="cpu", **kw):
    kw.setdefault("collisions", True)
    return pt.TallyEngine(mesh, n, device=device, **kw)


def _placed(mesh, p, device="cpu", **kw):
    eng = _engine(mesh, len(p), device, **kw)
    eng.copy_initial_position(p.ravel())
    return eng


def _moved_to(mesh, p, seed, device="cpu", **kw):
    """Engine whose particles flew from uniform interior origins to p."""
    n = len(p)
    o = np.random.default_rng(seed).uniform(0.05, 0.95, size=(n, 3))
    eng = _placed(mesh, o, device, **kw)
    eng.move(o.ravel(), p.ravel(), np.ones(n, np.int8), np.ones(n))
    return eng


def _state(eng):
    return (np.asarray(eng.positions()).copy().view(np.uint64),
            np.asarray(eng.elem_ids()).copy(),
            np.asarray(eng.escaped()).copy())


def _same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _outside(p):
    return ~((p > 0.0) & (p < 1.0)).all(axis=1)


# ------------------------------------------------------- 1. off by default

def test_off_by_default():
    m = _mesh((1, 1, 1))
    n = 4
    eng = pt.TallyEngine(m, n, device="cpu")
    assert eng.collision_tallies is False
    assert _engine(m, n).collision_tallies is True
    a, w, p = np.ones(n, np.int8), np.ones(n), np.full((n, 3), 0.5)
    calls = [lambda: eng.score_collisions(a, w),
             lambda: eng.score_points(p, w),
             lambda: eng.score_collisions_from_device(a, w),
             lambda: eng.score_points_from_device(p, w),
             eng.collisions, eng.collision_sum, eng.collision_sum_sq,
             eng.collision_statistics,
             # the layer below raises the same error on its own
             lambda: eng._eng.score_collisions(a, w),
             lambda: eng._eng.score_points(p.ravel(), w),
             lambda: eng._eng.score_collisions_device(0, 0),
             lambda: eng._eng.score_points_device(0, 0, 0),
             eng._eng.collisions, eng._eng.collision_sum,
             eng._eng.collision_sum_sq,
             lambda: eng._eng.set_collisions(np.zeros(m.nelems))]
    for call in calls:
        with pytest.raises(RuntimeError, match=OFF):
            call()
    st = eng.stats()
    assert st["collisions_scored"] == 0 and st["collision_misses"] == 0


def test_device_twins_need_the_gpu_engine():
    m = _mesh((1, 1, 1))
    eng = _engine(m, 4)
    with pytest.raises(RuntimeError, match="requires the GPU engine"):
        eng._eng.score_collisions_device(0, 0)
    with pytest.raises(RuntimeError, match="requires the GPU engine"):
        eng._eng.score_points_device(0, 0, 0)


# ---------------------------------------------------------- 2. golden cube

def test_golden_cube():
    m = _mesh((1, 1, 1))
    n = 5
    o = np.tile([0.1, 0.4, 0.5], (n, 1))
    d = np.tile([1.2, 0.4, 0.5], (n, 1))
    eng = _placed(m, o)
    a, w = np.ones(n, np.int8), np.arange(1.0, n + 1)
    eng.score_collisions(a, w)
    want = np.zeros(m.nelems)
    want[2] = w.sum()
    assert np.array_equal(eng.collisions(), want)
    assert eng.stats()["collisions_scored"] == n
    assert eng.stats()["collision_misses"] == 0
    # after the move they sit on the vacuum face they left through
    eng.move(o.ravel(), d.ravel(), np.ones(n, np.int8), np.ones(n))
    assert eng.escaped().all()
    eng.score_collisions(a, w)
    assert np.array_equal(eng.collisions(), want)
    assert eng.stats()["collisions_scored"] == n
    assert eng.stats()["collision_misses"] == n


# ------------------------------------------------- 3. score_points, oracle

@pytest.mark.parametrize("dims", MESHES)
def test_score_points_matches_oracle(dims):
    m = _mesh(dims)
    n = 5000
    t, p = _built_points(m, n, seed=7)
    w = _int_weights(n, 8)
    # precondition: the engine's localization puts every point in its t
    assert np.array_equal(_placed(m, p).elem_ids(), t)
    eng = _engine(m, 3)              # n is independent of num_particles
    eng.score_points(p, w)
    assert np.array_equal(eng.collisions(), _bincount(m, t, w))
    st = eng.stats()
    assert st["collisions_scored"] == n and st["collision_misses"] == 0
    before = eng.collisions().copy()
    eng.score_points(np.empty((0, 3)), np.empty(0))
    assert np.array_equal(eng.collisions(), before)
    assert eng.stats()["collisions_scored"] == n


# ------------------------------------ 4. score_collisions after a real move

@pytest.mark.parametrize("dims", MESHES)
def test_score_collisions_after_move(dims):
    m = _mesh(dims)
    n = 5000
    t, p = _built_points(m, n, seed=7)
    w = _int_weights(n, 9)
    eng = _moved_to(m, p, seed=10)
    assert np.array_equal(eng.elem_ids(), t)
    assert not eng.escaped().any() and eng.stats()["lost_particles"] == 0
    active = (np.random.default_rng(11).random(n) < 0.5).astype(np.int8)
    keep, state = active.copy(), _state(eng)
    eng.score_collisions(active, w)
    on = active != 0
    assert np.array_equal(eng.collisions(), _bincount(m, t[on], w[on]))
    assert np.array_equal(active, keep)
    assert _same_state(_state(eng), state)
    st = eng.stats()
    assert st["collisions_scored"] == on.sum() and st["collision_misses"] == 0


# ---------------------------------------------------------------- 5. misses

def test_misses_after_leaving_moves():
    m = _mesh((3, 3, 3))
    n = 5000
    rng = np.random.default_rng(12)
    o = rng.uniform(0.05, 0.95, size=(n, 3))
    d = rng.uniform(-0.3, 1.3, size=(n, 3))
    w = _int_weights(n, 13)
    eng = _placed(m, o)
    eng.move(o.ravel(), d.ravel(), np.ones(n, np.int8), np.ones(n))
    active = (rng.random(n) < 0.7).astype(np.int8)
    on = active != 0
    # escaped particles, then unlocated ones (placed outside the mesh)
    for want_unlocated in (False, True):
        esc, el = eng.escaped() != 0, eng.elem_ids()
        gone = esc | (el < 0)
        assert 0 < (gone & on).sum() < on.sum()
        assert (el < 0).any() == want_unlocated
        eng.score_collisions(active, w)
        st = eng.stats()
        assert st["collision_misses"] == \
            (esc & on).sum() + ((el < 0) & on).sum()
        assert st["collisions_scored"] == (on & ~gone).sum()
        hit = on & ~gone
        assert np.array_equal(eng.collisions(),
                              _bincount(m, el[hit], w[hit]))
        eng = _placed(m, d)


def test_misses_of_outside_points():
    m = _mesh((3, 3, 3))
    n = 5000
    p = np.random.default_rng(7).uniform(-0.3, 1.3, size=(n, 3))
    w = _int_weights(n, 14)
    out = _outside(p)
    located = _placed(m, p).elem_ids()
    assert np.array_equal(located < 0, out)      # what the engine locates
    eng = _engine(m, 1)
    eng.score_points(p, w)
    st = eng.stats()
    assert st["collision_misses"] == out.sum() > 0
    assert st["collisions_scored"] == n - out.sum()
    assert np.array_equal(eng.collisions(),
                          _bincount(m, located[~out], w[~out]))


# ------------------------------------------------------ 6. groups and scores

def _grouped_case(m, n, seed):
    rng = np.random.default_rng(seed)
    groups = rng.integers(0, 7, n).astype(np.uint16)     # wraps: % ngroups
    resp = rng.integers(1, 5, size=(n, 2)).astype(np.float64)
    return groups, resp


def test_groups_and_scores():
    m = _mesh((4, 3, 2))
    n, G, S = 5000, 3, 2
    t, p = _built_points(m, n, seed=7)
    w = _int_weights(n, 15)
    groups, resp = _grouped_case(m, n, 16)
    eng = _placed(m, p, ngroups=G, nscores=S)
    assert np.array_equal(eng.elem_ids(), t)
    a = np.ones(n, np.int8)
    eng.score_collisions(a, w, groups=groups, responses=resp)
    c = eng.collisions()
    assert c.shape == (S, G, m.nelems) == np.asarray(eng.flux()).shape
    want = _bincount(m, t, w, G, S, groups, resp)
    assert np.array_equal(c.ravel(), want)
    assert all(c[:, g].sum() > 0 for g in range(G))
    # the same through score_points
    pts = _engine(m, 1, ngroups=G, nscores=S)
    pts.score_points(p, w, groups=groups, responses=resp)
    assert np.array_equal(pts.collisions().ravel(), want)
    # null responses: score 0 only
    null = _placed(m, p, ngroups=G, nscores=S)
    null.score_collisions(a, w, groups=groups)
    cn = null.collisions()
    assert np.array_equal(cn.ravel(), _bincount(m, t, w, G, S, groups))
    assert cn[0].sum() == w.sum() and not cn[1].any()
    # one dimension only
    for kw, shape in (({"ngroups": G}, (G, m.nelems)),
                      ({"nscores": S}, (S, m.nelems))):
        assert _engine(m, 1, **kw).collisions().shape == shape


# ------------------------------------------------- 7. other tallies untouched

def _move_score_twice(m, seed, scoring, device="cpu", **kw):
    n = 800
    rng = np.random.default_rng(seed)
    a, b, c = (rng.uniform(0.05, 0.95, size=(n, 3)) for _ in range(3))
    w = rng.uniform(0.5, 2.0, n)
    act = (rng.random(n) < 0.5).astype(np.int8)
    eng = _placed(m, a, device, **kw)
    fl = np.ones(n, np.int8)
    for o, d in ((a, b), (b, c)):
        eng.move(o.ravel(), d.ravel(), fl, w)
        if scoring:
            eng.score_collisions(act, w)
            eng.score_points(d[:100], w[:100])
    return eng


@pytest.mark.parametrize("extra", [{}, {"linear": True}, {"currents": True}])
def test_other_tallies_untouched(extra):
    m = _mesh((3, 3, 3))
    scoring = _move_score_twice(m, 17, True, **extra)
    silent = _move_score_twice(m, 17, False, **extra)
    plain = _move_score_twice(m, 17, False, collisions=False, **extra)
    assert scoring.collisions().sum() > 0 and not silent.collisions().any()
    f = np.asarray(scoring.flux())
    assert f.sum() > 0
    assert np.array_equal(f, silent.flux())
    assert np.array_equal(f, plain.flux())
    assert _same_state(_state(scoring), _state(plain))
    if "linear" in extra:
        assert scoring.moments().sum() > 0
        assert np.array_equal(scoring.moments(), plain.moments())
    if "currents" in extra:
        assert scoring.currents().sum() > 0
        assert np.array_equal(scoring.currents(), plain.currents())


# ---------------------------------------------------------------- 8. batches

def test_batches():
    m = _mesh((3, 3, 3))
    n = 600
    t, p = _built_points(m, n, seed=18)
    eng = _placed(m, p)
    assert np.array_equal(eng.elem_ids(), t)
    a = np.ones(n, np.int8)
    loads = []
    for b in range(3):
        w = _int_weights(n, 19 + b) * (b + 1)
        for _ in range(b + 1):
            eng.score_collisions(a, w)
        loads.append((b + 1) * _bincount(m, t, w))
        assert np.array_equal(eng.collisions(), loads[-1])
        eng.end_batch()
        assert not eng.collisions().any()
    loads = np.array(loads)
    s1, s2 = loads.sum(axis=0), (loads * loads).sum(axis=0)
    assert np.array_equal(eng.collision_sum(), s1)
    assert np.array_equal(eng.collision_sum_sq(), s2)
    mean, rel = eng.collision_statistics()
    want_mean = s1 / 3
    var = np.maximum(s2 / 3 - want_mean * want_mean, 0.0)
    sem = np.sqrt(var / 2)
    want_rel = np.divide(sem, np.abs(want_mean), out=np.zeros_like(sem),
                         where=want_mean != 0)
    assert np.array_equal(mean, want_mean) and np.array_equal(rel, want_rel)
    assert mean.shape == (m.nelems,) and rel.max() > 0
    # the flux statistics are their own
    assert not eng._eng.batch_sum().any()


def test_statistics_need_a_batch():
    eng = _engine(_mesh((1, 1, 1)), 2)
    with pytest.raises(RuntimeError, match="no batches"):
        eng.collision_statistics()


# ------------------------------------------------------------- 9. checkpoint

def test_checkpoint_round_trip(tmp_path):
    m = _mesh((3, 3, 3))
    n = 500
    t, p = _built_points(m, n, seed=22)
    groups, resp = _grouped_case(m, n, 23)
    eng = _placed(m, p, ngroups=3, nscores=2)
    eng.score_collisions(np.ones(n, np.int8), _int_weights(n, 24),
                         groups=groups, responses=resp)
    want = eng.collisions()
    assert want.sum() > 0
    path = str(tmp_path / "ck.npz")
    eng.save_checkpoint(path)
    assert "collisions" in np.load(path).files
    back = _engine(m, n, ngroups=3, nscores=2)
    back.load_checkpoint(path)
    assert np.array_equal(back.collisions(), want)
    assert np.array_equal(back.elem_ids(), t)
    # a checkpoint written without the key: zeros, no error
    old = pt.TallyEngine(m, n, device="cpu", ngroups=3, nscores=2)
    old.copy_initial_position(p.ravel())
    opath = str(tmp_path / "old.npz")
    old.save_checkpoint(opath)
    assert "collisions" not in np.load(opath).files
    fresh = _engine(m, n, ngroups=3, nscores=2)
    fresh.load_checkpoint(opath)
    assert not fresh.collisions().any()
    assert np.array_equal(fresh.elem_ids(), t)
    # and an engine without the option ignores the key
    old.load_checkpoint(path)


# -------------------------------------------------------- 10. VTK and VTU

def _vtk_cell_field(text, name, nelems):
    assert f"CELL_DATA {nelems}" in text
    lines = text.split("\n")
    at = lines.index(f"SCALARS {name} double 1")
    assert lines[at + 1] == "LOOKUP_TABLE default"
    return np.array([float(x) for x in lines[at + 2:at + 2 + nelems]])


def _vtk_names(text):
    return [ln.split()[1] for ln in text.split("\n")
            if ln.startswith("SCALARS")]


def _scored_for_files(m, **kw):
    n = 400
    t, p = _built_points(m, n, seed=25)
    G, S = kw.get("ngroups", 1), kw.get("nscores", 1)
    groups, resp = _grouped_case(m, n, 26)
    run = {}
    if G > 1:
        run["groups"] = groups
    if S > 1:
        run["responses"] = resp
    eng = _moved_to(m, p, seed=27, **kw)
    eng.score_collisions(np.ones(n, np.int8), _int_weights(n, 28), **run)
    return eng


@pytest.mark.parametrize("kw", [{}, {"ngroups": 3}, {"nscores": 2},
                                {"ngroups": 3, "nscores": 2},
                                {"linear": True}, {"currents": True},
                                {"currents": True, "ngroups": 3}])
def test_vtk_has_collision_fields(tmp_path, kw):
    m = _mesh((2, 2, 2))
    eng = _scored_for_files(m, **kw)
    G, S = eng.ngroups, eng.nscores
    out = tmp_path / "coll.vtk"
    eng.write_tally_results(str(out))
    text = out.read_text()
    c = eng.collisions().reshape(S, G, m.nelems)
    vol = np.asarray(m.volumes)
    want = {}
    for k in range(S):
        stem = "collisions" if k == 0 else f"collisions_score{k}"
        want[stem] = c[k].sum(axis=0) / vol
        if G > 1:
            for g in range(G):
                want[f"{stem}_g{g}"] = c[k, g] / vol
    names = _vtk_names(text)
    assert [x for x in names if x.startswith("collisions")] == list(want)
    for name, vals in want.items():
        assert vals.sum() > 0
        assert np.array_equal(_vtk_cell_field(text, name, m.nelems), vals)
    # the other fields are exactly the ones an engine without the option
    # writes, and that engine's file has no such field
    _, p = _built_points(m, 400, seed=25)
    plain = _moved_to(m, p, seed=27, collisions=False, **kw)
    pout = tmp_path / "plain.vtk"
    plain.write_tally_results(str(pout))
    ptext = pout.read_text()
    assert "collisions" not in ptext
    assert [x for x in names if x not in want] == _vtk_names(ptext)
    assert np.array_equal(_vtk_cell_field(text, "flux", m.nelems),
                          _vtk_cell_field(ptext, "flux", m.nelems))
    if "linear" in kw:
        assert "nodal_flux" in text
    if "currents" in kw:
        assert "leakage" in names


def test_plain_engine_file_is_unchanged(tmp_path):
    """collisions=False writes byte for byte what write_tally_vtk writes."""
    m = _mesh((2, 2, 2))
    _, p = _built_points(m, 400, seed=25)
    plain = _moved_to(m, p, seed=27, collisions=False)
    a, b = tmp_path / "a.vtk", tmp_path / "b.vtk"
    plain.write_tally_results(str(a))
    pt.write_tally_vtk(str(b), m, plain.flux())
    assert a.read_bytes() == b.read_bytes()


def _vtu_cell_array(raw, name):
    head, _, app = raw.partition(b'<AppendedData encoding="raw">_')
    text = head.decode()
    assert "<CellData" in text
    line = [ln for ln in text.split("\n") if f'Name="{name}"' in ln][0]
    off = int(line.split('offset="')[1].split('"')[0])
    nbytes = int(np.frombuffer(app[off:off + 8], np.uint64)[0])
    return np.frombuffer(app[off + 8:off + 8 + nbytes], np.float64)


@pytest.mark.parametrize("kw", [{}, {"ngroups": 3, "nscores": 2}])
def test_vtu_has_collision_fields(tmp_path, kw):
    m = _mesh((2, 2, 2))
    eng = _scored_for_files(m, **kw)
    G, S = eng.ngroups, eng.nscores
    out = tmp_path / "coll.vtu"
    eng.write_tally_results(str(out))
    raw = out.read_bytes()
    c = eng.collisions().reshape(S, G, m.nelems)
    vol = np.asarray(m.volumes)
    assert np.array_equal(_vtu_cell_array(raw, "collisions"),
                          c[0].sum(axis=0) / vol)
    if kw:
        assert np.array_equal(_vtu_cell_array(raw, "collisions_g2"),
                              c[0, 2] / vol)
        assert np.array_equal(_vtu_cell_array(raw, "collisions_score1"),
                              c[1].sum(axis=0) / vol)
        assert np.array_equal(_vtu_cell_array(raw, "collisions_score1_g0"),
                              c[1, 0] / vol)
    _, p = _built_points(m, 400, seed=25)
    plain = _moved_to(m, p, seed=27, collisions=False, **kw)
    pout = tmp_path / "plain.vtu"
    plain.write_tally_results(str(pout))
    assert b"collisions" not in pout.read_bytes()


# ------------------------------------------------- 11. size and dtype errors

def test_bad_arguments_raise_and_tally_nothing():
    m = _mesh((3, 3, 3))
    n = 50
    _, p = _built_points(m, n, seed=29)
    eng = _placed(m, p, ngroups=3, nscores=2)
    a, w = np.ones(n, np.int8), np.ones(n)
    g, r = np.zeros(n, np.uint16), np.ones((n, 2))
    bad = [
        lambda: eng.score_collisions(a[:-1], w),
        lambda: eng.score_collisions(a, w[:-1]),
        lambda: eng.score_collisions(a, w, groups=g[:-1]),
        lambda: eng.score_collisions(a, w, responses=r[:, :1]),
        lambda: eng.score_collisions(a.astype(np.int32), w),
        lambda: eng.score_collisions(a.astype(bool), w),
        lambda: eng.score_collisions(a, w.astype(np.float32)),
        lambda: eng.score_points(p[:-1], w),
        lambda: eng.score_points(p, w[:-1]),
        lambda: eng.score_points(p, w, groups=g[:-1]),
        lambda: eng.score_points(p, w, responses=r[:-1]),
        lambda: eng.score_points(p.astype(np.float32), w),
        lambda: eng.score_points(p, w.astype(np.int64)),
        lambda: eng._eng.set_collisions(np.zeros(m.nelems)),
    ]
    for call in bad:
        with pytest.raises((RuntimeError, TypeError, ValueError)):
            call()
    assert not eng.collisions().any()
    st = eng.stats()
    assert st["collisions_scored"] == 0 and st["collision_misses"] == 0


# ------------------------------------------------------- 12. real weights

def _real_case(dims=(3, 3, 3)):
    m = _mesh(dims)
    n = 5000
    t, p = _built_points(m, n, seed=7)
    w = np.random.default_rng(30).uniform(0.1, 3.0, n)
    return m, t, p, w


def test_real_weights():
    """A sum of m non-negative terms in any order has relative error at most
    (m-1)*2^-53: 5.6e-13 for m = 5000, inside rtol = 1e-12."""
    m, t, p, w = _real_case()
    assert np.array_equal(_placed(m, p).elem_ids(), t)
    eng = _engine(m, 1)
    eng.score_points(p, w)
    assert np.allclose(eng.collisions(), _bincount(m, t, w), rtol=1e-12,
                       atol=0)


# ------------------------------------------------------------------- GPU ---

@functools.lru_cache(maxsize=None)
def _points_case(dims, n):
    """Points, weights and the CPU engine's result; shared, never mutated."""
    m = _mesh(dims)
    t, p = _built_points(m, n, seed=7)
    w = _int_weights(n, 31)
    assert np.array_equal(_placed(m, p).elem_ids(), t)
    cpu = _engine(m, 1)
    cpu.score_points(p, w)
    return m, t, p, w, cpu.collisions(), cpu.stats()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 5000])
def test_gpu_score_points(n):
    """(a) partial waves, one wave, several blocks."""
    dims = MESHES[n % 2]
    m, t, p, w, cpu, cst = _points_case(dims, n)
    gpu = _engine(m, 1, "cuda:0")
    gpu.score_points(p, w)
    got = gpu.collisions()
    assert np.array_equal(got, cpu)
    assert np.array_equal(got, _bincount(m, t, w))
    st = gpu.stats()
    assert st["collisions_scored"] == cst["collisions_scored"] == n
    assert st["collision_misses"] == 0
    gpu.score_points(np.empty((0, 3)), np.empty(0))
    assert np.array_equal(gpu.collisions(), cpu)


@pytest.mark.gpu
@pytest.mark.parametrize("dims", MESHES)
def test_gpu_score_collisions_across_resort(dims):
    """(b) random caller order, so the slot map is a real permutation after
    the sort; 17 chained moves cross the default re-sort cadence of 16."""
    m = _mesh(dims)
    n = 5000
    rng = np.random.default_rng(32)
    fl = np.ones(n, np.int8)
    ones = np.ones(n)
    w = _int_weights(n, 33)
    masks = [np.ones(n, np.int8), np.zeros(n, np.int8),
             (np.arange(n) % 2).astype(np.int8),
             (rng.random(n) < 0.5).astype(np.int8)]
    _, prev = _built_points(m, n, seed=34)
    engines = [_placed(m, prev, dev) for dev in ("cpu", "cuda:0")]
    want = np.zeros(m.nelems)
    for k in range(17):
        _, nxt = _built_points(m, n, seed=35 + k)
        for e in engines:
            e.move(prev.ravel(), nxt.ravel(), fl, ones)
        prev = nxt
        if k == 4:                       # one score call before the re-sort
            for e in engines:
                e.score_collisions(masks[3], w)
            el = engines[0].elem_ids()
            on = masks[3] != 0
            want += np.bincount(el[on], weights=w[on], minlength=m.nelems)
    cpu, gpu = engines
    # the chained moves start from committed positions, which the move
    # precondition of the CPU tests does not cover: compare the engines
    el = cpu.elem_ids()
    assert np.array_equal(gpu.elem_ids(), el)
    assert (el >= 0).all() and not cpu.escaped().any()
    assert not gpu.escaped().any()
    for mask in masks:
        for e in engines:
            e.score_collisions(mask, w)
        on = mask != 0
        want += np.bincount(el[on], weights=w[on], minlength=m.nelems)
        assert np.array_equal(gpu.collisions(), cpu.collisions())
        assert np.array_equal(gpu.collisions(), want)
    for key in ("collisions_scored", "collision_misses"):
        assert gpu.stats()[key] == cpu.stats()[key]
    assert gpu.stats()["collision_misses"] == 0
    assert np.array_equal(gpu.elem_ids(), el)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [130, 4097])
def test_gpu_hot_element(n):
    """(c) every particle in one tet: runs span wave and block boundaries."""
    m = _mesh((3, 3, 3))
    hot = 40
    t, p = _built_points(m, n, seed=36, tets=np.full(n, hot))
    w = _int_weights(n, 37)
    gpu = _placed(m, p, "cuda:0")
    assert np.array_equal(gpu.elem_ids(), t)
    gpu.score_collisions(np.ones(n, np.int8), w)
    want = np.zeros(m.nelems)
    want[hot] = w.sum()
    assert np.array_equal(gpu.collisions(), want)
    gpu.score_points(p, w)
    assert np.array_equal(gpu.collisions(), 2 * want)
    assert gpu.stats()["collisions_scored"] == 2 * n


@pytest.mark.gpu
@pytest.mark.parametrize("grouped", [False, True])
def test_gpu_grouped_and_plain_paths(grouped):
    """(d) groups/responses take the plain-atomic kernels, the bare call the
    run-aggregated ones."""
    m = _mesh((4, 3, 2))
    n, G, S = 5000, 3, 2
    t, p = _built_points(m, n, seed=7)
    w = _int_weights(n, 38)
    groups, resp = _grouped_case(m, n, 39)
    run = dict(groups=groups, responses=resp) if grouped else {}
    a = (np.random.default_rng(40).random(n) < 0.8).astype(np.int8)
    cpu = _moved_to(m, p, seed=41, ngroups=G, nscores=S)
    gpu = _moved_to(m, p, seed=41, device="cuda:0", ngroups=G, nscores=S)
    assert np.array_equal(cpu.elem_ids(), t)
    assert np.array_equal(gpu.elem_ids(), t)
    on = a != 0
    want = _bincount(m, t[on], w[on], G, S, groups[on] if grouped else None,
                     resp[on] if grouped else None)
    for e in (cpu, gpu):
        e.score_collisions(a, w, **run)
    assert np.array_equal(cpu.collisions().ravel(), want)
    assert np.array_equal(gpu.collisions().ravel(), want)
    want = want + _bincount(m, t, w, G, S, groups if grouped else None,
                            resp if grouped else None)
    for e in (cpu, gpu):
        e.score_points(p, w, **run)
    assert np.array_equal(cpu.collisions().ravel(), want)
    assert np.array_equal(gpu.collisions().ravel(), want)
    if grouped:                          # null responses, groups alone
        for e in (cpu, gpu):
            e.score_collisions(a, w, groups=groups)
        assert np.array_equal(gpu.collisions(), cpu.collisions())
    gpu.end_batch()
    assert not gpu.collisions().any()
    assert np.array_equal(gpu.collision_sum(), cpu.collisions())
    assert np.array_equal(gpu.collision_sum_sq(), cpu.collisions() ** 2)


class _U16View:
    """int16 torch storage presented as the uint16 array it holds."""

    def __init__(self, t):
        self.t = t
        self.__cuda_array_interface__ = dict(t.__cuda_array_interface__,
                                             typestr="<u2")


@pytest.mark.gpu
@pytest.mark.parametrize("grouped", [False, True])
def test_gpu_device_twins(grouped):
    """(e) torch tensors through the device entries equal the host calls."""
    import torch

    m = _mesh((3, 3, 3))
    n, G, S = 3000, 3, 2
    t, p = _built_points(m, n, seed=42)
    w = _int_weights(n, 43)
    groups, resp = _grouped_case(m, n, 44)
    a = (np.random.default_rng(45).random(n) < 0.5).astype(np.int8)
    host = _placed(m, p, "cuda:0", ngroups=G, nscores=S)
    dev = _placed(m, p, "cuda:0", ngroups=G, nscores=S)
    assert np.array_equal(dev.elem_ids(), t)
    d = torch.device("cuda:0")
    t_a, t_w = torch.from_numpy(a).to(d), torch.from_numpy(w).to(d)
    t_p = torch.from_numpy(p).to(d)
    t_g = _U16View(torch.from_numpy(groups.view(np.int16)).to(d))
    t_r = torch.from_numpy(resp).to(d)
    hrun = dict(groups=groups, responses=resp) if grouped else {}
    drun = dict(groups=t_g, responses=t_r) if grouped else {}
    host.score_collisions(a, w, **hrun)
    dev.score_collisions_from_device(t_a, t_w, **drun)
    assert host.collisions().sum() > 0
    assert np.array_equal(dev.collisions(), host.collisions())
    host.score_points(p[:777], w[:777], **{k: v[:777] for k, v in hrun.items()})
    t_g7 = _U16View(t_g.t[:777].contiguous())
    drun7 = dict(groups=t_g7, responses=t_r[:777].contiguous()) \
        if grouped else {}
    dev.score_points_from_device(t_p[:777].contiguous(),
                                 t_w[:777].contiguous(), **drun7)
    assert np.array_equal(dev.collisions(), host.collisions())
    assert dev.stats()["collisions_scored"] == \
        host.stats()["collisions_scored"]
    before = dev.collisions().copy()
    bad = [
        lambda: dev.score_collisions_from_device(t_a.to(torch.int32), t_w),
        lambda: dev.score_collisions_from_device(t_a, t_w.to(torch.float32)),
        lambda: dev.score_collisions_from_device(t_a[:-1], t_w),
        lambda: dev.score_collisions_from_device(a, w),      # host arrays
        lambda: dev.score_collisions_from_device(
            torch.ones(2 * n, dtype=torch.int8, device=d)[::2], t_w),
        lambda: dev.score_points_from_device(t_p.to(torch.float32), t_w),
        lambda: dev.score_points_from_device(t_p.t(), t_w),  # not contiguous
        lambda: dev.score_points_from_device(t_p[:-1], t_w),
    ]
    for call in bad:
        with pytest.raises(TypeError):
            call()
    assert np.array_equal(dev.collisions(), before)


def _dyadic_ends(m, n, seed):
    """Two points per particle inside one tet, on a 2^-16 lattice and
    2^-9 apart along x: every track length, hence every flux contribution
    with integer weights, is a dyadic number and every flux sum is exact
    whatever order the device adds in."""
    t, p = _built_points(m, n, seed)
    a = np.round(p * 65536.0) / 65536.0
    b = a + np.array([2.0 ** -9, 0.0, 0.0])
    return t, a, b


@pytest.mark.gpu
def test_gpu_elision_untouched():
    """(f) score calls between chained moves leave origin elision and the
    flux alone."""
    m = _mesh((3, 3, 3))
    n = 4000
    t, a, b = _dyadic_ends(m, n, seed=46)
    w = _int_weights(n, 47)
    fl = np.ones(n, np.int8)
    act = (np.random.default_rng(48).random(n) < 0.5).astype(np.int8)
    scoring = _placed(m, a, "cuda:0")
    silent = _placed(m, a, "cuda:0")
    plain = _placed(m, a, "cuda:0", collisions=False)
    ends = (a, b)
    for k in range(6):
        o, d = ends[k % 2], ends[(k + 1) % 2]
        for e in (scoring, silent, plain):
            e.move(o.ravel().copy(), d.ravel().copy(), fl, w)
        scoring.score_collisions(act, w)
        scoring.score_points(d[:500], w[:500])
    for e in (scoring, silent, plain):
        assert np.array_equal(e.elem_ids(), t)
    f = np.asarray(scoring.flux())
    assert np.array_equal(f, np.bincount(t, weights=6 * w * 2.0 ** -9,
                                         minlength=m.nelems))
    assert np.array_equal(f, silent.flux())
    assert np.array_equal(f, plain.flux())
    elided = scoring.stats()["origins_elided"]
    assert elided == 5 * n
    assert silent.stats()["origins_elided"] == elided
    assert plain.stats()["origins_elided"] == elided
    on = act != 0
    assert np.array_equal(
        scoring.collisions(),
        6 * (np.bincount(t[on], weights=w[on], minlength=m.nelems)
             + np.bincount(t[:500], weights=w[:500], minlength=m.nelems)))
    assert not silent.collisions().any()


@pytest.mark.gpu
def test_gpu_counters_match_cpu():
    """(g) misses and scored, particles and points."""
    m = _mesh((3, 3, 3))
    n = 5000
    rng = np.random.default_rng(49)
    o = rng.uniform(0.05, 0.95, size=(n, 3))
    d = rng.uniform(-0.3, 1.3, size=(n, 3))
    w = _int_weights(n, 50)
    act = (rng.random(n) < 0.7).astype(np.int8)
    fl = np.ones(n, np.int8)
    cpu, gpu = _placed(m, o), _placed(m, o, "cuda:0")
    for e in (cpu, gpu):
        e.move(o.ravel(), d.ravel(), fl, np.ones(n))
    assert np.array_equal(gpu.elem_ids(), cpu.elem_ids())
    assert np.array_equal(gpu.escaped(), cpu.escaped())
    assert cpu.escaped().any()
    for e in (cpu, gpu):
        e.score_collisions(act, w)
    c0, g0 = cpu.stats(), gpu.stats()
    assert c0["collision_misses"] > 0 and c0["collisions_scored"] > 0
    # unlocated particles: placed outside the mesh
    for e in (cpu, gpu):
        e.copy_initial_position(d.ravel())
    assert np.array_equal(gpu.elem_ids(), cpu.elem_ids())
    assert (cpu.elem_ids() < 0).any()
    for e in (cpu, gpu):
        e.score_collisions(act, w)
    c1, g1 = cpu.stats(), gpu.stats()
    assert c1["collision_misses"] > c0["collision_misses"]
    for e in (cpu, gpu):
        e.score_points(d, w)
    c2, g2 = cpu.stats(), gpu.stats()
    assert c2["collision_misses"] - c1["collision_misses"] == _outside(d).sum()
    for key in ("collisions_scored", "collision_misses"):
        assert g0[key] == c0[key] and g1[key] == c1[key]
        assert g2[key] == c2[key]
    assert np.array_equal(gpu.collisions(), cpu.collisions())
    assert np.array_equal(gpu.elem_ids(), cpu.elem_ids())


@pytest.mark.gpu
def test_gpu_real_weights():
    """(h) the bound of test_real_weights."""
    m, t, p, w = _real_case()
    want = _bincount(m, t, w)
    gpu = _placed(m, p, "cuda:0")
    assert np.array_equal(gpu.elem_ids(), t)
    gpu.score_points(p, w)
    assert np.allclose(gpu.collisions(), want, rtol=1e-12, atol=0)
    gpu.end_batch()
    gpu.score_collisions(np.ones(len(w), np.int8), w)
    assert np.allclose(gpu.collisions(), want, rtol=1e-12, atol=0)
