"""Face-current tallies: TallyEngine(currents=True).

For every tallied crossing where the walk leaves element e through local face
f, the particle's weight is added to J[e, f] (docs/DESIGN.md, "Face-current
tallies"): the outward partial current J+ integrated over the face.  The
final partial segment of a track counts nothing.

Weights (and responses) are small integers wherever exact equality is asked
for, so every sum is exact in fp64 whatever the order of the adds.

Oracle: a numpy routine that uses NO face planes -- per tet it inverts
[[x0..x3],[1,1,1,1]] for the barycentric coordinates of both end points,
clips t to the interval where all four stay non-negative, and books the
weight on the local vertex whose coordinate is smallest (zero) at the exit.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import pumiumtally_amd as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- helpers ---

def oracle_currents(mesh, o, d, w, tie=1e-9):
    """Plane-free currents of the segments o->d: ((nelems, 4) array,
    crossings, dropped crossings, smallest gap seen)."""
    X = np.asarray(mesh.coords)[np.asarray(mesh.tet2vert)]      # (ne, 4, 3)
    ne = X.shape[0]
    A = np.concatenate([X.transpose(0, 2, 1), np.ones((ne, 1, 4))], axis=1)
    Ainv = np.linalg.inv(A)
    out = np.zeros((ne, 4))
    crossings = dropped = 0
    gap = np.inf
    for i in range(len(w)):
        l0 = Ainv @ np.append(o[i], 1.0)
        l1 = Ainv @ np.append(d[i], 1.0)
        dl = l1 - l0
        with np.errstate(divide="ignore", invalid="ignore"):
            tx = -l0 / dl
        t0 = np.where(dl > 0, tx, 0.0).max(axis=1).clip(min=0.0)
        t1 = np.where(dl < 0, tx, 1.0).min(axis=1).clip(max=1.0)
        never = ((dl == 0) & (l0 < 0)).any(axis=1)
        hit = np.flatnonzero((t1 > t0) & ~never & (t1 < 1.0))
        lb = l0[hit] + t1[hit, None] * dl[hit]
        srt = np.sort(lb, axis=1)
        g = min((srt[:, 1] - srt[:, 0]).min(initial=np.inf),
                (t1[hit] - t0[hit]).min(initial=np.inf))
        gap = min(gap, g)
        crossings += len(hit)
        if g < tie:
            dropped += len(hit)
            continue
        out[hit, lb.argmin(axis=1)] += w[i]
    return out, crossings, dropped, gap


def _int_segments(n, seed, leave=True):
    rng = np.random.default_rng(seed)
    o = rng.uniform(0.05, 0.95, size=(n, 3))
    d = rng.uniform(-0.3, 1.3, size=(n, 3)) if leave else \
        rng.uniform(0.05, 0.95, size=(n, 3))
    w = rng.integers(1, 5, n).astype(np.float64)
    return o, d, w, rng


def _moved(mesh, o, d, w, device="cpu", currents=True, **kw):
    n = len(w)
    groups = kw.pop("groups", None)
    responses = kw.pop("responses", None)
    eng = pt.TallyEngine(mesh, n, device=device, currents=currents, **kw)
    eng.copy_initial_position(o.ravel())
    eng.move(o.ravel(), d.ravel(), np.ones(n, np.int8), w, groups=groups,
             responses=responses)
    eng.synchronize()
    return eng


def _periodic_x_box(nx=3, ny=3, nz=3):
    m = pt.build_box(nx, ny, nz)
    fid, cen, _ = m.boundary_faces()
    hi = fid[np.abs(cen[:, 0] - 1.0) < 1e-12]
    lo = fid[np.abs(cen[:, 0] - 0.0) < 1e-12]
    m.set_periodic_faces(hi, lo, np.array([-1.0, 0.0, 0.0]))
    return m


# ------------------------------------------------------------ 1. golden cube

def test_golden_cube_currents():
    m = pt.build_box(1, 1, 1)
    n = 5
    o = np.tile([0.1, 0.4, 0.5], (n, 1))
    d = np.tile([1.2, 0.4, 0.5], (n, 1))
    eng = _moved(m, o, d, np.ones(n))
    nbr = np.asarray(m.neighbors)
    fid, cen, _ = m.boundary_faces()
    x1 = [int(f) for f, c in zip(fid, cen) if f // 4 == 4 and abs(c[0] - 1) < 1e-12]
    assert len(x1) == 1
    want = np.zeros((m.nelems, 4))
    want[2, list(nbr[2]).index(3)] = 5.0
    want[3, list(nbr[3]).index(4)] = 5.0
    want[4, x1[0] % 4] = 5.0
    J = eng.currents()
    assert J.shape == (m.nelems, 4)
    assert np.array_equal(J, want)
    assert np.count_nonzero(J) == 3
    assert eng.leakage() == 5
    # the particles escaped and are not relocated: a second identical move
    # adds nothing (leaving again where they sit is the same departure)
    eng.move(o.ravel(), d.ravel(), np.ones(n, np.int8), np.ones(n))
    assert np.array_equal(eng.currents(), want)


def test_face_twins_and_areas():
    m = pt.build_box(2, 2, 2)
    tw = np.asarray(m.face_twins)
    nbr = np.asarray(m.neighbors)
    assert tw.shape == (m.nelems, 4) and tw.dtype == np.int64
    assert np.array_equal(tw >= 0, nbr >= 0)
    has = np.flatnonzero(tw.ravel() >= 0)
    assert np.array_equal(tw.ravel()[tw.ravel()[has]], has)      # involution
    assert np.array_equal(tw.ravel()[has] // 4, nbr.ravel()[has])
    ar = np.asarray(m.face_areas)
    assert ar.shape == (m.nelems, 4)
    assert np.array_equal(ar.ravel()[tw.ravel()[has]], ar.ravel()[has])
    fid, _, _ = m.boundary_faces()
    assert abs(ar.ravel()[fid].sum() - 6.0) < 1e-12              # unit cube
    p = _periodic_x_box(2, 2, 2)
    ptw = np.asarray(p.face_twins).ravel()
    pf, cen, _ = p.boundary_faces()
    for f, c in zip(pf, cen):
        if abs(c[0]) < 1e-12 or abs(c[0] - 1) < 1e-12:
            assert ptw[f] >= 0 and ptw[ptw[f]] == f
        else:
            assert ptw[f] == -1


# ----------------------------------------------------- 2. plane-free oracle

@pytest.mark.parametrize("cells", [3, 4])
def test_currents_match_plane_free_oracle(cells):
    m = pt.build_box(cells, cells, cells)
    o, d, w, _ = _int_segments(400, seed=7)
    eng = _moved(m, o, d, w)
    ref, crossings, dropped, gap = oracle_currents(m, o, d, w)
    print(f"cells {cells}: crossings {crossings} dropped {dropped} "
          f"smallest gap {gap:.2e} leaving {int(eng.escaped().sum())}")
    assert dropped <= 0.01 * crossings
    if dropped == 0:
        assert np.array_equal(eng.currents(), ref)
    else:
        # a dropped segment is missing from the oracle as a whole
        assert (eng.currents() >= ref).all()
        assert eng.currents().sum() - ref.sum() <= 4 * dropped
    assert eng.stats()["lost_particles"] == 0


# -------------------------------------------------------- 3. element balance

def _check_balance(eng, mesh, o, w):
    J = eng.currents().reshape(-1)
    twins, refl, _ = eng._face_classes()
    ne = mesh.nelems
    out = np.where(refl, 0.0, J).reshape(ne, 4).sum(axis=1)
    has = twins >= 0
    inflow = np.bincount(twins[has] // 4, weights=J[has], minlength=ne)
    born = np.bincount(mesh.locate(o), weights=w, minlength=ne)
    stay = ~eng.escaped().astype(bool)
    stopped = np.bincount(eng.elem_ids()[stay], weights=w[stay], minlength=ne)
    assert eng.stats()["lost_particles"] == 0
    assert J.sum() > 0
    assert np.array_equal(out - inflow, born - stopped)


def test_element_balance_vacuum():
    m = pt.build_box(3, 3, 3)
    o, d, w, _ = _int_segments(300, seed=61)
    eng = _moved(m, o, d, w)
    assert eng.escaped().sum() > 0
    _check_balance(eng, m, o, w)


def test_element_balance_per_face_reflective():
    m = pt.build_box(3, 3, 3)
    fid, cen, _ = m.boundary_faces()
    side = fid[np.abs(cen[:, 0] - 1.0) < 1e-12]
    m.set_reflective_faces(side)
    o, d, w, _ = _int_segments(300, seed=62)
    eng = _moved(m, o, d, w)
    assert eng.escaped().sum() > 0
    J = eng.currents().reshape(-1)
    assert J[side].sum() > 0                  # the outward crossing is recorded
    assert not eng.net_current().reshape(-1)[side].any()
    _check_balance(eng, m, o, w)


def test_element_balance_fp32_traversal(monkeypatch):
    monkeypatch.setenv("PUMITALLY_WALK", "fp32")
    m = pt.build_box(3, 3, 3)
    o, d, w, _ = _int_segments(300, seed=63)
    eng = _moved(m, o, d, w)
    assert eng.escaped().sum() > 0
    _check_balance(eng, m, o, w)


# ---------------------------------------------------------------- 4. leakage

def test_leakage_is_escaped_weight():
    m = pt.build_box(3, 3, 3)
    o, d, w, _ = _int_segments(300, seed=64)
    eng = _moved(m, o, d, w)
    esc = eng.escaped().astype(bool)
    assert esc.sum() > 50
    assert eng.leakage() == w[esc].sum()
    # net current on a vacuum face is the current itself
    fid, _, _ = m.boundary_faces()
    assert np.array_equal(eng.net_current().reshape(-1)[fid],
                          eng.currents().reshape(-1)[fid])


def test_leakage_zero_under_global_reflective(monkeypatch):
    monkeypatch.setenv("PUMITALLY_BC", "reflective")
    m = pt.build_box(3, 3, 3)
    o, d, w, _ = _int_segments(300, seed=65)
    eng = _moved(m, o, d, w)
    assert eng.escaped().sum() == 0
    assert eng.leakage() == 0
    fid, _, _ = m.boundary_faces()
    assert eng.currents().reshape(-1)[fid].sum() > 0
    assert not eng.net_current().reshape(-1)[fid].any()


# --------------------------------------------------------- 5. periodic x-box

def test_periodic_x_box_wraps_once():
    m = _periodic_x_box(4, 4, 4)
    n = 300
    o, d, w, rng = _int_segments(n, seed=66, leave=False)
    d[:, 0] = rng.uniform(1.05, 1.95, n)
    eng = _moved(m, o, d, w)
    assert eng.escaped().sum() == 0
    fid, cen, _ = m.boundary_faces()
    hi = fid[np.abs(cen[:, 0] - 1.0) < 1e-12]
    lo = fid[np.abs(cen[:, 0] - 0.0) < 1e-12]
    J = eng.currents().reshape(-1)
    assert J[hi].sum() == w.sum()
    assert J[lo].sum() == 0
    net = eng.net_current().reshape(-1)
    twins = np.asarray(m.face_twins).reshape(-1)
    assert np.array_equal(np.sort(twins[hi]), np.sort(lo))
    assert np.array_equal(net[hi], -net[twins[hi]])
    assert eng.leakage() == 0


# ----------------------------------------------------- 6. groups and scores

def test_scored_grouped_currents_match_reweighted_plain_runs():
    m = pt.build_box(3, 3, 3)
    n, S, G = 200, 3, 2
    o, d, w, rng = _int_segments(n, seed=67)
    resp = rng.uniform(0.0, 2.0, size=(n, S))
    grp = rng.integers(0, G, n).astype(np.uint16)
    eng = _moved(m, o, d, w, ngroups=G, nscores=S, groups=grp, responses=resp)
    got = eng.currents()
    assert got.shape == (S, G, m.nelems, 4)
    for k in range(S):
        for g in range(G):
            sel = grp == g
            ref = _moved(m, o[sel], d[sel], (w * resp[:, k])[sel]).currents()
            assert np.allclose(got[k, g], ref, rtol=0.0, atol=1e-12)
    lk = eng.leakage()
    assert lk.shape == (S, G)
    esc = eng.escaped().astype(bool)
    for k in range(S):
        for g in range(G):
            sel = esc & (grp == g)
            assert abs(lk[k, g] - (w * resp[:, k])[sel].sum()) < 1e-10
    assert _moved(m, o, d, w, ngroups=G, groups=grp).currents().shape == \
        (G, m.nelems, 4)


def test_scored_null_responses_currents_land_in_score0():
    m = pt.build_box(2, 2, 2)
    o, d, w, _ = _int_segments(80, seed=68)
    got = _moved(m, o, d, w, nscores=2).currents()
    ref = _moved(m, o, d, w).currents()
    assert ref.sum() > 0
    assert np.array_equal(got[0], ref)
    assert not got[1].any()


# -------------------------------------------------------------- 7. walk_raw

def test_walk_raw_matches_move():
    m = pt.build_box(3, 3, 3)
    n, S = 150, 2
    o, d, w, rng = _int_segments(n, seed=69)
    resp = rng.integers(1, 4, size=(n, S)).astype(np.float64)
    elem = m.locate(o).astype(np.int32)
    mv = _moved(m, o, d, w, nscores=S, responses=resp)
    raw = pt.TallyEngine(m, 1, device="cpu", nscores=S, currents=True)
    raw.walk_raw(o.ravel(), d.ravel(), elem, w, responses=resp)
    assert mv.currents().sum() > 0
    assert np.array_equal(raw.currents(), mv.currents())
    assert np.array_equal(raw.flux(), mv.flux())


# ------------------------------------------------------------ 8. cut in two

def test_walk_cut_in_two_matches_uncut_walk():
    """Cut every walk by hand at a submesh boundary and resume it on the
    other submesh from the exported handoff state, the way the partitioned
    driver does: the halves' currents add up to the uncut walk's, and a cut
    face is counted once -- by the sender."""
    from pumiumtally_amd import _core

    m = pt.build_box(4, 4, 4)
    cents = np.array([m.centroid(t) for t in range(m.nelems)])
    owners = (cents[:, 0] > 0.5).astype(np.int32)
    subs = [_core.extract_submesh(m, owners, p, 0) for p in range(2)]
    l2g = [np.asarray(s.elem_l2g) for s in subs]
    g2l = [np.full(m.nelems, -1, np.int64) for _ in range(2)]
    for p in range(2):
        g2l[p][l2g[p]] = np.arange(len(l2g[p]))
    engines = [pt.TallyEngine(s.local, 1, device="cpu", currents=True)
               for s in subs]

    n = 200
    o, d, w, _ = _int_segments(n, seed=33, leave=False)
    gids = m.locate(o)
    work = {}
    for p in range(2):
        sel = owners[gids] == p
        work[p] = dict(pos=o[sel], dst=d[sel], w=w[sel],
                       elem=g2l[p][gids[sel]].astype(np.int32),
                       in_t=None, in_prev=None)
    handoffs = 0
    handed_weight = 0.0
    for _ in range(32):
        nxt = {p: [] for p in range(2)}
        for p in range(2):
            k = work[p]
            if not len(k["w"]):
                continue
            (out_pos, out_elem, status, out_dest, out_o, out_t,
             out_prev) = engines[p].walk_raw(
                k["pos"].ravel(), k["dst"].ravel(), k["elem"], k["w"],
                in_t=k["in_t"], in_prev=k["in_prev"], resume=True)
            assert not (status == 3).any()
            for j in np.flatnonzero(status == 2):
                f = -(int(out_elem[j]) + 2)
                to = int(np.asarray(subs[p].foreign_owner)[f])
                tgt = int(np.asarray(subs[p].foreign_gid)[f])
                prev_gid = int(l2g[p][out_prev[j]])
                nxt[to].append((out_o[j], out_dest[j], k["w"][j],
                                g2l[to][tgt], out_t[j], g2l[to][prev_gid]))
                handoffs += 1
                handed_weight += k["w"][j]
        if not any(nxt.values()):
            break
        for p in range(2):
            r = nxt[p]
            work[p] = dict(
                pos=np.array([a[0] for a in r]).reshape(-1, 3),
                dst=np.array([a[1] for a in r]).reshape(-1, 3),
                w=np.array([a[2] for a in r], np.float64),
                elem=np.array([a[3] for a in r], np.int32),
                in_t=np.array([a[4] for a in r], np.float64),
                in_prev=np.array([a[5] for a in r], np.int32))
    else:
        raise AssertionError("handoff did not converge")
    assert handoffs > 50

    got = np.zeros((m.nelems, 4))
    on_cut = 0.0
    for p in range(2):
        J = engines[p].currents()
        got[l2g[p]] += J
        cut = np.asarray(subs[p].local.neighbors) < -1
        assert (np.asarray(subs[p].local.face_twins)[cut] == -1).all()
        on_cut += J[cut].sum()
    ref = _moved(m, o, d, w).currents()
    assert np.array_equal(got, ref)
    assert on_cut == handed_weight


# -------------------------------------------------- 9. threaded CPU path

_THREADED = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.environ["PT_ROOT"])
import pumiumtally_amd as pt

n, G, S = 70_000, 2, 2
mesh = pt.build_box(6, 6, 6, 1.0, 1.0, 1.0)
rng = np.random.default_rng(3)
pos = rng.uniform(0.05, 0.95, (n, 3))
dest = pos + rng.normal(0, 0.2, (n, 3))
w = rng.integers(1, 5, n).astype(np.float64)
grp = rng.integers(0, G, n).astype(np.uint16)
rsp = rng.integers(1, 4, (n, S)).astype(np.float64)
eng = pt.TallyEngine(mesh, n, device="cpu", ngroups=G, nscores=S,
                     currents=True)
eng.copy_initial_position(pos.ravel())
eng.move(pos.ravel(), dest.ravel(), np.ones(n, np.int8), w,
         groups=grp, responses=rsp)
raw = pt.TallyEngine(mesh, 1, device="cpu", ngroups=G, nscores=S,
                     currents=True)
raw.walk_raw(pos.ravel(), dest.ravel(), mesh.locate(pos).astype(np.int32), w,
             groups=grp, responses=rsp)
np.savez(os.environ["PT_OUT"], currents=eng.currents(),
         raw_currents=raw.currents(), leakage=eng.leakage())
print("MOVE_OK")
"""


def _run_threaded(tmp_path, threads, tag):
    out = str(tmp_path / f"cur_{tag}.npz")
    env = dict(os.environ)
    env["PT_ROOT"] = ROOT
    env["PT_OUT"] = out
    if threads is not None:
        env["PUMITALLY_CPU_THREADS"] = str(threads)
    r = subprocess.run([sys.executable, "-c", _THREADED], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (threads, r.stdout, r.stderr)
    assert "MOVE_OK" in r.stdout
    return np.load(out)


def test_threaded_cpu_currents_match_serial(tmp_path):
    """A batch large enough for the multithreaded CPU move (and walk_raw)
    with nscores > 1: per-thread partials must cover the currents' full
    shape.  In a subprocess, so an undersized partial kills the child."""
    mt = _run_threaded(tmp_path, None, "mt")  # hardware thread count
    st = _run_threaded(tmp_path, 1, "st")
    assert mt["currents"].shape == (2, 2, 6 * 6 * 6 * 6, 4)
    assert st["currents"].sum() > 0 and st["leakage"].sum() > 0
    assert np.array_equal(mt["currents"], st["currents"])
    # walk_raw threads on the hardware count alone (it ignores the override)
    assert np.array_equal(mt["raw_currents"], st["currents"])


# ------------------------------------------------ 10. batches and checkpoint

def test_end_batch_zeroes_and_sums_accumulate():
    m = pt.build_box(2, 2, 2)
    o, d, w, _ = _int_segments(80, seed=41, leave=False)
    eng = _moved(m, o, d, w)
    first = eng.currents().copy()
    assert first.sum() > 0
    assert not eng.current_sum().any() and not eng.current_sum_sq().any()
    eng.end_batch()
    assert not eng.currents().any()
    assert np.array_equal(eng.current_sum(), first)
    assert np.array_equal(eng.current_sum_sq(), first * first)
    eng.move(d.ravel(), o.ravel(), np.ones(80, np.int8), w)
    second = eng.currents().copy()
    assert second.sum() > 0
    eng.end_batch()
    assert np.array_equal(eng.current_sum(), first + second)
    assert np.array_equal(eng.current_sum_sq(), first ** 2 + second ** 2)
    # derived quantities from the batch sums
    assert np.array_equal(eng.net_current(eng.current_sum()).shape, first.shape)
    assert eng.leakage(eng.current_sum()) == 0


def test_checkpoint_round_trip_restores_currents(tmp_path):
    m = pt.build_box(2, 2, 2)
    o, d, w, _ = _int_segments(80, seed=42)
    eng = _moved(m, o, d, w)
    path = str(tmp_path / "cur.npz")
    eng.save_checkpoint(path)
    assert "currents" in np.load(path).files
    fresh = pt.TallyEngine(m, 80, device="cpu", currents=True)
    fresh.load_checkpoint(path)
    assert np.array_equal(fresh.currents(), eng.currents())
    assert np.array_equal(fresh.flux(), eng.flux())
    # checkpoints without the key (engines without the option, old files)
    plain = _moved(m, o, d, w, currents=False)
    ppath = str(tmp_path / "plain.npz")
    plain.save_checkpoint(ppath)
    assert "currents" not in np.load(ppath).files
    fresh2 = pt.TallyEngine(m, 80, device="cpu", currents=True)
    fresh2.load_checkpoint(ppath)
    assert np.array_equal(fresh2.flux(), plain.flux())
    assert not fresh2.currents().any()


def test_engine_without_the_option_raises():
    m = pt.build_box(2, 2, 2)
    eng = pt.TallyEngine(m, 4, device="cpu")
    assert eng.face_currents is False and eng._eng.face_currents is False
    for call in (eng.currents, eng.current_sum, eng.current_sum_sq,
                 eng.net_current, eng.leakage):
        with pytest.raises(RuntimeError, match="currents"):
            call()
    for call in (eng._eng.currents, eng._eng.current_sum,
                 eng._eng.current_sum_sq,
                 lambda: eng._eng.set_currents(np.zeros(m.nelems * 4))):
        with pytest.raises(RuntimeError, match="currents"):
            call()
    assert pt.TallyEngine(m, 4, device="cpu", currents=True).face_currents


def test_currents_with_linear_is_rejected():
    from pumiumtally_amd import _core

    m = pt.build_box(2, 2, 2)
    with pytest.raises(ValueError, match="linear"):
        pt.TallyEngine(m, 4, device="cpu", currents=True, linear=True)
    with pytest.raises(ValueError, match="linear"):
        _core.Engine(m, 4, "cpu", 1, 1, True, True)


def test_currents_flag_leaves_flux_bit_identical():
    m = pt.build_box(3, 3, 3)
    n, S, G = 200, 2, 2
    rng = np.random.default_rng(46)
    o = rng.uniform(0.05, 0.95, size=(n, 3))
    d = rng.uniform(0.05, 0.95, size=(n, 3))
    d[::7] = o[::7] + 1.5
    w = rng.uniform(0.1, 1.0, n)
    grp = rng.integers(0, G, n).astype(np.uint16)
    resp = rng.uniform(0.0, 2.0, size=(n, S))
    for kw in ({}, dict(ngroups=G, nscores=S, groups=grp, responses=resp)):
        a = _moved(m, o, d, w, currents=False, **kw)
        b = _moved(m, o, d, w, currents=True, **kw)
        assert np.array_equal(a.flux(), b.flux())
        assert np.array_equal(a.positions(), b.positions())
        assert np.array_equal(a.elem_ids(), b.elem_ids())
        assert np.array_equal(a.escaped(), b.escaped())


# ----------------------------------------------------------- 11. output files

def _vtk_cell_field(text, name, nelems):
    assert f"CELL_DATA {nelems}" in text
    lines = text.split("\n")
    at = lines.index(f"SCALARS {name} double 1")
    assert lines[at + 1] == "LOOKUP_TABLE default"
    return np.array([float(x) for x in lines[at + 2:at + 2 + nelems]])


def _element_leakage(eng):
    _, _, vac = eng._face_classes()
    ne = eng.mesh.nelems
    J = eng.currents().reshape(eng.nscores, eng.ngroups, ne, 4)
    return (J * vac.reshape(ne, 4)).sum(axis=-1)


@pytest.mark.parametrize("kw", [{}, {"ngroups": 2}, {"nscores": 2}])
def test_vtk_has_leakage_cell_field(tmp_path, kw):
    m = pt.build_box(2, 2, 2)
    n = 120
    o, d, w, rng = _int_segments(n, seed=43)
    run = dict(kw)
    if "ngroups" in kw:
        run["groups"] = rng.integers(0, 2, n).astype(np.uint16)
    if "nscores" in kw:
        run["responses"] = np.column_stack(
            [np.ones(n), rng.integers(1, 4, n).astype(np.float64)])
    eng = _moved(m, o, d, w, **run)
    out = tmp_path / "cur.vtk"
    eng.write_tally_results(str(out))
    text = out.read_text()
    lk = _element_leakage(eng)
    assert lk.sum() > 0
    assert np.array_equal(_vtk_cell_field(text, "leakage", m.nelems),
                          lk[0].sum(axis=0))
    if "ngroups" in kw:
        for g in range(2):
            assert np.array_equal(
                _vtk_cell_field(text, f"leakage_g{g}", m.nelems), lk[0, g])
    if "nscores" in kw:
        assert np.array_equal(
            _vtk_cell_field(text, "leakage_score1", m.nelems),
            lk[1].sum(axis=0))
    # the flux fields are the ones an engine without the option writes
    plain = _moved(m, o, d, w, currents=False, **run)
    pout = tmp_path / "plain.vtk"
    plain.write_tally_results(str(pout))
    ptext = pout.read_text()
    assert "leakage" not in ptext
    assert np.array_equal(_vtk_cell_field(text, "flux", m.nelems),
                          _vtk_cell_field(ptext, "flux", m.nelems))
    assert text.count("SCALARS") == 2 * ptext.count("SCALARS") - \
        (1 if not kw else 0)                     # "volume" has no twin


def test_vtu_has_leakage_cell_field(tmp_path):
    m = pt.build_box(2, 2, 2)
    o, d, w, _ = _int_segments(120, seed=44)
    eng = _moved(m, o, d, w)
    out = tmp_path / "cur.vtu"
    eng.write_tally_results(str(out))
    raw = out.read_bytes()
    head, _, app = raw.partition(b'<AppendedData encoding="raw">_')
    text = head.decode()
    assert "<CellData" in text and 'Name="leakage"' in text
    line = [ln for ln in text.split("\n") if 'Name="leakage"' in ln][0]
    off = int(line.split('offset="')[1].split('"')[0])
    nbytes = int(np.frombuffer(app[off:off + 8], np.uint64)[0])
    assert nbytes == m.nelems * 8
    vals = np.frombuffer(app[off + 8:off + 8 + nbytes], np.float64)
    assert vals.sum() > 0
    assert np.array_equal(vals, _element_leakage(eng)[0, 0])
    plain = _moved(m, o, d, w, currents=False)
    pout = tmp_path / "plain.vtu"
    plain.write_tally_results(str(pout))
    assert b"leakage" not in pout.read_bytes()


# ------------------------------------------------------------------- GPU ---

def _gpu_bound(ref):
    # reassociation of fp64 adds only (same reasoning and bound as the
    # linear-moment GPU tests)
    return 1e-10 * max(1.0, np.abs(ref).max())


def _assert_gpu_matches(gpu, cpu, exact):
    cj, gj = cpu.currents(), gpu.currents()
    cf, gf = np.asarray(cpu.flux()), np.asarray(gpu.flux())
    assert cj.sum() > 0
    ej, ef = np.abs(cj - gj).max(), np.abs(cf - gf).max()
    print(f"max |currents diff| {ej:.3e}  max |flux diff| {ef:.3e}")
    if exact:
        assert np.array_equal(gj, cj)
    else:
        assert ej < _gpu_bound(cj), ej
    assert ef < _gpu_bound(cf), ef
    assert gpu.stats()["lost_particles"] == 0


@functools.lru_cache(maxsize=None)
def _gpu_case(n, grouped, integer):
    """Inputs + CPU reference, computed once and shared (never mutated)."""
    m = pt.build_box(6, 6, 6)
    rng = np.random.default_rng(42 + n)
    o = rng.uniform(0.02, 0.98, size=(n, 3))
    d = rng.uniform(0.02, 0.98, size=(n, 3))
    d[::9] = o[::9] + rng.normal(0, 1.0, size=(len(d[::9]), 3))  # escapes
    w = rng.integers(1, 5, n).astype(np.float64) if integer else \
        rng.uniform(0.1, 1.0, n)
    kw = {}
    if grouped:
        resp = rng.integers(1, 4, size=(n, 3)).astype(np.float64) if integer \
            else rng.uniform(0.0, 2.0, size=(n, 3))
        kw = dict(ngroups=2, nscores=3,
                  groups=rng.integers(0, 2, n).astype(np.uint16),
                  responses=resp)
    return m, o, d, w, kw, _moved(m, o, d, w, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("integer", [True, False], ids=["integer", "real"])
@pytest.mark.parametrize("grouped", [False, True],
                         ids=["aggregated", "grouped_scored"])
@pytest.mark.parametrize("n", [20000, 1000])
def test_gpu_move_matches_cpu(n, grouped, integer):
    """Plain moves take the wave-aggregated currents kernel (aggregation is
    on by default); groups + responses take the plain-atomic one.  n=1000
    is no multiple of 64: partial waves."""
    m, o, d, w, kw, cpu = _gpu_case(n, grouped, integer)
    gpu = _moved(m, o, d, w, device="cuda:0", **kw)
    assert gpu.is_gpu
    _assert_gpu_matches(gpu, cpu, exact=integer)
    assert np.sum(cpu.leakage()) > 0
    if integer:
        assert np.array_equal(gpu.leakage(), cpu.leakage())


@pytest.mark.gpu
def test_gpu_clustered_source_matches_cpu():
    """All particles start inside one cell of the box: neighbouring lanes
    share elements, so the aggregated kernel sees run lengths above 1."""
    m = pt.build_box(6, 6, 6)
    n = 20000
    rng = np.random.default_rng(5)
    o = (np.array([2.0, 3.0, 1.0]) + rng.uniform(0.05, 0.95, (n, 3))) / 6.0
    d = o + rng.normal(0, 0.15, size=(n, 3))
    w = rng.integers(1, 5, n).astype(np.float64)
    cpu = _moved(m, o, d, w)
    gpu = _moved(m, o, d, w, device="cuda:0")
    _assert_gpu_matches(gpu, cpu, exact=True)
    # second move from the committed state + a batch close on device
    for e in (cpu, gpu):
        e.move_continue(o.ravel(), np.ones(n, np.int8), w)
    _assert_gpu_matches(gpu, cpu, exact=True)
    before = gpu.currents()
    gpu.end_batch()
    assert not gpu.currents().any()
    assert np.array_equal(gpu.current_sum(), before)
    assert np.array_equal(gpu.current_sum_sq(), before * before)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [20000, 1000])
def test_gpu_keyed_aggregation_matches_cpu(monkeypatch, n):
    """PUMITALLY_CURRENTS_AGG=1 (read per engine, at construction) books the
    currents through the run aggregation keyed on the flat face index
    instead of plain atomics; same result."""
    monkeypatch.setenv("PUMITALLY_CURRENTS_AGG", "1")
    m = pt.build_box(6, 6, 6)
    rng = np.random.default_rng(6 + n)
    o = (np.array([2.0, 3.0, 1.0]) + rng.uniform(0.05, 0.95, (n, 3))) / 6.0
    d = o + rng.normal(0, 0.3, size=(n, 3))
    w = rng.integers(1, 5, n).astype(np.float64)
    cpu = _moved(m, o, d, w)
    assert cpu.escaped().sum() > 0
    gpu = _moved(m, o, d, w, device="cuda:0")
    _assert_gpu_matches(gpu, cpu, exact=True)
    assert gpu.leakage() == cpu.leakage()


@pytest.mark.gpu
def test_gpu_walk_raw_matches_cpu():
    m = pt.build_box(5, 5, 5)
    n, S = 4000, 2
    rng = np.random.default_rng(51)
    o = rng.uniform(0.02, 0.98, size=(n, 3))
    d = rng.uniform(-0.2, 1.2, size=(n, 3))
    w = rng.integers(1, 5, n).astype(np.float64)
    resp = rng.integers(1, 4, size=(n, S)).astype(np.float64)
    elem = m.locate(o).astype(np.int32)
    cpu = pt.TallyEngine(m, 1, device="cpu", nscores=S, currents=True)
    cpu.walk_raw(o.ravel(), d.ravel(), elem, w, responses=resp)
    gpu = pt.TallyEngine(m, 1, device="cuda:0", nscores=S, currents=True)
    gpu.walk_raw(o.ravel(), d.ravel(), elem, w, responses=resp)
    gpu.synchronize()
    _assert_gpu_matches(gpu, cpu, exact=True)


@pytest.mark.gpu
def test_gpu_move_from_device_matches_move():
    import torch

    m, o, d, w, _, cpu = _gpu_case(1000, False, True)
    n = len(w)
    host = _moved(m, o, d, w, device="cuda:0")
    dev = torch.device("cuda:0")
    eng = pt.TallyEngine(m, n, device="cuda:0", currents=True)
    eng.copy_initial_position(o.ravel())
    eng.move_from_device(
        torch.from_numpy(d.ravel().copy()).to(dev),
        torch.ones(n, dtype=torch.int8, device=dev),
        torch.from_numpy(w.copy()).to(dev),
        origin=torch.from_numpy(o.ravel().copy()).to(dev))
    eng.synchronize()
    _assert_gpu_matches(eng, host, exact=True)
    _assert_gpu_matches(eng, cpu, exact=True)


@pytest.mark.gpu
def test_gpu_periodic_matches_cpu():
    m = _periodic_x_box(5, 5, 5)
    n = 5000
    rng = np.random.default_rng(77)
    o = rng.uniform(0.05, 0.95, size=(n, 3))
    d = o + np.column_stack([rng.uniform(0.5, 2.5, n),
                             rng.uniform(-0.02, 0.02, n),
                             rng.uniform(-0.02, 0.02, n)])
    d[:, 1:] = np.clip(d[:, 1:], 0.05, 0.95)
    w = rng.integers(1, 5, n).astype(np.float64)
    cpu = _moved(m, o, d, w)
    gpu = _moved(m, o, d, w, device="cuda:0")
    _assert_gpu_matches(gpu, cpu, exact=True)


_GPU_FP32 = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.environ["PT_ROOT"])
import pumiumtally_amd as pt

n = 5000
mesh = pt.build_box(6, 6, 6)
rng = np.random.default_rng(88)
o = rng.uniform(0.02, 0.98, (n, 3))
d = rng.uniform(0.02, 0.98, (n, 3))
d[::9] = o[::9] + rng.normal(0, 1.0, (len(d[::9]), 3))
w = rng.integers(1, 5, n).astype(np.float64)
out = {}
for dev in ("cpu", "cuda:0"):
    e = pt.TallyEngine(mesh, n, device=dev, currents=True)
    e.copy_initial_position(o.ravel())
    e.move(o.ravel(), d.ravel(), np.ones(n, np.int8), w)
    e.synchronize()
    assert e.stats()["lost_particles"] == 0
    out[dev] = (e.currents(), np.asarray(e.flux()), e.leakage())
assert out["cpu"][0].sum() > 0 and out["cpu"][2] > 0
assert np.array_equal(out["cpu"][0], out["cuda:0"][0])
assert out["cpu"][2] == out["cuda:0"][2]
ef = np.abs(out["cpu"][1] - out["cuda:0"][1]).max()
assert ef < 1e-10 * max(1.0, np.abs(out["cpu"][1]).max()), ef
print("FP32_OK")
"""


@pytest.mark.gpu
def test_gpu_fp32_traversal_matches_cpu():
    env = dict(os.environ)
    env["PT_ROOT"] = ROOT
    env["PUMITALLY_WALK"] = "fp32"
    r = subprocess.run([sys.executable, "-c", _GPU_FP32], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "FP32_OK" in r.stdout


@pytest.mark.gpu
def test_gpu_engine_without_the_option_raises_and_checkpoint(tmp_path):
    m, o, d, w, _, cpu = _gpu_case(1000, False, True)
    plain = pt.TallyEngine(m, 4, device="cuda:0")
    for call in (plain.currents, plain.current_sum, plain.current_sum_sq,
                 plain._eng.currents,
                 lambda: plain._eng.set_currents(np.zeros(m.nelems * 4))):
        with pytest.raises(RuntimeError, match="currents"):
            call()
    with pytest.raises(ValueError, match="linear"):
        pt.TallyEngine(m, 4, device="cuda:0", currents=True, linear=True)
    gpu = _moved(m, o, d, w, device="cuda:0")
    path = str(tmp_path / "gpu_cur.npz")
    gpu.save_checkpoint(path)
    fresh = pt.TallyEngine(m, len(w), device="cuda:0", currents=True)
    fresh.load_checkpoint(path)
    assert np.array_equal(fresh.currents(), gpu.currents())
    assert np.array_equal(fresh.currents(), cpu.currents())
