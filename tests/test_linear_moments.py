"""Linear (per-vertex) track-length moment tallies: TallyEngine(linear=True).

For every (element e, local vertex f) the walk tallies the first barycentric
moment of the track, m[e, f] = integral of weight * lambda_f dl, next to the
usual flux (docs/DESIGN.md, csrc/core/walk.h tet_moments).  The reference
has no higher-order tally; this is an extension like groups and scores.

Oracle: a numpy routine that uses NO face planes -- per tet it inverts
[[x0..x3],[1,1,1,1]] to get the barycentric coordinates of both segment
end points, clips t in [0,1] to the interval where all four stay
non-negative, and integrates the (linear) coordinates with the trapezoid
rule, which is exact.  Its sum over f reproduces flux() to ~1e-15, so the
1e-12 comparison bound is ~400x the fp64 noise.

Invariants used where no oracle applies (reflective / periodic / fp32
traversal): partition of unity (sum_f m_f == flux), non-negativity, the
mean of the element-local P1 coefficients equals flux/volume, and the
lumped nodal field integrates to the total track length.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import pumiumtally_amd as pt


# ---------------------------------------------------------------- helpers ---

def oracle_moments(mesh, o, d, w):
    """Plane-free moments of the segments o->d (weights w): (nelems, 4)."""
    X = np.asarray(mesh.coords)[np.asarray(mesh.tet2vert)]      # (ne, 4, 3)
    ne = X.shape[0]
    A = np.concatenate([X.transpose(0, 2, 1), np.ones((ne, 1, 4))], axis=1)
    Ainv = np.linalg.inv(A)                                      # (ne, 4, 4)
    out = np.zeros((ne, 4))
    for i in range(len(w)):
        l0 = Ainv @ np.append(o[i], 1.0)                         # (ne, 4)
        l1 = Ainv @ np.append(d[i], 1.0)
        dl = l1 - l0
        with np.errstate(divide="ignore", invalid="ignore"):
            tx = -l0 / dl
        t0 = np.where(dl > 0, tx, 0.0).max(axis=1).clip(min=0.0)
        t1 = np.where(dl < 0, tx, 1.0).min(axis=1).clip(max=1.0)
        # constant negative coordinate: the segment never enters the tet
        never = ((dl == 0) & (l0 < 0)).any(axis=1)
        ok = (t1 > t0) & ~never
        L = np.linalg.norm(d[i] - o[i])
        la = l0 + t0[:, None] * dl
        lb = l0 + t1[:, None] * dl
        out[ok] += (w[i] * L * (t1 - t0)[ok])[:, None] * 0.5 * (la + lb)[ok]
    return out


def _segments(n, seed, lo=0.05, hi=0.95):
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo, hi, size=(n, 3))
    d = rng.uniform(lo, hi, size=(n, 3))
    w = rng.uniform(0.1, 1.0, n)
    return o, d, w, rng


def _moved(mesh, o, d, w, device="cpu", linear=True, **kw):
    n = len(w)
    groups = kw.pop("groups", None)
    responses = kw.pop("responses", None)
    eng = pt.TallyEngine(mesh, n, device=device, linear=linear, **kw)
    eng.copy_initial_position(o.ravel())
    eng.move(o.ravel(), d.ravel(), np.ones(n, np.int8), w, groups=groups,
             responses=responses)
    eng.synchronize()
    return eng


def _lumped_volumes(mesh):
    t2v = np.asarray(mesh.tet2vert).reshape(-1)
    return np.bincount(t2v, weights=np.repeat(np.asarray(mesh.volumes) / 4, 4),
                       minlength=mesh.nverts)


def _check_invariants(eng):
    f = np.asarray(eng.flux())
    m = eng.moments()
    assert m.shape == f.shape + (4,)
    assert f.sum() > 0
    err = np.abs(m.sum(-1) - f).max()
    assert err <= 1e-12 * max(1.0, np.abs(f).max()), err
    assert m.min() >= -1e-12, m.min()
    assert np.allclose(eng.linear_coefficients().mean(-1),
                       eng.normalized_flux(), rtol=1e-12, atol=0.0)
    nodal = eng.nodal_flux()
    assert nodal.shape == f.shape[:-1] + (eng.mesh.nverts,)
    total = (nodal * _lumped_volumes(eng.mesh)).sum()
    assert abs(total - f.sum()) <= 1e-12 * f.sum(), (total, f.sum())


def _periodic_x_box(nx=3, ny=3, nz=3):
    m = pt.build_box(nx, ny, nz)
    fid, cen, _ = m.boundary_faces()
    hi = fid[np.abs(cen[:, 0] - 1.0) < 1e-12]
    lo = fid[np.abs(cen[:, 0] - 0.0) < 1e-12]
    m.set_periodic_faces(hi, lo, np.array([-1.0, 0.0, 0.0]))
    return m


# ------------------------------------------------------ 1. independent oracle

@pytest.mark.parametrize("cells", [3, 4])
def test_moments_match_plane_free_oracle(cells):
    m = pt.build_box(cells, cells, cells)
    o, d, w, _ = _segments(200, seed=100 + cells)
    eng = _moved(m, o, d, w)
    ref = oracle_moments(m, o, d, w)
    # the oracle itself reproduces the flux tally to fp64 noise
    assert np.abs(ref.sum(-1) - eng.flux()).max() < 1e-13
    assert np.allclose(eng.moments(), ref, rtol=0.0, atol=1e-12), \
        np.abs(eng.moments() - ref).max()


def test_moments_match_oracle_with_vacuum_clip():
    m = pt.build_box(3, 3, 3)
    o, d, w, rng = _segments(200, seed=7)
    out = np.arange(200) % 4 == 0      # a quarter of the destinations leave
    d[out] = o[out] + rng.normal(0, 1.0, size=(int(out.sum()), 3)) * 3.0
    far = out & ((d < 0).any(axis=1) | (d > 1).any(axis=1))
    assert far.sum() >= 40
    eng = _moved(m, o, d, w)
    assert eng.escaped().sum() == far.sum()
    ref = oracle_moments(m, o, d, w)
    assert np.allclose(eng.moments(), ref, rtol=0.0, atol=1e-12), \
        np.abs(eng.moments() - ref).max()


# ------------------------------------------------------------ 2. golden cube

def test_golden_cube_moments():
    m = pt.build_box(1, 1, 1)
    o = np.array([[0.1, 0.4, 0.5]])
    d = np.array([[1.2, 0.4, 0.5]])
    w = np.ones(1)
    eng = _moved(m, o, d, w)
    mom = eng.moments()
    assert mom.shape == (6, 4)
    ref = oracle_moments(m, o, d, w)
    assert np.allclose(mom, ref, rtol=0.0, atol=1e-12)
    # the pinned path 2 -> 3 -> 4 and its flux (test_engine_golden.py)
    expect = np.zeros(6)
    expect[[2, 3, 4]] = [0.3, 0.1, 0.5]
    assert np.allclose(mom.sum(-1), expect, rtol=0.0, atol=1e-12)
    assert np.count_nonzero(mom[[2, 3, 4]]) == 12
    assert not mom[[0, 1, 5]].any()


# ------------------------------------------- 3. invariants, every walk mode

def _leaving_segments(n, seed):
    o, d, w, rng = _segments(n, seed)
    d = o + rng.normal(0, 0.7, size=(n, 3))   # many leave the unit box
    return o, d, w


def test_invariants_global_reflective(monkeypatch):
    monkeypatch.setenv("PUMITALLY_BC", "reflective")
    m = pt.build_box(3, 3, 3)
    o, d, w = _leaving_segments(300, seed=21)
    eng = _moved(m, o, d, w)
    assert eng.escaped().sum() == 0
    seg = np.linalg.norm(d - o, axis=1)
    assert abs(eng.moments().sum() - (seg * w).sum()) < 1e-10
    _check_invariants(eng)


def test_invariants_per_face_reflective():
    m = pt.build_box(3, 3, 3)
    fid, cen, _ = m.boundary_faces()
    m.set_reflective_faces(fid[np.abs(cen[:, 0] - 1.0) < 1e-12])
    o, d, w = _leaving_segments(300, seed=22)
    eng = _moved(m, o, d, w)
    assert eng.escaped().sum() > 0           # the other five sides are vacuum
    _check_invariants(eng)


def test_invariants_periodic():
    m = _periodic_x_box(4, 4, 4)
    o, d, w, rng = _segments(300, seed=23)
    d = o + np.column_stack([rng.uniform(0.5, 2.5, 300),
                             rng.uniform(-0.02, 0.02, 300),
                             rng.uniform(-0.02, 0.02, 300)])
    d[:, 1:] = np.clip(d[:, 1:], 0.05, 0.95)
    eng = _moved(m, o, d, w)
    seg = np.linalg.norm(d - o, axis=1)
    assert abs(eng.moments().sum() - (seg * w).sum()) < 1e-10
    _check_invariants(eng)


def test_invariants_fp32_traversal(monkeypatch):
    monkeypatch.setenv("PUMITALLY_WALK", "fp32")
    m = _periodic_x_box(3, 3, 3)
    o, d, w = _leaving_segments(300, seed=24)
    d[:, 1:] = np.clip(d[:, 1:], 0.05, 0.95)
    eng = _moved(m, o, d, w)
    _check_invariants(eng)
    # moments are fp64 also under fp32 traversal: still the oracle's
    plain = pt.build_box(3, 3, 3)
    o2, d2, w2, _ = _segments(200, seed=25)
    e2 = _moved(plain, o2, d2, w2)
    ref = oracle_moments(plain, o2, d2, w2)
    assert np.allclose(e2.moments(), ref, rtol=0.0, atol=1e-12)


def test_invariants_groups_and_scores():
    m = pt.build_box(3, 3, 3)
    n, G, S = 300, 3, 2
    o, d, w = _leaving_segments(n, seed=26)
    rng = np.random.default_rng(27)
    grp = rng.integers(0, G, n).astype(np.uint16)
    resp = rng.uniform(0.2, 2.0, size=(n, S))
    eng = _moved(m, o, d, w, ngroups=G, nscores=S, groups=grp, responses=resp)
    assert eng.moments().shape == (S, G, m.nelems, 4)
    _check_invariants(eng)
    # grouped only / scored only shapes
    eg = _moved(m, o, d, w, ngroups=G, groups=grp)
    assert eg.moments().shape == (G, m.nelems, 4)
    _check_invariants(eg)
    es = _moved(m, o, d, w, nscores=S, responses=resp)
    assert es.moments().shape == (S, m.nelems, 4)
    _check_invariants(es)


# ------------------------------------------------------ 4. scores and groups

def test_scored_grouped_moments_match_reweighted_oracle():
    m = pt.build_box(3, 3, 3)
    n, S, G = 150, 3, 2
    o, d, w, rng = _segments(n, seed=9)
    resp = rng.uniform(0.0, 2.0, size=(n, S))
    grp = rng.integers(0, G, n).astype(np.uint16)
    got = _moved(m, o, d, w, ngroups=G, nscores=S, groups=grp,
                 responses=resp).moments()
    for k in range(S):
        ref = _moved(m, o, d, w * resp[:, k], ngroups=G, groups=grp).moments()
        assert np.allclose(got[k], ref, rtol=1e-12, atol=1e-14)
        for g in range(G):
            sel = grp == g
            orc = oracle_moments(m, o[sel], d[sel], (w * resp[:, k])[sel])
            assert np.allclose(got[k, g], orc, rtol=0.0, atol=1e-12)


def test_scored_null_responses_moments_land_in_score0():
    m = pt.build_box(2, 2, 2)
    o, d, w, _ = _segments(50, seed=11)
    got = _moved(m, o, d, w, nscores=2).moments()
    ref = _moved(m, o, d, w).moments()
    assert np.array_equal(got[0], ref)
    assert not got[1].any()


# -------------------------------------------------------------- 5. walk_raw

def test_walk_raw_matches_move():
    m = pt.build_box(3, 3, 3)
    n, S = 120, 2
    o, d, w, rng = _segments(n, seed=15)
    d[::5] = o[::5] + 2.0                       # some escape
    resp = rng.uniform(0.0, 2.0, size=(n, S))
    elem = m.locate(o).astype(np.int32)
    mv = _moved(m, o, d, w, nscores=S, responses=resp)
    raw = pt.TallyEngine(m, 1, device="cpu", nscores=S, linear=True)
    raw.walk_raw(o.ravel(), d.ravel(), elem, w, responses=resp)
    assert np.allclose(raw.moments(), mv.moments(), rtol=0.0, atol=1e-12)
    assert np.allclose(raw.flux(), mv.flux(), rtol=0.0, atol=1e-12)


def test_walk_cut_in_two_matches_uncut_walk():
    """Cut every walk by hand at a submesh boundary and resume it on the
    other submesh from the exported (out_o, out_t, out_prev) handoff state,
    the way the partitioned driver does: the two halves' moments add up to
    the uncut walk's."""
    from pumiumtally_amd import _core

    m = pt.build_box(4, 4, 4)
    cents = np.array([m.centroid(t) for t in range(m.nelems)])
    owners = (cents[:, 0] > 0.5).astype(np.int32)
    subs = [_core.extract_submesh(m, owners, p, 0) for p in range(2)]
    l2g = [np.asarray(s.elem_l2g) for s in subs]
    g2l = [np.full(m.nelems, -1, np.int64) for _ in range(2)]
    for p in range(2):
        g2l[p][l2g[p]] = np.arange(len(l2g[p]))
    engines = [pt.TallyEngine(s.local, 1, device="cpu", linear=True)
               for s in subs]

    n = 200
    o, d, w, _ = _segments(n, seed=33)
    gids = m.locate(o)
    work = {}
    for p in range(2):
        sel = owners[gids] == p
        work[p] = dict(pos=o[sel], dst=d[sel], w=w[sel],
                       elem=g2l[p][gids[sel]].astype(np.int32),
                       in_t=None, in_prev=None)
    handoffs = 0
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
    for p in range(2):
        got[l2g[p]] += engines[p].moments()
    ref = _moved(m, o, d, w).moments()
    assert np.allclose(got, ref, rtol=0.0, atol=1e-12), np.abs(got - ref).max()


# -------------------------------------------------- 6. threaded CPU path

_THREADED = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.environ["PT_ROOT"])
import pumiumtally_amd as pt

n, G, S = 70_000, 2, 2
mesh = pt.build_box(6, 6, 6, 1.0, 1.0, 1.0)
rng = np.random.default_rng(3)
pos = rng.uniform(0.05, 0.95, (n, 3))
dest = np.clip(pos + rng.normal(0, 0.2, (n, 3)), 0.01, 0.99)
w = rng.uniform(0.2, 1.0, n)
grp = rng.integers(0, G, n).astype(np.uint16)
rsp = rng.uniform(0.5, 2.0, (n, S))
eng = pt.TallyEngine(mesh, n, device="cpu", ngroups=G, nscores=S, linear=True)
eng.copy_initial_position(pos.ravel())
eng.move(pos.ravel(), dest.ravel(), np.ones(n, np.int8), w,
         groups=grp, responses=rsp)
raw = pt.TallyEngine(mesh, 1, device="cpu", ngroups=G, nscores=S, linear=True)
raw.walk_raw(pos.ravel(), dest.ravel(), mesh.locate(pos).astype(np.int32), w,
             groups=grp, responses=rsp)
np.savez(os.environ["PT_OUT"], moments=eng.moments(), flux=eng.flux(),
         raw_moments=raw.moments())
print("MOVE_OK")
"""


def _run_threaded(tmp_path, threads, tag):
    out = str(tmp_path / f"lin_{tag}.npz")
    env = dict(os.environ)
    env["PT_ROOT"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PT_OUT"] = out
    if threads is not None:
        env["PUMITALLY_CPU_THREADS"] = str(threads)
    r = subprocess.run([sys.executable, "-c", _THREADED], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (threads, r.stdout, r.stderr)
    assert "MOVE_OK" in r.stdout
    return np.load(out)


def test_threaded_cpu_moments_match_serial(tmp_path):
    """A batch large enough for the multithreaded CPU move (and walk_raw)
    with nscores > 1: per-thread partials must cover the moments' full
    shape.  In a subprocess, so an undersized partial kills the child."""
    mt = _run_threaded(tmp_path, None, "mt")  # hardware thread count
    st = _run_threaded(tmp_path, 1, "st")
    assert mt["moments"].shape == (2, 2, 6 * 6 * 6 * 6, 4)
    assert np.allclose(mt["moments"], st["moments"], rtol=0.0, atol=1e-12), \
        np.abs(mt["moments"] - st["moments"]).max()
    assert np.allclose(mt["flux"], st["flux"], rtol=0.0, atol=1e-12)
    # walk_raw threads on the hardware count alone (it ignores the override)
    assert np.allclose(mt["raw_moments"], st["moments"], rtol=0.0, atol=1e-12)
    assert st["moments"].sum() > 0


# ------------------------------------------------------ 7. behaviour and I/O

def test_end_batch_zeroes_and_moment_sum_accumulates():
    m = pt.build_box(2, 2, 2)
    o, d, w, _ = _segments(60, seed=41)
    eng = _moved(m, o, d, w)
    first = eng.moments().copy()
    assert first.sum() > 0
    assert not eng.moment_sum().any()
    eng.end_batch()
    assert not eng.moments().any()
    assert np.array_equal(eng.moment_sum(), first)
    eng.move(d.ravel(), o.ravel(), np.ones(60, np.int8), w)
    second = eng.moments().copy()
    eng.end_batch()
    assert np.allclose(eng.moment_sum(), first + second, rtol=1e-15, atol=0)
    # reconstruction from the batch-summed moments
    nodal = eng.nodal_flux(eng.moment_sum())
    assert nodal.shape == (m.nverts,)
    total = (nodal * _lumped_volumes(m)).sum()
    assert abs(total - (first + second).sum()) < 1e-12 * total


def test_checkpoint_round_trip_restores_moments(tmp_path):
    m = pt.build_box(2, 2, 2)
    o, d, w, _ = _segments(60, seed=42)
    eng = _moved(m, o, d, w)
    path = str(tmp_path / "lin.npz")
    eng.save_checkpoint(path)
    assert "moments" in np.load(path).files
    fresh = pt.TallyEngine(m, 60, device="cpu", linear=True)
    fresh.load_checkpoint(path)
    assert np.array_equal(fresh.moments(), eng.moments())
    assert np.array_equal(fresh.flux(), eng.flux())
    # non-linear checkpoints carry no moments key and load into either kind
    plain = _moved(m, o, d, w, linear=False)
    ppath = str(tmp_path / "plain.npz")
    plain.save_checkpoint(ppath)
    assert "moments" not in np.load(ppath).files
    fresh2 = pt.TallyEngine(m, 60, device="cpu", linear=True)
    fresh2.load_checkpoint(ppath)
    assert np.array_equal(fresh2.flux(), plain.flux())
    assert not fresh2.moments().any()


def _vtk_point_field(text, name, nverts):
    head, _, rest = text.partition(f"POINT_DATA {nverts}\n")
    assert rest, "no POINT_DATA section"
    assert "CELL_DATA" in head
    lines = rest.split("\n")
    assert lines[0] == f"SCALARS {name} double 1"
    assert lines[1] == "LOOKUP_TABLE default"
    return np.array([float(x) for x in lines[2:2 + nverts]])


@pytest.mark.parametrize("kw", [{}, {"ngroups": 2}, {"nscores": 2}])
def test_vtk_has_nodal_flux_point_field(tmp_path, kw):
    m = pt.build_box(2, 2, 2)
    n = 60
    o, d, w, rng = _segments(n, seed=43)
    run = dict(kw)
    if "ngroups" in kw:
        run["groups"] = rng.integers(0, 2, n).astype(np.uint16)
    if "nscores" in kw:
        run["responses"] = np.column_stack([np.ones(n), rng.uniform(1, 2, n)])
    eng = _moved(m, o, d, w, **run)
    out = tmp_path / "lin.vtk"
    eng.write_tally_results(str(out))
    got = _vtk_point_field(out.read_text(), "nodal_flux", m.nverts)
    # score 0 summed over groups == the plain single-tally nodal field
    ref = _moved(m, o, d, w).nodal_flux()
    assert np.allclose(got, ref, rtol=1e-12, atol=1e-14)


def test_vtu_has_nodal_flux_point_field(tmp_path):
    m = pt.build_box(2, 2, 2)
    o, d, w, _ = _segments(60, seed=44)
    eng = _moved(m, o, d, w)
    out = tmp_path / "lin.vtu"
    eng.write_tally_results(str(out))
    raw = out.read_bytes()
    head, _, app = raw.partition(b'<AppendedData encoding="raw">_')
    text = head.decode()
    assert "<PointData>" in text and 'Name="nodal_flux"' in text
    line = [ln for ln in text.split("\n") if 'Name="nodal_flux"' in ln][0]
    off = int(line.split('offset="')[1].split('"')[0])
    nbytes = int(np.frombuffer(app[off:off + 8], np.uint64)[0])
    assert nbytes == m.nverts * 8
    vals = np.frombuffer(app[off + 8:off + 8 + nbytes], np.float64)
    assert np.array_equal(vals, eng.nodal_flux())


def test_non_linear_files_have_no_point_data(tmp_path):
    m = pt.build_box(2, 2, 2)
    o, d, w, _ = _segments(60, seed=45)
    plain = _moved(m, o, d, w, linear=False)
    lin = _moved(m, o, d, w)
    for ext in ("vtk", "vtu"):
        a, b = tmp_path / f"plain.{ext}", tmp_path / f"lin.{ext}"
        plain.write_tally_results(str(a))
        lin.write_tally_results(str(b))
        pa, pb = a.read_bytes(), b.read_bytes()
        assert b"POINT_DATA" not in pa and b"PointData" not in pa
        assert b"nodal_flux" not in pa
        assert b"nodal_flux" in pb
    # the legacy file of a linear engine is the non-linear file plus the
    # trailing point section: everything before it is byte-identical
    pa = (tmp_path / "plain.vtk").read_bytes()
    pb = (tmp_path / "lin.vtk").read_bytes()
    assert pb.startswith(pa) and pb[len(pa):].startswith(b"POINT_DATA ")


def test_non_linear_engine_raises():
    m = pt.build_box(2, 2, 2)
    eng = pt.TallyEngine(m, 4, device="cpu")
    assert eng.linear is False
    for call in (eng.moments, eng.moment_sum, eng.nodal_flux,
                 eng.linear_coefficients):
        with pytest.raises(RuntimeError, match="linear"):
            call()
    for call in (eng._eng.moments, eng._eng.moment_sum,
                 lambda: eng._eng.set_moments(np.zeros(m.nelems * 4))):
        with pytest.raises(RuntimeError, match="linear"):
            call()


def test_linear_flag_leaves_flux_bit_identical():
    m = pt.build_box(3, 3, 3)
    n, S, G = 200, 2, 2
    o, d, w, rng = _segments(n, seed=46)
    d[::7] = o[::7] + 1.5
    grp = rng.integers(0, G, n).astype(np.uint16)
    resp = rng.uniform(0.0, 2.0, size=(n, S))
    for kw in ({}, dict(ngroups=G, nscores=S, groups=grp, responses=resp)):
        a = _moved(m, o, d, w, linear=False, **kw)
        b = _moved(m, o, d, w, linear=True, **kw)
        assert np.array_equal(a.flux(), b.flux())
        assert np.array_equal(a.positions(), b.positions())
        assert np.array_equal(a.elem_ids(), b.elem_ids())


# ------------------------------------------------------------------- GPU ---

def _gpu_bound(ref):
    return 1e-10 * max(1.0, np.abs(ref).max())


def _assert_gpu_matches(gpu, cpu):
    cm, gm = cpu.moments(), gpu.moments()
    cf, gf = np.asarray(cpu.flux()), np.asarray(gpu.flux())
    assert cm.sum() > 0
    em, ef = np.abs(cm - gm).max(), np.abs(cf - gf).max()
    print(f"max |moments diff| {em:.3e}  max |flux diff| {ef:.3e}")
    assert em < _gpu_bound(cm), em
    assert ef < _gpu_bound(cf), ef
    assert gpu.stats()["lost_particles"] == 0


@functools.lru_cache(maxsize=None)
def _gpu_case(n, grouped):
    """Inputs + CPU reference, computed once and shared (never mutated)."""
    m = pt.build_box(6, 6, 6)
    rng = np.random.default_rng(42 + n)
    o = rng.uniform(0.02, 0.98, size=(n, 3))
    d = rng.uniform(0.02, 0.98, size=(n, 3))
    d[::9] = o[::9] + rng.normal(0, 1.0, size=(len(d[::9]), 3))  # escapes
    w = rng.uniform(0.1, 1.0, n)
    kw = {}
    if grouped:
        kw = dict(ngroups=2, nscores=3,
                  groups=rng.integers(0, 2, n).astype(np.uint16),
                  responses=rng.uniform(0.0, 2.0, size=(n, 3)))
    return m, o, d, w, kw, _moved(m, o, d, w, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("grouped", [False, True],
                         ids=["aggregated", "grouped_scored"])
@pytest.mark.parametrize("n", [20000, 1000])
def test_gpu_move_matches_cpu(n, grouped):
    """Plain moves take the wave-aggregated linear kernel (aggregation is
    on by default); groups + responses take the plain-atomic one.  n=1000
    is no multiple of 64: partial waves."""
    m, o, d, w, kw, cpu = _gpu_case(n, grouped)
    gpu = _moved(m, o, d, w, device="cuda:0", **kw)
    assert gpu.is_gpu
    _assert_gpu_matches(gpu, cpu)
    _check_invariants(gpu)


@pytest.mark.gpu
def test_gpu_clustered_source_matches_cpu():
    """All particles start inside one cell of the box: neighbouring lanes
    share elements, so the aggregated kernel sees run lengths above 1."""
    m = pt.build_box(6, 6, 6)
    n = 20000
    rng = np.random.default_rng(5)
    o = (np.array([2.0, 3.0, 1.0]) + rng.uniform(0.05, 0.95, (n, 3))) / 6.0
    d = o + rng.normal(0, 0.15, size=(n, 3))
    w = rng.uniform(0.1, 1.0, n)
    cpu = _moved(m, o, d, w)
    gpu = _moved(m, o, d, w, device="cuda:0")
    _assert_gpu_matches(gpu, cpu)
    # second move from the committed state + a batch close on device
    for e in (cpu, gpu):
        e.move_continue(o.ravel(), np.ones(n, np.int8), w)
    _assert_gpu_matches(gpu, cpu)
    before = gpu.moments()
    gpu.end_batch()
    assert not gpu.moments().any()
    assert np.array_equal(gpu.moment_sum(), before)


@pytest.mark.gpu
def test_gpu_walk_raw_matches_cpu():
    m = pt.build_box(5, 5, 5)
    n, S = 4000, 2
    rng = np.random.default_rng(51)
    o = rng.uniform(0.02, 0.98, size=(n, 3))
    d = rng.uniform(0.02, 0.98, size=(n, 3))
    w = rng.uniform(0.1, 1.0, n)
    resp = rng.uniform(0.0, 2.0, size=(n, S))
    elem = m.locate(o).astype(np.int32)
    cpu = pt.TallyEngine(m, 1, device="cpu", nscores=S, linear=True)
    cpu.walk_raw(o.ravel(), d.ravel(), elem, w, responses=resp)
    gpu = pt.TallyEngine(m, 1, device="cuda:0", nscores=S, linear=True)
    gpu.walk_raw(o.ravel(), d.ravel(), elem, w, responses=resp)
    gpu.synchronize()
    _assert_gpu_matches(gpu, cpu)


@pytest.mark.gpu
def test_gpu_move_from_device_matches_move():
    import torch

    m, o, d, w, _, cpu = _gpu_case(1000, False)
    n = len(w)
    host = _moved(m, o, d, w, device="cuda:0")
    dev = torch.device("cuda:0")
    eng = pt.TallyEngine(m, n, device="cuda:0", linear=True)
    eng.copy_initial_position(o.ravel())
    eng.move_from_device(
        torch.from_numpy(d.ravel().copy()).to(dev),
        torch.ones(n, dtype=torch.int8, device=dev),
        torch.from_numpy(w.copy()).to(dev),
        origin=torch.from_numpy(o.ravel().copy()).to(dev))
    eng.synchronize()
    _assert_gpu_matches(eng, host)
    _assert_gpu_matches(eng, cpu)


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
    w = rng.uniform(0.1, 1.0, n)
    cpu = _moved(m, o, d, w)
    gpu = _moved(m, o, d, w, device="cuda:0")
    _assert_gpu_matches(gpu, cpu)


@pytest.mark.gpu
def test_gpu_non_linear_engine_raises_and_checkpoint(tmp_path):
    m, o, d, w, _, cpu = _gpu_case(1000, False)
    plain = pt.TallyEngine(m, 4, device="cuda:0")
    with pytest.raises(RuntimeError, match="linear"):
        plain.moments()
    gpu = _moved(m, o, d, w, device="cuda:0")
    path = str(tmp_path / "gpu_lin.npz")
    gpu.save_checkpoint(path)
    fresh = pt.TallyEngine(m, len(w), device="cuda:0", linear=True)
    fresh.load_checkpoint(path)
    assert np.array_equal(fresh.moments(), gpu.moments())
