"""Multi-score tallies: several responses tallied from one walk.

The reference has exactly one score (track-length flux,
/root/reference/src/pumitally/PumiTallyImpl.cpp:352-380); nscores>1 is an
extension: score k of each crossing tallies seg * weight * responses[i, k]
into flux[k, group, elem].  The oracle for score k is therefore a plain
single-score engine run with weights[i] * responses[i, k].
"""
import numpy as np
import pytest

import pumiumtally_amd as pt


def _mk(n=200, seed=4):
    rng = np.random.default_rng(seed)
    o = rng.uniform(0.05, 0.95, size=(n, 3))
    d = rng.uniform(0.05, 0.95, size=(n, 3))
    w = rng.uniform(0.1, 1.0, n)
    return o, d, w, rng


def test_scored_move_matches_reweighted_oracle():
    m = pt.build_box(3, 3, 3)
    n, S = 200, 3
    o, d, w, rng = _mk(n)
    resp = rng.uniform(0.0, 2.0, size=(n, S))

    eng = pt.TallyEngine(m, n, device="cpu", nscores=S)
    assert eng.nscores == S
    eng.copy_initial_position(o.ravel())
    eng.move(o.ravel(), d.ravel(), np.ones(n, np.int8), w, responses=resp)
    got = eng.flux()
    assert got.shape == (S, m.nelems)

    for k in range(S):
        ref = pt.TallyEngine(m, n, device="cpu")
        ref.copy_initial_position(o.ravel())
        ref.move(o.ravel(), d.ravel(), np.ones(n, np.int8), w * resp[:, k])
        assert np.allclose(got[k], ref.flux(), rtol=1e-12, atol=1e-14)


def test_scored_null_responses_is_plain_flux():
    """nscores>1 with no responses: every crossing lands in score 0 only
    (documented contract: resp==null means multiplier 1 on the single
    unscored path)."""
    m = pt.build_box(2, 2, 2)
    n = 50
    o, d, w, _ = _mk(n, seed=7)
    eng = pt.TallyEngine(m, n, device="cpu", nscores=2)
    eng.copy_initial_position(o.ravel())
    eng.move(o.ravel(), d.ravel(), np.ones(n, np.int8), w)
    got = eng.flux()
    ref = pt.TallyEngine(m, n, device="cpu")
    ref.copy_initial_position(o.ravel())
    ref.move(o.ravel(), d.ravel(), np.ones(n, np.int8), w)
    assert np.allclose(got[0], ref.flux(), atol=1e-14)
    assert got[1].sum() == 0.0


def test_scored_and_grouped_combined():
    m = pt.build_box(3, 3, 3)
    n, S, G = 150, 2, 3
    o, d, w, rng = _mk(n, seed=9)
    resp = rng.uniform(0.5, 1.5, size=(n, S))
    grp = rng.integers(0, G, n).astype(np.uint16)

    eng = pt.TallyEngine(m, n, device="cpu", ngroups=G, nscores=S)
    eng.copy_initial_position(o.ravel())
    eng.move(o.ravel(), d.ravel(), np.ones(n, np.int8), w, groups=grp,
             responses=resp)
    got = eng.flux()
    assert got.shape == (S, G, m.nelems)

    for k in range(S):
        ref = pt.TallyEngine(m, n, device="cpu", ngroups=G)
        ref.copy_initial_position(o.ravel())
        ref.move(o.ravel(), d.ravel(), np.ones(n, np.int8), w * resp[:, k],
                 groups=grp)
        assert np.allclose(got[k], ref.flux(), rtol=1e-12, atol=1e-14)


def test_scored_accumulates_across_moves():
    m = pt.build_box(2, 2, 2)
    n, S = 60, 2
    o, d, w, rng = _mk(n, seed=12)
    resp = rng.uniform(0.0, 2.0, size=(n, S))
    eng = pt.TallyEngine(m, n, device="cpu", nscores=S)
    eng.copy_initial_position(o.ravel())
    eng.move(o.ravel(), d.ravel(), np.ones(n, np.int8), w, responses=resp)
    once = eng.flux().copy()
    # walk back with the same responses: tally doubles (same segment set)
    eng.move(d.ravel(), o.ravel(), np.ones(n, np.int8), w, responses=resp)
    assert np.allclose(eng.flux(), 2 * once, rtol=1e-12)


def test_scored_walk_raw():
    m = pt.build_box(3, 3, 3)
    n, S = 120, 3
    o, d, w, rng = _mk(n, seed=15)
    resp = rng.uniform(0.0, 2.0, size=(n, S))
    elem = m.locate(o).astype(np.int32)
    assert (elem >= 0).all()

    eng = pt.TallyEngine(m, 1, device="cpu", nscores=S)
    eng.walk_raw(o.ravel(), d.ravel(), elem, w, responses=resp)
    got = eng.flux()

    for k in range(S):
        ref = pt.TallyEngine(m, 1, device="cpu")
        ref.walk_raw(o.ravel(), d.ravel(), elem, w * resp[:, k])
        assert np.allclose(got[k], ref.flux(), rtol=1e-12, atol=1e-14)


def test_scored_vtk_fields(tmp_path):
    m = pt.build_box(2, 2, 2)
    n, S = 40, 2
    o, d, w, rng = _mk(n, seed=20)
    resp = rng.uniform(0.5, 1.5, size=(n, S))
    eng = pt.TallyEngine(m, n, device="cpu", nscores=S)
    eng.copy_initial_position(o.ravel())
    eng.move(o.ravel(), d.ravel(), np.ones(n, np.int8), w, responses=resp)
    out = tmp_path / "scored.vtk"
    eng.write_tally_results(str(out))
    text = out.read_text(errors="ignore")
    assert "flux" in text and "score1" in text


def test_scored_batch_stats():
    m = pt.build_box(2, 2, 2)
    n, S = 40, 2
    o, d, w, rng = _mk(n, seed=23)
    resp = rng.uniform(0.5, 1.5, size=(n, S))
    eng = pt.TallyEngine(m, n, device="cpu", nscores=S)
    eng.copy_initial_position(o.ravel())
    eng.move(o.ravel(), d.ravel(), np.ones(n, np.int8), w, responses=resp)
    f = eng.flux().copy()
    eng.end_batch()
    mean, rel = eng.batch_statistics()
    assert mean.shape == (S, m.nelems)
    assert np.allclose(mean, f, atol=1e-14)  # one batch: mean == tally
    assert eng.flux().sum() == 0.0


def test_scored_partitioned_single_rank():
    """PartitionedTally with responses == scored single-mesh oracle, with
    the responses riding the (9+nscores)-double handoff record."""
    from pumiumtally_amd.parallel.partition import PartitionedTally

    m = pt.build_box(3, 3, 3)
    n, S = 150, 2
    o, d, w, rng = _mk(n, seed=31)
    resp = rng.uniform(0.0, 2.0, size=(n, S))

    ptal = PartitionedTally(m, device="cpu", nscores=S)
    ptal.run_segments(o, d, w, responses=resp)
    got = ptal.flux_global()
    assert got.shape == (S, m.nelems)

    ref = pt.TallyEngine(m, n, device="cpu", nscores=S)
    ref.copy_initial_position(o.ravel())
    ref.move(o.ravel(), d.ravel(), np.ones(n, np.int8), w, responses=resp)
    assert np.allclose(got, ref.flux(), atol=1e-12)


@pytest.mark.gpu
def test_scored_move_gpu_matches_cpu():
    m = pt.build_box(6, 6, 6)
    n, S, G = 20000, 3, 2
    rng = np.random.default_rng(42)
    o = rng.uniform(0.02, 0.98, size=(n, 3))
    d = rng.uniform(0.02, 0.98, size=(n, 3))
    w = rng.uniform(0.1, 1.0, n)
    resp = rng.uniform(0.0, 2.0, size=(n, S))
    grp = rng.integers(0, G, n).astype(np.uint16)

    cpu = pt.TallyEngine(m, n, device="cpu", ngroups=G, nscores=S)
    cpu.copy_initial_position(o.ravel())
    cpu.move(o.ravel(), d.ravel(), np.ones(n, np.int8), w, groups=grp,
             responses=resp)

    gpu = pt.TallyEngine(m, n, device="cuda:0", ngroups=G, nscores=S)
    assert gpu.is_gpu
    gpu.copy_initial_position(o.ravel())
    gpu.move(o.ravel(), d.ravel(), np.ones(n, np.int8), w, groups=grp,
             responses=resp)
    gpu.synchronize()

    cf, gf = cpu.flux(), gpu.flux()
    assert np.abs(cf - gf).max() < 1e-10 * max(1.0, np.abs(cf).max())
    # conservation: total of score k == sum over particles of
    # seg_total * w * resp[:,k]; cross-check scores against each other via
    # the flux-weighted ratio on a per-element basis is overkill -- the
    # CPU equality above is the oracle.  Just pin non-triviality:
    assert cf.sum() > 0


@pytest.mark.gpu
def test_scored_null_responses_is_plain_flux_gpu():
    """GPU twin of test_scored_null_responses_is_plain_flux: a move without
    responses on an nscores=2 engine books score 0 only, whichever flux
    slice a block tallies into; a scored move on the same engine then lands
    in both scores.  n = 5000 runs more than one block, hence more than one
    slice.  Integer weights and responses."""
    m = pt.build_box(4, 4, 4)
    n, S = 5000, 2
    rng = np.random.default_rng(77)
    o = rng.uniform(0.02, 0.98, size=(n, 3))
    d = rng.uniform(0.02, 0.98, size=(n, 3))
    d2 = rng.uniform(0.02, 0.98, size=(n, 3))
    w = rng.integers(1, 5, n).astype(np.float64)
    resp = rng.integers(1, 4, size=(n, S)).astype(np.float64)
    fly = np.ones(n, np.int8)

    def bound(ref):
        return 1e-10 * max(1.0, np.abs(ref).max())

    engines = [pt.TallyEngine(m, n, device=dev, nscores=S)
               for dev in ("cpu", "cuda:0")]
    assert engines[1].is_gpu
    for eng in engines:
        eng.copy_initial_position(o.ravel())
        eng.move(o.ravel(), d.ravel(), fly, w)
        eng.synchronize()
    cf, gf = (np.asarray(e.flux()).copy() for e in engines)
    assert cf[0].any() and not cf[1].any()
    print(f"null responses: max |score 1| {np.abs(gf[1]).max():.3e}, "
          f"max |score 0 diff| {np.abs(gf[0] - cf[0]).max():.3e}")
    assert not gf[1].any(), np.abs(gf[1]).max()
    assert np.abs(gf[0] - cf[0]).max() < bound(cf[0])

    for eng in engines:
        eng.move(d.ravel(), d2.ravel(), fly, w, responses=resp)
        eng.synchronize()
    cf, gf = (np.asarray(e.flux()).copy() for e in engines)
    assert cf[1].any()
    err = np.abs(gf - cf).max()
    print(f"then scored: max |flux diff| {err:.3e} (bound {bound(cf):.3e})")
    assert err < bound(cf)


@pytest.mark.gpu
def test_scored_walk_raw_gpu():
    m = pt.build_box(5, 5, 5)
    n, S = 4000, 2
    rng = np.random.default_rng(51)
    o = rng.uniform(0.02, 0.98, size=(n, 3))
    d = rng.uniform(0.02, 0.98, size=(n, 3))
    w = rng.uniform(0.1, 1.0, n)
    resp = rng.uniform(0.0, 2.0, size=(n, S))
    elem = m.locate(o).astype(np.int32)

    cpu = pt.TallyEngine(m, 1, device="cpu", nscores=S)
    cpu.walk_raw(o.ravel(), d.ravel(), elem, w, responses=resp)

    gpu = pt.TallyEngine(m, 1, device="cuda:0", nscores=S)
    assert gpu.is_gpu
    gpu.walk_raw(o.ravel(), d.ravel(), elem, w, responses=resp)
    gpu.synchronize()
    assert np.abs(cpu.flux() - gpu.flux()).max() < 1e-10
