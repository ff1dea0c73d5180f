"""GPU against CPU over every k_move / k_walk_raw instantiation.

Both engines tally through one contribution sink (csrc/core/tally_sink.h);
the CPU engine is the oracle.  The k_move matrix is traversal {fp64, fp32} x
tally arm {plain -> wave-aggregated, groups -> plain atomics, groups +
responses -> scored} x mesh {box, periodic-x box} x mode {flux, linear,
currents}: 36 kernels.  k_walk_raw is traversal x mode, each with and without
responses.  One small shape: build_box(4, 4, 4), n = 1000 (no multiple of
64: partial waves), every 9th destination thrown outside the box, integer
weights and responses, so currents are exact whatever the order of the adds.

Bound for flux and moments: reassociation of fp64 adds only (every
per-contribution value is bit-identical on both engines), the bound the other
GPU tests use.
"""
import functools

import numpy as np
import pytest

import pumiumtally_amd as pt

N = 1000
CELLS = 4
MODES = ("flux", "linear", "currents")
ARMS = ("plain", "groups", "groups_responses")


def _bound(ref):
    return 1e-10 * max(1.0, np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def _mesh(periodic):
    m = pt.build_box(CELLS, CELLS, CELLS)
    if periodic:
        fid, cen, _ = m.boundary_faces()
        hi = fid[np.abs(cen[:, 0] - 1.0) < 1e-12]
        lo = fid[np.abs(cen[:, 0] - 0.0) < 1e-12]
        m.set_periodic_faces(hi, lo, np.array([-1.0, 0.0, 0.0]))
    return m


@functools.lru_cache(maxsize=None)
def _inputs():
    """Shared by every case; never mutated."""
    rng = np.random.default_rng(7)
    o = rng.uniform(0.02, 0.98, size=(N, 3))
    d = rng.uniform(0.02, 0.98, size=(N, 3))
    d[::9] = o[::9] + rng.normal(0, 1.0, size=(len(d[::9]), 3))
    w = rng.integers(1, 5, N).astype(np.float64)
    grp = rng.integers(0, 2, N).astype(np.uint16)
    resp = rng.integers(1, 4, size=(N, 2)).astype(np.float64)
    for a in (o, d, w, grp, resp):
        a.setflags(write=False)
    return o, d, w, grp, resp


def _arm_kwargs(arm):
    _, _, _, grp, resp = _inputs()
    if arm == "plain":
        return {}, {}
    if arm == "groups":
        return dict(ngroups=2), dict(groups=grp)
    return dict(ngroups=2, nscores=2), dict(groups=grp, responses=resp)


def _mode_kwargs(mode):
    return dict(linear=mode == "linear", currents=mode == "currents")


def _results(eng, mode):
    eng.synchronize()
    out = {"flux": np.asarray(eng.flux()).copy()}
    if mode == "linear":
        out["moments"] = np.asarray(eng.moments()).copy()
    if mode == "currents":
        out["currents"] = np.asarray(eng.currents()).copy()
    out["lost"] = eng.stats()["lost_particles"]
    return out


def _run_move(device, mode, arm, periodic):
    o, d, w, _, _ = _inputs()
    ekw, rkw = _arm_kwargs(arm)
    eng = pt.TallyEngine(_mesh(periodic), N, device=device,
                         **_mode_kwargs(mode), **ekw)
    eng.copy_initial_position(o.ravel())
    eng.move(o.ravel(), d.ravel(), np.ones(N, np.int8), w, **rkw)
    return _results(eng, mode)


def _run_walk_raw(device, mode, scored):
    o, d, w, grp, resp = _inputs()
    m = _mesh(False)
    ekw = dict(ngroups=2, nscores=2) if scored else dict(ngroups=2)
    rkw = dict(groups=grp, responses=resp) if scored else dict(groups=grp)
    eng = pt.TallyEngine(m, 1, device=device, **_mode_kwargs(mode), **ekw)
    eng.walk_raw(o.ravel(), d.ravel(), m.locate(o).astype(np.int32), w, **rkw)
    return _results(eng, mode)


# The CPU references, one per case.  The traversal is part of the key only:
# PUMITALLY_WALK is read when an engine is constructed, and the caller has
# set it by then.
@functools.lru_cache(maxsize=None)
def _cpu_move(traversal, mode, arm, periodic):
    return _run_move("cpu", mode, arm, periodic)


@functools.lru_cache(maxsize=None)
def _cpu_walk_raw(traversal, mode, scored):
    return _run_walk_raw("cpu", mode, scored)


def _assert_matches(gpu, cpu, mode):
    assert cpu["lost"] == 0 and gpu["lost"] == 0
    for key in ("flux", "moments"):
        if key in cpu:
            ref = cpu[key]
            assert ref.any()
            err = np.abs(gpu[key] - ref).max()
            print(f"max |{key} diff| {err:.3e} (bound {_bound(ref):.3e})")
            assert err < _bound(ref), (key, err)
    if mode == "currents":
        assert cpu["currents"].any()
        assert np.array_equal(gpu["currents"], cpu["currents"])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("periodic", [False, True], ids=["box", "periodic_x"])
@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("traversal", ["fp64", "fp32"])
def test_k_move_matches_cpu(monkeypatch, traversal, arm, periodic, mode):
    monkeypatch.setenv("PUMITALLY_WALK", traversal)
    cpu = _cpu_move(traversal, mode, arm, periodic)
    gpu = _run_move("cuda:0", mode, arm, periodic)
    _assert_matches(gpu, cpu, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scored", [False, True],
                         ids=["groups", "groups_responses"])
@pytest.mark.parametrize("traversal", ["fp64", "fp32"])
def test_k_walk_raw_matches_cpu(monkeypatch, traversal, scored, mode):
    monkeypatch.setenv("PUMITALLY_WALK", traversal)
    cpu = _cpu_walk_raw(traversal, mode, scored)
    gpu = _run_walk_raw("cuda:0", mode, scored)
    _assert_matches(gpu, cpu, mode)
