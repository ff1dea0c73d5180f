"""The HIP engine against the CPU engine at the launch shapes the benchmark
runs: several chunked launches per move, several trips of the slot loop per
thread (the later ones under a partial active mask), every slice count, the
plain-atomic arm, and holes in the flying mask.

At the particle counts the other GPU tests use, grid_blocks() gives every
particle its own thread and chunk_particles() issues one launch, so none of
that executes.  The knobs that select it are read once per process, so each
configuration below is one child process running tests/launch_battery.py on
the GPU with its own environment; the CPU reference is the same battery run
once, in this process.

Bounds: flux, moments and the batch sums differ by reassociation of fp64
adds only -- 1e-10 * max(1, |ref|.max()), the bound of the other GPU tests.
Everything else (currents and collisions of integer weights, counters,
walk_raw outputs, particle state) is bitwise equal.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_battery as lb  # noqa: E402

HELPER = os.path.abspath(lb.__file__)
CHILD_TIMEOUT = 120  # s; a child is one process start and ~15 tiny engines

# fp64 reassociation applies to these; every other record is exact
TOLERANCE_NAMES = ("flux", "flux_call1", "moments", "batch_sum",
                   "batch_sum_sq")

CONFIGS = {
    # baseline; 256 slices
    "default": {},
    # 5 launches, the last of 600 slots: lo/hi offsets under the XCD remap
    "chunked": {"PUMITALLY_CHUNK": "1100"},
    # 8 blocks x 625 slots: 3 trips, the last with 113 live lanes
    "strided": {"PUMITALLY_GRID_CAP": "8"},
    # 10 trips, the last with 49 live lanes
    "strided_b64": {"PUMITALLY_GRID_CAP": "8", "PUMITALLY_BLOCK": "64"},
    # 2 chunks x 2 trips: the benchmark's shape in small
    "bench_like": {"PUMITALLY_CHUNK": "2600", "PUMITALLY_GRID_CAP": "8"},
    # no privatisation, reduce skipped
    "slices1": {"PUMITALLY_FLUX_SLICES": "1"},
    # rounds down to 2
    "slices3": {"PUMITALLY_FLUX_SLICES": "3"},
    # 80 blocks over 16 slices: the mask wraps
    "slices_wrap": {"PUMITALLY_FLUX_SLICES": "16", "PUMITALLY_BLOCK": "64"},
    # plain-atomic arm for ungrouped moves and scores
    "noagg": {"PUMITALLY_WAVE_AGG": "0"},
    # 16 waves per block
    "block1024": {"PUMITALLY_BLOCK": "1024"},
    # device re-sort after every move
    "resort": {"PUMITALLY_SORT": "1"},
}
KNOBS = ("PUMITALLY_CHUNK", "PUMITALLY_GRID_CAP", "PUMITALLY_BLOCK",
         "PUMITALLY_FLUX_SLICES", "PUMITALLY_WAVE_AGG", "PUMITALLY_SORT")

# Set by the first child that is killed by its timeout or dies on a signal:
# the configurations after it fail without starting anything on the GPU.
_casualty = None


def _bound(ref):
    return 1e-10 * max(1.0, np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def _reference():
    ref = lb.run_battery("cpu")
    for a in ref.values():
        a.setflags(write=False)
    return ref


def _run_child(device, env_extra, out):
    """(return code or None on timeout, output) of one battery child."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(env_extra)
    try:
        r = subprocess.run(
            [sys.executable, HELPER, "--device", device, "--out", out],
            env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        return None, f"{e.stdout}\n{e.stderr}"
    return r.returncode, r.stdout + r.stderr


def _leaf(key):
    return key.split(".", 1)[1]


# ---- CPU side: the reference is anchored, the child protocol works --------

def _clipped_length(o, d):
    """Length of each segment o -> d inside [0, 1]^3 (slab clip)."""
    v = d - o
    t0 = np.zeros(len(o))
    t1 = np.ones(len(o))
    for ax in range(3):
        with np.errstate(divide="ignore", invalid="ignore"):
            ta = (0.0 - o[:, ax]) / v[:, ax]
            tb = (1.0 - o[:, ax]) / v[:, ax]
        par = v[:, ax] == 0.0
        lo = np.where(par, -np.inf, np.minimum(ta, tb))
        hi = np.where(par, np.inf, np.maximum(ta, tb))
        t0 = np.maximum(t0, lo)
        t1 = np.minimum(t1, hi)
    return np.maximum(t1 - t0, 0.0) * np.linalg.norm(v, axis=1)


def test_reference_is_anchored():
    x = lb.inputs()
    ref = _reference()
    first = ref["plain.flux_call1"]
    expected = (x["w"] * _clipped_length(x["o1"], x["d1"])).sum()
    rel = abs(first.sum() - expected) / expected
    print(f"call 1 conservation rel err {rel:.3e}")
    assert rel < 1e-12
    # without responses an nscores=2 engine books score 0 only
    null = ref["null_responses.flux"]
    assert null.shape == (2, lb.mesh().nelems)
    assert not null[1:].any()
    assert np.array_equal(null[0], first)


def test_every_reference_record_is_nonzero():
    ref = _reference()
    cases = {k.split(".", 1)[0] for k in ref}
    assert cases == {"plain", "linear", "currents", "currents_keyed",
                     "periodic_plain", "scored_mixed", "null_responses",
                     "point_source", "point_source_linear", "collisions",
                     "tracks", "walk_raw"}
    for key, a in ref.items():
        if _leaf(key) == "lost_particles":
            assert a == 0, key
        else:
            assert a.any(), key


def test_child_round_trips_on_cpu(tmp_path):
    """The child protocol on a machine without a GPU: a CPU child under a
    knob the CPU engine ignores writes exactly the in-process reference."""
    out = str(tmp_path / "cpu.npz")
    rc, text = _run_child("cpu", {"PUMITALLY_CHUNK": "1100"}, out)
    assert rc == 0 and "BATTERY_OK" in text, (rc, text)
    ref = _reference()
    with np.load(out) as got:
        assert set(got.files) == set(ref)
        for key, a in ref.items():
            g = got[key]
            assert g.dtype == a.dtype and g.shape == a.shape, key
            assert np.array_equal(g, a), key


# ---- GPU side: one child per configuration ------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("config", list(CONFIGS))
def test_launch_geometry_matches_cpu(tmp_path, config):
    global _casualty
    if _casualty is not None:
        pytest.fail(f"not started: the child of configuration {_casualty} "
                    "hung or died on a signal")
    ref = _reference()
    out = str(tmp_path / f"{config}.npz")
    rc, text = _run_child("cuda:0", CONFIGS[config], out)
    if rc is None or rc < 0 or rc in (134, 139):
        _casualty = f"{config!r} (return code {rc})"
        pytest.fail(f"child of {_casualty} hung or died:\n{text[-4000:]}")
    assert rc == 0 and "BATTERY_OK" in text, (rc, text[-4000:])

    failures = []
    worst = 0.0
    with np.load(out) as got:
        assert set(got.files) == set(ref)
        for key, a in ref.items():
            g = got[key]
            leaf = _leaf(key)
            assert g.dtype == a.dtype and g.shape == a.shape, key
            if leaf == "lost_particles":
                if a != 0 or g != 0:
                    failures.append(f"{key}: cpu {a}, gpu {g}")
                continue
            assert a.any(), key
            if leaf in TOLERANCE_NAMES:
                err = np.abs(g - a).max()
                rel = err / max(1.0, np.abs(a).max())
                worst = max(worst, rel)
                print(f"{config}: max |{key} diff| {err:.3e} "
                      f"(bound {_bound(a):.3e})")
                if not err < _bound(a):
                    failures.append(f"{key}: max diff {err:.3e}, "
                                    f"bound {_bound(a):.3e}")
            elif not np.array_equal(g, a):
                bad = np.flatnonzero(g.ravel() != a.ravel())
                failures.append(f"{key}: {bad.size} of {a.size} entries "
                                f"differ, first at {bad[:5].tolist()}")
    print(f"{config}: worst flux-like diff / max(1, |ref|.max()) "
          f"{worst:.3e} (bound 1e-10)")
    assert not failures, "\n".join(failures)
