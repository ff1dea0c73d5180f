"""Deleting a GPU engine gives all of its device memory back.

Both GPU engines own their buffers, streams and events through the RAII
types of csrc/hip/hip_util.h; nothing else frees them.  A buffer that an
engine forgot to own would leak once per create/use/delete cycle, so the
free device memory after cycle 6 is compared with that after cycle 2 (the
first cycle pays one-off runtime setup and is not counted).  Each cycle
touches every buffer the two engines have, lazy ones included.
"""
import functools
import gc

import numpy as np
import pytest

import pumiumtally_amd as pt

N = 1 << 18
CYCLES = 6
# The same six cycles on the commit before the RAII conversion (which did
# not leak on this path) measured a drop of MEASURED_PARENT_DROP bytes on an
# MI355X: 0, the free-memory reading was identical after every cycle (and is
# 0 with the RAII owners too).  The margin is four times its absolute value
# with a floor of 1 MiB, so 1 MiB.  One leaked 3*N-double buffer per cycle
# comes to 4 * 24 * N = 24 MiB over the four counted cycles, well above it.
MEASURED_PARENT_DROP = 0
MARGIN = max(4 * abs(MEASURED_PARENT_DROP), 1 << 20)


@functools.lru_cache(maxsize=None)
def _inputs():
    rng = np.random.default_rng(5)
    pts = [rng.uniform(0.05, 0.95, size=(N, 3)) for _ in range(5)]
    # second move: origins are the first move's destinations, a few changed
    o2 = pts[1].copy()
    o2[::1000] = pts[0][::1000]
    return dict(
        mesh=pt.build_box(4, 4, 4), p=pts, o2=o2,
        fly=np.ones(N, np.int8), w=rng.uniform(0.1, 1.0, N),
        grp=rng.integers(0, 2, N).astype(np.uint16),
        resp=rng.uniform(0.5, 2.0, size=(N, 2)))


def _free_bytes():
    return pt._core.device_mem_info(0)[0]


def _cycle():
    d = _inputs()
    p, fly, w, grp, resp = d["p"], d["fly"], d["w"], d["grp"], d["resp"]

    eng = pt.TallyEngine(d["mesh"], N, device="cuda:0", ngroups=2, nscores=2)
    eng.copy_initial_position(p[0].ravel())
    eng.move(p[0].ravel(), p[1].ravel(), fly.copy(), w)
    eng.move(d["o2"].ravel(), p[2].ravel(), fly.copy(), w)  # elided + patches
    assert eng.stats()["origins_elided"] > 0
    eng.move(p[2].ravel(), p[3].ravel(), fly.copy(), w, groups=grp,
             responses=resp)
    eng.move_continue(p[4].ravel(), fly.copy(), w)
    eng.end_batch()
    eng.walk_raw(eng.positions(), p[0].ravel(), eng.elem_ids(), w, groups=grp,
                 responses=resp, resume=True)
    eng.flux()
    del eng

    pe = pt._core.PartitionedEngine(d["mesh"], N, device="cuda:0", ngroups=2,
                                    nscores=2)
    pe.localize(p[0].ravel())
    pe.step(p[1].ravel(), fly, w, origin=p[0].ravel(), groups=grp,
            responses=resp)
    frame = np.asarray(pe.resident_list())
    assert len(frame) == N
    pe.step_local(p[2][frame].ravel(), fly[frame], w[frame],
                  origin=p[1][frame].ravel(), groups=grp[frame],
                  responses=resp[frame])
    pe.flux_global()
    del pe
    gc.collect()


def measure_drop(free_bytes=_free_bytes):
    """Free memory after cycle 2 minus free memory after cycle 6."""
    free = []
    for _ in range(CYCLES):
        _cycle()
        free.append(free_bytes())
    return free[1] - free[CYCLES - 1], free


@pytest.mark.gpu
def test_engines_return_device_memory():
    assert 4 * 24 * N > MARGIN
    drop, free = measure_drop()
    print(f"free bytes after each cycle: {free}; drop {drop}, margin {MARGIN}")
    assert drop <= MARGIN
