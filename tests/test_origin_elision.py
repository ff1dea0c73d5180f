"""Origin elision: move() skips the upload of every origin that is bit for
bit the destination of the previous move() and rebuilds it on device
(csrc/hip/engine_gpu.hip, stage_elided).  It must never change a result.

Three engines are fed identical call streams -- GPU with elision on, GPU
with elision off (the plain full upload) and the CPU oracle -- and after
every move positions / element ids / escaped flags must be bitwise equal
across all three, flux within the suite's 1e-10 convention (atomic order
differs).  The host chunk is 257 particles for n = 3001: 12 chunks, a
ragged last one, nothing a multiple of the 64-wide wavefront.  The stats
counters prove the feature engaged (or stood down) where it should.
"""
import numpy as np
import pytest

import pumiumtally_amd as pt

pytestmark = pytest.mark.gpu

N = 3001
CHUNK = 257


@pytest.fixture(scope="module")
def mesh():
    m = pt.build_box(6, 6, 6)
    assert m.nelems == 1296
    return m


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


class Trio:
    """elide-on GPU, elide-off GPU and CPU engines driven in lockstep.

    Every host move goes through per-engine buffers that are overwritten
    with garbage the moment move() returns and refilled before the next
    call (stream (h)): nothing may keep reading caller memory."""

    def __init__(self, mesh, n=N, ngroups=1, nscores=1):
        self.n = n
        self.on = pt.TallyEngine(mesh, n, device="cuda:0", ngroups=ngroups,
                                 nscores=nscores)
        self.off = pt.TallyEngine(mesh, n, device="cuda:0", ngroups=ngroups,
                                  nscores=nscores)
        self.cpu = pt.TallyEngine(mesh, n, device="cpu", ngroups=ngroups,
                                  nscores=nscores)
        self.on.origin_elide = True
        self.on.origin_chunk = CHUNK
        self.off.origin_elide = False
        self.off.origin_chunk = CHUNK
        assert self.on.origin_elide and not self.off.origin_elide
        self.engines = (self.on, self.off, self.cpu)
        self.obuf = [np.empty(n * 3) for _ in self.engines]
        self.dbuf = [np.empty(n * 3) for _ in self.engines]
        self.moves = 0

    def copy_initial_position(self, p):
        for e in self.engines:
            e.copy_initial_position(np.ascontiguousarray(p).ravel().copy())

    def move(self, origin, dest, flying=None, weights=None, groups=None,
             responses=None):
        """Host move on all three; origin=None means move_continue.
        Returns (delta origins_elided, delta origin_bytes_uploaded) of the
        elide-on engine."""
        n = self.n
        fl = np.ones(n, np.int8) if flying is None else flying
        w = np.ones(n) if weights is None else weights
        before = self.on.stats()
        for e, ob, db in zip(self.engines, self.obuf, self.dbuf):
            db[:] = np.asarray(dest).ravel()
            f = fl.copy()
            if origin is None:
                e.move_continue(db, f, w, groups=groups, responses=responses)
            else:
                ob[:] = np.asarray(origin).ravel()
                e.move(ob, db, f, w, groups=groups, responses=responses)
            # the caller scribbles over its buffers right after the call
            ob[:] = np.nan
            db[:] = -7.25e30
            f[:] = 3
        self.moves += 1
        self.check()
        after = self.on.stats()
        return (after["origins_elided"] - before["origins_elided"],
                after["origin_bytes_uploaded"]
                - before["origin_bytes_uploaded"])

    def move_from_device(self, origin, dest, weights=None):
        """Device-resident move on the two GPU engines; the CPU engine has
        no such entry and takes the same arrays through move()."""
        import torch

        n = self.n
        w = np.ones(n) if weights is None else weights
        dev = torch.device("cuda:0")
        t_d = torch.from_numpy(np.asarray(dest).ravel().copy()).to(dev)
        t_f = torch.ones(n, dtype=torch.int8, device=dev)
        t_w = torch.from_numpy(w.copy()).to(dev)
        t_o = None
        if origin is not None:
            t_o = torch.from_numpy(np.asarray(origin).ravel().copy()).to(dev)
        for e in (self.on, self.off):
            e.move_from_device(t_d, t_f, t_w, origin=t_o)
            e.synchronize()
        fl = np.ones(n, np.int8)
        if origin is None:
            self.cpu.move_continue(np.asarray(dest).ravel().copy(), fl, w)
        else:
            self.cpu.move(np.asarray(origin).ravel().copy(),
                          np.asarray(dest).ravel().copy(), fl, w)
        self.moves += 1
        self.check()

    def check(self):
        ref_pos = _bits(self.cpu.positions())
        ref_elem = self.cpu.elem_ids()
        ref_esc = self.cpu.escaped()
        ref_flux = np.asarray(self.cpu.flux())
        tol = 1e-10 * max(1.0, np.abs(ref_flux).max())
        for name, e in (("elide-on", self.on), ("elide-off", self.off)):
            where = f"{name} after move {self.moves}"
            assert np.array_equal(_bits(e.positions()), ref_pos), where
            assert np.array_equal(e.elem_ids(), ref_elem), where
            assert np.array_equal(e.escaped(), ref_esc), where
            err = np.abs(np.asarray(e.flux()) - ref_flux).max()
            assert err <= tol, f"{where}: flux err {err:.3e} > {tol:.3e}"
        for e in self.engines:
            assert e.stats()["lost_particles"] == 0
        assert self.cpu.stats()["origins_elided"] == 0
        assert self.off.stats()["origins_elided"] == 0


def _ends(rng, n=N):
    return (rng.uniform(0.05, 0.95, size=(n, 3)),
            rng.uniform(0.05, 0.95, size=(n, 3)))


def test_pingpong_nothing_changed(mesh):
    """(a) after the seeding first move nothing more is uploaded."""
    rng = np.random.default_rng(11)
    ends = _ends(rng)
    t = Trio(mesh)
    t.copy_initial_position(ends[0])
    el, up = t.move(ends[0], ends[1])
    assert (el, up) == (0, N * 24)  # no staged destination yet: full upload
    for k in range(1, 6):
        el, up = t.move(ends[k % 2], ends[(k + 1) % 2])
        assert (el, up) == (N, 0), k
    # the plain path uploaded every origin of every move
    assert t.off.stats()["origin_bytes_uploaded"] == 6 * N * 24


def test_single_changed_origin_first_and_last(mesh):
    """(b) exactly one changed origin: index 0, then index n-1."""
    rng = np.random.default_rng(12)
    ends = _ends(rng)
    t = Trio(mesh)
    t.copy_initial_position(ends[0])
    t.move(ends[0], ends[1])
    o = ends[1].copy()
    o[0] = (0.31, 0.42, 0.53)
    el, up = t.move(o, ends[0])
    assert el + up // 24 == N and up % 24 == 0
    assert (el, up) == (N - 1, 24)
    o = ends[0].copy()
    o[N - 1] = (0.61, 0.22, 0.13)
    el, up = t.move(o, ends[1])
    assert (el, up) == (N - 1, 24)
    # -0.0 is not 0.0: a sign-of-zero difference alone must be uploaded
    # (particle 5 sits both moves out, so the boundary value is never walked)
    fl = np.ones(N, np.int8)
    fl[5] = 0
    d0 = ends[0].copy()
    d0[5, 0] = 0.0
    t.move(ends[1], d0, flying=fl)
    o = d0.copy()
    o[5, 0] = -0.0
    el, up = t.move(o, ends[1], flying=fl)
    assert (el, up) == (N - 1, 24)


def test_random_resampling_with_escapes_and_resort(mesh):
    """(c) + (g): ~10 % resampled origins per move over 20 moves (a device
    re-sort happens at move 16), destinations partly outside the box so
    escaped particles come back with origin == previous dest."""
    rng = np.random.default_rng(13)
    p = rng.uniform(0.05, 0.95, size=(N, 3))
    t = Trio(mesh)
    t.copy_initial_position(p)
    prev = p
    total_el = 0
    for k in range(20):
        o = prev.copy()
        idx = np.flatnonzero(rng.random(N) < 0.10)
        o[idx] = rng.uniform(0.05, 0.95, size=(idx.size, 3))
        d = rng.uniform(-0.2, 1.2, size=(N, 3))
        w = rng.uniform(0.1, 1.0, N)
        el, up = t.move(o, d, weights=w)
        if k > 0:
            assert up % 24 == 0 and el + up // 24 == N, k
            # a chunk that changed by more than half may upload whole;
            # at 10 % none does, so exactly the resampled ones travel
            assert up == idx.size * 24, k
        total_el += el
        prev = d
    assert t.moves >= 18
    assert total_el > 15 * N
    assert t.cpu.escaped().any()


def test_not_flying_then_origin_is_unused_dest(mesh):
    """(d) particles sit out a move (flying = 0); their next origin is the
    destination they never went to, which is not where they are."""
    rng = np.random.default_rng(14)
    ends = _ends(rng)
    third = rng.uniform(0.05, 0.95, size=(N, 3))
    t = Trio(mesh)
    t.copy_initial_position(ends[0])
    t.move(ends[0], ends[1])
    fl = np.ones(N, np.int8)
    fl[rng.random(N) < 0.3] = 0
    el, up = t.move(ends[1], third, flying=fl)
    assert (el, up) == (N, 0)
    el, up = t.move(third, ends[0])
    assert (el, up) == (N, 0)
    el, up = t.move(ends[0], ends[1])
    assert (el, up) == (N, 0)


def test_everything_changed_falls_back_then_backs_off(mesh):
    """(e) every origin fresh: whole-chunk uploads, then the host pass
    stands down for a while (plain uploads) and later probes again."""
    rng = np.random.default_rng(15)
    ends = _ends(rng)
    t = Trio(mesh)
    t.copy_initial_position(ends[0])
    t.move(ends[0], ends[1])
    fresh = rng.uniform(0.05, 0.95, size=(N, 3))
    el, up = t.move(fresh, ends[0])
    assert (el, up) == (0, N * 24)  # whole-chunk fallback
    # origins equal the previous destinations again, but the pass is in
    # back-off: plain uploads, nothing elided
    for k in range(3):
        el, up = t.move(ends[k % 2], ends[(k + 1) % 2])
        assert (el, up) == (0, N * 24), k
    # ... until it probes again and finds the workload elidable
    resumed = False
    for k in range(3, 40):
        el, up = t.move(ends[k % 2], ends[(k + 1) % 2])
        assert up % 24 == 0 and el + up // 24 == N, k
        if el == N:
            resumed = True
            break
    assert resumed


def test_interleaved_continue_device_and_initial_position(mesh):
    """(f) move_continue, move_from_device and copy_initial_position
    between move() calls."""
    rng = np.random.default_rng(16)
    ends = _ends(rng)
    third = rng.uniform(0.05, 0.95, size=(N, 3))
    t = Trio(mesh)
    t.copy_initial_position(ends[0])
    t.move(ends[0], ends[1])
    assert t.move(ends[1], ends[0]) == (N, 0)
    # continue-mode stages a dest the shadow never saw: next move() must
    # upload everything (and re-seed), the one after elides again
    assert t.move(None, ends[1]) == (0, 0)
    assert t.move(ends[1], ends[0]) == (0, N * 24)
    assert t.move(ends[0], ends[1]) == (N, 0)
    # device-resident moves stage nothing: the staged dest is still ends[1]
    t.move_from_device(None, third)
    t.move_from_device(ends[0], ends[1])
    assert t.move(ends[1], ends[0]) == (N, 0)
    # re-localization resets particle state, not the staged destinations
    t.copy_initial_position(third)
    assert t.move(ends[0], ends[1]) == (N, 0)
    t.copy_initial_position(ends[1])
    assert t.move(None, third) == (0, 0)
    assert t.move(third, ends[0]) == (0, N * 24)
    o = ends[0].copy()
    o[7::13] = rng.uniform(0.05, 0.95, size=(len(o[7::13]), 3))
    el, up = t.move(o, ends[1])
    assert (el, up) == (N - len(o[7::13]), 24 * len(o[7::13]))


def test_groups_and_scored_responses(mesh):
    """(i) ngroups = 2 with nscores = 2 responses ride the chunked path."""
    rng = np.random.default_rng(17)
    ends = _ends(rng)
    t = Trio(mesh, ngroups=2, nscores=2)
    t.copy_initial_position(ends[0])
    prev = ends[0]
    for k in range(5):
        o = prev.copy()
        idx = np.flatnonzero(rng.random(N) < 0.10)
        if k:
            o[idx] = rng.uniform(0.05, 0.95, size=(idx.size, 3))
        d = ends[(k + 1) % 2]
        g = rng.integers(0, 2, N).astype(np.uint16)
        r = rng.uniform(0.5, 2.0, size=(N, 2))
        w = rng.uniform(0.1, 1.0, N)
        el, up = t.move(o, d, weights=w, groups=g, responses=r)
        if k:
            assert (el, up) == (N - idx.size, idx.size * 24), k
        prev = d
    assert np.asarray(t.cpu.flux()).shape == (2, 2, mesh.nelems)


def test_thread_counts_give_the_same_patch(mesh):
    """The worker count is a per-engine setting (capped at 16) and must not
    show in results or counters, even with more workers than a chunk has
    particles to share out evenly."""
    rng = np.random.default_rng(18)
    ends = _ends(rng)
    for threads in (1, 3, 16, 99):
        t = Trio(mesh)
        t.on.origin_threads = threads
        t.copy_initial_position(ends[0])
        t.move(ends[0], ends[1])
        o = ends[1].copy()
        o[::7] = rng.uniform(0.05, 0.95, size=(len(o[::7]), 3))
        el, up = t.move(o, ends[0])
        assert (el, up) == (N - len(o[::7]), 24 * len(o[::7])), threads
