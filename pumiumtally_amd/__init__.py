"""pumiumtally_amd: MI355X-native unstructured-mesh track-length tally engine.

A from-scratch re-implementation of the capabilities of Fuad-HH/PumiUMTally
(PUMI-Tally) for AMD Instinct MI355X: track-length flux tallies on
unstructured tetrahedral meshes for Monte Carlo particle transport, with the
element walk as a hand-written CDNA4 HIP kernel, fp64 throughout, and
multi-GPU scaling over RCCL (see pumiumtally_amd.parallel).

Public surface:
    Mesh / build_box / read_mesh / read_gmsh / read_osh   mesh core
    TallyEngine                                            engine (CPU or GPU)
    PumiTally                                              4-call C++ API parity facade
    parallel.DistributedTally                              multi-GPU driver
"""
from __future__ import annotations

import os as _os

# ROCm runtime ordering: torch wheels bundle their own libamdhip64.so.7
# (same SONAME as /opt/rocm's).  Whichever loads FIRST owns the process;
# loading ours first and torch later leaves torch's HIP dead ("No HIP GPUs
# are available") and poisons subsequent HIP calls.  Importing torch first
# is safe in both orders of use, so do it here, before _core loads, unless
# explicitly disabled.  (Verified on MI355X: torch-first shares one runtime
# and both torch.cuda and our engine work.)
if _os.environ.get("PUMITALLY_NO_TORCH", "0") != "1":
    try:
        import torch as _torch  # noqa: F401
    except ImportError:
        pass


def _load_core():
    try:
        from . import _core  # type: ignore
        return _core
    except ImportError as e:
        if _os.environ.get("PUMITALLY_AUTOBUILD", "1") == "1":
            from ._build import build
            build()
            from . import _core  # type: ignore
            return _core
        raise ImportError(
            "pumiumtally_amd._core is not built. Run "
            "`python -m pumiumtally_amd._build` first."
        ) from e


_core = _load_core()

Mesh = _core.Mesh
PumiTally = _core.PumiTally
build_box = _core.build_box
read_mesh = _core.read_mesh
read_gmsh = _core.read_gmsh
read_osh = _core.read_osh
mesh_from_arrays = _core.mesh_from_arrays
have_gpu = _core.have_gpu
pinned_array = _core.pinned_array
normalize_flux = _core.normalize_flux
write_tally_vtk = _core.write_tally_vtk


def _device_ptr(t, dtype, numel, who):
    """Device address of t (0 for None) after checking that it exposes
    __cuda_array_interface__ with exactly `dtype` x `numel`, C-contiguous.
    `who` names the calling method in the error messages."""
    if t is None:
        return 0
    iface = getattr(t, "__cuda_array_interface__", None)
    if iface is None:
        raise TypeError(f"{who} expects CUDA tensors/arrays")
    import math
    n = math.prod(iface["shape"]) if iface["shape"] else 1
    if iface["typestr"] != dtype or n != numel:
        raise TypeError(
            f"expected {dtype} x{numel}, got {iface['typestr']} x{n}")
    strides = iface.get("strides")
    if strides is not None:
        # C-contiguity required (None == C-contiguous per protocol)
        itemsize = int(dtype[-1])
        expect = []
        acc = itemsize
        for s in reversed(iface["shape"]):
            expect.append(acc)
            acc *= s
        if list(strides) != list(reversed(expect)):
            raise TypeError(f"{who} requires contiguous tensors")
    return iface["data"][0]


def _sync_torch():
    """Order against torch's stream: tensors produced by torch ops
    (.to(device), fills) must be materialized before an engine kernel,
    which runs on the engine's own HIP stream."""
    import sys
    if "torch" in sys.modules:
        torch = sys.modules["torch"]
        if torch.cuda.is_available():
            torch.cuda.synchronize()


class TallyEngine:
    """Track-length tally engine over a tet mesh.

    device: "auto" (GPU if present, else CPU), "cpu", or "cuda[:N]".
    Semantics follow the reference PumiTally flow; see csrc/core/engine.h.

    linear=True additionally tallies, per (element, local vertex), the first
    barycentric moments of every track (moments()), from which nodal_flux()
    and linear_coefficients() give a P1 field; flux() is unchanged by it.
    Off by default; fixed at construction.

    currents=True additionally tallies, per (element, local face), the
    weight of every tallied crossing that leaves the element through that
    face (currents(): the outward partial current J+ integrated over the
    face), from which net_current() and leakage() follow; flux() is
    unchanged by it.  Off by default; fixed at construction
    (face_currents tells); not available together with linear=True.

    collisions=True adds a second, flux-shaped tally filled only by the
    explicit scoring calls score_collisions() / score_points() (and their
    *_from_device twins), never by move(): the collision estimator, scored
    at particle positions with no track and no geometry (collisions()).
    flux(), moments() and currents() are unchanged by it.  Off by default;
    fixed at construction (collision_tallies tells); combines with
    linear=True and with currents=True.
    """

    def __init__(self, mesh, num_particles: int, device: str = "auto",
                 ngroups: int = 1, nscores: int = 1, linear: bool = False,
                 currents: bool = False, collisions: bool = False):
        if linear and currents:
            raise ValueError(
                "currents=True cannot be combined with linear=True "
                "(not implemented)")
        self._eng = _core.Engine(mesh, num_particles, device, ngroups,
                                 nscores, bool(linear), bool(currents),
                                 bool(collisions))
        self.mesh = mesh
        self.ngroups = ngroups
        self.nscores = nscores
        self.linear = bool(linear)
        self.face_currents = bool(currents)
        self.collision_tallies = bool(collisions)

    @property
    def num_particles(self) -> int:
        return self._eng.num_particles

    @property
    def is_gpu(self) -> bool:
        return self._eng.is_gpu

    @property
    def max_steps(self) -> int:
        return self._eng.max_steps

    @max_steps.setter
    def max_steps(self, v: int) -> None:
        self._eng.max_steps = v

    # Origin elision (GPU engine): move() skips the upload of origins that
    # are bit-identical to the previous move's destinations.  Results do
    # not depend on any of the three; see docs/CONFIG.md.
    @property
    def origin_elide(self) -> bool:
        return self._eng.origin_elide

    @origin_elide.setter
    def origin_elide(self, v: bool) -> None:
        self._eng.origin_elide = bool(v)

    @property
    def origin_threads(self) -> int:
        return self._eng.origin_threads

    @origin_threads.setter
    def origin_threads(self, v: int) -> None:
        self._eng.origin_threads = int(v)

    @property
    def origin_chunk(self) -> int:
        return self._eng.origin_chunk

    @origin_chunk.setter
    def origin_chunk(self, v: int) -> None:
        self._eng.origin_chunk = int(v)

    def copy_initial_position(self, positions):
        self._eng.copy_initial_position(positions)

    def move(self, origin, dest, flying, weights, groups=None,
             responses=None):
        """One transport step.  groups (optional): per-particle energy-group
        indices (uint16, in [0, ngroups)); contributions land in
        flux()[group, elem].  responses (optional, n x nscores float64):
        per-particle score multipliers -- score k tallies
        seg*weight*responses[i,k] (flux + heating + ... from one walk).
        The reference has a single scalar tally; ngroups=nscores=1
        (default) matches it exactly."""
        self._eng.move(origin, dest, flying, weights, groups, responses)

    def move_continue(self, dest, flying, weights, groups=None,
                      responses=None):
        """move() without the phase-A origin upload: valid when no particle
        was resampled this step (origin == committed position)."""
        self._eng.move_continue(dest, flying, weights, groups, responses)

    def move_from_device(self, dest, flying, weights, origin=None,
                         sync_torch=True, groups=None, responses=None):
        """Device-resident move: dest/flying/weights (and optionally origin,
        groups, responses) are GPU tensors (torch CUDA tensors or anything
        with data_ptr() semantics via __cuda_array_interface__) already on
        this engine's device -- no host staging.  For GPU-side transport
        codes."""
        def ptr(t, dtype, numel):
            return _device_ptr(t, dtype, numel, "move_from_device")

        n = self.num_particles
        if sync_torch:
            _sync_torch()
        self._eng.move_device(
            ptr(origin, "<f8", n * 3), ptr(dest, "<f8", n * 3),
            ptr(flying, "|i1", n), ptr(weights, "<f8", n),
            ptr(groups, "<u2", n), ptr(responses, "<f8", n * self.nscores))

    def walk_raw(self, pos, dest, elem, weights, groups=None,
                 responses=None, in_t=None, in_prev=None, resume=False):
        """Batched raw segment walk (domain-decomposition support): returns
        (out_pos, out_elem, status, out_dest) with status 0=done 1=escaped
        2=handoff 3=lost; tallies into this engine's flux.  out_dest is the
        walk's final destination -- reflective/periodic restarts mutate it,
        and a handoff must resume toward out_dest, not the original dest.
        groups: optional uint16 per-segment energy-group indices (flux row
        group*nelems+elem); responses: optional n x nscores score
        multipliers.  With resume=True (or in_t/in_prev given) the tuple
        additionally carries (out_o, out_t, out_prev) -- the bitwise
        handoff-resume state (csrc/core/walk.h): ship them in the handoff
        record (pos column = out_o row) and seed the receiving walk via
        in_t/in_prev so it replays the sender's fp decisions exactly."""
        return self._eng.walk_raw(pos, dest, elem, weights, groups,
                                  responses, in_t, in_prev, resume)

    def tally_tracks(self, origins, dests, weights, groups=None,
                     responses=None):
        """Stateless track tallies: n free segments origins[i] -> dests[i]
        (n x 3 float64 each) with weights (n float64); n is independent of
        num_particles and n == 0 is a no-op.  A track may start or end
        anywhere: it is tallied wherever it runs inside the mesh, entering
        through vacuum boundary faces as often as it takes (a hole, a notch,
        a mesh that covers part of the geometry), and a track that never
        meets the mesh counts as a miss.  Contributions land where move()'s
        do -- flux(), and moments() / currents() on engines that have them
        -- with groups and responses applied as in move(); particle state
        and the collision tally are never touched.  stats() counts
        "tracks", "track_entries" (entries from outside through a boundary
        face; a start inside is none) and "track_misses".  Raises ValueError
        on a mesh with partition-cut faces."""
        import numpy as np
        self._eng.tally_tracks(
            self._exact(origins, np.float64, "origins").ravel(),
            self._exact(dests, np.float64, "dests").ravel(),
            self._exact(weights, np.float64, "weights").ravel(),
            groups, responses)

    def tally_tracks_from_device(self, origins, dests, weights, groups=None,
                                 responses=None, sync_torch=True):
        """tally_tracks() on GPU tensors already on this engine's device:
        origins, dests (n x 3 float64) and weights (n float64) set n.  The
        call is queued on the engine's stream; readbacks and synchronize()
        wait for it.  GPU engines only."""
        who = "tally_tracks_from_device"
        iface = getattr(weights, "__cuda_array_interface__", None)
        if iface is None:
            raise TypeError(f"{who} expects CUDA tensors/arrays")
        import math
        n = math.prod(iface["shape"]) if iface["shape"] else 1
        ptrs = (_device_ptr(origins, "<f8", n * 3, who),
                _device_ptr(dests, "<f8", n * 3, who),
                _device_ptr(weights, "<f8", n, who),
                _device_ptr(groups, "<u2", n, who),
                _device_ptr(responses, "<f8", n * self.nscores, who))
        if sync_torch:
            _sync_torch()
        self._eng.tally_tracks_device(n, *ptrs)

    def synchronize(self):
        self._eng.synchronize()

    def flux(self):
        """Raw tally.  Shape: (nelems,) for ngroups=nscores=1;
        (ngroups, nelems) for grouped single-score;
        (nscores, nelems) for scored single-group;
        (nscores, ngroups, nelems) for both."""
        f = self._eng.flux()
        if self.nscores > 1 and self.ngroups > 1:
            return f.reshape(self.nscores, self.ngroups, self.mesh.nelems)
        if self.nscores > 1:
            return f.reshape(self.nscores, self.mesh.nelems)
        if self.ngroups > 1:
            return f.reshape(self.ngroups, self.mesh.nelems)
        return f

    def set_flux(self, flux):
        self._eng.set_flux(flux)

    # ---- linear (per-vertex) moment tallies; linear=True engines only ----

    def _tally_shape(self):
        if self.nscores > 1 and self.ngroups > 1:
            return (self.nscores, self.ngroups, self.mesh.nelems)
        if self.nscores > 1:
            return (self.nscores, self.mesh.nelems)
        if self.ngroups > 1:
            return (self.ngroups, self.mesh.nelems)
        return (self.mesh.nelems,)

    def _require_linear(self, what):
        if not self.linear:
            raise RuntimeError(
                f"{what} needs linear moment tallies: create the engine "
                "with TallyEngine(..., linear=True)")

    def moments(self):
        """Raw first barycentric moments of the tallied tracks, shaped
        flux().shape + (4,): moments()[..., e, f] is the integral of
        weight * lambda_f along every chord inside element e, lambda_f the
        barycentric coordinate of the element's local vertex f
        (mesh.tet2vert[e, f]).  moments().sum(-1) equals flux() up to
        rounding.  Groups and scores apply exactly as for flux()."""
        self._require_linear("moments()")
        return self._eng.moments().reshape(self._tally_shape() + (4,))

    def moment_sum(self):
        """Moments accumulated over the closed batches (end_batch() adds
        the per-batch moments here and zeroes them); shaped like moments().
        Moments carry no sum of squares."""
        self._require_linear("moment_sum()")
        return self._eng.moment_sum().reshape(self._tally_shape() + (4,))

    def nodal_flux(self, moments=None):
        """Lumped-mass nodal (P1) flux, shaped flux().shape[:-1] + (nverts,):
        phi_v = sum_{e contains v} m[e, local(v)] / sum_{e contains v} vol_e/4.
        sum_v phi_v * (lumped volume of v) equals the total tallied track
        length.  moments: optional array shaped like moments() (e.g.
        moment_sum()) to reconstruct from instead of the current batch."""
        import numpy as np

        self._require_linear("nodal_flux()")
        m = self.moments() if moments is None else np.asarray(moments)
        nv = self.mesh.nverts
        t2v = np.asarray(self.mesh.tet2vert).reshape(-1)
        lumped = np.bincount(t2v, weights=np.repeat(
            np.asarray(self.mesh.volumes) / 4.0, 4), minlength=nv)
        flat = m.reshape(-1, t2v.size)
        out = np.stack([np.bincount(t2v, weights=row, minlength=nv)
                        for row in flat])
        out = np.divide(out, lumped, out=np.zeros_like(out),
                        where=lumped > 0)
        return out.reshape(m.shape[:-2] + (nv,))

    def linear_coefficients(self, moments=None):
        """Element-local P1 reconstruction, shaped like moments(): the
        vertex values c_f = (20/vol) * (m_f - sum_g m_g / 5) of the linear
        function whose moments are m (exact inverse of the tet mass matrix
        vol/20 * (I + J)).  Their mean over f equals normalized_flux()."""
        import numpy as np

        self._require_linear("linear_coefficients()")
        m = self.moments() if moments is None else np.asarray(moments)
        vol = np.asarray(self.mesh.volumes)[:, None]
        return (20.0 / vol) * (m - m.sum(axis=-1, keepdims=True) / 5.0)

    # ---- face-current tallies; currents=True engines only ----

    def _require_currents(self, what):
        if not self.face_currents:
            raise RuntimeError(
                f"{what} needs face-current tallies: create the engine "
                "with TallyEngine(..., currents=True)")

    def currents(self):
        """Outward partial currents of the current batch, shaped
        flux().shape + (4,): currents()[..., e, f] is the summed weight of
        the tallied tracks that left element e through its local face f
        (the face opposite local vertex f; flat face index e*4+f as in
        mesh.boundary_faces()).  No track length and no cosine enter; divide
        by mesh.face_areas for a current density.  Groups and scores apply
        exactly as for flux().  The final partial segment of a track counts
        nothing; a reflective face records the outward crossing only."""
        self._require_currents("currents()")
        return self._eng.currents().reshape(self._tally_shape() + (4,))

    def current_sum(self):
        """Currents accumulated over the closed batches (end_batch() adds
        the per-batch currents here and zeroes them); shaped like
        currents()."""
        self._require_currents("current_sum()")
        return self._eng.current_sum().reshape(self._tally_shape() + (4,))

    def current_sum_sq(self):
        """Sum over the closed batches of the squared per-batch currents;
        shaped like currents()."""
        self._require_currents("current_sum_sq()")
        return self._eng.current_sum_sq().reshape(self._tally_shape() + (4,))

    def _face_classes(self):
        """(twins (nelems*4,), reflective mask, vacuum mask) of the mesh's
        faces as this engine treats them."""
        import numpy as np

        twins = np.asarray(self.mesh.face_twins).reshape(-1)
        nbr = np.asarray(self.mesh.neighbors).reshape(-1)
        boundary = (nbr == -1) & (twins < 0)
        refl = np.zeros(nbr.size, dtype=bool)
        if self._eng.reflective:      # global BC, fixed at construction
            refl = boundary.copy()
        else:
            for fid in np.nonzero(boundary)[0]:
                refl[fid] = self.mesh.face_is_reflective(int(fid))
        return twins, refl, boundary & ~refl

    def net_current(self, currents=None):
        """Net outward current per (element, face), shaped like currents():
        J[e, f] - J[twin of (e, f)].  On vacuum and partition-cut faces it
        is J[e, f]; on reflective faces it is 0 (every crossing returns).
        currents: optional array shaped like currents() (e.g.
        current_sum()) to use instead of the current batch."""
        import numpy as np

        self._require_currents("net_current()")
        j = self.currents() if currents is None else np.asarray(currents)
        twins, refl, _ = self._face_classes()
        flat = j.reshape(-1, twins.size)
        has = twins >= 0
        net = flat.copy()
        net[:, has] -= flat[:, twins[has]]
        net[:, refl] = 0.0
        return net.reshape(j.shape)

    def leakage(self, currents=None):
        """Weight that left through the vacuum boundary: currents summed
        over the vacuum boundary faces, per score and group (shape
        flux().shape[:-1]; a scalar for ngroups=nscores=1)."""
        import numpy as np

        self._require_currents("leakage()")
        j = self.currents() if currents is None else np.asarray(currents)
        _, _, vac = self._face_classes()
        flat = j.reshape(-1, vac.size)
        out = flat[:, vac].sum(axis=1).reshape(j.shape[:-2])
        return float(out) if out.ndim == 0 else out

    def _element_leakage(self):
        """(nscores, ngroups, nelems): per element, the currents summed over
        its vacuum boundary faces."""
        import numpy as np

        _, _, vac = self._face_classes()
        j = self.currents().reshape(self.nscores, self.ngroups,
                                    self.mesh.nelems, 4)
        return (j * vac.reshape(self.mesh.nelems, 4)).sum(axis=-1)

    def _write_with_leakage(self, filename):
        # The flux fields exactly as write_tally_results names them, each
        # followed at the end by its leakage twin.
        S, G, ne = self.nscores, self.ngroups, self.mesh.nelems
        f = self.flux().reshape(S, G, ne)
        lk = self._element_leakage()
        flux_fields, leak_fields = [], []
        for k in range(S):
            name = "flux" if k == 0 else f"score{k}"
            lname = "leakage" if k == 0 else f"leakage_score{k}"
            flux_fields.append(
                (name, _core.normalize_flux(self.mesh, f[k].sum(axis=0))))
            leak_fields.append((lname, lk[k].sum(axis=0)))
            if G > 1:
                flux_fields += [(f"{name}_g{g}",
                                 _core.normalize_flux(self.mesh, f[k, g]))
                                for g in range(G)]
                leak_fields += [(f"{lname}_g{g}", lk[k, g]) for g in range(G)]
        if S == 1 and G == 1:
            flux_fields.append(("volume", self.mesh.volumes))
        self.mesh.write_vtk_fields(
            filename, flux_fields + leak_fields + self._collision_fields())

    # ---- collision-estimator tallies; collisions=True engines only ----

    def _require_collisions(self, what):
        if not self.collision_tallies:
            raise RuntimeError(
                f"{what}: collision tallies are off: create the engine "
                "with collisions=true (TallyEngine(..., collisions=True))")

    @staticmethod
    def _exact(a, dtype, what):
        # no silent conversion: a converted copy would hide a wrong dtype
        import numpy as np
        a = np.asarray(a)
        if a.dtype != dtype:
            raise TypeError(f"{what} must have dtype {np.dtype(dtype).name}, "
                            f"got {a.dtype.name}")
        return np.ascontiguousarray(a)

    def score_collisions(self, active, weights, groups=None, responses=None):
        """Collision estimator at the particles' committed positions: every
        particle i with active[i] != 0 (int8, num_particles) that sits in
        the mesh adds weights[i] (float64) -- times responses[i, k] per
        score when responses (n x nscores) are given, else to score 0 only
        -- to collisions()[..., e] at the element e the engine holds for
        it, in group groups[i] % ngroups (uint16; group 0 without).  An
        active particle that is unlocated or escaped adds nothing and
        counts into stats()["collision_misses"]; the others into
        stats()["collisions_scored"].  Nothing else changes: not active,
        not the particle state, not flux()."""
        self._require_collisions("score_collisions()")
        import numpy as np
        self._eng.score_collisions(
            self._exact(active, np.int8, "active").ravel(),
            self._exact(weights, np.float64, "weights").ravel(),
            groups, responses)

    def score_points(self, points, weights, groups=None, responses=None):
        """Collision estimator at n free points (n x 3 float64; n is
        independent of num_particles, n == 0 is a no-op): each point is
        localized like copy_initial_position() does and then scores like a
        particle in score_collisions(); a point outside the mesh is a
        miss."""
        self._require_collisions("score_points()")
        import numpy as np
        self._eng.score_points(
            self._exact(points, np.float64, "points").ravel(),
            self._exact(weights, np.float64, "weights").ravel(),
            groups, responses)

    def score_collisions_from_device(self, active, weights, groups=None,
                                     responses=None, sync_torch=True):
        """score_collisions() on GPU tensors already on this engine's device
        (same checking and torch ordering as move_from_device); nothing is
        staged.  GPU engines only."""
        self._require_collisions("score_collisions_from_device()")
        who = "score_collisions_from_device"
        n = self.num_particles
        ptrs = (_device_ptr(active, "|i1", n, who),
                _device_ptr(weights, "<f8", n, who),
                _device_ptr(groups, "<u2", n, who),
                _device_ptr(responses, "<f8", n * self.nscores, who))
        if sync_torch:
            _sync_torch()
        self._eng.score_collisions_device(*ptrs)

    def score_points_from_device(self, points, weights, groups=None,
                                 responses=None, sync_torch=True):
        """score_points() on GPU tensors already on this engine's device:
        points (n x 3 float64) and weights (n float64) set n.  The call is
        queued on the engine's stream; readbacks and synchronize() wait for
        it.  GPU engines only."""
        self._require_collisions("score_points_from_device()")
        who = "score_points_from_device"
        iface = getattr(weights, "__cuda_array_interface__", None)
        if iface is None:
            raise TypeError(f"{who} expects CUDA tensors/arrays")
        import math
        n = math.prod(iface["shape"]) if iface["shape"] else 1
        ptrs = (_device_ptr(points, "<f8", n * 3, who),
                _device_ptr(weights, "<f8", n, who),
                _device_ptr(groups, "<u2", n, who),
                _device_ptr(responses, "<f8", n * self.nscores, who))
        if sync_torch:
            _sync_torch()
        self._eng.score_points_device(n, *ptrs)

    def collisions(self):
        """Collision tally of the current batch, shaped like flux()."""
        self._require_collisions("collisions()")
        return self._eng.collisions().reshape(self._tally_shape())

    def collision_sum(self):
        """Collisions accumulated over the closed batches (end_batch() adds
        the per-batch collisions here and zeroes them); shaped like
        flux()."""
        self._require_collisions("collision_sum()")
        return self._eng.collision_sum().reshape(self._tally_shape())

    def collision_sum_sq(self):
        """Sum over the closed batches of the squared per-batch collisions;
        shaped like flux()."""
        self._require_collisions("collision_sum_sq()")
        return self._eng.collision_sum_sq().reshape(self._tally_shape())

    def collision_statistics(self):
        """batch_statistics() of the collision tally: (mean, rel_std_error)
        over the closed batches, shaped like flux()."""
        self._require_collisions("collision_statistics()")
        mean, rel = self._mean_rel(self._eng.collision_sum(),
                                   self._eng.collision_sum_sq())
        return (mean.reshape(self._tally_shape()),
                rel.reshape(self._tally_shape()))

    def _collision_fields(self):
        """Cell fields of write_tally_results for the collision tally: named
        like the flux fields with the stem "collisions", each divided by the
        element volume.  Empty without collision tallies."""
        if not self.collision_tallies:
            return []
        S, G, ne = self.nscores, self.ngroups, self.mesh.nelems
        c = self.collisions().reshape(S, G, ne)
        fields = []
        for k in range(S):
            name = "collisions" if k == 0 else f"collisions_score{k}"
            fields.append(
                (name, _core.normalize_flux(self.mesh, c[k].sum(axis=0))))
            if G > 1:
                fields += [(f"{name}_g{g}",
                            _core.normalize_flux(self.mesh, c[k, g]))
                           for g in range(G)]
        return fields

    def elem_ids(self):
        return self._eng.elem_ids()

    def positions(self):
        return self._eng.positions()

    def escaped(self):
        return self._eng.escaped()

    def stats(self):
        return self._eng.stats()

    def lost_records(self):
        """First-K records of walks dropped at max_steps: (k, 4) array of
        (particle index, drop x, drop y, drop z).  Pairs with
        stats()["lost_particles"] so a nonzero lost count on a real mesh is
        reproducible, not just counted (the reference only printfs)."""
        return self._eng.lost_records()

    def end_batch(self):
        """Close the current batch: accumulate the per-batch tally into
        running sum / sum-of-squares and zero it (standard MC batch
        statistics; the reference has no variance accounting)."""
        self._eng.end_batch()

    def _mean_rel(self, s1, s2):
        """(mean, rel_std_error) of a tally from its batch sum and sum of
        squares (flat arrays)."""
        import numpy as np

        nb = self._eng.num_batches
        if nb < 1:
            raise RuntimeError("no batches closed yet (call end_batch)")
        mean = s1 / nb
        var = np.maximum(s2 / nb - mean * mean, 0.0)
        sem = np.sqrt(var / max(nb - 1, 1))
        rel = np.divide(sem, np.abs(mean), out=np.zeros_like(sem),
                        where=mean != 0)
        return mean, rel

    def batch_statistics(self):
        """Returns (mean, rel_std_error) over the closed batches, shaped
        like flux().  rel_std_error = sigma_of_mean / |mean| (0 where
        mean == 0)."""
        mean, rel = self._mean_rel(self._eng.batch_sum(),
                                   self._eng.batch_sum_sq())
        if self.nscores > 1 and self.ngroups > 1:
            shape = (self.nscores, self.ngroups, self.mesh.nelems)
        elif self.nscores > 1:
            shape = (self.nscores, self.mesh.nelems)
        elif self.ngroups > 1:
            shape = (self.ngroups, self.mesh.nelems)
        else:
            return mean, rel
        return mean.reshape(shape), rel.reshape(shape)

    def save_checkpoint(self, path: str):
        """Persist the full tally state (flux accumulator + particle
        positions/elements/escaped flags) so a crashed batch can resume.
        The reference has no checkpointing (a crash loses the batch)."""
        import numpy as np

        self.synchronize()
        # linear engines add a "moments" key; everything else is unchanged
        extra = {"moments": self.moments()} if self.linear else {}
        # ... and face-current engines a "currents" key
        if self.face_currents:
            extra["currents"] = self.currents()
        # ... and collision-tally engines a "collisions" key
        if self.collision_tallies:
            extra["collisions"] = self.collisions()
        np.savez_compressed(
            path,
            flux=self.flux(),
            positions=self.positions(),
            elem_ids=self.elem_ids(),
            escaped=self.escaped(),
            num_particles=np.int64(self.num_particles),
            nelems=np.int64(self.mesh.nelems),
            **extra,
        )

    def load_checkpoint(self, path: str):
        import numpy as np

        d = np.load(path)
        if int(d["num_particles"]) != self.num_particles or \
           int(d["nelems"]) != self.mesh.nelems:
            raise ValueError("checkpoint does not match engine shape")
        self._eng.set_flux(d["flux"])
        if self.linear and "moments" in d.files:
            self._eng.set_moments(
                np.ascontiguousarray(d["moments"], dtype=np.float64).ravel())
        if self.face_currents and "currents" in d.files:
            self._eng.set_currents(
                np.ascontiguousarray(d["currents"], dtype=np.float64).ravel())
        if self.collision_tallies and "collisions" in d.files:
            self._eng.set_collisions(
                np.ascontiguousarray(d["collisions"],
                                     dtype=np.float64).ravel())
        self._eng.set_particle_state(
            np.ascontiguousarray(d["positions"], dtype=np.float64).ravel(),
            np.ascontiguousarray(d["elem_ids"], dtype=np.int32),
            np.ascontiguousarray(d["escaped"], dtype=np.uint8))

    def normalized_flux(self):
        """flux / element volume; shape matches flux() (per group/score
        when ngroups/nscores > 1)."""
        import numpy as np

        f = self.flux()
        if self.nscores > 1 or self.ngroups > 1:
            flat = np.asarray(f).reshape(-1, self.mesh.nelems)
            out = np.stack([_core.normalize_flux(self.mesh, row)
                            for row in flat])
            return out.reshape(np.asarray(f).shape)
        return _core.normalize_flux(self.mesh, f)

    def write_tally_results(self, filename: str = "fluxresult.vtk"):
        """Write the normalized tally (legacy .vtk, or .vtu by extension).
        Linear engines additionally write the point field "nodal_flux"
        (score 0 summed over groups, like the cell field "flux").
        Face-current engines additionally write one cell field "leakage"
        per flux field (same name suffixes: leakage, leakage_g0, score1 ->
        leakage_score1, ...): the element's currents summed over its vacuum
        boundary faces, not normalized.
        Collision-tally engines additionally write, after everything else,
        one cell field "collisions" per flux field (collisions,
        collisions_g0, collisions_score1, ...): collisions() divided by the
        element volume.  Engines without these options write exactly the
        reference's file."""
        if self.face_currents:
            self._write_with_leakage(filename)
            return
        coll = self._collision_fields()
        points = []
        if self.linear:
            m0 = self.moments().reshape(self.nscores, self.ngroups,
                                        self.mesh.nelems, 4)[0].sum(axis=0)
            points = [("nodal_flux", self.nodal_flux(m0))]
        if self.nscores > 1:
            # one field per score (score 0 keeps the name "flux"),
            # plus per-group fields when also grouped
            f = self.flux().reshape(self.nscores, self.ngroups,
                                    self.mesh.nelems)
            fields = []
            for k in range(self.nscores):
                name = "flux" if k == 0 else f"score{k}"
                fields.append(
                    (name, _core.normalize_flux(self.mesh, f[k].sum(axis=0))))
                if self.ngroups > 1:
                    fields += [(f"{name}_g{g}",
                                _core.normalize_flux(self.mesh, f[k, g]))
                               for g in range(self.ngroups)]
            self.mesh.write_vtk_fields(filename, fields + coll, points)
            return
        if self.ngroups > 1:
            # one normalized field per energy group + the total
            f = self.flux()
            fields = [("flux", _core.normalize_flux(self.mesh, f.sum(axis=0)))]
            fields += [(f"flux_g{g}", _core.normalize_flux(self.mesh, f[g]))
                       for g in range(self.ngroups)]
            self.mesh.write_vtk_fields(filename, fields + coll, points)
            return
        if points or coll:
            # same two cell fields write_tally_vtk writes
            self.mesh.write_vtk_fields(
                filename,
                [("flux", _core.normalize_flux(self.mesh, self._eng.flux())),
                 ("volume", self.mesh.volumes)] + coll, points)
            return
        _core.write_tally_vtk(filename, self.mesh, self._eng.flux())


__all__ = [
    "Mesh",
    "PumiTally",
    "TallyEngine",
    "build_box",
    "read_mesh",
    "read_gmsh",
    "read_osh",
    "mesh_from_arrays",
    "have_gpu",
    "pinned_array",
    "normalize_flux",
    "write_tally_vtk",
]
