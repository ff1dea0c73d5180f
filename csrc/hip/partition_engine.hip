// GPU stateful domain-decomposed tally engine (see partition_engine.h;
// the device-independent half and the factory are in
// csrc/core/partition_engine_common.cpp, the CPU twin in
// csrc/core/partition_engine_cpu.cpp).
//
// Per-global-particle state arrays in HBM, device-compacted walk lists,
// the replicated engine's fused walk kernel via walk_raw_device, and
// handoff records (csrc/core/partition_record.h) exchanged over
// Comm::alltoallv_device (RCCL grouped send/recv over xGMI) or, without
// device collectives, staged through the host.
//
// Replaces the reference's pumipic picparts + migrate-inside-search with
// persistent residency: a steady-state step uploads only the step inputs.
#include "../comm/comm.h"
#include "../core/partition_engine_common.h"
#include "hip_util.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>

namespace pumitally {

namespace {

constexpr int kPBlock = 256;
constexpr int kMaxChunks = 8; // step() copy/walk pipeline depth

// slots of the device counter array; [kCtrBuckets .. +2*world) are the
// per-destination counts and cursors of the pack pass, then kMaxChunks
// per-chunk walk counters
enum : int { kCtrWalk = 0, kCtrDep = 1, kCtrEject = 2, kCtrReloc = 3,
             kCtrFrame = 5, kCtrBuckets = 8 };

inline int pgrid(int64_t n) {
  int64_t b = (n + kPBlock - 1) / kPBlock;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (int)b;
}

// Streaming one-pass kernels (prepare/gather/collect/unpack) want one
// item per thread: the grid-stride cap that suits the walk launches
// leaves them latency-bound (~0.24 ms per 1.25M-item prepare measured
// at 2048 blocks).
inline int pgrid_flat(int64_t n) {
  int64_t b = (n + kPBlock - 1) / kPBlock;
  if (b > 65535) b = 65535;
  if (b < 1) b = 1;
  return (int)b;
}

// ---------------------------------------------------------------------------
// kernel argument views (passed by value)
// ---------------------------------------------------------------------------

// per-global-particle state, indexed by gid
struct ParticleState {
  double *__restrict__ pos; // committed position, n*3
  int32_t *__restrict__ elem; // LOCAL element, -1: outside the mesh
  uint8_t *res; // resident on this rank (read and cleared in one pass)
  uint8_t *__restrict__ esc;
};

// this rank's submesh and its lookup tables
struct DecompView {
  const Plane *__restrict__ planes;
  GridView grid;
  const int32_t *__restrict__ lowner; // local elem -> owner rank
  const int32_t *__restrict__ l2g;    // local elem -> global
  const int32_t *__restrict__ g2l;    // global elem -> local, -1: absent
  const int32_t *__restrict__ fgid;   // foreign slot -> global elem
  const int32_t *__restrict__ fowner; // foreign slot -> owner rank
  int myrank;
  double tol;
};

// a step's inputs as the caller gave them: indexed by gid in step(), by
// frame position in step_local().  orig/grp/resp may be null.
struct StepInputs {
  const int8_t *__restrict__ fly;
  const double *__restrict__ orig;
  const double *__restrict__ dest;
  const double *__restrict__ w;
  const uint16_t *__restrict__ grp;
  const double *__restrict__ resp;
};

// gid-indexed inputs of the walk lists that are gathered by gid.  Round 0
// of step() reads the uploaded global arrays (t0/prev null: fresh walks);
// later rounds read what k_part_unpack scattered from the arrivals'
// records, with dest pointing at the carried destinations.
struct GidInputs {
  double *__restrict__ dest;
  double *__restrict__ w;
  uint16_t *__restrict__ grp;
  double *__restrict__ resp;
  double *__restrict__ t0;
  int32_t *__restrict__ prev;
};

// walk scratch, indexed by walk-list slot.  grp/resp/t0/prev may be null.
struct WalkIn {
  double *__restrict__ pos;
  double *__restrict__ dest;
  int32_t *__restrict__ elem;
  double *__restrict__ w;
  uint16_t *__restrict__ grp;
  double *__restrict__ resp;
  double *__restrict__ t0;
  int32_t *__restrict__ prev;
};

struct WalkOut {
  const double *__restrict__ pos;
  const int32_t *__restrict__ elem;
  const int8_t *__restrict__ status;
  const double *__restrict__ dest;
  const double *__restrict__ o; // wrap-segment origin at a cut crossing
  const double *__restrict__ t;
  const int32_t *__restrict__ prev;
};

// where phase A and collect put what leaves this rank
struct DepartureOut {
  HandoffLayout rec;
  double *__restrict__ dep;              // departure entries
  int32_t *__restrict__ eject;           // input indices the host resolves
  unsigned long long *__restrict__ ctr;  // kCtr* slots
};

// Wave-aggregated append slot: one atomicAdd per 64-wide wavefront
// instead of one per lane (the single global counter was 1.9 ms/step of
// the prepare pass at 10M particles -- measured, profiles/README.md).
// Call from exactly the lanes that append; the ballot captures them.
__device__ __forceinline__ int64_t wave_append(unsigned long long *ctr) {
  const unsigned long long mask = __ballot(1);
  const int lane = (int)(threadIdx.x & 63u);
  const int leader = __ffsll((long long)mask) - 1;
  unsigned long long base = 0;
  if (lane == leader)
    base = atomicAdd(ctr, (unsigned long long)__popcll(mask));
  base = (unsigned long long)__shfl((long long)base, leader);
  return (int64_t)(base + __popcll(mask & ((1ull << lane) - 1ull)));
}

__device__ __forceinline__ Vec3 load3(const double *a, int64_t i) {
  return Vec3{a[i * 3], a[i * 3 + 1], a[i * 3 + 2]};
}

__device__ __forceinline__ void store3(double *a, int64_t i, Vec3 v) {
  a[i * 3] = v.x;
  a[i * 3 + 1] = v.y;
  a[i * 3 + 2] = v.z;
}

// particle g becomes resident here, unescaped, in local element le at q
__device__ __forceinline__ void place(const ParticleState &s, int64_t g,
                                      int32_t le, Vec3 q) {
  s.res[g] = 1;
  s.esc[g] = 0;
  s.elem[g] = le;
  store3(s.pos, g, q);
}

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------

__global__ void k_part_localize(DecompView d,
                                const double *__restrict__ origins, int64_t n,
                                ParticleState s,
                                unsigned long long *__restrict__ claim) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n; g += stride) {
    s.res[g] = 0;
    const Vec3 q = load3(origins, g);
    bool lo = false;
    const int32_t le = grid_locate(d.grid, d.planes, q, d.tol, &lo);
    // claim STRICT hits only: a loose (tol*1e4) hit on the SUBMESH can
    // steal a point whose true element is absent from this rank's ghost
    // ring (found at ~7e-7 depth by tools/part_world2_soak); such points
    // are resolved on the host against the FULL mesh -- the same
    // decision the replicated oracle makes -- so the starting element
    // (and hence the first tally sliver) matches bitwise.
    if (le >= 0 && !lo && d.lowner[le] == d.myrank) {
      place(s, g, le, q);
      atomicOr(&claim[g >> 6], 1ull << (g & 63));
    }
  }
}

__global__ void k_part_claim_rest(const unsigned long long *__restrict__ claim,
                                  const double *__restrict__ origins,
                                  int64_t n, ParticleState s) {
  // rank 0 claims globally-unfound particles (outside the mesh): they
  // stay resident with elem = -1 and tally nothing (replicated-engine
  // semantics for out-of-mesh particles)
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n; g += stride)
    if (!((claim[g >> 6] >> (g & 63)) & 1ull))
      place(s, g, -1, load3(origins, g));
}

// apply host-resolved full-mesh claims from localize(): particle gids[i]
// becomes resident here in local element lels[i] at its origin
__global__ void k_part_apply_claims(const int32_t *__restrict__ gids,
                                    const int32_t *__restrict__ lels,
                                    int64_t m,
                                    const double *__restrict__ origins,
                                    ParticleState s) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride)
    place(s, gids[i], lels[i], load3(origins, gids[i]));
}

// apply host-resolved ejects: gids[0 .. nleft) left this rank (their
// reroute records are already in the departure list); gids[nleft .. m)
// are outside the mesh and stay resident here with elem = -1, parked at
// their requested origin q[(i - nleft)*3 ..]
__global__ void k_part_apply_ejects(const int32_t *__restrict__ gids,
                                    int64_t nleft, int64_t m,
                                    const double *__restrict__ q,
                                    ParticleState s) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
    const int64_t g = gids[i];
    if (i < nleft) {
      s.res[g] = 0;
    } else {
      s.elem[g] = -1;
      store3(s.pos, g, load3(q, i - nleft));
    }
  }
}

// Phase A for one flying, resident, unescaped particle g whose inputs sit
// at index i: if its requested origin differs from the committed position
// it was resampled, and is relocated on the local submesh grid.
enum class PhaseA {
  Unchanged, // origin == committed position
  Relocated, // into an element this rank owns
  Rerouted,  // into a ghost element: departure entry written, res cleared
  Ejected    // not (strictly) in this submesh: the host resolves index i
};

__device__ __forceinline__ PhaseA phase_a(int64_t g, int64_t i,
                                          const ParticleState &s,
                                          const StepInputs &in,
                                          const DecompView &d,
                                          const DepartureOut &out) {
  const Vec3 q = load3(in.orig, i);
  const Vec3 p = load3(s.pos, g);
  if (q.x == p.x && q.y == p.y && q.z == p.z) return PhaseA::Unchanged;
  atomicAdd(&out.ctr[kCtrReloc], 1ull);
  bool lo = false;
  const int32_t le = grid_locate(d.grid, d.planes, q, d.tol, &lo);
  // loose submesh hits are NOT trusted (see k_part_localize): the host
  // resolves them on the full mesh, bitwise-matching the replicated
  // oracle's relocation
  if (le < 0 || lo) {
    out.eject[atomicAdd(&out.ctr[kCtrEject], 1ull)] = (int32_t)i;
    return PhaseA::Ejected;
  }
  if (d.lowner[le] == d.myrank) {
    s.elem[g] = le;
    store3(s.pos, g, q);
    return PhaseA::Relocated;
  }
  // fresh walk on the owner: t = 0, no exited-from element
  const unsigned long long k = atomicAdd(&out.ctr[kCtrDep], 1ull);
  out.rec.write(out.dep + k * out.rec.dep_width(), g, q, d.l2g[le],
                load3(in.dest, i), in.w[i], 0.0, -1,
                in.grp ? in.grp[i] : (uint16_t)0,
                in.resp ? in.resp + i * out.rec.nscores : nullptr,
                d.lowner[le]);
  s.res[g] = 0;
  return PhaseA::Rerouted;
}

// Round 0: phase A, then append every particle that walks to the list.
// kFrame == false (step): inputs are indexed by gid over [lo, hi); step()
//   pipelines chunks of the batch so chunk c's prepare+walk overlap chunk
//   c+1's H2D copies.  The chunk's walk list lives in list[lo ...] with its
//   own counter (nwalk_ctr), so segments never collide; k_part_gather fills
//   the walk scratch afterwards.
// kFrame == true (step_local): inputs are indexed by frame position over
//   [0, hi), state by the frame's gid; the gather into the walk scratch is
//   fused (there is no gid-indexed input array to gather from).
template <bool kFrame>
__global__ void k_part_prepare(int64_t lo, int64_t hi,
                               const int32_t *__restrict__ frame,
                               ParticleState s, StepInputs in, DecompView d,
                               DepartureOut out, int32_t *__restrict__ list,
                               WalkIn wk,
                               unsigned long long *__restrict__ nwalk_ctr) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = lo + blockIdx.x * blockDim.x + threadIdx.x; i < hi;
       i += stride) {
    const int64_t g = kFrame ? (int64_t)frame[i] : i;
    if (!s.res[g] || !in.fly[i]) continue;
    if (in.orig != nullptr && !s.esc[g] &&
        phase_a(g, i, s, in, d, out) >= PhaseA::Rerouted)
      continue;
    if (s.elem[g] < 0) continue; // outside mesh: nothing to walk
    const int64_t slot = lo + wave_append(nwalk_ctr);
    list[slot] = (int32_t)g;
    if constexpr (kFrame) {
      store3(wk.pos, slot, load3(s.pos, g));
      store3(wk.dest, slot, load3(in.dest, i));
      wk.elem[slot] = s.elem[g];
      wk.w[slot] = in.w[i];
      if (wk.grp) wk.grp[slot] = in.grp[i];
      if (wk.resp)
        for (int k = 0; k < out.rec.nscores; ++k)
          wk.resp[slot * out.rec.nscores + k] =
              in.resp[i * out.rec.nscores + k];
    }
  }
}

__global__ void k_part_gather(const int32_t *__restrict__ list, int64_t m,
                              ParticleState s, GidInputs in, int nscores,
                              WalkIn wk) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
    const int64_t g = list[j];
    store3(wk.pos, j, load3(s.pos, g));
    store3(wk.dest, j, load3(in.dest, g));
    wk.elem[j] = s.elem[g];
    wk.w[j] = in.w[g];
    if (wk.grp) wk.grp[j] = in.grp[g];
    if (wk.resp)
      for (int k = 0; k < nscores; ++k)
        wk.resp[j * nscores + k] = in.resp[g * nscores + k];
    if (wk.t0) wk.t0[j] = in.t0 ? in.t0[g] : 0.0;
    if (wk.prev) wk.prev[j] = in.prev ? in.prev[g] : -1;
  }
}

// after a walk: commit the particles that stopped here, write a departure
// entry (with the resume state) for those that crossed a cut
__global__ void k_part_collect(const int32_t *__restrict__ list, int64_t m,
                               WalkOut wo, WalkIn wk, DecompView d,
                               ParticleState s, DepartureOut out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
    const int64_t g = list[j];
    const int8_t st = wo.status[j];
    if (st == 2) {
      const int32_t k = -(wo.elem[j] + 2); // foreign slot entered
      const unsigned long long e = atomicAdd(&out.ctr[kCtrDep], 1ull);
      out.rec.write(out.dep + e * out.rec.dep_width(), g, load3(wo.o, j),
                    d.fgid[k], load3(wo.dest, j), wk.w[j], wo.t[j],
                    wo.prev[j] >= 0 ? d.l2g[wo.prev[j]] : -1,
                    wk.grp ? wk.grp[j] : (uint16_t)0,
                    wk.resp ? wk.resp + j * out.rec.nscores : nullptr,
                    d.fowner[k]);
      s.res[g] = 0;
    } else {
      store3(s.pos, g, load3(wo.pos, j));
      s.elem[g] = wo.elem[j];
      s.esc[g] = (st == 1) ? 1 : 0;
    }
  }
}

__global__ void k_part_count(const double *__restrict__ dep, int64_t m,
                             HandoffLayout rec,
                             unsigned long long *__restrict__ dcnt) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride)
    atomicAdd(&dcnt[rec.owner(dep + i * rec.dep_width())], 1ull);
}

// bucket the departure entries by owner; the owner column stays behind
__global__ void k_part_pack(const double *__restrict__ dep, int64_t m,
                            HandoffLayout rec,
                            const int64_t *__restrict__ offs,
                            unsigned long long *__restrict__ cur,
                            double *__restrict__ send) {
  const int rec_w = rec.width();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
    const double *e = dep + i * rec.dep_width();
    const int o = rec.owner(e);
    const int64_t s = offs[o] + (int64_t)atomicAdd(&cur[o], 1ull);
    for (int k = 0; k < rec_w; ++k) send[s * rec_w + k] = e[k];
  }
}

// arrivals become resident and form the next round's walk list; their
// carried step inputs are scattered by gid so the shared gather-by-gid
// path sees them regardless of which mode sent them
__global__ void k_part_unpack(const double *__restrict__ recv, int64_t m,
                              HandoffLayout rec, DecompView d,
                              ParticleState s, GidInputs in,
                              int32_t *__restrict__ list,
                              unsigned long long *__restrict__ ctr) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
    const double *e = recv + i * rec.width();
    const int64_t g = rec.gid(e);
    place(s, g, d.g2l[rec.target_gid(e)], rec.pos(e));
    store3(in.dest, g, rec.dest(e));
    in.w[g] = rec.weight(e);
    in.t0[g] = rec.t(e);
    const int64_t pg = rec.prev_gid(e);
    in.prev[g] = pg >= 0 ? d.g2l[pg] : -1; // -1: outside submesh (no rings)
    if (rec.carry_grp && in.grp) in.grp[g] = rec.group(e);
    if (in.resp)
      for (int k = 0; k < rec.nscores; ++k)
        in.resp[g * rec.nscores + k] = rec.responses(e)[k];
    list[wave_append(&ctr[kCtrWalk])] = (int32_t)g;
  }
}

// compact the resident mask into an ordered gid list (coupled-host
// frame); wave_append keeps rough gid order
__global__ void k_part_compact(const uint8_t *__restrict__ res, int64_t n,
                               int32_t *__restrict__ frame,
                               unsigned long long *__restrict__ ctr) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n; g += stride)
    if (res[g]) frame[wave_append(ctr)] = (int32_t)g;
}

// ---------------------------------------------------------------------------
// GPU implementation
// ---------------------------------------------------------------------------

class GpuPartitionedEngine final : public PartitionedEngineBase {
public:
  GpuPartitionedEngine(const PartitionedEngineArgs &a, int device)
      : PartitionedEngineBase(a), device_(device) {
    PT_HIP_CHECK(hipSetDevice(device_));
    eng_ = make_gpu_engine(dec_.sub.local, 1, device_, ngroups_, nscores_);
    if (!eng_) throw std::runtime_error("no HIP device for PartitionedEngine");
    if (!eng_->device_mesh(&dmesh_))
      throw std::runtime_error("GPU engine did not expose its device mesh");
    cs_ = (hipStream_t)dmesh_.stream; // the engine's compute stream
    s_copy_.create();
    for (auto &ev : ev_in_) ev.create();

    // lookup tables
    d_lowner_ = upload(dec_.lowner);
    d_l2g_ = upload(dec_.l2g32);
    d_g2l_ = upload(dec_.g2l);
    if (!dec_.sub.foreign_gid.empty()) {
      d_fgid_ = upload(std::vector<int32_t>(dec_.sub.foreign_gid.begin(),
                                            dec_.sub.foreign_gid.end()));
      d_fowner_ = upload(dec_.sub.foreign_owner);
    }

    // per-global-particle state
    d_pos_.allocate(n_ * 3);
    d_elem_.allocate(n_);
    d_res_.allocate(n_);
    d_esc_.allocate(n_);
    PT_HIP_CHECK(hipMemset(d_res_, 0, n_));
    PT_HIP_CHECK(hipMemset(d_esc_, 0, n_));

    // step inputs (global)
    d_dest_.allocate(n_ * 3);
    d_fly_.allocate(n_);
    d_w_.allocate(n_);

    // work buffers
    d_list_.allocate(n_);
    d_dep_.allocate(n_ * rec_.dep_width());
    d_dest_ovr_.allocate(n_ * 3);
    d_eject_.allocate(n_);
    ctr_chunk0_ = kCtrBuckets + 2 * world_;
    d_ctr_.allocate(ctr_chunk0_ + kMaxChunks);
    d_wpos_.allocate(n_ * 3);
    d_wdest_.allocate(n_ * 3);
    d_welem_.allocate(n_);
    d_ww_.allocate(n_);
    d_wout_pos_.allocate(n_ * 3);
    d_wout_dest_.allocate(n_ * 3);
    d_wout_elem_.allocate(n_);
    d_wstatus_.allocate(n_);
    d_offs_.allocate(world_);
    // bitwise handoff-resume state (partition_record.h)
    d_t0_.allocate(n_);
    d_prev_.allocate(n_);
    d_wt0_.allocate(n_);
    d_wprev_.allocate(n_);
    d_wout_o_.allocate(n_ * 3);
    d_wout_t_.allocate(n_);
    d_wout_prev_.allocate(n_);
  }

  ~GpuPartitionedEngine() override {
    (void)hipSetDevice(device_);
    (void)hipDeviceSynchronize();
    // members release themselves: buffers, then events and s_copy_, then
    // (in the base) the inner engine that lends cs_
  }

  void localize(const double *origins, int64_t n) override {
    check_n(n);
    PT_HIP_CHECK(hipSetDevice(device_));
    eng_->synchronize();
    PT_HIP_CHECK(
        hipMemcpy(d_dest_, origins, n_ * 3 * 8, hipMemcpyHostToDevice));
    const int64_t nwords = (n_ + 63) / 64;
    DeviceBuffer<unsigned long long> d_claim(nwords);
    PT_HIP_CHECK(hipMemset(d_claim, 0, nwords * 8));
    k_part_localize<<<pgrid_flat(n_), kPBlock>>>(decomp(), d_dest_, n_,
                                                 state(), d_claim);
    PT_HIP_CHECK(hipGetLastError());
    PT_HIP_CHECK(hipDeviceSynchronize());
    std::vector<int64_t> words(nwords);
    PT_HIP_CHECK(hipMemcpy(words.data(), d_claim, nwords * 8,
                           hipMemcpyDeviceToHost));
    std::vector<int32_t> cg, cl;
    resolve_unclaimed(origins, words, cg, cl);
    if (!cg.empty()) {
      const DeviceBuffer<int32_t> d_cg = upload(cg), d_cl = upload(cl);
      k_part_apply_claims<<<pgrid((int64_t)cg.size()), kPBlock>>>(
          d_cg, d_cl, (int64_t)cg.size(), d_dest_, state());
      PT_HIP_CHECK(hipGetLastError());
      PT_HIP_CHECK(hipDeviceSynchronize()); // before d_cg/d_cl go away
    }
    PT_HIP_CHECK(hipMemcpy(d_claim, words.data(), nwords * 8,
                           hipMemcpyHostToDevice));
    if (rank_ == 0) {
      k_part_claim_rest<<<pgrid_flat(n_), kPBlock>>>(d_claim, d_dest_, n_,
                                                     state());
      PT_HIP_CHECK(hipGetLastError());
    }
    PT_HIP_CHECK(hipDeviceSynchronize()); // d_claim is released on return
  }

  void step(const double *dest, const int8_t *flying, const double *weights,
            int64_t n, const double *origin, const uint16_t *groups,
            const double *responses) override {
    check_n(n);
    PT_HIP_CHECK(hipSetDevice(device_));
    check_groups(groups, ngroups_);
    eng_->synchronize();
    ensure_optional(origin ? &d_orig_ : nullptr, groups, responses);

    // Chunked copy/walk pipeline: all chunks' H2D copies are enqueued up
    // front on the copy stream; chunk c's prepare/gather/walk on the
    // compute stream waits only for chunk c's event, so the walk of
    // chunk c overlaps the copies of chunks c+1..  (measured: the
    // monolithic step serialized ~5.9 ms of H2D against ~6.5 ms of
    // kernels).
    const int C = (int)std::min<int64_t>(
        kMaxChunks, std::max<int64_t>(1, n_ >> 20)); // >=1M particles/chunk
    PT_HIP_CHECK(hipMemsetAsync(d_ctr_, 0,
                                (ctr_chunk0_ + kMaxChunks) * 8, cs_));
    std::vector<int64_t> clo(C + 1);
    for (int c = 0; c <= C; ++c) clo[c] = n_ * c / C;
    for (int c = 0; c < C; ++c) {
      const int64_t lo = clo[c], hi = clo[c + 1];
      PT_HIP_CHECK(hipMemcpyAsync(d_fly_ + lo, flying + lo, hi - lo,
                                  hipMemcpyHostToDevice, s_copy_));
      PT_HIP_CHECK(hipMemcpyAsync(d_w_ + lo, weights + lo, (hi - lo) * 8,
                                  hipMemcpyHostToDevice, s_copy_));
      PT_HIP_CHECK(hipMemcpyAsync(d_dest_ + lo * 3, dest + lo * 3,
                                  (hi - lo) * 24, hipMemcpyHostToDevice,
                                  s_copy_));
      if (origin)
        PT_HIP_CHECK(hipMemcpyAsync(d_orig_ + lo * 3, origin + lo * 3,
                                    (hi - lo) * 24, hipMemcpyHostToDevice,
                                    s_copy_));
      if (groups)
        PT_HIP_CHECK(hipMemcpyAsync(d_grp_ + lo, groups + lo, (hi - lo) * 2,
                                    hipMemcpyHostToDevice, s_copy_));
      if (responses)
        PT_HIP_CHECK(hipMemcpyAsync(d_resp_ + lo * nscores_,
                                    responses + lo * nscores_,
                                    (hi - lo) * nscores_ * 8,
                                    hipMemcpyHostToDevice, s_copy_));
      PT_HIP_CHECK(hipEventRecord(ev_in_[c], s_copy_));
    }

    const StepInputs in{d_fly_,
                        origin ? d_orig_.get() : nullptr,
                        d_dest_,
                        d_w_,
                        groups ? d_grp_.get() : nullptr,
                        responses ? d_resp_.get() : nullptr};
    for (int c = 0; c < C; ++c) {
      const int64_t lo = clo[c], hi = clo[c + 1];
      PT_HIP_CHECK(hipStreamWaitEvent(cs_, ev_in_[c], 0));
      k_part_prepare<false><<<pgrid_flat(hi - lo), kPBlock, 0, cs_>>>(
          lo, hi, nullptr, state(), in, decomp(), departures(), d_list_,
          WalkIn{}, &d_ctr_[ctr_chunk0_ + c]);
      PT_HIP_CHECK(hipGetLastError());
      PT_HIP_CHECK(hipStreamSynchronize(cs_));
      unsigned long long cw = 0;
      PT_HIP_CHECK(hipMemcpy(&cw, &d_ctr_[ctr_chunk0_ + c], 8,
                             hipMemcpyDeviceToHost));
      if (cw == 0) continue;
      walk_list(d_list_ + lo, (int64_t)cw, Feed::Uploaded, groups != nullptr,
                responses != nullptr);
    }
    PT_HIP_CHECK(hipStreamSynchronize(cs_));

    finish_round0(origin, dest, weights, groups, responses, nullptr);
    run_exchange_rounds(groups != nullptr, responses != nullptr);
    stats_.moves++;
  }

  std::vector<int64_t> resident_list() override {
    PT_HIP_CHECK(hipSetDevice(device_));
    eng_->synchronize();
    if (!d_frame_) d_frame_.allocate(n_);
    PT_HIP_CHECK(hipMemsetAsync(&d_ctr_[kCtrFrame], 0, 8, cs_));
    k_part_compact<<<pgrid_flat(n_), kPBlock, 0, cs_>>>(d_res_, n_, d_frame_,
                                                       &d_ctr_[kCtrFrame]);
    PT_HIP_CHECK(hipGetLastError());
    PT_HIP_CHECK(hipStreamSynchronize(cs_));
    unsigned long long nf = 0;
    PT_HIP_CHECK(
        hipMemcpy(&nf, &d_ctr_[kCtrFrame], 8, hipMemcpyDeviceToHost));
    n_frame_ = (int64_t)nf;
    std::vector<int32_t> f32(n_frame_);
    if (n_frame_)
      PT_HIP_CHECK(hipMemcpy(f32.data(), d_frame_, n_frame_ * 4,
                             hipMemcpyDeviceToHost));
    h_frame_.assign(f32.begin(), f32.end());
    return h_frame_;
  }

  void step_local(const double *dest, const int8_t *flying,
                  const double *weights, int64_t n_local,
                  const double *origin, const uint16_t *groups,
                  const double *responses) override {
    PT_HIP_CHECK(hipSetDevice(device_));
    check_step_local(n_local, n_frame_, groups);
    eng_->synchronize();
    if (!d_ldest_) {
      d_ldest_.allocate(n_ * 3);
      d_lw_.allocate(n_);
      d_lfly_.allocate(n_);
    }
    if (groups && !d_lgrp_) d_lgrp_.allocate(n_);
    if (responses && !d_lresp_) d_lresp_.allocate(n_ * nscores_);
    ensure_optional(origin ? &d_lorig_ : nullptr, groups, responses);
    if (n_local) {
      PT_HIP_CHECK(hipMemcpy(d_ldest_, dest, n_local * 24,
                             hipMemcpyHostToDevice));
      PT_HIP_CHECK(hipMemcpy(d_lfly_, flying, n_local,
                             hipMemcpyHostToDevice));
      PT_HIP_CHECK(hipMemcpy(d_lw_, weights, n_local * 8,
                             hipMemcpyHostToDevice));
      if (origin)
        PT_HIP_CHECK(hipMemcpy(d_lorig_, origin, n_local * 24,
                               hipMemcpyHostToDevice));
      if (groups)
        PT_HIP_CHECK(hipMemcpy(d_lgrp_, groups, n_local * 2,
                               hipMemcpyHostToDevice));
      if (responses)
        PT_HIP_CHECK(hipMemcpy(d_lresp_, responses,
                               n_local * nscores_ * 8,
                               hipMemcpyHostToDevice));
    }
    PT_HIP_CHECK(hipMemsetAsync(d_ctr_, 0,
                                (ctr_chunk0_ + kMaxChunks) * 8, cs_));
    if (n_local) {
      const StepInputs in{d_lfly_,
                          origin ? d_lorig_.get() : nullptr,
                          d_ldest_,
                          d_lw_,
                          groups ? d_lgrp_.get() : nullptr,
                          responses ? d_lresp_.get() : nullptr};
      k_part_prepare<true><<<pgrid_flat(n_local), kPBlock, 0, cs_>>>(
          0, n_local, d_frame_, state(), in, decomp(), departures(), d_list_,
          walk_in(groups != nullptr, responses != nullptr, false),
          &d_ctr_[ctr_chunk0_]);
      PT_HIP_CHECK(hipGetLastError());
    }
    PT_HIP_CHECK(hipStreamSynchronize(cs_));
    unsigned long long cw = 0;
    PT_HIP_CHECK(hipMemcpy(&cw, &d_ctr_[ctr_chunk0_], 8,
                           hipMemcpyDeviceToHost));
    finish_round0(origin, dest, weights, groups, responses, h_frame_.data());
    if (cw > 0) {
      walk_list(d_list_, (int64_t)cw, Feed::Fused, groups != nullptr,
                responses != nullptr);
      PT_HIP_CHECK(hipStreamSynchronize(cs_));
    }
    run_exchange_rounds(groups != nullptr, responses != nullptr);
    n_frame_ = -1; // residency changed; a new snapshot is required
    stats_.moves++;
  }

  int64_t resident() const override {
    int64_t c = 0;
    for (uint8_t v : resident_mask()) c += v;
    return c;
  }

  std::vector<uint8_t> resident_mask() const override {
    return download(d_res_, n_);
  }
  std::vector<double> positions() const override {
    return download(d_pos_, n_ * 3);
  }
  std::vector<int32_t> elem_ids() const override {
    return download(d_elem_, n_);
  }
  std::vector<uint8_t> escaped_mask() const override {
    return download(d_esc_, n_);
  }

  std::vector<int32_t> elem_ids_global() const override {
    const std::vector<int32_t> le = elem_ids();
    const std::vector<uint8_t> r = resident_mask();
    std::vector<int32_t> out(n_, -1);
    for (int64_t g = 0; g < n_; ++g)
      if (r[g] && le[g] >= 0) out[g] = dec_.l2g32[le[g]];
    return out;
  }

  void set_state(const double *pos, const int32_t *gelem,
                 const uint8_t *escaped, int64_t n) override {
    check_n(n);
    PT_HIP_CHECK(hipSetDevice(device_));
    eng_->synchronize();
    // host-side: once per restore/repartition, not a hot path
    std::vector<uint8_t> res;
    std::vector<int32_t> lel;
    claim_state(gelem, res, lel);
    PT_HIP_CHECK(hipMemcpy(d_pos_, pos, n_ * 24, hipMemcpyHostToDevice));
    PT_HIP_CHECK(
        hipMemcpy(d_elem_, lel.data(), n_ * 4, hipMemcpyHostToDevice));
    PT_HIP_CHECK(hipMemcpy(d_res_, res.data(), n_, hipMemcpyHostToDevice));
    PT_HIP_CHECK(
        hipMemcpy(d_esc_, escaped, n_, hipMemcpyHostToDevice));
    n_frame_ = -1;
  }

private:
  // where a walk list's inputs come from
  enum class Feed {
    Fused,    // already in the walk scratch (k_part_prepare<true>)
    Uploaded, // gathered by gid from the uploaded global arrays
    Arrivals  // gathered by gid from what the arrivals' records carried
  };

  ParticleState state() const { return {d_pos_, d_elem_, d_res_, d_esc_}; }
  DecompView decomp() const {
    return {dmesh_.planes, dmesh_.grid, d_lowner_, d_l2g_,  d_g2l_,
            d_fgid_,       d_fowner_,   rank_,     loc_tol_};
  }
  DepartureOut departures() const {
    return {rec_, d_dep_, d_eject_, d_ctr_};
  }
  WalkIn walk_in(bool groups, bool resp, bool resume) const {
    return {d_wpos_,
            d_wdest_,
            d_welem_,
            d_ww_,
            groups ? d_wgrp_.get() : nullptr,
            resp ? d_wresp_.get() : nullptr,
            resume ? d_wt0_.get() : nullptr,
            resume ? d_wprev_.get() : nullptr};
  }

  // orders the NULL-stream copy behind cs_ work
  template <class T>
  std::vector<T> download(const DeviceBuffer<T> &d, int64_t count) const {
    PT_HIP_CHECK(hipSetDevice(device_));
    eng_->synchronize();
    std::vector<T> h(count);
    PT_HIP_CHECK(
        hipMemcpy(h.data(), d, count * sizeof(T), hipMemcpyDeviceToHost));
    return h;
  }

  // First-use allocation of the optional step inputs, shared by step() and
  // step_local(): the origin buffer of the calling mode (null: no origins
  // passed), and the gid-indexed + walk-list copies of groups / responses.
  void ensure_optional(DeviceBuffer<double> *orig, bool groups,
                       bool responses) {
    if (orig && !*orig) orig->allocate(n_ * 3);
    if (responses && !d_resp_) {
      d_resp_.allocate(n_ * nscores_);
      d_wresp_.allocate(n_ * nscores_);
    }
    if (groups && !d_grp_) {
      d_grp_.allocate(n_);
      d_wgrp_.allocate(n_);
    }
  }

  // (gather ->) walk -> collect of one walk list on cs_; the caller syncs
  void walk_list(const int32_t *list, int64_t m, Feed feed, bool groups,
                 bool resp) {
    const bool resume = feed == Feed::Arrivals;
    const WalkIn wk = walk_in(groups, resp, resume);
    if (feed != Feed::Fused) {
      const GidInputs in{resume ? d_dest_ovr_ : d_dest_,
                         d_w_,
                         d_grp_,
                         d_resp_,
                         resume ? d_t0_.get() : nullptr,
                         resume ? d_prev_.get() : nullptr};
      k_part_gather<<<pgrid_flat(m), kPBlock, 0, cs_>>>(list, m, state(), in,
                                                       nscores_, wk);
      PT_HIP_CHECK(hipGetLastError());
    }
    eng_->walk_raw_device(m, d_wpos_, d_wdest_, d_welem_, d_ww_, d_wout_pos_,
                          d_wout_elem_, d_wstatus_, wk.grp, wk.resp,
                          d_wout_dest_, wk.t0, wk.prev, d_wout_o_, d_wout_t_,
                          d_wout_prev_);
    const WalkOut wo{d_wout_pos_, d_wout_elem_, d_wstatus_, d_wout_dest_,
                     d_wout_o_,   d_wout_t_,    d_wout_prev_};
    k_part_collect<<<pgrid_flat(m), kPBlock, 0, cs_>>>(
        list, m, wo, wk, decomp(), state(), departures());
    PT_HIP_CHECK(hipGetLastError());
  }

  // after round 0's phase A: relocation stats and the host-resolved ejects
  // (rare: resampled origins that missed the local submesh grid); their
  // reroute records join the departure list before the first exchange
  void finish_round0(const double *origin, const double *dest,
                     const double *weights, const uint16_t *groups,
                     const double *responses, const int64_t *frame) {
    unsigned long long hctr[4];
    PT_HIP_CHECK(hipMemcpy(hctr, d_ctr_, sizeof hctr, hipMemcpyDeviceToHost));
    if (hctr[kCtrEject] > 0)
      host_resolve_ejects((int64_t)hctr[kCtrEject], origin, dest, weights,
                          groups, responses, frame);
    stats_.relocated += (int64_t)hctr[kCtrReloc];
  }

  // Rare path: a resampled origin missed the local submesh grid.  Resolve
  // it on the full mesh (host): a hit becomes a reroute record in the
  // departure list (self-routes included -- they come back through the
  // exchange uniformly) and the particle leaves this rank; a miss is
  // outside the mesh and stays resident, parked at its origin.  The eject
  // list holds INPUT indices i; the particle is frame[i], or i itself when
  // frame is null (gid-indexed inputs).
  void host_resolve_ejects(int64_t ne, const double *origin,
                           const double *dest, const double *weights,
                           const uint16_t *groups, const double *responses,
                           const int64_t *frame) {
    std::vector<int32_t> idx(ne);
    PT_HIP_CHECK(
        hipMemcpy(idx.data(), d_eject_, ne * 4, hipMemcpyDeviceToHost));
    const int dw = rec_.dep_width();
    std::vector<double> depx, parked_q;
    std::vector<int32_t> left, parked;
    for (int64_t i : idx) {
      const int64_t g = frame ? frame[i] : i;
      const Vec3 q{origin[i * 3], origin[i * 3 + 1], origin[i * 3 + 2]};
      const int32_t ge = locate_full(q);
      if (ge >= 0) {
        depx.resize(depx.size() + dw, 0.0);
        rec_.write(&depx[depx.size() - dw], g, q, ge,
                   Vec3{dest[i * 3], dest[i * 3 + 1], dest[i * 3 + 2]},
                   weights[i], 0.0, -1, groups ? groups[i] : (uint16_t)0,
                   responses ? responses + i * nscores_ : nullptr,
                   dec_.owners[ge]);
        left.push_back((int32_t)g);
      } else {
        parked.push_back((int32_t)g);
        parked_q.insert(parked_q.end(), {q.x, q.y, q.z});
      }
    }
    if (!left.empty()) {
      // append to the device departure list (capacity n_*dep_width() is
      // plenty: ejects are a subset of residents)
      unsigned long long ndep = 0;
      PT_HIP_CHECK(
          hipMemcpy(&ndep, &d_ctr_[kCtrDep], 8, hipMemcpyDeviceToHost));
      PT_HIP_CHECK(hipMemcpy(d_dep_ + (int64_t)ndep * dw, depx.data(),
                             depx.size() * 8, hipMemcpyHostToDevice));
      ndep += (unsigned long long)left.size();
      PT_HIP_CHECK(
          hipMemcpy(&d_ctr_[kCtrDep], &ndep, 8, hipMemcpyHostToDevice));
    }
    const int64_t nleft = (int64_t)left.size();
    left.insert(left.end(), parked.begin(), parked.end());
    const DeviceBuffer<int32_t> d_gids = upload(left);
    const DeviceBuffer<double> d_q = upload(parked_q);
    k_part_apply_ejects<<<pgrid(ne), kPBlock>>>(d_gids, nleft, ne, d_q,
                                                state());
    PT_HIP_CHECK(hipGetLastError());
    PT_HIP_CHECK(hipDeviceSynchronize()); // before d_gids/d_q go away
  }

  // rounds 1+ of a step: walk lists come from exchanged records (round
  // 0's walks already ran); shared by step() and step_local().
  void run_exchange_rounds(bool groups_used, bool resp_used) {
    const int rec_w = rec_.width();
    int64_t nwalk_r = 0;
    for (int round = 1; round <= max_rounds(); ++round) {
      if (nwalk_r > 0) {
        walk_list(d_list_, nwalk_r, Feed::Arrivals, groups_used, resp_used);
        PT_HIP_CHECK(hipStreamSynchronize(cs_));
      }
      unsigned long long ndep = 0;
      PT_HIP_CHECK(
          hipMemcpy(&ndep, &d_ctr_[kCtrDep], 8, hipMemcpyDeviceToHost));
      const int64_t m = (int64_t)ndep;

      // per-destination counts -> offsets -> packed send buffer
      std::vector<int64_t> scounts(world_, 0), rcounts;
      if (m > 0) {
        unsigned long long *d_cnt = &d_ctr_[kCtrBuckets];
        PT_HIP_CHECK(hipMemsetAsync(d_cnt, 0, world_ * 8, cs_));
        k_part_count<<<pgrid_flat(m), kPBlock, 0, cs_>>>(d_dep_, m, rec_,
                                                       d_cnt);
        PT_HIP_CHECK(hipGetLastError());
        PT_HIP_CHECK(hipStreamSynchronize(cs_));
        std::vector<unsigned long long> dc(world_);
        PT_HIP_CHECK(hipMemcpy(dc.data(), d_cnt, world_ * 8,
                               hipMemcpyDeviceToHost));
        std::vector<int64_t> offs(world_);
        int64_t acc = 0;
        for (int r = 0; r < world_; ++r) {
          offs[r] = acc;
          scounts[r] = (int64_t)dc[r];
          acc += (int64_t)dc[r];
        }
        d_send_.reserve(m * rec_w);
        PT_HIP_CHECK(hipMemcpy(d_offs_, offs.data(), world_ * 8,
                               hipMemcpyHostToDevice));
        PT_HIP_CHECK(hipMemsetAsync(d_cnt + world_, 0, world_ * 8, cs_));
        k_part_pack<<<pgrid_flat(m), kPBlock, 0, cs_>>>(
            d_dep_, m, rec_, d_offs_, d_cnt + world_, d_send_);
        PT_HIP_CHECK(hipGetLastError());
        PT_HIP_CHECK(hipStreamSynchronize(cs_));
      }

      // global termination + recv counts
      if (!exchange_counts(scounts, rcounts)) break;
      int64_t nrecv = 0;
      for (int64_t c : rcounts) nrecv += c;
      const double *recv_ptr = nullptr;
      if (world_ == 1) {
        recv_ptr = d_send_; // self-exchange
      } else {
        // counts are in records; collectives speak doubles
        std::vector<int64_t> sc(world_), rc(world_);
        for (int r = 0; r < world_; ++r) {
          sc[r] = scounts[r] * rec_w;
          rc[r] = rcounts[r] * rec_w;
        }
        if (comm_->has_device_collectives()) {
          double *d_recv = nullptr;
          comm_->alltoallv_device(d_send_, sc, rc, &d_recv);
          recv_ptr = d_recv;
        } else {
          // host-staged exchange (TCP fallback): D2H -> alltoallv -> H2D
          std::vector<double> hsend(m * rec_w);
          if (m)
            PT_HIP_CHECK(hipMemcpy(hsend.data(), d_send_, m * rec_w * 8,
                                   hipMemcpyDeviceToHost));
          std::vector<double> hrecv = comm_->alltoallv(hsend.data(), sc);
          d_recv_.reserve((int64_t)hrecv.size());
          if (!hrecv.empty())
            PT_HIP_CHECK(hipMemcpy(d_recv_, hrecv.data(), hrecv.size() * 8,
                                   hipMemcpyHostToDevice));
          recv_ptr = d_recv_;
        }
      }

      // unpack received records; they form the next round's walk list
      PT_HIP_CHECK(hipMemsetAsync(d_ctr_, 0, 2 * 8, cs_)); // nwalk, ndep
      if (nrecv > 0) {
        const GidInputs carried{d_dest_ovr_, d_w_,  d_grp_,
                                d_resp_,     d_t0_, d_prev_};
        k_part_unpack<<<pgrid_flat(nrecv), kPBlock, 0, cs_>>>(
            recv_ptr, nrecv, rec_, decomp(), state(), carried, d_list_,
            d_ctr_);
        PT_HIP_CHECK(hipGetLastError());
      }
      PT_HIP_CHECK(hipStreamSynchronize(cs_));
      nwalk_r = nrecv;
      if (round == max_rounds()) throw_not_converged();
    }
  }

  int device_;
  Engine::DeviceMeshView dmesh_{};
  // the base's eng_ lends cs_, and s_copy_ / ev_in_ order work on the
  // buffers: all three outlive every buffer below.
  hipStream_t cs_ = nullptr; // the inner engine's compute stream
  Stream s_copy_;            // step-input H2D pipeline
  Event ev_in_[kMaxChunks];
  int ctr_chunk0_ = kCtrBuckets;
  DeviceBuffer<int32_t> d_frame_; // coupled-host frame (resident gids)
  int64_t n_frame_ = -1;          // -1: no snapshot taken
  std::vector<int64_t> h_frame_;  // host copy of the frame
  DeviceBuffer<double> d_ldest_, d_lw_, d_lorig_, d_lresp_;
  DeviceBuffer<int8_t> d_lfly_;
  DeviceBuffer<uint16_t> d_lgrp_;

  DeviceBuffer<int32_t> d_lowner_, d_l2g_, d_g2l_;
  DeviceBuffer<int32_t> d_fgid_, d_fowner_;
  DeviceBuffer<double> d_pos_;
  DeviceBuffer<int32_t> d_elem_;
  DeviceBuffer<uint8_t> d_res_, d_esc_;
  DeviceBuffer<double> d_dest_, d_w_, d_orig_;
  DeviceBuffer<double> d_resp_, d_wresp_;
  DeviceBuffer<int8_t> d_fly_;
  DeviceBuffer<uint16_t> d_grp_, d_wgrp_;
  DeviceBuffer<int32_t> d_list_, d_eject_;
  DeviceBuffer<double> d_dep_;
  DeviceBuffer<unsigned long long> d_ctr_;
  DeviceBuffer<double> d_wpos_, d_wdest_, d_ww_;
  DeviceBuffer<int32_t> d_welem_, d_wout_elem_;
  DeviceBuffer<double> d_wout_pos_, d_wout_dest_;
  DeviceBuffer<double> d_dest_ovr_;
  DeviceBuffer<int8_t> d_wstatus_;
  DeviceBuffer<int64_t> d_offs_;
  DeviceBuffer<double> d_send_, d_recv_; // grown with reserve()
  // bitwise handoff-resume state (partition_record.h)
  DeviceBuffer<double> d_t0_, d_wt0_;
  DeviceBuffer<int32_t> d_prev_, d_wprev_;
  DeviceBuffer<double> d_wout_o_, d_wout_t_;
  DeviceBuffer<int32_t> d_wout_prev_;
};

} // namespace

std::unique_ptr<PartitionedEngine>
make_gpu_partitioned_engine(const PartitionedEngineArgs &a, int ordinal) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= ordinal) {
    (void)hipGetLastError();
    return nullptr;
  }
  return std::make_unique<GpuPartitionedEngine>(a, ordinal);
}

} // namespace pumitally
