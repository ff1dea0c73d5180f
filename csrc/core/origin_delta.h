// Host delta pass for origin elision (host-only, no HIP dependency).
//
// In steady state a particle's origin in move() is bit for bit the
// destination it was given in the previous move(), which is still in device
// memory.  The engine keeps a host shadow of the previous call's dest; this
// pass finds, for a particle range [lo, hi), the particles whose origin is
// NOT bit-identical to the shadow (the only origins that still have to cross
// the host-to-device link) and, in the same sweep, refreshes the shadow from
// the caller's dest for the next call.
//
// The comparison is on the 64-bit patterns, never floating-point ==, so
// -0.0 vs 0.0 counts as changed and a NaN with identical bits as unchanged:
// "unchanged" means the device copy is exactly what an upload would deliver.
//
// Changed particles go to a patch list in structure-of-arrays form (int32
// caller index + 3 doubles = 28 B per entry).  The range is cut into blocks;
// workers claim blocks from a shared counter (a thread on a slower core or
// farther from the memory simply takes fewer -- a fixed split would wait for
// it) and the worker that owns a block appends to that block's own disjoint
// segment of the list, so the list itself needs no atomics; compact() then
// closes the gaps between segments so it uploads as one copy per array.
#pragma once

#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace pumitally {

constexpr int kOriginDeltaMaxThreads = 16;

// Clamp a requested worker count to [1, kOriginDeltaMaxThreads].
int origin_delta_clamp_threads(int requested);

// Fixed pool of workers; run(f) executes f(t) for t in [0, nthreads) and
// returns when all are done.  The calling thread runs part 0 itself.
class OriginDeltaPool {
public:
  explicit OriginDeltaPool(int nthreads);
  ~OriginDeltaPool();
  OriginDeltaPool(const OriginDeltaPool &) = delete;
  OriginDeltaPool &operator=(const OriginDeltaPool &) = delete;

  int nthreads() const { return nthreads_; }
  void run(const std::function<void(int)> &f);

private:
  void worker(int t);

  int nthreads_;
  std::vector<std::thread> threads_;
  std::mutex mu_;
  std::condition_variable cv_start_, cv_done_;
  const std::function<void(int)> *job_ = nullptr;
  uint64_t generation_ = 0;
  int pending_ = 0;
  bool stop_ = false;
};

// Segment layout of one pass: block b covers particles
// [lo + b*block, min(hi, lo + (b+1)*block)) and owns patch entries
// [seg_off[b], seg_off[b] + seg_cap[b]).  A large block's segment holds only
// half of the block (+1): past that a patch entry (28 B) costs more than the
// origin it replaces (24 B) and the caller uploads the whole range instead,
// so the space is never needed.
struct OriginDeltaResult {
  int64_t block = 0; // particles per block (the last one may be shorter)
  int64_t nsegs = 0; // number of blocks == number of segments
  std::vector<int64_t> seg_off, seg_cap;
  std::vector<int64_t> seg_count; // changed particles in block b
  int64_t changed = 0;            // sum of seg_count
  bool overflow = false; // some block changed more than its segment holds:
                         // the patch list is incomplete, upload the range whole
};

// Block length the pass uses for `len` particles on `nthreads` workers.
int64_t origin_delta_block(int64_t len, int nthreads);

// Patch entries one pass over `len` particles on `nthreads` workers can need.
int64_t origin_delta_patch_capacity(int64_t len, int nthreads);

// One fused pass over particles [lo, hi):
//   changed(i) := bits(origin[3i..3i+2]) != bits(shadow[3i..3i+2])
//   shadow[3i..3i+2] = dest[3i..3i+2]
// origin/dest/shadow are indexed by absolute particle index; patch_idx /
// patch_xyz point at this pass's patch region (origin_delta_patch_capacity
// entries) and receive absolute particle indices, strictly increasing within
// each segment and from one segment to the next.  Counts stay exact on
// overflow; only the entries are dropped.
// nontemporal: write the shadow with streaming stores (no read-for-ownership;
// the shadow is far larger than any cache).  On the MI355X host ordinary
// stores measured slightly faster (profiles/README.md), hence the default.
OriginDeltaResult origin_delta_pass(OriginDeltaPool &pool,
                                    const double *origin, const double *dest,
                                    double *shadow, int64_t lo, int64_t hi,
                                    int32_t *patch_idx, double *patch_xyz,
                                    bool nontemporal = false);

// Close the gaps between segments: afterwards entries [0, r.changed) of the
// patch region are the whole list, indices strictly increasing.  Must not be
// called on an overflowed result.
void origin_delta_compact(const OriginDeltaResult &r, int32_t *patch_idx,
                          double *patch_xyz);

// shadow[3lo..3hi) = dest[3lo..3hi), split over the pool (seeds the shadow
// on a move that uploads every origin).
void origin_delta_seed(OriginDeltaPool &pool, const double *dest,
                       double *shadow, int64_t lo, int64_t hi,
                       bool nontemporal = false);

} // namespace pumitally
