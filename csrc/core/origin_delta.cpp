#include "origin_delta.h"

#include <algorithm>
#include <atomic>
#include <cstring>

#if defined(__SSE2__) && !defined(__HIP_DEVICE_COMPILE__)
#include <emmintrin.h>
#define PT_HAVE_STREAM_STORE 1
#else
#define PT_HAVE_STREAM_STORE 0
#endif

namespace pumitally {

int origin_delta_clamp_threads(int requested) {
  return std::max(1, std::min(requested, kOriginDeltaMaxThreads));
}

OriginDeltaPool::OriginDeltaPool(int nthreads)
    : nthreads_(origin_delta_clamp_threads(nthreads)) {
  for (int t = 1; t < nthreads_; ++t)
    threads_.emplace_back([this, t] { worker(t); });
}

OriginDeltaPool::~OriginDeltaPool() {
  {
    std::lock_guard<std::mutex> lk(mu_);
    stop_ = true;
  }
  cv_start_.notify_all();
  for (auto &th : threads_) th.join();
}

void OriginDeltaPool::worker(int t) {
  uint64_t seen = 0;
  for (;;) {
    const std::function<void(int)> *job;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_start_.wait(lk, [&] { return stop_ || generation_ != seen; });
      if (stop_) return;
      seen = generation_;
      job = job_;
    }
    (*job)(t);
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (--pending_ == 0) cv_done_.notify_one();
    }
  }
}

void OriginDeltaPool::run(const std::function<void(int)> &f) {
  if (nthreads_ > 1) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      job_ = &f;
      pending_ = nthreads_ - 1;
      ++generation_;
    }
    cv_start_.notify_all();
  }
  f(0);
  if (nthreads_ > 1) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_done_.wait(lk, [&] { return pending_ == 0; });
    job_ = nullptr;
  }
}

namespace {

constexpr int64_t kMaxBlock = 16384; // particles; 384 KiB per array
constexpr int64_t kHalfCapFrom = 1024; // blocks this long get half segments

inline int64_t seg_capacity(int64_t block_len) {
  return block_len >= kHalfCapFrom ? block_len / 2 + 1 : block_len;
}

inline uint64_t load_bits(const double *p) {
  uint64_t u;
  std::memcpy(&u, p, sizeof u);
  return u;
}

template <bool NT> inline void store_bits(double *p, uint64_t u) {
#if PT_HAVE_STREAM_STORE
  if (NT) {
    _mm_stream_si64(reinterpret_cast<long long *>(p), (long long)u);
    return;
  }
#endif
  std::memcpy(p, &u, sizeof u);
}

inline void store_fence() {
#if PT_HAVE_STREAM_STORE
  _mm_sfence(); // streaming stores are weakly ordered; publish before join
#endif
}

template <bool NT>
int64_t delta_part(const double *origin, const double *dest, double *shadow,
                   int64_t lo, int64_t hi, int32_t *pidx, double *pxyz,
                   int64_t cap) {
  int64_t count = 0;
  for (int64_t i = lo; i < hi; ++i) {
    const double *o = origin + i * 3;
    double *s = shadow + i * 3;
    const uint64_t diff = (load_bits(o) ^ load_bits(s)) |
                          (load_bits(o + 1) ^ load_bits(s + 1)) |
                          (load_bits(o + 2) ^ load_bits(s + 2));
    if (diff) {
      if (count < cap) {
        pidx[count] = (int32_t)i;
        pxyz[count * 3] = o[0];
        pxyz[count * 3 + 1] = o[1];
        pxyz[count * 3 + 2] = o[2];
      }
      ++count;
    }
    const double *d = dest + i * 3;
    store_bits<NT>(s, load_bits(d));
    store_bits<NT>(s + 1, load_bits(d + 1));
    store_bits<NT>(s + 2, load_bits(d + 2));
  }
  if (NT) store_fence();
  return count;
}

template <bool NT>
void copy_part(const double *dest, double *shadow, int64_t lo, int64_t hi) {
  for (int64_t k = lo * 3; k < hi * 3; ++k)
    store_bits<NT>(shadow + k, load_bits(dest + k));
  if (NT) store_fence();
}

} // namespace

int64_t origin_delta_block(int64_t len, int nthreads) {
  // at least ~4 blocks per worker so the shared counter can balance load
  const int64_t t = origin_delta_clamp_threads(nthreads);
  const int64_t b = (len + 4 * t - 1) / (4 * t);
  return std::max<int64_t>(1, std::min(b, kMaxBlock));
}

int64_t origin_delta_patch_capacity(int64_t len, int nthreads) {
  if (len <= 0) return 0;
  const int64_t block = origin_delta_block(len, nthreads);
  const int64_t full = len / block, tail = len % block;
  return full * seg_capacity(block) + (tail ? seg_capacity(tail) : 0);
}

OriginDeltaResult origin_delta_pass(OriginDeltaPool &pool,
                                    const double *origin, const double *dest,
                                    double *shadow, int64_t lo, int64_t hi,
                                    int32_t *patch_idx, double *patch_xyz,
                                    bool nontemporal) {
  OriginDeltaResult r;
  const int64_t len = hi - lo;
  if (len <= 0) return r;
  r.block = origin_delta_block(len, pool.nthreads());
  r.nsegs = (len + r.block - 1) / r.block;
  r.seg_off.resize(r.nsegs);
  r.seg_cap.resize(r.nsegs);
  r.seg_count.assign(r.nsegs, 0);
  for (int64_t b = 0; b < r.nsegs; ++b) {
    const int64_t blen = std::min(r.block, len - b * r.block);
    r.seg_off[b] = b * seg_capacity(r.block);
    r.seg_cap[b] = seg_capacity(blen);
  }
  std::atomic<int64_t> next{0};
  const std::function<void(int)> job = [&](int) {
    for (;;) {
      const int64_t b = next.fetch_add(1, std::memory_order_relaxed);
      if (b >= r.nsegs) return;
      const int64_t a = lo + b * r.block;
      const int64_t e = std::min(hi, a + r.block);
      int32_t *pi = patch_idx + r.seg_off[b];
      double *px = patch_xyz + r.seg_off[b] * 3;
      r.seg_count[b] =
          nontemporal
              ? delta_part<true>(origin, dest, shadow, a, e, pi, px,
                                 r.seg_cap[b])
              : delta_part<false>(origin, dest, shadow, a, e, pi, px,
                                  r.seg_cap[b]);
    }
  };
  pool.run(job);
  for (int64_t b = 0; b < r.nsegs; ++b) {
    r.changed += r.seg_count[b];
    if (r.seg_count[b] > r.seg_cap[b]) r.overflow = true;
  }
  return r;
}

void origin_delta_compact(const OriginDeltaResult &r, int32_t *patch_idx,
                          double *patch_xyz) {
  int64_t out = 0;
  for (int64_t b = 0; b < r.nsegs; ++b) {
    const int64_t cnt = r.seg_count[b];
    if (cnt && r.seg_off[b] != out) {
      std::memmove(patch_idx + out, patch_idx + r.seg_off[b],
                   cnt * sizeof(int32_t));
      std::memmove(patch_xyz + out * 3, patch_xyz + r.seg_off[b] * 3,
                   cnt * 3 * sizeof(double));
    }
    out += cnt;
  }
}

void origin_delta_seed(OriginDeltaPool &pool, const double *dest,
                       double *shadow, int64_t lo, int64_t hi,
                       bool nontemporal) {
  const int64_t len = hi - lo;
  if (len <= 0) return;
  const int64_t block = origin_delta_block(len, pool.nthreads());
  const int64_t nblocks = (len + block - 1) / block;
  std::atomic<int64_t> next{0};
  const std::function<void(int)> job = [&](int) {
    for (;;) {
      const int64_t b = next.fetch_add(1, std::memory_order_relaxed);
      if (b >= nblocks) return;
      const int64_t a = lo + b * block;
      const int64_t e = std::min(hi, a + block);
      if (nontemporal)
        copy_part<true>(dest, shadow, a, e);
      else
        copy_part<false>(dest, shadow, a, e);
    }
  };
  pool.run(job);
}

} // namespace pumitally
