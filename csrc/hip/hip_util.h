// Internal RAII owners for the HIP resources of the GPU translation units:
// device and pinned allocations, streams and events.  Not installed.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace pumitally {

#define PT_HIP_CHECK(expr)                                                     \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess)                                                      \
      throw std::runtime_error(std::string("HIP error at " __FILE__ ":") +     \
                               std::to_string(__LINE__) + ": " +               \
                               hipGetErrorString(_e));                         \
  } while (0)

// Move-only owner of `size()` elements of T in device memory.  A count of 0
// holds nothing.  Converts to T* so kernel launch lines and null tests read
// as they do with raw pointers.
template <class T> class DeviceBuffer {
public:
  DeviceBuffer() = default;
  explicit DeviceBuffer(int64_t count) { allocate(count); }
  DeviceBuffer(DeviceBuffer &&o) noexcept
      : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  DeviceBuffer &operator=(DeviceBuffer &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      n_ = std::exchange(o.n_, 0);
    }
    return *this;
  }
  ~DeviceBuffer() { reset(); }

  T *get() const { return p_; }
  int64_t size() const { return n_; }
  operator T *() const { return p_; }

  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    n_ = 0;
  }

  // Drops the old block, then holds exactly `count` elements.
  void allocate(int64_t count) {
    reset();
    if (count <= 0) return;
    void *p = nullptr;
    PT_HIP_CHECK(hipMalloc(&p, (size_t)count * sizeof(T)));
    p_ = (T *)p;
    n_ = count;
  }

  // Growth policy of every scratch buffer: keep a block that is large
  // enough, else replace it by one with 25 % headroom.  Contents are lost.
  void reserve(int64_t count) {
    if (count > n_) allocate(count + count / 4);
  }

private:
  T *p_ = nullptr;
  int64_t n_ = 0;
};

// The same for pinned host memory.
template <class T> class PinnedBuffer {
public:
  PinnedBuffer() = default;
  explicit PinnedBuffer(int64_t count) { allocate(count); }
  PinnedBuffer(PinnedBuffer &&o) noexcept
      : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  PinnedBuffer &operator=(PinnedBuffer &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      n_ = std::exchange(o.n_, 0);
    }
    return *this;
  }
  ~PinnedBuffer() { reset(); }

  T *get() const { return p_; }
  int64_t size() const { return n_; }
  operator T *() const { return p_; }

  void reset() {
    if (p_) (void)hipHostFree(p_);
    p_ = nullptr;
    n_ = 0;
  }

  void allocate(int64_t count) {
    reset();
    if (count <= 0) return;
    void *p = nullptr;
    PT_HIP_CHECK(
        hipHostMalloc(&p, (size_t)count * sizeof(T), hipHostMallocDefault));
    p_ = (T *)p;
    n_ = count;
  }

private:
  T *p_ = nullptr;
  int64_t n_ = 0;
};

// Device copy of a host vector (synchronous H2D).
template <class T> DeviceBuffer<T> upload(const std::vector<T> &v) {
  DeviceBuffer<T> d((int64_t)v.size());
  if (!v.empty())
    PT_HIP_CHECK(hipMemcpy(d.get(), v.data(), v.size() * sizeof(T),
                           hipMemcpyHostToDevice));
  return d;
}

// Non-blocking stream.  Empty until create(), which needs the device set.
class Stream {
public:
  Stream() = default;
  Stream(const Stream &) = delete;
  Stream &operator=(const Stream &) = delete;
  ~Stream() {
    if (s_) (void)hipStreamDestroy(s_);
  }
  void create() {
    PT_HIP_CHECK(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking));
  }
  operator hipStream_t() const { return s_; }

private:
  hipStream_t s_ = nullptr;
};

// Event without timing.  Empty until create().
class Event {
public:
  Event() = default;
  Event(const Event &) = delete;
  Event &operator=(const Event &) = delete;
  ~Event() {
    if (e_) (void)hipEventDestroy(e_);
  }
  void create() {
    PT_HIP_CHECK(hipEventCreateWithFlags(&e_, hipEventDisableTiming));
  }
  operator hipEvent_t() const { return e_; }

private:
  hipEvent_t e_ = nullptr;
};

} // namespace pumitally
