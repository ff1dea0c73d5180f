// RCCL transport: device-buffer collectives over xGMI.
//
// One rcclComm per process (one process per GPU, the MI355X-native
// scaling shape); the unique id is exchanged over the TcpComm bootstrap,
// so no MPI anywhere.  Flux all-reduce uses ncclAllReduce (the nelems-
// sized fp64 tally, once per batch); the partitioned particle handoff
// uses grouped ncclSend/ncclRecv pairs -- on xGMI every GPU pair has a
// direct link (7 links/GPU), so pairwise send/recv IS the right
// all-to-all shape, not a ring.
//
// Replaces the MPI communication the reference delegates to
// pumipic::Library / picparts migration (/root/reference/src/pumitally/
// PumiTallyImpl.cpp:238-241,454).
#include "comm.h"
#include "../hip/hip_util.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstring>
#include <stdexcept>
#include <string>

namespace pumitally {

namespace {

#define PT_NCCL_CK(expr)                                                       \
  do {                                                                         \
    ncclResult_t _r = (expr);                                                  \
    if (_r != ncclSuccess)                                                     \
      throw std::runtime_error(std::string("RCCL error at comm_rccl:") +       \
                               std::to_string(__LINE__) + ": " +               \
                               ncclGetErrorString(_r));                        \
  } while (0)

class RcclComm final : public Comm {
public:
  RcclComm(int rank, int world, const std::string &addr, int port, int device)
      : device_(device) {
    boot_ = make_tcp_comm(rank, world, addr, port);
    PT_HIP_CHECK(hipSetDevice(device_));
    ncclUniqueId id;
    if (rank == 0) PT_NCCL_CK(ncclGetUniqueId(&id));
    boot_->bcast(&id, sizeof id, 0);
    PT_NCCL_CK(ncclCommInitRank(&comm_, world, id, rank));
    stream_.create();
  }

  ~RcclComm() override {
    (void)hipSetDevice(device_);
    if (comm_) (void)ncclCommDestroy(comm_);
  }

  int rank() const override { return boot_->rank(); }
  int world() const override { return boot_->world(); }
  void barrier() override { boot_->barrier(); }

  void allreduce_sum(double *data, int64_t n) override {
    // host buffer: stage through device scratch; xGMI all-reduce is far
    // faster than the TCP hub for the nelems-sized flux arrays
    PT_HIP_CHECK(hipSetDevice(device_));
    d_a_.reserve(n);
    PT_HIP_CHECK(hipMemcpy(d_a_, data, n * 8, hipMemcpyHostToDevice));
    allreduce_sum_device(d_a_, n);
    PT_HIP_CHECK(hipMemcpy(data, d_a_, n * 8, hipMemcpyDeviceToHost));
  }

  void allreduce_sum(int64_t *data, int64_t n) override {
    boot_->allreduce_sum(data, n); // small control-plane data
  }

  void allreduce_max(double *data, int64_t n) override {
    boot_->allreduce_max(data, n); // small control-plane data
  }

  void bcast(void *data, int64_t bytes, int root) override {
    boot_->bcast(data, bytes, root);
  }

  std::vector<int64_t> allgather(int64_t v) override {
    return boot_->allgather(v);
  }

  std::vector<double> alltoallv(
      const double *send, const std::vector<int64_t> &send_counts) override {
    // host-buffer convenience: exchange counts over TCP, data over xGMI
    PT_HIP_CHECK(hipSetDevice(device_));
    const int w = world();
    std::vector<int64_t> flat(w * w, 0);
    for (int r = 0; r < w; ++r) flat[(int64_t)rank() * w + r] = send_counts[r];
    boot_->allreduce_sum(flat.data(), w * w); // zeros elsewhere -> allgather
    std::vector<int64_t> recv_counts(w);
    for (int s = 0; s < w; ++s) recv_counts[s] = flat[(int64_t)s * w + rank()];
    int64_t stot = 0, rtot = 0;
    for (int64_t c : send_counts) stot += c;
    for (int64_t c : recv_counts) rtot += c;
    d_a_.reserve(stot);
    PT_HIP_CHECK(hipMemcpy(d_a_, send, stot * 8, hipMemcpyHostToDevice));
    double *d_recv = nullptr;
    alltoallv_device(d_a_, send_counts, recv_counts, &d_recv);
    std::vector<double> out(rtot);
    if (rtot)
      PT_HIP_CHECK(
          hipMemcpy(out.data(), d_recv, rtot * 8, hipMemcpyDeviceToHost));
    return out;
  }

  bool has_device_collectives() const override { return true; }

  void allreduce_sum_device(double *d_data, int64_t n) override {
    PT_HIP_CHECK(hipSetDevice(device_));
    PT_NCCL_CK(ncclAllReduce(d_data, d_data, (size_t)n, ncclDouble, ncclSum,
                             comm_, stream_));
    PT_HIP_CHECK(hipStreamSynchronize(stream_));
  }

  int64_t alltoallv_device(const double *d_send,
                           const std::vector<int64_t> &send_counts,
                           const std::vector<int64_t> &recv_counts,
                           double **d_recv) override {
    PT_HIP_CHECK(hipSetDevice(device_));
    const int w = world();
    int64_t rtot = 0;
    for (int64_t c : recv_counts) rtot += c;
    d_b_.reserve(rtot);
    PT_NCCL_CK(ncclGroupStart());
    int64_t soff = 0, roff = 0;
    for (int r = 0; r < w; ++r) {
      if (send_counts[r])
        PT_NCCL_CK(ncclSend(d_send + soff, (size_t)send_counts[r], ncclDouble,
                            r, comm_, stream_));
      if (recv_counts[r])
        PT_NCCL_CK(ncclRecv(d_b_ + roff, (size_t)recv_counts[r], ncclDouble,
                            r, comm_, stream_));
      soff += send_counts[r];
      roff += recv_counts[r];
    }
    PT_NCCL_CK(ncclGroupEnd());
    PT_HIP_CHECK(hipStreamSynchronize(stream_));
    *d_recv = d_b_;
    return rtot;
  }

private:
  int device_;
  std::unique_ptr<Comm> boot_;
  ncclComm_t comm_ = nullptr;
  Stream stream_;
  DeviceBuffer<double> d_a_, d_b_; // staging / recv scratch
};

} // namespace

std::unique_ptr<Comm> make_rccl_comm(int rank, int world,
                                     const std::string &addr, int port,
                                     int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= device) {
    (void)hipGetLastError();
    return nullptr;
  }
  return std::make_unique<RcclComm>(rank, world, addr, port, device);
}

} // namespace pumitally
