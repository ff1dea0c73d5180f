// Linked ONLY by the CPU-only CMake configuration (a host compiler that
// is not hipcc): the GPU engine factories honor their documented contract
// ("returns nullptr when no HIP device is available") so the PumiTally
// facade, the engine_api example and make_partitioned_engine fall back to
// the CPU engines.  The hipcc build replaces this TU with the real
// factories in csrc/hip/engine_gpu.hip and csrc/hip/partition_engine.hip.
#include "engine.h"
#include "partition_engine_common.h"

namespace pumitally {

std::unique_ptr<Engine> make_gpu_engine(Mesh, int64_t, int, int, int, bool linear,
                                        bool currents, bool) {
  check_tally_options(linear, currents);
  return nullptr;
}

std::unique_ptr<PartitionedEngine>
make_gpu_partitioned_engine(const PartitionedEngineArgs &, int) {
  return nullptr;
}

} // namespace pumitally
