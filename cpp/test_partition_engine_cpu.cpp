// CPU stateful partitioned engine against the replicated CPU engine
// (scenario in partition_cpu_scenario.h).  No GPU: passes in a build
// configured with a plain host compiler.
#include "partition_cpu_scenario.h"

int main() {
  const int fail = pumitally::partition_cpu_scenario();
  std::printf("test_partition_engine_cpu: %s\n", fail ? "FAIL" : "PASS");
  return fail ? 1 : 0;
}
