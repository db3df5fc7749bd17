// The exclusive scan of per-block counts, in place, with the total behind them: the step between
// the count pass and the write pass of the stream compaction and of the CSV line ends.  One block
// walks the array with the row walker of scan.h, four consecutive entries per thread.  (A first
// version had each thread sum a contiguous 1/1024 of the array serially: 150 us for the counts of
// a 0.9 GB CSV input.)
#include "scan_host.h"

#include <stdexcept>

#include "scan.h"

namespace dq4ml {
namespace {

constexpr int kCountWaves = 1024 / kWave;

__global__ __launch_bounds__(1024) void scan_counts_kernel(long long* counts, int64_t nb) {
  __shared__ long long red[kCountWaves];
  const long long total = scan_row<AddI64, kCountWaves, 4>(counts, nb, 0, red);
  if (threadIdx.x == 0) counts[nb] = total;
}

}  // namespace

void scan_counts(int64_t* counts, int64_t nb, hipStream_t st) {
  if (nb < 0) throw std::invalid_argument("scan_counts: negative length");
  if (counts == nullptr) throw std::invalid_argument("scan_counts: null buffer");
  hipLaunchKernelGGL(scan_counts_kernel, dim3(1), dim3(1024), 0, st, reinterpret_cast<long long*>(counts), nb);
  DQ_HIP_CHECK(hipGetLastError());
}

}  // namespace dq4ml
