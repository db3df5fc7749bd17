// The block-count scan shared by the stream compaction (rowops.hip) and the CSV line ends
// (csv_scan.hip); see scan.hip.  The device side of every scan is scan.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dq4ml {

// counts[0 .. nb) becomes its exclusive scan, in place, and counts[nb] the total
void scan_counts(int64_t* counts, int64_t nb, hipStream_t st);

}  // namespace dq4ml
