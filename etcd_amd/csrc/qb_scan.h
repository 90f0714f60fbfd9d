// qb_scan.h — exclusive prefix sum of a u32 array on the device
// (qb_scan.hip).  The caller checks the launches (QB_CHECK_LAUNCH) after the
// call.
#pragma once

#include "qb_common.h"

namespace qb {
namespace scan {

constexpr int kScanPer = 4096;  // elements per scan block (1024 x 4)

inline u32 blocks(u64 n) { return u32((n + kScanPer - 1) / kScanPer); }

// data[0..n) <- exclusive prefix sums, data[n] <- total (data has n+1
// entries); bsum: scratch of blocks(n) + 1 u32.
void launch(u32* data, u64 n, u32* bsum, hipStream_t st);

// The same without the add-back: data[i] <- exclusive prefix sum within its
// block of kScanPer, bsum[b] <- exclusive prefix sum of the block totals,
// *total_slot <- total.  The caller adds bsum[i / kScanPer] to data[i].
void launch_partial(u32* data, u64 n, u32* bsum, u32* total_slot, hipStream_t st);

}  // namespace scan
}  // namespace qb
