// Device data of batched scans (batch.hip, verify.hip's batch instantiation).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "verify.h"

namespace yamd {

constexpr uint32_t kBatchUnit = 256;   // arena candidates per wave of the partition

// The partition of an arena's candidate stream into its buffers' streams.
struct BatchParams {
  const uint64_t* positions;   // the arena scan's ascending candidates
  uint64_t count;
  uint64_t units;              // ceil(count / kBatchUnit)
  const uint8_t* data;         // the arena (position 0)
  const uint64_t* starts;      // [n] ascending, 16-byte aligned
  const uint64_t* sizes;       // [n]
  uint32_t n;
  const uint32_t* exact;       // ScanParams::exact and its 3-byte table
  uint32_t t3_off, t3_mask, len_mask;
  uint32_t* tmp_buf;           // [count] each arena candidate's buffer, or dropped
  uint32_t* unit_count;        // [units] kept candidates
  uint64_t* unit_off;          // [units + 1] their exclusive offsets, the kept total
  uint64_t* out_pos;           // [kept] positions local to the buffer
  uint32_t* out_buf;           // [kept] the buffer
  uint32_t* out_index;         // [kept] index in the buffer's own stream
  uint64_t* cand_off;          // [n + 1] CSR offsets of the buffers' streams
};

hipError_t launch_batch_partition(const BatchParams& p, uint64_t* summary, hipStream_t s);

// What batch pre-verification decides a candidate against: its own buffer.
struct BatchView {
  const uint64_t* starts;      // [n]
  const uint64_t* sizes;       // [n]
  const uint64_t* bases;       // [n] YR_MEMORY_BLOCK.base of each buffer, or null: all 0
  const uint32_t* cand_buf;    // [count] BatchParams::out_buf
};

// The passes of verify.hip over a batch's stream (launch_verify's roles), and
// the CSR offsets of the buffers' records from pass 0's counts.
hipError_t launch_verify_batch(const VerifyParams& p, const BatchView& b, int pass, hipStream_t s);
hipError_t launch_batch_rec_offsets(const VerifyParams& p, const uint64_t* cand_off, uint32_t n,
                                    uint64_t* rec_off, hipStream_t s);

constexpr uint32_t kGatherChunk = 512;   // arena granules (16 bytes) per wave and step: 8 KiB

// Packing an arena from buffers scattered in device memory (gather.hip).
struct GatherParams {
  uint8_t* arena;              // 16-byte aligned; [0, arena_size) is written, nothing else
  uint64_t arena_size;
  const uint64_t* starts;      // [n] ascending, 16-byte aligned, buffers not overlapping
  const uint64_t* sizes;       // [n]
  const uint64_t* ptrs;        // [n] device addresses of the buffers, any alignment
  uint32_t n;
};

hipError_t launch_batch_gather(const GatherParams& p, hipStream_t s);

}  // namespace yamd
