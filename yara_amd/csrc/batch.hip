// gfx950 kernels of batched scans (yr_amd_scan_batch_device, include/yara_amd.h).
//
// A batch is N independent buffers lying in one device arena at 16-byte-aligned
// starts.  The arena is scanned as ONE block by the unchanged scan kernel; these
// kernels then cut its ascending candidate stream into the N buffers' own
// streams.  Why that is exact:
//   - position i is a candidate iff some key (at most 4 bytes, limits.h:68) is a
//     suffix of the bytes before it, so at a local position >= 4 the arena's
//     walk and the buffer's own walk agree;
//   - at local positions 1..3 the arena sees bytes of the gap or of the buffer
//     before, so its stream is a superset there: those candidates are decided
//     again here, from the buffer's own first bytes and the exact key sets
//     (ScanParams::exact) -- never from anything outside the buffer;
//   - arena positions in no (start_k, start_k + size_k] belong to no buffer.
// Candidates are only ever dropped, so the order is the scan's.
//
// Passes (all queued on the scanner's stream, no host round trip):
//   decide   one wave per unit of 256 candidates: each candidate's buffer
//            (binary search over the starts) or kDropped, the unit's kept count
//   (exclusive offsets of the unit counts: kernels.hip launch_counts_offsets)
//   scatter  local positions and buffer indices, compacted in order
//   csr      cand_off[k] = first kept candidate of buffer k (lower bound), and
//            each kept candidate's index in its own buffer's stream
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "batch.h"
#include "internal.h"

namespace yamd {

namespace {

constexpr uint32_t kDropped = 0xFFFFFFFFu;

// The largest k with starts[k] < i, or kDropped.  Empty buffers may share a
// start with the buffer after them: the last of equal starts is the one that
// can hold bytes.
__device__ __forceinline__ uint32_t find_buffer(const uint64_t* __restrict__ starts, uint32_t n,
                                                uint64_t i) {
  uint32_t lo = 0, hi = n;   // first k in [0, n] with starts[k] >= i
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (starts[mid] < i) lo = mid + 1; else hi = mid;
  }
  return lo == 0 ? kDropped : lo - 1;
}

__device__ __forceinline__ bool bucket_has(const uint4& a, const uint4& b, uint32_t k) {
  return a.x == k || a.y == k || a.z == k || a.w == k || b.x == k || b.y == k || b.z == k ||
         b.w == k;
}

// Does a key of length L <= n (n = 1..3) equal the last L of the buffer's
// first n bytes?  (kernels.hip exact_check for a position below 4.)
__device__ bool short_key_ends(const BatchParams& p, const uint8_t* __restrict__ buf, uint32_t n) {
  uint32_t w = 0;   // the n bytes, oldest lowest, at the top of the word
  for (uint32_t j = 0; j < n; ++j) w |= (uint32_t)buf[j] << (8 * (4 - n + j));
  const uint32_t* __restrict__ ex = p.exact;
  const uint32_t k1 = w >> 24, k2 = w >> 16, k3 = (w >> 8) | (1u << 24);
  if ((p.len_mask & 2u) && ((ex[kExactBm1 + (k1 >> 5)] >> (k1 & 31u)) & 1u)) return true;
  if (n >= 2 && (p.len_mask & 4u) && ((ex[kExactBm2 + (k2 >> 5)] >> (k2 & 31u)) & 1u)) return true;
  if (n >= 3 && (p.len_mask & 8u)) {
    const uint4 a = *reinterpret_cast<const uint4*>(ex + p.t3_off + (bucket_hash1(k3) & p.t3_mask) * 4);
    const uint4 b = *reinterpret_cast<const uint4*>(ex + p.t3_off + (bucket_hash2(k3) & p.t3_mask) * 4);
    if (bucket_has(a, b, k3)) return true;
  }
  return false;
}

__device__ __forceinline__ uint32_t decide(const BatchParams& p, uint64_t c) {
  const uint64_t i = p.positions[c];
  const uint32_t k = find_buffer(p.starts, p.n, i);
  if (k == kDropped) return kDropped;
  const uint64_t local = i - p.starts[k];
  if (local > p.sizes[k]) return kDropped;   // a gap, or the bytes behind the last buffer
  if (local < 4 && !short_key_ends(p, p.data + p.starts[k], (uint32_t)local)) return kDropped;
  return k;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ __launch_bounds__(256) void batch_decide_kernel(BatchParams p) {
  const uint64_t u = (uint64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (u >= p.units) return;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t kept = 0;
  for (uint32_t j = 0; j < kBatchUnit / 64; ++j) {
    const uint64_t c = u * kBatchUnit + j * 64 + lane;
    uint32_t k = kDropped;
    if (c < p.count) {
      k = decide(p, c);
      p.tmp_buf[c] = k;
    }
    kept += (uint32_t)__popcll(__ballot(k != kDropped));
  }
  if (lane == 0) p.unit_count[u] = kept;
}

__global__ __launch_bounds__(256) void batch_scatter_kernel(BatchParams p) {
  const uint64_t u = (uint64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (u >= p.units) return;
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t o = p.unit_off[u];
  for (uint32_t j = 0; j < kBatchUnit / 64; ++j) {
    const uint64_t c = u * kBatchUnit + j * 64 + lane;
    const uint32_t k = c < p.count ? p.tmp_buf[c] : kDropped;
    const uint64_t m = __ballot(k != kDropped);
    if (k != kDropped) {
      const uint64_t at = o + lanes_below(m);
      p.out_pos[at] = p.positions[c] - p.starts[k];
      p.out_buf[at] = k;
    }
    o += (uint64_t)__popcll(m);
  }
}

// cand_off[k], k in [0, n]: the first kept candidate whose buffer is >= k
// (out_buf ascends); cand_off[n] = the kept total.
__global__ __launch_bounds__(256) void batch_csr_kernel(BatchParams p) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > p.n) return;
  const uint64_t total = p.unit_off[p.units];
  uint64_t lo = 0, hi = total;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (p.out_buf[mid] < k) lo = mid + 1; else hi = mid;
  }
  p.cand_off[k] = lo;
}

// Each kept candidate's index in its own buffer's stream (the records'
// candidate field).
__global__ __launch_bounds__(256) void batch_local_index_kernel(BatchParams p) {
  const uint64_t total = p.unit_off[p.units];
  for (uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total;
       o += (uint64_t)gridDim.x * blockDim.x)
    p.out_index[o] = (uint32_t)(o - p.cand_off[p.out_buf[o]]);
}

}  // namespace

hipError_t launch_counts_offsets(const uint32_t* counts, uint32_t n, uint64_t* offsets, uint64_t* summary,
                                 hipStream_t s);   // (kernels.hip)

hipError_t launch_batch_partition(const BatchParams& p, uint64_t* summary, hipStream_t s) {
  if (p.count == 0 || p.units == 0) return hipErrorInvalidValue;
  const uint32_t blocks = (uint32_t)((p.units + 3) / 4);
  hipLaunchKernelGGL(batch_decide_kernel, dim3(blocks), dim3(256), 0, s, p);
  hipError_t e = launch_counts_offsets(p.unit_count, (uint32_t)p.units, p.unit_off, summary, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(batch_scatter_kernel, dim3(blocks), dim3(256), 0, s, p);
  hipLaunchKernelGGL(batch_csr_kernel, dim3((uint32_t)(((uint64_t)p.n + 1 + 255) / 256)), dim3(256), 0,
                     s, p);
  const uint32_t iblocks = (uint32_t)std::min<uint64_t>((p.count + 255) / 256, 4096);
  hipLaunchKernelGGL(batch_local_index_kernel, dim3(iblocks), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace yamd
