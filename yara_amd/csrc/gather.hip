// gfx950 kernel that packs a batch's arena from buffers scattered in device
// memory (yr_amd_batch_gather, include/yara_amd.h).
//
// Buffer k's bytes [ptrs[k], ptrs[k] + sizes[k]) go to [starts[k], starts[k] +
// sizes[k]) of the arena and every other byte of [0, arena_size) becomes zero,
// so a packed arena is a function of the buffers alone (the host path zeroes
// its staging the same way).
//
// The work is cut by DESTINATION.  Starts are 16-byte aligned and buffers do
// not overlap, so an aligned 16-byte granule of the arena holds bytes of at
// most one buffer: its owner, the LAST k with starts[k] <= the granule's
// address (batch.hip find_buffer's rule for the equal starts of empty
// buffers).  A wave takes chunks of kGatherChunk granules, whatever the sizes:
// one 1 GiB buffer and 70,000 buffers of a few bytes are both flat grids.
//   - per chunk, once per wave: the range of owners, by 64-ary searches over
//     the starts (every lane probes, one ballot per level: 3 dependent loads
//     for 65,536 buffers where a binary search takes 16);
//   - a chunk inside one buffer: whole loads and stores, nothing per lane;
//   - else per granule, each lane: its owner inside that range (a binary
//     search over a handful of entries), four granules in flight.
// Destination: one aligned 16-byte store per lane, consecutive lanes on
// consecutive granules, bytes outside the buffer zeroed in registers; plain
// stores, so the lines stay in L2 for the scan that follows.  Only a last
// granule cut by arena_size is written with narrower stores (8/4/2/1, each
// naturally aligned): no byte at or beyond arena_size is written.
// Source: any alignment.  A granule whose 16 bytes all lie inside the buffer
// is ONE unaligned 16-byte load (gfx950 global loads take any address); head
// and tail granules load their 1..15 valid bytes as 8/4/2/1-byte pieces.  No
// load touches a byte outside [ptrs[k], ptrs[k] + sizes[k]).  Sources are
// read once: non-temporal loads.
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "batch.h"

namespace yamd {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// sources: global memory (global_load, not flat_load), at any address
#define YAMD_GLOBAL __attribute__((address_space(1)))
typedef u32x4 u32x4_any __attribute__((aligned(1)));
typedef uint64_t u64_any __attribute__((aligned(1)));
typedef uint32_t u32_any __attribute__((aligned(1)));
typedef uint16_t u16_any __attribute__((aligned(1)));
typedef const YAMD_GLOBAL uint8_t* src_ptr;

template <typename T>
__device__ __forceinline__ T load_once(src_ptr at) {
  return __builtin_nontemporal_load(reinterpret_cast<const YAMD_GLOBAL T*>(at));
}

constexpr uint32_t kGatherSteps = kGatherChunk / 64;   // granules per lane and chunk
constexpr uint32_t kGatherBatch = 4;                   // of them in flight on the general path

// How many of the ascending starts[0, n) are <= a, known to lie in [lo, hi]:
// a 64-ary search by the whole wave.  The result is wave-uniform.
__device__ __forceinline__ uint32_t wave_count_le(const uint64_t* __restrict__ starts, uint32_t lo,
                                                  uint32_t hi, uint64_t a, uint32_t lane) {
  while (lo < hi) {
    const uint64_t step = (uint64_t)(hi - lo) / 64 + 1;   // 64 * step > hi - lo
    const uint64_t at = lo + lane * step;
    const bool le = at < hi && starts[at] <= a;           // true for the first c lanes only
    const uint32_t c = (uint32_t)__popcll(__ballot(le));
    // starts[lo + (c - 1) * step] <= a < starts[lo + c * step] (where probed)
    const uint64_t below = lo + c * step;
    if (c > 0) lo = (uint32_t)(below - step + 1);
    hi = (uint32_t)std::min<uint64_t>(hi, below);
  }
  return lo;
}

// 1..15 bytes at src as the low bytes of a granule: pieces of 8, 4, 2, 1, all
// inside the buffer; a piece starts at a multiple of its size in the granule,
// so none straddles a half.
__device__ __forceinline__ u32x4 load_tail(src_ptr src, uint32_t left) {
  uint64_t h[2] = {0, 0};   // two little-endian halves
  uint32_t at = 0;
  if (left & 8) {
    h[0] = load_once<u64_any>(src);
    at = 8;
  }
  if (left & 4) {
    const uint64_t x = load_once<u32_any>(src + at);
    if (at) h[1] = x; else h[0] = x;
    at += 4;
  }
  if (left & 2) {
    const uint64_t x = load_once<u16_any>(src + at);
    if (at & 8) h[1] |= x << (8 * (at & 7)); else h[0] |= x << (8 * at);
    at += 2;
  }
  if (left & 1) {
    const uint64_t x = load_once<uint8_t>(src + at);
    if (at & 8) h[1] |= x << (8 * (at & 7)); else h[0] |= x << (8 * at);
  }
  return u32x4{(uint32_t)h[0], (uint32_t)(h[0] >> 32), (uint32_t)h[1], (uint32_t)(h[1] >> 32)};
}

// The arena granule at address a: one 16-byte store, or, for a last granule
// cut by arena_size, its 1..15 bytes as 8/4/2/1 (each naturally aligned).
__device__ __forceinline__ void store_granule(uint8_t* __restrict__ arena, uint64_t arena_size,
                                              uint64_t a, const u32x4& v) {
  if (a + 16 <= arena_size) {
    *reinterpret_cast<u32x4*>(arena + a) = v;
    return;
  }
  const uint32_t left = (uint32_t)(arena_size - a);   // 1..15
  uint8_t* d = arena + a;
  if (left & 8) {
    *reinterpret_cast<uint64_t*>(d) = v.x | (uint64_t)v.y << 32;
    d += 8;
  }
  const uint32_t w[2] = {(left & 8) ? v.z : v.x, (left & 8) ? v.w : v.y};
  uint32_t at = 0;   // (bytes of w)
  if (left & 4) {
    *reinterpret_cast<uint32_t*>(d) = w[0];
    at = 4;
  }
  const uint32_t r = at ? w[1] : w[0];
  if (left & 2) {
    *reinterpret_cast<uint16_t*>(d + at) = (uint16_t)r;
    at += 2;
  }
  if (left & 1) d[at] = (uint8_t)((at & 2) ? r >> 16 : r);
}

__global__ __launch_bounds__(256) void batch_gather_kernel(GatherParams p) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64);
  const uint64_t granules = (p.arena_size + 15) / 16;
  const uint64_t chunks = (granules + kGatherChunk - 1) / kGatherChunk;
  const uint64_t* __restrict__ starts = p.starts;
  uint8_t* __restrict__ arena = p.arena;
  for (uint64_t c = (uint64_t)blockIdx.x * (blockDim.x / 64) + wave; c < chunks; c += waves) {
    const uint64_t g0 = c * kGatherChunk, g1 = std::min<uint64_t>(g0 + kGatherChunk, granules);
    // the owners of the chunk's granules are k = lo - 1 .. hi - 1 (hi: first
    // among the next 64 starts, one probe, which all but empty buffers settle)
    const uint32_t lo = wave_count_le(starts, 0, p.n, g0 * 16, lane);
    const uint32_t near = (uint32_t)std::min<uint64_t>((uint64_t)lo + 64, p.n);
    uint32_t hi = wave_count_le(starts, lo, near, (g1 - 1) * 16, lane);
    if (hi == near) hi = wave_count_le(starts, hi, p.n, (g1 - 1) * 16, lane);
    if (lo == hi && lo > 0 && g1 * 16 <= p.arena_size) {
      // one owner: (wave-uniform) inside it, every granule is a whole load
      const uint32_t k = lo - 1;
      const uint64_t start = starts[k], size = p.sizes[k];
      if (start <= g0 * 16 && g1 * 16 - start <= size) {
        const src_ptr src = reinterpret_cast<src_ptr>(p.ptrs[k]) + (g0 * 16 - start);   // granule g0
        u32x4 v[kGatherSteps];
#pragma unroll
        for (uint32_t j = 0; j < kGatherSteps; ++j) {
          const uint64_t g = g0 + j * 64 + lane;
          v[j] = u32x4{0u, 0u, 0u, 0u};
          if (g < g1) v[j] = load_once<u32x4_any>(src + (g - g0) * 16);
        }
#pragma unroll
        for (uint32_t j = 0; j < kGatherSteps; ++j) {
          const uint64_t g = g0 + j * 64 + lane;
          if (g < g1) *reinterpret_cast<u32x4*>(arena + g * 16) = v[j];
        }
        continue;
      }
    }
    // several owners, heads, tails, gaps.  A lane resolves kGatherBatch granules
    // at a time, phase by phase, so that each phase's loads are in flight
    // together: the owner (a binary search over [lo, hi] in a wave-uniform
    // number of steps, after which a range of hi - lo has closed), its table
    // entries, the bytes.
    uint32_t iters = 0;
    while (((uint64_t)1 << iters) <= hi - lo) ++iters;
    for (uint32_t j0 = 0; j0 < kGatherSteps && g0 + j0 * 64 < g1; j0 += kGatherBatch) {
      uint64_t a[kGatherBatch];
      uint32_t l[kGatherBatch], h[kGatherBatch];
      bool live[kGatherBatch];
#pragma unroll
      for (uint32_t b = 0; b < kGatherBatch; ++b) {
        const uint64_t g = g0 + (j0 + b) * 64 + lane;
        live[b] = g < g1;
        a[b] = g * 16;
        l[b] = lo;
        h[b] = live[b] ? hi : lo;
      }
      for (uint32_t it = 0; it < iters; ++it) {
#pragma unroll
        for (uint32_t b = 0; b < kGatherBatch; ++b) {   // (iters > 0: n > 0, starts[0] exists)
          const bool open = l[b] < h[b];
          const uint32_t mid = l[b] + (h[b] - l[b]) / 2;
          const bool le = starts[open ? mid : 0] <= a[b];
          l[b] = open && le ? mid + 1 : l[b];
          h[b] = open && !le ? mid : h[b];
        }
      }
      uint64_t start[kGatherBatch], size[kGatherBatch], ptr[kGatherBatch];
#pragma unroll
      for (uint32_t b = 0; b < kGatherBatch; ++b) {
        start[b] = size[b] = ptr[b] = 0;
        if (live[b] && l[b] > 0) {   // (else: before the first buffer)
          start[b] = starts[l[b] - 1];
          size[b] = p.sizes[l[b] - 1];
          ptr[b] = p.ptrs[l[b] - 1];
        }
      }
      src_ptr src[kGatherBatch];
      uint32_t left[kGatherBatch];   // bytes of the granule inside its owner, 0..16
      u32x4 v[kGatherBatch];
#pragma unroll
      for (uint32_t b = 0; b < kGatherBatch; ++b) {
        const uint64_t off = a[b] - start[b];   // (size 0: a gap, an empty owner, or no owner)
        left[b] = off < size[b] ? (uint32_t)std::min<uint64_t>(size[b] - off, 16) : 0u;
        src[b] = reinterpret_cast<src_ptr>(ptr[b]) + off;
        v[b] = u32x4{0u, 0u, 0u, 0u};
        if (left[b] == 16) v[b] = load_once<u32x4_any>(src[b]);
      }
#pragma unroll
      for (uint32_t b = 0; b < kGatherBatch; ++b)
        if (left[b] - 1u < 15u) v[b] = load_tail(src[b], left[b]);
#pragma unroll
      for (uint32_t b = 0; b < kGatherBatch; ++b)
        if (live[b]) store_granule(arena, p.arena_size, a[b], v[b]);
    }
  }
}

}  // namespace

hipError_t launch_batch_gather(const GatherParams& p, hipStream_t s) {
  if (p.arena_size == 0) return hipSuccess;
  const uint64_t granules = (p.arena_size + 15) / 16;
  const uint64_t chunks = (granules + kGatherChunk - 1) / kGatherChunk;
  // (a capped grid, the waves stride over the chunks: 2,048 blocks of 4 waves)
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((chunks + 3) / 4, 2048);
  hipLaunchKernelGGL(batch_gather_kernel, dim3(blocks), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace yamd
