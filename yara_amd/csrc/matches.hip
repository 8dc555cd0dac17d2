// gfx950 kernels of the final-match stage (yr_amd_match_device): the records
// of the pre-verification (verify.hip) whose string is FINAL (matches.h) become
// YR_MATCH-equivalent records on the device -- string, offset, length, xor key
// -- de-duplicated and ordered as libyara's per-string match lists are.
//
// A kept call of a final string is a match (verify.hip call_matters restates
// _yr_scan_verify_literal_match and the FULL_WORD test); what the host step
// still adds is (a) forward_matches and the xor key of scan.c:907-972, which
// call_matters computes and drops, and (b) _yr_scan_add_match_to_list
// (scan.c:290-352): per string a list ascending by offset, a second match at
// an offset already present discarded (replace_if_exists == 0 for literals).
//
//   1. match_classify_kernel, one lane per record: final test, window test,
//      the comparisons again in their length-returning form, a 64-bit key
//      string << 32 | offset (offsets are block positions below the block's
//      size, and yr_amd_match_device refuses a block of more than
//      YR_AMD_MATCH_MAX_BLOCK = 2^32 bytes, so they fit 32 bits).  Records that are
//      not matches get the string field n_strings: they sort behind every
//      match and are the REST, compacted in order by match_rest_kernel
//      (ballot + mbcnt per wave, verify.hip's offset kernels over the waves).
//   2. a stable radix sort of (key, record index) (sort_*_kernel below; the
//      ROCm library sorts carry code paths and names of other architectures
//      into the library, which holds gfx950 code only): equal keys stay in
//      record order, so the first call of a (string, offset) comes first --
//      the one whose match libyara keeps.
//   3. match_unique_kernel: an entry is kept iff its key differs from its
//      predecessor's; kept entries are compacted in order into MatchRec.
//
// With the hex class (yr_amd_scanner_set_match_classes) a record of a final
// hex string is measured too and can be several matches: hex_measure_kernel,
// hex_expand_kernel and hex_unique_kernel below take the place of 1. and 3.,
// the sort runs over the items (matches.h HexMatchParams).
// A batch with the hex class (yr_amd_scanner_set_batch_match_classes) counts
// its CSR over the items: the batch_hex_* kernels (BatchHexParams, 18.3).
// With yr_amd_scanner_set_hex_wide the records whose set leaves hex_run's 64
// positions are queued and measured one WAVE each, the whole 4096-position
// set across the lanes: the hex_wide_* kernels (HexWideParams, 18.4).  A batch
// has that path too (yr_amd_scanner_set_batch_hex_wide), each record measured
// inside its own buffer: the batch_hex_wide_* kernels (BatchHexWideParams, 18.5).
//
// The comparisons are restated here rather than shared with verify.hip: that
// file's kernels stay byte for byte what they were (their register budgets are
// tuned), and these read global memory directly -- a
// record is one in thousands of positions, and every final record's bytes were
// just read by the pre-verification, so they sit in L2.
#include <algorithm>

#include "internal.h"
#include "matches.h"
#include "match_measure.h"

namespace yamd {

namespace {

__device__ __forceinline__ uint64_t wave_offset(const MatchParams& p, uint64_t g) {
  return p.chunk_off[g / kChunkGroups] + p.block_off[g];
}

__global__ __launch_bounds__(256) void match_classify_kernel(MatchParams p) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool rest = false;
  if (r < p.n) {
    const VerifyRec rec = p.recs[r];
    const DevPoolRec e = p.pool[rec.pool_index];
    MatchMeasure m;
    const bool is_match = measure(p, e, rec.offset, m);
    const uint32_t string = is_match ? p.pool_string[rec.pool_index] : p.n_strings;
    p.keys[r] = (uint64_t)string << 32 | (rec.offset & 0xFFFFFFFFull);
    p.index[r] = (uint32_t)r;
    p.meas[r] = m;
    rest = !is_match;
  }
  const uint64_t mask = __ballot(rest);
  if ((threadIdx.x & 63u) == 0 && r < p.n) p.block_off[r / kGroup] = (uint64_t)__popcll(mask);
}

__global__ __launch_bounds__(256) void match_rest_kernel(MatchParams p) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool rest = r < p.n && (uint32_t)(p.keys[r] >> 32) == p.n_strings;
  const uint64_t mask = __ballot(rest);
  if (rest) p.rest[wave_offset(p, r / kGroup) + lanes_below(mask)] = p.recs[r];
}

template <int PASS>
__global__ __launch_bounds__(256) void match_unique_kernel(MatchParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool keep = false;
  uint64_t key = 0;
  if (i < p.n) {
    key = p.sorted_keys[i];
    keep = (uint32_t)(key >> 32) < p.n_strings && (i == 0 || p.sorted_keys[i - 1] != key);
  }
  const uint64_t mask = __ballot(keep);
  if (PASS == 0) {
    if ((threadIdx.x & 63u) == 0 && i < p.n) p.block_off[i / kGroup] = (uint64_t)__popcll(mask);
    return;
  }
  if (!keep) return;
  const uint32_t r = p.sorted_index[i];   // the first call of this (string, offset)
  const MatchMeasure m = p.meas[r];
  MatchRec o;
  o.offset = key & 0xFFFFFFFFull;
  o.string = (uint32_t)(key >> 32);
  o.length = m.length;
  o.xor_key = m.xor_key;
  o.pool_index = p.recs[r].pool_index;
  p.out[wave_offset(p, i / kGroup) + lanes_below(mask)] = o;
}

inline dim3 match_grid(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

// ---- Stable LSD radix sort of (key, index) pairs, 8 bits a pass ----
// One wave per tile of kSortTile consecutive items.  Pass: (1) each tile's
// digit histogram, stored digit-major (hist[d * tiles + t]), so that (2) one
// exclusive scan over it (verify.hip's offset kernels) gives every (digit,
// tile) its first output slot; (3) each tile walks its items again IN ORDER,
// 64 at a time: the lanes holding one digit find each other with one ballot
// per digit bit, an item's slot is the digit's running counter (LDS) plus the
// number of such lanes below it.  Order within a digit is input order -- tiles
// by the scan, rounds by the counter, lanes by the rank -- i.e. stable.
struct SortPass {
  const uint64_t* kin;
  uint64_t* kout;
  const uint32_t* vin;
  uint32_t* vout;
  uint64_t n, tiles;
  uint32_t shift, mask;     // digit = (key >> shift) & mask, mask < 256
  uint64_t* hist;           // [(mask + 1) * tiles + 1] counts, then offsets within chunks
  const uint64_t* chunk;    // the chunks' offsets (launch_block_offsets)
};

__global__ __launch_bounds__(64) void sort_hist_kernel(SortPass p) {
  __shared__ uint32_t cnt[256];
  const uint32_t lane = threadIdx.x;
  const uint64_t t = blockIdx.x;
  for (uint32_t d = lane; d < 256; d += 64) cnt[d] = 0;
  __syncthreads();
  const uint64_t lo = t * kSortTile, hi = min(lo + (uint64_t)kSortTile, p.n);
  for (uint64_t i = lo + lane; i < hi; i += 64)
    atomicAdd(&cnt[(uint32_t)(p.kin[i] >> p.shift) & p.mask], 1u);
  __syncthreads();
  for (uint32_t d = lane; d <= p.mask; d += 64) p.hist[(uint64_t)d * p.tiles + t] = cnt[d];
}

__global__ __launch_bounds__(64) void sort_scatter_kernel(SortPass p) {
  __shared__ uint32_t cnt[256];   // per digit: the next output slot of this tile
  const uint32_t lane = threadIdx.x;
  const uint64_t t = blockIdx.x;
  for (uint32_t d = lane; d <= p.mask; d += 64) {
    const uint64_t e = (uint64_t)d * p.tiles + t;
    cnt[d] = (uint32_t)(p.chunk[e / kChunkGroups] + p.hist[e]);   // (n < 2^31)
  }
  __syncthreads();
  const uint64_t lo = t * kSortTile, hi = min(lo + (uint64_t)kSortTile, p.n);
  for (uint64_t base = lo; base < hi; base += 64) {   // (uniform: barriers inside)
    const uint64_t i = base + lane;
    const bool valid = i < hi;
    const uint64_t key = valid ? p.kin[i] : 0ull;
    const uint32_t val = valid ? p.vin[i] : 0u;
    const uint32_t d = (uint32_t)(key >> p.shift) & p.mask;
    uint64_t peers = __ballot(valid);   // the valid lanes with this lane's digit
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t m = __ballot(valid && bit);
      peers &= bit ? m : ~m;
    }
    const uint32_t rank = lanes_below(peers);
    const uint32_t pos = valid ? cnt[d] + rank : 0u;
    __syncthreads();
    if (valid && rank == 0) cnt[d] += (uint32_t)__popcll(peers);
    __syncthreads();
    if (valid) {
      p.kout[pos] = key;
      p.vout[pos] = val;
    }
  }
}

// The twins of the two kernels above for the batch's buffer passes: the digit
// is of the buffer of the record that the item's value names.  (Twins, not a
// template over both: the single-block kernels stay instruction for
// instruction what they were.)
struct SortPassBuf {
  SortPass s;
  const uint32_t* buf;      // [n] by record; digit = (buf[value] >> shift) & mask
};

__global__ __launch_bounds__(64) void sort_hist_buf_kernel(SortPassBuf q) {
  __shared__ uint32_t cnt[256];
  const SortPass& p = q.s;
  const uint32_t lane = threadIdx.x;
  const uint64_t t = blockIdx.x;
  for (uint32_t d = lane; d < 256; d += 64) cnt[d] = 0;
  __syncthreads();
  const uint64_t lo = t * kSortTile, hi = min(lo + (uint64_t)kSortTile, p.n);
  for (uint64_t i = lo + lane; i < hi; i += 64)
    atomicAdd(&cnt[(q.buf[p.vin[i]] >> p.shift) & p.mask], 1u);
  __syncthreads();
  for (uint32_t d = lane; d <= p.mask; d += 64) p.hist[(uint64_t)d * p.tiles + t] = cnt[d];
}

__global__ __launch_bounds__(64) void sort_scatter_buf_kernel(SortPassBuf q) {
  __shared__ uint32_t cnt[256];   // per digit: the next output slot of this tile
  const SortPass& p = q.s;
  const uint32_t lane = threadIdx.x;
  const uint64_t t = blockIdx.x;
  for (uint32_t d = lane; d <= p.mask; d += 64) {
    const uint64_t e = (uint64_t)d * p.tiles + t;
    cnt[d] = (uint32_t)(p.chunk[e / kChunkGroups] + p.hist[e]);   // (n < 2^31)
  }
  __syncthreads();
  const uint64_t lo = t * kSortTile, hi = min(lo + (uint64_t)kSortTile, p.n);
  for (uint64_t base = lo; base < hi; base += 64) {   // (uniform: barriers inside)
    const uint64_t i = base + lane;
    const bool valid = i < hi;
    const uint64_t key = valid ? p.kin[i] : 0ull;
    const uint32_t val = valid ? p.vin[i] : 0u;
    const uint32_t d = valid ? (q.buf[val] >> p.shift) & p.mask : 0u;
    uint64_t peers = __ballot(valid);   // the valid lanes with this lane's digit
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t m = __ballot(valid && bit);
      peers &= bit ? m : ~m;
    }
    const uint32_t rank = lanes_below(peers);
    const uint32_t pos = valid ? cnt[d] + rank : 0u;
    __syncthreads();
    if (valid && rank == 0) cnt[d] += (uint32_t)__popcll(peers);
    __syncthreads();
    if (valid) {
      p.kout[pos] = key;
      p.vout[pos] = val;
    }
  }
}

// ---- The stage for a batch (matches.h BatchMatchParams) ----
// One lane per record: its buffer b is the one with rec_off[b] <= r <
// rec_off[b + 1] (empty buffers have no such r); measure() then sees the
// buffer as the whole block, as the batch pre-verification did -- no byte
// outside [starts[b], starts[b] + sizes[b]) is read, none in a gap.
__global__ __launch_bounds__(256) void batch_match_classify_kernel(BatchMatchParams p) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool rest = false;
  if (r < p.m.n) {
    uint32_t lo = 0, hi = p.nbuf;   // rec_off[lo] <= r < rec_off[hi]  (rec_off[nbuf] == n)
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (p.rec_off[mid] <= r) lo = mid; else hi = mid;
    }
    MatchParams q = p.m;
    q.data = p.m.data + p.starts[lo];
    q.size = p.sizes[lo];
    q.win_lo = 0;
    q.win_hi = q.size;
    const VerifyRec rec = p.m.recs[r];
    const DevPoolRec e = p.m.pool[rec.pool_index];
    MatchMeasure m;
    const bool is_match = measure(q, e, rec.offset, m);
    const uint32_t string = is_match ? p.m.pool_string[rec.pool_index] : p.m.n_strings;
    p.m.keys[r] = (uint64_t)string << 32 | (rec.offset & 0xFFFFFFFFull);
    p.m.index[r] = (uint32_t)r;
    p.m.meas[r] = m;
    p.buf[r] = lo;
    rest = !is_match;
  }
  const uint64_t mask = __ballot(rest);
  if ((threadIdx.x & 63u) == 0 && r < p.m.n) p.m.block_off[r / kGroup] = (uint64_t)__popcll(mask);
}

// Entry i of the sorted arrays opens a run of one (buffer, string, offset).
__device__ __forceinline__ bool batch_keep(const BatchMatchParams& p, uint64_t i, uint64_t key) {
  if ((uint32_t)(key >> 32) >= p.m.n_strings) return false;
  return i == 0 || p.m.sorted_keys[i - 1] != key ||
         p.buf[p.m.sorted_index[i - 1]] != p.buf[p.m.sorted_index[i]];
}

template <int PASS>
__global__ __launch_bounds__(256) void batch_match_unique_kernel(BatchMatchParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool keep = false;
  uint64_t key = 0;
  if (i < p.m.n) {
    key = p.m.sorted_keys[i];
    keep = batch_keep(p, i, key);
  }
  const uint64_t mask = __ballot(keep);
  if (PASS == 0) {
    if ((threadIdx.x & 63u) == 0 && i < p.m.n) p.m.block_off[i / kGroup] = (uint64_t)__popcll(mask);
    return;
  }
  if (!keep) return;
  const uint32_t r = p.m.sorted_index[i];   // the buffer's first call of this (string, offset)
  const MatchMeasure m = p.m.meas[r];
  MatchRec o;
  o.offset = key & 0xFFFFFFFFull;
  o.string = (uint32_t)(key >> 32);
  o.length = m.length;
  o.xor_key = m.xor_key;
  o.pool_index = p.m.recs[r].pool_index;
  p.m.out[wave_offset(p.m, i / kGroup) + lanes_below(mask)] = o;
}

// The CSR offsets, one lane per k in [0, nbuf].  Buffer k's records hold the
// slots [rec_off[k], rec_off[k + 1]) in record order and -- the buffer being
// the sort's most significant field -- in sorted order too, so the outputs
// before buffer k are those of the slots below c0 = rec_off[k]: the scanned
// count of c0's wave plus the flags of the wave's slots below c0 (as
// verify.hip's batch_rec_offsets_kernel counts records).  MATCHES 0: the rest
// records (keys in record order); 1: the kept entries (sorted arrays).
template <int MATCHES>
__global__ __launch_bounds__(256) void batch_match_offsets_kernel(BatchMatchParams p) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > p.nbuf) return;
  const uint64_t c0 = p.rec_off[k], g = c0 / kGroup;
  uint64_t o = wave_offset(p.m, g);   // (g == groups: the entry past the last wave, the total)
  for (uint64_t c = g * kGroup; c < c0; ++c) {
    if (MATCHES)
      o += batch_keep(p, c, p.m.sorted_keys[c]) ? 1u : 0u;
    else
      o += (uint32_t)(p.m.keys[c] >> 32) == p.m.n_strings ? 1u : 0u;
  }
  (MATCHES ? p.match_off : p.rest_off)[k] = o;
}

// ---- The stage with the hex class (matches.h HexMatchParams) ----

__device__ __forceinline__ uint32_t hex_items(uint64_t key, uint32_t n_strings, const HexSet& s) {
  return (uint32_t)(key >> 32) == n_strings ? 0u : (uint32_t)__popcll(s.mask);
}

__global__ __launch_bounds__(256) void hex_measure_kernel(HexMatchParams q) {
  // one code buffer per lane, + the operand bytes an opcode's read may reach
  // past the last lane's program
  __shared__ __attribute__((aligned(16))) uint8_t codebuf[256 * kHexCodeBytes + 16];
  const MatchParams& p = q.m;
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool rest = false;
  uint32_t items = 0;
  if (r < p.n) {
    const VerifyRec rec = p.recs[r];
    const DevPoolRec e = p.pool[rec.pool_index];
    MatchMeasure m;
    HexSet set{1ull, 0u, 0u};
    bool is_match;
    if ((q.classes & kMatchHex) && string_is_final_hex(e.flags)) {
      m.length = 0;
      m.xor_key = 0;
      // (the low 32 bits of a flat LDS address are the LDS offset)
      const uint32_t buf = (uint32_t)(uintptr_t)(codebuf + threadIdx.x * kHexCodeBytes);
      // (a record the runs find nothing for is not dropped here: the host
      // verifies it and finds what there is)
      is_match = measure_hex(q, e, rec.offset, buf, m, set) == kHexMatch;
      if (!is_match) set = HexSet{1ull, 0u, 0u};
    } else {
      is_match = measure(p, e, rec.offset, m);
    }
    const uint32_t string = is_match ? p.pool_string[rec.pool_index] : p.n_strings;
    p.keys[r] = (uint64_t)string << 32 | (rec.offset & 0xFFFFFFFFull);
    p.meas[r] = m;
    q.sets[r] = set;
    rest = !is_match;
    items = is_match ? (uint32_t)__popcll(set.mask) : 0u;
  }
  const uint64_t mask = __ballot(rest);
  const uint32_t total = (uint32_t)__shfl((int)wave_prefix(items), 63, 64);
  if ((threadIdx.x & 63u) == 0 && r < p.n) {
    p.block_off[r / kGroup] = (uint64_t)__popcll(mask);
    q.iblock_off[r / kGroup] = (uint64_t)total;
  }
}

// One lane per record: its items at the wave's offset plus the counts of the
// lanes below.  Records ascend in the item array, so the stable sort keeps
// "the first record of a (string, offset) wins".
__global__ __launch_bounds__(256) void hex_expand_kernel(HexMatchParams q) {
  const MatchParams& p = q.m;
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t key = 0;
  HexSet set{0ull, 0u, 0u};
  uint32_t items = 0;
  if (r < p.n) {
    key = p.keys[r];
    set = q.sets[r];
    items = hex_items(key, p.n_strings, set);
  }
  const uint32_t before = wave_prefix(items) - items;
  if (items == 0) return;
  const uint64_t g = r / kGroup;
  uint64_t at = q.ichunk_off[g / kChunkGroups] + q.iblock_off[g] + before;
  const uint64_t offset = key & 0xFFFFFFFFull;   // (B <= min(offset, YR_RE_SCAN_LIMIT))
  for (uint64_t x = set.mask; x != 0 && at < q.n_items; x &= x - 1, ++at) {
    const uint32_t B = set.base + (uint32_t)__builtin_ctzll(x);
    q.ikeys[at] = (key & 0xFFFFFFFF00000000ull) | (offset - B);
    q.iindex[at] = (uint32_t)r;
  }
}

template <int PASS>
__global__ __launch_bounds__(256) void hex_unique_kernel(HexMatchParams q) {
  const MatchParams& p = q.m;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool keep = false;
  uint64_t key = 0;
  if (i < q.n_items) {
    key = p.sorted_keys[i];
    keep = (uint32_t)(key >> 32) < p.n_strings && (i == 0 || p.sorted_keys[i - 1] != key);
  }
  const uint64_t mask = __ballot(keep);
  if (PASS == 0) {
    if ((threadIdx.x & 63u) == 0 && i < q.n_items)
      q.ublock_off[i / kGroup] = (uint64_t)__popcll(mask);
    return;
  }
  if (!keep) return;
  const uint32_t r = p.sorted_index[i];   // the first record with this (string, offset)
  const MatchMeasure m = p.meas[r];
  const VerifyRec rec = p.recs[r];
  MatchRec o;
  o.offset = key & 0xFFFFFFFFull;
  o.string = (uint32_t)(key >> 32);
  // B + F: B is how far the item lies before its record's offset
  o.length = m.length + (uint32_t)((rec.offset & 0xFFFFFFFFull) - o.offset);
  o.xor_key = m.xor_key;
  o.pool_index = rec.pool_index;
  const uint64_t g = i / kGroup;
  p.out[q.uchunk_off[g / kChunkGroups] + q.ublock_off[g] + lanes_below(mask)] = o;
}

// ---- The batch's stage with the hex class (matches.h BatchHexParams) ----
// hex_measure_kernel with batch_match_classify_kernel's view: the record's
// buffer is the whole block of both runs (max_bytes_matched = min(local
// offset, YR_RE_SCAN_LIMIT) backwards, min(size - local offset, ...) forwards),
// never a window -- hex_run reads live positions only, so no byte of a gap or
// of a neighbouring buffer.
__global__ __launch_bounds__(256) void batch_hex_measure_kernel(BatchHexParams b) {
  __shared__ __attribute__((aligned(16))) uint8_t codebuf[256 * kHexCodeBytes + 16];
  const MatchParams& p = b.h.m;
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool rest = false;
  uint32_t items = 0;
  if (r < p.n) {
    uint32_t lo = 0, hi = b.nbuf;   // rec_off[lo] <= r < rec_off[hi]  (rec_off[nbuf] == n)
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (b.rec_off[mid] <= r) lo = mid; else hi = mid;
    }
    HexMatchParams q = b.h;
    q.m.data = p.data + b.starts[lo];
    q.m.size = b.sizes[lo];
    q.m.win_lo = 0;
    q.m.win_hi = q.m.size;
    const VerifyRec rec = p.recs[r];
    const DevPoolRec e = p.pool[rec.pool_index];
    MatchMeasure m;
    HexSet set{1ull, 0u, 0u};
    bool is_match;
    if ((q.classes & kMatchHex) && string_is_final_hex(e.flags)) {
      m.length = 0;
      m.xor_key = 0;
      const uint32_t buf = (uint32_t)(uintptr_t)(codebuf + threadIdx.x * kHexCodeBytes);
      is_match = measure_hex(q, e, rec.offset, buf, m, set) == kHexMatch;
      if (!is_match) set = HexSet{1ull, 0u, 0u};
    } else {
      is_match = measure(q.m, e, rec.offset, m);
    }
    const uint32_t string = is_match ? p.pool_string[rec.pool_index] : p.n_strings;
    p.keys[r] = (uint64_t)string << 32 | (rec.offset & 0xFFFFFFFFull);
    p.meas[r] = m;
    b.h.sets[r] = set;
    b.buf[r] = lo;
    rest = !is_match;
    items = is_match ? (uint32_t)__popcll(set.mask) : 0u;
  }
  const uint64_t mask = __ballot(rest);
  const uint32_t total = (uint32_t)__shfl((int)wave_prefix(items), 63, 64);
  if ((threadIdx.x & 63u) == 0 && r < p.n) {
    p.block_off[r / kGroup] = (uint64_t)__popcll(mask);
    b.h.iblock_off[r / kGroup] = (uint64_t)total;
  }
}

// Item i of the sorted arrays opens a run of one (buffer, string, offset).
__device__ __forceinline__ bool batch_hex_keep(const BatchHexParams& b, uint64_t i, uint64_t key) {
  const MatchParams& p = b.h.m;
  if ((uint32_t)(key >> 32) >= p.n_strings) return false;
  return i == 0 || p.sorted_keys[i - 1] != key ||
         b.buf[p.sorted_index[i - 1]] != b.buf[p.sorted_index[i]];
}

template <int PASS>
__global__ __launch_bounds__(256) void batch_hex_unique_kernel(BatchHexParams b) {
  const MatchParams& p = b.h.m;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool keep = false;
  uint64_t key = 0;
  if (i < b.h.n_items) {
    key = p.sorted_keys[i];
    keep = batch_hex_keep(b, i, key);
  }
  const uint64_t mask = __ballot(keep);
  if (PASS == 0) {
    if ((threadIdx.x & 63u) == 0 && i < b.h.n_items)
      b.h.ublock_off[i / kGroup] = (uint64_t)__popcll(mask);
    return;
  }
  if (!keep) return;
  const uint32_t r = p.sorted_index[i];   // the buffer's first record with this (string, offset)
  const MatchMeasure m = p.meas[r];
  const VerifyRec rec = p.recs[r];
  MatchRec o;
  o.offset = key & 0xFFFFFFFFull;
  o.string = (uint32_t)(key >> 32);
  o.length = m.length + (uint32_t)((rec.offset & 0xFFFFFFFFull) - o.offset);   // B + F
  o.xor_key = m.xor_key;
  o.pool_index = rec.pool_index;
  const uint64_t g = i / kGroup;
  p.out[b.h.uchunk_off[g / kChunkGroups] + b.h.ublock_off[g] + lanes_below(mask)] = o;
}

// The CSR offsets over items, one lane per k in [0, nbuf] (as
// batch_match_offsets_kernel counts over records).  MATCHES 0: item_off[k] =
// the items of the records below c0 = rec_off[k]: the scanned item count of
// c0's wave plus the item counts of the wave's records below c0.  1:
// match_off[k] = the kept entries below slot c0 = item_off[k] of the sorted
// arrays.  (g == groups: the entry past the last wave, the total.)
template <int MATCHES>
__global__ __launch_bounds__(256) void batch_hex_offsets_kernel(BatchHexParams b) {
  const MatchParams& p = b.h.m;
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > b.nbuf) return;
  const uint64_t c0 = MATCHES ? b.item_off[k] : b.rec_off[k], g = c0 / kGroup;
  uint64_t o = MATCHES ? b.h.uchunk_off[g / kChunkGroups] + b.h.ublock_off[g]
                       : b.h.ichunk_off[g / kChunkGroups] + b.h.iblock_off[g];
  for (uint64_t c = g * kGroup; c < c0; ++c) {
    if (MATCHES)
      o += batch_hex_keep(b, c, p.sorted_keys[c]) ? 1u : 0u;
    else
      o += hex_items(p.keys[c], p.n_strings, b.h.sets[c]);
  }
  (MATCHES ? b.match_off : b.item_off)[k] = o;
}

// ---- The wave-wide path of the hex class (matches.h HexWideParams) ----

// hex_measure_kernel's twin with the queue: a record that hex_run gives up on
// for WIDTH (kHexWide) is a rest record here, as it is there, and its index is
// appended to the queue -- one ballot and one atomic add per wave, then
// lane-wise stores.  (A twin: hex_measure_kernel stays what it is.)
__global__ __launch_bounds__(256) void hex_measure_queue_kernel(HexWideParams w) {
  __shared__ __attribute__((aligned(16))) uint8_t codebuf[256 * kHexCodeBytes + 16];
  const HexMatchParams& q = w.h;
  const MatchParams& p = q.m;
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool wide = false;
  if (r < p.n) {
    const VerifyRec rec = p.recs[r];
    const DevPoolRec e = p.pool[rec.pool_index];
    MatchMeasure m;
    HexSet set{1ull, 0u, 0u};
    bool is_match;
    if ((q.classes & kMatchHex) && string_is_final_hex(e.flags)) {
      m.length = 0;
      m.xor_key = 0;
      const uint32_t buf = (uint32_t)(uintptr_t)(codebuf + threadIdx.x * kHexCodeBytes);
      const int v = measure_hex<true>(q, e, rec.offset, buf, m, set);
      is_match = v == kHexMatch;
      wide = v == kHexWide;
      if (!is_match) set = HexSet{1ull, 0u, 0u};
    } else {
      is_match = measure(p, e, rec.offset, m);
    }
    const uint32_t string = is_match ? p.pool_string[rec.pool_index] : p.n_strings;
    p.keys[r] = (uint64_t)string << 32 | (rec.offset & 0xFFFFFFFFull);
    p.meas[r] = m;
    q.sets[r] = set;
    w.icount[r] = is_match ? (uint32_t)__popcll(set.mask) : 0u;
  }
  const uint64_t qmask = __ballot(wide);
  if (qmask != 0) {   // (wave-uniform)
    uint32_t at = 0;
    if ((threadIdx.x & 63u) == 0) at = atomicAdd(w.qlen, (uint32_t)__popcll(qmask));
    at = (uint32_t)__shfl((int)at, 0, 64) + lanes_below(qmask);
    if (wide && at < w.qcap) w.queue[at] = (uint32_t)r;
  }
  // (the per-wave counts are hex_wide_recount_kernel's: they include the wide results)
}

__global__ void hex_wide_clear_kernel(HexWideParams w) { *w.qlen = 0; }

constexpr uint32_t kWideSlice = 4096 + 16;   // a wave's input bytes: a run's reach + the alignment head
constexpr uint32_t kWideCode = 512;          // a wave's staged program
constexpr int kWideTop = 4096;               // the bytes_matched value of the set's 65th word

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
  return (uint64_t)hi << 32 | lo;
}

// The 4096-bit set << d: w'[l] = w[l - d / 64] << (d % 64) | w[l - d / 64 - 1]
// >> (64 - d % 64).  Every lane of the wave calls it.
__device__ __forceinline__ uint64_t wide_shl(uint64_t w, uint32_t d) {
  const int lane = (int)(threadIdx.x & 63u);
  const int q = (int)(d >> 6), s = (int)(d & 63u);
  if (q >= 64) return 0;
  const uint64_t a = shfl64(w, (lane - q) & 63), b = shfl64(w, (lane - q - 1) & 63);
  const uint64_t hi = lane >= q ? a : 0ull, lo = lane >= q + 1 ? b : 0ull;
  return s == 0 ? hi : (hi << s | lo >> (64 - s));
}

// The bits of w below position maxb (lane l holds the positions [64 l, 64 l + 64)).
__device__ __forceinline__ uint64_t wide_live(uint64_t w, int maxb) {
  const int lim = maxb - 64 * (int)(threadIdx.x & 63u);
  return lim >= 64 ? w : (lim <= 0 ? 0ull : w & ((1ull << lim) - 1));
}

// One run's input in the wave's LDS slice: byte j of the slice is input byte b
// = j - head, forwards the memory from the 16-byte boundary at or below the
// record's offset on, backwards the memory below the boundary at or above it,
// REVERSED -- so both directions read alike.  Staged 1 KiB a pass (lane l the
// 16 bytes at (64 i + l) 16, one aligned load where all 16 lie in [lo, hi), the
// bytes that do one by one otherwise), and only the passes that hold a live
// position.
struct WideInput {
  uint8_t* slice;         // LDS
  const uint8_t* org;     // the boundary
  const uint8_t* lo;      // what may be loaded: [lo, hi)
  const uint8_t* hi;
  uint32_t head;          // input byte 0 in the slice
  uint32_t chunks;        // 16-byte chunks that hold a byte below max_bytes_matched
  uint32_t staged;        // chunks staged (a multiple of 64)
  bool backwards;

  __device__ void open(uint8_t* lds, const uint8_t* input, int maxb, bool back, const uint8_t* l,
                       const uint8_t* h) {
    slice = lds;
    backwards = back;
    lo = l;
    hi = h;
    const uintptr_t a = (uintptr_t)input;
    const uintptr_t o = back ? (a + 15) & ~(uintptr_t)15 : a & ~(uintptr_t)15;
    org = (const uint8_t*)o;
    head = (uint32_t)(back ? o - a : a - o);
    chunks = (head + (uint32_t)maxb + 15) / 16;
    staged = 0;
  }

  // Input bytes [0, need) are in the slice afterwards (need <= max_bytes_matched).
  __device__ void ensure(uint32_t need) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const uint32_t want = (head + need + 15) / 16;
    if (staged >= want) return;
    while (staged < want) {
      const uint32_t c = staged + (threadIdx.x & 63u);
      if (c < chunks) {
        const uint8_t* g = backwards ? org - 16 * (uintptr_t)(c + 1) : org + 16 * (uintptr_t)c;
        u32x4 v;
        if (g >= lo && g + 16 <= hi) {
          const u32x4 m = *reinterpret_cast<const u32x4*>(g);
          if (backwards) {
            v.x = __builtin_bswap32(m.w);
            v.y = __builtin_bswap32(m.z);
            v.z = __builtin_bswap32(m.y);
            v.w = __builtin_bswap32(m.x);
          } else {
            v = m;
          }
        } else {
          uint32_t d[4] = {0, 0, 0, 0};
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const uint8_t* a = backwards ? g + 15 - j : g + j;
            const uint32_t byte = (a >= lo && a < hi) ? *a : 0u;
            d[j / 4] |= byte << (8 * (j % 4));
          }
          v.x = d[0];
          v.y = d[1];
          v.z = d[2];
          v.w = d[3];
        }
        *reinterpret_cast<u32x4*>(slice + 16 * c) = v;
      }
      staged += 64;
    }
    // (one wave writes and reads the slice: LDS serves a wave's requests in order)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }

  // Bit i: this lane's i-th input byte c passes ((c & mask) == val) != neg.
  // SWAR over 16 dwords: the exact zero-byte flags of (x & mask4) ^ val4.
  __device__ uint64_t pass(uint32_t mask, uint32_t val, bool neg) const {
    const uint32_t at = head + 64 * (threadIdx.x & 63u);
    const uint32_t* dw = reinterpret_cast<const uint32_t*>(slice) + (at >> 2);
    const uint32_t sh = at & 3u, mask4 = mask * 0x01010101u, val4 = val * 0x01010101u;
    uint64_t out = 0;
    uint32_t prev = dw[0];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t next = dw[i + 1];
      const uint32_t x = __builtin_amdgcn_alignbyte(next, prev, sh);
      prev = next;
      const uint32_t t = (x & mask4) ^ val4;
      // 0x80 in every byte of t that is zero, no borrow between bytes
      uint32_t z = ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);
      // the four flags (bits 7, 15, 23, 31) side by side
      uint32_t f = (((z >> 7) * 0x00204081u) >> 21) & 0xFu;
      if (neg) f ^= 0xFu;
      out |= (uint64_t)f << (4 * i);
    }
    return out;
  }
};

// hex_run's rule on the whole domain (matches.h): w = this lane's word of the
// set at MATCH, top = the value YR_RE_SCAN_LIMIT is in it.  Wave-uniform
// control flow: every lane runs every step.  A consuming opcode is S' = ((S n
// live) n pass) << 1, the carry of a word from the lane below; REPEAT_ANY {mn,
// mx} is S' = OR_d (S n live) << d over d = mn .. mx, smeared by doubling, cut
// to the positions below max_bytes_matched (re.c:2314; the b + mn copy at or
// past it dies at the next opcode, which is not MATCH).
// *ordered: forwards the reference returns the first element of its LIST to
// reach MATCH (re.c:2392-2400), and the list ascends only while one live
// position builds it: with live positions a < b, a's new positions are placed
// by comparison with b's pointer BEFORE b advances by mn (re.c:2302-2365), so
// b + mn can stand in front of smaller values.  A forward REPEAT_ANY with mx >
// mn on more than one live position leaves the order to the host: undecided.
template <class Code>
__device__ int hex_wide_run(const Code code, uint32_t len, WideInput& in, int maxb, bool backwards,
                            uint64_t& w, bool& top) {
  const uint32_t lane = threadIdx.x & 63u;
  w = lane == 0 ? 1ull : 0ull;
  top = false;
  uint32_t ip = 0;
  while (ip < len) {
    const uint32_t op = uniform(code[ip]), b1 = uniform(code[ip + 1]), b2 = uniform(code[ip + 2]);
    if (op == kReMatch) return kHexMatch;   // (not empty: every transition returns on an empty set)
    const uint64_t live = wide_live(w, maxb);   // (top: 4096 >= max_bytes_matched, dead)
    const uint64_t busy = __ballot(live != 0);
    if (busy == 0) return kHexNone;
    if (op == kReRepeatAnyUngreedy) {
      const uint32_t mn = b1 | (b2 << 8);
      const uint32_t mx = uniform(code[ip + 3]) | (uniform(code[ip + 4]) << 8);
      if (mx < mn || uniform(code[ip + 5]) == kReMatch) return kHexUndecided;
      if (!backwards && mx > mn) {
        const uint32_t n = wave_prefix((uint32_t)__popcll(live));
        if ((uint32_t)__shfl((int)n, 63, 64) != 1) return kHexUndecided;
      }
      uint64_t acc = wide_shl(live, mn);
      const uint32_t r = mx - mn + 1;   // copies
      uint32_t have = 1;
      while (2 * have <= r) {
        acc |= wide_shl(acc, have);
        have *= 2;
      }
      if (have < r) acc |= wide_shl(acc, r - have);
      w = wide_live(acc, maxb);
      top = false;
      if (__ballot(w != 0) == 0) return kHexNone;
      ip += 5;
      continue;
    }
    uint32_t mask, val, sz;
    bool neg = false;
    switch (op) {
      case kReAny: mask = 0; val = 0; sz = 1; break;
      case kReLiteral: mask = 0xFF; val = b1; sz = 2; break;
      case kReNotLiteral: mask = 0xFF; val = b1; sz = 2; neg = true; break;
      case kReMaskedLiteral: mask = b2; val = b1; sz = 3; break;
      case kReMaskedNotLiteral: mask = b2; val = b1; sz = 3; neg = true; break;
      default: return kHexUndecided;
    }
    // the bytes of the highest live word's lane and below, none at or past maxb
    const uint32_t top_lane = 63u - (uint32_t)__builtin_clzll(busy);
    in.ensure(min((uint32_t)maxb, 64u * (top_lane + 1)));
    uint64_t res = 0;
    if (live != 0) res = live & in.pass(mask, val, neg);   // (a lane with nothing live skips)
    const uint32_t out = (uint32_t)(res >> 63);
    const uint32_t carry = (uint32_t)__shfl_up((int)out, 1, 64);
    top = __shfl((int)out, 63, 64) != 0;
    w = res << 1 | (lane == 0 ? 0u : carry);
    if (__ballot(w != 0) == 0 && !top) return kHexNone;
    ip += sz;
  }
  return kHexUndecided;
}

// One program of a wave's record into the wave's LDS when it fits (with the
// operand bytes a read may reach past MATCH: the blob carries 64 bytes of padding).
__device__ __forceinline__ bool wide_stage_code(const uint8_t* code, uint32_t len, uint8_t* buf) {
  if (len + 8 > kWideCode) return false;
  for (uint32_t i = threadIdx.x & 63u; i < len + 8; i += 64) buf[i] = code[i];
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  return true;
}

__device__ int hex_wide_program(const uint8_t* code, uint32_t len, uint8_t* codebuf, WideInput& in,
                                int maxb, bool backwards, uint64_t& w, bool& top) {
  if (wide_stage_code(code, len, codebuf))
    return hex_wide_run(LdsCode{(uint32_t)(uintptr_t)codebuf}, len, in, maxb, backwards, w, top);
  return hex_wide_run(GlobalCode{code}, len, in, maxb, backwards, w, top);
}

// One queued record, measured by the calling WAVE in the block [data, data +
// size), loads bounded by [lo, hi).  hex_call's two runs: F = the lowest
// position of the forward set, the backward set to wsets.  A match overwrites
// what the queue kernel left of the record: its key (the string in place of
// n_strings), F, the item count, and the set's mark (mask 0, pad 1).  Anything
// else leaves the record in the rest.
__device__ __forceinline__ void hex_wide_record(const HexWideParams& q, uint32_t r, uint32_t slot,
                                                const uint8_t* data, uint64_t size,
                                                const uint8_t* lo, const uint8_t* hi, uint8_t* slice,
                                                uint8_t* codebuf) {
  const MatchParams& p = q.h.m;
  const uint32_t lane = threadIdx.x & 63u;
  const VerifyRec rec = p.recs[r];
  const DevRe re = p.pool[rec.pool_index].re;
  const uint64_t offset = rec.offset;
  const uint8_t* d = data + offset;
  WideInput in;
  uint64_t w;
  bool top;
  int maxb = (int)min<uint64_t>(size - offset, (uint64_t)kReScanLimit);
  in.open(slice, d, maxb, false, lo, hi);
  int v = hex_wide_program(q.h.re_code + re.fwd_off, re.fwd_len, codebuf, in, maxb, false, w, top);
  if (v != kHexMatch) return;
  const uint64_t ends = __ballot(w != 0);
  uint32_t F = kWideTop;   // (top alone)
  if (ends != 0) {
    const int first = __builtin_ctzll(ends);
    F = 64u * first + (uint32_t)__builtin_ctzll(shfl64(w, first) | 1ull << 63);
  }
  uint32_t items = 1;
  w = lane == 0 ? 1ull : 0ull;   // (no backward program: {0})
  top = false;
  if (re.bwd_len == 0) {
    if (F == 0) return;
  } else {
    maxb = (int)min<uint64_t>(offset, (uint64_t)kReScanLimit);
    in.open(slice, d, maxb, true, lo, hi);
    v = hex_wide_program(q.h.re_code + re.bwd_off, re.bwd_len, codebuf, in, maxb, true, w, top);
    if (v != kHexMatch) return;
    items = (uint32_t)__shfl((int)wave_prefix((uint32_t)__popcll(w)), 63, 64) + (top ? 1u : 0u);
  }
  uint64_t* ws = q.wsets + (uint64_t)slot * kWideWords;
  ws[lane] = w;
  if (lane == 0) {
    ws[kWideWords - 1] = top ? 1ull : 0ull;
    p.keys[r] = (uint64_t)p.pool_string[rec.pool_index] << 32 | (offset & 0xFFFFFFFFull);
    p.meas[r] = MatchMeasure{F, 0u};
    q.h.sets[r] = HexSet{0ull, 0u, 1u};
    q.icount[r] = items;
  }
}

// One WAVE per queued record, the waves of a fixed grid striding over the
// queue.  measure_hex's window test lies behind the record already; [win_lo,
// win_hi) bounds every load.
__global__ __launch_bounds__(256) void hex_wide_measure_kernel(HexWideParams q) {
  __shared__ __attribute__((aligned(16))) uint8_t slices[4][kWideSlice];
  __shared__ __attribute__((aligned(16))) uint8_t codes[4][kWideCode];
  const MatchParams& p = q.h.m;
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t n = min(*q.qlen, q.qcap);
  const uint8_t* lo = p.data + p.win_lo;
  const uint8_t* hi = p.data + p.win_hi;
  for (uint32_t slot = blockIdx.x * 4 + wave; slot < n; slot += gridDim.x * 4)
    hex_wide_record(q, q.queue[slot], slot, p.data, p.size, lo, hi, slices[wave], codes[wave]);
}

// The per-wave counts of hex_measure_kernel, from the per-record arrays once
// the wide records are in them, + each record's items' start within its wave.
__global__ __launch_bounds__(256) void hex_wide_recount_kernel(HexWideParams w) {
  const MatchParams& p = w.h.m;
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r == 0) *w.qlen_out = *w.qlen;
  bool rest = false;
  uint32_t items = 0;
  if (r < p.n) {
    rest = (uint32_t)(p.keys[r] >> 32) == p.n_strings;
    items = rest ? 0u : w.icount[r];
  }
  const uint64_t mask = __ballot(rest);
  const uint32_t incl = wave_prefix(items);
  const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
  if (r < p.n) w.istart[r] = incl - items;
  if ((threadIdx.x & 63u) == 0 && r < p.n) {
    p.block_off[r / kGroup] = (uint64_t)__popcll(mask);
    w.h.iblock_off[r / kGroup] = (uint64_t)total;
  }
}

// hex_expand_kernel's twin: the start within the wave from istart (the lanes
// below may be wide records); a wide match has mask 0, no item here.
__global__ __launch_bounds__(256) void hex_expand_at_kernel(HexWideParams w) {
  const HexMatchParams& q = w.h;
  const MatchParams& p = q.m;
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.n) return;
  const uint64_t key = p.keys[r];
  const HexSet set = q.sets[r];
  if (hex_items(key, p.n_strings, set) == 0) return;
  const uint64_t g = r / kGroup;
  uint64_t at = q.ichunk_off[g / kChunkGroups] + q.iblock_off[g] + w.istart[r];
  const uint64_t offset = key & 0xFFFFFFFFull;
  for (uint64_t x = set.mask; x != 0 && at < q.n_items; x &= x - 1, ++at) {
    const uint32_t B = set.base + (uint32_t)__builtin_ctzll(x);
    q.ikeys[at] = (key & 0xFFFFFFFF00000000ull) | (offset - B);
    q.iindex[at] = (uint32_t)r;
  }
}

// One wave per wide record: lane l expands word l at the record's start plus
// the bits of the lanes below; the value YR_RE_SCAN_LIMIT comes last.
__global__ __launch_bounds__(256) void hex_wide_expand_kernel(HexWideParams w) {
  const HexMatchParams& q = w.h;
  const MatchParams& p = q.m;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t n = min(*w.qlen, w.qcap);
  for (uint32_t slot = blockIdx.x * 4 + (threadIdx.x >> 6); slot < n; slot += gridDim.x * 4) {
    const uint32_t r = w.queue[slot];
    if (q.sets[r].pad != 1u) continue;   // (not measured a match: a rest record)
    const uint64_t key = p.keys[r];
    const uint64_t* ws = w.wsets + (uint64_t)slot * kWideWords;
    const uint64_t word = ws[lane];
    const uint32_t bits = (uint32_t)__popcll(word);
    const uint32_t incl = wave_prefix(bits);
    const uint64_t g = r / kGroup;
    const uint64_t start = q.ichunk_off[g / kChunkGroups] + q.iblock_off[g] + w.istart[r];
    const uint64_t offset = key & 0xFFFFFFFFull;   // (B <= min(offset, YR_RE_SCAN_LIMIT))
    uint64_t at = start + incl - bits;
    for (uint64_t x = word; x != 0 && at < q.n_items; x &= x - 1, ++at) {
      const uint32_t B = 64u * lane + (uint32_t)__builtin_ctzll(x);
      q.ikeys[at] = (key & 0xFFFFFFFF00000000ull) | (offset - B);
      q.iindex[at] = r;
    }
    if (lane == 63 && ws[kWideWords - 1] != 0 && start + incl < q.n_items) {
      q.ikeys[start + incl] = (key & 0xFFFFFFFF00000000ull) | (offset - (uint64_t)kWideTop);
      q.iindex[start + incl] = r;
    }
  }
}

// ---- The batch's wave-wide path (matches.h BatchHexWideParams) ----

// batch_hex_measure_kernel's twin with the queue (as hex_measure_queue_kernel
// is hex_measure_kernel's): the record's buffer is the whole block of both
// runs, a record given up on for width is appended with its buffer -- the
// binary search over rec_off is done once, here.
__global__ __launch_bounds__(256) void batch_hex_measure_queue_kernel(BatchHexWideParams b) {
  __shared__ __attribute__((aligned(16))) uint8_t codebuf[256 * kHexCodeBytes + 16];
  const HexWideParams& w = b.w;
  const MatchParams& p = w.h.m;
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool wide = false;
  uint32_t lo = 0;
  if (r < p.n) {
    uint32_t hi = b.nbuf;   // rec_off[lo] <= r < rec_off[hi]  (rec_off[nbuf] == n)
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (b.rec_off[mid] <= r) lo = mid; else hi = mid;
    }
    HexMatchParams q = w.h;
    q.m.data = p.data + b.starts[lo];
    q.m.size = b.sizes[lo];
    q.m.win_lo = 0;
    q.m.win_hi = q.m.size;
    const VerifyRec rec = p.recs[r];
    const DevPoolRec e = p.pool[rec.pool_index];
    MatchMeasure m;
    HexSet set{1ull, 0u, 0u};
    bool is_match;
    if ((q.classes & kMatchHex) && string_is_final_hex(e.flags)) {
      m.length = 0;
      m.xor_key = 0;
      const uint32_t buf = (uint32_t)(uintptr_t)(codebuf + threadIdx.x * kHexCodeBytes);
      const int v = measure_hex<true>(q, e, rec.offset, buf, m, set);
      is_match = v == kHexMatch;
      wide = v == kHexWide;
      if (!is_match) set = HexSet{1ull, 0u, 0u};
    } else {
      is_match = measure(q.m, e, rec.offset, m);
    }
    const uint32_t string = is_match ? p.pool_string[rec.pool_index] : p.n_strings;
    p.keys[r] = (uint64_t)string << 32 | (rec.offset & 0xFFFFFFFFull);
    p.meas[r] = m;
    w.h.sets[r] = set;
    b.buf[r] = lo;
    w.icount[r] = is_match ? (uint32_t)__popcll(set.mask) : 0u;
  }
  const uint64_t qmask = __ballot(wide);
  if (qmask != 0) {   // (wave-uniform)
    uint32_t at = 0;
    if ((threadIdx.x & 63u) == 0) at = atomicAdd(w.qlen, (uint32_t)__popcll(qmask));
    at = (uint32_t)__shfl((int)at, 0, 64) + lanes_below(qmask);
    if (wide && at < w.qcap) {
      w.queue[at] = (uint32_t)r;
      b.qbuf[at] = lo;
    }
  }
  // (the per-wave counts are hex_wide_recount_kernel's: they include the wide results)
}

// hex_wide_measure_kernel for a batch: one WAVE per queued record, a fixed grid
// striding over the queue.  The wave's record and buffer come from the queue
// entry, the buffer's bounds from starts / sizes through scalar registers (one
// value for the wave); both runs see the buffer as the whole block -- position
// 0 at arena + starts[k], max_bytes_matched = min(size_k - local offset, 4096)
// forwards and min(local offset, 4096) backwards -- and WideInput loads only
// from [start, start + size): a 16-byte chunk wholly inside in one aligned load
// (buffer starts are 16-byte aligned in the arena, their ends are not), the
// bytes of any other chunk that lie inside one by one, no byte of a gap or of a
// neighbouring buffer.  The record itself is measured by hex_wide_record.
__global__ __launch_bounds__(256) void batch_hex_wide_measure_kernel(BatchHexWideParams b) {
  __shared__ __attribute__((aligned(16))) uint8_t slices[4][kWideSlice];
  __shared__ __attribute__((aligned(16))) uint8_t codes[4][kWideCode];
  const HexWideParams& q = b.w;
  const MatchParams& p = q.h.m;
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t n = min(*q.qlen, q.qcap);
  for (uint32_t slot = uniform(blockIdx.x * 4 + wave); slot < n; slot += gridDim.x * 4) {
    const uint32_t r = uniform(q.queue[slot]), k = uniform(b.qbuf[slot]);
    if (r >= p.n || k >= b.nbuf) continue;   // (never: what the measure pass appended)
    const uint8_t* lo = p.data + b.starts[k];
    const uint64_t size = b.sizes[k];
    if (p.recs[r].offset >= size) continue;   // (never: measure_hex queues no such record)
    hex_wide_record(q, r, slot, lo, size, lo, lo + size, slices[wave], codes[wave]);
  }
}

// The CSR offsets over items, one lane per k in [0, nbuf], without a loop:
// item_off[k] = the items of the records below c0 = rec_off[k] = the scanned
// item count of c0's wave plus, where c0 is not the wave's first record, what
// the recount left of the record before it: its items' start within the wave
// and its item count.  (g == groups: the entry past the last wave, the total.)
__global__ __launch_bounds__(256) void batch_hex_wide_offsets_kernel(BatchHexWideParams b) {
  const HexWideParams& w = b.w;
  const MatchParams& p = w.h.m;
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > b.nbuf) return;
  const uint64_t c0 = b.rec_off[k], g = c0 / kGroup;
  uint64_t o = w.h.ichunk_off[g / kChunkGroups] + w.h.iblock_off[g];
  if (c0 % kGroup != 0) {   // (c0 - 1 is a record of the same wave)
    const uint64_t c = c0 - 1;
    o += w.istart[c] + ((uint32_t)(p.keys[c] >> 32) == p.n_strings ? 0u : w.icount[c]);
  }
  b.item_off[k] = o;
}

}  // namespace

hipError_t launch_match_classify(const MatchParams& p, hipStream_t s) {
  if (p.n == 0 || p.n > kMatchMaxRecords) return p.n == 0 ? hipSuccess : hipErrorInvalidValue;
  hipLaunchKernelGGL(match_classify_kernel, match_grid(p.n), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_match_rest(const MatchParams& p, hipStream_t s) {
  if (p.n == 0 || p.n > kMatchMaxRecords) return p.n == 0 ? hipSuccess : hipErrorInvalidValue;
  hipLaunchKernelGGL(match_rest_kernel, match_grid(p.n), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t match_sort(uint64_t* const keys[2], uint32_t* const index[2], uint64_t n, int lo_bits,
                      int hi_bits, uint64_t* hist, uint64_t* chunk, uint64_t* total, hipStream_t s,
                      int* result) {
  *result = 0;
  if (n > kMatchMaxRecords) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const KeptLists none{{0, 0, 0, 0}};
  int src = 0;
  for (int field = 0; field < 2; ++field) {
    const int first = field == 0 ? 0 : 32, last = first + (field == 0 ? lo_bits : hi_bits);
    for (int shift = first; shift < last; shift += 8) {
      SortPass p;
      p.kin = keys[src];
      p.kout = keys[src ^ 1];
      p.vin = index[src];
      p.vout = index[src ^ 1];
      p.n = n;
      p.tiles = match_sort_tiles(n);
      p.shift = (uint32_t)shift;
      p.mask = (1u << std::min(8, last - shift)) - 1u;
      p.hist = hist;
      p.chunk = chunk;
      const uint64_t entries = (uint64_t)(p.mask + 1) * p.tiles;
      hipLaunchKernelGGL(sort_hist_kernel, dim3((uint32_t)p.tiles), dim3(64), 0, s, p);
      // (the offset kernels count in groups of kGroup candidates: one entry each)
      const hipError_t e = launch_block_offsets(hist, chunk, entries * kGroup, total, nullptr, none, s);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(sort_scatter_kernel, dim3((uint32_t)p.tiles), dim3(64), 0, s, p);
      src ^= 1;
    }
  }
  *result = src;
  return hipGetLastError();
}

hipError_t launch_match_unique(const MatchParams& p, int pass, hipStream_t s) {
  if (p.n == 0 || p.n > kMatchMaxRecords) return p.n == 0 ? hipSuccess : hipErrorInvalidValue;
  if (pass == 0)
    hipLaunchKernelGGL(match_unique_kernel<0>, match_grid(p.n), dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(match_unique_kernel<1>, match_grid(p.n), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_hex_measure(const HexMatchParams& p, hipStream_t s) {
  if (p.m.n == 0 || p.m.n > kMatchMaxRecords) return p.m.n == 0 ? hipSuccess : hipErrorInvalidValue;
  hipLaunchKernelGGL(hex_measure_kernel, match_grid(p.m.n), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_hex_expand(const HexMatchParams& p, hipStream_t s) {
  if (p.m.n == 0 || p.n_items == 0) return hipSuccess;
  if (p.m.n > kMatchMaxRecords || p.n_items > kMatchMaxRecords) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hex_expand_kernel, match_grid(p.m.n), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_hex_unique(const HexMatchParams& p, int pass, hipStream_t s) {
  if (p.n_items == 0 || p.n_items > kMatchMaxRecords)
    return p.n_items == 0 ? hipSuccess : hipErrorInvalidValue;
  if (pass == 0)
    hipLaunchKernelGGL(hex_unique_kernel<0>, match_grid(p.n_items), dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(hex_unique_kernel<1>, match_grid(p.n_items), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_hex_wide_measure(const HexWideParams& w, uint32_t waves, hipStream_t s) {
  const uint64_t n = w.h.m.n;
  if (n == 0 || n > kMatchMaxRecords) return n == 0 ? hipSuccess : hipErrorInvalidValue;
  if (waves == 0 || w.qcap == 0) return hipErrorInvalidValue;
  // (a kernel, not a memset: the stage may be recorded into a graph)
  hipLaunchKernelGGL(hex_wide_clear_kernel, dim3(1), dim3(1), 0, s, w);
  hipLaunchKernelGGL(hex_measure_queue_kernel, match_grid(n), dim3(256), 0, s, w);
  hipLaunchKernelGGL(hex_wide_measure_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, w);
  hipLaunchKernelGGL(hex_wide_recount_kernel, match_grid(n), dim3(256), 0, s, w);
  return hipGetLastError();
}

hipError_t launch_hex_wide_piece(const HexWideParams& w, uint32_t waves, int piece, hipStream_t s) {
  const uint64_t n = w.h.m.n;
  if (n == 0 || n > kMatchMaxRecords) return n == 0 ? hipSuccess : hipErrorInvalidValue;
  if (waves == 0 || w.qcap == 0 || piece < 0 || piece > 2) return hipErrorInvalidValue;
  if (piece == 0)
    hipLaunchKernelGGL(hex_wide_clear_kernel, dim3(1), dim3(1), 0, s, w);
  else if (piece == 1)
    hipLaunchKernelGGL(hex_wide_measure_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, w);
  else
    hipLaunchKernelGGL(hex_wide_recount_kernel, match_grid(n), dim3(256), 0, s, w);
  return hipGetLastError();
}

hipError_t launch_hex_wide_expand(const HexWideParams& w, uint32_t waves, hipStream_t s) {
  const HexMatchParams& p = w.h;
  if (p.m.n == 0 || p.n_items == 0) return hipSuccess;
  if (p.m.n > kMatchMaxRecords || p.n_items > kMatchMaxRecords || waves == 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(hex_expand_at_kernel, match_grid(p.m.n), dim3(256), 0, s, w);
  hipLaunchKernelGGL(hex_wide_expand_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, w);
  return hipGetLastError();
}

hipError_t launch_batch_hex_wide_measure(const BatchHexWideParams& p, uint32_t waves, hipStream_t s) {
  const uint64_t n = p.w.h.m.n;
  if (n == 0 || n > kMatchMaxRecords) return n == 0 ? hipSuccess : hipErrorInvalidValue;
  if (waves == 0 || p.w.qcap == 0 || p.nbuf == 0) return hipErrorInvalidValue;
  // (a kernel, not a memset: the stage may be recorded into a graph)
  hipLaunchKernelGGL(hex_wide_clear_kernel, dim3(1), dim3(1), 0, s, p.w);
  hipLaunchKernelGGL(batch_hex_measure_queue_kernel, match_grid(n), dim3(256), 0, s, p);
  hipLaunchKernelGGL(batch_hex_wide_measure_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, p);
  hipLaunchKernelGGL(hex_wide_recount_kernel, match_grid(n), dim3(256), 0, s, p.w);
  return hipGetLastError();
}

hipError_t launch_batch_hex_wide_waves(const BatchHexWideParams& p, uint32_t waves, hipStream_t s) {
  const uint64_t n = p.w.h.m.n;
  if (n == 0 || n > kMatchMaxRecords) return n == 0 ? hipSuccess : hipErrorInvalidValue;
  if (waves == 0 || p.w.qcap == 0 || p.nbuf == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(batch_hex_wide_measure_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_batch_hex_wide_offsets(const BatchHexWideParams& p, hipStream_t s) {
  const uint64_t n = p.w.h.m.n;
  if (n == 0 || n > kMatchMaxRecords) return n == 0 ? hipSuccess : hipErrorInvalidValue;
  hipLaunchKernelGGL(batch_hex_wide_offsets_kernel, match_grid((uint64_t)p.nbuf + 1), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_batch_match_classify(const BatchMatchParams& p, hipStream_t s) {
  if (p.m.n == 0 || p.m.n > kMatchMaxRecords || p.nbuf == 0)
    return p.m.n == 0 ? hipSuccess : hipErrorInvalidValue;
  hipLaunchKernelGGL(batch_match_classify_kernel, match_grid(p.m.n), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_batch_match_offsets(const BatchMatchParams& p, int matches, hipStream_t s) {
  if (p.m.n == 0 || p.m.n > kMatchMaxRecords) return p.m.n == 0 ? hipSuccess : hipErrorInvalidValue;
  const dim3 grid = match_grid((uint64_t)p.nbuf + 1);
  if (matches)
    hipLaunchKernelGGL(batch_match_offsets_kernel<1>, grid, dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(batch_match_offsets_kernel<0>, grid, dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t batch_match_sort(uint64_t* const keys[2], uint32_t* const index[2], uint64_t n,
                            int lo_bits, int hi_bits, const uint32_t* buf, uint32_t nbuf,
                            uint64_t* hist, uint64_t* chunk, uint64_t* total, hipStream_t s,
                            int* result) {
  hipError_t e = match_sort(keys, index, n, lo_bits, hi_bits, hist, chunk, total, s, result);
  if (e != hipSuccess || n == 0 || nbuf < 2) return e;
  int bits = 1;   // the bits of nbuf - 1
  while (bits < 32 && ((nbuf - 1) >> bits) != 0) ++bits;
  const KeptLists none{{0, 0, 0, 0}};
  int src = *result;
  for (int shift = 0; shift < bits; shift += 8) {
    SortPassBuf p;
    p.s.kin = keys[src];
    p.s.kout = keys[src ^ 1];
    p.s.vin = index[src];
    p.s.vout = index[src ^ 1];
    p.s.n = n;
    p.s.tiles = match_sort_tiles(n);
    p.s.shift = (uint32_t)shift;
    p.s.mask = (1u << std::min(8, bits - shift)) - 1u;
    p.s.hist = hist;
    p.s.chunk = chunk;
    p.buf = buf;
    const uint64_t entries = (uint64_t)(p.s.mask + 1) * p.s.tiles;
    hipLaunchKernelGGL(sort_hist_buf_kernel, dim3((uint32_t)p.s.tiles), dim3(64), 0, s, p);
    e = launch_block_offsets(hist, chunk, entries * kGroup, total, nullptr, none, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sort_scatter_buf_kernel, dim3((uint32_t)p.s.tiles), dim3(64), 0, s, p);
    src ^= 1;
  }
  *result = src;
  return hipGetLastError();
}

hipError_t launch_batch_match_unique(const BatchMatchParams& p, int pass, hipStream_t s) {
  if (p.m.n == 0 || p.m.n > kMatchMaxRecords) return p.m.n == 0 ? hipSuccess : hipErrorInvalidValue;
  if (pass == 0)
    hipLaunchKernelGGL(batch_match_unique_kernel<0>, match_grid(p.m.n), dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(batch_match_unique_kernel<1>, match_grid(p.m.n), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_batch_hex_measure(const BatchHexParams& p, hipStream_t s) {
  if (p.h.m.n == 0 || p.h.m.n > kMatchMaxRecords || p.nbuf == 0)
    return p.h.m.n == 0 ? hipSuccess : hipErrorInvalidValue;
  hipLaunchKernelGGL(batch_hex_measure_kernel, match_grid(p.h.m.n), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_batch_hex_offsets(const BatchHexParams& p, int matches, hipStream_t s) {
  if (p.h.m.n == 0 || p.h.m.n > kMatchMaxRecords)
    return p.h.m.n == 0 ? hipSuccess : hipErrorInvalidValue;
  if (matches && (p.h.n_items == 0 || p.h.n_items > kMatchMaxRecords))
    return p.h.n_items == 0 ? hipSuccess : hipErrorInvalidValue;
  const dim3 grid = match_grid((uint64_t)p.nbuf + 1);
  if (matches)
    hipLaunchKernelGGL(batch_hex_offsets_kernel<1>, grid, dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(batch_hex_offsets_kernel<0>, grid, dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_batch_hex_unique(const BatchHexParams& p, int pass, hipStream_t s) {
  if (p.h.n_items == 0 || p.h.n_items > kMatchMaxRecords)
    return p.h.n_items == 0 ? hipSuccess : hipErrorInvalidValue;
  if (pass == 0)
    hipLaunchKernelGGL(batch_hex_unique_kernel<0>, match_grid(p.h.n_items), dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(batch_hex_unique_kernel<1>, match_grid(p.h.n_items), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace yamd
