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
// The comparisons are restated here rather than shared with verify.hip: that
// file's kernels stay byte for byte what they were (their register budgets are
// tuned), and these read global memory directly -- a
// record is one in thousands of positions, and every final record's bytes were
// just read by the pre-verification, so they sit in L2.
#include <algorithm>

#include "internal.h"
#include "matches.h"

namespace yamd {

namespace {

// _yr_scan_compare / _yr_scan_icompare (scan.c:142-179): the forward match
// length of the ascii form, 0 if none.  No byte is read unless all n are in
// the block (avail = size - offset).
__device__ uint32_t len_ascii(const uint8_t* __restrict__ d, uint64_t avail,
                              const uint8_t* __restrict__ s, uint32_t n,
                              const uint8_t* __restrict__ lower) {
  if (avail < n) return 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t a = d[i], b = s[i];
    if (lower == nullptr ? a != b : lower[a] != lower[b]) return 0;
  }
  return n;
}

// _yr_scan_wcompare / _yr_scan_wicompare (scan.c:181-255): every character
// followed by 0x00; 2 * n.
__device__ uint32_t len_wide(const uint8_t* __restrict__ d, uint64_t avail,
                             const uint8_t* __restrict__ s, uint32_t n,
                             const uint8_t* __restrict__ lower) {
  if (avail < 2ull * n) return 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t a = d[2 * i], b = s[i];
    if ((lower == nullptr ? a != b : lower[a] != lower[b]) || d[2 * i + 1] != 0) return 0;
  }
  return 2 * n;
}

// _yr_scan_xor_compare (scan.c:62-103) and _yr_scan_xor_wcompare (:105-140):
// key = data[0] ^ string[0], written only when the comparison succeeds.
__device__ uint32_t len_xor(const uint8_t* __restrict__ d, uint64_t avail,
                            const uint8_t* __restrict__ s, uint32_t n, bool wide, uint32_t& key) {
  if (avail < (wide ? 2ull * n : (uint64_t)n)) return 0;
  if (n == 0) return 0;   // both reference loops yield 0 for an empty string
  const uint8_t k = d[0] ^ s[0];
  for (uint32_t i = 0; i < n; ++i) {
    if (wide) {
      if (d[2 * i] != (uint8_t)(s[i] ^ k) || (uint8_t)(d[2 * i + 1] ^ k) != 0) return 0;
    } else if (d[i] != (uint8_t)(s[i] ^ k)) {
      return 0;
    }
  }
  key = k;
  return wide ? 2 * n : n;
}

// One record: is it a match, and then forward_matches and the xor key of
// _yr_scan_verify_literal_match (scan.c:907-972).
__device__ bool measure(const MatchParams& p, const DevPoolRec& e, uint64_t offset,
                        MatchMeasure& m) {
  m.length = 0;
  m.xor_key = 0;
  if (!string_is_final(e.flags) || offset >= p.size) return false;
  // scan.c:912-915, decided without reading data (as call_matters does, before
  // its window test)
  if ((e.flags & kStrFitsInAtom) && !(e.flags & kStrFullWord)) {
    m.length = e.backtrack;
    return m.length != 0;
  }
  // A window scan keeps a call whose bytes are not all in the window without
  // deciding it (verify.hip call_matters, the same bounds): not a match yet.
  if (p.win_lo != 0 || p.win_hi != p.size) {
    const uint64_t need_lo = offset - min<uint64_t>(offset, (uint64_t)kReScanLimit);
    const uint64_t need_hi =
        min<uint64_t>(p.size, offset + max<uint64_t>((uint64_t)kReScanLimit, 2ull * e.length + 2));
    if (need_lo < p.win_lo || need_hi > p.win_hi) return false;
  }
  if (e.flags & kStrFitsInAtom) {   // (FULL_WORD: the pre-verification tested the word)
    m.length = e.backtrack;
    return m.length != 0;
  }
  const uint8_t* d = p.data + offset;
  const uint64_t avail = p.size - offset;
  const uint8_t* s = p.str_bytes + e.bytes_off;
  const uint32_t n = e.length;
  const uint8_t* lower = (e.flags & kStrNoCase) ? p.lowercase : nullptr;
  uint32_t fm = 0;
  if (e.flags & kStrAscii) fm = len_ascii(d, avail, s, n, lower);
  if (fm == 0 && (e.flags & kStrWide)) fm = len_wide(d, avail, s, n, lower);
  if (fm == 0 && !(e.flags & kStrNoCase) && (e.flags & kStrXor)) {
    if (e.flags & kStrWide) fm = len_xor(d, avail, s, n, true, m.xor_key);
    if (fm == 0) fm = len_xor(d, avail, s, n, false, m.xor_key);
  }
  m.length = fm;
  // Defensive: the pre-verification keeps a final string's call only where one
  // of these comparisons succeeds, so fm != 0 here.  Should that ever not hold,
  // the record goes to the rest -- the host verifies it and finds what there
  // is -- rather than out as a match of length 0.
  return fm != 0;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                   __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
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

}  // namespace yamd
