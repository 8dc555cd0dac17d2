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

// ---- The stage with the hex class (matches.h HexMatchParams) ----

// Regexp code from the blob in global memory or from this lane's LDS copy
// (verify.hip's two readers, restated).
struct GlobalCode {
  const uint8_t* __restrict__ p;
  __device__ uint8_t operator[](uint32_t i) const { return p[i]; }
};
struct LdsCode {
  uint32_t a;   // LDS byte address
  __device__ uint8_t operator[](uint32_t i) const {
    return *reinterpret_cast<const __attribute__((address_space(3))) uint8_t*>((uintptr_t)(a + i));
  }
};
constexpr uint32_t kHexCodeBytes = 48;   // LDS per lane: three aligned 16-byte loads
constexpr uint32_t kNoLds = 0xFFFFFFFFu;

// verify.hip stage_code: a program that fits goes into this lane's LDS with
// three independent loads (the blob carries 64 bytes of padding).
__device__ __forceinline__ uint32_t hex_stage_code(const uint8_t* code, uint32_t len, uint32_t buf) {
  const uintptr_t a = (uintptr_t)code, lo = a & ~(uintptr_t)15;
  const uint32_t head = (uint32_t)(a - lo);
  if (head + len > kHexCodeBytes) return kNoLds;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const u32x4* g = reinterpret_cast<const u32x4*>(lo);
  const u32x4 c0 = g[0], c1 = g[1], c2 = g[2];
  typedef __attribute__((address_space(3))) u32x4 lds_u4;
  lds_u4* d = reinterpret_cast<lds_u4*>((uintptr_t)buf);
  d[0] = c0;
  d[1] = c1;
  d[2] = c2;
  return buf + head;
}

constexpr int kHexNone = 0, kHexMatch = 1, kHexUndecided = 2;

// yr_re_fast_exec (re.c:2150-2423) in position-set form, verify.hip
// fast_re_set's transitions, but with the set at RE_OPCODE_MATCH as the
// result: bit i of out.mask = bytes_matched value out.base + i.  Byte b of the
// input is input[b], backwards input[-1 - b]; only live positions (b < maxb)
// are read, so no byte outside the block.  kHexUndecided: the set would leave
// the 64-position window or come near YR_RE_SCAN_LIMIT, an opcode outside the
// fast set, a program that does not end in MATCH, or a REPEAT_ANY right
// before MATCH (whose b + min the reference does not bound).
template <class Code>
__device__ int hex_run(const Code code, uint32_t len, const uint8_t* __restrict__ input, int maxb,
                       bool backwards, HexSet& out) {
  int base = 0;
  uint64_t m = 1;
  uint32_t ip = 0;
  while (ip < len) {
    const uint8_t op = code[ip], b1 = code[ip + 1], b2 = code[ip + 2];
    if (op == kReMatch) {
      out.mask = m;
      out.base = (uint32_t)base;
      return kHexMatch;   // (m != 0: every transition below returns on an empty set)
    }
    const int lim = maxb - base;   // bits i < lim are live (b < max_bytes_matched)
    const uint64_t live = lim >= 64 ? m : (lim <= 0 ? 0ull : m & ((1ull << lim) - 1));
    if (live == 0) return kHexNone;
    if (op == kReRepeatAnyUngreedy) {
      const int mn = b1 | (b2 << 8);
      const int mx = code[ip + 3] | (code[ip + 4] << 8);
      if (mx < mn || code[ip + 5] == kReMatch) return kHexUndecided;
      const int lo = __builtin_ctzll(live), hi = 63 - __builtin_clzll(live);
      const int span = hi - lo + (mx - mn);
      const int nb = base + lo + mn;
      if (span > 63 || nb + span >= kReScanLimit) return kHexUndecided;
      // t | t << 1 | ... | t << (mx - mn), by doubling
      uint64_t acc = live >> lo;
      const int r = mx - mn + 1;   // copies
      int have = 1;
      while (2 * have <= r) {
        acc |= acc << have;
        have *= 2;
      }
      if (have < r) acc |= acc << (r - have);
      // (b + min at or past maxb dies at the next, consuming, opcode)
      const int lim2 = maxb - nb;
      acc &= lim2 >= 64 ? ~0ull : (lim2 <= 0 ? 0ull : (1ull << lim2) - 1);
      if (acc == 0) return kHexNone;
      m = acc;
      base = nb;
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
    uint64_t res = 0, x = live;
    while (x) {   // live positions only (never past the block)
      const int i = __builtin_ctzll(x);
      const int b = base + i;
      const uint8_t c = backwards ? input[-1 - b] : input[b];
      res |= (uint64_t)((((uint32_t)c & mask) == val) != neg) << i;
      x &= x - 1;
    }
    if (res == 0) return kHexNone;
    m = res;
    base += 1;
    ip += sz;
  }
  return kHexUndecided;
}

// _yr_scan_verify_re_match (scan.c:778-885) of a final hex string's record:
// kHexMatch with m.length = F, the forward program's smallest bytes_matched,
// and the backward program's set in `set` ({0} without one).
template <class Code>
__device__ int hex_call(const MatchParams& p, const DevRe& r, const Code fwd, const Code bwd,
                        uint64_t offset, MatchMeasure& m, HexSet& set) {
  const uint8_t* d = p.data + offset;
  HexSet f;
  int v = hex_run(fwd, r.fwd_len, d, (int)min<uint64_t>(p.size - offset, (uint64_t)kReScanLimit),
                  false, f);
  if (v != kHexMatch) return v;
  m.length = f.base + (uint32_t)__builtin_ctzll(f.mask);   // the first of the ascending list
  if (r.bwd_len == 0) return m.length != 0 ? kHexMatch : kHexNone;
  return hex_run(bwd, r.bwd_len, d, (int)min<uint64_t>(offset, (uint64_t)kReScanLimit), true, set);
}

__device__ int measure_hex(const HexMatchParams& q, const DevPoolRec& e, uint64_t offset,
                           uint32_t codebuf, MatchMeasure& m, HexSet& set) {
  const MatchParams& p = q.m;
  if (offset >= p.size) return kHexNone;
  // (measure()'s bounds: every byte either run may read)
  if (p.win_lo != 0 || p.win_hi != p.size) {
    const uint64_t need_lo = offset - min<uint64_t>(offset, (uint64_t)kReScanLimit);
    const uint64_t need_hi =
        min<uint64_t>(p.size, offset + max<uint64_t>((uint64_t)kReScanLimit, 2ull * e.length + 2));
    if (need_lo < p.win_lo || need_hi > p.win_hi) return kHexUndecided;
  }
  const DevRe r = e.re;
  if (r.fwd_len == 0) return kHexUndecided;
  const uint8_t* fwd = q.re_code + r.fwd_off;
  const uint8_t* bwd = q.re_code + r.bwd_off;
  // (contiguous in the blob: both programs staged at once when they fit)
  if (r.bwd_len == 0 || r.bwd_off == r.fwd_off + r.fwd_len) {
    const uint32_t at = hex_stage_code(fwd, r.fwd_len + r.bwd_len, codebuf);
    if (at != kNoLds) return hex_call(p, r, LdsCode{at}, LdsCode{at + r.fwd_len}, offset, m, set);
  }
  return hex_call(p, r, GlobalCode{fwd}, GlobalCode{bwd}, offset, m, set);
}

// The inclusive prefix sum of v over the wave's lanes.
__device__ __forceinline__ uint32_t wave_prefix(uint32_t v) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}
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
