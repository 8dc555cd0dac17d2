// Device data of the final-match stage for literal and hex strings (matches.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "verify.h"

namespace yamd {

constexpr uint32_t kStrChainPart = 0x2000;   // STRING_FLAGS_CHAIN_PART (types.h:66-88)

// A FINAL string: a kept call of it goes from _yr_scan_verify_literal_match
// through _yr_scan_match_callback straight to _yr_scan_add_match_to_list
// (scan.c:707-757) -- the call IS a match.  Literal, not a chain part (those
// are assembled by _yr_scan_verify_chained_string_match), not base64 (whose
// comparison the device does not restate).
__host__ __device__ inline bool string_is_final(uint32_t flags) {
  return (flags & kStrLiteral) != 0 && (flags & (kStrChainPart | kStrBase64Any)) == 0;
}

// The classes of strings the match stage settles (include/yara_amd.h
// YR_AMD_MATCH_*).
constexpr uint32_t kMatchLiteral = 1u, kMatchHex = 2u;
constexpr uint32_t kStrGreedyRegexp = 0x10000;   // STRING_FLAGS_GREEDY_REGEXP

// A FINAL HEX string: yr_re_fast_exec programs (only the hex lexer sets
// FAST_REGEXP) run on the plain ascii form.  _yr_scan_verify_re_match
// (scan.c:778-885) hands every backward MATCH of such a call to
// _yr_scan_add_match_to_list; the device restates both runs in position-set
// form (matches.hip hex_run).  The excluded flags do not occur on a
// compiler-made hex string: a hand-made table with one falls to the rest.
__host__ __device__ inline bool string_is_final_hex(uint32_t flags) {
  return (flags & (kStrFastRegexp | kStrAscii)) == (kStrFastRegexp | kStrAscii) &&
         (flags & (kStrLiteral | kStrChainPart | kStrWide | kStrNoCase | kStrFullWord |
                   kStrGreedyRegexp | kStrBase64Any)) == 0;
}
__host__ __device__ inline bool string_in_classes(uint32_t flags, uint32_t classes) {
  return ((classes & kMatchLiteral) && string_is_final(flags)) ||
         ((classes & kMatchHex) && string_is_final_hex(flags));
}

// Same layout as yr_amd_match_rec (include/yara_amd.h).
struct MatchRec {
  uint64_t offset;
  uint32_t string, length, xor_key, pool_index;
};
static_assert(sizeof(MatchRec) == 24, "match record layout");

// What the classify pass measured of a record: YR_MATCH.match_length, xor_key.
struct MatchMeasure {
  uint32_t length, xor_key;
};

struct MatchParams {
  const uint8_t* data;          // block (position 0; only [win_lo, win_hi) is read)
  uint64_t size;
  uint64_t win_lo, win_hi;
  const VerifyRec* recs;        // yr_amd_verify_device's records
  uint64_t n;                   // (at most kMatchMaxRecords)
  const DevPoolRec* pool;
  const uint32_t* pool_string;  // [n_pool] YR_STRING.idx of the pool entry's string
  uint32_t n_strings;           // a key's string field == n_strings: not a match (rest)
  const uint8_t* str_bytes;
  const uint8_t* lowercase;
  uint64_t* keys;               // [n] string << 32 | offset, in record order
  uint32_t* index;              // [n] record index (the sort's values)
  MatchMeasure* meas;           // [n] by record
  const uint64_t* sorted_keys;  // [n] after the stable sort
  const uint32_t* sorted_index;
  uint64_t* block_off;          // [verify_groups(n) + 1] per-wave counts -> offsets
  uint64_t* chunk_off;          // [verify_chunks(n) + 1] (launch_block_offsets)
  VerifyRec* rest;              // [n]
  MatchRec* out;                // [n]
};

// Output slots and one dispatch's work-items are 32-bit counts.
constexpr uint64_t kMatchMaxRecords = 0x7FFFFFFFull;

// Classify + measure: keys, index, meas, and the rest records per wave into block_off.
hipError_t launch_match_classify(const MatchParams& p, hipStream_t s);
// The rest records, stably compacted (block_off / chunk_off scanned).
hipError_t launch_match_rest(const MatchParams& p, hipStream_t s);
// Stable radix sort of (keys[0], index[0]) by the key bits [0, lo_bits) and
// [32, 32 + hi_bits), ping-pong between the two buffers of each pair:
// *result = the buffer that holds the sorted arrays.  hist: [match_sort_hist(n)
// + 1] and chunk: [verify_chunks(match_sort_hist(n) * kGroup) + 1] workspace,
// total: one scratch word (device-writable).
constexpr uint32_t kSortTile = 2048;   // items per wave
inline uint64_t match_sort_tiles(uint64_t n) { return (n + kSortTile - 1) / kSortTile; }
inline uint64_t match_sort_hist(uint64_t n) { return 256 * match_sort_tiles(n); }
hipError_t match_sort(uint64_t* const keys[2], uint32_t* const index[2], uint64_t n, int lo_bits,
                      int hi_bits, uint64_t* hist, uint64_t* chunk, uint64_t* total, hipStream_t s,
                      int* result);
// pass 0: distinct keys per wave into block_off; pass 1 (offsets scanned):
// the first entry of every run of equal keys as a MatchRec.
hipError_t launch_match_unique(const MatchParams& p, int pass, hipStream_t s);

// ---- The same stage for a batch (yr_amd_match_batch_device) ----
// The key gets a third, most significant field, the record's buffer, kept in
// an array of its own (any n fits: no batch is refused for key width).  The
// records of a batch lie in buffer order, rec_off[] their CSR; the sort by
// (buffer, string, offset) keeps every buffer's entries in the very slots
// [rec_off[k], rec_off[k + 1]) -- which is what the CSR offsets of the
// matches are counted from.
// A struct of its own: MatchParams is a kernel argument of the single-block
// kernels, which stay what they are.
struct BatchMatchParams {
  MatchParams m;                // data = the arena; size, win_lo, win_hi unused
  const uint64_t* starts;       // [nbuf] the buffers in the arena
  const uint64_t* sizes;        // [nbuf]
  const uint64_t* rec_off;      // [nbuf + 1] CSR of m.recs (yr_amd_verify_batch_device)
  uint32_t nbuf;
  uint32_t* buf;                // [m.n] by record: its buffer
  uint64_t* match_off;          // [nbuf + 1] CSR of m.out
  uint64_t* rest_off;           // [nbuf + 1] CSR of m.rest
};

// Classify: as launch_match_classify, each record measured in its own buffer, + buf.
hipError_t launch_batch_match_classify(const BatchMatchParams& p, hipStream_t s);
// rest_off from the scanned rest counts (before anything reuses block_off), and
// match_off from the scanned unique counts (after launch_batch_match_unique 0).
hipError_t launch_batch_match_offsets(const BatchMatchParams& p, int matches, hipStream_t s);
// match_sort, then the passes over the bits of nbuf - 1 (none for nbuf == 1),
// digits read from buf through the sorted index.
hipError_t batch_match_sort(uint64_t* const keys[2], uint32_t* const index[2], uint64_t n,
                            int lo_bits, int hi_bits, const uint32_t* buf, uint32_t nbuf,
                            uint64_t* hist, uint64_t* chunk, uint64_t* total, hipStream_t s,
                            int* result);
// As launch_match_unique; an entry is kept iff it is a match and its (buffer,
// key) differs from its predecessor's.
hipError_t launch_batch_match_unique(const BatchMatchParams& p, int pass, hipStream_t s);

// ---- The stage with the hex class (yr_amd_scanner_set_match_classes) ----
// A record of a final hex string can be several matches: one per
// bytes_matched value B of the backward program at MATCH, at offset - B with
// length B + F (F the forward program's smallest).  Records become ITEMS, one
// per match to be, and the sort and the unique pass work on items.  What a
// record contributes is its set of B values, a 64-bit mask over [base, base +
// 64); a literal record's set is {0}.
struct HexSet {
  uint64_t mask;   // bit i: B = base + i
  uint32_t base;
  uint32_t pad;
};

// A struct of its own: MatchParams is a kernel argument of the literal-only
// kernels, which stay what they are.  m.keys / m.block_off / m.chunk_off /
// m.rest are per RECORD here (the key of a record that yields no item has the
// string field n_strings: match_rest_kernel reads exactly that); the items'
// arrays are ikeys / iindex, and m.sorted_* / m.out hold items.
struct HexMatchParams {
  MatchParams m;
  const uint8_t* re_code;
  uint32_t classes;
  HexSet* sets;                 // [m.n] by record
  uint64_t* iblock_off;         // [verify_groups(m.n) + 1] items per wave of records -> offsets
  uint64_t* ichunk_off;         // [verify_chunks(m.n) + 1]
  uint64_t n_items;             // (expand, unique: after the wait for the count)
  uint64_t* ikeys;              // [n_items] string << 32 | (offset - B), records ascending
  uint32_t* iindex;             // [n_items] the item's record
  uint64_t* ublock_off;         // [verify_groups(n_items) + 1] unique pass
  uint64_t* uchunk_off;
};

// Measure: per record its key, measure, set; per wave the rest records into
// m.block_off and the items into iblock_off.
hipError_t launch_hex_measure(const HexMatchParams& p, hipStream_t s);
// The items of every record at its offset (iblock_off / ichunk_off scanned).
hipError_t launch_hex_expand(const HexMatchParams& p, hipStream_t s);
// As launch_match_unique over the items: the length is the record's forward
// length plus the distance from the item's offset to the record's.
hipError_t launch_hex_unique(const HexMatchParams& p, int pass, hipStream_t s);

// ---- The batch's stage with the hex class (yr_amd_scanner_set_batch_match_classes) ----
// Both of the above at once: records become items as in HexMatchParams, and
// the CSR of the matches is counted over ITEMS.  hex_expand_kernel writes the
// items ascending by record, i.e. by buffer, so buffer k's items hold the slots
// [item_off[k], item_off[k + 1]) -- item_off[k] = the items of the records
// below rec_off[k] -- and the sort by (buffer, string, offset) keeps them
// there, as it keeps the records' slots in BatchMatchParams.  An item's value
// is its record, and buf[] is by record: buf[index[i]] is the item's buffer
// (the buffer passes of batch_match_sort as they are).
// A struct of its own: HexMatchParams and BatchMatchParams are kernel
// arguments of the kernels above, which stay what they are.  The rest goes
// through match_rest_kernel and batch_match_offsets_kernel<0> (h.m.keys /
// h.m.block_off / h.m.chunk_off are per record, as in HexMatchParams), the
// expansion through hex_expand_kernel.
struct BatchHexParams {
  HexMatchParams h;             // h.m.data = the arena; size, win_lo, win_hi unused
  const uint64_t* starts;       // [nbuf] the buffers in the arena
  const uint64_t* sizes;        // [nbuf]
  const uint64_t* rec_off;      // [nbuf + 1] CSR of h.m.recs
  uint32_t nbuf;
  uint32_t* buf;                // [h.m.n] by record: its buffer
  uint64_t* item_off;           // [nbuf + 1] CSR of the items
  uint64_t* match_off;          // [nbuf + 1] CSR of h.m.out
};

// Measure: as launch_hex_measure, each record in its own buffer, + buf.
hipError_t launch_batch_hex_measure(const BatchHexParams& p, hipStream_t s);
// matches == 0: item_off from the scanned item counts (iblock_off / ichunk_off);
// 1: match_off from the scanned unique counts (after launch_batch_hex_unique 0)
// at the slots item_off names.
hipError_t launch_batch_hex_offsets(const BatchHexParams& p, int matches, hipStream_t s);
// As launch_hex_unique; an item is kept iff it is a match and its key or its
// record's buffer differs from its predecessor's.
hipError_t launch_batch_hex_unique(const BatchHexParams& p, int pass, hipStream_t s);

}  // namespace yamd
