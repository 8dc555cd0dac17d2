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

// ---- The wave-wide path of the hex class (yr_amd_scanner_set_hex_wide) ----
// A record whose set leaves HexSet's 64 positions is measured by one WAVE: the
// whole domain of yr_re_fast_exec, bytes_matched 0 .. YR_RE_SCAN_LIMIT, is 64
// lanes x 64 bits, word l of the set in lane l, plus one bit for the value
// YR_RE_SCAN_LIMIT itself (a consuming opcode at 4095).  The measure pass
// queues such records; their backward sets go to wsets by queue slot, word
// kWideWords - 1 holding that last bit.  In sets[] a wide match is marked by
// mask 0, pad 1: it has no item for the lane-per-record expansion.
constexpr uint32_t kWideWords = 65;
// A struct of its own: HexMatchParams is a kernel argument of the kernels
// above, which stay what they are.
struct HexWideParams {
  HexMatchParams h;
  uint32_t* queue;              // [qcap] the queued records, in no particular order
  uint32_t* qlen;               // records appended; above qcap: the host grows and runs again
  uint32_t qcap;
  uint64_t* qlen_out;           // qlen for the host (pinned)
  uint64_t* wsets;              // [qcap][kWideWords]
  uint32_t* icount;             // [h.m.n] items by record
  uint32_t* istart;             // [h.m.n] the items of the records below it in its wave
};

// The measure pass with the queue: launch_hex_measure's outputs + icount, then
// one wave per queued record (a fixed grid of `waves` waves strides over the
// queue: no wait for its length), then the per-wave counts again from the
// per-record arrays, + istart.
hipError_t launch_hex_wide_measure(const HexWideParams& w, uint32_t waves, hipStream_t s);
// launch_hex_expand by istart, then the wide records' items, one wave each.
hipError_t launch_hex_wide_expand(const HexWideParams& w, uint32_t waves, hipStream_t s);

// ---- The batch's wave-wide path (yr_amd_scanner_set_batch_hex_wide) ----
// BatchHexParams and HexWideParams at once.  A queue entry is
// a pair: the record in queue[slot], its buffer in qbuf[slot] -- the measure
// pass has searched rec_off for it already, and the wide wave takes its bounds
// [arena + starts[k], + sizes[k]) from there.  A record can be kReScanLimit + 1
// items, so the items' CSR is read from icount / istart, not from the sets'
// masks.  The recount and both expansion kernels are the single-block ones:
// they read none of w.h.m.data / size / win_*, and the queue's first array is
// theirs as it is.  The sort, the unique pass and match_off go through
// BatchHexParams (h = w.h) unchanged.
// A struct of its own: HexWideParams and BatchHexParams are kernel arguments
// of the kernels above, which stay what they are.
struct BatchHexWideParams {
  HexWideParams w;              // w.h.m.data = the arena; size, win_lo, win_hi unused
  const uint64_t* starts;       // [nbuf] the buffers in the arena
  const uint64_t* sizes;        // [nbuf]
  const uint64_t* rec_off;      // [nbuf + 1] CSR of w.h.m.recs
  uint32_t nbuf;
  uint32_t* buf;                // [w.h.m.n] by record: its buffer
  uint32_t* qbuf;               // [w.qcap] by queue slot: the queued record's buffer
  uint64_t* item_off;           // [nbuf + 1] CSR of the items
};

// launch_hex_wide_measure for a batch: every record, narrow or wide, measured
// in its own buffer, + buf.
hipError_t launch_batch_hex_wide_measure(const BatchHexWideParams& p, uint32_t waves, hipStream_t s);
// item_off from the scanned item counts (iblock_off / ichunk_off) and istart.
hipError_t launch_batch_hex_wide_offsets(const BatchHexWideParams& p, hipStream_t s);

// The pieces of launch_hex_wide_measure one by one, for a driver that runs a
// measure pass of its own between them (alternations.hip): 0 the queue's
// length cleared, 1 one wave per queued record, 2 the recount.
hipError_t launch_hex_wide_piece(const HexWideParams& w, uint32_t waves, int piece, hipStream_t s);

// ---- Alternation strings (yr_amd_scanner_set_alternations; alternations.hip) ----
// A string whose programs are loop-free yr_re_exec programs (hex strings with
// alternatives, regexps without * and +) is measured one WAVE per record from
// a table of fixed-size instructions the host decodes at upload: instruction
// i of a program in lane i, its position set (bit b: bytes_matched = b) in
// lane i of a VGPR pair, every byte test one vector compare whose result is
// the wave mask.
constexpr uint32_t kAltMaxInsns = 64;     // a program's instructions live in the wave's lanes
constexpr uint32_t kAltClassWords = 9;    // RE_CLASS: 8 words of bitmap, then `negated`
enum AltOp : uint8_t {
  kAltByte = 0,    // ((c & b) == a) != flag     LITERAL / NOT_ / MASKED_ / MASKED_NOT_
  kAltAny,         // DOT_ALL || c != 0x0A
  kAltClass,       // bit c of class a | b << 16, != its negated byte
  kAltWord,        // \w, flag: \W
  kAltSpace,       // \s, flag: \S
  kAltDigit,       // \d, flag: \D
  kAltRepeat,      // REPEAT_ANY {a, b}; flag: greedy
  kAltSplit,       // flag 0: SPLIT_A (prefers next), 1: SPLIT_B (prefers target)
  kAltJump,
  kAltMatch,
};
struct AltInsn {
  uint8_t op, next, target, flag;   // next / target: instruction INDICES, above its own
  uint16_t a, b;
};
static_assert(sizeof(AltInsn) == 8, "decoded instruction layout");
// Per pool entry: its programs in the instruction table (n_fwd 0: not an
// alternation string's entry; n_bwd 0: no backward program).
struct AltProg {
  uint32_t fwd, bwd;
  uint8_t n_fwd, n_bwd;
  uint16_t pad;
};
struct AltTables {
  const AltProg* progs;         // [n_pool]
  const AltInsn* insns;
  const uint32_t* classes;      // [..][kAltClassWords]
  const uint8_t* str_alt;       // [n_strings] 1: an alternation string
};
// A struct of its own: HexWideParams is a kernel argument of the kernels
// above, which stay what they are.  w.queue / w.qlen are the wide path's (its
// queue stays empty with `wide` 0), w.icount / w.istart are used either way.
struct AltParams {
  HexWideParams w;
  AltTables t;
  uint32_t* queue;              // [qcap] the queued alternation records
  uint32_t* qlen;
  uint32_t qcap;
  uint64_t* qlen_out;           // qlen for the host (pinned)
  uint32_t wide;                // the wave-wide path of the hex class is on too
};
// The measure pass with both queues: the wide path's clear, the twin of
// hex_measure_queue_kernel that queues alternation records too, one wave per
// queued alternation record, (wide) one wave per queued wide record, the recount.
hipError_t launch_alt_measure(const AltParams& a, uint32_t waves, hipStream_t s);

// ---- The batch's alternation strings (yr_amd_scanner_set_batch_alternations) ----
// BatchHexWideParams and AltParams at once.  A queue entry is a pair, as the
// batch's wide queue's: the record in queue[slot], its buffer in qbuf[slot];
// the wave takes the buffer's bounds [arena + starts[k], + sizes[k]) from
// there and sees the buffer as the whole block of both runs.  A settled record
// leaves what the narrow hex path leaves, so the items' CSR (icount / istart,
// launch_batch_hex_wide_offsets), the expansion, the sort, the unique pass and
// match_off run unchanged.
// A struct of its own: BatchHexWideParams and AltParams are kernel arguments
// of the kernels above, which stay what they are.  b.w.queue / b.w.qlen /
// b.qbuf are the wide path's (its queue stays empty with `wide` 0), b.w.icount
// / b.w.istart are used either way.
struct BatchAltParams {
  BatchHexWideParams b;
  AltTables t;
  uint32_t* queue;              // [qcap] the queued alternation records
  uint32_t* qbuf;               // [qcap] by queue slot: the queued record's buffer
  uint32_t* qlen;
  uint32_t qcap;
  uint64_t* qlen_out;           // qlen for the host (pinned)
  uint32_t wide;                // the batch's wave-wide path is on too
};
// launch_alt_measure for a batch: both queues cleared, the twin of
// batch_hex_measure_queue_kernel that queues alternation records too, one wave
// per queued alternation pair, (wide) one wave per queued wide pair, the recount.
hipError_t launch_batch_alt_measure(const BatchAltParams& a, uint32_t waves, hipStream_t s);
// The middle piece of launch_batch_hex_wide_measure on its own, for that
// launcher: one wave per queued wide pair.
hipError_t launch_batch_hex_wide_waves(const BatchHexWideParams& p, uint32_t waves, hipStream_t s);

// One wave per queued alternation record on its own (alt_measure_kernel), for
// a driver that runs a measure pass with more queues (loops.hip).
hipError_t launch_alt_waves(const AltParams& a, uint32_t waves, hipStream_t s);

// ---- Loop strings (yr_amd_scanner_set_loops; loops.hip) ----
// A text regexp with * or + and no counters: byte tests, SPLIT, JUMP, MATCH,
// at least one backward edge, every cycle through a byte test.  A fiber is
// its instruction, so yr_re_exec's list at input position b is a set of at
// most 64 instructions, one 64-bit word: the wave keeps one word PER POSITION
// (0 .. YR_RE_SCAN_LIMIT) in LDS where the alternation kernels keep one
// 64-position word per instruction.  Instructions are AltInsn (kAltRepeat
// never occurs, next / target are indices in either direction, a CLASS keeps
// its `negated` in flag and its bitmap's index in a | b << 16); masks holds per
// instruction {eps, succ}: eps the RESTING instructions (byte tests, MATCH)
// reachable over SPLIT / JUMP edges alone (the instruction itself if it
// rests), succ = eps[next] of a byte test, else 0.
constexpr uint32_t kLoopPositions = 4097;   // bytes_matched 0 .. YR_RE_SCAN_LIMIT
constexpr uint32_t kLoopClassWords = 8;
constexpr uint8_t kLoopString = 1, kLoopGreedy = 2;   // str_loop bits
struct LoopTables {
  const AltProg* progs;         // [n_pool] n_fwd 0: not a loop string's entry
  const AltInsn* insns;
  const uint64_t* masks;        // [2 * insns] eps, succ
  const uint32_t* classes;      // [..][kLoopClassWords]
  const uint8_t* str_loop;      // [n_strings] kLoopString | kLoopGreedy (STRING_FLAGS_GREEDY_REGEXP)
};
// A struct of its own: AltParams is a kernel argument of the kernels above,
// which stay what they are.  a.w is used either way (as AltParams uses w);
// a.t / a.queue / a.qlen only with `alts`.
struct LoopParams {
  AltParams a;
  LoopTables t;
  uint32_t* queue;              // [qcap] the queued loop records
  uint32_t* qlen;
  uint32_t qcap;
  uint64_t* qlen_out;           // qlen for the host (pinned)
  uint32_t alts;                // alternation strings are settled too
};
// The measure pass with three queues: all cleared, the twin of
// alt_measure_queue_kernel that queues loop records too, one wave per queued
// alternation record (alts), per queued loop record, per wide record (a.wide),
// the recount.
hipError_t launch_loop_measure(const LoopParams& l, uint32_t waves, hipStream_t s);
// launch_hex_unique pass 1 with scan.c:756's replace_if_exists: of the items
// with one (string, offset) the FIRST supplies length and pool_index, but for
// a greedy loop string the LAST.  (Pass 0 is launch_hex_unique's.)
struct LoopUniqueParams {
  HexMatchParams h;
  const uint8_t* str_loop;
};
hipError_t launch_loop_unique(const LoopUniqueParams& u, hipStream_t s);

// ---- The batch's loop strings (yr_amd_scanner_set_batch_loops) ----
// BatchAltParams and LoopParams at once.  A queue entry is a pair, as the
// batch's other queues': the record in queue[slot], its buffer in qbuf[slot];
// the wave sees the buffer [arena + starts[k], + sizes[k]) as the whole block
// of both runs.  A run inside a buffer reads at most min(sizes[k],
// YR_RE_SCAN_LIMIT) bytes, so the wave's table of live sets is `words` =
// min(largest buffer, YR_RE_SCAN_LIMIT) + 1 words of dynamic LDS, not
// kLoopPositions; the wave treats `words` as a hard bound.  A settled record
// leaves {mask, base} as in LoopParams, so the items' CSR (icount / istart),
// the expansion, the sort and match_off run unchanged.
// A struct of its own: BatchAltParams and LoopParams are kernel arguments of
// the kernels above, which stay what they are.  a.b is used either way (as
// BatchAltParams uses b); a.t / a.queue / a.qbuf / a.qlen only with `alts`.
struct BatchLoopParams {
  BatchAltParams a;
  LoopTables t;
  uint32_t* queue;              // [qcap] the queued loop records
  uint32_t* qbuf;               // [qcap] by queue slot: the queued record's buffer
  uint32_t* qlen;
  uint32_t qcap;
  uint64_t* qlen_out;           // qlen for the host (pinned)
  uint32_t alts;                // alternation strings are settled too
  uint32_t words;               // the table's words: 2 .. kLoopPositions
};
// launch_loop_measure for a batch: all queues cleared, the twin of
// batch_alt_measure_queue_kernel that queues loop pairs too, one wave per
// queued alternation pair (alts), per queued loop pair (words * 8 bytes of
// dynamic LDS each), per wide pair (a.wide), the recount.
hipError_t launch_batch_loop_measure(const BatchLoopParams& l, uint32_t waves, hipStream_t s);
// One wave per queued alternation pair on its own (batch_alt_measure_kernel),
// for that launcher.
hipError_t launch_batch_alt_waves(const BatchAltParams& a, uint32_t waves, hipStream_t s);
// launch_batch_hex_unique pass 1 with replace_if_exists, as launch_loop_unique:
// a run of items with one (buffer, string, offset) is in record order; a greedy
// loop string takes its last item's record, everything else the first's.
// (Pass 0 is launch_batch_hex_unique's.)
struct BatchLoopUniqueParams {
  BatchHexParams b;
  const uint8_t* str_loop;
};
hipError_t launch_batch_loop_unique(const BatchLoopUniqueParams& u, hipStream_t s);

// ---- Chained strings (yr_amd_scanner_set_chains; chains.hip) ----
// libyara splits a hex string at every jump wider than
// YR_STRING_CHAINING_THRESHOLD into a chain S0 <- S1 <- ... (chained_to links
// a part to the one before it); _yr_scan_verify_chained_string_match
// (scan.c:406-632) assembles the parts' matches into the head's.  A chain is
// SETTLED with the classes when each part, the chain bits masked off, is a
// string of the classes; its records then become EVENTS, replayed per chain in
// record order by one wave.
constexpr uint32_t kStrChainTail = 0x4000;   // STRING_FLAGS_CHAIN_TAIL
constexpr uint32_t kNoChain = 0xFFFFFFFFu;
constexpr uint32_t kChainMaxLevels = 64;     // a level's state lives in its lane

// (Not an XOR part: a chain's match carries xor_key 0, the parts' keys are not
// kept.  The compiler makes chains of hex strings and regexps, which have none.)
__host__ __device__ inline bool string_settles_in_chain(uint32_t flags, uint32_t classes) {
  return (flags & kStrXor) == 0 &&
         string_in_classes(flags & ~(kStrChainPart | kStrChainTail), classes);
}

// The tables' chain records on the device (yr_amd_tables_set_chains).
struct ChainTables {
  const uint32_t* chain_of;     // [n_strings] the string's chain, kNoChain: none
  const uint32_t* level_of;     // [n_strings] its place in the chain, the head's 0
  const int32_t* gap_min;       // [n_strings] YR_STRING.chain_gap_min / _max: the distance
  const int32_t* gap_max;       //   from the end of the part before it
  const uint32_t* chain_off;    // [n_chains + 1] CSR of chain_strs
  const uint32_t* chain_strs;   // the chains' strings by level
  const uint8_t* settled;       // [n_chains] bit (classes >> 1): settled with LITERAL / + HEX
  uint32_t n_chains;
};

// m / re_code / classes / sets are the measure pass's (HexMatchParams): the
// stage runs behind it and rewrites what it wrote for the records it consumes
// -- key string field n_strings + 1 (neither a match nor the rest), an empty
// set, the per-wave rest counts in m.block_off.
struct ChainParams {
  HexMatchParams h;
  ChainTables t;
  uint32_t* rchain;             // [n] by record: its chain if it is an event, else n_chains
  uint32_t* ev_level;           // [n] by record: the event {level, offset, length}
  uint32_t* ev_offset;
  uint32_t* ev_length;
  uint32_t* dirty;              // [n_chains] some record of the chain is not exactly one event
  uint64_t* str_off;            // [n_strings + 1] events per string -> offsets within chunks
  uint64_t* str_chunk;          // [verify_chunks(n_strings * kGroup) + 1]
  uint64_t* skeys;              // [n] the sort's keys: rchain (values: the record)
  uint32_t* sindex;
  const uint64_t* sorted_keys;  // after the stable sort by chain
  const uint32_t* sorted_index;
  uint32_t* cbegin;             // [n_chains] the chain's events in the sorted arrays
  uint32_t* cend;
  uint32_t* lists;              // [4][n] the unconfirmed lists past the LDS share: offset,
                                //   length, chain_length, record; string k's at str_off(k)
  uint64_t* item_keys;          // [n] the confirmed heads: string << 32 | offset
  uint32_t* item_index;         // [n] the head's record
  uint32_t* item_count;         // items appended
};

// Clear; one lane per record: the event or the dirty flag; then, the flags
// complete, the consumed records marked and the rest recounted + skeys / sindex.
hipError_t launch_chain_events(const ChainParams& c, hipStream_t s);
// (str_off scanned, skeys sorted) the chains' bounds, then one wave per chain
// with events: scan.c:406-632 over its events, the confirmed heads appended as
// items and their lengths left in m.meas at the head's record.
hipError_t launch_chain_replay(const ChainParams& c, uint32_t waves, hipStream_t s);

// ---- The batch's chains (yr_amd_scanner_set_batch_chains) ----
// A chain is replayed per (buffer, chain) GROUP, its events measured inside
// their own buffer.  Nothing here is sized by nbuf x n_chains or nbuf x
// n_strings: the events and the dirty-makers (records that are not exactly one
// event) get their chain as sort key, batch_match_sort orders them by (buffer,
// chain) -- stable, so each group is one contiguous run in record order -- and
// the groups are found in that stream.  A group's dirtiness is read off its
// own run, its lists live in its own slots [begin, end) of `lists` (a list
// holds at most its level's events), and the confirmed heads are counted per
// buffer so that the items' CSR can account for them.
// A struct of its own: ChainParams and BatchHexParams are kernel arguments of
// the kernels above, which stay what they are.
constexpr uint32_t kChainDirtyMaker = 0xFFFFFFFFu;   // ev_level of a dirty-maker
struct BatchChainParams {
  BatchHexParams b;             // the measure pass's, + buf; h.m.keys / h.sets / h.m.block_off are
                                //   rewritten for the consumed records as in ChainParams
  ChainTables t;
  uint32_t* ev_level;           // [n] by record: the event {level, local offset, length},
  uint32_t* ev_offset;          //   level kChainDirtyMaker: no event, its group is dirty
  uint32_t* ev_length;
  uint64_t* skeys;              // [n] the sort's keys: the chain of an event or dirty-maker,
  uint32_t* sindex;             //   else n_chains (values: the record)
  const uint64_t* sorted_keys;  // after the stable sort by (buffer, chain)
  const uint32_t* sorted_index;
  uint32_t* gbegin;             // [n] the group list: each group's first sorted slot
  uint32_t* counts;             // {groups, items appended}
  uint32_t* lists;              // [4][n] the unconfirmed lists past the LDS share
  uint64_t* item_keys;          // [n] the confirmed heads: string << 32 | local offset
  uint32_t* item_index;         // [n] the head's record
  uint64_t* buf_items;          // [nbuf + 1] chain items per buffer -> offsets within chunks
  uint64_t* buf_chunk;          // [verify_chunks(nbuf * kGroup) + 1] (launch_block_offsets)
};

// Clear; one lane per record (behind the batch measure pass): the event or the
// dirty-maker, + skeys / sindex.
hipError_t launch_batch_chain_events(const BatchChainParams& c, hipStream_t s);
// (skeys sorted by batch_match_sort) the group list; one wave per group: a
// clean group's events leave the rest and are replayed, the confirmed heads
// appended as items and counted into buf_items; then the per-wave rest counts
// again.  Ahead of the rest's offsets.
hipError_t launch_batch_chain_replay(const BatchChainParams& c, uint32_t waves, hipStream_t s);
// (buf_items scanned, item_off written) item_off[k] += the chain items of the
// buffers below k.
hipError_t launch_batch_chain_item_offsets(const BatchChainParams& c, hipStream_t s);

}  // namespace yamd
