// gfx950 kernels of the match stage for ALTERNATION strings
// (yr_amd_scanner_set_alternations; matches.h AltParams): the
// strings whose programs are loop-free yr_re_exec programs -- hex strings with
// alternatives, regexps without * and + -- measured one WAVE per record.
//
// yr_re_exec (re.c:1693-2068) runs an ordered list of fibers; without
// EXHAUSTIVE a fiber at MATCH kills the fibers behind it, so the forward
// result is the bytes_matched of the HIGHEST-PRIORITY path that reaches MATCH,
// not the shortest; with EXHAUSTIVE (backwards) every bytes_matched at MATCH is
// a match.  In a loop-free program without counter stacks a fiber's future is a
// function of (instruction, rc) alone, so both results follow from position
// sets:
//
//   * lane b of the wave holds input byte b of the run (one coalesced load);
//   * a byte test is one vector compare, its result the 64-bit wave mask
//     "byte b passes instruction i", kept in lane i of a VGPR pair;
//   * the set of positions at which instruction i is live is a 64-bit scalar,
//     kept in lane i of another pair, read with readlane and written by a
//     wave-uniform select on the lane id; all
//     set algebra -- shift, and, or -- runs on the scalar unit, wave-uniform:
//     no per-lane divergence, no choice stack, no step budget;
//   * the host has decoded every program into fixed-size instructions whose
//     successors are instruction INDICES above their own (AltInsn), so one
//     ascending sweep is a topological order.
//
// Backwards that sweep's set at MATCH is the answer.  Forwards a descending
// sweep gives R[i], the positions from which instruction i still reaches
// MATCH, and a walk of one state (i, b) takes at every SPLIT / REPEAT_ANY the
// preferred branch whose R has the bit.  Position 64 (a consuming instruction
// that passes at byte 63) is carried as one bit per INSTRUCTION; a run that
// would have to read byte 64 leaves the record in the rest.
//
// The batch calls (yr_amd_scanner_set_batch_alternations; matches.h
// BatchAltParams) run the same machinery per buffer: the queue
// holds (record, buffer) pairs and alt_record gets the buffer as its block.
#include "internal.h"
#include "matches.h"
#include "match_measure.h"

namespace yamd {

namespace {

__device__ __forceinline__ uint32_t lane_read(uint32_t v, uint32_t i) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)i);
}
__device__ __forceinline__ uint64_t lane_get(uint32_t lo, uint32_t hi, uint32_t i) {
  return (uint64_t)lane_read(hi, i) << 32 | lane_read(lo, i);
}
__device__ __forceinline__ void lane_set(uint32_t& lo, uint32_t& hi, uint32_t i, uint64_t v) {
  // a writelane with wave-uniform v and i, as a select on the lane id (the
  // compiler at hand has no builtin for v_writelane_b32): one compare, two moves
  const bool mine = (threadIdx.x & 63u) == i;
  lo = mine ? (uint32_t)v : lo;
  hi = mine ? (uint32_t)(v >> 32) : hi;
}
__device__ __forceinline__ void lane_or(uint32_t& lo, uint32_t& hi, uint32_t i, uint64_t v) {
  lane_set(lo, hi, i, lane_get(lo, hi, i) | v);
}

// One program of one record in the wave's registers: instruction i in lane i
// (op | next << 8 | target << 16 | flag << 24; a | b << 16) and, for the
// instructions that read a byte, lane i's mask of the input bytes that pass.
struct AltRun {
  uint32_t ilo, ihi;
  uint32_t plo, phi;
  uint32_t n;
  int maxb;   // max_bytes_matched
};

constexpr uint32_t kAltNoInsn = 0xFFu;

struct AltDecoded {
  uint32_t op, next, target, flag, a, b;
};
__device__ __forceinline__ AltDecoded alt_decode(const AltRun& r, uint32_t i) {
  const uint32_t lo = lane_read(r.ilo, i), hi = lane_read(r.ihi, i);
  return AltDecoded{lo & 0xFFu, (lo >> 8) & 0xFFu, (lo >> 16) & 0xFFu, lo >> 24, hi & 0xFFFFu, hi >> 16};
}

// The program's instructions and its pass masks.  c: this lane's input byte,
// valid: the byte exists (b < max_bytes_matched).  cls: the wave's LDS words
// for one CLASS at a time.  false: an instruction the host never emits.
__device__ bool alt_load(const AltTables& t, uint32_t first, uint32_t n, uint32_t c, bool valid,
                         bool dot_all, uint32_t* cls, int maxb, AltRun& r) {
  const uint32_t lane = threadIdx.x & 63u;
  r.n = n;
  r.maxb = maxb;
  r.ilo = r.ihi = r.plo = r.phi = 0;
  if (lane < n) {
    const AltInsn in = t.insns[first + lane];
    r.ilo = in.op | (uint32_t)in.next << 8 | (uint32_t)in.target << 16 | (uint32_t)in.flag << 24;
    r.ihi = in.a | (uint32_t)in.b << 16;
  }
  for (uint32_t i = 0; i < n; ++i) {
    const AltDecoded d = alt_decode(r, i);
    bool ok;
    switch (d.op) {
      case kAltByte: ok = ((c & d.b) == d.a) != (d.flag != 0); break;
      case kAltAny:
      case kAltRepeat: ok = dot_all || c != 0x0Au; break;
      case kAltClass: {
        // (one wave writes and reads its words: LDS serves a wave's requests in order)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane < kAltClassWords) cls[lane] = t.classes[(uint64_t)(d.a | d.b << 16) * kAltClassWords + lane];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        ok = (((cls[c >> 5] >> (c & 31u)) & 1u) != 0) != ((cls[8] & 0xFFu) != 0);
        break;
      }
      case kAltWord:
        ok = ((c - '0' < 10u) || ((c | 0x20u) - 'a' < 26u) || c == '_') != (d.flag != 0);
        break;
      case kAltSpace: ok = (c == ' ' || (c - 9u) < 5u) != (d.flag != 0); break;   // \t \n \v \f \r
      case kAltDigit: ok = (c - '0' < 10u) != (d.flag != 0); break;
      case kAltSplit:
      case kAltJump:
      case kAltMatch: continue;
      default: return false;
    }
    lane_set(r.plo, r.phi, i, __ballot(ok && valid));
  }
  return true;
}

constexpr int kAltOk = 0, kAltLeaves = 1;   // kAltLeaves: a live position would leave the window

// The ascending sweep: S[0] = {0}; a consuming instruction sends (S n pass) <<
// 1 to its successor, SPLIT its set to both, JUMP to one, REPEAT_ANY {mn, mx}
// the OR of S << k over k = mn .. mx along runs of passing bytes.  `top`: bit
// i = position 64 is live at instruction i -- it can reach MATCH through
// SPLIT / JUMP / an empty repeat, and nothing else unless max_bytes_matched is
// 64 (where it dies as the reference's fiber does).  M / mtop: the set at MATCH.
__device__ int alt_sets(const AltRun& r, uint64_t& M, bool& mtop, uint64_t& top) {
  uint32_t slo = 0, shi = 0;
  lane_set(slo, shi, 0, 1ull);
  top = 0;
  M = 0;
  mtop = false;
  for (uint32_t i = 0; i < r.n; ++i) {
    const uint64_t s = lane_get(slo, shi, i);
    const bool t = (top >> i) & 1u;
    if (s == 0 && !t) continue;
    const AltDecoded d = alt_decode(r, i);
    const uint64_t pm = lane_get(r.plo, r.phi, i);
    if (d.op <= kAltDigit) {
      if (t && r.maxb > 64) return kAltLeaves;
      const uint64_t x = s & pm;
      if (x >> 63) top |= 1ull << d.next;
      lane_or(slo, shi, d.next, x << 1);
    } else if (d.op == kAltRepeat) {
      if (t) {
        if (r.maxb > 64) return kAltLeaves;
        if (d.a == 0) top |= 1ull << d.next;
      }
      uint64_t cur = s, out = d.a == 0 ? s : 0ull;
      for (uint32_t k = 1; k <= d.b && cur != 0; ++k) {
        const uint64_t x = cur & pm;
        if (x >> 63) {
          if (k >= d.a) top |= 1ull << d.next;
          if (k < d.b && r.maxb > 64) return kAltLeaves;
        }
        cur = x << 1;
        if (k >= d.a) out |= cur;
      }
      lane_or(slo, shi, d.next, out);
    } else if (d.op == kAltSplit) {
      lane_or(slo, shi, d.next, s);
      lane_or(slo, shi, d.target, s);
      if (t) top |= 1ull << d.next | 1ull << d.target;
    } else if (d.op == kAltJump) {
      lane_or(slo, shi, d.target, s);
      if (t) top |= 1ull << d.target;
    } else {   // kAltMatch
      M |= s;
      mtop = mtop || t;
    }
  }
  return kAltOk;
}

// The descending sweep and the priority walk: F = bytes_matched of the
// highest-priority path to MATCH.  R[i] bit b: from (i, b) MATCH is reachable;
// rtop bit i: from (i, 64).  The walk starts at (0, 0), which the caller has
// found to reach MATCH, and every step raises i: at most n steps.
__device__ bool alt_priority(const AltRun& r, uint32_t& F) {
  uint32_t rlo = 0, rhi = 0;
  uint64_t rtop = 0;
  for (uint32_t i = r.n; i-- > 0;) {
    const AltDecoded d = alt_decode(r, i);
    const uint64_t pm = lane_get(r.plo, r.phi, i);
    uint64_t R = 0;
    bool rt = false;
    if (d.op <= kAltDigit) {
      R = pm & (lane_get(rlo, rhi, d.next) >> 1 | ((rtop >> d.next) & 1ull) << 63);
    } else if (d.op == kAltRepeat) {
      uint64_t h = lane_get(rlo, rhi, d.next), htop = (rtop >> d.next) & 1ull;
      if (d.a == 0) {
        R = h;
        rt = htop != 0;
      }
      for (uint32_t k = 1; k <= d.b; ++k) {
        h = pm & (h >> 1 | htop << 63);
        htop = 0;
        if (h == 0) break;
        if (k >= d.a) R |= h;
      }
    } else if (d.op == kAltSplit) {
      R = lane_get(rlo, rhi, d.next) | lane_get(rlo, rhi, d.target);
      rt = ((rtop >> d.next | rtop >> d.target) & 1ull) != 0;
    } else if (d.op == kAltJump) {
      R = lane_get(rlo, rhi, d.target);
      rt = ((rtop >> d.target) & 1ull) != 0;
    } else {   // kAltMatch
      R = ~0ull;
      rt = true;
    }
    lane_set(rlo, rhi, i, R);
    if (rt) rtop |= 1ull << i;
  }
  auto has = [&](uint32_t i, uint32_t b) {
    return b < 64 ? ((lane_get(rlo, rhi, i) >> b) & 1ull) != 0 : ((rtop >> i) & 1ull) != 0;
  };
  uint32_t i = 0, b = 0;
  if (!has(0, 0)) return false;
  for (uint32_t step = 0; step < r.n; ++step) {
    const AltDecoded d = alt_decode(r, i);
    if (d.op == kAltMatch) {
      F = b;
      return true;
    }
    if (b > 64) return false;
    if (d.op <= kAltDigit) {
      b += 1;
      i = d.next;
    } else if (d.op == kAltJump) {
      i = d.target;
    } else if (d.op == kAltSplit) {
      const uint32_t pref = d.flag ? d.target : d.next, other = d.flag ? d.next : d.target;
      i = has(pref, b) ? pref : other;
    } else {   // kAltRepeat: greedy the most repetitions first, ungreedy the fewest
      uint32_t run = 0;   // passing bytes from b on
      if (b < 64) {
        const uint64_t x = ~(lane_get(r.plo, r.phi, i) >> b);
        run = x != 0 ? (uint32_t)__builtin_ctzll(x) : 64u;
      }
      const uint32_t last = min(d.b, run);
      uint32_t k = kAltNoInsn;
      if (d.a <= last) {
        if (d.flag) {
          for (uint32_t j = last + 1; j-- > d.a;)
            if (has(d.next, b + j)) { k = j; break; }
        } else {
          for (uint32_t j = d.a; j <= last; ++j)
            if (has(d.next, b + j)) { k = j; break; }
        }
      }
      if (k == kAltNoInsn) return false;
      b += k;
      i = d.next;
    }
  }
  return false;
}

// hex_measure_queue_kernel's twin (matches.hip) with the second queue: a
// record of an alternation string all of whose bytes are in the window is a
// rest record for now and its index is appended to the alternation queue.
// WIDE: as hex_measure_queue_kernel queues the wide records; else a final hex
// string's record is measured as hex_measure_kernel measures it.
template <bool WIDE>
__global__ __launch_bounds__(256) void alt_measure_queue_kernel(AltParams a) {
  __shared__ __attribute__((aligned(16))) uint8_t codebuf[256 * kHexCodeBytes + 16];
  const HexWideParams& w = a.w;
  const HexMatchParams& q = w.h;
  const MatchParams& p = q.m;
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool wide = false, alt = false;
  if (r < p.n) {
    const VerifyRec rec = p.recs[r];
    const DevPoolRec e = p.pool[rec.pool_index];
    MatchMeasure m;
    HexSet set{1ull, 0u, 0u};
    bool is_match;
    if (a.t.str_alt[p.pool_string[rec.pool_index]] != 0) {
      m.length = 0;
      m.xor_key = 0;
      is_match = false;
      alt = rec.offset < p.size;
      // (measure_hex's bounds: every byte either run may read)
      if (alt && (p.win_lo != 0 || p.win_hi != p.size)) {
        const uint64_t need_lo = rec.offset - min<uint64_t>(rec.offset, (uint64_t)kReScanLimit);
        const uint64_t need_hi = min<uint64_t>(p.size, rec.offset + (uint64_t)kReScanLimit);
        alt = need_lo >= p.win_lo && need_hi <= p.win_hi;
      }
    } else if ((q.classes & kMatchHex) && string_is_final_hex(e.flags)) {
      m.length = 0;
      m.xor_key = 0;
      const uint32_t buf = (uint32_t)(uintptr_t)(codebuf + threadIdx.x * kHexCodeBytes);
      const int v = measure_hex<WIDE>(q, e, rec.offset, buf, m, set);
      is_match = v == kHexMatch;
      wide = WIDE && v == kHexWide;
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
  if (WIDE) {
    const uint64_t qmask = __ballot(wide);
    if (qmask != 0) {   // (wave-uniform)
      uint32_t at = 0;
      if ((threadIdx.x & 63u) == 0) at = atomicAdd(w.qlen, (uint32_t)__popcll(qmask));
      at = (uint32_t)__shfl((int)at, 0, 64) + lanes_below(qmask);
      if (wide && at < w.qcap) w.queue[at] = (uint32_t)r;
    }
  }
  const uint64_t amask = __ballot(alt);
  if (amask != 0) {   // (wave-uniform)
    uint32_t at = 0;
    if ((threadIdx.x & 63u) == 0) at = atomicAdd(a.qlen, (uint32_t)__popcll(amask));
    at = (uint32_t)__shfl((int)at, 0, 64) + lanes_below(amask);
    if (alt && at < a.qcap) a.queue[at] = (uint32_t)r;
  }
  // (the per-wave counts are hex_wide_recount_kernel's: they include both queues' results)
}

__global__ void alt_clear_kernel(AltParams a) { *a.qlen = 0; }

// One queued record, measured by the calling WAVE: _yr_scan_verify_re_match
// (scan.c:778-885) with yr_re_exec's two runs.  A match overwrites what the
// queue kernel left of the record -- its key, F, its set {mask, base 0}, the
// item count -- which is what the narrow hex path leaves; anything else
// leaves the record in the rest.
// The block of both runs is [data, data + size) and `offset` the record's
// position in it: the scanned block, or -- a batch -- the record's own buffer
// and its local offset.  Lane b is loaded only where b < max_bytes_matched, so
// no byte outside the block is read.
__device__ void alt_record(const AltTables& t, const HexWideParams& w, uint32_t r, const uint8_t* data,
                           uint64_t size, uint64_t offset, uint32_t* cls) {
  const HexMatchParams& q = w.h;
  const MatchParams& p = q.m;
  const uint32_t lane = threadIdx.x & 63u;
  const VerifyRec rec = p.recs[r];
  const AltProg prog = t.progs[rec.pool_index];
  if (prog.n_fwd == 0 || prog.n_fwd > kAltMaxInsns || prog.n_bwd > kAltMaxInsns || offset >= size)
    return;   // (never: what the measure pass appended)
  const bool dot_all = (p.pool[rec.pool_index].flags & kStrDotAll) != 0;
  const uint8_t* d = data + offset;
  AltRun run;
  // forwards: lane b holds data[offset + b]
  int maxb = (int)min<uint64_t>(size - offset, (uint64_t)kReScanLimit);
  bool valid = (int)lane < maxb;
  uint32_t c = valid ? d[lane] : 0u;
  if (!alt_load(t, prog.fwd, prog.n_fwd, c, valid, dot_all, cls, maxb, run)) return;
  uint64_t M, top;
  bool mtop;
  if (alt_sets(run, M, mtop, top) != kAltOk) return;
  if (M == 0 && !mtop) return;   // (no path to MATCH: the host verifies it and finds nothing)
  uint32_t F = 0;
  if (!alt_priority(run, F)) return;
  uint64_t B = 1;   // (no backward program: {0})
  if (prog.n_bwd == 0) {
    if (F == 0) return;
  } else {
    // backwards: lane b holds data[offset - 1 - b]
    maxb = (int)min<uint64_t>(offset, (uint64_t)kReScanLimit);
    valid = (int)lane < maxb;
    c = valid ? *(d - 1 - (int)lane) : 0u;
    if (!alt_load(t, prog.bwd, prog.n_bwd, c, valid, dot_all, cls, maxb, run)) return;
    if (alt_sets(run, B, mtop, top) != kAltOk) return;
    // (bytes_matched 64 is outside HexSet's base-0 mask.  Position 64 at any other
    // instruction died above, as the reference's fiber does: max_bytes_matched is 64)
    if (mtop || B == 0) return;
  }
  if (lane == 0) {
    p.keys[r] = (uint64_t)p.pool_string[rec.pool_index] << 32 | (offset & 0xFFFFFFFFull);
    p.meas[r] = MatchMeasure{F, 0u};
    q.sets[r] = HexSet{B, 0u, 0u};
    w.icount[r] = (uint32_t)__popcll(B);
  }
}

// One WAVE per queued record, the waves of a fixed grid striding over the queue.
__global__ __launch_bounds__(256) void alt_measure_kernel(AltParams a) {
  __shared__ uint32_t classes[4][16];
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t len = *a.qlen;
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.qlen_out = len;
  const uint32_t n = min(len, a.qcap);
  for (uint32_t slot = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave); slot < n;
       slot += gridDim.x * 4) {
    const uint32_t r = __builtin_amdgcn_readfirstlane(a.queue[slot]);
    if (r >= a.w.h.m.n) continue;   // (never)
    const MatchParams& p = a.w.h.m;
    alt_record(a.t, a.w, r, p.data, p.size, p.recs[r].offset, classes[wave]);
  }
}

// ---- The batch's alternation strings (matches.h BatchAltParams) ----

// batch_hex_measure_queue_kernel's twin (matches.hip) with the second queue, as
// alt_measure_queue_kernel is hex_measure_queue_kernel's: the record's buffer is
// searched in rec_off once, here; a record of an alternation string inside its
// buffer is a rest record for now and is appended to the alternation queue as
// the pair (record, buffer).  Every batch buffer is whole -- never a window --
// so the single-block twin's window test has no counterpart.  WIDE: the wide
// records are queued as batch_hex_measure_queue_kernel queues them; else a
// final hex string's record is measured as batch_hex_measure_kernel measures it.
template <bool WIDE>
__global__ __launch_bounds__(256) void batch_alt_measure_queue_kernel(BatchAltParams a) {
  __shared__ __attribute__((aligned(16))) uint8_t codebuf[256 * kHexCodeBytes + 16];
  const BatchHexWideParams& b = a.b;
  const HexWideParams& w = b.w;
  const MatchParams& p = w.h.m;
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool wide = false, alt = false;
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
    if (a.t.str_alt[p.pool_string[rec.pool_index]] != 0) {
      m.length = 0;
      m.xor_key = 0;
      is_match = false;
      alt = rec.offset < q.m.size;
    } else if ((q.classes & kMatchHex) && string_is_final_hex(e.flags)) {
      m.length = 0;
      m.xor_key = 0;
      const uint32_t buf = (uint32_t)(uintptr_t)(codebuf + threadIdx.x * kHexCodeBytes);
      const int v = measure_hex<WIDE>(q, e, rec.offset, buf, m, set);
      is_match = v == kHexMatch;
      wide = WIDE && v == kHexWide;
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
  if (WIDE) {
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
  }
  const uint64_t amask = __ballot(alt);
  if (amask != 0) {   // (wave-uniform)
    uint32_t at = 0;
    if ((threadIdx.x & 63u) == 0) at = atomicAdd(a.qlen, (uint32_t)__popcll(amask));
    at = (uint32_t)__shfl((int)at, 0, 64) + lanes_below(amask);
    if (alt && at < a.qcap) {
      a.queue[at] = (uint32_t)r;
      a.qbuf[at] = lo;
    }
  }
  // (the per-wave counts are hex_wide_recount_kernel's: they include both queues' results)
}

__global__ void batch_alt_clear_kernel(BatchAltParams a) { *a.qlen = 0; }

// alt_measure_kernel for a batch: one WAVE per queued pair, a fixed grid
// striding over the queue.  Record and buffer come from the queue entry, the
// buffer's bounds from starts / sizes through scalar registers (one value for
// the wave).  alt_record sees the buffer as the whole block of both runs --
// position 0 at arena + starts[k], max_bytes_matched = min(size_k - local
// offset, YR_RE_SCAN_LIMIT) forwards and min(local offset, ...) backwards --
// and loads lane b only below that bound: no byte of a gap or of a
// neighbouring buffer.
__global__ __launch_bounds__(256) void batch_alt_measure_kernel(BatchAltParams a) {
  __shared__ uint32_t classes[4][16];
  const HexWideParams& w = a.b.w;
  const MatchParams& p = w.h.m;
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t len = *a.qlen;
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.qlen_out = len;
  const uint32_t n = min(len, a.qcap);
  for (uint32_t slot = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave); slot < n;
       slot += gridDim.x * 4) {
    const uint32_t r = __builtin_amdgcn_readfirstlane(a.queue[slot]);
    const uint32_t k = __builtin_amdgcn_readfirstlane(a.qbuf[slot]);
    if (r >= p.n || k >= a.b.nbuf) continue;   // (never: what the measure pass appended)
    alt_record(a.t, w, r, p.data + a.b.starts[k], a.b.sizes[k], p.recs[r].offset, classes[wave]);
  }
}

}  // namespace

hipError_t launch_alt_measure(const AltParams& a, uint32_t waves, hipStream_t s) {
  const uint64_t n = a.w.h.m.n;
  if (n == 0 || n > kMatchMaxRecords) return n == 0 ? hipSuccess : hipErrorInvalidValue;
  if (waves == 0 || a.qcap == 0 || a.w.qcap == 0) return hipErrorInvalidValue;
  const dim3 grid((uint32_t)((n + 255) / 256));
  // (kernels, not memsets: the stage may be recorded into a graph)
  hipError_t e = launch_hex_wide_piece(a.w, waves, 0, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(alt_clear_kernel, dim3(1), dim3(1), 0, s, a);
  if (a.wide)
    hipLaunchKernelGGL(alt_measure_queue_kernel<true>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(alt_measure_queue_kernel<false>, grid, dim3(256), 0, s, a);
  hipLaunchKernelGGL(alt_measure_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.wide) {
    e = launch_hex_wide_piece(a.w, waves, 1, s);
    if (e != hipSuccess) return e;
  }
  return launch_hex_wide_piece(a.w, waves, 2, s);
}

hipError_t launch_alt_waves(const AltParams& a, uint32_t waves, hipStream_t s) {
  const uint64_t n = a.w.h.m.n;
  if (n == 0 || n > kMatchMaxRecords) return n == 0 ? hipSuccess : hipErrorInvalidValue;
  if (waves == 0 || a.qcap == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(alt_measure_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_batch_alt_waves(const BatchAltParams& a, uint32_t waves, hipStream_t s) {
  const uint64_t n = a.b.w.h.m.n;
  if (n == 0 || n > kMatchMaxRecords) return n == 0 ? hipSuccess : hipErrorInvalidValue;
  if (waves == 0 || a.qcap == 0 || a.b.nbuf == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(batch_alt_measure_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_batch_alt_measure(const BatchAltParams& a, uint32_t waves, hipStream_t s) {
  const HexWideParams& w = a.b.w;
  const uint64_t n = w.h.m.n;
  if (n == 0 || n > kMatchMaxRecords) return n == 0 ? hipSuccess : hipErrorInvalidValue;
  if (waves == 0 || a.qcap == 0 || w.qcap == 0 || a.b.nbuf == 0) return hipErrorInvalidValue;
  const dim3 grid((uint32_t)((n + 255) / 256));
  // (kernels, not memsets: the stage may be recorded into a graph)
  hipError_t e = launch_hex_wide_piece(w, waves, 0, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(batch_alt_clear_kernel, dim3(1), dim3(1), 0, s, a);
  if (a.wide)
    hipLaunchKernelGGL(batch_alt_measure_queue_kernel<true>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(batch_alt_measure_queue_kernel<false>, grid, dim3(256), 0, s, a);
  hipLaunchKernelGGL(batch_alt_measure_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.wide) {
    e = launch_batch_hex_wide_waves(a.b, waves, s);
    if (e != hipSuccess) return e;
  }
  return launch_hex_wide_piece(w, waves, 2, s);
}

}  // namespace yamd
