// gfx950 kernels of the match stage for LOOP strings (yr_amd_scanner_set_loops;
// matches.h LoopParams): text regexps with * and + whose
// programs are byte tests, SPLIT, JUMP and MATCH -- /[a-z]+\.php/, /x.*y/ --
// measured one WAVE per record.
//
// Without counters a fiber of yr_re_exec (re.c:1693-2068) is its instruction:
// two fibers at one (instruction, position) have one future and
// _yr_re_fiber_exists keeps the earlier one.  The fiber list at input position
// b is therefore a SET of at most 64 instructions, one 64-bit word, and a run
// of up to YR_RE_SCAN_LIMIT bytes is a table of 4097 such words in LDS -- the
// transpose of alternations.hip, which keeps one 64-position word per
// instruction and stops at byte 64:
//
//   * instruction i of the program lives in lane i: its decoded form and two
//     masks the host made at upload, eps (the resting instructions -- byte
//     tests and MATCH -- reachable over SPLIT / JUMP alone) and succ (eps of
//     the instruction behind a byte test);
//   * per 64-byte chunk of the run lane b loads input byte b and builds P_b,
//     bit i = "instruction i passes this byte", by running over the
//     instructions with wave-uniform operands: no transpose, no divergence;
//   * the live set A is a scalar.  A[0] = eps[entry]; A[b + 1] is the OR of
//     succ[i] over the set bits i of A[b] & P_b, a loop over the set bits
//     (s_ff1 + two v_readlane): live sets hold a handful of instructions, so
//     this is a few scalar operations per position where a cross-lane OR of 64
//     lanes costs twelve DPP steps whatever the set;
//   * backwards (EXHAUSTIVE) the positions with MATCH in A[b] are the result;
//   * forwards a descending sweep turns A[b] into R[b], the instructions of
//     A[b] that still reach MATCH (one vector AND, one compare, one ballot per
//     position), and a walk of one state (i, b) takes at every SPLIT the
//     preferred branch X iff eps[X] meets R[b]: the bytes_matched of the
//     highest-priority path that reaches MATCH, which is what yr_re_exec's
//     last write to *matches holds.
//
// One wave per workgroup: the table is 32 KiB, the class bitmaps 2 KiB, so
// four waves share a CU's LDS -- and the sweeps are serial chains on the
// scalar unit, which more waves per SIMD would not hide anyway.
//
// The batch calls (yr_amd_scanner_set_batch_loops; matches.h BatchLoopParams,
// DESIGN.md 18.11) run the same machinery per buffer: the queue holds (record,
// buffer) pairs, loop_record gets the buffer as its block, and the table is
// dynamic LDS sized to the batch's largest buffer.
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
  // (a writelane with wave-uniform v and i, as a select on the lane id)
  const bool mine = (threadIdx.x & 63u) == i;
  lo = mine ? (uint32_t)v : lo;
  hi = mine ? (uint32_t)(v >> 32) : hi;
}
// (one wave writes and reads its LDS words: LDS serves a wave's requests in order)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32 |
         (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// One program in the wave's registers: instruction i in lane i
// (op | next << 8 | target << 16 | flag << 24; a | b << 16), its eps and succ.
struct LoopProg {
  uint32_t ilo, ihi;
  uint32_t elo, ehi;
  uint32_t slo, shi;
  uint32_t n;
  uint64_t match;   // bit i: instruction i is MATCH
};
struct LoopDecoded {
  uint32_t op, next, target, flag;
};
__device__ __forceinline__ LoopDecoded loop_decode(const LoopProg& g, uint32_t i) {
  const uint32_t lo = lane_read(g.ilo, i);
  return LoopDecoded{lo & 0xFFu, (lo >> 8) & 0xFFu, (lo >> 16) & 0xFFu, lo >> 24};
}

// The program's lanes, and the bitmaps of its CLASS instructions in the wave's
// LDS words cls[64][kLoopClassWords], by instruction.
__device__ void loop_load(const LoopTables& t, uint32_t first, uint32_t n, uint32_t* cls, LoopProg& g) {
  const uint32_t lane = threadIdx.x & 63u;
  g.n = n;
  g.ilo = g.ihi = g.elo = g.ehi = g.slo = g.shi = 0;
  uint32_t op = 0xFFu;
  wave_sync();   // (the words may still be read for the program before)
  if (lane < n) {
    const AltInsn in = t.insns[first + lane];
    op = in.op;
    g.ilo = in.op | (uint32_t)in.next << 8 | (uint32_t)in.target << 16 | (uint32_t)in.flag << 24;
    g.ihi = in.a | (uint32_t)in.b << 16;
    const uint64_t eps = t.masks[2 * (uint64_t)(first + lane)];
    const uint64_t succ = t.masks[2 * (uint64_t)(first + lane) + 1];
    g.elo = (uint32_t)eps;
    g.ehi = (uint32_t)(eps >> 32);
    g.slo = (uint32_t)succ;
    g.shi = (uint32_t)(succ >> 32);
    if (op == kAltClass)
      for (uint32_t w = 0; w < kLoopClassWords; ++w)
        cls[lane * kLoopClassWords + w] = t.classes[(uint64_t)g.ihi * kLoopClassWords + w];
  }
  g.match = __ballot(op == kAltMatch);
  wave_sync();
}

// P of this lane's input byte c (valid: the byte exists, its position is
// below max_bytes_matched): bit i = byte test i passes.  false: an instruction
// the host never emits.
__device__ bool loop_pass(const LoopProg& g, uint32_t c, bool valid, bool dot_all, const uint32_t* cls,
                          uint32_t& plo, uint32_t& phi) {
  plo = phi = 0;
  for (uint32_t i = 0; i < g.n; ++i) {
    const LoopDecoded d = loop_decode(g, i);
    bool ok;
    switch (d.op) {
      case kAltByte: {
        const uint32_t ab = lane_read(g.ihi, i);
        ok = ((c & (ab >> 16)) == (ab & 0xFFFFu)) != (d.flag != 0);
        break;
      }
      case kAltAny: ok = dot_all || c != 0x0Au; break;
      case kAltClass:
        ok = (((cls[i * kLoopClassWords + (c >> 5)] >> (c & 31u)) & 1u) != 0) != (d.flag != 0);
        break;
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
    const uint32_t bit = (ok && valid) ? 1u << (i & 31u) : 0u;
    if (i < 32) plo |= bit; else phi |= bit;   // (wave-uniform)
  }
  return true;
}

// This lane's byte of the chunk at c0: forwards d[c0 + lane], backwards
// d[-1 - (c0 + lane)], only below max_bytes_matched -- which is at most the
// bytes the block has on that side, so no byte outside the block is read.
template <bool FWD>
__device__ __forceinline__ uint32_t loop_byte(const uint8_t* d, uint32_t c0, int maxb, bool& valid) {
  const uint32_t pos = c0 + (threadIdx.x & 63u);
  valid = (int)pos < maxb;
  if (!valid) return 0u;
  return FWD ? d[pos] : *(d - 1 - (int64_t)pos);
}

// The ascending sweep from A[0] = eps[entry] until the set is empty or
// position max_bytes_matched has been seen (a byte test there dies in the
// reference's prolog; MATCH there matches).  Forwards A[b] goes to tab[b] for
// b = 0 .. last (last <= maxb <= YR_RE_SCAN_LIMIT: inside the table's 4097
// words).  Backwards the positions with MATCH live are the result, settled as
// {mask, base} while they span fewer than 64 positions.  false: the record
// stays in the rest.
template <bool FWD>
__device__ bool loop_sweep(const LoopProg& g, const uint8_t* d, int maxb, bool dot_all, const uint32_t* cls,
                           uint64_t* tab, uint32_t& last, HexSet& B) {
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t A = lane_get(g.elo, g.ehi, 0);
  if (A == 0) return false;   // (never: the entry reaches a resting instruction)
  uint32_t b = 0;
  B = HexSet{0ull, 0u, 0u};
  for (uint32_t c0 = 0; A != 0; c0 += 64) {
    bool valid;
    const uint32_t c = loop_byte<FWD>(d, c0, maxb, valid);
    uint32_t plo, phi;
    if (!loop_pass(g, c, valid, dot_all, cls, plo, phi)) return false;
    for (uint32_t k = 0; k < 64 && A != 0; ++k) {
      b = c0 + k;
      if (FWD) {
        if (lane == 0) tab[b] = A;
      } else if ((A & g.match) != 0) {
        if (B.mask == 0) B.base = b;
        if (b - B.base + 1 >= 64) return false;   // (spans 64 positions or more)
        B.mask |= 1ull << (b - B.base);
      }
      last = b;
      if ((int)b >= maxb) {   // (position max_bytes_matched: nothing reads a byte)
        A = 0;
        break;
      }
      uint64_t x = A & lane_get(plo, phi, k);
      A = 0;
      while (x != 0) {
        const uint32_t i = (uint32_t)__builtin_ctzll(x);
        x &= x - 1;
        A |= lane_get(g.slo, g.shi, i);
      }
    }
  }
  return true;
}

// The descending sweep over tab[0 .. last]: A[b] becomes R[b], its instructions
// that still reach MATCH -- MATCH itself, and byte test i iff it passes byte b
// and succ[i] meets R[b + 1].
__device__ bool loop_reach(const LoopProg& g, const uint8_t* d, int maxb, bool dot_all, const uint32_t* cls,
                           uint64_t* tab, uint32_t last) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t succ = (uint64_t)g.shi << 32 | g.slo;
  uint64_t Rn = 0;
  wave_sync();
  for (int c0 = (int)(last & ~63u); c0 >= 0; c0 -= 64) {
    bool valid;
    const uint32_t c = loop_byte<true>(d, (uint32_t)c0, maxb, valid);
    uint32_t plo, phi;
    if (!loop_pass(g, c, valid, dot_all, cls, plo, phi)) return false;
    const uint32_t pos = (uint32_t)c0 + lane;
    const uint64_t a = pos <= last ? tab[pos] : 0ull;
    const uint32_t alo = (uint32_t)a, ahi = (uint32_t)(a >> 32);
    uint32_t rlo = 0, rhi = 0;
    for (int k = (int)min(63u, last - (uint32_t)c0); k >= 0; --k) {
      const uint64_t C = __ballot((succ & Rn) != 0);
      Rn = lane_get(alo, ahi, (uint32_t)k) & (g.match | (lane_get(plo, phi, (uint32_t)k) & C));
      lane_set(rlo, rhi, (uint32_t)k, Rn);
    }
    if (pos <= last) tab[pos] = (uint64_t)rhi << 32 | rlo;
  }
  wave_sync();
  return true;
}

// The priority walk from (entry, 0): F = bytes_matched of the highest-priority
// path to MATCH.  A byte test in R[b] leads to R[b + 1], so b stays <= last;
// within one position the SPLIT / JUMP edges form a DAG (the class), so the
// steps are bounded by positions x instructions.
__device__ bool loop_walk(const LoopProg& g, const uint64_t* tab, uint32_t last, uint32_t& F) {
  uint32_t i = 0, b = 0;
  uint64_t R = uniform64(tab[0]);
  if ((lane_get(g.elo, g.ehi, 0) & R) == 0) return false;   // no path to MATCH
  for (uint32_t step = 0; step < kLoopPositions * kAltMaxInsns; ++step) {
    const LoopDecoded d = loop_decode(g, i);
    if (d.op == kAltMatch) {
      F = b;
      return true;
    }
    if (d.op <= kAltDigit) {
      if (++b > last) return false;   // (never)
      R = uniform64(tab[b]);
      i = d.next;
    } else if (d.op == kAltJump) {
      i = d.target;
    } else if (d.op == kAltSplit) {
      const uint32_t pref = d.flag ? d.target : d.next, other = d.flag ? d.next : d.target;
      i = (lane_get(g.elo, g.ehi, pref) & R) != 0 ? pref : other;
    } else {
      return false;   // (never)
    }
  }
  return false;
}

// alt_measure_queue_kernel's twin (alternations.hip) with the third queue: a
// record of a loop string all of whose bytes are in the window is a rest record
// for now and its index is appended to the loop queue; alternation records
// (alts) and wide records (WIDE) are queued as there.
template <bool WIDE>
__global__ __launch_bounds__(256) void loop_measure_queue_kernel(LoopParams l) {
  __shared__ __attribute__((aligned(16))) uint8_t codebuf[256 * kHexCodeBytes + 16];
  const AltParams& a = l.a;
  const HexWideParams& w = a.w;
  const HexMatchParams& q = w.h;
  const MatchParams& p = q.m;
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool wide = false, alt = false, loop = false;
  if (r < p.n) {
    const VerifyRec rec = p.recs[r];
    const DevPoolRec e = p.pool[rec.pool_index];
    const uint32_t str = p.pool_string[rec.pool_index];
    MatchMeasure m;
    HexSet set{1ull, 0u, 0u};
    bool is_match;
    const bool is_loop = l.t.str_loop[str] != 0;
    if (is_loop || (l.alts != 0 && a.t.str_alt[str] != 0)) {
      m.length = 0;
      m.xor_key = 0;
      is_match = false;
      bool in = rec.offset < p.size;
      // (measure_hex's bounds: every byte either run may read)
      if (in && (p.win_lo != 0 || p.win_hi != p.size)) {
        const uint64_t need_lo = rec.offset - min<uint64_t>(rec.offset, (uint64_t)kReScanLimit);
        const uint64_t need_hi = min<uint64_t>(p.size, rec.offset + (uint64_t)kReScanLimit);
        in = need_lo >= p.win_lo && need_hi <= p.win_hi;
      }
      loop = in && is_loop;
      alt = in && !is_loop;
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
    const uint32_t string = is_match ? str : p.n_strings;
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
  if (amask != 0) {   // (wave-uniform; only with alts)
    uint32_t at = 0;
    if ((threadIdx.x & 63u) == 0) at = atomicAdd(a.qlen, (uint32_t)__popcll(amask));
    at = (uint32_t)__shfl((int)at, 0, 64) + lanes_below(amask);
    if (alt && at < a.qcap) a.queue[at] = (uint32_t)r;
  }
  const uint64_t lmask = __ballot(loop);
  if (lmask != 0) {   // (wave-uniform)
    uint32_t at = 0;
    if ((threadIdx.x & 63u) == 0) at = atomicAdd(l.qlen, (uint32_t)__popcll(lmask));
    at = (uint32_t)__shfl((int)at, 0, 64) + lanes_below(lmask);
    if (loop && at < l.qcap) l.queue[at] = (uint32_t)r;
  }
  // (the per-wave counts are hex_wide_recount_kernel's: they include all queues' results)
}

__global__ void loop_clear_kernel(LoopParams l) {
  *l.qlen = 0;
  if (l.alts != 0) *l.a.qlen = 0;
}

// One queued record, measured by the calling WAVE: _yr_scan_verify_re_match
// (scan.c:778-885) with yr_re_exec's two runs.  A match overwrites what the
// queue kernel left of the record -- its key, F, its set {mask, base}, the item
// count -- which is what the narrow hex path leaves; anything else leaves the
// record in the rest.
// The block of both runs is [data, data + size) and `offset` the record's
// position in it: the scanned block, or -- a batch -- the record's own buffer
// and its local offset.  loop_byte reads only below max_bytes_matched, so no
// byte outside the block is read.  tab holds `words` words: a forward run whose
// last position max_bytes_matched is not inside them leaves the record in the
// rest before anything is written.
__device__ void loop_record(const LoopTables& t, const HexWideParams& w, uint32_t r, const uint8_t* data,
                            uint64_t size, uint64_t offset, uint32_t* cls, uint64_t* tab, uint32_t words) {
  const HexMatchParams& q = w.h;
  const MatchParams& p = q.m;
  const VerifyRec rec = p.recs[r];
  const AltProg prog = t.progs[rec.pool_index];
  if (prog.n_fwd == 0 || prog.n_fwd > kAltMaxInsns || prog.n_bwd > kAltMaxInsns || offset >= size)
    return;   // (never: what the measure pass appended)
  const bool dot_all = (p.pool[rec.pool_index].flags & kStrDotAll) != 0;
  const uint8_t* d = data + offset;
  LoopProg g;
  HexSet B;
  uint32_t last = 0, F = 0;
  int maxb = (int)min<uint64_t>(size - offset, (uint64_t)kReScanLimit);
  if ((uint32_t)maxb >= words) return;   // (never: the host sizes the table to the largest buffer)
  loop_load(t, prog.fwd, prog.n_fwd, cls, g);
  if (!loop_sweep<true>(g, d, maxb, dot_all, cls, tab, last, B)) return;
  if (!loop_reach(g, d, maxb, dot_all, cls, tab, last)) return;
  if (!loop_walk(g, tab, last, F)) return;   // (no path to MATCH: the host verifies it and finds nothing)
  if (prog.n_bwd == 0) {
    if (F == 0) return;
    B = HexSet{1ull, 0u, 0u};
  } else {
    maxb = (int)min<uint64_t>(offset, (uint64_t)kReScanLimit);
    loop_load(t, prog.bwd, prog.n_bwd, cls, g);
    if (!loop_sweep<false>(g, d, maxb, dot_all, cls, tab, last, B)) return;
    if (B.mask == 0) return;
  }
  if ((threadIdx.x & 63u) == 0) {
    p.keys[r] = (uint64_t)p.pool_string[rec.pool_index] << 32 | (offset & 0xFFFFFFFFull);
    p.meas[r] = MatchMeasure{F, 0u};
    q.sets[r] = B;
    w.icount[r] = (uint32_t)__popcll(B.mask);
  }
}

// One WAVE (one workgroup) per queued record, a fixed grid striding over the queue.
__global__ __launch_bounds__(64) void loop_measure_kernel(LoopParams l) {
  __shared__ uint64_t tab[kLoopPositions];
  __shared__ uint32_t classes[kAltMaxInsns * kLoopClassWords];
  const uint32_t len = *l.qlen;
  if (blockIdx.x == 0 && threadIdx.x == 0) *l.qlen_out = len;
  const uint32_t n = min(len, l.qcap);
  for (uint32_t slot = blockIdx.x; slot < n; slot += gridDim.x) {
    const uint32_t r = __builtin_amdgcn_readfirstlane(l.queue[slot]);
    if (r >= l.a.w.h.m.n) continue;   // (never)
    const MatchParams& p = l.a.w.h.m;
    loop_record(l.t, l.a.w, r, p.data, p.size, p.recs[r].offset, classes, tab, kLoopPositions);
  }
}

// hex_unique_kernel's pass 1 (matches.hip) with replace_if_exists: the run of
// items with one key is in record order (the sort is stable); a greedy loop
// string takes its last item's record, everything else the first's.
__global__ __launch_bounds__(256) void loop_unique_kernel(LoopUniqueParams u) {
  const HexMatchParams& q = u.h;
  const MatchParams& p = q.m;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool keep = false;
  uint64_t key = 0;
  if (i < q.n_items) {
    key = p.sorted_keys[i];
    keep = (uint32_t)(key >> 32) < p.n_strings && (i == 0 || p.sorted_keys[i - 1] != key);
  }
  const uint64_t mask = __ballot(keep);
  if (!keep) return;
  uint64_t from = i;
  if (u.str_loop[(uint32_t)(key >> 32)] == (kLoopString | kLoopGreedy))
    while (from + 1 < q.n_items && p.sorted_keys[from + 1] == key) ++from;
  const uint32_t r = p.sorted_index[from];
  const MatchMeasure m = p.meas[r];
  const VerifyRec rec = p.recs[r];
  MatchRec o;
  o.offset = key & 0xFFFFFFFFull;
  o.string = (uint32_t)(key >> 32);
  o.length = m.length + (uint32_t)((rec.offset & 0xFFFFFFFFull) - o.offset);
  o.xor_key = m.xor_key;
  o.pool_index = rec.pool_index;
  const uint64_t g = i / kGroup;
  p.out[q.uchunk_off[g / kChunkGroups] + q.ublock_off[g] + lanes_below(mask)] = o;
}

// ---- The batch's loop strings (matches.h BatchLoopParams) ----

// batch_alt_measure_queue_kernel's twin (alternations.hip) with the third
// queue, as loop_measure_queue_kernel is alt_measure_queue_kernel's: the
// record's buffer is searched in rec_off once, here; a record of a loop string
// inside its buffer is a rest record for now and is appended to the loop queue
// as the pair (record, buffer); alternation records (alts) and wide records
// (WIDE) are queued as there.  Every batch buffer is whole -- never a window.
template <bool WIDE>
__global__ __launch_bounds__(256) void batch_loop_measure_queue_kernel(BatchLoopParams l) {
  __shared__ __attribute__((aligned(16))) uint8_t codebuf[256 * kHexCodeBytes + 16];
  const BatchAltParams& a = l.a;
  const BatchHexWideParams& b = a.b;
  const HexWideParams& w = b.w;
  const MatchParams& p = w.h.m;
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool wide = false, alt = false, loop = false;
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
    const uint32_t str = p.pool_string[rec.pool_index];
    MatchMeasure m;
    HexSet set{1ull, 0u, 0u};
    bool is_match;
    const bool is_loop = l.t.str_loop[str] != 0;
    if (is_loop || (l.alts != 0 && a.t.str_alt[str] != 0)) {
      m.length = 0;
      m.xor_key = 0;
      is_match = false;
      const bool in = rec.offset < q.m.size;
      loop = in && is_loop;
      alt = in && !is_loop;
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
    const uint32_t string = is_match ? str : p.n_strings;
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
  if (amask != 0) {   // (wave-uniform; only with alts)
    uint32_t at = 0;
    if ((threadIdx.x & 63u) == 0) at = atomicAdd(a.qlen, (uint32_t)__popcll(amask));
    at = (uint32_t)__shfl((int)at, 0, 64) + lanes_below(amask);
    if (alt && at < a.qcap) {
      a.queue[at] = (uint32_t)r;
      a.qbuf[at] = lo;
    }
  }
  const uint64_t lmask = __ballot(loop);
  if (lmask != 0) {   // (wave-uniform)
    uint32_t at = 0;
    if ((threadIdx.x & 63u) == 0) at = atomicAdd(l.qlen, (uint32_t)__popcll(lmask));
    at = (uint32_t)__shfl((int)at, 0, 64) + lanes_below(lmask);
    if (loop && at < l.qcap) {
      l.queue[at] = (uint32_t)r;
      l.qbuf[at] = lo;
    }
  }
  // (the per-wave counts are hex_wide_recount_kernel's: they include all queues' results)
}

__global__ void batch_loop_clear_kernel(BatchLoopParams l) {
  *l.qlen = 0;
  if (l.alts != 0) *l.a.qlen = 0;
}

// loop_measure_kernel for a batch: one WAVE (one workgroup) per queued pair, a
// fixed grid striding over the queue.  Record and buffer come from the queue
// entry, the buffer's bounds from starts / sizes through scalar registers.
// loop_record sees the buffer as the whole block of both runs, so a run reads
// at most min(sizes[k], YR_RE_SCAN_LIMIT) bytes of it and its positions are 0
// .. that: the table is the launch's dynamic LDS, l.words = min(largest buffer,
// YR_RE_SCAN_LIMIT) + 1 words the host sized to the batch -- 32 KiB only where
// a buffer is 4 KiB or more, a quarter of that for 1 KiB buffers, so that more
// workgroups share a CU's LDS.  l.words is the hard bound: loop_record leaves a
// record whose run would pass it in the rest without a write.
__global__ __launch_bounds__(64) void batch_loop_measure_kernel(BatchLoopParams l) {
  extern __shared__ uint64_t batch_tab[];   // [l.words]
  __shared__ uint32_t classes[kAltMaxInsns * kLoopClassWords];
  const BatchHexWideParams& b = l.a.b;
  const MatchParams& p = b.w.h.m;
  const uint32_t len = *l.qlen;
  if (blockIdx.x == 0 && threadIdx.x == 0) *l.qlen_out = len;
  const uint32_t n = min(len, l.qcap);
  for (uint32_t slot = blockIdx.x; slot < n; slot += gridDim.x) {
    const uint32_t r = __builtin_amdgcn_readfirstlane(l.queue[slot]);
    const uint32_t k = __builtin_amdgcn_readfirstlane(l.qbuf[slot]);
    if (r >= p.n || k >= b.nbuf) continue;   // (never: what the measure pass appended)
    loop_record(l.t, b.w, r, p.data + b.starts[k], b.sizes[k], p.recs[r].offset, classes, batch_tab,
                l.words);
  }
}

// batch_hex_unique_kernel<1> (matches.hip) with replace_if_exists, as
// loop_unique_kernel: the run of items with one (buffer, string, offset) has
// one key and one buf[sorted_index[.]] and is in record order (the sort is
// stable); a greedy loop string takes its last item's record, everything else
// the first's.  The run ends at another key or another buffer: two buffers
// with the same bytes at the same local offset never merge.
__global__ __launch_bounds__(256) void batch_loop_unique_kernel(BatchLoopUniqueParams u) {
  const BatchHexParams& b = u.b;
  const HexMatchParams& q = b.h;
  const MatchParams& p = q.m;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool keep = false;
  uint64_t key = 0;
  uint32_t k = 0;
  if (i < q.n_items) {
    key = p.sorted_keys[i];
    k = b.buf[p.sorted_index[i]];
    keep = (uint32_t)(key >> 32) < p.n_strings &&
           (i == 0 || p.sorted_keys[i - 1] != key || b.buf[p.sorted_index[i - 1]] != k);
  }
  const uint64_t mask = __ballot(keep);
  if (!keep) return;
  uint64_t from = i;
  if (u.str_loop[(uint32_t)(key >> 32)] == (kLoopString | kLoopGreedy))
    while (from + 1 < q.n_items && p.sorted_keys[from + 1] == key && b.buf[p.sorted_index[from + 1]] == k)
      ++from;
  const uint32_t r = p.sorted_index[from];
  const MatchMeasure m = p.meas[r];
  const VerifyRec rec = p.recs[r];
  MatchRec o;
  o.offset = key & 0xFFFFFFFFull;
  o.string = (uint32_t)(key >> 32);
  o.length = m.length + (uint32_t)((rec.offset & 0xFFFFFFFFull) - o.offset);
  o.xor_key = m.xor_key;
  o.pool_index = rec.pool_index;
  const uint64_t g = i / kGroup;
  p.out[q.uchunk_off[g / kChunkGroups] + q.ublock_off[g] + lanes_below(mask)] = o;
}

}  // namespace

hipError_t launch_loop_measure(const LoopParams& l, uint32_t waves, hipStream_t s) {
  const AltParams& a = l.a;
  const uint64_t n = a.w.h.m.n;
  if (n == 0 || n > kMatchMaxRecords) return n == 0 ? hipSuccess : hipErrorInvalidValue;
  if (waves == 0 || l.qcap == 0 || a.w.qcap == 0 || (l.alts != 0 && a.qcap == 0))
    return hipErrorInvalidValue;
  const dim3 grid((uint32_t)((n + 255) / 256));
  // (kernels, not memsets: the stage may be recorded into a graph)
  hipError_t e = launch_hex_wide_piece(a.w, waves, 0, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(loop_clear_kernel, dim3(1), dim3(1), 0, s, l);
  if (a.wide)
    hipLaunchKernelGGL(loop_measure_queue_kernel<true>, grid, dim3(256), 0, s, l);
  else
    hipLaunchKernelGGL(loop_measure_queue_kernel<false>, grid, dim3(256), 0, s, l);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (l.alts != 0) {
    e = launch_alt_waves(a, waves, s);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(loop_measure_kernel, dim3(waves), dim3(64), 0, s, l);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.wide) {
    e = launch_hex_wide_piece(a.w, waves, 1, s);
    if (e != hipSuccess) return e;
  }
  return launch_hex_wide_piece(a.w, waves, 2, s);
}

hipError_t launch_loop_unique(const LoopUniqueParams& u, hipStream_t s) {
  if (u.h.n_items == 0) return hipSuccess;
  hipLaunchKernelGGL(loop_unique_kernel, dim3((uint32_t)((u.h.n_items + 255) / 256)), dim3(256), 0, s, u);
  return hipGetLastError();
}

hipError_t launch_batch_loop_measure(const BatchLoopParams& l, uint32_t waves, hipStream_t s) {
  const BatchAltParams& a = l.a;
  const HexWideParams& w = a.b.w;
  const uint64_t n = w.h.m.n;
  if (n == 0 || n > kMatchMaxRecords) return n == 0 ? hipSuccess : hipErrorInvalidValue;
  if (waves == 0 || l.qcap == 0 || w.qcap == 0 || a.b.nbuf == 0 || (l.alts != 0 && a.qcap == 0) ||
      l.words < 2 || l.words > kLoopPositions)
    return hipErrorInvalidValue;
  const dim3 grid((uint32_t)((n + 255) / 256));
  // (kernels, not memsets: the stage may be recorded into a graph)
  hipError_t e = launch_hex_wide_piece(w, waves, 0, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(batch_loop_clear_kernel, dim3(1), dim3(1), 0, s, l);
  if (a.wide)
    hipLaunchKernelGGL(batch_loop_measure_queue_kernel<true>, grid, dim3(256), 0, s, l);
  else
    hipLaunchKernelGGL(batch_loop_measure_queue_kernel<false>, grid, dim3(256), 0, s, l);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (l.alts != 0) {
    e = launch_batch_alt_waves(a, waves, s);
    if (e != hipSuccess) return e;
  }
  // (the table: l.words words of dynamic LDS, at most 32 KiB + 8 beside the 2 KiB of bitmaps)
  hipLaunchKernelGGL(batch_loop_measure_kernel, dim3(waves), dim3(64), l.words * sizeof(uint64_t), s, l);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.wide) {
    e = launch_batch_hex_wide_waves(a.b, waves, s);
    if (e != hipSuccess) return e;
  }
  return launch_hex_wide_piece(w, waves, 2, s);
}

hipError_t launch_batch_loop_unique(const BatchLoopUniqueParams& u, hipStream_t s) {
  const uint64_t n = u.b.h.n_items;
  if (n == 0 || n > kMatchMaxRecords) return n == 0 ? hipSuccess : hipErrorInvalidValue;
  hipLaunchKernelGGL(batch_loop_unique_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, u);
  return hipGetLastError();
}

}  // namespace yamd
