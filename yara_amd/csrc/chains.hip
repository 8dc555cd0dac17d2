// gfx950 kernels that settle chained hex strings in the final-match stage
// (yr_amd_scanner_set_chains; matches.h ChainParams).
//
// libyara reports a chain S0 <- S1 <- ... <- Sn-1 as matches of its head S0.
// _yr_scan_verify_chained_string_match (scan.c:406-632) assembles them from the
// parts' matches as they arrive: per non-tail part a list of UNCONFIRMED
// matches ascending by offset, pruned as later parts match, and on every tail
// match a marking of chain lengths from the tail down and a sweep that moves
// the head's fully chained entries to its match list.  The result depends on
// the order of the calls, so the stage restates the procedure itself:
//
//   1. chain_events_kernel, one lane per record: a record of a settled chain's
//      part is measured as the hex stage measures a final string (the literal
//      comparisons, the 64-position fast_re_set walk) and becomes one EVENT
//      {level, offset, length}; a record that is not exactly one event (two
//      backward results, a set past the window, no forward program) makes its
//      chain DIRTY.  chain_mark_kernel then takes the events of clean chains
//      out of the rest and hands the stable sort its keys: the chain.
//   2. the stage's stable radix sort groups the events by chain, in record
//      order; the per-string event counts, scanned, place every string's
//      unconfirmed list in a workspace it cannot overflow.
//   3. chain_replay_kernel, one WAVE per chain: it walks the chain's events in
//      order.  A list is four parallel arrays (offset, length, chain_length,
//      record); lane l of a step holds entry b + l, and every list operation
//      of the reference is a sweep of such steps decided by ballots.  Chains
//      whose lists fit the wave's LDS share keep them there, the others in the
//      workspace (L2).  Confirmed heads leave as items {head << 32 | offset,
//      the head's record}; the match length goes to the record's measure, so
//      the items join the hex stage's sort and unique pass as they are.
//
// A wave touches no other chain's state; the only atomics are the dirty flags,
// the per-string counts and the item counter.
//
// The batch (yr_amd_scanner_set_batch_chains; BatchChainParams, DESIGN.md
// 18.7) replays the same procedure -- the same device functions -- one wave per
// (buffer, chain) group found in the sorted stream of events.
#include "internal.h"
#include "matches.h"
#include "match_measure.h"

namespace yamd {

namespace {

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
// Lane `lane`'s v (lane wave-uniform).
__device__ __forceinline__ uint32_t lane_of(uint32_t v, uint32_t lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)uni(lane));
}
__device__ __forceinline__ uint64_t str_offset(const ChainParams& c, uint32_t k) {
  return c.str_chunk[k / kChunkGroups] + c.str_off[k];
}

__global__ __launch_bounds__(256) void chain_clear_kernel(ChainParams c) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= c.h.m.n_strings) c.str_off[i] = 0;
  if (i < c.t.n_chains) {
    c.dirty[i] = 0;
    c.cbegin[i] = 0;
    c.cend[i] = 0;
  }
  if (i == 0) *c.item_count = 0;
}

// hex_measure_kernel's view of a record, the chain bits masked off its flags:
// what _yr_scan_match_callback hands to the chain assembly for this call.
__global__ __launch_bounds__(256) void chain_events_kernel(ChainParams c) {
  __shared__ __attribute__((aligned(16))) uint8_t codebuf[256 * kHexCodeBytes + 16];
  const HexMatchParams& q = c.h;
  const MatchParams& p = q.m;
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.n) return;
  const VerifyRec rec = p.recs[r];
  const uint32_t string = p.pool_string[rec.pool_index];
  const uint32_t chain = string < p.n_strings ? c.t.chain_of[string] : kNoChain;
  uint32_t ev = c.t.n_chains;
  if (chain != kNoChain && ((c.t.settled[chain] >> (q.classes >> 1)) & 1u)) {
    DevPoolRec e = p.pool[rec.pool_index];
    e.flags &= ~(kStrChainPart | kStrChainTail);
    MatchMeasure m{0, 0};
    uint64_t offset = rec.offset;
    bool event = false, dirty = false;
    if (string_is_final(e.flags)) {
      event = measure(p, e, rec.offset, m);
    } else {
      HexSet set{1ull, 0u, 0u};
      const uint32_t buf = (uint32_t)(uintptr_t)(codebuf + threadIdx.x * kHexCodeBytes);
      const int v = measure_hex(q, e, rec.offset, buf, m, set);
      if (v == kHexMatch && m.length != 0) {
        // one callback per backward result, in an order that is not restated
        dirty = (set.mask & (set.mask - 1)) != 0;
        const uint32_t B = set.base + (uint32_t)__builtin_ctzll(set.mask);
        offset -= B;   // (B <= min(offset, YR_RE_SCAN_LIMIT))
        m.length += B;
        event = !dirty;
      } else {
        dirty = v == kHexUndecided;
      }
    }
    if (dirty) atomicOr(&c.dirty[chain], 1u);
    if (event) {
      ev = chain;
      c.ev_level[r] = c.t.level_of[string];
      c.ev_offset[r] = (uint32_t)offset;   // (below the block's size, at most 2^32)
      c.ev_length[r] = m.length;
      atomicAdd(reinterpret_cast<unsigned long long*>(c.str_off + string), 1ull);
    }
  }
  c.rchain[r] = ev;
}

// The dirty flags are complete: an event of a clean chain leaves the rest (key
// string field n_strings + 1, no item), one of a dirty chain is no event.  The
// per-wave rest counts again, as the measure pass wrote them.
__global__ __launch_bounds__(256) void chain_mark_kernel(ChainParams c) {
  const MatchParams& p = c.h.m;
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool rest = false;
  if (r < p.n) {
    uint32_t ev = c.rchain[r];
    uint64_t key = p.keys[r];
    if (ev < c.t.n_chains) {
      if (c.dirty[ev] != 0) {
        ev = c.t.n_chains;
        c.rchain[r] = ev;
      } else {
        key = (uint64_t)(p.n_strings + 1) << 32 | (key & 0xFFFFFFFFull);
        p.keys[r] = key;
        c.h.sets[r] = HexSet{0ull, 0u, 0u};
      }
    }
    c.skeys[r] = ev;
    c.sindex[r] = (uint32_t)r;
    rest = (uint32_t)(key >> 32) == p.n_strings;
  }
  const uint64_t mask = __ballot(rest);
  if ((threadIdx.x & 63u) == 0 && r < p.n) p.block_off[r / kGroup] = (uint64_t)__popcll(mask);
}

// One lane per sorted entry: where its chain's run begins and ends.
__global__ __launch_bounds__(256) void chain_bounds_kernel(ChainParams c) {
  const uint64_t n = c.h.m.n;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = c.sorted_keys[i];
  if (k >= c.t.n_chains) return;
  if (i == 0 || c.sorted_keys[i - 1] != k) c.cbegin[k] = (uint32_t)i;
  if (i + 1 == n || c.sorted_keys[i + 1] != k) c.cend[k] = (uint32_t)(i + 1);
}

constexpr uint32_t kChainWaves = 4;          // waves per workgroup, a chain each
constexpr uint32_t kChainLdsEntries = 512;   // a wave's LDS share: 4 x 2 KiB
constexpr uint32_t kChainNew = 0x80000000u;  // chain_length: marked by the event under way

// A chain's lists: flat pointers into the wave's LDS share or the workspace.
struct Lists {
  uint32_t* off;
  uint32_t* len;
  uint32_t* cl;
  uint32_t* rec;
};

// Stores of one sweep are read by other lanes in the next: the wave's own
// memory operations in order, for LDS and for L2 alike.
__device__ __forceinline__ void lists_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// scan.c:465-498: the walk over the preceding part's list [base, base + n) for
// a match at moff.  Entries that are too far from `lowest` are removed up to
// the first entry in the gap; `found`: there is one.  Returns the new length.
__device__ uint32_t chain_prune(const Lists& L, uint32_t base, uint32_t n, int64_t moff,
                                int64_t lowest, int64_t gmin, int64_t gmax, bool& found) {
  const uint32_t lane = threadIdx.x & 63u;
  found = false;
  uint32_t w = 0;   // entries kept so far
  for (uint32_t b = 0; b < n; b += 64) {
    const uint32_t i = b + lane;
    const bool v = i < n;
    uint32_t o = 0, l = 0, cl = 0, rc = 0;
    if (v) {
      o = L.off[base + i];
      l = L.len[base + i];
      cl = L.cl[base + i];
      rc = L.rec[base + i];
    }
    const int64_t end = (int64_t)o + (int64_t)l;
    bool far = v && !found && end + gmax < lowest;
    const bool gap = v && !found && !far && end + gmax >= moff && end + gmin <= moff;
    const uint64_t G = __ballot(gap);
    if (G != 0) {   // the walk breaks here: later entries stay
      far = far && lane < (uint32_t)__builtin_ctzll(G);
      found = true;
    }
    const bool keep = v && !far;
    const uint64_t K = __ballot(keep);
    const uint32_t at = w + lanes_below(K);
    if (keep && at != i) {   // (at <= i: below what later steps read)
      L.off[base + at] = o;
      L.len[base + at] = l;
      L.cl[base + at] = cl;
      L.rec[base + at] = rc;
    }
    w += (uint32_t)__popcll(K);
    if (found && w == min(b + 64, n)) return n;   // nothing removed: the list is as it was
  }
  lists_fence();
  return w;
}

// _yr_scan_add_match_to_list on an unconfirmed list: ascending, a second entry
// at an offset is dropped.  Returns the new length.
__device__ uint32_t chain_insert(const Lists& L, uint32_t base, uint32_t n, uint32_t moff,
                                 uint32_t mlen, uint32_t mrec) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t at = n;
  if (n != 0 && uni(L.off[base + n - 1]) >= moff) {
    at = 0;
    bool dup = false;
    for (uint32_t b = 0; b < n; b += 64) {
      const uint32_t i = b + lane;
      const uint32_t o = i < n ? L.off[base + i] : 0xFFFFFFFFu;
      at += (uint32_t)__popcll(__ballot(i < n && o < moff));
      dup = dup || __ballot(i < n && o == moff) != 0;
    }
    if (dup) return n;
    // [at, n) one up, from the top: a step reads its 64 entries, then writes them
    for (uint32_t b = (n - 1) & ~63u;; b -= 64) {
      const uint32_t i = b + lane;
      const bool v = i < n && i >= at;
      uint32_t o = 0, l = 0, cl = 0, rc = 0;
      if (v) {
        o = L.off[base + i];
        l = L.len[base + i];
        cl = L.cl[base + i];
        rc = L.rec[base + i];
      }
      __builtin_amdgcn_wave_barrier();
      if (v) {
        L.off[base + i + 1] = o;
        L.len[base + i + 1] = l;
        L.cl[base + i + 1] = cl;
        L.rec[base + i + 1] = rc;
      }
      if (b <= at) break;
    }
  }
  if (lane == 0) {
    L.off[base + at] = moff;
    L.len[base + at] = mlen;
    L.cl[base + at] = 0;
    L.rec[base + at] = mrec;
  }
  lists_fence();
  return n + 1;
}

// One frontier step of _yr_scan_update_match_chain_length: the entries of
// [base, base + n) in the gap before a match at moff whose chain_length is not
// `val` get it, flagged as new.  Returns how many.  (Entry b + l is always lane
// l's: a lane reads back its own stores only.)
__device__ uint32_t chain_mark(const Lists& L, uint32_t base, uint32_t n, int64_t moff, int64_t gmin,
                               int64_t gmax, uint32_t val) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t count = 0;
  for (uint32_t b = 0; b < n; b += 64) {
    const uint32_t i = b + lane;
    bool hit = false;
    if (i < n) {
      const int64_t end = (int64_t)L.off[base + i] + (int64_t)L.len[base + i];
      hit = end + gmax >= moff && end + gmin <= moff && (L.cl[base + i] & ~kChainNew) != val;
      if (hit) L.cl[base + i] = val | kChainNew;
    }
    count += (uint32_t)__popcll(__ballot(hit));
  }
  return count;
}

// Where the confirmed heads go: items {head << 32 | offset, the head's record},
// one atomic per step of the sweep.
struct ChainSink {
  uint64_t* item_keys;
  uint32_t* item_index;
  uint32_t* item_count;
};

// scan.c:546-583 on the head's list [base, base + n) at a tail match {moff,
// mlen}: the entries with the full chain length leave as items, the others
// close up.  Returns the new length; `confirmed` counts the items.
__device__ __forceinline__ uint32_t chain_confirm(const Lists& L, uint32_t base, uint32_t n,
                                                  uint32_t levels, uint32_t head, uint32_t moff,
                                                  uint32_t mlen, const MatchParams& p,
                                                  const ChainSink& k, uint32_t& confirmed) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t w = 0;
  for (uint32_t b = 0; b < n; b += 64) {
    const uint32_t i = b + lane;
    const bool v = i < n;
    uint32_t o = 0, l = 0, cl = 0, rc = 0;
    if (v) {
      o = L.off[base + i];
      l = L.len[base + i];
      cl = L.cl[base + i] & ~kChainNew;
      rc = L.rec[base + i];
    }
    const bool done = v && cl == levels - 1;
    const uint64_t D = __ballot(done), K = __ballot(v && !done);
    if (D != 0) {
      uint32_t slot = 0;
      if (lane == 0) slot = atomicAdd(k.item_count, (uint32_t)__popcll(D));
      slot = lane_of(slot, 0) + lanes_below(D);
      if (done && slot < p.n) {
        k.item_keys[slot] = (uint64_t)head << 32 | o;
        k.item_index[slot] = rc;
        // hex_unique_kernel adds the record's distance from the item's offset
        MatchMeasure m;
        m.length = moff + mlen - (uint32_t)p.recs[rc].offset;
        m.xor_key = 0;
        p.meas[rc] = m;
      }
      confirmed += (uint32_t)__popcll(D);
    }
    const uint32_t at = w + lanes_below(K);
    if (v && !done && at != i) {
      L.off[base + at] = o;
      L.len[base + at] = l;
      L.cl[base + at] = cl;
      L.rec[base + at] = rc;
    }
    w += (uint32_t)__popcll(K);
  }
  return w;
}

// One event {lvl, moff, mlen, mrec} of a chain of `levels` parts, the whole of
// _yr_scan_verify_chained_string_match for that call.  Level l's state is lane
// l's: its list's place lbase and length llen, its gaps lgmin / lgmax.
__device__ __forceinline__ void chain_event(const Lists& L, uint32_t levels, uint32_t head,
                                            uint32_t lvl, uint32_t moff, uint32_t mlen,
                                            uint32_t mrec, uint32_t lbase, uint32_t& llen,
                                            int32_t lgmin, int32_t lgmax, const MatchParams& p,
                                            const ChainSink& k, uint32_t& confirmed) {
  const uint32_t lane = threadIdx.x & 63u;
  if (lvl >= levels) return;   // (never: level_of is below the chain's length)
  const bool tail = lvl + 1 == levels;
  if (lvl != 0) {
    // scan.c:452-498 on the list of the part before this one
    const uint32_t own = tail ? 0u : lane_of(llen, lvl);
    const int64_t lowest = own != 0 ? (int64_t)uni(L.off[lane_of(lbase, lvl)]) : (int64_t)moff;
    const int64_t gmin = (int32_t)lane_of((uint32_t)lgmin, lvl);
    const int64_t gmax = (int32_t)lane_of((uint32_t)lgmax, lvl);
    bool found;
    const uint32_t left = chain_prune(L, lane_of(lbase, lvl - 1), lane_of(llen, lvl - 1), moff,
                                      lowest, gmin, gmax, found);
    if (lane == lvl - 1) llen = left;
    if (!found) return;
    if (tail) {
      // scan.c:519-534, the recursion a frontier per level: level lv's new
      // entries mark level lv - 1 with the next chain length
      uint32_t fresh = chain_mark(L, lane_of(lbase, lvl - 1), left, moff, gmin, gmax, 1u);
      for (uint32_t lv = lvl - 1; lv != 0 && fresh != 0; --lv) {
        const uint32_t base = lane_of(lbase, lv), n = lane_of(llen, lv);
        const int64_t g0 = (int32_t)lane_of((uint32_t)lgmin, lv);
        const int64_t g1 = (int32_t)lane_of((uint32_t)lgmax, lv);
        const uint32_t val = levels - lv;
        fresh = 0;
        for (uint32_t b = 0; b < n; b += 64) {
          const uint32_t i = b + lane;
          uint32_t cl = 0, o = 0;
          if (i < n) {
            cl = L.cl[base + i];
            o = L.off[base + i];
            if (cl & kChainNew) L.cl[base + i] = cl & ~kChainNew;
          }
          for (uint64_t N = __ballot((cl & kChainNew) != 0); N != 0; N &= N - 1)
            fresh += chain_mark(L, lane_of(lbase, lv - 1), lane_of(llen, lv - 1),
                                (int64_t)lane_of(o, (uint32_t)__builtin_ctzll(N)), g0, g1, val);
        }
      }
      // scan.c:546-583: the head's entries with the full chain length are matches
      const uint32_t w = chain_confirm(L, lane_of(lbase, 0), lane_of(llen, 0), levels, head, moff,
                                       mlen, p, k, confirmed);
      if (lane == 0) llen = w;
      lists_fence();
      return;
    }
  }
  // scan.c:585-628: a part that is not the tail joins its unconfirmed list
  const uint32_t n = chain_insert(L, lane_of(lbase, lvl), lane_of(llen, lvl), moff, mlen, mrec);
  if (lane == lvl) llen = n;
}

__global__ __launch_bounds__(64 * kChainWaves) void chain_replay_kernel(ChainParams c, uint32_t waves) {
  __shared__ uint32_t share[kChainWaves][4 * kChainLdsEntries];
  const MatchParams& p = c.h.m;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const ChainSink sink{c.item_keys, c.item_index, c.item_count};
  for (uint32_t chain = blockIdx.x * kChainWaves + wave; chain < c.t.n_chains; chain += waves) {
    const uint32_t begin = uni(c.cbegin[chain]), end = uni(c.cend[chain]);
    if (begin >= end) continue;
    const uint32_t s0 = uni(c.t.chain_off[chain]);
    const uint32_t levels = uni(c.t.chain_off[chain + 1]) - s0;   // (2 .. kChainMaxLevels)
    // lane l: level l's string, its gaps, its list's place and length
    uint32_t lstr = 0, lbase = 0, llen = 0, cap = 0;
    int32_t lgmin = 0, lgmax = 0;
    if (lane < levels) {
      lstr = c.t.chain_strs[s0 + lane];
      lgmin = c.t.gap_min[lstr];
      lgmax = c.t.gap_max[lstr];
      lbase = (uint32_t)str_offset(c, lstr);
      if (lane + 1 < levels) cap = (uint32_t)str_offset(c, lstr + 1) - lbase;   // (the tail keeps none)
    }
    const uint32_t upto = wave_prefix(cap);
    Lists L;
    if (lane_of(upto, 63) <= kChainLdsEntries) {
      lbase = upto - cap;
      L.off = share[wave];
    } else {
      L.off = c.lists;
    }
    const uint64_t stride = L.off == c.lists ? p.n : kChainLdsEntries;
    L.len = L.off + stride;
    L.cl = L.len + stride;
    L.rec = L.cl + stride;
    const uint32_t head = lane_of(lstr, 0);
    uint32_t confirmed = 0;

    for (uint32_t eb = begin; eb < end; eb += 64) {
      const uint32_t cnt = min(64u, end - eb);
      uint32_t erec = 0, elvl = 0, eoff = 0, elen = 0;
      if (lane < cnt) {
        erec = c.sorted_index[eb + lane];
        elvl = c.ev_level[erec];
        eoff = c.ev_offset[erec];
        elen = c.ev_length[erec];
      }
      for (uint32_t j = 0; j < cnt; ++j)
        chain_event(L, levels, head, lane_of(elvl, j), lane_of(eoff, j), lane_of(elen, j),
                    lane_of(erec, j), lbase, llen, lgmin, lgmax, p, sink, confirmed);
    }
  }
}

// ---- The batch's chains (matches.h BatchChainParams) ----
// The same replay, one wave per (buffer, chain) GROUP.  Nothing is indexed by
// (buffer, chain) or (buffer, string): the groups are found in the events'
// stream once batch_match_sort has ordered it by (buffer, chain), and each
// group's lists live in the group's own slots of that stream.

__global__ __launch_bounds__(256) void batch_chain_clear_kernel(BatchChainParams c) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= c.b.nbuf) c.buf_items[i] = 0;
  if (i < 2) c.counts[i] = 0;
}

// chain_events_kernel with batch_hex_measure_kernel's view: the record's buffer
// (buf[], the measure pass has searched for it) is the whole block of both
// runs, offsets are local to it.  An event and a dirty-maker both get their
// chain as the sort's key -- dirtiness is a property of the (buffer, chain)
// group, derived from the group's run, so no flag array is written here.
__global__ __launch_bounds__(256) void batch_chain_events_kernel(BatchChainParams c) {
  __shared__ __attribute__((aligned(16))) uint8_t codebuf[256 * kHexCodeBytes + 16];
  const MatchParams& p = c.b.h.m;
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.n) return;
  const VerifyRec rec = p.recs[r];
  const uint32_t string = p.pool_string[rec.pool_index];
  const uint32_t chain = string < p.n_strings ? c.t.chain_of[string] : kNoChain;
  const uint32_t k = c.b.buf[r];
  uint32_t key = c.t.n_chains;
  if (chain != kNoChain && k < c.b.nbuf && ((c.t.settled[chain] >> (c.b.h.classes >> 1)) & 1u)) {
    HexMatchParams q = c.b.h;
    q.m.data = p.data + c.b.starts[k];
    q.m.size = c.b.sizes[k];
    q.m.win_lo = 0;
    q.m.win_hi = q.m.size;
    DevPoolRec e = p.pool[rec.pool_index];
    e.flags &= ~(kStrChainPart | kStrChainTail);
    MatchMeasure m{0, 0};
    uint64_t offset = rec.offset;
    bool event = false, dirty = false;
    if (string_is_final(e.flags)) {
      event = measure(q.m, e, rec.offset, m);
    } else {
      HexSet set{1ull, 0u, 0u};
      const uint32_t buf = (uint32_t)(uintptr_t)(codebuf + threadIdx.x * kHexCodeBytes);
      const int v = measure_hex(q, e, rec.offset, buf, m, set);
      if (v == kHexMatch && m.length != 0) {
        // one callback per backward result, in an order that is not restated
        dirty = (set.mask & (set.mask - 1)) != 0;
        const uint32_t B = set.base + (uint32_t)__builtin_ctzll(set.mask);
        offset -= B;   // (B <= min(offset, YR_RE_SCAN_LIMIT))
        m.length += B;
        event = !dirty;
      } else {
        dirty = v == kHexUndecided;
      }
    }
    if (event || dirty) {
      key = chain;
      c.ev_level[r] = dirty ? kChainDirtyMaker : c.t.level_of[string];
      c.ev_offset[r] = (uint32_t)offset;   // (below the buffer's size)
      c.ev_length[r] = m.length;
    }
  }
  c.skeys[r] = key;
  c.sindex[r] = (uint32_t)r;
}

// One lane per sorted entry: the first entry of a (buffer, chain) run appends
// the run's place to the group list -- one atomic per wave, the list in no
// particular order.
__global__ __launch_bounds__(256) void batch_chain_groups_kernel(BatchChainParams c) {
  const uint64_t n = c.b.h.m.n;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool first = false;
  if (i < n) {
    const uint64_t key = c.sorted_keys[i];
    first = key < c.t.n_chains &&
            (i == 0 || c.sorted_keys[i - 1] != key ||
             c.b.buf[c.sorted_index[i - 1]] != c.b.buf[c.sorted_index[i]]);
  }
  const uint64_t F = __ballot(first);
  if (F == 0) return;   // (wave-uniform)
  uint32_t slot = 0;
  if ((threadIdx.x & 63u) == 0) slot = atomicAdd(c.counts, (uint32_t)__popcll(F));
  slot = lane_of(slot, 0) + lanes_below(F);
  if (first && slot < n) c.gbegin[slot] = (uint32_t)i;
}

// One WAVE per group, a fixed grid striding over the group list (its length is
// read here, not waited for).  The wave walks its run twice.  First to its end
// -- the run is contiguous: the entries that share the first one's chain and
// buffer -- looking for a dirty-maker and counting the events per level into
// lane `level`: a level's list holds at most its own events, so the prefix sum
// of the counts places every list inside the run's own E slots, of the wave's
// LDS share (E <= kChainLdsEntries) or of the [4][n] workspace at `begin`.  A
// dirty group is left as the measure pass wrote it.  Then the events of a clean
// group leave the rest (key string field n_strings + 1, an empty set) and are
// replayed by chain_event; the confirmed heads are counted per buffer.
__global__ __launch_bounds__(64 * kChainWaves) void batch_chain_replay_kernel(BatchChainParams c,
                                                                              uint32_t waves) {
  __shared__ uint32_t share[kChainWaves][4 * kChainLdsEntries];
  const MatchParams& p = c.b.h.m;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t n = (uint32_t)p.n;   // (at most kMatchMaxRecords)
  const uint32_t groups = min(uni(c.counts[0]), n);
  const ChainSink sink{c.item_keys, c.item_index, c.counts + 1};
  for (uint32_t g = blockIdx.x * kChainWaves + wave; g < groups; g += waves) {
    const uint32_t begin = uni(c.gbegin[g]);
    if (begin >= n) continue;   // (never)
    // (a key is a chain or n_chains: 32 bits)
    const uint32_t chain = uni((uint32_t)c.sorted_keys[begin]);
    const uint32_t k = uni(c.b.buf[c.sorted_index[begin]]);
    if (chain >= c.t.n_chains || k >= c.b.nbuf) continue;   // (never)
    const uint32_t s0 = uni(c.t.chain_off[chain]);
    const uint32_t levels = uni(c.t.chain_off[chain + 1]) - s0;   // (2 .. kChainMaxLevels)
    uint32_t lstr = 0, lbase = 0, llen = 0, cap = 0;
    int32_t lgmin = 0, lgmax = 0;
    if (lane < levels) {
      lstr = c.t.chain_strs[s0 + lane];
      lgmin = c.t.gap_min[lstr];
      lgmax = c.t.gap_max[lstr];
    }
    uint32_t end = begin;
    bool dirty = false;
    for (uint32_t eb = begin; !dirty; eb += 64) {
      const uint32_t i = eb + lane;
      bool in = false;
      uint32_t lv = 0;
      if (i < n && c.sorted_keys[i] == chain) {
        const uint32_t r = c.sorted_index[i];
        in = c.b.buf[r] == k;
        lv = c.ev_level[r];
      }
      const uint64_t out = ~__ballot(in);
      const uint32_t cnt = out == 0 ? 64u : (uint32_t)__builtin_ctzll(out);
      const bool v = lane < cnt;
      dirty = __ballot(v && lv == kChainDirtyMaker) != 0;
      for (uint32_t l = 0; l + 1 < levels; ++l) {   // (the tail keeps no list)
        const uint32_t here = (uint32_t)__popcll(__ballot(v && lv == l));
        if (lane == l) cap += here;
      }
      end = eb + cnt;
      if (cnt < 64) break;
    }
    if (dirty) continue;
    const uint32_t upto = wave_prefix(cap);
    Lists L;
    if (lane_of(upto, 63) <= kChainLdsEntries) {
      lbase = upto - cap;
      L.off = share[wave];
    } else {
      lbase = begin + upto - cap;   // (upto <= end - begin: inside the run's slots)
      L.off = c.lists;
    }
    const uint64_t stride = L.off == c.lists ? p.n : kChainLdsEntries;
    L.len = L.off + stride;
    L.cl = L.len + stride;
    L.rec = L.cl + stride;
    const uint32_t head = lane_of(lstr, 0);
    uint32_t confirmed = 0;
    for (uint32_t eb = begin; eb < end; eb += 64) {
      const uint32_t cnt = min(64u, end - eb);
      uint32_t erec = 0, elvl = 0, eoff = 0, elen = 0;
      if (lane < cnt) {
        erec = c.sorted_index[eb + lane];
        elvl = c.ev_level[erec];
        eoff = c.ev_offset[erec];
        elen = c.ev_length[erec];
        p.keys[erec] = (uint64_t)(p.n_strings + 1) << 32 | (p.keys[erec] & 0xFFFFFFFFull);
        c.b.h.sets[erec] = HexSet{0ull, 0u, 0u};
      }
      for (uint32_t j = 0; j < cnt; ++j)
        chain_event(L, levels, head, lane_of(elvl, j), lane_of(eoff, j), lane_of(elen, j),
                    lane_of(erec, j), lbase, llen, lgmin, lgmax, p, sink, confirmed);
    }
    if (lane == 0 && confirmed != 0)
      atomicAdd(reinterpret_cast<unsigned long long*>(c.buf_items + k), (unsigned long long)confirmed);
  }
}

// The per-wave rest counts again, as the measure pass wrote them, now that the
// clean groups' events have left the rest.
__global__ __launch_bounds__(256) void batch_chain_recount_kernel(BatchChainParams c) {
  const MatchParams& p = c.b.h.m;
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool rest = r < p.n && (uint32_t)(p.keys[r] >> 32) == p.n_strings;
  const uint64_t mask = __ballot(rest);
  if ((threadIdx.x & 63u) == 0 && r < p.n) p.block_off[r / kGroup] = (uint64_t)__popcll(mask);
}

// One lane per k in [0, nbuf]: buffer k's slots in the sorted item arrays begin
// behind the records' items AND the chain items of the buffers before it.
__global__ __launch_bounds__(256) void batch_chain_item_offsets_kernel(BatchChainParams c) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > c.b.nbuf) return;
  c.b.item_off[k] += c.buf_chunk[k / kChunkGroups] + c.buf_items[k];
}

inline dim3 chain_grid(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

}  // namespace

hipError_t launch_chain_events(const ChainParams& c, hipStream_t s) {
  const uint64_t n = c.h.m.n;
  if (n == 0 || n > kMatchMaxRecords || c.t.n_chains == 0) return hipErrorInvalidValue;
  // (kernels, not memsets: the stage may be recorded into a graph)
  hipLaunchKernelGGL(chain_clear_kernel,
                     chain_grid(std::max<uint64_t>((uint64_t)c.h.m.n_strings + 1, c.t.n_chains)),
                     dim3(256), 0, s, c);
  hipLaunchKernelGGL(chain_events_kernel, chain_grid(n), dim3(256), 0, s, c);
  hipLaunchKernelGGL(chain_mark_kernel, chain_grid(n), dim3(256), 0, s, c);
  return hipGetLastError();
}

hipError_t launch_chain_replay(const ChainParams& c, uint32_t waves, hipStream_t s) {
  const uint64_t n = c.h.m.n;
  if (n == 0 || n > kMatchMaxRecords || c.t.n_chains == 0 || waves == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(chain_bounds_kernel, chain_grid(n), dim3(256), 0, s, c);
  const uint32_t blocks = (std::min(waves, c.t.n_chains) + kChainWaves - 1) / kChainWaves;
  hipLaunchKernelGGL(chain_replay_kernel, dim3(blocks), dim3(64 * kChainWaves), 0, s, c,
                     blocks * kChainWaves);
  return hipGetLastError();
}

hipError_t launch_batch_chain_events(const BatchChainParams& c, hipStream_t s) {
  const uint64_t n = c.b.h.m.n;
  if (n == 0 || n > kMatchMaxRecords || c.t.n_chains == 0 || c.b.nbuf == 0) return hipErrorInvalidValue;
  // (a kernel, not memsets: the stage may be recorded into a graph)
  hipLaunchKernelGGL(batch_chain_clear_kernel, chain_grid((uint64_t)c.b.nbuf + 1), dim3(256), 0, s, c);
  hipLaunchKernelGGL(batch_chain_events_kernel, chain_grid(n), dim3(256), 0, s, c);
  return hipGetLastError();
}

hipError_t launch_batch_chain_replay(const BatchChainParams& c, uint32_t waves, hipStream_t s) {
  const uint64_t n = c.b.h.m.n;
  if (n == 0 || n > kMatchMaxRecords || c.t.n_chains == 0 || waves == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(batch_chain_groups_kernel, chain_grid(n), dim3(256), 0, s, c);
  // (at most a wave per record: there are no more groups than that)
  const uint32_t blocks = ((uint32_t)std::min<uint64_t>(waves, n) + kChainWaves - 1) / kChainWaves;
  hipLaunchKernelGGL(batch_chain_replay_kernel, dim3(blocks), dim3(64 * kChainWaves), 0, s, c,
                     blocks * kChainWaves);
  hipLaunchKernelGGL(batch_chain_recount_kernel, chain_grid(n), dim3(256), 0, s, c);
  return hipGetLastError();
}

hipError_t launch_batch_chain_item_offsets(const BatchChainParams& c, hipStream_t s) {
  hipLaunchKernelGGL(batch_chain_item_offsets_kernel, chain_grid((uint64_t)c.b.nbuf + 1), dim3(256), 0,
                     s, c);
  return hipGetLastError();
}

}  // namespace yamd
