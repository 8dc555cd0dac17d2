// Device code that measures one record of the match stage: the literal
// comparisons in their length-returning form and yr_re_fast_exec in position-set
// form.  Shared by the kernels of matches.hip and chains.hip, each of which
// includes it into its own translation unit.
#pragma once

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
// (WIDE only) undecided because the set leaves the window: the wave-wide path decides
constexpr int kHexWide = 3;

// yr_re_fast_exec (re.c:2150-2423) in position-set form, verify.hip
// fast_re_set's transitions, but with the set at RE_OPCODE_MATCH as the
// result: bit i of out.mask = bytes_matched value out.base + i.  Byte b of the
// input is input[b], backwards input[-1 - b]; only live positions (b < maxb)
// are read, so no byte outside the block.  kHexUndecided: the set would leave
// the 64-position window or come near YR_RE_SCAN_LIMIT, an opcode outside the
// fast set, a program that does not end in MATCH, or a REPEAT_ANY right
// before MATCH (whose b + min the reference does not bound).
template <class Code, bool WIDE = false>
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
      if (span > 63 || nb + span >= kReScanLimit) return WIDE ? kHexWide : kHexUndecided;
      // (with the wave-wide path on: a forward jump with 0 < min < max run from
      // several positions leaves the reference's list unsorted -- hex_wide_run's
      // note -- and the lowest bit need not be its first element: undecided)
      if (WIDE && !backwards && mn > 0 && mx > mn && (live & (live - 1)) != 0) return kHexUndecided;
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
template <class Code, bool WIDE = false>
__device__ int hex_call(const MatchParams& p, const DevRe& r, const Code fwd, const Code bwd,
                        uint64_t offset, MatchMeasure& m, HexSet& set) {
  const uint8_t* d = p.data + offset;
  HexSet f;
  int v = hex_run<Code, WIDE>(fwd, r.fwd_len, d,
                              (int)min<uint64_t>(p.size - offset, (uint64_t)kReScanLimit), false, f);
  if (v != kHexMatch) return v;
  m.length = f.base + (uint32_t)__builtin_ctzll(f.mask);   // the first of the ascending list
  if (r.bwd_len == 0) return m.length != 0 ? kHexMatch : kHexNone;
  return hex_run<Code, WIDE>(bwd, r.bwd_len, d, (int)min<uint64_t>(offset, (uint64_t)kReScanLimit),
                             true, set);
}

template <bool WIDE = false>
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
    if (at != kNoLds)
      return hex_call<LdsCode, WIDE>(p, r, LdsCode{at}, LdsCode{at + r.fwd_len}, offset, m, set);
  }
  return hex_call<GlobalCode, WIDE>(p, r, GlobalCode{fwd}, GlobalCode{bwd}, offset, m, set);
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

}  // namespace

}  // namespace yamd
