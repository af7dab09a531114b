// sam_line.h — one SAM text line -> one BAM record (block_size + record), the per-line half of
// hbam_sam.hip.  Everything here is plain C++ over pointers (host and device), so the rules can be
// run on a CPU as they stand.
//
// The rules restate a subset of htsjdk's SAMLineParser.parseLine and BAMRecordCodec.encode (htsjdk
// is not in the reference tree: parity unpinned, DESIGN.md lists them).  A line is checked in this
// order and the first failure is its status: the field count, empty fields, then QNAME, FLAG,
// RNAME, POS, MAPQ, CIGAR, RNEXT, PNEXT, TLEN, the SEQ / QUAL lengths, the tags left to right; the
// SEQ and QUAL bytes themselves are checked by the unit functions at the end (the bulk pass).
#pragma once
#include <stdint.h>

#include "hbam.h"

#ifdef __HIPCC__
#define HBAM_HD __host__ __device__ inline
#else
#define HBAM_HD inline
#endif

namespace hbam {

constexpr uint32_t SAM_MAX_NAME = 254;     // l_read_name is one byte and counts the NUL
constexpr uint32_t SAM_MAX_CIGAR = 65535;  // n_cigar_op is 16 bits (no CG tag here)
constexpr int32_t SAM_FLOAT_MAX_DIGITS = 9;
constexpr int32_t SAM_FLOAT_MAX_EXP = 20;  // |decimal exponent| once the digits are an integer

// the tab bitmap of the structural pass (k_vcf_scan) read as 64-bit words; positions are `shifted`
// (relative to the 16-byte boundary at or below the window's first byte): the line is [p0, pe)
struct SamTabs {
  const uint64_t* map;
  uint32_t p0, pe;
};
// the first tab at or after line-relative `from`, or the line's length
HBAM_HD uint32_t sam_next_tab(const SamTabs& t, uint32_t from) {
  const uint32_t len = t.pe - t.p0;
  if (from >= len) return len;
  const uint32_t p = t.p0 + from;
  uint32_t word = p >> 6;
  uint64_t bits = t.map[word] & (~0ull << (p & 63u));
  while (bits == 0) {
    ++word;
    if (((uint64_t)word << 6) >= t.pe) return len;
    bits = t.map[word];
  }
  const uint32_t at = (word << 6) + (uint32_t)__builtin_ctzll(bits);
  return at >= t.pe ? len : at - t.p0;
}

#ifdef __HIPCC__
typedef uint32_t sam_u32x4_a1 __attribute__((ext_vector_type(4), aligned(1)));
#endif
typedef uint32_t sam_u32_a1 __attribute__((aligned(1)));
typedef uint16_t sam_u16_a1 __attribute__((aligned(1)));

// The line's bytes through a 16-byte register cache.  A lane per line reads its own line, so every
// load instruction of a wave touches 64 different cache lines whatever its width: a byte per load
// made the per-line passes cost as many cache-line requests as the line has bytes.  Here a load
// brings 16 bytes and the parsers, which walk the line front to back, take them from registers.
// (A load may pass the line's end by up to 15 bytes: inside the window's 64 readable pad bytes.)
struct SamBytes {
  const uint8_t* p;
  uint32_t at;  // the cached chunk, ~0u: none
  uint32_t w0, w1, w2, w3;
  HBAM_HD explicit SamBytes(const uint8_t* line) : p(line), at(~0u), w0(0), w1(0), w2(0), w3(0) {}
  HBAM_HD uint32_t operator[](uint32_t i) {
    const uint32_t c = i >> 4;
    if (c != at) {
#ifdef __HIPCC__
      const sam_u32x4_a1 q = *reinterpret_cast<const sam_u32x4_a1*>(p + 16ull * c);
      w0 = q[0];
      w1 = q[1];
      w2 = q[2];
      w3 = q[3];
#else  // a host compiler without vector types: four unaligned words
      const sam_u32_a1* const q = reinterpret_cast<const sam_u32_a1*>(p + 16ull * c);
      w0 = q[0];
      w1 = q[1];
      w2 = q[2];
      w3 = q[3];
#endif
      at = c;
    }
    const uint32_t k = i & 15u;
    const uint32_t w = k < 8u ? (k < 4u ? w0 : w1) : (k < 12u ? w2 : w3);
    return (w >> (8u * (k & 3u))) & 0xffu;
  }
};

// [+-]? digit+ -> the value, saturated at +-2^40 (any count of digits); false when not that shape
HBAM_HD bool sam_parse_i64(SamBytes& l, uint32_t o, uint32_t n, int64_t* out) {
  if (n == 0) return false;
  uint32_t i = 0;
  const bool neg = l[o] == '-';
  if (neg || l[o] == '+') i = 1;
  if (i == n) return false;
  int64_t v = 0;
  for (; i < n; ++i) {
    const uint32_t d = l[o + i] - '0';
    if (d > 9u) return false;
    v = v * 10 + (int64_t)d;
    if (v > (1ll << 40)) v = 1ll << 40;
  }
  *out = neg ? -v : v;
  return true;
}
// Integer.parseInt
HBAM_HD bool sam_parse_i32(SamBytes& l, uint32_t o, uint32_t n, int32_t* out) {
  int64_t v;
  if (!sam_parse_i64(l, o, n, &v) || v < -2147483648ll || v > 2147483647ll) return false;
  *out = (int32_t)v;
  return true;
}

// the @SQ dictionary (hbam_vcf_contig layout): FNV-1a slot, linear probing -> ordinal or -1
HBAM_HD int32_t sam_lookup(const hbam_vcf_contig* table, uint32_t tmask, const uint8_t* names, SamBytes& l,
                           uint32_t o, uint32_t n) {
  uint32_t h = 2166136261u;
  for (uint32_t i = 0; i < n; ++i) h = (h ^ l[o + i]) * 16777619u;
  for (h &= tmask;; h = (h + 1) & tmask) {
    const hbam_vcf_contig e = table[h];
    if (e.ordinal < 0) return -1;  // an empty slot: the table is at most half full
    if (e.name_len != n) continue;
    const uint8_t* nm = names + e.name_off;
    uint32_t j = 0;
    while (j < n && nm[j] == l[o + j]) ++j;
    if (j == n) return e.ordinal;
  }
}

// SAM spec 5.3 over the 0-based half-open [beg, end), on ints as the reference computes it
HBAM_HD int32_t sam_reg2bin(int32_t beg, int32_t end) {
  --end;
  if (beg >> 14 == end >> 14) return ((1 << 15) - 1) / 7 + (beg >> 14);
  if (beg >> 17 == end >> 17) return ((1 << 12) - 1) / 7 + (beg >> 17);
  if (beg >> 20 == end >> 20) return ((1 << 9) - 1) / 7 + (beg >> 20);
  if (beg >> 23 == end >> 23) return ((1 << 6) - 1) / 7 + (beg >> 23);
  if (beg >> 26 == end >> 26) return ((1 << 3) - 1) / 7 + (beg >> 26);
  return 0;
}

// unaligned little-endian stores, one instruction each (a record starts at any byte of ubuf)
HBAM_HD void sam_st16(uint8_t* d, uint32_t v) { *reinterpret_cast<sam_u16_a1*>(d) = (uint16_t)v; }
HBAM_HD void sam_st32(uint8_t* d, uint32_t v) { *reinterpret_cast<sam_u32_a1*>(d) = v; }
// n line bytes from offset o to d, four per store
HBAM_HD void sam_copy(SamBytes& l, uint32_t o, uint32_t n, uint8_t* d) {
  uint32_t k = 0;
  for (; k + 4 <= n; k += 4)
    sam_st32(d + k, l[o + k] | l[o + k + 1] << 8 | l[o + k + 2] << 16 | l[o + k + 3] << 24);
  for (; k < n; ++k) d[k] = (uint8_t)l[o + k];
}

// Decimal text -> the nearest float32, ties to even, exactly.  Domain: [+-]? digits [. digits]
// ([eE] [+-]? digits)?, at least one digit before the exponent, at most SAM_FLOAT_MAX_DIGITS
// significant digits once leading and trailing zeros are dropped, and a decimal exponent within
// +-SAM_FLOAT_MAX_EXP once those digits are read as an integer M (value = M x 10^E); zero with any
// exponent.  Then M < 2^30, M x 10^20 < 2^97 and 10^20 < 2^67: the quotient's bits come from a
// restoring division in 128-bit integers (shifts, compares and subtractions only), the result is
// a normal float32.  Returns false outside the domain.
HBAM_HD bool sam_parse_float(SamBytes& l, uint32_t o, uint32_t n, uint32_t* bits) {
  typedef unsigned __int128 u128;
  uint32_t i = 0;
  uint32_t sign = 0;
  if (i < n && (l[o] == '-' || l[o] == '+')) sign = l[o + i++] == '-' ? 0x80000000u : 0u;
  uint64_t M = 0;
  int32_t nd = 0, E = 0;
  bool any = false, point = false;
  for (; i < n; ++i) {
    if (l[o + i] == '.') {
      if (point) return false;
      point = true;
      continue;
    }
    const uint32_t d = l[o + i] - '0';
    if (d > 9u) break;
    any = true;
    if (nd == 0 && d == 0) {  // a leading zero
      if (point) --E;
    } else if (nd < SAM_FLOAT_MAX_DIGITS) {
      M = M * 10 + d;
      ++nd;
      if (point) --E;
    } else {
      if (d != 0) return false;  // a 10th significant digit
      if (!point) ++E;
    }
    if (nd && (E < -10000 || E > 10000)) return false;  // (zero takes any count of digits)
  }
  if (!any) return false;
  if (i < n) {
    if (l[o + i] != 'e' && l[o + i] != 'E') return false;
    int64_t x;
    if (!sam_parse_i64(l, o + i + 1, n - i - 1, &x)) return false;
    if (x < -10000 || x > 10000) {
      if (M != 0) return false;
      x = 0;
    }
    E += (int32_t)x;
  }
  if (M == 0) {
    *bits = sign;
    return true;
  }
  while (M % 10 == 0) {  // trailing zeros of the digits belong to the exponent
    M /= 10;
    ++E;
  }
  if (E < -SAM_FLOAT_MAX_EXP || E > SAM_FLOAT_MAX_EXP) return false;
  u128 N = M, D = 1;
  for (int32_t k = 0; k < E; ++k) N = (N << 3) + (N << 1);
  for (int32_t k = 0; k < -E; ++k) D = (D << 3) + (D << 1);
  int32_t a = 0, b = 0;
  for (u128 t = N; t != 0; t >>= 1) ++a;
  for (u128 t = D; t != 0; t >>= 1) ++b;
  // q = floor(N x 2^s / D) lies in (2^24, 2^26)
  int32_t s = 25 - (a - b);
  uint64_t q = 0;
  u128 R = 0;
  bool sticky = false;
  const int32_t steps = a + s;  // the bits of N x 2^s that enter the division (s < 0: the top a + s of N)
  for (int32_t k = 0; k < steps; ++k) {
    const int32_t src = a - 1 - k;  // bit of N, or a shifted-in zero below it
    const uint32_t bit = src >= 0 ? (uint32_t)(N >> src) & 1u : 0u;
    R = (R << 1) | bit;
    q <<= 1;
    if (R >= D) {
      R -= D;
      q |= 1;
    }
  }
  if (s < 0 && (N & (((u128)1 << -s) - 1)) != 0) sticky = true;
  if (R != 0) sticky = true;
  if (q >= (1ull << 25)) {
    sticky = sticky || (q & 1);
    q >>= 1;
    --s;
  }
  // value = (q + fraction) x 2^-s, q in [2^24, 2^25): 24 bits and the rounding bit
  uint64_t mant = q >> 1;
  if ((q & 1) && (sticky || (mant & 1))) ++mant;
  int32_t e2 = 1 - s;  // value ~ mant x 2^e2
  if (mant == (1ull << 24)) {
    mant >>= 1;
    ++e2;
  }
  *bits = sign | (uint32_t)(127 + 23 + e2) << 23 | ((uint32_t)mant & 0x7fffffu);
  return true;
}

// one integer of a B array into `w` bytes, range-checked for the subtype
HBAM_HD bool sam_array_int(uint32_t sub, SamBytes& l, uint32_t o, uint32_t n, uint8_t* out) {
  int64_t v;
  if (!sam_parse_i64(l, o, n, &v)) return false;
  int64_t lo, hi;
  uint32_t w;
  switch (sub) {
    case 'c': lo = -128; hi = 127; w = 1; break;
    case 'C': lo = 0; hi = 255; w = 1; break;
    case 's': lo = -32768; hi = 32767; w = 2; break;
    case 'S': lo = 0; hi = 65535; w = 2; break;
    case 'i': lo = -2147483648ll; hi = 2147483647ll; w = 4; break;
    default: lo = 0; hi = 4294967295ll; w = 4; break;
  }
  if (v < lo || v > hi) return false;
  if (out)
    for (uint32_t k = 0; k < w; ++k) out[k] = (uint8_t)((uint64_t)v >> (8 * k));
  return true;
}

// One tag field XX:T:value = line bytes [f, f + n) -> its BAM bytes at out (nullptr: size only).
// *used = the bytes.
HBAM_HD int32_t sam_tag(SamBytes& l, uint32_t f, uint32_t n, uint8_t* out, uint32_t* used) {
  *used = 0;
  if (n < 6 || l[f + 2] != ':' || l[f + 4] != ':') return HBAM_EFORMAT;  // an empty value too
  const uint32_t ty = l[f + 3];
  const uint32_t v = f + 5, vn = n - 5;
  if (out) sam_st16(out, l[f] | l[f + 1] << 8);
  switch (ty) {
    case 'A':
      if (vn != 1) return HBAM_EFORMAT;
      if (out) sam_st16(out + 2, 'A' | l[v] << 8);
      *used = 4;
      return HBAM_OK;
    case 'Z':
      if (out) {
        out[2] = 'Z';
        sam_copy(l, v, vn, out + 3);
        out[3 + vn] = 0;
      }
      *used = 4 + vn;
      return HBAM_OK;
    case 'i': {
      int64_t x;
      if (!sam_parse_i64(l, v, vn, &x) || x < -2147483648ll || x > 4294967295ll) return HBAM_EFORMAT;
      // the narrowest type, in htsjdk's order (BinaryTagCodec.getIntegerType)
      uint8_t t;
      uint32_t w;
      if (x > 2147483647ll) { t = 'I'; w = 4; }
      else if (x > 65535) { t = 'i'; w = 4; }
      else if (x > 32767) { t = 'S'; w = 2; }
      else if (x > 255) { t = 's'; w = 2; }
      else if (x > 127) { t = 'C'; w = 1; }
      else if (x >= -128) { t = 'c'; w = 1; }
      else if (x >= -32768) { t = 's'; w = 2; }
      else { t = 'i'; w = 4; }
      if (out) {
        out[2] = t;
        for (uint32_t k = 0; k < w; ++k) out[3 + k] = (uint8_t)((uint64_t)x >> (8 * k));
      }
      *used = 3 + w;
      return HBAM_OK;
    }
    case 'f': {
      uint32_t b;
      if (!sam_parse_float(l, v, vn, &b)) return HBAM_EUNSUPPORTED;
      if (out) {
        out[2] = 'f';
        sam_st32(out + 3, b);
      }
      *used = 7;
      return HBAM_OK;
    }
    case 'B': {
      const uint32_t sub = l[v];
      uint32_t w;
      switch (sub) {
        case 'c': case 'C': w = 1; break;
        case 's': case 'S': w = 2; break;
        case 'i': case 'I': case 'f': w = 4; break;
        default: return HBAM_EFORMAT;
      }
      uint32_t cnt = 0, at = 1;
      while (at < vn) {  // at a ','
        if (l[v + at] != ',') return HBAM_EFORMAT;
        uint32_t e = at + 1;
        while (e < vn && l[v + e] != ',') ++e;
        uint8_t* o = out ? out + 8 + (uint64_t)w * cnt : nullptr;
        if (e == at + 1) return HBAM_EFORMAT;  // an empty element
        if (sub == 'f') {
          uint32_t b;
          if (!sam_parse_float(l, v + at + 1, e - at - 1, &b)) return HBAM_EUNSUPPORTED;
          if (o) sam_st32(o, b);
        } else if (!sam_array_int(sub, l, v + at + 1, e - at - 1, o)) {
          return HBAM_EFORMAT;
        }
        ++cnt;
        at = e;
      }
      if (out) {
        sam_st16(out + 2, 'B' | sub << 8);
        sam_st32(out + 4, cnt);
      }
      *used = 8 + w * cnt;
      return HBAM_OK;
    }
    case 'H':
      return HBAM_EUNSUPPORTED;
    default:
      return HBAM_EFORMAT;
  }
}

struct SamLine {
  int32_t status;
  uint32_t size;       // 4 + block_size
  uint32_t seq_rel;    // line-relative offset of SEQ
  uint32_t l_seq;
  uint32_t qual_star;  // QUAL is "*": l_seq bytes of 0xff
  uint32_t seq_out;    // record-relative offset of the packed SEQ (QUAL follows it)
};

// The line [l, l + len) -> *r, and with out != nullptr everything of the record but SEQ and QUAL.
HBAM_HD void sam_line(const uint8_t* line, const SamTabs& tb, const hbam_vcf_contig* table, uint32_t tmask,
                      const uint8_t* names, uint8_t* out, SamLine* r) {
  const uint32_t len = tb.pe - tb.p0;
  SamBytes l(line);
  *r = SamLine{HBAM_EFORMAT, 0, 0, 0, 0, 0};
  uint32_t b[11], e[11];  // field k = [b[k], e[k])
  uint32_t from = 0;
  for (uint32_t k = 0; k < 11; ++k) {
    if (k && e[k - 1] >= len) return;  // fewer than 11 fields
    b[k] = from;
    e[k] = sam_next_tab(tb, from);
    from = e[k] + 1;
  }
  for (uint32_t k = 0; k < 11; ++k)
    if (e[k] == b[k]) return;  // an empty field
  const uint32_t nl = e[0];
  if (nl > SAM_MAX_NAME) {
    r->status = HBAM_EUNSUPPORTED;
    return;
  }
  int32_t flag, pos1, mapq, pnext1, tlen;
  if (!sam_parse_i32(l, b[1], e[1] - b[1], &flag)) return;
  const auto ref_of = [&](uint32_t k) -> int32_t {
    if (e[k] - b[k] == 1 && l[b[k]] == '*') return -1;
    return sam_lookup(table, tmask, names, l, b[k], e[k] - b[k]);
  };
  const int32_t ref = ref_of(2);
  if (!sam_parse_i32(l, b[3], e[3] - b[3], &pos1)) return;
  if (!sam_parse_i32(l, b[4], e[4] - b[4], &mapq)) return;
  // CIGAR: (digits op)+, op from MIDNSHP=X, or "*"
  uint32_t ncig = 0, reflen = 0;
  uint8_t* const cig_out = out ? out + 36 + nl + 1 : nullptr;
  if (!(e[5] - b[5] == 1 && l[b[5]] == '*')) {
    uint32_t i = b[5];
    while (i < e[5]) {
      uint64_t v = 0;
      const uint32_t d0 = i;
      while (i < e[5] && l[i] - '0' <= 9u) {
        v = v * 10 + (l[i] - '0');
        if (v > (1ull << 28)) v = 1ull << 28;
        ++i;
      }
      if (i == d0 || i == e[5] || v >= (1ull << 28)) return;
      uint32_t op;
      switch (l[i]) {
        case 'M': op = 0; break;
        case 'I': op = 1; break;
        case 'D': op = 2; break;
        case 'N': op = 3; break;
        case 'S': op = 4; break;
        case 'H': op = 5; break;
        case 'P': op = 6; break;
        case '=': op = 7; break;
        case 'X': op = 8; break;
        default: return;
      }
      ++i;
      if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) reflen += (uint32_t)v;
      if (ncig < SAM_MAX_CIGAR && cig_out) sam_st32(cig_out + 4ull * ncig, (uint32_t)v << 4 | op);
      if (ncig <= SAM_MAX_CIGAR) ++ncig;
    }
    if (ncig > SAM_MAX_CIGAR) {
      r->status = HBAM_EUNSUPPORTED;
      return;
    }
  }
  int32_t nref;
  if (e[6] - b[6] == 1 && l[b[6]] == '=') nref = ref;
  else nref = ref_of(6);
  if (!sam_parse_i32(l, b[7], e[7] - b[7], &pnext1)) return;
  if (!sam_parse_i32(l, b[8], e[8] - b[8], &tlen)) return;
  const bool seq_star = e[9] - b[9] == 1 && l[b[9]] == '*';
  const bool qual_star = e[10] - b[10] == 1 && l[b[10]] == '*';
  const uint32_t lseq = seq_star ? 0u : e[9] - b[9];
  if (!qual_star && (seq_star || e[10] - b[10] != lseq)) return;
  const uint32_t seq_out = 36 + nl + 1 + 4 * ncig;
  uint64_t size = (uint64_t)seq_out + (lseq + 1) / 2 + lseq;
  // tags
  for (uint32_t at = e[10]; at < len;) {  // at a tab
    const uint32_t fb = at + 1, fe = sam_next_tab(tb, fb);
    uint32_t used;
    const int32_t st = sam_tag(l, fb, fe - fb, out ? out + size : nullptr, &used);
    if (st != HBAM_OK) {
      r->status = st;
      return;
    }
    size += used;
    at = fe;
  }
  if (size > 0x7fffffffull) {
    r->status = HBAM_EUNSUPPORTED;
    return;
  }
  r->status = HBAM_OK;
  r->size = (uint32_t)size;
  r->seq_rel = b[9];
  r->l_seq = lseq;
  r->qual_star = qual_star ? 1u : 0u;
  r->seq_out = seq_out;
  if (!out) return;
  // computeIndexingBin: reg2bin(start - 1, end), end = the alignment end (1-based, inclusive: the
  // start plus the CIGAR's reference length minus one; 0 for an unmapped read), start when that is
  // not positive.  POS 0 gives reg2bin(-1, 0) = 4680.
  const int32_t pos0 = (int32_t)((uint32_t)pos1 - 1u);
  int32_t end = (flag & 4) ? 0 : (int32_t)((uint32_t)pos0 + reflen);
  if (end <= 0) end = (int32_t)((uint32_t)pos0 + 1u);
  const int32_t bin = sam_reg2bin(pos0, end);
  sam_st32(out, (uint32_t)size - 4u);
  sam_st32(out + 4, (uint32_t)ref);
  sam_st32(out + 8, (uint32_t)pos0);
  sam_st32(out + 12, (nl + 1) | ((uint32_t)mapq & 0xffu) << 8 | ((uint32_t)bin & 0xffffu) << 16);
  sam_st32(out + 16, ncig | ((uint32_t)flag & 0xffffu) << 16);
  sam_st32(out + 20, lseq);
  sam_st32(out + 24, (uint32_t)nref);
  sam_st32(out + 28, (uint32_t)pnext1 - 1u);
  sam_st32(out + 32, (uint32_t)tlen);
  sam_copy(l, 0, nl, out + 36);
  out[36 + nl] = 0;
}

// ---- SEQ and QUAL, 16 output bytes at a time (the bulk pass's units) ----------------------------
// the 4-bit code of a base by the low five bits of its byte: letters of either case share them,
// '.' (0x2e) shares 'N''s (0x4e) and '=' (0x3d) has 29.  "=ACMGRSVTWYHKDBN"
HBAM_HD uint32_t sam_base_code(uint32_t c) {
  const uint32_t k = c & 31u;
  // code by low5: 1 A=1, 2 B=14, 3 C=2, 4 D=13, 7 G=4, 8 H=11, 11 K=12, 13 M=3, 14 N=15,
  //               18 R=5, 19 S=6, 20 T=8, 22 V=7, 23 W=9, 25 Y=10, 29 '='=0
  const uint64_t lo = (1ull << 4) | (14ull << 8) | (2ull << 12) | (13ull << 16) | (4ull << 28) | (11ull << 32) |
                      (12ull << 44) | (3ull << 52) | (15ull << 56);
  const uint64_t hi = (5ull << 8) | (6ull << 12) | (8ull << 16) | (7ull << 24) | (9ull << 28) | (10ull << 36);
  return (uint32_t)((k < 16u ? lo >> (4u * k) : hi >> (4u * (k - 16u))) & 15u);
}
HBAM_HD bool sam_base_ok(uint32_t c) {
  const uint32_t letters = 1u << 1 | 1u << 2 | 1u << 3 | 1u << 4 | 1u << 7 | 1u << 8 | 1u << 11 | 1u << 13 |
                           1u << 14 | 1u << 18 | 1u << 19 | 1u << 20 | 1u << 22 | 1u << 23 | 1u << 25;
  if ((c & 0xc0u) == 0x40u) return (letters >> (c & 31u)) & 1u;
  return c == '=' || c == '.';
}
// 16 packed SEQ bytes from the 32 characters in w[0..8) (little-endian words), `nchar` of them
// real (1..32): the others pack as 0 and are not checked.  false: a byte outside the table.
HBAM_HD bool sam_seq_unit(const uint32_t (&w)[8], uint32_t nchar, uint32_t (&o)[4]) {
  bool ok = true;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    uint32_t acc = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {  // characters 8j + k: two per output byte, high nibble first
      const uint32_t ci = 8u * j + k;
      const uint32_t c = (w[ci >> 2] >> (8u * (ci & 3u))) & 0xffu;
      const bool in = ci < nchar;
      ok = ok && (!in || sam_base_ok(c));
      const uint32_t code = in ? sam_base_code(c) : 0u;
      acc |= code << (8u * (k >> 1) + ((k & 1u) ? 0u : 4u));
    }
    o[j] = acc;
  }
  return ok;
}
// 16 QUAL bytes (character - 33) from w[0..4), `nq` of them real (1..16)
HBAM_HD bool sam_qual_unit(const uint32_t (&w)[4], uint32_t nq, uint32_t (&o)[4]) {
  bool ok = true;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    uint32_t acc = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t c = (w[j] >> (8u * k)) & 0xffu;
      ok = ok && (4u * j + k >= nq || c >= 33u);
      acc |= ((c - 33u) & 0xffu) << (8u * k);
    }
    o[j] = acc;
  }
  return ok;
}

// ---- the key of a record that is not placed (BAMRecordReader.getKey :88-95) ---------------------
HBAM_HD uint64_t sam_rotl(uint64_t x, int r) { return x << r | x >> (64 - r); }
HBAM_HD uint64_t sam_fmix(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  return k ^ k >> 33;
}
// util/MurmurHash3.java:32-102 (byte[]) over get(0..n), h1 = h2 = (long)seed; the :59 h2 step kept
template <class G>
HBAM_HD int64_t sam_murmur_bytes(G get, uint32_t n, int32_t seed) {
  const uint64_t c1 = 0x87c37b91114253d5ull, c2 = 0x4cf5ad432745937full;
  uint64_t h1 = (uint64_t)(int64_t)seed, h2 = h1;
  const uint32_t nb = n / 16;
  for (uint32_t i = 0; i < nb; ++i) {
    uint64_t k1 = 0, k2 = 0;
    for (uint32_t j = 0; j < 8; ++j) {
      k1 |= (uint64_t)get(16 * i + j) << (8 * j);
      k2 |= (uint64_t)get(16 * i + 8 + j) << (8 * j);
    }
    k1 *= c1; k1 = sam_rotl(k1, 31); k1 *= c2; h1 ^= k1;
    h1 = sam_rotl(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729ull;
    k2 *= c2; k2 = sam_rotl(k2, 33); k2 *= c1; h2 ^= k2;
    h2 = h2 << 31 | h1 >> 33; h2 += h1; h2 = h2 * 5 + 0x38495ab5ull;
  }
  const uint32_t t = n & 15u;
  uint64_t k1 = 0, k2 = 0;
  for (uint32_t j = 0; j < t; ++j) {
    if (j < 8) k1 |= (uint64_t)get(16 * nb + j) << (8 * j);
    else k2 |= (uint64_t)get(16 * nb + j) << (8 * (j - 8));
  }
  if (t > 8) { k2 *= c2; k2 = sam_rotl(k2, 33); k2 *= c1; h2 ^= k2; }
  if (t > 0) { k1 *= c1; k1 = sam_rotl(k1, 31); k1 *= c2; h1 ^= k1; }
  h1 ^= n; h2 ^= n;
  h1 += h2;
  h2 += h1;
  h1 = sam_fmix(h1);
  h2 = sam_fmix(h2);
  return (int64_t)(h1 + h2);
}

}  // namespace hbam
