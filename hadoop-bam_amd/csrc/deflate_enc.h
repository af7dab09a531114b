// deflate_enc.h — what one thread of the device BGZF compressor (hbam_deflate.hip) computes on its
// own: the match hash and the common-prefix length, the RFC 1951 length / distance codes, the
// length-limited Huffman code lengths and canonical codes, the serial bit writer, and the dynamic
// block header (HLIT / HDIST, the run-length coded code lengths, the code-length code, the header
// bits).  Everything here is plain C++ over pointers (host and device), so the rules can be run on
// a CPU as they stand (tools/deflate_enc_host.cpp, with the address and undefined-behaviour
// sanitizers; tests/test_deflate_enc.py compares with tests/deflate_ref.py).  What needs the
// workgroup (staging, the chunk parse, the frequency sort, the bit offsets) stays in
// hbam_deflate.hip.
#pragma once
#include <stdint.h>

#ifndef HBAM_HD
#ifdef __HIPCC__
#define HBAM_HD __host__ __device__ inline
#else
#define HBAM_HD inline
#endif
#endif

namespace hbam {

constexpr uint32_t DF_HBITS = 11;             // 2048-entry hash heads
constexpr uint32_t DF_WINDOW = 32768;
constexpr uint32_t DF_PROBE = 16;             // match bytes verified per position in parallel
constexpr uint32_t DF_NSYM = 286 + 30;        // lit/len + distance frequencies per block
// code length limits (RFC 1951): lit/len and distance codes 15 bits, the code-length code 7
constexpr uint32_t DF_MAXL_LIT = 15;
constexpr uint32_t DF_MAXL_DIST = 15;
constexpr uint32_t DF_MAXL_CL = 7;
// scratch of the Huffman builder and the header writer, in elements (k_deflate_encode's LDS arrays)
constexpr uint32_t DF_SORTED_N = 320;
constexpr uint32_t DF_WT_N = 640;
constexpr uint32_t DF_PAR_N = 640;
constexpr uint32_t DF_RLE_N = 320;

HBAM_HD uint32_t df_hash(uint32_t w) { return (w * 2654435761u) >> (32 - DF_HBITS); }

// unaligned dword (the device runs in unaligned access mode, as k_resolve relies on)
HBAM_HD uint32_t df_lds32(const uint8_t* s, uint32_t p) {
#ifdef __HIP_DEVICE_COMPILE__
  return *(const uint32_t*)(s + p);
#else
  return (uint32_t)s[p] | (uint32_t)s[p + 1] << 8 | (uint32_t)s[p + 2] << 16 | (uint32_t)s[p + 3] << 24;
#endif
}

// length of the common prefix of s[a..] and s[p..], at most lim
HBAM_HD uint32_t df_match(const uint8_t* s, uint32_t a, uint32_t p, uint32_t lim) {
  uint32_t l = 0;
  while (l + 4 <= lim) {
    const uint32_t x = df_lds32(s, a + l) ^ df_lds32(s, p + l);
    if (x) return l + (__builtin_ctz(x) >> 3);
    l += 4;
  }
  while (l < lim && s[a + l] == s[p + l]) ++l;
  return l;
}

// RFC 1951 length code of a match length 3..258: symbol, extra bits, extra value
HBAM_HD void df_len_code(uint32_t len, uint32_t& sym, uint32_t& eb, uint32_t& ev) {
  if (len == 258) {
    sym = 285; eb = 0; ev = 0;
    return;
  }
  const uint32_t x = len - 3;
  if (x < 8) {
    sym = 257 + x; eb = 0; ev = 0;
    return;
  }
  eb = 31 - __builtin_clz(x) - 2;  // x in [8, 255]: 1..5 extra bits
  const uint32_t base = (4u + ((x >> eb) & 3u)) << eb;
  sym = 257 + 4 * eb + 4 + ((x >> eb) & 3u);
  ev = x - base;
}
// distance code of 1..32768
HBAM_HD void df_dist_code(uint32_t d, uint32_t& sym, uint32_t& eb, uint32_t& ev) {
  const uint32_t x = d - 1;
  if (x < 4) {
    sym = x; eb = 0; ev = 0;
    return;
  }
  eb = 31 - __builtin_clz(x) - 1;  // x in [4, 32767]: 1..13 extra bits
  const uint32_t hb = (x >> eb) & 1u;
  sym = 2 * eb + 2 + hb;
  ev = x - ((2u + hb) << eb);
}

// ---- Huffman code lengths (one thread): Huffman tree by two queues over the symbols sorted
// by frequency, then lengths limited to maxl.  sorted[] / wt[] / par[] are LDS scratch.
HBAM_HD void df_lengths(const uint32_t* f, uint32_t n, uint32_t maxl, uint8_t* len,
                        uint16_t* sorted, uint32_t* wt, uint16_t* par, uint32_t m) {
  // m = number of used symbols (listed in sorted[0..m) by ascending frequency)
  for (uint32_t i = 0; i < n; ++i) len[i] = 0;
  if (m == 0) return;
  if (m == 1) {
    len[sorted[0]] = 1;
    return;
  }
  // nodes: 0..m-1 leaves (in sorted order), m..2m-2 internal; two-queue merge
  for (uint32_t i = 0; i < m; ++i) wt[i] = f[sorted[i]];
  uint32_t ql = 0, qi = m, ni = m;
  for (uint32_t k = 0; k < m - 1; ++k) {
    uint32_t pick[2];
    for (int j = 0; j < 2; ++j) {
      if (ql < m && (qi >= ni || wt[ql] <= wt[qi])) pick[j] = ql++;
      else pick[j] = qi++;
    }
    wt[ni] = wt[pick[0]] + wt[pick[1]];
    par[pick[0]] = (uint16_t)ni;
    par[pick[1]] = (uint16_t)ni;
    ++ni;
  }
  // depths: root = ni - 1
  uint32_t* dep = wt;  // reuse: depth of node i (computed top-down: parents have larger ids)
  dep[ni - 1] = 0;
  for (int i = (int)ni - 2; i >= 0; --i) dep[i] = dep[par[i]] + 1;
  // bit-length counts, limited to maxl with zlib's repair step (trees.c gen_bitlen): leaves
  // deeper than maxl are clamped to maxl, which over-subscribes the code; each repair step
  // moves a leaf from the deepest level L < maxl down to L+1 and a leaf from maxl up beside
  // it, lowering the Kraft sum (in units of 2^-maxl) by exactly one.  The step count is the
  // Kraft excess itself, so the result is complete (inflate rejects incomplete lit/len and
  // code-length sets).  (r02 counted only the clamped leaves, which under-repairs any
  // subtree of 4+ leaves below depth maxl: ADVICE r02.)
  uint32_t cnt[16];
  for (int L = 0; L < 16; ++L) cnt[L] = 0;
  for (uint32_t i = 0; i < m; ++i) {
    const uint32_t d = dep[i];
    ++cnt[d > maxl ? maxl : d];
  }
  uint32_t kraft = 0;
  for (uint32_t L = 1; L <= maxl; ++L) kraft += cnt[L] << (maxl - L);
  for (uint32_t excess = kraft - (1u << maxl); excess > 0u && cnt[maxl] > 0u; --excess) {
    uint32_t L = maxl - 1;
    while (L > 0 && cnt[L] == 0) --L;
    if (L == 0) break;  // cannot happen for m <= 2^maxl leaves (guard)
    --cnt[L];
    cnt[L + 1] += 2;
    --cnt[maxl];
  }
  // lengths by frequency: the least frequent symbols (front of sorted[]) get the longest codes
  uint32_t k = 0;
  for (uint32_t L = maxl; L >= 1; --L)
    for (uint32_t c = 0; c < cnt[L]; ++c) len[sorted[k++]] = (uint8_t)L;
}

HBAM_HD uint32_t df_rev32(uint32_t v) {
#if defined(__has_builtin)
#if __has_builtin(__builtin_bitreverse32)
#define HBAM_DF_HAS_BITREVERSE 1
#endif
#endif
#ifdef HBAM_DF_HAS_BITREVERSE
  return __builtin_bitreverse32(v);
#else
  uint32_t r = 0;
  for (int k = 0; k < 32; ++k) r |= ((v >> k) & 1u) << (31 - k);
  return r;
#endif
}

// canonical codes, bit-reversed for the LSB-first bit stream
HBAM_HD void df_codes(const uint8_t* len, uint32_t n, uint16_t* code) {
  uint32_t cnt[16], next[16];
  for (int L = 0; L < 16; ++L) cnt[L] = 0;
  for (uint32_t i = 0; i < n; ++i) ++cnt[len[i]];
  cnt[0] = 0;
  uint32_t c = 0;
  for (int L = 1; L < 16; ++L) {
    c = (c + cnt[L - 1]) << 1;
    next[L] = c;
  }
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t L = len[i];
    if (!L) {
      code[i] = 0;
      continue;
    }
    const uint32_t v = next[L]++;
    code[i] = (uint16_t)(df_rev32(v) >> (32 - L));
  }
}

struct DfBits {  // serial bit writer into the LDS image (one thread)
  uint32_t* w;
  uint32_t pos;
  HBAM_HD void put(uint32_t v, uint32_t nb) {
    if (!nb) return;
    const uint64_t x = (uint64_t)v << (pos & 31u);
    w[pos >> 5] |= (uint32_t)x;
    if ((pos & 31u) + nb > 32u) w[(pos >> 5) + 1] |= (uint32_t)(x >> 32);
    pos += nb;
  }
};

// HLIT / HDIST and the run-length coded length sequence (RFC 1951 3.2.7) of the 286 lit/len and 30
// distance code lengths in len[0..316): rle[] gets sym | extra << 5 per code-length symbol, clf[19]
// their frequencies (made two symbols at least: the code-length code must be complete).  Returns
// the number of rle[] entries (at most hlit + hdist <= DF_RLE_N).
HBAM_HD uint32_t df_rle_lengths(const uint8_t* len, uint16_t* rle, uint32_t* clf, uint32_t* hlit_out,
                                uint32_t* hdist_out) {
  uint32_t hlit = 286;
  while (hlit > 257 && !len[hlit - 1]) --hlit;
  uint32_t hdist = 30;
  while (hdist > 1 && !len[286 + hdist - 1]) --hdist;
  *hlit_out = hlit;
  *hdist_out = hdist;
  for (int i = 0; i < 19; ++i) clf[i] = 0;
  uint32_t nr = 0;
  const uint32_t tot = hlit + hdist;
  uint32_t i = 0;
  while (i < tot) {
    const uint32_t v = i < hlit ? len[i] : len[286 + i - hlit];
    uint32_t r = 1;
    while (i + r < tot && (i + r < hlit ? len[i + r] : len[286 + i + r - hlit]) == v) ++r;
    uint32_t left = r;
    if (v == 0) {
      while (left >= 11) {
        const uint32_t k = left < 138 ? left : 138;
        rle[nr++] = (uint16_t)(18 | (k - 11) << 5);
        ++clf[18];
        left -= k;
      }
      if (left >= 3) {
        rle[nr++] = (uint16_t)(17 | (left - 3) << 5);
        ++clf[17];
        left = 0;
      }
    } else {
      rle[nr++] = (uint16_t)v;
      ++clf[v];
      --left;
      while (left >= 3) {
        const uint32_t k = left < 6 ? left : 6;
        rle[nr++] = (uint16_t)(16 | (k - 3) << 5);
        ++clf[16];
        left -= k;
      }
    }
    while (left) {
      rle[nr++] = (uint16_t)v;
      ++clf[v];
      --left;
    }
    i += r;
  }
  // the code-length code must be complete: at least two symbols
  uint32_t used = 0;
  for (int k = 0; k < 19; ++k) used += clf[k] ? 1u : 0u;
  if (used < 2) clf[clf[0] ? 1 : 0] += 1;
  return nr;
}

// The dynamic block's header bits from bit 0 of bw: BFINAL, BTYPE, HLIT, HDIST, HCLEN, the
// code-length code's lengths cll[19] (codes clc[19]) in RFC order, then the rle[] sequence.
HBAM_HD void df_put_header(DfBits& bw, uint32_t hlit, uint32_t hdist, const uint8_t* cll, const uint16_t* clc,
                           const uint16_t* rle, uint32_t nrle) {
  bw.put(1, 1);  // BFINAL
  bw.put(2, 2);  // dynamic
  bw.put(hlit - 257, 5);
  bw.put(hdist - 1, 5);
  const uint8_t ord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint32_t hclen = 19;
  while (hclen > 4 && !cll[ord[hclen - 1]]) --hclen;
  bw.put(hclen - 4, 4);
  for (uint32_t k = 0; k < hclen; ++k) bw.put(cll[ord[k]], 3);
  for (uint32_t k = 0; k < nrle; ++k) {
    const uint32_t sy = rle[k] & 31u, ex = rle[k] >> 5;
    bw.put(clc[sy], cll[sy]);
    if (sy == 16) bw.put(ex, 2);
    else if (sy == 17) bw.put(ex, 3);
    else if (sy == 18) bw.put(ex, 7);
  }
}

}  // namespace hbam
