// sam_text.h — one BAM record (block_size + record) -> one SAM text line, the per-record half of
// hbam_samtext.hip and the inverse of sam_line.h.  Everything here is plain C++ over pointers (host
// and device), so the rules can be run on a CPU as they stand (tools/sam_text_host.cpp).
//
// The rules restate htsjdk's SAMTextWriter.writeAlignment (htsjdk is not in the reference tree:
// parity unpinned, DESIGN.md lists them).  sam_text renders fields 1-9 and the tags; with out ==
// nullptr it only counts, so the sizes and the bytes come from one function and cannot disagree.
// SEQ \t QUAL, about two thirds of a line, is left to sam_text_unit (the bulk pass's 16-byte
// units).  A record is checked in this order and the first failure is its status: block_size
// against the record's slot, l_read_name, l_seq, the fixed lengths against block_size, the two
// reference indices, the CIGAR ops, the tags left to right; the quality bytes are checked by the
// unit function.  Every length is checked against block_size before it is used: no byte at or past
// 4 + block_size is ever asked for (a 16-byte cache load may pass it by up to 15 bytes, inside the
// 64 readable bytes behind the records).
#pragma once
#include "sam_line.h"

namespace hbam {

HBAM_HD void sam_ld16(const uint8_t* p, uint64_t* lo, uint64_t* hi) {
#ifdef __HIPCC__
  const sam_u32x4_a1 q = *reinterpret_cast<const sam_u32x4_a1*>(p);
  *lo = (uint64_t)q[0] | (uint64_t)q[1] << 32;
  *hi = (uint64_t)q[2] | (uint64_t)q[3] << 32;
#else
  const sam_u32_a1* const q = reinterpret_cast<const sam_u32_a1*>(p);
  *lo = (uint64_t)q[0] | (uint64_t)q[1] << 32;
  *hi = (uint64_t)q[2] | (uint64_t)q[3] << 32;
#endif
}

// The record's bytes through a 16-byte register cache, as SamBytes takes a line's.  The chunk is
// one 128-bit value and a byte is a shift of it: SamBytes' four words are picked by selects, which
// the compiler turns into one load through a selected address, and the struct then lives in LDS
// (32 bytes a lane, 8 KiB a workgroup) instead of registers.
struct SamRecBytes {
  const uint8_t* p;
  uint32_t at;
  unsigned __int128 w;
  HBAM_HD explicit SamRecBytes(const uint8_t* rec) : p(rec), at(~0u), w(0) {}
  HBAM_HD uint32_t operator[](uint32_t i) {
    const uint32_t c = i >> 4;
    if (c != at) {
      uint64_t lo, hi;
      sam_ld16(p + 16ull * c, &lo, &hi);
      w = (unsigned __int128)hi << 64 | lo;
      at = c;
    }
    return (uint32_t)(w >> (8u * (i & 15u))) & 0xffu;
  }
};

constexpr uint32_t SAMTEXT_FLOAT_LIMIT = 10000000u;  // |v| < 10^7: Float.toString writes N.0

// Text out, four bytes per store: the bytes gather in a register and leave as one unaligned dword
// (a lane per record pays a cache line per store instruction whatever its width).  p == nullptr:
// count only.
struct SamOut {
  uint8_t* p;
  uint32_t acc, n;
  uint64_t len;
  HBAM_HD explicit SamOut(uint8_t* out) : p(out), acc(0), n(0), len(0) {}
  HBAM_HD void put(uint32_t c) {
    ++len;
    if (!p) return;
    acc |= (c & 0xffu) << (8u * n);
    if (++n == 4u) {
      sam_st32(p, acc);
      p += 4;
      acc = 0;
      n = 0;
    }
  }
  HBAM_HD void flush() {
    if (p) {
      if (n & 2u) {
        sam_st16(p, acc);
        p += 2;
        acc >>= 16;
      }
      if (n & 1u) *p++ = (uint8_t)acc;
    }
    acc = 0;
    n = 0;
  }
  // k bytes that another pass writes
  HBAM_HD void skip(uint32_t k) {
    flush();
    len += k;
    if (p) p += k;
  }
  // decimal, without an array: the digits wait in a register, four bits each
  HBAM_HD void put_u32(uint32_t v) {
    uint64_t bcd = 0;
    uint32_t nd = 0;
    do {
      bcd = bcd << 4 | (v % 10u);
      v /= 10u;
      ++nd;
    } while (v);
    for (; nd; --nd) {
      put('0' + (uint32_t)(bcd & 15u));
      bcd >>= 4;
    }
  }
  HBAM_HD void put_i32(int32_t v) {
    if (v < 0) put('-');
    put_u32(v < 0 ? 0u - (uint32_t)v : (uint32_t)v);
  }
};

HBAM_HD uint32_t sam_rd16(SamRecBytes& b, uint32_t o) { return b[o] | b[o + 1] << 8; }
HBAM_HD uint32_t sam_rd32(SamRecBytes& b, uint32_t o) { return b[o] | b[o + 1] << 8 | b[o + 2] << 16 | b[o + 3] << 24; }

// a float32 whose Float.toString is trivially exact: +-0 and the integers below 10^7 in magnitude
// ("N.0"); *mag = |v|
HBAM_HD bool sam_float_simple(uint32_t bits, uint32_t* mag) {
  const uint32_t e = (bits >> 23) & 0xffu, m = bits & 0x7fffffu;
  *mag = 0;
  if (e == 0) return m == 0;
  if (e < 127u || e > 150u) return false;  // below 1 or at least 2^24 (Inf and NaN too)
  const uint32_t full = m | 0x800000u, s = 150u - e;
  if (full & ((1u << s) - 1u)) return false;
  const uint32_t v = full >> s;
  if (v >= SAMTEXT_FLOAT_LIMIT) return false;
  *mag = v;
  return true;
}
HBAM_HD bool sam_put_float(SamOut& w, uint32_t bits) {
  uint32_t mag;
  if (!sam_float_simple(bits, &mag)) return false;
  if (bits >> 31) w.put('-');
  w.put_u32(mag);
  w.put('.');
  w.put('0');
  return true;
}

// the value of an integer tag or array element of type t (cCsSiI) at record offset o
HBAM_HD void sam_put_int(SamOut& w, SamRecBytes& b, uint32_t t, uint32_t o) {
  switch (t) {
    case 'c': w.put_i32((int32_t)(int8_t)b[o]); break;
    case 'C': w.put_u32(b[o]); break;
    case 's': w.put_i32((int32_t)(int16_t)sam_rd16(b, o)); break;
    case 'S': w.put_u32(sam_rd16(b, o)); break;
    case 'i': w.put_i32((int32_t)sam_rd32(b, o)); break;
    default: w.put_u32(sam_rd32(b, o)); break;
  }
}
// the width of a fixed-size tag type, 0: not one
HBAM_HD uint32_t sam_type_width(uint32_t t) {
  switch (t) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    default: return 0;
  }
}

struct SamTextRec {
  int32_t status;
  uint32_t deferred;   // a float outside the device's domain, or an H tag: the host renders the line
  uint32_t len;        // the line with its '\n'; 0 for a failing or a deferred record
  uint32_t bulk_out;   // line-relative offset of SEQ \t QUAL
  uint32_t bulk_len;   // its bytes, 0 when this function wrote it ("*\t*"); a deferred record keeps
                       // its own, for the bulk pass to check the qualities without storing
  uint32_t l_seq;
  uint32_t qual_star;  // the first quality byte is 0xff: QUAL is "*"
  uint32_t seq_in;     // record-relative offset of the packed SEQ (the qualities follow it)
};

HBAM_HD void sam_put_name(SamOut& w, int32_t ref, const uint8_t* names, const uint32_t* name_off) {
  if (ref < 0) {
    w.put('*');
    return;
  }
  for (uint32_t k = name_off[ref]; k < name_off[ref + 1]; ++k) w.put(names[k]);
}

// The record in the `avail` bytes at rec (its slot: rec_off[i + 1] - rec_off[i]) -> *r, and with
// out != nullptr the line's bytes at out, all but SEQ \t QUAL.  names / name_off: the dictionary
// names back to back, n_ref + 1 offsets.
HBAM_HD void sam_text(const uint8_t* rec, uint64_t avail, const uint8_t* names, const uint32_t* name_off,
                      int32_t n_ref, uint8_t* out, SamTextRec* r) {
  *r = SamTextRec{HBAM_EFORMAT, 0, 0, 0, 0, 0, 0, 0};
  if (avail < 36) return;
  SamRecBytes b(rec);
  const int32_t bs = (int32_t)sam_rd32(b, 0);
  if (bs < 32 || (uint64_t)bs + 4u > avail) return;
  const uint32_t end = 4u + (uint32_t)bs;
  const int32_t ref = (int32_t)sam_rd32(b, 4), pos = (int32_t)sam_rd32(b, 8);
  const uint32_t w12 = sam_rd32(b, 12), w16 = sam_rd32(b, 16);
  const uint32_t lrn = w12 & 0xffu, mapq = (w12 >> 8) & 0xffu, ncig = w16 & 0xffffu, flag = w16 >> 16;
  const int32_t lseq = (int32_t)sam_rd32(b, 20), nref = (int32_t)sam_rd32(b, 24);
  const int32_t npos = (int32_t)sam_rd32(b, 28), tlen = (int32_t)sam_rd32(b, 32);
  if (lrn == 0 || lseq < 0) return;
  const uint32_t packed = ((uint32_t)lseq + 1u) / 2u;
  if (32ull + lrn + 4ull * ncig + packed + (uint32_t)lseq > (uint64_t)bs) return;
  if (ref < -1 || ref >= n_ref || nref < -1 || nref >= n_ref) {
    r->status = HBAM_EREFID;
    return;
  }
  SamOut w(out);
  for (uint32_t k = 0; k + 1 < lrn; ++k) w.put(b[36 + k]);
  w.put('\t');
  w.put_u32(flag);
  w.put('\t');
  sam_put_name(w, ref, names, name_off);
  w.put('\t');
  w.put_i32((int32_t)((uint32_t)pos + 1u));
  w.put('\t');
  w.put_u32(mapq);
  w.put('\t');
  const uint32_t cig = 36u + lrn;
  if (ncig == 0) w.put('*');
  for (uint32_t k = 0; k < ncig; ++k) {
    const uint32_t c = sam_rd32(b, cig + 4u * k), op = c & 15u;
    if (op > 8u) {
      r->status = HBAM_EREFID;
      return;
    }
    w.put_u32(c >> 4);
    // "MIDNSHP=X"
    w.put((uint32_t)((op < 8u ? 0x3d5048534e44494dull >> (8u * op) : (uint64_t)'X') & 0xffu));
  }
  w.put('\t');
  if (nref >= 0 && nref == ref) w.put('=');
  else sam_put_name(w, nref, names, name_off);
  w.put('\t');
  w.put_i32((int32_t)((uint32_t)npos + 1u));
  w.put('\t');
  w.put_i32(tlen);
  w.put('\t');
  const uint32_t seq_in = cig + 4u * ncig, qual_in = seq_in + packed;
  const uint32_t bulk_out = (uint32_t)w.len;
  uint32_t qual_star = 0, bulk_len = 0;
  if (lseq == 0) {
    w.put('*');
    w.put('\t');
    w.put('*');
  } else {
    qual_star = b[qual_in] == 0xffu ? 1u : 0u;
    bulk_len = (uint32_t)lseq + 1u + (qual_star ? 1u : (uint32_t)lseq);
    w.skip(bulk_len);
  }
  // tags
  uint32_t deferred = 0;
  uint32_t p = qual_in + (uint32_t)lseq;
  while (p < end) {
    if (end - p < 3u) return;  // a tag that runs past the record
    const uint32_t t = b[p + 2];
    w.put('\t');
    w.put(b[p]);
    w.put(b[p + 1]);
    w.put(':');
    p += 3;
    const uint32_t width = sam_type_width(t);
    if (width) {
      if (end - p < width) return;
      w.put(t == 'A' || t == 'f' ? t : (uint32_t)'i');
      w.put(':');
      if (t == 'A') w.put(b[p]);
      else if (t == 'f') deferred |= sam_put_float(w, sam_rd32(b, p)) ? 0u : 1u;
      else sam_put_int(w, b, t, p);
      p += width;
    } else if (t == 'Z' || t == 'H') {
      w.put(t);
      w.put(':');
      for (;; ++p) {
        if (p >= end) return;  // no NUL
        const uint32_t c = b[p];
        if (c == 0) break;
        w.put(c);
      }
      ++p;
      if (t == 'H') deferred = 1;
    } else if (t == 'B') {
      if (end - p < 5u) return;
      const uint32_t sub = b[p], ew = sam_type_width(sub);
      const int32_t cnt = (int32_t)sam_rd32(b, p + 1);
      if (ew == 0 || sub == 'A' || cnt < 0) return;
      p += 5;
      if ((uint64_t)ew * (uint32_t)cnt > (uint64_t)(end - p)) return;
      w.put('B');
      w.put(':');
      w.put(sub);
      for (int32_t k = 0; k < cnt; ++k, p += ew) {
        w.put(',');
        if (sub == 'f') deferred |= sam_put_float(w, sam_rd32(b, p)) ? 0u : 1u;
        else sam_put_int(w, b, sub, p);
      }
    } else {
      return;  // an unknown tag type
    }
  }
  w.put('\n');
  w.flush();
  if (w.len > 0x7fffffffull) {
    r->status = HBAM_EUNSUPPORTED;
    return;
  }
  r->status = HBAM_OK;
  r->deferred = deferred;
  r->len = deferred ? 0u : (uint32_t)w.len;
  r->bulk_out = bulk_out;
  r->bulk_len = bulk_len;
  r->l_seq = (uint32_t)lseq;
  r->qual_star = qual_star;
  r->seq_in = seq_in;
}

// ---- SEQ \t QUAL, 16 output bytes at a time (the bulk pass's units) -----------------------------
// The region is l_seq bases, a tab, then l_seq qualities + 33 or "*".  The units are cut on 16-byte
// boundaries of the OUTPUT, so an edge unit is partial: a unit is the region bytes [p0, p0 + nb),
// nb in 1..16, written to o[0..4) (little-endian words; the bytes past nb are not to be stored).
// seq = the packed SEQ in the record, the qualities stand (l_seq + 1) / 2 bytes behind it.  The
// two 16-byte loads stay inside the record and the 15 bytes behind its last quality.
// false: a quality byte above 93.
HBAM_HD uint32_t sam_base_char(uint32_t nib) {  // "=ACMGRSVTWYHKDBN"
  const uint64_t t = nib < 8u ? 0x565352474d43413dull : 0x4e42444b48595754ull;
  return (uint32_t)(t >> (8u * (nib & 7u))) & 0xffu;
}
HBAM_HD bool sam_text_unit(const uint8_t* seq, uint32_t lseq, uint32_t qual_star, uint32_t p0, uint32_t nb,
                           uint32_t (&o)[4]) {
  const uint8_t* const qual = seq + (lseq + 1u) / 2u;
  uint64_t nibs = 0, qlo = 0, qhi = 0;
  if (p0 < lseq) {
    // bases p0 .. p0 + 15 = the nibbles from p0 on, high nibble first: swap the nibbles of every
    // byte and the sequence order is the bit order
    uint64_t lo, hi;
    sam_ld16(seq + (p0 >> 1), &lo, &hi);
    const uint64_t m = 0x0f0f0f0f0f0f0f0full;
    lo = (lo & m) << 4 | ((lo >> 4) & m);
    hi = (hi & m) << 4 | ((hi >> 4) & m);
    nibs = (p0 & 1u) ? (lo >> 4 | hi << 60) : lo;
  }
  const bool quals = !qual_star && p0 + nb > lseq + 1u;
  // byte j of this load is quality p0 + j - (l_seq + 1); at or before the tab it starts inside the
  // record's earlier bytes, which are not selected
  if (quals) sam_ld16(qual + (int64_t)p0 - (int64_t)(lseq + 1u), &qlo, &qhi);
  bool ok = true;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    uint32_t acc = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t i = 4u * j + k, p = p0 + i;
      const uint32_t q = (uint32_t)((i < 8u ? qlo >> (8u * i) : qhi >> (8u * (i - 8u))) & 0xffu);
      uint32_t c;
      if (p < lseq) c = sam_base_char((uint32_t)(nibs >> (4u * i)) & 15u);
      else if (p == lseq) c = '\t';
      else if (qual_star) c = '*';
      else {
        c = q + 33u;
        ok = ok && (i >= nb || q <= 93u);
      }
      acc |= (c & 0xffu) << (8u * k);
    }
    o[j] = acc;
  }
  return ok;
}

// the units of a region of `len` bytes that begins at output offset R (len > 0)
HBAM_HD uint32_t sam_text_units(uint64_t R, uint32_t len) {
  return len ? (uint32_t)(((R + len + 15u) >> 4) - (R >> 4)) : 0u;
}
// unit k of that region: its first region byte and its length
HBAM_HD void sam_text_unit_span(uint64_t R, uint32_t len, uint32_t k, uint32_t* p0, uint32_t* nb) {
  const uint64_t lo = k ? ((R >> 4) + k) << 4 : R;
  const uint64_t nxt = ((R >> 4) + k + 1u) << 4;
  const uint64_t hi = nxt < R + len ? nxt : R + len;
  *p0 = (uint32_t)(lo - R);
  *nb = (uint32_t)(hi - lo);
}

}  // namespace hbam
