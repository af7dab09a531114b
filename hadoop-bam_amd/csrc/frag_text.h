// frag_text.h — one SequencedFragment (a record of hbam_frag_columns) -> one FASTQ record or one
// QSEQ line, the per-record half of hbam_fragtext.hip and the inverse of hbam_fastq.hip.  Everything
// here is plain C++ over pointers (host and device), so the rules can be run on a CPU as they stand.
//
// The rules restate FastqRecordWriter.write / makeId (FastqOutputFormat.java:94-147), its
// SequencedFragment.convertQuality (SequencedFragment.java:234-247) and QseqRecordWriter.write
// (QseqOutputFormat.java:100-159); include/hbam.h lists them.  frag_text renders everything but the
// sequence, the separator behind it and the quality; with out == nullptr it only counts and reads
// no pool or window byte, so the sizes and the bytes come from one function and cannot disagree.
// That bulk region is left to frag_text_unit (the bulk pass's 16-byte units), which also applies
// the byte transforms ('N' -> '.', + 31) and the range checks.
#pragma once
#include "sam_text.h"

namespace hbam {

// device (or host) views of the hbam_frag_columns a render reads, and the window its string pairs
// point into
struct FragIn {
  uint64_t n;
  const uint32_t* present;
  const int32_t *run, *lane, *tile, *xpos, *ypos, *read, *filter_passed, *control;
  const uint32_t *instrument, *flowcell, *index;
  const uint64_t *key_off, *seq_off, *qual_off;
  const uint8_t *key, *seq, *qual;
  uint64_t key_len, seq_len, qual_len;
  const uint8_t* window;
  uint64_t window_len;
};

constexpr uint32_t FRAG_P_INSTRUMENT = 0x001, FRAG_P_RUN = 0x002, FRAG_P_FLOWCELL = 0x004, FRAG_P_LANE = 0x008,
                   FRAG_P_TILE = 0x010, FRAG_P_XPOS = 0x020, FRAG_P_YPOS = 0x040, FRAG_P_READ = 0x080,
                   FRAG_P_FILTER = 0x100, FRAG_P_CONTROL = 0x200, FRAG_P_INDEX = 0x400;

struct FragRec {
  uint32_t present;
  int32_t run, lane, tile, xpos, ypos, read, filter_passed, control;
  uint32_t ins_o, ins_n, fc_o, fc_n, ix_o, ix_n;  // a pair whose bit is clear is (0, 0)
  uint64_t ko, so, qo;                            // pool offsets
  uint32_t kn, ls, lq;
};

// record i of the columns -> *r; false: an offset array that does not ascend or leaves its pool, a
// length of 2^31 or more, a present string pair that runs past the window (nothing of the record
// may then be read)
HBAM_HD bool frag_text_load(const FragIn& in, uint64_t i, bool want_key, FragRec* r) {
  if (i >= in.n) return false;
  const uint64_t s0 = in.seq_off[i], s1 = in.seq_off[i + 1], q0 = in.qual_off[i], q1 = in.qual_off[i + 1];
  if (s1 < s0 || s1 > in.seq_len || q1 < q0 || q1 > in.qual_len) return false;
  if (s1 - s0 > 0x7fffffffull || q1 - q0 > 0x7fffffffull) return false;
  r->so = s0;
  r->ls = (uint32_t)(s1 - s0);
  r->qo = q0;
  r->lq = (uint32_t)(q1 - q0);
  r->ko = 0;
  r->kn = 0;
  if (want_key) {
    const uint64_t k0 = in.key_off[i], k1 = in.key_off[i + 1];
    if (k1 < k0 || k1 > in.key_len || k1 - k0 > 0x7fffffffull) return false;
    r->ko = k0;
    r->kn = (uint32_t)(k1 - k0);
  }
  const uint32_t p = r->present = in.present[i];
  r->run = in.run[i];
  r->lane = in.lane[i];
  r->tile = in.tile[i];
  r->xpos = in.xpos[i];
  r->ypos = in.ypos[i];
  r->read = in.read[i];
  r->filter_passed = in.filter_passed[i];
  r->control = in.control[i];
  r->ins_o = r->ins_n = r->fc_o = r->fc_n = r->ix_o = r->ix_n = 0;
  if (p & FRAG_P_INSTRUMENT) {
    r->ins_o = in.instrument[2 * i];
    r->ins_n = in.instrument[2 * i + 1];
  }
  if (p & FRAG_P_FLOWCELL) {
    r->fc_o = in.flowcell[2 * i];
    r->fc_n = in.flowcell[2 * i + 1];
  }
  if (p & FRAG_P_INDEX) {
    r->ix_o = in.index[2 * i];
    r->ix_n = in.index[2 * i + 1];
  }
  if ((uint64_t)r->ins_o + r->ins_n > in.window_len || (uint64_t)r->fc_o + r->fc_n > in.window_len ||
      (uint64_t)r->ix_o + r->ix_n > in.window_len)
    return false;
  if ((r->ins_n | r->fc_n | r->ix_n) > 0x0fffffffu) return false;  // the line's length stays below 2^32
  return true;
}

// n bytes at s (the window: any alignment, no byte behind the string is readable)
HBAM_HD void frag_put_bytes(SamOut& w, const uint8_t* s, uint32_t n) {
  if (!w.p) {
    w.len += n;
    return;
  }
  for (uint32_t k = 0; k < n; ++k) w.put(s[k]);
}
// ... with every byte `from` written as `to`
HBAM_HD void frag_put_mapped(SamOut& w, const uint8_t* s, uint32_t n, uint32_t from, uint32_t to) {
  if (!w.p) {
    w.len += n;
    return;
  }
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t c = s[k];
    w.put(c == from ? to : c);
  }
}
HBAM_HD void frag_put_int(SamOut& w, bool present, int32_t v) {
  if (present) w.put_i32(v);
}

constexpr uint32_t FRAG_SEP_FASTQ = 3, FRAG_SEP_QSEQ = 1;  // "\n+\n" and "\t" between sequence and quality

// The record without its bulk region (sequence, separator, quality) at out, or counted with out ==
// nullptr.  *bulk_rel = the region's offset in the record's text; returns the text's length.
HBAM_HD uint64_t frag_text(const FragRec& r, const FragIn& in, int32_t format, uint32_t flags, uint8_t* out,
                           uint32_t* bulk_rel) {
  SamOut w(out);
  const uint32_t p = r.present;
  const uint8_t* const win = in.window;
  if (format == HBAM_FRAG_FASTQ) {
    w.put('@');
    if (flags & HBAM_FRAG_USE_KEY) {
      if (!w.p) {
        w.len += r.kn;
      } else {
        SamRecBytes kb(in.key + r.ko);  // (a load may pass the key by 15 bytes: the pool's slack)
        for (uint32_t k = 0; k < r.kn; ++k) w.put(kb[k]);
      }
    } else {  // makeId
      frag_put_bytes(w, win + r.ins_o, r.ins_n);
      w.put(':');
      frag_put_int(w, p & FRAG_P_RUN, r.run);
      w.put(':');
      frag_put_bytes(w, win + r.fc_o, r.fc_n);
      w.put(':');
      frag_put_int(w, p & FRAG_P_LANE, r.lane);
      w.put(':');
      frag_put_int(w, p & FRAG_P_TILE, r.tile);
      w.put(':');
      frag_put_int(w, p & FRAG_P_XPOS, r.xpos);
      w.put(':');
      frag_put_int(w, p & FRAG_P_YPOS, r.ypos);
      w.put(' ');
      frag_put_int(w, p & FRAG_P_READ, r.read);
      w.put(':');
      w.put(!(p & FRAG_P_FILTER) || r.filter_passed ? 'N' : 'Y');
      w.put(':');
      if (p & FRAG_P_CONTROL) w.put_i32(r.control);
      else w.put('0');
      w.put(':');
      if (flags & HBAM_FRAG_INDEX_DOTS) frag_put_mapped(w, win + r.ix_o, r.ix_n, '.', 'N');
      else frag_put_bytes(w, win + r.ix_o, r.ix_n);
    }
    w.put('\n');
    *bulk_rel = (uint32_t)w.len;
    w.skip(r.ls + FRAG_SEP_FASTQ + r.lq);
    w.put('\n');
  } else {
    frag_put_bytes(w, win + r.ins_o, r.ins_n);
    w.put('\t');
    frag_put_int(w, p & FRAG_P_RUN, r.run);
    w.put('\t');
    frag_put_int(w, p & FRAG_P_LANE, r.lane);
    w.put('\t');
    frag_put_int(w, p & FRAG_P_TILE, r.tile);
    w.put('\t');
    frag_put_int(w, p & FRAG_P_XPOS, r.xpos);
    w.put('\t');
    frag_put_int(w, p & FRAG_P_YPOS, r.ypos);
    w.put('\t');
    if (r.ix_n == 0) w.put('0');  // null or empty
    else frag_put_mapped(w, win + r.ix_o, r.ix_n, 'N', '.');
    w.put('\t');
    frag_put_int(w, p & FRAG_P_READ, r.read);
    w.put('\t');
    *bulk_rel = (uint32_t)w.len;
    w.skip(r.ls + FRAG_SEP_QSEQ + r.lq);
    w.put('\t');
    w.put(!(p & FRAG_P_FILTER) || r.filter_passed ? '1' : '0');
    w.put('\n');
  }
  w.flush();
  return w.len;
}

// ---- sequence, separator, quality: 16 output bytes at a time (the bulk pass's units) -------------
// The region is ls sequence bytes, the separator ("\n+\n" or "\t"), lq quality bytes.  The units are
// cut on 16-byte boundaries of the OUTPUT (sam_text_units / sam_text_unit_span), so a unit is the
// region bytes [p0, p0 + nb), nb in 1..16, written to o[0..4) (little-endian words; the bytes past
// nb are not to be stored).  Each pool is loaded 16 bytes at a time from the unit's first byte in it,
// so a load may pass the record's bytes by up to 15: inside the 16 readable bytes behind a pool.
// No load begins before the record's first byte in a pool.
constexpr uint32_t FRAG_MODE_QSEQ = 1, FRAG_MODE_ILLUMINA = 2;
constexpr uint32_t FRAG_BAD_RANGE = 1;  // FASTQ: FormatException; QSEQ: RuntimeException
constexpr uint32_t FRAG_BAD_BYTE = 2;   // QSEQ: a byte >= 0x80 (HBAM_EUNSUPPORTED)

typedef unsigned __int128 frag_u128;
constexpr uint64_t FRAG_L = 0x0101010101010101ull, FRAG_H = 0x8080808080808080ull, FRAG_7 = 0x7f7f7f7f7f7f7f7full;

HBAM_HD frag_u128 frag_ld16(const uint8_t* p) {
  uint64_t lo, hi;
  sam_ld16(p, &lo, &hi);
  return (frag_u128)hi << 64 | lo;
}
// the low n bytes set
HBAM_HD frag_u128 frag_bm(uint32_t n) { return n >= 16u ? ~(frag_u128)0 : (((frag_u128)1 << (8u * n)) - 1u); }
// per byte: (b & 0x7f) + k, k <= 0x80: no carry between bytes; bit 7 = (b & 0x7f) >= 0x80 - k
HBAM_HD uint64_t frag_add7(uint64_t x, uint32_t k) { return (x & FRAG_7) + FRAG_L * k; }
// every byte 'N' as '.' (they differ in 0x60)
HBAM_HD uint64_t frag_n_to_dot(uint64_t x) {
  const uint64_t t = x ^ (FRAG_L * 'N');
  const uint64_t zero = ~(((t & FRAG_7) + FRAG_7) | t) & FRAG_H;
  return x ^ ((zero >> 7) * 0x60u);
}
// every byte + 31 mod 256
HBAM_HD uint64_t frag_plus31(uint64_t x) { return frag_add7(x, 31) ^ (x & FRAG_H); }

// -> FRAG_BAD_* bits of the unit's own bytes
HBAM_HD uint32_t frag_text_unit(const uint8_t* seq, uint32_t ls, const uint8_t* qual, uint32_t sep, uint32_t mode,
                                uint32_t p0, uint32_t nb, uint32_t (&o)[4]) {
  const uint32_t qs = ls + sep;  // the quality's first region byte
  frag_u128 s = 0, q = 0;
  if (p0 < ls) s = frag_ld16(seq + p0);
  if (p0 + nb > qs) q = p0 >= qs ? frag_ld16(qual + (p0 - qs)) : frag_ld16(qual) << (8u * (qs - p0));
  const uint32_t a = p0 < ls ? ls - p0 : 0u;  // unit bytes below a are sequence ...
  const uint32_t b = p0 < qs ? qs - p0 : 0u;  // ... at and above b quality
  const frag_u128 valid = frag_bm(nb), ma = frag_bm(a), mb = frag_bm(b);
  const frag_u128 smask = ma & valid, qmask = valid & ~mb;
  uint64_t s0 = (uint64_t)s, s1 = (uint64_t)(s >> 64), q0 = (uint64_t)q, q1 = (uint64_t)(q >> 64);
  const uint64_t sm0 = (uint64_t)smask, sm1 = (uint64_t)(smask >> 64), qm0 = (uint64_t)qmask,
                 qm1 = (uint64_t)(qmask >> 64);
  // the bytes to check: those outside the unit's part of the pool read as '@', which passes every check
  const uint64_t at = FRAG_L * '@';
  const uint64_t c0 = (q0 & qm0) | (at & ~qm0), c1 = (q1 & qm1) | (at & ~qm1);
  uint32_t bad = 0;
  if (mode & FRAG_MODE_QSEQ) {
    if ((((s0 & sm0) | (s1 & sm1)) | (c0 | c1)) & FRAG_H) bad |= FRAG_BAD_BYTE;
    s0 = frag_n_to_dot(s0);
    s1 = frag_n_to_dot(s1);
    if (mode & FRAG_MODE_ILLUMINA) {
      // b + 31 > 126: b >= 96 (a byte >= 0x80 is FRAG_BAD_BYTE, which wins)
      if ((frag_add7(c0, 32) | frag_add7(c1, 32)) & FRAG_H) bad |= FRAG_BAD_RANGE;
      q0 = frag_plus31(q0);
      q1 = frag_plus31(q1);
    }
  } else if (mode & FRAG_MODE_ILLUMINA) {
    // a signed byte in [33, 126]: no bit 7, >= 33, not 127
    const uint64_t f0 = c0 | ~frag_add7(c0, 128 - 33) | frag_add7(c0, 1);
    const uint64_t f1 = c1 | ~frag_add7(c1, 128 - 33) | frag_add7(c1, 1);
    if ((f0 | f1) & FRAG_H) bad |= FRAG_BAD_RANGE;
    q0 = frag_plus31(q0);
    q1 = frag_plus31(q1);
  }
  // the separator's bytes, region byte ls first
  const frag_u128 sepc = sep == FRAG_SEP_FASTQ ? (frag_u128)0x0a2b0au : (frag_u128)'\t';
  const frag_u128 sepv = p0 <= ls ? (ls - p0 >= 16u ? (frag_u128)0 : sepc << (8u * (ls - p0)))
                                  : (p0 - ls >= sep ? (frag_u128)0 : sepc >> (8u * (p0 - ls)));
  const frag_u128 v = (((frag_u128)s1 << 64 | s0) & ma) | (sepv & ~ma & mb) | (((frag_u128)q1 << 64 | q0) & ~mb);
  o[0] = (uint32_t)v;
  o[1] = (uint32_t)(v >> 32);
  o[2] = (uint32_t)(v >> 64);
  o[3] = (uint32_t)(v >> 96);
  return bad;
}

}  // namespace hbam
