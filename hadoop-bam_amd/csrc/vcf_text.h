// vcf_text.h — one BCF2 record (l_shared | l_indiv | site | genotypes) -> one VCF text line, the
// per-record half of hbam_vcftext.hip.  Everything here is plain C++ over pointers (host and
// device), as sam_text.h is for SAM text.
//
// The rules restate htsjdk's VCFEncoder and the BCF2 value decoders (htsjdk is not in the reference
// tree: parity unpinned; include/hbam.h at hbam_vcf_render and DESIGN.md list them).  Every function
// that writes takes a SamOut, which only counts without an output pointer, so a line's size and its
// bytes come from the same code and cannot disagree.
//
// A record is checked in this order and the first failure is its status: the frame (l_shared,
// l_indiv against the bytes behind the record's offset), CHROM, the sample count, n_allele, ID, the
// alleles, FILTER, the INFO pairs left to right, the genotype fields' keys and descriptors left to
// right (vcf_geno_headers), then the samples' GT calls and the FORMAT key rule (vcf_geno_scan /
// vcf_geno_keys).  A deferred record is checked like any other.  Every typed value's extent is
// checked against its block's end before a byte of it is read: no byte at or past 8 + l_shared +
// l_indiv is ever asked for (a 16-byte cache load may pass it by up to 15 bytes, inside the 64
// readable bytes behind the records).
//
// The genotype block is stored field by field and VCF text wants it sample by sample.  Nothing is
// tabled: vcf_field walks the field headers (two typed descriptors each) with a cursor, so fields in
// order cost one step each; the per-record key order is a 4-bit list in one register.
#pragma once
#include "sam_text.h"

namespace hbam {

struct VcfMeta {  // hbam_vcf_meta with device pointers, and the header's counts
  const uint8_t* contig;
  const uint32_t* contig_off;
  const uint8_t* dict;
  const uint32_t* dict_off;
  const uint32_t* rank;
  const uint32_t* flags;
  const int32_t* number;
  int32_t n_contig, n_dict, n_sample;
};

constexpr uint32_t VCF_MISSING_FLOAT = 0x7F800001u;
constexpr uint32_t VCF_F_1 = 0x3F800000u;       // 1.0f
constexpr uint32_t VCF_F_1E7 = 0x4B189680u;     // 10^7 (exact in float32)
constexpr uint32_t VCF_F_GE_001 = 0x3C23D70Bu;  // the smallest float32 that is >= the double 0.01
constexpr uint32_t VCF_NO_FIELD = 0xffffffffu;

HBAM_HD uint32_t vcf_tb(uint32_t t) { return t == 1 ? 1u : t == 2 ? 2u : (t == 3 || t == 5) ? 4u : t == 7 ? 1u : 0u; }
HBAM_HD bool vcf_is_int(uint32_t t) { return t - 1u < 3u; }
HBAM_HD int32_t vcf_int(SamRecBytes& b, uint32_t o, uint32_t t) {
  return t == 1 ? (int32_t)(int8_t)b[o] : t == 2 ? (int32_t)(int16_t)sam_rd16(b, o) : (int32_t)sam_rd32(b, o);
}
HBAM_HD int32_t vcf_int_missing(uint32_t t) { return t == 1 ? -128 : t == 2 ? -32768 : (int32_t)0x80000000u; }
HBAM_HD uint32_t vcf_kind(const VcfMeta& M, uint32_t key) { return (M.flags[key] >> 4) & 7u; }

// A typed value's descriptor at *at inside a block that ends at `end` (record-relative offsets), as
// bcf_typed reads it; the values are `mult` vectors of k (the samples of a genotype field).  *at
// moves behind the descriptor, not behind the values.
struct VcfTV {
  uint32_t t, k, off;
};
HBAM_HD int32_t vcf_typed(SamRecBytes& b, uint32_t end, uint32_t* at, uint32_t mult, VcfTV* v) {
  if (*at >= end) return HBAM_ETRIBBLE;
  const uint32_t d = b[(*at)++];
  uint32_t t = d & 15u, k = d >> 4;
  if (k == 15u) {
    if (*at >= end) return HBAM_ETRIBBLE;
    const uint32_t t2 = b[(*at)++] & 15u;
    if (!vcf_is_int(t2)) return HBAM_ERUNTIME;
    if (end - *at < vcf_tb(t2)) return HBAM_ETRIBBLE;
    const int32_t kk = vcf_int(b, *at, t2);
    *at += vcf_tb(t2);
    k = kk < 0 ? 0u : (uint32_t)kk;
  }
  v->t = t;
  v->k = k;
  v->off = *at;
  if (k == 0) return HBAM_OK;
  const uint32_t tb = vcf_tb(t);
  if (!tb) return HBAM_ERUNTIME;
  if ((uint64_t)k * tb * mult > (uint64_t)(end - *at)) return HBAM_ETRIBBLE;
  return HBAM_OK;
}

// a string's bytes without its trailing NULs
HBAM_HD uint32_t vcf_str_len(SamRecBytes& b, uint32_t off, uint32_t k) {
  while (k && b[off + k - 1] == 0) --k;
  return k;
}

// decodeTypedValue(...) == null
HBAM_HD bool vcf_value_null(SamRecBytes& b, uint32_t t, uint32_t k, uint32_t off) {
  if (k == 0) return true;
  if (t == 7) return vcf_str_len(b, off, k) == 0;
  if (t == 5) {
    for (uint32_t i = 0; i < k; ++i)
      if (sam_rd32(b, off + 4u * i) != VCF_MISSING_FLOAT) return false;
    return true;
  }
  const uint32_t tb = vcf_tb(t);
  for (uint32_t i = 0; i < k; ++i)
    if (vcf_int(b, off + tb * i, t) != vcf_int_missing(t)) return false;
  return true;
}

// round_half_up(v * 10^D) as I.FFF for a finite float32 v in [0, 10^7): exact integer arithmetic on
// the mantissa and the exponent.  drop00: QUAL's rule, a fraction of zeros is not written.
HBAM_HD void vcf_put_fixed(SamOut& w, uint32_t bits, uint32_t D, bool drop00) {
  const uint32_t ex = (bits >> 23) & 0xffu;
  const uint32_t m = ex ? (bits & 0x7fffffu) | 0x800000u : bits & 0x7fffffu;
  const uint32_t s = 150u - (ex ? ex : 1u);  // v = m / 2^s; v < 2^24, so s >= 0
  const uint32_t p10 = D == 3u ? 1000u : 100u;
  const uint64_t P = (uint64_t)m * p10;      // < 2^34
  const uint64_t N = s == 0 ? P : s > 40u ? 0 : (P >> s) + ((P >> (s - 1u)) & 1u);
  const uint32_t ip = (uint32_t)(N / p10), fp = (uint32_t)(N % p10);
  w.put_u32(ip);
  if (drop00 && fp == 0) return;
  w.put('.');
  if (D == 3u) w.put('0' + fp / 100u);
  w.put('0' + fp / 10u % 10u);
  w.put('0' + fp % 10u);
}
// formatVCFDouble inside the device's domain; false: the host renders this record
HBAM_HD bool vcf_put_float(SamOut& w, uint32_t bits) {
  if ((bits & 0x7fffffffu) == 0) {
    w.put('0');
    w.put('.');
    w.put('0');
    w.put('0');
    return true;
  }
  if ((bits >> 31) || bits >= VCF_F_1E7 || bits < VCF_F_GE_001) return false;
  vcf_put_fixed(w, bits, bits >= VCF_F_1 ? 2u : 3u, false);
  return true;
}
// QUAL: false outside the domain (negative, not finite, >= 10^7, or 8q an odd integer: a %.2f tie)
HBAM_HD bool vcf_put_qual(SamOut& w, uint32_t bits) {
  if (bits == VCF_MISSING_FLOAT) {
    w.put('.');
    return true;
  }
  if ((bits >> 31) || bits >= VCF_F_1E7) return false;
  const uint32_t ex = (bits >> 23) & 0xffu;
  const uint32_t m = ex ? (bits & 0x7fffffu) | 0x800000u : bits & 0x7fffffu;
  if (m) {
    uint32_t tz = 0;
    while (!((m >> tz) & 1u)) ++tz;
    if ((int32_t)(ex ? ex : 1u) - 150 + (int32_t)tz == -3) return false;
  }
  vcf_put_fixed(w, bits, 2u, true);
  return true;
}

// the text of a non-null value (INFO, generic FORMAT); *defer: a float outside the domain
HBAM_HD void vcf_put_value(SamOut& w, SamRecBytes& b, uint32_t t, uint32_t k, uint32_t off, uint32_t* defer) {
  if (t == 7) {
    const uint32_t n = vcf_str_len(b, off, k);
    for (uint32_t i = b[off] == ',' ? 1u : 0u; i < n; ++i) w.put(b[off + i]);
    return;
  }
  const uint32_t tb = vcf_tb(t);
  bool first = true;
  for (uint32_t i = 0; i < k; ++i) {
    const uint32_t o = off + tb * i;
    if (t == 5) {
      const uint32_t f = sam_rd32(b, o);
      if (f == VCF_MISSING_FLOAT) continue;
      if (!first) w.put(',');
      if (!vcf_put_float(w, f)) *defer = 1;
    } else {
      const int32_t v = vcf_int(b, o, t);
      if (v == vcf_int_missing(t)) continue;
      if (!first) w.put(',');
      w.put_i32(v);
    }
    first = false;
  }
}

HBAM_HD void vcf_put_name(SamOut& w, const uint8_t* names, const uint32_t* off, uint32_t i) {
  for (uint32_t k = off[i]; k < off[i + 1]; ++k) w.put(names[k]);
}

// an allele of n > 0 bytes: symbolic ones as they are, the others with a-z upper-cased
HBAM_HD void vcf_put_allele(SamOut& w, SamRecBytes& b, uint32_t off, uint32_t n) {
  const uint32_t c0 = b[off], c1 = b[off + n - 1];
  bool sym = (c0 == '<' && c1 == '>') || c0 == '.' || c1 == '.';
  for (uint32_t i = 0; i < n && !sym; ++i) {
    const uint32_t c = b[off + i];
    sym = c == '[' || c == ']';
  }
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c = b[off + i];
    w.put(!sym && c - 'a' < 26u ? c - 32u : c);
  }
}

struct VcfRec {
  int32_t status;
  uint32_t deferred;
  uint32_t len;       // the bytes written / counted by vcf_text
  uint32_t by_wave;   // vcf_text stopped behind INFO: the samples are a wave's work
  uint32_t n_allele, n_sample, n_fmt;
  uint32_t indiv, end;  // the genotype block, record-relative
  uint32_t gt_f;        // the GT field's index, VCF_NO_FIELD without one
};

// ---- the genotype block ------------------------------------------------------------------------
struct VcfField {
  uint32_t key, t, k, off, tb;  // off: sample 0's first value; sample s stands s * k * tb behind it
};
struct VcfFmtCur {
  uint32_t f, at;
};
// field f of a block whose headers vcf_geno_headers accepted
HBAM_HD VcfField vcf_field(SamRecBytes& b, const VcfRec& R, VcfFmtCur& c, uint32_t f) {
  if (f < c.f) c = VcfFmtCur{0, R.indiv};
  for (;;) {
    VcfTV kv{0, 0, 0}, dv{0, 0, 0};
    uint32_t at = c.at;
    vcf_typed(b, R.end, &at, 1, &kv);
    const uint32_t key = (uint32_t)vcf_int(b, kv.off, kv.t);
    at = kv.off + vcf_tb(kv.t);
    vcf_typed(b, R.end, &at, R.n_sample, &dv);
    const uint32_t tb = vcf_tb(dv.t);
    if (c.f == f) return VcfField{key, dv.t, dv.k, dv.off, tb};
    ++c.f;
    c.at = dv.off + dv.k * tb * R.n_sample;
  }
}

// The fields' keys and descriptors, left to right.  Sets R->gt_f and the deferral that the headers
// alone decide: a float or char field, an FT, more fields or alleles per call than the caps.
HBAM_HD void vcf_geno_headers(SamRecBytes& b, const VcfMeta& M, VcfRec* R) {
  uint32_t at = R->indiv;
  R->gt_f = VCF_NO_FIELD;
  if (R->n_fmt > HBAM_VCF_MAX_FORMAT) R->deferred = 1;
  for (uint32_t f = 0; f < R->n_fmt; ++f) {
    VcfTV kv{0, 0, 0}, dv{0, 0, 0};
    int32_t rc = vcf_typed(b, R->end, &at, 1, &kv);
    if (rc == HBAM_OK && !(kv.k == 1 && vcf_is_int(kv.t))) rc = HBAM_ERUNTIME;
    int32_t key = 0;
    if (rc == HBAM_OK) {
      key = vcf_int(b, kv.off, kv.t);
      at = kv.off + vcf_tb(kv.t);
      if (key < 0 || key >= M.n_dict || !(M.flags[key] & HBAM_VCF_HAS_FORMAT)) rc = HBAM_ERUNTIME;
    }
    if (rc == HBAM_OK) rc = vcf_typed(b, R->end, &at, R->n_sample, &dv);
    if (rc == HBAM_OK) {
      const uint32_t kind = vcf_kind(M, (uint32_t)key);
      const bool ints = dv.k == 0 || vcf_is_int(dv.t);
      if (kind == HBAM_VCF_KIND_GT) {
        if (!ints || R->gt_f != VCF_NO_FIELD) rc = HBAM_ERUNTIME;
        R->gt_f = f;
        if (dv.k > HBAM_VCF_MAX_PLOIDY) R->deferred = 1;
      } else if (kind == HBAM_VCF_KIND_DP || kind == HBAM_VCF_KIND_GQ) {
        if (dv.k != 1) rc = HBAM_EUNSUPPORTED;
        else if (!ints) rc = HBAM_ERUNTIME;
      } else if (kind == HBAM_VCF_KIND_AD || kind == HBAM_VCF_KIND_PL) {
        if (!ints) rc = HBAM_ERUNTIME;
      } else if (kind == HBAM_VCF_KIND_FT || !ints) {
        R->deferred = 1;
      }
    }
    if (rc != HBAM_OK) {
      R->status = rc;
      return;
    }
    at = dv.off + dv.k * vcf_tb(dv.t) * R->n_sample;
  }
}

// is field F null in sample s (what calcVCFGenotypeKeys and the trailing-value rule ask)
HBAM_HD bool vcf_fmt_null(SamRecBytes& b, const VcfField& F, uint32_t kind, uint32_t s) {
  if (F.k == 0) return true;
  const uint32_t o = F.off + s * F.k * F.tb;
  if (kind == HBAM_VCF_KIND_GENERIC || kind == HBAM_VCF_KIND_FT) return vcf_value_null(b, F.t, F.k, o);
  return vcf_int(b, o, F.t) == vcf_int_missing(F.t);  // decodeIntArray: nothing before the first missing value
}

// What a pass over samples learns; the lanes of a wave OR theirs together.
struct VcfScan {
  uint32_t present;  // bit f: field f (not GT) is non-null in some sample; bit 31: such a field past the cap
  uint32_t nullm;    // bit f: field f is null in some sample
  uint32_t gt_present, gt_null;  // some sample's GT array is non-null / null (or there is no GT field)
  uint32_t bad;      // a GT allele outside [0, n_allele]
};
HBAM_HD void vcf_geno_scan(SamRecBytes& b, const VcfMeta& M, const VcfRec& R, uint32_t s0, uint32_t stride,
                           VcfScan* a) {
  VcfFmtCur c{0, R.indiv};
  for (uint32_t s = s0; s < R.n_sample; s += stride) {
    if (R.gt_f == VCF_NO_FIELD) a->gt_null = 1;
    for (uint32_t f = 0; f < R.n_fmt; ++f) {
      const VcfField F = vcf_field(b, R, c, f);
      const uint32_t kind = vcf_kind(M, F.key);
      const bool null = vcf_fmt_null(b, F, kind, s);
      if (kind == HBAM_VCF_KIND_GT) {
        if (null) a->gt_null = 1;
        else a->gt_present = 1;
        const uint32_t o = F.off + s * F.k * F.tb;
        for (uint32_t i = 0; i < F.k; ++i) {
          const int32_t v = vcf_int(b, o + i * F.tb, F.t);
          if (v == vcf_int_missing(F.t)) break;
          if ((v >> 1) < 0 || (v >> 1) > (int32_t)R.n_allele) a->bad = 1;
        }
      } else {
        const uint32_t bit = f < HBAM_VCF_MAX_FORMAT ? 1u << f : 1u << 31;
        if (null) a->nullm |= bit;
        else a->present |= bit;
      }
    }
  }
}

// calcVCFGenotypeKeys from the scan of all samples
struct VcfKeys {
  uint64_t order;   // 4 bits a key: the field indices of the keys behind GT, ascending by name
  uint32_t n;       // their number
  uint32_t gt;      // GT is a key
};
HBAM_HD void vcf_geno_keys(SamRecBytes& b, const VcfMeta& M, VcfRec* R, const VcfScan& a, VcfKeys* K) {
  *K = VcfKeys{0, 0, 0};
  if (R->n_sample == 0) return;
  K->gt = a.gt_present || a.present == 0;  // an empty set is written as [GT]
  if (a.bad || (K->gt && a.gt_null)) {
    R->status = HBAM_ERUNTIME;
    return;
  }
  if (R->deferred) return;  // (more fields than the order holds, among others)
  VcfFmtCur c{0, R->indiv};
  int64_t last = -1;
  for (;;) {
    int64_t best = INT64_MAX;
    uint32_t bf = 0;
    for (uint32_t f = 0; f < R->n_fmt; ++f) {
      if (!((a.present >> f) & 1u)) continue;
      const VcfField F = vcf_field(b, *R, c, f);
      // (rank, field): a key stored twice is written twice, in field order
      const int64_t rk = (int64_t)M.rank[F.key] << 5 | f;
      if (rk > last && rk < best) {
        best = rk;
        bf = f;
      }
      if (M.number[F.key] == HBAM_VCF_NUMBER_G && ((a.nullm >> f) & 1u) && vcf_kind(M, F.key) == HBAM_VCF_KIND_GENERIC)
        R->deferred = 1;
    }
    if (best == INT64_MAX) break;
    K->order |= (uint64_t)bf << (4u * K->n);
    ++K->n;
    last = best;
  }
}

// \tGT:KEY:KEY
HBAM_HD void vcf_put_format(SamOut& w, SamRecBytes& b, const VcfMeta& M, const VcfRec& R, const VcfKeys& K) {
  VcfFmtCur c{0, R.indiv};
  w.put('\t');
  if (K.gt) {
    w.put('G');
    w.put('T');
  }
  for (uint32_t j = 0; j < K.n; ++j) {
    if (j || K.gt) w.put(':');
    vcf_put_name(w, M.dict, M.dict_off, vcf_field(b, R, c, (uint32_t)(K.order >> (4u * j)) & 15u).key);
  }
}

// \t and sample s's column
HBAM_HD void vcf_put_sample(SamOut& w, SamRecBytes& b, const VcfMeta& M, const VcfRec& R, const VcfKeys& K,
                            uint32_t s) {
  VcfFmtCur c{0, R.indiv};
  w.put('\t');
  if (K.gt) {
    const VcfField F = vcf_field(b, R, c, R.gt_f);
    const uint32_t o = F.off + s * F.k * F.tb;
    const uint32_t sep = (vcf_int(b, o, F.t) & 1) ? '|' : '/';
    for (uint32_t i = 0; i < F.k; ++i) {
      const int32_t v = vcf_int(b, o + i * F.tb, F.t);
      if (v == vcf_int_missing(F.t)) break;
      if (i) w.put(sep);
      if ((v >> 1) == 0) w.put('.');
      else w.put_u32((uint32_t)(v >> 1) - 1u);
    }
  }
  // the keys up to the last one whose value is not null: the trailing ones are dropped
  uint32_t keep = 0;
  for (uint32_t j = 0; j < K.n; ++j) {
    const VcfField F = vcf_field(b, R, c, (uint32_t)(K.order >> (4u * j)) & 15u);
    if (!vcf_fmt_null(b, F, vcf_kind(M, F.key), s)) keep = j + 1u;
  }
  for (uint32_t j = 0; j < keep; ++j) {
    if (j || K.gt) w.put(':');
    const VcfField F = vcf_field(b, R, c, (uint32_t)(K.order >> (4u * j)) & 15u);
    const uint32_t kind = vcf_kind(M, F.key), o = F.off + s * F.k * F.tb;
    if (vcf_fmt_null(b, F, kind, s)) {
      uint32_t dots = 1;
      if (kind == HBAM_VCF_KIND_GENERIC) {
        const int32_t num = M.number[F.key];
        const int32_t cnt = num == HBAM_VCF_NUMBER_A ? (int32_t)R.n_allele - 1 : num == HBAM_VCF_NUMBER_R ? (int32_t)R.n_allele : num;
        if (cnt > 1) dots = (uint32_t)cnt;
      }
      w.put('.');
      for (uint32_t i = 1; i < dots; ++i) {
        w.put(',');
        w.put('.');
      }
    } else if (kind == HBAM_VCF_KIND_GENERIC) {
      uint32_t defer = 0;
      vcf_put_value(w, b, F.t, F.k, o, &defer);
    } else {  // DP, GQ: the value; AD, PL: the values before the first missing one
      for (uint32_t i = 0; i < F.k; ++i) {
        const int32_t v = vcf_int(b, o + i * F.tb, F.t);
        if (v == vcf_int_missing(F.t)) break;
        if (i) w.put(',');
        w.put_i32(v);
      }
    }
  }
}

// ---- the line ----------------------------------------------------------------------------------
// The record in the `avail` bytes at rec (data_len - rec_off[i]) -> *r and, with out != nullptr, the
// line's bytes at out.  A record of wave_cut samples or more stops behind INFO (r->by_wave): the
// caller renders FORMAT, the samples and the '\n' (hbam_vcftext.hip's wave kernels).
HBAM_HD void vcf_text(const uint8_t* rec, uint64_t avail, const VcfMeta& M, uint32_t wave_cut, uint8_t* out,
                      VcfRec* r) {
  *r = VcfRec{HBAM_ETRIBBLE, 0, 0, 0, 0, 0, 0, 0, 0, VCF_NO_FIELD};
  if (avail < 8) return;
  SamRecBytes b(rec);
  const int32_t ls = (int32_t)sam_rd32(b, 0), li = (int32_t)sam_rd32(b, 4);
  if (ls < 24 || li < 0 || 8ull + (uint32_t)ls + (uint32_t)li > avail) return;
  const uint32_t send = 8u + (uint32_t)ls;
  r->indiv = send;
  r->end = send + (uint32_t)li;
  const int32_t chrom = (int32_t)sam_rd32(b, 8), pos = (int32_t)sam_rd32(b, 12);
  const uint32_t qual = sam_rd32(b, 20), nai = sam_rd32(b, 24), nfs = sam_rd32(b, 28);
  const uint32_t n_allele = nai >> 16, n_info = nai & 0xffffu;
  r->n_allele = n_allele;
  r->n_sample = nfs & 0xffffffu;
  r->n_fmt = nfs >> 24;
  if (chrom < 0 || chrom >= M.n_contig) {
    r->status = HBAM_ERUNTIME;
    return;
  }
  if ((int32_t)r->n_sample != M.n_sample || n_allele < 1) return;
  SamOut w(out);
  uint32_t deferred = 0, at = 32;
  int32_t rc;
  VcfTV v{0, 0, 0};
#define VCF_FAIL(code)  \
  do {                  \
    r->status = (code); \
    return;             \
  } while (0)
  vcf_put_name(w, M.contig, M.contig_off, (uint32_t)chrom);
  w.put('\t');
  w.put_i32((int32_t)((uint32_t)pos + 1u));
  w.put('\t');
  if ((rc = vcf_typed(b, send, &at, 1, &v))) VCF_FAIL(rc);  // ID
  if (v.k && v.t != 7) VCF_FAIL(HBAM_ERUNTIME);
  {
    const uint32_t n = v.k ? vcf_str_len(b, v.off, v.k) : 0;
    if (n == 0) w.put('.');
    for (uint32_t i = 0; i < n; ++i) w.put(b[v.off + i]);
    at = v.off + v.k;
  }
  for (uint32_t a = 0; a < n_allele; ++a) {
    if ((rc = vcf_typed(b, send, &at, 1, &v))) VCF_FAIL(rc);
    if (v.k && v.t != 7) VCF_FAIL(HBAM_ERUNTIME);
    const uint32_t n = v.k ? vcf_str_len(b, v.off, v.k) : 0;
    if (n == 0) VCF_FAIL(HBAM_ERUNTIME);
    w.put(a == 0 || a == 1 ? '\t' : ',');
    vcf_put_allele(w, b, v.off, n);
    at = v.off + v.k;
  }
  if (n_allele == 1) {
    w.put('\t');
    w.put('.');
  }
  w.put('\t');
  if (!vcf_put_qual(w, qual)) deferred = 1;
  w.put('\t');
  // FILTER: the distinct entries ascending by name (each pass takes the smallest one not yet written)
  if ((rc = vcf_typed(b, send, &at, 1, &v))) VCF_FAIL(rc);
  if (v.k && !vcf_is_int(v.t)) VCF_FAIL(HBAM_ERUNTIME);
  {
    const uint32_t tb = vcf_tb(v.t);
    for (uint32_t i = 0; i < v.k; ++i) {
      const int32_t e = vcf_int(b, v.off + i * tb, v.t);
      if (e < 0 || e >= M.n_dict) VCF_FAIL(HBAM_ERUNTIME);
    }
    if (v.k > HBAM_VCF_MAX_FILTER) deferred = 1;
    else if (v.k == 0) w.put('.');
    else {
      int64_t last = -1;
      for (;;) {
        int64_t best = INT64_MAX;
        uint32_t be = 0;
        for (uint32_t i = 0; i < v.k; ++i) {
          const uint32_t e = (uint32_t)vcf_int(b, v.off + i * tb, v.t);
          const int64_t rk = M.rank[e];
          if (rk > last && rk < best) {
            best = rk;
            be = e;
          }
        }
        if (best == INT64_MAX) break;
        if (last >= 0) w.put(';');
        vcf_put_name(w, M.dict, M.dict_off, be);
        last = best;
      }
    }
    at = v.off + v.k * tb;
  }
  w.put('\t');
  // INFO: the pairs are checked left to right, then written ascending by key
  const uint32_t info_at = at;
  for (uint32_t i = 0; i < n_info; ++i) {
    if ((rc = vcf_typed(b, send, &at, 1, &v))) VCF_FAIL(rc);
    if (!(v.k == 1 && vcf_is_int(v.t))) VCF_FAIL(HBAM_ERUNTIME);
    const int32_t key = vcf_int(b, v.off, v.t);
    if (key < 0 || key >= M.n_dict) VCF_FAIL(HBAM_ERUNTIME);
    if (!(M.flags[key] & HBAM_VCF_HAS_INFO)) VCF_FAIL(HBAM_ETRIBBLE);
    at = v.off + vcf_tb(v.t);
    if ((rc = vcf_typed(b, send, &at, 1, &v))) VCF_FAIL(rc);
    at = v.off + v.k * vcf_tb(v.t);
  }
  if (n_info > HBAM_VCF_MAX_INFO) deferred = 1;
  else if (n_info == 0) w.put('.');
  else {
    int64_t last = -1;
    for (;;) {
      int64_t best = INT64_MAX;
      uint32_t bkey = 0, twice = 0;
      VcfTV bv{0, 0, 0};
      at = info_at;
      for (uint32_t i = 0; i < n_info; ++i) {
        vcf_typed(b, send, &at, 1, &v);
        const uint32_t key = (uint32_t)vcf_int(b, v.off, v.t);
        at = v.off + vcf_tb(v.t);
        vcf_typed(b, send, &at, 1, &v);
        at = v.off + v.k * vcf_tb(v.t);
        const int64_t rk = M.rank[key];
        if (rk == best) twice = 1;
        if (rk > last && rk < best) {
          best = rk;
          bkey = key;
          bv = v;
          twice = 0;
        }
      }
      if (best == INT64_MAX) break;
      if (twice) deferred = 1;  // a key stored twice: the host applies last-wins
      if (last >= 0) w.put(';');
      vcf_put_name(w, M.dict, M.dict_off, bkey);
      if (!(M.flags[bkey] & HBAM_VCF_INFO_FLAG)) {
        if (vcf_value_null(b, bv.t, bv.k, bv.off)) {
          w.put('=');
          w.put('.');
        } else if (!(bv.t == 7 && vcf_str_len(b, bv.off, bv.k) == 1u && b[bv.off] == ',')) {  // an empty text: KEY alone
          w.put('=');
          vcf_put_value(w, b, bv.t, bv.k, bv.off, &deferred);
        }
      }
      last = best;
    }
  }
  // the genotype block
  r->deferred = deferred;
  r->status = HBAM_OK;
  vcf_geno_headers(b, M, r);
  if (r->status != HBAM_OK) return;
  if (r->n_sample >= wave_cut) {
    w.flush();
    r->by_wave = 1;
    r->len = (uint32_t)w.len;
    return;
  }
  if (r->n_sample) {
    VcfScan a{0, 0, 0, 0, 0};
    VcfKeys K;
    vcf_geno_scan(b, M, *r, 0, 1, &a);
    vcf_geno_keys(b, M, r, a, &K);
    if (r->status != HBAM_OK) return;
    if (!r->deferred) {
      vcf_put_format(w, b, M, *r, K);
      for (uint32_t s = 0; s < r->n_sample; ++s) vcf_put_sample(w, b, M, *r, K, s);
    }
  }
  w.put('\n');
  w.flush();
  if (w.len > 0x7fffffffull) VCF_FAIL(HBAM_EUNSUPPORTED);
  r->len = (uint32_t)w.len;
#undef VCF_FAIL
}

}  // namespace hbam
