// hbam_fragtext.hip — FASTQ and QSEQ text out of the device: FastqRecordWriter.write and
// QseqRecordWriter.write over hbam_frag_columns (FastqOutputFormat, QseqOutputFormat), the inverse
// of hbam_fastq.hip.  Included at the end of hbam_capi.hip, after hbam_fastq.hip, over the host
// sequence of hbam_textout.hip (no deferred records).  gfx950, wave64.
//
//   k_fragtext_sizes   a lane per output record: the record's fields gathered from the columns
//                      (frag_text_load) and its text counted by frag_text (frag_text.h) in its
//                      counting mode: offsets, the present mask and the digit counts, no pool or
//                      window byte.  It leaves the bulk pass's descriptor, and stops the output at
//                      a record whose offsets or string pairs cannot be followed (HBAM_EINVAL).
//   (textout_layout)   lengths -> line_off
//   k_fragtext_head    a lane per record: the same frag_text with an output pointer writes the id
//                      line or the eight leading QSEQ fields and what follows the quality, four
//                      bytes per store (SamOut)
//   k_fragtext_bulk    sequence, separator, quality: nearly all of the text.  As k_samtext_bulk
//                      (unit_tiles.h), each record's region is cut into 16-byte units aligned in
//                      the OUTPUT.  frag_text_unit applies 'N' -> '.'
//                      and + 31 and checks the unit's bytes; a bad byte marks its record and the
//                      first such record (atomicMin) ends the output.
//
// Loads past a record's bytes in a pool stay inside the 16 readable bytes behind it.

#include "frag_text.h"

namespace hbam {

constexpr uint32_t FRAGTEXT_WG = 256;

// desc[2k] = (ls, lq, record-relative offset of the bulk region, 0), desc[2k + 1] = the record's
// offsets into the seq and the qual pool (lo, hi each)
__global__ __launch_bounds__(FRAGTEXT_WG) void k_fragtext_sizes(FragIn in, const uint32_t* __restrict__ perm,
                                                                uint32_t n, int32_t format, uint32_t flags,
                                                                uint32_t* __restrict__ len,
                                                                uint32_t* __restrict__ bad,
                                                                uint4* __restrict__ desc,
                                                                unsigned long long* first_stop) {
  const uint32_t k = blockIdx.x * FRAGTEXT_WG + threadIdx.x;
  if (k >= n) return;
  const uint64_t i = perm ? perm[k] : k;
  FragRec r;
  uint32_t bulk_rel = 0;
  uint64_t l = 0;
  const bool ok = frag_text_load(in, i, format == HBAM_FRAG_FASTQ && (flags & HBAM_FRAG_USE_KEY), &r);
  if (ok) l = frag_text(r, in, format, flags, nullptr, &bulk_rel);
  bad[k] = 0;
  if (!ok || l > 0x7fffffffull) {
    len[k] = 0;
    desc[2 * (uint64_t)k] = make_uint4(0, 0, 0, 0);
    desc[2 * (uint64_t)k + 1] = make_uint4(0, 0, 0, 0);
    atomicMin(first_stop, (unsigned long long)k);
    return;
  }
  len[k] = (uint32_t)l;
  desc[2 * (uint64_t)k] = make_uint4(r.ls, r.lq, bulk_rel, 0);
  desc[2 * (uint64_t)k + 1] = make_uint4((uint32_t)r.so, (uint32_t)(r.so >> 32), (uint32_t)r.qo, (uint32_t)(r.qo >> 32));
}

__global__ __launch_bounds__(FRAGTEXT_WG) void k_fragtext_head(FragIn in, const uint32_t* __restrict__ perm,
                                                               uint32_t n, int32_t format, uint32_t flags,
                                                               const uint64_t* __restrict__ line_off,
                                                               uint8_t* __restrict__ text) {
  const uint32_t k = blockIdx.x * FRAGTEXT_WG + threadIdx.x;
  if (k >= n) return;
  const uint64_t i = perm ? perm[k] : k;
  FragRec r;
  uint32_t bulk_rel;
  // (every record below the first stop loaded in the sizes pass)
  if (!frag_text_load(in, i, format == HBAM_FRAG_FASTQ && (flags & HBAM_FRAG_USE_KEY), &r)) return;
  frag_text(r, in, format, flags, text + line_off[k], &bulk_rel);
}

__global__ __launch_bounds__(FRAGTEXT_WG) void k_fragtext_bulk(const uint8_t* __restrict__ seq,
                                                               const uint8_t* __restrict__ qual,
                                                               const uint4* __restrict__ desc,
                                                               const uint64_t* __restrict__ line_off, uint32_t n,
                                                               uint32_t sep, uint32_t mode,
                                                               uint8_t* __restrict__ text, uint32_t* __restrict__ bad,
                                                               unsigned long long* first_stop) {
  __shared__ uint4 s_len[FRAGTEXT_WG / 64][64];   // ls, lq, R lo, R hi
  __shared__ uint4 s_src[FRAGTEXT_WG / 64][64];   // seq offset lo, hi, qual offset lo, hi
  uint4* const sl = s_len[threadIdx.x >> 6];
  uint4* const ss = s_src[threadIdx.x >> 6];
  uint4 d0, d1;
  uint64_t R;
  unit_tiles<FRAGTEXT_WG>(
      n,
      [&](uint32_t line) {
        d0 = d1 = make_uint4(0, 0, 0, 0);
        R = 0;
        uint32_t blen = 0;
        if (line < n) {
          d0 = desc[2 * (uint64_t)line];
          d1 = desc[2 * (uint64_t)line + 1];
          R = line_off[line] + d0.z;
          blen = d0.x + sep + d0.y;
        }
        return sam_text_units(R, blen);
      },
      [&](uint32_t lane) {
        sl[lane] = make_uint4(d0.x, d0.y, (uint32_t)R, (uint32_t)(R >> 32));
        ss[lane] = d1;
      },
      [&](uint32_t t, uint32_t r, uint32_t k) {
        const uint4 L = sl[r], S = ss[r];
        const uint64_t Rr = (uint64_t)L.z | (uint64_t)L.w << 32;
        uint32_t p0, nb, o[4];
        sam_text_unit_span(Rr, L.x + sep + L.y, k, &p0, &nb);
        const uint32_t f = frag_text_unit(seq + ((uint64_t)S.x | (uint64_t)S.y << 32), L.x,
                                          qual + ((uint64_t)S.z | (uint64_t)S.w << 32), sep, mode, p0, nb, o);
        const u32x4_a1 v = u32x4_a1{o[0], o[1], o[2], o[3]};
        HBAM_G uint8_t* const gd = (HBAM_G uint8_t*)(text + Rr + p0);
        if (nb >= 16u) *(HBAM_G u32x4_a1*)gd = v;
        else st_part_g(gd, nb, v);
        if (f) {
          const uint32_t at = t * 64u + r;
          atomicOr(bad + at, f);
          atomicMin(first_stop, (unsigned long long)at);
        }
      });
}

}  // namespace hbam

namespace {

// a host copy of the columns into context buffers -> *in; EINVAL for arrays a kernel could not follow
int fragtext_upload(hbam_ctx* c, const hbam_frag_columns* h, uint64_t window_len, FragIn* in) {
  const uint64_t n = h->n, m = (n + 4) & ~3ull;  // n + 1 entries fit; every array stays 16-byte aligned
  *in = FragIn{};
  in->n = n;
  uint8_t *base, *pool[3];
  int rc;
  const uint64_t* hoff[3] = {h->key_off, h->seq_off, h->qual_off};
  const uint8_t* hpool[3] = {h->key, h->seq, h->qual};
  const uint64_t hlen[3] = {h->key_len, h->seq_len, h->qual_len};
  uint64_t used[3] = {0, 0, 0};
  if (n) {
    if (!h->present || !h->run || !h->lane || !h->tile || !h->xpos || !h->ypos || !h->read || !h->filter_passed ||
        !h->control || !h->instrument || !h->flowcell || !h->index)
      return set_err(c, HBAM_EINVAL, "hbam_frag_render: a column is missing");
    for (int j = 0; j < 3; ++j) {
      if (!hoff[j]) return set_err(c, HBAM_EINVAL, "hbam_frag_render: an offset array is missing");
      for (uint64_t i = 0; i < n; ++i)
        if (hoff[j][i + 1] < hoff[j][i]) return set_err(c, HBAM_EINVAL, "hbam_frag_render: key_off, seq_off and qual_off must ascend");
      used[j] = hoff[j][n];
      if (used[j] > hlen[j] || (used[j] && !hpool[j]))
        return set_err(c, HBAM_EINVAL, "hbam_frag_render: an offset array runs past its pool");
    }
    const uint32_t* pairs[3] = {h->instrument, h->flowcell, h->index};
    const uint32_t bits[3] = {hbam::FRAG_P_INSTRUMENT, hbam::FRAG_P_FLOWCELL, hbam::FRAG_P_INDEX};
    for (int j = 0; j < 3; ++j)
      for (uint64_t i = 0; i < n; ++i)
        if ((h->present[i] & bits[j]) && (uint64_t)pairs[j][2 * i] + pairs[j][2 * i + 1] > window_len)
          return set_err(c, HBAM_EINVAL, "hbam_frag_render: a string of record %llu runs past the window",
                         (unsigned long long)i);
  }
  // u64: off[3]; u32: present ints[8] strs[3] x 2 = 15
  if ((rc = ensure(c, B_FT_COLS, m * (3 * 8 + 15 * 4), &base)) || (rc = ensure(c, B_FT_KEY, used[0] + 16, &pool[0])) ||
      (rc = ensure(c, B_FT_SEQ, used[1] + 16, &pool[1])) || (rc = ensure(c, B_FT_QUAL, used[2] + 16, &pool[2])))
    return rc;
  uint64_t* q = (uint64_t*)base;
  uint32_t* w = (uint32_t*)(q + 3 * m);
  auto up = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess;
  };
  if (n) {
    for (int j = 0; j < 3; ++j) {
      HIPCHK(c, up(q + j * m, hoff[j], 8 * (n + 1)));
      HIPCHK(c, up(pool[j], hpool[j], used[j]));
    }
    const void* u32s[9] = {h->present, h->run, h->lane, h->tile, h->xpos, h->ypos, h->read, h->filter_passed, h->control};
    for (int j = 0; j < 9; ++j) HIPCHK(c, up(w + j * m, u32s[j], 4 * n));
    HIPCHK(c, up(w + 9 * m, h->instrument, 8 * n));
    HIPCHK(c, up(w + 11 * m, h->flowcell, 8 * n));
    HIPCHK(c, up(w + 13 * m, h->index, 8 * n));
  }
  in->key_off = q;
  in->seq_off = q + m;
  in->qual_off = q + 2 * m;
  in->present = w;
  in->run = (const int32_t*)(w + m);
  in->lane = (const int32_t*)(w + 2 * m);
  in->tile = (const int32_t*)(w + 3 * m);
  in->xpos = (const int32_t*)(w + 4 * m);
  in->ypos = (const int32_t*)(w + 5 * m);
  in->read = (const int32_t*)(w + 6 * m);
  in->filter_passed = (const int32_t*)(w + 7 * m);
  in->control = (const int32_t*)(w + 8 * m);
  in->instrument = w + 9 * m;
  in->flowcell = w + 11 * m;
  in->index = w + 13 * m;
  in->key = pool[0];
  in->seq = pool[1];
  in->qual = pool[2];
  in->key_len = used[0];
  in->seq_len = used[1];
  in->qual_len = used[2];
  return HBAM_OK;
}

}  // namespace

extern "C" int hbam_frag_render(hbam_ctx* c, const hbam_frag_columns* cols, const uint8_t* window,
                                int window_on_device, uint64_t window_len, const uint32_t* perm, uint64_t n,
                                int32_t format, int32_t encoding, uint32_t flags, hbam_frag_text* out) {
  using namespace hbam;
  if (!c || !out || !cols || (window_len && !window)) return HBAM_EINVAL;
  memset(out, 0, sizeof *out);
  HIPCHK(c, hipSetDevice(c->device));
  if (format != HBAM_FRAG_FASTQ && format != HBAM_FRAG_QSEQ)
    return set_err(c, HBAM_EINVAL, "hbam_frag_render: unknown format %d", format);
  if (encoding != HBAM_QUAL_SANGER && encoding != HBAM_QUAL_ILLUMINA)
    return set_err(c, HBAM_EINVAL, "hbam_frag_render: unknown base quality encoding %d", encoding);
  if (flags & ~(HBAM_FRAG_USE_KEY | HBAM_FRAG_INDEX_DOTS))
    return set_err(c, HBAM_EINVAL, "hbam_frag_render: unknown flags 0x%x", flags);
  if (n >= 0xffffffffull) return set_err(c, HBAM_EINVAL, "hbam_frag_render: at most 2^32 - 2 records a call");
  if (cols->host && perm) return set_err(c, HBAM_EINVAL, "hbam_frag_render: perm needs device columns");
  if (!perm && n > cols->n) return set_err(c, HBAM_EINVAL, "hbam_frag_render: n is above the columns' record count");
  if (window_len > 0xffffffffull) return set_err(c, HBAM_EINVAL, "hbam_frag_render: a window is below 4 GiB");
  c->timing = hbam_timing{};
  int rc;
  FragIn in{};
  if (cols->host) {
    if ((rc = fragtext_upload(c, cols, window_len, &in))) return rc;
  } else {
    in.n = cols->n;
    in.present = cols->present;
    in.run = cols->run;
    in.lane = cols->lane;
    in.tile = cols->tile;
    in.xpos = cols->xpos;
    in.ypos = cols->ypos;
    in.read = cols->read;
    in.filter_passed = cols->filter_passed;
    in.control = cols->control;
    in.instrument = cols->instrument;
    in.flowcell = cols->flowcell;
    in.index = cols->index;
    in.key_off = cols->key_off;
    in.seq_off = cols->seq_off;
    in.qual_off = cols->qual_off;
    in.key = cols->key;
    in.seq = cols->seq;
    in.qual = cols->qual;
    in.key_len = cols->key_len;
    in.seq_len = cols->seq_len;
    in.qual_len = cols->qual_len;
  }
  in.window = window;
  in.window_len = window_len;
  if (!window_on_device) {
    uint8_t* dwin;
    if ((rc = ensure(c, B_FT_WINDOW, window_len + 16, &dwin))) return rc;
    if (window_len) HIPCHK(c, hipMemcpyAsync(dwin, window, window_len, hipMemcpyHostToDevice, c->stream));
    in.window = dwin;
  }
  TextOut T{{B_FT_LEN, B_FT_BAD, B_FT_LINEOFF, B_FT_SMALL, B_FT_TEXT, false}};
  uint4* desc;
  if ((rc = ensure(c, B_FT_DESC, 2 * n + 2, &desc)) || (rc = textout_begin(c, n, &T))) return rc;
  uint32_t* const bad = (uint32_t*)T.lstatus;  // FRAG_BAD_* bits, not a status
  if (n)
    k_fragtext_sizes<<<grid_for(n, FRAGTEXT_WG), FRAGTEXT_WG, 0, c->stream>>>(in, perm, (uint32_t)n, format, flags,
                                                                            T.len, bad, desc, T.first_stop);
  HIPCHK(c, hipGetLastError());
  if ((rc = textout_stop(c, &T))) return rc;
  if (T.cut) T.status = HBAM_EINVAL;  // the sizes pass has one reason to stop
  if ((rc = textout_layout(c, &T))) return rc;
  if (T.m)
    k_fragtext_head<<<grid_for(T.m, FRAGTEXT_WG), FRAGTEXT_WG, 0, c->stream>>>(in, perm, (uint32_t)T.m, format, flags,
                                                                             T.line_off, T.text);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  if ((rc = textout_arm(c, T))) return rc;
  const uint32_t sep = format == HBAM_FRAG_FASTQ ? FRAG_SEP_FASTQ : FRAG_SEP_QSEQ;
  const uint32_t mode = (format == HBAM_FRAG_QSEQ ? FRAG_MODE_QSEQ : 0u) |
                        (encoding == HBAM_QUAL_ILLUMINA ? FRAG_MODE_ILLUMINA : 0u);
  if (T.m)
    k_fragtext_bulk<<<(uint32_t)std::min<uint64_t>(grid_for(T.m, FRAGTEXT_WG), POOLS_MAX_WG), FRAGTEXT_WG, 0,
                      c->stream>>>(in.seq, in.qual, desc, T.line_off, (uint32_t)T.m, sep, mode, T.text, bad,
                                   T.first_stop);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  if ((rc = textout_stop(c, &T))) return rc;
  if (T.cut) {  // a byte of the sequence or the quality: the records before that one stand
    uint32_t f = 0;
    uint64_t lo[2];
    uint4 d0;
    HIPCHK(c, copy_sync(c, &f, bad + T.m, 4, hipMemcpyDeviceToHost));
    HIPCHK(c, copy_sync(c, lo, T.line_off + T.m, 16, hipMemcpyDeviceToHost));
    HIPCHK(c, copy_sync(c, &d0, desc + 2 * T.m, 16, hipMemcpyDeviceToHost));
    T.text_len = lo[0];
    if (format == HBAM_FRAG_QSEQ) {
      T.status = (f & FRAG_BAD_BYTE) ? HBAM_EUNSUPPORTED : HBAM_ERUNTIME;
    } else {
      T.status = HBAM_ESEQFORMAT;
      // "@id\nseq\n+\n", the record without its quality (d0.y) and last '\n': the stream holds it when
      // convertQuality throws
      out->partial_len = lo[1] - lo[0] - d0.y - 1;
    }
  }
  textout_finish(c, T, out);  // (partial_len stays)
  return HBAM_OK;
}
