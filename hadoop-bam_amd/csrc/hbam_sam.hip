// hbam_sam.hip — SAM text on the device: SAMRecordReader (SAMRecordReader.java) over one FileSplit.
// The lines of the split become BAM records (BAMRecordCodec.encode, what SAMRecordWritable.write
// sends through the shuffle) packed into the context's ubuf, and the BAM path's own k_decode_fixed,
// pool scans and k_decode_pools run over them (finish_pools, columns_out): the result is the
// hbam_columns of hbam_decode_split.  Included at the end of hbam_capi.hip, after hbam_lines.hip (the
// line-structure front end and the name table's helpers) and hbam_vcf.hip (the CharSequence hash).
// gfx950, wave64.
//
//   k_line_scan<false, true>, k_vcf_starts   newline / tab bitmaps, the start of every line
//                      (text_lines, hbam_lines.hip)
//   k_sam_sizes        a lane per line: the line parsed by sam_line (sam_line.h) for its record
//                      size and status; the tabs come from the tab bitmap, the tags decide the aux
//                      size.  SEQ and QUAL are not read (their lengths are tab positions); the other
//                      bytes come through a 16-byte register cache (SamBytes), since a lane per line
//                      pays a cache line per lane for every load instruction whatever its width.
//   (scan_exclusive)   sizes -> rec_off
//   k_sam_encode       a lane per line: the fixed fields, name, CIGAR and aux written at rec_off, and
//                      the line's SEQ / QUAL descriptor for the bulk pass
//   k_sam_bulk         SEQ and QUAL, about two thirds of the text, the way k_decode_pools moves
//                      pools: the lines' packed SEQ and QUAL cut into 16-byte output units and given
//                      to consecutive lanes (unit_tiles.h).  A SEQ unit reads 32 characters (two
//                      unaligned 16-byte loads), a QUAL unit 16.  A byte outside the SEQ table or a
//                      QUAL byte below '!' stops the split at that line.
//   k_sam_keys         the key of the records that are not placed (BAMRecordReader.getKey :88-95):
//                      k_decode_fixed hashes the raw variable block, which a SAM record does not have
//
// Loads past a field stay inside the 64 readable bytes behind the window (include/hbam.h).

#include "sam_line.h"
#include "unit_tiles.h"

namespace hbam {

constexpr uint32_t SAM_WG = 256;

// line i = window bytes [s, s + len): its start, and its length without "\n" / "\r\n"
__device__ __forceinline__ uint32_t sam_line_bounds(const uint8_t* __restrict__ text,
                                                    const uint32_t* __restrict__ starts, uint32_t i, uint32_t total,
                                                    uint32_t* len) {
  const uint32_t s = starts[i], nxt = starts[i + 1];
  uint32_t n = nxt - 1u - s;
  if (i + 1 < total && n && text[s + n - 1] == '\r') --n;
  *len = n;
  return s;
}

__global__ __launch_bounds__(SAM_WG) void k_sam_sizes(const uint8_t* __restrict__ text,
                                                      const uint64_t* __restrict__ tabmap64, uint32_t shift,
                                                      const uint32_t* __restrict__ starts, uint32_t total, uint32_t hi,
                                                      const hbam_vcf_contig* __restrict__ table, uint32_t tmask,
                                                      const uint8_t* __restrict__ names, uint32_t* __restrict__ rsize,
                                                      int32_t* __restrict__ status, unsigned long long* first_stop,
                                                      uint32_t* n_cand) {
  const uint32_t i = blockIdx.x * SAM_WG + threadIdx.x;
  if (i >= total) return;
  if (starts[i] >= hi) return;
  if (i + 1 >= total || starts[i + 1] >= hi) *n_cand = i + 1;  // one lane: the starts ascend
  uint32_t len;
  const uint32_t s = sam_line_bounds(text, starts, i, total, &len);
  const SamTabs tb{tabmap64, s + shift, s + shift + len};
  SamLine r;
  sam_line(text + s, tb, table, tmask, names, nullptr, &r);
  rsize[i] = r.size;
  status[i] = r.status;
  if (r.status != HBAM_OK) atomicMin(first_stop, (unsigned long long)i);
}

// desc[i] = (window offset of SEQ, l_seq | QUAL-is-"*" << 31, ubuf offset of the packed SEQ lo, hi)
__global__ __launch_bounds__(SAM_WG) void k_sam_encode(const uint8_t* __restrict__ text,
                                                       const uint64_t* __restrict__ tabmap64, uint32_t shift,
                                                       const uint32_t* __restrict__ starts, uint32_t total, uint32_t n,
                                                       uint64_t text_base, const hbam_vcf_contig* __restrict__ table,
                                                       uint32_t tmask, const uint8_t* __restrict__ names,
                                                       const uint64_t* __restrict__ rec_off, uint8_t* __restrict__ ub,
                                                       uint64_t* __restrict__ voff, uint4* __restrict__ desc) {
  const uint32_t i = blockIdx.x * SAM_WG + threadIdx.x;
  if (i >= n) return;
  uint32_t len;
  const uint32_t s = sam_line_bounds(text, starts, i, total, &len);
  const SamTabs tb{tabmap64, s + shift, s + shift + len};
  const uint64_t ro = rec_off[i];
  SamLine r;
  sam_line(text + s, tb, table, tmask, names, ub + ro, &r);
  const uint64_t d = ro + r.seq_out;
  desc[i] = make_uint4(s + r.seq_rel, r.l_seq | r.qual_star << 31, (uint32_t)d, (uint32_t)(d >> 32));
  voff[i] = text_base + s;
}

__global__ __launch_bounds__(SAM_WG) void k_sam_bulk(const uint8_t* __restrict__ text,
                                                     const uint4* __restrict__ desc, uint32_t n,
                                                     uint8_t* __restrict__ ub, int32_t* __restrict__ status,
                                                     unsigned long long* first_stop) {
  __shared__ uint4 s_desc[SAM_WG / 64][64];
  uint4* const sd = s_desc[threadIdx.x >> 6];
  uint4 d;
  unit_tiles<SAM_WG>(
      n,
      [&](uint32_t line) {
        d = line < n ? desc[line] : make_uint4(0, 0, 0, 0);
        const uint32_t lseq = d.y & 0x7fffffffu;
        return ((lseq + 1u) / 2u + 15u) / 16u + (lseq + 15u) / 16u;
      },
      [&](uint32_t lane) { sd[lane] = d; },
      [&](uint32_t t, uint32_t r, uint32_t k) {
        const uint4 D = sd[r];
        const uint32_t ls = D.y & 0x7fffffffu, packed = (ls + 1u) / 2u, us = (packed + 15u) / 16u;
        const uint8_t* const src = text + D.x;
        uint8_t* dst = ub + ((uint64_t)D.z | (uint64_t)D.w << 32);
        uint32_t o[4], nbytes;
        bool ok = true;
        if (k < us) {
          const uint32_t nchar = min(32u, ls - 32u * k);
          const u32x4_a1 a = *(const HBAM_G u32x4_a1*)(src + 32u * k);
          const u32x4_a1 b = *(const HBAM_G u32x4_a1*)(src + 32u * k + 16u);
          const uint32_t w[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
          ok = sam_seq_unit(w, nchar, o);
          nbytes = (nchar + 1u) / 2u;
          dst += 16u * k;
        } else {
          const uint32_t kq = k - us;
          nbytes = min(16u, ls - 16u * kq);
          dst += packed + 16u * kq;
          if (D.y >> 31) {
            o[0] = o[1] = o[2] = o[3] = 0xffffffffu;
          } else {
            const u32x4_a1 a = *(const HBAM_G u32x4_a1*)(src + ls + 1u + 16u * kq);
            const uint32_t w[4] = {a[0], a[1], a[2], a[3]};
            ok = sam_qual_unit(w, nbytes, o);
          }
        }
        const u32x4_a1 v = u32x4_a1{o[0], o[1], o[2], o[3]};
        HBAM_G uint8_t* const gd = (HBAM_G uint8_t*)dst;
        if (nbytes >= 16u) *(HBAM_G u32x4_a1*)gd = v;
        else st_part_g(gd, nbytes, v);
        if (!ok) {
          const uint32_t bad = t * 64u + r;
          status[bad] = HBAM_EFORMAT;
          atomicMin(first_stop, (unsigned long long)bad);
        }
      });
}

// key[i] of the records k_decode_fixed gave the raw-bytes hash: the chained hash of the read name
// (chars), the normalised read bases, the quality values and the CIGAR string (chars), each seeded
// with the previous one truncated to int; Integer.MAX_VALUE << 32 | hash.  The name and the CIGAR
// are hashed as the line writes them (a CIGAR length with leading zeros is not re-rendered).
__global__ __launch_bounds__(SAM_WG) void k_sam_keys(const uint8_t* __restrict__ text,
                                                     const uint64_t* __restrict__ tabmap64, uint32_t shift,
                                                     const uint32_t* __restrict__ starts, uint32_t total, uint32_t n,
                                                     const uint8_t* __restrict__ ub,
                                                     const uint64_t* __restrict__ rec_off, DevColumns c) {
  const uint16_t* const flag = c.flag;
  const int32_t *const ref = c.ref_id, *const pos = c.pos;
  int64_t* const key = c.key;
  const uint32_t i = blockIdx.x * SAM_WG + threadIdx.x;
  if (i >= n) return;
  const int32_t start = (int32_t)((uint32_t)pos[i] + 1u);
  if (!((flag[i] & 4) || ref[i] < 0 || start < 0)) return;
  uint32_t len;
  const uint32_t s = sam_line_bounds(text, starts, i, total, &len);
  const SamTabs tb{tabmap64, s + shift, s + shift + len};
  const uint8_t* const l = text + s;
  uint32_t b[11], e[11], from = 0;
  for (uint32_t k = 0; k < 11; ++k) {
    b[k] = from;
    e[k] = sam_next_tab(tb, from);
    from = e[k] + 1;
  }
  const bool seq_star = e[9] - b[9] == 1 && l[b[9]] == '*';
  const bool qual_star = e[10] - b[10] == 1 && l[b[10]] == '*';
  const uint8_t* const sq = l + b[9];
  int32_t h = (int32_t)murmur3_java_chars(l, e[0], 0);
  h = (int32_t)sam_murmur_bytes(
      [sq](uint32_t j) -> uint8_t {
        const uint8_t c = sq[j];
        return c == '.' ? (uint8_t)'N' : (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c;
      },
      seq_star ? 0u : e[9] - b[9], h);
  // the quality values stand in the record as the bulk pass wrote them: the BAM path's byte hash
  // over them, seeded (none for "*")
  const uint8_t* const rq =
      ub + rec_off[i] + 36u + c.l_read_name[i] + 4u * c.n_cigar[i] + ((uint32_t)c.l_seq[i] + 1u) / 2u;
  h = (int32_t)murmur3_java(rq, qual_star ? 0 : (int32_t)(e[10] - b[10]), h);
  h = (int32_t)murmur3_java_chars(l + b[5], e[5] - b[5], h);
  key[i] = (int64_t)((uint64_t)0x7fffffffULL << 32 | (uint64_t)(int64_t)h);
}

}  // namespace hbam

extern "C" int hbam_sam_decode_split(hbam_ctx* c, const uint8_t* text, int on_device, uint64_t text_base,
                                     uint64_t text_len, uint64_t file_len, uint64_t start, uint64_t length,
                                     uint64_t data_start, const hbam_vcf_contig* table, uint32_t table_size,
                                     const uint8_t* names, uint64_t names_len, int32_t n_ref, hbam_columns* out) {
  if (!c || !text || !out || !table || (names_len && !names)) return HBAM_EINVAL;
  memset(out, 0, sizeof *out);
  HIPCHK(c, hipSetDevice(c->device));
  if (table_size == 0 || (table_size & (table_size - 1)))
    return set_err(c, HBAM_EINVAL, "the dictionary table's size must be a power of two");
  if (text_len > VCF_MAX_WINDOW) return set_err(c, HBAM_EINVAL, "a SAM window is at most 2 GiB");
  if (text_base + text_len > file_len) return set_err(c, HBAM_EINVAL, "window past the end of the file");
  if (start != 0 && start < data_start)
    return set_err(c, HBAM_EUNSUPPORTED, "a SAM split that begins inside the header (start %llu < data_start %llu)",
                   (unsigned long long)start, (unsigned long long)data_start);
  int rc = contig_table_check(c, table, table_size, names_len, DICTIONARY_TABLE);
  if (rc) return rc;
  // The split returns the lines whose first byte b has max(start, data_start) <= b < start + length
  // (SAMRecordReader.initialize and its WorkaroundingStream): a split at 0 begins at data_start, any
  // other opens at start - 1 and discards through the first '\n' (reader_bounds)
  const uint64_t hi_abs = std::min(start + length, file_len);
  ReaderBounds b;
  if ((rc = reader_bounds(c, start, data_start, text_base, text_len, hi_abs, &b))) return rc;
  c->timing = hbam_timing{};
  TextLines L;
  if ((rc = text_lines(c, text, on_device, text_len, b.q0, b.explicit_first, false, false, true, &L))) return rc;
  const uint64_t total = L.total;
  const uint8_t* const d = L.d;
  const uint32_t shift = L.shift;
  uint32_t* const starts = L.starts;
  const uint16_t* const tabmap = L.tabmap;
  uint32_t* rsize;
  int32_t* lstatus;
  uint4* desc;
  uint64_t* small;
  if ((rc = ensure(c, B_SAM_RSIZE, total + 1, &rsize)) || (rc = ensure(c, B_SAM_STATUS, total + 1, &lstatus)) ||
      (rc = ensure(c, B_SAM_DESC, total + 1, &desc)) || (rc = ensure(c, B_VCF_SMALL, 4, &small)))
    return rc;
  unsigned long long* first_stop = (unsigned long long*)small;
  uint32_t* n_cand_d = (uint32_t*)(small + 1);
  HIPCHK(c, hipMemsetAsync(small, 0xff, 8, c->stream));
  HIPCHK(c, hipMemsetAsync(small + 1, 0, 8, c->stream));
  hbam_vcf_contig* dtab = nullptr;
  uint8_t* dnames = nullptr;
  if (total) {
    if ((rc = contig_table_upload(c, table, table_size, names, names_len, &dtab, &dnames))) return rc;
    k_sam_sizes<<<grid_for(total, SAM_WG), SAM_WG, 0, c->stream>>>(d, (const uint64_t*)tabmap, shift, starts,
                                                                  (uint32_t)total, b.hi, dtab, table_size - 1, dnames,
                                                                  rsize, lstatus, first_stop, n_cand_d);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipMemcpyAsync(c->pinned_small + 8, small, 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  uint64_t n;
  int32_t status;
  if ((rc = window_cut(c, c->pinned_small[8], c->pinned_small[9] & 0xffffffffull, total, text_base + text_len, file_len,
                       hi_abs, lstatus, &n, &status)))
    return rc;
  // record offsets, the records, SEQ and QUAL
  uint64_t *rec_off, *voff;
  uint64_t utotal = 0;
  if ((rc = ensure(c, B_RECOFF, n + 1, &rec_off)) || (rc = ensure(c, B_VOFF, n + 1, &voff))) return rc;
  if ((rc = scan_exclusive<uint32_t>(c, rsize, n, rec_off, &utotal))) return rc;
  uint8_t* ub;
  if ((rc = ensure(c, B_UBUF, utotal + UBUF_SLACK, &ub))) return rc;
  HIPCHK(c, hipMemsetAsync(ub + utotal, 0, UBUF_SLACK, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  HIPCHK(c, hipMemsetAsync(small, 0xff, 8, c->stream));
  if (n) {
    k_sam_encode<<<grid_for(n, SAM_WG), SAM_WG, 0, c->stream>>>(d, (const uint64_t*)tabmap, shift, starts,
                                                               (uint32_t)total, (uint32_t)n, text_base, dtab,
                                                               table_size - 1, dnames, rec_off, ub, voff, desc);
    HIPCHK(c, hipEventRecord(c->ev[11], c->stream));
    k_sam_bulk<<<(uint32_t)std::min<uint64_t>(grid_for(n, SAM_WG), POOLS_MAX_WG), SAM_WG, 0, c->stream>>>(
        d, desc, (uint32_t)n, ub, lstatus, first_stop);
    HIPCHK(c, hipGetLastError());
  } else {
    HIPCHK(c, hipEventRecord(c->ev[11], c->stream));
  }
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  HIPCHK(c, hipMemcpyAsync(c->pinned_small + 8, small, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint64_t fs2 = c->pinned_small[8];
  if (fs2 < n) {  // a SEQ or QUAL byte: the records before that line stand
    n = fs2;
    HIPCHK(c, copy_sync(c, &status, lstatus + fs2, 4, hipMemcpyDeviceToHost));
    HIPCHK(c, copy_sync(c, &utotal, rec_off + n, 8, hipMemcpyDeviceToHost));
  }
  // ---- the BAM path over the new ubuf: no empty-block events, a hard end at the end of the records
  DevColumns dc{};
  if ((rc = fill_columns(c, n, &dc))) return rc;
  HIPCHK(c, hipMemsetAsync(small, 0xff, 8, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
  if (n) {
    k_decode_fixed<<<grid_for(n, 256), 256, 0, c->stream>>>(ub, n, rec_off, voff, (uint64_t)INT64_MAX, utotal,
                                                            HBAM_EEOF, nullptr, 0, n_ref, 0, dc, first_stop);
    k_sam_keys<<<grid_for(n, SAM_WG), SAM_WG, 0, c->stream>>>(d, (const uint64_t*)tabmap, shift, starts,
                                                             (uint32_t)total, (uint32_t)n, ub, rec_off, dc);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
  // (small: k_decode_fixed's first stop comes back with the pool totals)
  if ((rc = finish_pools(c, ub, n, rec_off, dc, small))) return rc;
  columns_out(out, dc, voff, rec_off, ub, utotal, n, status, status ? n : 0);

  c->timing.scan_ms = ev_ms(c, 0, 1);
  c->timing.walk_ms = ev_ms(c, 1, 2);
  c->timing.inflate_ms = ev_ms(c, 2, 3);
  c->timing.huffman_ms = ev_ms(c, 2, 11);  // of the encode: the per-line pass ...
  c->timing.resolve_ms = ev_ms(c, 11, 3);  // ... and SEQ / QUAL
  c->timing.decode_ms = ev_ms(c, 5, 6);
  c->timing.total_ms = ev_ms(c, 0, 8);
  c->timing.comp_bytes = text_len;
  c->timing.ubuf_bytes = utotal;
  c->timing.n_records = n;
  return HBAM_OK;
}
