// hbam_sam.hip — SAM text on the device: SAMRecordReader (SAMRecordReader.java) over one FileSplit.
// The lines of the split become BAM records (BAMRecordCodec.encode, what SAMRecordWritable.write
// sends through the shuffle) packed into the context's ubuf, and the BAM path's own k_decode_fixed,
// pool scans and k_decode_pools run over them: the result is the hbam_columns of hbam_decode_split.
// Included at the end of hbam_capi.hip, after hbam_vcf.hip (it uses that file's structural pass,
// line-start scatter and contig table).  gfx950, wave64.
//
//   k_vcf_scan, k_vcf_starts   newline / tab bitmaps, the start of every line (hbam_vcf.hip)
//   k_sam_sizes        a lane per line: the line parsed by sam_line (sam_line.h) for its record
//                      size and status; the tabs come from the tab bitmap, the tags decide the aux
//                      size.  SEQ and QUAL are not read (their lengths are tab positions); the other
//                      bytes come through a 16-byte register cache (SamBytes), since a lane per line
//                      pays a cache line per lane for every load instruction whatever its width.
//   (scan_exclusive)   sizes -> rec_off
//   k_sam_encode       a lane per line: the fixed fields, name, CIGAR and aux written at rec_off, and
//                      the line's SEQ / QUAL descriptor for the bulk pass
//   k_sam_bulk         SEQ and QUAL, about two thirds of the text, the way k_decode_pools moves
//                      pools: a wave takes a tile of 64 lines, cuts their packed SEQ and their QUAL
//                      into 16-byte output units, numbers the units with a wave scan and gives them
//                      to consecutive lanes, so a wave store covers 1 KiB of consecutive record bytes
//                      and a 6 KB long-read line is the whole wave's work.  A SEQ unit reads 32
//                      characters (two unaligned 16-byte loads), a QUAL unit 16.  A byte outside
//                      the SEQ table or a QUAL byte below '!' stops the split at that line.
//   k_sam_keys         the key of the records that are not placed (BAMRecordReader.getKey :88-95):
//                      k_decode_fixed hashes the raw variable block, which a SAM record does not have
//
// Loads past a field stay inside the 64 readable bytes behind the window (include/hbam.h).

#include "sam_line.h"

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
  __shared__ uint32_t s_excl[SAM_WG / 64][64];
  __shared__ uint4 s_desc[SAM_WG / 64][64];
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t* const ex = s_excl[threadIdx.x >> 6];
  uint4* const sd = s_desc[threadIdx.x >> 6];
  const uint32_t ntiles = (n + 63u) / 64u;
  const uint32_t wstride = gridDim.x * (SAM_WG / 64);
  for (uint32_t t = blockIdx.x * (SAM_WG / 64) + (threadIdx.x >> 6); t < ntiles; t += wstride) {
    const uint32_t line = t * 64u + lane;
    const uint4 d = line < n ? desc[line] : make_uint4(0, 0, 0, 0);
    const uint32_t lseq = d.y & 0x7fffffffu;
    const uint32_t units = ((lseq + 1u) / 2u + 15u) / 16u + (lseq + 15u) / 16u;
    const uint32_t incl = wave_scan_dpp(units), T = wave_last(incl);
    if (T == 0u) continue;  // wave-uniform
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");  // the previous tile's reads of ex / sd precede these writes
    ex[lane] = incl - units;
    sd[lane] = d;
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");  // (one wave: its LDS operations run in issue order)
    for (uint32_t q0 = 0; q0 < T; q0 += 64u) {
      const uint32_t q = q0 + lane;
      if (q >= T) continue;
      // the last line whose first unit is <= q (ex[0] = 0; lines without units tie with the next one)
      uint32_t r = 0, hi = 63;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const uint32_t mid = (r + hi + 1u) >> 1;
        if (ex[mid] <= q) r = mid;
        else hi = mid - 1u;
      }
      const uint4 D = sd[r];
      const uint32_t k = q - ex[r];
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
    }
  }
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
  uint32_t used = 0;
  for (uint32_t i = 0; i < table_size; ++i) {
    if (table[i].ordinal < 0) continue;
    ++used;
    if ((uint64_t)table[i].name_off + table[i].name_len > names_len)
      return set_err(c, HBAM_EINVAL, "dictionary table entry %u points outside the names", i);
  }
  if ((uint64_t)used * 2 > table_size)  // a probe ends at an empty slot
    return set_err(c, HBAM_EINVAL, "the dictionary table must be at least twice the number of sequences");
  // The split returns the lines whose first byte b has max(start, data_start) <= b < start + length
  // (SAMRecordReader.initialize and its WorkaroundingStream): a split at 0 begins at data_start, any
  // other opens at start - 1 and discards through the first '\n'
  const uint64_t q0_abs = start ? start - 1 : data_start;
  if (q0_abs < text_base) return set_err(c, HBAM_EINVAL, "the window starts after the reader's first byte");
  const uint64_t q0 = std::min(q0_abs - text_base, text_len);
  const uint64_t hi_abs = std::min(start + length, file_len);
  const uint32_t hi = (uint32_t)std::min<uint64_t>(hi_abs > text_base ? hi_abs - text_base : 0, 0xffffffffull);
  const uint32_t explicit_first = (start == 0 && q0_abs - text_base < text_len) ? 1u : 0u;
  const uint64_t window_end = text_base + text_len;
  c->timing = hbam_timing{};
  const uint8_t* d;
  int rc = stage_comp(c, text, on_device, text_len, &d);
  if (rc) return rc;
  const uint32_t shift = (uint32_t)((uintptr_t)d & 15u);
  const uint32_t end = (uint32_t)text_len + shift;
  const uint32_t ntiles = (end + VCF_TILE - 1) / VCF_TILE;
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  uint64_t m_all = 0;
  uint16_t *nlmap = nullptr, *tabmap = nullptr;
  uint64_t* tfirst = nullptr;
  if (ntiles) {
    uint32_t* cnt;
    const uint64_t quads = (uint64_t)ntiles * (VCF_TILE / 16);
    if ((rc = ensure(c, B_VCF_NL, quads, &nlmap)) || (rc = ensure(c, B_VCF_TAB, quads + 4, &tabmap)) ||
        (rc = ensure(c, B_VCF_CNT, (uint64_t)ntiles + 1, &cnt)) ||
        (rc = ensure(c, B_VCF_OFF, (uint64_t)ntiles + 1, &tfirst)))
      return rc;
    k_vcf_scan<<<grid_for(ntiles, VCF_WG / 64), VCF_WG, 0, c->stream>>>(d - shift, end, (uint32_t)q0 + shift, ntiles,
                                                                         nlmap, tabmap, cnt);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    if ((rc = scan_exclusive<uint32_t>(c, cnt, ntiles, tfirst, &m_all))) return rc;
  } else {
    HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  }
  const uint64_t total = m_all + explicit_first;
  uint32_t *starts, *rsize;
  int32_t* lstatus;
  uint4* desc;
  uint64_t* small;
  if ((rc = ensure(c, B_VCF_STARTS, total + 2, &starts)) || (rc = ensure(c, B_SAM_RSIZE, total + 1, &rsize)) ||
      (rc = ensure(c, B_SAM_STATUS, total + 1, &lstatus)) || (rc = ensure(c, B_SAM_DESC, total + 1, &desc)) ||
      (rc = ensure(c, B_VCF_SMALL, 4, &small)))
    return rc;
  unsigned long long* first_stop = (unsigned long long*)small;
  uint32_t* n_cand_d = (uint32_t*)(small + 1);
  HIPCHK(c, hipMemsetAsync(small, 0xff, 8, c->stream));
  HIPCHK(c, hipMemsetAsync(small + 1, 0, 8, c->stream));
  if (ntiles)
    k_vcf_starts<<<grid_for(ntiles, VCF_WG / 64), VCF_WG, 0, c->stream>>>(
        nlmap, ntiles, tfirst, shift, explicit_first, (uint32_t)q0, (uint32_t)total, (uint32_t)text_len, starts);
  HIPCHK(c, hipGetLastError());
  hbam_vcf_contig* dtab = nullptr;
  uint8_t* dnames = nullptr;
  if (total) {
    if ((rc = ensure(c, B_VCF_TABLE, (uint64_t)table_size, &dtab)) ||
        (rc = ensure(c, B_VCF_NAMES, names_len + 1, &dnames)))
      return rc;
    HIPCHK(c, hipMemcpyAsync(dtab, table, (size_t)table_size * sizeof *table, hipMemcpyHostToDevice, c->stream));
    if (names_len) HIPCHK(c, hipMemcpyAsync(dnames, names, names_len, hipMemcpyHostToDevice, c->stream));
    k_sam_sizes<<<grid_for(total, SAM_WG), SAM_WG, 0, c->stream>>>(d, (const uint64_t*)tabmap, shift, starts,
                                                                  (uint32_t)total, hi, dtab, table_size - 1, dnames,
                                                                  rsize, lstatus, first_stop, n_cand_d);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipMemcpyAsync(c->pinned_small + 8, small, 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint64_t fs = c->pinned_small[8];
  const uint64_t n_cand = c->pinned_small[9] & 0xffffffffull;
  uint64_t n = n_cand;
  int32_t status = HBAM_OK;
  // the window ends inside the last line it would return (or before the split's bound with no line
  // at all), and the file goes on: the caller passes a longer window
  const bool cut = window_end < file_len &&
                   (total == 0 ? window_end < hi_abs : (n_cand == total && fs >= total - 1));
  if (cut) {
    n = total ? total - 1 : 0;
    status = HBAM_EMORE;
  } else if (fs < n_cand) {
    n = fs;
    HIPCHK(c, copy_sync(c, &status, lstatus + fs, 4, hipMemcpyDeviceToHost));
  }
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
  uint64_t tot_name = 0, tot_cig = 0, tot_seq = 0, tot_aux = 0;
  {
    const uint32_t tiles = (uint32_t)std::max<uint64_t>(1, (n + SCAN4_TILE - 1) / SCAN4_TILE);
    uint64_t* partial;
    if ((rc = ensure(c, B_PARTIAL, 4ull * tiles + 1, &partial))) return rc;
    const Scan4In in{{dc.name_len, dc.cigar_n, dc.seq_len, dc.aux_len}};
    const Scan4Out so{{dc.name_off, dc.cigar_off, dc.seq_off, dc.aux_off}};
    k_scan4_reduce<<<tiles, 256, 0, c->stream>>>(in, n, partial, tiles);
    k_scan4_partials<<<4, 256, 0, c->stream>>>(partial, tiles, so, n);
    k_scan4_apply<<<tiles, 256, 0, c->stream>>>(in, n, partial, tiles, so);
    HIPCHK(c, hipGetLastError());
    const uint64_t* offs[4] = {dc.name_off, dc.cigar_off, dc.seq_off, dc.aux_off};
    for (int q = 0; q < 4; ++q)
      HIPCHK(c, hipMemcpyAsync(c->pinned_small + 96 + q, offs[q] + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->pinned_small + 8, small, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    tot_name = c->pinned_small[96];
    tot_cig = c->pinned_small[97];
    tot_seq = c->pinned_small[98];
    tot_aux = c->pinned_small[99];
  }
  if (c->pinned_small[8] < n)  // k_decode_fixed stops at no record the encoder wrote
    return set_err(c, HBAM_EDEVICE, "hbam_sam_decode_split: record %llu does not decode",
                   (unsigned long long)c->pinned_small[8]);
  if ((rc = ensure(c, B_C_NAMES, tot_name + 1, &dc.names))) return rc;
  if ((rc = ensure(c, B_C_CIGARS, tot_cig + 1, &dc.cigars))) return rc;
  if ((rc = ensure(c, B_C_SEQ, tot_seq + 1, &dc.seq))) return rc;
  if ((rc = ensure(c, B_C_QUAL, tot_seq + 1, &dc.qual))) return rc;
  if ((rc = ensure(c, B_C_AUX, tot_aux + 1, &dc.aux))) return rc;
  HIPCHK(c, hipEventRecord(c->ev[7], c->stream));
  if (n)
    k_decode_pools<<<(uint32_t)std::min<uint64_t>(grid_for(n, 256), POOLS_MAX_WG), 256, 0, c->stream>>>(ub, n, rec_off,
                                                                                                       dc);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev[8], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));

  out->n_records = n;
  out->status = status;
  out->err_record = status ? n : 0;
  out->voffset = voff;
  out->key = dc.key;
  out->rec_off = rec_off;
  out->ubuf = ub;
  out->ubuf_len = utotal;
  out->block_size = dc.block_size;
  out->ref_id = dc.ref_id;
  out->pos = dc.pos;
  out->l_read_name = dc.l_read_name;
  out->mapq = dc.mapq;
  out->bin = dc.bin;
  out->n_cigar = dc.n_cigar;
  out->flag = dc.flag;
  out->l_seq = dc.l_seq;
  out->next_ref_id = dc.next_ref_id;
  out->next_pos = dc.next_pos;
  out->tlen = dc.tlen;
  out->layout_ok = dc.layout_ok;
  out->name_off = dc.name_off;
  out->names = dc.names;
  out->cigar_off = dc.cigar_off;
  out->cigars = dc.cigars;
  out->seq_off = dc.seq_off;
  out->seq = dc.seq;
  out->qual = dc.qual;
  out->aux_off = dc.aux_off;
  out->aux = dc.aux;

  c->timing.scan_ms = ev_ms(c, 0, 1);
  c->timing.walk_ms = ev_ms(c, 1, 2);
  c->timing.inflate_ms = ev_ms(c, 2, 3);
  c->timing.huffman_ms = ev_ms(c, 2, 11);  // of the encode: the per-line pass ...
  c->timing.resolve_ms = ev_ms(c, 11, 3);  // ... and SEQ / QUAL
  c->timing.decode_ms = ev_ms(c, 5, 6);
  c->timing.pools_ms = ev_ms(c, 7, 8);
  c->timing.total_ms = ev_ms(c, 0, 8);
  c->timing.comp_bytes = text_len;
  c->timing.ubuf_bytes = utotal;
  c->timing.n_records = n;
  c->timing.pool_bytes = tot_name + 4 * tot_cig + 2 * tot_seq + tot_aux;
  return HBAM_OK;
}
