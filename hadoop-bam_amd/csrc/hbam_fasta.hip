// hbam_fasta.hip — FASTA on the device: FastaInputFormat.getSplits' '>' offsets and FastaRecordReader
// (FastaInputFormat.java:59-144, :146-361) over one FileSplit, filling ReferenceFragment columns.
// Included by hbam_capi.hip after hbam_fastq.hip (it uses that file's frag_text_lines / seq_line, the
// front end of hbam_lines.hip and hbam_capi.hip's buffers, scan and staging helpers).  gfx950, wave64.
//
//   k_fa_gt_scan      every lane loads one aligned quad (a wave covers 1 KiB per step, a tile is
//                     VCF_STEPS steps) and stores vcf_eq16(q, '>') as a 16-bit mask plus the tile's
//                     count: the text is read once.  Positions are `shifted` as in k_line_scan.
//   (scan_exclusive)  counts per tile -> first output index of each tile.
//   k_fa_gt_scatter   the absolute u64 offsets in ascending order, from the bitmap alone.
//
//   k_line_scan<true, false>, (scan_exclusive), k_vcf_starts    the lines from byte `start` under
//                     LineReader.readLine's rule (text_lines): line 0 is the header line, line k + 1
//                     is record k.
//   k_fa_header       a wave over the header line: its stored length min(content, 20000, end -
//                     start), the bytes it consumes, any byte >= 0x80 in what is stored.
//   k_fa_lines        a lane per line: rec_off, pos_after, position, line_len, the key length (the
//                     decimal width of position), the lines that start below the split's end and the
//                     first line that consumes 20000 bytes or more (a min-reduction).
//   k_fa_maxup        per-group maxima of the stored lengths, 64 lines per group, then groups of
//                     groups, up to FA_LEVELS levels: lv[0] = the lengths, lv[l + 1][i] = max
//                     lv[l][64 i .. 64 i + 63].
//   k_fa_cap          a wave per 64 lines: cap_k = max(L_-1, L_0 .. L_k), an in-wave inclusive
//                     max-scan seeded with the maxima of the earlier siblings on every level.
//   (scan_exclusive x2)  cap_k and the key lengths -> seq_off and key_off.
//   k_fa_seq          the sequence pool, organised by output bytes: a wave per run of 64 lines, its
//                     lanes over the aligned 16-byte quads of the run's output.  Byte c of record k
//                     is line k's own for c < L_k, else byte c of the most recent earlier line (the
//                     header is line -1) longer than c: Hadoop 1.2.1's Text keeps its backing array
//                     and the reader appends the whole array (the stale tail).  fa_cover finds that
//                     line through the maxima: it scans at most 63 earlier siblings per level going
//                     up and 64 children per level going down, never one step per earlier line.
//   k_fa_keys         the key pool: the indexSequence bytes with '\t' as ':', then the digits.
//
// A lane bounds every read by a line's stored length; a 16-byte load that begins inside the window
// ends inside its 64 bytes of slack.

namespace hbam {

constexpr uint32_t FA_MAX_LINE = 20000;  // FastaInputFormat.java:171
constexpr uint32_t FA_NONE = 0xffffffffu;
constexpr uint32_t FA_LEVELS = 6;  // 64^6 > 2^31 lines

__global__ __launch_bounds__(VCF_WG) void k_fa_gt_scan(const uint8_t* __restrict__ text16, uint32_t end, uint32_t shift,
                                                       uint32_t ntiles, uint16_t* __restrict__ gtmap,
                                                       uint32_t* __restrict__ count) {
  const uint32_t wave = blockIdx.x * (VCF_WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (wave >= ntiles) return;  // wave-uniform
  uint32_t cnt = 0;
#pragma unroll
  for (uint32_t s = 0; s < VCF_STEPS; ++s) {
    const uint64_t b = (uint64_t)wave * VCF_TILE + s * 1024u + lane * 16u;
    uint32_t m = 0;
    if (b < end) {
      const uint4 q = *reinterpret_cast<const uint4*>(text16 + b);
      const uint32_t hi = (uint32_t)min((uint64_t)16, (uint64_t)end - b);
      const uint32_t lo = shift > b ? (uint32_t)min((uint64_t)16, (uint64_t)shift - b) : 0u;
      m = vcf_eq16(q, '>') & ((1u << hi) - 1u) & ~((1u << lo) - 1u);
    }
    gtmap[b >> 4] = (uint16_t)m;
    cnt += (uint32_t)__popc(m);
  }
  const uint32_t tot = wave_last(wave_scan_dpp(cnt));
  if (lane == 0) count[wave] = tot;
}

__global__ __launch_bounds__(VCF_WG) void k_fa_gt_scatter(const uint16_t* __restrict__ gtmap, uint32_t ntiles,
                                                          const uint64_t* __restrict__ tile_first, uint32_t shift,
                                                          uint64_t text_base, uint64_t total,
                                                          uint64_t* __restrict__ out) {
  const uint32_t wave = blockIdx.x * (VCF_WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (wave >= ntiles) return;
  uint64_t base = tile_first[wave];
  for (uint32_t s = 0; s < VCF_STEPS; ++s) {
    const uint64_t b = (uint64_t)wave * VCF_TILE + s * 1024u + lane * 16u;
    uint32_t m = gtmap[b >> 4];
    const uint32_t c = (uint32_t)__popc(m);
    const uint32_t incl = wave_scan_dpp(c);
    uint64_t at = base + incl - c;
    while (m) {
      const uint32_t j = (uint32_t)__builtin_ctz(m);
      m &= m - 1u;
      if (at < total) out[at] = text_base + b + j - shift;  // (at < total always: a bound, not a rule)
      ++at;
    }
    base += wave_last(incl);
  }
}

__device__ __forceinline__ uint32_t fa_wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}

// positionAtFirstRecord's readLine over line 0 of `starts`: out[0] = the bytes stored, out[1] = the
// bytes consumed, out[2] = a stored byte >= 0x80.  One wave.
__global__ __launch_bounds__(64) void k_fa_header(const uint8_t* __restrict__ text, const uint32_t* __restrict__ starts,
                                                  uint32_t total, uint32_t wlen, uint32_t max_stored,
                                                  uint32_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x;
  const SeqLine l = seq_line(text, starts, 0, total, wlen);
  const uint32_t stored = min(l.content, max_stored);
  uint32_t acc = 0;
  for (uint32_t i = lane; i < stored; i += 64u) acc |= text[l.s + i];
  const bool high = __ballot((acc & 0x80u) != 0u) != 0ull;
  if (lane == 0) {
    out[0] = stored;
    out[1] = l.consumed;
    out[2] = high ? 1u : 0u;
  }
}

// Integer.toString's length
__device__ __forceinline__ uint32_t fa_width(int32_t v) {
  uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v, w = v < 0 ? 2u : 1u;
  while (a >= 10u) {
    a /= 10u;
    ++w;
  }
  return w;
}

struct FaCols {
  uint64_t *rec_off, *pos_after;
  int32_t* position;
  uint32_t *len, *klen;
};

// next() over data line k = line k + 1 of `starts`, k < m.  first_rel = first_pos - text_base.
// small[0] = the lines that start below hi (the split's end), small[1] = the first line that consumes
// FA_MAX_LINE bytes or more.
__global__ __launch_bounds__(VCF_WG) void k_fa_lines(const uint8_t* __restrict__ text,
                                                     const uint32_t* __restrict__ starts, uint32_t total, uint32_t wlen,
                                                     uint32_t m, uint32_t hi, uint64_t text_base, uint32_t first_rel,
                                                     uint32_t index_len, FaCols o, uint32_t* __restrict__ small) {
  const uint32_t k = blockIdx.x * VCF_WG + threadIdx.x;
  if (k >= m) return;
  const SeqLine a = seq_line(text, starts, k + 1u, total, wlen);
  const uint32_t after = a.s + a.consumed;
  if (a.s < hi && (k + 1u == m || after >= hi)) small[0] = k + 1u;  // one lane: the starts ascend
  if (a.consumed >= FA_MAX_LINE) atomicMin(&small[1], k);
  // current_split_pos is an int that advances by the bytes consumed: 1 + (offset - first_pos) mod 2^32
  const int32_t position = (int32_t)(1u + (a.s - first_rel));
  o.rec_off[k] = text_base + a.s;
  o.pos_after[k] = text_base + after;
  o.position[k] = position;
  o.len[k] = min(a.content, FA_MAX_LINE);
  o.klen[k] = index_len + fa_width(position);
}

// out[i] = max in[64 i .. 64 i + 63], a wave per output
__global__ __launch_bounds__(VCF_WG) void k_fa_maxup(const uint32_t* __restrict__ in, uint32_t n,
                                                     uint32_t* __restrict__ out) {
  const uint32_t wave = blockIdx.x * (VCF_WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if ((uint64_t)wave * 64u >= n) return;  // wave-uniform
  const uint32_t i = wave * 64u + lane;
  const uint32_t v = fa_wave_max(i < n ? in[i] : 0u);
  if (lane == 0) out[wave] = v;
}

struct FaTree {
  const uint32_t* lv[FA_LEVELS];
  uint32_t nlev;  // lv[nlev - 1] has at most 64 entries
};

// cap[k] = max(hdr_len, len[0 .. k]), a wave per 64 lines
__global__ __launch_bounds__(VCF_WG) void k_fa_cap(FaTree t, uint32_t n, uint32_t hdr_len, uint32_t* __restrict__ cap) {
  const uint32_t wave = blockIdx.x * (VCF_WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if ((uint64_t)wave * 64u >= n) return;  // wave-uniform
  const uint32_t k = wave * 64u + lane;
  uint32_t v = k < n ? t.lv[0][k] : 0u;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)v, o);
    if ((int)lane >= o) v = max(v, u);
  }
  // the lines before this group: on level l the earlier siblings of the group's ancestor
  uint32_t p = hdr_len, i = wave;
  for (uint32_t l = 1; l < t.nlev; ++l) {
    const uint32_t lo = i & ~63u;
    if (lo + lane < i) p = max(p, t.lv[l][lo + lane]);
    i >>= 6;
  }
  p = fa_wave_max(p);
  if (k < n) cap[k] = max(v, p);
}

// The largest j < r with lv[0][j] > c; FA_NONE when no data line before r is longer than c (the
// header then covers column c).  Going up, level l looks at the earlier siblings of r's ancestor
// (at most 63); the group found is complete (it lies before that ancestor), so going down each
// level looks at 64 children of which one exceeds c.
__device__ __forceinline__ uint32_t fa_cover(const FaTree& t, uint32_t r, uint32_t c) {
  uint32_t l = 0, i = r;
  for (;;) {
    const uint32_t lo = i & ~63u;
    uint32_t j = i;
    while (j > lo && t.lv[l][j - 1u] <= c) --j;
    if (j > lo) {
      uint32_t f = j - 1u;
      while (l > 0) {
        --l;
        const uint32_t b = f * 64u;
        uint32_t e = b + 64u;
        while (e > b && t.lv[l][e - 1u] <= c) --e;
        if (e == b) return FA_NONE;  // (not reached: the group's maximum exceeds c)
        f = e - 1u;
      }
      return f;
    }
    if (l + 1u >= t.nlev) return FA_NONE;
    i >>= 6;
    ++l;
  }
}

// the low n bytes of (s0, s1) into (w0, w1) at byte d; d + n <= 16
__device__ __forceinline__ void fa_put(uint64_t& w0, uint64_t& w1, uint64_t s0, uint64_t s1, uint32_t d, uint32_t n) {
  if (n < 8u) {
    s0 &= (1ull << (8u * n)) - 1ull;
    s1 = 0;
  } else if (n < 16u) {
    s1 &= (1ull << (8u * (n - 8u))) - 1ull;
  }
  if (d >= 8u) {
    s1 = s0 << (8u * (d - 8u));
    s0 = 0;
  } else if (d) {
    s1 = s1 << (8u * d) | s0 >> (64u - 8u * d);
    s0 <<= 8u * d;
  }
  w0 |= s0;
  w1 |= s1;
}

// The sequence pool.  Wave w fills the output of lines [64 w, 64 w + 64): bytes seq_off[64 w] ..
// seq_off[64 w + 64), walked in aligned 16-byte quads, a quad per lane and 1 KiB per step.  A quad is
// put together in registers from at most 16 source runs (a line's own bytes, then one run per step of
// the staircase of covering lines) and stored whole; the run's first and last quad, which it shares
// with its neighbours, are stored by bytes.  hdr_s = the header line's window-relative start.
__global__ __launch_bounds__(VCF_WG) void k_fa_seq(const uint8_t* __restrict__ text,
                                                   const uint32_t* __restrict__ starts, FaTree t, uint32_t n,
                                                   uint32_t hdr_s, const uint64_t* __restrict__ seq_off,
                                                   uint8_t* __restrict__ out) {
  const uint32_t wave = blockIdx.x * (VCF_WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if ((uint64_t)wave * 64u >= n) return;
  const uint32_t k0 = wave * 64u, k1 = min(n, k0 + 64u);
  const uint64_t o0 = seq_off[k0], o1 = seq_off[k1];
  for (uint64_t q = (o0 & ~15ull) + 16ull * lane; q < o1; q += 1024ull) {
    const uint64_t lo = max(q, o0), hi = min(q + 16u, o1);
    // the record that holds byte lo (every record has at least the header's one byte)
    uint32_t r = k0, rb = k1;
    while (rb - r > 1u) {
      const uint32_t mid = (r + rb) >> 1;
      if (seq_off[mid] <= lo) r = mid;
      else rb = mid;
    }
    uint64_t w0 = 0, w1 = 0, pos = lo;
    uint64_t ro = seq_off[r], re = seq_off[r + 1u];
    while (pos < hi) {
      const uint32_t c = (uint32_t)(pos - ro), own = t.lv[0][r];
      uint32_t src, run;
      if (c < own) {
        src = starts[r + 1u];
        run = own - c;
      } else {
        const uint32_t j = fa_cover(t, r, c);
        src = j == FA_NONE ? hdr_s : starts[j + 1u];
        run = j == FA_NONE ? (uint32_t)(re - pos) : t.lv[0][j] - c;
      }
      run = (uint32_t)min((uint64_t)run, min(re, hi) - pos);
      const uint8_t* const p = text + src + c;
      fa_put(w0, w1, seq_ld8(p), seq_ld8(p + 8), (uint32_t)(pos - q), run);
      pos += run;
      if (pos == re && pos < hi) {
        ++r;
        ro = re;
        re = seq_off[r + 1u];
      }
    }
    if (hi - lo == 16ull) {
      *reinterpret_cast<uint4*>(out + q) =
          make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
    } else {
      for (uint64_t b = lo; b < hi; ++b) {
        const uint32_t d = (uint32_t)(b - q);
        out[b] = (uint8_t)((d < 8u ? w0 >> (8u * d) : w1 >> (8u * (d - 8u))) & 0xffu);
      }
    }
  }
}

// The key pool: a thread per 16-byte piece of a key (`pieces` per record).  index_s = the
// indexSequence's window-relative start.
__global__ __launch_bounds__(VCF_WG) void k_fa_keys(const uint8_t* __restrict__ text, uint32_t index_s,
                                                    uint32_t index_len, uint32_t pieces, uint64_t n,
                                                    const int32_t* __restrict__ position,
                                                    const uint64_t* __restrict__ key_off, uint8_t* __restrict__ out) {
  const uint64_t tid = (uint64_t)blockIdx.x * VCF_WG + threadIdx.x;
  const uint64_t r = tid / pieces;
  if (r >= n) return;
  const uint32_t b0 = 16u * (uint32_t)(tid % pieces);
  const uint64_t ko = key_off[r];
  const uint32_t klen = (uint32_t)(key_off[r + 1u] - ko);
  if (b0 >= klen) return;
  const uint32_t b1 = min(b0 + 16u, klen), nd = klen - index_len;
  const int32_t pv = position[r];
  const uint32_t a = pv < 0 ? 0u - (uint32_t)pv : (uint32_t)pv;
  for (uint32_t b = b0; b < b1; ++b) {
    uint8_t ch;
    if (b < index_len) {
      ch = text[index_s + b];
      if (ch == '\t') ch = ':';
    } else if (pv < 0 && b == index_len) {
      ch = '-';
    } else {
      uint32_t v = a;
      for (uint32_t e = nd - 1u - (b - index_len); e; --e) v /= 10u;
      ch = (uint8_t)('0' + v % 10u);
    }
    out[ko + b] = ch;
  }
}

}  // namespace hbam

namespace {

int fa_check_window(hbam_ctx* c, const uint8_t* text, uint64_t text_len) {
  if (!c || (!text && text_len)) return HBAM_EINVAL;
  if (text_len > VCF_MAX_WINDOW) return set_err(c, HBAM_EINVAL, "a FASTA window is at most 2 GiB");
  return HBAM_OK;
}

// a call that ends before any record is read: status and positions only, both pools empty
int fa_nothing(hbam_ctx* c, uint32_t wlen, uint64_t text_base, uint64_t first_pos, int32_t status,
               hbam_fasta_columns* out) {
  uint64_t* off;
  int rc = ensure(c, B_FA_SCAN, 4, &off);
  if (rc) return rc;
  HIPCHK(c, hipMemsetAsync(off, 0, 16, c->stream));
  for (int e = 2; e <= 4; ++e) HIPCHK(c, hipEventRecord(c->ev[e], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  out->status = status;
  out->first_pos = out->end_pos = first_pos;
  out->err_pos = status != HBAM_OK ? first_pos : 0;
  out->seq_off = off;
  out->key_off = off + 1;
  out->text_base = text_base;
  c->timing.scan_ms = ev_ms(c, 0, 1);
  c->timing.walk_ms = ev_ms(c, 1, 2);
  c->timing.total_ms = ev_ms(c, 0, 4);
  c->timing.ubuf_bytes = wlen;
  return HBAM_OK;
}

}  // namespace

extern "C" int hbam_fasta_sections(hbam_ctx* c, const uint8_t* text, int on_device, uint64_t text_base,
                                   uint64_t text_len, uint64_t* out_off, uint64_t cap, uint64_t* n) {
  int rc = fa_check_window(c, text, text_len);
  if (rc) return rc;
  if (!n || (cap && !out_off)) return HBAM_EINVAL;
  *n = 0;
  if (text_len == 0) return HBAM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  c->timing = hbam_timing{};
  const uint8_t* d;
  if ((rc = stage_comp(c, text, on_device, text_len, &d))) return rc;
  const uint32_t shift = (uint32_t)((uintptr_t)d & 15u);
  const uint32_t end = (uint32_t)text_len + shift;
  const uint32_t ntiles = (end + VCF_TILE - 1) / VCF_TILE;
  uint16_t* gtmap;
  uint32_t* cnt;
  uint64_t* tfirst;
  if ((rc = ensure(c, B_FA_GT, (uint64_t)ntiles * (VCF_TILE / 16), &gtmap)) ||
      (rc = ensure(c, B_FA_CNT, (uint64_t)ntiles + 1, &cnt)) || (rc = ensure(c, B_FA_OFF, (uint64_t)ntiles + 1, &tfirst)))
    return rc;
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  k_fa_gt_scan<<<grid_for(ntiles, VCF_WG / 64), VCF_WG, 0, c->stream>>>(d - shift, end, shift, ntiles, gtmap, cnt);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  uint64_t total = 0;
  if ((rc = scan_exclusive<uint32_t>(c, cnt, ntiles, tfirst, &total))) return rc;
  *n = total;
  if (total > cap) return set_err(c, HBAM_EMORE, "%llu section starts, room for %llu", (unsigned long long)total,
                                  (unsigned long long)cap);
  if (total) {
    uint64_t* offs;
    if ((rc = ensure(c, B_FA_SECT, total, &offs))) return rc;
    k_fa_gt_scatter<<<grid_for(ntiles, VCF_WG / 64), VCF_WG, 0, c->stream>>>(gtmap, ntiles, tfirst, shift, text_base,
                                                                             total, offs);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    HIPCHK(c, copy_sync(c, out_off, offs, 8 * total, hipMemcpyDeviceToHost));
    c->timing.scan_ms = ev_ms(c, 0, 1);
    c->timing.walk_ms = ev_ms(c, 1, 2);
    c->timing.total_ms = ev_ms(c, 0, 2);
  }
  c->timing.ubuf_bytes = text_len;
  c->timing.n_records = total;
  return HBAM_OK;
}

extern "C" int hbam_fasta_decode_split(hbam_ctx* c, const uint8_t* text, int on_device, uint64_t text_base,
                                       uint64_t text_len, uint64_t file_len, uint64_t start, uint64_t length,
                                       hbam_fasta_columns* out) {
  if (!c || !text || !out) return HBAM_EINVAL;
  memset(out, 0, sizeof *out);
  int rc = fa_check_window(c, text, text_len);
  if (rc) return rc;
  if (text_base + text_len > file_len) return set_err(c, HBAM_EINVAL, "window past the end of the file");
  if (start > file_len) return set_err(c, HBAM_EINVAL, "the split starts past the end of the file");
  if (text_base > start) return set_err(c, HBAM_EINVAL, "the window starts after the reader's first byte");
  HIPCHK(c, hipSetDevice(c->device));
  const uint64_t q0 = std::min(start - text_base, text_len);
  const bool at_eof = text_base + text_len == file_len;
  const uint64_t end_abs = length > ~0ull - start ? ~0ull : start + length;
  c->timing = hbam_timing{};
  FragLines L;
  if ((rc = frag_text_lines(c, text, on_device, text_len, q0, 1, at_eof, false, &L))) return rc;
  // readLine(buffer, min(20000, end - start)) stores nothing for an empty split, whatever the line
  // holds; the header line does not exist at the end of the file: substring(1, 0) raises either way
  if (length == 0 || (L.nl == 0 && at_eof)) return fa_nothing(c, L.wlen, text_base, start, HBAM_EINDEX, out);
  if (L.nl == 0) return fa_nothing(c, L.wlen, text_base, start, HBAM_EMORE, out);
  uint32_t* small;
  if ((rc = ensure(c, B_FA_SMALL, 8, &small))) return rc;
  k_fa_header<<<1, 64, 0, c->stream>>>(L.d, L.starts, L.total, L.wlen,
                                       (uint32_t)std::min<uint64_t>(FA_MAX_LINE, length), small);
  HIPCHK(c, hipGetLastError());
  uint32_t hd[3];
  HIPCHK(c, copy_sync(c, hd, small, 12, hipMemcpyDeviceToHost));
  const uint32_t hdr_len = hd[0], hdr_s = (uint32_t)q0;
  if (hdr_len == 0) return fa_nothing(c, L.wlen, text_base, start, HBAM_EINDEX, out);
  if (hd[2]) return fa_nothing(c, L.wlen, text_base, start, HBAM_EUNSUPPORTED, out);
  const uint32_t first_rel = hdr_s + hd[1], index_len = hdr_len - 1u;
  const uint64_t first_pos = text_base + first_rel;
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));

  const uint32_t m = L.nl - 1u;  // complete data lines
  const uint64_t hi64 = end_abs > text_base ? end_abs - text_base : 0;
  const uint32_t hi = (uint32_t)std::min<uint64_t>(hi64, 0xffffffffull);
  FaCols cols{};
  {
    uint8_t* base;
    const uint64_t mm = ((uint64_t)m + 4) & ~3ull;  // every array stays 16-byte aligned
    if ((rc = ensure(c, B_FA_COLS, mm * (8 + 8 + 4 + 4 + 4), &base))) return rc;
    cols.rec_off = (uint64_t*)base;
    cols.pos_after = cols.rec_off + mm;
    cols.position = (int32_t*)(cols.pos_after + mm);
    cols.len = (uint32_t*)cols.position + mm;
    cols.klen = cols.len + mm;
  }
  uint32_t nbelow = 0, first_err = FA_NONE;
  if (m) {
    HIPCHK(c, hipMemsetAsync(small, 0, 4, c->stream));
    HIPCHK(c, hipMemsetAsync(small + 1, 0xff, 4, c->stream));
    k_fa_lines<<<grid_for(m, VCF_WG), VCF_WG, 0, c->stream>>>(L.d, L.starts, L.total, L.wlen, m, hi, text_base, first_rel,
                                                              index_len, cols, small);
    HIPCHK(c, hipGetLastError());
    uint32_t h[2];
    HIPCHK(c, copy_sync(c, h, small, 8, hipMemcpyDeviceToHost));
    nbelow = h[0];
    first_err = h[1];
  }
  uint32_t n = nbelow;
  int32_t status = HBAM_OK;
  uint64_t err_pos = 0, end_pos = first_pos;
  if (first_err < nbelow) {
    n = first_err;  // "found abnormally large line": the reader's position is behind it
    status = HBAM_ERUNTIME;
    HIPCHK(c, copy_sync(c, &err_pos, cols.rec_off + n, 8, hipMemcpyDeviceToHost));
    HIPCHK(c, copy_sync(c, &end_pos, cols.pos_after + n, 8, hipMemcpyDeviceToHost));
  } else {
    if (n) HIPCHK(c, copy_sync(c, &end_pos, cols.pos_after + (n - 1), 8, hipMemcpyDeviceToHost));
    if (!at_eof && nbelow == m) {
      // the window's incomplete last line (line nl of `starts`): the reader reads it when it starts
      // below the split's end
      uint32_t s_last;
      if ((rc = frag_start(c, L.starts, L.nl, L.total, L.wlen, &s_last))) return rc;
      if (s_last < hi) {
        status = HBAM_EMORE;
        err_pos = text_base + s_last;
      }
    }
  }

  // cap_k and the two pools' offsets
  uint32_t* cap = nullptr;
  uint64_t *seq_off, *key_off;
  {
    uint64_t* scans;
    const uint64_t n1 = (((uint64_t)n + 1) + 1) & ~1ull;
    if ((rc = ensure(c, B_FA_SCAN, 2 * n1, &scans))) return rc;
    seq_off = scans;
    key_off = scans + n1;
  }
  FaTree tree{};
  uint64_t seq_len = 0, key_len = 0;
  if (n) {
    uint32_t* up;
    if ((rc = ensure(c, B_FA_TREE, (uint64_t)n / 32 + 64 * FA_LEVELS, &up)) || (rc = ensure(c, B_FA_CAP, (uint64_t)n, &cap)))
      return rc;
    tree.lv[0] = cols.len;
    tree.nlev = 1;
    for (uint32_t cnt = n; cnt > 64u && tree.nlev < FA_LEVELS;) {
      const uint32_t nout = (cnt + 63u) / 64u;
      k_fa_maxup<<<grid_for(nout, VCF_WG / 64), VCF_WG, 0, c->stream>>>(tree.lv[tree.nlev - 1], cnt, up);
      tree.lv[tree.nlev++] = up;
      up += (nout + 3u) & ~3u;
      cnt = nout;
    }
    k_fa_cap<<<grid_for((n + 63u) / 64u, VCF_WG / 64), VCF_WG, 0, c->stream>>>(tree, n, hdr_len, cap);
    HIPCHK(c, hipGetLastError());
    if ((rc = scan_exclusive<uint32_t>(c, cap, n, seq_off, &seq_len)) ||
        (rc = scan_exclusive<uint32_t>(c, cols.klen, n, key_off, &key_len)))
      return rc;
  } else {
    HIPCHK(c, hipMemsetAsync(seq_off, 0, 8, c->stream));
    HIPCHK(c, hipMemsetAsync(key_off, 0, 8, c->stream));
  }
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));

  uint8_t *seq, *key;
  if ((rc = ensure(c, B_FA_SEQ, seq_len + 16, &seq)) || (rc = ensure(c, B_FA_KEY, key_len + 16, &key))) return rc;
  if (n) {
    k_fa_seq<<<grid_for((n + 63u) / 64u, VCF_WG / 64), VCF_WG, 0, c->stream>>>(L.d, L.starts, tree, n, hdr_s, seq_off, seq);
    const uint32_t pieces = (index_len + 11u + 15u) / 16u;
    const uint64_t kg = ((uint64_t)n * pieces + VCF_WG - 1) / VCF_WG;
    if (kg > 0x7fffffffull) return set_err(c, HBAM_ENOMEM, "the key pool of %u records does not fit", n);
    k_fa_keys<<<(uint32_t)kg, VCF_WG, 0, c->stream>>>(L.d, hdr_s + 1u, index_len, pieces, n, cols.position, key_off, key);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  out->n = n;
  out->status = status;
  out->err_pos = err_pos;
  out->first_pos = first_pos;
  out->end_pos = end_pos;
  out->rec_off = cols.rec_off;
  out->pos_after = cols.pos_after;
  out->position = cols.position;
  out->line_len = cols.len;
  out->key_off = key_off;
  out->seq_off = seq_off;
  out->key = key;
  out->seq = seq;
  out->key_len = key_len;
  out->seq_len = seq_len;
  out->index_off = hdr_s + 1u;
  out->index_len = index_len;
  out->text_base = text_base;
  c->timing.scan_ms = ev_ms(c, 0, 1);
  c->timing.walk_ms = ev_ms(c, 1, 2);
  c->timing.decode_ms = ev_ms(c, 2, 3);
  c->timing.pools_ms = ev_ms(c, 3, 4);
  c->timing.total_ms = ev_ms(c, 0, 4);
  c->timing.ubuf_bytes = L.wlen;
  c->timing.n_records = n;
  c->timing.pool_bytes = key_len + seq_len;
  return HBAM_OK;
}

extern "C" int hbam_fasta_columns_to_host(hbam_ctx* c, const hbam_fasta_columns* dv, hbam_fasta_columns* h) {
  if (!c || !dv || !h || dv->host) return HBAM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  *h = *dv;
  h->host = 1;
  const uint64_t n = dv->n, m = n + 1;
  // one allocation, rec_off first: hbam_fasta_release frees it through that pointer
  const uint64_t bytes = 8 * (2 * n + 2 * m) + 4 * (2 * n) + dv->key_len + dv->seq_len + 64;
  uint8_t* blk = (uint8_t*)malloc(bytes);
  if (!blk) {
    memset(h, 0, sizeof *h);
    return set_err(c, HBAM_ENOMEM, "hbam_fasta_columns_to_host: %llu records", (unsigned long long)n);
  }
  uint8_t* p = blk;
  hipError_t e = hipSuccess;
  auto take = [&](const void* src, size_t b) -> void* {
    void* dst = p;
    if (b && e == hipSuccess) e = hipMemcpyAsync(dst, src, b, hipMemcpyDeviceToHost, c->stream);
    p += b;
    return dst;
  };
  h->rec_off = (uint64_t*)take(dv->rec_off, 8 * n);
  h->pos_after = (uint64_t*)take(dv->pos_after, 8 * n);
  h->key_off = (uint64_t*)take(dv->key_off, 8 * m);
  h->seq_off = (uint64_t*)take(dv->seq_off, 8 * m);
  h->position = (int32_t*)take(dv->position, 4 * n);
  h->line_len = (uint32_t*)take(dv->line_len, 4 * n);
  h->key = (uint8_t*)take(dv->key, dv->key_len);
  h->seq = (uint8_t*)take(dv->seq, dv->seq_len);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    free(blk);
    memset(h, 0, sizeof *h);
    return set_err(c, HBAM_EDEVICE, "hbam_fasta_columns_to_host: %s", hipGetErrorString(e));
  }
  return HBAM_OK;
}

extern "C" void hbam_fasta_release(hbam_ctx* c, hbam_fasta_columns* cols) {
  (void)c;
  if (!cols) return;
  if (cols->host) free(cols->rec_off);
  memset(cols, 0, sizeof *cols);
}
