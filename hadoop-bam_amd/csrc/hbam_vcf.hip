// hbam_vcf.hip — text VCF on the device: VCFRecordReader (VCFRecordReader.java:72-142) over one
// FileSplit, and the line gather of the vcf-sort plugin (cli/plugins/VCFSort.java).  Included at
// the end of hbam_capi.hip, after hbam_lines.hip (it uses that file's buffers, scan and staging
// helpers, and the shared line-structure front end).  gfx950, wave64.
//
//   k_line_scan<false, true>, (scan_exclusive), k_vcf_starts   the '\n' and '\t' bitmaps and the
//                       start offset of every line: text_lines (hbam_lines.hip).
//   k_vcf_fields        field pass, a lane per line: the first 8 tabs from the tab bitmap, the line
//                       length ('\r' before the '\n' trimmed), POS, len(REF), CHROM -> contig
//                       ordinal (open-addressing table, byte compare) or the CharSequence
//                       MurmurHash3, the key and the status.  The walk ends at the 8th tab (or at the
//                       end of a line that has fewer): the sample columns are never touched, and the
//                       line length comes from the next line's start.
//   hbam_vcf_gather_lines  lines perm[0..n), each followed by '\n', packed: the Sort path's unit
//                       gather (k_gather_records_tile) over k_vcf_line_rel's offsets, then
//                       k_vcf_line_ends.
//
// The line and decode rules restate htsjdk's AsciiLineReader / AsciiLineReaderIterator and a subset
// of VCFCodec.decode (htsjdk is not in the reference tree: parity unpinned, DESIGN.md lists them).
// A lone '\r' (not followed by '\n') is not a line end here.

namespace hbam {

struct VcfCols {
  uint64_t* line_off;
  int64_t* key;
  uint32_t* tab;
  uint32_t* line_len;
  int32_t* chrom;
  int32_t* pos;
  int32_t* ref_len;
  int32_t* status;
};

__device__ __forceinline__ uint64_t vcf_rotl(uint64_t x, int r) { return x << r | x >> (64 - r); }
__device__ __forceinline__ uint64_t vcf_fmix(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  return k ^ k >> 33;
}
// util/MurmurHash3.java:108-171 over a CharSequence whose UTF-16 code units are the n bytes at c,
// h1 = h2 = (long)seed (sign-extended).  Both quirks of the reference are kept: the block step rotates h2 as
// h2 << 31 | h1 >>> 33 (:139), and the tail (n & 7) reads charAt(0..6), the START of the string.
__device__ int64_t murmur3_java_chars(const uint8_t* c, uint32_t n, int32_t seed = 0) {
  const uint64_t c1 = 0x87c37b91114253d5ull, c2 = 0x4cf5ad432745937full;
  uint64_t h1 = (uint64_t)(int64_t)seed, h2 = h1;
  for (uint32_t i = 0; i + 8 <= n; i += 8) {
    uint64_t k1 = (uint64_t)c[i] | (uint64_t)c[i + 1] << 16 | (uint64_t)c[i + 2] << 32 | (uint64_t)c[i + 3] << 48;
    uint64_t k2 = (uint64_t)c[i + 4] | (uint64_t)c[i + 5] << 16 | (uint64_t)c[i + 6] << 32 | (uint64_t)c[i + 7] << 48;
    k1 *= c1; k1 = vcf_rotl(k1, 31); k1 *= c2; h1 ^= k1;
    h1 = vcf_rotl(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729ull;
    k2 *= c2; k2 = vcf_rotl(k2, 33); k2 *= c1; h2 ^= k2;
    h2 = h2 << 31 | h1 >> 33; h2 += h1; h2 = h2 * 5 + 0x38495ab5ull;
  }
  const uint32_t r = n & 7u;
  uint64_t k1 = 0, k2 = 0;
  if (r >= 5) {
    for (uint32_t j = 4; j < r; ++j) k2 ^= (uint64_t)c[j] << (16 * (j - 4));
    k2 *= c2; k2 = vcf_rotl(k2, 33); k2 *= c1; h2 ^= k2;
  }
  if (r >= 1) {
    for (uint32_t j = 0; j < (r < 4 ? r : 4u); ++j) k1 ^= (uint64_t)c[j] << (16 * j);
    k1 *= c1; k1 = vcf_rotl(k1, 31); k1 *= c2; h1 ^= k1;
  }
  h1 ^= n; h2 ^= n;
  h1 += h2;
  h2 += h1;
  h1 = vcf_fmix(h1);
  h2 = vcf_fmix(h2);
  return (int64_t)(h1 + h2);
}

// the contig table's hash (host and device): FNV-1a over the name's bytes
__host__ __device__ __forceinline__ uint32_t vcf_name_hash(const uint8_t* p, uint32_t n) {
  uint32_t h = 2166136261u;
  for (uint32_t i = 0; i < n; ++i) h = (h ^ p[i]) * 16777619u;
  return h;
}

// Integer.valueOf: [+-]? digit+ inside int32
__device__ __forceinline__ bool vcf_parse_int(const uint8_t* p, uint32_t n, int32_t* out) {
  if (n == 0) return false;
  uint32_t i = 0;
  const bool neg = p[0] == '-';
  if (neg || p[0] == '+') i = 1;
  if (i == n) return false;
  uint64_t v = 0;
  for (; i < n; ++i) {
    const uint32_t d = (uint32_t)p[i] - '0';
    if (d > 9u) return false;
    v = v * 10 + d;
    if (v > 0x80000000ull) v = 0x80000001ull;  // saturate: any count of digits
  }
  if (v > (neg ? 0x80000000ull : 0x7fffffffull)) return false;
  *out = neg ? (int32_t)(0 - (uint32_t)v) : (int32_t)v;
  return true;
}

// VCFRecordReader.nextKeyValue per line.  text = the window (unshifted), tabmap64 the shifted tab
// bitmap read as 64-bit words; hi = the window-relative bound a line must start below to be
// returned (min(position limit, end of file)).  *n_cand = the lines that start below it.
__global__ __launch_bounds__(VCF_WG) void k_vcf_fields(const uint8_t* __restrict__ text,
                                                       const uint64_t* __restrict__ tabmap64, uint32_t shift,
                                                       const uint32_t* __restrict__ starts, uint32_t total, uint32_t hi,
                                                       uint64_t text_base, const hbam_vcf_contig* __restrict__ table,
                                                       uint32_t tmask, const uint8_t* __restrict__ names, VcfCols o,
                                                       unsigned long long* first_stop, uint32_t* n_cand) {
  const uint32_t i = blockIdx.x * VCF_WG + threadIdx.x;
  if (i >= total) return;
  const uint32_t s = starts[i];
  if (s >= hi) return;
  const uint32_t nxt = starts[i + 1];
  const bool has_nl = i + 1 < total;
  if (!has_nl || nxt >= hi) *n_cand = i + 1;  // one lane: the starts ascend
  uint32_t len = nxt - 1u - s;
  const uint8_t* const l = text + s;
  if (has_nl && len && l[len - 1] == '\r') --len;
  // the first 8 tabs inside the line
  uint32_t tab[8];
  uint32_t k = 0;
  {
    const uint32_t p = s + shift, pe = p + len;
    uint32_t word = p >> 6;
    uint64_t bits = tabmap64[word] & (~0ull << (p & 63u));
    while (k < 8) {
      if (bits == 0) {
        ++word;
        if (((uint64_t)word << 6) >= pe) break;
        bits = tabmap64[word];
        continue;
      }
      const uint32_t at = (word << 6) + (uint32_t)__builtin_ctzll(bits);
      if (at >= pe) break;
      bits &= bits - 1;
      tab[k++] = at - p;
    }
  }
  const uint32_t ntab = k;
  for (; k < 8; ++k) tab[k] = len;
  int32_t status = HBAM_OK, chrom = 0, pos = 0, ref_len = 0;
  int64_t key = 0;
  if (len && l[0] == '#') {
    status = HBAM_ERUNTIME;  // VCFCodec.decode returns null for a header line: NullPointerException
  } else if (ntab < 7) {
    status = HBAM_ETRIBBLE;  // fewer than 8 fields
  } else if (!vcf_parse_int(l + tab[0] + 1, tab[1] - tab[0] - 1, &pos)) {
    status = HBAM_ETRIBBLE;
  } else {
    ref_len = (int32_t)(tab[3] - tab[2] - 1);
    const uint32_t cl = tab[0];
    bool hit = false;
    for (uint32_t h = vcf_name_hash(l, cl) & tmask;; h = (h + 1) & tmask) {
      const hbam_vcf_contig e = table[h];
      if (e.ordinal < 0) break;  // an empty slot: the table is at most half full
      if (e.name_len != cl) continue;
      const uint8_t* nm = names + e.name_off;
      uint32_t j = 0;
      while (j < cl && nm[j] == l[j]) ++j;
      if (j == cl) {
        chrom = e.ordinal;
        hit = true;
        break;
      }
    }
    if (!hit) chrom = (int32_t)murmur3_java_chars(l, cl);
    key = (int64_t)((uint64_t)(int64_t)chrom << 32) | (int64_t)(int32_t)((uint32_t)pos - 1u);
  }
  o.line_off[i] = text_base + s;
  o.line_len[i] = len;
  uint4* const t4 = reinterpret_cast<uint4*>(o.tab + 8ull * i);
  t4[0] = make_uint4(tab[0], tab[1], tab[2], tab[3]);
  t4[1] = make_uint4(tab[4], tab[5], tab[6], tab[7]);
  o.chrom[i] = chrom;
  o.pos[i] = pos;
  o.ref_len[i] = ref_len;
  o.key[i] = key;
  o.status[i] = status;
  if (status != HBAM_OK) atomicMin(first_stop, (unsigned long long)i);
}

__global__ __launch_bounds__(VCF_WG) void k_vcf_line_lens(const uint32_t* __restrict__ line_len,
                                                          const uint32_t* __restrict__ perm, uint64_t n,
                                                          uint32_t* __restrict__ lens) {
  const uint64_t i = (uint64_t)blockIdx.x * VCF_WG + threadIdx.x;
  if (i < n) lens[i] = line_len[perm ? perm[i] : i] + 1u;
}

// The line gather is the record gather of the Sort path (k_gather_records_tile, hbam_sort.hip: a
// wave per 64 output lines, every line cut into 16-byte units dealt to consecutive lanes, so a long
// line is the whole wave's job) over window-relative line offsets: it copies line_len + 1 bytes per
// line, the line and the byte after it, and k_vcf_line_ends then makes that last byte '\n' (it
// is '\r' for a "\r\n" line, and the pad after the text for a last line without '\n').
__global__ __launch_bounds__(VCF_WG) void k_vcf_line_rel(const uint64_t* __restrict__ line_off, uint64_t text_base,
                                                         uint64_t n, uint64_t* __restrict__ rel) {
  const uint64_t i = (uint64_t)blockIdx.x * VCF_WG + threadIdx.x;
  if (i < n) rel[i] = line_off[i] - text_base;
}

__global__ __launch_bounds__(VCF_WG) void k_vcf_line_ends(const uint64_t* __restrict__ out_off, uint64_t n,
                                                          uint8_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * VCF_WG + threadIdx.x;
  if (i < n) out[out_off[i + 1] - 1] = '\n';
}

}  // namespace hbam

namespace {

int vcf_cols(hbam_ctx* c, uint64_t n, VcfCols* k) {
  uint8_t* base;
  int rc;
  const uint64_t m = (n + 4) & ~3ull;  // a multiple of 4: every column stays 16-byte aligned
  if ((rc = ensure(c, B_VCF_COLS, m * (2 * 8 + 8 * 4 + 5 * 4) + 64, &base))) return rc;
  k->line_off = (uint64_t*)base;
  k->key = (int64_t*)(base + 8 * m);
  k->tab = (uint32_t*)(base + 16 * m);
  uint32_t* q4 = (uint32_t*)(base + 48 * m);
  k->line_len = q4;
  k->chrom = (int32_t*)(q4 + m);
  k->pos = (int32_t*)(q4 + 2 * m);
  k->ref_len = (int32_t*)(q4 + 3 * m);
  k->status = (int32_t*)(q4 + 4 * m);
  return HBAM_OK;
}

}  // namespace

extern "C" int hbam_vcf_decode_split(hbam_ctx* c, const uint8_t* text, int on_device, uint64_t text_base,
                                     uint64_t text_len, uint64_t file_len, uint64_t start, uint64_t length,
                                     uint64_t data_start, const hbam_vcf_contig* table, uint32_t table_size,
                                     const uint8_t* names, uint64_t names_len, int32_t keep_text,
                                     hbam_vcf_columns* out) {
  if (!c || !text || !out || !table || (names_len && !names)) return HBAM_EINVAL;
  memset(out, 0, sizeof *out);
  HIPCHK(c, hipSetDevice(c->device));
  if (table_size == 0 || (table_size & (table_size - 1)))
    return set_err(c, HBAM_EINVAL, "the contig table's size must be a power of two");
  if (text_len > VCF_MAX_WINDOW) return set_err(c, HBAM_EINVAL, "a VCF window is at most 2 GiB");
  if (text_base + text_len > file_len) return set_err(c, HBAM_EINVAL, "window past the end of the file");
  int rc = contig_table_check(c, table, table_size, names_len, CONTIG_TABLE);
  if (rc) return rc;
  // VCFRecordReader.java:101-117 opens the reader (reader_bounds).  nextKeyValue: a line is returned
  // while one exists and its position < length (:129), positions counted from where the reader was
  // opened (0, or start - 1)
  const uint64_t hi_abs = std::min(start ? start + length - 1 : length, file_len);
  ReaderBounds b;
  if ((rc = reader_bounds(c, start, data_start, text_base, text_len, hi_abs, &b))) return rc;
  c->timing = hbam_timing{};
  TextLines L;
  if ((rc = text_lines(c, text, on_device, text_len, b.q0, b.explicit_first, false, false, true, &L))) return rc;
  const uint64_t total = L.total;
  const uint8_t* const d = L.d;
  VcfCols vc;
  uint64_t* small;
  if ((rc = vcf_cols(c, total, &vc)) || (rc = ensure(c, B_VCF_SMALL, 4, &small))) return rc;
  unsigned long long* first_stop = (unsigned long long*)small;
  uint32_t* n_cand_d = (uint32_t*)(small + 1);
  HIPCHK(c, hipMemsetAsync(small, 0xff, 8, c->stream));
  HIPCHK(c, hipMemsetAsync(small + 1, 0, 8, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  if (total) {
    hbam_vcf_contig* dtab;
    uint8_t* dnames;
    if ((rc = contig_table_upload(c, table, table_size, names, names_len, &dtab, &dnames))) return rc;
    k_vcf_fields<<<grid_for(total, VCF_WG), VCF_WG, 0, c->stream>>>(d, (const uint64_t*)L.tabmap, L.shift, L.starts,
                                                                    (uint32_t)total, b.hi, text_base, dtab,
                                                                    table_size - 1, dnames, vc, first_stop, n_cand_d);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  HIPCHK(c, hipMemcpyAsync(c->pinned_small, small, 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  uint64_t n;
  int32_t status;
  if ((rc = window_cut(c, c->pinned_small[0], c->pinned_small[1] & 0xffffffffull, total, text_base + text_len, file_len,
                       hi_abs, vc.status, &n, &status)))
    return rc;
  out->n = n;
  out->status = status;
  out->line_off = vc.line_off;
  out->line_len = vc.line_len;
  out->tab = vc.tab;
  out->chrom = vc.chrom;
  out->pos = vc.pos;
  out->ref_len = vc.ref_len;
  out->key = vc.key;
  out->text = keep_text ? (uint8_t*)d : nullptr;
  out->text_base = text_base;
  out->text_len = text_len;
  c->timing.scan_ms = ev_ms(c, 0, 1);
  c->timing.walk_ms = ev_ms(c, 1, 2);
  c->timing.decode_ms = ev_ms(c, 2, 3);
  c->timing.total_ms = ev_ms(c, 0, 3);
  c->timing.ubuf_bytes = text_len;
  c->timing.n_records = n;
  return HBAM_OK;
}

extern "C" int hbam_vcf_columns_to_host(hbam_ctx* c, const hbam_vcf_columns* dv, hbam_vcf_columns* h) {
  if (!c || !dv || !h || dv->host) return HBAM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  memset(h, 0, sizeof *h);
  h->host = 1;
  h->n = dv->n;
  h->status = dv->status;
  h->text_base = dv->text_base;
  const uint64_t n = dv->n;
  if (n == 0) return HBAM_OK;
  uint8_t* blk = (uint8_t*)malloc(n * (2 * 8 + 8 * 4 + 4 * 4));
  if (!blk) return set_err(c, HBAM_ENOMEM, "hbam_vcf_columns_to_host: %llu lines", (unsigned long long)n);
  // one allocation, line_off first: hbam_vcf_release frees it through that pointer
  h->line_off = (uint64_t*)blk;
  h->key = (int64_t*)(blk + 8 * n);
  h->tab = (uint32_t*)(blk + 16 * n);
  h->line_len = (uint32_t*)(blk + 48 * n);
  h->chrom = (int32_t*)(blk + 52 * n);
  h->pos = (int32_t*)(blk + 56 * n);
  h->ref_len = (int32_t*)(blk + 60 * n);
  hipError_t e = hipSuccess;
  auto cp = [&](void* dst, const void* src, size_t bytes) {
    if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
  };
  cp(h->line_off, dv->line_off, 8 * n);
  cp(h->key, dv->key, 8 * n);
  cp(h->tab, dv->tab, 32 * n);
  cp(h->line_len, dv->line_len, 4 * n);
  cp(h->chrom, dv->chrom, 4 * n);
  cp(h->pos, dv->pos, 4 * n);
  cp(h->ref_len, dv->ref_len, 4 * n);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    free(blk);
    memset(h, 0, sizeof *h);
    return set_err(c, HBAM_EDEVICE, "hbam_vcf_columns_to_host: %s", hipGetErrorString(e));
  }
  return HBAM_OK;
}

extern "C" void hbam_vcf_release(hbam_ctx* c, hbam_vcf_columns* cols) {
  (void)c;
  if (!cols) return;
  if (cols->host) free(cols->line_off);
  memset(cols, 0, sizeof *cols);
}

extern "C" int hbam_vcf_gather_lines(hbam_ctx* c, const hbam_vcf_columns* dv, const uint32_t* perm, uint64_t n,
                                     uint8_t* out, uint64_t out_cap, uint64_t* out_off, uint64_t* total_bytes) {
  if (!c || !dv || dv->host || !out_off || (n && (!dv->line_len || !dv->line_off))) return HBAM_EINVAL;
  if (n && (dv->n == 0 || (!perm && n > dv->n)))
    return set_err(c, HBAM_EINVAL, "hbam_vcf_gather_lines: n > the columns' lines");
  if (out && n && !dv->text) return set_err(c, HBAM_EINVAL, "hbam_vcf_gather_lines: the decode did not keep the text");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  uint32_t* lens;
  if ((rc = ensure(c, B_S_LENS, n + 1, &lens))) return rc;
  HIPCHK(c, hipEventRecord(c->ev[9], c->stream));
  if (n) k_vcf_line_lens<<<grid_for(n, VCF_WG), VCF_WG, 0, c->stream>>>(dv->line_len, perm, n, lens);
  HIPCHK(c, hipGetLastError());
  uint64_t tot = 0;
  if ((rc = scan_exclusive(c, lens, n, out_off, &tot))) return rc;
  if (total_bytes) *total_bytes = tot;
  if (!out) return HBAM_OK;  // size query
  if (tot > out_cap)
    return set_err(c, HBAM_EINVAL, "hbam_vcf_gather_lines: %llu bytes > out_cap %llu", (unsigned long long)tot,
                   (unsigned long long)out_cap);
  if (n) {
    uint64_t* rel;  // by source line: perm indexes it
    if ((rc = ensure(c, B_VCF_REL, dv->n + 1, &rel))) return rc;
    k_vcf_line_rel<<<grid_for(dv->n, VCF_WG), VCF_WG, 0, c->stream>>>(dv->line_off, dv->text_base, dv->n, rel);
    k_gather_records_tile<<<(uint32_t)std::min<uint64_t>((n + 255) / 256, POOLS_MAX_WG), 256, 0, c->stream>>>(
        dv->text, rel, perm, n, out_off, out);
    k_vcf_line_ends<<<grid_for(n, VCF_WG), VCF_WG, 0, c->stream>>>(out_off, n, out);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev[10], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->timing.pools_ms = ev_ms(c, 9, 10);
  c->timing.pool_bytes = tot;
  return HBAM_OK;
}
