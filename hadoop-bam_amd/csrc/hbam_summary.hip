// hbam_summary.hip — the reduce side of the summarize plugin and SummarySort, device side + C ABI.
// Included at the end of hbam_capi.hip (one translation unit; it uses hbam_sort_keys, the scans,
// hbam_consumers.hip's f4_key0, hbam_lines.hip's front end through hbam_fastq.hip's frag_text_lines /
// seq_line, and hbam_vcf.hip's vcf_parse_int).  gfx950, wave64.
//
//  * hbam_summarize_reduce — SummarizeReducer (cli/plugins/chipster/Summarize.java:466-561) as one
//    reducer over the whole job: the ranges ordered by key (hbam_sort_keys: ties in input order),
//    cut into segments where the key's high word changes, each strand's ranges of a segment cut
//    into groups of L for every level L, one RangeCount line per group.  The stateful loop becomes
//      k_sm_flags     per sorted position: forward-strand flag, segment-head flag
//      (scan x 2)     position inside the strand, segment index
//      k_sm_scatter   stable partition: beg / end compacted, forward strand first, then reverse;
//                     per segment its bounds in each strand's compacted index space and its rid
//      (scan x 2)     64-bit prefix sums of the sign-extended beg and end (wraparound is Java's)
//      k_sm_gcount    groups per (level, strand, segment) = ceil(ranges / L)
//      (scan)         first output line of each (level, strand, segment); of each stream
//      k_sm_groups    a lane per output line: sums as prefix differences, Java's truncating long
//                     division, the four columns
//      k_sm_linekey + hbam_sort_keys per stream + k_sm_apply   (sort_output: SummarySort's order)
//      k_sm_linelen, (scan), k_sm_render   RangeCount.toString + '\n' per line
//    No atomics: every output has one writer, so a call's bytes are reproducible.
//    The reducer's flush quirk is kept: reduce() sets currentReferenceID to the NEW reference before
//    doAllSummaries() (:508-511), so a trailing partial group flushed at a segment change carries the
//    rid of the segment that follows; the last segment's (flushed by cleanup) carries its own.
//  * hbam_summary_keys — SortRecordReader.nextKeyValue (chipster/SummarySort.java:240-260) over an
//    inflated summary file read as one split: LineReader lines, the first two tabs from the tab
//    bitmap, Integer.parseInt of both fields, getKey0(rid, pos).
//  * hbam_summary_gather_lines — SortOutputFormat's text: lines perm[0..n), each ended by '\n'.

namespace hbam {

constexpr uint32_t SM_WG = 256;

// ---- reduce ---------------------------------------------------------------------------------
__global__ __launch_bounds__(SM_WG) void k_sm_flags(const int64_t* __restrict__ skey, const uint32_t* __restrict__ perm,
                                                    const uint8_t* __restrict__ rev, uint64_t n,
                                                    uint32_t* __restrict__ isf, uint32_t* __restrict__ head) {
  const uint64_t i = (uint64_t)blockIdx.x * SM_WG + threadIdx.x;
  if (i >= n) return;
  isf[i] = rev[perm[i]] ? 0u : 1u;
  head[i] = (i == 0 || ((uint64_t)skey[i] >> 32) != ((uint64_t)skey[i - 1] >> 32)) ? 1u : 0u;
}

// posf / segp: the exclusive scans of isf / head.  Compacted index: forward ranges at [0, nf) in
// stream order, reverse ranges at [nf, n).  sb: u64[2][nseg + 1], each strand's segment bounds in
// its own index space (forward: [0, nf], reverse: [0, n - nf]).
__global__ __launch_bounds__(SM_WG) void k_sm_scatter(const int64_t* __restrict__ skey, const uint32_t* __restrict__ perm,
                                                      const int32_t* __restrict__ beg, const int32_t* __restrict__ end,
                                                      uint64_t n, const uint32_t* __restrict__ isf,
                                                      const uint32_t* __restrict__ head, const uint64_t* __restrict__ posf,
                                                      const uint64_t* __restrict__ segp, uint64_t nf, uint64_t nseg,
                                                      int32_t* __restrict__ cbeg, int32_t* __restrict__ cend,
                                                      uint64_t* __restrict__ sb, int32_t* __restrict__ srid) {
  const uint64_t i = (uint64_t)blockIdx.x * SM_WG + threadIdx.x;
  if (i >= n) return;
  const uint32_t src = perm[i];
  const uint64_t pf = posf[i], pr = i - pf;
  const uint64_t dst = isf[i] ? pf : nf + pr;
  cbeg[dst] = beg[src];
  cend[dst] = end[src];
  if (head[i]) {
    const uint64_t s = segp[i];
    if (s < nseg) {  // (always: a bound, not a rule)
      sb[s] = pf;
      sb[nseg + 1 + s] = pr;
      srid[s] = (int32_t)((uint64_t)skey[i] >> 32);
    }
  }
  if (i == 0) {
    sb[nseg] = nf;
    sb[2 * nseg + 1] = n - nf;
  }
}

// entry e = (level * 2 + strand) * nseg + segment
__global__ __launch_bounds__(SM_WG) void k_sm_gcount(const uint64_t* __restrict__ sb, uint64_t nseg,
                                                     const int32_t* __restrict__ levels, uint64_t m,
                                                     uint32_t* __restrict__ gc) {
  const uint64_t e = (uint64_t)blockIdx.x * SM_WG + threadIdx.x;
  if (e >= m) return;
  const uint64_t seg = e % nseg, st = e / nseg, s = st & 1u;
  const uint64_t L = (uint64_t)levels[st >> 1];
  const uint64_t cnt = sb[s * (nseg + 1) + seg + 1] - sb[s * (nseg + 1) + seg];
  gc[e] = (uint32_t)((cnt + L - 1) / L);
}

// out[k] = src[k * stride] (first line of each stream from the per-entry bases), k <= n_streams
__global__ __launch_bounds__(64) void k_sm_pick(const uint64_t* __restrict__ src, uint64_t stride, uint32_t count,
                                                uint64_t* __restrict__ out) {
  const uint32_t k = blockIdx.x * 64 + threadIdx.x;
  if (k < count) out[k] = src[(uint64_t)k * stride];
}
// out[k] = src[idx[k]]
__global__ __launch_bounds__(64) void k_sm_pick_at(const uint64_t* __restrict__ src, const uint64_t* __restrict__ idx,
                                                   uint32_t count, uint64_t* __restrict__ out) {
  const uint32_t k = blockIdx.x * 64 + threadIdx.x;
  if (k < count) out[k] = src[idx[k]];
}

// SummarizeReducer.doSummary (:548-560) for output line j.  gbase: the exclusive scan of gc (m + 1
// entries); pbeg / pend: the exclusive prefix sums over the compacted arrays (n + 1 entries).
__global__ __launch_bounds__(SM_WG) void k_sm_groups(const uint64_t* __restrict__ gbase, uint64_t m, uint64_t nseg,
                                                     const int32_t* __restrict__ levels, const uint64_t* __restrict__ sb,
                                                     uint64_t nf, const int32_t* __restrict__ srid,
                                                     const uint64_t* __restrict__ pbeg, const uint64_t* __restrict__ pend,
                                                     uint64_t total, int32_t* __restrict__ rid, int32_t* __restrict__ beg,
                                                     int32_t* __restrict__ end, int32_t* __restrict__ count) {
  const uint64_t j = (uint64_t)blockIdx.x * SM_WG + threadIdx.x;
  if (j >= total) return;
  // the last entry whose base is <= j: the entries between it and the next larger base are empty
  uint64_t lo = 0, hi = m;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (gbase[mid] <= j) lo = mid;
    else hi = mid;
  }
  const uint64_t e = lo, seg = e % nseg, st = e / nseg, s = st & 1u;
  const uint64_t L = (uint64_t)levels[st >> 1];
  const uint64_t a = sb[s * (nseg + 1) + seg], b = sb[s * (nseg + 1) + seg + 1];
  const uint64_t g = j - gbase[e];
  const uint64_t off = s ? nf : 0;
  const uint64_t r0 = min(a + g * L, b), r1 = min(r0 + L, b);
  const uint64_t cnt = r1 - r0;
  if (cnt == 0) return;  // (never: gc counted this group; a bound, not a rule)
  const int64_t sum_beg = (int64_t)(pbeg[off + r1] - pbeg[off + r0]);
  const int64_t sum_end = (int64_t)(pend[off + r1] - pend[off + r0]);
  // a partial group is written by doAllSummaries: at a segment change currentReferenceID is
  // already the next segment's (:508-511), at cleanup it is still the last segment's
  rid[j] = (cnt < L && seg + 1 < nseg) ? srid[seg + 1] : srid[seg];
  beg[j] = (int32_t)(sum_beg / (int64_t)cnt);  // long division truncates toward zero, (int) narrows
  end[j] = (int32_t)(sum_end / (int64_t)cnt);
  count[j] = (int32_t)cnt;
}

__global__ __launch_bounds__(SM_WG) void k_sm_linekey(const int32_t* __restrict__ rid, const int32_t* __restrict__ beg,
                                                      uint64_t n, int64_t* __restrict__ key) {
  const uint64_t j = (uint64_t)blockIdx.x * SM_WG + threadIdx.x;
  if (j < n) key[j] = f4_key0(rid[j], beg[j]);
}

// one stream's lines [first, first + cnt): dst[first + i] = src[first + lperm[first + i]] for the
// four columns (cols: rid, beg, end, count, each `pitch` apart)
__global__ __launch_bounds__(SM_WG) void k_sm_apply(const int32_t* __restrict__ src, const uint32_t* __restrict__ lperm,
                                                    uint64_t first, uint64_t cnt, uint64_t pitch,
                                                    int32_t* __restrict__ dst) {
  const uint64_t i = (uint64_t)blockIdx.x * SM_WG + threadIdx.x;
  if (i >= cnt) return;
  const uint64_t p = lperm[first + i];
  if (p >= cnt) return;  // (never: hbam_sort_keys' permutation; a bound, not a rule)
#pragma unroll
  for (uint32_t c = 0; c < 4; ++c) dst[c * pitch + first + i] = src[c * pitch + first + p];
}

__device__ __forceinline__ uint32_t sm_mag(int32_t v) { return v < 0 ? 0u - (uint32_t)v : (uint32_t)v; }
__device__ __forceinline__ uint32_t sm_digits(uint32_t m) {
  uint32_t d = 1;
  for (uint32_t p = 10; d < 10 && m >= p; p *= 10) ++d;  // p = 10^d: 10^9 < 2^32, the loop ends at d = 10
  return d;
}
__device__ __forceinline__ uint32_t sm_int_len(int32_t v) { return sm_digits(sm_mag(v)) + (v < 0 ? 1u : 0u); }
// Integer.toString(v) ending just before `e`; returns its first byte
__device__ __forceinline__ uint8_t* sm_put_int(uint8_t* e, int32_t v) {
  uint32_t m = sm_mag(v);
  do {
    *--e = (uint8_t)('0' + m % 10u);
    m /= 10u;
  } while (m);
  if (v < 0) *--e = '-';
  return e;
}

// RangeCount.toString (:601-606) + TextOutputFormat's newline: the line's length
__global__ __launch_bounds__(SM_WG) void k_sm_linelen(const int32_t* __restrict__ rid, const int32_t* __restrict__ beg,
                                                      const int32_t* __restrict__ end, const int32_t* __restrict__ count,
                                                      uint64_t n, uint32_t* __restrict__ len) {
  const uint64_t j = (uint64_t)blockIdx.x * SM_WG + threadIdx.x;
  if (j < n) len[j] = sm_int_len(rid[j]) + sm_int_len(beg[j]) + sm_int_len(end[j]) + sm_int_len(count[j]) + 4u;
}

__global__ __launch_bounds__(SM_WG) void k_sm_render(const int32_t* __restrict__ rid, const int32_t* __restrict__ beg,
                                                     const int32_t* __restrict__ end, const int32_t* __restrict__ count,
                                                     uint64_t n, const uint64_t* __restrict__ off,
                                                     uint8_t* __restrict__ text) {
  const uint64_t j = (uint64_t)blockIdx.x * SM_WG + threadIdx.x;
  if (j >= n) return;
  uint8_t* e = text + off[j + 1];
  *--e = '\n';
  e = sm_put_int(e, count[j]);
  *--e = '\t';
  e = sm_put_int(e, end[j]);
  *--e = '\t';
  e = sm_put_int(e, beg[j]);
  *--e = '\t';
  sm_put_int(e, rid[j]);
}

// ---- SummarySort's reader ---------------------------------------------------------------------
// SortRecordReader.nextKeyValue (SummarySort.java:240-260) for line i of nl.  tabmap64: the shifted
// tab bitmap as 64-bit words.  The exceptions, in the order the Java raises them: no tab ->
// Text.decode with length -1 (HBAM_EINDEX); rid not an int -> HBAM_ENUMBER; no second tab ->
// Text.decode with a negative length (HBAM_EINDEX); pos not an int -> HBAM_ENUMBER.
__global__ __launch_bounds__(VCF_WG) void k_sm_keys(const uint8_t* __restrict__ text,
                                                    const uint64_t* __restrict__ tabmap64, uint32_t shift,
                                                    const uint32_t* __restrict__ starts, uint32_t total, uint32_t nl,
                                                    uint32_t wlen, uint32_t* __restrict__ lstart,
                                                    uint32_t* __restrict__ llen, int64_t* __restrict__ key,
                                                    int32_t* __restrict__ status, uint32_t* __restrict__ bad) {
  const uint32_t i = blockIdx.x * VCF_WG + threadIdx.x;
  if (i >= nl) return;
  const SeqLine a = seq_line(text, starts, i, total, wlen);
  const uint8_t* const l = text + a.s;
  const uint32_t len = a.content;
  uint32_t tab[2] = {len, len};
  uint32_t nt = 0;
  if (len) {
    const uint32_t p = a.s + shift, pe = p + len;
    uint32_t word = p >> 6;
    uint64_t bits = tabmap64[word] & (~0ull << (p & 63u));
    while (nt < 2) {
      if (bits == 0) {
        ++word;
        if (((uint64_t)word << 6) >= pe) break;
        bits = tabmap64[word];
        continue;
      }
      const uint32_t at = (word << 6) + (uint32_t)__builtin_ctzll(bits);
      if (at >= pe) break;
      bits &= bits - 1;
      tab[nt++] = at - p;
    }
  }
  int32_t st = HBAM_OK, rid = 0, pos = 0;
  if (nt < 1) st = HBAM_EINDEX;
  else if (!vcf_parse_int(l, tab[0], &rid)) st = HBAM_ENUMBER;
  else if (nt < 2) st = HBAM_EINDEX;
  else if (!vcf_parse_int(l + tab[0] + 1, tab[1] - tab[0] - 1, &pos)) st = HBAM_ENUMBER;
  lstart[i] = a.s;
  llen[i] = len;
  key[i] = f4_key0(rid, pos);
  status[i] = st;
  bad[i] = st != HBAM_OK ? 1u : 0u;
}

// the first line with a status: the one bad line that no bad line precedes (one writer)
__global__ __launch_bounds__(VCF_WG) void k_sm_first_bad(const uint32_t* __restrict__ bad, const uint64_t* __restrict__ before,
                                                         const int32_t* __restrict__ status, uint32_t nl,
                                                         uint64_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * VCF_WG + threadIdx.x;
  if (i >= nl) return;
  if (bad[i] && before[i] == 0) {
    out[0] = i;
    out[1] = (uint64_t)(int64_t)status[i];
  }
}

// ---- SummarySort's writer ---------------------------------------------------------------------
__global__ __launch_bounds__(VCF_WG) void k_sm_glens(const uint32_t* __restrict__ llen, const uint32_t* __restrict__ perm,
                                                     uint64_t n, uint64_t n_src, uint32_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * VCF_WG + threadIdx.x;
  if (i >= n) return;
  const uint64_t p = perm ? perm[i] : i;
  out[i] = p < n_src ? llen[p] + 1u : 0u;
}

__global__ __launch_bounds__(VCF_WG) void k_sm_gather(const uint8_t* __restrict__ text, const uint32_t* __restrict__ lstart,
                                                      const uint32_t* __restrict__ perm, uint64_t n, uint64_t n_src,
                                                      const uint64_t* __restrict__ off, uint8_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * VCF_WG + threadIdx.x;
  if (i >= n) return;
  const uint64_t o = off[i], o1 = off[i + 1];
  if (o1 == o) return;
  const uint64_t p = perm ? perm[i] : i;
  if (p >= n_src) return;
  const uint8_t* s = text + lstart[p];
  const uint64_t len = o1 - o - 1;
  for (uint64_t k = 0; k < len; ++k) out[o + k] = s[k];
  out[o + len] = '\n';
}

}  // namespace hbam

// ---- C ABI ------------------------------------------------------------------------------------
extern "C" int hbam_device_copy(hbam_ctx* c, void* dst, const void* src, uint64_t bytes) {
  if (!c || (bytes && (!dst || !src))) return HBAM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, copy_sync(c, dst, src, bytes, hipMemcpyDeviceToDevice));
  return HBAM_OK;
}

extern "C" int hbam_summarize_reduce(hbam_ctx* c, const int64_t* key, const int32_t* beg, const int32_t* end,
                                     const uint8_t* rev, uint64_t n, const int32_t* levels, uint32_t n_levels,
                                     int sort_output, hbam_summary* out) {
  if (!c || !out) return HBAM_EINVAL;
  if (n && (!key || !beg || !end || !rev)) return set_err(c, HBAM_EINVAL, "hbam_summarize_reduce: null ranges");
  if (n > 0xffffffffull) return set_err(c, HBAM_EINVAL, "hbam_summarize_reduce: n > 2^32-1");
  if (!levels || n_levels == 0 || n_levels > 1024)
    return set_err(c, HBAM_EINVAL, "hbam_summarize_reduce: 1 to 1024 levels");
  for (uint32_t k = 0; k < n_levels; ++k)
    if (levels[k] <= 0) return set_err(c, HBAM_EINVAL, "hbam_summarize_reduce: level %d is not positive", levels[k]);
  HIPCHK(c, hipSetDevice(c->device));
  *out = hbam_summary{};
  const uint32_t ns = 2 * n_levels;
  int rc;
  uint64_t *first, *toff;
  int32_t* dlev;
  if ((rc = ensure(c, B_SM_FIRST, (uint64_t)ns + 1, &first)) || (rc = ensure(c, B_SM_TOFF, (uint64_t)ns + 1, &toff)) ||
      (rc = ensure(c, B_SM_LEVELS, n_levels, &dlev)))
    return rc;
  out->n_streams = ns;
  out->first = first;
  out->text_off = toff;
  if (n == 0) {  // every stream is empty
    int32_t* cols;
    uint8_t* text;
    if ((rc = ensure(c, B_SM_COLS, 4, &cols)) || (rc = ensure(c, B_SM_TEXT, 1, &text))) return rc;
    HIPCHK(c, hipMemsetAsync(first, 0, ((uint64_t)ns + 1) * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(toff, 0, ((uint64_t)ns + 1) * 8, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->rid = cols;
    out->beg = cols + 1;
    out->end = cols + 2;
    out->count = cols + 3;
    out->text = text;
    c->timing = hbam_timing{};
    return HBAM_OK;
  }
  // the shuffle: key order, ties in input order
  int64_t* skey;
  uint32_t *perm, *isf, *head;
  uint64_t *posf, *segp;
  if ((rc = ensure(c, B_SM_SKEY, n, &skey)) || (rc = ensure(c, B_SM_PERM, n, &perm)) ||
      (rc = ensure(c, B_SM_ISF, n + 1, &isf)) || (rc = ensure(c, B_SM_HEAD, n + 1, &head)) ||
      (rc = ensure(c, B_SM_POSF, n + 1, &posf)) || (rc = ensure(c, B_SM_SEGP, n + 1, &segp)))
    return rc;
  HIPCHK(c, hipEventRecord(c->ev[13], c->stream));
  if ((rc = hbam_sort_keys(c, key, n, skey, perm))) return rc;
  const double sort_ms = c->timing.total_ms;
  HIPCHK(c, hipMemcpyAsync(dlev, levels, (size_t)n_levels * 4, hipMemcpyHostToDevice, c->stream));
  k_sm_flags<<<grid_for(n, SM_WG), SM_WG, 0, c->stream>>>(skey, perm, rev, n, isf, head);
  HIPCHK(c, hipGetLastError());
  uint64_t nf = 0, nseg = 0;
  if ((rc = scan_exclusive(c, isf, n, posf, &nf)) || (rc = scan_exclusive(c, head, n, segp, &nseg))) return rc;
  const uint64_t m = (uint64_t)ns * nseg;  // nseg >= 1
  int32_t *cbeg, *cend, *srid;
  uint64_t *sb, *pbeg, *pend, *gbase;
  uint32_t* gc;
  if ((rc = ensure(c, B_SM_CBEG, n + 1, &cbeg)) || (rc = ensure(c, B_SM_CEND, n + 1, &cend)) ||
      (rc = ensure(c, B_SM_SB, 2 * (nseg + 1), &sb)) || (rc = ensure(c, B_SM_SRID, nseg + 1, &srid)) ||
      (rc = ensure(c, B_SM_PBEG, n + 1, &pbeg)) || (rc = ensure(c, B_SM_PEND, n + 1, &pend)) ||
      (rc = ensure(c, B_SM_GC, m + 1, &gc)) || (rc = ensure(c, B_SM_GBASE, m + 1, &gbase)))
    return rc;
  k_sm_scatter<<<grid_for(n, SM_WG), SM_WG, 0, c->stream>>>(skey, perm, beg, end, n, isf, head, posf, segp, nf, nseg,
                                                            cbeg, cend, sb, srid);
  HIPCHK(c, hipGetLastError());
  // sign-extended 64-bit prefix sums (scan_exclusive widens each int32_t to uint64_t)
  if ((rc = scan_exclusive<int32_t>(c, cbeg, n, pbeg, nullptr)) || (rc = scan_exclusive<int32_t>(c, cend, n, pend, nullptr)))
    return rc;
  k_sm_gcount<<<grid_for(m, SM_WG), SM_WG, 0, c->stream>>>(sb, nseg, dlev, m, gc);
  HIPCHK(c, hipGetLastError());
  uint64_t total = 0;
  if ((rc = scan_exclusive(c, gc, m, gbase, &total))) return rc;
  k_sm_pick<<<grid_for((uint64_t)ns + 1, 64), 64, 0, c->stream>>>(gbase, nseg, ns + 1, first);
  HIPCHK(c, hipGetLastError());
  const uint64_t pitch = total + 1;
  int32_t* cols;
  if ((rc = ensure(c, B_SM_COLS, 4 * pitch, &cols))) return rc;
  if (total)
    k_sm_groups<<<grid_for(total, SM_WG), SM_WG, 0, c->stream>>>(gbase, m, nseg, dlev, sb, nf, srid, pbeg, pend, total,
                                                                 cols, cols + pitch, cols + 2 * pitch, cols + 3 * pitch);
  HIPCHK(c, hipGetLastError());
  double linesort_ms = 0;
  if (sort_output && total) {  // SummarySort over each stream: getKey0(rid, beg), ties in file order
    std::vector<uint64_t> hf((size_t)ns + 1);
    HIPCHK(c, copy_sync(c, hf.data(), first, hf.size() * 8, hipMemcpyDeviceToHost));
    int64_t* lkey;
    uint32_t* lperm;
    int32_t* cols2;
    if ((rc = ensure(c, B_SM_LKEY, total, &lkey)) || (rc = ensure(c, B_SM_LPERM, total, &lperm)) ||
        (rc = ensure(c, B_SM_COLS2, 4 * pitch, &cols2)))
      return rc;
    k_sm_linekey<<<grid_for(total, SM_WG), SM_WG, 0, c->stream>>>(cols, cols + pitch, total, lkey);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemsetAsync(lperm, 0, total * 4, c->stream));  // a stream of one line: the identity
    for (uint32_t k = 0; k < ns; ++k) {
      const uint64_t f = hf[k], cnt = hf[k + 1] - hf[k];
      if (cnt > 1) {
        if ((rc = hbam_sort_keys(c, lkey + f, cnt, nullptr, lperm + f))) return rc;
        linesort_ms += c->timing.total_ms;
      }
      if (cnt) k_sm_apply<<<grid_for(cnt, SM_WG), SM_WG, 0, c->stream>>>(cols, lperm, f, cnt, pitch, cols2);
      HIPCHK(c, hipGetLastError());
    }
    cols = cols2;
  }
  // text
  uint32_t* llen;
  uint64_t* loff;
  if ((rc = ensure(c, B_SM_LLEN, total + 1, &llen)) || (rc = ensure(c, B_SM_LOFF, total + 1, &loff))) return rc;
  if (total)
    k_sm_linelen<<<grid_for(total, SM_WG), SM_WG, 0, c->stream>>>(cols, cols + pitch, cols + 2 * pitch, cols + 3 * pitch,
                                                                  total, llen);
  HIPCHK(c, hipGetLastError());
  uint64_t bytes = 0;
  if ((rc = scan_exclusive(c, llen, total, loff, &bytes))) return rc;
  uint8_t* text;
  if ((rc = ensure(c, B_SM_TEXT, bytes + 1, &text))) return rc;
  if (total)
    k_sm_render<<<grid_for(total, SM_WG), SM_WG, 0, c->stream>>>(cols, cols + pitch, cols + 2 * pitch, cols + 3 * pitch,
                                                                 total, loff, text);
  k_sm_pick_at<<<grid_for((uint64_t)ns + 1, 64), 64, 0, c->stream>>>(loff, first, ns + 1, toff);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev[14], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->timing = hbam_timing{};
  c->timing.total_ms = ev_ms(c, 13, 14);
  c->timing.scan_ms = sort_ms;        // the shuffle's radix sort
  c->timing.walk_ms = linesort_ms;    // sort_output's radix sorts
  c->timing.n_records = n;
  c->timing.n_blocks = total;
  c->timing.pool_bytes = bytes;
  out->n_lines = total;
  out->text_len = bytes;
  out->n_segments = nseg;
  out->rid = cols;
  out->beg = cols + pitch;
  out->end = cols + 2 * pitch;
  out->count = cols + 3 * pitch;
  out->text = text;
  return HBAM_OK;
}

extern "C" int hbam_summary_keys(hbam_ctx* c, const uint8_t* text, int on_device, uint64_t len,
                                 hbam_summary_lines* out) {
  if (!c || !out || (len && !text)) return HBAM_EINVAL;
  if (len > VCF_MAX_WINDOW) return set_err(c, HBAM_EINVAL, "hbam_summary_keys: more than 2^31 bytes");
  HIPCHK(c, hipSetDevice(c->device));
  *out = hbam_summary_lines{};
  c->timing = hbam_timing{};
  if (len == 0) return HBAM_OK;
  int rc;
  FragLines L;
  if ((rc = frag_text_lines(c, text, on_device, len, 0, 1, true, true, &L))) return rc;
  const uint32_t nl = L.nl;
  uint32_t *lstart, *llen, *bad;
  int64_t* key;
  int32_t* status;
  uint64_t *before, *small;
  if ((rc = ensure(c, B_SM_KSTART, (uint64_t)nl + 1, &lstart)) || (rc = ensure(c, B_SM_KLEN, (uint64_t)nl + 1, &llen)) ||
      (rc = ensure(c, B_SM_KKEY, (uint64_t)nl + 1, &key)) || (rc = ensure(c, B_SM_KST, (uint64_t)nl + 1, &status)) ||
      (rc = ensure(c, B_SM_KBAD, (uint64_t)nl + 1, &bad)) || (rc = ensure(c, B_SM_KBEFORE, (uint64_t)nl + 1, &before)) ||
      (rc = ensure(c, B_SM_KSMALL, 2, &small)))
    return rc;
  uint64_t n = nl;
  int32_t st = HBAM_OK;
  if (nl) {
    k_sm_keys<<<grid_for(nl, VCF_WG), VCF_WG, 0, c->stream>>>(L.d, (const uint64_t*)L.tabmap, L.shift, L.starts, L.total,
                                                              nl, L.wlen, lstart, llen, key, status, bad);
    HIPCHK(c, hipGetLastError());
    uint64_t nbad = 0;
    if ((rc = scan_exclusive(c, bad, nl, before, &nbad))) return rc;
    if (nbad) {
      k_sm_first_bad<<<grid_for(nl, VCF_WG), VCF_WG, 0, c->stream>>>(bad, before, status, nl, small);
      HIPCHK(c, hipGetLastError());
      uint64_t h[2] = {0, 0};
      HIPCHK(c, copy_sync(c, h, small, 16, hipMemcpyDeviceToHost));
      n = h[0];
      st = (int32_t)(int64_t)h[1];
    }
  }
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->timing.scan_ms = ev_ms(c, 0, 1);
  c->timing.total_ms = ev_ms(c, 0, 2);
  c->timing.ubuf_bytes = len;
  c->timing.n_records = n;
  out->n = n;
  out->status = st;
  out->text = L.d;
  out->start = lstart;
  out->len = llen;
  out->key = key;
  return HBAM_OK;
}

extern "C" int hbam_summary_gather_lines(hbam_ctx* c, const hbam_summary_lines* lines, const uint32_t* perm,
                                         uint64_t n, uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                                         uint64_t* total_bytes) {
  if (!c || !lines || !out_off) return HBAM_EINVAL;
  if (n && (!lines->text || !lines->start || !lines->len || (!perm && n > lines->n)))
    return set_err(c, HBAM_EINVAL, "hbam_summary_gather_lines: n > the lines");
  if (n > 0xffffffffull) return set_err(c, HBAM_EINVAL, "hbam_summary_gather_lines: n > 2^32-1");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  uint32_t* lens;
  if ((rc = ensure(c, B_SM_GLEN, n + 1, &lens))) return rc;
  HIPCHK(c, hipEventRecord(c->ev[9], c->stream));
  if (n) k_sm_glens<<<grid_for(n, VCF_WG), VCF_WG, 0, c->stream>>>(lines->len, perm, n, lines->n, lens);
  HIPCHK(c, hipGetLastError());
  uint64_t tot = 0;
  if ((rc = scan_exclusive(c, lens, n, out_off, &tot))) return rc;
  if (total_bytes) *total_bytes = tot;
  if (!out) return HBAM_OK;  // size query
  if (tot > out_cap)
    return set_err(c, HBAM_EINVAL, "hbam_summary_gather_lines: %llu bytes > out_cap %llu", (unsigned long long)tot,
                   (unsigned long long)out_cap);
  if (n) k_sm_gather<<<grid_for(n, VCF_WG), VCF_WG, 0, c->stream>>>(lines->text, lines->start, perm, n, lines->n, out_off, out);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev[10], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->timing.pools_ms = ev_ms(c, 9, 10);
  c->timing.pool_bytes = tot;
  return HBAM_OK;
}
