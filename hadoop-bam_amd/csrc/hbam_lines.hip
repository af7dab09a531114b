// hbam_lines.hip — the line structure of a text window, and what the line-oriented readers share
// around it: the front end of hbam_vcf.hip, hbam_sam.hip and hbam_fastq.hip.  Included by
// hbam_capi.hip ahead of them (it uses that file's buffers, scan and staging helpers).  gfx950, wave64.
//
//   k_line_scan<HADOOP_EOL, TABS>   structural pass: every lane loads 16 bytes (a wave covers 1 KiB
//                       per step, a tile is VCF_STEPS steps), turns them into a 16-bit line-end mask
//                       and (TABS) a 16-bit '\t' mask, stores the bitmaps and the tile's line count.
//                       HADOOP_EOL = false: a line ends at '\n' (htsjdk's AsciiLineReader as the VCF
//                       and SAM readers use it; a lone '\r' is not a line end).  HADOOP_EOL = true:
//                       LineReader.readLine's rule (LineReader.java:111-173), LF, a lone CR and CRLF
//                       all end a line.  Bit i is then set iff b[i] == '\n', or b[i] == '\r' and the
//                       byte after it is not '\n': the bit marks the LAST byte of a terminator, so
//                       k_vcf_starts works on it unchanged.  The byte after a quad is one more load
//                       (it crosses quad, step, tile and window boundaries alike); the byte after the
//                       window is "not LF" at the end of the file and "LF" before it (a CR there
//                       stays open: the line is incomplete).
//   (scan_exclusive)    line counts per tile -> first line index of each tile.
//   k_vcf_starts        scatter: the start offset of every line (the byte after each line end) from
//                       the line-end bitmap alone (1/8 of the text's bytes).
//   text_lines          the host driver of the three: staging, bitmaps, scan, starts.
//
// The window contract lives here: a window is at most VCF_MAX_WINDOW bytes, may start at any
// address (the kernels work on `shifted` positions), and a cut inside its last line is answered
// with HBAM_EMORE (window_cut) so that the caller passes a longer one.

namespace hbam {

constexpr uint32_t VCF_WG = 256;
constexpr uint32_t VCF_STEPS = 4;                 // 1 KiB wave steps per tile
constexpr uint32_t VCF_TILE = 1024 * VCF_STEPS;   // bytes per wave
constexpr uint64_t VCF_MAX_WINDOW = 1ull << 31;   // relative offsets are u32

// bit j = (byte j of the 16 == c)
__device__ __forceinline__ uint32_t vcf_eq4(uint32_t w, uint32_t c4) {
  const uint32_t x = w ^ c4;
  const uint32_t t = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);  // 0x80 in every zero byte
  return (((t >> 7) * 0x00204081u) >> 21) & 0xfu;
}
__device__ __forceinline__ uint32_t vcf_eq16(const uint4 q, uint32_t c) {
  const uint32_t c4 = c * 0x01010101u;
  return vcf_eq4(q.x, c4) | vcf_eq4(q.y, c4) << 4 | vcf_eq4(q.z, c4) << 8 | vcf_eq4(q.w, c4) << 12;
}

// Positions in the two structural kernels are `shifted`: relative to text16 = the window's first
// byte rounded down to 16 (shift = the bytes in between), so every load is an aligned quad.
// end = window bytes + shift; q0 = the first position whose line end starts a line of this reader;
// tail_lf (HADOOP_EOL only) = the byte after the window counts as '\n'.
template <bool HADOOP_EOL, bool TABS>
__global__ __launch_bounds__(VCF_WG) void k_line_scan(const uint8_t* __restrict__ text16, uint32_t end, uint32_t q0,
                                                      uint32_t ntiles, uint16_t* __restrict__ nlmap,
                                                      uint16_t* __restrict__ tabmap, uint32_t* __restrict__ count,
                                                      uint32_t tail_lf) {
  const uint32_t wave = blockIdx.x * (VCF_WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (wave >= ntiles) return;  // wave-uniform
  uint32_t cnt = 0;
#pragma unroll
  for (uint32_t s = 0; s < VCF_STEPS; ++s) {
    const uint64_t b = (uint64_t)wave * VCF_TILE + s * 1024u + lane * 16u;
    uint32_t nl = 0, tb = 0;
    if (b < end) {
      const uint4 q = *reinterpret_cast<const uint4*>(text16 + b);
      // the byte after the quad: inside the window a load, behind it the caller's answer
      bool next_lf = false;
      if constexpr (HADOOP_EOL) next_lf = b + 16 < end ? text16[b + 16] == '\n' : tail_lf != 0;
      const uint32_t hi = (uint32_t)min((uint64_t)16, (uint64_t)end - b);
      const uint32_t lo = q0 > b ? (uint32_t)min((uint64_t)16, (uint64_t)q0 - b) : 0u;
      const uint32_t in = (1u << hi) - 1u;
      if constexpr (TABS) tb = vcf_eq16(q, '\t') & in;
      nl = vcf_eq16(q, '\n') & in;
      if constexpr (HADOOP_EOL) {
        // LF directly after byte i: bit i + 1 of the LF mask, the quad's successor for i = 15, the
        // window's for the window's last byte (hi < 16 only in the window's last quad)
        uint32_t lf_after = nl >> 1;
        if (next_lf) lf_after |= 1u << (hi - 1u);
        nl |= vcf_eq16(q, '\r') & in & ~lf_after;
      }
      nl &= ~((1u << lo) - 1u);
    }
    nlmap[b >> 4] = (uint16_t)nl;
    if constexpr (TABS) tabmap[b >> 4] = (uint16_t)tb;
    cnt += (uint32_t)__popc(nl);
  }
  const uint32_t tot = wave_last(wave_scan_dpp(cnt));
  if (lane == 0) count[wave] = tot;
}

// starts[first + k] = the byte after the k-th counted line end (window-relative, unshifted);
// starts[0] = first_start when the reader has a first line that no line end of the window precedes
// (explicit = 1: a split starting at 0 begins at data_start); starts[total] = wlen + 1, so the
// last line's end (starts[i + 1] - 1) is the end of the window.
__global__ __launch_bounds__(VCF_WG) void k_vcf_starts(const uint16_t* __restrict__ nlmap, uint32_t ntiles,
                                                       const uint64_t* __restrict__ tile_first, uint32_t shift,
                                                       uint32_t explicit_first, uint32_t first_start, uint32_t total,
                                                       uint32_t wlen, uint32_t* __restrict__ starts) {
  const uint32_t wave = blockIdx.x * (VCF_WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (wave >= ntiles) return;
  if (wave == 0 && lane == 0) {
    if (explicit_first) starts[0] = first_start;
    starts[total] = wlen + 1u;
  }
  uint32_t base = (uint32_t)tile_first[wave] + explicit_first;
  for (uint32_t s = 0; s < VCF_STEPS; ++s) {
    const uint64_t b = (uint64_t)wave * VCF_TILE + s * 1024u + lane * 16u;
    uint32_t m = nlmap[b >> 4];
    const uint32_t c = (uint32_t)__popc(m);
    const uint32_t incl = wave_scan_dpp(c);
    uint32_t at = base + incl - c;
    while (m) {
      const uint32_t j = (uint32_t)__builtin_ctz(m);
      m &= m - 1u;
      if (at < total) starts[at] = (uint32_t)b + j + 1u - shift;  // (at < total always: a bound, not a rule)
      ++at;
    }
    base += wave_last(incl);
  }
}

}  // namespace hbam

namespace {

struct TextLines {
  const uint8_t* d;  // the window on the device
  uint32_t shift, total, wlen;
  uint32_t* starts;
  uint16_t* tabmap;  // nullptr without tabs (and for an empty window)
};

// Structural pass + line starts over one window: events 0 (begin) and 1 (after the structural
// kernel); the caller records event 2 where its own walk ends.  q0 = the first window-relative
// position whose line end counts; explicit_first: the reader's first line starts at q0 itself.
// hadoop_eol picks the line rule (k_line_scan), at_eof what follows the window under it.
int text_lines(hbam_ctx* c, const uint8_t* text, int on_device, uint64_t text_len, uint64_t q0,
               uint32_t explicit_first, bool hadoop_eol, bool at_eof, bool want_tabs, TextLines* L) {
  int rc = stage_comp(c, text, on_device, text_len, &L->d);
  if (rc) return rc;
  if (q0 >= text_len) explicit_first = 0;  // the reader opens at the window's end: no line starts there
  const uint32_t shift = (uint32_t)((uintptr_t)L->d & 15u);
  const uint32_t end = (uint32_t)text_len + shift;
  const uint32_t ntiles = (end + VCF_TILE - 1) / VCF_TILE;
  L->shift = shift;
  L->wlen = (uint32_t)text_len;
  L->tabmap = nullptr;
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  uint64_t m_all = 0;
  uint16_t* nlmap = nullptr;
  uint64_t* tfirst = nullptr;
  if (ntiles) {
    uint32_t* cnt;
    const uint64_t quads = (uint64_t)ntiles * (VCF_TILE / 16);
    if (!hadoop_eol) want_tabs = true;  // (the '\n' rule has no caller without tabs)
    // + 4: a field pass reads the 64-bit tab word of a line that starts at the window's last byte + 1
    if ((rc = ensure(c, B_VCF_NL, quads, &nlmap)) || (want_tabs && (rc = ensure(c, B_VCF_TAB, quads + 4, &L->tabmap))) ||
        (rc = ensure(c, B_VCF_CNT, (uint64_t)ntiles + 1, &cnt)) ||
        (rc = ensure(c, B_VCF_OFF, (uint64_t)ntiles + 1, &tfirst)))
      return rc;
    const auto scan = !hadoop_eol ? k_line_scan<false, true> : want_tabs ? k_line_scan<true, true> : k_line_scan<true, false>;
    scan<<<grid_for(ntiles, VCF_WG / 64), VCF_WG, 0, c->stream>>>(L->d - shift, end, (uint32_t)q0 + shift, ntiles, nlmap,
                                                                   L->tabmap, cnt, at_eof ? 0u : 1u);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    if ((rc = scan_exclusive<uint32_t>(c, cnt, ntiles, tfirst, &m_all))) return rc;
  } else {
    HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  }
  const uint64_t total = m_all + explicit_first;
  if ((rc = ensure(c, B_VCF_STARTS, total + 2, &L->starts))) return rc;
  if (ntiles)
    k_vcf_starts<<<grid_for(ntiles, VCF_WG / 64), VCF_WG, 0, c->stream>>>(
        nlmap, ntiles, tfirst, shift, explicit_first, (uint32_t)q0, (uint32_t)total, (uint32_t)text_len, L->starts);
  HIPCHK(c, hipGetLastError());
  L->total = (uint32_t)total;
  return HBAM_OK;
}

// ---- the name table of the VCF and SAM readers (hbam_vcf_contig: open addressing, FNV-1a) ----

struct TableWords {
  const char *table, *items;  // the error messages' wording
};
constexpr TableWords CONTIG_TABLE{"contig", "contigs"}, DICTIONARY_TABLE{"dictionary", "sequences"};

int contig_table_check(hbam_ctx* c, const hbam_vcf_contig* table, uint32_t table_size, uint64_t names_len,
                       const TableWords& what) {
  uint32_t used = 0;
  for (uint32_t i = 0; i < table_size; ++i) {
    if (table[i].ordinal < 0) continue;
    ++used;
    if ((uint64_t)table[i].name_off + table[i].name_len > names_len)
      return set_err(c, HBAM_EINVAL, "%s table entry %u points outside the names", what.table, i);
  }
  if ((uint64_t)used * 2 > table_size)  // a probe ends at an empty slot
    return set_err(c, HBAM_EINVAL, "the %s table must be at least twice the number of %s", what.table, what.items);
  return HBAM_OK;
}

int contig_table_upload(hbam_ctx* c, const hbam_vcf_contig* table, uint32_t table_size, const uint8_t* names,
                        uint64_t names_len, hbam_vcf_contig** dtab, uint8_t** dnames) {
  int rc;
  if ((rc = ensure(c, B_VCF_TABLE, (uint64_t)table_size, dtab)) || (rc = ensure(c, B_VCF_NAMES, names_len + 1, dnames)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(*dtab, table, (size_t)table_size * sizeof *table, hipMemcpyHostToDevice, c->stream));
  if (names_len) HIPCHK(c, hipMemcpyAsync(*dnames, names, names_len, hipMemcpyHostToDevice, c->stream));
  return HBAM_OK;
}

// ---- the window of a reader that opens one byte before its split (VCF, SAM) ----

struct ReaderBounds {
  uint64_t q0;              // window-relative: the first position whose '\n' starts a line of the reader
  uint32_t hi;              // window-relative: a line must start below it to be returned
  uint32_t explicit_first;  // the reader's first line starts at q0 itself
};

// The reader is opened at q0: a split at 0 reads from data_start, any other discards through the
// first '\n' at or after start - 1.  hi_abs = the file offset below which a returned line starts
// (the format's own rule).
int reader_bounds(hbam_ctx* c, uint64_t start, uint64_t data_start, uint64_t text_base, uint64_t text_len,
                  uint64_t hi_abs, ReaderBounds* b) {
  const uint64_t q0_abs = start ? start - 1 : data_start;
  if (q0_abs < text_base) return set_err(c, HBAM_EINVAL, "the window starts after the reader's first byte");
  b->q0 = std::min(q0_abs - text_base, text_len);
  b->hi = (uint32_t)std::min<uint64_t>(hi_abs > text_base ? hi_abs - text_base : 0, 0xffffffffull);
  b->explicit_first = (start == 0 && q0_abs - text_base < text_len) ? 1u : 0u;
  return HBAM_OK;
}

// What the per-line pass found -> the lines returned and the call's status.  fs = the first line
// with a status (>= total: none), n_cand = the lines that start below hi.  The window ends inside
// the last line it would return (or before the reader's bound with no line at all), and the file
// goes on: HBAM_EMORE, the caller passes a longer window.
int window_cut(hbam_ctx* c, uint64_t fs, uint64_t n_cand, uint64_t total, uint64_t window_end, uint64_t file_len,
               uint64_t hi_abs, const int32_t* line_status, uint64_t* n, int32_t* status) {
  *n = n_cand;
  *status = HBAM_OK;
  const bool cut = window_end < file_len &&
                   (total == 0 ? window_end < hi_abs : (n_cand == total && fs >= total - 1));
  if (cut) {
    *n = total ? total - 1 : 0;
    *status = HBAM_EMORE;
  } else if (fs < n_cand) {
    *n = fs;
    HIPCHK(c, copy_sync(c, status, line_status + fs, 4, hipMemcpyDeviceToHost));
  }
  return HBAM_OK;
}

}  // namespace
