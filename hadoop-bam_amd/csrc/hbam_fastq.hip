// hbam_fastq.hip — FASTQ and QSEQ on the device: FastqRecordReader (FastqInputFormat.java:56-393) and
// QseqRecordReader (QseqInputFormat.java:58-429) over one FileSplit, both filling SequencedFragment
// columns.  Included at the end of hbam_capi.hip (it uses that file's buffers, scan and staging
// helpers, hbam_lines.hip's front end, hbam_vcf.hip's vcf_parse_int, and the Sort path's unit
// gather).  gfx950, wave64.
//
//   k_line_scan<true, false> (FASTQ), <true, true> (QSEQ, with the tab bitmap), (scan_exclusive),
//   k_vcf_starts      the structural pass under LineReader.readLine's line rule (LF, a lone CR and
//                     CRLF all end a line) and the start offset of every line: text_lines
//                     (hbam_lines.hip).
//   k_fq_stop         FASTQ positioning (positionAtFirstRecord, :158-200) as a per-line predicate and
//                     a min-reduction: the first '@' line below the split's end whose line + 2 is a
//                     non-empty '+' line, or (the walk's other exit) whose line + 2 does not exist.
//   k_fq_frame        a lane per four-line record: the frame's status, the three lengths, the
//                     Illumina identifier (one forward scan, the pattern needs no backtracking), the
//                     first record whose key does not match (min-reduction: the sticky flag).
//   k_fq_resolve      a lane per record once the sticky record is known: which fields the record
//                     carries, the QC filter's drop flag, the quality check.
//   k_qs_fields       QSEQ, a lane per line: the 11 fields from the tab bitmap, the ints, the flags,
//                     the quality check.
//   k_frag_select     which records the reader reads: those starting below the split's end, plus
//                     the run of QC-dropped records that carries the filter loop past it; the first
//                     record that raises (two min-reductions).
//   (scan_exclusive x4)   kept flags and the three lengths -> output rank and pool offsets.
//   k_frag_emit       compaction of the columns; k_gather_records_tile packs the pools;
//   k_qs_keys, k_frag_qual, k_frag_dots   the QSEQ key, Phred+64 -> Phred+33, '.' -> 'N'.
//
// A lane that walks a line bounds every read by the line's end, which comes from the next line's
// start (or the window's end): no read leaves the window and its 64 bytes of slack.

namespace hbam {

constexpr uint32_t FQ_MAX_LINE = 10000;   // FastqInputFormat.java:103
constexpr uint32_t QS_MAX_LINE = 20000;   // QseqInputFormat.java:103
constexpr uint32_t FRAG_NONE = 0xffffffffu;

// SequencedFragment's *_Present bits (SequencedFragment.java:53-63)
constexpr uint32_t FP_INSTRUMENT = 0x001, FP_RUN = 0x002, FP_FLOWCELL = 0x004, FP_LANE = 0x008, FP_TILE = 0x010,
                   FP_XPOS = 0x020, FP_YPOS = 0x040, FP_READ = 0x080, FP_FILTER = 0x100, FP_CONTROL = 0x200,
                   FP_INDEX = 0x400;
// per-candidate flags (FragCand.flags)
constexpr uint32_t FC_MATCH = 1, FC_HIBYTE = 2, FC_NUMERR = 4, FC_DROP = 8, FC_NAMEREAD = 16;

// candidate records of one call (indexed by candidate, before the QC filter's compaction)
struct FragCand {
  uint32_t* rstart;     // window-relative start of the record
  uint32_t* pos_after;  // window-relative reader position after the record
  uint32_t* err_pos;    // window-relative position the exception's message carries
  int32_t* status;
  uint32_t* flags;
  uint32_t* present;
  int32_t* ints;        // 8 per candidate: run lane tile xpos ypos read filter_passed control
  uint32_t* strs;       // 6 per candidate: instrument, flowcell, index as (offset, length)
  uint32_t* src;        // 3 per candidate: window-relative sources of key, seq, qual
  uint32_t* len;        // 3 arrays of ncand: key, seq, qual lengths (0 when not kept)
  uint32_t* keep;
};

struct FragOut {
  uint64_t *rec_off, *pos_after;
  uint32_t* present;
  int32_t* ints[8];
  uint32_t* strs[3];
  uint64_t* off[3];
  uint64_t* src[3];
};

// Line i of `total` starts (k_vcf_starts' array): its start, the bytes readLine consumes and the
// bytes of its content.  Only the last start can be an unterminated line; its end is the window's.
struct SeqLine {
  uint32_t s, consumed, content;
};
__device__ __forceinline__ SeqLine seq_line(const uint8_t* __restrict__ text, const uint32_t* __restrict__ starts,
                                            uint32_t i, uint32_t total, uint32_t wlen) {
  SeqLine l;
  l.s = starts[i];
  if (i + 1 < total) {
    const uint32_t nxt = starts[i + 1];
    l.consumed = nxt - l.s;
    uint32_t term = 1;
    if (text[nxt - 1] == '\n' && l.consumed >= 2 && text[nxt - 2] == '\r') term = 2;
    l.content = l.consumed - term;
  } else {
    l.consumed = l.content = wlen - l.s;
  }
  return l;
}

// positionAtFirstRecord's exits over the lines that start below hi (the split's end): the walk reads
// with maxLineLength = min(MAX_LINE_LENGTH, end - start), so from `end` on nothing is stored, no line
// is seen to begin with '@' and the walk runs to the end of the file.  stop = min(i << 2 | kind);
// kind 0 = line i is '@' and line i + 2 is a non-empty '+' line (the record starts at line i); 1 =
// line i is '@' and the file has no line i + 2 (the reference's third read returns 0 and its loop
// ends with start at line i + 1); 2 = line i + 2, or line i itself (i == nl, the window's incomplete
// last line), lies behind the window.
__global__ __launch_bounds__(VCF_WG) void k_fq_stop(const uint8_t* __restrict__ text,
                                                    const uint32_t* __restrict__ starts, uint32_t total, uint32_t nl,
                                                    uint32_t wlen, uint32_t at_eof, uint32_t hi,
                                                    unsigned long long* stop) {
  const uint32_t i = blockIdx.x * VCF_WG + threadIdx.x;
  if (i >= total || i > nl) return;
  if (starts[i] >= hi) return;
  if (i == nl) {  // (!at_eof only: at the end of the file lines [nl, total) do not exist)
    if (!at_eof) atomicMin(stop, (unsigned long long)i << 2 | 2u);
    return;
  }
  const SeqLine a = seq_line(text, starts, i, total, wlen);
  if (a.content == 0 || text[a.s] != '@') return;
  uint32_t kind;
  if (i + 2 < nl) {
    const SeqLine c = seq_line(text, starts, i + 2, total, wlen);
    if (c.content == 0 || text[c.s] != '+') return;
    kind = 0;
  } else {
    kind = at_eof ? 1u : 2u;
  }
  atomicMin(stop, (unsigned long long)i << 2 | kind);
}

__device__ __forceinline__ bool fq_digit(uint8_t c) { return (uint32_t)c - '0' <= 9u; }

// Eight bytes at any address in one load.  A lane per record walks bytes that are far from its
// neighbours' (every byte load of a wave is 64 cache lines), so the per-record passes read words and
// take the bytes from registers.  The up to 7 bytes read past a range lie in the window or its slack.
__device__ __forceinline__ uint64_t seq_ld8(const uint8_t* p) {
  uint64_t w;
  __builtin_memcpy(&w, p, 8);
  return w;
}
// any byte >= 0x80 in p[0, n)
__device__ __forceinline__ bool seq_high_byte(const uint8_t* __restrict__ p, uint32_t n) {
  uint64_t acc = 0;
  for (uint32_t b = 0; b < n; b += 8) {
    uint64_t w = seq_ld8(p + b);
    if (n - b < 8) w &= (1ull << (8 * (n - b))) - 1ull;
    acc |= w;
  }
  return (acc & 0x8080808080808080ull) != 0;
}
// p[i] for ascending i through an eight-byte window
struct SeqBytes {
  const uint8_t* p;
  uint64_t w;
  uint32_t base;
  __device__ __forceinline__ explicit SeqBytes(const uint8_t* q) : p(q), w(0), base(~7u) {}
  __device__ __forceinline__ uint8_t operator[](uint32_t i) {
    if (i - base >= 8u) {
      base = i & ~7u;
      w = seq_ld8(p + base);
    }
    return (uint8_t)(w >> (8u * (i - base)));
  }
};

// ILLUMINA_PATTERN (FastqInputFormat.java:95) matched against the whole key:
// ([^:]+):(\d+):([^:]*):(\d+):(\d+):(-?\d+):(-?\d+)\s+([123]):([YN]):(\d+):(.*)
// Every group ends at a byte its own class excludes, so one forward scan decides.  Returns FC_MATCH,
// | FC_NUMERR when a numeric group lies outside int32 (Integer.parseInt raises).  o = the key's
// window-relative offset; ints / strs as FragCand's.
__device__ __forceinline__ uint32_t fq_illumina(const uint8_t* __restrict__ key, uint32_t n, uint32_t o,
                                                int32_t* ints, uint32_t* strs) {
  SeqBytes p(key);
  uint32_t i = 0, b;
  bool numerr = false;
  // ([^:]+):
  while (i < n && p[i] != ':') ++i;
  if (i == 0 || i >= n) return 0;
  strs[0] = o;
  strs[1] = i;
  ++i;
  // -?\d+ as Integer.parseInt reads it (vcf_parse_int's saturation: any count of digits)
  auto digits = [&](bool sign, int32_t* out) -> bool {
    bool neg = false;
    if (sign && i < n && p[i] == '-') {
      neg = true;
      ++i;
    }
    const uint32_t d0 = i;
    uint64_t v = 0;
    while (i < n && fq_digit(p[i])) {
      v = v * 10 + (uint32_t)(p[i] - '0');
      if (v > 0x80000000ull) v = 0x80000001ull;
      ++i;
    }
    if (i == d0) return false;
    if (v > (neg ? 0x80000000ull : 0x7fffffffull)) numerr = true;
    else *out = neg ? (int32_t)(0 - (uint32_t)v) : (int32_t)v;
    return true;
  };
  auto colon = [&]() -> bool {
    if (i >= n || p[i] != ':') return false;
    ++i;
    return true;
  };
  if (!digits(false, &ints[0]) || !colon()) return 0;  // run
  b = i;
  while (i < n && p[i] != ':') ++i;  // ([^:]*):
  if (i >= n) return 0;
  strs[2] = o + b;
  strs[3] = i - b;
  ++i;
  if (!digits(false, &ints[1]) || !colon()) return 0;  // lane
  if (!digits(false, &ints[2]) || !colon()) return 0;  // tile
  if (!digits(true, &ints[3]) || !colon()) return 0;   // x
  if (!digits(true, &ints[4])) return 0;               // y
  b = i;  // \s+ (a key holds neither '\n' nor '\r')
  while (i < n && (p[i] == ' ' || p[i] == '\t' || p[i] == 0x0b || p[i] == '\f')) ++i;
  if (i == b) return 0;
  if (i >= n || p[i] < '1' || p[i] > '3') return 0;
  ints[5] = p[i] - '0';
  ++i;
  if (!colon()) return 0;
  if (i >= n || (p[i] != 'Y' && p[i] != 'N')) return 0;
  ints[6] = p[i] == 'N';  // setFilterPassed("N".equals(group 9))
  ++i;
  if (!colon()) return 0;
  if (!digits(false, &ints[7]) || !colon()) return 0;  // control number
  strs[4] = o + i;
  strs[5] = n - i;
  return FC_MATCH | (numerr ? FC_NUMERR : 0u);
}

// lowLevelFastqRead over candidate k = lines r0 + 4k .. r0 + 4k + 3 of nl lines.  ncand counts a
// last partial record (at_eof) or the sentinel behind the window's complete lines (!at_eof).
__global__ __launch_bounds__(VCF_WG) void k_fq_frame(const uint8_t* __restrict__ text,
                                                     const uint32_t* __restrict__ starts, uint32_t total, uint32_t nl,
                                                     uint32_t wlen, uint32_t at_eof, uint32_t r0, uint32_t ncand,
                                                     uint32_t hi, FragCand c, uint32_t* sticky, uint32_t* nbelow) {
  const uint32_t k = blockIdx.x * VCF_WG + threadIdx.x;
  if (k >= ncand) return;
  const uint32_t l0 = r0 + 4u * k;
  const uint32_t have = nl > l0 ? min(4u, nl - l0) : 0u;
  // (l0 <= total - 1 always: the sentinel's line is the window's incomplete last line)
  const uint32_t rstart = l0 < total ? starts[l0] : wlen;
  const uint32_t after = l0 + 4u < total ? starts[l0 + 4u] : wlen;
  if (rstart < hi && (k + 1 == ncand || after >= hi)) *nbelow = k + 1;  // one lane: the starts ascend
  int32_t status = HBAM_OK;
  uint32_t flags = 0, err = wlen, klen = 0, slen = 0, qlen = 0;
  uint32_t src[3] = {0, 0, 0};
  int32_t ints[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t strs[6] = {0, 0, 0, 0, 0, 0};
  SeqLine a{}, b{}, d{};
  if (have) a = seq_line(text, starts, l0, total, wlen);
  if (!at_eof && have < 4) {
    status = HBAM_EMORE;  // the record runs behind the window
  } else if (have == 0) {
    status = HBAM_ERUNTIME;  // (not reached: ncand counts no empty record at the end of the file)
  } else if (a.content == 0) {
    // skip(1) eats the terminator.  Followed by the end of the file, the next read hits it:
    // "unexpected end of file".  Followed by data, the four-line frame shifts: not restated.
    status = (at_eof && l0 + 1 == nl) ? HBAM_ERUNTIME : HBAM_EUNSUPPORTED;
  } else {
    if (have >= 3) {
      const SeqLine pl = seq_line(text, starts, l0 + 2, total, wlen);
      if (pl.content == 0 || text[pl.s] != '+') {
        status = HBAM_ERUNTIME;  // "unexpected fastq line separating sequence and quality"
        err = l0 + 3 < total ? starts[l0 + 3] : wlen;
      }
    }
    if (status == HBAM_OK && have < 4) status = HBAM_ERUNTIME;  // EOFException inside the record
  }
  if (status == HBAM_OK) {
    b = seq_line(text, starts, l0 + 1, total, wlen);
    d = seq_line(text, starts, l0 + 3, total, wlen);
    klen = min(a.content - 1u, FQ_MAX_LINE);
    slen = min(b.content, FQ_MAX_LINE);
    qlen = min(d.content, FQ_MAX_LINE);
    src[0] = a.s + 1u;
    src[1] = b.s;
    src[2] = d.s;
    err = after;
    const uint8_t* const key = text + src[0];
    flags = seq_high_byte(key, klen) ? FC_HIBYTE : fq_illumina(key, klen, src[0], ints, strs);
    if (klen >= 2 && key[klen - 2] == '/' && fq_digit(key[klen - 1])) flags |= FC_NAMEREAD;
    if (!(flags & FC_MATCH)) atomicMin(sticky, k);
  }
  c.rstart[k] = rstart;
  c.pos_after[k] = after;
  c.err_pos[k] = err;
  c.status[k] = status;
  c.flags[k] = flags;
#pragma unroll
  for (uint32_t j = 0; j < 8; ++j) c.ints[8ull * k + j] = ints[j];
#pragma unroll
  for (uint32_t j = 0; j < 6; ++j) c.strs[6ull * k + j] = strs[j];
#pragma unroll
  for (uint32_t j = 0; j < 3; ++j) c.src[3ull * k + j] = src[j];
  c.len[k] = klen;
  c.len[(uint64_t)ncand + k] = slen;
  c.len[2ull * ncand + k] = qlen;
}

// SequencedFragment.verifyQuality / convertQuality's range check over the stored quality bytes
// (bytes are signed in Java: 0x80 and above are below any minimum)
__device__ __forceinline__ bool frag_qual_ok(const uint8_t* __restrict__ q, uint32_t n, uint32_t illumina) {
  const uint32_t lo = illumina ? 64u : 33u;
  bool bad = false;
  for (uint32_t b = 0; b < n; b += 8) {
    const uint64_t w = seq_ld8(q + b);
    const uint32_t m = min(8u, n - b);
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) bad |= j < m && (uint32_t)((w >> (8 * j)) & 0xffu) - lo > 126u - lo;
  }
  return !bad;
}

// lookForIlluminaIdentifier is true for records before `sticky`.  Their Illumina fields stand; the
// sticky record and every later one carry scanNameForReadNumber's read only.
__global__ __launch_bounds__(VCF_WG) void k_fq_resolve(const uint8_t* __restrict__ text, uint32_t ncand,
                                                       uint32_t sticky, uint32_t filter, uint32_t illumina,
                                                       FragCand c) {
  const uint32_t k = blockIdx.x * VCF_WG + threadIdx.x;
  if (k >= ncand) return;
  int32_t status = c.status[k];
  uint32_t flags = c.flags[k], present = 0, keep = 0;
  if (status == HBAM_OK) {
    if (k < sticky) {  // matched (a record that does not match is the sticky one or behind it)
      present = 0x7ff;
      if (flags & FC_NUMERR) status = HBAM_ENUMBER;
    } else {
      if (k == sticky && (flags & FC_HIBYTE)) status = HBAM_EUNSUPPORTED;  // the pattern runs on the decoded string
      if (flags & FC_NAMEREAD) {
        present = FP_READ;
        c.ints[8ull * k + 5] = text[c.src[3ull * k] + c.len[k] - 1u] - '0';
      }
    }
    if (status == HBAM_OK) {
      if (filter && (present & FP_FILTER) && c.ints[8ull * k + 6] == 0) {
        flags |= FC_DROP;
      } else if (!frag_qual_ok(text + c.src[3ull * k + 2], c.len[2ull * ncand + k], illumina)) {
        status = HBAM_ESEQFORMAT;
      } else {
        keep = 1;
      }
    }
  }
  c.status[k] = status;
  c.flags[k] = flags;
  c.present[k] = present;
  c.keep[k] = keep;
  if (!keep) c.len[k] = c.len[(uint64_t)ncand + k] = c.len[2ull * ncand + k] = 0;
}

// lowLevelQseqRead + next()'s post-processing over line k of nl (a sentinel behind them when the
// window ends before the file).  tabmap64: the shifted tab bitmap as 64-bit words.
__global__ __launch_bounds__(VCF_WG) void k_qs_fields(const uint8_t* __restrict__ text,
                                                      const uint64_t* __restrict__ tabmap64, uint32_t shift,
                                                      const uint32_t* __restrict__ starts, uint32_t total, uint32_t nl,
                                                      uint32_t wlen, uint32_t ncand, uint32_t hi, uint32_t filter,
                                                      uint32_t illumina, FragCand c, uint32_t* nbelow) {
  const uint32_t k = blockIdx.x * VCF_WG + threadIdx.x;
  if (k >= ncand) return;
  const uint32_t rstart = k < total ? starts[k] : wlen;
  const uint32_t after = k + 1 < total ? starts[k + 1] : wlen;
  if (rstart < hi && (k + 1 == ncand || after >= hi)) *nbelow = k + 1;
  int32_t status = HBAM_OK;
  uint32_t flags = 0, present = 0, keep = 0, err = rstart, klen = 0, slen = 0, qlen = 0;
  uint32_t src[3] = {0, 0, 0};
  int32_t ints[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t strs[6] = {0, 0, 0, 0, 0, 0};
  if (k >= nl) {
    status = HBAM_EMORE;  // the line runs behind the window
  } else {
    const SeqLine a = seq_line(text, starts, k, total, wlen);
    const uint8_t* const l = text + a.s;
    const uint32_t len = a.content;
    if (a.consumed >= QS_MAX_LINE) {
      status = HBAM_ERUNTIME;  // "found abnormally large line"
    } else {
      // the first 11 tabs inside the line
      uint32_t tab[11];
      uint32_t nt = 0;
      {
        const uint32_t p = a.s + shift, pe = p + len;
        uint32_t word = p >> 6;
        uint64_t bits = tabmap64[word] & (~0ull << (p & 63u));
        while (nt < 11) {
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
      // setFieldPositionsAndLengths: the loop ends when pos reaches the line's length, so a field
      // that would begin there (an empty line's only field, the one after a trailing tab) is not counted
      const uint32_t nfields = len == 0 ? 0u : min(11u, nt + (l[len - 1] == '\t' ? 0u : 1u));
      if (nfields != 11) {
        status = HBAM_ESEQFORMAT;
        err = after - len;  // this.pos - line.getLength()
      } else {
        const uint32_t f10 = tab[9] + 1u;
        auto fpos = [&](uint32_t f) { return f ? tab[f - 1] + 1u : 0u; };
        auto flen = [&](uint32_t f) { return (f < 10 ? tab[f] : (nt > 10 ? tab[10] : len)) - fpos(f); };
        const bool hib = seq_high_byte(l, tab[7]);
        bool numerr = false;
#pragma unroll
        for (uint32_t j = 0; j < 6; ++j) {  // run lane tile xpos ypos read <- fields 1 2 3 4 5 7
          const uint32_t f = j < 5 ? j + 1 : 7;
          numerr |= !vcf_parse_int(l + fpos(f), flen(f), &ints[j]);
        }
        if (hib) {
          status = HBAM_EUNSUPPORTED;  // Text.decode of fields 0-7 is not restated
        } else if (numerr) {
          status = HBAM_ENUMBER;
        } else {
          ints[6] = l[f10] != '0';
          present = FP_INSTRUMENT | FP_RUN | FP_LANE | FP_TILE | FP_XPOS | FP_YPOS | FP_READ | FP_FILTER;
          strs[0] = a.s;
          strs[1] = flen(0);
          if (!(flen(6) > 0 && l[fpos(6)] == '0')) {
            present |= FP_INDEX;
            strs[4] = a.s + fpos(6);
            strs[5] = flen(6);
          }
          klen = tab[5] + 1u + flen(7);
          slen = flen(8);
          qlen = flen(9);
          src[0] = a.s;
          src[1] = a.s + fpos(8);
          src[2] = a.s + fpos(9);
          // the read number's source, for k_qs_keys: strs[2..3] are free (QSEQ has no flowcell)
          strs[2] = a.s + fpos(7);
          strs[3] = 0;
          if (filter && ints[6] == 0) {
            flags |= FC_DROP;
          } else if (!frag_qual_ok(text + src[2], qlen, illumina)) {
            status = HBAM_ESEQFORMAT;
          } else {
            keep = 1;
          }
        }
      }
    }
  }
  if (!keep) klen = slen = qlen = 0;
  c.rstart[k] = rstart;
  c.pos_after[k] = after;
  c.err_pos[k] = err;
  c.status[k] = status;
  c.flags[k] = flags;
  c.present[k] = present;
  c.keep[k] = keep;
#pragma unroll
  for (uint32_t j = 0; j < 8; ++j) c.ints[8ull * k + j] = ints[j];
#pragma unroll
  for (uint32_t j = 0; j < 6; ++j) c.strs[6ull * k + j] = strs[j];
#pragma unroll
  for (uint32_t j = 0; j < 3; ++j) c.src[3ull * k + j] = src[j];
  c.len[k] = klen;
  c.len[(uint64_t)ncand + k] = slen;
  c.len[2ull * ncand + k] = qlen;
}

// next() tests pos >= end once per call, and its filter loop reads on after a dropped record without
// testing: the reader reads records [0, g] where g = the first record at or after nbelow - 1 that the
// filter does not drop.  first_err = the first record with a status.
__global__ __launch_bounds__(VCF_WG) void k_frag_select(uint32_t ncand, uint32_t nbelow, FragCand c, uint32_t* g,
                                                        uint32_t* first_err) {
  const uint32_t k = blockIdx.x * VCF_WG + threadIdx.x;
  if (k >= ncand) return;
  if (c.status[k] != HBAM_OK) atomicMin(first_err, k);
  if (k + 1 >= nbelow && !(c.flags[k] & FC_DROP)) atomicMin(g, k);
}

// candidates [0, nproc) -> the kept records' columns at their rank; the pools' offsets and sources
__global__ __launch_bounds__(VCF_WG) void k_frag_emit(uint32_t nproc, uint32_t ncand, uint64_t n, uint64_t text_base,
                                                      FragCand c, const uint64_t* __restrict__ rank,
                                                      const uint64_t* __restrict__ koff,
                                                      const uint64_t* __restrict__ soff,
                                                      const uint64_t* __restrict__ qoff, FragOut o) {
  const uint32_t k = blockIdx.x * VCF_WG + threadIdx.x;
  if (k == 0) {
    o.off[0][n] = koff[nproc];
    o.off[1][n] = soff[nproc];
    o.off[2][n] = qoff[nproc];
  }
  if (k >= nproc || !c.keep[k]) return;
  const uint64_t r = rank[k];
  o.rec_off[r] = text_base + c.rstart[k];
  o.pos_after[r] = text_base + c.pos_after[k];
  o.present[r] = c.present[k];
#pragma unroll
  for (uint32_t j = 0; j < 8; ++j) o.ints[j][r] = c.ints[8ull * k + j];
#pragma unroll
  for (uint32_t j = 0; j < 3; ++j) {
    o.strs[j][2 * r] = c.strs[6ull * k + 2 * j];
    o.strs[j][2 * r + 1] = c.strs[6ull * k + 2 * j + 1];
    o.src[j][r] = c.src[3ull * k + j];
  }
  o.off[0][r] = koff[k];
  o.off[1][r] = soff[k];
  o.off[2][r] = qoff[k];
}

// scanQseqLine's key: fields 0-5 with their tabs as ':', then ':' and field 7
__global__ __launch_bounds__(VCF_WG) void k_qs_keys(const uint8_t* __restrict__ text, uint64_t n,
                                                    const uint64_t* __restrict__ ksrc,
                                                    const uint32_t* __restrict__ flow,
                                                    const uint64_t* __restrict__ koff, uint8_t* __restrict__ out) {
  const uint64_t r = (uint64_t)blockIdx.x * VCF_WG + threadIdx.x;
  if (r >= n) return;
  const uint8_t* const l = text + ksrc[r];
  const uint8_t* const rd = text + flow[2 * r];
  uint8_t* const d = out + koff[r];
  const uint32_t len = (uint32_t)(koff[r + 1] - koff[r]);
  uint32_t i = 0, tabs = 0;
  for (; i < len; ++i) {  // fields 0-5 end at the 6th tab
    const uint8_t b = l[i];
    if (b == '\t' && ++tabs == 6) break;
    d[i] = b == '\t' ? ':' : b;
  }
  if (i < len) d[i++] = ':';
  for (uint32_t j = 0; i < len; ++i, ++j) d[i] = rd[j];
}

// Phred+64 -> Phred+33 over the quality pool (convertQuality: byte - 31)
__global__ __launch_bounds__(VCF_WG) void k_frag_qual(uint8_t* __restrict__ q, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * VCF_WG + threadIdx.x;
  if (i < n) q[i] = (uint8_t)(q[i] - 31u);
}
// '.' -> 'N' over the sequence pool (postProcessSequencedFragment)
__global__ __launch_bounds__(VCF_WG) void k_frag_dots(uint8_t* __restrict__ s, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * VCF_WG + threadIdx.x;
  if (i < n && s[i] == '.') s[i] = 'N';
}

}  // namespace hbam

namespace {

int frag_cand(hbam_ctx* c, uint64_t n, FragCand* k) {
  uint32_t* base;
  const uint64_t m = (n + 4) & ~3ull;
  int rc = ensure(c, B_FQ_CAND, m * 27, &base);
  if (rc) return rc;
  k->rstart = base;
  k->pos_after = base + m;
  k->err_pos = base + 2 * m;
  k->status = (int32_t*)(base + 3 * m);
  k->flags = base + 4 * m;
  k->present = base + 5 * m;
  k->keep = base + 6 * m;
  k->ints = (int32_t*)(base + 7 * m);
  k->strs = base + 15 * m;
  k->src = base + 21 * m;
  k->len = base + 24 * m;  // 3 arrays of n (n <= m)
  return HBAM_OK;
}

int frag_out(hbam_ctx* c, uint64_t n, FragOut* o) {
  uint8_t* base;
  const uint64_t m = (n + 4) & ~3ull;  // n + 1 entries fit; every array stays 16-byte aligned
  // u64: rec_off pos_after off[3] src[3] = 8; u32: present ints[8] strs[3] x 2 = 15
  int rc = ensure(c, B_FQ_OUT, m * (8 * 8 + 15 * 4), &base);
  if (rc) return rc;
  uint64_t* q = (uint64_t*)base;
  o->rec_off = q;
  o->pos_after = q + m;
  for (int j = 0; j < 3; ++j) {
    o->off[j] = q + (2 + j) * m;
    o->src[j] = q + (5 + j) * m;
  }
  uint32_t* w = (uint32_t*)(q + 8 * m);
  o->present = w;
  for (int j = 0; j < 8; ++j) o->ints[j] = (int32_t*)(w + (1 + j) * m);
  for (int j = 0; j < 3; ++j) o->strs[j] = w + (9 + 2 * j) * m;
  return HBAM_OK;
}

struct FragLines : TextLines {
  uint32_t nl, at_eof;  // nl = the usable lines of `total`
};

// text_lines under LineReader's line rule, and the usable lines: before the end of the file the
// last start is an incomplete line; at it, a start at the window's end is no line
int frag_text_lines(hbam_ctx* c, const uint8_t* text, int on_device, uint64_t text_len, uint64_t q0,
                    uint32_t explicit_first, bool at_eof, bool want_tabs, FragLines* L) {
  int rc = text_lines(c, text, on_device, text_len, q0, explicit_first, true, at_eof, want_tabs, L);
  if (rc) return rc;
  L->at_eof = at_eof;
  uint32_t last = 0;
  if (L->total) HIPCHK(c, copy_sync(c, &last, L->starts + (L->total - 1), 4, hipMemcpyDeviceToHost));
  L->nl = L->total == 0 ? 0u : (at_eof ? L->total - (last >= L->wlen ? 1u : 0u) : L->total - 1u);
  return HBAM_OK;
}

int frag_start(hbam_ctx* c, uint32_t* starts, uint32_t i, uint32_t total, uint32_t wlen, uint32_t* out) {
  *out = wlen;
  if (i < total) HIPCHK(c, copy_sync(c, out, starts + i, 4, hipMemcpyDeviceToHost));
  if (*out > wlen) *out = wlen;
  return HBAM_OK;
}

// select + scans + compaction + pools, shared by the two formats.  cand: ncand candidates with their
// status / flags / keep / lengths final; nbelow = those starting below the split's end.
int frag_finish(hbam_ctx* c, const FragLines& L, const FragCand& cand, uint32_t ncand, uint32_t nbelow,
                uint64_t text_base, uint64_t first_pos, bool qseq, bool illumina, hbam_frag_columns* out) {
  int rc;
  uint32_t* small;
  if ((rc = ensure(c, B_FQ_SMALL, 8, &small))) return rc;
  uint32_t nproc = 0;
  int32_t status = HBAM_OK;
  uint64_t err_pos = 0, end_pos = first_pos;
  if (ncand && nbelow) {
    HIPCHK(c, hipMemsetAsync(small, 0xff, 8, c->stream));
    k_frag_select<<<grid_for(ncand, VCF_WG), VCF_WG, 0, c->stream>>>(ncand, nbelow, cand, small, small + 1);
    HIPCHK(c, hipGetLastError());
    uint32_t h[2];
    HIPCHK(c, copy_sync(c, h, small, 8, hipMemcpyDeviceToHost));
    const uint32_t nread = h[0] == FRAG_NONE ? ncand : h[0] + 1u;
    nproc = nread;
    if (h[1] < nread) {
      nproc = h[1];
      uint32_t ep;
      HIPCHK(c, copy_sync(c, &status, cand.status + nproc, 4, hipMemcpyDeviceToHost));
      HIPCHK(c, copy_sync(c, &ep, cand.err_pos + nproc, 4, hipMemcpyDeviceToHost));
      err_pos = end_pos = text_base + ep;
    } else {
      uint32_t pa;
      HIPCHK(c, copy_sync(c, &pa, cand.pos_after + (nread - 1), 4, hipMemcpyDeviceToHost));
      end_pos = text_base + pa;
    }
  }
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  uint64_t *rank, *off[3];
  const uint64_t nc1 = (uint64_t)ncand + 1;
  uint64_t* scans;
  if ((rc = ensure(c, B_FQ_SCAN, 4 * nc1 + 4, &scans))) return rc;
  rank = scans;
  uint64_t n = 0, tot[3] = {0, 0, 0};
  if (nproc) {
    // (scans over the read records only: the arrays behind nproc are not looked at)
    if ((rc = scan_exclusive<uint32_t>(c, cand.keep, nproc, rank, &n))) return rc;
    for (int j = 0; j < 3; ++j) {
      off[j] = scans + (1 + j) * nc1;
      if ((rc = scan_exclusive<uint32_t>(c, cand.len + (uint64_t)j * ncand, nproc, off[j], &tot[j]))) return rc;
    }
  }
  FragOut o;
  uint8_t* pool[3];
  if ((rc = frag_out(c, n, &o)) || (rc = ensure(c, B_FQ_KEY, tot[0] + 16, &pool[0])) ||
      (rc = ensure(c, B_FQ_SEQ, tot[1] + 16, &pool[1])) || (rc = ensure(c, B_FQ_QUAL, tot[2] + 16, &pool[2])))
    return rc;
  if (nproc) {
    k_frag_emit<<<grid_for(nproc, VCF_WG), VCF_WG, 0, c->stream>>>(nproc, ncand, n, text_base, cand, rank, off[0],
                                                                    off[1], off[2], o);
  } else {
    HIPCHK(c, hipMemsetAsync(o.off[0], 0, 8, c->stream));
    HIPCHK(c, hipMemsetAsync(o.off[1], 0, 8, c->stream));
    HIPCHK(c, hipMemsetAsync(o.off[2], 0, 8, c->stream));
  }
  HIPCHK(c, hipGetLastError());
  if (n) {
    const uint32_t gw = (uint32_t)std::min<uint64_t>((n + 255) / 256, POOLS_MAX_WG);
    for (int j = qseq ? 1 : 0; j < 3; ++j)
      k_gather_records_tile<<<gw, 256, 0, c->stream>>>(L.d, o.src[j], nullptr, n, o.off[j], pool[j]);
    if (qseq) {
      k_qs_keys<<<grid_for(n, VCF_WG), VCF_WG, 0, c->stream>>>(L.d, n, o.src[0], o.strs[1], o.off[0], pool[0]);
      if (tot[1]) k_frag_dots<<<grid_for(tot[1], VCF_WG), VCF_WG, 0, c->stream>>>(pool[1], tot[1]);
    }
    if (illumina && tot[2]) k_frag_qual<<<grid_for(tot[2], VCF_WG), VCF_WG, 0, c->stream>>>(pool[2], tot[2]);
    HIPCHK(c, hipGetLastError());
    // QSEQ has no flowcell: the slot carried the read number's source for k_qs_keys
    if (qseq) HIPCHK(c, hipMemsetAsync(o.strs[1], 0, 8 * n, c->stream));
  }
  HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  out->n = n;
  out->status = status;
  out->err_pos = err_pos;
  out->first_pos = first_pos;
  out->end_pos = end_pos;
  out->rec_off = o.rec_off;
  out->pos_after = o.pos_after;
  out->present = o.present;
  out->run = o.ints[0];
  out->lane = o.ints[1];
  out->tile = o.ints[2];
  out->xpos = o.ints[3];
  out->ypos = o.ints[4];
  out->read = o.ints[5];
  out->filter_passed = o.ints[6];
  out->control = o.ints[7];
  out->instrument = o.strs[0];
  out->flowcell = o.strs[1];
  out->index = o.strs[2];
  out->key_off = o.off[0];
  out->seq_off = o.off[1];
  out->qual_off = o.off[2];
  out->key = pool[0];
  out->seq = pool[1];
  out->qual = pool[2];
  out->key_len = tot[0];
  out->seq_len = tot[1];
  out->qual_len = tot[2];
  out->text_base = text_base;
  c->timing.scan_ms = ev_ms(c, 0, 1);
  c->timing.walk_ms = ev_ms(c, 1, 2);
  c->timing.decode_ms = ev_ms(c, 2, 3);
  c->timing.pools_ms = ev_ms(c, 3, 4);
  c->timing.total_ms = ev_ms(c, 0, 4);
  c->timing.ubuf_bytes = L.wlen;
  c->timing.n_records = n;
  c->timing.pool_bytes = tot[0] + tot[1] + tot[2];
  return HBAM_OK;
}

// a call that ends before any record is read: status and positions only, every pool empty
int frag_nothing(hbam_ctx* c, const FragLines& L, uint64_t text_base, uint64_t first_pos, int32_t status,
                 hbam_frag_columns* out) {
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  FragCand none{};
  int rc = frag_finish(c, L, none, 0, 0, text_base, first_pos, false, false, out);
  out->status = status;
  out->err_pos = status != HBAM_OK ? first_pos : 0;
  return rc;
}

int frag_check_args(hbam_ctx* c, const uint8_t* text, uint64_t text_base, uint64_t text_len, uint64_t file_len,
                    uint64_t start, int32_t encoding, hbam_frag_columns* out) {
  if (!c || !text || !out) return HBAM_EINVAL;
  memset(out, 0, sizeof *out);
  if (text_len > VCF_MAX_WINDOW) return set_err(c, HBAM_EINVAL, "a FASTQ / QSEQ window is at most 2 GiB");
  if (text_base + text_len > file_len) return set_err(c, HBAM_EINVAL, "window past the end of the file");
  if (start > file_len) return set_err(c, HBAM_EINVAL, "the split starts past the end of the file");
  if (encoding != HBAM_QUAL_SANGER && encoding != HBAM_QUAL_ILLUMINA)
    return set_err(c, HBAM_EINVAL, "unknown base quality encoding %d", encoding);
  return HBAM_OK;
}

}  // namespace

extern "C" int hbam_fastq_decode_split(hbam_ctx* c, const uint8_t* text, int on_device, uint64_t text_base,
                                       uint64_t text_len, uint64_t file_len, uint64_t start, uint64_t length,
                                       int32_t encoding, int32_t filter_failed_qc, hbam_frag_columns* out) {
  int rc = frag_check_args(c, text, text_base, text_len, file_len, start, encoding, out);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  // the lines are counted from byte `start` itself (:165-166), for start == 0 from the file's first
  if (text_base > start) return set_err(c, HBAM_EINVAL, "the window starts after the reader's first byte");
  const uint64_t q0 = std::min(start - text_base, text_len);
  const bool at_eof = text_base + text_len == file_len;
  const uint64_t end_abs = length > ~0ull - start ? ~0ull : start + length;
  c->timing = hbam_timing{};
  FragLines L;
  if ((rc = frag_text_lines(c, text, on_device, text_len, q0, 1, at_eof, false, &L))) return rc;
  uint32_t r0 = 0;
  uint64_t first_pos = start;
  const uint64_t hi64 = end_abs > text_base ? end_abs - text_base : 0;
  const uint32_t hi = (uint32_t)std::min<uint64_t>(hi64, 0xffffffffull);
  if (start > 0) {
    uint64_t* stop_d;
    if ((rc = ensure(c, B_FQ_STOP, 2, &stop_d))) return rc;
    HIPCHK(c, hipMemsetAsync(stop_d, 0xff, 8, c->stream));
    if (L.total)
      k_fq_stop<<<grid_for(L.total, VCF_WG), VCF_WG, 0, c->stream>>>(L.d, L.starts, L.total, L.nl, L.wlen, L.at_eof, hi,
                                                                    (unsigned long long*)stop_d);
    HIPCHK(c, hipGetLastError());
    uint64_t stop;
    HIPCHK(c, copy_sync(c, &stop, stop_d, 8, hipMemcpyDeviceToHost));
    const bool none = stop == ~0ull;
    const uint32_t j = (uint32_t)(stop >> 2), kind = none ? 3u : (uint32_t)(stop & 3u);
    if (kind == 2) return frag_nothing(c, L, text_base, start, HBAM_EMORE, out);
    // no exit among the lines below the split's end: the walk ends at the end of the file
    if (none) return frag_nothing(c, L, text_base, file_len, HBAM_OK, out);
    uint32_t s_r0;
    r0 = kind == 0 ? j : j + 1;
    if ((rc = frag_start(c, L.starts, r0, L.nl, L.wlen, &s_r0))) return rc;
    first_pos = text_base + s_r0;
  }
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  const uint32_t lines = L.nl > r0 ? L.nl - r0 : 0u;
  const uint32_t ncand = at_eof ? (lines + 3) / 4 : lines / 4 + 1;
  FragCand cand{};
  uint32_t* small;
  if ((rc = frag_cand(c, ncand, &cand)) || (rc = ensure(c, B_FQ_SMALL2, 4, &small))) return rc;
  uint32_t nbelow = 0;
  if (ncand) {
    HIPCHK(c, hipMemsetAsync(small, 0xff, 4, c->stream));
    HIPCHK(c, hipMemsetAsync(small + 1, 0, 4, c->stream));
    k_fq_frame<<<grid_for(ncand, VCF_WG), VCF_WG, 0, c->stream>>>(L.d, L.starts, L.total, L.nl, L.wlen, L.at_eof, r0,
                                                                  ncand, hi, cand, small, small + 1);
    HIPCHK(c, hipGetLastError());
    uint32_t h[2];
    HIPCHK(c, copy_sync(c, h, small, 8, hipMemcpyDeviceToHost));
    nbelow = h[1];
    k_fq_resolve<<<grid_for(ncand, VCF_WG), VCF_WG, 0, c->stream>>>(L.d, ncand, h[0], filter_failed_qc ? 1u : 0u,
                                                                    encoding == HBAM_QUAL_ILLUMINA ? 1u : 0u, cand);
    HIPCHK(c, hipGetLastError());
  }
  return frag_finish(c, L, cand, ncand, nbelow, text_base, first_pos, false, encoding == HBAM_QUAL_ILLUMINA, out);
}

extern "C" int hbam_qseq_decode_split(hbam_ctx* c, const uint8_t* text, int on_device, uint64_t text_base,
                                      uint64_t text_len, uint64_t file_len, uint64_t start, uint64_t length,
                                      int32_t encoding, int32_t filter_failed_qc, hbam_frag_columns* out) {
  int rc = frag_check_args(c, text, text_base, text_len, file_len, start, encoding, out);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  // start > 0: the reader opens at start - 1 and drops the line it reads there (:147-152)
  const uint64_t open_abs = start ? start - 1 : 0;
  if (text_base > open_abs) return set_err(c, HBAM_EINVAL, "the window starts after the reader's first byte");
  const uint64_t q0 = std::min(open_abs - text_base, text_len);
  const bool at_eof = text_base + text_len == file_len;
  const uint64_t end_abs = length > ~0ull - start ? ~0ull : start + length;
  c->timing = hbam_timing{};
  FragLines L;
  if ((rc = frag_text_lines(c, text, on_device, text_len, q0, start == 0 ? 1u : 0u, at_eof, true, &L))) return rc;
  uint64_t first_pos = 0;
  if (start > 0) {
    if (L.total == 0 && !at_eof) return frag_nothing(c, L, text_base, start, HBAM_EMORE, out);
    uint32_t s0;
    if ((rc = frag_start(c, L.starts, 0, L.total, L.wlen, &s0))) return rc;
    first_pos = text_base + s0;
  }
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  const uint32_t ncand = at_eof ? L.nl : L.nl + 1;  // (!at_eof: total >= 1 here, the sentinel is line total - 1)
  const uint64_t hi64 = end_abs > text_base ? end_abs - text_base : 0;
  const uint32_t hi = (uint32_t)std::min<uint64_t>(hi64, 0xffffffffull);
  FragCand cand{};
  uint32_t* small;
  if ((rc = frag_cand(c, ncand, &cand)) || (rc = ensure(c, B_FQ_SMALL2, 4, &small))) return rc;
  uint32_t nbelow = 0;
  if (ncand) {
    HIPCHK(c, hipMemsetAsync(small, 0, 8, c->stream));
    k_qs_fields<<<grid_for(ncand, VCF_WG), VCF_WG, 0, c->stream>>>(
        L.d, (const uint64_t*)L.tabmap, L.shift, L.starts, L.total, L.nl, L.wlen, ncand, hi, filter_failed_qc ? 1u : 0u,
        encoding == HBAM_QUAL_ILLUMINA ? 1u : 0u, cand, small);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, copy_sync(c, &nbelow, small, 4, hipMemcpyDeviceToHost));
  }
  return frag_finish(c, L, cand, ncand, nbelow, text_base, first_pos, true, encoding == HBAM_QUAL_ILLUMINA, out);
}

extern "C" int hbam_frag_columns_to_host(hbam_ctx* c, const hbam_frag_columns* dv, hbam_frag_columns* h) {
  if (!c || !dv || !h || dv->host) return HBAM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  *h = *dv;
  h->host = 1;
  const uint64_t n = dv->n, m = n + 1;
  // one allocation, rec_off first: hbam_frag_release frees it through that pointer
  const uint64_t bytes = 8 * (2 * n + 3 * m) + 4 * (15 * n) + dv->key_len + dv->seq_len + dv->qual_len + 64;
  uint8_t* blk = (uint8_t*)malloc(bytes);
  if (!blk) {
    memset(h, 0, sizeof *h);
    return set_err(c, HBAM_ENOMEM, "hbam_frag_columns_to_host: %llu records", (unsigned long long)n);
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
  h->qual_off = (uint64_t*)take(dv->qual_off, 8 * m);
  h->present = (uint32_t*)take(dv->present, 4 * n);
  h->run = (int32_t*)take(dv->run, 4 * n);
  h->lane = (int32_t*)take(dv->lane, 4 * n);
  h->tile = (int32_t*)take(dv->tile, 4 * n);
  h->xpos = (int32_t*)take(dv->xpos, 4 * n);
  h->ypos = (int32_t*)take(dv->ypos, 4 * n);
  h->read = (int32_t*)take(dv->read, 4 * n);
  h->filter_passed = (int32_t*)take(dv->filter_passed, 4 * n);
  h->control = (int32_t*)take(dv->control, 4 * n);
  h->instrument = (uint32_t*)take(dv->instrument, 8 * n);
  h->flowcell = (uint32_t*)take(dv->flowcell, 8 * n);
  h->index = (uint32_t*)take(dv->index, 8 * n);
  h->key = (uint8_t*)take(dv->key, dv->key_len);
  h->seq = (uint8_t*)take(dv->seq, dv->seq_len);
  h->qual = (uint8_t*)take(dv->qual, dv->qual_len);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    free(blk);
    memset(h, 0, sizeof *h);
    return set_err(c, HBAM_EDEVICE, "hbam_frag_columns_to_host: %s", hipGetErrorString(e));
  }
  return HBAM_OK;
}

extern "C" void hbam_frag_release(hbam_ctx* c, hbam_frag_columns* cols) {
  (void)c;
  if (!cols) return;
  if (cols->host) free(cols->rec_off);
  memset(cols, 0, sizeof *cols);
}
