// hbam_samtext.hip — SAM text out of the device: SAMTextWriter.writeAlignment over packed BAM
// records (SAMRecordWriter, AnySAMOutputFormat's SAM half, the View plugin), the inverse of
// hbam_sam.hip.  Included at the end of hbam_capi.hip, after hbam_sam.hip.  gfx950, wave64.
//
//   k_samtext_sizes    a lane per output line: the record rendered by sam_text (sam_text.h) in its
//                      counting mode for the line's length, its status, whether the host has to
//                      render it (a float outside the device's domain, an H tag) and the SEQ / QUAL
//                      descriptor of the bulk pass.  SEQ and QUAL are not read but for the first
//                      quality byte; the other bytes come through the 16-byte register cache
//                      (SamRecBytes), since a lane per record pays a cache line per lane for every
//                      load instruction whatever its width.
//   (scan_exclusive)   lengths -> line_off; deferred flags -> their ranks, k_samtext_deferred
//                      compacts the deferred output positions, ascending
//   k_samtext_head     a lane per line: the same sam_text with an output pointer writes fields 1-9
//                      and the tags at line_off, four bytes per store (SamOut)
//   k_samtext_bulk     SEQ \t QUAL, about two thirds of the text, the way k_sam_bulk moves it the
//                      other way: a wave takes a tile of 64 lines, cuts each line's region into
//                      16-byte units aligned in the OUTPUT, numbers the units with a wave scan and
//                      gives them to consecutive lanes, so a wave store covers 1 KiB of consecutive
//                      text and a 6 KB long read is the whole wave's work.  A unit's bytes come from
//                      the packed nibbles or from the quality bytes + 33; the units at a region's
//                      ends are partial.  A quality byte above 93 stops the output at that line.
//
// Loads past a record stay inside the 64 readable bytes behind the records (include/hbam.h).

#include "sam_text.h"

namespace hbam {

constexpr uint32_t SAMTEXT_WG = 256;

// desc[k] = (l_seq | QUAL-is-"*" << 31, line-relative offset of SEQ \t QUAL, ubuf offset of the
// packed SEQ lo, hi); the offset is SAMTEXT_NONE for a line without bulk bytes and SAMTEXT_CHECK for
// a deferred record, whose units are formed for their quality check and not stored
constexpr uint32_t SAMTEXT_NONE = 0xffffffffu, SAMTEXT_CHECK = 0xfffffffeu;
__global__ __launch_bounds__(SAMTEXT_WG) void k_samtext_sizes(const uint8_t* __restrict__ ub,
                                                              const uint64_t* __restrict__ rec_off,
                                                              const uint32_t* __restrict__ perm, uint32_t n,
                                                              const uint8_t* __restrict__ names,
                                                              const uint32_t* __restrict__ name_off, int32_t n_ref,
                                                              uint32_t* __restrict__ len, int32_t* __restrict__ status,
                                                              uint32_t* __restrict__ dflag, uint4* __restrict__ desc,
                                                              unsigned long long* first_stop) {
  const uint32_t k = blockIdx.x * SAMTEXT_WG + threadIdx.x;
  if (k >= n) return;
  const uint32_t i = perm ? perm[k] : k;
  const uint64_t ro = rec_off[i];
  SamTextRec r;
  sam_text(ub + ro, rec_off[i + 1] - ro, names, name_off, n_ref, nullptr, &r);
  len[k] = r.len;
  status[k] = r.status;
  dflag[k] = r.deferred;
  const uint64_t s = ro + r.seq_in;
  const uint32_t where = r.bulk_len == 0 ? SAMTEXT_NONE : r.deferred ? SAMTEXT_CHECK : r.bulk_out;
  desc[k] = make_uint4(r.l_seq | r.qual_star << 31, where, (uint32_t)s, (uint32_t)(s >> 32));
  if (r.status != HBAM_OK) atomicMin(first_stop, (unsigned long long)k);
}

__global__ __launch_bounds__(SAMTEXT_WG) void k_samtext_deferred(const uint32_t* __restrict__ dflag,
                                                                 const uint64_t* __restrict__ dpos, uint32_t n,
                                                                 uint32_t* __restrict__ deferred) {
  const uint32_t k = blockIdx.x * SAMTEXT_WG + threadIdx.x;
  if (k < n && dflag[k]) deferred[dpos[k]] = k;
}

__global__ __launch_bounds__(SAMTEXT_WG) void k_samtext_head(const uint8_t* __restrict__ ub,
                                                             const uint64_t* __restrict__ rec_off,
                                                             const uint32_t* __restrict__ perm, uint32_t n,
                                                             const uint8_t* __restrict__ names,
                                                             const uint32_t* __restrict__ name_off, int32_t n_ref,
                                                             const uint64_t* __restrict__ line_off,
                                                             uint8_t* __restrict__ text) {
  const uint32_t k = blockIdx.x * SAMTEXT_WG + threadIdx.x;
  if (k >= n) return;
  const uint64_t lo = line_off[k];
  if (line_off[k + 1] == lo) return;  // deferred
  const uint32_t i = perm ? perm[k] : k;
  const uint64_t ro = rec_off[i];
  SamTextRec r;
  sam_text(ub + ro, rec_off[i + 1] - ro, names, name_off, n_ref, text + lo, &r);
}

__global__ __launch_bounds__(SAMTEXT_WG) void k_samtext_bulk(const uint8_t* __restrict__ ub,
                                                             const uint4* __restrict__ desc,
                                                             const uint64_t* __restrict__ line_off, uint32_t n,
                                                             uint8_t* __restrict__ text, int32_t* __restrict__ status,
                                                             unsigned long long* first_stop) {
  __shared__ uint32_t s_excl[SAMTEXT_WG / 64][64];
  __shared__ uint4 s_desc[SAMTEXT_WG / 64][64];
  __shared__ uint2 s_reg[SAMTEXT_WG / 64][64];
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t* const ex = s_excl[threadIdx.x >> 6];
  uint4* const sd = s_desc[threadIdx.x >> 6];
  uint2* const sr = s_reg[threadIdx.x >> 6];
  const uint32_t ntiles = (n + 63u) / 64u;
  const uint32_t wstride = gridDim.x * (SAMTEXT_WG / 64);
  for (uint32_t t = blockIdx.x * (SAMTEXT_WG / 64) + (threadIdx.x >> 6); t < ntiles; t += wstride) {
    const uint32_t line = t * 64u + lane;
    uint4 d = make_uint4(0, SAMTEXT_NONE, 0, 0);
    uint64_t R = 0;
    uint32_t blen = 0;
    if (line < n) {
      d = desc[line];
      if (d.y != SAMTEXT_NONE) {
        const uint32_t ls = d.x & 0x7fffffffu;
        R = d.y == SAMTEXT_CHECK ? 0 : line_off[line] + d.y;
        blen = ls + 1u + ((d.x >> 31) ? 1u : ls);
      }
    }
    const uint32_t units = sam_text_units(R, blen);
    const uint32_t incl = wave_scan_dpp(units), T = wave_last(incl);
    if (T == 0u) continue;  // wave-uniform
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");  // the previous tile's reads of ex / sd / sr precede these writes
    ex[lane] = incl - units;
    sd[lane] = d;
    sr[lane] = make_uint2((uint32_t)R, (uint32_t)(R >> 32));
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
      const uint2 RR = sr[r];
      const uint64_t Rr = (uint64_t)RR.x | (uint64_t)RR.y << 32;
      const uint32_t ls = D.x & 0x7fffffffu, star = D.x >> 31;
      uint32_t p0, nb, o[4];
      sam_text_unit_span(Rr, ls + 1u + (star ? 1u : ls), q - ex[r], &p0, &nb);
      const bool ok = sam_text_unit(ub + ((uint64_t)D.z | (uint64_t)D.w << 32), ls, star, p0, nb, o);
      const u32x4_a1 v = u32x4_a1{o[0], o[1], o[2], o[3]};
      HBAM_G uint8_t* const gd = (HBAM_G uint8_t*)(text + Rr + p0);
      if (D.y != SAMTEXT_CHECK) {
        if (nb >= 16u) *(HBAM_G u32x4_a1*)gd = v;
        else st_part_g(gd, nb, v);
      }
      if (!ok) {
        const uint32_t bad = t * 64u + r;
        status[bad] = HBAM_EREFID;
        atomicMin(first_stop, (unsigned long long)bad);
      }
    }
  }
}

}  // namespace hbam

extern "C" int hbam_sam_render(hbam_ctx* c, const uint8_t* ubuf, const uint64_t* rec_off, const uint32_t* perm,
                               uint64_t n, int on_device, const uint8_t* names, const uint32_t* name_off,
                               int32_t n_ref, hbam_sam_text* out) {
  if (!c || !out || n_ref < 0 || !name_off || (n && (!ubuf || !rec_off))) return HBAM_EINVAL;
  memset(out, 0, sizeof *out);
  HIPCHK(c, hipSetDevice(c->device));
  if (n >= 0xffffffffull) return set_err(c, HBAM_EINVAL, "hbam_sam_render: at most 2^32 - 2 lines a call");
  if (!on_device && perm) return set_err(c, HBAM_EINVAL, "hbam_sam_render: perm needs device arguments");
  for (int32_t k = 0; k < n_ref; ++k)
    if (name_off[k + 1] < name_off[k]) return set_err(c, HBAM_EINVAL, "hbam_sam_render: name_off must ascend");
  const uint64_t names_len = name_off[n_ref];
  if (names_len && !names) return HBAM_EINVAL;
  c->timing = hbam_timing{};
  int rc;
  uint8_t* dnames;
  uint32_t* dname_off;
  if ((rc = ensure(c, B_ST_NAMES, names_len + 1, &dnames)) ||
      (rc = ensure(c, B_ST_NAMEOFF, (uint64_t)n_ref + 1, &dname_off)))
    return rc;
  if (names_len) HIPCHK(c, hipMemcpyAsync(dnames, names, names_len, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dname_off, name_off, ((size_t)n_ref + 1) * 4, hipMemcpyHostToDevice, c->stream));
  const uint8_t* ub = ubuf;
  const uint64_t* ro = rec_off;
  if (!on_device && n) {
    for (uint64_t i = 0; i < n; ++i)
      if (rec_off[i + 1] < rec_off[i]) return set_err(c, HBAM_EINVAL, "hbam_sam_render: rec_off must ascend");
    const uint64_t bytes = rec_off[n];
    uint8_t* dub;
    uint64_t* dro;
    if ((rc = ensure(c, B_ST_UBUF, bytes + 64, &dub)) || (rc = ensure(c, B_ST_RECOFF, n + 1, &dro))) return rc;
    if (bytes) HIPCHK(c, hipMemcpyAsync(dub, ubuf, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(dub + bytes, 0, 64, c->stream));
    HIPCHK(c, hipMemcpyAsync(dro, rec_off, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    ub = dub;
    ro = dro;
  }
  uint32_t *len, *dflag, *deferred;
  int32_t* lstatus;
  uint4* desc;
  uint64_t *line_off, *dpos, *small;
  if ((rc = ensure(c, B_ST_LEN, n + 1, &len)) || (rc = ensure(c, B_ST_STATUS, n + 1, &lstatus)) ||
      (rc = ensure(c, B_ST_DFLAG, n + 1, &dflag)) || (rc = ensure(c, B_ST_DESC, n + 1, &desc)) ||
      (rc = ensure(c, B_ST_LINEOFF, n + 1, &line_off)) || (rc = ensure(c, B_ST_DPOS, n + 1, &dpos)) ||
      (rc = ensure(c, B_ST_DEFERRED, n + 1, &deferred)) || (rc = ensure(c, B_ST_SMALL, 2, &small)))
    return rc;
  unsigned long long* first_stop = (unsigned long long*)small;
  HIPCHK(c, hipMemsetAsync(small, 0xff, 8, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  if (n)
    k_samtext_sizes<<<grid_for(n, SAMTEXT_WG), SAMTEXT_WG, 0, c->stream>>>(ub, ro, perm, (uint32_t)n, dnames,
                                                                          dname_off, n_ref, len, lstatus, dflag,
                                                                          desc, first_stop);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->pinned_small + 8, small, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  uint64_t m = n;  // the lines that stand
  int32_t status = HBAM_OK;
  if (c->pinned_small[8] < n) {
    m = c->pinned_small[8];
    HIPCHK(c, copy_sync(c, &status, lstatus + m, 4, hipMemcpyDeviceToHost));
  }
  uint64_t text_len = 0, n_def = 0;
  if ((rc = scan_exclusive<uint32_t>(c, len, m, line_off, &text_len))) return rc;
  if ((rc = scan_exclusive<uint32_t>(c, dflag, m, dpos, &n_def))) return rc;
  if (m) k_samtext_deferred<<<grid_for(m, SAMTEXT_WG), SAMTEXT_WG, 0, c->stream>>>(dflag, dpos, (uint32_t)m, deferred);
  HIPCHK(c, hipGetLastError());
  uint8_t* text;
  if ((rc = ensure(c, B_ST_TEXT, text_len + 64, &text))) return rc;
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  if (m)
    k_samtext_head<<<grid_for(m, SAMTEXT_WG), SAMTEXT_WG, 0, c->stream>>>(ub, ro, perm, (uint32_t)m, dnames,
                                                                         dname_off, n_ref, line_off, text);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  HIPCHK(c, hipMemsetAsync(small, 0xff, 8, c->stream));
  if (m)
    k_samtext_bulk<<<(uint32_t)std::min<uint64_t>(grid_for(m, SAMTEXT_WG), POOLS_MAX_WG), SAMTEXT_WG, 0,
                     c->stream>>>(ub, desc, line_off, (uint32_t)m, text, lstatus, first_stop);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  HIPCHK(c, hipMemcpyAsync(c->pinned_small + 8, small, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->pinned_small[8] < m) {  // a quality byte: the lines before that record stand
    m = c->pinned_small[8];
    HIPCHK(c, copy_sync(c, &status, lstatus + m, 4, hipMemcpyDeviceToHost));
    HIPCHK(c, copy_sync(c, &text_len, line_off + m, 8, hipMemcpyDeviceToHost));
    HIPCHK(c, copy_sync(c, &n_def, dpos + m, 8, hipMemcpyDeviceToHost));
  }
  out->n_records = m;
  out->status = status;
  out->err_record = status ? m : 0;
  out->text_len = text_len;
  out->text = text;
  out->line_off = line_off;
  out->n_deferred = n_def;
  out->deferred = deferred;
  c->timing.walk_ms = ev_ms(c, 0, 1);
  c->timing.huffman_ms = ev_ms(c, 1, 2);
  c->timing.resolve_ms = ev_ms(c, 2, 3);
  c->timing.total_ms = ev_ms(c, 0, 3);
  c->timing.n_records = m;
  c->timing.ubuf_bytes = text_len;
  return HBAM_OK;
}
