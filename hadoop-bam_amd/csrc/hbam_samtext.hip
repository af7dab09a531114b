// hbam_samtext.hip — SAM text out of the device: SAMTextWriter.writeAlignment over packed BAM
// records (SAMRecordWriter, AnySAMOutputFormat's SAM half, the View plugin), the inverse of
// hbam_sam.hip.  Included at the end of hbam_capi.hip, after hbam_sam.hip and hbam_textout.hip (the
// host sequence the three text writers share).  gfx950, wave64.
//
//   k_samtext_sizes    a lane per output line: the record rendered by sam_text (sam_text.h) in its
//                      counting mode for the line's length, its status, whether the host has to
//                      render it (a float outside the device's domain, an H tag) and the SEQ / QUAL
//                      descriptor of the bulk pass.  SEQ and QUAL are not read but for the first
//                      quality byte; the other bytes come through the 16-byte register cache
//                      (SamRecBytes), since a lane per record pays a cache line per lane for every
//                      load instruction whatever its width.
//   (textout_layout)   lengths -> line_off; deferred flags -> the deferred output positions
//   k_samtext_head     a lane per line: the same sam_text with an output pointer writes fields 1-9
//                      and the tags at line_off, four bytes per store (SamOut)
//   k_samtext_bulk     SEQ \t QUAL, about two thirds of the text, the way k_sam_bulk moves it the
//                      other way (unit_tiles.h): each line's region is cut into 16-byte units aligned
//                      in the OUTPUT.  A unit's bytes come from the packed nibbles or from the
//                      quality bytes + 33; the units at a region's ends are partial.  A quality
//                      byte above 93 stops the output at that line.
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
  __shared__ uint4 s_desc[SAMTEXT_WG / 64][64];
  __shared__ uint2 s_reg[SAMTEXT_WG / 64][64];
  uint4* const sd = s_desc[threadIdx.x >> 6];
  uint2* const sr = s_reg[threadIdx.x >> 6];
  uint4 d;
  uint64_t R;
  unit_tiles<SAMTEXT_WG>(
      n,
      [&](uint32_t line) {
        d = make_uint4(0, SAMTEXT_NONE, 0, 0);
        R = 0;
        uint32_t blen = 0;
        if (line < n) {
          d = desc[line];
          if (d.y != SAMTEXT_NONE) {
            const uint32_t ls = d.x & 0x7fffffffu;
            R = d.y == SAMTEXT_CHECK ? 0 : line_off[line] + d.y;
            blen = ls + 1u + ((d.x >> 31) ? 1u : ls);
          }
        }
        return sam_text_units(R, blen);
      },
      [&](uint32_t lane) {
        sd[lane] = d;
        sr[lane] = make_uint2((uint32_t)R, (uint32_t)(R >> 32));
      },
      [&](uint32_t t, uint32_t r, uint32_t k) {
        const uint4 D = sd[r];
        const uint2 RR = sr[r];
        const uint64_t Rr = (uint64_t)RR.x | (uint64_t)RR.y << 32;
        const uint32_t ls = D.x & 0x7fffffffu, star = D.x >> 31;
        uint32_t p0, nb, o[4];
        sam_text_unit_span(Rr, ls + 1u + (star ? 1u : ls), k, &p0, &nb);
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
      });
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
    // n + 1 offsets: k_samtext_* take a record's length from rec_off[i + 1]
    if ((rc = stage_records(c, B_ST_UBUF, B_ST_RECOFF, ubuf, rec_off[n], rec_off, n + 1, &ub, &ro))) return rc;
  }
  TextOut T{{B_ST_LEN, B_ST_STATUS, B_ST_LINEOFF, B_ST_SMALL, B_ST_TEXT, true, B_ST_DFLAG, B_ST_DPOS, B_ST_DEFERRED}};
  uint4* desc;
  if ((rc = ensure(c, B_ST_DESC, n + 1, &desc)) || (rc = textout_begin(c, n, &T))) return rc;
  if (n)
    k_samtext_sizes<<<grid_for(n, SAMTEXT_WG), SAMTEXT_WG, 0, c->stream>>>(ub, ro, perm, (uint32_t)n, dnames,
                                                                          dname_off, n_ref, T.len, T.lstatus, T.dflag,
                                                                          desc, T.first_stop);
  HIPCHK(c, hipGetLastError());
  if ((rc = textout_stop(c, &T))) return rc;
  if (T.cut) HIPCHK(c, copy_sync(c, &T.status, T.lstatus + T.m, 4, hipMemcpyDeviceToHost));
  if ((rc = textout_layout(c, &T))) return rc;
  if (T.m)
    k_samtext_head<<<grid_for(T.m, SAMTEXT_WG), SAMTEXT_WG, 0, c->stream>>>(ub, ro, perm, (uint32_t)T.m, dnames,
                                                                           dname_off, n_ref, T.line_off, T.text);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  if ((rc = textout_arm(c, T))) return rc;
  if (T.m)
    k_samtext_bulk<<<(uint32_t)std::min<uint64_t>(grid_for(T.m, SAMTEXT_WG), POOLS_MAX_WG), SAMTEXT_WG, 0,
                     c->stream>>>(ub, desc, T.line_off, (uint32_t)T.m, T.text, T.lstatus, T.first_stop);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  if ((rc = textout_stop(c, &T))) return rc;
  if (T.cut) {  // a quality byte: the lines before that record stand, and the deferred ones among them
    HIPCHK(c, copy_sync(c, &T.status, T.lstatus + T.m, 4, hipMemcpyDeviceToHost));
    HIPCHK(c, copy_sync(c, &T.text_len, T.line_off + T.m, 8, hipMemcpyDeviceToHost));
    HIPCHK(c, copy_sync(c, &T.n_def, T.dpos + T.m, 8, hipMemcpyDeviceToHost));
  }
  textout_finish(c, T, out);
  out->n_deferred = T.n_def;
  out->deferred = T.deferred;
  return HBAM_OK;
}
