// hbam_vcftext.hip — VCF text out of the device: htsjdk's VCFEncoder over BCF2 records
// (VCFRecordWriter, the VCF half of VCFSort over a BCF input), over the host sequence of
// hbam_textout.hip.  Included at the end of hbam_capi.hip.  gfx950, wave64.
//
//   k_vcftext_sizes    a lane per output line: the record rendered by vcf_text (vcf_text.h) in its
//                      counting mode for the line's length, its status and whether the host has to
//                      render it.  A record of fewer than HBAM_VCF_WAVE_SAMPLES samples is counted
//                      whole; a larger one up to INFO, with its genotype fields' headers checked.
//   k_vcftext_geno     (sizes) a wave per line, which leaves at once unless the lane pass marked the
//                      line: lanes stride the samples for the GT checks and the FORMAT key set (the
//                      lanes' findings are OR-ed through the wave), the key order is then computed
//                      once, and each lane counts its samples' columns; a wave scan of the lengths
//                      per 64 samples gives every column's offset.
//   (textout_layout)   lengths -> line_off; deferred flags -> the deferred output positions
//   k_vcftext_write    a lane per line: the same vcf_text with an output pointer, four bytes per
//                      store (SamOut); a marked line's site columns only
//   k_vcftext_geno     (write) the same wave pass with an output pointer: lane 0 writes the FORMAT
//                      column and the '\n', every lane its samples' columns at the scanned offsets
//
// Loads past a record stay inside the 64 readable bytes behind the records (include/hbam.h).

#include "vcf_text.h"

namespace hbam {

constexpr uint32_t VCFTEXT_WG = 256;
constexpr uint32_t VCFTEXT_WAVE = 0x80000000u;  // site[k]: the samples are k_vcftext_geno's

__global__ __launch_bounds__(VCFTEXT_WG) void k_vcftext_sizes(const uint8_t* __restrict__ data, uint64_t data_len,
                                                              const uint64_t* __restrict__ rec_off,
                                                              const uint32_t* __restrict__ perm, uint32_t n,
                                                              VcfMeta M, uint32_t* __restrict__ len,
                                                              int32_t* __restrict__ status,
                                                              uint32_t* __restrict__ dflag, uint32_t* __restrict__ site,
                                                              unsigned long long* first_stop) {
  const uint32_t k = blockIdx.x * VCFTEXT_WG + threadIdx.x;
  if (k >= n) return;
  const uint32_t i = perm ? perm[k] : k;
  const uint64_t ro = rec_off[i];
  VcfRec r;
  r.status = HBAM_ETRIBBLE;
  r.deferred = r.len = r.by_wave = 0;
  if (ro <= data_len) vcf_text(data + ro, data_len - ro, M, HBAM_VCF_WAVE_SAMPLES, nullptr, &r);
  status[k] = r.status;
  dflag[k] = r.deferred;
  site[k] = r.len | (r.by_wave ? VCFTEXT_WAVE : 0u);
  len[k] = r.deferred || r.by_wave ? 0u : r.len;
  if (r.status != HBAM_OK) atomicMin(first_stop, (unsigned long long)k);
}

__device__ __forceinline__ uint32_t wave_or(uint32_t x) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) x |= (uint32_t)__shfl_xor((int)x, o);
  return x;
}

// text == nullptr: the sizes pass (len, status, dflag are updated); else the write pass
__global__ __launch_bounds__(VCFTEXT_WG) void k_vcftext_geno(const uint8_t* __restrict__ data, uint64_t data_len,
                                                             const uint64_t* __restrict__ rec_off,
                                                             const uint32_t* __restrict__ perm, uint32_t n, VcfMeta M,
                                                             const uint32_t* __restrict__ site,
                                                             uint32_t* __restrict__ len, int32_t* __restrict__ status,
                                                             uint32_t* __restrict__ dflag,
                                                             const uint64_t* __restrict__ line_off,
                                                             uint8_t* __restrict__ text,
                                                             unsigned long long* first_stop) {
  const uint32_t k = blockIdx.x * (VCFTEXT_WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (k >= n) return;  // (wave-uniform, as every branch below but the ones on `lane`)
  const uint32_t sk = site[k];
  if (!(sk & VCFTEXT_WAVE)) return;
  uint8_t* out = nullptr;
  if (text) {
    if (line_off[k + 1] == line_off[k]) return;  // deferred
    out = text + line_off[k] + (sk & ~VCFTEXT_WAVE);
  } else if (status[k] != HBAM_OK) {
    return;
  }
  // the frame and the field headers passed k_vcftext_sizes' checks
  const uint64_t ro = rec_off[perm ? perm[k] : k];
  SamRecBytes b(data + ro);
  VcfRec R;
  R.status = HBAM_OK;
  R.deferred = text ? 0u : dflag[k];
  R.indiv = 8u + sam_rd32(b, 0);
  R.end = R.indiv + sam_rd32(b, 4);
  R.n_allele = sam_rd32(b, 24) >> 16;
  const uint32_t nfs = sam_rd32(b, 28);
  R.n_sample = nfs & 0xffffffu;
  R.n_fmt = nfs >> 24;
  {
    const uint32_t d0 = R.deferred;
    vcf_geno_headers(b, M, &R);  // for gt_f
    R.deferred = d0 | (text ? 0u : R.deferred);
  }
  VcfScan a{0, 0, 0, 0, 0};
  vcf_geno_scan(b, M, R, lane, 64, &a);
  a.present = wave_or(a.present);
  a.nullm = wave_or(a.nullm);
  a.gt_present = wave_or(a.gt_present);
  a.gt_null = wave_or(a.gt_null);
  a.bad = wave_or(a.bad);
  VcfKeys K;
  vcf_geno_keys(b, M, &R, a, &K);
  if (!text) {
    if (R.status != HBAM_OK) {
      if (lane == 0) {
        status[k] = R.status;
        atomicMin(first_stop, (unsigned long long)k);
      }
      return;
    }
    if (R.deferred) {
      if (lane == 0) {
        dflag[k] = 1;
        len[k] = 0;
      }
      return;
    }
  }
  // FORMAT, counted by every lane and written by lane 0
  uint32_t base;
  {
    SamOut w(lane == 0 ? out : nullptr);
    vcf_put_format(w, b, M, R, K);
    w.flush();
    base = (uint32_t)w.len;
  }
  for (uint32_t c = 0; c < R.n_sample; c += 64u) {
    const uint32_t s = c + lane;
    uint32_t l = 0;
    if (s < R.n_sample) {
      SamOut w(nullptr);
      vcf_put_sample(w, b, M, R, K, s);
      l = (uint32_t)w.len;
    }
    const uint32_t incl = wave_scan_dpp(l);
    if (out && s < R.n_sample) {
      SamOut w(out + base + (incl - l));
      vcf_put_sample(w, b, M, R, K, s);
      w.flush();
    }
    base += wave_last(incl);
  }
  if (lane == 0) {
    if (out) out[base] = '\n';
    else {
      const uint64_t total = (uint64_t)(sk & ~VCFTEXT_WAVE) + base + 1u;
      if (total > 0x7fffffffull) {
        status[k] = HBAM_EUNSUPPORTED;
        atomicMin(first_stop, (unsigned long long)k);
      } else {
        len[k] = (uint32_t)total;
      }
    }
  }
}

__global__ __launch_bounds__(VCFTEXT_WG) void k_vcftext_write(const uint8_t* __restrict__ data, uint64_t data_len,
                                                              const uint64_t* __restrict__ rec_off,
                                                              const uint32_t* __restrict__ perm, uint32_t n, VcfMeta M,
                                                              const uint64_t* __restrict__ line_off,
                                                              uint8_t* __restrict__ text) {
  const uint32_t k = blockIdx.x * VCFTEXT_WG + threadIdx.x;
  if (k >= n) return;
  const uint64_t lo = line_off[k];
  if (line_off[k + 1] == lo) return;  // deferred
  const uint64_t ro = rec_off[perm ? perm[k] : k];
  VcfRec r;
  vcf_text(data + ro, data_len - ro, M, HBAM_VCF_WAVE_SAMPLES, text + lo, &r);
}

}  // namespace hbam

extern "C" int hbam_bcf_header_text(hbam_ctx* c, const uint8_t* file, uint64_t len, uint8_t* out, uint64_t cap,
                                    uint64_t* text_len) {
  if (!c || !file || !text_len) return HBAM_EINVAL;
  hbam_bcf_header h;
  std::vector<uint8_t> u;
  const uint8_t* stream = nullptr;
  int rc = bcf_header_stream(c, file, len, &h, &u, &stream);
  if (rc) return rc;
  uint64_t n = h.header_len - 9;
  while (n && stream[9 + n - 1] == 0) --n;
  *text_len = n;
  if (!out) return HBAM_OK;
  if (cap < n) return set_err(c, HBAM_EINVAL, "hbam_bcf_header_text: the text has %llu bytes", (unsigned long long)n);
  memcpy(out, stream + 9, n);
  return HBAM_OK;
}

extern "C" int hbam_vcf_render(hbam_ctx* c, const uint8_t* data, uint64_t data_len, const uint64_t* rec_off,
                               const uint32_t* perm, uint64_t n, int on_device, const hbam_bcf_header* hdr,
                               const hbam_vcf_meta* meta, hbam_vcf_text* out) {
  if (!c || !out || !hdr || !meta || (n && (!data || !rec_off))) return HBAM_EINVAL;
  memset(out, 0, sizeof *out);
  HIPCHK(c, hipSetDevice(c->device));
  if (n >= 0xffffffffull) return set_err(c, HBAM_EINVAL, "hbam_vcf_render: at most 2^32 - 2 lines a call");
  if (!on_device && perm) return set_err(c, HBAM_EINVAL, "hbam_vcf_render: perm needs device arguments");
  const int32_t nc = hdr->n_contig, nd = hdr->n_dict;
  if (nc < 0 || nd < 0 || hdr->n_sample < 0 || !meta->contig_off || !meta->dict_off || (nd && (!meta->dict_rank ||
      !meta->dict_flags || !meta->dict_number)))
    return set_err(c, HBAM_EINVAL, "hbam_vcf_render: incomplete meta");
  for (int32_t k = 0; k < nc; ++k)
    if (meta->contig_off[k + 1] < meta->contig_off[k]) return set_err(c, HBAM_EINVAL, "hbam_vcf_render: contig_off must ascend");
  for (int32_t k = 0; k < nd; ++k)
    if (meta->dict_off[k + 1] < meta->dict_off[k]) return set_err(c, HBAM_EINVAL, "hbam_vcf_render: dict_off must ascend");
  const uint64_t cn_len = meta->contig_off[nc], dn_len = meta->dict_off[nd];
  if ((cn_len && !meta->contig_names) || (dn_len && !meta->dict_names)) return HBAM_EINVAL;
  c->timing = hbam_timing{};
  int rc;
  // meta: one device buffer, the u32 arrays first
  const uint64_t w_co = 0, w_do = w_co + (uint64_t)nc + 1, w_rank = w_do + (uint64_t)nd + 1, w_flags = w_rank + nd,
                 w_num = w_flags + nd, words = w_num + nd;
  std::vector<uint32_t> hm(words + (cn_len + dn_len + 3) / 4 + 1);
  memcpy(hm.data() + w_co, meta->contig_off, ((size_t)nc + 1) * 4);
  memcpy(hm.data() + w_do, meta->dict_off, ((size_t)nd + 1) * 4);
  if (nd) {
    memcpy(hm.data() + w_rank, meta->dict_rank, (size_t)nd * 4);
    memcpy(hm.data() + w_flags, meta->dict_flags, (size_t)nd * 4);
    memcpy(hm.data() + w_num, meta->dict_number, (size_t)nd * 4);
  }
  uint8_t* hb = (uint8_t*)(hm.data() + words);
  if (cn_len) memcpy(hb, meta->contig_names, cn_len);
  if (dn_len) memcpy(hb + cn_len, meta->dict_names, dn_len);
  uint32_t* dm;
  if ((rc = ensure(c, B_VT_META, hm.size(), &dm))) return rc;
  HIPCHK(c, copy_sync(c, dm, hm.data(), hm.size() * 4, hipMemcpyHostToDevice));
  VcfMeta M;
  M.contig_off = dm + w_co;
  M.dict_off = dm + w_do;
  M.rank = dm + w_rank;
  M.flags = dm + w_flags;
  M.number = (const int32_t*)(dm + w_num);
  M.contig = (const uint8_t*)(dm + words);
  M.dict = M.contig + cn_len;
  M.n_contig = nc;
  M.n_dict = nd;
  M.n_sample = hdr->n_sample;
  const uint8_t* ub = data;
  const uint64_t* ro = rec_off;
  // n offsets: a BCF record carries its own length, and k_vcftext_* never read rec_off[i + 1]
  if (!on_device && n && (rc = stage_records(c, B_VT_DATA, B_VT_RECOFF, data, data_len, rec_off, n, &ub, &ro)))
    return rc;
  TextOut T{{B_VT_LEN, B_VT_STATUS, B_VT_LINEOFF, B_VT_SMALL, B_VT_TEXT, true, B_VT_DFLAG, B_VT_DPOS, B_VT_DEFERRED}};
  uint32_t* site;
  if ((rc = ensure(c, B_VT_SITE, n + 1, &site)) || (rc = textout_begin(c, n, &T))) return rc;
  const bool waves = (uint32_t)hdr->n_sample >= HBAM_VCF_WAVE_SAMPLES;  // (a record's count must be the header's)
  if (n) {
    k_vcftext_sizes<<<grid_for(n, VCFTEXT_WG), VCFTEXT_WG, 0, c->stream>>>(ub, data_len, ro, perm, (uint32_t)n, M,
                                                                          T.len, T.lstatus, T.dflag, site,
                                                                          T.first_stop);
    if (waves)
      k_vcftext_geno<<<grid_for(n, VCFTEXT_WG / 64), VCFTEXT_WG, 0, c->stream>>>(
          ub, data_len, ro, perm, (uint32_t)n, M, site, T.len, T.lstatus, T.dflag, nullptr, nullptr, T.first_stop);
  }
  HIPCHK(c, hipGetLastError());
  if ((rc = textout_stop(c, &T))) return rc;
  if (T.cut) HIPCHK(c, copy_sync(c, &T.status, T.lstatus + T.m, 4, hipMemcpyDeviceToHost));
  if ((rc = textout_layout(c, &T))) return rc;
  if (T.m)
    k_vcftext_write<<<grid_for(T.m, VCFTEXT_WG), VCFTEXT_WG, 0, c->stream>>>(ub, data_len, ro, perm, (uint32_t)T.m, M,
                                                                            T.line_off, T.text);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  if (T.m && waves)
    k_vcftext_geno<<<grid_for(T.m, VCFTEXT_WG / 64), VCFTEXT_WG, 0, c->stream>>>(
        ub, data_len, ro, perm, (uint32_t)T.m, M, site, T.len, T.lstatus, T.dflag, T.line_off, T.text, T.first_stop);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  // no second stop: every check ran in the sizes passes, and the write passes do not touch first_stop
  HIPCHK(c, hipStreamSynchronize(c->stream));
  textout_finish(c, T, out);
  out->n_deferred = T.n_def;
  out->deferred = T.deferred;
  return HBAM_OK;
}
