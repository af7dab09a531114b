// hbam_bai.hip — the BAI index of a decoded file and the region filter of an indexed query, device
// side + C ABI.  Included at the end of hbam_capi.hip (one translation unit).
//
// Replaces cli/plugins/Index.java:61-127 (every record fed to [htsjdk] BAMIndexer, which writes
// <file>.bai) and the per-record overlap test behind reader.queryOverlapping in
// cli/plugins/View.java:164-221.  htsjdk is not in the reference tree: every rule below is restated
// from memory and unpinned (DESIGN.md lists them); tests/bai_ref.py restates the same rules over the
// CPU oracle's decode.
//
//  * hbam_bai_build over the device columns of a whole-file decode:
//      k_bai_span     lane per record: CIGAR walk -> alignment end, the two 16 KiB windows, the
//                     per-reference metadata (wave-aggregated atomics), the first raising record
//      scan + k_bai_compact   the coordinate-bearing records (pos >= 0), in file order
//      k_bai_order    reference order of those records ("Unexpected reference")
//      k_bai_linear   lin[ref][w] = min voffset over the records covering window w (u64 atomicMin;
//                     integer, so the same on every run)
//      hbam_sort_keys stable radix sort by (ref << 16 | bin): ties keep file order
//      k_bai_heads / scan / k_bai_chunks   a chunk opens at the first record of a (ref, bin) run or
//                     where the previous record's end is not in the same or the next BGZF block
//    The host then serialises: it walks the chunk list once and fills the empty linear slots.
//  * hbam_overlap_filter: k_ov_flags (predicate + per-wave ballot count), scan, k_ov_scatter
//    (rank inside the wave from the ballot): the kept indices ascending.
//
// Every read of a record's CIGAR is bounded by n_cigar, the pool offsets and the pool size; a
// record's reference index and windows are range-checked before they index anything.
#pragma once

namespace hbam {

constexpr uint32_t BAI_WG = 256;
constexpr uint32_t BAI_MAX_WIN = 32768;  // [htsjdk] LinearIndex.MAX_LINEAR_INDEX_SIZE (positions < 2^29)
constexpr uint32_t BAI_META_BIN = 37450;

// the columns the indexer and the filter read
struct BaiIn {
  const uint64_t* voffset;
  const int32_t* ref_id;
  const int32_t* pos;
  const uint16_t* bin;
  const uint16_t* n_cigar;
  const uint16_t* flag;
  const uint8_t* layout_ok;
  const uint64_t* cigar_off;
  const uint32_t* cigars;
  uint64_t n;
  uint64_t pool_n;  // u32 ops in the CIGAR pool
};

// per-reference accumulators (u64 each): windows seen, min chunk begin, max chunk end, records
// with flag 4 clear / set
struct BaiMeta {
  unsigned long long* n_intv;
  unsigned long long* first_off;
  unsigned long long* last_off;
  unsigned long long* aligned;
  unsigned long long* unaligned;
};

// reference length of record i's CIGAR (M, D, N, =, X; an op code above 8 adds nothing); 0 where the
// variable block is inconsistent (layout_ok = 0: the pool holds no ops for the record)
__device__ __forceinline__ int64_t bai_reflen(const BaiIn& in, uint64_t i) {
  if (!in.layout_ok[i]) return 0;
  const uint64_t o = in.cigar_off[i], e = in.cigar_off[i + 1];
  if (o > e || e > in.pool_n) return 0;
  const uint64_t cnt = (uint64_t)in.n_cigar[i] < e - o ? (uint64_t)in.n_cigar[i] : e - o;
  int64_t len = 0;
  for (uint64_t j = 0; j < cnt; ++j) {
    const uint32_t c = in.cigars[o + j];
    const uint32_t op = c & 15u;
    if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) len += (int64_t)(c >> 4);
  }
  return len;
}

// [htsjdk] SAMRecord.getAlignmentStart / getAlignmentEnd (1-based; end 0 for an unmapped read)
__device__ __forceinline__ void bai_span(const BaiIn& in, uint64_t i, int64_t* start1, int64_t* end1) {
  *start1 = (int64_t)in.pos[i] + 1;
  *end1 = (in.flag[i] & 4u) ? 0 : *start1 + bai_reflen(in, i) - 1;
}

// [htsjdk] LinearIndex.convertToLinearIndexOffset
__device__ __forceinline__ int64_t bai_window(int64_t p) { return (p <= 0 ? 0 : p - 1) >> 14; }

__device__ __forceinline__ uint64_t bai_wmin(uint64_t v) {
  for (int d = 32; d; d >>= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, d);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ uint64_t bai_wmax(uint64_t v) {
  for (int d = 32; d; d >>= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, d);
    v = o > v ? o : v;
  }
  return v;
}

// first raising record: atomicMin of (record << 1 | kind), kind 0 = HBAM_EDATA, 1 = HBAM_EINDEX (the
// reference check comes first in BAMIndexer.processAlignment)
__global__ __launch_bounds__(BAI_WG) void k_bai_span(BaiIn in, int32_t n_ref, uint64_t end_voffset, BaiMeta meta,
                                                     uint32_t* __restrict__ has, uint32_t* __restrict__ w0o,
                                                     uint32_t* __restrict__ w1o,
                                                     unsigned long long* __restrict__ first_err,
                                                     unsigned long long* __restrict__ n_no_coor) {
  const uint64_t i = (uint64_t)blockIdx.x * BAI_WG + threadIdx.x;
  const bool live = i < in.n;
  const uint32_t lane = threadIdx.x & 63u;
  bool coord = false, ok = false;
  int32_t ref = -1;
  uint64_t w0 = 0, w1 = 0, beg = ~0ull, end = 0;
  bool unal = false;
  if (live) {
    coord = in.pos[i] >= 0;
    ref = in.ref_id[i];
    if (coord) {
      int64_t s, e;
      bai_span(in, i, &s, &e);
      if (e == 0) w0 = w1 = (uint64_t)bai_window(s - 1);
      else { w0 = (uint64_t)bai_window(s); w1 = (uint64_t)bai_window(e); }
      unsigned long long err = ~0ull;
      if (ref < 0 || ref >= n_ref) err = i << 1;
      else if (w0 >= BAI_MAX_WIN || w1 >= BAI_MAX_WIN) err = i << 1 | 1u;
      if (err != ~0ull) atomicMin(first_err, err);
      ok = err == ~0ull;
      beg = in.voffset[i];
      end = i + 1 < in.n ? in.voffset[i + 1] : end_voffset;
      unal = (in.flag[i] & 4u) != 0;
    }
    has[i] = coord ? 1u : 0u;
    w0o[i] = (uint32_t)(w0 < BAI_MAX_WIN ? w0 : BAI_MAX_WIN);
    w1o[i] = (uint32_t)(w1 < BAI_MAX_WIN ? w1 : BAI_MAX_WIN);
  }
  // records without coordinates: one add per wave
  const uint64_t nc = __ballot(live && !coord);
  if (lane == 0 && nc) atomicAdd(n_no_coor, (unsigned long long)__popcll(nc));
  // per-reference metadata: one round per distinct reference in the wave (one, in a sorted file)
  uint64_t todo = __ballot(ok);
  while (todo) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const int32_t r = __shfl(ref, leader);
    const bool mine = ok && ref == r;
    const uint64_t m = __ballot(mine);
    const uint64_t b = bai_wmin(mine ? beg : ~0ull);
    const uint64_t e = bai_wmax(mine ? end : 0ull);
    const uint64_t w = bai_wmax(mine ? w1 + 1 : 0ull);
    const uint64_t nu = __ballot(mine && unal);
    if ((int)lane == leader) {
      atomicMax(meta.n_intv + r, (unsigned long long)w);
      atomicMin(meta.first_off + r, (unsigned long long)b);
      atomicMax(meta.last_off + r, (unsigned long long)e);
      const unsigned long long u = (unsigned long long)__popcll(nu), a = (unsigned long long)__popcll(m) - u;
      if (a) atomicAdd(meta.aligned + r, a);
      if (u) atomicAdd(meta.unaligned + r, u);
    }
    todo &= ~m;
  }
}

// the coordinate-bearing records in file order: sort key, chunk [begin, end), source record
__global__ __launch_bounds__(BAI_WG) void k_bai_compact(BaiIn in, uint64_t end_voffset,
                                                        const uint32_t* __restrict__ has,
                                                        const uint64_t* __restrict__ coff, int64_t* __restrict__ ckey,
                                                        uint64_t* __restrict__ cbeg, uint64_t* __restrict__ cend,
                                                        uint32_t* __restrict__ crec) {
  const uint64_t i = (uint64_t)blockIdx.x * BAI_WG + threadIdx.x;
  if (i >= in.n || !has[i]) return;
  const uint64_t j = coff[i];
  ckey[j] = (int64_t)(((uint64_t)(int64_t)in.ref_id[i] << 16) | (uint64_t)in.bin[i]);
  cbeg[j] = in.voffset[i];
  cend[j] = i + 1 < in.n ? in.voffset[i + 1] : end_voffset;
  crec[j] = (uint32_t)i;
}

// [htsjdk] BAMIndexer.advanceToReference: a reference smaller than the previous coordinate-bearing
// record's raises ("Unexpected reference")
__global__ __launch_bounds__(BAI_WG) void k_bai_order(const int64_t* __restrict__ ckey,
                                                      const uint32_t* __restrict__ crec, uint64_t m,
                                                      unsigned long long* __restrict__ first_err) {
  const uint64_t j = (uint64_t)blockIdx.x * BAI_WG + threadIdx.x;
  if (j == 0 || j >= m) return;
  if ((ckey[j] >> 16) < (ckey[j - 1] >> 16)) atomicMin(first_err, (unsigned long long)crec[j] << 1);
}

// linear index: min voffset per (reference, window); lin is 0xff-filled (empty)
__global__ __launch_bounds__(BAI_WG) void k_bai_linear(BaiIn in, int32_t n_ref, const uint32_t* __restrict__ has,
                                                       const uint32_t* __restrict__ w0, const uint32_t* __restrict__ w1,
                                                       const uint64_t* __restrict__ lin_off,
                                                       unsigned long long* __restrict__ lin) {
  const uint64_t i = (uint64_t)blockIdx.x * BAI_WG + threadIdx.x;
  if (i >= in.n || !has[i]) return;
  const int32_t r = in.ref_id[i];
  if (r < 0 || r >= n_ref) return;
  const uint64_t base = lin_off[r], cnt = lin_off[r + 1] - base;
  const unsigned long long v = in.voffset[i];
  for (uint64_t w = w0[i]; w <= (uint64_t)w1[i] && w < cnt; ++w) atomicMin(lin + base + w, v);
}

// [htsjdk] BlockCompressedFilePointerUtil.areInSameOrAdjacentBlocks (the + 1 is on the byte address)
__device__ __forceinline__ bool bai_adjacent(uint64_t a, uint64_t b) {
  return (a >> 16) == (b >> 16) || (a >> 16) + 1 == (b >> 16);
}

__global__ __launch_bounds__(BAI_WG) void k_bai_heads(const int64_t* __restrict__ ckey,
                                                      const uint64_t* __restrict__ cbeg,
                                                      const uint64_t* __restrict__ cend,
                                                      const uint32_t* __restrict__ perm, uint64_t m,
                                                      uint32_t* __restrict__ head) {
  const uint64_t j = (uint64_t)blockIdx.x * BAI_WG + threadIdx.x;
  if (j >= m) return;
  const uint32_t e = perm[j];
  bool h = j == 0;
  if (!h) {
    const uint32_t p = perm[j - 1];
    h = ckey[p] != ckey[e] || !bai_adjacent(cend[p], cbeg[e]);
  }
  head[j] = h ? 1u : 0u;
}

// chunk c = [begin of its head, end of its last element]; hoff = exclusive scan of head
__global__ __launch_bounds__(BAI_WG) void k_bai_chunks(const int64_t* __restrict__ ckey,
                                                       const uint64_t* __restrict__ cbeg,
                                                       const uint64_t* __restrict__ cend,
                                                       const uint32_t* __restrict__ perm, uint64_t m,
                                                       const uint32_t* __restrict__ head,
                                                       const uint64_t* __restrict__ hoff, uint64_t n_chunk,
                                                       int64_t* __restrict__ ck, uint64_t* __restrict__ cb,
                                                       uint64_t* __restrict__ ce) {
  const uint64_t j = (uint64_t)blockIdx.x * BAI_WG + threadIdx.x;
  if (j >= m) return;
  const uint32_t e = perm[j];
  const uint64_t c = hoff[j] + head[j] - 1;  // head[0] = 1, so c >= 0
  if (c >= n_chunk) return;
  if (head[j]) {
    ck[c] = ckey[e];
    cb[c] = cbeg[e];
  }
  if (j + 1 == m || head[j + 1]) ce[c] = cend[e];
}

// ---- region filter --------------------------------------------------------------------------
// [htsjdk] the overlap test of BAMFileReader's query iterators: a read without an end (unmapped, or
// a CIGAR without reference bases at position 1) counts as its start position
__global__ __launch_bounds__(BAI_WG) void k_ov_flags(BaiIn in, int32_t ref, int64_t qbeg, int64_t qend,
                                                     int contained, uint8_t* __restrict__ keep,
                                                     uint32_t* __restrict__ wave_cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * BAI_WG + threadIdx.x;
  bool k = false;
  if (i < in.n && in.ref_id[i] == ref) {
    int64_t s, e;
    bai_span(in, i, &s, &e);
    if (e == 0) e = s;
    k = contained ? (s >= qbeg && e <= qend) : (s <= qend && e >= qbeg);
  }
  if (i < in.n) keep[i] = k ? 1 : 0;
  const uint64_t m = __ballot(k);
  if ((threadIdx.x & 63u) == 0) wave_cnt[i >> 6] = (uint32_t)__popcll(m);
}

__global__ __launch_bounds__(BAI_WG) void k_ov_scatter(const uint8_t* __restrict__ keep, uint64_t n,
                                                       const uint64_t* __restrict__ wave_off, uint64_t total,
                                                       uint32_t* __restrict__ idx_out) {
  const uint64_t i = (uint64_t)blockIdx.x * BAI_WG + threadIdx.x;
  const bool k = i < n && keep[i];
  const uint64_t m = __ballot(k);
  if (!k) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t o = wave_off[i >> 6] + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
  if (o < total) idx_out[o] = (uint32_t)i;
}

}  // namespace hbam

// ---- C ABI ------------------------------------------------------------------------------------
namespace {

int bai_input(hbam_ctx* c, const hbam_columns* dv, BaiIn* in) {
  const uint64_t n = dv->n_records;
  if (n > 0xffffffffull) return set_err(c, HBAM_EINVAL, "records: n > 2^32-1");
  if (n && (!dv->voffset || !dv->ref_id || !dv->pos || !dv->bin || !dv->n_cigar || !dv->flag || !dv->layout_ok ||
            !dv->cigar_off))
    return set_err(c, HBAM_EINVAL, "records: a column is missing (device columns of a decode are expected)");
  *in = BaiIn{dv->voffset, dv->ref_id, dv->pos, dv->bin, dv->n_cigar, dv->flag, dv->layout_ok,
              dv->cigar_off, dv->cigars, n, 0};
  if (n) {
    uint64_t pn = 0;
    HIPCHK(c, copy_sync(c, &pn, dv->cigar_off + n, 8, hipMemcpyDeviceToHost));
    in->pool_n = dv->cigars ? pn : 0;
  }
  return HBAM_OK;
}

inline void bai_put32(std::vector<uint8_t>& o, uint32_t v) {
  for (int k = 0; k < 4; ++k) o.push_back((uint8_t)(v >> (8 * k)));
}
inline void bai_put64(std::vector<uint8_t>& o, uint64_t v) {
  for (int k = 0; k < 8; ++k) o.push_back((uint8_t)(v >> (8 * k)));
}

}  // namespace

extern "C" uint64_t hbam_bai_bound(uint64_t n_records, int32_t n_ref) {
  const uint64_t r = n_ref > 0 ? (uint64_t)n_ref : 0;
  // magic, n_ref, n_no_coor; per reference n_bin, the metadata bin, n_intv and every window; per
  // record at most one bin header and one chunk
  return 16 + r * (4 + 40 + 4 + 8ull * BAI_MAX_WIN) + n_records * 24;
}

extern "C" int64_t hbam_bai_build(hbam_ctx* c, const hbam_columns* dv, int32_t n_ref, uint64_t end_voffset,
                                  uint8_t* out, uint64_t cap, uint64_t* err_record) {
  if (!c || !dv || n_ref < 0 || (!out && cap)) return HBAM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (err_record) *err_record = ~0ull;
  if (dv->status != HBAM_OK) {
    if (err_record) *err_record = dv->err_record;
    return set_err(c, dv->status, "hbam_bai_build: the decode raised %d", dv->status);
  }
  BaiIn in;
  int rc;
  if ((rc = bai_input(c, dv, &in))) return rc;
  const uint64_t n = in.n, R = (uint64_t)n_ref;
  HIPCHK(c, hipEventRecord(c->ev[12], c->stream));

  uint32_t *has, *w0, *w1;
  uint64_t *coff, *refm, *small;
  if ((rc = ensure(c, B_BAI_HAS, n + 1, &has)) || (rc = ensure(c, B_BAI_W0, n + 1, &w0)) ||
      (rc = ensure(c, B_BAI_W1, n + 1, &w1)) || (rc = ensure(c, B_BAI_COFF, n + 1, &coff)) ||
      (rc = ensure(c, B_BAI_REF, 5 * R + 1, &refm)) || (rc = ensure(c, B_BAI_SMALL, 2, &small)))
    return rc;
  BaiMeta meta{(unsigned long long*)refm, (unsigned long long*)refm + R, (unsigned long long*)refm + 2 * R,
               (unsigned long long*)refm + 3 * R, (unsigned long long*)refm + 4 * R};
  HIPCHK(c, hipMemsetAsync(refm, 0, 5 * R * 8 + 8, c->stream));
  if (R) HIPCHK(c, hipMemsetAsync(meta.first_off, 0xff, R * 8, c->stream));
  HIPCHK(c, hipMemsetAsync(small, 0xff, 8, c->stream));
  HIPCHK(c, hipMemsetAsync(small + 1, 0, 8, c->stream));
  uint64_t m = 0;
  if (n) {
    k_bai_span<<<grid_for(n, BAI_WG), BAI_WG, 0, c->stream>>>(in, n_ref, end_voffset, meta, has, w0, w1,
                                                             (unsigned long long*)small,
                                                             (unsigned long long*)small + 1);
    HIPCHK(c, hipGetLastError());
    if ((rc = scan_exclusive(c, has, n, coff, &m))) return rc;
  }
  int64_t* ckey;
  uint64_t *cbeg, *cend;
  uint32_t *crec, *perm;
  if ((rc = ensure(c, B_BAI_KEY, m + 1, &ckey)) || (rc = ensure(c, B_BAI_CBEG, m + 1, &cbeg)) ||
      (rc = ensure(c, B_BAI_CEND, m + 1, &cend)) || (rc = ensure(c, B_BAI_CREC, m + 1, &crec)) ||
      (rc = ensure(c, B_BAI_PERM, m + 1, &perm)))
    return rc;
  if (m) {
    k_bai_compact<<<grid_for(n, BAI_WG), BAI_WG, 0, c->stream>>>(in, end_voffset, has, coff, ckey, cbeg, cend, crec);
    k_bai_order<<<grid_for(m, BAI_WG), BAI_WG, 0, c->stream>>>(ckey, crec, m, (unsigned long long*)small);
    HIPCHK(c, hipGetLastError());
  }
  uint64_t hs[2];
  HIPCHK(c, copy_sync(c, hs, small, 16, hipMemcpyDeviceToHost));
  if (hs[0] != ~0ull) {
    if (err_record) *err_record = hs[0] >> 1;
    const int code = (hs[0] & 1u) ? HBAM_EINDEX : HBAM_EDATA;
    return set_err(c, code, (hs[0] & 1u) ? "hbam_bai_build: record %llu lies past position 2^29"
                                         : "hbam_bai_build: unexpected reference at record %llu",
                   (unsigned long long)(hs[0] >> 1));
  }
  const uint64_t n_no_coor = hs[1];
  std::vector<uint64_t> hm(5 * R + 1);
  HIPCHK(c, copy_sync(c, hm.data(), refm, 5 * R * 8, hipMemcpyDeviceToHost));

  // linear index: the windows of every reference back to back
  std::vector<uint64_t> lin_off(R + 1, 0);
  for (uint64_t r = 0; r < R; ++r) lin_off[r + 1] = lin_off[r] + std::min<uint64_t>(hm[r], BAI_MAX_WIN);
  const uint64_t n_lin = lin_off[R];
  uint64_t *dlin_off, *dlin;
  if ((rc = ensure(c, B_BAI_LINOFF, R + 1, &dlin_off)) || (rc = ensure(c, B_BAI_LIN, n_lin + 1, &dlin))) return rc;
  HIPCHK(c, hipMemcpyAsync(dlin_off, lin_off.data(), (R + 1) * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(dlin, 0xff, n_lin * 8 + 8, c->stream));
  if (m && n_lin) {
    k_bai_linear<<<grid_for(n, BAI_WG), BAI_WG, 0, c->stream>>>(in, n_ref, has, w0, w1, dlin_off,
                                                               (unsigned long long*)dlin);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));  // lin_off (host memory) is read by the copy above

  // bin chunks
  uint64_t n_chunk = 0;
  int64_t* ck = nullptr;
  uint64_t *cb = nullptr, *ce = nullptr;
  if (m) {
    if ((rc = hbam_sort_keys(c, ckey, m, nullptr, perm))) return rc;
    uint32_t* head;
    uint64_t* hoff;
    if ((rc = ensure(c, B_BAI_HEAD, m + 1, &head)) || (rc = ensure(c, B_BAI_HOFF, m + 1, &hoff))) return rc;
    HIPCHK(c, hipMemsetAsync(head + m, 0, 4, c->stream));
    k_bai_heads<<<grid_for(m, BAI_WG), BAI_WG, 0, c->stream>>>(ckey, cbeg, cend, perm, m, head);
    HIPCHK(c, hipGetLastError());
    if ((rc = scan_exclusive(c, head, m, hoff, &n_chunk))) return rc;
    if ((rc = ensure(c, B_BAI_CK, n_chunk + 1, &ck)) || (rc = ensure(c, B_BAI_CB, n_chunk + 1, &cb)) ||
        (rc = ensure(c, B_BAI_CE, n_chunk + 1, &ce)))
      return rc;
    k_bai_chunks<<<grid_for(m, BAI_WG), BAI_WG, 0, c->stream>>>(ckey, cbeg, cend, perm, m, head, hoff, n_chunk, ck,
                                                               cb, ce);
    HIPCHK(c, hipGetLastError());
  }
  std::vector<int64_t> hk(n_chunk);
  std::vector<uint64_t> hb(n_chunk), he(n_chunk), hl(n_lin);
  if (n_chunk) {
    HIPCHK(c, hipMemcpyAsync(hk.data(), ck, n_chunk * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hb.data(), cb, n_chunk * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(he.data(), ce, n_chunk * 8, hipMemcpyDeviceToHost, c->stream));
  }
  if (n_lin) HIPCHK(c, hipMemcpyAsync(hl.data(), dlin, n_lin * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[13], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->timing = hbam_timing{};
  c->timing.total_ms = ev_ms(c, 12, 13);
  c->timing.n_records = n;
  c->timing.n_blocks = n_chunk;

  // serialise ([htsjdk] BinaryBAMIndexWriter: little-endian)
  std::vector<uint8_t> o;
  o.reserve(16 + R * 56 + n_chunk * 24 + n_lin * 8);
  o.insert(o.end(), {'B', 'A', 'I', 1});
  bai_put32(o, (uint32_t)n_ref);
  uint64_t q = 0;
  for (uint64_t r = 0; r < R; ++r) {
    uint64_t q1 = q;
    uint32_t n_bin = 0;
    while (q1 < n_chunk && (uint64_t)(hk[q1] >> 16) == r) {
      if (q1 == q || hk[q1] != hk[q1 - 1]) ++n_bin;
      ++q1;
    }
    bai_put32(o, n_bin ? n_bin + 1 : 0);
    while (q < q1) {
      uint64_t z = q;
      while (z < q1 && hk[z] == hk[q]) ++z;
      bai_put32(o, (uint32_t)(hk[q] & 0xffff));
      bai_put32(o, (uint32_t)(z - q));
      for (; q < z; ++q) {
        bai_put64(o, hb[q]);
        bai_put64(o, he[q]);
      }
    }
    if (n_bin) {  // the metadata pseudo-bin
      bai_put32(o, BAI_META_BIN);
      bai_put32(o, 2);
      bai_put64(o, hm[R + r]);
      bai_put64(o, hm[2 * R + r]);
      bai_put64(o, hm[3 * R + r]);
      bai_put64(o, hm[4 * R + r]);
    }
    const uint64_t ni = lin_off[r + 1] - lin_off[r];
    bai_put32(o, (uint32_t)ni);
    uint64_t last = 0;
    for (uint64_t w = 0; w < ni; ++w) {  // an empty slot repeats the last value before it
      const uint64_t v = hl[lin_off[r] + w];
      if (v != ~0ull) last = v;
      bai_put64(o, last);
    }
  }
  bai_put64(o, n_no_coor);
  if (o.size() > cap)
    return set_err(c, HBAM_EMORE, "hbam_bai_build: %llu bytes > cap %llu", (unsigned long long)o.size(),
                   (unsigned long long)cap);
  memcpy(out, o.data(), o.size());
  return (int64_t)o.size();
}

extern "C" int64_t hbam_overlap_filter(hbam_ctx* c, const hbam_columns* dv, int32_t ref_id, int64_t beg, int64_t end,
                                       int contained, uint32_t* idx_out) {
  if (!c || !dv || (dv->n_records && !idx_out)) return HBAM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  BaiIn in;
  int rc;
  if ((rc = bai_input(c, dv, &in))) return rc;
  const uint64_t n = in.n;
  if (n == 0) return 0;
  const int64_t qbeg = beg <= 0 ? 1 : beg;
  const int64_t qend = end <= 0 ? INT64_MAX : end;  // the end of the reference
  const uint64_t nw = (n + 63) / 64;
  uint8_t* keep;
  uint32_t* cnt;
  uint64_t* woff;
  // the grid covers whole workgroups: wave_cnt has a slot for every wave launched
  const uint64_t nw_launch = (uint64_t)grid_for(n, BAI_WG) * (BAI_WG / 64);
  if ((rc = ensure(c, B_OV_KEEP, n + 1, &keep)) || (rc = ensure(c, B_OV_CNT, nw_launch + 1, &cnt)) ||
      (rc = ensure(c, B_OV_OFF, nw_launch + 1, &woff)))
    return rc;
  k_ov_flags<<<grid_for(n, BAI_WG), BAI_WG, 0, c->stream>>>(in, ref_id, qbeg, qend, contained, keep, cnt);
  HIPCHK(c, hipGetLastError());
  uint64_t total = 0;
  if ((rc = scan_exclusive(c, cnt, nw, woff, &total))) return rc;
  if (total) {
    k_ov_scatter<<<grid_for(n, BAI_WG), BAI_WG, 0, c->stream>>>(keep, n, woff, total, idx_out);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return (int64_t)total;
}
