// vcf_text_host.cpp — the per-record rules of csrc/vcf_text.h run on a CPU, as they stand.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       -Ihadoop-bam_amd/csrc -o vcf_text_host tools/vcf_text_host.cpp
//   vcf_text_host in.bin out.bin
//
// in.bin:  i32 n_contig, n_dict, n_sample; u32 wave_cut; u32 contig_off[n_contig + 1], the contig
//          names; u32 dict_off[n_dict + 1], the dictionary strings; u32 rank[n_dict], u32 flags[n_dict],
//          i32 number[n_dict]; u64 n, u64 rec_off[n], u64 data_len, the record bytes.
// out.bin: per record i32 status, u32 deferred, u32 length, then the line's bytes.
//
// Every record goes through vcf_text twice (sizes, then bytes at the line's offset in one text
// buffer, as k_vcftext_write writes it).  A record of wave_cut samples or more takes k_vcftext_geno's
// path with its 64 lanes run one after the other: each lane's scan of its samples, the OR of the
// scans, the key order, the per-sample lengths and their prefix sums per 64 samples, then each
// sample's bytes at its offset.  The records stand in a heap block of exactly their bytes + the 64
// bytes of slack and the text in one of exactly its length, so the address sanitizer sees any access
// the rules do not allow.  A failing record gets length 0 and does not end the run (the kernels'
// first-stop rule, the DPP scan and the wave OR need the GPU tests).  tests/test_vcftext.py compares
// with tests/vcftext_ref.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "hbam.h"
#include "vcf_text.h"

using namespace hbam;

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

struct Line {
  int32_t status;
  uint32_t deferred, len, site, by_wave;
};

// k_vcftext_geno for one record: out == nullptr counts (and checks), else writes behind the site columns
static void geno(const uint8_t* rec, const VcfMeta& M, Line* L, uint8_t* out) {
  SamRecBytes b(rec);
  VcfRec R;
  R.status = HBAM_OK;
  R.deferred = out ? 0u : L->deferred;
  R.indiv = 8u + sam_rd32(b, 0);
  R.end = R.indiv + sam_rd32(b, 4);
  R.n_allele = sam_rd32(b, 24) >> 16;
  const uint32_t nfs = sam_rd32(b, 28);
  R.n_sample = nfs & 0xffffffu;
  R.n_fmt = nfs >> 24;
  const uint32_t d0 = R.deferred;
  vcf_geno_headers(b, M, &R);
  R.deferred = d0 | (out ? 0u : R.deferred);
  VcfScan a{0, 0, 0, 0, 0};
  for (uint32_t lane = 0; lane < 64; ++lane) {
    VcfScan l{0, 0, 0, 0, 0};
    vcf_geno_scan(b, M, R, lane, 64, &l);
    a.present |= l.present;
    a.nullm |= l.nullm;
    a.gt_present |= l.gt_present;
    a.gt_null |= l.gt_null;
    a.bad |= l.bad;
  }
  VcfKeys K;
  vcf_geno_keys(b, M, &R, a, &K);
  if (!out) {
    if (R.status != HBAM_OK) {
      L->status = R.status;
      return;
    }
    if (R.deferred) {
      L->deferred = 1;
      L->len = 0;
      return;
    }
  }
  uint32_t base;
  {
    SamOut w(out);
    vcf_put_format(w, b, M, R, K);
    w.flush();
    base = (uint32_t)w.len;
  }
  for (uint32_t c = 0; c < R.n_sample; c += 64u) {
    uint32_t len[64], excl = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {
      len[lane] = 0;
      if (c + lane < R.n_sample) {
        SamOut w(nullptr);
        vcf_put_sample(w, b, M, R, K, c + lane);
        len[lane] = (uint32_t)w.len;
      }
    }
    for (uint32_t lane = 0; lane < 64; ++lane) {
      if (out && c + lane < R.n_sample) {
        SamOut w(out + base + excl);
        vcf_put_sample(w, b, M, R, K, c + lane);
        w.flush();
      }
      excl += len[lane];
    }
    base += excl;
  }
  if (out) out[base] = '\n';
  else L->len = L->site + base + 1u;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hd[3];
  uint32_t wave_cut;
  if (!rd(f, hd, 12) || !rd(f, &wave_cut, 4) || hd[0] < 0 || hd[1] < 0) return 2;
  const size_t nc = (size_t)hd[0], nd = (size_t)hd[1];
  std::vector<uint32_t> co(nc + 1), dof(nd + 1), rank(nd + 1), flags(nd + 1);
  std::vector<int32_t> number(nd + 1);
  if (!rd(f, co.data(), 4 * (nc + 1))) return 2;
  std::vector<uint8_t> cn(co[nc] + 1);
  if (!rd(f, cn.data(), co[nc]) || !rd(f, dof.data(), 4 * (nd + 1))) return 2;
  std::vector<uint8_t> dn(dof[nd] + 1);
  if (!rd(f, dn.data(), dof[nd]) || !rd(f, rank.data(), 4 * nd) || !rd(f, flags.data(), 4 * nd) ||
      !rd(f, number.data(), 4 * nd))
    return 2;
  uint64_t n, data_len;
  if (!rd(f, &n, 8)) return 2;
  std::vector<uint64_t> rec_off(n + 1);
  if (!rd(f, rec_off.data(), 8 * n) || !rd(f, &data_len, 8)) return 2;
  uint8_t* const data = new uint8_t[data_len + 64];  // the 64 readable bytes behind the records
  memset(data + data_len, 0, 64);
  if (!rd(f, data, data_len)) return 2;
  fclose(f);
  const VcfMeta M{cn.data(), co.data(), dn.data(), dof.data(), rank.data(), flags.data(), number.data(),
                  hd[0], hd[1], hd[2]};

  std::vector<Line> ls(n);
  std::vector<uint64_t> line_off(n + 1, 0);
  for (uint64_t i = 0; i < n; ++i) {
    VcfRec r;
    r.status = HBAM_ETRIBBLE;
    r.deferred = r.len = r.by_wave = 0;
    if (rec_off[i] <= data_len) vcf_text(data + rec_off[i], data_len - rec_off[i], M, wave_cut, nullptr, &r);
    ls[i] = Line{r.status, r.deferred, (r.deferred || r.by_wave) ? 0u : r.len, r.len, r.by_wave};
    if (r.status == HBAM_OK && r.by_wave) geno(data + rec_off[i], M, &ls[i], nullptr);
    if (ls[i].status != HBAM_OK || ls[i].deferred) ls[i].len = 0;
    line_off[i + 1] = line_off[i] + ls[i].len;
  }
  const uint64_t total = line_off[n];
  uint8_t* const text = new uint8_t[total ? total : 1];
  memset(text, 0xAA, total);
  for (uint64_t i = 0; i < n; ++i) {
    if (ls[i].status != HBAM_OK || ls[i].deferred) continue;
    VcfRec r2;
    vcf_text(data + rec_off[i], data_len - rec_off[i], M, wave_cut, text + line_off[i], &r2);
    if (r2.status != HBAM_OK || r2.deferred || r2.by_wave != ls[i].by_wave ||
        r2.len != (ls[i].by_wave ? ls[i].site : ls[i].len)) {
      fprintf(stderr, "the two passes disagree at record %llu\n", (unsigned long long)i);
      return 1;
    }
    if (ls[i].by_wave) geno(data + rec_off[i], M, &ls[i], text + line_off[i] + ls[i].site);
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t h[3] = {(uint32_t)ls[i].status, ls[i].deferred, ls[i].len};
    fwrite(h, 4, 3, o);
    fwrite(text + line_off[i], 1, ls[i].len, o);
  }
  fclose(o);
  delete[] text;
  delete[] data;
  return 0;
}
