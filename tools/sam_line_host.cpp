// sam_line_host.cpp — the per-line rules of csrc/sam_line.h run on a CPU, as they stand.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -Iinclude -Ihadoop-bam_amd/csrc \
//       -o sam_line_host tools/sam_line_host.cpp
//   sam_line_host in.sam out.bin
//
// Reads a SAM text file, takes the dictionary from its @SQ lines, builds the tab bitmap the
// structural pass would, and runs every data line through sam_line twice (sizes, then bytes) and
// its SEQ and QUAL through the bulk pass's unit functions, unit by unit.  Per line it writes
// status (i32), record size (u32, 0 on a failure), sam_murmur_bytes of the raw line with seed -7
// (i64) and the record's bytes.  tests/test_sam.py compares that with tests/sam_ref.py.  What the
// kernels add to these functions (the wave's unit numbering, the scans) needs the GPU tests.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "sam_line.h"

using namespace hbam;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> d;
  {
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + n);
  }
  fclose(f);
  const size_t N = d.size();
  d.resize(N + 64, 0);  // the 64 readable bytes behind a window
  // the header: the run of '@' lines; @SQ SN -> ordinal
  size_t p = 0;
  std::map<std::string, int> dic;
  while (p < N && d[p] == '@') {
    size_t e = p;
    while (e < N && d[e] != '\n') ++e;
    std::string ln((const char*)&d[p], e - p);
    if (!ln.empty() && ln.back() == '\r') ln.pop_back();
    if (ln.rfind("@SQ", 0) == 0) {
      const size_t a = ln.find("\tSN:");
      if (a != std::string::npos) {
        const size_t b = ln.find('\t', a + 1);
        const int ordinal = (int)dic.size();
        dic.emplace(ln.substr(a + 4, b == std::string::npos ? std::string::npos : b - a - 4), ordinal);
      }
    }
    p = e + 1;
  }
  uint32_t size = 2;
  while (size < 2 * dic.size()) size *= 2;
  std::vector<hbam_vcf_contig> tab(size);
  for (auto& e : tab) e.ordinal = -1;
  std::string names;
  for (const auto& kv : dic) {
    uint32_t h = 2166136261u;
    for (unsigned char c : kv.first) h = (h ^ c) * 16777619u;
    h &= size - 1;
    while (tab[h].ordinal >= 0) h = (h + 1) & (size - 1);
    tab[h].name_off = (uint32_t)names.size();
    tab[h].name_len = (uint32_t)kv.first.size();
    tab[h].ordinal = kv.second;
    names += kv.first;
  }
  std::vector<uint64_t> tabmap((N + 63) / 64 + 2, 0);
  for (size_t i = 0; i < N; ++i)
    if (d[i] == '\t') tabmap[i >> 6] |= 1ull << (i & 63);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const uint8_t* const nm = (const uint8_t*)names.data();
  while (p < N) {
    size_t e = p;
    while (e < N && d[e] != '\n') ++e;
    size_t z = e;
    if (e < N && z > p && d[z - 1] == '\r') --z;
    const SamTabs tb{tabmap.data(), (uint32_t)p, (uint32_t)z};
    SamLine r;
    sam_line(&d[p], tb, tab.data(), size - 1, nm, nullptr, &r);
    int32_t st = r.status;
    std::vector<uint8_t> rec(r.size + 64, 0xAA);
    if (st == HBAM_OK) {
      SamLine r2;
      sam_line(&d[p], tb, tab.data(), size - 1, nm, rec.data(), &r2);
      if (r2.size != r.size || r2.status != HBAM_OK) {
        fprintf(stderr, "the two passes disagree at offset %zu\n", p);
        return 1;
      }
      const uint32_t ls = r.l_seq, packed = (ls + 1) / 2, us = (packed + 15) / 16, uq = (ls + 15) / 16;
      const uint8_t* src = &d[p] + r.seq_rel;
      for (uint32_t k = 0; k < us + uq; ++k) {
        uint32_t ob[4], nb;
        uint8_t* dst;
        bool ok = true;
        if (k < us) {
          uint32_t w[8];
          memcpy(w, src + 32 * k, 32);
          const uint32_t nchar = std::min(32u, ls - 32 * k);
          ok = sam_seq_unit(w, nchar, ob);
          nb = (nchar + 1) / 2;
          dst = rec.data() + r.seq_out + 16 * k;
        } else {
          const uint32_t kq = k - us;
          nb = std::min(16u, ls - 16 * kq);
          dst = rec.data() + r.seq_out + packed + 16 * kq;
          if (r.qual_star) {
            ob[0] = ob[1] = ob[2] = ob[3] = ~0u;
          } else {
            uint32_t w[4];
            memcpy(w, src + ls + 1 + 16 * kq, 16);
            ok = sam_qual_unit(w, nb, ob);
          }
        }
        memcpy(dst, ob, nb);
        if (!ok) st = HBAM_EFORMAT;
      }
    }
    const uint8_t* lp = &d[p];
    const int64_t mh = sam_murmur_bytes([lp](uint32_t j) -> uint8_t { return lp[j]; }, (uint32_t)(z - p), -7);
    const uint32_t sz = st == HBAM_OK ? r.size : 0;
    fwrite(&st, 4, 1, o);
    fwrite(&sz, 4, 1, o);
    fwrite(&mh, 8, 1, o);
    if (sz) fwrite(rec.data(), 1, sz, o);
    p = e + 1;
  }
  fclose(o);
  return 0;
}
