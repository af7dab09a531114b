// inflate_tok.h — Huffman pass of the batched BGZF inflate (k_inflate_tokens), gfx950.
//
// Replaces [htsjdk] BlockGunzipper.unzipBlock -> java.util.zip.Inflater (JDK zlib) on the BAM
// read path; the observable contract is zlib 1.2.11's as documented in inflate_dev.h (ONE
// inflate(Z_PARTIAL_FLUSH) call with avail_out = ISIZE; identical error conditions).
//
// One lane decodes one BGZF block (SIMT over 64 blocks per wave).  What makes a lane-per-
// block decoder slow on CDNA is not the bit arithmetic but memory waits: a per-lane refill
// that loads the next 16 compressed bytes when the lane runs dry puts an
// `s_waitcnt vmcnt(...)` on the critical path of EVERY loop iteration, because some lane of
// the 64 is always refilling and the wait is per wave.  Here the input moves in wave-uniform
// epochs instead:
//   * each lane holds 32 compressed bytes in two register banks and a bit cursor over them;
//   * every TOK_K iterations (the same iteration for every active lane) a lane merges
//     the 16-byte quad it requested at the previous epoch into a free bank and requests the
//     next one, so a load has a whole epoch to land before anything waits on it;
//   * a lane that would need more bits than its banks hold skips the iteration (stall) until
//     the next epoch, which only happens on runs of long, far matches.
// Output (TSink): literals at their final ubuf offsets, a 3-byte descriptor (len-3, dist-1)
// at the start of every match hole, one bitmap bit per match start (64-position windows
// written as 8-byte stores), a 16-byte register write-combine chunk for the bytes.
// k_resolve (resolve_dev.h) then fills the holes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "inflate_dev.h"

namespace hbam {

#if defined(HBAM_PROF) && !defined(HBAM_PROF_NOSTAMP)
// Profiling build only: wave-level cycles per region of the Huffman pass (tools/prof_regions.py)
#define TOK_PT(i)                                   \
  do {                                              \
    const uint64_t t_ = __builtin_amdgcn_s_memtime(); \
    pt[i] += t_ - tq;                               \
    tq = t_;                                        \
  } while (0)
#define TOK_PC(i) (++pc[i])
#else
#define TOK_PT(i) \
  do {            \
  } while (0)
#define TOK_PC(i) (void)0
#endif
// CPU model only (tools/cpu_model/tok_model.cpp): counts the symbol-loop entries per body
#ifndef TOK_BODY_ENTERED
#define TOK_BODY_ENTERED(v) (void)0
#endif
// ... and the iterations per body (0 generic, 1 specialised, 2 specialised interior)
#ifndef TOK_ITER
#define TOK_ITER(v) (void)0
#endif
// ... and of those the ones a running lane skips because its banks are short of bits (stalls)
#ifndef TOK_STALL
#define TOK_STALL(c, v) (void)0
#endif

constexpr uint32_t TOK_K = 4;  // symbol-loop iterations per input epoch (power of two)


// The fast path (tok_fast_spec): up to two literals and a match per iteration, decoded first
// (both lit/len lookups before either LDS symbol read), then written as one packet
// (TSink::put): 66.4 -> 60.3 ms at 10 GB against the same decode with one sink call per token
// (profiles/r02/s2/ab_spec_10g.txt).
// stream bits one fast-path iteration may consume: 2 lit/len codes + length extra + distance
// code + distance extra = 15+15+5+15+13 = 63 (<= 64)
constexpr uint32_t TOK_FAST_BITS = 64u;
// output bytes one fast-path iteration may produce: two literals and a match of 258
constexpr uint32_t TOK_ITER_OUT = 260u;
constexpr uint32_t TOK_LENS_LL = 32;    // lens scratch: lit/len code lengths at +32 ..
constexpr uint32_t TOK_LENS_D = 320;    //               distance code lengths at +320 (<= 30)
constexpr uint32_t TOK_LENS_END = 352;  // = LENS_SLOT (hbam_internal.h)

// ---- input: two register banks + one quad in flight ------------------------------------
typedef const __attribute__((address_space(1))) u32x4_t* gq_ptr;  // global (not flat) loads
__device__ __forceinline__ u32x4_t ein_load(const uint4* p) { return *(gq_ptr)p; }
// The reader is a bit cursor over the ring of the two banks: an iteration forms the 64 bits at
// the cursor once (ein_window: three ring dwords through shared select levels, two
// v_alignbit_b32), reads every code and extra field at an offset into that window and adds the
// offsets' sum to the cursor.  cur, fill and total count stream bits from the start of the first
// quad (bit 0 = bit 0 of the quad that holds the stream's first byte), so cur & 255 is the ring
// position and cur & 7 the phase inside the stream's byte.
struct EIn {
  const uint4* fp;    // quad held in t (merged at the next epoch); == fend when the fetch is done
  const uint4* fend;  // one past the last quad that holds stream bytes
  const uint4* safe;  // an address already read (target of the dummy load after the fetch)
  uint4 q0, q1;       // banks: stream dwords, ring positions 0..3 and 4..7
  u32x4_t t;          // quad requested at the last epoch
  uint32_t cur;       // bit cursor: the next stream bit to read
  uint32_t fill;      // fill mark: the banks hold the bits [fill - 256, fill); 128 per merged quad
  uint32_t total;     // the cursor at the end of the stream: 8 * (address & 15) + 8 * deflated bytes
};

// the two dwords of a 64-bit funnel: ((hi:lo) >> (s & 31)) & 0xffffffff, v_alignbit_b32 (a shift
// of 0 gives lo, so no guard)
__device__ __forceinline__ uint32_t ein_align(uint32_t hi, uint32_t lo, uint32_t s) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (s & 31u));
}
// The 64 stream bits at the cursor: ring dwords idx, idx + 1, idx + 2 (idx = (cur >> 5) & 7).
// (component-wise selects: a select between two uint4 lvalues becomes a select between their
// addresses, which pins the whole reader in scratch.)  The first level picks by idx & 1 inside
// each pair of neighbours and serves all three dwords: a[k] is dword 2k or 2k + 1, b[k] the one
// after it; the other two levels pick the pair.
__device__ __forceinline__ uint64_t ein_window(const EIn& e) {
  const uint32_t idx = e.cur >> 5;
  const bool o = (idx & 1u) != 0u, z = (idx & 2u) != 0u, h = (idx & 4u) != 0u;
  const uint32_t a0 = o ? e.q0.y : e.q0.x, a1 = o ? e.q0.w : e.q0.z;
  const uint32_t a2 = o ? e.q1.y : e.q1.x, a3 = o ? e.q1.w : e.q1.z;
  const uint32_t b0 = o ? e.q0.z : e.q0.y, b1 = o ? e.q1.x : e.q0.w;
  const uint32_t b2 = o ? e.q1.z : e.q1.y, b3 = o ? e.q0.x : e.q1.w;
  const uint32_t d0 = h ? (z ? a3 : a2) : (z ? a1 : a0);
  const uint32_t d1 = h ? (z ? b3 : b2) : (z ? b1 : b0);
  const uint32_t d2 = h ? (z ? a0 : a3) : (z ? a2 : a1);
  const uint32_t lo = ein_align(d1, d0, e.cur), hi = ein_align(d2, d1, e.cur);
  return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ void ein_init(EIn& e, const uint8_t* p, uint32_t nbytes) {
  const uintptr_t a = (uintptr_t)p & 15u;
  const uint4* base = (const uint4*)(p - a);
  e.fend = (const uint4*)(((uintptr_t)(p + nbytes) + 15u) & ~(uintptr_t)15u);
  e.safe = base;
  e.q0 = base[0];
  e.q1 = base[1];
  e.fp = base + 2;
  if (e.fp > e.fend) e.fp = e.fend;
  e.t = ein_load(e.fp < e.fend ? e.fp : e.safe);
  e.cur = 8u * (uint32_t)a;
  e.fill = 256u;
  e.total = e.cur + nbytes * 8u;
}
// length / distance bases without branches (DEFLATE tables as arithmetic; RFC 1951 3.2.5)
// (one formula for every code, the exceptions as constant selects: written as a select between
// two computed arms, the compiler turned the length base back into a branch)
__device__ __forceinline__ void length_base_sel(uint32_t sym, uint32_t& base, uint32_t& extra) {
  const uint32_t i = sym - 257u;  // [0, 28]
  const uint32_t ex = ((i > 4u ? i : 4u) - 4u) >> 2;  // 0 for codes 257-264
  const uint32_t b = ((4u + (i & 3u)) << ex) + 3u - (i < 4u ? 4u : 0u);
  extra = i < 28u ? ex : 0u;
  base = i < 28u ? b : 258u;
}
__device__ __forceinline__ void dist_base_sel(uint32_t d, uint32_t& base, uint32_t& extra) {
  const uint32_t ex = ((d > 2u ? d : 2u) >> 1) - 1u;  // 0 for codes 0-3
  extra = ex;
  base = ((2u + (d & 1u)) << ex) + 1u - (d < 2u ? 2u : 0u);
}
// epoch boundary: merge the quad in flight into the bank that lies wholly behind the cursor,
// request the next one.  fill grows by 128 per quad, so the bank it overwrites is (fill >> 7) & 1.
__device__ __forceinline__ void ein_epoch_merge(EIn& e) {
  if (e.fp < e.fend && e.fill - e.cur <= 128u) {
    const bool hi = (e.fill & 128u) != 0u;
    const u32x4_t t = e.t;
    e.q0.x = hi ? e.q0.x : t[0];
    e.q0.y = hi ? e.q0.y : t[1];
    e.q0.z = hi ? e.q0.z : t[2];
    e.q0.w = hi ? e.q0.w : t[3];
    e.q1.x = hi ? t[0] : e.q1.x;
    e.q1.y = hi ? t[1] : e.q1.y;
    e.q1.z = hi ? t[2] : e.q1.z;
    e.q1.w = hi ? t[3] : e.q1.w;
    e.fill += 128u;
    ++e.fp;
  }
}
__device__ __forceinline__ void ein_epoch_load(EIn& e) { e.t = ein_load(e.fp < e.fend ? e.fp : e.safe); }
__device__ __forceinline__ void ein_epoch(EIn& e) {
  ein_epoch_merge(e);
  ein_epoch_load(e);
}
// bits the lane can use without another epoch
__device__ __forceinline__ bool ein_short(const EIn& e, uint32_t need) {
  return e.fill - e.cur < need && e.fp < e.fend;
}
// synchronous top-up (header phase): epochs until `need` bits are in the banks or the fetch is done
__device__ __forceinline__ void ein_ensure(EIn& e, uint32_t need) {
  while (ein_short(e, need)) ein_epoch(e);
}
__device__ __forceinline__ uint32_t ein_avail(const EIn& e) { return e.total - e.cur; }
__device__ __forceinline__ uint32_t ein_peek(uint64_t w, uint32_t n) {
  return (uint32_t)w & ((1u << n) - 1u);
}
__device__ __forceinline__ void ein_drop(EIn& e, uint32_t n) { e.cur += n; }
// drop n bits of a window held in w as well (the careful symbol and the header phase)
__device__ __forceinline__ void ein_take(EIn& e, uint64_t& w, uint32_t n) {
  w >>= n;
  e.cur += n;
}
__device__ __forceinline__ uint32_t ein_rev15(uint64_t w) {
  return __builtin_bitreverse32((uint32_t)w) >> 17;
}

// ---- packed canonical decode tables (symbol loop) ---------------------------------------
// The lookup is the loop's largest VALU cost: 14 compares of the 15-bit code against the
// per-length limits, each feeding a length count, an index offset and (lit/len) the symbol's
// bit 8.  Pairs of limits in 16-bit halves let one v_pk_sub_u16 (clamp) + v_pk_min_u16 form
// two compare results as 0/1 halves and v_pk_mad_u16 fold them into the offsets, about half
// the instructions of the 32-bit chain.  Offsets are kept as 16-bit deltas: the sums are exact
// mod 2^16 and every valid index is < 288.
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
typedef int16_t i16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u16x2 as_u16x2(uint32_t x) { return __builtin_bit_cast(u16x2, x); }
__device__ __forceinline__ uint32_t as_u32(u16x2 x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ uint32_t pk2(uint32_t lo, uint32_t hi) { return (lo & 0xffffu) | hi << 16; }
struct HuffP {
  uint32_t lim[7];  // (lim[2j], lim[2j+1]) as u16 halves
  uint32_t dof[7];  // (doff[2j+1], doff[2j+2])
  uint32_t dhl[7];  // lit/len: (hlim[2j+1] - hlim[2j], hlim[2j+2] - hlim[2j+1])
  uint32_t lim14;   // v < lim14 <=> v starts a valid code
  uint32_t o0;      // doff[0]
  uint32_t t0;      // hlim[0]
};
__device__ __forceinline__ void huffp_make(const Huff& h, HuffP& p) {
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    p.lim[j] = pk2(h.lim[2 * j], h.lim[2 * j + 1]);
    p.dof[j] = pk2((uint32_t)h.doff[2 * j + 1], (uint32_t)h.doff[2 * j + 2]);
    p.dhl[j] = pk2(h.hlim[2 * j + 1] - h.hlim[2 * j], h.hlim[2 * j + 2] - h.hlim[2 * j + 1]);
  }
  p.lim14 = h.lim[14];
  p.o0 = (uint32_t)h.doff[0];
  p.t0 = h.hlim[0];
}
// code length / symbol index (/ bit 8 of a lit/len symbol) of a left-justified 15-bit value;
// false: no code starts with v
// Per pair j (inline VOP3P, one asm statement per group of pairs: written as vector C, LLVM
// turns min(sub_sat) back into per-half compares and selects, and separate asm statements
// each cost a hazard s_nop):
//   g  = min(sat(v+1 - lim_j), 1)   the two "v >= lim" bits as 0/1 halves
//   sl += g;  so += g * dof_j;  st += g * dhl_j
// v_dot2_u32_u16 folds both halves into one u32 accumulator per pair, so the sums need no
// final (x & 0xffff) + (x >> 16) step (offsets stay exact mod 2^16: results are masked)
#define HBAM_PK_PAIR(LIM, DOF, DHL)                 \
  "v_pk_sub_u16 %[g], %[vv], " LIM " clamp\n\t"     \
  "v_pk_min_u16 %[g], %[g], %[one]\n\t"              \
  "v_dot2_u32_u16 %[sl], %[g], %[one], %[sl]\n\t"    \
  "v_dot2_u32_u16 %[so], %[g], " DOF ", %[so]\n\t"   \
  "v_dot2_u32_u16 %[st], %[g], " DHL ", %[st]\n\t"
#define HBAM_PK_PAIR_NT(LIM, DOF)                   \
  "v_pk_sub_u16 %[g], %[vv], " LIM " clamp\n\t"     \
  "v_pk_min_u16 %[g], %[g], %[one]\n\t"              \
  "v_dot2_u32_u16 %[sl], %[g], %[one], %[sl]\n\t"    \
  "v_dot2_u32_u16 %[so], %[g], " DOF ", %[so]\n\t"
// Two pairs at a time with two compare registers: the sub -> min -> dot2 chain of one pair has the
// other pair's instructions between its links instead of stalling on them (A/B at 5 GB: Huffman
// 34.1 -> 33.8 ms, same output; profiles/r05/ab/pools_windows_tok_ilv_5g.txt).
#define HBAM_PK2_PAIR(LA, DA, TA, LB, DB, TB)          \
  "v_pk_sub_u16 %[g], %[vv], " LA " clamp\n\t"        \
  "v_pk_sub_u16 %[h], %[vv], " LB " clamp\n\t"        \
  "v_pk_min_u16 %[g], %[g], %[one]\n\t"               \
  "v_pk_min_u16 %[h], %[h], %[one]\n\t"               \
  "v_dot2_u32_u16 %[sl], %[g], %[one], %[sl]\n\t"     \
  "v_dot2_u32_u16 %[so], %[g], " DA ", %[so]\n\t"     \
  "v_dot2_u32_u16 %[st], %[g], " TA ", %[st]\n\t"     \
  "v_dot2_u32_u16 %[sl], %[h], %[one], %[sl]\n\t"     \
  "v_dot2_u32_u16 %[so], %[h], " DB ", %[so]\n\t"     \
  "v_dot2_u32_u16 %[st], %[h], " TB ", %[st]\n\t"
#define HBAM_PK2_PAIR_NT(LA, DA, LB, DB)               \
  "v_pk_sub_u16 %[g], %[vv], " LA " clamp\n\t"        \
  "v_pk_sub_u16 %[h], %[vv], " LB " clamp\n\t"        \
  "v_pk_min_u16 %[g], %[g], %[one]\n\t"               \
  "v_pk_min_u16 %[h], %[h], %[one]\n\t"               \
  "v_dot2_u32_u16 %[sl], %[g], %[one], %[sl]\n\t"     \
  "v_dot2_u32_u16 %[so], %[g], " DA ", %[so]\n\t"     \
  "v_dot2_u32_u16 %[sl], %[h], %[one], %[sl]\n\t"     \
  "v_dot2_u32_u16 %[so], %[h], " DB ", %[so]\n\t"
// Specialised pair ranges [P0, P1) (tok_symbols picks them per wave from tok_build's TOK_FIT_* bits):
//   P0 = 1: the code has no length 1 or 2, so lim[0] == lim[1] == 0 and pair 0 always gives g = (1,1);
//           its sums are per-lane constants, folded into o0 / t0 by huffp_fold and into the length base here;
//   P1 < 7: the code is complete with no length above 2 * P1 - 1, so every limit from pair P1 on is 32768
//           and its compares never hold.
// A specialised range is only ever given a complete code, where v < lim14 (== 32768) always holds.
template <bool HI, int P0 = 0, int P1 = 7>
__device__ __forceinline__ bool huffp_lookup(const HuffP& h, uint32_t v, uint32_t& L, uint32_t& idx,
                                             uint32_t& hi) {
  constexpr bool ALL = P0 == 0 && P1 == 7;
  static_assert(ALL || (HI && P0 == 1 && P1 == 7) || (!HI && P0 == 1 && P1 == 5),
                "huffp_lookup: pair range without an instruction sequence");
  const uint32_t vv = (v + 1u) * 0x10001u;  // v + 1 <= 32768 in both halves
  const uint32_t one = 0x10001u;
  uint32_t sl = 0, so = 0, st = 0, g;
  uint32_t g2;
  if (HI && !ALL) {  // lit/len, pairs 1..6
    asm(HBAM_PK2_PAIR("%[l1]", "%[d1]", "%[t1]", "%[l2]", "%[d2]", "%[t2]")
        HBAM_PK2_PAIR("%[l3]", "%[d3]", "%[t3]", "%[l4]", "%[d4]", "%[t4]")
        : [sl] "+v"(sl), [so] "+v"(so), [st] "+v"(st), [g] "=&v"(g), [h] "=&v"(g2)
        : [vv] "v"(vv), [one] "v"(one), [l1] "v"(h.lim[1]), [l2] "v"(h.lim[2]), [l3] "v"(h.lim[3]),
          [l4] "v"(h.lim[4]), [d1] "v"(h.dof[1]), [d2] "v"(h.dof[2]), [d3] "v"(h.dof[3]),
          [d4] "v"(h.dof[4]), [t1] "v"(h.dhl[1]), [t2] "v"(h.dhl[2]), [t3] "v"(h.dhl[3]),
          [t4] "v"(h.dhl[4]));
    asm(HBAM_PK2_PAIR("%[l5]", "%[d5]", "%[t5]", "%[l6]", "%[d6]", "%[t6]")
        : [sl] "+v"(sl), [so] "+v"(so), [st] "+v"(st), [g] "=&v"(g), [h] "=&v"(g2)
        : [vv] "v"(vv), [one] "v"(one), [l5] "v"(h.lim[5]), [l6] "v"(h.lim[6]), [d5] "v"(h.dof[5]),
          [d6] "v"(h.dof[6]), [t5] "v"(h.dhl[5]), [t6] "v"(h.dhl[6]));
  } else if (!ALL) {  // distance, pairs 1..4
    asm(HBAM_PK2_PAIR_NT("%[l1]", "%[d1]", "%[l2]", "%[d2]") HBAM_PK2_PAIR_NT("%[l3]", "%[d3]", "%[l4]", "%[d4]")
        : [sl] "+v"(sl), [so] "+v"(so), [g] "=&v"(g), [h] "=&v"(g2)
        : [vv] "v"(vv), [one] "v"(one), [l1] "v"(h.lim[1]), [l2] "v"(h.lim[2]), [l3] "v"(h.lim[3]),
          [l4] "v"(h.lim[4]), [d1] "v"(h.dof[1]), [d2] "v"(h.dof[2]), [d3] "v"(h.dof[3]),
          [d4] "v"(h.dof[4]));
  } else if (HI) {
    asm(HBAM_PK2_PAIR("%[l0]", "%[d0]", "%[t0]", "%[l1]", "%[d1]", "%[t1]")
        HBAM_PK2_PAIR("%[l2]", "%[d2]", "%[t2]", "%[l3]", "%[d3]", "%[t3]")
        : [sl] "+v"(sl), [so] "+v"(so), [st] "+v"(st), [g] "=&v"(g), [h] "=&v"(g2)
        : [vv] "v"(vv), [one] "v"(one), [l0] "v"(h.lim[0]), [l1] "v"(h.lim[1]), [l2] "v"(h.lim[2]),
          [l3] "v"(h.lim[3]), [d0] "v"(h.dof[0]), [d1] "v"(h.dof[1]), [d2] "v"(h.dof[2]),
          [d3] "v"(h.dof[3]), [t0] "v"(h.dhl[0]), [t1] "v"(h.dhl[1]), [t2] "v"(h.dhl[2]),
          [t3] "v"(h.dhl[3]));
    asm(HBAM_PK2_PAIR("%[l4]", "%[d4]", "%[t4]", "%[l5]", "%[d5]", "%[t5]")
        HBAM_PK_PAIR("%[l6]", "%[d6]", "%[t6]")
        : [sl] "+v"(sl), [so] "+v"(so), [st] "+v"(st), [g] "=&v"(g), [h] "=&v"(g2)
        : [vv] "v"(vv), [one] "v"(one), [l4] "v"(h.lim[4]), [l5] "v"(h.lim[5]), [l6] "v"(h.lim[6]),
          [d4] "v"(h.dof[4]), [d5] "v"(h.dof[5]), [d6] "v"(h.dof[6]), [t4] "v"(h.dhl[4]),
          [t5] "v"(h.dhl[5]), [t6] "v"(h.dhl[6]));
  } else {
    asm(HBAM_PK2_PAIR_NT("%[l0]", "%[d0]", "%[l1]", "%[d1]") HBAM_PK2_PAIR_NT("%[l2]", "%[d2]", "%[l3]", "%[d3]")
        HBAM_PK2_PAIR_NT("%[l4]", "%[d4]", "%[l5]", "%[d5]") HBAM_PK_PAIR_NT("%[l6]", "%[d6]")
        : [sl] "+v"(sl), [so] "+v"(so), [g] "=&v"(g), [h] "=&v"(g2)
        : [vv] "v"(vv), [one] "v"(one), [l0] "v"(h.lim[0]), [l1] "v"(h.lim[1]), [l2] "v"(h.lim[2]),
          [l3] "v"(h.lim[3]), [l4] "v"(h.lim[4]), [l5] "v"(h.lim[5]), [l6] "v"(h.lim[6]),
          [d0] "v"(h.dof[0]), [d1] "v"(h.dof[1]), [d2] "v"(h.dof[2]), [d3] "v"(h.dof[3]),
          [d4] "v"(h.dof[4]), [d5] "v"(h.dof[5]), [d6] "v"(h.dof[6]));
  }
  const uint32_t l = 1u + 2u * (uint32_t)P0 + sl;
  L = l;
  idx = (h.o0 + so + (v >> (15u - l))) & 0xffffu;
  if (HI) hi = v >= ((h.t0 + st) & 0xffffu) ? 256u : 0u;
  return ALL ? v < h.lim14 : true;
}
// the table a lookup with P0 = 1 takes: pair 0's constant sums (g = (1,1)) moved into o0 and t0
__device__ __forceinline__ HuffP huffp_fold(const HuffP& p) {
  HuffP f = p;
  f.o0 = p.o0 + (p.dof[0] & 0xffffu) + (p.dof[0] >> 16);
  f.t0 = p.t0 + (p.dhl[0] & 0xffffu) + (p.dhl[0] >> 16);
  return f;
}

// ---- output ------------------------------------------------------------------------------
struct TSink {
  uint8_t* cbase;   // 16-aligned address of chunk 0 (the chunk holding the block's first byte)
  uint32_t soff;    // block start inside chunk 0
  uint32_t iend;    // soff + isize
  uint32_t curc;    // chunk held in lo/hi (0 at the start: the block's first byte is in chunk 0)
  uint64_t lo, hi;
  uint32_t* bm;     // match-start bitmap of the block (BITMAP_WORDS words)
  uint32_t bwin;    // 64-position window held in wl
  uint32_t nwin;    // windows covering the block (an even count: k_resolve_units reads 128 positions at a time)
  uint64_t wl;
  uint32_t* tail;   // [0] = op | n<<16 | 1<<31 for a final match shorter than 3 bytes, [1] = dist
  uint32_t t0, t1;  // tail[0..1], stored by finish() (a store behind a branch in the loop cost
                    // every iteration its exec-mask bookkeeping; with the unconditional chunk 0
                    // and the 64-bit bitmap words: Huffman 32.5 -> 31.0 ms at 5 GB, same output,
                    // profiles/r05/ab/huffman_sink_tail_mark_5g.txt)
  uint8_t* edge;    // 32 B: the block's partial first / last 16-byte chunk (k_edge_merge)
  uint8_t* cdst;    // where the chunk in lo/hi goes when the symbol loop leaves it (flush_cur)

  __device__ __forceinline__ void init(uint8_t* ubuf, uint64_t start, uint32_t isize, uint32_t* bmp,
                                       uint32_t* tl, uint8_t* eg) {
    edge = eg;
    cbase = ubuf + (start & ~15ull);
    soff = (uint32_t)(start & 15u);
    iend = soff + isize;
    curc = 0;  // (a flush before any output writes zeros to the block's own chunk 0 / edge slot)
    cdst = soff != 0u ? edge : cbase;
    lo = hi = 0;
    bm = bmp;
    bwin = 0;
    nwin = ((isize + 127u) >> 7) * 2u;
    wl = 0;
    tail = tl;
    t0 = t1 = 0;
  }
  __device__ __forceinline__ void flush() {
    const uint32_t r0 = curc << 4;
    // A chunk shared with a neighbouring block (the block's first chunk when it does not
    // start 16-aligned, its last when it does not end so) goes to the block's edge slot
    // instead, whole; k_edge_merge writes this block's bytes of it afterwards.  So every flush
    // is one 16-byte store and the loop carries no byte-store fallback.
    const bool full = r0 >= soff && r0 + 16u <= iend;
    uint8_t* dst = full ? cbase + r0 : edge + (r0 < soff ? 0u : 16u);
    st_out((uint4*)dst, make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)));
  }
  // A chunk the block leaves for a later one is never its last: it is chunk 0 (the edge slot when
  // the block does not start 16-aligned) or a whole chunk of its own, and cdst says which, set
  // when the chunk was entered.  Only finish() flushes the last chunk and needs flush()'s test.
  __device__ __forceinline__ void flush_cur() {
    st_out((uint4*)cdst, make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)));
  }
  __device__ __forceinline__ void enter_if(bool sw, uint32_t c) {
    uint8_t* const d = cbase + ((uint64_t)c << 4);
    cdst = sw ? d : cdst;
  }
  __device__ __forceinline__ void chunk(uint32_t c) {
    if (c != curc) {
      flush();
      enter_if(true, c);
      curc = c;
      lo = 0;
      hi = 0;
    }
  }
  // One 64-bit word per 64 positions, stored as 8 bytes (the bitmap in memory is what it was when
  // the window was 128 positions in two words and a 16-byte store; one word halves the selects of
  // mark_if, and the store rides in a side block the wave enters in nearly every iteration anyway).
  __device__ __forceinline__ void win_store() { *(uint64_t*)(bm + 2u * bwin) = wl; }
  __device__ __forceinline__ void mark(uint32_t op) { mark_if(true, op); }
  // the match-start bit of op when em: the bit as selects, only the window store behind a branch
  __device__ __forceinline__ void mark_if(bool em, uint32_t op) {
    const uint32_t w = op >> 6;
    if (em && bwin < w) {
      win_store();
      wl = 0;
      ++bwin;
      while (bwin < w) {  // a match longer than the window: zero windows
        win_store();
        ++bwin;
      }
    }
    wl |= em ? 1ull << (op & 63u) : 0ull;
  }
  __device__ __forceinline__ void literal(uint32_t op, uint32_t b) {
    const uint32_t r = soff + op;
    chunk(r >> 4);
    const uint64_t v = (uint64_t)(b & 0xffu) << ((r & 7u) << 3);
    if (r & 8u) hi |= v;
    else lo |= v;
  }
  __device__ __forceinline__ void match(uint32_t op, uint32_t n, uint32_t dist) {
    if (n < 3u) {  // the output filled up inside the match: last token of the block
      t0 = op | n << 16 | 0x80000000u;
      t1 = dist;
      return;
    }
    const uint64_t d = (uint64_t)((n - 3u) | (dist - 1u) << 8);  // 3 bytes
    const uint32_t r = soff + op;
    const uint32_t c = r >> 4, k = r & 15u;
    chunk(c);
    if (k < 8u) {
      lo |= d << (8u * k);
      if (k > 5u) hi |= d >> (64u - 8u * k);
    } else {
      hi |= d << (8u * (k - 8u));  // bytes past the chunk (k >= 14) fall off here ...
    }
    if (k >= 14u) {  // ... and start the next chunk
      const uint64_t spill = d >> (8u * (16u - k));
      flush();
      enter_if(true, c + 1u);
      curc = c + 1u;
      lo = spill;
      hi = 0;
    }
    mark(op);
  }
  // chunk switch as a predicated step: only the flush (a store) sits behind a branch
  __device__ __forceinline__ void switch_if(bool sw, uint32_t c) {
    if (sw) flush_cur();
    enter_if(sw, c);
    curc = sw ? c : curc;
    lo = sw ? 0ull : lo;
    hi = sw ? 0ull : hi;
  }
  // One iteration's output as one packet: nb (<= 5) bytes P (LSB first) at ubuf position
  // soff + op: up to two literals and a 3-byte match descriptor, always contiguous, so one
  // chunk switch and at most one spill into the next chunk (tok_fast_spec).
  __device__ __forceinline__ void put(uint32_t op, uint64_t P, uint32_t nb) {
    const bool any = nb != 0u;
    const uint32_t r = soff + op;
    const uint32_t c = r >> 4, k = r & 15u;
    switch_if(any && c != curc, c);
    // shift amounts below 64 in every select arm (P < 2^40: at most 5 bytes)
    const uint32_t kl = k < 8u ? k : 0u, kh = k < 8u ? 0u : k - 8u;
    const uint32_t kr = (k > 1u && k < 8u) ? 64u - 8u * k : 8u;
    lo |= k < 8u ? P << (8u * kl) : 0ull;
    hi |= (k > 1u && k < 8u) ? P >> kr : 0ull;
    hi |= k < 8u ? 0ull : P << (8u * kh);
    const bool sp = any && k + nb > 16u;
    if (sp) flush_cur();
    enter_if(sp, c + 1u);
    const uint64_t spill = P >> (8u * (16u - (k >= 10u ? k : 10u)));
    curc = sp ? c + 1u : curc;
    lo = sp ? spill : lo;
    hi = sp ? 0ull : hi;
  }
  __device__ __forceinline__ void finish() {
    flush();
    tail[0] = t0;
    tail[1] = t1;
    while (bwin < nwin) {
      win_store();
      wl = 0;
      ++bwin;
    }
  }
};

// ---- canonical tables from code lengths in global scratch ---------------------------------
// lens: 16-aligned global bytes (n of them); kind 0 = code lengths, 1 = lit/len, 2 = distances.
// The lengths are read 16 at a time, the next quad requested before the current one is
// processed (one wait per 16 symbols instead of one per symbol).
__device__ __forceinline__ uint32_t quad_byte(const uint4& q, uint32_t j) {  // j compile-time
  const uint32_t w = j < 4 ? q.x : j < 8 ? q.y : j < 12 ? q.z : q.w;
  return (w >> (8u * (j & 3u))) & 0xffu;
}
// Returns 0 for a set zlib rejects, else TOK_BUILT plus what a specialised symbol loop may rely on:
//   TOK_FIT_FULL  the code is complete (so lim[14] == 32768: every 15-bit value starts a code);
//   TOK_FIT_LOW   ... and has no code of length 1 or 2 (lim[0] == lim[1] == 0);
//   TOK_FIT_M11   ... and none longer than 11 (lim[10 ..] == 32768).
// The incomplete-but-legal sets (a single distance code, no distance code) get none of them.
constexpr uint32_t TOK_BUILT = 1u, TOK_FIT_FULL = 2u, TOK_FIT_LOW = 4u, TOK_FIT_M11 = 8u;
constexpr uint32_t TOK_FIT_MAXL = 8u;  // ... and from this bit on the longest code length of the set (0..15)
// Out of line: called once per DEFLATE block, and inlining its unrolled counters into the
// kernel pushes the symbol loop's state into scratch.
__device__ __attribute__((noinline)) uint32_t tok_build(const uint8_t* __restrict__ lens, int n,
                                                        uint8_t* __restrict__ syms, Huff& h, int kind) {
  typedef uint8_t SymT;
  const uint4* lq = (const uint4*)lens;
  const int nq = (n + 15) >> 4;
  uint32_t cnt[16], nhi[16];
#pragma unroll
  for (int L = 0; L < 16; ++L) cnt[L] = nhi[L] = 0;
  uint4 qn = lq[0];
  for (int k = 0; k < nq; ++k) {
    const uint4 q = qn;
    if (k + 1 < nq) qn = lq[k + 1];
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
      const int s = 16 * k + (int)j;
      const uint32_t len = s < n ? quad_byte(q, j) : 0u;
      const uint32_t hb = (kind == 1 && s >= 256) ? 1u : 0u;
#pragma unroll
      for (int L = 1; L < 16; ++L) {
        cnt[L] += (len == (uint32_t)L) ? 1u : 0u;
        nhi[L] += (len == (uint32_t)L) ? hb : 0u;
      }
    }
  }
  uint32_t maxl = 0;
#pragma unroll
  for (int L = 1; L < 16; ++L) maxl = cnt[L] ? (uint32_t)L : maxl;
  h.empty = (maxl == 0);
  uint32_t fit = TOK_BUILT;
  if (maxl != 0) {
    int32_t left = 1;
    bool over = false;
#pragma unroll
    for (int L = 1; L < 16; ++L) {
      left = 2 * left - (int32_t)cnt[L];
      over |= left < 0;
    }
    if (over) return 0u;
    if (left > 0 && (kind == 0 || maxl != 1)) return 0u;  // incomplete set
    if (left == 0) {
      fit |= TOK_FIT_FULL;
      fit |= (cnt[1] | cnt[2]) == 0u ? TOK_FIT_LOW : 0u;
      fit |= maxl <= 11u ? TOK_FIT_M11 : 0u;
    }
  }
  uint32_t code = 0, base = 0;
  uint32_t next[16];
  int32_t prev_off = 0;
#pragma unroll
  for (int L = 1; L < 16; ++L) {
    h.lim[L - 1] = (code + cnt[L]) << (15 - L);
    h.hlim[L - 1] = (code + cnt[L] - nhi[L]) << (15 - L);
    const int32_t off = (int32_t)base - (int32_t)code;
    h.doff[L - 1] = off - prev_off;
    prev_off = off;
    next[L] = base;
    base += cnt[L];
    code = (code + cnt[L]) << 1;
  }
  if (maxl == 0) {
#pragma unroll
    for (int L = 0; L < 15; ++L) h.lim[L] = h.hlim[L] = 0;
  }
  qn = lq[0];
  for (int k = 0; k < nq; ++k) {
    const uint4 q = qn;
    if (k + 1 < nq) qn = lq[k + 1];
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
      const int s = 16 * k + (int)j;
      const uint32_t len = s < n ? quad_byte(q, j) : 0u;
      if (len) {
        uint32_t pos = 0;
#pragma unroll
        for (int L = 1; L < 16; ++L) {
          const bool eq = (len == (uint32_t)L);
          pos = eq ? next[L] : pos;
          next[L] += eq ? 1u : 0u;
        }
        syms[pos] = (SymT)s;
      }
    }
  }
  return fit | maxl << TOK_FIT_MAXL;
}

// One iteration of the symbol loop with >= 64 stream bits left: two lit/len codes + length
// extra + distance code + distance extra (15+15+5+15+13) fit, so zlib's end-of-input outcomes
// cannot occur and none is checked.  The caller has seen to it that the banks hold what the
// block's tables can make an iteration read (tok_epoch's `need`); the one window's bits past that
// may be stale, and only fields that turn out unused (the second lookup after a length symbol,
// the distance lookup after a literal) ever look at them.  A literal is followed by a second lit/len decode in the same iteration (the wave pays for the match path once per
// iteration either way, and most symbols are literals).  Every lane runs the whole iteration
// and flags say which of its results count (SIMT runs the union of the paths anyway); the
// first exit code a lane meets wins, as zlib's early returns.  Both lit/len lookups run before
// either symbol read (the second on the bits after the first code, whether or not it turns out
// to be used), so the two LDS reads are in flight together; the iteration's bytes (up to two
// literals and a match descriptor, contiguous) go to the sink as one packet.
// Returns 0 next, 1 end of block, 2 output full (zlib stops), 3 data error.
// An iteration's packet and match mark are handed to the next iteration (TPend), which writes
// them while its own symbol reads are in flight (the packet after the two lit/len reads, the mark
// after the distance read); whether a symbol is a literal comes from the code's bit 8 (huffp_lookup's
// hi), not from the LDS byte.  Each LDS round trip costs a wave ~100 cycles of its ~3.3 k-cycle
// iteration (a probe with every symbol read doubled into two dependent reads: Huffman 30.4 ->
// 32.5 ms at 5 GB); with the writes in the shadow of the reads: 30.95 / 31.15 -> 30.10 / 30.10 ms,
// same output (profiles/r06/ab/huffman_deferred_packet_5g.txt).
struct TPend {
  uint64_t P;
  uint32_t op1, nb, opm;
  bool em;
  __device__ __forceinline__ void clear() {
    P = 0;
    op1 = nb = opm = 0;
    em = false;
  }
  __device__ __forceinline__ void flush(TSink& sink) {
    sink.put(op1, P, nb);
    sink.mark_if(em, opm);
    P = 0;  // put ORs P in whatever nb says
    nb = 0;
    em = false;
  }
};
// SPEC: the specialised lookups (lit/len pairs 1..6, distance pairs 1..4) on tables folded by
// huffp_fold; they return a constant true (a complete code), so the ok1 / ok2 / okd tests and the
// selects that hang off them fold away.
// INTERIOR (with SPEC): the caller guarantees op + TOK_ITER_OUT <= isize, so the output cannot fill
// up in this iteration: no `op == isize` test, the match is never cut short (n == mlen, no tail
// token, never exit code 2).
template <bool SPEC, bool INTERIOR = false>
__device__ __forceinline__ uint32_t tok_fast_spec(EIn& in, const HuffP& hl, const HuffP& hd,
                                                  const uint8_t* __restrict__ syms_ll,
                                                  const uint8_t* __restrict__ syms_d, TSink& sink,
                                                  uint32_t& op, uint32_t isize, TPend& pd) {
  const uint64_t w = ein_window(in);  // the iteration's <= 63 bits, read at the running offset `off`
  uint32_t L1, idx1, hi1 = 0, L2, idx2, hi2 = 0;
  const bool ok1 = huffp_lookup<true, SPEC ? 1 : 0, 7>(hl, ein_rev15(w), L1, idx1, hi1);
  const uint32_t l1 = ok1 ? L1 : 0u;
  const bool ok2 = huffp_lookup<true, SPEC ? 1 : 0, 7>(hl, ein_rev15(w >> l1), L2, idx2, hi2);
  const uint32_t sym1 = (uint32_t)syms_ll[ok1 ? idx1 : 0u] | hi1;
  const uint32_t sym2 = (uint32_t)syms_ll[ok2 ? idx2 : 0u] | hi2;
  sink.put(pd.op1, pd.P, pd.nb);  // the previous iteration's packet
  uint32_t ex = ok1 ? 0u : 3u;
  uint32_t off = l1;
  const bool lit1 = ok1 && hi1 == 0u;
  if (!INTERIOR) ex = (ex == 0u && lit1 && op == isize) ? 2u : ex;
  const bool emit1 = ex == 0u && lit1;
  const uint32_t op1 = op;
  op += emit1 ? 1u : 0u;
  ex = (emit1 && !ok2) ? 3u : ex;
  off += (emit1 && ok2) ? L2 : 0u;
  const bool lit2 = emit1 && ok2 && hi2 == 0u;
  if (!INTERIOR) ex = (ex == 0u && lit2 && op == isize) ? 2u : ex;
  const bool emit2 = ex == 0u && lit2;
  op += emit2 ? 1u : 0u;
  const uint32_t m = emit1 ? sym2 : sym1;
  const bool ism = ex == 0u && !emit2 && !lit2;
  ex = (ism && m == 256u) ? 1u : ex;
  ex = (ism && m > 285u) ? 3u : ex;
  const bool dom = ism && m > 256u && m <= 285u;
  uint32_t lbase, lext;
  length_base_sel(dom ? m : 257u, lbase, lext);
  lext = dom ? lext : 0u;
  const uint32_t mlen = lbase + ein_peek(w >> off, lext);
  off += lext;
  uint32_t L, idx, dh;
  const bool okd = huffp_lookup<false, SPEC ? 1 : 0, SPEC ? 5 : 7>(hd, ein_rev15(w >> off), L, idx, dh);
  const uint32_t dsym = syms_d[okd ? idx : 0u];
  sink.mark_if(pd.em, pd.opm);  // the previous iteration's match mark
  ex = (dom && !okd) ? 3u : ex;
  off += (dom && okd) ? L : 0u;
  ex = (dom && okd && dsym > 29u) ? 3u : ex;
  const bool dom2 = dom && ex == 0u;
  uint32_t dbase, dext;
  dist_base_sel(dom2 ? dsym : 0u, dbase, dext);
  dext = dom2 ? dext : 0u;
  const uint32_t dist = dbase + ein_peek(w >> off, dext);
  ein_drop(in, off + dext);
  if (!INTERIOR) ex = (dom2 && op == isize) ? 2u : ex;
  ex = (dom2 && ex == 0u && dist > op) ? 3u : ex;
  const bool domatch = dom2 && ex == 0u;
  uint32_t n = mlen;
  bool em = domatch;
  if (!INTERIOR) {
    n = isize - op;
    n = mlen < n ? mlen : n;
    const bool last = domatch && n < 3u;  // the output filled up inside the match: last token
    sink.t0 = last ? (op | n << 16 | 0x80000000u) : sink.t0;
    sink.t1 = last ? dist : sink.t1;
    em = domatch && n >= 3u;
  }
  uint64_t P = emit1 ? (uint64_t)(sym1 & 0xffu) : 0ull;
  P |= emit2 ? (uint64_t)(sym2 & 0xffu) << 8 : 0ull;
  const uint32_t nl = (emit1 ? 1u : 0u) + (emit2 ? 1u : 0u);
  P |= em ? (uint64_t)((n - 3u) | (dist - 1u) << 8) << (8u * nl) : 0ull;
  pd.op1 = op1;
  pd.P = P;
  pd.nb = nl + (em ? 3u : 0u);
  pd.em = em;
  pd.opm = op;
  op += domatch ? n : 0u;
  if (!INTERIOR) ex = (domatch && n < mlen) ? 2u : ex;
  return ex;
}
// One symbol with every zlib outcome checked (the stream's last 64 bits).
__device__ __forceinline__ uint32_t tok_careful(EIn& in, const HuffP& hl, const HuffP& hd,
                                                const uint8_t* __restrict__ syms_ll,
                                                const uint8_t* __restrict__ syms_d, TSink& sink,
                                                uint32_t& op, uint32_t isize) {
  // one window serves the symbol: 15 + 5 + 15 + 13 = 48 bits at most
  uint64_t w = ein_window(in);
  uint32_t L, idx, hi = 0;
  if (!huffp_lookup<true>(hl, ein_rev15(w), L, idx, hi)) return ein_avail(in) >= 1u ? 3u : 2u;
  if (L > ein_avail(in)) return 2u;
  const uint32_t sym = (uint32_t)syms_ll[idx] | hi;
  ein_take(in, w, L);
  if (sym < 256u) {
    if (op == isize) return 2u;
    sink.literal(op++, sym);
    return 0u;
  }
  if (sym == 256u) return 1u;
  if (sym > 285u) return 3u;
  uint32_t lbase, lext;
  length_base(sym, lbase, lext);
  if (lext > ein_avail(in)) return 2u;
  const uint32_t mlen = lbase + ein_peek(w, lext);
  ein_take(in, w, lext);
  uint32_t dh;
  if (!huffp_lookup<false>(hd, ein_rev15(w), L, idx, dh)) return ein_avail(in) >= 1u ? 3u : 2u;
  if (L > ein_avail(in)) return 2u;
  const uint32_t dsym = syms_d[idx];
  ein_take(in, w, L);
  if (dsym > 29u) return 3u;
  uint32_t dbase, dext;
  dist_base(dsym, dbase, dext);
  if (dext > ein_avail(in)) return 2u;
  const uint32_t dist = dbase + ein_peek(w, dext);
  ein_drop(in, dext);
  if (op == isize) return 2u;
  if (dist > op) return 3u;
  uint32_t n = isize - op;
  n = mlen < n ? mlen : n;
  sink.match(op, n, dist);
  op += n;
  return n < mlen ? 2u : 0u;
}

// The symbol loop's input step: every TOK_K-th iteration is the wave's epoch.  A bank is 128 bits and
// comes free only as a whole, so a lane that could not merge at an epoch may hold as few as 129
// bits, and three wide iterations can use them up before the next epoch: such a lane skips
// iterations until then (the stall rule).  `need` is what one iteration can read with the block's
// tables (inflate_tokens_block), not the 64 bits of the widest tables: on the eight generated
// bodies a lane then skips 0.13 % of its interior iterations (0.30 % with 64).  Giving the short
// lane an epoch of its own in the iteration in which it runs short skips none, but was measured
// 1 ms slower at 10 GB than letting it wait: the epoch block, with its wait for the wave's
// outstanding memory operations, then runs whenever one lane of the 64 is short, far more often
// than every fourth iteration (profiles/huffman_window/model_iterations.txt, ab.txt section 2).
__device__ __forceinline__ void tok_epoch(EIn& in, uint32_t& it, uint32_t ex, uint32_t need, int body) {
  if ((__builtin_amdgcn_readfirstlane(++it) & (TOK_K - 1u)) == 0u) ein_epoch(in);
  TOK_STALL(ex == 0u && ein_short(in, need), body);
}

// The symbol loop of one Huffman-coded DEFLATE block; returns the lane's exit code (1 end of block,
// 2 leave (zlib stops), 3 data error).  SPEC: every lane that enters has complete lit/len and
// distance codes without lengths 1 and 2 and no distance code longer than 11 bits (tok_build's
// TOK_FIT_* bits), which is what BAM bodies at zlib's default levels give (profiles/
// huffman_length_ranges/ranges.txt): the fast path then runs the shorter lookups (tok_fast_spec).
// The careful symbol keeps the generic lookup on the unfolded tables.
// Structured loops (no continue / goto inside): every path of an iteration joins at
// the loop's end with an exit code, so the decoder state needs no per-path copies.
//
// interior (wave-uniform, SPEC only; 0 with env HBAM_TOK_INTERIOR=0): the specialised loop has a
// second, shorter body for the iterations in which no running lane can reach an end: every one of
// them has >= TOK_FAST_BITS stream bits left (no careful symbol, no `fast` routing) and
// op + TOK_ITER_OUT <= isize (none of the output-full logic, tok_fast_spec<true, true>).  One ballot
// at the top of the iteration asks that; when some running lane no longer qualifies (the last 64
// bits of its stream, the last 260 bytes of its output) the wave goes on in the full body with the
// same in / op / sink / it / ex and the pending packet, and comes back once every running lane
// qualifies again (the lane that was near its end has ended, the others are mid-block).
template <bool SPEC>
__device__ __forceinline__ uint32_t tok_symbols(EIn& in, const HuffP& hl, const HuffP& hd,
                                                const uint8_t* __restrict__ syms_ll,
                                                const uint8_t* __restrict__ syms_d, TSink& sink,
                                                uint32_t& op, uint32_t isize, uint32_t& it, uint32_t interior,
                                                uint32_t need
#ifdef HBAM_PROF
                                                , uint64_t* pt, uint64_t* pc, uint64_t& tq
#endif
                                                ) {
  const HuffP fl = SPEC ? huffp_fold(hl) : hl, fd = SPEC ? huffp_fold(hd) : hd;
  uint32_t ex = 0;  // 0 next symbol, 1 end of block, 2 leave (zlib stops), 3 data error
  TPend pd;
  pd.clear();
  const bool two = SPEC && interior != 0u;
#define TOK_ANY(c) (__builtin_amdgcn_ballot_w64(c) != 0u)
#define TOK_INNER (in.total - in.cur >= TOK_FAST_BITS && op + TOK_ITER_OUT <= isize)
  for (;;) {
    if (two) {
      while (TOK_ANY(ex == 0u) && !TOK_ANY(ex == 0u && !TOK_INNER)) {
        TOK_PC(0);
        TOK_PC(4);  // of which in the interior body
        TOK_ITER(2);
#ifdef HBAM_PROF
        TOK_PT(2);
#endif
        tok_epoch(in, it, ex, need, 2);
#ifdef HBAM_PROF
        TOK_PT(0);
#endif
        if (ex == 0u && !ein_short(in, need))
          ex = tok_fast_spec<SPEC, SPEC>(in, fl, fd, syms_ll, syms_d, sink, op, isize, pd);
#ifdef HBAM_PROF
        TOK_PT(1);
#endif
      }
    }
    if (!TOK_ANY(ex == 0u)) break;
    // A wave-uniform loop (the exit is a ballot): a lane whose block has ended idles in it, as
    // it idled at the exit of a divergent loop, without the per-iteration exec-mask bookkeeping
    // of one.  The careful symbol (a lane's last 64 stream bits) runs behind a wave-uniform test.
    // With the predicated match mark and the branch-free bases: Huffman 31.1 -> 30.65 ms at
    // 5 GB, same output (profiles/r05/ab/huffman_uniform_loop_5g.txt).
    // (with the interior body it also ends once every running lane qualifies for that again)
    do {
      TOK_PC(0);
      TOK_ITER(SPEC ? 1 : 0);
#ifdef HBAM_PROF
      TOK_PT(2);
#endif
      tok_epoch(in, it, ex, need, SPEC ? 1 : 0);
#ifdef HBAM_PROF
      TOK_PT(0);  // the epoch: merge (waits for the quad in flight) + the next request
#endif
      const bool run = ex == 0u && !ein_short(in, need);
      const bool fast = in.total - in.cur >= TOK_FAST_BITS;
      if (run && fast) ex = tok_fast_spec<SPEC>(in, fl, fd, syms_ll, syms_d, sink, op, isize, pd);
      if (__builtin_amdgcn_ballot_w64(run && !fast) != 0u) {
        if (run && !fast) {
          pd.flush(sink);
          ex = tok_careful(in, hl, hd, syms_ll, syms_d, sink, op, isize);
        }
      }
#ifdef HBAM_PROF
      TOK_PT(1);
#endif
    } while (TOK_ANY(ex == 0u) && !(two && !TOK_ANY(ex == 0u && !TOK_INNER)));
  }
#undef TOK_INNER
#undef TOK_ANY
  pd.flush(sink);  // the last fast iteration's packet and mark
  return ex;
}

// Inflate one raw DEFLATE stream (cdata, nbytes) to exactly isize bytes into the token sink.
// syms_ll: 288 u8 LDS slots (symbol & 255; bit 8 from Huff.hlim); syms_d: 32 u8 LDS slots;
// lens: LENS_SLOT bytes of 16-aligned global scratch.  tok_generic (wave-uniform): never take the
// specialised symbol loop; tok_interior (wave-uniform): 0 keeps the specialised loop out of its
// interior body.  Returns INF_OK / INF_SHORT / INF_DATA.
__device__ __forceinline__ int32_t inflate_tokens_block(const uint8_t* __restrict__ cdata, uint32_t nbytes,
                                        uint32_t isize, uint8_t* __restrict__ syms_ll,
                                        uint8_t* __restrict__ syms_d, uint8_t* __restrict__ lens,
                                        TSink& sink, uint32_t* produced, uint32_t tok_generic,
                                        uint32_t tok_interior
#ifdef HBAM_PROF
                                        , uint64_t* pt, uint64_t* pc
#endif
                                        ) {
#ifdef HBAM_PROF
  uint64_t tq = __builtin_amdgcn_s_memtime();
#endif
  EIn in;
  ein_init(in, cdata, nbytes);
  uint32_t op = 0;
  HuffP hl, hd;
  uint32_t fit_ll = 0, fit_d = 0;  // tok_build's TOK_FIT_* bits of hl / hd
  bool last = false;
  int32_t rc = INF_OK;
  uint32_t it = 0;  // iteration counter shared by the lanes of a phase (epoch clock)
  for (;;) {
    if (last) break;  // stream end
    ein_ensure(in, 64);
    if (ein_avail(in) < 3u) goto leave;
    {
      const uint32_t hb = (uint32_t)ein_window(in);
      last = (hb & 1u) != 0;
      const uint32_t type = (hb >> 1) & 3u;
      ein_drop(in, 3);
      if (type == 0u) {
        // stored: byte align (the cursor counts from a 16-byte edge, so its low 3 bits are the
        // phase inside the stream's byte), LEN/NLEN, then LEN literal bytes
        const uint32_t pad = (8u - (in.cur & 7u)) & 7u;
        ein_drop(in, pad);
        ein_ensure(in, 64);
        if (ein_avail(in) < 32u) goto leave;
        const uint32_t w = (uint32_t)ein_window(in);
        if ((w & 0xffffu) != ((w >> 16) ^ 0xffffu)) { rc = INF_DATA; goto done; }
        ein_drop(in, 32);
        uint32_t len = w & 0xffffu;
        for (; len; --len) {
          if (op == isize) goto leave;
          if ((++it & (TOK_K - 1u)) == 0u) ein_epoch(in);
          if (ein_short(in, 8)) { ++len; continue; }  // stall: retry this byte next epoch
          if (ein_avail(in) < 8u) goto leave;
          sink.literal(op++, (uint32_t)ein_window(in) & 0xffu);
          ein_drop(in, 8);
        }
        continue;
      } else if (type == 1u) {
        // fixed Huffman code: lengths 8/9/7/8 for lit/len, 5 for distances
        uint32_t* l32 = (uint32_t*)(lens + TOK_LENS_LL);
        for (int s = 0; s < 288; s += 4) {
          const uint32_t v = s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u;
          l32[s / 4] = v * 0x01010101u;
        }
        uint32_t* d32 = (uint32_t*)(lens + TOK_LENS_D);
        for (int s = 0; s < 32; s += 4) d32[s / 4] = 0x05050505u;
        Huff t;
        fit_ll = tok_build(lens + TOK_LENS_LL, 288, syms_ll, t, 1);
        huffp_make(t, hl);
        fit_d = tok_build(lens + TOK_LENS_D, 32, syms_d, t, 2);
        huffp_make(t, hd);
      } else if (type == 2u) {
        ein_ensure(in, 64);
        if (ein_avail(in) < 14u) goto leave;
        const uint32_t hw = (uint32_t)ein_window(in);
        const uint32_t nlen = (hw & 31u) + 257u;
        const uint32_t ndist = ((hw >> 5) & 31u) + 1u;
        const uint32_t ncode = ((hw >> 10) & 15u) + 4u;
        ein_drop(in, 14);
        if (nlen > 286u || ndist > 30u) { rc = INF_DATA; goto done; }
        // 19 code-length code lengths (3 bits each, RFC 1951 order), at lens[0..19)
        const uint64_t ord_lo = 0x022caa324e804a30ULL, ord_hi = 0x00000003c2e1346cULL;
        {
          uint4* l4 = (uint4*)lens;
          l4[0] = make_uint4(0, 0, 0, 0);
          l4[1] = make_uint4(0, 0, 0, 0);
        }
        ein_ensure(in, 64);  // 19 * 3 = 57 bits at most: one window
        uint64_t cw = ein_window(in);
        for (uint32_t i = 0; i < ncode; ++i) {
          if (ein_avail(in) < 3u) goto leave;
          const uint32_t o = (uint32_t)((i < 12u ? ord_lo >> (5u * i) : ord_hi >> (5u * (i - 12u))) & 31u);
          lens[o] = (uint8_t)(cw & 7u);
          ein_take(in, cw, 3);
        }
        Huff hc;
        {
          Huff t;  // the build writes through a pointer; the decoder keeps its copy in registers
          if (!tok_build(lens, 19, syms_ll, t, 0)) { rc = INF_DATA; goto done; }
          hc = t;
        }
#ifdef HBAM_PROF
        TOK_PT(3);  // header bits + the code-length table
#endif
        // lit/len lengths -> lens[32 ..], distance lengths -> lens[320 ..].  The scratch is zeroed
        // first (20 quads), so a run of zero lengths (codes 17 / 18, up to 138 each) only advances
        // `have`; the loop is wave-uniform with the symbol loop's epoch clock (a per-lane clock put
        // an epoch, whose vmcnt(0) also waits for the last length's store, in nearly every
        // iteration of the divergent loop).
        const uint32_t total = nlen + ndist;
        {
          uint4* l4 = (uint4*)(lens + TOK_LENS_LL);
#pragma unroll
          for (int q = 0; q < (int)((TOK_LENS_END - TOK_LENS_LL) / 16u); ++q) l4[q] = make_uint4(0, 0, 0, 0);
        }
        uint32_t have = 0;
        uint32_t prev = 0;
        uint32_t hx = 0;  // 0 go on, 2 leave (zlib stops), 3 data error
        for (;;) {
          if ((__builtin_amdgcn_readfirstlane(++it) & (TOK_K - 1u)) == 0u) ein_epoch(in);
          const bool act = hx == 0u && have < total;
          if (__builtin_amdgcn_ballot_w64(act) == 0u) break;
          if (act && !ein_short(in, 14)) {
            const uint64_t lw = ein_window(in);  // a code (<= 7 bits) and its extra bits (<= 7)
            uint32_t L = 1, sym = 0;
            if (hc.empty) {
              hx = ein_avail(in) < 1u ? 2u : 0u;
            } else {
              int32_t idx;
              huff_lookup(hc, ein_rev15(lw), L, idx);  // CODES sets are complete
              if (L > ein_avail(in)) hx = 2u;
              else sym = syms_ll[idx];
            }
            if (hx == 0u) {
              if (sym < 16u) {
                ein_drop(in, L);
                lens[have < nlen ? TOK_LENS_LL + have : TOK_LENS_D + (have - nlen)] = (uint8_t)sym;
                ++have;
                prev = sym;
              } else {
                const uint32_t xb = sym == 16u ? 2u : sym == 17u ? 3u : 7u;
                if (L + xb > ein_avail(in)) {
                  hx = 2u;
                } else {
                  ein_drop(in, L);
                  if (sym == 16u && have == 0u) {
                    hx = 3u;
                  } else {
                    const uint64_t xw = lw >> L;
                    const uint32_t rep = sym == 16u ? 3u + ein_peek(xw, 2) : sym == 17u ? 3u + ein_peek(xw, 3)
                                                                                        : 11u + ein_peek(xw, 7);
                    ein_drop(in, xb);
                    if (have + rep > total) {
                      hx = 3u;
                    } else {
                      if (sym == 16u)  // a repeat of the previous length (3-6); zeros are already there
                        for (uint32_t k = 0; k < rep; ++k)
                          lens[have + k < nlen ? TOK_LENS_LL + have + k : TOK_LENS_D + (have + k - nlen)] = (uint8_t)prev;
                      else
                        prev = 0;
                      have += rep;
                    }
                  }
                }
              }
            }
          }
        }
        if (hx == 2u) goto leave;
        if (hx == 3u) { rc = INF_DATA; goto done; }
#ifdef HBAM_PROF
        TOK_PT(4);  // the code lengths
#endif
        if (lens[TOK_LENS_LL + 256] == 0) { rc = INF_DATA; goto done; }
        {
          Huff t;
          if (!(fit_ll = tok_build(lens + TOK_LENS_LL, (int)nlen, syms_ll, t, 1))) { rc = INF_DATA; goto done; }
          huffp_make(t, hl);
          if (!(fit_d = tok_build(lens + TOK_LENS_D, (int)ndist, syms_d, t, 2))) { rc = INF_DATA; goto done; }
          huffp_make(t, hd);
        }
#ifdef HBAM_PROF
        TOK_PT(5);  // the lit/len and distance tables
#endif
      } else {
        rc = INF_DATA;  // invalid block type
        goto done;
      }
    }
    // Drain the table copies (scratch) before the symbol loop: otherwise the loop carries
    // `s_waitcnt vmcnt(n)` on the distance tables into every iteration, which also waits for
    // the iteration's own output stores.
    __builtin_amdgcn_s_waitcnt(0);
    // ---- symbols of a Huffman-coded block: tok_symbols, in the body the wave's tables allow.
    // One ballot over the lanes that enter the loop (a lane with a stored block, a finished or a
    // failed one is not here and so has no say) and a scalar branch; nothing inside the iteration.
    TOK_PT(6);  // header + tables
    {
      // the most one iteration reads with these tables: two lit/len codes, 5 extra bits, a distance
      // code, 13 extra bits (63 at the longest codes; TOK_FAST_BITS covers every table)
      const uint32_t need = 2u * (fit_ll >> TOK_FIT_MAXL) + (fit_d >> TOK_FIT_MAXL) + 18u;
      const uint32_t fit = tok_generic ? 0u : (fit_ll & fit_d);
      const bool mine = (fit & TOK_FIT_LOW) != 0u && (fit_d & TOK_FIT_M11) != 0u;
      uint32_t ex;
#ifdef HBAM_PROF
#define TOK_SYMBOLS_ARGS in, hl, hd, syms_ll, syms_d, sink, op, isize, it, tok_interior, need, pt, pc, tq
#else
#define TOK_SYMBOLS_ARGS in, hl, hd, syms_ll, syms_d, sink, op, isize, it, tok_interior, need
#endif
      if (__builtin_amdgcn_ballot_w64(!mine) == 0u) {
        TOK_BODY_ENTERED(1);
        ex = tok_symbols<true>(TOK_SYMBOLS_ARGS);
      } else {
        TOK_BODY_ENTERED(0);
        ex = tok_symbols<false>(TOK_SYMBOLS_ARGS);
      }
#undef TOK_SYMBOLS_ARGS
      if (ex == 2u) goto leave;
      if (ex == 3u) {
        rc = INF_DATA;
        goto done;
      }
    }
  }
leave:
  rc = (op == isize) ? INF_OK : INF_SHORT;
done:
  sink.finish();
  *produced = op;
#ifdef HBAM_PROF
  // decoder state at exit (tools/diag_inflate_build.py)
  pc[1] = in.cur - 8u * ((uint32_t)(uintptr_t)cdata & 15u);  // stream bits consumed
  pc[2] = in.fill - in.cur;                                   // bits left in the banks
  pc[3] = it;
#endif
  return rc;
}

}  // namespace hbam
