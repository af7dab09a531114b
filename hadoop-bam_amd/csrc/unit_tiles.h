// unit_tiles.h — the wave loop over 16-byte units of k_sam_bulk, k_samtext_bulk and k_fragtext_bulk:
// a wave takes a tile of 64 lines, numbers the lines' units with a wave scan and gives the units to
// consecutive lanes, so a wave store covers 1 KiB of consecutive output and a 6 KB long read is the
// whole wave's work.  Device only (wave_scan_dpp, resolve_dev.h).  gfx950, wave64.
#pragma once

namespace hbam {

// count(line) -> the units of the lane's line (0 past n); its payload stays in the kernel's registers
// publish(lane)  the payload into the kernel's own LDS arrays, slot `lane` of this wave
// unit(t, r, k)  unit k of line r of tile t: load, convert, store, and the stop (atomicMin on the
//                kernel's first_stop with t * 64 + r).  Every thread of a block of WG calls it.
template <uint32_t WG, class Count, class Publish, class Unit>
__device__ __forceinline__ void unit_tiles(uint32_t n, Count count, Publish publish, Unit unit) {
  __shared__ uint32_t s_excl[WG / 64][64];
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t* const ex = s_excl[threadIdx.x >> 6];
  const uint32_t ntiles = (n + 63u) / 64u;
  const uint32_t wstride = gridDim.x * (WG / 64);
  for (uint32_t t = blockIdx.x * (WG / 64) + (threadIdx.x >> 6); t < ntiles; t += wstride) {
    const uint32_t units = count(t * 64u + lane);
    const uint32_t incl = wave_scan_dpp(units), T = wave_last(incl);
    if (T == 0u) continue;  // wave-uniform
    // ex and the payload are one wave's, whose LDS operations run in issue order: no s_barrier, but
    // the compiler must keep the order.  The previous tile's reads precede these writes, ...
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    ex[lane] = incl - units;
    publish(lane);
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");  // ... and the writes precede the other lanes' reads below
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
      unit(t, r, q - ex[r]);
    }
  }
}

}  // namespace hbam
