// The ascending filter list of one score row walked beside the row's ascending column steps (loss_kernels.hip: the all-entity
// cross-entropy and the streamed filtered rank).  A wave takes 256 consecutive columns per step (one float4 per lane) and keeps 64
// list entries in its registers (one per lane): the entries inside the step's 256-entity window are found by one ballot, and each
// is handed to the lane that owns its column.  A list of <= 64 entries (all but hub rows) is loaded once; a hub row's list is
// reloaded 64 further entries at a time as the steps pass it.  Every wave of a workgroup walks the list on its own.
#pragma once
#include "common.hpp"

namespace temp {

#define FCE_NO_ENTRY 0x7fffffff

struct RowFilter {
  const int32_t* ids;
  int pos, end;                 // the 64 entries in the registers are ids[pos .. pos + 64) (clipped to end)
  int v;                        // this lane's entry, FCE_NO_ENTRY past the end
};
__device__ __forceinline__ void filter_load(RowFilter& f, int lane) { f.v = f.pos + lane < f.end ? f.ids[f.pos + lane] : FCE_NO_ENTRY; }
__device__ __forceinline__ RowFilter filter_open(const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, const int32_t* __restrict__ ids, int p, int lane) {
  RowFilter f;
  f.ids = ids;
  f.pos = lo ? lo[p] : 0;
  f.end = lo ? hi[p] : 0;
  filter_load(f, lane);
  return f;
}
// Bit u set <=> entity w0 + 4 * lane + u is in the list; w0 = the first entity of the wave's step.  Called by all 64 lanes, with
// w0 ascending from call to call.
__device__ __forceinline__ unsigned filter_mask(RowFilter& f, int w0, int lane) {
  unsigned mask = 0;
  for (;;) {
    unsigned long long hit = __ballot(f.v >= w0 && f.v < w0 + 256);
    while (hit) {
      const int i = __builtin_ctzll(hit);
      hit &= hit - 1;
      const int t = __shfl(f.v, i) - w0;
      if ((t >> 2) == lane) mask |= 1u << (t & 3);
    }
    if (f.pos + 64 >= f.end || __shfl(f.v, 63) >= w0 + 256) break;       // the list, or this window, ends inside these 64 entries
    f.pos += 64;
    filter_load(f, lane);
  }
  return mask;
}
// -> the lane's four scores with everything inadmissible (listed and not the truth, or a pad column j >= N) replaced by `fill`
__device__ __forceinline__ float4 filter_select(float4 x, unsigned mask, int e0, int truth, int left, float fill) {
  const unsigned t = (unsigned)(truth - e0);
  if (t < 4u) mask &= ~(1u << t);
  if (left < 4) mask |= 0xfu << left;                                     // left >= 1 columns of the four lie below N
  return make_float4((mask & 1u) ? fill : x.x, (mask & 2u) ? fill : x.y, (mask & 4u) ? fill : x.z, (mask & 8u) ? fill : x.w);
}

}  // namespace temp
