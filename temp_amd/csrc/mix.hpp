// The one mixing expression of the gated (post-aggregation) kernels: mix(w, a, b) = w a + (1 - w) b as fmaf(w, a, (1 - w) * b).
// Every kernel that forms a gated row -- the gated query, the mixed candidate cross-entropy of the bilinear scorers, the gated
// TransE candidate loss and dense scores -- uses it, forward and backward, so a backward pass recomputes the forward's value bit
// for bit.  For finite a and b:  w == 1 gives a exactly ((1 - w) * b is a zero and fmaf(1, a, +-0) rounds the exact a), and
// w == 0 gives b exactly (1 * b is b and fmaf(0, a, b) rounds the exact b); an a or b that is a zero may come back with the other
// zero's sign.  The tests rely on both.
#pragma once
#include "common.hpp"

namespace temp {

__device__ __forceinline__ float mix1(float w, float a, float b) { return fmaf(w, a, (1.f - w) * b); }
__device__ __forceinline__ float4 mix4(float w, float4 a, float4 b) {
  return make_float4(mix1(w, a.x, b.x), mix1(w, a.y, b.y), mix1(w, a.z, b.z), mix1(w, a.w, b.w));
}

}  // namespace temp
