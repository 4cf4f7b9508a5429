// Wave and workgroup reductions of the loss kernels (loss_kernels.hip, gated_loss.hip, l1_loss.hip): one statement of every
// summation order, so that kernels whose results are compared bit for bit reduce alike.  256-thread workgroups of four waves.
#pragma once
#include "common.hpp"

namespace temp {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// 256-thread reductions over `red[4]`; `red` may be reused right after: the leading barrier orders it against the last read
__device__ __forceinline__ float block_sum_256(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float block_max_256(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// (0 + 1) + (2 + 3) of the four waves' float4 partials of one 256-column pass; the result is valid in wave 0.
__device__ __forceinline__ float4 combine_waves_4(float4 acc, float (*part)[256], int w, int lane) {
  __syncthreads();                                       // part may still be read from the pass before
  if (w > 0) st4(&part[w - 1][lane * 4], acc);
  __syncthreads();
  if (w > 0) return acc;
  const float4 a1 = ld4(&part[0][lane * 4]), a2 = ld4(&part[1][lane * 4]), a3 = ld4(&part[2][lane * 4]);
  return make_float4((acc.x + a1.x) + (a2.x + a3.x), (acc.y + a1.y) + (a2.y + a3.y), (acc.z + a1.z) + (a2.z + a3.z), (acc.w + a1.w) + (a2.w + a3.w));
}

// Candidate multiplicities of one row in this wave's N counters of `cnt_all` (one wave per row, four rows per workgroup): no
// workgroup barriers -- a wave's LDS operations complete in issue order, so its zero fill, its integer atomics and its reads of
// the counters need only the waits below between them.
__device__ __forceinline__ int* gather_ce_wave_counts(int* cnt_all, int N, int C, const int32_t* __restrict__ crow) {
  const int lane = threadIdx.x & 63;
  int* cnt = cnt_all + (threadIdx.x >> 6) * N;
  for (int i = lane; i < N; i += 64) cnt[i] = 0;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  for (int k = lane; k < C; k += 64) atomicAdd(&cnt[crow[k]], 1);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  return cnt;
}

}  // namespace temp
