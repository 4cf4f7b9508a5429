// Loss and evaluation kernels: candidate-list cross-entropy, the folded query of the scorers, the L1 (TransE) candidate loss and
// dense scores, their gated forms over two all-entity tables (the post-aggregation models), filtered negative sampling and the
// filtered rank, with their entry points.
#include "common.hpp"
#include "mix.hpp"

namespace temp {

// ---------------------------------------------------------------------------------------------
// Link-prediction loss over candidate lists (TKG_Module.train_link_prediction, models/TKG_Module.py:202-213):
// the scores of every positive against ALL entities come from one MFMA GEMM (query . all_embeds^T);
// these kernels pick the 1 + negative_rate candidates of each row out of that matrix and do the
// cross-entropy with label 0 -- nothing of shape (P, 1+neg, D) is ever materialised.
// One workgroup per row.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_reduce_256(float v, float* red, bool is_max) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(v, off);
    v = is_max ? fmaxf(v, o) : v + o;
  }
  __syncthreads();                                     // red may still be read from a previous reduction
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return is_max ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
}

// Candidate lists shorter than half a score row: gather the C logits once (<= 4 per thread in registers).
__global__ void __launch_bounds__(256) k_gather_ce_fwd(int C, int N, const float* __restrict__ scores, const int32_t* __restrict__ cand,
                                                       float* __restrict__ loss_rows, float* __restrict__ lse_rows) {
  __shared__ float red[4];
  const int p = blockIdx.x;
  const float* srow = scores + (size_t)p * N;
  const int32_t* crow = cand + (size_t)p * C;
  float mx = -INFINITY, sum = 0.f;
  if (C <= 1024) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = threadIdx.x + 256 * u;
      v[u] = k < C ? srow[crow[k]] : -INFINITY;
      mx = fmaxf(mx, v[u]);
    }
    mx = block_reduce_256(mx, red, true);
#pragma unroll
    for (int u = 0; u < 4; ++u) sum += expf(v[u] - mx);                 // exp(-inf) = 0 for the padding
  } else {
    for (int k = threadIdx.x; k < C; k += 256) mx = fmaxf(mx, srow[crow[k]]);
    mx = block_reduce_256(mx, red, true);
    for (int k = threadIdx.x; k < C; k += 256) sum += expf(srow[crow[k]] - mx);
  }
  sum = block_reduce_256(sum, red, false);
  if (threadIdx.x == 0) {
    const float lse = mx + logf(sum);
    lse_rows[p] = lse;
    loss_rows[p] = lse - srow[crow[0]];
  }
}

// Candidate lists about as long as the row (negative_rate ~ N_ents: the same entity is drawn several times): count the
// multiplicity of every entity with integer LDS atomics (order-independent), then ONE coalesced pass over the score row:
//   lse = log sum_e cnt[e] exp(s[e]).
__global__ void __launch_bounds__(256) k_gather_ce_fwd_cnt(int C, int N, const float* __restrict__ scores, const int32_t* __restrict__ cand,
                                                           float* __restrict__ loss_rows, float* __restrict__ lse_rows) {
  extern __shared__ int cnt[];
  __shared__ float red[4];
  const int p = blockIdx.x;
  for (int i = threadIdx.x; i < N; i += 256) cnt[i] = 0;
  __syncthreads();
  const float* srow = scores + (size_t)p * N;
  const int32_t* crow = cand + (size_t)p * C;
  for (int k = threadIdx.x; k < C; k += 256) atomicAdd(&cnt[crow[k]], 1);
  __syncthreads();
  float mx = -INFINITY;
  for (int i = threadIdx.x; i < N; i += 256)
    if (cnt[i]) mx = fmaxf(mx, srow[i]);
  mx = block_reduce_256(mx, red, true);
  float sum = 0.f;
  for (int i = threadIdx.x; i < N; i += 256)
    if (cnt[i]) sum += (float)cnt[i] * expf(srow[i] - mx);
  sum = block_reduce_256(sum, red, false);
  if (threadIdx.x == 0) {
    const float lse = mx + logf(sum);
    lse_rows[p] = lse;
    loss_rows[p] = lse - srow[crow[0]];
  }
}

// The same for SHORT score rows (N <= 1024: GDELT's 500 entities under 48 000 loss rows): one WAVE per row, four rows per
// workgroup -- no workgroup barriers, no cross-wave reductions; a wave's LDS operations complete in issue order, so its zero fill,
// its integer atomics and its reads of the counters need no barrier between them.
__device__ __forceinline__ float wave_reduce_f(float v, bool is_max) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(v, off);
    v = is_max ? fmaxf(v, o) : v + o;
  }
  return v;
}

__device__ __forceinline__ int* gather_ce_wave_counts(int* cnt_all, int N, int C, const int32_t* __restrict__ crow) {
  const int lane = threadIdx.x & 63;
  int* cnt = cnt_all + (threadIdx.x >> 6) * N;
  for (int i = lane; i < N; i += 64) cnt[i] = 0;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  for (int k = lane; k < C; k += 64) atomicAdd(&cnt[crow[k]], 1);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  return cnt;
}

__global__ void __launch_bounds__(256) k_gather_ce_fwd_cnt_w(int P, int C, int N, const float* __restrict__ scores, const int32_t* __restrict__ cand,
                                                             float* __restrict__ loss_rows, float* __restrict__ lse_rows) {
  extern __shared__ int cnt_all[];
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= P) return;
  const float* srow = scores + (size_t)p * N;
  const int32_t* crow = cand + (size_t)p * C;
  const int* cnt = gather_ce_wave_counts(cnt_all, N, C, crow);
  float mx = -INFINITY;
  float sv[16];                                                           // the row's scores of this lane (N <= 1024): read once
  int cv[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int i = lane + 64 * u;
    cv[u] = i < N ? cnt[i] : 0;
    sv[u] = i < N ? srow[i] : 0.f;
    if (cv[u]) mx = fmaxf(mx, sv[u]);
  }
  mx = wave_reduce_f(mx, true);
  float sum = 0.f;
#pragma unroll
  for (int u = 0; u < 16; ++u)
    if (cv[u]) sum += (float)cv[u] * expf(sv[u] - mx);
  sum = wave_reduce_f(sum, false);
  if (lane == 0) {
    const float lse = mx + logf(sum);
    lse_rows[p] = lse;
    loss_rows[p] = lse - srow[crow[0]];
  }
}

__global__ void __launch_bounds__(256) k_gather_ce_bwd_w(int P, int C, int N, const float* __restrict__ scores, const int32_t* __restrict__ cand,
                                                         const float* __restrict__ lse_rows, const float* __restrict__ scale_ptr, float inv_rows,
                                                         const float* __restrict__ row_scale, float* __restrict__ d_scores) {
  extern __shared__ int cnt_all[];
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= P) return;
  const float* srow = scores + (size_t)p * N;
  const int32_t* crow = cand + (size_t)p * C;
  const int* cnt = gather_ce_wave_counts(cnt_all, N, C, crow);
  const float lse = lse_rows[p];
  const float scale = scale_ptr[0] * (row_scale ? row_scale[p] : inv_rows);
  const int truth = crow[0];
  float* drow = d_scores + (size_t)p * N;
  for (int i = lane; i < N; i += 64) {
    const int c = cnt[i];
    float g = c ? (float)c * expf(srow[i] - lse) : 0.f;
    if (i == truth) g -= 1.f;
    drow[i] = g * scale;
  }
}

// d_scores[p, e] = scale * (cnt[e] * softmax(e) - [e == cand[p,0]])   (row written once, coalesced; multiplicities counted
// with integer LDS atomics, so the result does not depend on the order the candidates are visited in)
__global__ void __launch_bounds__(256) k_gather_ce_bwd(int C, int N, const float* __restrict__ scores, const int32_t* __restrict__ cand,
                                                       const float* __restrict__ lse_rows, const float* __restrict__ scale_ptr, float inv_rows,
                                                       const float* __restrict__ row_scale, float* __restrict__ d_scores) {
  extern __shared__ int cnt[];
  const int p = blockIdx.x;
  for (int i = threadIdx.x; i < N; i += 256) cnt[i] = 0;
  __syncthreads();
  const float* srow = scores + (size_t)p * N;
  const int32_t* crow = cand + (size_t)p * C;
  for (int k = threadIdx.x; k < C; k += 256) atomicAdd(&cnt[crow[k]], 1);
  __syncthreads();
  const float lse = lse_rows[p];
  const float scale = scale_ptr[0] * (row_scale ? row_scale[p] : inv_rows);
  const int truth = crow[0];
  float* drow = d_scores + (size_t)p * N;
  for (int i = threadIdx.x; i < N; i += 256) {
    const int c = cnt[i];
    float g = c ? (float)c * expf(srow[i] - lse) : 0.f;
    if (i == truth) g -= 1.f;
    drow[i] = g * scale;
  }
}

// ---------------------------------------------------------------------------------------------
// Folded query of the bilinear scorers (utils/scores.py:4-12 DistMult, :26-44 ComplEx), with the two row gathers
// fused in:  k = ent_rows[known_idx[p]],  r = rel[rel_idx[p]],
//   DistMult            q = k * r
//   ComplEx, tail mode  q = [re_k re_r - im_k im_r | re_k im_r + im_k re_r]      (k is the subject, candidates are objects)
//   ComplEx, head mode  q = [re_r re_k + im_r im_k | re_r im_k - im_r re_k]      (k is the object, candidates are subjects)
// so that score(candidate c) = <q, c>, and the translation query of TransE (utils/scores.py:46-55)
//   TransE, tail mode   q = k + r         TransE, head mode   q = k - r           score(candidate c) = -|q - c|_1
// (one IEEE add / subtract per element: bit-equal to the tensor expression).  One thread per float4 of the half width; the backward writes the per-row
// gradients of k and r (the caller reduces them over the static index lists with temp_segment_sum_rows).
// ---------------------------------------------------------------------------------------------
template <bool BWD>
__global__ void __launch_bounds__(256) k_bilinear_query(int P, int d, int kind, const float* __restrict__ ent_rows, const int32_t* __restrict__ known_idx,
                                                        const float* __restrict__ rel, const int32_t* __restrict__ rel_idx,
                                                        const int32_t* __restrict__ is_tail, const float* __restrict__ dq, float* __restrict__ o0,
                                                        float* __restrict__ o1) {
  const int half = kind == TEMP_SCORE_COMPLEX ? d / 2 : d;
  const int g4 = half / 4;
  const size_t total = (size_t)P * g4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int p = (int)(i / g4), j = (int)(i - (size_t)p * g4) * 4;
    const float* k = ent_rows + (size_t)known_idx[p] * d + j;
    const float* r = rel + (size_t)rel_idx[p] * d + j;
    const size_t o = (size_t)p * d + j;
    if (kind == TEMP_SCORE_TRANSE) {
      const float sg = is_tail[p] ? 1.f : -1.f;       // sg * r is exact, so k + sg * r rounds once: the same value as k + r / k - r
      if (!BWD) {
        const float4 kv = ld4(k), rv = ld4(r);
        st4(o0 + o, make_float4(kv.x + sg * rv.x, kv.y + sg * rv.y, kv.z + sg * rv.z, kv.w + sg * rv.w));
      } else {
        const float4 g = ld4(dq + o);
        st4(o0 + o, g);
        st4(o1 + o, make_float4(sg * g.x, sg * g.y, sg * g.z, sg * g.w));
      }
      continue;
    }
    if (kind != TEMP_SCORE_COMPLEX) {
      const float4 kv = ld4(k), rv = ld4(r);
      if (!BWD) {
        st4(o0 + o, make_float4(kv.x * rv.x, kv.y * rv.y, kv.z * rv.z, kv.w * rv.w));
      } else {
        const float4 g = ld4(dq + o);
        st4(o0 + o, make_float4(g.x * rv.x, g.y * rv.y, g.z * rv.z, g.w * rv.w));
        st4(o1 + o, make_float4(g.x * kv.x, g.y * kv.y, g.z * kv.z, g.w * kv.w));
      }
      continue;
    }
    const float4 rk = ld4(k), ik = ld4(k + half), rr = ld4(r), ir = ld4(r + half);
    const float sg = is_tail[p] ? 1.f : -1.f;       // tail: q1 = rk rr - ik ir, q2 = rk ir + ik rr;  head: q1 = rk rr + ik ir, q2 = ik rr - rk ir
    if (!BWD) {
      st4(o0 + o, make_float4(rk.x * rr.x - sg * ik.x * ir.x, rk.y * rr.y - sg * ik.y * ir.y, rk.z * rr.z - sg * ik.z * ir.z, rk.w * rr.w - sg * ik.w * ir.w));
      st4(o0 + o + half, make_float4(ik.x * rr.x + sg * rk.x * ir.x, ik.y * rr.y + sg * rk.y * ir.y, ik.z * rr.z + sg * rk.z * ir.z, ik.w * rr.w + sg * rk.w * ir.w));
    } else {
      const float4 a = ld4(dq + o), b = ld4(dq + o + half);
      // q1 = rk rr - sg ik ir ; q2 = ik rr + sg rk ir
      st4(o0 + o, make_float4(a.x * rr.x + sg * b.x * ir.x, a.y * rr.y + sg * b.y * ir.y, a.z * rr.z + sg * b.z * ir.z, a.w * rr.w + sg * b.w * ir.w));                 // d re_k
      st4(o0 + o + half, make_float4(b.x * rr.x - sg * a.x * ir.x, b.y * rr.y - sg * a.y * ir.y, b.z * rr.z - sg * a.z * ir.z, b.w * rr.w - sg * a.w * ir.w));          // d im_k
      st4(o1 + o, make_float4(a.x * rk.x + b.x * ik.x, a.y * rk.y + b.y * ik.y, a.z * rk.z + b.z * ik.z, a.w * rk.w + b.w * ik.w));                                     // d re_r
      st4(o1 + o + half, make_float4(sg * (b.x * rk.x - a.x * ik.x), sg * (b.y * rk.y - a.y * ik.y), sg * (b.z * rk.z - a.z * ik.z), sg * (b.w * rk.w - a.w * ik.w)));  // d im_r
    }
  }
}

// ---------------------------------------------------------------------------------------------
// TransE (utils/scores.py:46-55) is not bilinear: score(p, c) = -sum_d |q[p,d] - c[d]| with the translation query q above, so
// no GEMM carries it.  The training loss needs the score at the 1 + negative_rate candidates of a row only -- a gather of
// P C d elements, N / C times fewer than the dense matrix -- and never as a (P, C, D) tensor:
//   k_l1_ce_fwd        one workgroup per row; a 16-lane group owns a candidate (float4 per lane, ceil(d / 64) passes, four xor
//                      steps to reduce), two candidates per group in flight; then the row's logsumexp.
//   k_l1_ce_bwd_q      g = scale * (softmax - [k == 0]);  d_q[p] = -sum_k g_k sgn(q[p] - e_k): wave w sums the candidates
//                      k = w mod 4 in ascending order, the four partials combine as (0 + 1) + (2 + 3).
//   k_l1_ce_bwd_table  the candidate-side adjoint over the slots of one table row (a stable sort of the flat positions by table
//                      row), split over the four waves and combined in the same way: no atomics, fixed order.
// sgn(0) = 0, the gradient torch.abs takes.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float l1_4(float4 a, float4 b) { return (fabsf(a.x - b.x) + fabsf(a.y - b.y)) + (fabsf(a.z - b.z) + fabsf(a.w - b.w)); }
__device__ __forceinline__ float sgnf(float x) { return (float)((x > 0.f) - (x < 0.f)); }
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// NP > 0: d <= 64 NP and q[p] stays in registers; NP == 0: any d, q[p] is re-read per candidate (it stays in the L1).
template <int NP>
__global__ void __launch_bounds__(256) k_l1_ce_fwd(int C, int d, const float* __restrict__ q, const float* __restrict__ table,
                                                   const int32_t* __restrict__ base, const int32_t* __restrict__ cand, float* s_out,
                                                   float* __restrict__ loss_rows, float* __restrict__ lse_rows) {
  __shared__ float red[4];
  const int p = blockIdx.x, grp = threadIdx.x >> 4, l = threadIdx.x & 15;
  const float* qrow = q + (size_t)p * d;
  const int32_t* crow = cand + (size_t)p * C;
  float* srow = s_out + (size_t)p * C;
  const size_t b = base ? (size_t)base[p] : 0;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 qv[NP > 0 ? NP : 1];
#pragma unroll
  for (int u = 0; u < NP; ++u) qv[u] = l * 4 + 64 * u < d ? ld4(qrow + l * 4 + 64 * u) : zero;
  for (int k0 = grp; k0 < C; k0 += 32) {
    const int k1 = k0 + 16;
    const float* e0 = table + (b + (size_t)crow[k0]) * d;
    const float* e1 = k1 < C ? table + (b + (size_t)crow[k1]) * d : e0;
    float a0 = 0.f, a1 = 0.f;
    if (NP > 0) {
      float4 x0[NP > 0 ? NP : 1], x1[NP > 0 ? NP : 1];
#pragma unroll
      for (int u = 0; u < NP; ++u) {                      // both candidates' rows are requested before either is consumed
        const int j = l * 4 + 64 * u;
        x0[u] = j < d ? ld4(e0 + j) : zero;
        x1[u] = j < d ? ld4(e1 + j) : zero;
      }
#pragma unroll
      for (int u = 0; u < NP; ++u) { a0 += l1_4(qv[u], x0[u]); a1 += l1_4(qv[u], x1[u]); }
    } else {
      for (int j = l * 4; j < d; j += 64) {
        const float4 qq = ld4(qrow + j), x0 = ld4(e0 + j), x1 = ld4(e1 + j);
        a0 += l1_4(qq, x0);
        a1 += l1_4(qq, x1);
      }
    }
    a0 = group16_sum(a0);
    a1 = group16_sum(a1);
    if (l == 0) {
      srow[k0] = -a0;
      if (k1 < C) srow[k1] = -a1;
    }
  }
  __syncthreads();                                       // the row's scores, written by this workgroup, are read back below
  float mx = -INFINITY, sum = 0.f;
  for (int k = threadIdx.x; k < C; k += 256) mx = fmaxf(mx, srow[k]);
  mx = block_reduce_256(mx, red, true);
  for (int k = threadIdx.x; k < C; k += 256) sum += expf(srow[k] - mx);
  sum = block_reduce_256(sum, red, false);
  if (threadIdx.x == 0) {
    const float lse = mx + logf(sum);
    lse_rows[p] = lse;
    loss_rows[p] = lse - srow[0];
  }
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

__global__ void __launch_bounds__(256) k_l1_ce_bwd_q(int C, int d, const float* __restrict__ q, const float* __restrict__ table,
                                                     const int32_t* __restrict__ base, const int32_t* __restrict__ cand,
                                                     const float* __restrict__ s, const float* __restrict__ lse_rows,
                                                     const float* __restrict__ scale_ptr, float inv_rows, const float* __restrict__ row_scale,
                                                     float* g_out, float* __restrict__ d_q) {
  __shared__ __attribute__((aligned(16))) float part[3][256];
  const int p = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* qrow = q + (size_t)p * d;
  const int32_t* crow = cand + (size_t)p * C;
  const float* srow = s + (size_t)p * C;
  float* grow = g_out + (size_t)p * C;
  const size_t b = base ? (size_t)base[p] : 0;
  const float lse = lse_rows[p];
  const float scale = scale_ptr[0] * (row_scale ? row_scale[p] : inv_rows);
  for (int k = threadIdx.x; k < C; k += 256) grow[k] = scale * (expf(srow[k] - lse) - (k == 0 ? 1.f : 0.f));
  __syncthreads();                                       // g of the row, written by this workgroup, is read back below
  for (int j0 = 0; j0 < d; j0 += 256) {
    const int j = j0 + lane * 4;
    const bool act = j < d;
    const float4 qv = act ? ld4(qrow + j) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int k = w; k < C; k += 4) {
      const float gk = grow[k];
      const float* e = table + (b + (size_t)crow[k]) * d;
      if (act) {
        const float4 x = ld4(e + j);
        acc.x -= gk * sgnf(qv.x - x.x); acc.y -= gk * sgnf(qv.y - x.y); acc.z -= gk * sgnf(qv.z - x.z); acc.w -= gk * sgnf(qv.w - x.w);
      }
    }
    acc = combine_waves_4(acc, part, w, lane);
    if (w == 0 && act) st4(d_q + (size_t)p * d + j, acc);
  }
}

__global__ void __launch_bounds__(256) k_l1_ce_bwd_table(int d, int C, const float* __restrict__ q, const float* __restrict__ table,
                                                         const int32_t* __restrict__ slot_ptr, const int32_t* __restrict__ slot,
                                                         const float* __restrict__ g, float* __restrict__ d_table) {
  __shared__ __attribute__((aligned(16))) float part[3][256];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t n = blockIdx.x;
  const int s0 = slot_ptr[n], s1 = slot_ptr[n + 1];
  for (int j0 = 0; j0 < d; j0 += 256) {
    const int j = j0 + lane * 4;
    const bool act = j < d;
    const float4 tv = act ? ld4(table + n * d + j) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int i = s0 + w; i < s1; i += 4) {
      const int sl = slot[i];
      const float gk = g[sl];
      const float* qr = q + (size_t)(sl / C) * d;
      if (act) {
        const float4 x = ld4(qr + j);
        acc.x += gk * sgnf(x.x - tv.x); acc.y += gk * sgnf(x.y - tv.y); acc.z += gk * sgnf(x.z - tv.z); acc.w += gk * sgnf(x.w - tv.w);
      }
    }
    acc = combine_waves_4(acc, part, w, lane);
    if (w == 0 && act) st4(d_table + n * d + j, acc);      // a row without slots gets its zeros here
  }
}

// Dense L1 scores for the ranking: scores[p, n] = -|q[p] - table[n]|_1, columns [N, ld) = -inf.  No MFMA applies (|a - b| is not
// a product); a VALU register tile instead: 64 x 64 outputs per workgroup, 4 x 4 per thread, 16-wide k-chunks of both operands
// staged k-major in LDS (row stride 68 floats: the float4 reads of a k-row stay 16-byte aligned, the 16 distinct ones of a wave
// are contiguous and the row operand is a broadcast).  Per output and k: one subtract, one add with the |.| source modifier.
// The transposing staging stores are 2-way bank-conflicted (any 16-byte-aligned stride puts the k-groups 0 / 8 and 4 / 12 of a
// half-wave on one bank): 8 stores per thread and chunk beside its 512 VALU operations, left as it is.
#define L1S_TILE 64
#define L1S_KC 16
#define L1S_LD 68
__global__ void __launch_bounds__(256) k_l1_scores(int P, int N, int d, const float* __restrict__ q, const float* __restrict__ table, int ld,
                                                   float* __restrict__ scores) {
  __shared__ __attribute__((aligned(16))) float As[L1S_KC][L1S_LD];
  __shared__ __attribute__((aligned(16))) float Bs[L1S_KC][L1S_LD];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int p0 = blockIdx.y * L1S_TILE, n0 = blockIdx.x * L1S_TILE;
  const int lr = threadIdx.x >> 2, lk = (threadIdx.x & 3) * 4;        // the float4 of the k-chunk this thread stages: row lr, columns lk..lk+3
  const bool a_ok = p0 + lr < P, b_ok = n0 + lr < N;
  const float* arow = q + (size_t)(a_ok ? p0 + lr : 0) * d;
  const float* brow = table + (size_t)(b_ok ? n0 + lr : 0) * d;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float acc[4][4] = {};
  for (int k0 = 0; k0 < d; k0 += L1S_KC) {
    const bool k_ok = k0 + lk < d;                                    // d % 4 == 0: a float4 is inside the row or past it
    const float4 av = a_ok && k_ok ? ld4(arow + k0 + lk) : zero;     // rows and columns past the edge: |0 - 0| adds nothing
    const float4 bv = b_ok && k_ok ? ld4(brow + k0 + lk) : zero;
    __syncthreads();                                                  // the chunk before is consumed
    As[lk][lr] = av.x; As[lk + 1][lr] = av.y; As[lk + 2][lr] = av.z; As[lk + 3][lr] = av.w;
    Bs[lk][lr] = bv.x; Bs[lk + 1][lr] = bv.y; Bs[lk + 2][lr] = bv.z; Bs[lk + 3][lr] = bv.w;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < L1S_KC; ++k) {
      const float4 a = ld4(&As[k][ty * 4]), b = ld4(&Bs[k][tx * 4]);
      const float ar[4] = {a.x, a.y, a.z, a.w}, br[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[i][jj] += fabsf(ar[i] - br[jj]);
    }
  }
  const int n = n0 + tx * 4;
  if (n >= ld) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = p0 + ty * 4 + i;
    if (p >= P) break;
    st4(scores + (size_t)p * ld + n, make_float4(n < N ? -acc[i][0] : -INFINITY, n + 1 < N ? -acc[i][1] : -INFINITY,
                                                 n + 2 < N ? -acc[i][2] : -INFINITY, n + 3 < N ? -acc[i][3] : -INFINITY));
  }
}

// ---------------------------------------------------------------------------------------------
// Gated TransE (PostDynamicRGCN.train_link_prediction, models/PostDynamicRGCN.py:261-282 with utils/scores.py:46-55): the candidate
// is the per-row mix e[p,k] = mix(w[p], TA[row], TB[row]) of the two all-entity tables (mix.hpp).  |q - e|_1 is not linear in e, so
// the mix cannot move to two score matrices as it does for the bilinear scorers (gated_loss.hip): these kernels are the L1
// kernels above reading BOTH table rows of a candidate and mixing in registers -- still no (P, C, D) tensor.
//   k_l1_mix_ce_fwd        k_l1_ce_fwd with two rows per candidate.
//   k_l1_mix_ce_bwd_q      g, d_q as k_l1_ce_bwd_q, and d_w[p] = sum_k g_k sum_d sgn(q - e_k) (TA - TB)[row] from the rows it holds:
//                          every thread sums its own (k, d) terms in loop order, then lanes (xor tree) and waves ((0 + 1) + (2 + 3)).
//   k_l1_mix_ce_bwd_table  one pass over a table row's slots writes d_TA = sum w g sgn and d_TB = sum (1 - w) g sgn; the mixed row
//                          differs per slot (the slot's row weight), so it is recomputed per slot from the two rows in registers.
//   k_l1_mix_scores        k_l1_scores with both tables staged; the mix is formed per (row, entity, k) by mix1, so a score
//                          agrees with the candidate kernels' to the summation order.
// ---------------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(256) k_l1_mix_ce_fwd(int C, int d, const float* __restrict__ q, const float* __restrict__ ta,
                                                       const float* __restrict__ tb, const float* __restrict__ w,
                                                       const int32_t* __restrict__ base, const int32_t* __restrict__ cand, float* s_out,
                                                       float* __restrict__ loss_rows, float* __restrict__ lse_rows) {
  __shared__ float red[4];
  const int p = blockIdx.x, grp = threadIdx.x >> 4, l = threadIdx.x & 15;
  const float* qrow = q + (size_t)p * d;
  const int32_t* crow = cand + (size_t)p * C;
  float* srow = s_out + (size_t)p * C;
  const size_t b = base ? (size_t)base[p] : 0;
  const float wp = w[p];
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 qv[NP > 0 ? NP : 1];
#pragma unroll
  for (int u = 0; u < NP; ++u) qv[u] = l * 4 + 64 * u < d ? ld4(qrow + l * 4 + 64 * u) : zero;
  for (int k0 = grp; k0 < C; k0 += 32) {
    const int k1 = k0 + 16;
    const size_t r0 = (b + (size_t)crow[k0]) * d, r1 = k1 < C ? (b + (size_t)crow[k1]) * d : r0;
    float a0 = 0.f, a1 = 0.f;
    if (NP > 0) {
      float4 x0[NP > 0 ? NP : 1], y0[NP > 0 ? NP : 1], x1[NP > 0 ? NP : 1], y1[NP > 0 ? NP : 1];
#pragma unroll
      for (int u = 0; u < NP; ++u) {                      // all four rows are requested before any is consumed
        const int j = l * 4 + 64 * u;
        x0[u] = j < d ? ld4(ta + r0 + j) : zero;
        y0[u] = j < d ? ld4(tb + r0 + j) : zero;
        x1[u] = j < d ? ld4(ta + r1 + j) : zero;
        y1[u] = j < d ? ld4(tb + r1 + j) : zero;
      }
#pragma unroll
      for (int u = 0; u < NP; ++u) { a0 += l1_4(qv[u], mix4(wp, x0[u], y0[u])); a1 += l1_4(qv[u], mix4(wp, x1[u], y1[u])); }
    } else {
      for (int j = l * 4; j < d; j += 64) {
        const float4 qq = ld4(qrow + j), x0 = ld4(ta + r0 + j), y0 = ld4(tb + r0 + j), x1 = ld4(ta + r1 + j), y1 = ld4(tb + r1 + j);
        a0 += l1_4(qq, mix4(wp, x0, y0));
        a1 += l1_4(qq, mix4(wp, x1, y1));
      }
    }
    a0 = group16_sum(a0);
    a1 = group16_sum(a1);
    if (l == 0) {
      srow[k0] = -a0;
      if (k1 < C) srow[k1] = -a1;
    }
  }
  __syncthreads();                                       // the row's scores, written by this workgroup, are read back below
  float mx = -INFINITY, sum = 0.f;
  for (int k = threadIdx.x; k < C; k += 256) mx = fmaxf(mx, srow[k]);
  mx = block_reduce_256(mx, red, true);
  for (int k = threadIdx.x; k < C; k += 256) sum += expf(srow[k] - mx);
  sum = block_reduce_256(sum, red, false);
  if (threadIdx.x == 0) {
    const float lse = mx + logf(sum);
    lse_rows[p] = lse;
    loss_rows[p] = lse - srow[0];
  }
}

__device__ __forceinline__ float4 sgn4(float4 a, float4 b) { return make_float4(sgnf(a.x - b.x), sgnf(a.y - b.y), sgnf(a.z - b.z), sgnf(a.w - b.w)); }

__global__ void __launch_bounds__(256) k_l1_mix_ce_bwd_q(int C, int d, const float* __restrict__ q, const float* __restrict__ ta,
                                                         const float* __restrict__ tb, const float* __restrict__ w,
                                                         const int32_t* __restrict__ base, const int32_t* __restrict__ cand,
                                                         const float* __restrict__ s, const float* __restrict__ lse_rows,
                                                         const float* __restrict__ scale_ptr, float inv_rows, const float* __restrict__ row_scale,
                                                         float* g_out, float* __restrict__ d_q, float* __restrict__ d_w) {
  __shared__ __attribute__((aligned(16))) float part[3][256];
  __shared__ float red[4];
  const int p = blockIdx.x, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* qrow = q + (size_t)p * d;
  const int32_t* crow = cand + (size_t)p * C;
  const float* srow = s + (size_t)p * C;
  float* grow = g_out + (size_t)p * C;
  const size_t b = base ? (size_t)base[p] : 0;
  const float wp = w[p], lse = lse_rows[p];
  const float scale = scale_ptr[0] * (row_scale ? row_scale[p] : inv_rows);
  for (int k = threadIdx.x; k < C; k += 256) grow[k] = scale * (expf(srow[k] - lse) - (k == 0 ? 1.f : 0.f));
  __syncthreads();                                       // g of the row, written by this workgroup, is read back below
  float wacc = 0.f;
  for (int j0 = 0; j0 < d; j0 += 256) {
    const int j = j0 + lane * 4;
    const bool act = j < d;
    const float4 qv = act ? ld4(qrow + j) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int k = wv; k < C; k += 4) {
      const float gk = grow[k];
      const size_t r = (b + (size_t)crow[k]) * d;
      if (act) {
        const float4 x = ld4(ta + r + j), y = ld4(tb + r + j);
        const float4 sg = sgn4(qv, mix4(wp, x, y));
        acc.x -= gk * sg.x; acc.y -= gk * sg.y; acc.z -= gk * sg.z; acc.w -= gk * sg.w;
        wacc += gk * ((sg.x * (x.x - y.x) + sg.y * (x.y - y.y)) + (sg.z * (x.z - y.z) + sg.w * (x.w - y.w)));
      }
    }
    acc = combine_waves_4(acc, part, wv, lane);
    if (wv == 0 && act) st4(d_q + (size_t)p * d + j, acc);
  }
  wacc = block_reduce_256(wacc, red, false);
  if (threadIdx.x == 0) d_w[p] = wacc;
}

__global__ void __launch_bounds__(256) k_l1_mix_ce_bwd_table(int d, int C, const float* __restrict__ q, const float* __restrict__ ta,
                                                             const float* __restrict__ tb, const float* __restrict__ w,
                                                             const int32_t* __restrict__ slot_ptr, const int32_t* __restrict__ slot,
                                                             const float* __restrict__ g, float* __restrict__ d_ta, float* __restrict__ d_tb) {
  __shared__ __attribute__((aligned(16))) float part[3][256];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t n = blockIdx.x;
  const int s0 = slot_ptr[n], s1 = slot_ptr[n + 1];
  for (int j0 = 0; j0 < d; j0 += 256) {
    const int j = j0 + lane * 4;
    const bool act = j < d;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 x = act ? ld4(ta + n * d + j) : zero, y = act ? ld4(tb + n * d + j) : zero;
    float4 aa = zero, ab = zero;
#pragma unroll 4
    for (int i = s0 + wv; i < s1; i += 4) {
      const int sl = slot[i];
      const int p = sl / C;
      const float gk = g[sl], wp = w[p];
      const float* qr = q + (size_t)p * d;
      if (act) {
        const float4 sg = sgn4(ld4(qr + j), mix4(wp, x, y));
        const float4 t = scale4(sg, gk);                  // g sgn: exact
        aa = fma4(wp, t, aa);
        ab = fma4(1.f - wp, t, ab);
      }
    }
    aa = combine_waves_4(aa, part, wv, lane);
    if (wv == 0 && act) st4(d_ta + n * d + j, aa);       // a row without slots gets its zeros here
    ab = combine_waves_4(ab, part, wv, lane);
    if (wv == 0 && act) st4(d_tb + n * d + j, ab);
  }
}

__global__ void __launch_bounds__(256) k_l1_mix_scores(int P, int N, int d, const float* __restrict__ q, const float* __restrict__ ta,
                                                       const float* __restrict__ tb, const float* __restrict__ w, int ld,
                                                       float* __restrict__ scores) {
  __shared__ __attribute__((aligned(16))) float Qs[L1S_KC][L1S_LD];
  __shared__ __attribute__((aligned(16))) float As[L1S_KC][L1S_LD];
  __shared__ __attribute__((aligned(16))) float Bs[L1S_KC][L1S_LD];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int p0 = blockIdx.y * L1S_TILE, n0 = blockIdx.x * L1S_TILE;
  const int lr = threadIdx.x >> 2, lk = (threadIdx.x & 3) * 4;        // the float4 of the k-chunk this thread stages: row lr, columns lk..lk+3
  const bool q_ok = p0 + lr < P, t_ok = n0 + lr < N;
  const float* qrow = q + (size_t)(q_ok ? p0 + lr : 0) * d;
  const size_t trow = (size_t)(t_ok ? n0 + lr : 0) * d;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float wr[4], omw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = p0 + ty * 4 + i;
    wr[i] = p < P ? w[p] : 0.f;
    omw[i] = 1.f - wr[i];                                              // mix1's (1 - w), once per row
  }
  float acc[4][4] = {};
  for (int k0 = 0; k0 < d; k0 += L1S_KC) {
    const bool k_ok = k0 + lk < d;                                    // d % 4 == 0: a float4 is inside the row or past it
    const float4 qv = q_ok && k_ok ? ld4(qrow + k0 + lk) : zero;     // rows and columns past the edge: |0 - mix(w, 0, 0)| adds nothing
    const float4 av = t_ok && k_ok ? ld4(ta + trow + k0 + lk) : zero;
    const float4 bv = t_ok && k_ok ? ld4(tb + trow + k0 + lk) : zero;
    __syncthreads();                                                  // the chunk before is consumed
    Qs[lk][lr] = qv.x; Qs[lk + 1][lr] = qv.y; Qs[lk + 2][lr] = qv.z; Qs[lk + 3][lr] = qv.w;
    As[lk][lr] = av.x; As[lk + 1][lr] = av.y; As[lk + 2][lr] = av.z; As[lk + 3][lr] = av.w;
    Bs[lk][lr] = bv.x; Bs[lk + 1][lr] = bv.y; Bs[lk + 2][lr] = bv.z; Bs[lk + 3][lr] = bv.w;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < L1S_KC; ++k) {
      const float4 qq = ld4(&Qs[k][ty * 4]), a = ld4(&As[k][tx * 4]), b = ld4(&Bs[k][tx * 4]);
      const float qr[4] = {qq.x, qq.y, qq.z, qq.w}, ar[4] = {a.x, a.y, a.z, a.w}, br[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[i][jj] += fabsf(qr[i] - fmaf(wr[i], ar[jj], omw[i] * br[jj]));   // mix1, (1 - w) hoisted
    }
  }
  const int n = n0 + tx * 4;
  if (n >= ld) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = p0 + ty * 4 + i;
    if (p >= P) break;
    st4(scores + (size_t)p * ld + n, make_float4(n < N ? -acc[i][0] : -INFINITY, n + 1 < N ? -acc[i][1] : -INFINITY,
                                                 n + 2 < N ? -acc[i][2] : -INFINITY, n + 3 < N ? -acc[i][3] : -INFINITY));
  }
}

// ---------------------------------------------------------------------------------------------
// Filtered negative sampling (CorruptTriples.negative_sampling / corrupt_triple, utils/CorrptTriples.py:36-85):
// for every positive row, K corrupted entities drawn uniformly over ALL entities, redrawing those that form a true
// triple of the target snapshot (the row's known-true set is the slice ids[lo[row] .. hi[row]) of a resident store).
// One thread per candidate; the draw is a counter-based hash of (seed, row, column, attempt), so a step's samples
// are a pure function of its seed (no generator state, no rejection ROUNDS over the whole matrix).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__global__ void __launch_bounds__(256) k_corrupt_sample(long long total, int K1, int N, unsigned long long seed, const int32_t* __restrict__ truth,
                                                        const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                        const int32_t* __restrict__ ids, int32_t* __restrict__ cand) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int row = (int)(i / K1), k = (int)(i - (long long)row * K1);
    if (k == 0) { cand[i] = truth[row]; continue; }
    const int a = lo ? lo[row] : 0, b = lo ? hi[row] : 0;
    const unsigned long long base = splitmix64(seed ^ ((unsigned long long)row * 0xD1B54A32D192ED03ull + (unsigned long long)k));
    const int len = b - a;
    int c = 0;
    bool done = false;
    if (len > 16 && len < N) {                        // long known-true set: rejection with a binary search per attempt
      for (int attempt = 0; attempt < 64 && !done; ++attempt) {
        const unsigned long long x = splitmix64(base + attempt);
        c = (int)(((x >> 32) * (unsigned long long)N) >> 32);
        int l = a, h = b;
        while (l < h) { const int m = (l + h) >> 1; if (ids[m] < c) l = m + 1; else h = m; }
        done = !(l < b && ids[l] == c);
      }
    }
    if (!done) {
      // exact: the u-th entity of the complement, u uniform in [0, N - len) -- walk the ascending list, skipping its members
      const int free_n = len < N ? N - len : N;       // nothing allowed (the reference would loop forever): plain uniform draw
      const unsigned long long x = splitmix64(base + 64);
      c = (int)(((x >> 32) * (unsigned long long)free_n) >> 32);
      if (len < N)
        for (int j = a; j < b && ids[j] <= c; ++j) ++c;
    }
    cand[i] = c;
  }
}

// ---------------------------------------------------------------------------------------------
// Filtered rank of one test triple per workgroup (utils/evaluation.py:40-106): the reference sets the scores of the
// other known-true entities to -10e6, applies a sigmoid and takes the target's position in a descending sort.
// Position in a STABLE descending order = #(strictly larger) + #(equal with a smaller entity id) + 1, so nothing is
// sorted: one pass over the score row counts, a second pass over the row's filter list replaces the contribution of
// each filtered entity by that of sigmoid(-10e6) = 0.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float rank_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ int rank_ahead(float v, int j, float ts, int tgt) { return (v > ts) | ((v == ts) & (j < tgt)); }

__global__ void __launch_bounds__(256) k_filtered_rank(int N, int ld, const float* __restrict__ scores, const int32_t* __restrict__ target,
                                                       const int32_t* __restrict__ filt_ptr, const int32_t* __restrict__ filt_ids,
                                                       int32_t* __restrict__ ranks) {
  __shared__ int red[4];
  const int p = blockIdx.x;
  const float* srow = scores + (size_t)p * ld;
  const int tgt = target[p];
  const float ts = rank_sigmoid(srow[tgt]);
  int cnt = 0;
  const int n4 = N & ~3;
  for (int j = threadIdx.x * 4; j < n4; j += 1024) {
    const float4 s = *reinterpret_cast<const float4*>(srow + j);
    cnt += rank_ahead(rank_sigmoid(s.x), j, ts, tgt) + rank_ahead(rank_sigmoid(s.y), j + 1, ts, tgt)
         + rank_ahead(rank_sigmoid(s.z), j + 2, ts, tgt) + rank_ahead(rank_sigmoid(s.w), j + 3, ts, tgt);
  }
  for (int j = n4 + threadIdx.x; j < N; j += 256) cnt += rank_ahead(rank_sigmoid(srow[j]), j, ts, tgt);
  if (filt_ptr) {
    for (int f = filt_ptr[p] + threadIdx.x; f < filt_ptr[p + 1]; f += 256) {
      const int j = filt_ids[f];
      if (j == tgt) continue;
      cnt += rank_ahead(0.0f, j, ts, tgt) - rank_ahead(rank_sigmoid(srow[j]), j, ts, tgt);
    }
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) ranks[p] = red[0] + red[1] + red[2] + red[3] + 1;
}

}  // namespace temp

using namespace temp;

extern "C" {

static int bilinear_query_args(int P, int d, int kind, const void* a, const void* b, const void* c, const void* e, const void* f) {
  if (P < 0 || d <= 0 || (kind != TEMP_SCORE_DISTMULT && kind != TEMP_SCORE_COMPLEX && kind != TEMP_SCORE_TRANSE)) return TEMP_E_BADARG;
  if (kind == TEMP_SCORE_COMPLEX ? d % 8 : d % 4) return TEMP_E_UNSUPPORTED;
  if (P > 0 && (!a || !b || !c || !e || (kind != TEMP_SCORE_DISTMULT && !f))) return TEMP_E_BADARG;
  return TEMP_OK;
}

int temp_bilinear_query_fwd(int P, int d, int kind, const float* ent_rows, const int32_t* known_idx, const float* rel, const int32_t* rel_idx,
                            const int32_t* is_tail, float* q, void* stream) {
  int rc = bilinear_query_args(P, d, kind, ent_rows, known_idx, rel, rel_idx, is_tail);
  if (rc != TEMP_OK || P == 0) return rc;
  if (!q) return TEMP_E_BADARG;
  int grid = ceil_div((long long)P * (d / 4), 256);
  if (grid > 8192) grid = 8192;
  TEMP_LAUNCH(K_GATHER_CE, k_bilinear_query<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, P, d, kind, ent_rows, known_idx, rel, rel_idx, is_tail,
              (const float*)nullptr, q, (float*)nullptr);
  return launch_status();
}

int temp_bilinear_query_bwd(int P, int d, int kind, const float* ent_rows, const int32_t* known_idx, const float* rel, const int32_t* rel_idx,
                            const int32_t* is_tail, const float* d_q, float* d_known_rows, float* d_rel_rows, void* stream) {
  int rc = bilinear_query_args(P, d, kind, ent_rows, known_idx, rel, rel_idx, is_tail);
  if (rc != TEMP_OK || P == 0) return rc;
  if (!d_q || !d_known_rows || !d_rel_rows) return TEMP_E_BADARG;
  int grid = ceil_div((long long)P * (d / 4), 256);
  if (grid > 8192) grid = 8192;
  TEMP_LAUNCH(K_GATHER_CE, k_bilinear_query<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, P, d, kind, ent_rows, known_idx, rel, rel_idx, is_tail,
              d_q, d_known_rows, d_rel_rows);
  return launch_status();
}

int temp_gather_ce_fwd(int P, int C, int N, const float* scores, const int32_t* cand, float* loss_rows, float* lse_rows, void* stream) {
  if (P < 0 || C <= 0 || N <= 0 || (P > 0 && (!scores || !cand || !loss_rows || !lse_rows))) return TEMP_E_BADARG;
  if (P == 0) return TEMP_OK;
  if (2 * (long long)C >= N && N <= 1024)
    TEMP_LAUNCH(K_GATHER_CE, k_gather_ce_fwd_cnt_w, dim3(ceil_div(P, 4)), dim3(256), (size_t)4 * N * sizeof(int), (hipStream_t)stream, P, C, N, scores, cand, loss_rows, lse_rows);
  else if (2 * (long long)C >= N && (size_t)N * sizeof(int) <= 64 * 1024) {
    const size_t lds = (size_t)N * sizeof(int);
    if (lds + 64 > 65536) {                             // with the kernel's static `red` the workgroup is past the default 64 KB
      if (hipFuncSetAttribute((const void*)k_gather_ce_fwd_cnt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return TEMP_E_LAUNCH;
    }
    TEMP_LAUNCH(K_GATHER_CE, k_gather_ce_fwd_cnt, dim3(P), dim3(256), lds, (hipStream_t)stream, C, N, scores, cand, loss_rows, lse_rows);
  } else
    TEMP_LAUNCH(K_GATHER_CE, k_gather_ce_fwd, dim3(P), dim3(256), 0, (hipStream_t)stream, C, N, scores, cand, loss_rows, lse_rows);
  return launch_status();
}

int temp_gather_ce_bwd(int P, int C, int N, const float* scores, const int32_t* cand, const float* lse_rows, const float* scale,
                       float inv_rows, const float* row_scale, float* d_scores, void* stream) {
  if (P < 0 || C <= 0 || N <= 0 || !scale || (P > 0 && (!scores || !cand || !lse_rows || !d_scores))) return TEMP_E_BADARG;
  if ((size_t)N * sizeof(float) > 160 * 1024 - 1024) return TEMP_E_UNSUPPORTED;
  if (P == 0) return TEMP_OK;
  if (N <= 1024) {
    TEMP_LAUNCH(K_GATHER_CE, k_gather_ce_bwd_w, dim3(ceil_div(P, 4)), dim3(256), (size_t)4 * N * sizeof(int), (hipStream_t)stream, P, C, N, scores, cand, lse_rows, scale,
                inv_rows, row_scale, d_scores);
    return launch_status();
  }
  const size_t lds = (size_t)N * sizeof(float);
  if (lds > 65536) {
    if (hipFuncSetAttribute((const void*)k_gather_ce_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return TEMP_E_LAUNCH;
  }
  TEMP_LAUNCH(K_GATHER_CE, k_gather_ce_bwd, dim3(P), dim3(256), lds, (hipStream_t)stream, C, N, scores, cand, lse_rows, scale, inv_rows, row_scale, d_scores);
  return launch_status();
}

static int l1_ce_args(int P, int C, int d) {
  if (P < 0 || C <= 0 || d <= 0) return TEMP_E_BADARG;
  if (d % 4 || (long long)P * C >= (1ll << 31)) return TEMP_E_UNSUPPORTED;
  return TEMP_OK;
}

int temp_l1_ce_fwd(int P, int C, int d, const float* q, const float* table, const int32_t* base, const int32_t* cand, float* s_out,
                   float* loss_rows, float* lse_rows, void* stream) {
  const int rc = l1_ce_args(P, C, d);
  if (rc != TEMP_OK || P == 0) return rc;
  if (!q || !table || !cand || !s_out || !loss_rows || !lse_rows) return TEMP_E_BADARG;
#define L1_FWD(NP) TEMP_LAUNCH(K_GATHER_CE, k_l1_ce_fwd<NP>, dim3(P), dim3(256), 0, (hipStream_t)stream, C, d, q, table, base, cand, s_out, loss_rows, lse_rows)
  if (d <= 64) L1_FWD(1);
  else if (d <= 128) L1_FWD(2);
  else if (d <= 192) L1_FWD(3);
  else if (d <= 256) L1_FWD(4);
  else L1_FWD(0);
#undef L1_FWD
  return launch_status();
}

int temp_l1_ce_bwd_q(int P, int C, int d, const float* q, const float* table, const int32_t* base, const int32_t* cand, const float* s,
                     const float* lse_rows, const float* scale, float inv_rows, const float* row_scale, float* g_out, float* d_q, void* stream) {
  const int rc = l1_ce_args(P, C, d);
  if (rc != TEMP_OK) return rc;
  if (!scale) return TEMP_E_BADARG;
  if (P == 0) return TEMP_OK;
  if (!q || !table || !cand || !s || !lse_rows || !g_out || !d_q) return TEMP_E_BADARG;
  TEMP_LAUNCH(K_GATHER_CE, k_l1_ce_bwd_q, dim3(P), dim3(256), 0, (hipStream_t)stream, C, d, q, table, base, cand, s, lse_rows, scale, inv_rows, row_scale,
              g_out, d_q);
  return launch_status();
}

int temp_l1_ce_bwd_table(int n_rows, int d, int C, const float* q, const float* table, const int32_t* slot_ptr, const int32_t* slot, const float* g,
                         float* d_table, void* stream) {
  if (n_rows < 0 || C <= 0 || d <= 0) return TEMP_E_BADARG;
  if (d % 4) return TEMP_E_UNSUPPORTED;
  if (n_rows == 0) return TEMP_OK;
  if (!table || !slot_ptr || !d_table) return TEMP_E_BADARG;          // q, slot and g may be NULL when every list is empty
  TEMP_LAUNCH(K_GATHER_CE, k_l1_ce_bwd_table, dim3(n_rows), dim3(256), 0, (hipStream_t)stream, d, C, q, table, slot_ptr, slot, g, d_table);
  return launch_status();
}

int temp_l1_scores(int P, int N, int d, const float* q, const float* table, int ld, float* scores, void* stream) {
  if (P < 0 || N <= 0 || d <= 0 || ld < N) return TEMP_E_BADARG;
  if (d % 4 || ld % 4 || ceil_div(P, L1S_TILE) > 65535) return TEMP_E_UNSUPPORTED;
  if (P == 0) return TEMP_OK;
  if (!q || !table || !scores) return TEMP_E_BADARG;
  TEMP_LAUNCH(K_GATHER_CE, k_l1_scores, dim3(ceil_div(ld, L1S_TILE), ceil_div(P, L1S_TILE)), dim3(256), 0, (hipStream_t)stream, P, N, d, q, table, ld, scores);
  return launch_status();
}

int temp_l1_mix_ce_fwd(int P, int C, int d, const float* q, const float* table_a, const float* table_b, const float* w, const int32_t* base,
                       const int32_t* cand, float* s_out, float* loss_rows, float* lse_rows, void* stream) {
  const int rc = l1_ce_args(P, C, d);
  if (rc != TEMP_OK || P == 0) return rc;
  if (!q || !table_a || !table_b || !w || !cand || !s_out || !loss_rows || !lse_rows) return TEMP_E_BADARG;
#define L1M_FWD(NP) TEMP_LAUNCH(K_GATHER_CE_MIX, k_l1_mix_ce_fwd<NP>, dim3(P), dim3(256), 0, (hipStream_t)stream, C, d, q, table_a, table_b, w, base, cand, s_out, loss_rows, lse_rows)
  if (d <= 64) L1M_FWD(1);
  else if (d <= 128) L1M_FWD(2);
  else if (d <= 192) L1M_FWD(3);
  else if (d <= 256) L1M_FWD(4);
  else L1M_FWD(0);
#undef L1M_FWD
  return launch_status();
}

int temp_l1_mix_ce_bwd_q(int P, int C, int d, const float* q, const float* table_a, const float* table_b, const float* w, const int32_t* base,
                         const int32_t* cand, const float* s, const float* lse_rows, const float* scale, float inv_rows, const float* row_scale,
                         float* g_out, float* d_q, float* d_w, void* stream) {
  const int rc = l1_ce_args(P, C, d);
  if (rc != TEMP_OK) return rc;
  if (!scale) return TEMP_E_BADARG;
  if (P == 0) return TEMP_OK;
  if (!q || !table_a || !table_b || !w || !cand || !s || !lse_rows || !g_out || !d_q || !d_w) return TEMP_E_BADARG;
  TEMP_LAUNCH(K_GATHER_CE_MIX, k_l1_mix_ce_bwd_q, dim3(P), dim3(256), 0, (hipStream_t)stream, C, d, q, table_a, table_b, w, base, cand, s, lse_rows,
              scale, inv_rows, row_scale, g_out, d_q, d_w);
  return launch_status();
}

int temp_l1_mix_ce_bwd_table(int n_rows, int d, int C, const float* q, const float* table_a, const float* table_b, const float* w,
                             const int32_t* slot_ptr, const int32_t* slot, const float* g, float* d_table_a, float* d_table_b, void* stream) {
  if (n_rows < 0 || C <= 0 || d <= 0) return TEMP_E_BADARG;
  if (d % 4) return TEMP_E_UNSUPPORTED;
  if (n_rows == 0) return TEMP_OK;
  if (!table_a || !table_b || !slot_ptr || !d_table_a || !d_table_b) return TEMP_E_BADARG;   // q, w, slot and g may be NULL when every list is empty
  TEMP_LAUNCH(K_GATHER_CE_MIX, k_l1_mix_ce_bwd_table, dim3(n_rows), dim3(256), 0, (hipStream_t)stream, d, C, q, table_a, table_b, w, slot_ptr, slot, g,
              d_table_a, d_table_b);
  return launch_status();
}

int temp_l1_mix_scores(int P, int N, int d, const float* q, const float* table_a, const float* table_b, const float* w, int ld, float* scores,
                       void* stream) {
  if (P < 0 || N <= 0 || d <= 0 || ld < N) return TEMP_E_BADARG;
  if (d % 4 || ld % 4 || ceil_div(P, L1S_TILE) > 65535) return TEMP_E_UNSUPPORTED;
  if (P == 0) return TEMP_OK;
  if (!q || !table_a || !table_b || !w || !scores) return TEMP_E_BADARG;
  TEMP_LAUNCH(K_GATHER_CE_MIX, k_l1_mix_scores, dim3(ceil_div(ld, L1S_TILE), ceil_div(P, L1S_TILE)), dim3(256), 0, (hipStream_t)stream, P, N, d, q,
              table_a, table_b, w, ld, scores);
  return launch_status();
}

int temp_corrupt_sample(int R, int K, int N, uint64_t seed, const int32_t* truth, const int32_t* lo, const int32_t* hi, const int32_t* ids,
                        int32_t* cand, void* stream) {
  if (R < 0 || K < 0 || N <= 0 || (R > 0 && (!truth || !cand)) || ((lo != nullptr) != (hi != nullptr))) return TEMP_E_BADARG;
  if (R == 0) return TEMP_OK;
  const long long total = (long long)R * (K + 1);
  int grid = ceil_div(total, 256);
  if (grid > 16384) grid = 16384;
  TEMP_LAUNCH(K_GATHER_CE, k_corrupt_sample, dim3(grid), dim3(256), 0, (hipStream_t)stream, total, K + 1, N, (unsigned long long)seed, truth, lo, hi, ids, cand);
  return launch_status();
}

int temp_filtered_rank(int P, int N, int ld, const float* scores, const int32_t* target, const int32_t* filt_ptr,
                       const int32_t* filt_ids, int32_t* ranks, void* stream) {
  if (P < 0 || N <= 0 || ld < N || ld % 4 || (P > 0 && (!scores || !target || !ranks))) return TEMP_E_BADARG;
  if (P == 0) return TEMP_OK;
  TEMP_LAUNCH(K_GATHER_CE, k_filtered_rank, dim3(P), dim3(256), 0, (hipStream_t)stream, N, ld, scores, target, filt_ptr, filt_ids, ranks);
  return launch_status();
}

}  // extern "C"
