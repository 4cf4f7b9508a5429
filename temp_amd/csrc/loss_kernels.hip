// Loss and evaluation kernels: candidate-list cross-entropy, the folded query of the scorers (TransE's translation query among
// them; its L1 candidate loss and dense scores are in l1_loss.hip), filtered negative sampling, the filtered rank (whole rows, and
// streamed over column panels with a carry, plain and gate-mixed) and the all-entity cross-entropy under the same filter, with
// their entry points.
#include "common.hpp"
#include "mix.hpp"
#include "reduce.hpp"
#include "row_filter.hpp"

namespace temp {

// ---------------------------------------------------------------------------------------------
// Link-prediction loss over candidate lists (TKG_Module.train_link_prediction, models/TKG_Module.py:202-213):
// the scores of every positive against ALL entities come from one MFMA GEMM (query . all_embeds^T);
// these kernels pick the 1 + negative_rate candidates of each row out of that matrix and do the
// cross-entropy with label 0 -- nothing of shape (P, 1+neg, D) is ever materialised.
// One workgroup per row.
// ---------------------------------------------------------------------------------------------
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
    mx = block_max_256(mx, red);
#pragma unroll
    for (int u = 0; u < 4; ++u) sum += expf(v[u] - mx);                 // exp(-inf) = 0 for the padding
  } else {
    for (int k = threadIdx.x; k < C; k += 256) mx = fmaxf(mx, srow[crow[k]]);
    mx = block_max_256(mx, red);
    for (int k = threadIdx.x; k < C; k += 256) sum += expf(srow[crow[k]] - mx);
  }
  sum = block_sum_256(sum, red);
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
  mx = block_max_256(mx, red);
  float sum = 0.f;
  for (int i = threadIdx.x; i < N; i += 256)
    if (cnt[i]) sum += (float)cnt[i] * expf(srow[i] - mx);
  sum = block_sum_256(sum, red);
  if (threadIdx.x == 0) {
    const float lse = mx + logf(sum);
    lse_rows[p] = lse;
    loss_rows[p] = lse - srow[crow[0]];
  }
}

// The same for SHORT score rows (N <= 1024: GDELT's 500 entities under 48 000 loss rows): one WAVE per row, four rows per
// workgroup -- no workgroup barriers, no cross-wave reductions (the counters: gather_ce_wave_counts, reduce.hpp).
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
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int u = 0; u < 16; ++u)
    if (cv[u]) sum += (float)cv[u] * expf(sv[u] - mx);
  sum = wave_sum(sum);
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
// (one IEEE add / subtract per element: bit-equal to the tensor expression), and the pair fold of SimplE (utils/scores.py:14-24) over
// PAIR rows k = [e | e_inv], r = [rel | rel_inv] of width d = 2 h, candidates c = [o | o_inv]:
//   SimplE, tail mode   q = 1/2 [k_inv r_inv | k_fwd r_fwd]      SimplE, head mode   q = 1/2 [k_inv r_fwd | k_fwd r_inv]
// so that <q, c> is the mean of the two DistMult directions (the factor 1/2 is exact: every element is ONE rounded product).
// One thread per float4 of the half width; the backward writes the per-row
// gradients of k and r (the caller reduces them over the static index lists with temp_segment_sum_rows).
// ---------------------------------------------------------------------------------------------
template <bool BWD>
__global__ void __launch_bounds__(256) k_bilinear_query(int P, int d, int kind, const float* __restrict__ ent_rows, const int32_t* __restrict__ known_idx,
                                                        const float* __restrict__ rel, const int32_t* __restrict__ rel_idx,
                                                        const int32_t* __restrict__ is_tail, const float* __restrict__ dq, float* __restrict__ o0,
                                                        float* __restrict__ o1) {
  const int half = (kind == TEMP_SCORE_COMPLEX || kind == TEMP_SCORE_SIMPLE) ? d / 2 : d;
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
    if (kind == TEMP_SCORE_SIMPLE) {
      // q[:h] = 1/2 k[h:] rx, q[h:] = 1/2 k[:h] ry with (rx, ry) = (r[h:], r[:h]) for the tail mode and (r[:h], r[h:]) for the head mode
      const int tail = is_tail[p];
      const int ox = tail ? half : 0, oy = half - ox;               // where rx / ry sit in the relation row
      const float4 kf = ld4(k), ki = ld4(k + half), rx = ld4(r + ox), ry = ld4(r + oy);
      if (!BWD) {
        st4(o0 + o, make_float4(0.5f * (ki.x * rx.x), 0.5f * (ki.y * rx.y), 0.5f * (ki.z * rx.z), 0.5f * (ki.w * rx.w)));
        st4(o0 + o + half, make_float4(0.5f * (kf.x * ry.x), 0.5f * (kf.y * ry.y), 0.5f * (kf.z * ry.z), 0.5f * (kf.w * ry.w)));
      } else {
        const float4 a = ld4(dq + o), b = ld4(dq + o + half);
        st4(o0 + o, make_float4(0.5f * (b.x * ry.x), 0.5f * (b.y * ry.y), 0.5f * (b.z * ry.z), 0.5f * (b.w * ry.w)));                 // d k[:h]
        st4(o0 + o + half, make_float4(0.5f * (a.x * rx.x), 0.5f * (a.y * rx.y), 0.5f * (a.z * rx.z), 0.5f * (a.w * rx.w)));          // d k[h:]
        st4(o1 + o + ox, make_float4(0.5f * (a.x * ki.x), 0.5f * (a.y * ki.y), 0.5f * (a.z * ki.z), 0.5f * (a.w * ki.w)));            // d rx
        st4(o1 + o + oy, make_float4(0.5f * (b.x * kf.x), 0.5f * (b.y * kf.y), 0.5f * (b.z * kf.z), 0.5f * (b.w * kf.w)));            // d ry
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

// ---------------------------------------------------------------------------------------------
// All-entity cross-entropy under the row's known-true filter (include/temp_amd.h: temp_filtered_ce_*): every admissible entity
// of the row exactly once -- the truth, and whatever is not in ids[lo[p] .. hi[p]).  The score row is STREAMED: a wave takes 256
// consecutive columns per step (one float4 per lane), so nothing is counted in LDS and N has no ceiling.
// Dispatch (both kernels): N <= FCE_WAVE_MAX_N (1024) -- one WAVE per row, four rows per workgroup, steps of 256 columns, no
// barrier; above it one 256-thread workgroup per row, wave w on the steps w, w + 4, ... and one cross-wave reduction at the end.
// The filter EXCLUDES: a listed entity gets the weight 0 before anything is summed (sum-then-subtract would cancel -- the listed
// entities are the best-scored ones).  The ascending list is walked beside the ascending column steps, 64 entries at a time in
// the wave's registers (row_filter.hpp, shared with the streamed rank below).
// ---------------------------------------------------------------------------------------------
#define FCE_WAVE_MAX_N 1024

template <bool GROUP>
__global__ void __launch_bounds__(256) k_filtered_ce_fwd(int P, int N, int ld, int col0, const float* __restrict__ scores, const int32_t* __restrict__ truth,
                                                         const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, const int32_t* __restrict__ ids,
                                                         int carry, float* __restrict__ run_max, float* __restrict__ run_sum,
                                                         float* __restrict__ truth_score, float* __restrict__ lse_rows, float* __restrict__ loss_rows) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int p = GROUP ? blockIdx.x : blockIdx.x * 4 + w;
  if (!GROUP && p >= P) return;                                           // (a whole wave: the wave route has no barrier)
  const float* srow = scores + (size_t)p * ld;
  const int tr = truth[p];
  RowFilter f = filter_open(lo, hi, ids, p, lane);
  float m = -INFINITY, s = 0.f;                                           // this lane's running (max, sum exp(. - max))
  for (int c = GROUP ? w * 256 : 0; c < N; c += GROUP ? 1024 : 256) {
    const unsigned mask = filter_mask(f, col0 + c, lane);
    const int j = c + lane * 4;
    if (j < N) {
      const float4 x = filter_select(ld4(srow + j), mask, col0 + j, tr, N - j, -INFINITY);
      const float mn = fmaxf(fmaxf(m, fmaxf(x.x, x.y)), fmaxf(x.z, x.w));
      if (mn > -INFINITY) {                                               // (else nothing admissible so far: no -inf - -inf)
        s = s * expf(m - mn) + ((expf(x.x - mn) + expf(x.y - mn)) + (expf(x.z - mn) + expf(x.w - mn)));
        m = mn;
      }
    }
  }
  const float M = GROUP ? block_max_256(m, red) : wave_max(m);
  const float part = m > -INFINITY ? s * expf(m - M) : 0.f;
  const float S = GROUP ? block_sum_256(part, red) : wave_sum(part);
  if (GROUP ? threadIdx.x == 0 : lane == 0) {
    float rm = M, rs = S;
    if (carry) {
      const float om = run_max[p], os = run_sum[p];
      rm = fmaxf(om, M);
      rs = (om > -INFINITY ? os * expf(om - rm) : 0.f) + (M > -INFINITY ? S * expf(M - rm) : 0.f);     // expf(0) = 1: an empty panel changes nothing
    }
    const int jt = tr - col0;
    const float ts = (jt >= 0 && jt < N) ? srow[jt] : (carry ? truth_score[p] : 0.f);
    const float lse = rm + logf(rs);
    run_max[p] = rm;
    run_sum[p] = rs;
    truth_score[p] = ts;
    lse_rows[p] = lse;
    loss_rows[p] = lse - ts;
  }
}

template <bool GROUP>
__global__ void __launch_bounds__(256) k_filtered_ce_bwd(int P, int N, int ld, int col0, const float* __restrict__ scores, const int32_t* __restrict__ truth,
                                                         const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, const int32_t* __restrict__ ids,
                                                         const float* __restrict__ lse_rows, const float* __restrict__ scale_ptr, float inv_rows,
                                                         const float* __restrict__ row_scale, float* __restrict__ d_scores) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int p = GROUP ? blockIdx.x : blockIdx.x * 4 + w;
  if (!GROUP && p >= P) return;
  const float* srow = scores + (size_t)p * ld;
  float* drow = d_scores + (size_t)p * ld;
  const int tr = truth[p];
  const float lse = lse_rows[p];
  const float scale = scale_ptr[0] * (row_scale ? row_scale[p] : inv_rows);
  RowFilter f = filter_open(lo, hi, ids, p, lane);
  for (int c = GROUP ? w * 256 : 0; c < ld; c += GROUP ? 1024 : 256) {     // (to ld: the pad columns are written too)
    const unsigned mask = c < N ? filter_mask(f, col0 + c, lane) : 0u;     // (c is the same in all 64 lanes)
    const int j = c + lane * 4;
    if (j >= ld) continue;
    float4 g = zero4();
    if (j < N && scale != 0.f) {                                          // a weight-0 row is exactly 0 whatever its lse
      const float4 x = filter_select(ld4(srow + j), mask, col0 + j, tr, N - j, -INFINITY);
      const unsigned t = (int)(tr - col0 - j) < N - j ? (unsigned)(tr - col0 - j) : 4u;        // the truth's place among the four, if it is there
      g = make_float4(x.x > -INFINITY ? expf(x.x - lse) : 0.f, x.y > -INFINITY ? expf(x.y - lse) : 0.f,      // filtered and pad columns: 0
                      x.z > -INFINITY ? expf(x.z - lse) : 0.f, x.w > -INFINITY ? expf(x.w - lse) : 0.f);
      g = make_float4(g.x - (t == 0u ? 1.f : 0.f), g.y - (t == 1u ? 1.f : 0.f), g.z - (t == 2u ? 1.f : 0.f), g.w - (t == 3u ? 1.f : 0.f));
      g = scale4(g, scale);
    }
    st4(drow + j, g);
  }
}

// ---------------------------------------------------------------------------------------------
// Streamed filtered rank (include/temp_amd.h: temp_filtered_rank_stream*): k_filtered_rank's definition on a COLUMN PANEL of the
// row, entities col0 .. col0 + N - 1, with the target's score and the count carried from panel to panel.  The row is streamed as
// in k_filtered_ce_fwd (one float4 per lane, 256 columns per wave step; MIX: two float4 and mix4 in registers) with the filter
// list walked beside it: a listed entity that is not the target gets -inf, which rank_sigmoid turns into exactly 0 -- its VALUE,
// it is still compared -- and a column j >= N is left out BY INDEX (`left`), whatever it holds: in a panel that is not the last
// its would-be id lies below later targets.  No second pass, no random access into the row but the one read of the target's
// column.  The target's own column goes through the same mix1 and rank_sigmoid as `ts`, compares equal and is not ahead.
// Dispatch as the filtered cross-entropy's; TEMP_RANK_COLLECT reads one column per row and always takes the wave route.
// ---------------------------------------------------------------------------------------------
template <bool MIX>
__device__ __forceinline__ float rank_stream_score(const float* __restrict__ arow, const float* __restrict__ brow, float w, int j) {
  return MIX ? mix1(w, arow[j], brow[j]) : arow[j];
}

template <bool MIX, bool GROUP>
__global__ void __launch_bounds__(256) k_filtered_rank_stream(int P, int N, int ld, int col0, const float* __restrict__ scores_a,
                                                              const float* __restrict__ scores_b, const float* __restrict__ wrow,
                                                              const int32_t* __restrict__ target, const int32_t* __restrict__ filt_ptr,
                                                              const int32_t* __restrict__ filt_ids, int mode, float* __restrict__ target_score,
                                                              int32_t* __restrict__ count, int32_t* __restrict__ ranks) {
  __shared__ int red[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int p = GROUP ? blockIdx.x : blockIdx.x * 4 + w;
  if (!GROUP && p >= P) return;                                           // (a whole wave: the wave route has no barrier)
  const float* arow = scores_a + (size_t)p * ld;
  const float* brow = MIX ? scores_b + (size_t)p * ld : nullptr;
  const float wp = MIX ? wrow[p] : 0.f;
  const int tgt = target[p];
  const int jt = tgt - col0;
  const bool inside = jt >= 0 && jt < N;
  if (mode == TEMP_RANK_COLLECT) {
    if (inside && lane == 0 && (!GROUP || w == 0)) target_score[p] = rank_stream_score<MIX>(arow, brow, wp, jt);
    return;
  }
  // (TEMP_RANK_WHOLE with a target outside the panel breaks the contract: nothing is read out of bounds, the rank is that of a score of -inf)
  const float ts = rank_sigmoid(mode == TEMP_RANK_WHOLE ? (inside ? rank_stream_score<MIX>(arow, brow, wp, jt) : -INFINITY) : target_score[p]);
  RowFilter f = filter_open(filt_ptr, filt_ptr ? filt_ptr + 1 : nullptr, filt_ids, p, lane);
  int cnt = 0;
  for (int c = GROUP ? w * 256 : 0; c < N; c += GROUP ? 1024 : 256) {
    const unsigned mask = filter_mask(f, col0 + c, lane);
    const int j = c + lane * 4;
    if (j < N) {
      const int left = N - j, e = col0 + j;
      const float4 raw = MIX ? mix4(wp, ld4(arow + j), ld4(brow + j)) : ld4(arow + j);
      const float4 x = filter_select(raw, mask, e, tgt, left, -INFINITY);
      cnt += rank_ahead(rank_sigmoid(x.x), e, ts, tgt) + ((left > 1) & rank_ahead(rank_sigmoid(x.y), e + 1, ts, tgt))
           + ((left > 2) & rank_ahead(rank_sigmoid(x.z), e + 2, ts, tgt)) + ((left > 3) & rank_ahead(rank_sigmoid(x.w), e + 3, ts, tgt));
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if (GROUP) {
    if (lane == 0) red[w] = cnt;
    __syncthreads();
    cnt = (red[0] + red[1]) + (red[2] + red[3]);
  }
  if (GROUP ? threadIdx.x == 0 : lane == 0) {
    if (mode == TEMP_RANK_COUNT_ADD) cnt += count[p];
    if (mode != TEMP_RANK_WHOLE) count[p] = cnt;
    ranks[p] = cnt + 1;
  }
}

}  // namespace temp

using namespace temp;

extern "C" {

static int bilinear_query_args(int P, int d, int kind, const void* a, const void* b, const void* c, const void* e, const void* f) {
  if (P < 0 || d <= 0 || (kind != TEMP_SCORE_DISTMULT && kind != TEMP_SCORE_COMPLEX && kind != TEMP_SCORE_TRANSE && kind != TEMP_SCORE_SIMPLE))
    return TEMP_E_BADARG;
  if ((kind == TEMP_SCORE_COMPLEX || kind == TEMP_SCORE_SIMPLE) ? d % 8 : d % 4) return TEMP_E_UNSUPPORTED;
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

static int filtered_ce_args(int P, int N, int ld, int col0, const void* scores, const void* truth, const void* lo, const void* hi, const void* out) {
  if (P < 0 || N <= 0 || ld < N || col0 < 0 || (long long)col0 + ld + 256 >= 0x7fffffffLL || ((lo != nullptr) != (hi != nullptr))) return TEMP_E_BADARG;
  if (P > 0 && (!scores || !truth || !out)) return TEMP_E_BADARG;
  if (ld % 4 || (uintptr_t)scores % 16 || (uintptr_t)out % 16) return TEMP_E_UNSUPPORTED;
  return TEMP_OK;
}

int temp_filtered_ce_fwd(int P, int N, int ld, int col0, const float* scores, const int32_t* truth, const int32_t* lo, const int32_t* hi,
                         const int32_t* ids, int carry, float* run_max, float* run_sum, float* truth_score, float* lse_rows, float* loss_rows,
                         void* stream) {
  int rc = filtered_ce_args(P, N, ld, col0, scores, truth, lo, hi, scores);
  if (rc == TEMP_OK && ((carry != 0 && carry != 1) || (P > 0 && (!run_max || !run_sum || !truth_score || !lse_rows || !loss_rows)))) rc = TEMP_E_BADARG;
  if (rc != TEMP_OK || P == 0) return rc;
  if (N <= FCE_WAVE_MAX_N)
    TEMP_LAUNCH(K_FILTERED_CE_FWD, k_filtered_ce_fwd<false>, dim3(ceil_div(P, 4)), dim3(256), 0, (hipStream_t)stream, P, N, ld, col0, scores, truth, lo, hi, ids,
                carry, run_max, run_sum, truth_score, lse_rows, loss_rows);
  else
    TEMP_LAUNCH(K_FILTERED_CE_FWD, k_filtered_ce_fwd<true>, dim3(P), dim3(256), 0, (hipStream_t)stream, P, N, ld, col0, scores, truth, lo, hi, ids, carry,
                run_max, run_sum, truth_score, lse_rows, loss_rows);
  return launch_status();
}

int temp_filtered_ce_bwd(int P, int N, int ld, int col0, const float* scores, const int32_t* truth, const int32_t* lo, const int32_t* hi,
                         const int32_t* ids, const float* lse_rows, const float* scale, float inv_rows, const float* row_scale, float* d_scores,
                         void* stream) {
  int rc = filtered_ce_args(P, N, ld, col0, scores, truth, lo, hi, d_scores);
  if (rc == TEMP_OK && (!scale || (P > 0 && !lse_rows))) rc = TEMP_E_BADARG;
  if (rc != TEMP_OK || P == 0) return rc;
  if (N <= FCE_WAVE_MAX_N)
    TEMP_LAUNCH(K_FILTERED_CE_BWD, k_filtered_ce_bwd<false>, dim3(ceil_div(P, 4)), dim3(256), 0, (hipStream_t)stream, P, N, ld, col0, scores, truth, lo, hi, ids,
                lse_rows, scale, inv_rows, row_scale, d_scores);
  else
    TEMP_LAUNCH(K_FILTERED_CE_BWD, k_filtered_ce_bwd<true>, dim3(P), dim3(256), 0, (hipStream_t)stream, P, N, ld, col0, scores, truth, lo, hi, ids, lse_rows,
                scale, inv_rows, row_scale, d_scores);
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

// the argument checks of both streamed-rank entry points (include/temp_amd.h); TEMP_OK with *launch = false for P == 0
static int rank_stream_check(int P, int N, int ld, int col0, const float* a, const float* b, const float* w, bool mix, const void* target, int mode,
                             const void* target_score, const void* count, const void* ranks, bool* launch) {
  *launch = false;
  if (P < 0 || N <= 0 || ld < N || col0 < 0 || (long long)col0 + ld + 256 >= 0x7fffffffLL || mode < TEMP_RANK_WHOLE || mode > TEMP_RANK_COUNT_ADD)
    return TEMP_E_BADARG;
  if (P > 0) {
    if (!a || !target || (mix && (!b || !w))) return TEMP_E_BADARG;
    if (mode == TEMP_RANK_COLLECT ? !target_score : !ranks) return TEMP_E_BADARG;
    if ((mode == TEMP_RANK_COUNT_FIRST || mode == TEMP_RANK_COUNT_ADD) && (!target_score || !count)) return TEMP_E_BADARG;
  }
  if (ld % 4 || (uintptr_t)a % 16 || (mix && (uintptr_t)b % 16)) return TEMP_E_UNSUPPORTED;
  *launch = P > 0;
  return TEMP_OK;
}

#define RANK_STREAM_LAUNCH(KID, MIX)                                                                                                              \
  do {                                                                                                                                            \
    if (N <= FCE_WAVE_MAX_N || mode == TEMP_RANK_COLLECT)                                                                                         \
      TEMP_LAUNCH(KID, (k_filtered_rank_stream<MIX, false>), dim3(ceil_div(P, 4)), dim3(256), 0, (hipStream_t)stream, P, N, ld, col0, scores_a,   \
                  scores_b, w, target, filt_ptr, filt_ids, mode, target_score, count, ranks);                                                     \
    else                                                                                                                                          \
      TEMP_LAUNCH(KID, (k_filtered_rank_stream<MIX, true>), dim3(P), dim3(256), 0, (hipStream_t)stream, P, N, ld, col0, scores_a, scores_b, w,    \
                  target, filt_ptr, filt_ids, mode, target_score, count, ranks);                                                                  \
  } while (0)

int temp_filtered_rank_stream(int P, int N, int ld, int col0, const float* scores, const int32_t* target, const int32_t* filt_ptr,
                              const int32_t* filt_ids, int mode, float* target_score, int32_t* count, int32_t* ranks, void* stream) {
  bool launch;
  const int rc = rank_stream_check(P, N, ld, col0, scores, nullptr, nullptr, false, target, mode, target_score, count, ranks, &launch);
  if (!launch) return rc;
  const float *scores_a = scores, *scores_b = nullptr, *w = nullptr;
  RANK_STREAM_LAUNCH(K_FILTERED_RANK_STREAM, false);
  return launch_status();
}

int temp_filtered_rank_stream_mix(int P, int N, int ld, int col0, const float* scores_a, const float* scores_b, const float* w,
                                  const int32_t* target, const int32_t* filt_ptr, const int32_t* filt_ids, int mode, float* target_score,
                                  int32_t* count, int32_t* ranks, void* stream) {
  bool launch;
  const int rc = rank_stream_check(P, N, ld, col0, scores_a, scores_b, w, true, target, mode, target_score, count, ranks, &launch);
  if (!launch) return rc;
  RANK_STREAM_LAUNCH(K_FILTERED_RANK_STREAM_MIX, true);
  return launch_status();
}
#undef RANK_STREAM_LAUNCH

}  // extern "C"
