// Gated link-prediction loss of the post-aggregation models (PostDynamicRGCN / PostBiDynamicRGCN.train_link_prediction,
// models/PostDynamicRGCN.py:261-282): the KNOWN entity is the per-triple mix w * local + (1 - w) * temporal of its two target rows,
// the candidates are the same mix of the two all-entity rows with a second weight.  DistMult and ComplEx are linear in the
// candidate, so the candidate mix is applied to the two score matrices (query . all_loc^T, query . all_rec^T) at the candidate
// columns only:  score_k = w * s_a[cand_k] + (1 - w) * s_b[cand_k]  -- no (P, C, D) tensor and no mixed (P, N) matrix.
//
//   k_gated_query<BWD>    one wave per row: the known-row mix, the bilinear fold of temp_bilinear_query, and in the backward the
//                         per-row gradients of both sources, the relation row and the mixing weight (wave reduction)
//   k_gather_ce_mix_fwd   one wave per row over the candidate list: logsumexp of the mixed candidate scores
//   k_gather_ce_mix_bwd*  the mixed-score gradient G written through both weights over the full row (multiplicities counted
//                         as in k_gather_ce_bwd) and d_w = sum_e G (s_a - s_b) in the same pass
//   k_frozen_mix_ce       frozen streams (Aggregator): the candidates scored straight from the two tables, loss rows and d_w in one launch
// No floating-point atomics and no workspace: every output element has one writer and every sum a fixed order.
#include "common.hpp"
#include "mix.hpp"
#include "reduce.hpp"

namespace temp {
namespace {

// (the mixing expression mix1 / mix4 of the forward and backward passes: mix.hpp)
__device__ __forceinline__ float4 sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }

// ---------------------------------------------------------------------------------------------
// Gated folded query.  Row p: known = ia[p] >= 0 ? w[p] A[ia[p]] + (1 - w[p]) B[ib[p]] : B[ib[p]] (temporal-only row), r = rel[rel_idx[p]]
//   DistMult            q = known * r
//   ComplEx, tail mode  q = [re_k re_r - im_k im_r | re_k im_r + im_k re_r]
//   ComplEx, head mode  q = [re_r re_k + im_r im_k | re_r im_k - im_r re_k]
//   TransE              q = known + r (tail) / known - r (head): one IEEE add / subtract after the mix (the translation query of
//                       k_bilinear_query); backward d_k = d_q, d_rel = +-d_q
// Backward (d_k = the adjoint of the fold, as in k_bilinear_query):  o0 = d_A rows = w d_k (0 on temporal-only rows),
// o1 = d_B rows = (1 - w) d_k (d_k), o2 = d_rel rows, dw[p] = <d_k, A[ia] - B[ib]> (0).
// ---------------------------------------------------------------------------------------------
template <bool BWD>
__global__ void __launch_bounds__(256) k_gated_query(int P, int d, int kind, const float* __restrict__ A, const int32_t* __restrict__ ia,
                                                     const float* __restrict__ B, const int32_t* __restrict__ ib, const float* __restrict__ w,
                                                     const float* __restrict__ rel, const int32_t* __restrict__ rel_idx,
                                                     const int32_t* __restrict__ is_tail, const float* __restrict__ dq, float* __restrict__ o0,
                                                     float* __restrict__ o1, float* __restrict__ o2, float* __restrict__ dw) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= P) return;
  const int a_row = ia[p];
  const bool gated = a_row >= 0;
  const float wp = gated ? w[p] : 0.f;
  const float* brow = B + (size_t)ib[p] * d;
  const float* arow = gated ? A + (size_t)a_row * d : brow;
  const float* rrow = rel + (size_t)rel_idx[p] * d;
  const size_t o = (size_t)p * d;
  float acc = 0.f;
  if (kind != TEMP_SCORE_COMPLEX) {
    for (int j = lane * 4; j < d; j += 256) {
      const float4 bv = ld4(brow + j), av = gated ? ld4(arow + j) : bv;
      const float4 kv = gated ? mix4(wp, av, bv) : bv, rv = ld4(rrow + j);
      if (kind == TEMP_SCORE_TRANSE) {
        const float sg = is_tail[p] ? 1.f : -1.f;       // sg * r is exact: known + sg * r rounds once, as known + r / known - r
        if (!BWD) {
          st4(o0 + o + j, make_float4(kv.x + sg * rv.x, kv.y + sg * rv.y, kv.z + sg * rv.z, kv.w + sg * rv.w));
          continue;
        }
        const float4 dk = ld4(dq + o + j);
        st4(o0 + o + j, gated ? scale4(dk, wp) : zero4());
        st4(o1 + o + j, gated ? scale4(dk, 1.f - wp) : dk);
        st4(o2 + o + j, scale4(dk, sg));
        if (gated) acc += dot4(dk, sub4(av, bv));
        continue;
      }
      if (!BWD) {
        st4(o0 + o + j, mul4(kv, rv));
        continue;
      }
      const float4 g = ld4(dq + o + j);
      const float4 dk = mul4(g, rv);
      st4(o0 + o + j, gated ? scale4(dk, wp) : zero4());
      st4(o1 + o + j, gated ? scale4(dk, 1.f - wp) : dk);
      st4(o2 + o + j, mul4(g, kv));
      if (gated) acc += dot4(dk, sub4(av, bv));
    }
  } else {
    const int half = d / 2;
    const float sg = is_tail[p] ? 1.f : -1.f;
    for (int j = lane * 4; j < half; j += 256) {
      const float4 rb = ld4(brow + j), ib4 = ld4(brow + j + half);
      const float4 ra = gated ? ld4(arow + j) : rb, ia4 = gated ? ld4(arow + j + half) : ib4;
      const float4 rk = gated ? mix4(wp, ra, rb) : rb, ik = gated ? mix4(wp, ia4, ib4) : ib4;
      const float4 rr = ld4(rrow + j), ir = ld4(rrow + j + half);
      if (!BWD) {
        st4(o0 + o + j, make_float4(rk.x * rr.x - sg * ik.x * ir.x, rk.y * rr.y - sg * ik.y * ir.y, rk.z * rr.z - sg * ik.z * ir.z,
                                    rk.w * rr.w - sg * ik.w * ir.w));
        st4(o0 + o + j + half, make_float4(ik.x * rr.x + sg * rk.x * ir.x, ik.y * rr.y + sg * rk.y * ir.y, ik.z * rr.z + sg * rk.z * ir.z,
                                           ik.w * rr.w + sg * rk.w * ir.w));
        continue;
      }
      const float4 a = ld4(dq + o + j), b = ld4(dq + o + j + half);
      // q1 = rk rr - sg ik ir ; q2 = ik rr + sg rk ir
      const float4 drk = make_float4(a.x * rr.x + sg * b.x * ir.x, a.y * rr.y + sg * b.y * ir.y, a.z * rr.z + sg * b.z * ir.z, a.w * rr.w + sg * b.w * ir.w);
      const float4 dik = make_float4(b.x * rr.x - sg * a.x * ir.x, b.y * rr.y - sg * a.y * ir.y, b.z * rr.z - sg * a.z * ir.z, b.w * rr.w - sg * a.w * ir.w);
      st4(o0 + o + j, gated ? scale4(drk, wp) : zero4());
      st4(o0 + o + j + half, gated ? scale4(dik, wp) : zero4());
      st4(o1 + o + j, gated ? scale4(drk, 1.f - wp) : drk);
      st4(o1 + o + j + half, gated ? scale4(dik, 1.f - wp) : dik);
      st4(o2 + o + j, make_float4(a.x * rk.x + b.x * ik.x, a.y * rk.y + b.y * ik.y, a.z * rk.z + b.z * ik.z, a.w * rk.w + b.w * ik.w));
      st4(o2 + o + j + half, make_float4(sg * (b.x * rk.x - a.x * ik.x), sg * (b.y * rk.y - a.y * ik.y), sg * (b.z * rk.z - a.z * ik.z),
                                         sg * (b.w * rk.w - a.w * ik.w)));
      if (gated) acc += dot4(drk, sub4(ra, rb)) + dot4(dik, sub4(ia4, ib4));
    }
  }
  if (BWD) {
    acc = wave_sum(acc);
    if (lane == 0) dw[p] = acc;
  }
}

// ---------------------------------------------------------------------------------------------
// Gated candidate cross-entropy, forward: one wave per row, the candidate list walked twice (max, then the exp-sum);
// a duplicate candidate counts once per occurrence, as in the reference's gathered (P, 1 + neg) score matrix.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_gather_ce_mix_fwd(int P, int C, int N, const float* __restrict__ s_a, const float* __restrict__ s_b,
                                                           const float* __restrict__ w, const int32_t* __restrict__ cand,
                                                           float* __restrict__ loss_rows, float* __restrict__ lse_rows) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= P) return;
  const float* ra = s_a + (size_t)p * N;
  const float* rb = s_b + (size_t)p * N;
  const int32_t* crow = cand + (size_t)p * C;
  const float wp = w[p];
  float mx = -INFINITY;
  for (int k = lane; k < C; k += 64) {
    const int c = crow[k];
    mx = fmaxf(mx, mix1(wp, ra[c], rb[c]));
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int k = lane; k < C; k += 64) {
    const int c = crow[k];
    sum += expf(mix1(wp, ra[c], rb[c]) - mx);
  }
  sum = wave_sum(sum);
  if (lane == 0) {
    const int t = crow[0];
    const float lse = mx + logf(sum);
    lse_rows[p] = lse;
    loss_rows[p] = lse - mix1(wp, ra[t], rb[t]);
  }
}

// Backward: G[e] = scale * (cnt[e] * exp(m[e] - lse) - [e == cand[0]]), m = the mixed score; d_s_a = w G, d_s_b = (1 - w) G over the
// FULL row (zero off-candidate), d_w = sum_e G[e] (s_a[e] - s_b[e]).  Multiplicities come from integer LDS counters (order-independent
// sums of integers, as in k_gather_ce_bwd), so the result does not depend on the order the candidates are visited in.
// Short rows (N <= 1024): one wave per row, four rows per workgroup; a wave's LDS operations complete in issue order.
__global__ void __launch_bounds__(256) k_gather_ce_mix_bwd_w(int P, int C, int N, const float* __restrict__ s_a, const float* __restrict__ s_b,
                                                             const float* __restrict__ w, const int32_t* __restrict__ cand,
                                                             const float* __restrict__ lse_rows, const float* __restrict__ scale_ptr, float inv_rows,
                                                             const float* __restrict__ row_scale, float* __restrict__ d_a, float* __restrict__ d_b,
                                                             float* __restrict__ d_w) {
  extern __shared__ int cnt_all[];
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= P) return;
  const int32_t* crow = cand + (size_t)p * C;
  const int* cnt = gather_ce_wave_counts(cnt_all, N, C, crow);
  const float* ra = s_a + (size_t)p * N;
  const float* rb = s_b + (size_t)p * N;
  const float wp = w[p], lse = lse_rows[p];
  const float scale = scale_ptr[0] * (row_scale ? row_scale[p] : inv_rows);
  const int truth = crow[0];
  float* da = d_a + (size_t)p * N;
  float* db = d_b + (size_t)p * N;
  float acc = 0.f;
  for (int i = lane; i < N; i += 64) {
    const int c = cnt[i];
    float g = 0.f;
    if (c) {
      const float a = ra[i], b = rb[i];
      g = (float)c * expf(mix1(wp, a, b) - lse);
      if (i == truth) g -= 1.f;
      g *= scale;
      acc += g * (a - b);
    }
    da[i] = wp * g;
    db[i] = (1.f - wp) * g;
  }
  acc = wave_sum(acc);
  if (lane == 0) d_w[p] = acc;
}

// Long rows: one workgroup per row, N counters in LDS.
__global__ void __launch_bounds__(256) k_gather_ce_mix_bwd(int C, int N, const float* __restrict__ s_a, const float* __restrict__ s_b,
                                                           const float* __restrict__ w, const int32_t* __restrict__ cand,
                                                           const float* __restrict__ lse_rows, const float* __restrict__ scale_ptr, float inv_rows,
                                                           const float* __restrict__ row_scale, float* __restrict__ d_a, float* __restrict__ d_b,
                                                           float* __restrict__ d_w) {
  extern __shared__ int cnt[];
  __shared__ float red[4];
  const int p = blockIdx.x;
  for (int i = threadIdx.x; i < N; i += 256) cnt[i] = 0;
  __syncthreads();
  const int32_t* crow = cand + (size_t)p * C;
  for (int k = threadIdx.x; k < C; k += 256) atomicAdd(&cnt[crow[k]], 1);
  __syncthreads();
  const float* ra = s_a + (size_t)p * N;
  const float* rb = s_b + (size_t)p * N;
  const float wp = w[p], lse = lse_rows[p];
  const float scale = scale_ptr[0] * (row_scale ? row_scale[p] : inv_rows);
  const int truth = crow[0];
  float* da = d_a + (size_t)p * N;
  float* db = d_b + (size_t)p * N;
  float acc = 0.f;
  for (int i = threadIdx.x; i < N; i += 256) {
    const int c = cnt[i];
    float g = 0.f;
    if (c) {
      const float a = ra[i], b = rb[i];
      g = (float)c * expf(mix1(wp, a, b) - lse);
      if (i == truth) g -= 1.f;
      g *= scale;
      acc += g * (a - b);
    }
    da[i] = wp * g;
    db[i] = (1.f - wp) * g;
  }
  acc = block_sum_256(acc, red);
  if (threadIdx.x == 0) d_w[p] = acc;
}

// ---------------------------------------------------------------------------------------------
// Frozen-ensemble candidate cross-entropy (Aggregator, models/aggregator.py:200-206, 339-342): both streams are frozen, so the only
// gradient is d loss / d w[p], and it has a closed form in the quantities of the forward:
//   x_c = mix1(w, a_c, b_c),   loss = logsumexp_c x_c - x_0,   d_w = scale (sum_c softmax_c (a_c - b_c) - (a_0 - b_0)).
// The candidate scores come straight from the tables (gather-dot / gather-L1): no (P, N) matrix, no saved tensor, no backward launch.
// One wave per row, four rows per workgroup.  The 64 lanes are four groups of 16: a group scores one candidate at a time, lane l of
// it holding the float4 slices l, l + 16, ... of the row's two queries in registers (NJ slices: widths up to 64 NJ) and reading the
// gathered table row as 16 x float4 per step; the 16 partial sums meet in DPP row rotations.  Every group runs its own online
// (m, s, u), u = sum_c e^(x_c - m) (a_c - b_c), over the candidates k = 4 i + group in ascending i, two candidates per step so that
// the second row's loads are in flight under the first one's reduction; the four triples are merged once, (0 + 1) + (2 + 3).  No LDS,
// no atomics: results are bit-repeatable.
// ---------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float dpp_row(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// sum over the 16 lanes of a DPP row (= one lane group), every lane of the row gets the same bits: row_ror 8, 4, 2, 1
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_row<0x128>(v);
  v += dpp_row<0x124>(v);
  v += dpp_row<0x122>(v);
  v += dpp_row<0x121>(v);
  return v;
}

struct OnlineMix {
  float m, s, u;
  __device__ __forceinline__ void add(float x, float dlt) {
    if (x > m) {                                        // (m = -inf at the start: e^(-inf) = 0 and s = u = 0)
      const float r = expf(m - x);
      s = fmaf(s, r, 1.f);
      u = fmaf(u, r, dlt);
      m = x;
    } else {                                            // (a NaN score lands here and poisons s and u)
      const float e = expf(x - m);
      s += e;
      u = fmaf(e, dlt, u);
    }
  }
};

template <int KIND, int NJ>
__device__ __forceinline__ float frozen_score(const float4 (&q)[NJ], const float* __restrict__ trow, int d, int l) {
  float4 t[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (j * 64 + l * 4 < d) t[j] = ld4(trow + j * 64 + l * 4);
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (j * 64 + l * 4 < d) {
      if (KIND == TEMP_FROZEN_DOT) {
        acc = fmaf(q[j].x, t[j].x, acc); acc = fmaf(q[j].y, t[j].y, acc); acc = fmaf(q[j].z, t[j].z, acc); acc = fmaf(q[j].w, t[j].w, acc);
      } else {
        acc += fabsf(q[j].x - t[j].x); acc += fabsf(q[j].y - t[j].y); acc += fabsf(q[j].z - t[j].z); acc += fabsf(q[j].w - t[j].w);
      }
    }
  acc = row16_sum(acc);
  return KIND == TEMP_FROZEN_DOT ? acc : -acc;
}

template <int KIND, int NJ>
__global__ void __launch_bounds__(256) k_frozen_mix_ce(int P, int C, int Da, int Db, const float* __restrict__ q_a, const float* __restrict__ T_a,
                                                       const float* __restrict__ q_b, const float* __restrict__ T_b, const float* __restrict__ w,
                                                       const int32_t* __restrict__ cand, const float* __restrict__ row_scale, float inv_rows,
                                                       float* __restrict__ loss_rows, float* __restrict__ d_w) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= P) return;
  const int grp = lane >> 4, l = lane & 15;
  float4 qa[NJ], qb[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (j * 64 + l * 4 < Da) qa[j] = ld4(q_a + (size_t)p * Da + j * 64 + l * 4);
    if (j * 64 + l * 4 < Db) qb[j] = ld4(q_b + (size_t)p * Db + j * 64 + l * 4);
  }
  const int32_t* crow = cand + (size_t)p * C;
  const float wp = w[p];
  OnlineMix om{-INFINITY, 0.f, 0.f};
  float x0 = 0.f, dlt0 = 0.f;                           // the truth's mixed score and a_0 - b_0 (group 0 meets candidate 0 first)
  for (int k0 = 0; k0 < C; k0 += 64) {
    const int mine = k0 + lane < C ? crow[k0 + lane] : 0;       // 64 candidate ids per load, handed to the groups by shuffles
    const int steps = min(16, (C - k0 + 3) >> 2);
    for (int i = 0; i < steps; i += 2) {
      const int r0 = __shfl(mine, i * 4 + grp), r1 = __shfl(mine, min(i + 1, 15) * 4 + grp);
      const bool v0 = k0 + i * 4 + grp < C, v1 = i + 1 < 16 && k0 + (i + 1) * 4 + grp < C;
      float a0 = 0.f, b0 = 0.f, a1 = 0.f, b1 = 0.f;
      if (v0) {
        a0 = frozen_score<KIND, NJ>(qa, T_a + (size_t)r0 * Da, Da, l);
        b0 = frozen_score<KIND, NJ>(qb, T_b + (size_t)r0 * Db, Db, l);
      }
      if (v1) {
        a1 = frozen_score<KIND, NJ>(qa, T_a + (size_t)r1 * Da, Da, l);
        b1 = frozen_score<KIND, NJ>(qb, T_b + (size_t)r1 * Db, Db, l);
      }
      if (v0) {
        const float x = mix1(wp, a0, b0);
        if (k0 == 0 && i == 0) { x0 = x; dlt0 = a0 - b0; }
        om.add(x, a0 - b0);
      }
      if (v1) om.add(mix1(wp, a1, b1), a1 - b1);
    }
  }
  // merge the four groups' triples in a fixed order; a group without candidates (C < 4) carries (-inf, 0, 0) and adds 0
  float gm[4], gs[4], gu[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) { gm[g] = __shfl(om.m, g * 16); gs[g] = __shfl(om.s, g * 16); gu[g] = __shfl(om.u, g * 16); }
  float M = gm[0];                                      // (group 0 always has candidate 0; a NaN there stays: fmaxf is not used on it)
#pragma unroll
  for (int g = 1; g < 4; ++g) M = gm[g] > M ? gm[g] : M;
  float e[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) e[g] = expf(gm[g] - M);
  const float S = (gs[0] * e[0] + gs[1] * e[1]) + (gs[2] * e[2] + gs[3] * e[3]);
  const float U = (gu[0] * e[0] + gu[1] * e[1]) + (gu[2] * e[2] + gu[3] * e[3]);
  x0 = __shfl(x0, 0);
  dlt0 = __shfl(dlt0, 0);
  if (lane == 0) {
    loss_rows[p] = (M + logf(S)) - x0;
    d_w[p] = (row_scale ? row_scale[p] : inv_rows) * (U / S - dlt0);
  }
}

template <int KIND>
void launch_frozen_mix_ce(int nj, int P, int C, int Da, int Db, const float* q_a, const float* T_a, const float* q_b, const float* T_b, const float* w,
                          const int32_t* cand, const float* row_scale, float inv_rows, float* loss_rows, float* d_w, hipStream_t st) {
#define TEMP_FROZEN_CASE(NJ)                                                                                                             \
  TEMP_LAUNCH(K_FROZEN_MIX_CE, (k_frozen_mix_ce<KIND, NJ>), dim3(ceil_div(P, 4)), dim3(256), 0, st, P, C, Da, Db, q_a, T_a, q_b, T_b, w, cand, \
              row_scale, inv_rows, loss_rows, d_w)
  if (nj <= 1) TEMP_FROZEN_CASE(1);
  else if (nj <= 2) TEMP_FROZEN_CASE(2);
  else if (nj <= 4) TEMP_FROZEN_CASE(4);
  else TEMP_FROZEN_CASE(8);
#undef TEMP_FROZEN_CASE
}

int gated_query_args(int P, int d, int kind, const void* A, const void* ia, const void* B, const void* ib, const void* w, const void* rel,
                     const void* rel_idx, const void* is_tail) {
  if (P < 0 || d <= 0 || (kind != TEMP_SCORE_DISTMULT && kind != TEMP_SCORE_COMPLEX && kind != TEMP_SCORE_TRANSE)) return TEMP_E_BADARG;
  if (kind == TEMP_SCORE_COMPLEX ? d % 8 : d % 4) return TEMP_E_UNSUPPORTED;
  if (P > 0 && (!A || !ia || !B || !ib || !w || !rel || !rel_idx || (kind != TEMP_SCORE_DISTMULT && !is_tail))) return TEMP_E_BADARG;
  return TEMP_OK;
}

// the long-row backward keeps N int counters in LDS (gfx950: 160 KB per workgroup)
constexpr size_t kMixLdsMax = 160 * 1024 - 1024;

}  // namespace
}  // namespace temp

using namespace temp;

extern "C" {

int temp_gated_query_fwd(int P, int d, int kind, const float* A, const int32_t* ia, const float* B, const int32_t* ib, const float* w,
                         const float* rel, const int32_t* rel_idx, const int32_t* is_tail, float* q, void* stream) {
  int rc = gated_query_args(P, d, kind, A, ia, B, ib, w, rel, rel_idx, is_tail);
  if (rc != TEMP_OK || P == 0) return rc;
  if (!q) return TEMP_E_BADARG;
  TEMP_LAUNCH(K_GATED_QUERY, k_gated_query<false>, dim3(ceil_div(P, 4)), dim3(256), 0, (hipStream_t)stream, P, d, kind, A, ia, B, ib, w, rel,
              rel_idx, is_tail, (const float*)nullptr, q, (float*)nullptr, (float*)nullptr, (float*)nullptr);
  return launch_status();
}

int temp_gated_query_bwd(int P, int d, int kind, const float* A, const int32_t* ia, const float* B, const int32_t* ib, const float* w,
                         const float* rel, const int32_t* rel_idx, const int32_t* is_tail, const float* d_q, float* d_a_rows, float* d_b_rows,
                         float* d_rel_rows, float* d_w, void* stream) {
  int rc = gated_query_args(P, d, kind, A, ia, B, ib, w, rel, rel_idx, is_tail);
  if (rc != TEMP_OK || P == 0) return rc;
  if (!d_q || !d_a_rows || !d_b_rows || !d_rel_rows || !d_w) return TEMP_E_BADARG;
  TEMP_LAUNCH(K_GATED_QUERY, k_gated_query<true>, dim3(ceil_div(P, 4)), dim3(256), 0, (hipStream_t)stream, P, d, kind, A, ia, B, ib, w, rel,
              rel_idx, is_tail, d_q, d_a_rows, d_b_rows, d_rel_rows, d_w);
  return launch_status();
}

int temp_gather_ce_mix_fwd(int P, int C, int N, const float* s_a, const float* s_b, const float* w, const int32_t* cand, float* loss_rows,
                           float* lse_rows, void* stream) {
  if (P < 0 || C <= 0 || N <= 0 || (P > 0 && (!s_a || !s_b || !w || !cand || !loss_rows || !lse_rows))) return TEMP_E_BADARG;
  if (P == 0) return TEMP_OK;
  TEMP_LAUNCH(K_GATHER_CE_MIX, k_gather_ce_mix_fwd, dim3(ceil_div(P, 4)), dim3(256), 0, (hipStream_t)stream, P, C, N, s_a, s_b, w, cand,
              loss_rows, lse_rows);
  return launch_status();
}

int temp_gather_ce_mix_bwd(int P, int C, int N, const float* s_a, const float* s_b, const float* w, const int32_t* cand, const float* lse_rows,
                           const float* scale, float inv_rows, const float* row_scale, float* d_s_a, float* d_s_b, float* d_w, void* stream) {
  if (P < 0 || C <= 0 || N <= 0 || !scale || (P > 0 && (!s_a || !s_b || !w || !cand || !lse_rows || !d_s_a || !d_s_b || !d_w)))
    return TEMP_E_BADARG;
  if ((size_t)N * sizeof(int) > kMixLdsMax) return TEMP_E_UNSUPPORTED;
  if (P == 0) return TEMP_OK;
  if (N <= 1024) {
    TEMP_LAUNCH(K_GATHER_CE_MIX, k_gather_ce_mix_bwd_w, dim3(ceil_div(P, 4)), dim3(256), (size_t)4 * N * sizeof(int), (hipStream_t)stream, P, C, N,
                s_a, s_b, w, cand, lse_rows, scale, inv_rows, row_scale, d_s_a, d_s_b, d_w);
    return launch_status();
  }
  const size_t lds = (size_t)N * sizeof(int);
  if (lds + 64 > 65536) {                               // (the kernel's static `red` counts towards the default 64 KB)
    if (hipFuncSetAttribute((const void*)k_gather_ce_mix_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return TEMP_E_LAUNCH;
  }
  TEMP_LAUNCH(K_GATHER_CE_MIX, k_gather_ce_mix_bwd, dim3(P), dim3(256), lds, (hipStream_t)stream, C, N, s_a, s_b, w, cand, lse_rows, scale, inv_rows,
              row_scale, d_s_a, d_s_b, d_w);
  return launch_status();
}

int temp_frozen_mix_ce(int P, int C, int Da, int Db, int kind, const float* q_a, const float* T_a, const float* q_b, const float* T_b,
                       const float* w, const int32_t* cand, const float* row_scale, float inv_rows, float* loss_rows, float* d_w, void* stream) {
  if (P < 0 || C <= 0 || Da <= 0 || Db <= 0 || (kind != TEMP_FROZEN_DOT && kind != TEMP_FROZEN_L1)) return TEMP_E_BADARG;
  if (Da % 4 || Db % 4 || Da > 512 || Db > 512) return TEMP_E_UNSUPPORTED;
  if (P == 0) return TEMP_OK;
  if (!q_a || !T_a || !q_b || !T_b || !w || !cand || !loss_rows || !d_w) return TEMP_E_BADARG;
  const int nj = ceil_div(Da > Db ? Da : Db, 64);
  if (kind == TEMP_FROZEN_DOT)
    launch_frozen_mix_ce<TEMP_FROZEN_DOT>(nj, P, C, Da, Db, q_a, T_a, q_b, T_b, w, cand, row_scale, inv_rows, loss_rows, d_w, (hipStream_t)stream);
  else
    launch_frozen_mix_ce<TEMP_FROZEN_L1>(nj, P, C, Da, Db, q_a, T_a, q_b, T_b, w, cand, row_scale, inv_rows, loss_rows, d_w, (hipStream_t)stream);
  return launch_status();
}

}  // extern "C"
