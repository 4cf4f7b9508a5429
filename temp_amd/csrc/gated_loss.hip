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

}  // extern "C"
