// Candidate-gather loss kernels: the score of a row at its own candidates alone, read straight from the all-entity table(s).  Two
// scoring operations -- L1 (TransE, utils/scores.py:46-55) and the inner product of a folded bilinear query (distmult / complex /
// simple, utils/scores.py:4-44) -- each plain over one table and gated over two all-entity tables (the post-aggregation models),
// with their entry points; and the dense L1 scores of the ranking.
//
// The three candidate kernels (k_cand_ce_fwd / _bwd_q / _bwd_table below) are written once over TWO policies: the candidate SOURCE
// (further down) and the scoring OPERATION,
//   L1Op    score -sum |q - e|;  d_q = -sum_k g_k sgn(q - e_k);  d_table[n] = +sum_slots g sgn(q - table[n]).  What follows in this
//           comment describes it; its instantiations are the k_l1_ce_* kernels (temp_l1_*), arithmetic unchanged.
//   DotOp   score +sum q e;  d_q = sum_k g_k e_k;  d_table[n] = sum_slots g[slot] q[slot / C] -- the table row is not read by the
//           plain bwd_table.  The mix stays linear in the candidate here, but is still formed in registers (one pass reads both rows):
//           d_w[p] = sum_k g_k sum_d q_d (TA - TB)[row, d],  d_TA = sum w g q,  d_TB = sum (1 - w) g q.  These are the k_dot_ce_* /
//           k_dot_mix_ce_* launches (temp_dot_*): the gather route of the bilinear scorers, which has no ceiling on the entity count
//           (temp_gather_ce_bwd keeps N counters in LDS) and never forms a (rows, N) matrix.
// Everything else -- work split, load order, reduction orders, no atomics, outputs fully written -- is shared.
//
// The L1 form (k_l1_ce_x = k_cand_ce_x<L1Op, .>).  TransE is not bilinear: score(p, c) = -sum_d |q[p,d] - c[d]| with the translation query q of k_bilinear_query / k_gated_query,
// so no GEMM carries it.  The training loss needs the score at the 1 + negative_rate candidates of a row only -- a gather of
// P C d elements, N / C times fewer than the dense matrix -- and never as a (P, C, D) tensor:
//   k_l1_ce_fwd        one workgroup per row; a 16-lane group owns a candidate (float4 per lane, ceil(d / 64) passes, four xor
//                      steps to reduce), two candidates per group in flight; then the row's logsumexp.
//   k_l1_ce_bwd_q      g = scale * (softmax - [k == 0]);  d_q[p] = -sum_k g_k sgn(q[p] - e_k): wave w sums the candidates
//                      k = w mod 4 in ascending order, the four partials combine as (0 + 1) + (2 + 3).
//   k_l1_ce_bwd_table  the candidate-side adjoint over the slots of one table row (a stable sort of the flat positions by table
//                      row), split over the four waves and combined in the same way: no atomics, fixed order.
//   k_l1_scores        the dense scores of the ranking, a VALU register tile (below).
// sgn(0) = 0, the gradient torch.abs takes.
//
// Every kernel is written once over a candidate SOURCE, which says how the row e_k of a candidate is fetched and formed:
//   OneTable   e = table[row]: the row as loaded, no arithmetic.
//   TwoTables  the gated form (PostDynamicRGCN.train_link_prediction, models/PostDynamicRGCN.py:261-282): e[p] = mix(w[p], TA[row],
//              TB[row]) of the two all-entity tables (mix.hpp).  |q - e|_1 is not linear in e, so the mix cannot move to two score
//              matrices as it does for the bilinear scorers (gated_loss.hip): BOTH rows are read and mixed in registers.  The
//              backward kernels also return the adjoints of the mix:
//                bwd_q      d_w[p] = sum_k g_k sum_d sgn(q - e_k) (TA - TB)[row] from the rows it holds: every thread sums its own
//                           (k, d) terms in loop order, then lanes (xor tree) and waves ((0 + 1) + (2 + 3)).
//                bwd_table  d_TA = sum w g sgn and d_TB = sum (1 - w) g sgn in one pass; the mixed row differs per slot (the slot's
//                           row weight), so it is recomputed per slot from the two rows in registers.
//                scores     the mix is formed per (row, entity, k) by mix1, so a score agrees with the candidate kernels' to the
//                           summation order.
// A source is passed by value where the table pointers stood.  Raw is what one float4 column of a row occupies in registers
// before it is used (the loads are issued ahead of their use), value() the row's float4 from it.
#include "common.hpp"
#include "mix.hpp"
#include "reduce.hpp"

namespace temp {
namespace {

struct OneTable {
  static constexpr bool kMixed = false;
  static constexpr int kLaunchTag = K_GATHER_CE;
  struct Raw { float4 x; };
  const float* table;
  bool has_tables() const { return table; }
  bool has_weights() const { return true; }
  __device__ __forceinline__ float weight(int) const { return 0.f; }
  __device__ __forceinline__ Raw load(size_t off) const { return {ld4(table + off)}; }
  static __device__ __forceinline__ Raw none() { return {zero4()}; }
  static __device__ __forceinline__ float4 value(float, const Raw& r) { return r.x; }
};

struct TwoTables {
  static constexpr bool kMixed = true;
  static constexpr int kLaunchTag = K_GATHER_CE_MIX;
  struct Raw { float4 x, y; };
  const float *ta, *tb, *w;
  bool has_tables() const { return ta && tb; }
  bool has_weights() const { return w; }
  __device__ __forceinline__ float weight(int p) const { return w[p]; }
  __device__ __forceinline__ Raw load(size_t off) const { return {ld4(ta + off), ld4(tb + off)}; }
  static __device__ __forceinline__ Raw none() { return {zero4(), zero4()}; }
  static __device__ __forceinline__ float4 value(float wp, const Raw& r) { return mix4(wp, r.x, r.y); }
};

__device__ __forceinline__ float l1_4(float4 a, float4 b) { return (fabsf(a.x - b.x) + fabsf(a.y - b.y)) + (fabsf(a.z - b.z) + fabsf(a.w - b.w)); }
__device__ __forceinline__ float sgnf(float x) { return (float)((x > 0.f) - (x < 0.f)); }
__device__ __forceinline__ float4 sgn4(float4 a, float4 b) { return make_float4(sgnf(a.x - b.x), sgnf(a.y - b.y), sgnf(a.z - b.z), sgnf(a.w - b.w)); }

__device__ __forceinline__ float dot4(float4 a, float4 b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }

// The scoring OPERATION of the three candidate kernels: what one float4 column adds to a candidate's sum (term), how the sum becomes
// the score, and -- in the backward kernels, under `if constexpr (Op::kDot)` -- the adjoints of that score.  role: 0 fwd, 1 bwd_q,
// 2 bwd_table; the L1 kernels keep the launch tags they had, the dot kernels have one of their own per entry point.
struct L1Op {
  static constexpr bool kDot = false;
  template <class Src> static constexpr int tag(int) { return Src::kLaunchTag; }
  static __device__ __forceinline__ float term(float4 q, float4 e) { return l1_4(q, e); }
  static __device__ __forceinline__ float score(float a) { return -a; }
};

struct DotOp {
  static constexpr bool kDot = true;
  template <class Src> static constexpr int tag(int role) { return (Src::kMixed ? K_DOT_MIX_CE_FWD : K_DOT_CE_FWD) + role; }
  static __device__ __forceinline__ float term(float4 q, float4 e) { return dot4(q, e); }
  static __device__ __forceinline__ float score(float a) { return a; }
};

// NP > 0: d <= 64 NP and q[p] stays in registers; NP == 0: any d, q[p] is re-read per candidate (it stays in the L1).
template <int NP, class Op, class Src>
__global__ void __launch_bounds__(256) k_cand_ce_fwd(int C, int d, const float* __restrict__ q, Src src, const int32_t* __restrict__ base,
                                                   const int32_t* __restrict__ cand, float* s_out, float* __restrict__ loss_rows,
                                                   float* __restrict__ lse_rows) {
  using Raw = typename Src::Raw;
  __shared__ float red[4];
  const int p = blockIdx.x, grp = threadIdx.x >> 4, l = threadIdx.x & 15;
  const float* qrow = q + (size_t)p * d;
  const int32_t* crow = cand + (size_t)p * C;
  float* srow = s_out + (size_t)p * C;
  const size_t b = base ? (size_t)base[p] : 0;
  const float wp = src.weight(p);
  float4 qv[NP > 0 ? NP : 1];
#pragma unroll
  for (int u = 0; u < NP; ++u) qv[u] = l * 4 + 64 * u < d ? ld4(qrow + l * 4 + 64 * u) : zero4();
  for (int k0 = grp; k0 < C; k0 += 32) {
    const int k1 = k0 + 16;
    const size_t r0 = (b + (size_t)crow[k0]) * d, r1 = k1 < C ? (b + (size_t)crow[k1]) * d : r0;
    float a0 = 0.f, a1 = 0.f;
    if (NP > 0) {
      Raw x0[NP > 0 ? NP : 1], x1[NP > 0 ? NP : 1];
#pragma unroll
      for (int u = 0; u < NP; ++u) {                      // both candidates' rows are requested before either is consumed
        const int j = l * 4 + 64 * u;
        x0[u] = j < d ? src.load(r0 + j) : Src::none();
        x1[u] = j < d ? src.load(r1 + j) : Src::none();
      }
#pragma unroll
      for (int u = 0; u < NP; ++u) { a0 += Op::term(qv[u], Src::value(wp, x0[u])); a1 += Op::term(qv[u], Src::value(wp, x1[u])); }
    } else {
      for (int j = l * 4; j < d; j += 64) {
        const float4 qq = ld4(qrow + j);
        const Raw x0 = src.load(r0 + j), x1 = src.load(r1 + j);
        a0 += Op::term(qq, Src::value(wp, x0));
        a1 += Op::term(qq, Src::value(wp, x1));
      }
    }
    a0 = group16_sum(a0);
    a1 = group16_sum(a1);
    if (l == 0) {
      srow[k0] = Op::score(a0);
      if (k1 < C) srow[k1] = Op::score(a1);
    }
  }
  __syncthreads();                                       // the row's scores, written by this workgroup, are read back below
  float mx = -INFINITY, sum = 0.f;
  for (int k = threadIdx.x; k < C; k += 256) mx = fmaxf(mx, srow[k]);
  mx = block_max_256(mx, red);
  for (int k = threadIdx.x; k < C; k += 256) sum += expf(srow[k] - mx);
  sum = block_sum_256(sum, red);
  if (threadIdx.x == 0) {
    const float lse = mx + logf(sum);
    lse_rows[p] = lse;
    loss_rows[p] = lse - srow[0];
  }
}

// d_w is written by the mixed source only (NULL otherwise)
template <class Op, class Src>
__global__ void __launch_bounds__(256) k_cand_ce_bwd_q(int C, int d, const float* __restrict__ q, Src src, const int32_t* __restrict__ base,
                                                     const int32_t* __restrict__ cand, const float* __restrict__ s,
                                                     const float* __restrict__ lse_rows, const float* __restrict__ scale_ptr, float inv_rows,
                                                     const float* __restrict__ row_scale, float* g_out, float* __restrict__ d_q,
                                                     float* __restrict__ d_w) {
  __shared__ __attribute__((aligned(16))) float part[3][256];
  const int p = blockIdx.x, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* qrow = q + (size_t)p * d;
  const int32_t* crow = cand + (size_t)p * C;
  const float* srow = s + (size_t)p * C;
  float* grow = g_out + (size_t)p * C;
  const size_t b = base ? (size_t)base[p] : 0;
  const float wp = src.weight(p), lse = lse_rows[p];
  const float scale = scale_ptr[0] * (row_scale ? row_scale[p] : inv_rows);
  for (int k = threadIdx.x; k < C; k += 256) grow[k] = scale * (expf(srow[k] - lse) - (k == 0 ? 1.f : 0.f));
  __syncthreads();                                       // g of the row, written by this workgroup, is read back below
  float wacc = 0.f;
  for (int j0 = 0; j0 < d; j0 += 256) {
    const int j = j0 + lane * 4;
    const bool act = j < d;
    const float4 qv = act ? ld4(qrow + j) : zero4();
    float4 acc = zero4();
#pragma unroll 4
    for (int k = wv; k < C; k += 4) {
      const float gk = grow[k];
      const size_t r = (b + (size_t)crow[k]) * d;
      if (act) {
        const typename Src::Raw e = src.load(r + j);
        if constexpr (Op::kDot) {
          acc = fma4(gk, Src::value(wp, e), acc);
          if constexpr (Src::kMixed) {
            const float4 x = e.x, y = e.y;
            wacc += gk * ((qv.x * (x.x - y.x) + qv.y * (x.y - y.y)) + (qv.z * (x.z - y.z) + qv.w * (x.w - y.w)));
          }
        } else {
          const float4 sg = sgn4(qv, Src::value(wp, e));
          acc.x -= gk * sg.x; acc.y -= gk * sg.y; acc.z -= gk * sg.z; acc.w -= gk * sg.w;
          if constexpr (Src::kMixed) {
            const float4 x = e.x, y = e.y;
            wacc += gk * ((sg.x * (x.x - y.x) + sg.y * (x.y - y.y)) + (sg.z * (x.z - y.z) + sg.w * (x.w - y.w)));
          }
        }
      }
    }
    acc = combine_waves_4(acc, part, wv, lane);
    if (wv == 0 && act) st4(d_q + (size_t)p * d + j, acc);
  }
  if constexpr (Src::kMixed) {
    __shared__ float red[4];
    wacc = block_sum_256(wacc, red);
    if (threadIdx.x == 0) d_w[p] = wacc;
  }
}

// d_a is the table's adjoint, or TA's with d_b TB's (NULL otherwise); the slot's row weight enters only when mixed.  The dot
// adjoint sum g q does not depend on the table row: it is not loaded.
template <class Op, class Src>
__global__ void __launch_bounds__(256) k_cand_ce_bwd_table(int d, int C, const float* __restrict__ q, Src src, const int32_t* __restrict__ slot_ptr,
                                                         const int32_t* __restrict__ slot, const float* __restrict__ g, float* __restrict__ d_a,
                                                         float* __restrict__ d_b) {
  __shared__ __attribute__((aligned(16))) float part[3][256];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t n = blockIdx.x;
  const int s0 = slot_ptr[n], s1 = slot_ptr[n + 1];
  for (int j0 = 0; j0 < d; j0 += 256) {
    const int j = j0 + lane * 4;
    const bool act = j < d;
    const typename Src::Raw tv = !Op::kDot && act ? src.load(n * d + j) : Src::none();
    float4 aa = zero4(), ab = zero4();
#pragma unroll 4
    for (int i = s0 + wv; i < s1; i += 4) {
      const int sl = slot[i];
      const int p = sl / C;
      const float gk = g[sl], wp = src.weight(p);
      const float* qr = q + (size_t)p * d;
      if (act) {
        if constexpr (Op::kDot) {
          const float4 qq = ld4(qr + j);
          if constexpr (Src::kMixed) {
            const float4 t = scale4(qq, gk);              // g q: one rounding
            aa = fma4(wp, t, aa);
            ab = fma4(1.f - wp, t, ab);
          } else {
            aa = fma4(gk, qq, aa);
          }
        } else {
          const float4 sg = sgn4(ld4(qr + j), Src::value(wp, tv));
          if constexpr (Src::kMixed) {
            const float4 t = scale4(sg, gk);                // g sgn: exact
            aa = fma4(wp, t, aa);
            ab = fma4(1.f - wp, t, ab);
          } else {
            aa = fma4(gk, sg, aa);                          // (the product is exact: one rounding, fused or not)
          }
        }
      }
    }
    aa = combine_waves_4(aa, part, wv, lane);
    if (wv == 0 && act) st4(d_a + n * d + j, aa);        // a row without slots gets its zeros here
    if constexpr (Src::kMixed) {
      ab = combine_waves_4(ab, part, wv, lane);
      if (wv == 0 && act) st4(d_b + n * d + j, ab);
    }
  }
}

// Dense L1 scores for the ranking: scores[p, n] = -|q[p] - e[n]|_1, columns [N, ld) = -inf.  No MFMA applies (|a - b| is not
// a product); a VALU register tile instead: 64 x 64 outputs per workgroup, 4 x 4 per thread, 16-wide k-chunks of the operands
// staged k-major in LDS (row stride 68 floats: the float4 reads of a k-row stay 16-byte aligned, the 16 distinct ones of a wave
// are contiguous and the row operand is a broadcast).  Per output and k: one subtract, one add with the |.| source modifier
// (mixed: mix1 before them, its (1 - w) once per row).
// The transposing staging stores are 2-way bank-conflicted (any 16-byte-aligned stride puts the k-groups 0 / 8 and 4 / 12 of a
// half-wave on one bank): 8 stores per thread and chunk beside its 512 VALU operations, left as it is.
#define L1S_TILE 64
#define L1S_KC 16
#define L1S_LD 68
__device__ __forceinline__ void l1s_stage(float (*S)[L1S_LD], int lk, int lr, float4 v) {
  S[lk][lr] = v.x; S[lk + 1][lr] = v.y; S[lk + 2][lr] = v.z; S[lk + 3][lr] = v.w;
}

template <class Src>
__global__ void __launch_bounds__(256) k_l1_scores(int P, int N, int d, const float* __restrict__ q, Src src, int ld, float* __restrict__ scores) {
  __shared__ __attribute__((aligned(16))) float Qs[L1S_KC][L1S_LD];
  __shared__ __attribute__((aligned(16))) float Ts[Src::kMixed ? 2 : 1][L1S_KC][L1S_LD];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int p0 = blockIdx.y * L1S_TILE, n0 = blockIdx.x * L1S_TILE;
  const int lr = threadIdx.x >> 2, lk = (threadIdx.x & 3) * 4;        // the float4 of the k-chunk this thread stages: row lr, columns lk..lk+3
  const bool q_ok = p0 + lr < P, t_ok = n0 + lr < N;
  const float* qrow = q + (size_t)(q_ok ? p0 + lr : 0) * d;
  const size_t trow = (size_t)(t_ok ? n0 + lr : 0) * d;
  float wr[4], omw[4];
  if constexpr (Src::kMixed) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = p0 + ty * 4 + i;
      wr[i] = p < P ? src.weight(p) : 0.f;
      omw[i] = 1.f - wr[i];                                            // mix1's (1 - w), once per row
    }
  }
  float acc[4][4] = {};
  for (int k0 = 0; k0 < d; k0 += L1S_KC) {
    const bool k_ok = k0 + lk < d;                                    // d % 4 == 0: a float4 is inside the row or past it
    const float4 qv = q_ok && k_ok ? ld4(qrow + k0 + lk) : zero4();  // rows and columns past the edge: |0 - 0| adds nothing
    const typename Src::Raw tv = t_ok && k_ok ? src.load(trow + k0 + lk) : Src::none();
    __syncthreads();                                                  // the chunk before is consumed
    l1s_stage(Qs, lk, lr, qv);
    l1s_stage(Ts[0], lk, lr, tv.x);
    if constexpr (Src::kMixed) l1s_stage(Ts[1], lk, lr, tv.y);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < L1S_KC; ++k) {
      const float4 qq = ld4(&Qs[k][ty * 4]), a = ld4(&Ts[0][k][tx * 4]);
      const float qr[4] = {qq.x, qq.y, qq.z, qq.w}, ar[4] = {a.x, a.y, a.z, a.w};
      if constexpr (Src::kMixed) {
        const float4 b = ld4(&Ts[1][k][tx * 4]);
        const float br[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) acc[i][jj] += fabsf(qr[i] - fmaf(wr[i], ar[jj], omw[i] * br[jj]));   // mix1, (1 - w) hoisted
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) acc[i][jj] += fabsf(qr[i] - ar[jj]);
      }
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

// ---- host side: one launcher per role; the entry points below are its instantiations (operation x source) ----
int l1_ce_args(int P, int C, int d) {
  if (P < 0 || C <= 0 || d <= 0) return TEMP_E_BADARG;
  if (d % 4 || (long long)P * C >= (1ll << 31)) return TEMP_E_UNSUPPORTED;
  return TEMP_OK;
}

template <class Op, class Src>
int cand_ce_fwd(int P, int C, int d, const float* q, Src src, const int32_t* base, const int32_t* cand, float* s_out, float* loss_rows,
              float* lse_rows, void* stream) {
  const int rc = l1_ce_args(P, C, d);
  if (rc != TEMP_OK || P == 0) return rc;
  if (!q || !src.has_tables() || !src.has_weights() || !cand || !s_out || !loss_rows || !lse_rows) return TEMP_E_BADARG;
#define L1_FWD(NP) TEMP_LAUNCH(Op::template tag<Src>(0), (k_cand_ce_fwd<NP, Op, Src>), dim3(P), dim3(256), 0, (hipStream_t)stream, C, d, q, src, base, cand, s_out, loss_rows, lse_rows)
  if (d <= 64) L1_FWD(1);
  else if (d <= 128) L1_FWD(2);
  else if (d <= 192) L1_FWD(3);
  else if (d <= 256) L1_FWD(4);
  else L1_FWD(0);
#undef L1_FWD
  return launch_status();
}

template <class Op, class Src>
int cand_ce_bwd_q(int P, int C, int d, const float* q, Src src, const int32_t* base, const int32_t* cand, const float* s, const float* lse_rows,
                const float* scale, float inv_rows, const float* row_scale, float* g_out, float* d_q, float* d_w, void* stream) {
  const int rc = l1_ce_args(P, C, d);
  if (rc != TEMP_OK) return rc;
  if (!scale) return TEMP_E_BADARG;
  if (P == 0) return TEMP_OK;
  if (!q || !src.has_tables() || !src.has_weights() || !cand || !s || !lse_rows || !g_out || !d_q || (Src::kMixed && !d_w)) return TEMP_E_BADARG;
  TEMP_LAUNCH(Op::template tag<Src>(1), (k_cand_ce_bwd_q<Op, Src>), dim3(P), dim3(256), 0, (hipStream_t)stream, C, d, q, src, base, cand, s, lse_rows, scale, inv_rows,
              row_scale, g_out, d_q, d_w);
  return launch_status();
}

template <class Op, class Src>
int cand_ce_bwd_table(int n_rows, int d, int C, const float* q, Src src, const int32_t* slot_ptr, const int32_t* slot, const float* g, float* d_a,
                    float* d_b, void* stream) {
  if (n_rows < 0 || C <= 0 || d <= 0) return TEMP_E_BADARG;
  if (d % 4) return TEMP_E_UNSUPPORTED;
  if (n_rows == 0) return TEMP_OK;
  if (!src.has_tables() || !slot_ptr || !d_a || (Src::kMixed && !d_b)) return TEMP_E_BADARG;   // q, w, slot and g may be NULL when every list is empty
  TEMP_LAUNCH(Op::template tag<Src>(2), (k_cand_ce_bwd_table<Op, Src>), dim3(n_rows), dim3(256), 0, (hipStream_t)stream, d, C, q, src, slot_ptr, slot, g, d_a, d_b);
  return launch_status();
}

template <class Src>
int l1_scores(int P, int N, int d, const float* q, Src src, int ld, float* scores, void* stream) {
  if (P < 0 || N <= 0 || d <= 0 || ld < N) return TEMP_E_BADARG;
  if (d % 4 || ld % 4 || ceil_div(P, L1S_TILE) > 65535) return TEMP_E_UNSUPPORTED;
  if (P == 0) return TEMP_OK;
  if (!q || !src.has_tables() || !src.has_weights() || !scores) return TEMP_E_BADARG;
  TEMP_LAUNCH(Src::kLaunchTag, k_l1_scores<Src>, dim3(ceil_div(ld, L1S_TILE), ceil_div(P, L1S_TILE)), dim3(256), 0, (hipStream_t)stream, P, N, d, q, src,
              ld, scores);
  return launch_status();
}

}  // namespace
}  // namespace temp

using namespace temp;

extern "C" {

int temp_l1_ce_fwd(int P, int C, int d, const float* q, const float* table, const int32_t* base, const int32_t* cand, float* s_out,
                   float* loss_rows, float* lse_rows, void* stream) {
  return cand_ce_fwd<L1Op>(P, C, d, q, OneTable{table}, base, cand, s_out, loss_rows, lse_rows, stream);
}

int temp_l1_mix_ce_fwd(int P, int C, int d, const float* q, const float* table_a, const float* table_b, const float* w, const int32_t* base,
                       const int32_t* cand, float* s_out, float* loss_rows, float* lse_rows, void* stream) {
  return cand_ce_fwd<L1Op>(P, C, d, q, TwoTables{table_a, table_b, w}, base, cand, s_out, loss_rows, lse_rows, stream);
}

int temp_l1_ce_bwd_q(int P, int C, int d, const float* q, const float* table, const int32_t* base, const int32_t* cand, const float* s,
                     const float* lse_rows, const float* scale, float inv_rows, const float* row_scale, float* g_out, float* d_q, void* stream) {
  return cand_ce_bwd_q<L1Op>(P, C, d, q, OneTable{table}, base, cand, s, lse_rows, scale, inv_rows, row_scale, g_out, d_q, nullptr, stream);
}

int temp_l1_mix_ce_bwd_q(int P, int C, int d, const float* q, const float* table_a, const float* table_b, const float* w, const int32_t* base,
                         const int32_t* cand, const float* s, const float* lse_rows, const float* scale, float inv_rows, const float* row_scale,
                         float* g_out, float* d_q, float* d_w, void* stream) {
  return cand_ce_bwd_q<L1Op>(P, C, d, q, TwoTables{table_a, table_b, w}, base, cand, s, lse_rows, scale, inv_rows, row_scale, g_out, d_q, d_w, stream);
}

int temp_l1_ce_bwd_table(int n_rows, int d, int C, const float* q, const float* table, const int32_t* slot_ptr, const int32_t* slot, const float* g,
                         float* d_table, void* stream) {
  return cand_ce_bwd_table<L1Op>(n_rows, d, C, q, OneTable{table}, slot_ptr, slot, g, d_table, nullptr, stream);
}

int temp_l1_mix_ce_bwd_table(int n_rows, int d, int C, const float* q, const float* table_a, const float* table_b, const float* w,
                             const int32_t* slot_ptr, const int32_t* slot, const float* g, float* d_table_a, float* d_table_b, void* stream) {
  return cand_ce_bwd_table<L1Op>(n_rows, d, C, q, TwoTables{table_a, table_b, w}, slot_ptr, slot, g, d_table_a, d_table_b, stream);
}

int temp_dot_ce_fwd(int P, int C, int d, const float* q, const float* table, const int32_t* base, const int32_t* cand, float* s_out,
                   float* loss_rows, float* lse_rows, void* stream) {
  return cand_ce_fwd<DotOp>(P, C, d, q, OneTable{table}, base, cand, s_out, loss_rows, lse_rows, stream);
}

int temp_dot_mix_ce_fwd(int P, int C, int d, const float* q, const float* table_a, const float* table_b, const float* w, const int32_t* base,
                       const int32_t* cand, float* s_out, float* loss_rows, float* lse_rows, void* stream) {
  return cand_ce_fwd<DotOp>(P, C, d, q, TwoTables{table_a, table_b, w}, base, cand, s_out, loss_rows, lse_rows, stream);
}

int temp_dot_ce_bwd_q(int P, int C, int d, const float* q, const float* table, const int32_t* base, const int32_t* cand, const float* s,
                     const float* lse_rows, const float* scale, float inv_rows, const float* row_scale, float* g_out, float* d_q, void* stream) {
  return cand_ce_bwd_q<DotOp>(P, C, d, q, OneTable{table}, base, cand, s, lse_rows, scale, inv_rows, row_scale, g_out, d_q, nullptr, stream);
}

int temp_dot_mix_ce_bwd_q(int P, int C, int d, const float* q, const float* table_a, const float* table_b, const float* w, const int32_t* base,
                         const int32_t* cand, const float* s, const float* lse_rows, const float* scale, float inv_rows, const float* row_scale,
                         float* g_out, float* d_q, float* d_w, void* stream) {
  return cand_ce_bwd_q<DotOp>(P, C, d, q, TwoTables{table_a, table_b, w}, base, cand, s, lse_rows, scale, inv_rows, row_scale, g_out, d_q, d_w, stream);
}

int temp_dot_ce_bwd_table(int n_rows, int d, int C, const float* q, const float* table, const int32_t* slot_ptr, const int32_t* slot, const float* g,
                         float* d_table, void* stream) {
  return cand_ce_bwd_table<DotOp>(n_rows, d, C, q, OneTable{table}, slot_ptr, slot, g, d_table, nullptr, stream);
}

int temp_dot_mix_ce_bwd_table(int n_rows, int d, int C, const float* q, const float* table_a, const float* table_b, const float* w,
                             const int32_t* slot_ptr, const int32_t* slot, const float* g, float* d_table_a, float* d_table_b, void* stream) {
  return cand_ce_bwd_table<DotOp>(n_rows, d, C, q, TwoTables{table_a, table_b, w}, slot_ptr, slot, g, d_table_a, d_table_b, stream);
}

int temp_l1_scores(int P, int N, int d, const float* q, const float* table, int ld, float* scores, void* stream) {
  return l1_scores(P, N, d, q, OneTable{table}, ld, scores, stream);
}

int temp_l1_mix_scores(int P, int N, int d, const float* q, const float* table_a, const float* table_b, const float* w, int ld, float* scores,
                       void* stream) {
  return l1_scores(P, N, d, q, TwoTables{table_a, table_b, w}, ld, scores, stream);
}

}  // extern "C"
