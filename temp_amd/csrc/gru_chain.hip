// Persistent window-chain kernels of the TeMP snapshot encoder on gfx950 (include/temp_amd.h: TempGruChain).
//
// The GRU recurrence over the train-seq-len window (models/DynamicRGCN.py:156-174, models/BiDynamicRGCN.py:51-100,
// GRRGCNLayer.forward models/RRGCN.py:77-89) is independent per (window, direction, entity): position p of an entity
// reads only that entity's state at position p-1.  A workgroup therefore owns a PANEL of 32 entity tracks, keeps the 32
// current states in LDS and walks every position of the chain inside one launch -- no grid barrier, no relaunch, the
// state never leaves the CU.  512 (forward) / 768 (backward) threads per workgroup, one workgroup per CU:
//   waves 0-3  "matrix" role, one per SIMD:  acc[32 x tile] += W_hh-fragment x state-fragment on v_mfma_f32_32x32x2_f32.
//              W_hh arrives straight from L2 in MFMA fragment order (packed once per step by k_gru_chain_pack: one
//              coalesced 1-KB load per wave per 4 MFMAs per tile), the state fragment is one ds_read_b128 per 4 MFMAs of
//              all tiles; the raw 32 x 3d products are handed over through LDS.
//   waves 4+   "memory" role: everything that touches HBM.  The hoisted input gates (forward) / saved gate planes
//              (backward) of the NEXT position are loaded into registers while the matrix waves work on the current one;
//              after the hand-over barrier these waves apply the gates, write the saved planes / gate gradients with
//              row-contiguous float4 stores and put the new state (resp. d_prev) back into LDS.
// The matrix waves never wait on HBM: their only global loads are L2 hits on the packed weights.
#include <atomic>
#include "common.hpp"
#include "gru_math.hpp"
#include "gemm_bx.hpp"

namespace temp {

#define CH_SLOTS TEMP_CHAIN_TRACKS
#define CH_HAS_PREV TEMP_CHAIN_HAS_PREV
#define CH_ROW_MASK (TEMP_CHAIN_HAS_PREV - 1)
#define CH_LDS_LIMIT (160 * 1024)

struct ChainRnn {
  const float4* wf; const float4* wb; const float* b_hh; const unsigned* kf; const unsigned* kb;   // kf / kb: column keys of the f16 planes (gru_chain_hx.hpp)
  const float* decay_wb;                 // nullable: device {w, b} of the learnable decay exp(-max(w dt + b, 0)) (gru_math.hpp: decay_factor)
};
struct ChainArgs {
  int D, n_panels, max_steps, dbg;
  int layout;                            // TEMP_CHAIN_PACK_*: the arithmetic the packed weights were written for (the kernels follow it)
  int n_rnn_keys;                        // GRUs of the chain (rows of the column-key result in front of the per-panel partials)
  const int32_t* panel; const int32_t* rows; const int32_t* sinfo;
  const float* dt;
  const int32_t* gi_index;
  float lambda;
  size_t plane;
  ChainRnn rnn[TEMP_CHAIN_MAX_RNN];
  float* d_arg;                          // nullable (backward, learnable decay): [N_total] dL / d(w dt + b) of every row with a previous state
  // State offset (TempChainOffset; --use-time-embedding): row rho leaves s = h + off_table[off_index[rho]] (an index outside
  // [0, off_rows) = no offset).  All nullable; k_gru_chain_fwd / _bwd only (the f16 kernels split the state with a constant scale).
  const float* off_table; const int32_t* off_index; int off_rows;
  float* d_state;                        // nullable (backward): [N_total][d] the total gradient reaching every row's state
  long long* stamp;                      // development only (temp_set_debug_buffer): cycle stamps of the f16 kernels' DEV instantiations, else nullptr
};
struct ChainUps { const float* p[TEMP_CHAIN_MAX_UP]; };

struct ChainGeom {
  int NT, NQ;        // forward: tiles of 32 gate columns (3d), k-steps of 8 (d), even
  int NTb, NQb;      // backward: tiles of 32 state columns (d), k-steps of 8 (3d), multiple of 4
  int lda, ldh;      // forward LDS strides (floats): product rows, state rows
  int ldA, ldz;      // backward LDS strides: dgh rows, gz / d_prev rows
};
__host__ __device__ inline ChainGeom chain_geom(int D) {
  ChainGeom g;
  g.NT = (3 * D + 31) >> 5; g.NQ = ((D + 15) >> 4) << 1;          // k-steps come in groups (the loops are unrolled by two,
  g.NTb = (D + 31) >> 5; g.NQb = ((3 * D + 31) >> 5) << 2;        // by four in the backward, branch-free): padded with zero stages
  g.lda = g.NT * 32 + 4; g.ldh = g.NQ * 8 + 4;          // (stride / 4) odd: conflict-free ds_read_b128 / ds_write_b128 across rows
  g.ldA = g.NQb * 8 + 4; g.ldz = g.NTb * 32 + 4;
  return g;
}
#define CH_MAX_STEPS 64      // steps of one panel: its row table, decay factors and step flags are staged in LDS
// `ms` = the longest panel of the launch (<= CH_MAX_STEPS)
inline size_t chain_lds_fwd(int D, int ms) { ChainGeom g = chain_geom(D); return ((size_t)CH_SLOTS * g.lda + 2 * CH_SLOTS * g.ldh + (2 * CH_SLOTS + 1) * (size_t)ms) * 4; }
inline size_t chain_lds_bwd(int D, int ms) { ChainGeom g = chain_geom(D); return ((size_t)CH_SLOTS * g.ldA + 2 * CH_SLOTS * g.ldz + (2 * CH_SLOTS + 3) * (size_t)ms) * 4; }


// Learnable decay, backward: the row rho that continues track `slot` at the next position has hd = dec . h_pi, dec = exp(-max(arg, 0)),
// arg = w dt_rho + b, so dL/d arg_rho = -[arg_rho > 0] <d_hd . dec, h_pi> = -[arg_rho > 0] <d_prev_rho, h_pi>  (d_prev_rho is what the
// matrix waves left in dpb; h_pi = (1 - z) n + z hd from the saved planes of pi -- both cells' output equation).  Every lane of the
// wave hands in its partial dot product; the 64 partials are summed in a fixed order (a DPP butterfly inside each row of 16 lanes,
// then the four rows), so the result is bit-repeatable.  (With a state offset the decayed state is h_pi + offset_pi: k_gru_chain_bwd<OFS> adds
// <d_prev_rho, offset_pi> to the lanes' partials.)
__device__ __forceinline__ float chain_wave_sum(float v) {
  auto dpp = [](float x, auto ctrl) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), decltype(ctrl)::value, 0xf, 0xf, true)); };
  v += dpp(v, std::integral_constant<int, 0xB1>());     // quad_perm [1, 0, 3, 2]
  v += dpp(v, std::integral_constant<int, 0x4E>());     // quad_perm [2, 3, 0, 1]
  v += dpp(v, std::integral_constant<int, 0x141>());    // row_half_mirror
  v += dpp(v, std::integral_constant<int, 0x140>());    // row_mirror
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
  return (r0 + r1) + (r2 + r3);
}
__device__ __forceinline__ float chain_dot_prev(const float4 dp, const float4 z, const float4 n, const float4 hd) {
  const float4 h = make_float4((1.f - z.x) * n.x + z.x * hd.x, (1.f - z.y) * n.y + z.y * hd.y, (1.f - z.z) * n.z + z.z * hd.z, (1.f - z.w) * n.w + z.w * hd.w);
  return (dp.x * h.x + dp.y * h.y) + (dp.z * h.z + dp.w * h.w);
}
// (all 64 lanes call it; `en` = the table entry of rho)
__device__ __forceinline__ void chain_store_d_arg(const ChainArgs& a, const ChainRnn& R, int en, float part, int lane) {
  const float dot = chain_wave_sum(part);
  if (lane == 0) {
    const int row = en & CH_ROW_MASK;
    a.d_arg[row] = fmaf(R.decay_wb[0], a.dt[row], R.decay_wb[1]) > 0.f ? -dot : 0.f;
  }
}

}  // namespace temp
#include "gru_chain_hx.hpp"
namespace temp {

// ---- W_hh -> fragment order ---------------------------------------------------------------------------------------
// forward  piece (tile, q, lane): float4 e -> W_hh[tile*32 + li][8q + 4hh + e]      (gate column x k)
// backward piece (tile, q, lane): float4 e -> W_hh[8q + 4hh + e][tile*32 + li]      (k = gate column, state column)
// zero outside the matrix.  li = lane & 31, hh = lane >> 5: the A-operand layout of v_mfma_f32_32x32x2_f32 (lane supplies
// A[i = li][k = hh]); one float4 feeds 4 consecutive MFMAs, the state fragment uses the same k order.
__global__ void __launch_bounds__(256) k_gru_chain_pack(int D, const float* __restrict__ W, float4* __restrict__ out) {
  const ChainGeom g = chain_geom(D);
  const int nf = g.NT * g.NQ * 64, nb = g.NTb * g.NQb * 64;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nf + nb; i += gridDim.x * blockDim.x) {
    const bool fwd = i < nf;
    const int j = fwd ? i : i - nf;
    const int lane = j & 63, rest = j >> 6;
    const int nq = fwd ? g.NQ : g.NQb;
    const int tile = rest / nq, q = rest - tile * nq;
    const int n = tile * 32 + (lane & 31), k = 8 * q + 4 * (lane >> 5);
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (fwd) v[e] = (n < 3 * D && k + e < D) ? W[(size_t)n * D + k + e] : 0.f;
      else v[e] = (n < D && k + e < 3 * D) ? W[(size_t)(k + e) * D + n] : 0.f;
    }
    out[i] = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// ---- forward --------------------------------------------------------------------------------------------------------
// TPW = tiles per matrix wave (ceil(NT / 4)), MW = memory waves (4 or 8).
// BX = 1: the products run on the bf16 matrix pipe as six products of the exact three-way operand split (gemm_bx.hpp): W_hh
// arrives pre-split (k_bx_pack: three planes in fragment order), the state fragment is split by the matrix wave itself.
// OFS = 1: the state offset of ChainArgs (off_table / off_index).  An instantiation of its own: held as a run-time branch, the
// offset rows' registers cost the offset-free kernels 34 VGPRs and three of them their scratch-free allocation.
template <int VARIANT, int TPW, int MW, int BX, int OFS = 0>
__global__ void __launch_bounds__(256 + 64 * MW) k_gru_chain_fwd(ChainArgs a, const float* __restrict__ gi, float* __restrict__ H,
                                                                  float* __restrict__ saved) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int PASSES = CH_SLOTS / MW;
  const int D = a.D, D4 = D >> 2;
  const int G = (VARIANT == TEMP_GRU_TORCH) ? 3 * D : D;
  const ChainGeom g = chain_geom(D);
  const int NT = g.NT, NQ = g.NQ, lda = g.lda, ldh = g.ldh;
  float* accb = lds;                                   // [32][lda]  raw products of the current position
  float* hb = accb + CH_SLOTS * lda;                   // [2][32][ldh] states (double buffered)
  int* tabb = (int*)(hb + 2 * CH_SLOTS * ldh);         // [ms][32] the panel's row table
  float* decb = (float*)(tabb + CH_SLOTS * a.max_steps);   // [ms][32] decay factor of every row
  int* flagb = (int*)(decb + CH_SLOTS * a.max_steps);  // [ms] step flags
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const size_t plane = a.plane;

  for (int p = blockIdx.x; p < a.n_panels; p += gridDim.x) {
    const int rnn_id = a.panel[4 * p], s0 = a.panel[4 * p + 1], ns = a.panel[4 * p + 2];
    const ChainRnn R = a.rnn[rnn_id];
    for (int i = tid; i < 2 * CH_SLOTS * ldh; i += blockDim.x) hb[i] = 0.f;      // k padding of the state rows must be 0, not NaN
    for (int i = tid; i < ns * CH_SLOTS; i += blockDim.x) {
      const int e = a.rows[(size_t)s0 * CH_SLOTS + i];
      tabb[i] = e;
      decb[i] = e >= 0 ? decay_factor(a.dt[e & CH_ROW_MASK], a.lambda, R.decay_wb) : 0.f;
    }
    if (tid < ns) flagb[tid] = a.sinfo[4 * (size_t)(s0 + tid)];
    __syncthreads();

    if (wave < 4) {
      // ------------------------------------------------------------------ matrix role
      const int li = lane & 31, hh = lane >> 5;
      bool tval[TPW];
      int tidx[TPW];
#pragma unroll
      for (int j = 0; j < TPW; ++j) { tidx[j] = wave + 4 * j; tval[j] = tidx[j] < NT; if (!tval[j]) tidx[j] = NT - 1; }
      f32x16 acc[TPW];
#pragma unroll
      for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
      if constexpr (BX) {
        // W_hh planes of ONE slab (16 k) in registers: [tile][lane] per plane, packed[((slab * NT + tile) * 3 + plane) * 64 + lane].
        // The products of a slab go plane by plane -- L.ah | M.am, M.ah | H.al, H.am, H.ah (small terms first within a plane),
        // interleaved over the wave's tiles -- so that a plane's registers are free after its last round and are refilled
        // with the NEXT slab's plane at once: 3 to 5 rounds (TPW MFMAs each) of L2 latency cover with a single buffer.
        const bx_u32x4* wp = reinterpret_cast<const bx_u32x4*>(R.wf);
        const int NS = NQ >> 1;
        bx_u32x4 wh[TPW] = {}, wm[TPW] = {}, wl[TPW] = {};
        // (a wave's tile slot past the last tile keeps whatever its registers hold: its products are never stored, and its
        //  share of the plane stream -- 1/20 of the forward's, 1/8 of the backward's -- stays in L2)
        const bool dup_loads = (a.dbg & 128) != 0;
        auto wload = [&](bx_u32x4 (&w)[TPW], int sl, int pl) {
#pragma unroll
          for (int j = 0; j < TPW; ++j)
            if (tval[j] || dup_loads) w[j] = wp[((size_t)(sl * NT + tidx[j]) * 3 + pl) * 64 + lane];
        };
        // Every CU of an XCD walks the same 720 KB of planes; started at the same slab they ask the same L2 lines at the same
        // time.  The walk of a block starts at its own slab (k order of a sum is free; fixed per block, so results stay
        // bit-repeatable).
        const int rot = (a.dbg & 64) ? 0 : (int)(blockIdx.x >> 3) % NS;
        wload(wh, rot, 0); wload(wm, rot, 1); wload(wl, rot, 2);
        for (int s = 0; s < ns; ++s) {
          const int cur = s & 1;
          const int flags = flagb[s];
          if (flags & 1) {
            const int e = tabb[s * CH_SLOTS + li];
            const float decm = (e >= 0 && (e & CH_HAS_PREV)) ? decb[s * CH_SLOTS + li] : 0.f;
            const float* hrow = hb + (size_t)cur * CH_SLOTS * ldh + li * ldh + 8 * hh;     // k = 16 slab + 8 hh .. +7 of track li
            bx_u32x4 AH, AM, AL, NH, NM, NL;
            {
              const float4 r0 = scale4(ld4(hrow + 16 * rot), decm), r1 = scale4(ld4(hrow + 16 * rot + 4), decm);
              unsigned h_, m_, l_;
              bx_split_pair(r0.x, r0.y, h_, m_, l_); AH[0] = h_; AM[0] = m_; AL[0] = l_;
              bx_split_pair(r0.z, r0.w, h_, m_, l_); AH[1] = h_; AM[1] = m_; AL[1] = l_;
              bx_split_pair(r1.x, r1.y, h_, m_, l_); AH[2] = h_; AM[2] = m_; AL[2] = l_;
              bx_split_pair(r1.z, r1.w, h_, m_, l_); AH[3] = h_; AM[3] = m_; AL[3] = l_;
            }
            for (int j = 0, sl = rot; j < NS; ++j) {
              const int sn = sl + 1 < NS ? sl + 1 : 0;            // (after the last slab of the walk: the first one of the NEXT position, weights only)
              const float4 n0 = scale4(ld4(hrow + 16 * sn), decm), n1 = scale4(ld4(hrow + 16 * sn + 4), decm);
              const bx_bf16x8 ah = bx_frag(AH), am = bx_frag(AM), al = bx_frag(AL);
              unsigned h_, m_, l_;
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int j = 0; j < TPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bx_frag(wl[j]), ah, acc[j], 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
              wload(wl, sn, 2);
              bx_split_pair(n0.x, n0.y, h_, m_, l_); NH[0] = h_; NM[0] = m_; NL[0] = l_;
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int j = 0; j < TPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bx_frag(wm[j]), am, acc[j], 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
              bx_split_pair(n0.z, n0.w, h_, m_, l_); NH[1] = h_; NM[1] = m_; NL[1] = l_;
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int j = 0; j < TPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bx_frag(wm[j]), ah, acc[j], 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
              wload(wm, sn, 1);
              bx_split_pair(n1.x, n1.y, h_, m_, l_); NH[2] = h_; NM[2] = m_; NL[2] = l_;
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int j = 0; j < TPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bx_frag(wh[j]), al, acc[j], 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
              bx_split_pair(n1.z, n1.w, h_, m_, l_); NH[3] = h_; NM[3] = m_; NL[3] = l_;
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int j = 0; j < TPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bx_frag(wh[j]), am, acc[j], 0, 0, 0);
#pragma unroll
              for (int j = 0; j < TPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bx_frag(wh[j]), ah, acc[j], 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
              wload(wh, sn, 0);
              AH = NH; AM = NM; AL = NL;
              sl = sn;
            }
          // lane (li, hh) owns track li and, per register quad qq, gate columns tile*32 + 8qq + 4hh .. +3
#pragma unroll
          for (int j = 0; j < TPW; ++j) {
            if (!tval[j]) continue;
            float* dst = accb + (size_t)li * lda + tidx[j] * 32 + 4 * hh;
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
              st4(dst + 8 * qq, make_float4(acc[j][4 * qq], acc[j][4 * qq + 1], acc[j][4 * qq + 2], acc[j][4 * qq + 3]));
              acc[j][4 * qq] = 0.f; acc[j][4 * qq + 1] = 0.f; acc[j][4 * qq + 2] = 0.f; acc[j][4 * qq + 3] = 0.f;
            }
          }
          }
          __syncthreads();      // A: products of position s are in LDS
          __syncthreads();      // B: states of position s are in LDS
        }
      } else {
      float4 wA[TPW], wB[TPW];
      auto wload = [&](float4 (&w)[TPW], int q) {
#pragma unroll
        for (int j = 0; j < TPW; ++j) w[j] = R.wf[((size_t)tidx[j] * NQ + q) * 64 + lane];
      };
      wload(wA, 0);
      for (int s = 0; s < ns; ++s) {
        const int cur = s & 1;
        const int flags = flagb[s];
        if (flags & 1) {
          const int e = tabb[s * CH_SLOTS + li];
          // decayed previous state (models/RRGCN.py:83); a track without one multiplies (finite) stale LDS contents by 0
          const float decm = (e >= 0 && (e & CH_HAS_PREV)) ? decb[s * CH_SLOTS + li] : 0.f;
          const float* hrow = hb + (size_t)cur * CH_SLOTS * ldh + li * ldh + 4 * hh;
          auto stage = [&](const float4 (&w)[TPW], const float4 h4) {
#pragma unroll
            for (int j = 0; j < TPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j].x, h4.x, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < TPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j].y, h4.y, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < TPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j].z, h4.z, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < TPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j].w, h4.w, acc[j], 0, 0, 0);
          };
          // both operands of stage q + 1 (weights: L2, state: LDS) are requested before the MFMAs of stage q issue; the
          // scheduling barriers keep the compiler from sinking a prefetch down to its first use
          float4 hA = scale4(ld4(hrow), decm), hB;
          for (int q = 0; q < NQ; q += 2) {
            const int q2 = q + 2 < NQ ? q + 2 : 0;
            wload(wB, q + 1);
            hB = scale4(ld4(hrow + 8 * (q + 1)), decm);
            __builtin_amdgcn_sched_barrier(0);
            stage(wA, hA);
            __builtin_amdgcn_sched_barrier(0);
            wload(wA, q2);                                            // past the end: stage 0 of the NEXT position
            hA = scale4(ld4(hrow + 8 * q2), decm);
            __builtin_amdgcn_sched_barrier(0);
            stage(wB, hB);
            __builtin_amdgcn_sched_barrier(0);
          }
          // lane (li, hh) owns track li and, per register quad qq, gate columns tile*32 + 8qq + 4hh .. +3
#pragma unroll
          for (int j = 0; j < TPW; ++j) {
            if (!tval[j]) continue;
            float* dst = accb + (size_t)li * lda + tidx[j] * 32 + 4 * hh;
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
              st4(dst + 8 * qq, make_float4(acc[j][4 * qq], acc[j][4 * qq + 1], acc[j][4 * qq + 2], acc[j][4 * qq + 3]));
              acc[j][4 * qq] = 0.f; acc[j][4 * qq + 1] = 0.f; acc[j][4 * qq + 2] = 0.f; acc[j][4 * qq + 3] = 0.f;
            }
          }
        }
        __syncthreads();      // A: products of position s are in LDS
        __syncthreads();      // B: states of position s are in LDS
      }
      }
    } else {
      // ------------------------------------------------------------------ memory role
      const int mw = wave - 4, c4 = lane, col = 4 * c4;
      const bool cact = c4 < D4;
      float4 bhr = zero4(), bhz = zero4(), bhn = zero4();
      if (cact) { bhr = ld4(R.b_hh + col); bhz = ld4(R.b_hh + D + col); bhn = ld4(R.b_hh + 2 * D + col); }
      int erow[PASSES];
      float4 g0[PASSES], g1[PASSES], g2[PASSES];
      float4 ofs[OFS ? PASSES : 1];            // OFS: the rows' state offsets
      auto prefetch = [&](int s) {
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
          const int e = tabb[s * CH_SLOTS + ps * MW + mw];
          erow[ps] = e;
          const bool ok = e >= 0 && cact;
          const int er = e & CH_ROW_MASK;
          const float* src = gi + (ok ? (size_t)(a.gi_index ? a.gi_index[er] : er) * G + col : 0);
          if (VARIANT == TEMP_GRU_TORCH) { g0[ps] = ld4(src); g1[ps] = ld4(src + (ok ? D : 0)); g2[ps] = ld4(src + (ok ? 2 * D : 0)); }
          else { g0[ps] = zero4(); g1[ps] = zero4(); g2[ps] = ld4(src); }
          if constexpr (OFS) {                 // travels with the position's input gates: off the per-position critical path
            const int k = ok ? a.off_index[er] : -1;
            ofs[ps] = (k >= 0 && k < a.off_rows) ? ld4(a.off_table + (size_t)k * D + col) : zero4();
          }
        }
      };
      prefetch(0);
      for (int s = 0; s < ns; ++s) {
        const int cur = s & 1;
        const int flags = flagb[s];
        __syncthreads();      // A
        const float* hcur = hb + (size_t)cur * CH_SLOTS * ldh;
        float* hnext = hb + (size_t)(cur ^ 1) * CH_SLOTS * ldh;
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
          const int slot = ps * MW + mw;
          const int e = erow[ps];
          if (e < 0 || !cact) continue;
          const size_t row = (size_t)(e & CH_ROW_MASK);
          const bool hp = (e & CH_HAS_PREV) != 0;
          float4 ar = zero4(), az = zero4(), an = zero4(), hd = zero4();
          if (hp) {                                   // (a track without a previous state contributed zeros to the products)
            const float* ab = accb + (size_t)slot * lda + col;
            ar = ld4(ab); az = ld4(ab + D); an = ld4(ab + 2 * D);
            hd = scale4(ld4(hcur + (size_t)slot * ldh + col), decb[s * CH_SLOTS + slot]);
          }
          float o_h[4], o_r[4], o_z[4], o_n[4], o_hn[4];
          const float arv[4] = {ar.x, ar.y, ar.z, ar.w}, azv[4] = {az.x, az.y, az.z, az.w}, anv[4] = {an.x, an.y, an.z, an.w};
          const float hdv[4] = {hd.x, hd.y, hd.z, hd.w};
          const float g0v[4] = {g0[ps].x, g0[ps].y, g0[ps].z, g0[ps].w}, g1v[4] = {g1[ps].x, g1[ps].y, g1[ps].z, g1[ps].w};
          const float g2v[4] = {g2[ps].x, g2[ps].y, g2[ps].z, g2[ps].w};
          const float brv[4] = {bhr.x, bhr.y, bhr.z, bhr.w}, bzv[4] = {bhz.x, bhz.y, bhz.z, bhz.w}, bnv[4] = {bhn.x, bhn.y, bhn.z, bhn.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            float xr = arv[k], xz = azv[k];
            if (VARIANT == TEMP_GRU_TORCH) { xr += g0v[k]; xz += g1v[k]; }
            const float rg = gate_sigmoid(xr + brv[k]);
            const float zg = gate_sigmoid(xz + bzv[k]);
            const float hn = anv[k] + bnv[k];
            const float ng = gate_tanh(g2v[k] + rg * hn);
            o_h[k] = (VARIANT == TEMP_GRU_TORCH) ? ((1.f - zg) * ng + zg * hdv[k]) : (ng + zg * (hdv[k] - ng));
            o_r[k] = rg; o_z[k] = zg; o_n[k] = ng; o_hn[k] = hn;
          }
          float4 h4 = make_float4(o_h[0], o_h[1], o_h[2], o_h[3]);
          if constexpr (OFS) h4 = add4(h4, ofs[ps]);    // the sum is the state: h_out and what the next position decays
          st4(hnext + (size_t)slot * ldh + col, h4);
          const size_t o = row * D + col;
          if (flags & 2) st4(H + o, h4);
          st4(saved + o, make_float4(o_r[0], o_r[1], o_r[2], o_r[3]));
          st4(saved + plane + o, make_float4(o_z[0], o_z[1], o_z[2], o_z[3]));
          st4(saved + 2 * plane + o, make_float4(o_n[0], o_n[1], o_n[2], o_n[3]));
          st4(saved + 3 * plane + o, make_float4(o_hn[0], o_hn[1], o_hn[2], o_hn[3]));
          st4(saved + 4 * plane + o, hd);
        }
        __syncthreads();      // B
        // issued AFTER the barrier: the 24 loads + table look-ups of a prefetch take ~4 k cycles to issue, which the matrix waves
        // would otherwise spend waiting at B (measured with s_memtime stamps: 9 % of a position)
        if (s + 1 < ns) prefetch(s + 1);       // in flight while the matrix waves run position s + 1
      }
    }
    __syncthreads();          // LDS is re-initialised for the next panel
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------
// G4 = 1 (nn.GRU gate layout): the gate gradients are written ONCE, as dgi = [n][4d] = [dr | dz | dn_i | dn_h] (dgh unused) -- two
// thirds of dgh repeat dgi; the weight-gradient and d_x kernels address their columns of the one matrix (gru_wgrad.hpp).
// OFS = 1: the state offset (d_state out; the offset rows in the learnable decay's d_arg), an instantiation of its own as in the forward.
template <int VARIANT, int TPWB, int MW, int BX, int G4 = 0, int OFS = 0>
__global__ void __launch_bounds__(256 + 64 * MW) k_gru_chain_bwd(ChainArgs a, ChainUps ups, const float* __restrict__ saved,
                                                                  float* __restrict__ dgi, float* __restrict__ dgh) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int PASSES = CH_SLOTS / MW;
  const int D = a.D, D4 = D >> 2;
  const int G = (VARIANT == TEMP_GRU_TORCH) ? 3 * D : D;
  const ChainGeom g = chain_geom(D);
  const int NTb = g.NTb, NQb = g.NQb, ldA = g.ldA, ldz = g.ldz;
  float* ab = lds;                                     // [32][ldA]  gate gradients w.r.t. the recurrent pre-activations (dgh)
  float* gzb = ab + CH_SLOTS * ldA;                    // [32][ldz]  dh * z
  float* dpb = gzb + CH_SLOTS * ldz;                   // [32][ldz]  d_prev of the position just processed
  int* tabb = (int*)(dpb + CH_SLOTS * ldz);            // [ms][32] the panel's row table
  float* decb = (float*)(tabb + CH_SLOTS * a.max_steps);   // [ms][32]
  int* flagb = (int*)(decb + CH_SLOTS * a.max_steps);  // [ms]
  int* upb = flagb + a.max_steps;                      // [ms][2] upstream block and its first row of every step
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const size_t plane = a.plane;

  for (int p = blockIdx.x; p < a.n_panels; p += gridDim.x) {
    const int rnn_id = a.panel[4 * p], s0 = a.panel[4 * p + 1], ns = a.panel[4 * p + 2];
    const ChainRnn R = a.rnn[rnn_id];
    for (int i = tid; i < CH_SLOTS * ldA; i += blockDim.x) ab[i] = 0.f;          // k padding of the dgh rows
    if (tid < ns) { upb[2 * tid] = a.sinfo[4 * (size_t)(s0 + tid) + 1]; upb[2 * tid + 1] = a.sinfo[4 * (size_t)(s0 + tid) + 2]; }
    for (int i = tid; i < ns * CH_SLOTS; i += blockDim.x) {
      const int e = a.rows[(size_t)s0 * CH_SLOTS + i];
      tabb[i] = e;
      decb[i] = e >= 0 ? decay_factor(a.dt[e & CH_ROW_MASK], a.lambda, R.decay_wb) : 0.f;
    }
    if (tid < ns) flagb[tid] = a.sinfo[4 * (size_t)(s0 + tid)];
    __syncthreads();

    if (wave < 4) {
      // ------------------------------------------------------------------ matrix role: d_prev = (dgh . W_hh + dh*z) * decay
      const int li = lane & 31, hh = lane >> 5;
      bool tval[TPWB];
      int tidx[TPWB];
#pragma unroll
      for (int j = 0; j < TPWB; ++j) { tidx[j] = wave + 4 * j; tval[j] = tidx[j] < NTb; if (!tval[j]) tidx[j] = NTb - 1; }
      f32x16 acc[TPWB];
#pragma unroll
      for (int j = 0; j < TPWB; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
      if constexpr (BX) {
        // W_hh planes of TWO slabs (16 k each) in registers; the planes of slab sl + 2 replace those of slab sl as soon as
        // their last round of slab sl has issued (L after round 0, M after round 2, H after round 5): nine to eleven rounds of
        // L2 latency cover.  NQb is a multiple of 4, so the slab count is even.
        const bx_u32x4* wp = reinterpret_cast<const bx_u32x4*>(R.wb);
        const int NS = NQb >> 1;
        bx_u32x4 wh0[TPWB] = {}, wm0[TPWB] = {}, wl0[TPWB] = {}, wh1[TPWB] = {}, wm1[TPWB] = {}, wl1[TPWB] = {};
        const bool dup_loads = (a.dbg & 128) != 0;
        auto wload = [&](bx_u32x4 (&w)[TPWB], int sl, int pl) {
#pragma unroll
          for (int j = 0; j < TPWB; ++j)
            if (tval[j] || dup_loads) w[j] = wp[((size_t)(sl * NTb + tidx[j]) * 3 + pl) * 64 + lane];
        };
        const int rot = (a.dbg & 64) ? 0 : 2 * ((int)(blockIdx.x >> 3) % (NS >> 1));     // per-block start of the slab walk (see the forward kernel)
        wload(wh0, rot, 0); wload(wm0, rot, 1); wload(wl0, rot, 2);
        wload(wh1, rot + 1, 0); wload(wm1, rot + 1, 1); wload(wl1, rot + 1, 2);
        for (int s = ns - 1; s >= 0; --s) {
          const int flags = flagb[s];
          __syncthreads();      // A: dgh / dh*z / decay of position s are in LDS
          if (flags & 1) {
            const float* arow = ab + (size_t)li * ldA + 8 * hh;                 // k = 16 slab + 8 hh .. +7 of track li
            bx_u32x4 AH, AM, AL, NH, NM, NL;
            {
              const float4 r0 = ld4(arow + 16 * rot), r1 = ld4(arow + 16 * rot + 4);
              unsigned h_, m_, l_;
              bx_split_pair(r0.x, r0.y, h_, m_, l_); AH[0] = h_; AM[0] = m_; AL[0] = l_;
              bx_split_pair(r0.z, r0.w, h_, m_, l_); AH[1] = h_; AM[1] = m_; AL[1] = l_;
              bx_split_pair(r1.x, r1.y, h_, m_, l_); AH[2] = h_; AM[2] = m_; AL[2] = l_;
              bx_split_pair(r1.z, r1.w, h_, m_, l_); AH[3] = h_; AM[3] = m_; AL[3] = l_;
            }
            // one slab out of the plane registers (wh, wm, wl); `sl2` = the slab they are refilled with
            auto slab = [&](bx_u32x4 (&wh)[TPWB], bx_u32x4 (&wm)[TPWB], bx_u32x4 (&wl)[TPWB], int sl, int sl2) {
              const int sn = sl + 1 < NS ? sl + 1 : 0;
              const float4 n0 = ld4(arow + 16 * sn), n1 = ld4(arow + 16 * sn + 4);
              const bx_bf16x8 ah = bx_frag(AH), am = bx_frag(AM), al = bx_frag(AL);
              unsigned h_, m_, l_;
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int j = 0; j < TPWB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bx_frag(wl[j]), ah, acc[j], 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
              wload(wl, sl2, 2);
              bx_split_pair(n0.x, n0.y, h_, m_, l_); NH[0] = h_; NM[0] = m_; NL[0] = l_;
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int j = 0; j < TPWB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bx_frag(wm[j]), am, acc[j], 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
              bx_split_pair(n0.z, n0.w, h_, m_, l_); NH[1] = h_; NM[1] = m_; NL[1] = l_;
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int j = 0; j < TPWB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bx_frag(wm[j]), ah, acc[j], 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
              wload(wm, sl2, 1);
              bx_split_pair(n1.x, n1.y, h_, m_, l_); NH[2] = h_; NM[2] = m_; NL[2] = l_;
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int j = 0; j < TPWB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bx_frag(wh[j]), al, acc[j], 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
              bx_split_pair(n1.z, n1.w, h_, m_, l_); NH[3] = h_; NM[3] = m_; NL[3] = l_;
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int j = 0; j < TPWB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bx_frag(wh[j]), am, acc[j], 0, 0, 0);
#pragma unroll
              for (int j = 0; j < TPWB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bx_frag(wh[j]), ah, acc[j], 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
              wload(wh, sl2, 0);
              AH = NH; AM = NM; AL = NL;
            };
            for (int j = 0, sl = rot; j < NS; j += 2) {
              const int a2 = sl + 2 < NS ? sl + 2 : 0, b2 = a2 + 1;          // (after the walk's last pair: the first pair of the NEXT position)
              slab(wh0, wm0, wl0, sl, a2);
              slab(wh1, wm1, wl1, sl + 1, b2);
              sl = a2;
            }
          const float dec = decb[s * CH_SLOTS + li];
#pragma unroll
          for (int j = 0; j < TPWB; ++j) {
            if (!tval[j]) continue;
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
              const int c = tidx[j] * 32 + 8 * qq + 4 * hh;
              const float4 gz = ld4(gzb + (size_t)li * ldz + c);
              st4(dpb + (size_t)li * ldz + c, make_float4((acc[j][4 * qq] + gz.x) * dec, (acc[j][4 * qq + 1] + gz.y) * dec,
                                                           (acc[j][4 * qq + 2] + gz.z) * dec, (acc[j][4 * qq + 3] + gz.w) * dec));
              acc[j][4 * qq] = 0.f; acc[j][4 * qq + 1] = 0.f; acc[j][4 * qq + 2] = 0.f; acc[j][4 * qq + 3] = 0.f;
            }
          }
          }
          __syncthreads();      // B: d_prev of position s is in LDS
        }
      } else {
      // weights: a ring of four stage buffers, i.e. three stages (3 x 8 MFMAs = 1.5 k cycles) of L2 latency cover
      float4 w0[TPWB], w1[TPWB], w2[TPWB], w3[TPWB];
      auto wload = [&](float4 (&w)[TPWB], int q) {
#pragma unroll
        for (int j = 0; j < TPWB; ++j) w[j] = R.wb[((size_t)tidx[j] * NQb + q) * 64 + lane];
      };
      wload(w0, 0); wload(w1, 1); wload(w2, 2);
      for (int s = ns - 1; s >= 0; --s) {
        const int cur = s & 1;
        const int flags = flagb[s];
        __syncthreads();      // A: dgh / dh*z / decay of position s are in LDS
        if (flags & 1) {
          const float* arow = ab + (size_t)li * ldA + 4 * hh;
          auto stage = [&](const float4 (&w)[TPWB], const float4 d4) {
#pragma unroll
            for (int j = 0; j < TPWB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j].x, d4.x, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < TPWB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j].y, d4.y, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < TPWB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j].z, d4.z, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < TPWB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j].w, d4.w, acc[j], 0, 0, 0);
          };
          float4 dA = ld4(arow), dB;
          for (int q = 0; q < NQb; q += 4) {
            const int qa = q + 4 < NQb ? q + 4 : 0, qb = q + 5 < NQb ? q + 5 : 1, qc = q + 6 < NQb ? q + 6 : 2;   // wrap: the NEXT position
            wload(w3, q + 3);
            dB = ld4(arow + 8 * (q + 1));
            __builtin_amdgcn_sched_barrier(0);
            stage(w0, dA);
            __builtin_amdgcn_sched_barrier(0);
            wload(w0, qa);
            dA = ld4(arow + 8 * (q + 2));
            __builtin_amdgcn_sched_barrier(0);
            stage(w1, dB);
            __builtin_amdgcn_sched_barrier(0);
            wload(w1, qb);
            dB = ld4(arow + 8 * (q + 3));
            __builtin_amdgcn_sched_barrier(0);
            stage(w2, dA);
            __builtin_amdgcn_sched_barrier(0);
            wload(w2, qc);
            dA = ld4(arow + 8 * (q + 4 < NQb ? q + 4 : 0));
            __builtin_amdgcn_sched_barrier(0);
            stage(w3, dB);
            __builtin_amdgcn_sched_barrier(0);
          }
          const float dec = decb[s * CH_SLOTS + li];
#pragma unroll
          for (int j = 0; j < TPWB; ++j) {
            if (!tval[j]) continue;
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
              const int c = tidx[j] * 32 + 8 * qq + 4 * hh;
              const float4 gz = ld4(gzb + (size_t)li * ldz + c);
              st4(dpb + (size_t)li * ldz + c, make_float4((acc[j][4 * qq] + gz.x) * dec, (acc[j][4 * qq + 1] + gz.y) * dec,
                                                           (acc[j][4 * qq + 2] + gz.z) * dec, (acc[j][4 * qq + 3] + gz.w) * dec));
              acc[j][4 * qq] = 0.f; acc[j][4 * qq + 1] = 0.f; acc[j][4 * qq + 2] = 0.f; acc[j][4 * qq + 3] = 0.f;
            }
          }
        }
        __syncthreads();      // B: d_prev of position s is in LDS
      }
      }
    } else {
      // ------------------------------------------------------------------ memory role: gate gradients
      const int mw = wave - 4, c4 = lane, col = 4 * c4;
      const bool cact = c4 < D4;
      int erow[PASSES];
      int enx[PASSES];                                            // the track's entry at the next position when that row continues this one's state, else -1
      float4 sr[PASSES], sz[PASSES], sn[PASSES], shn[PASSES], shd[PASSES];
      auto prefetch = [&](int s) {
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
          const int slot = ps * MW + mw;
          const int e = tabb[s * CH_SLOTS + slot];
          erow[ps] = e;
          int en = -1;
          if (s + 1 < ns) en = tabb[(s + 1) * CH_SLOTS + slot];
          enx[ps] = (en >= 0 && (en & CH_HAS_PREV)) ? en : -1;
          const bool ok = e >= 0 && cact;
          const size_t row = ok ? (size_t)(e & CH_ROW_MASK) : 0;
          const float* src = saved + row * D + (ok ? col : 0);
          sr[ps] = ld4(src); sz[ps] = ld4(src + plane); sn[ps] = ld4(src + 2 * plane); shn[ps] = ld4(src + 3 * plane);
          shd[ps] = ld4(src + 4 * plane);
        }
      };
      prefetch(ns - 1);
      for (int s = ns - 1; s >= 0; --s) {
        const int cur = s & 1;
        // upstream gradient of the step's rows (only the positions whose states are consumed outside the chain -- the
        // target, the last history position -- have one: loaded on demand instead of holding registers for it all the time)
        const int up_sel = upb[2 * s], up_row0 = upb[2 * s + 1];       // (staged in LDS: two dependent global loads per step otherwise)
        const float* upp = up_sel >= 0 ? ups.p[up_sel] : nullptr;
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
          const int slot = ps * MW + mw;
          const int e = erow[ps];
          if (e < 0) continue;                 // idle track: whatever its LDS rows hold only reaches its own, unread, d_prev row
          if (a.d_arg && enx[ps] >= 0) {       // (wave-uniform; lanes past the width take part in the sum with zeros)
            float part = 0.f;
            if (cact) {
              const float4 dp = ld4(dpb + (size_t)slot * ldz + col);
              part = chain_dot_prev(dp, sz[ps], sn[ps], shd[ps]);
              if constexpr (OFS) {             // the state the successor decayed is h + offset (loaded on demand: decay and offset together)
                const int k = a.off_index[e & CH_ROW_MASK];
                if (k >= 0 && k < a.off_rows) {
                  const float4 o = ld4(a.off_table + (size_t)k * D + col);
                  part += (dp.x * o.x + dp.y * o.y) + (dp.z * o.z + dp.w * o.w);
                }
              }
            }
            chain_store_d_arg(a, R, enx[ps], part, lane);
          }
          if (!cact) continue;
          const size_t row = (size_t)(e & CH_ROW_MASK);
          float4 gd = upp ? ld4(upp + (row - (size_t)up_row0) * D + col) : zero4();
          if (enx[ps] >= 0) gd = add4(gd, ld4(dpb + (size_t)slot * ldz + col));
          if constexpr (OFS) if (a.d_state) st4(a.d_state + row * D + col, gd);      // ds/dh = I: what reaches the state reaches its offset row (every row once)
          const float4 rg = sr[ps], zg = sz[ps], ng = sn[ps], hn = shn[ps], hd = shd[ps];
          float4 dr_pre, dz_pre, dn_pre, dhn, gz;
#define TEMP_GATE(c)                                          \
          {                                                   \
            const float dn = gd.c * (1.f - zg.c);             \
            const float dz = gd.c * (hd.c - ng.c);            \
            dn_pre.c = dn * (1.f - ng.c * ng.c);              \
            dr_pre.c = dn_pre.c * hn.c * rg.c * (1.f - rg.c); \
            dz_pre.c = dz * zg.c * (1.f - zg.c);              \
            dhn.c = dn_pre.c * rg.c;                          \
            gz.c = gd.c * zg.c;                               \
          }
          TEMP_GATE(x) TEMP_GATE(y) TEMP_GATE(z) TEMP_GATE(w)
#undef TEMP_GATE
          float* arow = ab + (size_t)slot * ldA + col;
          st4(arow, dr_pre); st4(arow + D, dz_pre); st4(arow + 2 * D, dhn);
          st4(gzb + (size_t)slot * ldz + col, gz);
          if constexpr (G4) {
            const size_t b4 = row * 4 * D + col;
            st4(dgi + b4, dr_pre); st4(dgi + b4 + D, dz_pre); st4(dgi + b4 + 2 * D, dn_pre); st4(dgi + b4 + 3 * D, dhn);
          } else {
          const size_t b3 = row * 3 * D + col;
          if (VARIANT == TEMP_GRU_TORCH) { st4(dgi + b3, dr_pre); st4(dgi + b3 + D, dz_pre); st4(dgi + b3 + 2 * D, dn_pre); }
          else st4(dgi + row * D + col, dn_pre);
          st4(dgh + b3, dr_pre); st4(dgh + b3 + D, dz_pre); st4(dgh + b3 + 2 * D, dhn);
          }
        }
        __syncthreads();      // A
        if (s > 0) prefetch(s - 1);            // issued behind the barrier (the matrix waves start at once), in flight while they
        __syncthreads();      // B             // run position s
      }
    }
    __syncthreads();
  }
}

// ---- learnable decay: d_arg -> (d_w, d_b) of every GRU -----------------------------------------------------------------
// arg = w dt + b per row, so d_w = sum d_arg . dt and d_b = sum d_arg over the rows with a previous state (the others have no
// decay and their d_arg is never written).  One block per panel walks the panel's part of the row table: thread t takes entries
// t, t + 256, ... in order, the block sums its 256 partials as a fixed tree -> part[p] = {d_w, d_b} of the panel.
// k_chain_decay_final then adds the panels of every GRU in index order.  No floating-point atomics: bit-repeatable.
#define CH_DECAY_THREADS 256
__global__ void __launch_bounds__(CH_DECAY_THREADS) k_chain_decay_reduce(int n_panels, const int32_t* __restrict__ panel, const int32_t* __restrict__ rows,
                                                                       const float* __restrict__ dt, const float* __restrict__ d_arg, float2* __restrict__ part) {
  __shared__ float2 red[CH_DECAY_THREADS];
  const int p = blockIdx.x;
  if (p >= n_panels) return;
  const int s0 = panel[4 * p + 1], ns = panel[4 * p + 2];
  float dw = 0.f, db = 0.f;
  for (int i = threadIdx.x; i < ns * CH_SLOTS; i += CH_DECAY_THREADS) {
    const int e = rows[(size_t)s0 * CH_SLOTS + i];
    if (e >= 0 && (e & CH_HAS_PREV)) {
      const int row = e & CH_ROW_MASK;
      const float g = d_arg[row];
      dw = fmaf(g, dt[row], dw);
      db += g;
    }
  }
  red[threadIdx.x] = make_float2(dw, db);
  __syncthreads();
  for (int w = CH_DECAY_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { red[threadIdx.x].x += red[threadIdx.x + w].x; red[threadIdx.x].y += red[threadIdx.x + w].y; }
    __syncthreads();
  }
  if (threadIdx.x == 0) part[p] = red[0];
}
// one wave per GRU: lane l adds panels l, l + 64, ... of its GRU in order, then the 64 lanes as a fixed tree
__global__ void __launch_bounds__(64) k_chain_decay_final(int n_panels, const int32_t* __restrict__ panel, const float2* __restrict__ part, float2* __restrict__ d_wb) {
  __shared__ float2 red[64];
  const int r = blockIdx.x;
  float dw = 0.f, db = 0.f;
  for (int p = threadIdx.x; p < n_panels; p += 64)
    if (panel[4 * p] == r) { dw += part[p].x; db += part[p].y; }
  red[threadIdx.x] = make_float2(dw, db);
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { red[threadIdx.x].x += red[threadIdx.x + w].x; red[threadIdx.x].y += red[threadIdx.x + w].y; }
    __syncthreads();
  }
  if (threadIdx.x == 0) d_wb[r] = red[0];
}

static bool chain_layout_ok(int layout, int d);
static int chain_check(const TempGruChain* c) {
  if (!c || c->d <= 0 || c->n_panels < 0 || c->n_steps < 0 || c->n_rnn <= 0 || c->n_rnn > TEMP_CHAIN_MAX_RNN) return TEMP_E_BADARG;
  if (c->variant != TEMP_GRU_TORCH && c->variant != TEMP_GRU_TYPE1) return TEMP_E_BADARG;
  if (c->n_panels > 0 && (!c->panel || !c->rows || !c->sinfo || !c->dt)) return TEMP_E_BADARG;
  for (int i = 0; i < c->n_rnn; ++i) if (!c->packed[i] || !c->b_hh[i]) return TEMP_E_BADARG;
  if (c->max_steps <= 0 || c->max_steps > CH_MAX_STEPS) return TEMP_E_BADARG;
  if (!temp_gru_chain_supported(c->d)) return TEMP_E_UNSUPPORTED;
  if (!chain_layout_ok(c->pack_layout, c->d)) return TEMP_E_BADARG;    // (a layout the packs cannot have been written in for this width)
  return TEMP_OK;
}

// the products of the chain run on the bf16 matrix pipe (three-way split) unless TEMP_MFMA=f32 or d is not a multiple of 8
static bool chain_bx(int d) { return bx_enabled() && d % 8 == 0; }
// ... and on the f16 pipe as three products of the scaled two-way split (gru_chain_hx.hpp) unless TEMP_MFMA=bf16x3 or its LDS images do not fit
// (the width's part of it: the f16 kernels' LDS images fit and their tiles fit the waves' registers)
static bool chain_hx_fits(int d) {
  if (d % 8) return false;
  const ChainGeomHx g = chain_geom_hx(d);
  return chain_lds_fwd_hx(d, CH_MAX_STEPS) <= CH_LDS_LIMIT && chain_lds_bwd_hx(d, CH_MAX_STEPS) <= CH_LDS_LIMIT && g.NT <= 20 && g.NTb <= 8;   // (six tiles per matrix wave: the two register sets spill)
}
static bool chain_hx(int d) { return chain_bx(d) && hx_enabled() && chain_hx_fits(d); }
// the layout temp_gru_chain_pack / _pack_multi write now (the options select it); the packs carry it from then on (TempGruChain.pack_layout)
static int chain_pack_layout(int d) { return chain_hx(d) ? TEMP_CHAIN_PACK_HX : chain_bx(d) ? TEMP_CHAIN_PACK_BX : TEMP_CHAIN_PACK_F32; }
static bool chain_layout_ok(int layout, int d) {
  if (layout == TEMP_CHAIN_PACK_F32) return true;
  if (layout == TEMP_CHAIN_PACK_BX) return d % 8 == 0;
  return (layout == TEMP_CHAIN_PACK_HX || layout == TEMP_CHAIN_PACK_HX_X) && chain_hx_fits(d);
}
static bool layout_hx(int layout) { return layout == TEMP_CHAIN_PACK_HX || layout == TEMP_CHAIN_PACK_HX_X; }

// c->decay / c->offset: nullable (TempChainDecay: c->lambda is not read then; TempChainOffset); d_arg / d_state: nullable, backward only
static ChainArgs chain_args(const TempGruChain* c, float* d_arg = nullptr, float* d_state = nullptr) {
  ChainArgs a = {};
  a.d_arg = d_arg;
  if (c->offset) { a.off_table = c->offset->table; a.off_index = c->offset->index; a.off_rows = c->offset->n_rows; }
  a.d_state = d_state;
  const ChainGeom g = chain_geom(c->d);
  a.D = c->d; a.n_panels = c->n_panels; a.max_steps = c->max_steps; a.panel = c->panel; a.rows = c->rows; a.sinfo = c->sinfo; a.dt = c->dt;
  a.layout = c->pack_layout;
  a.n_rnn_keys = c->n_rnn; a.lambda = c->lambda; a.plane = c->saved_plane; a.gi_index = c->gi_index; a.dbg = option(TEMP_OPT_DEBUG) >> 8; a.stamp = debug_buffer_chain(CHX_STAMP_WORDS);      // development A/B switches (bit 6: no per-block rotation of the slab walk); 0 in every product run
  for (int i = 0; i < c->n_rnn; ++i) {
    a.rnn[i].wf = (const float4*)c->packed[i];
    a.rnn[i].wb = (const float4*)c->packed[i] + (a.layout == TEMP_CHAIN_PACK_BX ? (size_t)(g.NQ >> 1) * g.NT * 192 : (size_t)g.NT * g.NQ * 64);
    a.rnn[i].b_hh = c->b_hh[i];
    a.rnn[i].decay_wb = c->decay ? c->decay->wb[i] : nullptr;
    a.rnn[i].kf = a.rnn[i].kb = nullptr;
    if (layout_hx(a.layout)) {
      const ChainGeomHx gx = chain_geom_hx(c->d);
      a.rnn[i].wb = (const float4*)c->packed[i] + chain_hx_fwd_items(c->d);
      a.rnn[i].kf = (const unsigned*)((const float4*)c->packed[i] + chain_hx_fwd_items(c->d) + chain_hx_bwd_items(c->d));
      a.rnn[i].kb = a.rnn[i].kf + gx.NT * 32;
    }
  }
  return a;
}

template <class K>
static int chain_lds_attr(K kernel, size_t bytes, bool* done) {
  if (*done) return TEMP_OK;
  if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, CH_LDS_LIMIT) != hipSuccess) return TEMP_E_LAUNCH;
  (void)bytes;
  *done = true;
  return TEMP_OK;
}

template <int VARIANT, int TPW>
static int launch_chain_fwd(const ChainArgs& a, const float* gi, float* h, float* saved, hipStream_t st) {
  static bool attr = false;
  static bool attr_bx = false;
  static bool attr_hx = false;
  if (layout_hx(a.layout)) {
    const size_t lds_hx = chain_lds_fwd_hx(a.D, a.max_steps);
    // 8 + 8 waves (two matrix and two memory waves per SIMD, 128 registers each): a memory wave then has 28 stores + 12 loads
    // in flight per position instead of 56 + 24 -- beyond the 63 a wave's counter can track, every further access waits for the oldest
    constexpr int TPW8 = (TPW * 4 + 7) / 8 < 1 ? 1 : (TPW * 4 + 7) / 8;
    const int cfg = (a.dbg >> 4) & 3;                          // development A/B: 0 = 8 + 8 waves, 1 = 4 + 4, 2 = 4 + 8
    if (cfg == 1) {
      auto kernel = k_gru_chain_fwd_hx<VARIANT, TPW, 4, 4>;
      int rc = chain_lds_attr(kernel, lds_hx, &attr_hx);
      if (rc) return rc;
      TEMP_LAUNCH(K_GRU_CHAIN_FWD, kernel, dim3(a.n_panels), dim3(512), lds_hx, st, a, gi, h, saved);
    } else if (cfg == 2) {
      static bool attr_48 = false;
      auto kernel = k_gru_chain_fwd_hx<VARIANT, TPW, 8, 4>;
      int rc = chain_lds_attr(kernel, lds_hx, &attr_48);
      if (rc) return rc;
      TEMP_LAUNCH(K_GRU_CHAIN_FWD, kernel, dim3(a.n_panels), dim3(768), lds_hx, st, a, gi, h, saved);
    } else if (cfg == 3) {                                      // (development A/B: 8 + 8 waves, TWO register sets of planes: 37 spills, 291 us against 233)
      static bool attr_882 = false;
      auto kernel = k_gru_chain_fwd_hx<VARIANT, TPW8, 8, 8, 1>;
      int rc = chain_lds_attr(kernel, lds_hx, &attr_882);
      if (rc) return rc;
      TEMP_LAUNCH(K_GRU_CHAIN_FWD, kernel, dim3(a.n_panels), dim3(1024), lds_hx, st, a, gi, h, saved);
    } else {
      static bool attr_88 = false;
      auto kernel = k_gru_chain_fwd_hx<VARIANT, TPW8, 8, 8>;
      int rc = chain_lds_attr(kernel, lds_hx, &attr_88);
      if (rc) return rc;
      TEMP_LAUNCH(K_GRU_CHAIN_FWD, kernel, dim3(a.n_panels), dim3(1024), lds_hx, st, a, gi, h, saved);
    }
    hx_count();
    return launch_status();
  }
  const size_t lds = chain_lds_fwd(a.D, a.max_steps);
  if (a.off_table) {                                            // state offset: the instantiations of their own (chain_offset_check: never an f16 layout)
    static bool attr_o = false, attr_bx_o = false;
    auto launch = [&](auto kernel, bool* granted) {
      int rc = chain_lds_attr(kernel, lds, granted);
      if (rc) return rc;
      TEMP_LAUNCH(K_GRU_CHAIN_FWD, kernel, dim3(a.n_panels), dim3(512), lds, st, a, gi, h, saved);
      return launch_status();
    };
    return a.layout == TEMP_CHAIN_PACK_BX ? launch(k_gru_chain_fwd<VARIANT, TPW, 4, 1, 1>, &attr_bx_o) : launch(k_gru_chain_fwd<VARIANT, TPW, 4, 0, 1>, &attr_o);
  }
  if (a.layout == TEMP_CHAIN_PACK_BX) {
    auto kernel = k_gru_chain_fwd<VARIANT, TPW, 4, 1>;
    int rc = chain_lds_attr(kernel, lds, &attr_bx);
    if (rc) return rc;
    TEMP_LAUNCH(K_GRU_CHAIN_FWD, kernel, dim3(a.n_panels), dim3(512), lds, st, a, gi, h, saved);
    return launch_status();
  }
  auto kernel = k_gru_chain_fwd<VARIANT, TPW, 4, 0>;
  int rc = chain_lds_attr(kernel, lds, &attr);
  if (rc) return rc;
  TEMP_LAUNCH(K_GRU_CHAIN_FWD, kernel, dim3(a.n_panels), dim3(512), lds, st, a, gi, h, saved);
  return launch_status();
}

// ---- the forward with the input gates inside (gru_chain_hx.hpp: k_gru_chain_fwd_x) ------------------------------------
#define CH_FWD_X_OFF 0x400000        // TEMP_DEBUG bit 22: development A/B, callers take the gi route (temp_gru_chain_fwd + its GEMM)
static std::atomic<long long> g_fwd_x_launches{0};
// the W_ih planes behind the W_hh layout of chain_args() (floats)
static size_t chain_x_ih_offset(int d) { return chain_hx_pack_floats(d); }
// the kernel takes this width and panel length (its LDS images: at d = 200, 158 848 + 260 max_steps bytes -- max_steps <= 19)
static bool chain_fwd_x_fits(int d, int max_steps) {
  return chain_hx_fits(d) && d / 4 <= 64 && max_steps > 0 && max_steps <= CH_MAX_STEPS && chain_lds_fwd_x(d, max_steps) <= CH_LDS_LIMIT &&
         (chain_geom_hx(d).NT + 7) / 8 <= 3;
}
// ... and callers should take it: f16 arithmetic selected, TEMP_DEBUG bit 22 clear
static bool chain_fwd_x_ok(int d, int max_steps) { return chain_hx(d) && !(option(TEMP_OPT_DEBUG) & CH_FWD_X_OFF) && chain_fwd_x_fits(d, max_steps); }

template <int VARIANT, int TPWB, int G4 = 0>
static int launch_chain_bwd(const ChainArgs& a, const ChainUps& ups, const float* saved, float* dgi, float* dgh, hipStream_t st,
                            unsigned* row_keys = nullptr, unsigned* col_keys = nullptr) {
  static bool attr = false;
  static bool attr_bx = false;
  static bool attr_hx = false;
  if (layout_hx(a.layout)) {
    const size_t lds_hx = chain_lds_bwd_hx(a.D, a.max_steps);
    constexpr int TPWB8 = (TPWB * 4 + 7) / 8 < 1 ? 1 : (TPWB * 4 + 7) / 8;
    // 4 + 8 waves (168 registers); 8 + 8 waves with a ring of eight slabs -- two matrix waves per SIMD covering each other's L2
    // latency -- leaves the memory role 128 registers: 31 spills, 374 us against 306 (development A/B: TEMP_DEBUG = 8192)
    const int cfg = (a.dbg >> 4) & 3;
    if (cfg == 3) {                                            // (development A/B: a ring of five slabs)
      static bool attr_5 = false;
      auto kernel = k_gru_chain_bwd_hx<VARIANT, TPWB, 8, G4, 4, 5>;
      int rc = chain_lds_attr(kernel, lds_hx, &attr_5);
      if (rc) return rc;
      TEMP_LAUNCH(K_GRU_CHAIN_BWD, kernel, dim3(a.n_panels), dim3(768), lds_hx, st, a, ups, saved, dgi, dgh, row_keys, col_keys);
    } else if (cfg != 2 && a.stamp && VARIANT == TEMP_GRU_TORCH && TPWB == 2 && G4 == 1) {     // (development: the headline instantiation with cycle stamps)
      static bool attr_dev = false;
      auto kernel = k_gru_chain_bwd_hx<TEMP_GRU_TORCH, 2, 8, 1, 4, 4, 1>;
      int rc = chain_lds_attr(kernel, lds_hx, &attr_dev);
      if (rc) return rc;
      TEMP_LAUNCH(K_GRU_CHAIN_BWD, kernel, dim3(a.n_panels), dim3(768), lds_hx, st, a, ups, saved, dgi, dgh, row_keys, col_keys);
    } else if (cfg != 2) {
      auto kernel = k_gru_chain_bwd_hx<VARIANT, TPWB, 8, G4, 4, 4>;
      int rc = chain_lds_attr(kernel, lds_hx, &attr_hx);
      if (rc) return rc;
      TEMP_LAUNCH(K_GRU_CHAIN_BWD, kernel, dim3(a.n_panels), dim3(768), lds_hx, st, a, ups, saved, dgi, dgh, row_keys, col_keys);
    } else {
      static bool attr_88 = false;
      auto kernel = k_gru_chain_bwd_hx<VARIANT, TPWB8, 8, G4, 8, 8>;
      int rc = chain_lds_attr(kernel, lds_hx, &attr_88);
      if (rc) return rc;
      TEMP_LAUNCH(K_GRU_CHAIN_BWD, kernel, dim3(a.n_panels), dim3(1024), lds_hx, st, a, ups, saved, dgi, dgh, row_keys, col_keys);
    }
    hx_count();
    if (col_keys) TEMP_LAUNCH(K_GRU_CHAIN_PACK, k_keys_reduce, dim3(ceil_div(4 * a.D, 32), a.n_rnn_keys), dim3(1024), 0, st, a.n_panels, 4 * a.D, col_keys + (size_t)a.n_rnn_keys * 4 * a.D, col_keys, a.panel, 4);
    return launch_status();
  }
  if (row_keys || col_keys) return TEMP_E_UNSUPPORTED;          // (only the f16 kernels produce keys: ask temp_gru_chain_keys_supported first)
  const size_t lds = chain_lds_bwd(a.D, a.max_steps);
  if (a.off_table) {
    static bool attr_o = false, attr_bx_o = false;
    auto launch = [&](auto kernel, bool* granted) {
      int rc = chain_lds_attr(kernel, lds, granted);
      if (rc) return rc;
      TEMP_LAUNCH(K_GRU_CHAIN_BWD, kernel, dim3(a.n_panels), dim3(768), lds, st, a, ups, saved, dgi, dgh);
      return launch_status();
    };
    return a.layout == TEMP_CHAIN_PACK_BX ? launch(k_gru_chain_bwd<VARIANT, TPWB, 8, 1, G4, 1>, &attr_bx_o) : launch(k_gru_chain_bwd<VARIANT, TPWB, 8, 0, G4, 1>, &attr_o);
  }
  if (a.layout == TEMP_CHAIN_PACK_BX) {
    auto kernel = k_gru_chain_bwd<VARIANT, TPWB, 8, 1, G4>;
    int rc = chain_lds_attr(kernel, lds, &attr_bx);
    if (rc) return rc;
    TEMP_LAUNCH(K_GRU_CHAIN_BWD, kernel, dim3(a.n_panels), dim3(768), lds, st, a, ups, saved, dgi, dgh);
    return launch_status();
  }
  auto kernel = k_gru_chain_bwd<VARIANT, TPWB, 8, 0, G4>;
  int rc = chain_lds_attr(kernel, lds, &attr);
  if (rc) return rc;
  TEMP_LAUNCH(K_GRU_CHAIN_BWD, kernel, dim3(a.n_panels), dim3(768), lds, st, a, ups, saved, dgi, dgh);
  return launch_status();
}

}  // namespace temp

using namespace temp;

extern "C" {

int temp_gru_chain_supported(int d) {
  if (d <= 0 || d % 4) return 0;
  return chain_lds_fwd(d, CH_MAX_STEPS) <= CH_LDS_LIMIT && chain_lds_bwd(d, CH_MAX_STEPS) <= CH_LDS_LIMIT && chain_geom(d).NT <= 24 && chain_geom(d).NTb <= 8;
}

size_t temp_gru_chain_pack_floats(int d) {
  if (d <= 0) return 0;
  const ChainGeom g = chain_geom(d);
  const size_t f32 = ((size_t)g.NT * g.NQ + (size_t)g.NTb * g.NQb) * 64 * 4;
  // three bf16 planes in fragment order: (slabs of 16 k) x tiles x 192 sixteen-byte items, forward then backward
  const size_t bx = ((size_t)(g.NQ >> 1) * g.NT + (size_t)(g.NQb >> 1) * g.NTb) * 192 * 4;
  const size_t hx = chain_hx_pack_floats(d);           // two f16 planes + column keys (gru_chain_hx.hpp)
  const size_t m = f32 > bx ? f32 : bx;
  return m > hx ? m : hx;                              // any arithmetic (TEMP_MFMA) fits the caller's buffer
}

// one W_hh in the F32 or BX layout
static int chain_pack_one(int layout, int d, const float* w_hh, float* packed, void* stream) {
  const ChainGeom g = chain_geom(d);
  if (layout == TEMP_CHAIN_PACK_BX) {
    // forward: gate column x k = W_hh as stored ([3d][d], k contiguous); backward: k = gate column, state column = W_hh as [K][N]
    const int nsf = g.NQ >> 1, nsb = g.NQb >> 1;
    bx_u32x4* pf = reinterpret_cast<bx_u32x4*>(packed);
    bx_u32x4* pb = pf + (size_t)nsf * g.NT * 192;
    TEMP_LAUNCH(K_GRU_CHAIN_PACK, (k_bx_pack<1>), dim3(ceil_div((long long)nsf * g.NT, 4)), dim3(256), 0, (hipStream_t)stream, d, 3 * d, g.NT, nsf,
                w_hh, d, pf);
    TEMP_LAUNCH(K_GRU_CHAIN_PACK, (k_bx_pack<0>), dim3(ceil_div((long long)nsb * g.NTb, 4)), dim3(256), 0, (hipStream_t)stream, 3 * d, d, g.NTb, nsb,
                w_hh, d, pb);
    return launch_status();
  }
  const size_t n4 = ((size_t)g.NT * g.NQ + (size_t)g.NTb * g.NQb) * 64;
  int gx = ceil_div((long long)n4, 256);
  if (gx > 1024) gx = 1024;
  TEMP_LAUNCH(K_GRU_CHAIN_PACK, k_gru_chain_pack, dim3(gx), dim3(256), 0, (hipStream_t)stream, d, w_hh, (float4*)packed);
  return launch_status();
}

int temp_gru_chain_pack(int d, const float* w_hh, float* packed, void* stream) {
  if (d <= 0 || !w_hh || !packed) return TEMP_E_BADARG;
  if (d % 4) return TEMP_E_UNSUPPORTED;
  if (chain_hx(d)) return temp_gru_chain_pack_multi(1, d, &w_hh, &packed, stream);
  return chain_pack_one(chain_pack_layout(d), d, w_hh, packed, stream);
}

int temp_gru_chain_pack_multi(int count, int d, const float* const* w_hh, float* const* packed, void* stream) {
  return temp_gru_chain_pack_multi_layout(d > 0 ? chain_pack_layout(d) : 0, count, d, w_hh, packed, stream);
}

int temp_gru_chain_pack_multi_layout(int layout, int count, int d, const float* const* w_hh, float* const* packed, void* stream) {
  if (count <= 0 || count > TEMP_CHAIN_MAX_RNN || d <= 0 || !w_hh || !packed) return TEMP_E_BADARG;
  for (int i = 0; i < count; ++i) if (!w_hh[i] || !packed[i]) return TEMP_E_BADARG;
  if (d % 4) return TEMP_E_UNSUPPORTED;
  if (layout != TEMP_CHAIN_PACK_F32 && layout != TEMP_CHAIN_PACK_BX && layout != TEMP_CHAIN_PACK_HX) return TEMP_E_BADARG;
  if (!chain_layout_ok(layout, d)) return TEMP_E_UNSUPPORTED;
  if (layout == TEMP_CHAIN_PACK_HX) {
    // two f16 planes with per-column scales: forward (gate column x k: W_hh as stored), backward (k = gate column, state column:
    // W_hh as [K][N], its slab count rounded up to the kernel's multiple of four), then the keys of both
    const ChainGeomHx gx = chain_geom_hx(d);
    HxPackJobs jobs = {};
    for (int i = 0; i < count; ++i) {
      hx_u32x4* pf = reinterpret_cast<hx_u32x4*>(packed[i]);
      hx_u32x4* pb = pf + chain_hx_fwd_items(d);
      unsigned* kf = reinterpret_cast<unsigned*>(pb + chain_hx_bwd_items(d));
      if (jobs.count + 2 > HX_PACK_JOBS) { hx_pack_launch(jobs, K_GRU_CHAIN_PACK, (hipStream_t)stream); jobs = HxPackJobs{}; }
      hx_pack_jobs_add(jobs, w_hh[i], pf, kf, d, 3 * d, d, 1);
      hx_pack_jobs_add(jobs, w_hh[i], pb, kf + gx.NT * 32, 3 * d, d, d, 0, gx.NSb);
    }
    hx_pack_launch(jobs, K_GRU_CHAIN_PACK, (hipStream_t)stream);
    return launch_status();
  }
  if (layout != TEMP_CHAIN_PACK_BX || 2 * count > BX_PACK_JOBS) {
    for (int i = 0; i < count; ++i) { const int rc = chain_pack_one(layout, d, w_hh[i], packed[i], stream); if (rc) return rc; }
    return TEMP_OK;
  }
  const ChainGeom g = chain_geom(d);
  BxPackJobs jobs = {};
  for (int i = 0; i < count; ++i) {                           // forward planes (W_hh as stored: [3d][d], k contiguous), then backward planes (W_hh as [K][N])
    bx_u32x4* pf = reinterpret_cast<bx_u32x4*>(packed[i]);
    bx_pack_jobs_add(jobs, w_hh[i], pf, d, 3 * d, d, 1);
    bx_pack_jobs_add(jobs, w_hh[i], pf + (size_t)(g.NQ >> 1) * g.NT * 192, 3 * d, d, d, 0, g.NQb >> 1);      // (the backward kernel's slab count, as chain_pack_one)
  }
  TEMP_LAUNCH(K_GRU_CHAIN_PACK, k_bx_pack_multi, dim3(ceil_div(jobs.total_units, 4)), dim3(256), 0, (hipStream_t)stream, jobs);
  return launch_status();
}

}  // extern "C"

// launches of a chain forward / backward kernel with a learnable decay / a state offset since the library was loaded (diagnostic)
static std::atomic<long long> g_decay_launches{0};
static std::atomic<long long> g_offset_launches{0};
static void chain_count(const TempGruChain* c) {
  if (c->decay) g_decay_launches.fetch_add(1, std::memory_order_relaxed);
  if (c->offset) g_offset_launches.fetch_add(1, std::memory_order_relaxed);
}
static int chain_decay_check(const TempGruChain* c) {
  if (!c->decay) return TEMP_OK;
  for (int i = 0; i < c->n_rnn; ++i) if (!c->decay->wb[i]) return TEMP_E_BADARG;
  return temp_gru_chain_decay_supported(c->d, c->variant) ? TEMP_OK : TEMP_E_UNSUPPORTED;
}
static int chain_offset_check(const TempGruChain* c) {
  if (!c->offset) return TEMP_OK;
  if (!c->offset->table || !c->offset->index || c->offset->n_rows <= 0) return TEMP_E_BADARG;
  if (!temp_gru_chain_offset_supported(c->d, c->variant)) return TEMP_E_UNSUPPORTED;
  return layout_hx(c->pack_layout) ? TEMP_E_UNSUPPORTED : TEMP_OK;      // (the f16 kernels split the state with the constant scale 2^14: |state| < 4)
}
// the checks both directions and both forward routes start with (include/temp_amd.h: return contract, 1 - 3)
static int chain_desc_check(const TempGruChain* c, const void* io) {
  int rc = io ? chain_check(c) : TEMP_E_BADARG;
  if (!rc) rc = chain_decay_check(c);
  if (!rc) rc = chain_offset_check(c);
  return rc;
}

static int chain_fwd_gi(const TempGruChain* c, const TempChainFwd* io, hipStream_t st) {
  if (c->n_panels == 0) return TEMP_OK;
  if (!io->gi || !io->h_out || !io->saved) return TEMP_E_BADARG;
  const ChainArgs a = chain_args(c);
  chain_count(c);
  const int tpw = ceil_div(chain_geom(c->d).NT, 4);
#define TEMP_CHAIN_FWD(V)                                                            \
  switch (tpw) {                                                                     \
    case 1: return launch_chain_fwd<V, 1>(a, io->gi, io->h_out, io->saved, st);      \
    case 2: return launch_chain_fwd<V, 2>(a, io->gi, io->h_out, io->saved, st);      \
    case 3: return launch_chain_fwd<V, 3>(a, io->gi, io->h_out, io->saved, st);      \
    case 4: return launch_chain_fwd<V, 4>(a, io->gi, io->h_out, io->saved, st);      \
    case 5: return launch_chain_fwd<V, 5>(a, io->gi, io->h_out, io->saved, st);      \
    case 6: return launch_chain_fwd<V, 6>(a, io->gi, io->h_out, io->saved, st);      \
    default: return TEMP_E_UNSUPPORTED;                                              \
  }
  if (c->variant == TEMP_GRU_TORCH) { TEMP_CHAIN_FWD(TEMP_GRU_TORCH) }
  TEMP_CHAIN_FWD(TEMP_GRU_TYPE1)
#undef TEMP_CHAIN_FWD
}

// the x route: a kernel of its own (gru_chain_hx.hpp: k_gru_chain_fwd_x)
static int chain_fwd_x(const TempGruChain* c, const TempChainFwd* io, hipStream_t st) {
  if (c->pack_layout != TEMP_CHAIN_PACK_HX_X) return TEMP_E_BADARG;        // (the W_ih planes sit behind temp_gru_chain_pack_x_multi's packs only)
  if (c->variant != TEMP_GRU_TORCH || !chain_fwd_x_fits(c->d, c->max_steps)) return TEMP_E_UNSUPPORTED;
  if (c->n_panels == 0) return TEMP_OK;
  if (!io->x_index || !io->b_ih || !io->h_out || !io->saved) return TEMP_E_BADARG;
  for (int i = 0; i < c->n_rnn; ++i) if (!io->b_ih[i]) return TEMP_E_BADARG;
  const ChainArgs a = chain_args(c);
  chain_count(c);
  int rc = TEMP_OK;
  ChainX X = {};
  X.x = io->x; X.x_index = io->x_index;
  const ChainGeomHx gx = chain_geom_hx(c->d);
  for (int i = 0; i < c->n_rnn; ++i) {
    X.b_ih[i] = io->b_ih[i];
    X.wi[i] = reinterpret_cast<const hx_u32x4*>(c->packed[i] + chain_x_ih_offset(c->d));
  }
  const size_t lds = chain_lds_fwd_x(c->d, c->max_steps);
  // 8 + 8 waves as k_gru_chain_fwd_hx's default configuration: two matrix waves per SIMD, 128 registers each
  // the development instantiation (cycle stamps, the switches of a.dbg) only where a debug buffer or TEMP_DEBUG asks for it
  const bool dev = a.stamp || (a.dbg & (1 | 2 | 4 | 64 | 2048 | 4096));
  const int tpw = (gx.NT + 7) / 8;
  auto launch = [&](auto kernel, bool* granted) {
    if ((rc = chain_lds_attr(kernel, lds, granted))) return rc;
    TEMP_LAUNCH(K_GRU_CHAIN_FWD, kernel, dim3(a.n_panels), dim3(1024), lds, st, a, X, io->h_out, io->saved);
    return (int)TEMP_OK;
  };
  static bool attr3 = false, attr2 = false, attr1 = false, attr3d = false, attr2d = false, attr1d = false;
  if (tpw == 3) rc = dev ? launch(k_gru_chain_fwd_x<3, 8, 8, 1>, &attr3d) : launch(k_gru_chain_fwd_x<3, 8, 8>, &attr3);
  else if (tpw == 2) rc = dev ? launch(k_gru_chain_fwd_x<2, 8, 8, 1>, &attr2d) : launch(k_gru_chain_fwd_x<2, 8, 8>, &attr2);
  else rc = dev ? launch(k_gru_chain_fwd_x<1, 8, 8, 1>, &attr1d) : launch(k_gru_chain_fwd_x<1, 8, 8>, &attr1);
  if (rc) return rc;
  hx_count();
  g_fwd_x_launches.fetch_add(1, std::memory_order_relaxed);
  return launch_status();
}

// The three backward routes in one place: g4 == NULL -> (dgi, dgh); g4 -> the gate gradients written once (nn.GRU layout); g4 with
// row_keys / col_keys (each nullable) -> the same on the f16 kernels, which also hand out the keys.
static int chain_bwd(const TempGruChain* c, const TempChainBwd* io, hipStream_t st) {
  const bool keys = io->row_keys || io->col_keys;
  if (io->d_state && !c->offset) return TEMP_E_BADARG;
  if (io->n_up < 0 || io->n_up > TEMP_CHAIN_MAX_UP || (io->n_up > 0 && !io->up)) return TEMP_E_BADARG;
  if ((c->decay != nullptr) != (io->d_arg != nullptr)) return TEMP_E_BADARG;
  if (io->g4 ? (io->dgi || io->dgh) : keys) return TEMP_E_BADARG;
  if (io->g4 && c->variant != TEMP_GRU_TORCH) return TEMP_E_UNSUPPORTED;    // (the type-1 cell's dgi is [n, d])
  if (keys && !layout_hx(c->pack_layout)) return TEMP_E_UNSUPPORTED;
  if (c->n_panels == 0) return TEMP_OK;
  if (!io->saved || (!io->g4 && (!io->dgi || !io->dgh))) return TEMP_E_BADARG;
  const ChainArgs a = chain_args(c, io->d_arg, io->d_state);
  chain_count(c);
  ChainUps ups = {};
  for (int i = 0; i < io->n_up; ++i) ups.p[i] = io->up[i];
  const int tpw = ceil_div(chain_geom(c->d).NTb, 4);
  if (io->g4) {
    if (tpw == 1) return launch_chain_bwd<TEMP_GRU_TORCH, 1, 1>(a, ups, io->saved, io->g4, nullptr, st, io->row_keys, io->col_keys);
    if (tpw == 2) return launch_chain_bwd<TEMP_GRU_TORCH, 2, 1>(a, ups, io->saved, io->g4, nullptr, st, io->row_keys, io->col_keys);
    return TEMP_E_UNSUPPORTED;
  }
  if (c->variant == TEMP_GRU_TORCH) {
    if (tpw == 1) return launch_chain_bwd<TEMP_GRU_TORCH, 1>(a, ups, io->saved, io->dgi, io->dgh, st);
    if (tpw == 2) return launch_chain_bwd<TEMP_GRU_TORCH, 2>(a, ups, io->saved, io->dgi, io->dgh, st);
  } else {
    if (tpw == 1) return launch_chain_bwd<TEMP_GRU_TYPE1, 1>(a, ups, io->saved, io->dgi, io->dgh, st);
    if (tpw == 2) return launch_chain_bwd<TEMP_GRU_TYPE1, 2>(a, ups, io->saved, io->dgi, io->dgh, st);
  }
  return TEMP_E_UNSUPPORTED;
}

extern "C" {

int temp_gru_chain_fwd(const TempGruChain* c, const TempChainFwd* io, void* stream) {
  const int rc = chain_desc_check(c, io);
  if (rc) return rc;
  if (io->gi && io->x) return TEMP_E_BADARG;
  return io->x ? chain_fwd_x(c, io, (hipStream_t)stream) : chain_fwd_gi(c, io, (hipStream_t)stream);
}
int temp_gru_chain_bwd(const TempGruChain* c, const TempChainBwd* io, void* stream) {
  const int rc = chain_desc_check(c, io);
  return rc ? rc : chain_bwd(c, io, (hipStream_t)stream);
}

int temp_gru_chain_offset_supported(int d, int variant) {
  return (variant == TEMP_GRU_TORCH || variant == TEMP_GRU_TYPE1) && temp_gru_chain_supported(d) ? 1 : 0;
}
int temp_gru_chain_offset_layout(int d) { return d > 0 ? (chain_bx(d) ? TEMP_CHAIN_PACK_BX : TEMP_CHAIN_PACK_F32) : 0; }
long long temp_gru_chain_offset_launches(void) { return g_offset_launches.load(std::memory_order_relaxed); }
int temp_gru_chain_decay_supported(int d, int variant) {
  return (variant == TEMP_GRU_TORCH || variant == TEMP_GRU_TYPE1) && temp_gru_chain_supported(d) ? 1 : 0;
}
long long temp_gru_chain_decay_launches(void) { return g_decay_launches.load(std::memory_order_relaxed); }
long long temp_gru_chain_fwd_x_launches(void) { return g_fwd_x_launches.load(std::memory_order_relaxed); }
int temp_gru_chain_pack_layout(int d) { return d > 0 ? chain_pack_layout(d) : 0; }
int temp_gru_chain_keys_supported(int d) { return d > 0 && chain_hx(d) ? 1 : 0; }

int temp_gru_chain_fwd_x_supported(int d, int variant, int max_steps) {
  return d > 0 && d % 8 == 0 && variant == TEMP_GRU_TORCH && chain_fwd_x_ok(d, max_steps) ? 1 : 0;
}

size_t temp_gru_chain_pack_x_floats(int d) {
  if (d <= 0) return 0;
  return chain_x_ih_offset(d) + chain_hx_fwd_items(d) * 4;
}

int temp_gru_chain_pack_x_multi(int count, int d, const float* const* w_hh, const float* const* w_ih, float* const* packed, void* stream) {
  if (count <= 0 || count > TEMP_CHAIN_MAX_RNN || d <= 0 || !w_hh || !w_ih || !packed) return TEMP_E_BADARG;
  for (int i = 0; i < count; ++i) if (!w_hh[i] || !w_ih[i] || !packed[i]) return TEMP_E_BADARG;
  if (d % 8 || !chain_hx(d)) return TEMP_E_UNSUPPORTED;
  // per GRU: W_hh laid out as temp_gru_chain_pack_multi lays it out, then W_ih's two f16 planes in the same forward layout (gate
  // column x k: W_ih as stored, [3d][d]).  The forward planes of both are scaled by the keys of their JOINT column maxima (kf);
  // the backward planes and keys are temp_gru_chain_pack_multi's.
  const ChainGeomHx gx = chain_geom_hx(d);
  HxPackJobs jobs = {};
  for (int i = 0; i < count; ++i) {
    hx_u32x4* pf = reinterpret_cast<hx_u32x4*>(packed[i]);
    hx_u32x4* pb = pf + chain_hx_fwd_items(d);
    unsigned* kf = reinterpret_cast<unsigned*>(pb + chain_hx_bwd_items(d));
    hx_u32x4* pi = reinterpret_cast<hx_u32x4*>(packed[i] + chain_x_ih_offset(d));
    if (jobs.count + 2 > HX_PACK_JOBS) { hx_pack_launch(jobs, K_GRU_CHAIN_PACK, (hipStream_t)stream); jobs = HxPackJobs{}; }
    hx_pack_jobs_add_joint(jobs, w_hh[i], pf, w_ih[i], pi, kf, d, 3 * d, d, 1);
    hx_pack_jobs_add(jobs, w_hh[i], pb, kf + gx.NT * 32, 3 * d, d, d, 0, gx.NSb);
  }
  hx_pack_launch(jobs, K_GRU_CHAIN_PACK, (hipStream_t)stream);
  return launch_status();
}

size_t temp_gru_chain_decay_reduce_workspace(const TempGruChain* c) {
  if (!c || c->n_panels <= 0) return 0;
  return (size_t)c->n_panels * sizeof(float2);
}

int temp_gru_chain_decay_reduce(const TempGruChain* c, const float* d_arg, float* d_wb, void* ws, size_t ws_bytes, void* stream) {
  if (!c || c->n_panels < 0 || c->n_rnn <= 0 || c->n_rnn > TEMP_CHAIN_MAX_RNN || !d_wb) return TEMP_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (c->n_panels == 0) return hipMemsetAsync(d_wb, 0, (size_t)c->n_rnn * 2 * sizeof(float), st) == hipSuccess ? TEMP_OK : TEMP_E_LAUNCH;
  if (!c->panel || !c->rows || !c->dt || !d_arg) return TEMP_E_BADARG;
  if (!ws || ws_bytes < temp_gru_chain_decay_reduce_workspace(c)) return TEMP_E_WORKSPACE;
  TEMP_LAUNCH(K_GRU_CHAIN_PACK, k_chain_decay_reduce, dim3(c->n_panels), dim3(CH_DECAY_THREADS), 0, st, c->n_panels, c->panel, c->rows, c->dt, d_arg, (float2*)ws);
  TEMP_LAUNCH(K_GRU_CHAIN_PACK, k_chain_decay_final, dim3(c->n_rnn), dim3(64), 0, st, c->n_panels, c->panel, (const float2*)ws, (float2*)d_wb);
  return launch_status();
}

}  // extern "C"
