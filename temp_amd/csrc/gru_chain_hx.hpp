// The window-chain kernels (gru_chain.hip) with their W_hh products on the f16 matrix pipe: three MFMA products of the scaled
// two-way operand split (split_f16.hpp) where the bf16 variant issues six, two weight planes streamed from L2 instead of three.
//
// What changes against k_gru_chain_fwd / _bwd<.., BX = 1>:
//  * The activations-side operand is split ONCE, by the memory-role wave that produces it, and lives in LDS as two f16 planes in
//    row-major order (track, k): the matrix waves read their MFMA fragments (8 consecutive k of track li) with one ds_read_b128
//    per plane and issue no VALU work at all (the bf16 variant split the fp32 panel in every one of the four matrix waves).
//      forward : the state h.  |h| <= 1 (a convex combination of tanh outputs, starting from 0), so the scale is the constant 2^14;
//                the decay of the previous state is a per-track factor and moves BEHIND the product: (dec h) W = dec (h W).
//                The fp32 state itself (the gates blend it) stays in LDS beside the planes, updated in place by the lane that owns it.
//      backward: the gate gradients [dr | dz | dn_h] of a track, scaled by the power of two that puts the row's largest magnitude into
//                [2^14, 2^15) (a wave holds a whole row: one DPP reduction); the matrix waves unscale d_prev.
//  * W_hh arrives as two f16 planes with per-column scales (hx_pack.hpp); the gates / d_prev epilogues unscale per column.
//  * The backward also hands out what the consumers of g4 need for THEIR split (temp_gru_grads_g4): per row the key of
//    max |[dr dz dn_i]| (d_x = g4[:, :3d] . W_ih) and per GRU and column of g4 the key of the column maximum (the weight gradients sum
//    over the rows: their scale is per column) -- integer maxima, order-independent, so the result is bit-repeatable.
#pragma once
#include "hx_pack.hpp"

namespace temp {

#define CHX_STATE_SCALE 16384.f
#define CHX_STATE_INV (1.f / 16384.f)

// Development only: cycle stamps of k_gru_chain_fwd_x and k_gru_chain_bwd_hx (their DEV = 1 instantiations, launched when a debug
// buffer is set: temp_set_debug_buffer; tools/chain_phases.py prints them).  Lane 0 of the first wave of each role stamps the first
// panel of block 0 and of the mid-grid block: [kernel fwd, bwd][block 0, mid][role matrix, memory][position < CH_MAX_STEPS][8 events].
//   forward   matrix: 0 position begins (behind B / Q)  1 h walk done  2 at A  3 past A  4 x walk done, at B  5 past B
//             memory: 0 position begins  1 x split done, at A  2 past A  3 x loads issued, gates begin  4 gates done, at B  5 past B
//   backward  matrix: 0 at A  1 past A  2 walk done  3 d_prev stored, at B  4 past B
//             memory: 0 gates begin  1 gates done, at A  2 past A  3 prefetch issued, at B  4 past B
#define CHX_STAMP_EVENTS 8
#define CHX_STAMP_BLOCK (2 * CH_MAX_STEPS * CHX_STAMP_EVENTS)
#define CHX_STAMP_WORDS (2 * 2 * CHX_STAMP_BLOCK)
// the stamp rows of this wave (nullptr: none): kernel 0 = forward, 1 = backward; role 0 = matrix, 1 = memory
template <int DEV>
__device__ __forceinline__ long long* chx_stamp_rows(long long* stamp, int kernel, int role, bool first_wave, int lane) {
  if constexpr (DEV) {
    if (!stamp || !first_wave || lane != 0) return nullptr;
    const int mid = (int)(gridDim.x >> 1);
    const int sel = blockIdx.x == 0 ? 0 : ((int)blockIdx.x == mid ? 1 : -1);
    return sel < 0 ? nullptr : stamp + ((size_t)(kernel * 2 + sel) * 2 + role) * (CH_MAX_STEPS * CHX_STAMP_EVENTS);
  }
  return nullptr;
}
#define CHX_STAMP(s, k) do { if constexpr (DEV) { if (stp) stp[(s) * CHX_STAMP_EVENTS + (k)] = (long long)__builtin_readcyclecounter(); } } while (0)

struct ChainGeomHx {
  int NT, NS;        // forward: tiles of 32 gate columns (3d), slabs of 16 k (d)
  int NTb, NSb;      // backward: tiles of 32 state columns (d), slabs of 16 k (3d) rounded up to a multiple of 8 (zero slabs)
  int lda, ldz;      // floats: forward product rows; backward gz / d_prev rows
  int ldp, ldpa;     // bytes: rows of the forward state planes / the backward gate-gradient planes (an odd number of 16-byte units)
  int ldh;           // floats: forward fp32 state rows
};
__host__ __device__ inline ChainGeomHx chain_geom_hx(int D) {
  ChainGeomHx g;
  g.NT = (3 * D + 31) >> 5; g.NS = (D + 15) >> 4;
  g.NTb = (D + 31) >> 5; g.NSb = (((3 * D + 15) >> 4) + 7) & ~7;      // (a multiple of the W ring of either wave configuration)
  g.lda = g.NT * 32 + 4; g.ldz = g.NTb * 32 + 4;
  g.ldp = g.NS * 32 + 16; g.ldpa = g.NSb * 32 + 16;
  g.ldh = g.NS * 16 + 4;
  return g;
}
inline size_t chain_lds_fwd_hx(int D, int ms) {
  const ChainGeomHx g = chain_geom_hx(D);
  return (size_t)CH_SLOTS * g.lda * 4 + 2 * (size_t)CH_SLOTS * g.ldp + (size_t)CH_SLOTS * g.ldh * 4 + (size_t)g.NT * 32 * 4 + (2 * CH_SLOTS + 1) * (size_t)ms * 4;
}
inline size_t chain_lds_bwd_hx(int D, int ms) {
  const ChainGeomHx g = chain_geom_hx(D);
  return 2 * (size_t)CH_SLOTS * g.ldpa + 2 * (size_t)CH_SLOTS * g.ldz * 4 + (2 * CH_SLOTS + 3) * (size_t)ms * 4 + CH_SLOTS * 4 + 4 * (size_t)D * 4 + (size_t)g.NTb * 32 * 4;
}
// packed W_hh of one GRU (16-byte items): [forward planes | backward planes | forward keys (NT * 32) | backward keys (NTb * 32)]
inline size_t chain_hx_fwd_items(int D) { const ChainGeomHx g = chain_geom_hx(D); return (size_t)g.NS * g.NT * 128; }
inline size_t chain_hx_bwd_items(int D) { const ChainGeomHx g = chain_geom_hx(D); return (size_t)g.NSb * g.NTb * 128; }
inline size_t chain_hx_pack_floats(int D) {
  const ChainGeomHx g = chain_geom_hx(D);
  return (chain_hx_fwd_items(D) + chain_hx_bwd_items(D)) * 4 + (size_t)(g.NT + g.NTb) * 32;
}

// ---- forward --------------------------------------------------------------------------------------------------------
// NMW matrix waves (4 or 8: one or two per SIMD) with TPW = ceil(NT / NMW) tiles each, MW memory waves
// TWOSETS (NMW = 8 only): two register sets of W_hh planes instead of one, paid for by reading the state fragments just in time
template <int VARIANT, int TPW, int MW, int NMW = 4, int TWOSETS = 0>
__global__ void __launch_bounds__(64 * (NMW + MW)) k_gru_chain_fwd_hx(ChainArgs a, const float* __restrict__ gi, float* __restrict__ H,
                                                                       float* __restrict__ saved) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int PASSES = CH_SLOTS / MW;
  const int D = a.D, D4 = D >> 2;
  const int G = (VARIANT == TEMP_GRU_TORCH) ? 3 * D : D;
  const ChainGeomHx g = chain_geom_hx(D);
  const int NT = g.NT, NS = g.NS, lda = g.lda, ldp = g.ldp, ldh = g.ldh;
  float* accb = lds;                                             // [32][lda]  raw (scaled) products of the current position
  char* hpl = (char*)(accb + CH_SLOTS * lda);                    // [2 planes][32][ldp bytes]  the state, split
  float* hb = (float*)(hpl + 2 * CH_SLOTS * ldp);                // [32][ldh]  the state in fp32 (read and rewritten by its owner lane only)
  float* ivt = hb + CH_SLOTS * ldh;                              // [NT * 32]  per gate column: 1 / (column scale . state scale)
  int* tabb = (int*)(ivt + NT * 32);                             // [ms][32] the panel's row table
  float* decb = (float*)(tabb + CH_SLOTS * a.max_steps);         // [ms][32] decay factor of every row
  int* flagb = (int*)(decb + CH_SLOTS * a.max_steps);            // [ms] step flags
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;    // (wave-uniform: scalar tile indices, scalar branches)
  const size_t plane = a.plane;

  for (int p = blockIdx.x; p < a.n_panels; p += gridDim.x) {
    const int rnn_id = a.panel[4 * p], s0 = a.panel[4 * p + 1], ns = a.panel[4 * p + 2];
    const ChainRnn R = a.rnn[rnn_id];
    for (int i = tid; i < 2 * CH_SLOTS * ldp / 16; i += blockDim.x) reinterpret_cast<hx_u32x4*>(hpl)[i] = hx_u32x4{0u, 0u, 0u, 0u};
    for (int i = tid; i < CH_SLOTS * ldh; i += blockDim.x) hb[i] = 0.f;
    for (int i = tid; i < NT * 32; i += blockDim.x) ivt[i] = hx_inv_scale(R.kf[i]) * CHX_STATE_INV;
    for (int i = tid; i < ns * CH_SLOTS; i += blockDim.x) {
      const int e = a.rows[(size_t)s0 * CH_SLOTS + i];
      tabb[i] = e;
      decb[i] = e >= 0 ? decay_factor(a.dt[e & CH_ROW_MASK], a.lambda, R.decay_wb) : 0.f;
    }
    if (tid < ns) flagb[tid] = a.sinfo[4 * (size_t)(s0 + tid)];
    __syncthreads();

    if (wave < NMW) {
      // ------------------------------------------------------------------ matrix role: pure MFMA + fragment reads
      const int li = lane & 31, hh = lane >> 5;
      bool tval[TPW];
      int tidx[TPW];
#pragma unroll
      for (int j = 0; j < TPW; ++j) { tidx[j] = wave + NMW * j; tval[j] = tidx[j] < NT; if (!tval[j]) tidx[j] = NT - 1; }
      f32x16 acc[TPW];
#pragma unroll
      for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
      // W_hh planes of TWO slabs in registers (sets 0 / 1 alternate along the slab walk; a set is refilled with the slab two ahead as
      // soon as its plane has had its last product: L after round 0, H after round 2).
      const hx_u32x4* wp = reinterpret_cast<const hx_u32x4*>(R.wf);
      constexpr bool ONESET = NMW > 4 && !TWOSETS;
      constexpr bool PREF = !(NMW > 4 && TWOSETS);               // read the next slab's state fragments one slab ahead
      hx_u32x4 w[ONESET ? 1 : 2][2][TPW] = {};                   // [set][plane h, l][tile]
      auto wload = [&](hx_u32x4 (&wr)[TPW], int sl, int pl) {
#pragma unroll
        for (int j = 0; j < TPW; ++j)
          if (tval[j]) wr[j] = wp[((size_t)(sl * NT + tidx[j]) * 2 + pl) * 64 + lane];
      };
      // every block starts its walk at its own slab (the CUs of an XCD do not ask L2 for the same lines at the same time; fixed
      // per block, so results stay bit-repeatable)
      const int rot = (a.dbg & 64) ? 0 : (int)(blockIdx.x >> 3) % NS;
      wload(w[0][0], rot, 0); wload(w[0][1], rot, 1);
      if constexpr (!ONESET) { wload(w[1][0], rot + 1 < NS ? rot + 1 : 0, 0); wload(w[1][1], rot + 1 < NS ? rot + 1 : 0, 1); }
      const char* hrow = hpl + (size_t)li * ldp + 16 * hh;       // + plane * 32 ldp + 32 slab: k = 16 slab + 8 hh .. + 7 of track li
      const int pl1 = CH_SLOTS * ldp;
      for (int s = 0; s < ns; ++s) {
        const int flags = flagb[s];
        if ((flags & 1) && !(a.dbg & 1)) {                      // (dbg bit 0: development ablation, no products)
          hx_u32x4 FH = *reinterpret_cast<const hx_u32x4*>(hrow + 32 * rot), FL = *reinterpret_cast<const hx_u32x4*>(hrow + pl1 + 32 * rot), NH, NL;
          int sl_cur = rot;
          // one slab out of register set SET (a compile-time index: the sets are registers, never addressed); sl1: the next slab
          // (its fragments are read now), sl2: the slab the set is refilled with
          auto slab = [&](auto set_c, int sl1, int sl2) {
            constexpr int SET = decltype(set_c)::value;
            if constexpr (PREF) {
              NH = *reinterpret_cast<const hx_u32x4*>(hrow + 32 * sl1);
              NL = *reinterpret_cast<const hx_u32x4*>(hrow + pl1 + 32 * sl1);
            } else {
              FH = *reinterpret_cast<const hx_u32x4*>(hrow + 32 * sl_cur);
              FL = *reinterpret_cast<const hx_u32x4*>(hrow + pl1 + 32 * sl_cur);
              sl_cur = sl1;
            }
            const hx_f16x8 ah = hx_frag(FH), al = hx_frag(FL);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < TPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hx_frag(w[SET][1][j]), ah, acc[j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            wload(w[SET][1], sl2, 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < TPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hx_frag(w[SET][0][j]), al, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < TPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hx_frag(w[SET][0][j]), ah, acc[j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            wload(w[SET][0], sl2, 0);
            if constexpr (PREF) { FH = NH; FL = NL; }
          };
          // Walk position j = 0 .. NS - 1 visits slab (rot + j) mod NS out of set j & 1.  A set is refilled with the slab of walk
          // position j + 2 -- or, behind the walk's last two slabs, with walk position j & 1 of the NEXT position (set 0 always holds
          // the even walk positions, also for an odd slab count: the loads behind the last slabs have the whole gate phase to land).
          auto at = [&](int j) { const int v = rot + j; return v < NS ? v : v - NS; };
          if constexpr (ONESET) {
            // two matrix waves per SIMD cover each other's L2 latency: ONE register set, refilled in place with the next slab
            for (int j = 0; j < NS; ++j) slab(std::integral_constant<int, 0>(), at(j + 1 < NS ? j + 1 : 0), at(j + 1 < NS ? j + 1 : 0));
          } else {
          int j = 0;
          for (; j + 1 < NS; j += 2) {
            slab(std::integral_constant<int, 0>(), at(j + 1), at(j + 2 < NS ? j + 2 : 0));
            slab(std::integral_constant<int, 1>(), at(j + 2 < NS ? j + 2 : 0), at(j + 3 < NS ? j + 3 : 1));
          }
          if (j < NS) slab(std::integral_constant<int, 0>(), at(0), at(0));
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
        __syncthreads();      // B: the split state of position s is in LDS
      }
    } else {
      // ------------------------------------------------------------------ memory role
      const int mw = wave - NMW, c4 = lane, col = 4 * c4;
      const bool cact = c4 < D4;
      const int colc = cact ? col : 0;
      const float4 bhr = ld4(R.b_hh + colc), bhz = ld4(R.b_hh + D + colc), bhn = ld4(R.b_hh + 2 * D + colc);
      int erow[PASSES];
      float4 g0[PASSES], g1[PASSES], g2[PASSES];
      auto prefetch = [&](int s) {
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
          const int e = tabb[s * CH_SLOTS + ps * MW + mw];
          erow[ps] = e;
          const bool ok = e >= 0 && cact && !(a.dbg & 4);       // (dbg bit 2: development ablation, no input-gate loads)
          const int er = e & CH_ROW_MASK;
          const float* src = gi + (ok ? (size_t)(a.gi_index ? a.gi_index[er] : er) * G + col : 0);
          if (VARIANT == TEMP_GRU_TORCH) { g0[ps] = ld4(src); g1[ps] = ld4(src + (ok ? D : 0)); g2[ps] = ld4(src + (ok ? 2 * D : 0)); }
          else { g0[ps] = zero4(); g1[ps] = zero4(); g2[ps] = ld4(src); }
        }
      };
      prefetch(0);
      for (int s = 0; s < ns; ++s) {
        const int flags = flagb[s];
        __syncthreads();      // A
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
          const int slot = ps * MW + mw;
          const int e = erow[ps];
          if (e < 0 || !cact) continue;
          const size_t row = (size_t)(e & CH_ROW_MASK);
          const bool hp = (e & CH_HAS_PREV) != 0;
          float4 ar = zero4(), az = zero4(), an = zero4(), hd = zero4();
          if (hp) {                                   // (a track without a previous state: whatever its planes held is not read)
            const float* ab = accb + (size_t)slot * lda + col;
            const float dec = decb[s * CH_SLOTS + slot];
            const float4 pr = ld4(ab), pz = ld4(ab + D), pn = ld4(ab + 2 * D);
            const float4 ivr = ld4(ivt + col), ivz = ld4(ivt + D + col), ivn = ld4(ivt + 2 * D + col);
            ar = make_float4(pr.x * (ivr.x * dec), pr.y * (ivr.y * dec), pr.z * (ivr.z * dec), pr.w * (ivr.w * dec));
            az = make_float4(pz.x * (ivz.x * dec), pz.y * (ivz.y * dec), pz.z * (ivz.z * dec), pz.w * (ivz.w * dec));
            an = make_float4(pn.x * (ivn.x * dec), pn.y * (ivn.y * dec), pn.z * (ivn.z * dec), pn.w * (ivn.w * dec));
            hd = scale4(ld4(hb + (size_t)slot * ldh + col), dec);   // decayed previous state (models/RRGCN.py:83)
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
          const float4 h4 = make_float4(o_h[0], o_h[1], o_h[2], o_h[3]);
          st4(hb + (size_t)slot * ldh + col, h4);
          hx_u32x2 SH, SL;
          hx_split4(h4, CHX_STATE_SCALE, SH, SL);
          char* hdst = hpl + (size_t)slot * ldp + 2 * col;
          *reinterpret_cast<hx_u32x2*>(hdst) = SH;
          *reinterpret_cast<hx_u32x2*>(hdst + CH_SLOTS * ldp) = SL;
          const size_t o = row * D + col;
          if (a.dbg & 2) continue;                              // (development ablation: no global stores)
          if (flags & 2) st4(H + o, h4);
          st4(saved + o, make_float4(o_r[0], o_r[1], o_r[2], o_r[3]));
          st4(saved + plane + o, make_float4(o_z[0], o_z[1], o_z[2], o_z[3]));
          st4(saved + 2 * plane + o, make_float4(o_n[0], o_n[1], o_n[2], o_n[3]));
          st4(saved + 3 * plane + o, make_float4(o_hn[0], o_hn[1], o_hn[2], o_hn[3]));
          st4(saved + 4 * plane + o, hd);
        }
        __syncthreads();      // B
        if (s + 1 < ns) prefetch(s + 1);       // in flight while the matrix waves run position s + 1
      }
    }
    __syncthreads();          // LDS is re-initialised for the next panel
  }
}

// ---- forward with the input gates computed inside (nn.GRU gate layout) -----------------------------------------------
// k_gru_chain_fwd_hx reads gi = x . W_ih^T + b_ih, written by a GEMM launch of its own, once per row and position (2 400 bytes
// at d = 200).  This kernel takes the chain's x rows instead (800 bytes) and runs x . W_ih on its matrix waves in the window where
// they used to wait for the gates of the previous position:
//   after barrier A of position s   x(s+1) . W_ih  -> acc           (the x planes of s+1 were written before A by the memory waves)
//   before barrier B                acc . 2^14 / (row scale): the units of the recurrent product (W_ih and W_hh share their column
//                                   scales, see below; exact: a power of two)
//   after barrier B                 n columns -> gin (LDS) and out of acc; acc += h(s+1) . W_hh on the r / z / n columns: the r and z
//                                   columns are one K-concatenated sum [x | h] . [W_ih | W_hh], n keeps gi_n apart (n = tanh(gi_n +
//                                   b_in + r (gh_n + b_hn)))
//   before barrier A of s+1         acc -> accb, as in k_gru_chain_fwd_hx
// The decay of the previous state moves INTO the state planes (the memory wave writes dec(s+1) . h(s), or zeros when the row of
// s+1 has no previous state), because the product now also carries gi.  The fp32 state lives in the memory waves' registers (a
// lane owns the same columns of the same tracks throughout), which, with 800 instead of 2 400 bytes of prefetch per row, frees
// the LDS for the x planes and gin.
// W_ih arrives like W_hh, as two f16 planes, and both are scaled per column by the power of two of the JOINT column maximum
// max(|W_hh[c]|, |W_ih[c]|) (temp_gru_chain_pack_x_multi; kf holds those keys); the x planes carry a scale per row (split_f16.hpp,
// from the row maximum, which the memory wave holding the row takes with one DPP reduction).
struct ChainX {
  const float* x;                            // [x rows][d]
  const int32_t* x_index;                    // [N_total] x row of chain row i
  const float* b_ih[TEMP_CHAIN_MAX_RNN];
  const hx_u32x4* wi[TEMP_CHAIN_MAX_RNN];    // W_ih planes (the forward layout of W_hh's, scaled by the joint keys kf)
};
inline size_t chain_lds_fwd_x(int D, int ms) {
  const ChainGeomHx g = chain_geom_hx(D);
  return (size_t)CH_SLOTS * (3 * D + 4) * 4 + 4 * (size_t)CH_SLOTS * g.ldp + (size_t)CH_SLOTS * (D + 4) * 4 + CH_SLOTS * 4 + (2 * CH_SLOTS + 1) * (size_t)ms * 4;
}
// NMW matrix waves with TPW tiles each (NMW * TPW >= NT), MW memory waves; one register set of weight planes (two matrix waves
// per SIMD cover each other's L2 latency)
// DEV = 1: the development instantiation (cycle stamps, see CHX_STAMP)
template <int TPW, int MW, int NMW, int DEV = 0>
__global__ void __launch_bounds__(64 * (NMW + MW)) k_gru_chain_fwd_x(ChainArgs a, ChainX X, float* __restrict__ H, float* __restrict__ saved) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int PASSES = CH_SLOTS / MW;
  const int D = a.D, D4 = D >> 2, G3 = 3 * D;
  const ChainGeomHx g = chain_geom_hx(D);
  const int NT = g.NT, NS = g.NS, ldp = g.ldp;
  const int lda = G3 + 4, ldn = D + 4;                           // (odd numbers of 16-byte units: d % 8 == 0)
  float* accb = lds;                                             // [32][lda]  products of the position: [x | h] . [W_ih | W_hh] (r, z), h . W_hh (n)
  char* hpl = (char*)(accb + CH_SLOTS * lda);                    // [2 planes][32][ldp bytes]  the decayed previous state, split
  char* xpl = hpl + 2 * CH_SLOTS * ldp;                          // [2 planes][32][ldp bytes]  x of the NEXT position, split
  float* gin = (float*)(xpl + 2 * CH_SLOTS * ldp);               // [32][ldn]  gi_n (without b_in, in the product's units) of the position
  unsigned* xkey = (unsigned*)(gin + CH_SLOTS * ldn);            // [32] row keys of the x planes
  int* tabb = (int*)(xkey + CH_SLOTS);                           // [ms][32] the panel's row table
  float* decb = (float*)(tabb + CH_SLOTS * a.max_steps);         // [ms][32] decay factor of every row
  int* flagb = (int*)(decb + CH_SLOTS * a.max_steps);            // [ms] step flags
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const size_t plane = a.plane;
  const int dbg = DEV ? a.dbg : 0;                               // (the development switches exist in the DEV instantiation only, but for bit 1: see the gate passes)

  // (each role runs its own panel loop: the loop invariants of one role are not hoisted above the role branch next to the
  //  other's, where both sets would be live at once)
  if (wave < NMW) {
  for (int p = blockIdx.x; p < a.n_panels; p += gridDim.x) {
    const int rnn_id = a.panel[4 * p], s0 = a.panel[4 * p + 1], ns = a.panel[4 * p + 2];
    const ChainRnn R = a.rnn[rnn_id];
    for (int i = tid; i < 4 * CH_SLOTS * ldp / 16; i += blockDim.x) reinterpret_cast<hx_u32x4*>(hpl)[i] = hx_u32x4{0u, 0u, 0u, 0u};   // (k padding)
    for (int i = tid; i < ns * CH_SLOTS; i += blockDim.x) {
      const int e = a.rows[(size_t)s0 * CH_SLOTS + i];
      tabb[i] = e;
      decb[i] = e >= 0 ? decay_factor(a.dt[e & CH_ROW_MASK], a.lambda, R.decay_wb) : 0.f;
    }
    if (tid < ns) flagb[tid] = a.sinfo[4 * (size_t)(s0 + tid)];
    __syncthreads();

      // ------------------------------------------------------------------ matrix role
      // Compiled once per number of valid tiles NV of the wave (TPW or TPW - 1: the launcher instantiates TPW = ceil(NT / NMW)) and
      // dispatched once per panel: with a validity flag per tile every plane load of a walk sat in a wave-uniform branch and the
      // compiler put `s_waitcnt vmcnt(0)` at the head of every slab -- a wait that also covered the plane loaded three products
      // earlier.  Straight-line slabs get counted waits (NV = 3: vmcnt(5), (4), (3) in front of a plane's three first products: the
      // other plane's loads stay in flight).  Loading the clamped tile instead (as k_gru_chain_bwd_hx does, for a reason this kernel
      // does not share: its roles run separate panel loops) would stream 5 of 24 tile columns twice at d = 200.
      auto role = [&](auto nv_c) __attribute__((always_inline)) {
      constexpr int NV = decltype(nv_c)::value, NVA = NV > 0 ? NV : 1;
      const int li = lane & 31, hh = lane >> 5;
      int tidx[NVA];
#pragma unroll
      for (int j = 0; j < NVA; ++j) tidx[j] = wave + NMW * j < NT ? wave + NMW * j : NT - 1;         // (never clamped for j < NV)
      f32x16 acc[NVA];
#pragma unroll
      for (int j = 0; j < NVA; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
      const hx_u32x4* wph = reinterpret_cast<const hx_u32x4*>(R.wf);
      const hx_u32x4* wpi = X.wi[rnn_id];
      hx_u32x4 w[2][NVA] = {};                                   // [plane h, l][tile]: one slab of the stream being walked
      const std::integral_constant<int, 0> P0;
      const std::integral_constant<int, 1> P1;
      // ln: the lane index (a walk hands in a copy the compiler cannot tell from a fresh value, so that the lane-dependent
      // addresses of a walk are formed at its head instead of living -- spilled -- across the whole position)
      auto wload = [&](const hx_u32x4* wp, int sl, auto pl_c, int ln) __attribute__((always_inline)) {
        constexpr int pl = decltype(pl_c)::value;
#pragma unroll
        for (int j = 0; j < NV; ++j)
          w[pl][j] = *reinterpret_cast<const hx_u32x4*>(reinterpret_cast<const char*>(wp) + (unsigned)((((sl * NT + tidx[j]) * 2 + pl) * 64 + ln) * 16));
      };
      const int rot = (dbg & 64) ? 0 : (int)(blockIdx.x >> 3) % NS;
      auto at = [&](int j) { const int v = rot + j; return v < NS ? v : v - NS; };
      // the walks issue ahead of the memory waves' gate arithmetic on the same SIMD (dbg bit 12: development A/B, equal priority)
      const bool prio = !(dbg & 4096);
      // a walk over the NS slabs of one stream (wcur) with the fragments of `pl0` (the state or the x planes); behind its last slab
      // the registers are refilled with the first slab of the stream walked next (wnext)
      bool holds_ih = true;
      // the first slab of a stream, loaded in the order a walk uses and refills the planes (l, then h) and kept in it: the wait at the
      // head of a walk is the weaker of what the ways into it ask for, and with h in front of l this one asked for vmcnt(0)
      auto prime = [&](const hx_u32x4* wp) __attribute__((always_inline)) {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        __builtin_amdgcn_sched_barrier(0);
        wload(wp, rot, P1, ln);
        __builtin_amdgcn_sched_barrier(0);
        wload(wp, rot, P0, ln);
        __builtin_amdgcn_sched_barrier(0);
      };
      prime(wpi);
      // prod = false (development probe, dbg bits 0 / 11): the weights stream, no products issue
      auto walk = [&](const bool prod, const char* pl0, const hx_u32x4* wcur, const hx_u32x4* wnext) __attribute__((always_inline)) {
        if constexpr (NV == 0) return;                           // (a wave without a tile only keeps the barriers)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const char* arow = pl0 + (size_t)(ln & 31) * ldp + 16 * (ln >> 5);
        const int pl1 = CH_SLOTS * ldp;
        hx_u32x4 FH = *reinterpret_cast<const hx_u32x4*>(arow + 32 * rot), FL = *reinterpret_cast<const hx_u32x4*>(arow + pl1 + 32 * rot), NH, NL;
        if (prio) __builtin_amdgcn_s_setprio(2);
        for (int j = 0; j < NS; ++j) {
          const bool last = j + 1 == NS;
          const int sn = at(last ? 0 : j + 1);
          const hx_u32x4* wn = last ? wnext : wcur;
          NH = *reinterpret_cast<const hx_u32x4*>(arow + 32 * sn);
          NL = *reinterpret_cast<const hx_u32x4*>(arow + pl1 + 32 * sn);
          const hx_f16x8 ah = hx_frag(FH), al = hx_frag(FL);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int t = 0; t < NV; ++t) {
            if (prod) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hx_frag(w[1][t]), ah, acc[t], 0, 0, 0);
            else asm volatile("" : : "v"(w[1][t]));
          }
          __builtin_amdgcn_sched_barrier(0);
          wload(wn, sn, P1, ln);
          __builtin_amdgcn_sched_barrier(0);
          if (prod) {
#pragma unroll
            for (int t = 0; t < NV; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hx_frag(w[0][t]), al, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < NV; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hx_frag(w[0][t]), ah, acc[t], 0, 0, 0);
          } else {
#pragma unroll
            for (int t = 0; t < NV; ++t) asm volatile("" : : "v"(w[0][t]));
          }
          __builtin_amdgcn_sched_barrier(0);
          wload(wn, sn, P0, ln);
          FH = NH; FL = NL;
        }
        if (prio) __builtin_amdgcn_s_setprio(0);
      };
      // x . W_ih of the next position into acc, then into the units the rest of the position expects
      auto xprod = [&]() __attribute__((always_inline)) {
        if (!holds_ih) prime(wpi);
        walk(!(dbg & (1 | 2048)), xpl, wpi, wph);
        holds_ih = false;
        const float f = hx_inv_scale(xkey[li]) * CHX_STATE_SCALE;       // (x . s_row) -> (x . 2^14): the units of the state's planes
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[j][r] *= f;
      };
      long long* stp = p == (int)blockIdx.x ? chx_stamp_rows<DEV>(a.stamp, 0, 0, wave == 0, lane) : nullptr;
      if (ns > 0) {
        __syncthreads();      // P: the x planes of position 0 are in LDS
        xprod();
        __syncthreads();      // Q
      }
      for (int s = 0; s < ns; ++s) {
        const int flags = flagb[s];
        CHX_STAMP(s, 0);
        // gi_n of position s -> gin, out of the accumulators
#pragma unroll
        for (int j = 0; j < NV; ++j) {
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            const int c = tidx[j] * 32 + 8 * qq + 4 * hh;
            if (c < 2 * D || c >= G3) continue;
            st4(gin + (size_t)li * ldn + (c - 2 * D), make_float4(acc[j][4 * qq], acc[j][4 * qq + 1], acc[j][4 * qq + 2], acc[j][4 * qq + 3]));
            acc[j][4 * qq] = 0.f; acc[j][4 * qq + 1] = 0.f; acc[j][4 * qq + 2] = 0.f; acc[j][4 * qq + 3] = 0.f;
          }
        }
        if ((flags & 1) && !(dbg & 1)) {
          if (holds_ih) prime(wph);
          walk(true, hpl, wph, wpi);
          holds_ih = true;
        }
        CHX_STAMP(s, 1);
        // lane (li, hh) owns track li and, per register quad qq, gate columns tile*32 + 8qq + 4hh .. +3
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          float* dst = accb + (size_t)li * lda + tidx[j] * 32 + 4 * hh;
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            if (tidx[j] * 32 + 8 * qq + 4 * hh < G3) st4(dst + 8 * qq, make_float4(acc[j][4 * qq], acc[j][4 * qq + 1], acc[j][4 * qq + 2], acc[j][4 * qq + 3]));
            acc[j][4 * qq] = 0.f; acc[j][4 * qq + 1] = 0.f; acc[j][4 * qq + 2] = 0.f; acc[j][4 * qq + 3] = 0.f;
          }
        }
        CHX_STAMP(s, 2);
        __syncthreads();      // A: products of position s (and gin) are in LDS; the x planes of s + 1 too
        CHX_STAMP(s, 3);
        if (s + 1 < ns) xprod();
        CHX_STAMP(s, 4);
        __syncthreads();      // B: the split (decayed) state of position s is in LDS
        CHX_STAMP(s, 5);
      }
      };
      if (wave + NMW * (TPW - 1) < NT) role(std::integral_constant<int, TPW>());
      else role(std::integral_constant<int, TPW - 1>());
    __syncthreads();          // LDS is re-initialised for the next panel
  }
  } else {
  for (int p = blockIdx.x; p < a.n_panels; p += gridDim.x) {
    const int rnn_id = a.panel[4 * p], s0 = a.panel[4 * p + 1], ns = a.panel[4 * p + 2];
    const ChainRnn R = a.rnn[rnn_id];
    for (int i = tid; i < 4 * CH_SLOTS * ldp / 16; i += blockDim.x) reinterpret_cast<hx_u32x4*>(hpl)[i] = hx_u32x4{0u, 0u, 0u, 0u};   // (k padding)
    for (int i = tid; i < ns * CH_SLOTS; i += blockDim.x) {
      const int e = a.rows[(size_t)s0 * CH_SLOTS + i];
      tabb[i] = e;
      decb[i] = e >= 0 ? decay_factor(a.dt[e & CH_ROW_MASK], a.lambda, R.decay_wb) : 0.f;
    }
    if (tid < ns) flagb[tid] = a.sinfo[4 * (size_t)(s0 + tid)];
    __syncthreads();

      // ------------------------------------------------------------------ memory role
      const int mw = wave - NMW, c4 = lane, col = 4 * c4;
      const bool cact = c4 < D4;
      const int colc = cact ? col : 0;
      const float* bih = X.b_ih[rnn_id];
      const float4 br = add4(ld4(bih + colc), ld4(R.b_hh + colc)), bz = add4(ld4(bih + D + colc), ld4(R.b_hh + D + colc));
      const float4 bhn = ld4(R.b_hh + 2 * D + colc), bin = ld4(bih + 2 * D + colc);
      float4 ivr, ivz, ivn;                                      // 1 / (column scale . state scale)
      {
        const hx_u32x4 kr = *reinterpret_cast<const hx_u32x4*>(R.kf + colc), kz = *reinterpret_cast<const hx_u32x4*>(R.kf + D + colc);
        const hx_u32x4 kn = *reinterpret_cast<const hx_u32x4*>(R.kf + 2 * D + colc);
        auto iv = [](const hx_u32x4 k) { return make_float4(hx_inv_scale(k[0]) * CHX_STATE_INV, hx_inv_scale(k[1]) * CHX_STATE_INV,
                                                            hx_inv_scale(k[2]) * CHX_STATE_INV, hx_inv_scale(k[3]) * CHX_STATE_INV); };
        ivr = iv(kr); ivz = iv(kz); ivn = iv(kn);
      }
      float4 hdr[PASSES];                                        // dec(s + 1) . h(s) of this lane's columns of its tracks (the fp32 state)
      float4 xr[PASSES];                                         // x rows of a coming position
      int xi[PASSES];                                            // their x row indices (-1: idle track), wave-uniform: scalar registers
#pragma unroll
      for (int ps = 0; ps < PASSES; ++ps) hdr[ps] = zero4();
      // The x row of a chain row goes through x_index: a load that the row load depends on.  A wave's track entries are the same in
      // every lane, so the indices of a position are read with scalar loads, all passes at once, ONE POSITION AHEAD of the row
      // loads that use them -- xload() then issues its rows without waiting for anything (four dependent L2 round trips per
      // position in front of the gate passes otherwise).  x_index is not written during the launch: the constant address space
      // lets the compiler keep the loads scalar beside the kernel's stores.
      typedef const int32_t __attribute__((address_space(4))) * chx_const_idx;
      const chx_const_idx xidx = (chx_const_idx)(uintptr_t)X.x_index;
      auto xindex = [&](int s) __attribute__((always_inline)) {
        int e[PASSES];
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) e[ps] = tabb[s * CH_SLOTS + ps * MW + mw];
        __builtin_amdgcn_sched_barrier(0);                       // (all the table reads, then all the index loads: one wait each)
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
          const int es = __builtin_amdgcn_readfirstlane(e[ps]);
          xi[ps] = (es >= 0 && !(dbg & 4)) ? xidx[es & CH_ROW_MASK] : -1;     // (dbg bit 2: development ablation, no x loads)
        }
      };
      auto xload = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
          xr[ps] = zero4();
          if (xi[ps] >= 0 && cact) xr[ps] = ld4(X.x + (size_t)xi[ps] * D + col);
        }
      };
      // the loaded rows -> the x planes (scaled per row) and their keys
      auto xsplit = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
          const int slot = ps * MW + mw;
          const unsigned key = hx_wave_max(cact ? hx_abs_bits4(xr[ps]) : 0u);
          if (cact) {
            hx_u32x2 SH, SL;
            hx_split4(xr[ps], hx_scale(key), SH, SL);
            char* xd = xpl + (size_t)slot * ldp + 2 * col;
            *reinterpret_cast<hx_u32x2*>(xd) = SH;
            *reinterpret_cast<hx_u32x2*>(xd + CH_SLOTS * ldp) = SL;
          }
          if (lane == 0) xkey[slot] = key;
        }
      };
      long long* stp = p == (int)blockIdx.x ? chx_stamp_rows<DEV>(a.stamp, 0, 1, mw == 0, lane) : nullptr;
      if (ns > 0) {
        xindex(0);
        xload();
        if (ns > 1) xindex(1);
        xsplit();
        __syncthreads();      // P
        if (ns > 1) xload();
        __syncthreads();      // Q
      }
      for (int s = 0; s < ns; ++s) {
        const int flags = flagb[s];
        CHX_STAMP(s, 0);
        if (s + 2 < ns) xindex(s + 2);                           // (issued here: they land while the matrix waves walk position s)
        if (s + 1 < ns) xsplit();                                // x(s + 1) for the matrix waves' window behind A
        CHX_STAMP(s, 1);
        __syncthreads();      // A
        CHX_STAMP(s, 2);
        if (s + 2 < ns) xload();                                 // x(s + 2): in flight during the gates of s
        // (the passes' LDS addresses are formed here, per position, from a copy of the column the compiler cannot tell from a fresh
        //  value: hoisted out of the position loop they were spilled, and reloaded with a vmcnt(0) inside the gate passes)
        int colv = col;
        asm volatile("" : "+v"(colv));
        CHX_STAMP(s, 3);
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
          const int slot = ps * MW + mw;
          const int e = tabb[s * CH_SLOTS + slot];
          if (!cact) continue;
          int en = -1;
          if (s + 1 < ns) en = tabb[(s + 1) * CH_SLOTS + slot];
          const bool hpn = en >= 0 && (en & CH_HAS_PREV);
          float4 h4 = zero4();
          if (e >= 0) {
            const size_t row = (size_t)(e & CH_ROW_MASK);
            const bool hp = (e & CH_HAS_PREV) != 0;
            const float* ab = accb + (size_t)slot * lda + colv;
            const float4 pr = ld4(ab), pz = ld4(ab + D), pn = ld4(ab + 2 * D), gn = ld4(gin + (size_t)slot * ldn + colv);
            const float4 hd = hp ? hdr[ps] : zero4();
            float o_h[4], o_r[4], o_z[4], o_n[4], o_hn[4];
            const float prv[4] = {pr.x, pr.y, pr.z, pr.w}, pzv[4] = {pz.x, pz.y, pz.z, pz.w}, pnv[4] = {pn.x, pn.y, pn.z, pn.w};
            const float ivrv[4] = {ivr.x, ivr.y, ivr.z, ivr.w}, ivzv[4] = {ivz.x, ivz.y, ivz.z, ivz.w}, ivnv[4] = {ivn.x, ivn.y, ivn.z, ivn.w};
            const float gnv[4] = {gn.x, gn.y, gn.z, gn.w}, hdv[4] = {hd.x, hd.y, hd.z, hd.w};
            const float brv[4] = {br.x, br.y, br.z, br.w}, bzv[4] = {bz.x, bz.y, bz.z, bz.w}, bnv[4] = {bhn.x, bhn.y, bhn.z, bhn.w};
            const float binv[4] = {bin.x, bin.y, bin.z, bin.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const float rg = gate_sigmoid(prv[k] * ivrv[k] + brv[k]);
              const float zg = gate_sigmoid(pzv[k] * ivzv[k] + bzv[k]);
              const float hn = pnv[k] * ivnv[k] + bnv[k];
              const float ng = gate_tanh((gnv[k] * ivnv[k] + binv[k]) + rg * hn);
              o_h[k] = (1.f - zg) * ng + zg * hdv[k];
              o_r[k] = rg; o_z[k] = zg; o_n[k] = ng; o_hn[k] = hn;
            }
            h4 = make_float4(o_h[0], o_h[1], o_h[2], o_h[3]);
            const size_t o = row * D + col;
            // (a.dbg bit 1, development ablation: no global stores.  The one switch read in every instantiation: with the stores in a
            //  block of their own hipcc fuses the gate arithmetic above exactly as it did before the switches left the kernel --
            //  without the test it forms two more packed FMAs per pass and the results move by an ulp)
            if (!(a.dbg & 2)) {
              if (flags & 2) st4(H + o, h4);
              st4(saved + o, make_float4(o_r[0], o_r[1], o_r[2], o_r[3]));
              st4(saved + plane + o, make_float4(o_z[0], o_z[1], o_z[2], o_z[3]));
              st4(saved + 2 * plane + o, make_float4(o_n[0], o_n[1], o_n[2], o_n[3]));
              st4(saved + 3 * plane + o, make_float4(o_hn[0], o_hn[1], o_hn[2], o_hn[3]));
              st4(saved + 4 * plane + o, hd);
            }
          }
          if (s + 1 < ns) {                                      // the state the next position's product reads: decayed, or 0
            hdr[ps] = hpn ? scale4(h4, decb[(s + 1) * CH_SLOTS + slot]) : zero4();
            hx_u32x2 SH, SL;
            hx_split4(hdr[ps], CHX_STATE_SCALE, SH, SL);
            char* hdst = hpl + (size_t)slot * ldp + 2 * colv;
            *reinterpret_cast<hx_u32x2*>(hdst) = SH;
            *reinterpret_cast<hx_u32x2*>(hdst + CH_SLOTS * ldp) = SL;
          }
        }
        CHX_STAMP(s, 4);
        __syncthreads();      // B
        CHX_STAMP(s, 5);
      }
    __syncthreads();          // LDS is re-initialised for the next panel
  }
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------
// row_keys (nullable): [N_total] key of max |[dr dz dn_i]| of every row; col_keys (nullable): [n_rnn + n_panels][4d]: the kernel writes row
// n_rnn + p (panel p's column maxima), k_keys_reduce (hx_pack.hpp) reduces them into rows 0 .. n_rnn - 1
// NMW matrix waves (4 or 8: one or two per SIMD) with TPWB = ceil(NTb / NMW) tiles each; RING = slabs of W_hh held in registers
// DEV = 1: the development instantiation (cycle stamps, see CHX_STAMP)
template <int VARIANT, int TPWB, int MW, int G4, int NMW = 4, int RING = 4, int DEV = 0>
__global__ void __launch_bounds__(64 * (NMW + MW)) k_gru_chain_bwd_hx(ChainArgs a, ChainUps ups, const float* __restrict__ saved,
                                                                     float* __restrict__ dgi, float* __restrict__ dgh,
                                                                     unsigned* __restrict__ row_keys, unsigned* __restrict__ col_keys) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int PASSES = CH_SLOTS / MW;
  const int D = a.D, D4 = D >> 2;
  const ChainGeomHx g = chain_geom_hx(D);
  const int NTb = g.NTb, NSb = g.NSb, ldpa = g.ldpa, ldz = g.ldz;
  char* apl = (char*)lds;                                        // [2 planes][32][ldpa bytes]  [dr | dz | dn_h] of the position, scaled per row, split
  float* gzb = (float*)(apl + 2 * CH_SLOTS * ldpa);              // [32][ldz]  dh * z
  float* dpb = gzb + CH_SLOTS * ldz;                             // [32][ldz]  d_prev of the position just processed
  float* kinv = dpb + CH_SLOTS * ldz;                            // [NTb * 32] 1 / column scale of the panel's W_hh planes (the d_prev epilogue: see there; 16-byte aligned)
  int* tabb = (int*)(kinv + NTb * 32);                           // [ms][32] the panel's row table
  float* decb = (float*)(tabb + CH_SLOTS * a.max_steps);         // [ms][32]
  int* flagb = (int*)(decb + CH_SLOTS * a.max_steps);            // [ms]
  int* upb = flagb + a.max_steps;                                // [ms][2] upstream block and its first row of every step
  float* rinv = (float*)(upb + 2 * a.max_steps);                 // [32] 1 / row scale of the position's planes
  unsigned* ckey = (unsigned*)(rinv + CH_SLOTS);                 // [4d] column maxima of this panel's g4 rows
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;    // (wave-uniform: scalar tile indices, scalar branches)
  const size_t plane = a.plane;

  for (int p = blockIdx.x; p < a.n_panels; p += gridDim.x) {
    const int rnn_id = a.panel[4 * p], s0 = a.panel[4 * p + 1], ns = a.panel[4 * p + 2];
    const ChainRnn R = a.rnn[rnn_id];
    for (int i = tid; i < 2 * CH_SLOTS * ldpa / 16; i += blockDim.x) reinterpret_cast<hx_u32x4*>(apl)[i] = hx_u32x4{0u, 0u, 0u, 0u};   // k padding
    for (int i = tid; i < 4 * D; i += blockDim.x) ckey[i] = 0u;
    for (int i = tid; i < NTb * 32; i += blockDim.x) kinv[i] = hx_inv_scale(R.kb[i]);
    if (tid < ns) { upb[2 * tid] = a.sinfo[4 * (size_t)(s0 + tid) + 1]; upb[2 * tid + 1] = a.sinfo[4 * (size_t)(s0 + tid) + 2]; }
    for (int i = tid; i < ns * CH_SLOTS; i += blockDim.x) {
      const int e = a.rows[(size_t)s0 * CH_SLOTS + i];
      tabb[i] = e;
      decb[i] = e >= 0 ? decay_factor(a.dt[e & CH_ROW_MASK], a.lambda, R.decay_wb) : 0.f;
    }
    if (tid < ns) flagb[tid] = a.sinfo[4 * (size_t)(s0 + tid)];
    __syncthreads();

    if (wave < NMW) {
      // ------------------------------------------------------------------ matrix role: d_prev = (dgh . W_hh + dh*z) * decay
      // (the role's lane-dependent values are formed per panel, from a copy of the lane index the compiler cannot tell from a fresh
      //  value: hoisted above the panel loop they are live -- and take registers -- throughout the memory role's gate passes)
      int rl = lane;
      asm volatile("" : "+v"(rl));
      const int li = rl & 31, hh = rl >> 5;
      bool tval[TPWB];
      int tidx[TPWB];
#pragma unroll
      for (int j = 0; j < TPWB; ++j) { tidx[j] = wave + NMW * j; tval[j] = tidx[j] < NTb; if (!tval[j]) tidx[j] = NTb - 1; }
      f32x16 acc[TPWB];
#pragma unroll
      for (int j = 0; j < TPWB; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
      // W_hh planes of FOUR slabs in registers (a slab is only 3 TPWB products): set q holds slab 4 i + q and is refilled with slab
      // 4 i + q + 4 as its planes fall free, so a plane has the products of three slabs (18 at TPWB = 2) to arrive in.  NSb is a
      // multiple of 4.  That cover exists only while the compiler can COUNT the loads in flight: the vector-memory counter is in
      // order, and the wait in front of a plane's first product must let the 14 loads younger than it (TPWB = 2) stay out.
      //  * The loads are unconditional.  A tile this wave does not own (tval[j] false) streams the clamped tile NTb - 1 into its
      //    registers; its products are never stored.  With `if (tval[j])` around each load every reload sat in a wave-uniform branch
      //    of its own, the number of loads in flight differed by path, and the wait insertion fell back to ONE `s_waitcnt vmcnt(0)`
      //    at the head of every group of four slabs: a full L2 round trip exposed per group, no cover from the ring at all.
      //    Specialising the role on the wave's number of valid tiles was built first (no byte streamed twice).  It puts two copies of
      //    the role into the kernel, and at the 168 registers this kernel is held to the MEMORY role's gate passes then came out with
      //    two scratch reloads and five scalar reloads of kernel arguments inside the position loop.  The clamped loads leave the
      //    memory role's code as it was; what they cost at d = 200 is one of eight tile streams read twice, by the neighbour wave of
      //    the one that owns it and at the same slab, out of the same cache lines.
      //  * The ring is primed in the order the walk uses and refills it (l, then h, slab by slab), and the priming stays in that
      //    order: the wait at the head of the walk is the weaker of what the ways into it ask for, and with the priming's loads in
      //    another order (the compiler's, without the barriers below) every group waited `vmcnt(1)`.
      const hx_u32x4* wp = reinterpret_cast<const hx_u32x4*>(R.wb);
      hx_u32x4 wh[RING][TPWB] = {}, wl[RING][TPWB] = {};
      auto wload = [&](hx_u32x4 (&w)[TPWB], int sl, int pl) {
#pragma unroll
        for (int j = 0; j < TPWB; ++j) w[j] = wp[((size_t)(sl * NTb + tidx[j]) * 2 + pl) * 64 + rl];         // (tidx[j] <= NTb - 1: inside the pack)
      };
      const int rot = (a.dbg & 64) ? 0 : RING * ((int)(blockIdx.x >> 3) % (NSb / RING));     // per-block start of the slab walk (NSb % RING == 0)
      // (a wave without any tile -- widths with NTb < NMW -- loads and multiplies nothing; it still keeps barriers A and B below)
      const bool walks = tval[0];
      if (walks) {
#pragma unroll
        for (int q = 0; q < RING; ++q) {
          wload(wl[q], rot + q, 1);
          __builtin_amdgcn_sched_barrier(0);
          wload(wh[q], rot + q, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      const char* arow = apl + (size_t)li * ldpa + 16 * hh;      // + plane * 32 ldpa + 32 slab
      const int pl1 = CH_SLOTS * ldpa;
      long long* stp = p == (int)blockIdx.x ? chx_stamp_rows<DEV>(a.stamp, 1, 0, wave == 0, lane) : nullptr;
      for (int s = ns - 1; s >= 0; --s) {
        const int flags = flagb[s];
        CHX_STAMP(s, 0);
        __syncthreads();      // A: the split gate gradients / dh*z / row scales of position s are in LDS
        CHX_STAMP(s, 1);
        if (walks && (flags & 1) && !(a.dbg & 1)) {             // (dbg bit 0: development ablation, no products)
          hx_u32x4 FH = *reinterpret_cast<const hx_u32x4*>(arow + 32 * rot), FL = *reinterpret_cast<const hx_u32x4*>(arow + pl1 + 32 * rot), NH, NL;
          for (int j = 0, sl = rot; j < NSb; j += RING) {
            const int base2 = sl + RING < NSb ? sl + RING : 0;          // (after the walk's last group: the first group of the NEXT position)
#pragma unroll
            for (int q = 0; q < RING; ++q) {
              const int sn = (q < RING - 1) ? sl + q + 1 : base2;
              NH = *reinterpret_cast<const hx_u32x4*>(arow + 32 * sn);
              NL = *reinterpret_cast<const hx_u32x4*>(arow + pl1 + 32 * sn);
              const hx_f16x8 ah = hx_frag(FH), al = hx_frag(FL);
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int t = 0; t < TPWB; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hx_frag(wl[q][t]), ah, acc[t], 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
              wload(wl[q], base2 + q, 1);
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int t = 0; t < TPWB; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hx_frag(wh[q][t]), al, acc[t], 0, 0, 0);
#pragma unroll
              for (int t = 0; t < TPWB; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hx_frag(wh[q][t]), ah, acc[t], 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
              wload(wh[q], base2 + q, 0);
              FH = NH; FL = NL;
            }
            sl = base2;
          }
          CHX_STAMP(s, 2);
          const float dec = decb[s * CH_SLOTS + li], ri = rinv[li];
#pragma unroll
          for (int j = 0; j < TPWB; ++j) {
            if (!tval[j]) continue;
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
              const int c = tidx[j] * 32 + 8 * qq + 4 * hh;
              const float4 gz = ld4(gzb + (size_t)li * ldz + c);
              // (the inverse column scales come out of LDS: read from global memory here, each of the eight reads waited, in order,
              //  behind the sixteen reloads the walk has just issued for the NEXT position -- 6 900 cycles where the parent took 2 300)
              const float4 kv = ld4(kinv + c);
              const float i0 = kv.x * ri, i1 = kv.y * ri, i2 = kv.z * ri, i3 = kv.w * ri;
              st4(dpb + (size_t)li * ldz + c, make_float4((acc[j][4 * qq] * i0 + gz.x) * dec, (acc[j][4 * qq + 1] * i1 + gz.y) * dec,
                                                           (acc[j][4 * qq + 2] * i2 + gz.z) * dec, (acc[j][4 * qq + 3] * i3 + gz.w) * dec));
              acc[j][4 * qq] = 0.f; acc[j][4 * qq + 1] = 0.f; acc[j][4 * qq + 2] = 0.f; acc[j][4 * qq + 3] = 0.f;
            }
          }
        }
        CHX_STAMP(s, 3);
        __syncthreads();      // B: d_prev of position s is in LDS
        CHX_STAMP(s, 4);
      }
    } else {
      // ------------------------------------------------------------------ memory role: gate gradients
      const int mw = wave - NMW, c4 = lane, col = 4 * c4;
      const bool cact = c4 < D4;
      const int colc = cact ? col : 0;
      int erow[PASSES];
      int enx[PASSES];                                           // the track's entry at the next position when that row continues this one's state, else -1
      float4 sr[PASSES], sz[PASSES], sn[PASSES], shn[PASSES], shd[PASSES];
      unsigned ck[4][4] = {};                                    // running maxima of this lane's four columns of dr, dz, dn_i, dn_h
      auto prefetch = [&](int s) {
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
          const int slot = ps * MW + mw;
          const int e = tabb[s * CH_SLOTS + slot];
          erow[ps] = e;
          int en = -1;
          if (s + 1 < ns) en = tabb[(s + 1) * CH_SLOTS + slot];
          enx[ps] = (en >= 0 && (en & CH_HAS_PREV)) ? en : -1;
          const bool ok = e >= 0 && cact && !(a.dbg & 4);       // (dbg bit 2: development ablation, every lane reads row 0)
          const size_t row = ok ? (size_t)(e & CH_ROW_MASK) : 0;
          const float* src = saved + row * D + (ok ? col : 0);
          sr[ps] = ld4(src); sz[ps] = ld4(src + plane); sn[ps] = ld4(src + 2 * plane); shn[ps] = ld4(src + 3 * plane);
          shd[ps] = ld4(src + 4 * plane);
        }
      };
      long long* stp = p == (int)blockIdx.x ? chx_stamp_rows<DEV>(a.stamp, 1, 1, mw == 0, lane) : nullptr;
      prefetch(ns - 1);
      for (int s = ns - 1; s >= 0; --s) {
        CHX_STAMP(s, 0);
        const int up_sel = upb[2 * s], up_row0 = upb[2 * s + 1];       // (staged in LDS: two dependent global loads per step otherwise)
        const float* upp = up_sel >= 0 ? ups.p[up_sel] : nullptr;
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
          const int slot = ps * MW + mw;
          const int e = erow[ps];
          if (e < 0) continue;                 // (wave-uniform) idle track: whatever its LDS rows hold only reaches its own, unread, d_prev row
          const size_t row = (size_t)(e & CH_ROW_MASK);
          // every lane runs the arithmetic (the row maxima are wave reductions); lanes past the width compute on zeros
          float4 gd = (upp && cact) ? ld4(upp + (row - (size_t)up_row0) * D + col) : zero4();
          if (enx[ps] >= 0 && cact) gd = add4(gd, ld4(dpb + (size_t)slot * ldz + col));
          const float4 rg = sr[ps], zg = sz[ps], ng = sn[ps], hn = shn[ps], hd = shd[ps];
          if (a.d_arg && enx[ps] >= 0) {       // (wave-uniform) learnable decay: dL/d arg of the row that continues this track (gru_chain.hip)
            const float part = cact ? chain_dot_prev(ld4(dpb + (size_t)slot * ldz + col), zg, ng, hd) : 0.f;
            chain_store_d_arg(a, R, enx[ps], part, lane);
          }
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
          const unsigned kr = cact ? hx_abs_bits4(dr_pre) : 0u, kz = cact ? hx_abs_bits4(dz_pre) : 0u;
          const unsigned kn = cact ? hx_abs_bits4(dn_pre) : 0u, kh = cact ? hx_abs_bits4(dhn) : 0u;
          if (cact && col_keys) {
            if constexpr (NMW > 4) {                             // (128 registers per wave: the column maxima go to LDS at once)
              auto upl = [&](int b4, const float4 v) {
                unsigned* k = ckey + b4 * D + col;
                atomicMax(k, hx_abs_bits(v.x)); atomicMax(k + 1, hx_abs_bits(v.y)); atomicMax(k + 2, hx_abs_bits(v.z)); atomicMax(k + 3, hx_abs_bits(v.w));
              };
              upl(0, dr_pre); upl(1, dz_pre); upl(2, dn_pre); upl(3, dhn);
            } else {
              auto upd = [](unsigned (&m)[4], const float4 v) { m[0] = max(m[0], hx_abs_bits(v.x)); m[1] = max(m[1], hx_abs_bits(v.y)); m[2] = max(m[2], hx_abs_bits(v.z)); m[3] = max(m[3], hx_abs_bits(v.w)); };
              upd(ck[0], dr_pre); upd(ck[1], dz_pre); upd(ck[2], dn_pre); upd(ck[3], dhn);
            }
          }
          const unsigned krz = max(kr, kz);
          const unsigned key_h = hx_wave_max(max(krz, kh));      // [dr dz dn_h]: this row of the recurrent product
          const float sc = hx_scale(key_h);
          if (cact) {
            hx_u32x2 SH, SL;
            char* ad = apl + (size_t)slot * ldpa + 2 * col;
            hx_split4(dr_pre, sc, SH, SL); *reinterpret_cast<hx_u32x2*>(ad) = SH; *reinterpret_cast<hx_u32x2*>(ad + CH_SLOTS * ldpa) = SL;
            hx_split4(dz_pre, sc, SH, SL); *reinterpret_cast<hx_u32x2*>(ad + 2 * D) = SH; *reinterpret_cast<hx_u32x2*>(ad + 2 * D + CH_SLOTS * ldpa) = SL;
            hx_split4(dhn, sc, SH, SL); *reinterpret_cast<hx_u32x2*>(ad + 4 * D) = SH; *reinterpret_cast<hx_u32x2*>(ad + 4 * D + CH_SLOTS * ldpa) = SL;
            st4(gzb + (size_t)slot * ldz + col, gz);
          }
          if (lane == 0) rinv[slot] = hx_inv_scale(key_h);
          if (row_keys) {
            const unsigned key_x = hx_wave_max(max(krz, kn));    // [dr dz dn_i]: this row of d_x = g4[:, :3d] . W_ih
            if (lane == 0) row_keys[row] = key_x;
          }
          if (cact && !(a.dbg & 2)) {                           // (dbg bit 1: development ablation, no global stores)
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
        }
        CHX_STAMP(s, 1);
        __syncthreads();      // A
        CHX_STAMP(s, 2);
        if (s > 0) prefetch(s - 1);            // issued behind the barrier (the matrix waves start at once), in flight while they
        CHX_STAMP(s, 3);
        __syncthreads();      // B             // run position s
        CHX_STAMP(s, 4);
      }
      if (col_keys && cact && NMW <= 4) {      // this lane's column maxima -> the panel's (LDS integer maxima over the eight waves)
#pragma unroll
        for (int b4 = 0; b4 < 4; ++b4)
#pragma unroll
          for (int e = 0; e < 4; ++e) atomicMax(&ckey[b4 * D + colc + e], ck[b4][e]);
      }
    }
    __syncthreads();
    if (col_keys) {
      // this panel's column maxima -> its own row of the partials (k_keys_reduce takes the maxima over a GRU's panels: same-address
      // atomics from 250 workgroups on eight L2s cost ~20 us)
      for (int i = tid; i < 4 * D; i += blockDim.x) col_keys[((size_t)a.n_rnn_keys + p) * 4 * D + i] = ckey[i];
      __syncthreads();
    }
  }
}

}  // namespace temp
